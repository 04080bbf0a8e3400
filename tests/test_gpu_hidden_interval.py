"""The hidden layer's knot interval in the fused [2, 10, 2] kernels (fetode_fused4_body.h: each lane
of a hidden unit's group counts its own four knots, the counts meet on the lanes that own the unit's
spline edges).  The other GPU tests put layer-0 inputs on and off their grid; with the default layer-1
grid the hidden values themselves sit in a few central intervals only.  Here layer 1's grid is set per
hidden unit so that its interior spans the 10th to 90th percentile of that unit's value over the
batch (uniform knots, the usual spline_order extension): the oracle's own hidden values then fall
into every one of the 11 knot intervals and off the grid on both sides — asserted from the oracle's
values, on the CPU.  A count that is off by more than a rounding at a knot moves the spline to a
neighbouring cubic: an O(1) error against the 1e-5 bars of tests/test_gpu_parity.py.
"""
import functools

import pytest
import torch

SEED = 0
B_ALL = 64
ODD = {1: [float("nan"), 0.5], 2: [0.5, float("inf")], 3: [-float("inf"), 1.0]}   # rows of y0


@functools.lru_cache(maxsize=None)
def _case():
    """(state dict with layer 1's per-unit grid, y0 (64, 2), the oracle's hidden values of the finite
    rows (n, 10)).  Computed once, shared by every test of this module."""
    import fet_ode_amd as F
    from oracle import torch_ref as O
    torch.manual_seed(SEED)
    m = F.KANFET([2, 10, 2], grid_size=5)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(SEED)
    y0 = (1.75 + 1.5 * torch.randn(B_ALL, 2, generator=g)).float()
    for r, v in ODD.items():
        y0[r] = torch.tensor(v)
    fin = torch.isfinite(y0).all(-1)
    ref = O.KANFETRef.from_state_dict(sd, 2)
    with torch.no_grad():
        h = O.kanlinear_forward(y0[fin], ref.kan[0]) + O.ferro_forward(y0[fin], ref.ferro[0], ref.states[0])
    lo = torch.quantile(h, 0.10, dim=0)
    hi = torch.quantile(h, 0.90, dim=0)
    step = (hi - lo) / 5
    grid = lo[:, None] + step[:, None] * torch.arange(-3, 9, dtype=torch.float32)[None, :]
    assert grid.shape == sd["layers.1.kan.grid"].shape
    sd["layers.1.kan.grid"] = grid.float().contiguous()
    return sd, y0, h


def _intervals(h, grid):
    """per value: the number of its unit's knots <= it, minus one (-1 / 11: off the grid)"""
    return (h[:, :, None] >= grid[None, :, :]).sum(-1) - 1


def test_oracle_hidden_values_cover_every_interval():
    sd, y0, h = _case()
    iv = _intervals(h, sd["layers.1.kan.grid"])
    seen = set(iv.flatten().tolist())
    print("hidden intervals seen:", sorted(seen), "counts:", torch.bincount((iv + 1).flatten(), minlength=13).tolist())
    assert seen == set(range(-1, 12)), sorted(seen)


def _oracle(sd):
    from oracle import torch_ref as O
    return O.KANFETRef.from_state_dict(sd, 2)


def _model(sd, dev):
    import fet_ode_amd as F
    m = F.KANFET([2, 10, 2], grid_size=5)
    m.load_state_dict(sd)
    return m.to(dev)


def _slice_rel_err(a, b):
    a = a.double().reshape(a.shape[0], -1)
    b = b.double().reshape(b.shape[0], -1)
    return ((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)).max().item()


# default: whatever the dispatch picks at this batch; the two fused4 lane maps forced at every batch
KERNELS = {"default": None,
           "two-per-wave": dict(small=0, tpw1=(0, 0), v8=(0, 0)),
           "one-per-wave": dict(small=0, tpw1=(0, 1 << 40), v8=(0, 0))}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("B", [1, 7, 64])
def test_hidden_interval_field_and_rk4_vs_oracle(dev, B, kernel):
    import fet_ode_amd as F
    from conftest import fused_ranges
    from oracle import torch_ref as O
    sd, y0, _ = _case()
    y = y0[:B].clone()
    t = torch.linspace(0, 3.5, 35, dtype=torch.float64)[:4]
    with torch.no_grad():
        f_ref = _oracle(sd)(y)
        s_ref, _ = O.rk4_with_states(_oracle(sd), y, t)
    with fused_ranges() as fr:
        if KERNELS[kernel] is not None:
            fr.set(**KERNELS[kernel])
        with torch.no_grad():
            f_gpu = _model(sd, dev)(y.to(dev)).cpu()
            s_gpu = F.odeint(F.autonomous(_model(sd, dev)), y.to(dev), t, method="rk4").cpu()
    # one field evaluation: the NaN pattern, and the finite values within 1e-5
    assert torch.equal(torch.isnan(f_gpu), torch.isnan(f_ref)), (f_gpu, f_ref)
    d = (torch.nan_to_num(f_gpu).double() - torch.nan_to_num(f_ref).double()).abs()
    print(f"B={B} {kernel}: field max abs diff {d.max().item():.3e}")
    assert bool((d <= 1e-5 * torch.nan_to_num(f_ref).double().abs() + 1e-5).all()), d.max().item()
    # three rk4 steps: the NaN pattern, and the finite trajectories within 1e-5 per slice
    assert torch.equal(torch.isnan(s_gpu), torch.isnan(s_ref)), "NaN pattern of the solve"
    fin = torch.isfinite(s_ref).all(-1).all(0)
    assert fin.any()
    err = _slice_rel_err(s_gpu[:, fin], s_ref[:, fin])
    print(f"B={B} {kernel}: rk4 3 steps max slice rel err {err:.3e}")
    assert err <= 1e-5, err
