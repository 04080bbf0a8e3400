"""MI355X: the wide-layer kernels (fetode_wide.hip) across the shape family wide_supported() admits,
not only the ETT widths 64 / 128 of test_gpu_wide.py: layers with in >= 16, in % 8 == 0, out >= 16,
out % 16 == 0 run the MFMA layer forward under no_grad, the one-pass Ferro VJP and (64 / 128
outputs) the MFMA KANLinear VJP, whatever model they belong to.  The shapes come from
tests/test_wide_shape_family.py, which checks without a GPU that the predicate admits them and
computes which branch each one takes: 1 / 2 / 4 input slices, a single chunk per slice (no prefetch
iteration), odd chunk counts (3, 5, 9, 17), 1 .. 9 output blocks, the 1- and 2-output tails and the
half-filled last group block of the Ferro VJP, in / 4 = 4 .. 34 input quads of the KANLinear VJP.

Every case calls the wide entry point itself and asserts it answered (not None): a silent fall
back to the generic kernels cannot pass here.  References are the oracle (oracle/torch_ref.py) in
fp32 and fp64; the gradient references are the fp64 oracle's autograd."""
import pytest
import torch

import fet_ode_amd as F
from fet_ode_amd import _lib
from fet_ode_amd import autograd_ops as A
from oracle import torch_ref as O

from test_gpu_wide import _ferro_with_edges, _x, row_rel
from test_wide_shape_family import (FERRO_BWD_BATCHES, FERRO_BWD_SHAPES, FIELD_SHAPES, FORWARD_BATCHES,
                                    FORWARD_SHAPES, KAN_BWD_BATCHES, KAN_BWD_SHAPES)

pytestmark = pytest.mark.gpu

FERRO_NAMES = ("k", "Ec", "Ps", "bias", "coef")
POISON = -7.25e33            # guard rows around the output: never written
GUARD_LO, GUARD_HI = 8, 72   # rows before / after (the tile is 64 rows: a whole tile past B fits)


def _wild(B):
    """Rows with |gate_slope x| > 80: row 0, the last row, both sides of the first tile boundary."""
    return tuple(sorted({0, B - 1} | ({63, 64} if B > 64 else set())))


def _ref_rows(B, i, o, K):
    """Rows the CPU oracle evaluates: all of them, or — where (rows, in, out, K) would pass 12 M
    elements — the wild rows, the on-knot row, the first rows, both sides of every 64-row tile
    boundary and a random fill.  Rows are independent given their own prev_x, and more than one row
    keeps the first-call rule (as test_wide_kanfet_field_b8192_both_slice_branches)."""
    cap = 12_000_000 // (i * o * K)
    if B <= cap:
        return None
    keep = set(_wild(B)) | {B // 2} | set(range(8))
    keep |= {r for t in range(64, B, 64) for r in (t - 1, t)}
    g = torch.Generator().manual_seed(B + i)
    for r in torch.randperm(B, generator=g).tolist():
        if len(keep) >= cap:
            break
        keep.add(r)
    assert 2 <= len(keep) <= cap
    return torch.tensor(sorted(keep))


def _forward_guarded(kan, fer, x, reinit):
    """fetode_wide_layer_forward into rows [GUARD_LO, GUARD_LO + B) of a poisoned buffer; the rows
    around them must come back untouched (a tile writes rows < B only)."""
    entry = A.wide_plan(kan, fer, x.device)
    assert entry is not None
    plan, kd, fd, _ = entry
    B = x.shape[0]
    outf = fer.out_dim if fer is not None else kan.out_features
    buf = torch.full((GUARD_LO + B + GUARD_HI, outf), POISON, device=x.device, dtype=torch.float32)
    out = buf[GUARD_LO:GUARD_LO + B]
    prev = None if (fer is None or reinit) else fer._prev
    assert prev is None or (prev.shape == x.shape and prev.is_contiguous())
    byref = _lib.ctypes.byref
    _lib.check(_lib.load().fetode_wide_layer_forward(
        byref(kd) if kd is not None else None, byref(fd) if fd is not None else None, plan.data_ptr(),
        x.data_ptr(), B, _lib.ptr(prev), int(reinit), out.data_ptr(), A._stream(x)), "fetode_wide_layer_forward")
    assert bool((buf[:GUARD_LO] == POISON).all()), "rows before the output were written"
    assert bool((buf[GUARD_LO + B:] == POISON).all()), "rows at or beyond B were written"
    return out


@pytest.mark.parametrize("K", [10, 12])
@pytest.mark.parametrize("B", FORWARD_BATCHES)
@pytest.mark.parametrize("i,o", FORWARD_SHAPES)
def test_wide_forward_shape_family(dev, i, o, B, K):
    """KANLinear alone, Ferro alone and both in one launch (autograd_ops.wide_apply), three
    stateful calls (first-call rule, then prev_x) with |gs x| > 80 rows at row 0, the last row and
    the tile boundary (calls 0 and 2), a value exactly on a knot, and the |gs Ec| > 80 / negative Ec
    parameters of _ferro_with_edges.  Each output: finite; 1e-5 per row against the fp32 oracle;
    within 4 x the fp32 oracle's own distance + 1e-6 of the fp64 oracle; bitwise the same when
    written between poisoned guard rows, which stay untouched; prev_x = the input afterwards.

    Measured on the MI355X, worst err / bar over the 48 cases: against the fp32 oracle KANLinear 0.090,
    Ferro 0.056, layer 0.057; against the fp64 oracle 0.27, 0.18, 0.18."""
    torch.manual_seed(1000 * i + o + K)
    kan = F.KANLinear(i, o)
    ksd = {k: v.clone() for k, v in kan.state_dict().items()}
    fer = _ferro_with_edges(i, o, K, seed=i * o + K)
    kp = O.KANLinearParams.from_state_dict(ksd)
    kp64 = kp.to(torch.float64)
    fp = O.FerroParams(*(getattr(fer, n).detach().clone() for n in FERRO_NAMES))
    fp64 = fp.to(torch.float64)
    st32, st64 = O.FerroState(i, o, K), O.FerroState(i, o, K, torch.float64)
    knot = kan.grid[0, 5].item()
    rows = _ref_rows(B, i, o, K)
    kan, fer = kan.to(dev), fer.to(dev)
    for call in range(3):
        x = _x(B, i, seed=100 * call + i + B, wild_rows=_wild(B) if call != 1 else ()) * (1.0 + 0.05 * call)
        x[B // 2, 0] = knot
        xr = x if rows is None else x[rows]
        ek32, ek64 = O.kanlinear_forward(xr, kp), O.kanlinear_forward(xr.double(), kp64)
        ef32, ef64 = O.ferro_forward(xr, fp, st32), O.ferro_forward(xr.double(), fp64, st64)
        xd = x.to(dev)
        reinit = fer._needs_reinit(xd)
        assert reinit == (call == 0 and B > 1)
        for what, k_, f_, e32, e64 in (("kan", kan, None, ek32, ek64), ("ferro", None, fer, ef32, ef64),
                                       ("layer", kan, fer, ek32 + ef32, ek64 + ef64)):
            got = A.wide_apply(k_, f_, xd, reinit=reinit)
            assert got is not None, f"{what}: no wide kernel took ({i}, {o}, K = {K})"
            assert got.shape == (B, o) and torch.isfinite(got).all(), (what, call)
            assert torch.equal(got, _forward_guarded(k_, f_, xd, reinit)), (what, call)
            gr = got.cpu() if rows is None else got.cpu()[rows]
            e = row_rel(gr, e32)
            print(f"forward {what} ({i},{o}) B={B} K={K} call {call}: fp32 {e / 1e-5:.3f}", end="")
            assert e <= 1e-5, (what, call, e)
            err, spread = row_rel(gr, e64), row_rel(e32, e64)
            print(f" fp64 {err / (4 * spread + 1e-6):.3f}")
            assert err <= 4 * spread + 1e-6, (what, call, err, spread)
        fer._commit_state(xd, reinit)
        assert torch.equal(fer.prev_x[:, :, 0, 0].cpu(), x)


def _row_chunks(B, per_row):
    """Row ranges of at most 8 M reference elements, none of a single row (a one-row batch would
    not re-initialise the oracle's (1, in, out, K) state)."""
    n = max(2, 8_000_000 // per_row)
    parts = list(torch.arange(B).split(n))
    if len(parts) > 1 and len(parts[-1]) == 1:
        parts[-2:] = [torch.cat(parts[-2:])]
    return parts


def _ferro_ref_grads(p0, prev, x, g, K):
    """d/dx and the five parameter gradients of sum(g * Ferro(x)) by the fp64 oracle's autograd, the
    state advanced by one prior call on `prev` (None: the first-call rule).  Evaluated in fp64 on the
    device, in row chunks whose parameter gradients accumulate: the (B, in, out, K) expansion of the
    largest case is 70 M elements."""
    dev = x.device
    i, o = p0[0].shape[:2]
    pr = [t.to(dev, torch.float64).requires_grad_(True) for t in p0]
    pd = O.FerroParams(*[t.detach() for t in pr])
    gx = []
    for r in _row_chunks(x.shape[0], i * o * K):
        r = r.to(dev)
        st = O.FerroState(i, o, K, torch.float64)
        if prev is not None:
            with torch.no_grad():
                O.ferro_forward(prev[r].double(), pd, st)
        xr = x[r].double().requires_grad_(True)
        out = O.ferro_forward(xr, O.FerroParams(*pr), st)
        (out * g[r].double()).sum().backward()
        gx.append(xr.grad)
    return torch.cat(gx), [t.grad for t in pr]


@pytest.mark.parametrize("K", [10, 12])
@pytest.mark.parametrize("B", FERRO_BWD_BATCHES)
@pytest.mark.parametrize("i,o", FERRO_BWD_SHAPES)
def test_wide_ferro_backward_shape_family(dev, i, o, B, K):
    """The one-pass Ferro VJP (_ferro_backward_wide), stateful and first-call forms, inputs as
    test_wide_ferro_backward_one_pass (wild rows, direct-gate parameters).  Against the fp64 oracle's
    autograd: d/dx within 2e-4 of the tensor's max, each parameter gradient within 2e-4 max + 1e-7
    (the bars of test_wide_ferro_autograd_sequence_and_grads).  Against the generic two-kernel VJP:
    2e-5 per tame row, 2e-5 of max overall, 1e-4 max + 1e-7 on parameters.  A second run is bitwise
    identical; the accumulating form equals base + gx bitwise.

    Measured on the MI355X, worst err / bar over the 30 cases: against the oracle d/dx 0.003, parameters
    0.007 (k); against the generic VJP tame rows 0.11, max 0.081, parameters 0.017 (k)."""
    m = _ferro_with_edges(i, o, K, seed=3 * i + o + K)
    p0 = [getattr(m, n).detach().clone() for n in FERRO_NAMES]
    m = m.to(dev)
    wild = (1, B // 2, B - 1)
    x = _x(B, i, seed=B + K, wild_rows=wild).to(dev)
    prev = (_x(B, i, seed=B + K + 1, wild_rows=(2, B // 2)) * 0.7).to(dev)
    g = torch.randn(B, o, generator=torch.Generator().manual_seed(B + 3)).to(dev)
    want = (True,) * 5
    tame = torch.ones(B, dtype=torch.bool)
    tame[list(wild)] = False
    for reinit in (False, True):
        r = A._ferro_backward_wide(m, x, prev, reinit, g, True, want, None)
        assert r is not None, f"no one-pass Ferro VJP took ({i}, {o}, K = {K})"
        gx_w, gp_w = r
        gx_w2, gp_w2 = A._ferro_backward_wide(m, x, prev, reinit, g, True, want, None)
        assert torch.equal(gx_w, gx_w2) and all(torch.equal(a, b) for a, b in zip(gp_w, gp_w2))
        assert torch.isfinite(gx_w).all() and all(torch.isfinite(t).all() for t in gp_w)
        tag = f"ferro vjp ({i},{o}) B={B} K={K} reinit={int(reinit)}"
        # the fp64 oracle's autograd
        gx_o, gp_o = _ferro_ref_grads(p0, None if reinit else prev, x, g, K)
        assert torch.isfinite(gx_o).all()
        err = (gx_w.double() - gx_o).abs().max().item()
        bar = 2e-4 * gx_o.abs().max().item()
        print(f"{tag}: oracle gx {err / bar:.3f}", end="")
        assert err <= bar, (reinit, err, bar)
        for n, a, b in zip(FERRO_NAMES, gp_w, gp_o):
            err = (a.double() - b).abs().max().item()
            bar = 2e-4 * b.abs().max().item() + 1e-7
            print(f" {n} {err / bar:.3f}", end="")
            assert err <= bar, (reinit, n, err, bar)
        # the generic two-kernel VJP
        gx_r, gp_r = A._ferro_backward_generic(m, x, prev, reinit, None, g, True, want, None)
        e_row = row_rel(gx_w[tame], gx_r[tame])
        e_max = (gx_w - gx_r).abs().max().item() / gx_r.abs().max().item()
        print(f" | generic rows {e_row / 2e-5:.3f} max {e_max / 2e-5:.3f}", end="")
        assert e_row <= 2e-5, (reinit, e_row)
        assert e_max <= 2e-5, (reinit, e_max)
        for n, a, b in zip(FERRO_NAMES, gp_w, gp_r):
            err = (a - b).abs().max().item()
            bar = 1e-4 * b.abs().max().item() + 1e-7
            print(f" {n} {err / bar:.3f}", end="")
            assert err <= bar, (reinit, n, err, bar)
        print()
    # accumulate: d/dx added into an existing buffer, parameter sums from zero
    base = torch.randn(B, i, generator=torch.Generator().manual_seed(9)).to(dev)
    acc = base.clone()
    gx_a, gp_a = A._ferro_backward_wide(m, x, prev, False, g, True, (False, True, False, False, True), acc)
    assert gx_a is acc
    gx_w, gp_w = A._ferro_backward_wide(m, x, prev, False, g, True, want, None)
    assert torch.equal(acc, base + gx_w)            # the same fixed-order sum, added once
    assert gp_a[0] is None and torch.equal(gp_a[1], gp_w[1]) and torch.equal(gp_a[4], gp_w[4])


KAN_FIELDS = ("base_weight", "spline_weight", "spline_scaler", "a", "b", "logistic_weight", "logistic_scaler")


@pytest.mark.parametrize("B", KAN_BWD_BATCHES)
@pytest.mark.parametrize("i,o", KAN_BWD_SHAPES)
def test_wide_kanlinear_backward_shape_family(dev, i, o, B):
    """The MFMA KANLinear VJP (_kan_backward_wide) with randomised spline / logistic scalers.
    (a) x in [-3, 3] with one value on a knot, against the fp64 oracle's autograd: d/dx within 1e-4
    of max, each of the seven parameter gradients within 2e-4 max + 1e-7 (the bars of
    test_wide_kanlinear_autograd_forward_and_grads; the oracle's own autograd is NaN at x = 40).
    (b) with a row at x = 40, against the generic kernels at the bars of
    test_wide_kanlinear_backward_mfma (1e-5 per row, 2e-5 max + 1e-7), a second run bitwise
    identical, the accumulating and the parameters-only forms.

    Measured on the MI355X, worst err / bar over the 15 cases: against the oracle d/dx 0.004, parameters
    0.002; against the generic kernels rows 0.052, parameters 0.070 (logistic b)."""
    torch.manual_seed(i + 2 * o + B)
    m = F.KANLinear(i, o)
    with torch.no_grad():
        m.spline_scaler.mul_(torch.rand_like(m.spline_scaler) + 0.5)
        m.logistic_scaler.mul_(torch.rand_like(m.logistic_scaler) + 0.5)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(dev)
    x = _x(B, i, seed=B + i)
    x[0, 0] = sd["grid"][0, 5]                  # exactly on a knot
    gc = torch.randn(B, o, generator=torch.Generator().manual_seed(B))
    g = gc.to(dev)
    want = tuple(p is not None for p in A.kan_params(m))
    assert sum(want) == 7
    tag = f"kan vjp ({i},{o}) B={B}"
    # (a) the fp64 oracle's autograd
    r = A._kan_backward_wide(m, x.to(dev), g, True, want)
    assert r is not None, f"no MFMA KANLinear VJP took ({i}, {o})"
    gx_w, gp_w = r
    p = O.KANLinearParams.from_state_dict(sd).to(torch.float64)
    ps = []
    for f in KAN_FIELDS:
        t = getattr(p, f).clone().requires_grad_(True)
        setattr(p, f, t)
        ps.append(t)
    xr = x.double().requires_grad_(True)
    (O.kanlinear_forward(xr, p) * gc.double()).sum().backward()
    assert torch.isfinite(xr.grad).all()
    err = (gx_w.cpu().double() - xr.grad).abs().max().item()
    bar = 1e-4 * xr.grad.abs().max().item()
    print(f"{tag}: oracle gx {err / bar:.3f}", end="")
    assert err <= bar, (err, bar)
    for name, a, b in zip(A.KAN_PARAM_NAMES, gp_w, ps):
        assert a is not None and b.grad is not None and torch.isfinite(b.grad).all(), name
        err = (a.cpu().double() - b.grad).abs().max().item()
        bar = 2e-4 * b.grad.abs().max().item() + 1e-7
        print(f" {name} {err / bar:.3f}", end="")
        assert err <= bar, (name, err, bar)
    # (b) the generic kernels, a row far outside the grid
    x = x.to(dev)
    x[min(3, B - 1), :] = 40.0
    gx_w, gp_w = A._kan_backward_wide(m, x, g, True, want)
    gx_w2, gp_w2 = A._kan_backward_wide(m, x, g, True, want)
    gx_r, gp_r = A._kan_backward_generic(m, x, g, True, want)
    assert torch.equal(gx_w, gx_w2)
    assert all(a is None or torch.equal(a, b) for a, b in zip(gp_w, gp_w2))
    e = row_rel(gx_w, gx_r)
    print(f" | generic rows {e / 1e-5:.3f}", end="")
    assert e <= 1e-5, e
    n = 0
    for name, a, b in zip(A.KAN_PARAM_NAMES, gp_w, gp_r):
        if b is None:
            continue
        err = (a - b).abs().max().item()
        bar = 2e-5 * b.abs().max().item() + 1e-7
        print(f" {name} {err / bar:.3f}", end="")
        assert err <= bar, (name, err, b.abs().max().item())
        n += 1
    print()
    assert n == 7
    # accumulate into existing d/dx; parameters-only (no d/dx)
    base = torch.randn(B, i, generator=torch.Generator().manual_seed(2)).to(dev)
    acc = base.clone()
    _, gp_a = A._kan_backward_wide(m, x, g, True, want, acc)
    assert torch.equal(acc, base + gx_w)
    assert all(a is None or torch.equal(a, b) for a, b in zip(gp_a, gp_w))
    gx_n, gp_n = A._kan_backward_wide(m, x, g, False, want)
    assert gx_n is None and all(a is None or torch.equal(a, b) for a, b in zip(gp_n, gp_w))


@pytest.mark.parametrize("widths,K", FIELD_SHAPES)
def test_wide_field_autograd_shape_family(dev, monkeypatch, widths, K):
    """KANFET([32, 64, 32], K = 10) and KANFET([16, 128, 16], K = 12) under autograd: layer 0 runs
    _WideLayerFn (wide forward, MFMA KANLinear VJP, one-pass Ferro VJP), layer 1 the per-module path
    with the generic KANLinear VJP and the one-pass Ferro VJP.  Two stateful calls (first-call rule,
    then prev_x), B = 100, loss through both, as test_wide_kanfet_field_autograd_two_calls.

    Reference: the fp64 KANFETRef (oracle/torch_ref.py) under autograd — it carries gradients to
    every parameter and to x.  Bars: 1e-5 per row on both outputs, 1e-4 of max on d/dx, 1e-4 max +
    1e-7 on every parameter gradient.  The wide entry points are counted: layer 0's forward and
    KANLinear VJP twice, the one-pass Ferro VJP four times (both layers, both calls).

    Measured on the MI355X, worst err / bar over both cases: rows 0.12, d/dx 0.17, parameters 0.094."""
    calls = {"wide_apply": 0, "_kan_backward_wide": 0, "_ferro_backward_wide": 0}
    for name in calls:
        def spy(*a, _f=getattr(A, name), _n=name, **kw):
            r = _f(*a, **kw)
            calls[_n] += r is not None
            return r
        monkeypatch.setattr(A, name, spy)
    torch.manual_seed(21 + K)
    m = F.KANFET(widths, grid_size=5, num_fet_basis=K)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    pnames = [n for n, _ in m.named_parameters()]
    B, D = 100, widths[0]
    x1 = _x(B, D, seed=1) * 0.5
    x2 = _x(B, D, seed=2, wild_rows=(9,)) * 0.5
    w = torch.randn(B, D, generator=torch.Generator().manual_seed(3))
    m = m.to(dev)
    xa, xb = x1.to(dev).requires_grad_(True), x2.to(dev).requires_grad_(True)
    y1 = m(xa)
    y2 = m(xb)
    ((y1 * w.to(dev)).sum() + (y2 * y2).mean()).backward()
    assert calls == {"wide_apply": 2, "_kan_backward_wide": 2, "_ferro_backward_wide": 4}, calls
    sd64 = {k: (v.double().requires_grad_(True) if k in pnames else v.double()) for k, v in sd.items()}
    ref = O.KANFETRef.from_state_dict(sd64, 2)
    ra, rb = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    r1 = ref(ra)
    r2 = ref(rb)
    ((r1 * w.double()).sum() + (r2 * r2).mean()).backward()
    e1, e2 = row_rel(y1.detach(), r1.detach()), row_rel(y2.detach(), r2.detach())
    print(f"field {widths} K={K}: rows {e1 / 1e-5:.3f} {e2 / 1e-5:.3f}", end="")
    assert e1 <= 1e-5 and e2 <= 1e-5, (e1, e2)
    for got, exp in ((xa.grad, ra.grad), (xb.grad, rb.grad)):
        err = (got.cpu().double() - exp).abs().max().item()
        bar = 1e-4 * exp.abs().max().item()
        print(f" gx {err / bar:.3f}", end="")
        assert err <= bar, (err, bar)
    assert len(pnames) >= 20
    worst = 0.0
    for n, t in m.named_parameters():
        exp = sd64[n].grad
        assert t.grad is not None and exp is not None, n
        err = (t.grad.cpu().double() - exp).abs().max().item()
        bar = 1e-4 * exp.abs().max().item() + 1e-7
        worst = max(worst, err / bar)
        assert err <= bar, (n, err, bar)
    print(f" params {worst:.3f}")

