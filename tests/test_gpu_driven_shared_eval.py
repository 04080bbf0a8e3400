"""One statement of the driven field's evaluation across the solvers (csrc/fetode_driven_dev.h, DESIGN
§4.23): evaluation 0 of the taped dopri5 solve, of the taped rk4 solve and of the taped euler grid solve
reads the same h0, prev0 and x(t[0]) through the same gate, element loop and meeting of the partial sums,
so its taped input row and pre-activation are the same bits in all three, in every samples-per-workgroup
variant of the fixed-grid kernels.  first_step is given, so the dopri5 solve's evaluation 0 is followed by
an attempt, not by the probe; nothing after evaluation 0 is compared."""
import ctypes

import pytest
import torch

import test_gpu_driven as G

pytestmark = pytest.mark.gpu
SHAPES = [(8, 1, 3), (24, 3, 12), (64, 4, 16)]
T, B, MAX_ATT = 3, 3, 8


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d-D%d-K%d" % s)
def test_evaluation_0_is_the_same_bits_in_every_solver(dev, shape):
    from fet_ode_amd import _lib, ecg
    from fet_ode_amd.dopri5 import _TABLEAU, _opts_array
    from fet_ode_amd.odeint import FIXED_METHODS, get_schedule
    H, D, K = shape
    In, lib = H + D, _lib.load()
    g = torch.Generator().manual_seed(31 * H + 7 * D + K)
    x = torch.randn(B, T, D, generator=g).to(dev)
    h0 = torch.randn(B, H, generator=g).to(dev)
    prev0 = torch.randn(B, In, generator=g).to(dev)
    f = G.gpu_field(H, D, K, dev)
    plan, d, keep = ecg._driven_plan(f, dev)
    tc = torch.linspace(0.0, 1.0, steps=T)
    nan = float("nan")

    # the taped dopri5 solve: rows (B, max_ev, .)
    max_ev = 2 + 6 * MAX_ATT
    opts = _opts_array({"first_step": 0.1})
    tg = tc.to(dev)
    sol, pout = torch.full((T, B, H), nan, device=dev), torch.full((B, In), nan, device=dev)
    stats = torch.full((B, 3), -1, device=dev, dtype=torch.int32)
    att = torch.zeros(B, MAX_ATT, 4, device=dev, dtype=torch.float64)
    hx5, phi5 = torch.full((B, max_ev, In), nan, device=dev), torch.full((B, max_ev, H), nan, device=dev)
    t5, sl5 = torch.full((B, max_ev), nan, device=dev), torch.full((B, max_ev, D), nan, device=dev)
    init = torch.zeros(B, 5, device=dev, dtype=torch.float64)
    _lib.check(lib.fetode_driven_dopri5_tape(
        ctypes.byref(d), plan.data_ptr(), h0.data_ptr(), B, x.data_ptr(), tg.data_ptr(), T, 1e-3, 1e-4,
        opts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _TABLEAU.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        prev0.data_ptr(), sol.data_ptr(), pout.data_ptr(), stats.data_ptr(), att.data_ptr(), MAX_ATT, hx5.data_ptr(),
        phi5.data_ptr(), t5.data_ptr(), sl5.data_ptr(), init.data_ptr(), max_ev, None), "fetode_driven_dopri5_tape")
    assert bool((stats[:, 0] >= 7).all()), stats.tolist()          # f0 and one attempt at least
    assert torch.isfinite(hx5[:, 0]).all() and torch.isfinite(phi5[:, 0]).all()
    assert torch.equal(hx5[:, 0], torch.cat([h0, x[:, 0]], dim=1))  # the input row is cat[h0, x(t[0])] itself

    def fixed_grid_tapes(family, method):
        """(tape_hx, tape_phi), rows (n_ev, B, .), of fetode_driven_<family>_tape on the same plan and inputs"""
        code = FIXED_METHODS[method]
        if family == "fixed":
            _, tq, coef = ecg._driven_grid(tc, dev)
        else:
            tq, coef, _ = ecg._driven_grid_arrays(get_schedule(tc, None, False), code, dev)
        ne = tq.numel()
        u = ecg.driven_table(tg, x, tq)
        s, p = torch.full((T - 1, B, H), nan, device=dev), torch.full((B, In), nan, device=dev)
        thx, tphi = torch.full((ne, B, In), nan, device=dev), torch.full((ne, B, H), nan, device=dev)
        name = "fetode_driven_%s_tape" % family
        _lib.check(getattr(lib, name)(ctypes.byref(d), plan.data_ptr(), code, h0.data_ptr(), B, u.data_ptr(), ne, 0,
                                      coef.data_ptr(), T - 1, prev0.data_ptr(), s.data_ptr(), p.data_ptr(),
                                      thx.data_ptr(), tphi.data_ptr(), None), name)
        return thx, tphi

    for v in G.SPW:
        with G.spw(v):
            for family, method in (("fixed", "rk4"), ("grid", "euler")):
                thx, tphi = fixed_grid_tapes(family, method)
                assert torch.equal(thx[0], hx5[:, 0]), (family, v, "hx")
                assert torch.equal(tphi[0], phi5[:, 0]), (family, v, "phi")
