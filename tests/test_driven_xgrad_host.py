"""Host-side logic of the gradient to the driving series in the one-launch driven solves:
the knob, its environment variable and its return value, who declines and who accepts a series that
requires grad, which entries the two backwards call, and what the three C entries decide before any
launch.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO
from test_driven_dopri5_host import _desc, _field
from test_driven_param_grad_host import _field_ctx, fake   # noqa: F401  (fake: a fixture)

NEW = ("fetode_driven_fixed_backward_x", "fetode_driven_dopri5_backward_x", "fetode_driven_table_backward",
       "fetode_driven_table_backward_workspace")


class Gpu(torch.Tensor):
    is_cuda = True


def test_symbols_exported_and_bound():
    import fet_ode_amd as F
    lib = os.path.join(REPO, "fet-ode_amd", "libfetode.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (fetode_\w+)", out))
    assert set(NEW) <= exported, set(NEW) - exported
    assert set(NEW) <= set(F._lib.SIGNATURES)
    hdr = open(os.path.join(REPO, "include", "fetode.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s


@pytest.mark.parametrize("env,expect", [(None, False), ("0", False), ("1", True), ("", False)])
def test_knob_env_and_return_value(env, expect):
    """Off by default; FETODE_DRIVEN_XGRAD=1 turns it on at import.  The setter returns the previous value."""
    e = {k: v for k, v in os.environ.items() if k != "FETODE_DRIVEN_XGRAD"}
    if env is not None:
        e["FETODE_DRIVEN_XGRAD"] = env
    code = ("import sys; sys.path.insert(0, %r); from fet_ode_amd import ecg; S = ecg.set_driven_series_grad; "
            "a = S(True); b = S(False); c = S(a); print(a, b, c, ecg._DRIVEN_XGRAD[0], sep='|')" % REPO)
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout
    assert out.strip().split("|") == [str(expect), "True", "False", str(expect)]


def test_rk4_recognition_declines_and_accepts():
    from fet_ode_amd import ecg
    from fet_ode_amd.odeint import FIXED_METHODS
    rk4 = FIXED_METHODS["rk4"]
    f, t = _field(ecg)
    y0 = torch.zeros(2, 8).as_subclass(Gpu)
    x = torch.randn(2, 9, 1, requires_grad=True)
    f.set_interpolator(ecg.LinearInterp1D(t, x))
    prev = ecg.set_driven_series_grad(False)
    try:
        assert ecg.driven_recognise(f, y0, t, t, None, False, rk4) is None          # today's decline
        with torch.no_grad():
            rec = ecg.driven_recognise(f, y0, t, t, None, False, rk4)
        assert rec is not None and not rec[0].requires_grad
        ecg.set_driven_series_grad(True)
        rec = ecg.driven_recognise(f, y0, t, t, None, False, rk4)
        assert rec is not None and rec[0] is x                                      # attached
        with torch.no_grad():
            assert not ecg.driven_recognise(f, y0, t, t, None, False, rk4)[0].requires_grad
        # a 2-D series shared by the batch goes in as its expand: autograd sums the rows
        x2 = torch.randn(9, 1, requires_grad=True)
        f.set_interpolator(ecg.LinearInterp1D(t, x2))
        xe = ecg.driven_recognise(f, y0, t, t, None, False, rk4)[0]
        assert xe.shape == (2, 9, 1) and xe.requires_grad and xe.data_ptr() == x2.data_ptr()
        # the rules are otherwise unchanged
        assert ecg.driven_recognise(f, y0, t, t, 0.1, False, rk4) is None
        assert ecg.driven_recognise(f, y0, t, t, None, False, FIXED_METHODS["euler"]) is None
        assert ecg.driven_recognise(f, torch.zeros(2, 8), t, t, None, False, rk4) is None
        f.set_interpolator(ecg.LinearInterp1D(t, torch.randn(2, 9, 1, dtype=torch.float64, requires_grad=True)))
        assert ecg.driven_recognise(f, y0, t, t, None, False, rk4) is None
    finally:
        ecg.set_driven_series_grad(prev)


def test_dopri5_train_declines_and_accepts(monkeypatch):
    from fet_ode_amd import ecg
    f, t = _field(ecg)
    y0 = torch.zeros(2, 8).as_subclass(Gpu)
    x = torch.randn(2, 9, 1, requires_grad=True)
    f.set_interpolator(ecg.LinearInterp1D(t, x))
    seen = []

    class Stub:
        last = "record"

        @staticmethod
        def apply(*a):
            seen.append(a)
            return "solution"

    monkeypatch.setattr(ecg, "_DrivenDopri5Fn", Stub)
    monkeypatch.setattr(ecg, "_driven_plan", lambda func, dev: object())
    train = lambda: ecg.driven_dopri5_train(f, y0, t, False, 1e-3, 1e-4, {}, reset=True, t=t)   # noqa: E731
    ptrain = ecg.set_resident_driven_dopri5_training(True)
    prev = ecg.set_driven_series_grad(False)
    try:
        for p in f.parameters():
            p.requires_grad_(False)
        assert train() is None and not seen                     # today's decline
        ecg.set_driven_series_grad(True)
        assert train() == ("solution", "record") and seen[0][1] is x and seen[0][3] is y0
        with torch.no_grad():
            assert train() is None
        ecg.set_resident_driven_dopri5_training(False)          # the training knob off: nobody
        assert train() is None and len(seen) == 1
        ecg.set_resident_driven_dopri5_training(True)
        x.requires_grad_(False)                                 # nothing requires grad
        assert train() is None and len(seen) == 1
        assert ecg.driven_dopri5_solve(f, y0, t, False, 1e-3, 1e-4, {"norm": None}) is None
    finally:
        ecg.set_driven_series_grad(prev)
        ecg.set_resident_driven_dopri5_training(*ptrain)


def test_encoder_declines_before_anything_is_set_up():
    from fet_ode_amd import ecg
    t = torch.linspace(0.0, 1.0, steps=9)
    ptrain = ecg.set_resident_driven_dopri5_training(True)
    prev = ecg.set_driven_series_grad(False)
    try:
        for xg, tr, past in ((False, True, False), (True, False, False), (False, False, False), (True, True, True)):
            ecg.set_driven_series_grad(xg)
            ecg.set_resident_driven_dopri5_training(tr)
            enc = ecg.OneODEEncoder(1, 8, 3, solver="dopri5")
            # on the CPU nothing is launched: None either way; the interpolator tells how far it got
            assert enc._solve_dopri5(torch.randn(2, 9, 1, requires_grad=True), t) is None
            assert (enc.odefunc._interp is not None) == past, (xg, tr)
    finally:
        ecg.set_driven_series_grad(prev)
        ecg.set_resident_driven_dopri5_training(*ptrain)


def test_rk4_backward_takes_the_x_entries_only_for_a_series_gradient(fake):   # noqa: F811
    from fet_ode_amd import ecg
    H, D, B, n_steps, T = 8, 1, 3, 2, 3
    f, d, keep, params = _field_ctx(ecg)
    ne = 4 * n_steps
    thx, tphi = torch.randn(ne, B, H + D), torch.randn(ne, B, H)
    grids = (torch.linspace(0, 1, T), torch.rand(ne), torch.ones(n_steps))
    ctx = SimpleNamespace(f=f, n_steps=n_steps, d=d, keep=keep, plan=torch.zeros(4), grids=grids,
                          saved_tensors=(grids[2], torch.zeros(B, H + D), thx, tphi, *params),
                          needs_input_grad=(False, True, False, False) + (False,) * 7)
    out = ecg._DrivenFn.backward(ctx, torch.randn(n_steps + 1, B, H))
    # only the series requires grad: no parameter sums of either kind, no d/dh0 returned
    assert fake.names() == ["fetode_driven_fixed_backward_x", "fetode_driven_table_backward_workspace",
                            "fetode_driven_table_backward"]
    assert out[1].shape == (B, T, D) and all(g is None for g in out[:1] + out[2:])
    a = fake.calls[-1][1]
    # the shared stage times, the knots, the (n_ev, B, D) layout, no nfev
    assert a[:4] == (grids[1].data_ptr(), 0, grids[0].data_ptr(), T) and a[5:9] == (B, ne, 1, B)
    assert a[9] is None and a[11] == D and a[12] == out[1].data_ptr() and a[13] is not None
    assert fake.calls[0][1][12] == a[4]                      # the sweep's adj_u is what the gather reads
    fake.calls.clear()
    ctx.needs_input_grad = (False, False, False, True) + (True,) * 7
    out = ecg._DrivenFn.backward(ctx, torch.randn(n_steps + 1, B, H))
    assert fake.names()[0] == "fetode_driven_fixed_backward" and out[1] is None
    assert not any(n.endswith("_x") or "table" in n for n in fake.names())


def test_dopri5_backward_takes_the_x_entries_only_for_a_series_gradient(fake):   # noqa: F811
    from fet_ode_amd import ecg
    from fet_ode_amd.dopri5 import _opts_array
    H, D, B, T, max_att = 8, 1, 2, 5, 4
    max_ev = 2 + 6 * max_att
    f, d, keep, params = _field_ctx(ecg)
    stats = torch.tensor([[14, 2, 0], [8, 1, 0]], dtype=torch.int32)
    tape = SimpleNamespace(hx=torch.zeros(B, max_ev, H + D), phi=torch.zeros(B, max_ev, H), slope=torch.zeros(B, max_ev, D),
                           t=torch.zeros(B, max_ev), init=torch.zeros(B, 5, dtype=torch.float64),
                           att=torch.zeros(B, max_att, 4, dtype=torch.float64), stats=stats, opts=_opts_array({}),
                           max_ev=max_ev, max_att=max_att)
    rec = ecg.DrivenDopri5Solve(stats, tape.att, None)
    ctx = SimpleNamespace(f=f, d=d, keep=keep, plan=torch.zeros(4), tape=tape, rec=rec, tg=torch.linspace(0, 1, T),
                          prev0=None, tols=(1e-2, 1e-3), step_grad=False, saved_tensors=tuple(params),
                          needs_input_grad=(False, True) + (False,) * 13)
    try:
        out = ecg._DrivenDopri5Fn.backward(ctx, torch.randn(T, B, H))
        assert fake.names() == ["fetode_driven_dopri5_backward_x", "fetode_driven_table_backward_workspace",
                                "fetode_driven_table_backward"]
        assert out[1].shape == (B, T, D) and all(g is None for g in out[:1] + out[2:])
        sweep, a = fake.calls[0][1], fake.calls[-1][1]
        assert sweep[19] == 0 and len(sweep) == 24              # step_grad as given, adj_u before the stream
        # the taped times, the (B, max_ev, D) layout up to the longest solve, stats as nfev with stride 3
        assert a[:4] == (tape.t.data_ptr(), max_ev, ctx.tg.data_ptr(), T) and a[4] == sweep[22]
        assert a[5:9] == (B, 14, max_ev, 1) and a[9] == stats.data_ptr() and a[10] == 3 and a[11] == D
        fake.calls.clear()
        ctx.needs_input_grad = (False,) * 3 + (True,) + (False,) * 4 + (True,) * 7
        out = ecg._DrivenDopri5Fn.backward(ctx, torch.randn(T, B, H))
        assert fake.names()[0] == "fetode_driven_dopri5_backward" and out[1] is None
        assert not any(n.endswith("_x") or "table" in n for n in fake.names())
    finally:
        ecg._DrivenDopri5Fn.last_adj = None


def test_abi_decides_before_any_launch():
    import fet_ode_amd as F
    from fet_ode_amd.dopri5 import _TABLEAU, _opts_array
    L = F._lib
    lib = L.load()
    fake_p = 0x1000
    tab = _TABLEAU.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    opts = _opts_array({})

    def rk4(d, method=L.RK4, B=2, adj_u=fake_p, adj=fake_p):
        return lib.fetode_driven_fixed_backward_x(ctypes.byref(d), fake_p, method, B, fake_p, 2, None, fake_p, fake_p,
                                                  fake_p, adj, fake_p, adj_u, None)

    def d5(d, B=2, T=9, stats=fake_p, adj_u=fake_p, max_ev=50, step_grad=0):
        return lib.fetode_driven_dopri5_backward_x(ctypes.byref(d), fake_p, B, fake_p, T, 1e-3, 1e-4,
                                                   opts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), tab, None, stats,
                                                   fake_p, 8, fake_p, fake_p, fake_p, fake_p, max_ev, fake_p, step_grad,
                                                   fake_p, fake_p, adj_u, None)

    ok = _desc(L, 8, 1, 3)
    for call in (rk4, d5):
        for H, D, K in ((65, 1, 10), (64, 5, 10), (64, 1, 17), (0, 1, 3)):
            assert call(_desc(L, H, D, K)) == L.FETODE_EUNSUPPORTED, (H, D, K)
        assert call(_desc(L, 8, 1, 3, bsign=0x2000)) == L.FETODE_EUNSUPPORTED
        assert call(_desc(L, 65, 1, 10), adj_u=None) == L.FETODE_EUNSUPPORTED
        assert call(ok, adj_u=None) == L.FETODE_EINVAL and b"null pointer" in lib.fetode_last_error()
        assert call(ok, B=0) == L.FETODE_OK and call(ok, B=0, adj_u=None) == L.FETODE_OK
    for method in (L.EULER, L.MIDPOINT, L.RK4_CLASSIC):
        assert rk4(ok, method=method) == L.FETODE_EUNSUPPORTED
    assert rk4(ok, adj=None) == L.FETODE_EINVAL
    assert d5(ok, T=1) == L.FETODE_EINVAL and d5(ok, stats=None) == L.FETODE_EINVAL and d5(ok, max_ev=0) == L.FETODE_EINVAL

    def tb(tq=fake_p, tq_sb=0, tg=fake_p, T=9, adj_u=fake_p, B=2, n_ev=8, sb=1, se=2, nfev=None, ns=0, D=1, gx=fake_p):
        return lib.fetode_driven_table_backward(tq, tq_sb, tg, T, adj_u, B, n_ev, sb, se, nfev, ns, D, gx, None, None)

    assert tb(T=1) == L.FETODE_EINVAL and tb(D=0) == L.FETODE_EINVAL
    for kw in ({"B": 0}, {"B": -1}, {"n_ev": 0}, {"n_ev": -3}, {"B": 0, "tq": None, "gx": None, "sb": 0}):
        assert tb(**kw) == L.FETODE_OK, kw                      # nothing to do: nothing is looked at
    for kw in ({"tq": None}, {"tg": None}, {"adj_u": None}, {"gx": None}):
        assert tb(**kw) == L.FETODE_EINVAL, kw
    assert b"null pointer" in lib.fetode_last_error()
    for kw in ({"sb": 0}, {"se": 0}, {"sb": -1}, {"tq_sb": -1}, {"nfev": fake_p, "ns": 0}):
        assert tb(**kw) == L.FETODE_EINVAL, kw
    assert b"stride" in lib.fetode_last_error()
    assert tb(B=1 << 31) == L.FETODE_EUNSUPPORTED and tb(T=1 << 24, D=4) == L.FETODE_EUNSUPPORTED
    # the gather keeps its pairs in LDS: no workspace today, whatever the sizes
    for B, n in ((2, 8), (256, 386), (0, 0), (-1, 5)):
        assert lib.fetode_driven_table_backward_workspace(B, n) == 0
