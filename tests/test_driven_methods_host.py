"""Host side of the one-launch driven solve for euler, midpoint, rk4_classic and the step_size option
(DESIGN §4.22): the four C entries and what they decide before any launch, the knob and its environment
variable, the eligibility rules, the stage-time tables against _per_stage_fixed's expressions, and the
output composition between steps against the oracle's FixedGridODESolver.  No GPU."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import torch_ref as O

NEW = ("fetode_driven_grid", "fetode_driven_grid_tape", "fetode_driven_grid_backward", "fetode_driven_grid_backward_x")
FAKE = 0x1000


class Gpu(torch.Tensor):
    is_cuda = True


def _desc(L, H, D, K, bsign=None):
    return L.FerroDesc(H + D, H, K, *[FAKE] * 5, 10.0, 0.8, bsign, 0)


def _field(ecg, H=8, D=1, K=3, T=9):
    torch.manual_seed(0)
    f = ecg.InputDrivenKANODEFunc(D, H, K)
    t = torch.linspace(0.0, 1.0, steps=T)
    f.set_interpolator(ecg.LinearInterp1D(t, torch.randn(2, T, D)))
    return f, t


@pytest.fixture
def knob():
    from fet_ode_amd import ecg
    prev = ecg.set_fused_driven_methods(True)
    yield ecg
    ecg.set_fused_driven_methods(prev)


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
    for n in ("set_fused_driven_methods", "driven_grid_eligible", "driven_grid_recognise"):
        assert hasattr(F.ecg, n), n


def _calls(L, lib):
    """The four entries as f(desc, method, B, n_eval, eval0, n_steps, required pointer or None)."""
    def fwd(d, m, B, n_eval, eval0, n, p=FAKE):
        return lib.fetode_driven_grid(ctypes.byref(d), p, m, p, B, p, n_eval, eval0, p, n, None, p, None, None)

    def tape(d, m, B, n_eval, eval0, n, p=FAKE, tp=FAKE):
        return lib.fetode_driven_grid_tape(ctypes.byref(d), p, m, p, B, p, n_eval, eval0, p, n, None, p, None, tp, tp,
                                           None)

    def bwd(d, m, B, n_eval, eval0, n, p=FAKE):
        return lib.fetode_driven_grid_backward(ctypes.byref(d), p, m, B, p, n, None, p, p, p, p, p, None)

    def bwdx(d, m, B, n_eval, eval0, n, p=FAKE, au=FAKE):
        return lib.fetode_driven_grid_backward_x(ctypes.byref(d), p, m, B, p, n, None, p, p, p, p, p, au, None)

    return fwd, tape, bwd, bwdx


def test_abi_status_table():
    """Every status is decided before a launch (the pointers are fake: a launch would fault)."""
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    ok, bad = _desc(L, 8, 1, 3), _desc(L, 65, 1, 10)
    n_m = {L.EULER: 1, L.MIDPOINT: 2, L.RK4: 4, L.RK4_CLASSIC: 4}
    for f in _calls(L, lib):
        for m, nm in n_m.items():
            assert f(bad, m, 2, 64, 0, 2) == L.FETODE_EUNSUPPORTED                    # outside the family
            assert f(_desc(L, 8, 1, 3, bsign=0x2000), m, 2, 64, 0, 2) == L.FETODE_EUNSUPPORTED
            assert f(ok, m, 1 << 33, 64, 0, 2) == L.FETODE_EUNSUPPORTED               # more than 2^31 - 1 workgroups
            assert f(ok, m, 0, 64, 0, 2) == L.FETODE_OK and f(ok, m, -3, 64, 0, 2) == L.FETODE_OK
            assert f(ok, m, 2, 64, 0, 0) == L.FETODE_OK and f(ok, m, 2, 64, 0, -1) == L.FETODE_OK
            assert f(ok, m, 2, 64, 0, 2, None) == L.FETODE_EINVAL                      # null required pointers
        for m in (4, 5, -1, 17):                                                       # dopri5's code and others
            assert f(ok, m, 2, 64, 0, 2) == L.FETODE_EUNSUPPORTED
            assert f(ok, m, 0, 64, 0, 2) == L.FETODE_EUNSUPPORTED                      # before the empty-batch rule
    fwd, tape, bwd, bwdx = _calls(L, lib)
    for f in (fwd, tape):
        for m, nm in n_m.items():
            assert f(ok, m, 2, nm * 3 - 1, 0, 3) == L.FETODE_EINVAL                    # n_eval < eval0 + n_m n_steps
            assert f(ok, m, 2, nm * 3 + 1, 2, 3) == L.FETODE_EINVAL
            assert f(ok, m, 2, nm * 3, -1, 3) == L.FETODE_EINVAL
            if nm > 1:                                                                 # 2^31 evaluations or more
                assert f(ok, m, 2, 1 << 40, 0, (1 << 31) - 1) == L.FETODE_EUNSUPPORTED
    assert tape(ok, L.EULER, 2, 8, 0, 2, FAKE, None) == L.FETODE_EINVAL                # a taped solve needs its tape
    assert bwdx(ok, L.EULER, 2, 8, 0, 2, FAKE, None) == L.FETODE_EINVAL                # and the x sweep its adj_u
    # the old entries keep declining the other methods
    for m in (L.EULER, L.MIDPOINT, L.RK4_CLASSIC):
        assert lib.fetode_driven_fixed(ctypes.byref(ok), FAKE, m, FAKE, 2, FAKE, 8, 0, FAKE, 2, None, FAKE, None,
                                       None) == L.FETODE_EUNSUPPORTED


@pytest.mark.parametrize("env,expect", [(None, False), ("0", False), ("1", True), ("", False)])
def test_knob_env_and_return_value(env, expect):
    """Off by default; FETODE_DRIVEN_METHODS=1 turns it on at import.  The setter returns the previous value."""
    e = {k: v for k, v in os.environ.items() if k != "FETODE_DRIVEN_METHODS"}
    if env is not None:
        e["FETODE_DRIVEN_METHODS"] = env
    code = ("import sys; sys.path.insert(0, %r); from fet_ode_amd import ecg; S = ecg.set_fused_driven_methods; "
            "a = S(True); b = S(False); c = S(a); print(a, b, c, ecg._DRIVEN_METHODS[0], sep='|')" % REPO)
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout
    assert out.strip().split("|") == [str(expect), "True", "False", str(expect)]


def test_knob_off_solve_declines():
    from fet_ode_amd import ecg
    from fet_ode_amd.odeint import FIXED_METHODS
    f, t = _field(ecg)
    y0 = torch.zeros(2, 8).as_subclass(Gpu)
    prev = ecg.set_fused_driven_methods(False)
    try:
        with torch.no_grad():
            assert ecg.driven_solve(f, y0, t, t, None, False, FIXED_METHODS["euler"]) is None
            assert ecg.driven_solve(f, y0, t, t, 0.05, False, FIXED_METHODS["rk4"]) is None
            for m in FIXED_METHODS.values():
                assert not ecg.driven_grid_eligible(f, t, t, 0.05, False, m)
                assert ecg.driven_grid_recognise(f, y0, t, t, 0.05, False, m) is None
    finally:
        ecg.set_fused_driven_methods(prev)


def test_eligibility_rules(knob):
    ecg = knob
    from fet_ode_amd.odeint import FIXED_METHODS
    rk4 = FIXED_METHODS["rk4"]

    def elig(f, t, step_size=None, method=rk4, tc=None):
        tc = t.detach().cpu() if tc is None else tc
        rev = bool(tc[0] > tc[1])
        return ecg.driven_grid_eligible(f, t, -tc if rev else tc, step_size, rev, method)

    f, t = _field(ecg)
    for name, m in FIXED_METHODS.items():
        assert elig(f, t, 0.05, m) and elig(f, t, 1, m) and elig(f, t.clone(), 0.3, m), name
        assert elig(f, t, None, m) == (name != "rk4"), name       # plain rk4 is the old path's
        assert ecg.driven_eligible(f, t, t, None, False, m) == (name == "rk4"), name
        assert not ecg.driven_eligible(f, t, t, 0.05, False, m), name
        for bad in (0, 0.0, -0.05, math.inf, -math.inf, math.nan, "0.05", True, torch.tensor(0.05)):
            assert not elig(f, t, bad, m), (name, bad)
        assert not elig(f, torch.flip(t, [0]), 0.05, m)           # reversed time
        assert not elig(f, t.double(), 0.05, m)
        assert not elig(f, torch.linspace(0.0, 1.0, steps=8), 0.05, m)
    for m in (4, 7, -1, None):
        assert not elig(f, t, 0.05, m) and not elig(f, t, None, m)
    t2 = t.clone()
    t2[3] += 1e-3
    assert not elig(f, t2, 0.05)

    class Sub(ecg.InputDrivenKANODEFunc):
        pass

    torch.manual_seed(0)
    fs = Sub(1, 8, 3)
    fs.set_interpolator(ecg.LinearInterp1D(t, torch.randn(2, 9, 1)))
    assert not elig(fs, t, 0.05)
    hk = f.register_forward_hook(lambda *a: None)
    assert not elig(f, t, 0.05)
    hk.remove()
    assert elig(f, t, 0.05)
    fw, tw = _field(ecg, H=65)
    assert not elig(fw, tw, 0.05)
    prev = ecg.set_fused_driven(False)                             # the one-launch solves' master knob
    try:
        assert not elig(f, t, 0.05)
    finally:
        ecg.set_fused_driven(prev)
    # recognition: the tensor rules of driven_recognise, and a series that requires grad needs its knob
    y0 = torch.zeros(2, 8).as_subclass(Gpu)
    eul = FIXED_METHODS["euler"]
    rec = ecg.driven_grid_recognise(f, y0, t, t, None, False, eul)
    assert rec is not None and rec[0].shape == (2, 9, 1) and torch.equal(rec[1], t)
    assert ecg.driven_grid_recognise(f, torch.zeros(2, 8), t, t, None, False, eul) is None
    assert ecg.driven_grid_recognise(f, y0, t, t, None, False, rk4) is None
    assert ecg.driven_recognise(f, y0, t, t, None, False, eul) is None and \
        ecg.driven_recognise(f, y0, t, t, 0.05, False, rk4) is None
    x = torch.randn(2, 9, 1, requires_grad=True)
    f.set_interpolator(ecg.LinearInterp1D(t, x))
    pg = ecg.set_driven_series_grad(False)
    try:
        assert ecg.driven_grid_recognise(f, y0, t, t, 0.05, False, rk4) is None
        assert ecg.driven_solve(f, y0, t, t, 0.05, False, rk4) is None      # per stage
        ecg.set_driven_series_grad(True)
        assert ecg.driven_grid_recognise(f, y0, t, t, 0.05, False, rk4)[0] is x
    finally:
        ecg.set_driven_series_grad(pg)


def _host_stage_times(g, method):
    """_per_stage_fixed's scalar expressions, step by step, on the schedule's numpy grid."""
    out = []
    for s in range(len(g) - 1):
        t0, t1 = g[s], g[s + 1]
        hs = t1 - t0
        if method == "euler":
            out += [t0]
        elif method == "midpoint":
            out += [t0, t0 + 0.5 * (t1 - t0)]
        else:
            out += [t0, t0 + 0.5 * hs, t0 + 0.5 * hs, t0 + hs]
    assert all(type(v) is g.dtype.type for v in out)
    return np.asarray(out, dtype=g.dtype)


@pytest.mark.parametrize("grid", ["linspace", "uneven"])
@pytest.mark.parametrize("step_size", [None, 0.05])
def test_stage_time_tables_bitwise(grid, step_size):
    from fet_ode_amd import _lib, ecg
    from fet_ode_amd.odeint import FIXED_METHODS, get_schedule
    if grid == "linspace":
        tp = torch.linspace(0.0, 1.0, steps=9)
    else:
        g = torch.Generator().manual_seed(11)
        tp = torch.cumsum(torch.rand(9, generator=g) * 0.3 + 0.01, 0)
    sched = get_schedule(tp, step_size, False)
    for m in ("euler", "midpoint", "rk4_classic"):
        got = ecg.driven_stage_times(sched.grid, FIXED_METHODS[m])
        exp = _host_stage_times(sched.grid, m)
        assert got.dtype == torch.float32 and got.shape == (len(exp),)
        assert len(exp) == ecg._GRID_STAGES[FIXED_METHODS[m]] * sched.n_steps
        assert np.array_equal(got.numpy().view(np.int32), exp.view(np.int32)), m
    got = ecg.driven_stage_times(sched.grid, _lib.RK4)
    gt = torch.from_numpy(sched.grid.copy())
    assert torch.equal(got, ecg._driven_grid(gt, torch.device("cpu"))[1])              # _driven_grid's four


@pytest.mark.parametrize("step_size,what", [(0.0625, "divides"), (0.05, "does not divide"),
                                            (0.3, "wider than the knots")])
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_output_composition_vs_oracle(step_size, what, method):
    """A linear ODE on CPU: the oracle's solve on the schedule's own grid gives the state after every step;
    driven_grid_outputs of those rows must be the oracle's solve with the step_size option."""
    from fet_ode_amd import ecg
    from fet_ode_amd.odeint import get_schedule
    tp = torch.linspace(0.0, 1.0, steps=9)
    A = torch.tensor([[-0.5, 1.0, 0.0], [-1.0, -0.3, 0.2], [0.1, 0.0, -0.7]])
    y0 = torch.tensor([[1.0, -0.5, 0.25], [0.3, 0.8, -1.0]])
    func = lambda t, y: y @ A.T + t                                                  # noqa: E731
    sched = get_schedule(tp, step_size, False)
    modes = set(sched.out_mode[1:].tolist())
    if what == "divides":
        assert modes == {1} and sched.n_steps == 16
    elif what == "does not divide":
        # 20 steps; the last grid point is t's own end (FixedGridODESolver overwrites it), so the last step
        # is not the arange's; the knots at odd multiples of 0.125 fall inside a step
        assert modes == {1, 2} and sched.n_steps == 20 and sched.grid[-1] == np.float32(1.0)
    else:
        assert np.bincount(sched.out_step[1:]).max() >= 2 and 2 in modes and sched.n_steps == 4
    grid = torch.from_numpy(sched.grid.copy())
    assert torch.equal(grid[[0, -1]], tp[[0, -1]])
    sol_all = O.odeint(func, y0, grid, method=method)
    exp = O.odeint(func, y0, tp, method=method, options={"step_size": step_size})
    sel = ecg.driven_grid_selection(sched, torch.device("cpu"))
    assert sel is not None
    got = ecg.driven_grid_outputs(sol_all, sel)
    assert got.shape == exp.shape == (9, 2, 3) and torch.equal(got, exp), (got - exp).abs().max().item()
    assert ecg.driven_grid_selection(get_schedule(tp, None, False), torch.device("cpu")) is None


def test_encoder_solver_options():
    from fet_ode_amd import ecg
    e = ecg.OneODEEncoder(1, 8, 3, solver="euler")
    assert e.solver_options is None and "solver_options" not in e.state_dict()
    seen = {}

    def fake_odeint(func, y0, t, **kw):
        seen.update(kw)
        return torch.zeros(t.numel(), *y0.shape)

    real = ecg.odeint
    ecg.odeint = fake_odeint
    try:
        e._solve(torch.randn(2, 9, 1), torch.linspace(0.0, 1.0, steps=9))
        assert seen["options"] is None and seen["method"] == "euler"
        e.solver_options = {"step_size": 0.05}
        e._solve(torch.randn(2, 9, 1), torch.linspace(0.0, 1.0, steps=9))
        assert seen["options"] == {"step_size": 0.05}
    finally:
        ecg.odeint = real
