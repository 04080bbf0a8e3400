"""Host-side logic of training through the one-launch dopri5 solve of the input-driven field: the knob,
its environment variable and its return value, who takes the new path, what the two C entries decide
before any launch, the cap -> rerun decision and the prev-row shift of the parameter-sum pass.  No GPU."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO
from test_driven_dopri5_host import _desc, _field


@pytest.mark.parametrize("env,expect", [(None, False), ("0", False), ("1", True), ("", False)])
def test_knob_env_and_return_value(env, expect):
    """Off by default; FETODE_DRIVEN_DOPRI5_TRAIN=1 turns it on at import.  The setter returns the previous
    (enabled, step_grad), which restores it."""
    e = {k: v for k, v in os.environ.items() if k != "FETODE_DRIVEN_DOPRI5_TRAIN"}
    if env is not None:
        e["FETODE_DRIVEN_DOPRI5_TRAIN"] = env
    code = ("import sys; sys.path.insert(0, %r); from fet_ode_amd import ecg; "
            "S = ecg.set_resident_driven_dopri5_training; "
            "a = S(True, step_grad=False); b = S(False); c = S(*a); d = S(False); print(a, b, c, d, sep='|')" % REPO)
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout
    first = str((expect, True))
    assert out.strip().split("|") == [first, "(True, False)", "(False, True)", first]


def test_who_takes_the_new_path():
    from fet_ode_amd import ecg
    assert ecg._DRIVEN_DOPRI5_TRAIN == [False, True] or os.environ.get("FETODE_DRIVEN_DOPRI5_TRAIN") == "1"
    f, t = _field(ecg)
    y0 = torch.zeros(1, 8, requires_grad=True)
    prev = ecg.set_resident_driven_dopri5_training(False)
    try:
        # the knob off: nobody
        assert ecg.driven_dopri5_train(f, y0, t, False, 1e-3, 1e-4, {}) is None
        enc = ecg.OneODEEncoder(1, 8, 3, solver="dopri5")
        assert enc._solve_dopri5(torch.randn(2, 9, 1), t) is None and enc.odefunc._interp is None
        ecg.set_resident_driven_dopri5_training(True)
        # without autograd, and without a GPU tensor, nothing is launched
        with torch.no_grad():
            assert ecg.driven_dopri5_train(f, y0, t, False, 1e-3, 1e-4, {}) is None
        assert ecg.driven_dopri5_train(f, y0, t, False, 1e-3, 1e-4, {}) is None
        assert ecg.driven_dopri5_odeint(f, y0, t, False, 1e-3, 1e-4, {}) is None
        # a driving series that requires grad is declined before anything is set up
        assert enc._solve_dopri5(torch.randn(2, 9, 1, requires_grad=True), t) is None and enc.odefunc._interp is None
        # the rules are driven_dopri5_eligible's: the shared input check asks it
        asked = []
        real = ecg.driven_dopri5_eligible
        ecg.driven_dopri5_eligible = lambda *a: asked.append(a) or real(*a)
        try:
            class Gpu(torch.Tensor):
                is_cuda = True
            y = torch.zeros(1, 8).as_subclass(Gpu)
            assert ecg._driven_dopri5_inputs(f, y, t, False, 1e-3, 1e-4, {"norm": None}, t) is None and len(asked) == 1
            assert ecg._driven_dopri5_inputs(f, y, torch.flip(t, [0]), False, 1e-3, 1e-4, {}, None) is None
            assert len(asked) == 2
        finally:
            ecg.driven_dopri5_eligible = real
    finally:
        ecg.set_resident_driven_dopri5_training(*prev)


def test_abi_decides_before_any_launch():
    import fet_ode_amd as F
    from fet_ode_amd.dopri5 import _TABLEAU, _opts_array
    L = F._lib
    lib = L.load()
    fake = 0x1000
    tab = _TABLEAU.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def tape(d, B=2, T=9, h0=fake, opts=None, sol=fake, stats=fake, att=fake, max_att=8, hx=fake, phi=fake, tt=fake,
             slope=fake, init=fake, max_ev=50, tableau=tab):
        o = _opts_array(opts or {})
        return lib.fetode_driven_dopri5_tape(ctypes.byref(d), fake, h0, B, fake, fake, T, 1e-3, 1e-4,
                                             o.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), tableau, None, sol, None,
                                             stats, att, max_att, hx, phi, tt, slope, init, max_ev, None)

    def back(d, B=2, T=9, stats=fake, att=fake, max_att=8, hx=fake, phi=fake, slope=fake, init=fake, max_ev=50,
             gsol=fake, adj=fake, gh0=fake, tableau=tab, step_grad=1):
        o = _opts_array({})
        return lib.fetode_driven_dopri5_backward(ctypes.byref(d), fake, B, fake, T, 1e-3, 1e-4,
                                                 o.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), tableau, None, stats,
                                                 att, max_att, hx, phi, slope, init, max_ev, gsol, step_grad, adj, gh0,
                                                 None)

    ok = _desc(L, 8, 1, 3)
    for call in (tape, back):
        # outside the family: EUNSUPPORTED, whatever else is wrong
        for H, D, K in ((65, 1, 10), (64, 5, 10), (64, 1, 17), (0, 1, 3)):
            assert call(_desc(L, H, D, K)) == L.FETODE_EUNSUPPORTED, (H, D, K)
        assert call(_desc(L, 8, 1, 3, bsign=0x2000)) == L.FETODE_EUNSUPPORTED
        assert call(_desc(L, 65, 1, 10), T=1) == L.FETODE_EUNSUPPORTED
        # bad sizes and null pointers: EINVAL
        assert call(ok, T=1) == L.FETODE_EINVAL and call(ok, B=-1) == L.FETODE_EINVAL
        assert call(ok, max_att=-1) == L.FETODE_EINVAL and call(ok, max_ev=0) == L.FETODE_EINVAL
        for k in ("stats", "att", "hx", "phi", "slope", "init", "tableau"):
            assert call(ok, **{k: None}) == L.FETODE_EINVAL, (call.__name__, k)
        assert b"null pointer" in lib.fetode_last_error()
        # an empty batch is done, with nothing launched (the null pointers are not even looked at)
        assert call(ok, B=0) == L.FETODE_OK and call(ok, B=0, stats=None, hx=None) == L.FETODE_OK
    for kw in ({"h0": None}, {"sol": None}, {"tt": None}):
        assert tape(ok, **kw) == L.FETODE_EINVAL, kw
    for kw in ({"gsol": None}, {"adj": None}, {"gh0": None}, {"max_att": 0}):
        assert back(ok, **kw) == L.FETODE_EINVAL, kw
    # the cases the forward declines
    for o in ({"min_step": 1e-3}, {"safety": 1.0}, {"dfactor": 1.0}, {"dfactor": 2.0, "max_num_steps": (1 << 20) + 1}):
        assert tape(ok, opts=o) == L.FETODE_EUNSUPPORTED, o
    assert b"max_num_steps" in lib.fetode_last_error()


def test_cap_to_rerun_decision():
    """From a fabricated stats: the solve is run again only where a sample's exact attempt count exceeds
    the cap, with room for the longest sample."""
    from fet_ode_amd import ecg
    stats = torch.tensor([[2 + 6 * 5, 5, 0], [2 + 6 * 70, 70, 0], [2 + 6 * 64, 64, 0]], dtype=torch.int32)
    rec = ecg.DrivenDopri5Solve(stats, torch.zeros(3, 64, 4, dtype=torch.float64), None)
    assert ecg.tape_attempts_needed(rec.n_attempts, 64) == 70
    assert ecg.tape_attempts_needed(rec.n_attempts, 70) == 0 and ecg.tape_attempts_needed(rec.n_attempts, 128) == 0
    assert ecg.tape_attempts_needed([64, 3], 64) == 0 and ecg.tape_attempts_needed([65, 3], 64) == 65
    assert ecg.tape_attempts_needed([], 64) == 0
    assert ecg._DRIVEN_TAPE_ATTEMPTS == 64
    # the default cap at B = 256, H = 64, D = 1: about 50 MB of tape
    max_ev = 2 + 6 * ecg._DRIVEN_TAPE_ATTEMPTS
    assert 256 * max_ev * (65 + 64 + 1 + 1) * 4 < 55e6


def test_prev_row_shift():
    """prev of a taped row is the preceding row of the SAME sample; a sample's row 0 has the initial
    prev (or the reset state's zeros), never the last row of the sample before it."""
    from fet_ode_amd import ecg
    thx = torch.arange(2 * 4 * 3, dtype=torch.float32).view(2, 4, 3) + 1.0
    prev0 = -torch.ones(2, 3) * torch.tensor([[1.0], [2.0]])
    p = ecg.tape_prev_rows(thx, prev0)
    assert p.shape == thx.shape
    assert torch.equal(p[:, 1:], thx[:, :-1]) and torch.equal(p[:, 0], prev0)
    z = ecg.tape_prev_rows(thx, None)
    assert torch.equal(z[:, 1:], thx[:, :-1]) and not z[:, 0].any()
    assert not torch.equal(z[1, 0], thx[0, -1])
