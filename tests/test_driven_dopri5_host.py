"""Host-side logic of the one-launch dopri5 solve of the input-driven field: the recognition rules,
the knob and its environment variable, what the C entry decides before any launch, and the per-sample
record.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO


def _desc(L, H, D, K, bsign=None):
    fake = 0x1000
    return L.FerroDesc(H + D, H, K, *[fake] * 5, 10.0, 0.8, bsign, 0)


def _field(ecg, H=8, D=1, K=3, T=9, cls=None):
    torch.manual_seed(0)
    f = (cls or ecg.InputDrivenKANODEFunc)(D, H, K)
    t = torch.linspace(0.0, 1.0, steps=T)
    f.set_interpolator(ecg.LinearInterp1D(t, torch.randn(2, T, D)))
    return f, t


def test_eligibility_rules():
    from fet_ode_amd import ecg
    from fet_ode_amd.odeint import FIXED_METHODS

    def elig(f, t, rtol=1e-3, atol=1e-4, options=None, tc=None):
        tc = t.detach().cpu() if tc is None else tc
        rev = bool(tc[0] > tc[1])
        return ecg.driven_dopri5_eligible(f, t, -tc if rev else tc, rev, rtol, atol, options or {})

    f, t = _field(ecg)
    assert elig(f, t) and elig(f, t.clone()) and elig(f, None, tc=t.clone())
    assert elig(f, t, rtol=1, atol=0)
    # the fixed-grid rule is untouched: never eligible for dopri5
    assert not ecg.driven_eligible(f, t, t, None, False, FIXED_METHODS.get("dopri5"))
    # scalar tolerances and only the scalar step options
    assert not elig(f, t, rtol=torch.tensor(1e-3)) and not elig(f, t, atol=[1e-4] * 8) and not elig(f, t, rtol=True)
    opts = {"first_step": 0.05, "safety": 0.8, "ifactor": 5.0, "dfactor": 0.3, "min_step": 0.0, "max_step": 0.5,
            "max_num_steps": 100}
    assert elig(f, t, options=opts)
    for k in ("norm", "step_t", "jump_t", "perturb", "norm_group", "replay"):
        assert not elig(f, t, options={k: None}), k
    # the grid: the interpolator's own, increasing, fp32, forward in time
    assert not elig(f, torch.flip(t, [0]))
    assert not elig(f, torch.linspace(0.0, 1.0, steps=8))
    t2 = t.clone()
    t2[3] += 1e-3
    assert not elig(f, t2) and not elig(f, t.double())

    class Sub(ecg.InputDrivenKANODEFunc):
        pass

    fs, ts = _field(ecg, cls=Sub)
    assert not elig(fs, ts)
    fh, th = _field(ecg)
    hk = fh.register_forward_hook(lambda *a: None)
    assert not elig(fh, th)
    hk.remove()
    assert elig(fh, th)

    class Interp(ecg.LinearInterp1D):
        pass

    ff, tf = _field(ecg)
    ff.set_interpolator(Interp(tf, torch.randn(2, 9, 1)))
    assert not elig(ff, tf)
    fw, tw = _field(ecg, H=65)
    assert not elig(fw, tw)
    fb, tb = _field(ecg)
    fb.basis._bsign = -torch.ones(1, 9, 8, 3)
    assert not elig(fb, tb)
    # the knob
    prev = ecg.set_resident_driven_dopri5(False)
    try:
        assert not elig(f, t)
        assert ecg.set_resident_driven_dopri5(True) is False
        assert elig(f, t)
    finally:
        ecg.set_resident_driven_dopri5(prev)
    # without a GPU tensor nothing is launched: the solve declines, the encoder has no CPU path
    assert ecg.driven_dopri5_solve(f, torch.zeros(2, 8), t, False, 1e-3, 1e-4, {}) is None
    assert ecg.driven_dopri5_odeint(f, torch.zeros(1, 8), t, False, 1e-3, 1e-4, {}) is None
    with pytest.raises(RuntimeError):
        ecg.OneODEEncoder(1, 8, 3, solver="dopri5")(torch.randn(2, 9, 1))


@pytest.mark.parametrize("env,expect", [(None, True), ("0", False), ("1", True), ("", True)])
def test_knob_env(env, expect):
    """The path is on by default (faster than the host loop at B = 1 and B = 8 at both
    tolerance pairs); FETODE_DRIVEN_DOPRI5=0 turns it off at import.  The setter returns the previous
    value."""
    e = {k: v for k, v in os.environ.items() if k != "FETODE_DRIVEN_DOPRI5"}
    if env is not None:
        e["FETODE_DRIVEN_DOPRI5"] = env
    code = ("import sys; sys.path.insert(0, %r); from fet_ode_amd import ecg; "
            "p = ecg.set_resident_driven_dopri5(False); q = ecg.set_resident_driven_dopri5(True); print(p, q)" % REPO)
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout
    assert out.split() == [str(expect), "False"]


def test_abi_decides_before_any_launch():
    import fet_ode_amd as F
    from fet_ode_amd.dopri5 import _TABLEAU, _opts_array
    L = F._lib
    lib = L.load()
    fake = 0x1000
    tab = _TABLEAU.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def call(d, B=2, T=9, h0=fake, opts=None, sol=fake, stats=fake, att=fake, max_att=8, max_ev=0, tableau=tab):
        o = _opts_array(opts or {})
        return lib.fetode_driven_dopri5(ctypes.byref(d), fake, h0, B, fake, fake, T, 1e-3, 1e-4,
                                        o.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), tableau, None, sol, None,
                                        stats, att, max_att, None, max_ev, None)

    ok = _desc(L, 8, 1, 3)
    # outside the family: EUNSUPPORTED, whatever else is wrong
    for H, D, K in ((65, 1, 10), (64, 5, 10), (64, 1, 17), (0, 1, 3)):
        assert call(_desc(L, H, D, K)) == L.FETODE_EUNSUPPORTED, (H, D, K)
    assert call(_desc(L, 8, 1, 3, bsign=0x2000)) == L.FETODE_EUNSUPPORTED
    assert call(_desc(L, 65, 1, 10), T=1) == L.FETODE_EUNSUPPORTED
    # bad sizes and null pointers: EINVAL
    assert call(ok, T=1) == L.FETODE_EINVAL and call(ok, T=0) == L.FETODE_EINVAL
    assert call(ok, B=-1) == L.FETODE_EINVAL
    assert call(ok, max_att=-1) == L.FETODE_EINVAL and call(ok, max_ev=-1) == L.FETODE_EINVAL
    for kw in ({"h0": None}, {"sol": None}, {"stats": None}, {"att": None}, {"tableau": None}):
        assert call(ok, **kw) == L.FETODE_EINVAL, kw
    assert b"null pointer" in lib.fetode_last_error()
    # an empty batch is done, with nothing launched (the null pointers are not even looked at)
    assert call(ok, B=0) == L.FETODE_OK and call(ok, B=0, h0=None, sol=None) == L.FETODE_OK
    # step options under which a rejected step need not shrink, without a bound on the steps
    for o in ({"min_step": 1e-3}, {"safety": 1.0}, {"dfactor": 1.0}, {"dfactor": 2.0, "max_num_steps": (1 << 20) + 1}):
        assert call(ok, opts=o) == L.FETODE_EUNSUPPORTED, o
    assert b"max_num_steps" in lib.fetode_last_error()


def test_per_sample_record():
    from fet_ode_amd import ecg
    stats = torch.tensor([[13, 2, 0], [7, 1, 3], [1, 0, 1]], dtype=torch.int32)
    att = torch.full((3, 4, 4), float("nan"), dtype=torch.float64)
    att[0, 0] = torch.tensor([0.0, 0.5, 2.0, 0.0])
    att[0, 1] = torch.tensor([0.0, 0.25, 0.5, 1.0])
    att[1, 0] = torch.tensor([0.0, 2.0, 1.5, 0.0])
    rec = ecg.DrivenDopri5Solve(stats, att, None)
    assert rec.nfev == [13, 7, 1] and rec.n_attempts == [2, 1, 0] and rec.status == [0, 3, 1]
    assert rec.attempts == [[(0.0, 0.5, 2.0, False), (0.0, 0.25, 0.5, True)], [(0.0, 2.0, 1.5, False)], []]
    one = rec.sample(0)
    assert (one.nfev, one.n_attempts, one.attempts) == (13, 2, rec.attempts[0])
    with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(sample 1\)"):
        rec.raise_for_status()
    ecg.DrivenDopri5Solve(stats[:1], att[:1], None).raise_for_status()
    # the count stays exact beyond the log
    long = ecg.DrivenDopri5Solve(torch.tensor([[61, 10, 0]], dtype=torch.int32), torch.zeros(1, 4, 4, dtype=torch.float64),
                                 None)
    assert long.n_attempts == [10] and len(long.attempts[0]) == 4
    assert np.isfinite(ecg._DRIVEN_MAX_TRACE) and ecg._DRIVEN_MAX_TRACE >= 256
