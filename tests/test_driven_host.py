"""Host-side logic of the input-driven (ECG NODE-RNN) path: the admitted family, the plan size, the
samples-per-workgroup knob, the recognition rules and the module surface.  No GPU."""
import os
import re
import subprocess

import pytest
import torch
import torch.nn as nn

from conftest import REPO, golden_sd, load_golden

LIB = os.path.join(REPO, "fet-ode_amd", "libfetode.so")
NEW = ("fetode_driven_supported", "fetode_driven_set_spw", "fetode_driven_plan_bytes", "fetode_driven_plan_build",
       "fetode_driven_table", "fetode_driven_fixed", "fetode_driven_fixed_tape", "fetode_driven_fixed_backward")


def _desc(L, H, D, K, bsign=None):
    fake = 0x1000
    return L.FerroDesc(H + D, H, K, *[fake] * 5, 10.0, 0.8, bsign, 0)


def test_symbols_exported_and_bound():
    import fet_ode_amd as F
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (fetode_\w+)", out))
    assert set(NEW) <= exported, set(NEW) - exported
    assert set(NEW) <= set(F._lib.SIGNATURES)
    hdr = open(os.path.join(REPO, "include", "fetode.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
    for n in ("LinearInterp1D", "InputDrivenKANODEFunc", "OneODEEncoder", "FullyNonlinearKANCell", "NODE_RNN",
              "set_fused_driven"):
        assert hasattr(F.ecg, n), n


def test_admitted_family_edges():
    import ctypes
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    sup = lambda *a, **k: lib.fetode_driven_supported(ctypes.byref(_desc(L, *a, **k)))   # noqa: E731
    # the issue's floor: D = 1..3, H up to 64, K up to 12; the family's own edges: D <= 4, K <= 16
    for H, D, K in ((1, 1, 1), (64, 1, 10), (64, 3, 12), (64, 4, 16), (8, 2, 3), (24, 3, 12)):
        assert sup(H, D, K) == 1, (H, D, K)
    for H, D, K in ((65, 1, 10), (64, 5, 10), (64, 1, 17), (64, 0, 10), (0, 1, 10), (64, 1, 0), (128, 1, 10)):
        assert sup(H, D, K) == 0, (H, D, K)
    assert sup(8, 1, 3, bsign=0x2000) == 0                      # an explicit branch_sign tensor
    assert lib.fetode_driven_supported(None) == 0
    d = L.FerroDesc(8, 9, 3, *[0x1000] * 5, 10.0, 0.8, None, 0)  # in_dim < out_dim
    assert lib.fetode_driven_supported(ctypes.byref(d)) == 0


def test_plan_bytes_and_unsupported_calls():
    import ctypes
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    for H, D, K in ((64, 1, 10), (8, 1, 3), (24, 3, 12)):
        # 4 constants per element + per output: sum bias*coef, gain, bias
        assert lib.fetode_driven_plan_bytes(ctypes.byref(_desc(L, H, D, K))) == 4 * (4 * (H + D) * H * K + 3 * H)
    assert lib.fetode_driven_plan_bytes(ctypes.byref(_desc(L, 64, 1, 10))) == 4 * (4 * 41600 + 192)
    bad = _desc(L, 65, 1, 10)
    assert lib.fetode_driven_plan_bytes(ctypes.byref(bad)) == -1
    fake = 0x1000
    assert lib.fetode_driven_plan_build(ctypes.byref(bad), fake, fake, fake, None) == L.FETODE_EUNSUPPORTED
    ok = _desc(L, 8, 1, 3)
    # outside the family / method: EUNSUPPORTED before anything is launched; a table too short: EINVAL
    assert lib.fetode_driven_fixed(ctypes.byref(bad), fake, L.RK4, fake, 2, fake, 8, 0, fake, 2, None, fake, None,
                                   None) == L.FETODE_EUNSUPPORTED
    for method in (L.EULER, L.MIDPOINT, L.RK4_CLASSIC):
        assert lib.fetode_driven_fixed(ctypes.byref(ok), fake, method, fake, 2, fake, 8, 0, fake, 2, None, fake,
                                       None, None) == L.FETODE_EUNSUPPORTED
        assert lib.fetode_driven_fixed_backward(ctypes.byref(ok), fake, method, 2, fake, 2, None, fake, fake, fake,
                                                fake, fake, None) == L.FETODE_EUNSUPPORTED
    assert lib.fetode_driven_fixed(ctypes.byref(ok), fake, L.RK4, fake, 2, fake, 7, 0, fake, 2, None, fake, None,
                                   None) == L.FETODE_EINVAL
    assert lib.fetode_driven_fixed(ctypes.byref(ok), fake, L.RK4, fake, 2, fake, 8, 4, fake, 2, None, fake, None,
                                   None) == L.FETODE_EINVAL
    assert lib.fetode_driven_fixed_tape(ctypes.byref(ok), fake, L.RK4, fake, 2, fake, 8, 0, fake, 2, None, fake, None,
                                        None, None, None) == L.FETODE_EINVAL   # a taped solve needs its tape
    assert lib.fetode_driven_table(fake, 4, fake, 1, fake, 2, 1, fake, None) == L.FETODE_EINVAL   # T >= 2


def test_spw_knob_contract():
    import fet_ode_amd as F
    f = F._lib.load().fetode_driven_set_spw
    prev = f(-1)
    try:
        assert prev in (0, 1, 2, 4) and f(-1) == prev
        assert f(1) == prev and f(-1) == 1
        for bad in (3, 5, 8, -7, 1 << 20):
            assert f(bad) == 1 and f(-1) == 1
        assert f(2) == 1 and f(4) == 2 and f(0) == 4 and f(-1) == 0
        assert F.ecg.set_driven_samples_per_workgroup(2) == 0 and F.ecg.set_driven_samples_per_workgroup(0) == 2
    finally:
        f(prev)


def _field(ecg, H=8, D=1, K=3, T=9, cls=None):
    torch.manual_seed(0)
    f = (cls or ecg.InputDrivenKANODEFunc)(D, H, K)
    t = torch.linspace(0.0, 1.0, steps=T)
    f.set_interpolator(ecg.LinearInterp1D(t, torch.randn(2, T, D)))
    return f, t


def test_recognition_rules():
    import fet_ode_amd as F
    from fet_ode_amd import ecg
    from fet_ode_amd.odeint import FIXED_METHODS
    rk4 = FIXED_METHODS["rk4"]

    def elig(f, t, step_size=None, method=rk4, tc=None):
        tc = t.detach().cpu() if tc is None else tc
        rev = bool(tc[0] > tc[1])
        return ecg.driven_eligible(f, t, -tc if rev else tc, step_size, rev, method)

    f, t = _field(ecg)
    assert elig(f, t)
    assert elig(f, t.clone())                         # another tensor holding the interpolator's grid
    assert not elig(f, t, step_size=0.05)
    assert not elig(f, torch.flip(t, [0]))            # decreasing grid
    assert not elig(f, torch.linspace(0.0, 1.0, steps=8))
    t2 = t.clone()
    t2[3] += 1e-3
    assert not elig(f, t2)                            # not the interpolator's grid
    assert not elig(f, t.double())
    for m in ("euler", "midpoint", "rk4_classic"):
        assert not elig(f, t, method=FIXED_METHODS[m])
    assert not elig(f, t, method=FIXED_METHODS.get("dopri5"))

    class Sub(ecg.InputDrivenKANODEFunc):
        pass

    fs, ts = _field(ecg, cls=Sub)
    assert not elig(fs, ts)
    fh, th = _field(ecg)
    hk = fh.register_forward_hook(lambda *a: None)
    assert not elig(fh, th)
    hk.remove()
    assert elig(fh, th)
    hk = fh.basis.register_forward_pre_hook(lambda *a: None)
    assert not elig(fh, th)
    hk.remove()

    class Interp(ecg.LinearInterp1D):
        pass

    ff, tf = _field(ecg)
    ff.set_interpolator(Interp(tf, torch.randn(2, 9, 1)))
    assert not elig(ff, tf)
    ff.set_interpolator(lambda tq: torch.zeros(1))
    assert not elig(ff, tf)
    fw, tw = _field(ecg, H=65)                        # outside the kernel's family
    assert not elig(fw, tw)
    fb, tb = _field(ecg)
    fb.basis._bsign = -torch.ones(1, 9, 8, 3)         # a loaded branch_sign that is not all ones
    assert not elig(fb, tb)
    prev = ecg.set_fused_driven(False)
    try:
        assert prev is True and not elig(f, t)
        assert ecg.set_fused_driven(True) is False
        assert elig(f, t)
    finally:
        ecg.set_fused_driven(prev)
    assert F.ecg.NODE_RNN is ecg.NODE_RNN


def test_module_surface_matches_the_reference_state_dict():
    """Constructor arguments, parameter names, state_dict keys and shapes, and the init RNG order (the
    fixture's state_dict was drawn from the reference classes under the same seed; gain / bias were
    moved afterwards)."""
    from fet_ode_amd import ecg
    g = load_golden("node_rnn")
    sd = golden_sd(g)
    torch.manual_seed(41)
    m = ecg.NODE_RNN(input_size=1, hidden_size=8, num_classes=2, num_basis=3, solver="rk4")
    own = m.state_dict()
    assert list(own) == list(sd)
    for k, v in own.items():
        exp = sd[k]
        if "prev_x" in k or "branch_sign" in k:
            assert v.shape == exp.shape and v.dtype == exp.dtype, k
        elif k in ("enc.odefunc.gain", "enc.odefunc.bias"):
            assert torch.equal(v, torch.ones(8) if k.endswith("gain") else torch.zeros(8)), k
        else:
            assert torch.equal(v, exp), k            # same init distributions in the same RNG order
    m.load_state_dict(sd)
    back = m.state_dict()
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    assert isinstance(m.enc.lift, nn.Linear) and m.enc.solver == "rk4" and m.enc.return_traj is True
    assert ecg.NODE_RNN().enc.odefunc.basis.in_dim == 65   # the ECG200 defaults: D = 1, H = 64, K = 10
    with pytest.raises(RuntimeError):
        m(torch.randn(2, 9, 1))                      # no CPU path
