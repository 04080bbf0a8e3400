"""The wave skew and the priority lift of the KAN-FET rk4 inference kernel at two trajectories per wave
(fetode_fused_set_wave_skew, fetode_fused_set_wave_prio: DESIGN.md §3 round 10) change when a wave
runs, never what it computes: solutions, hysteresis state, tape and gradients are bitwise the same at
every setting."""
import contextlib

import numpy as np
import pytest
import torch

from conftest import fused_ranges, golden_sd, load_golden

pytestmark = pytest.mark.gpu

# (skew units, lift per cent); the first is the reference: both off.  Skew: 1, the default (0, the
# reference itself) and s_sleep's maximum; lift: a share that rounds to no step on the short grid, a
# half, the default, the whole solve; and both knobs at their maxima together.
SETTINGS = [(0, 0), (1, 0), (127, 0), (0, 1), (0, 50), (0, 67), (0, 100), (127, 100)]


@contextlib.contextmanager
def two_per_wave():
    """Every batch on the two-trajectories-per-wave kernel; both knobs restored on exit."""
    from fet_ode_amd import _lib
    lib = _lib.load()
    skew, prio = lib.fetode_fused_set_wave_skew(-1), lib.fetode_fused_set_wave_prio(-1)
    with fused_ranges() as fr:
        fr.set(small=0, tpw1=(0, 0), v8=(0, 0))
        try:
            yield lib
        finally:
            lib.fetode_fused_set_wave_skew(skew)
            lib.fetode_fused_set_wave_prio(prio)


def _same(a, b):
    """Bitwise equality (a NaN equals the same NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _model(dev, kind):
    import fet_ode_amd as F
    m = (F.KANFET if kind == "kanfet" else F.KAN)([2, 10, 2], grid_size=5)
    m.load_state_dict(golden_sd(load_golden("traj_kanfet" if kind == "kanfet" else "traj_kan")))
    return m.to(dev)


def _two_solves(dev, lib, kind, B, npts, setting):
    """Two consecutive rk4 solves of a fresh model (the second starts from the first's hysteresis
    state): both solutions and the final prev_x of every Ferro layer."""
    import fet_ode_amd as F
    from oracle import torch_ref as O
    lib.fetode_fused_set_wave_skew(setting[0])
    lib.fetode_fused_set_wave_prio(setting[1])
    m = _model(dev, kind)
    t = torch.tensor(np.linspace(0, 3.5, 35))[:npts]
    y0 = O.lv_y0(B, seed=3).to(dev)
    with torch.no_grad():
        s1 = F.odeint(F.autonomous(m), y0, t, method="rk4")
        s2 = F.odeint(F.autonomous(m), s1[-1].contiguous(), t, method="rk4")
    state = [v.clone() for k, v in sorted(m.state_dict().items()) if k.endswith("prev_x")]
    return [s1, s2] + state


# B = 3: an odd tail (one invalid half-wave), no partner wave.  B = 2050: 1025 waves, one more than an
# MI355X has SIMDs, so one SIMD pair exists, the grid condition holds and both sides of the "younger
# wave" rule run.  B = 4096 on the 35-point grid: the headline launch, every SIMD a pair.
@pytest.mark.parametrize("B,npts", [(3, 6), (2050, 6), (4096, 35)])
def test_knobs_do_not_change_kanfet_results(dev, B, npts):
    with two_per_wave() as lib:
        ref = _two_solves(dev, lib, "kanfet", B, npts, SETTINGS[0])
        assert len(ref) == 4 and torch.isfinite(ref[0]).all()
        for setting in SETTINGS[1:] if npts == 6 else [(0, 67), (127, 100)]:
            got = _two_solves(dev, lib, "kanfet", B, npts, setting)
            for i, (a, b) in enumerate(zip(ref, got)):
                assert _same(a, b), (setting, i)


def test_knobs_do_not_touch_the_kan_kernel(dev):
    """The stateless KAN instantiation (FERRO = false) carries neither knob."""
    with two_per_wave() as lib:
        ref = _two_solves(dev, lib, "kan", 2050, 6, SETTINGS[0])
        for setting in [(127, 0), (0, 67), (127, 100)]:
            got = _two_solves(dev, lib, "kan", 2050, 6, setting)
            for a, b in zip(ref, got):
                assert _same(a, b), setting


def test_taped_solve_ignores_the_knobs(dev):
    """The taped (training) instantiation carries neither knob: at B = 2050 the tape and every gradient
    with both knobs at their maxima are bitwise those with both off."""
    import fet_ode_amd as F
    from oracle import torch_ref as O
    t = torch.tensor(np.linspace(0, 3.5, 35))[:6]
    w = torch.randn(6, 2050, 2, generator=torch.Generator().manual_seed(6)).to(dev)
    out = []
    with two_per_wave() as lib:
        for skew, prio in [(0, 0), (127, 100)]:
            lib.fetode_fused_set_wave_skew(skew)
            lib.fetode_fused_set_wave_prio(prio)
            m = _model(dev, "kanfet")
            y0 = O.lv_y0(2050, seed=3).to(dev).requires_grad_(True)
            sol = F.odeint(F.autonomous(m), y0, t, method="rk4")
            fn = sol.grad_fn   # the fused solve's node holds the tape (odeint.py _FusedFixedFn)
            while not hasattr(fn, "saved_tensors"):
                fn = fn.next_functions[0][0]
            tape = fn.saved_tensors[0].clone()
            assert tape.shape == (5 * 4, 2050, 12)
            (sol * w).sum().backward()
            out.append([sol.detach(), tape, y0.grad] + [p.grad for p in m.parameters() if p.grad is not None])
    assert len(out[0]) == len(out[1]) > 3
    for i, (a, b) in enumerate(zip(*out)):
        assert _same(a, b), i
