"""The multi-pass mode of the resident LV dopri5 launches (fetode_dopri5_set_multipass): a grid
smaller than the batch needs serves it in passes — inference, the taped training solve and the
reverse sweep.  The grid sums are formed over the virtual grid in the one-grid order and everything
a trajectory carries across a sum is parked raw (the sweep's gradient-sum registers included), so a
forced multi-pass run must equal the one-grid run of the same batch BITWISE: (1) and (2) tie the
multi-pass kernels to the one-grid kernels the oracle tests pin, (3) ties them to the host loop
beyond the natural grid, (4) is the timeout path."""
import numpy as np
import pytest
import torch

from conftest import fused_ranges, golden_sd, load_golden

pytestmark = pytest.mark.gpu

T3 = torch.tensor([0.0, 0.2, 0.5], dtype=torch.float64)


class knobs:
    """multipass / grid limit / spin limit / sweep shape and the fused kernel ranges, restored on exit."""

    def __enter__(self):
        from fet_ode_amd import _lib
        self.lib = _lib.load()
        self.fr = fused_ranges()
        self.fr.__enter__()
        self.mp = self.lib.fetode_dopri5_set_multipass(-1)
        self.limit = self.lib.fetode_dopri5_set_grid_limit(0)
        self.lib.fetode_dopri5_set_grid_limit(self.limit)
        self.shape = self.lib.fetode_integrate_dopri5_backward_set_shape(-1)
        self.spin = self.lib.fetode_dopri5_set_spin_limit(0)
        self.lib.fetode_dopri5_set_spin_limit(self.spin)
        return self

    def set(self, mp, limit=0):
        self.lib.fetode_dopri5_set_multipass(1 if mp else 0)
        self.lib.fetode_dopri5_set_grid_limit(limit)

    def __exit__(self, *exc):
        self.lib.fetode_dopri5_set_multipass(1 if self.mp else 0)
        self.lib.fetode_dopri5_set_grid_limit(self.limit)
        self.lib.fetode_integrate_dopri5_backward_set_shape(self.shape)
        self.lib.fetode_dopri5_set_spin_limit(self.spin)
        return self.fr.__exit__(*exc)


def _model(kind, dev):
    import fet_ode_amd as F
    g = load_golden("traj_kanfet" if kind == "kanfet" else "traj_kan")
    m = (F.KANFET if kind == "kanfet" else F.KAN)([2, 10, 2], grid_size=5)
    m.load_state_dict(golden_sd(g))
    return m.to(dev), g


def _y0(g, B, dev):
    return torch.from_numpy(g["y0_B64"]).repeat((B + 63) // 64, 1)[:B].to(dev).clone()


def _states(m, kind):
    return [l.ferro._prev.detach().cpu().clone() for l in m.layers] if kind == "kanfet" else []


def _infer(kind, dev, B, options=None, t=T3):
    """One inference solve: solution, hysteresis state, the attempt log, nfev, the attempt count."""
    import fet_ode_amd as F
    m, g = _model(kind, dev)
    with torch.no_grad():
        sol = F.odeint(F.autonomous(m), _y0(g, B, dev), t, rtol=1e-3, atol=1e-4, options=options).cpu()
    s = F.dopri5.dopri5_solve.last
    return sol, _states(m, kind), s


def _same_solve(a, b):
    (s0, st0, r0), (s1, st1, r1) = a, b
    assert torch.equal(s0, s1)
    assert len(st0) == len(st1) and all(torch.equal(x, y) for x, y in zip(st0, st1))
    assert r0.attempts == r1.attempts            # (t0, dt, error ratio, accepted) of every attempt
    assert r0.nfev == r1.nfev and r0.n_attempts == r1.n_attempts


# ---- (1) forced passes equal the single pass, bitwise: inference ----
@pytest.mark.parametrize("first_step", [None, 0.05], ids=["auto", "given"])
@pytest.mark.parametrize("kind", ["kanfet", "kan"])
@pytest.mark.parametrize("B,limits", [(7, (1, 2, 3)), (129, (8, 5))])
def test_forced_passes_equal_single_pass_inference(dev, kind, B, limits, first_step):
    """B = 7: 4 virtual workgroups, the last half-empty; limit 3 leaves a ragged last pass.  B = 129:
    65 virtual workgroups (more than the 64 leaf counters: leaves of two workgroups, a one-trajectory
    tail); limit 5 breaks the leaves' modulo-8 structure across passes."""
    from fet_ode_amd.dopri5 import ResidentSolve
    opts = None if first_step is None else {"first_step": first_step}
    with knobs() as k:
        k.fr.set(small=0)            # the reference is the v4 one-grid kernel
        k.set(False)
        ref = _infer(kind, dev, B, opts)
        assert isinstance(ref[2], ResidentSolve) and ref[2].n_attempts >= 2
        for limit in limits:
            k.set(True, limit)
            _same_solve(ref, _infer(kind, dev, B, opts))


@pytest.mark.parametrize("kind", ["kanfet", "kan"])
def test_forced_passes_raise_the_same_error(dev, kind):
    """max_num_steps too small for the first output interval: the same assertion in both runs."""
    msgs = []
    with knobs() as k:
        k.fr.set(small=0)
        for mp, limit in ((False, 0), (True, 2)):
            k.set(mp, limit)
            with pytest.raises(Exception) as ei:
                _infer(kind, dev, 7, {"max_num_steps": 1, "first_step": 0.01})
            msgs.append((type(ei.value), str(ei.value)))
    assert msgs[0] == msgs[1] and "max_num_steps" in msgs[0][1]


# ---- (2) forced passes equal the single pass: training ----
def _train(kind, dev, B, d5tape=None, t=T3):
    """loss = sol.square().sum(), y0 requires grad: solution, state, loss, d/d y0, parameter grads, nfev."""
    import fet_ode_amd as F
    from fet_ode_amd.dopri5 import ResidentSolve
    m, g = _model(kind, dev)
    if d5tape is not None:
        m._fetode_d5tape = d5tape
    y0 = _y0(g, B, dev).requires_grad_(True)
    sol = F.odeint(F.autonomous(m), y0, t, rtol=1e-3, atol=1e-4)
    s = F.dopri5.dopri5_solve.last
    assert isinstance(s, ResidentSolve)
    loss = sol.square().sum()
    loss.backward()
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
    return sol.detach().cpu(), _states(m, kind), loss.item(), y0.grad.cpu(), grads, s.nfev


def _same_train(a, b):
    assert torch.equal(a[0], b[0])
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert a[2] == b[2] and a[5] == b[5]
    assert torch.equal(a[3], b[3])
    for n in a[4]:    # the gradient sums are parked per virtual wave: bitwise too
        assert torch.equal(a[4][n], b[4][n]), n


@pytest.mark.parametrize("kind", ["kanfet", "kan"])
@pytest.mark.parametrize("B,limits", [(17, (1, 2)), (521, (5,))])
def test_forced_passes_equal_single_pass_training(dev, kind, B, limits):
    """B = 17: the sweep has 3 virtual workgroups of 8 trajectories (the last with one), the forward
    9.  B = 521: 66 sweep workgroups.  The reference is the one-grid solve and the one-grid sweep in
    the multi-pass sweep's shape (two trajectories per wave)."""
    with knobs() as k:
        k.fr.set(small=0)
        k.lib.fetode_integrate_dopri5_backward_set_shape(2)
        k.set(False)
        ref = _train(kind, dev, B)
        assert all(torch.isfinite(v).all() for v in ref[4].values()) and torch.isfinite(ref[3]).all()
        for limit in limits:
            k.set(True, limit)
            _same_train(ref, _train(kind, dev, B))


def test_tape_rerun_under_multipass(dev):
    """A tape too short for the solve (room for 2 attempts' log): the re-run with a roomy tape gives
    bitwise what the roomy tape gives at once."""
    with knobs() as k:
        k.fr.set(small=0)
        k.lib.fetode_integrate_dopri5_backward_set_shape(2)
        k.set(True, 2)
        roomy = _train("kanfet", dev, 17)
        assert roomy[5] > 2 + 6 * 2     # more than two attempts: the short log forces the re-run
        _same_train(roomy, _train("kanfet", dev, 17, d5tape=(8, 2)))


# ---- (3) beyond the natural grid ----
def _cap(kind, dev):
    """The one-grid cap of this field's training (solve and sweep), read at run time."""
    from fet_ode_amd import _lib
    from fet_ode_amd.autograd_ops import make_handle
    lib = _lib.load()
    m, _ = _model(kind, dev)
    h = make_handle(m, 64, dev)
    return min(lib.fetode_integrate_dopri5_max_batch(h.ref, 0), lib.fetode_integrate_dopri5_backward_max_batch(h.ref))


@pytest.mark.parametrize("kind", ["kanfet", "kan"])
def test_beyond_natural_grid_inference(dev, kind):
    """B = cap + 3 (cap: the field's one-grid training cap; the KAN inference grid alone still holds
    it): resident with the switch on; against the host loop the bars of
    test_dopri5_resident_matches_host_driven at B = 4096 (same accept pattern and nfev, dt within
    1e-5, solution and state within 1e-4); the natural grid equals a forced 1000 workgroups bitwise."""
    from fet_ode_amd.dopri5 import ResidentSolve, set_resident_dopri5
    B = _cap(kind, dev) + 3
    with knobs() as k:
        k.set(False)
        prev = set_resident_dopri5(False)    # the host loop (what the switch off gives beyond one grid)
        try:
            host = _infer(kind, dev, B)
        finally:
            set_resident_dopri5(prev)
        assert not isinstance(host[2], ResidentSolve)
        k.set(True)
        nat = _infer(kind, dev, B)
        assert isinstance(nat[2], ResidentSolve)
        k.set(True, 1000)
        _same_solve(nat, _infer(kind, dev, B))
    a0 = [(a[1], a[3]) for a in nat[2].attempts]
    a1 = [(float(a[1]), bool(a[3])) for a in host[2].attempts]
    assert nat[2].nfev == host[2].nfev and [a[1] for a in a0] == [a[1] for a in a1]
    np.testing.assert_allclose([a[0] for a in a0], [a[0] for a in a1], rtol=1e-5)
    s0, s1 = nat[0], host[0]
    assert ((s0 - s1).norm(dim=(1, 2)) / s1.norm(dim=(1, 2)).clamp_min(1e-30)).max() <= 1e-4
    for a, b in zip(nat[1], host[1]):
        assert ((a - b).norm() / b.norm()).item() <= 1e-4


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def test_beyond_natural_grid_training_kan(dev):
    """B = cap + 3, KAN: against host autograd with the bars of test_dopri5_train_bench_batch (same
    nfev, every tensor within 1e-3)."""
    import fet_ode_amd as F
    from fet_ode_amd.dopri5 import ResidentSolve
    B = _cap("kan", dev) + 3
    with knobs() as k:
        k.set(True)
        res = _train("kan", dev, B)
        k.set(False)     # beyond one grid the switch off is the host autograd
        m, g = _model("kan", dev)
        y0 = _y0(g, B, dev).requires_grad_(True)
        sol = F.odeint(F.autonomous(m), y0, T3, rtol=1e-3, atol=1e-4)
        s = F.dopri5.dopri5_solve.last
        assert not isinstance(s, ResidentSolve)
        sol.square().sum().backward()
    assert res[5] == s.nfev
    for n, p in m.named_parameters():
        assert _rel(res[4][n], p.grad.cpu()) <= 1e-3, n
    assert _rel(res[3], y0.grad.cpu()) <= 1e-3


def test_beyond_natural_grid_training_kanfet(dev):
    """B = cap + 3, KAN-FET: finite, bitwise reproducible, and bitwise equal under a forced limit."""
    B = _cap("kanfet", dev) + 3
    with knobs() as k:
        k.set(True)
        a = _train("kanfet", dev, B)
        b = _train("kanfet", dev, B)
        k.set(True, 100)
        c = _train("kanfet", dev, B)
    assert all(torch.isfinite(v).all() for v in a[4].values()) and torch.isfinite(a[3]).all()
    _same_train(a, b)
    _same_train(a, c)


# ---- (4) the timeout twin of test_dopri5_resident_timeout_restores_state ----
def test_multipass_timeout_restores_state(dev):
    """B = 7 in two physical workgroups with fetode_dopri5_set_spin_limit(1): the solve raises (status
    4), the hysteresis state is bitwise the pre-solve one, and the next solve with the limit restored
    succeeds.  (Two workgroups doing equal work run in lockstep; with a limit set the first poll is
    sampled at the last arrival, include/fetode.h, so the knob forces the path every time.)"""
    import fet_ode_amd as F
    from fet_ode_amd.dopri5 import ResidentSolve
    m, g = _model("kanfet", dev)
    y0 = _y0(g, 7, dev)
    with torch.no_grad():   # a carried (non-fresh) hysteresis state before the solve under test
        F.odeint(F.autonomous(m), y0, torch.tensor([0.0, 0.05], dtype=torch.float64), method="rk4")
    before = [l.ferro._prev.clone() for l in m.layers]
    with knobs() as k:
        k.set(True, 2)
        k.lib.fetode_dopri5_set_spin_limit(1)
        with torch.no_grad(), pytest.raises(RuntimeError, match="timed out"):
            F.odeint(F.autonomous(m), y0, T3, rtol=1e-3, atol=1e-4)
            torch.cuda.synchronize(dev)
        for a, b in zip(before, [l.ferro._prev for l in m.layers]):
            assert torch.equal(a, b), "the pre-solve hysteresis state must survive a timed-out solve"
        k.lib.fetode_dopri5_set_spin_limit(k.spin)
        with torch.no_grad():
            sol = F.odeint(F.autonomous(m), y0, T3, rtol=1e-3, atol=1e-4)
        assert isinstance(F.dopri5.dopri5_solve.last, ResidentSolve) and torch.isfinite(sol).all()
