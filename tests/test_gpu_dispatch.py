"""Every rk4 inference kernel fetode_integrate_fixed dispatches to (launch_fused: v6, v8 at two and at
one trajectory per workgroup, one trajectory per wave, two per wave), each forced at every batch
and pinned to the CPU oracle:

  (a) one step from the oracle's own (y_j, hysteresis state_j) at EVERY step of the bench horizon:
      y_{j+1} within 1e-5 per slice and the state the kernel leaves against the oracle's;
  (b) one launch == the same solve split into two launches, bitwise (solution and state): ties the
      in-kernel state carry over the whole horizon, schedule chunk reloads included, to the
      launch-boundary carry that (a) pins to the oracle;
  (c) the schedule code each kernel carries its own copy of (32 steps / 32 outputs staged in LDS,
      reloaded at chunk edges, a loop for several outputs inside one step) on the stateless, well
      conditioned KAN field, whole trajectories against the oracle within 1e-5 per slice.

All CPU oracle work is at B <= 129 and shared between the legs (computed once, never modified).
"""
import numpy as np
import pytest
import torch

from conftest import golden_sd, load_golden
from test_gpu_parity import DISPATCH_LEGS, REL, _set_states, forced_dispatch_leg, slice_rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(params=list(DISPATCH_LEGS))
def leg(request):
    with forced_dispatch_leg(request.param) as name:
        yield name


# ---------------------------------------------------------------------------------------------
# the bench workload's model at small batches: seed-0 KAN-FET [2, 10, 2], lv_y0(B, 0), 35 points
# ---------------------------------------------------------------------------------------------
_CACHE = {}


def _bench_sd():
    if "sd" not in _CACHE:
        import fet_ode_amd as F
        torch.manual_seed(0)
        _CACHE["sd"] = {k: v.clone() for k, v in F.KANFET([2, 10, 2], grid_size=5).state_dict().items()}
    return _CACHE["sd"]


def _bench_t():
    return torch.tensor(np.linspace(0, 3.5, 35))


def _bench_model(dev):
    import fet_ode_amd as F
    m = F.KANFET([2, 10, 2], grid_size=5)
    m.load_state_dict(_bench_sd())
    return m.to(dev)


def _layer_rel(a, r):
    return ((a.double() - r.double()).norm() / r.double().norm().clamp_min(1e-30)).item()


def _teacher(B):
    """The oracle's rk4 solve on this host with its (y_j, state_j) records, the state after the last
    step appended, and the worst teacher-forced one-step distance of three 6e-8 re-roundings of the
    oracle from it (y per slice, hysteresis state normwise per layer): what rounding alone gives."""
    key = ("teacher", B)
    if key not in _CACHE:
        from oracle import parity as P
        from oracle import torch_ref as O
        sd, t = _bench_sd(), _bench_t()
        ref = O.KANFETRef.from_state_dict(sd, 2)
        with torch.no_grad():
            sol, recs = O.rk4_with_states(ref, O.lv_y0(B, 0), t)
        states = [prevs for _, prevs in recs] + [[s.prev_x[:, :, 0, 0].clone() for s in ref.states]]
        tt = t
        worst_y, worst_s = 0.0, [0.0, 0.0]
        for sdp in P.perturbed_state_dicts(sd, 3, seed=4242):
            r = O.KANFETRef.from_state_dict(sdp, 2)
            f = lambda t_, yy: r(yy)
            for j, (y, prevs) in enumerate(recs):
                for st, p, fp in zip(r.states, prevs, r.ferro):   # the record's state, as _set_states
                    st.prev_x = p[:, :, None, None].expand(-1, -1, fp.k.shape[1], fp.k.shape[2]).clone()
                with torch.no_grad():
                    y1 = y + O.rk4_alt_step(f, tt[j], tt[j + 1] - tt[j], tt[j + 1], y)
                worst_y = max(worst_y, slice_rel_err(y1[None], sol[j + 1:j + 2]))
                for li, st in enumerate(r.states):
                    worst_s[li] = max(worst_s[li], _layer_rel(st.prev_x[:, :, 0, 0], states[j + 1][li]))
        _CACHE[key] = (sol, recs, states, worst_y, worst_s)
    return _CACHE[key]


@pytest.mark.parametrize("B", [7, 129])
def test_one_step_parity_at_every_step(dev, leg, B):
    """(a) From the oracle's own (y_j, state_j), each of the 34 steps under the forced kernel lands
    on the oracle's y_{j+1} within 1e-5 (per-slice relative; re-rounded references land at <= 3.6e-6
    at B = 7, <= 1.5e-6 at B = 129; a per-trajectory 1e-5 bar is not viable, re-roundings alone reach
    1.8e-5) and leaves the oracle's hysteresis state: per layer, normwise within max(1e-5, 4 x the
    worst of three re-rounded references driven the same way) (the factor of the envelope rules in
    test_gpu_ecg.py; measured references: layer 0 <= 4.5e-6, layer 1, the hidden h, 1.2e-5 ... 1.8e-5
    at B = 129 and 3.5e-5 at B = 7).  B odd: the last v8x2 / two-per-wave workgroup is half empty."""
    import fet_ode_amd as F
    sol, recs, states, ref_y, ref_s = _teacher(B)
    t = _bench_t()
    m = _bench_model(dev)
    worst_y, worst_s = 0.0, [0.0, 0.0]
    for j, (y, prevs) in enumerate(recs):
        _set_states(m, prevs, dev)
        with torch.no_grad():
            out = F.odeint(F.autonomous(m), y.to(dev), t[j:j + 2], method="rk4").cpu()
        worst_y = max(worst_y, slice_rel_err(out[1:], sol[j + 1:j + 2]))
        for li, layer in enumerate(m.layers):
            got = layer.ferro._prev.cpu()
            assert got.shape == states[j + 1][li].shape, (leg, j, li)
            worst_s[li] = max(worst_s[li], _layer_rel(got, states[j + 1][li]))
    bars = [max(1e-5, 4 * r) for r in ref_s]
    msg = (f"{leg} B={B}: y {worst_y:.3e} (re-rounded references {ref_y:.3e}, bar {REL}); state per layer "
           f"{worst_s} (re-rounded references {ref_s}, bars {bars})")
    print(msg)
    assert worst_y <= REL, msg
    assert worst_s[0] <= bars[0] and worst_s[1] <= bars[1], msg


@pytest.mark.parametrize("k", [1, 32, 33])
@pytest.mark.parametrize("B", [7, 129])
def test_one_launch_equals_split_launches(dev, leg, B, k):
    """(b) The 34-step solve in one launch == the launches t[:k+1] then t[k:] (from the first one's
    last row, the module carrying the hysteresis state across), bitwise, final states included: the
    same kernel and op order, the state round-tripped through memory as the fp32 it is.  k = 32 is
    the edge of the staged schedule chunk."""
    import fet_ode_amd as F
    from oracle import torch_ref as O
    t = _bench_t()
    y0 = O.lv_y0(B, 0).to(dev)
    key = ("one-launch", leg, B)
    if key not in _CACHE:
        m = _bench_model(dev)
        with torch.no_grad():
            one = F.odeint(F.autonomous(m), y0, t, method="rk4").cpu()
        _CACHE[key] = (one, [l.ferro._prev.cpu() for l in m.layers])
    one, one_states = _CACHE[key]
    m = _bench_model(dev)
    with torch.no_grad():
        a = F.odeint(F.autonomous(m), y0, t[:k + 1], method="rk4")
        b = F.odeint(F.autonomous(m), a[-1].clone(), t[k:], method="rk4")
    assert torch.equal(a[-1], b[0])
    split = torch.cat([a, b[1:]]).cpu()
    assert split.shape == one.shape
    assert torch.equal(split, one), (leg, B, k, slice_rel_err(split, one))
    for li, (layer, s) in enumerate(zip(m.layers, one_states)):
        assert torch.equal(layer.ferro._prev.cpu(), s), (leg, B, k, li)


# ---------------------------------------------------------------------------------------------
# (c) schedule edges on the stateless KAN field
# ---------------------------------------------------------------------------------------------
def _lin64(a, b, n):
    return torch.tensor(np.linspace(a, b, n))


# name -> (t, options): steps / outputs per step in the comments
SCHEDULES = {
    "32-steps": (lambda: _lin64(0, 3.5, 33), None),
    "33-steps": (lambda: _lin64(0, 3.5, 34), None),
    "64-steps": (lambda: _lin64(0, 3.5, 65), None),
    "65-steps": (lambda: _lin64(0, 3.5, 66), None),
    # 56 steps, the first output in step 38: three on-grid outputs, three interpolated, two in one step
    "56-steps-late-outputs": (lambda: torch.tensor([0, 2.40625, 2.4375, 2.45, 3.0, 3.49, 3.5], dtype=torch.float64),
                              {"step_size": 0.0625}),
    # 7 steps of 40 outputs: the multi-output loop reloads its chunk inside a step
    "40-outputs-per-step": (lambda: _lin64(0, 3.5, 281), {"step_size": 0.5}),
    "40-outputs-per-step-fp32-t": (lambda: torch.linspace(0, 3.5, 281), {"step_size": 0.5}),
    "reversed-35-steps": (lambda: _lin64(1, 0, 36), None),
    "reversed-50-outputs-per-step": (lambda: _lin64(1, 0, 101), {"step_size": 0.5}),
}
GENERIC_SCHEDULES = ["33-steps", "56-steps-late-outputs", "40-outputs-per-step", "reversed-35-steps"]


def _kan_problem(which):
    """(state dict, widths, y0): the golden traj_kan model with y0_B64, or the fieldn_kernel shape
    KAN [2, 16, 2] with seed-0 weights and lv_y0(64, 0)."""
    key = ("kan", which)
    if key not in _CACHE:
        if which == "golden":
            g = load_golden("traj_kan")
            _CACHE[key] = (golden_sd(g), [2, 10, 2], torch.from_numpy(g["y0_B64"]))
        else:
            import fet_ode_amd as F
            from oracle import torch_ref as O
            torch.manual_seed(0)
            sd = {k: v.clone() for k, v in F.KAN([2, 16, 2], grid_size=5).state_dict().items()}
            _CACHE[key] = (sd, [2, 16, 2], O.lv_y0(64, 0))
    return _CACHE[key]


def _kan_oracle(which, sched, method):
    key = ("kan-oracle", which, sched, method)
    if key not in _CACHE:
        from oracle import torch_ref as O
        sd, _, y0 = _kan_problem(which)
        ref = O.KANRef([O.KANLinearParams.from_state_dict(sd, f"layers.{l}.") for l in range(2)])
        mk, opts = SCHEDULES[sched]
        with torch.no_grad():
            _CACHE[key] = O.odeint(lambda tt, yy: ref(yy), y0, mk(), method=method, options=opts)
    return _CACHE[key]


def _check_schedule(dev, which, sched, method):
    import fet_ode_amd as F
    sd, widths, y0 = _kan_problem(which)
    exp = _kan_oracle(which, sched, method)
    m = F.KAN(widths, grid_size=5)
    m.load_state_dict(sd)
    m = m.to(dev)
    mk, opts = SCHEDULES[sched]
    with torch.no_grad():
        sol = F.odeint(F.autonomous(m), y0.to(dev), mk(), method=method, options=opts).cpu()
    assert sol.shape == exp.shape
    assert torch.isfinite(sol).all()
    assert torch.equal(sol[0], y0)
    err = slice_rel_err(sol, exp)
    print(f"{which} {sched} {method}: {err:.3e}")
    assert err <= REL, (which, sched, method, err)


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_schedule_edges_rk4(dev, leg, sched):
    """(c) rk4 under every forced kernel: 32 / 33 / 64 / 65 steps (the staged chunk and its
    neighbours), a first output 38 steps in, 40 and 50 outputs inside one step, interpolated
    outputs, fp32 time and reversed time, each whole trajectory within 1e-5 per slice of the oracle
    (fp32 vs fp64 oracle <= 1.9e-7 on every case)."""
    _check_schedule(dev, "golden", sched, "rk4")


@pytest.mark.parametrize("sched", GENERIC_SCHEDULES)
@pytest.mark.parametrize("method", ["rk4_classic", "midpoint", "euler"])
@pytest.mark.parametrize("leg", ["v6", "two-per-wave"], indirect=True)
def test_schedule_edges_generic_methods(dev, leg, method, sched):
    """(c) the generic (non-rk4-specialised) v6 and two-per-wave kernels carry their own schedule
    loop: the other fixed-grid methods on the same edges."""
    _check_schedule(dev, "golden", sched, method)


@pytest.mark.parametrize("sched", GENERIC_SCHEDULES)
@pytest.mark.parametrize("method", ["rk4", "rk4_classic", "midpoint", "euler"])
def test_schedule_edges_fieldn(dev, method, sched):
    """(c) fieldn_kernel (the single-launch integrator of the other field widths) at KAN [2, 16, 2]."""
    _check_schedule(dev, "fieldn", sched, method)
