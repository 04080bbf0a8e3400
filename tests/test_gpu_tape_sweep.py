"""The fixed-grid training path cut where it is well conditioned ("Anchored at the tape"):

  * the TAPE the three taped forward kernels record (v6, one and two trajectories per wave; the
    fieldn kernel for other widths) against the fp64 oracle's stage inputs, teacher-forced step by
    step, under the state bar of test_gpu_dispatch.test_one_step_parity_at_every_step;
  * every reverse SWEEP (the one-kernel sweep at two and at one trajectory per wave, the lane-group
    sweep with its sums inside and with kansum_kernel, fieldn_adj_kernel, the stateless KAN sweep)
    against the fp64 replay of the oracle solve anchored at the launch's OWN tape
    (oracle/tape_ref.py): given the tape the sweep is linear in the cotangent and both sides share
    its inputs exactly, so the bar is per tensor

        |gpu - fp64 replay| <= min(4 Y + 1e-5 scale, 1e-4 scale),   scale = max |fp64 replay|,

    Y = the worst distance from the fp64 replay of the fp32 replay, of three 6e-8 re-roundings of its
    parameters, and of the fp32 replay with the kernels' rounded logistic derivative (the one named
    approximation the first run of these tests made necessary; evidence in DESIGN.md §4.1), on the
    same tape.  tests/test_tape_ref.py shows on the CPU that the reference alone stays inside this
    bar and that a 1e-3 error of one constant leaves it by 7x or more.

Cotangents are N(0, 1) on every trajectory and every output row (row 0, the pass-through, included).
The tape and the saved initial state are read from the autograd node of the solution.  The CPU
replays are cached by the tape's bytes: the four sweeps of a (batch, step) share one reference.
"""
import contextlib
import hashlib

import numpy as np
import pytest
import torch

from test_gpu_dispatch import _bench_model, _layer_rel
from test_gpu_parity import REL, _set_states, forced_dispatch_leg, slice_rel_err
from test_tape_ref import HORIZON_SEED, ONE_STEP_SEED, WIDTHS, bench_sd, bench_t, cotangent, horizon_y0, teacher

pytestmark = pytest.mark.gpu

_CACHE = {}

# name -> (fetode_backward_set_v7, fetode_backward_set_tpw)
SWEEPS = {"fn": (0, 2), "fn1": (0, 1), "sweep7": (2, 0), "sweep7-kansum": (6, 0)}


@contextlib.contextmanager
def forced_sweep(name):
    from fet_ode_amd import _lib
    lib = _lib.load()
    v7, tpw = SWEEPS[name]
    prev_v7, prev_tpw = lib.fetode_backward_set_v7(v7), lib.fetode_backward_set_tpw(tpw)
    try:
        yield name
    finally:
        lib.fetode_backward_set_v7(prev_v7)
        lib.fetode_backward_set_tpw(prev_tpw)


@pytest.fixture(params=list(SWEEPS))
def sweep(request):
    with forced_sweep(request.param) as name:
        yield name


# ---------------------------------------------------------------------------------------------
# one training solve on the GPU: the solution, its tape and initial state, and the sweep's gradients
# ---------------------------------------------------------------------------------------------

def _train_solve(m, y0, t, method, options, dev):
    import fet_ode_amd as F
    y0g = y0.clone().to(dev).requires_grad_(True)
    sol = F.odeint(F.autonomous(m), y0g, t, method=method, options=options)
    node = sol.grad_fn
    assert type(node).__name__ == "_FusedFixedFnBackward", type(node)   # the fused training path
    tape, state0 = node.saved_tensors
    return y0g, sol, tape.detach().cpu(), None if state0 is None else state0.detach().cpu(), node.mask


def _sweep_grads(m, y0g, sol, w):
    names, params = zip(*m.named_parameters())
    g = torch.autograd.grad(sol, (y0g,) + params, grad_outputs=w.to(sol.device, torch.float32))
    return dict(zip(("y0",) + names, (x.cpu() for x in g)))


def _oracle_state0(state0, mask, B, widths):
    """The solve's initial hysteresis state for oracle.tape_ref.set_state: per layer the compact
    prev_x block of the saved buffer, or None where the init-mask bit says it is re-initialised."""
    if state0 is None and mask == 0:
        return "fresh"   # a stateless field
    out, off = [], 0
    for l, w in enumerate(widths[:-1]):
        out.append(None if (mask >> l) & 1 else state0[B * off:B * (off + w)].view(B, w).clone())
        off += w
    return out


def _envelope(sd, widths, y0, t, method, options, state0, tape, w, **kw):
    """The CPU replays of one (problem, tape, cotangent), cached by their bytes."""
    from oracle import tape_ref as R
    h = hashlib.sha1()
    for x in (y0, t, w, *tape, *[s for s in (state0 if isinstance(state0, list) else []) if s is not None]):
        h.update(x.contiguous().numpy().tobytes())
    key = ("env", tuple(widths), method, repr(options), repr(sorted(kw.items())), h.hexdigest(),
           "fresh" if isinstance(state0, str) else tuple(s is None for s in state0))
    if key not in _CACHE:
        _CACHE[key] = R.Envelope(sd, widths, y0, t, method, options, state0, tape, w, **kw)
    return _CACHE[key]


class _Worst:
    """The one line every test prints: the worst err / scale and Y / scale with tensor and step."""

    def __init__(self):
        self.err, self.Y, self.margin = (0.0, None, None), (0.0, None, None), (0.0, None, None)
        self.over, self.cap, self.rows = [], [], []

    def add(self, r, where):
        self.err = max(self.err, (*r["err"], where), key=lambda v: v[0])
        self.Y = max(self.Y, (*r["Y"], where), key=lambda v: v[0])
        self.margin = max(self.margin, (*r["margin"], where), key=lambda v: v[0])
        self.over += [(where, *o) for o in r["over"]]
        self.cap += [(where, *c) for c in r["cap"]]
        self.rows += [(where, k, *v) for k, v in r["rows"].items()]

    def line(self, tag):
        s = (f"{tag}: worst err/scale {self.err[0]:.2e} ({self.err[1]}, {self.err[2]}); worst Y/scale "
             f"{self.Y[0]:.2e} ({self.Y[1]}, {self.Y[2]}); worst err/bar {self.margin[0]:.2f} ({self.margin[1]}, "
             f"{self.margin[2]})")
        if self.cap:
            s += f"; bar capped at 1e-4 for {self.cap}"
        for where, k, well, n, rest in self.rows:
            s += f"; {where} {k}: {well} of {n} rows well chosen, the others reach {rest:.2e} of their own scale"
        return s


def _check(tag, worst):
    msg = worst.line(tag)
    print(msg)
    assert not worst.over, (msg, worst.over)


def _sweep_case(dev, m, sd, widths, y0, t, method, options, w, parse, worst, where, **kw):
    """One training solve under the default taped kernel, the forced sweep's gradients, and their
    report against the replay anchored at that solve's tape.  Returns the solution."""
    B = y0.shape[0]
    y0g, sol, tape, state0, mask = _train_solve(m, y0, t, method, options, dev)
    got = _sweep_grads(m, y0g, sol, w)
    env = _envelope(sd, widths, y0, t, method, options, _oracle_state0(state0, mask, B, widths), parse(tape), w, **kw)
    assert set(got) == set(env.g64), set(got) ^ set(env.g64)
    worst.add(env.report(got), where)
    return sol.detach()


def _rows(tape):
    from oracle import tape_ref as R
    return R.parse_tape_rows(tape, WIDTHS[0], WIDTHS[1])


# ---------------------------------------------------------------------------------------------
# (a) the tape
# ---------------------------------------------------------------------------------------------

def _tape_reference(B, method, steps):
    """Per step j of `steps`, teacher-forced from the oracle's (y_j, state_j): the fp64 oracle's tape
    of one `method` step, the fp32 oracle's y_{j+1}; and, over the steps, the worst distance of three
    6e-8 re-roundings of the fp32 oracle from that tape (per layer and evaluation, normwise)."""
    key = ("tape-ref", B, method, tuple(steps))
    if key not in _CACHE:
        from oracle import parity as P
        from oracle import tape_ref as R
        sd, t, recs = bench_sd(), bench_t(), teacher(B)[1]
        ref, ref_worst = {}, [0.0, 0.0]
        sds = list(P.perturbed_state_dicts(sd, 3, seed=4242))
        for j in steps:
            y, prevs = recs[j]
            _, t64, _ = R.record_tape(sd, WIDTHS, y, t[j:j + 2], method, state0=prevs, dtype=torch.float64)
            y1 = R.record_tape(sd, WIDTHS, y, t[j:j + 2], method, state0=prevs)[0][1:]
            ref[j] = (t64, y1)
            for sdp in sds:
                _, tp, _ = R.record_tape(sdp, WIDTHS, y, t[j:j + 2], method, state0=prevs)
                for l in range(2):
                    ref_worst[l] = max(ref_worst[l], max(_layer_rel(a, b) for a, b in zip(tp[l], t64[l])))
        _CACHE[key] = (ref, ref_worst)
    return _CACHE[key]


def _tape_pin(dev, leg, B, method, steps):
    t, recs = bench_t(), teacher(B)[1]
    ref, ref_worst = _tape_reference(B, method, steps)
    m = _bench_model(dev)
    n_ev = {"rk4": 4, "rk4_classic": 4, "midpoint": 2, "euler": 1}[method]
    worst_y, worst = (0.0, None), [(0.0, None), (0.0, None)]
    for j in steps:
        y, prevs = recs[j]
        _set_states(m, prevs, dev)
        _, sol, tape, _, mask = _train_solve(m, y, t[j:j + 2], method, None, dev)
        # (step 0's record is the fresh module's state, batch 1: re-initialised at B > 1)
        assert mask == (0 if prevs[0].shape[0] == B else 3) and tape.shape == (n_ev, B, 12), (j, mask, tape.shape)
        t64, y1 = ref[j]
        worst_y = max(worst_y, (slice_rel_err(sol.detach().cpu()[1:], y1), j), key=lambda v: v[0])
        for l, got in enumerate(_rows(tape)):
            e = max(_layer_rel(a, b) for a, b in zip(got, t64[l]))
            worst[l] = max(worst[l], (e, j), key=lambda v: v[0])
    bars = [max(1e-5, 4 * r) for r in ref_worst]
    msg = (f"{leg} B={B} {method}: tape (err, step) per layer {worst} (re-rounded references {ref_worst}, bars "
           f"{bars}); y {worst_y} (bar {REL})")
    print(msg)
    assert worst_y[0] <= REL, msg
    assert worst[0][0] <= bars[0] and worst[1][0] <= bars[1], msg


@pytest.mark.parametrize("B", [7, 129])
@pytest.mark.parametrize("leg", ["v6", "tpw1", "two-per-wave"])
def test_tape_pin_rk4_every_step(dev, leg, B):
    """(a) Each taped rk4 kernel, from the oracle's (y_j, state_j) at every step of the horizon: the
    four tape rows (x_e, h_e) against the fp64 oracle's stage inputs of the same step, per layer and
    evaluation normwise within max(1e-5, 4 x the worst of three re-rounded fp32 references driven the
    same way), and the taped launch's y_{j+1} within 1e-5 per slice of the fp32 oracle's (the taped
    instantiations are code objects of their own).  Measured on MI355X, B = 7 / 129, worst of the three
    kernels: layer 0 3.4e-6 / 2.9e-6 (re-rounded references 4.7e-6 / 3.3e-6), the hidden h 4.1e-5 /
    1.5e-5 (references 2.4e-5 / 1.3e-5, bars 9.8e-5 / 5.1e-5), y 2.7e-6 / 1.5e-6."""
    with forced_dispatch_leg(leg):
        _tape_pin(dev, leg, B, "rk4", range(34))


@pytest.mark.parametrize("B", [7, 129])
@pytest.mark.parametrize("method", ["rk4_classic", "midpoint", "euler"])
@pytest.mark.parametrize("leg", ["v6", "two-per-wave"])
def test_tape_pin_generic_methods(dev, leg, method, B):
    """(a) The generic taped kernels (small_tape / fn_tape) under the other fixed-grid methods, at the
    first, a middle and the last step; bars as above.  Measured: tape <= 4.0e-7 (references <= 9.8e-7,
    so both bars are the 1e-5 floor), y <= 4.3e-7."""
    with forced_dispatch_leg(leg):
        _tape_pin(dev, leg, B, method, (0, 17, 33))


# ---------------------------------------------------------------------------------------------
# (b) - (e) the four [2, 10, 2] KAN-FET sweeps
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [7, 129])
def test_one_step_sweep_pin(dev, sweep, B):
    """(b) At every step of the horizon, from the oracle's (y_j, state_j): the forced sweep's gradient
    of sum(w * out) against the replay anchored at that launch's tape.  B = 7: the last wave of the
    two-per-wave sweeps half empty, 4 partial rows, one of a workgroup's four waves busy in its second
    pair.  B = 129: 65 waves, 68 partial rows, so part_reduce_kernel runs with more rows than its 64
    chunks and a ragged last chunk.  Measured on MI355X (the four sweeps agree to three digits):
    B = 7 worst err / scale 1.6e-5 (layers.0.ferro.k, step 12), worst Y / scale 1.5e-5, worst err / bar
    0.47; B = 129 err 2.9e-5 and Y 2.9e-5 (both layers.0.kan.logistic_basis.a at step 32: the rounded
    logistic derivative), worst err / bar 0.52 (layers.0.ferro.k, step 19)."""
    sd, t, recs = bench_sd(), bench_t(), teacher(B)[1]
    ws = cotangent(ONE_STEP_SEED, 34, 2, B, 2)
    m = _bench_model(dev)
    worst = _Worst()
    for j, (y, prevs) in enumerate(recs):
        _set_states(m, prevs, dev)
        _sweep_case(dev, m, sd, WIDTHS, y, t[j:j + 2], "rk4", None, ws[j], _rows, worst, f"step {j}")
    _check(f"{sweep} B={B} one step", worst)


@pytest.mark.parametrize("B", [1, 7, 129])
def test_whole_horizon_sweep_pin(dev, sweep, B):
    """(c) One 34-step rk4 launch from a fresh module (evaluation 0 under both first-call rules:
    dx = x at B = 1, dx = 0 at B > 1), then a second solve of 11 steps from its last row and the
    carried state (init_mask 0, the saved state0; another whole horizon leaves the spline grid and the
    fp64 replay's own gradients overflow), the cotangent on every output row: the reverse step loop,
    the prefetch one step ahead and the ev < 0 tape reads.  Parameter tensors and y0 by max-norm; y0 per trajectory as well
    (|d loss / d y0| spans 1e0 ... 1e9 over the rows) on the rows whose own reference bar fits under
    the cap: on the others the fp32 replay itself leaves 1e-4 of the row (tests/test_tape_ref.py), so
    they are held by the max-norm bar only and their figure is printed; the well-chosen rows share one
    relative Y, the worst of theirs.  B = 129 starts from lv_y0(129, 4) (test_tape_ref.horizon_y0).
    Measured on MI355X, worst over the four sweeps: B = 1 err / scale 1.8e-5, Y 1.8e-5, err / bar 0.40;
    B = 7 2.6e-5, 2.6e-5, 0.59 (4 of 7 fresh rows well chosen, the others at 2.3e-5 of their scale);
    B = 129 6.9e-5 on a y0 row (Y 2.2e-5, err / bar 0.71), parameter tensors <= 0.6 of their bars; 89
    of 129 fresh and 122 of 129 carried rows well chosen, the others reach 1.0e-3 and 3.0e-5."""
    from oracle import torch_ref as O
    sd, t = bench_sd(), bench_t()
    m = _bench_model(dev)
    worst = _Worst()
    y0 = horizon_y0(B)
    for leg, tl in enumerate((t, t[:12])):
        w = cotangent(HORIZON_SEED + leg, len(tl), B, 2)
        sol = _sweep_case(dev, m, sd, WIDTHS, y0, tl, "rk4", None, w, _rows, worst, ("fresh", "carried")[leg],
                          rowwise=("y0",))
        y0 = sol[-1].cpu()
    _check(f"{sweep} B={B} whole horizon", worst)


# name -> (method, t, options)
SCHEDULES = {
    "rk4_classic": ("rk4_classic", lambda: bench_t()[:6], None),
    "midpoint": ("midpoint", lambda: bench_t()[:6], None),
    "euler": ("euler", lambda: bench_t()[:6], None),
    # steps of 0.1: three interpolated outputs (out_mode 2) and one on the grid
    "interpolated": ("rk4", lambda: torch.tensor([0, 0.13, 0.2, 0.37, 0.45], dtype=torch.float64), {"step_size": 0.1}),
    # steps of 0.25: two outputs inside the first step, one at its end, one inside the second
    "two-outputs-in-a-step": ("rk4", lambda: torch.tensor([0, 0.05, 0.1, 0.25, 0.4], dtype=torch.float64),
                              {"step_size": 0.25}),
    "reversed": ("rk4", lambda: torch.tensor(np.linspace(0.5, 0, 6)), None),
}


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_methods_and_schedules_sweep_pin(dev, sweep, sched):
    """(d) B = 7, a fresh module: the other fixed-grid methods over 6 points, interpolated outputs,
    two outputs inside one step, reversed time.  Measured on MI355X, worst over the four sweeps, err /
    scale (Y / scale): rk4_classic 3.3e-6 (1.2e-5), midpoint 4.5e-6 (1.3e-5), euler 4.8e-6 (6.4e-6),
    interpolated 6.5e-6 (8.7e-6), two outputs in a step 2.2e-5 (1.6e-5; err / bar 0.49), reversed
    2.3e-6 (1.0e-6)."""
    from oracle import torch_ref as O
    method, mk, options = SCHEDULES[sched]
    t = mk()
    worst = _Worst()
    w = cotangent(31, len(t), 7, 2)
    _sweep_case(dev, _bench_model(dev), bench_sd(), WIDTHS, O.lv_y0(7, 0), t, method, options, w, _rows, worst, sched)
    _check(f"{sweep} {sched}", worst)


@pytest.mark.parametrize("sweep", ["fn", "sweep7"], indirect=True)
def test_grid_stride_sweep_pin(dev, sweep):
    """(e) B = 16391, one rk4 step from a fresh module: more than 2 x 8192 waves' worth, so the second
    pass of the sweeps' b0 += gridDim.x * kTPB * 2 loop runs and ends in a half-empty wave, and
    part_reduce_kernel sees 8192 rows.  Y here is the single fp32 replay, without re-roundings, to
    keep the one large CPU reference (shared by both kernels) at a few seconds: a narrower bar than
    the other legs', never a wider one (the rounded-derivative replay is part of it as everywhere).
    Measured on MI355X: err / scale 7.5e-7 (fn), 7.1e-7 (sweep7), Y / scale 7.8e-6, err / bar 0.06."""
    from oracle import torch_ref as O
    B = 16391
    worst = _Worst()
    w = cotangent(41, 2, B, 2)
    _sweep_case(dev, _bench_model(dev), bench_sd(), WIDTHS, O.lv_y0(B, 0), bench_t()[:2], "rk4", None, w, _rows,
                worst, "one step", n_rerounded=0)
    _check(f"{sweep} B={B} grid stride", worst)


# ---------------------------------------------------------------------------------------------
# (f) other widths: the fieldn taped forward and fieldn_adj_kernel; (g) the stateless KAN sweep
# ---------------------------------------------------------------------------------------------

def _seeded(kind, widths, **kw):
    key = ("model", kind, tuple(widths))
    if key not in _CACHE:
        import fet_ode_amd as F
        torch.manual_seed(0)
        m = getattr(F, kind)(widths, grid_size=5, **kw)
        _CACHE[key] = {k: v.clone() for k, v in m.state_dict().items()}
    import fet_ode_amd as F
    m = getattr(F, kind)(widths, grid_size=5, **kw)
    m.load_state_dict(_CACHE[key])
    return _CACHE[key], m


@pytest.mark.parametrize("B", [5, 48])
@pytest.mark.parametrize("method", ["rk4", "midpoint"])
def test_fieldn_sweep_pin(dev, method, B):
    """(f) KAN-FET [3, 8, 3], K = 6 (no specialised kernel: the fieldn taped forward, two-plane tape,
    and fieldn_adj_kernel with the per-module parameter VJPs), a fresh module, 6 points.  Measured on
    MI355X, err / scale (Y / scale): rk4 4.1e-6 (3.4e-6) at B = 5, 1.6e-6 (1.0e-6) at B = 48; midpoint
    2.3e-6 (3.4e-6), 1.8e-6 (2.4e-6); err / bar <= 0.17."""
    from oracle import tape_ref as R
    widths = [3, 8, 3]
    sd, m = _seeded("KANFET", widths, num_fet_basis=6)
    g = torch.Generator().manual_seed(3)
    y0 = 0.5 + 1.5 * torch.rand(B, 3, generator=g)
    t = bench_t()[:6]
    n_ev = 5 * {"rk4": 4, "midpoint": 2}[method]
    worst = _Worst()
    _sweep_case(dev, m.to(dev), sd, widths, y0, t, method, None, cotangent(51, 6, B, 3),
                lambda tape: R.parse_tape_planes(tape, n_ev, B, 3, 8), worst, method)
    _check(f"fieldn {method} B={B}", worst)


def test_stateless_kan_sweep_pin(dev):
    """(g) KAN [2, 10, 2] (fixed_bwd_kernel<..., false, true, 1>), whole horizon, B = 7: the anchored
    replay with KANRef.  Measured on MI355X: err / scale 1.1e-6, Y / scale 9.3e-7, err / bar 0.08,
    all 7 y0 rows well chosen."""
    from oracle import torch_ref as O
    sd, m = _seeded("KAN", WIDTHS)
    worst = _Worst()
    _sweep_case(dev, m.to(dev), sd, WIDTHS, O.lv_y0(7, 0), bench_t(), "rk4", None, cotangent(61, 35, 7, 2), _rows,
                worst, "whole horizon", rowwise=("y0",))
    _check("KAN whole horizon B=7", worst)
