"""The ECG NODE-RNN encoder under dopri5 in one launch with a step controller per sample
(fetode_driven_dopri5) — against tests/node_rnn_ref.py's field under the oracle's dopri5, one sample
per solve (tests/driven_dopri5_ref.py).

The error ratio of this field differs by about 1e-4 relative between an fp32 and an fp64 run, so a
free-running comparison can flip an accept.  Two kinds of checks handle that:
  flip-proof    the GPU runs with first_step = 0.05 (no probe); the fp64 oracle and four fp32 controls
                replay each sample's OWN GPU attempt log (t0, dt, accepted), and the trajectory, the end
                state and every attempt's error ratio meet the bars of tests/test_gpu_driven.py: 1e-5
                per slice where the fp32 oracle is within 1e-6 of fp64, else
                |gpu - fp64| <= 4 worst fp32 control + 1e-5 scale
  free-running  only on inputs the oracle itself decides (fp32 and fp64 runs agree on every accept and
                no ratio lies in [0.95, 1.05] — asserted first, no sample skipped), with the bars of
                test_dopri5_kanfet_trace_resident: the same accept sequence, nfev = 2 + 6 attempts,
                first_step and every dt within 1e-3, ratios within 1e-2, the solution within 1e-4 per
                slice against the fp32 oracle; and against the host-driven loop of the same encoder the
                same accept sequence and 1e-5 per slice.
Then structure: rows are independent (bitwise), the logged evaluation times and x(t) are the host
expressions (bitwise), the entry points take the path they should, and failures are status words."""
from contextlib import contextmanager

import pytest
import torch

import driven_dopri5_ref as DR
import test_gpu_driven as TD

pytestmark = pytest.mark.gpu
FS = 0.05

# (H, D, K, T, B), rtol, atol — with first_step 0.05 on the fp32 CPU oracle (attempts, rejects) per
# sample: (16, 6) (8, 2) (12, 3) | (9, 2) (9, 2) (6, 0) | (9, 2) (8, 2) | 4-5 attempts over 23 intervals, no reject |
# (9-12, 1-4) | (4, 0) (6, 2) inside the single interval | the family's lower edge | K = 10
REPLAY = [((8, 1, 3, 9, 3), 1e-3, 1e-4), ((5, 2, 4, 6, 3), 1e-3, 1e-4), ((64, 4, 16, 5, 2), 1e-3, 1e-4),
          ((64, 1, 12, 24, 4), 1e-2, 1e-3), ((64, 1, 12, 24, 4), 1e-3, 1e-4), ((3, 1, 2, 2, 2), 1e-2, 1e-3),
          ((1, 1, 1, 3, 2), 1e-3, 1e-4), ((8, 1, 10, 4, 2), 1e-3, 1e-4)]
NO_REJECTS = (REPLAY[3], REPLAY[6])   # the cases that are not there for their rejected attempts
# on DR.free_series, decided on the CPU oracle: 0-1 rejects, closest ratio 0.63 from 1 | 0-2 rejects,
# closest 0.13 | 2-4 rejects, closest 0.11
FREE = [((8, 1, 3, 9, 3), 1e-2, 1e-3), ((8, 1, 3, 9, 3), 1e-3, 1e-4), ((64, 4, 16, 5, 2), 1e-3, 1e-4)]


def ids(c):
    return "H%d-D%d-K%d-T%d-B%d-rtol%g" % (*c[0], c[1])


@contextmanager
def knob(on):
    from fet_ode_amd import ecg
    prev = ecg.set_resident_driven_dopri5(on)
    try:
        yield
    finally:
        ecg.set_resident_driven_dopri5(prev)


def gpu_solve(case, rtol, atol, options, dev, rows=None, evlog=False, x=None):
    """ecg.driven_dopri5_solve of the case's samples `rows` (of x, by default the case's series) from the
    reset state: the solution (T, B, H), the record, the end state (B, H + D) and the evaluation log."""
    from fet_ode_amd import ecg
    H, D, K, T, B = case
    x = DR.series(*case) if x is None else x
    x = x if rows is None else x[rows]
    f = TD.gpu_field(H, D, K, dev)
    t_grid = DR.grid(T)
    f.set_interpolator(ecg.LinearInterp1D(t_grid.to(dev), x.to(dev)))
    f.basis.reset_state()
    ev = torch.full((x.shape[0], 160, 1 + D), float("nan"), device=dev) if evlog else None
    with torch.no_grad():
        out = ecg.driven_dopri5_solve(f, TD.lift(H, D, K, x).to(dev), t_grid, False, rtol, atol, options, reset=True,
                                      evlog=ev)
    assert out is not None
    return out[0], out[1], f.basis._prev, ev


def encoder(case, rtol, atol, dev):
    from fet_ode_amd import ecg
    H, D, K = case[:3]
    sd = DR.case_sd(H, D, K)
    e = ecg.OneODEEncoder(D, H, K, solver="dopri5", rtol=rtol, atol=atol)
    e.load_state_dict({k[len("enc."):]: v for k, v in sd.items() if k.startswith("enc.")}, strict=False)
    return e.to(dev)


def check_traj(got, c32, e64, ctl, what):
    """TD.check_traj's rule on a (T, H) trajectory."""
    own = TD.rows_rel(c32, e64)
    rel = TD.rows_rel(got, c32)
    well = own < 1e-6
    worst = rel[well].max().item() if well.any() else 0.0
    print(f"{what}: {int(well.sum())}/{len(well)} well-conditioned slices, worst rel {worst:.3e}, "
          f"oracle fp32-fp64 worst {own.max().item():.3e}")
    assert worst <= 1e-5, (what, worst)
    if not well.all():
        ill = ~well
        TD.envelope(got[ill.to(got.device)], [c[ill] for c in ctl], e64[ill], what + " (ill-conditioned slices)")


def check_log(att, nfev, probe):
    """The attempt log's own consistency."""
    assert nfev == (2 if probe else 1) + 6 * len(att)
    for n, (t0, dt, ratio, acc) in enumerate(att):
        assert acc == (ratio <= 1.0), (n, ratio, acc)
        if n + 1 < len(att):
            assert att[n + 1][0] == (t0 + dt if acc else t0), (n, att[n], att[n + 1])
            exp = DR.host_optimal_step(dt, ratio)
            assert abs(att[n + 1][1] - exp) <= 1e-12 * abs(exp), (n, att[n + 1][1], exp)
    assert att[0][0] == 0.0 and att[-1][3] and att[-1][0] + att[-1][1] >= 1.0


# ---------------------------------------------------------------------------------------------
# 1. flip-proof: the oracle replays each sample's own GPU attempt log
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REPLAY, ids=ids)
def test_replay_parity(dev, case):
    shape, rtol, atol = case
    H, D, K, T, B = shape
    sd, x = DR.case_sd(H, D, K), DR.series(*shape)
    sol, rec, prev, _ = gpu_solve(shape, rtol, atol, {"first_step": FS}, dev)
    assert sol.shape == (T, B, H) and rec.status == [0] * B
    assert torch.equal(sol[0].cpu(), TD.lift(H, D, K, x))
    n_rej = 0
    for b in range(B):
        att = rec.attempts[b]
        assert len(att) == rec.n_attempts[b] and att[0][1] == FS
        check_log(att, rec.nfev[b], False)
        n_rej += sum(1 for a in att if not a[3])
        e64, ctl = DR.replay_set(sd, x[b], rtol, atol, att, FS)
        what = f"{ids(case)} sample {b} ({len(att)} attempts, {sum(1 for a in att if not a[3])} rejects)"
        check_traj(sol[:, b], ctl[0].traj, e64.traj, [c.traj for c in ctl], what)
        if TD.rows_rel(ctl[0].end, e64.end).max().item() < 1e-6:
            r = TD.rows_rel(prev[b:b + 1], ctl[0].end).max().item()
            print(f"{what}: end state rel {r:.3e}")
            assert r <= 1e-5, (what, r)
        else:
            TD.envelope(prev[b:b + 1], [c.end for c in ctl], e64.end, what + " end state")
        TD.envelope(DR.ratios(att), [DR.ratios(c.trace.attempts) for c in ctl], DR.ratios(e64.trace.attempts),
                    what + " error ratios")
    assert n_rej >= 1 or case in NO_REJECTS, "the case is there for its rejected attempts"


# ---------------------------------------------------------------------------------------------
# 2. free-running on decided inputs: the initial step and the whole sequence
# ---------------------------------------------------------------------------------------------
def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("case", FREE, ids=ids)
def test_free_running_decided(dev, case):
    from fet_ode_amd import dopri5
    shape, rtol, atol = case
    H, D, K, T, B = shape
    pairs = DR.free_pair(shape, rtol, atol)
    for b, (r32, r64) in enumerate(pairs):   # a set-up error, not a kernel error, where this fails
        assert DR.decided(r32, r64), (b, r32.trace.attempts, r64.trace.attempts)
    x = DR.free_series(*shape).to(dev)
    enc = encoder(shape, rtol, atol, dev)
    with torch.no_grad():
        traj = enc(x)
    rec = enc.last_solve
    assert rec is not None and rec.status == [0] * B
    for b, (r32, _) in enumerate(pairs):
        att, exp = rec.attempts[b], r32.trace.attempts
        assert DR.accepts(att) == DR.accepts(exp), (b, att, exp)
        check_log(att, rec.nfev[b], True)
        assert rec.nfev[b] == r32.trace.nfev
        worst_dt = max(rel(a[1], e[1]) for a, e in zip(att, exp))
        worst_r = max(rel(a[2], e[2]) for a, e in zip(att, exp))
        worst_y = TD.rows_rel(traj[:, b], r32.traj).max().item()
        print(f"{ids(case)} sample {b}: {len(att)} attempts, first_step rel {rel(att[0][1], r32.trace.first_step):.3e}, "
              f"dt {worst_dt:.3e}, ratio {worst_r:.3e}, solution {worst_y:.3e}")
        assert rel(att[0][1], r32.trace.first_step) <= 1e-3 and worst_dt <= 1e-3
        assert worst_r <= 1e-2 and worst_y <= 1e-4
    # the host-driven loop of the same encoder, sample by sample
    with knob(False), torch.no_grad():
        for b in range(B):
            host = enc(x[b:b + 1])
            assert enc.last_solve is None and isinstance(dopri5.dopri5_solve.last, dopri5._Dopri5)
            assert DR.accepts(dopri5.dopri5_solve.last.attempts) == DR.accepts(rec.attempts[b]), b
            r = TD.rows_rel(traj[:, b], host[:, 0]).max().item()
            print(f"{ids(case)} sample {b}: against the host-driven loop {r:.3e}")
            assert r <= 1e-5, (b, r)


# ---------------------------------------------------------------------------------------------
# 3. rows are independent
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,options", [(FREE[1], {}), (REPLAY[4], {"first_step": FS})], ids=["probe", "first_step"])
def test_row_independence_bitwise(dev, case, options):
    shape, rtol, atol = case
    B = shape[4]
    sol, rec, prev, _ = gpu_solve(shape, rtol, atol, options, dev)
    assert len({tuple(DR.accepts(a)) for a in rec.attempts}) > 1   # the rows do take different step sequences
    for b in range(B):
        one, r1, p1, _ = gpu_solve(shape, rtol, atol, options, dev, rows=[b])
        assert torch.equal(one[:, 0], sol[:, b]) and torch.equal(p1[0], prev[b]), b
        assert (r1.nfev[0], r1.n_attempts[0], r1.status[0]) == (rec.nfev[b], rec.n_attempts[b], rec.status[b])
        assert r1.attempts[0] == rec.attempts[b], b
    perm = list(reversed(range(B)))
    ps, pr, pp, _ = gpu_solve(shape, rtol, atol, options, dev, rows=perm)
    for j, b in enumerate(perm):
        assert torch.equal(ps[:, j], sol[:, b]) and torch.equal(pp[j], prev[b]) and pr.attempts[j] == rec.attempts[b], b


def test_row_independence_more_samples_than_lanes(dev):
    """B = 67 ECG-shaped samples (more workgroups than a wave has lanes, an odd count): rows 0, 33 and 66
    are bitwise their own B = 1 solves."""
    shape, rtol, atol = (64, 1, 12, 24, 67), 1e-2, 1e-3
    sol, rec, prev, _ = gpu_solve(shape, rtol, atol, {}, dev)
    assert rec.status == [0] * 67 and torch.isfinite(sol).all()
    for b in (0, 33, 66):
        one, r1, p1, _ = gpu_solve(shape, rtol, atol, {}, dev, rows=[b])
        assert torch.equal(one[:, 0], sol[:, b]) and torch.equal(p1[0], prev[b]), b
        assert (r1.nfev[0], r1.attempts[0]) == (rec.nfev[b], rec.attempts[b]), b


# ---------------------------------------------------------------------------------------------
# 4. the evaluation times and the driving values
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,probe", [(REPLAY[1], False), (REPLAY[3], False), (FREE[1], True)],
                         ids=["D2", "ecg", "probe"])
def test_evaluation_times_and_driving_values(dev, case, probe):
    """Every logged x(t) is bitwise ecg.driven_table at the logged time, and the logged times are the
    host loop's fp32 expressions recomputed from the attempt log.  The probe's time fp32(t0 + h0)
    needs the trial step h0, which no log holds: it is held to the fp32 oracle's probe time within the
    1e-3 of the first-step bar (a decided case), every other time bitwise."""
    from fet_ode_amd import ecg
    shape, rtol, atol = case
    H, D, K, T, B = shape
    x = DR.free_series(*shape) if probe else DR.series(*shape)
    sol, rec, _, ev = gpu_solve(shape, rtol, atol, {} if probe else {"first_step": FS}, dev, evlog=True, x=x)
    tg = DR.grid(T).to(dev)
    for b in range(B):
        n = rec.nfev[b]
        assert n <= ev.shape[1] and torch.isnan(ev[b, n:]).all() and torch.isfinite(ev[b, :n]).all()
        times, vals = ev[b, :n, 0].contiguous(), ev[b, :n, 1:]
        exp = ecg.driven_table(tg, x[b:b + 1].to(dev).contiguous(), times)
        assert torch.equal(vals, exp[:, 0]), b
        host = DR.host_stage_times(rec.attempts[b], probe, 0.0, h0=0.0)
        if probe:
            t32 = DR.free_pair(shape, rtol, atol)[b][0].times[1].item()
            assert abs(times[1].item() - t32) <= 1e-3 * t32, (times[1].item(), t32)
            host[1] = times[1].item()
        assert torch.equal(times.cpu(), host), (b, times.cpu(), host)


# ---------------------------------------------------------------------------------------------
# 5. entry points
# ---------------------------------------------------------------------------------------------
def test_encoder_paths_and_state(dev):
    from fet_ode_amd import dopri5, ecg
    shape, rtol, atol = FREE[1]
    H, D, K, T, B = shape
    x = DR.series(*shape).to(dev)
    enc = encoder(shape, rtol, atol, dev)
    with torch.no_grad():
        traj = enc(x)
    assert isinstance(enc.last_solve, ecg.DrivenDopri5Solve) and traj.shape == (T, B, H)
    sol, rec, prev, _ = gpu_solve(shape, rtol, atol, {}, dev)
    assert torch.equal(traj, sol) and enc.last_solve.attempts == rec.attempts
    # afterwards the basis holds the last sample's last evaluation input, reference-shaped
    basis = enc.odefunc.basis
    assert torch.equal(basis._prev, prev[-1:]) and basis.prev_x.shape == (1, H + D, H, K)
    with torch.no_grad():
        assert torch.equal(enc(x, return_traj=False), sol[-1])
        one = enc(x[1:2])
    assert torch.equal(one[:, 0], sol[:, 1]) and enc.last_solve.n_attempts == [rec.n_attempts[1]]
    # under autograd and with the knob off: the per-sample host loop, as before
    out = enc(x[[0, 2]])
    assert enc.last_solve is None and out.requires_grad
    assert isinstance(dopri5.dopri5_solve.last, dopri5._Dopri5Grad)
    with knob(False), torch.no_grad():
        off = enc(x[[0, 2]])
        assert enc.last_solve is None and isinstance(dopri5.dopri5_solve.last, dopri5._Dopri5)
    assert not torch.equal(off, sol[:, [0, 2]])   # two different programs (guards a silent fall-back)
    assert TD.rows_rel(off, sol[:, [0, 2]]).max().item() <= 1e-5


def test_odeint_entry_one_row_only(dev):
    import fet_ode_amd as FA
    from fet_ode_amd import dopri5, ecg
    shape, rtol, atol = FREE[1]
    H, D, K, T, B = shape
    x = DR.series(*shape).to(dev)
    sol, rec, prev, _ = gpu_solve(shape, rtol, atol, {}, dev)
    t_grid = DR.grid(T).to(dev)
    h0 = TD.lift(H, D, K, x.cpu()).to(dev)
    f = TD.gpu_field(H, D, K, dev)
    with torch.no_grad():
        f.set_interpolator(ecg.LinearInterp1D(t_grid, x[1]))
        f.basis.reset_state()
        one = FA.odeint(f, h0[1:2], t_grid, method="dopri5", rtol=rtol, atol=atol)
        last = dopri5.dopri5_solve.last
        assert not isinstance(last, dopri5._Dopri5)
        assert torch.equal(one[:, 0], sol[:, 1]) and torch.equal(f.basis._prev, prev[1:2])
        assert (last.nfev, last.n_attempts, last.attempts) == (rec.nfev[1], rec.n_attempts[1], rec.attempts[1])
        # a second solve carries the stored (1, in) state over, as FerroelectricBasis's rules say
        again = FA.odeint(f, h0[1:2], t_grid, method="dopri5", rtol=rtol, atol=atol)
        assert not torch.equal(again, one) and torch.isfinite(again).all()
        with knob(False):
            FA.odeint(f, h0[1:2], t_grid, method="dopri5", rtol=rtol, atol=atol)
            assert isinstance(dopri5.dopri5_solve.last, dopri5._Dopri5)
        # more rows: odeint's error norm spans the batch — never this kernel
        f.set_interpolator(ecg.LinearInterp1D(t_grid, x))
        f.basis.reset_state()
        FA.odeint(f, h0, t_grid, method="dopri5", rtol=rtol, atol=atol)
        assert isinstance(dopri5.dopri5_solve.last, dopri5._Dopri5)


def test_node_rnn_reaches_the_kernel(dev):
    from fet_ode_amd import ecg
    shape, rtol, atol = FREE[1]
    H, D, K, T, B = shape
    m = ecg.NODE_RNN(input_size=D, hidden_size=H, num_classes=2, num_basis=K, solver="dopri5", rtol=rtol, atol=atol)
    m.load_state_dict(DR.case_sd(H, D, K))
    m = m.to(dev)
    x = DR.series(*shape).to(dev)
    with torch.no_grad():
        logits = m(x)
        assert isinstance(m.enc.last_solve, ecg.DrivenDopri5Solve) and m.enc.last_solve.status == [0] * B
        with knob(False):
            off = m(x)
            assert m.enc.last_solve is None
    r = TD.rows_rel(logits, off).max().item()
    print(f"NODE_RNN(dopri5) logits against the host-driven loop: {r:.3e}")
    assert not torch.equal(logits, off) and r <= 1e-5, r


# ---------------------------------------------------------------------------------------------
# 6. failures are status words
# ---------------------------------------------------------------------------------------------
def test_max_num_steps_names_the_sample(dev):
    """(3, 1, 2, 2, 2) at rtol 3e-2, first_step 2: on the CPU oracle sample 0 rejects the first attempt
    (ratio 1.65) and sample 1 accepts it (0.37) and is done; max_num_steps = 1 stops sample 0 only."""
    from fet_ode_amd import ecg
    shape, rtol, atol = (3, 1, 2, 2, 2), 3e-2, 3e-3
    opts = {"first_step": 2.0}
    free, rf, _, _ = gpu_solve(shape, rtol, atol, opts, dev)
    assert rf.status == [0, 0] and rf.n_attempts == [2, 1]
    sol, rec, prev, _ = gpu_solve(shape, rtol, atol, dict(opts, max_num_steps=1), dev)
    assert rec.status == [3, 0] and rec.n_attempts == [1, 1] and rec.nfev == [7, 7]
    with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(sample 0\)"):
        rec.raise_for_status()
    one, r1, p1, _ = gpu_solve(shape, rtol, atol, dict(opts, max_num_steps=1), dev, rows=[1])
    assert torch.equal(sol[:, 1], one[:, 0]) and torch.equal(sol[:, 1], free[:, 1]) and torch.equal(prev[1], p1[0])
    assert torch.equal(sol[0, 0], free[0, 0])   # the stopped sample wrote its first row only


def test_non_finite_series_names_the_sample(dev):
    shape, rtol, atol = FREE[1]
    x = DR.series(*shape).clone()
    enc = encoder(shape, rtol, atol, dev)
    with torch.no_grad():
        clean = enc(x.to(dev))
        x[1, 4, 0] = float("nan")
        with pytest.raises(AssertionError, match=r"non-finite values in state `y` \(sample 1\)"):
            enc(x.to(dev))
    rec = enc.last_solve
    assert rec.status[0] == 0 and rec.status[1] == 1 and rec.status[2] == 0
    assert torch.equal(rec.solution[:, 0], clean[:, 0]) and torch.equal(rec.solution[:, 2], clean[:, 2])
