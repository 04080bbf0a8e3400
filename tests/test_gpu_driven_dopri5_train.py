"""Training through the one-launch dopri5 solve of the ECG NODE-RNN encoder (fetode_driven_dopri5_tape /
_backward) — against tests/node_rnn_ref.py's field under the oracle's dopri5 with autograd,
one sample per solve (tests/driven_dopri5_grad_ref.py).

At production width most of this field's gradient runs through the step-size control, and no fp32
program reproduces that part better than 1e-3 .. 1e-2 (DESIGN §4.19 "Conditioning").  So the gradient
is checked in two parts, both by the envelope rule of tests/test_gpu_driven_dopri5.py
(|gpu - fp64| <= 4 worst fp32 control + 1e-5 scale per tensor; the controls are the fp32 oracle and
three re-roundings of its parameters, run like the GPU):
  frozen step   step_grad = False, first_step = 0.05; the oracles REPLAY each sample's own GPU attempt
                log under autograd, which makes every dt a constant: the same quantity, flip-proof
  full          step_grad = True, free-running, only on inputs the oracle itself decides and on which
                the controls agree with fp64 to 5e-2 per tensor (asserted first)
Then the tape against the untaped solve and the host expressions (bitwise), structure (rows are
independent, runs repeat bitwise, the entry points take the path they should), and one training step
of NODE_RNN(solver="dopri5") end to end."""
from contextlib import contextmanager
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import driven_dopri5_grad_ref as GR
import driven_dopri5_ref as DR
import node_rnn_ref as R
import test_gpu_driven as TD
import test_gpu_driven_dopri5 as TG

pytestmark = pytest.mark.gpu
FS = TG.FS
PAIRS = [(1e-2, 1e-3), (1e-3, 1e-4)]
TAPED = [(s, r, a) for s in [(8, 1, 3, 9, 3), (64, 4, 16, 5, 2)] for r, a in PAIRS]
ids = TG.ids


@contextmanager
def train_knob(on, step_grad=True):
    from fet_ode_amd import ecg
    prev = ecg.set_resident_driven_dopri5_training(on, step_grad)
    try:
        yield
    finally:
        ecg.set_resident_driven_dopri5_training(*prev)


def field_grads(f):
    g = {n: getattr(f.basis, n).grad for n in R.FERRO}
    g.update({"gain": f.gain.grad, "bias_out": f.bias.grad})
    return g


def gpu_train(shape, rtol, atol, options, dev, x, w, step_grad, backward=True):
    """ecg.driven_dopri5_train of the samples x (B, T, D) from the reset state with the encoder's lift
    in front, loss = sum(sol * w): the solution, the record, every gradient and the sweep's adj."""
    from fet_ode_amd import ecg
    H, D, K, T, _ = shape
    enc = TG.encoder(shape, rtol, atol, dev)
    f = enc.odefunc
    t_grid, xg = DR.grid(T).to(dev), x.to(dev)
    f.set_interpolator(ecg.LinearInterp1D(t_grid, xg))
    f.basis.reset_state()
    h0 = enc.lift(xg[:, 0])
    h0.retain_grad()
    with train_knob(True, step_grad):
        out = ecg.driven_dopri5_train(f, h0, t_grid.cpu(), False, rtol, atol, options, reset=True, t=t_grid)
        assert out is not None
        sol, rec = out
        if not backward:
            return SimpleNamespace(sol=sol, rec=rec)
        (sol * w.permute(1, 0, 2).to(dev, torch.float32)).sum().backward()
    g = field_grads(f)
    g.update({"h0": h0.grad, "lift.weight": enc.lift.weight.grad, "lift.bias": enc.lift.bias.grad})
    return SimpleNamespace(sol=sol.detach(), rec=rec, grads=g, adj=ecg._DrivenDopri5Fn.last_adj)


def check_envelope(got, e64, ctl, what, names=GR.NAMES):
    """Every tensor inside the envelope; returns the worst |gpu - fp64| / scale."""
    g64, gc = GR.batch_grads(e64), [GR.batch_grads(c) for c in ctl]
    worst = 0.0
    for n in names:
        TD.envelope(got[n], [c[n] for c in gc], g64[n], f"{what} d/d{n}")
        worst = max(worst, ((got[n].detach().double().cpu() - g64[n]).abs().max() / g64[n].abs().max()).item())
    return worst


# ---------------------------------------------------------------------------------------------
# 1. the taped forward
# ---------------------------------------------------------------------------------------------
def taped(shape, rtol, atol, dev, cap=None):
    from fet_ode_amd import ecg
    H, D, K, T, B = shape
    x = DR.series(*shape)
    f = TD.gpu_field(H, D, K, dev)
    t_grid = DR.grid(T).to(dev)
    xg = x.to(dev).contiguous()
    f.set_interpolator(ecg.LinearInterp1D(t_grid, xg))
    f.basis.reset_state()
    plan, d, _ = ecg._driven_plan(f, dev)
    with torch.no_grad():
        sol, rec, tape = ecg.driven_dopri5_taped_solve(f, plan, d, TD.lift(H, D, K, x).to(dev), xg, t_grid, rtol, atol,
                                                       {}, None, cap=cap)
    return sol, rec, tape, f.basis._prev


@pytest.mark.parametrize("case", TAPED, ids=ids)
def test_taped_forward_bitwise(dev, case):
    from fet_ode_amd import ecg
    shape, rtol, atol = case
    H, D, K, T, B = shape
    x = DR.series(*shape)
    ref, rref, pref, _ = TG.gpu_solve(shape, rtol, atol, {}, dev)
    sol, rec, tape, prev = taped(shape, rtol, atol, dev)
    assert torch.equal(sol, ref) and torch.equal(prev, pref)
    assert (rec.nfev, rec.n_attempts, rec.status) == (rref.nfev, rref.n_attempts, rref.status)
    assert rec.attempts == rref.attempts and rec.status == [0] * B
    tg = DR.grid(T)
    tgd = tg.to(dev)
    n_clamped = 0
    for b in range(B):
        n = rec.nfev[b]
        assert n == 2 + 6 * rec.n_attempts[b] <= tape.max_ev
        for v in (tape.hx, tape.phi, tape.t, tape.slope):
            assert not v[b, n:].any(), b                                  # rows at or beyond nfev are zero
        times = tape.t[b, :n].contiguous()
        host = DR.host_stage_times(rec.attempts[b], True, 0.0, h0=tape.init[b, 3].item())
        assert torch.equal(times.cpu(), host), (b, times.cpu(), host)
        xb = x[b:b + 1].to(dev).contiguous()
        assert torch.equal(tape.hx[b, :n, H:], ecg.driven_table(tgd, xb, times)[:, 0]), b
        assert torch.equal(tape.hx[b, 0, :H].cpu(), TD.lift(H, D, K, x)[b])
        # the slope of the interval LinearInterp1D used, the fp32 expression; 0 where the clamp cut the query
        tq = times.cpu()
        i = torch.searchsorted(tg, tq.clamp(tg[0], tg[-1])).clamp(1, T - 1)
        exp = (x[b][i] - x[b][i - 1]) / (tg[i] - tg[i - 1] + 1e-12).unsqueeze(1)
        cut = (tq < tg[0]) | (tq > tg[-1])
        exp[cut] = 0.0
        assert torch.equal(tape.slope[b, :n].cpu(), exp), b
        assert not tape.slope[b, :n][cut.to(dev)].any()
        n_clamped += int((tq > tg[-1]).sum())
        ini = tape.init[b].tolist()
        assert all(v > 0 for v in ini) and rec.attempts[b][0][1] == min(100 * ini[3], ini[4])
    assert n_clamped >= 1, "the case is there for its clamped stage times"
    # a cap of 2 attempts overflows: the solve runs again with room for all and gives the same bits
    assert max(rec.n_attempts) > 2
    sol2, rec2, tape2, prev2 = taped(shape, rtol, atol, dev, cap=2)
    m = max(rec.n_attempts)
    assert tape2.max_att == m and tape2.max_ev == 2 + 6 * m
    assert torch.equal(sol2, sol) and torch.equal(prev2, prev) and rec2.attempts == rec.attempts
    assert torch.equal(tape2.stats, tape.stats) and torch.equal(tape2.init, tape.init)
    for a, c in ((tape2.hx, tape.hx), (tape2.phi, tape.phi), (tape2.t, tape.t), (tape2.slope, tape.slope)):
        assert torch.equal(a, c[:, :tape2.max_ev])


# ---------------------------------------------------------------------------------------------
# 2. frozen step: the oracles replay each sample's own GPU attempt log under autograd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TG.REPLAY, ids=ids)
def test_frozen_step_gradient(dev, case):
    shape, rtol, atol = case
    H, D, K, T, B = shape
    sd, x, w = DR.case_sd(H, D, K), DR.series(*shape), GR.weights(shape)
    run = gpu_train(shape, rtol, atol, {"first_step": FS}, dev, x, w, step_grad=False)
    att = run.rec.attempts
    assert run.rec.status == [0] * B
    e64, ctl = GR.oracle_set(sd, x, rtol, atol, w, lambda b: DR.replay_options(att[b], FS))
    worst = check_envelope(run.grads, e64, ctl, f"frozen {ids(case)}")
    print(f"frozen {ids(case)}: worst |gpu - fp64| / scale over the tensors {worst:.3e}")
    n_rej = 0
    for b in range(B):
        n = run.rec.nfev[b]
        assert n == 1 + 6 * len(att[b]) and not run.adj[b, n:].any()
        assert run.adj[b, :n].any()
        for k, a in enumerate(att[b]):
            if not a[3]:
                n_rej += 1
                assert not run.adj[b, 1 + 6 * k:7 + 6 * k].any(), (b, k)      # exactly zero
    assert n_rej >= 1 or case in TG.NO_REJECTS, "the case is there for its rejected attempts"


# ---------------------------------------------------------------------------------------------
# 3. the full gradient, free-running on decided inputs
# ---------------------------------------------------------------------------------------------
def host_loop_grads(shape, rtol, atol, dev, x, w):
    """The knob-off path of the same encoder under autograd: _Dopri5Grad, sample by sample."""
    from fet_ode_amd import dopri5
    enc = TG.encoder(shape, rtol, atol, dev)
    loss = 0.0
    with train_knob(False):
        for b in range(x.shape[0]):
            traj = enc(x[b:b + 1].to(dev))
            assert enc.last_solve is None and isinstance(dopri5.dopri5_solve.last, dopri5._Dopri5Grad)
            loss = loss + (traj[:, 0] * w[b].to(dev, torch.float32)).sum()
        loss.backward()
    g = field_grads(enc.odefunc)
    g.update({"lift.weight": enc.lift.weight.grad, "lift.bias": enc.lift.bias.grad})
    return g


@pytest.mark.parametrize("case", TAPED, ids=ids)
def test_full_gradient_free_running(dev, case):
    shape, rtol, atol = case
    H, D, K, T, B = shape
    x, w = DR.free_series(*shape), GR.weights(shape)
    # preconditions, on the CPU oracle alone: a set-up error, not a kernel error, where these fail
    for b, (r32, r64) in enumerate(DR.free_pair(shape, rtol, atol)):
        assert DR.decided(r32, r64), (b, r32.trace.attempts, r64.trace.attempts)
    e64, ctl = GR.free_set(shape, rtol, atol)
    acc = [DR.accepts(r.trace.attempts) for r in e64]
    for c in ctl:
        assert [DR.accepts(r.trace.attempts) for r in c] == acc
    g64, gc = GR.batch_grads(e64), [GR.batch_grads(c) for c in ctl]
    for n in GR.NAMES:
        d = max(((c[n].double() - g64[n]).norm() / g64[n].norm()).item() for c in gc)
        print(f"full {ids(case)} d/d{n}: worst fp32 control stands {d:.3e} from fp64")
        assert d <= 5e-2, (n, d)
    run = gpu_train(shape, rtol, atol, {}, dev, x, w, step_grad=True)
    assert [DR.accepts(a) for a in run.rec.attempts] == acc
    worst = check_envelope(run.grads, e64, ctl, f"full {ids(case)}")
    print(f"full {ids(case)}: worst |gpu - fp64| / scale over the tensors {worst:.3e}")
    # the knob-off path of the same encoder stands inside the same envelope of the new one
    off = host_loop_grads(shape, rtol, atol, dev, x, w)
    for n in off:
        spread = max((c[n].double() - g64[n]).abs().max().item() for c in gc)
        err = (run.grads[n].double() - off[n].double()).abs().max().item()
        scale = g64[n].abs().max().item()
        print(f"full {ids(case)} d/d{n}: |gpu - host loop| = {err:.3e}, worst fp32 control {spread:.3e}, scale {scale:.3e}")
        assert err <= 4.0 * spread + 1e-5 * scale, (n, err, spread, scale)


def test_free_cases_have_rejects_and_a_clamped_last_step():
    """What the free-running cases are there for, on the fp64 oracle: rejected attempts in at least one,
    a last accepted step that overshoots t[-1] (its later stage times are clamped) in at least one."""
    rej = clamped = 0
    for shape, rtol, atol in TAPED:
        for r in GR.free_set(shape, rtol, atol)[0]:
            att = r.trace.attempts
            rej += sum(1 for a in att if not a[3])
            clamped += int(att[-1][0] + att[-1][1] > 1.0)
    assert rej >= 1 and clamped >= 1, (rej, clamped)


# ---------------------------------------------------------------------------------------------
# 4. structure
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,options", [(TAPED[1], {}), (TG.REPLAY[4], {"first_step": FS})], ids=["probe", "first_step"])
def test_rows_independent_bitwise(dev, case, options):
    shape, rtol, atol = case
    B = shape[4]
    x, w = DR.series(*shape), GR.weights(shape)
    full = gpu_train(shape, rtol, atol, options, dev, x, w, True)
    for b in range(B):
        one = gpu_train(shape, rtol, atol, options, dev, x[b:b + 1], w[b:b + 1], True)
        assert torch.equal(one.adj[0], full.adj[b]) and torch.equal(one.grads["h0"][0], full.grads["h0"][b]), b
    perm = list(reversed(range(B)))
    p = gpu_train(shape, rtol, atol, options, dev, x[perm], w[perm], True)
    for j, b in enumerate(perm):
        assert torch.equal(p.adj[j], full.adj[b]) and torch.equal(p.grads["h0"][j], full.grads["h0"][b]), b


def test_rows_independent_more_samples_than_lanes(dev):
    shape, rtol, atol = (64, 1, 12, 24, 67), 1e-2, 1e-3
    x, w = DR.series(*shape), GR.weights(shape)
    full = gpu_train(shape, rtol, atol, {}, dev, x, w, True)
    assert all(torch.isfinite(v).all() for v in full.grads.values())
    for b in (0, 33, 66):
        one = gpu_train(shape, rtol, atol, {}, dev, x[b:b + 1], w[b:b + 1], True)
        assert torch.equal(one.adj[0], full.adj[b]) and torch.equal(one.grads["h0"][0], full.grads["h0"][b]), b


@pytest.mark.parametrize("step_grad", [True, False])
def test_training_step_repeats_bitwise(dev, step_grad):
    shape, rtol, atol = TG.REPLAY[3]
    x, w = DR.series(*shape), GR.weights(shape)
    a = gpu_train(shape, rtol, atol, {}, dev, x, w, step_grad)
    b = gpu_train(shape, rtol, atol, {}, dev, x, w, step_grad)
    assert torch.equal(a.sol, b.sol) and torch.equal(a.adj, b.adj)
    for n in a.grads:
        assert torch.equal(a.grads[n], b.grads[n]), n


def test_step_grad_changes_the_gradient(dev):
    """step_grad on and off are two different quantities (guards a knob that is read nowhere)."""
    shape, rtol, atol = TAPED[1]
    x, w = DR.free_series(*shape), GR.weights(shape)
    on = gpu_train(shape, rtol, atol, {}, dev, x, w, True)
    off = gpu_train(shape, rtol, atol, {}, dev, x, w, False)
    assert torch.equal(on.sol, off.sol) and not torch.equal(on.grads["k"], off.grads["k"])
    assert off.adj[:, 1].eq(0).all() and on.adj[:, 1].ne(0).any()   # the probe: only the step control reads it


def test_encoder_paths(dev):
    from fet_ode_amd import dopri5, ecg
    shape, rtol, atol = TAPED[1]
    H, D, K, T, B = shape
    x = DR.series(*shape).to(dev)
    enc = TG.encoder(shape, rtol, atol, dev)
    with torch.no_grad():
        ref = enc(x)
        prev = enc.odefunc.basis._prev.clone()
    for rows in ([0, 1, 2], [1]):                # any B >= 1 is one batched call
        dopri5.dopri5_solve.last = None
        with train_knob(True):
            out = enc(x[rows])
        assert out.requires_grad and isinstance(enc.last_solve, ecg.DrivenDopri5Solve)
        assert dopri5.dopri5_solve.last is None                      # no _Dopri5Grad was built
        assert torch.equal(out.detach(), ref[:, rows]) and enc.last_solve.status == [0] * len(rows)
    with train_knob(True):
        out = enc(x)
        assert torch.equal(enc.odefunc.basis._prev, prev) and prev.shape == (1, H + D)
        out.sum().backward()
    assert all(p.grad is not None for p in enc.parameters())
    # the knob off: what it does today
    out = enc(x[[0, 2]])
    assert enc.last_solve is None and out.requires_grad and isinstance(dopri5.dopri5_solve.last, dopri5._Dopri5Grad)
    # a driving series that requires grad: the old path, knob or not
    dopri5.dopri5_solve.last = None
    with train_knob(True):
        xr = x[:1].clone().requires_grad_(True)
        out = enc(xr)
    assert enc.last_solve is None and isinstance(dopri5.dopri5_solve.last, dopri5._Dopri5Grad)


def test_odeint_entry_one_row_only(dev):
    import fet_ode_amd as FA
    from fet_ode_amd import dopri5, ecg
    shape, rtol, atol = TAPED[1]
    H, D, K, T, B = shape
    x = DR.series(*shape).to(dev)
    sol, rec, _, _ = TG.gpu_solve(shape, rtol, atol, {}, dev)
    t_grid = DR.grid(T).to(dev)
    h0 = TD.lift(H, D, K, x.cpu()).to(dev)
    f = TD.gpu_field(H, D, K, dev)
    with train_knob(True):
        f.set_interpolator(ecg.LinearInterp1D(t_grid, x[1]))
        f.basis.reset_state()
        one = FA.odeint(f, h0[1:2], t_grid, method="dopri5", rtol=rtol, atol=atol)
        last = dopri5.dopri5_solve.last
        assert one.requires_grad and not isinstance(last, dopri5._Dopri5)
        assert torch.equal(one.detach()[:, 0], sol[:, 1]) and last.attempts == rec.attempts[1]
        one.sum().backward()
        assert f.gain.grad is not None and torch.isfinite(f.basis.k.grad).all()
        # more rows: odeint's error norm spans the batch — never this kernel
        f.set_interpolator(ecg.LinearInterp1D(t_grid, x))
        f.basis.reset_state()
        FA.odeint(f, h0, t_grid, method="dopri5", rtol=rtol, atol=atol)
        assert isinstance(dopri5.dopri5_solve.last, dopri5._Dopri5Grad)
    f.set_interpolator(ecg.LinearInterp1D(t_grid, x[1]))
    f.basis.reset_state()
    FA.odeint(f, h0[1:2], t_grid, method="dopri5", rtol=rtol, atol=atol)
    assert isinstance(dopri5.dopri5_solve.last, dopri5._Dopri5Grad)   # the knob off: as before


def test_failing_sample_raises_in_forward(dev):
    """tests/test_gpu_driven_dopri5.py's case: with max_num_steps = 1 sample 0 stops after its rejected
    first attempt; the taped forward raises torchdiffeq's assertion, naming it, and builds no graph."""
    from fet_ode_amd import ecg
    shape, rtol, atol = (3, 1, 2, 2, 2), 3e-2, 3e-3
    x, w = DR.series(*shape), GR.weights(shape)
    ecg._DrivenDopri5Fn.last_adj = None
    with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(sample 0\)"):
        gpu_train(shape, rtol, atol, {"first_step": 2.0, "max_num_steps": 1}, dev, x, w, True)
    assert ecg._DrivenDopri5Fn.last.status == [3, 0] and ecg._DrivenDopri5Fn.last_adj is None
    ok = gpu_train(shape, rtol, atol, {"first_step": 2.0}, dev, x, w, True)
    assert ok.rec.status == [0, 0] and ok.rec.n_attempts == [2, 1]


# ---------------------------------------------------------------------------------------------
# 5. NODE_RNN(solver="dopri5"): one step of the training recipe
# ---------------------------------------------------------------------------------------------
def test_node_rnn_training_step(dev):
    from fet_ode_amd import ecg
    shape, rtol, atol = TAPED[1]
    H, D, K, T, B = shape
    sd = DR.case_sd(H, D, K)
    x, y = DR.free_series(*shape), torch.tensor([0, 1, 0])
    l64, g64 = GR.node_rnn_step(sd, x, y, rtol, atol, torch.float64)
    ctl = [GR.node_rnn_step(sd if s == 0 else R.rounded(sd, s), x, y, rtol, atol)[1] for s in (0, 1, 2, 3)]

    def step(on):
        m = ecg.NODE_RNN(input_size=D, hidden_size=H, num_classes=2, num_basis=K, solver="dopri5", rtol=rtol, atol=atol)
        m.load_state_dict(sd)
        m = m.to(dev)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)   # train_rnn_node's recipe
        opt.zero_grad()
        with train_knob(on):
            loss = F.cross_entropy(m(x.to(dev)), y.to(dev))
            assert (m.enc.last_solve is not None) == on
            loss.backward()
        return m, opt, loss.item()

    m, opt, loss = step(True)
    _, _, loss_off = step(False)
    print(f"NODE_RNN(dopri5) loss: knob on {loss:.8f}, off {loss_off:.8f}, fp64 oracle {l64.item():.8f}")
    assert abs(loss - loss_off) <= 1e-6 * abs(loss_off)
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        if "hidden_basis" in n:
            assert not p.grad.any(), n
        else:
            TD.envelope(p.grad, [c[n] for c in ctl], g64[n], f"NODE_RNN d/d{n}")
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt.step()
    assert all(not torch.equal(p.detach(), before[n]) for n, p in m.named_parameters())
