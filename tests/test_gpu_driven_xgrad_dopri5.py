"""The gradient to the driving series in the one-launch dopri5 solve of the ECG NODE-RNN encoder (DESIGN
§4.21): the sweep that also forms d loss / d x(t) (fetode_driven_dopri5_backward_x) beside the one that
does not (bitwise), d loss / d x with h0 detached against tests/driven_xgrad_ref.py in the two parts of
tests/test_gpu_driven_dopri5_train.py (frozen step: the oracles replay each sample's own GPU attempt
log; full: free-running on decided inputs), both by its envelope per sample
(|gpu - fp64| <= 4 worst fp32 control + 1e-5 scale), and the encoder's routing under the two knobs."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import driven_dopri5_grad_ref as GR
import driven_dopri5_ref as DR
import driven_xgrad_ref as XR
import test_gpu_driven as TD
import test_gpu_driven_dopri5 as TG
from test_gpu_driven_dopri5_train import train_knob
from test_gpu_driven_xgrad import xgrad

pytestmark = pytest.mark.gpu
FS = TG.FS
PAIRS = [(1e-2, 1e-3), (1e-3, 1e-4)]
FROZEN = [(s, r, a) for s in [(8, 1, 3, 9, 3), (64, 4, 16, 5, 2)] for r, a in PAIRS]
# (64, 4, 16, 5, 2) at 1e-2 / 1e-3 has a sample whose own fp32 controls stand 4.2e-2 from fp64: too close
# to the 5e-2 precondition to be a test
FULL = [((8, 1, 3, 9, 3), 1e-2, 1e-3), ((8, 1, 3, 9, 3), 1e-3, 1e-4), ((64, 4, 16, 5, 2), 1e-3, 1e-4)]
ids = TG.ids


# ---------------------------------------------------------------------------------------------
# 1. the sweep with adj_u beside the sweep without
# ---------------------------------------------------------------------------------------------
def taped(shape, rtol, atol, options, dev, x):
    from fet_ode_amd import ecg
    H, D, K, T, _ = shape
    f = TD.gpu_field(H, D, K, dev)
    tg = DR.grid(T).to(dev)
    xg = x.to(dev).contiguous()
    f.set_interpolator(ecg.LinearInterp1D(tg, xg))
    f.basis.reset_state()
    plan, d, keep = ecg._driven_plan(f, dev)
    with torch.no_grad():
        sol, rec, tape = ecg.driven_dopri5_taped_solve(f, plan, d, TD.lift(H, D, K, x).to(dev), xg, tg, rtol, atol,
                                                       options, None)
    return SimpleNamespace(f=f, plan=plan, d=d, keep=keep, tg=tg, sol=sol, rec=rec, tape=tape, tols=(rtol, atol), H=H, D=D)


def sweep(t, gsol, step_grad, with_u):
    """One of the two entries on the tape t: (adj, grad_h0, adj_u); every output starts as NaN."""
    from fet_ode_amd import _lib
    from fet_ode_amd.dopri5 import _TABLEAU
    tape, dev = t.tape, gsol.device
    T, B, H = gsol.shape
    adj = torch.full_like(tape.phi, float("nan"))
    gh0 = torch.full((B, H), float("nan"), device=dev)
    adj_u = torch.full((B, tape.max_ev, t.D), float("nan"), device=dev)
    args = [ctypes.byref(t.d), t.plan.data_ptr(), B, t.tg.data_ptr(), T, t.tols[0], t.tols[1],
            tape.opts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _TABLEAU.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
            None, tape.stats.data_ptr(), tape.att.data_ptr(), tape.max_att, tape.hx.data_ptr(), tape.phi.data_ptr(),
            tape.slope.data_ptr(), tape.init.data_ptr(), tape.max_ev, gsol.data_ptr(), int(step_grad), adj.data_ptr(),
            gh0.data_ptr()]
    lib = _lib.load()
    if with_u:
        _lib.check(lib.fetode_driven_dopri5_backward_x(*args, adj_u.data_ptr(), None), "x")
    else:
        _lib.check(lib.fetode_driven_dopri5_backward(*args, None), "plain")
    return adj, gh0, adj_u


@pytest.mark.parametrize("step_grad", [0, 1])
@pytest.mark.parametrize("case", [TG.REPLAY[0], TG.REPLAY[2]], ids=ids)
def test_sweep_bitwise_the_plain_sweep(dev, case, step_grad):
    shape, rtol, atol = case
    H, D, K, T, B = shape
    t = taped(shape, rtol, atol, {"first_step": FS}, dev, DR.series(*shape))
    assert t.rec.status == [0] * B
    gsol = torch.randn(T, B, H, generator=torch.Generator().manual_seed(5)).to(dev)
    a0, g0, _ = sweep(t, gsol, step_grad, False)
    a1, g1, u1 = sweep(t, gsol, step_grad, True)
    assert torch.isfinite(a0).all() and torch.equal(a0, a1) and torch.equal(g0, g1)
    n_rej = 0
    for b in range(B):
        n = t.rec.nfev[b]
        assert torch.isfinite(u1[b]).all() and u1[b, :n].any() and not u1[b, n:].any()   # rows at or beyond nfev: zero
        for k, a in enumerate(t.rec.attempts[b]):
            if not a[3]:
                n_rej += 1
                # a rejected attempt: exact zeros on the frozen step sequence, a contribution through the control
                assert bool(u1[b, 1 + 6 * k:7 + 6 * k].any()) == bool(step_grad and a0[b, 1 + 6 * k:7 + 6 * k].any())
    assert n_rej >= 1, "the cases are there for their rejected attempts"


def test_stopped_sample_gets_zeros(dev):
    """tests/test_gpu_driven_dopri5.py's case: max_num_steps = 1 stops sample 0 (status 3): all of its
    adj_u is zero, and the other sample's rows are bitwise its solo run."""
    shape, rtol, atol = (3, 1, 2, 2, 2), 3e-2, 3e-3
    H, D, K, T, B = shape
    opts = {"first_step": 2.0, "max_num_steps": 1}
    x = DR.series(*shape)
    gsol = torch.randn(T, B, H, generator=torch.Generator().manual_seed(6)).to(dev)
    t = taped(shape, rtol, atol, opts, dev, x)
    assert t.rec.status == [3, 0]
    adj, gh0, u = sweep(t, gsol, 1, True)
    assert not u[0].any() and not adj[0].any() and not gh0[0].any()
    one = taped(shape, rtol, atol, opts, dev, x[1:2])
    a1, g1, u1 = sweep(one, gsol[:, 1:2].contiguous(), 1, True)
    assert u1.any() and torch.equal(u[1], u1[0]) and torch.equal(adj[1], a1[0]) and torch.equal(gh0[1], g1[0])


# ---------------------------------------------------------------------------------------------
# 2. d loss / d x with h0 detached
# ---------------------------------------------------------------------------------------------
def gpu_train_x(shape, rtol, atol, options, dev, x, w, step_grad):
    """ecg.driven_dopri5_train with the series a leaf and h0 = lift(x[:, 0]) detached from it,
    loss = sum(sol * w): d loss / d x (B, T, D) and the record."""
    from fet_ode_amd import ecg
    H, D, K, T, _ = shape
    enc = TG.encoder(shape, rtol, atol, dev)
    f = enc.odefunc
    t_grid, xg = DR.grid(T).to(dev), x.to(dev).requires_grad_(True)
    f.set_interpolator(ecg.LinearInterp1D(t_grid, xg))
    f.basis.reset_state()
    h0 = enc.lift(xg[:, 0].detach())
    with train_knob(True, step_grad), xgrad(True):
        out = ecg.driven_dopri5_train(f, h0, t_grid.cpu(), False, rtol, atol, options, reset=True, t=t_grid)
        assert out is not None
        sol, rec = out
        (sol * w.permute(1, 0, 2).to(dev, torch.float32)).sum().backward()
    assert xg.grad is not None and xg.grad.shape == x.shape
    return xg.grad, rec


def check_samples(got, e64, ctl, what):
    for b in range(got.shape[0]):
        TD.envelope(got[b], [c[b].gx for c in ctl], e64[b].gx, f"{what} sample {b} d/dx")


@pytest.mark.parametrize("case", FROZEN, ids=ids)
def test_frozen_step_series_gradient(dev, case):
    shape, rtol, atol = case
    H, D, K, T, B = shape
    sd, x, w = DR.case_sd(H, D, K), DR.series(*shape), GR.weights(shape)
    got, rec = gpu_train_x(shape, rtol, atol, {"first_step": FS}, dev, x, w, step_grad=False)
    assert rec.status == [0] * B
    att = rec.attempts
    e64, ctl = XR.dopri5_set(sd, x, rtol, atol, w, lambda b: DR.replay_options(att[b], FS))
    check_samples(got, e64, ctl, f"frozen {ids(case)}")


@pytest.mark.parametrize("case", FULL, ids=ids)
def test_full_series_gradient_free_running(dev, case):
    shape, rtol, atol = case
    H, D, K, T, B = shape
    x, w = DR.free_series(*shape), GR.weights(shape)
    # preconditions, on the CPU oracle alone: a set-up error, not a kernel error, where these fail
    for b, (r32, r64) in enumerate(DR.free_pair(shape, rtol, atol)):
        assert DR.decided(r32, r64), (b, r32.trace.attempts, r64.trace.attempts)
    e64, ctl = XR.free_set(shape, rtol, atol)
    acc = [DR.accepts(r.trace.attempts) for r in e64]
    for c in ctl:
        assert [DR.accepts(r.trace.attempts) for r in c] == acc
    for b in range(B):
        d = max(TD.nrel(c[b].gx, e64[b].gx) for c in ctl)
        print(f"full {ids(case)} sample {b}: worst fp32 control stands {d:.3e} from fp64")
        assert d <= 5e-2, (b, d)
    got, rec = gpu_train_x(shape, rtol, atol, {}, dev, x, w, step_grad=True)
    assert [DR.accepts(a) for a in rec.attempts] == acc
    check_samples(got, e64, ctl, f"full {ids(case)}")


# ---------------------------------------------------------------------------------------------
# 3. the encoder's routing
# ---------------------------------------------------------------------------------------------
def test_encoder_routing(dev):
    from fet_ode_amd import dopri5, ecg
    shape, rtol, atol = FROZEN[1]
    x = DR.series(*shape).to(dev)
    enc = TG.encoder(shape, rtol, atol, dev)
    with torch.no_grad():
        ref = enc(x)
    for rows in ([0, 1, 2], [1]):
        dopri5.dopri5_solve.last = None
        xr = x[rows].clone().requires_grad_(True)
        with train_knob(True), xgrad(True):
            out = enc(xr)
            assert isinstance(enc.last_solve, ecg.DrivenDopri5Solve) and dopri5.dopri5_solve.last is None
            assert type(out.grad_fn).__name__ == "_DrivenDopri5FnBackward" and torch.equal(out.detach(), ref[:, rows])
            out.sum().backward()
        assert torch.isfinite(xr.grad).all() and xr.grad.any() and xr.grad.shape == xr.shape
        assert xr.grad[:, 1:].any()                     # beyond the lift's knot: the x(t) path
    # either knob off: the old path
    for tr, xg in ((True, False), (False, True)):
        dopri5.dopri5_solve.last = None
        xr = x[:1].clone().requires_grad_(True)
        with train_knob(tr), xgrad(xg):
            out = enc(xr)
        assert enc.last_solve is None and isinstance(dopri5.dopri5_solve.last, dopri5._Dopri5Grad), (tr, xg)
