"""The ECG NODE-RNN encoder under dopri5 on the CPU oracle WITH autograd — test side only:
tests/node_rnn_ref.py's field under oracle.torch_ref.odeint(method="dopri5"), one sample per solve like
the reference, differentiated by torch.autograd through every stage, the error ratio, the step-size
control, the initial-step selection and the dense output (torchdiffeq detaches none of them).

A solve that REPLAYS an attempt log (tests/driven_dopri5_ref.replay_options) takes every dt from the
log, so its step sizes, step starts and stage times are constants: its gradient is the gradient of the
discrete solve on that step sequence — what the sweep computes with step_grad = 0."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import driven_dopri5_ref as DR
import node_rnn_ref as R
from oracle import torch_ref as O

FIELD = list(R.FERRO) + ["gain", "bias_out"]          # the field's seven parameter tensors
NAMES = FIELD + ["h0", "lift.weight", "lift.bias"]


def weights(shape, seed=11):
    """The seeded loss weights w (B, T, H) of loss = sum(traj * w)."""
    H, D, K, T, B = shape
    return torch.randn(B, T, H, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def grad_solve(sd, xs, rtol, atol, w, dtype=torch.float32, options=None):
    """One sample xs (T, D) under autograd with loss = sum(traj * w), w (T, H): the trajectory, the
    oracle's trace and d loss / d (the seven field tensors, h0 (H,), the lift's weight and bias)."""
    r = R.NodeRnn(sd, dtype).requires_grad_()
    f = r.field
    t_grid = DR.grid(xs.shape[0], dtype)
    xs = xs.to(dtype)
    f.set(t_grid, xs)
    f.basis.st.reset()
    h0 = F.linear(xs[0:1], r.lift_w, r.lift_b)
    h0.retain_grad()
    tr = O.Dopri5Trace()
    traj = O.odeint(f, h0, t_grid, method="dopri5", rtol=rtol, atol=atol, options=options, trace=tr)
    (traj[:, 0] * w.to(dtype)).sum().backward()
    g = {n: p.grad for n, p in zip(FIELD, f.params())}
    g.update({"h0": h0.grad[0], "lift.weight": r.lift_w.grad, "lift.bias": r.lift_b.grad})
    return SimpleNamespace(traj=traj[:, 0].detach(), trace=tr, grads=g)


def batch_grads(runs):
    """Per-sample runs -> the batch's gradients: parameter tensors summed over the samples, h0 stacked."""
    return {n: torch.stack([r.grads[n] for r in runs]) if n == "h0" else sum(r.grads[n] for r in runs)
            for n in NAMES}


def oracle_set(sd, x, rtol, atol, w, options_of):
    """The fp64 oracle and the four fp32 controls (the fp32 oracle and three re-roundings of its
    parameters) over the batch x (B, T, D); options_of(b): sample b's solver options (None: a free
    run).  Returns (fp64 runs, [control runs])."""
    B = x.shape[0]
    e64 = [grad_solve(sd, x[b], rtol, atol, w[b], torch.float64, options_of(b)) for b in range(B)]
    ctl = []
    for s in (0, 1, 2, 3):
        sds = sd if s == 0 else R.rounded(sd, s)
        ctl.append([grad_solve(sds, x[b], rtol, atol, w[b], torch.float32, options_of(b)) for b in range(B)])
    return e64, ctl


@functools.lru_cache(maxsize=None)
def free_set(shape, rtol, atol):
    """oracle_set of a free-running case on DR.free_series; cached (shared, never modified)."""
    H, D, K, T, B = shape
    return oracle_set(DR.case_sd(H, D, K), DR.free_series(*shape), rtol, atol, weights(shape), lambda b: None)


def node_rnn_step(sd, x, y, rtol, atol, dtype=torch.float32):
    """NODE_RNN(solver="dopri5") on the oracle, one sample per solve: the cross-entropy loss and
    d loss / d every parameter (by the state_dict's names; None where autograd reaches none)."""
    r = R.NodeRnn(sd, dtype).requires_grad_()
    x = x.to(dtype)
    feats = []
    for b in range(x.shape[0]):
        t_grid = DR.grid(x.shape[1], dtype)
        r.field.set(t_grid, x[b])
        r.field.basis.st.reset()
        h0 = F.linear(x[b, 0:1], r.lift_w, r.lift_b)
        z_seq = O.odeint(r.field, h0, t_grid, method="dopri5", rtol=rtol, atol=atol)[:, 0, :]
        r.input_basis.st.reset()
        r.hidden_basis.st.reset()
        h = torch.zeros(1, r.H, dtype=dtype)
        for t in range(z_seq.size(0)):
            h = r.cell(z_seq[t:t + 1], h)
        feats.append(h)
    loss = F.cross_entropy(F.linear(torch.cat(feats, dim=0), r.head_w, r.head_b), y)
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in r.named_params().items()}
