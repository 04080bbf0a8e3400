"""d loss / d the driving series of the ECG NODE-RNN encoder on the CPU oracle — test side only:
tests/node_rnn_ref.py's field under the oracle's rk4 and dopri5 (tests/driven_dopri5_ref.py) with the
series an autograd leaf and, unless `lift` is set, h0 = lift(x[:, 0]) DETACHED from it.  Through the lift
the gradient is 5 to 600 times the one through x(t), so a comparison that lets both in would not see
the x(t) path fail.  One sample per solve, like the reference."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import driven_dopri5_ref as DR
import node_rnn_ref as R
from oracle import torch_ref as O


def knot_weights(t_grid, tq):
    """LinearInterp1D's interval and weight at the times tq in the arithmetic of t_grid's dtype:
    (i, w) with knot i - 1 weighted 1 - w and knot i weighted w (tests/node_rnn_ref.interp)."""
    T = t_grid.numel()
    t = torch.clamp(tq.to(t_grid.dtype), t_grid[0], t_grid[-1])
    i = torch.searchsorted(t_grid, t).clamp(1, T - 1)
    t0, t1 = t_grid[i - 1], t_grid[i]
    return i, (t - t0) / (t1 - t0 + 1e-12)


def table_backward(t_grid, tq, adj_u, live):
    """grad_x (B, T, D) in fp64 from adj_u (B, n, D) at the times tq (B, n), rows e < live[b] only, and
    per knot the contribution count and the sum of the contributions' magnitudes (both (B, T, D))."""
    B, n, D = adj_u.shape
    T = t_grid.numel()
    gx, cnt, mag = (torch.zeros(B, T, D, dtype=torch.float64) for _ in range(3))
    tg = t_grid.double()
    for b in range(B):
        i, w = knot_weights(tg, tq[b, :live[b]])
        for e in range(live[b]):
            g = adj_u[b, e].double()
            for k, c in ((i[e] - 1, (1.0 - w[e]) * g), (i[e], w[e] * g)):
                gx[b, k] += c
                cnt[b, k] += 1
                mag[b, k] += c.abs()
    return gx, cnt, mag


def rk4_xgrad(sd, x, w, dtype=torch.float32, lift=False):
    """d (sum_b <traj_b, w[:, b]>) / d x (B, T, D) under the oracle's rk4, sample by sample."""
    r = R.NodeRnn(sd, dtype)
    out = []
    for b in range(x.shape[0]):
        xs = x[b].detach().clone().to(dtype).requires_grad_(True)
        h0 = F.linear(xs[0:1] if lift else xs[0:1].detach(), r.lift_w, r.lift_b)
        (r.encode(xs, h0)[:, 0] * w[:, b].to(dtype)).sum().backward()
        out.append(xs.grad)
    return torch.stack(out)


def rk4_set(sd, x, w, lift=False):
    """(fp64 gradient, [the fp32 oracle's and three re-rounded fp32 controls'])."""
    return rk4_xgrad(sd, x, w, torch.float64, lift), [rk4_xgrad(sd if s == 0 else R.rounded(sd, s), x, w, lift=lift)
                                                      for s in (0, 1, 2, 3)]


def node_rnn_xgrad(sd, x, y, dtype=torch.float32):
    """d cross_entropy(NODE_RNN(x), y) / d x: the full gradient, the lift included."""
    x = x.detach().clone().to(dtype).requires_grad_(True)
    logits, _ = R.NodeRnn(sd, dtype)(x)
    F.cross_entropy(logits, y).backward()
    return x.grad


def dopri5_xgrad(sd, xs, rtol, atol, w, dtype=torch.float32, options=None):
    """One sample xs (T, D) under the oracle's dopri5 with loss = sum(traj * w), w (T, H): the oracle's
    trace and d loss / d xs with h0 detached.  A run that replays an attempt log (DR.replay_options) has
    constant step sizes: the gradient of the discrete solve, what the sweep forms with step_grad = 0."""
    r = R.NodeRnn(sd, dtype)
    f = r.field
    t_grid = DR.grid(xs.shape[0], dtype)
    xs = xs.detach().clone().to(dtype).requires_grad_(True)
    f.set(t_grid, xs)
    f.basis.st.reset()
    h0 = F.linear(xs[0:1].detach(), r.lift_w, r.lift_b)
    tr = O.Dopri5Trace()
    traj = O.odeint(f, h0, t_grid, method="dopri5", rtol=rtol, atol=atol, options=options, trace=tr)
    (traj[:, 0] * w.to(dtype)).sum().backward()
    return SimpleNamespace(trace=tr, gx=xs.grad)


def dopri5_set(sd, x, rtol, atol, w, options_of):
    """Over the batch x (B, T, D), w (B, T, H): (fp64 runs, [four fp32 control run lists])."""
    B = x.shape[0]
    e64 = [dopri5_xgrad(sd, x[b], rtol, atol, w[b], torch.float64, options_of(b)) for b in range(B)]
    ctl = [[dopri5_xgrad(sd if s == 0 else R.rounded(sd, s), x[b], rtol, atol, w[b], torch.float32, options_of(b))
            for b in range(B)] for s in (0, 1, 2, 3)]
    return e64, ctl


@functools.lru_cache(maxsize=None)
def free_set(shape, rtol, atol):
    """dopri5_set of a free-running case on DR.free_series; cached (shared, never modified)."""
    import driven_dopri5_grad_ref as GR
    H, D, K, T, B = shape
    return dopri5_set(DR.case_sd(H, D, K), DR.free_series(*shape), rtol, atol, GR.weights(shape), lambda b: None)
