"""CPU restatement of the input-driven Ferro field under the four fixed-grid methods and the step_size
option — test side only.  node_rnn_ref.DrivenField integrated by oracle.torch_ref.odeint (euler,
midpoint, rk4 3/8, rk4_classic; FixedGridODESolver's grid and linear interpolation between steps).
fp32: the controls; fp64: the yardstick; node_rnn_ref.rounded: the 6e-8 re-roundings.  One sample per
solve, from the reset state, like the reference."""
import torch
import torch.nn.functional as F

import node_rnn_ref as R
from oracle import torch_ref as O

METHODS = ("euler", "midpoint", "rk4", "rk4_classic")
N_M = {"euler": 1, "midpoint": 2, "rk4": 4, "rk4_classic": 4}


def options(step_size):
    return None if step_size is None else {"step_size": step_size}


class NodeRnn(R.NodeRnn):
    """node_rnn_ref.NodeRnn with the encoder's solver and step_size (NODE_RNN(solver=...), solver_options)."""

    def __init__(self, sd, dtype=torch.float32, method="rk4", step_size=None):
        super().__init__(sd, dtype)
        self.method, self.step_size = method, step_size

    def encode(self, xs, h0=None):
        t_grid = torch.linspace(0.0, 1.0, steps=xs.shape[0], dtype=xs.dtype)
        self.field.set(t_grid, xs)
        self.field.basis.st.reset()
        if h0 is None:
            h0 = F.linear(xs[0:1], self.lift_w, self.lift_b)
        return O.odeint(self.field, h0, t_grid, method=self.method, options=options(self.step_size))


def solve(sd, xs, method, step_size=None, dtype=torch.float32, h0=None, calls=True):
    """One sample xs (T, D) on linspace(0, 1, T): the trajectory (T, H), the end state prev (1, H + D) and
    every evaluation's (hx (1, H + D), phi (1, H)) in call order."""
    r = R.NodeRnn(sd, dtype)
    xs = xs.to(dtype)
    t_grid = torch.linspace(0.0, 1.0, steps=xs.shape[0], dtype=dtype)
    f = r.field
    f.set(t_grid, xs)
    f.basis.st.reset()
    f.calls = [] if calls else None
    if h0 is None:
        h0 = F.linear(xs[0:1], r.lift_w, r.lift_b)
    traj = O.odeint(f, h0.to(dtype), t_grid, method=method, options=options(step_size))
    return traj[:, 0], f.basis.prev.clone(), f.calls


def grads(sd, x, w, method, step_size=None, dtype=torch.float32):
    """d (sum_b <traj_b, w_b>) / d (the seven field parameters, h0, x) by autograd through the oracle,
    sample by sample; h0 = lift(x[:, 0]) is a leaf of its own, so x's gradient is the interpolator's."""
    r = R.NodeRnn(sd, dtype)
    ps = r.field.params()
    for p in ps:
        p.requires_grad_(True)
    x = x.to(dtype)
    h0 = F.linear(x[:, 0], r.lift_w, r.lift_b).detach().requires_grad_(True)
    xl = x.clone().requires_grad_(True)
    T = x.shape[1]
    t_grid = torch.linspace(0.0, 1.0, steps=T, dtype=dtype)
    loss = 0.0
    for b in range(x.shape[0]):
        r.field.set(t_grid, xl[b])
        r.field.basis.st.reset()
        traj = O.odeint(r.field, h0[b:b + 1], t_grid, method=method, options=options(step_size))
        loss = loss + (traj[:, 0] * w[:, b].to(dtype)).sum()
    loss.backward()
    return [p.grad for p in ps] + [h0.grad, xl.grad]


class Oracle:
    """Per sample of a batch x (B, T, D): "traj32" / "end32" / "calls32" (fp32), "traj64" / "end64" /
    "calls64" (fp64), "ctl" / "ctl_end" / "ctl_calls" (three re-rounded fp32 controls) — the keys of
    test_gpu_driven's oracle, so its check_traj / check_end read this one.  calls: per sample the
    evaluations' (hx (n_ev, H + D), phi (n_ev, H)).  Each group is computed once."""

    def __init__(self, sd, x, method, step_size=None):
        self.sd, self.x, self.method, self.step_size = sd, x, method, step_size
        self.B = x.shape[0]
        self.d = {}

    def __getitem__(self, key):
        if key not in self.d:
            with torch.no_grad():
                {"traj32": self._fp32, "end32": self._fp32, "calls32": self._fp32, "traj64": self._fp64,
                 "end64": self._fp64, "calls64": self._fp64, "ctl": self._controls, "ctl_end": self._controls,
                 "ctl_calls": self._controls}[key]()
        return self.d[key]

    def _run(self, sd, dtype):
        out = [solve(sd, self.x[b], self.method, self.step_size, dtype) for b in range(self.B)]
        # trajectories (T, 1, H), as test_gpu_driven's oracle keeps them
        return ([o[0].unsqueeze(1) for o in out], [o[1] for o in out],
                [(torch.cat([c[0] for c in o[2]]), torch.cat([c[1] for c in o[2]])) for o in out])

    def _fp32(self):
        self.d["traj32"], self.d["end32"], self.d["calls32"] = self._run(self.sd, torch.float32)

    def _fp64(self):
        self.d["traj64"], self.d["end64"], self.d["calls64"] = self._run(self.sd, torch.float64)

    def _controls(self):
        outs = [self._run(R.rounded(self.sd, s), torch.float32) for s in (1, 2, 3)]
        for k, key in enumerate(("ctl", "ctl_end", "ctl_calls")):
            self.d[key] = [[o[k][b] for o in outs] for b in range(self.B)]
