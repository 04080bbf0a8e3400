"""CPU restatement of the ECG NODE-RNN (compare_noise_ecg.py:848-986, :325-341) — test side only.

Composed from oracle.torch_ref (ferro_forward, FerroParams, FerroState, odeint), which already passes
t to the field.  Written in the reference's own op order, so on CPU in fp32 it reproduces the
reference classes bit for bit (pinned by tests/golden/node_rnn.npz, tests/test_node_rnn_golden.py);
in fp64 it is the yardstick the GPU tests measure against.  One sample per solve, like the reference.
"""
import torch
import torch.nn.functional as F

from oracle import torch_ref as O

FERRO = ("k", "Ec", "Ps", "bias", "coef")


def interp(t_grid, x_grid, t_query):
    """LinearInterp1D.__call__ (:861-872), x_grid (T, D)."""
    T = t_grid.numel()
    t = torch.clamp(t_query, t_grid[0], t_grid[-1])
    i = torch.searchsorted(t_grid, t).clamp(1, T - 1)
    t0, t1 = t_grid[i - 1], t_grid[i]
    x0, x1 = x_grid[i - 1], x_grid[i]
    w = (t - t0) / (t1 - t0 + 1e-12)
    return (1.0 - w) * x0 + w * x1


def stage_times(t_grid):
    """The 4 (T - 1) evaluation times of torchdiffeq's rk4 on the grid, in call order."""
    out = []
    for t0, t1 in zip(t_grid[:-1], t_grid[1:]):
        dt = t1 - t0
        out += [t0, t0 + dt * O._ONE_THIRD, t0 + dt * O._TWO_THIRDS, t1]
    return torch.stack(out)


class Ferro:
    """One FerroelectricBasis: parameters + its two state buffers."""

    def __init__(self, sd, prefix, dtype=torch.float32):
        self.p = O.FerroParams.from_state_dict(sd, prefix).to(dtype)
        i, o, K = self.p.k.shape
        self.st = O.FerroState(i, o, K, dtype)
        self.dtype = dtype

    def __call__(self, x):
        return O.ferro_forward(x, self.p, self.st)

    def params(self):
        return [getattr(self.p, n) for n in FERRO]

    @property
    def prev(self):
        """compact (B, in) view of prev_x"""
        return self.st.prev_x[:, :, 0, 0]


class DrivenField:
    """InputDrivenKANODEFunc (:875-907)."""

    def __init__(self, sd, prefix="", dtype=torch.float32):
        self.basis = Ferro(sd, prefix + "basis.", dtype)
        self.gain = sd[prefix + "gain"].detach().to(dtype)
        self.bias = sd[prefix + "bias"].detach().to(dtype)
        self.t_grid = self.x_grid = None
        self.calls = None   # optional record of (hx, phi) per evaluation

    def set(self, t_grid, x_grid):
        self.t_grid, self.x_grid = t_grid, x_grid

    def __call__(self, t, h):
        x_t = interp(self.t_grid, self.x_grid, t).unsqueeze(0)
        hx = torch.cat([h, x_t], dim=-1)
        phi = self.basis(hx)
        if self.calls is not None:
            self.calls.append((hx.detach().clone(), phi.detach().clone()))
        return torch.tanh(phi) * self.gain + self.bias

    def params(self):
        return self.basis.params() + [self.gain, self.bias]


class NodeRnn:
    """NODE_RNN (:949-986) with its OneODEEncoder (:910-946) and FullyNonlinearKANCell (:325-341)."""

    def __init__(self, sd, dtype=torch.float32):
        self.dtype = dtype
        self.field = DrivenField(sd, "enc.odefunc.", dtype)
        self.lift_w, self.lift_b = sd["enc.lift.weight"].detach().to(dtype), sd["enc.lift.bias"].detach().to(dtype)
        self.input_basis = Ferro(sd, "rnn_cell.input_basis.", dtype)
        self.hidden_basis = Ferro(sd, "rnn_cell.hidden_basis.", dtype)
        self.head_w, self.head_b = sd["head.weight"].detach().to(dtype), sd["head.bias"].detach().to(dtype)
        self.H = self.lift_w.shape[0]

    def named_params(self):
        out = {}
        for pre, fb in (("enc.odefunc.basis.", self.field.basis), ("rnn_cell.input_basis.", self.input_basis),
                        ("rnn_cell.hidden_basis.", self.hidden_basis)):
            for n, p in zip(FERRO, fb.params()):
                out[pre + n] = p
        out.update({"enc.odefunc.gain": self.field.gain, "enc.odefunc.bias": self.field.bias,
                    "enc.lift.weight": self.lift_w, "enc.lift.bias": self.lift_b,
                    "head.weight": self.head_w, "head.bias": self.head_b})
        return out

    def requires_grad_(self):
        for p in self.named_params().values():
            p.requires_grad_(True)
        return self

    def encode(self, xs, h0=None):
        """OneODEEncoder.forward for one sample xs (T, D): the trajectory (T, 1, H)."""
        T = xs.shape[0]
        t_grid = torch.linspace(0.0, 1.0, steps=T, dtype=xs.dtype)
        self.field.set(t_grid, xs)
        self.field.basis.st.reset()
        if h0 is None:
            h0 = F.linear(xs[0:1], self.lift_w, self.lift_b)
        return O.odeint(self.field, h0, t_grid, method="rk4", rtol=1e-3, atol=1e-4)

    def cell(self, x_t, h_prev):
        x_phi = self.input_basis(x_t).view(x_t.size(0), -1)
        h_phi = self.hidden_basis(h_prev).view(h_prev.size(0), -1)
        return torch.tanh(torch.cat([x_phi, h_phi], dim=1))[:, :self.H]

    def __call__(self, x):
        """logits (B, C) and the per-sample trajectories [(T, 1, H)]."""
        if x.dim() == 2:
            x = x.unsqueeze(-1)
        feats, trajs = [], []
        for b in range(x.shape[0]):
            h_traj = self.encode(x[b])
            trajs.append(h_traj)
            z_seq = h_traj[:, 0, :]
            self.input_basis.st.reset()
            self.hidden_basis.st.reset()
            h = torch.zeros(1, self.H, dtype=x.dtype)
            for t in range(z_seq.size(0)):
                h = self.cell(z_seq[t:t + 1], h)
            feats.append(h)
        return F.linear(torch.cat(feats, dim=0), self.head_w, self.head_b), trajs

    def end_states(self):
        return {"enc.odefunc.basis.prev_x": self.field.basis.st.prev_x,
                "rnn_cell.input_basis.prev_x": self.input_basis.st.prev_x,
                "rnn_cell.hidden_basis.prev_x": self.hidden_basis.st.prev_x}


def make_sd(H, D, K, C=2, seed=0):
    """A reference-shaped NODE_RNN state_dict (parameters only) with FerroelectricBasis's init
    distributions, for shapes the fixture does not hold.  Not the reference's RNG order."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def ferro(prefix, i, o):
        sd[prefix + "k"] = torch.rand(i, o, K, generator=g) * 2 + 0.5
        sd[prefix + "Ec"] = torch.rand(i, o, K, generator=g) * 2 + 0.5
        sd[prefix + "Ps"] = torch.rand(i, o, K, generator=g) * 1.5 + 0.5
        sd[prefix + "bias"] = torch.randn(i, o, K, generator=g) * 0.1
        sd[prefix + "coef"] = torch.randn(i, o, K, generator=g)

    sd["enc.lift.weight"] = (torch.rand(H, D, generator=g) * 2 - 1) / D ** 0.5
    sd["enc.lift.bias"] = (torch.rand(H, generator=g) * 2 - 1) / D ** 0.5
    ferro("enc.odefunc.basis.", H + D, H)
    sd["enc.odefunc.gain"] = 1.0 + 0.2 * torch.randn(H, generator=g)
    sd["enc.odefunc.bias"] = 0.1 * torch.randn(H, generator=g)
    ferro("rnn_cell.input_basis.", H, H)
    ferro("rnn_cell.hidden_basis.", H, H)
    sd["head.weight"] = (torch.rand(C, H, generator=g) * 2 - 1) / H ** 0.5
    sd["head.bias"] = (torch.rand(C, generator=g) * 2 - 1) / H ** 0.5
    return sd


def rounded(sd, seed, rel=6e-8):
    """Every parameter re-rounded by a relative 6e-8 (one fp32 ulp): the controls of the envelope
    bars (tests/test_gpu_ecg.py's rule)."""
    g = torch.Generator().manual_seed(seed)
    return {k: (v * (1.0 + rel * (2 * torch.randint(0, 2, v.shape, generator=g) - 1))).to(v.dtype)
            if v.is_floating_point() else v for k, v in sd.items()}
