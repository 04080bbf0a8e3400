"""The input-driven Ferro field (ECG NODE-RNN encoder) on the GPU: the driving table, the bare field,
the one-launch solve (fetode_driven_fixed) in every samples-per-workgroup variant, its tape and
reverse sweep, the per-stage path beside it, and NODE_RNN end to end — against tests/node_rnn_ref.py
(pinned bit for bit to the reference classes by tests/golden/node_rnn.npz).

Bars: 1e-5 per row / slice where the fp32 oracle itself is within 1e-6 of its fp64 run (the
project's single-evaluation and one-step bars); elsewhere the reference-fp32 envelope of
tests/test_gpu_ecg.py, |gpu - fp64| <= 4 worst(|fp32 oracle - fp64| over the oracle's own run and three
6e-8 re-roundings of its parameters) + 1e-5 scale.  Gradients: 2e-4 of the fixture, and at production
width max(1e-4, 2 x the per-stage path's error, 2 x the worst fp32 control) normwise per tensor
against the fp64 oracle's autograd (the rule of tests/test_gpu_dopri5_train.py)."""
import ctypes
import functools
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

import node_rnn_ref as R
from conftest import golden_sd, load_golden

pytestmark = pytest.mark.gpu
SPW = (1, 2, 4)
FIX = (8, 1, 3, 9)          # the fixture's H, D, K, T
WIDE = (64, 1, 10, 12)


@contextmanager
def spw(v):
    from fet_ode_amd import ecg
    prev = ecg.set_driven_samples_per_workgroup(v)
    try:
        yield
    finally:
        ecg.set_driven_samples_per_workgroup(prev)


@contextmanager
def per_stage():
    from fet_ode_amd import ecg
    prev = ecg.set_fused_driven(False)
    try:
        yield
    finally:
        ecg.set_fused_driven(prev)


@functools.lru_cache(maxsize=None)
def case_sd(H, D, K):
    if (H, D, K) == FIX[:3]:
        return golden_sd(load_golden("node_rnn"))
    return R.make_sd(H, D, K, seed=100 * H + 10 * D + K)


@functools.lru_cache(maxsize=None)
def case_x(H, D, K, T, B, ecg_like=False):
    if ecg_like:
        from oracle.ecg_ref import ecg_x
        return ecg_x(B, T=T, seed=5).unsqueeze(-1)
    g = torch.Generator().manual_seed(7 + T + 13 * D)
    return torch.randn(B, T, D, generator=g)


def rows_rel(a, b):
    """per-row relative error of (..., H) tensors"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-30))


class Oracle:
    """Per sample: the fp32 oracle's trajectory, its (h_j, prev_j) at every step start and its end
    state ("traj32", "recs", "end32"); the fp64 trajectory and end state ("traj64", "end64"); three
    re-rounded fp32 controls ("ctl", "ctl_end").  Each group is computed once, when first asked for."""

    def __init__(self, H, D, K, T, B, ecg_like):
        self.sd, self.x, self.T, self.B = case_sd(H, D, K), case_x(H, D, K, T, B, ecg_like), T, B
        self.d = {}

    def __getitem__(self, key):
        if key not in self.d:
            with torch.no_grad():
                {"traj32": self._fp32, "recs": self._fp32, "end32": self._fp32, "traj64": self._fp64,
                 "end64": self._fp64, "ctl": self._controls, "ctl_end": self._controls}[key]()
        return self.d[key]

    def _fp32(self):
        r32 = R.NodeRnn(self.sd)
        d = self.d
        d["traj32"], d["recs"], d["end32"] = [], [], []
        for b in range(self.B):
            xs = self.x[b]
            t_grid = torch.linspace(0.0, 1.0, steps=self.T)
            f = r32.field
            f.set(t_grid, xs)
            f.basis.st.reset()
            h = F.linear(xs[0:1], r32.lift_w, r32.lift_b)
            tr, recs = [h], []
            for t0, t1 in zip(t_grid[:-1], t_grid[1:]):
                recs.append((h.clone(), f.basis.prev.clone()))
                h = h + R.O.rk4_alt_step(f, t0, t1 - t0, t1, h)
                tr.append(h)
            d["traj32"].append(torch.stack(tr))
            d["recs"].append(recs)
            d["end32"].append(f.basis.prev.clone())
        assert torch.equal(d["traj32"][0], r32.encode(self.x[0]))   # the manual loop is the oracle's odeint

    def _fp64(self):
        r64 = R.NodeRnn(self.sd, torch.float64)
        self.d["traj64"], self.d["end64"] = [], []
        for b in range(self.B):
            self.d["traj64"].append(r64.encode(self.x[b].double()))
            self.d["end64"].append(r64.field.basis.prev.clone())

    def _controls(self):
        rc = [R.NodeRnn(R.rounded(self.sd, s)) for s in (1, 2, 3)]
        self.d["ctl"], self.d["ctl_end"] = [], []
        for b in range(self.B):
            self.d["ctl"].append([c.encode(self.x[b]) for c in rc])
            self.d["ctl_end"].append([c.field.basis.prev.clone() for c in rc])


@functools.lru_cache(maxsize=None)
def oracle(H, D, K, T, B, ecg_like=False):
    return Oracle(H, D, K, T, B, ecg_like)


def envelope(got, ctl32, e64, what):
    """|got - fp64| <= 4 worst |fp32 control - fp64| + 1e-5 scale (maxima over the tensor)."""
    got, e64 = got.detach().double().cpu(), e64.double()
    scale = e64.abs().max().item() + 1e-12
    spread = max((c.double() - e64).abs().max().item() for c in ctl32)
    err = (got - e64).abs().max().item()
    print(f"{what}: |gpu - fp64| = {err:.3e}, worst fp32 control {spread:.3e}, scale {scale:.3e}")
    assert err <= 4.0 * spread + 1e-5 * scale, (what, err, spread, scale)


def check_traj(got, orc, b, what):
    """A (T, H) trajectory of sample b: 1e-5 per slice where the oracle's fp32 - fp64 distance is below
    1e-6, the envelope otherwise."""
    t32, t64 = orc["traj32"][b][:, 0], orc["traj64"][b][:, 0]
    own = rows_rel(t32, t64)
    rel = rows_rel(got, t32)
    well = own < 1e-6
    worst = rel[well].max().item() if well.any() else 0.0
    print(f"{what}: {int(well.sum())}/{len(well)} well-conditioned slices, worst rel {worst:.3e}, "
          f"oracle fp32-fp64 worst {own.max().item():.3e}")
    assert worst <= 1e-5, (what, worst)
    if not well.all():
        ill = ~well
        envelope(got[ill.to(got.device)], [orc["traj32"][b][ill, 0]] + [c[ill, 0] for c in orc["ctl"][b]], t64[ill],
                 what + " (ill-conditioned slices)")


def check_end(got, orc, b, what):
    e32, e64 = orc["end32"][b], orc["end64"][b]
    if rows_rel(e32, e64).max().item() < 1e-6:
        r = rows_rel(got, e32).max().item()
        print(f"{what}: end state rel {r:.3e}")
        assert r <= 1e-5, (what, r)
    else:
        envelope(got, [e32] + orc["ctl_end"][b], e64, what + " end state")


def gpu_field(H, D, K, dev):
    from fet_ode_amd import ecg
    sd = case_sd(H, D, K)
    f = ecg.InputDrivenKANODEFunc(D, H, K)
    f.load_state_dict({k[len("enc.odefunc."):]: v for k, v in sd.items() if k.startswith("enc.odefunc.")},
                      strict=False)
    return f.to(dev)


def gpu_encoder(H, D, K, dev):
    from fet_ode_amd import ecg
    sd = case_sd(H, D, K)
    e = ecg.OneODEEncoder(D, H, K)
    e.load_state_dict({k[len("enc."):]: v for k, v in sd.items() if k.startswith("enc.")}, strict=False)
    return e.to(dev)


class Raw:
    """The C ABI driven directly: one field, one batch of driving series."""

    def __init__(self, H, D, K, T, x, dev):
        from fet_ode_amd import _lib, ecg
        self.L, self.lib = _lib, _lib.load()
        self.f = gpu_field(H, D, K, dev)
        self.plan, self.d, self.keep = ecg._driven_plan(self.f, dev)
        self.tg, self.tq, self.dt = ecg._driven_grid(torch.linspace(0.0, 1.0, steps=T), dev)
        self.x = x.to(dev).contiguous()
        self.u = ecg.driven_table(self.tg, self.x, self.tq)
        self.H, self.In, self.T, self.dev = H, H + D, T, dev

    def solve(self, h0, prev0=None, step0=0, n_steps=None, tape=False):
        n_steps = self.T - 1 - step0 if n_steps is None else n_steps
        B = h0.shape[0]
        h0 = h0.to(self.dev).contiguous()
        prev0 = None if prev0 is None else prev0.to(self.dev).contiguous()
        sol = torch.full((n_steps, B, self.H), float("nan"), device=self.dev)
        pout = torch.full((B, self.In), float("nan"), device=self.dev)
        dt = self.dt[step0:].contiguous()
        args = [ctypes.byref(self.d), self.plan.data_ptr(), self.L.RK4, h0.data_ptr(), B, self.u.data_ptr(),
                self.u.shape[0], 4 * step0, dt.data_ptr(), n_steps, self.L.ptr(prev0), sol.data_ptr(), pout.data_ptr()]
        if tape:
            thx = torch.full((self.u.shape[0], B, self.In), float("nan"), device=self.dev)
            tphi = torch.full((self.u.shape[0], B, self.H), float("nan"), device=self.dev)
            self.L.check(self.lib.fetode_driven_fixed_tape(*args, thx.data_ptr(), tphi.data_ptr(), None), "tape")
            return sol, pout, thx, tphi
        self.L.check(self.lib.fetode_driven_fixed(*args, None), "fixed")
        return sol, pout


def lift(H, D, K, x):
    sd = case_sd(H, D, K)
    return F.linear(x[:, 0], sd["enc.lift.weight"], sd["enc.lift.bias"])


# ---------------------------------------------------------------------------------------------
# 1. driving table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("T", [2, 9])
def test_driving_table_bitwise(dev, D, T):
    from fet_ode_amd import ecg
    t_grid = torch.linspace(0.0, 1.0, steps=T)
    g = torch.Generator().manual_seed(D + 10 * T)
    x = torch.randn(3, T, D, generator=g)
    tq = R.stage_times(t_grid)                      # every knot (first and last included) and the thirds
    tg_d, tq_d, dt_d = ecg._driven_grid(t_grid, dev)
    assert torch.equal(tq_d.cpu(), tq) and torch.equal(dt_d.cpu(), t_grid[1:] - t_grid[:-1])
    assert bool((tq[0] == t_grid[0]) & (tq[-1] == t_grid[-1])) and all(bool((tq == k).any()) for k in t_grid)
    tq = torch.cat([tq, torch.tensor([-0.5, 1.5, 0.123456, 0.999999])])   # clamped below / above, off-knot
    exp = torch.stack([torch.stack([R.interp(t_grid, x[b], tq[e]) for b in range(3)]) for e in range(len(tq))])
    got = ecg.driven_table(tg_d, x.to(dev), tq.to(dev))
    assert got.shape == exp.shape and torch.equal(got.cpu(), exp), (got.cpu() - exp).abs().max().item()


# ---------------------------------------------------------------------------------------------
# 2. bare field
# ---------------------------------------------------------------------------------------------
def test_bare_field_sequence(dev):
    from fet_ode_amd import ecg
    g = load_golden("node_rnn")
    H, D, K, T = FIX
    f = gpu_field(H, D, K, dev)
    x = torch.from_numpy(g["x"])
    f.set_interpolator(ecg.LinearInterp1D(torch.linspace(0.0, 1.0, steps=T).to(dev), x[1].to(dev)))
    f.basis.reset_state()
    hs, ts = torch.from_numpy(g["field/h"]), torch.from_numpy(g["field/t"])
    with torch.no_grad():
        for c in range(3):
            y = f(ts[c].to(dev), hs[c].to(dev))
            r = rows_rel(y, torch.from_numpy(g[f"field/y{c}"])).max().item()
            print(f"field call {c}: rel {r:.3e}")
            assert r <= 1e-5, (c, r)
            assert torch.equal(f.basis._prev.cpu(), torch.from_numpy(g[f"field/prev{c}"])), c
            assert f.basis.prev_x.shape == (1, H + D, H, K)


# ---------------------------------------------------------------------------------------------
# 3. one-step local parity at every step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [FIX, WIDE], ids=["fixture", "wide"])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_one_step_parity_every_step(dev, shape, B):
    H, D, K, T = shape
    orc = oracle(H, D, K, T, 5)
    raw = Raw(H, D, K, T, case_x(H, D, K, T, 5)[:B], dev)
    worst = 0.0
    for v in SPW:
        with spw(v):
            for j in range(T - 1):
                h = torch.cat([orc["recs"][b][j][0] for b in range(B)])
                p = torch.cat([orc["recs"][b][j][1] for b in range(B)])
                sol, _ = raw.solve(h, p, step0=j, n_steps=1)
                exp = torch.cat([orc["traj32"][b][j + 1] for b in range(B)])
                r = rows_rel(sol[0], exp).max().item()
                worst = max(worst, r)
                assert r <= 1e-5, (v, j, r)
    print(f"one-step parity H={H} K={K} B={B}: worst row rel {worst:.3e}")


# ---------------------------------------------------------------------------------------------
# 4. one launch == split launches, 5. row independence (bitwise)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [FIX, WIDE], ids=["fixture", "wide"])
def test_split_launches_bitwise(dev, shape):
    H, D, K, T = shape
    x = case_x(H, D, K, T, 5)[:3]
    raw = Raw(H, D, K, T, x, dev)
    h0 = lift(H, D, K, x)
    for v in SPW:
        with spw(v):
            full, pfull = raw.solve(h0)
            assert torch.isfinite(full).all() and torch.isfinite(pfull).all()
            for cut in sorted({1, (T - 1) // 2, T - 2}):
                a, pa = raw.solve(h0, n_steps=cut)
                b, pb = raw.solve(a[-1], pa, step0=cut)
                assert torch.equal(torch.cat([a, b]), full) and torch.equal(pb, pfull), (v, cut)
            # the taped kernel computes the same solve
            t_full = raw.solve(h0, tape=True)
            assert torch.equal(t_full[0], full) and torch.equal(t_full[1], pfull), v
            assert torch.equal(t_full[2][-1], pfull) and torch.isfinite(t_full[3]).all(), v


@pytest.mark.parametrize("shape", [FIX, WIDE], ids=["fixture", "wide"])
def test_row_independence_bitwise(dev, shape):
    H, D, K, T = shape
    x = case_x(H, D, K, T, 5)
    h0 = lift(H, D, K, x)
    ref = None
    for v in SPW:
        with spw(v):
            full, pfull = Raw(H, D, K, T, x, dev).solve(h0)      # odd B: the last workgroup is partly empty
            for b in range(5):
                one, pone = Raw(H, D, K, T, x[b:b + 1], dev).solve(h0[b:b + 1])
                assert torch.equal(one[:, 0], full[:, b]) and torch.equal(pone[0], pfull[b]), (v, b)
        # the variants share one arithmetic: their results are identical too
        ref = full if ref is None else ref
        assert torch.equal(full, ref), v


# ---------------------------------------------------------------------------------------------
# 6. shape edges, 7. production width, 8. fused against per-stage
# ---------------------------------------------------------------------------------------------
EDGES = [(8, 1, 3, 2), (8, 1, 3, 3), (8, 2, 3, 5), (24, 3, 12, 5), (24, 1, 10, 4), (64, 1, 10, 3), (64, 2, 12, 4),
         (64, 3, 3, 3)]


def encoder_run(H, D, K, T, B, dev, ecg_like=False):
    e = gpu_encoder(H, D, K, dev)
    with torch.no_grad():
        traj = e(case_x(H, D, K, T, B, ecg_like).to(dev), return_traj=True)
    return traj, e.odefunc.basis


@pytest.mark.parametrize("shape", EDGES, ids=lambda s: "H%d-D%d-K%d-T%d" % s)
def test_shape_edges_vs_oracle(dev, shape):
    H, D, K, T = shape
    B = 3
    orc = oracle(H, D, K, T, B)
    for v in SPW:
        with spw(v):
            traj, basis = encoder_run(H, D, K, T, B, dev)
        assert traj.shape == (T, B, H)
        for b in range(B):
            check_traj(traj[:, b], orc, b, f"spw {v} sample {b}")
        assert basis.prev_x.shape == (1, H + D, H, K)
        check_end(basis._prev, orc, B - 1, f"spw {v}")


def test_production_width_envelope(dev):
    """H = 64, K = 10, D = 1, T = 24, B = 4 on ECG-shaped series: the envelope bar over the whole
    trajectory, whatever the field's conditioning turns out to be."""
    H, D, K, T, B = 64, 1, 10, 24, 4
    orc = oracle(H, D, K, T, B, True)
    for v in SPW:
        with spw(v):
            traj, basis = encoder_run(H, D, K, T, B, dev, True)
        for b in range(B):
            envelope(traj[:, b], [orc["traj32"][b][:, 0]] + [c[:, 0] for c in orc["ctl"][b]], orc["traj64"][b][:, 0],
                     f"production spw {v} sample {b}")
        envelope(basis._prev, [orc["end32"][B - 1]] + orc["ctl_end"][B - 1], orc["end64"][B - 1],
                 f"production spw {v} end state")


@pytest.mark.parametrize("shape", [FIX, (24, 3, 12, 5), (64, 1, 10, 24)], ids=lambda s: "H%d-D%d-K%d-T%d" % s)
def test_fused_vs_per_stage(dev, shape):
    H, D, K, T = shape
    B, ecg_like = (4, True) if H == 64 else (3, False)
    orc = oracle(H, D, K, T, B, ecg_like)
    fused, fb = encoder_run(H, D, K, T, B, dev, ecg_like)
    with per_stage():
        staged, sb = encoder_run(H, D, K, T, B, dev, ecg_like)
    assert not torch.equal(fused, staged)    # two different programs (guards a silent fall-back)
    for b in range(B):
        check_traj(fused[:, b], orc, b, f"fused sample {b}")
        check_traj(staged[:, b], orc, b, f"per-stage sample {b}")
        well = (rows_rel(orc["traj32"][b][:, 0], orc["traj64"][b][:, 0]) < 1e-6).to(dev)
        if well.any():
            r = rows_rel(fused[:, b][well], staged[:, b][well]).max().item()
            print(f"fused vs per-stage sample {b}: {r:.3e}")
            assert r <= 1e-5, (b, r)
    check_end(fb._prev, orc, B - 1, "fused")
    check_end(sb._prev, orc, B - 1, "per-stage")
    assert fb.prev_x.shape == sb.prev_x.shape == (1, H + D, H, K)


def test_odeint_entry_and_state_rules(dev):
    """odeint(odefunc, h0, t_grid, method='rk4') takes the fused path too, with FerroelectricBasis's own
    state rules: a stored (B, in) state is the first gate's prev, a state of another shape is
    re-initialised to the first input — the same results as the per-stage path, which applies them
    call by call."""
    import fet_ode_amd as FA
    from fet_ode_amd import ecg
    H, D, K, T = FIX
    B = 3
    x = case_x(H, D, K, T, B).to(dev)
    t_grid = torch.linspace(0.0, 1.0, steps=T).to(dev)
    h0 = lift(H, D, K, x.cpu()).to(dev)
    res = {}
    for name in ("fused", "staged"):
        f = gpu_field(H, D, K, dev)
        f.set_interpolator(ecg.LinearInterp1D(t_grid, x))
        outs = []
        with torch.no_grad():
            prev = ecg.set_fused_driven(name == "fused")
            try:
                f.basis.reset_state()                                   # (1, in) zeros: re-initialised, dx = 0
                outs.append(FA.odeint(f, h0, t_grid, method="rk4"))
                outs.append(FA.odeint(f, h0, t_grid, method="rk4"))     # carries the (B, in) state over
                outs.append(f.basis._prev.clone())
            finally:
                ecg.set_fused_driven(prev)
        res[name] = outs
    assert not torch.equal(res["fused"][0], res["fused"][1])
    for a, b in zip(res["fused"], res["staged"]):
        assert a.shape == b.shape
        r = rows_rel(a, b).max().item()
        assert r <= 1e-5, r


# ---------------------------------------------------------------------------------------------
# 9. gradients
# ---------------------------------------------------------------------------------------------
def nrel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def oracle_grads(sd, x, w, dtype):
    """d (sum_b <traj_b, w_b>) / d (field parameters, h0) by the oracle's autograd, sample by sample."""
    r = R.NodeRnn(sd, dtype)
    ps = r.field.params()
    for p in ps:
        p.requires_grad_(True)
    h0 = F.linear(x[:, 0].to(dtype), r.lift_w, r.lift_b).detach().requires_grad_(True)
    loss = 0.0
    for b in range(x.shape[0]):
        loss = loss + (r.encode(x[b].to(dtype), h0[b:b + 1])[:, 0] * w[:, b].to(dtype)).sum()
    loss.backward()
    return [p.grad for p in ps] + [h0.grad]


def gpu_grads(H, D, K, x, w, dev):
    from fet_ode_amd import ecg
    f = gpu_field(H, D, K, dev)
    T = x.shape[1]
    t_grid = torch.linspace(0.0, 1.0, steps=T).to(dev)
    f.set_interpolator(ecg.LinearInterp1D(t_grid, x.to(dev)))
    f.basis.reset_state()
    f.basis._prev = torch.zeros(x.shape[0], H + D, device=dev)
    h0 = lift(H, D, K, x).to(dev).requires_grad_(True)
    import fet_ode_amd as FA
    traj = FA.odeint(f, h0, t_grid, method="rk4")
    (traj * w.to(dev)).sum().backward()
    return [getattr(f.basis, n).grad for n in R.FERRO] + [f.gain.grad, f.bias.grad, h0.grad]


NAMES = list(R.FERRO) + ["gain", "bias_out", "h0"]


@pytest.mark.parametrize("rows", ["last", "all"])
def test_gradients_fixture_shape(dev, rows):
    """Every parameter tensor of the field and d/dh0 within 2e-4 of the oracle's fp32 autograd (which
    the fixture pins bit for bit), in every samples-per-workgroup variant."""
    H, D, K, T = FIX
    x = torch.from_numpy(load_golden("node_rnn")["x"])
    g = torch.Generator().manual_seed(3)
    w = torch.randn(T, x.shape[0], H, generator=g)
    if rows == "last":
        w[:-1] = 0
    exp = oracle_grads(case_sd(H, D, K), x, w, torch.float32)
    for v in SPW:
        with spw(v):
            got = gpu_grads(H, D, K, x, w, dev)
        for n, a, b in zip(NAMES, got, exp):
            r = nrel(a, b)
            print(f"fixture-shape grad {n} ({rows} rows, spw {v}): {r:.3e}")
            assert r <= 2e-4, (n, v, r)


@pytest.mark.parametrize("rows", ["last", "all"])
def test_gradients_production_width(dev, rows):
    H, D, K, T, B = 64, 1, 10, 12, 4
    sd = case_sd(H, D, K)
    x = case_x(H, D, K, T, B, True)
    g = torch.Generator().manual_seed(4)
    w = torch.randn(T, B, H, generator=g)
    if rows == "last":
        w[:-1] = 0
    e64 = oracle_grads(sd, x, w, torch.float64)
    ctl = [oracle_grads(sd, x, w, torch.float32)] + [oracle_grads(R.rounded(sd, s), x, w, torch.float32)
                                                     for s in (1, 2, 3)]
    with per_stage():
        staged = gpu_grads(H, D, K, x, w, dev)
    for v in SPW:
        with spw(v):
            got = gpu_grads(H, D, K, x, w, dev)
        for i, n in enumerate(NAMES):
            err, st = nrel(got[i], e64[i]), nrel(staged[i], e64[i])
            c = max(nrel(cg[i], e64[i]) for cg in ctl)
            bar = max(1e-4, 2 * st, 2 * c)
            print(f"production grad {n} ({rows} rows, spw {v}): gpu {err:.3e}, per-stage {st:.3e}, "
                  f"worst fp32 control {c:.3e}, bar {bar:.3e}")
            assert err <= bar, (n, v, err, bar)


# ---------------------------------------------------------------------------------------------
# 10. NODE_RNN end to end
# ---------------------------------------------------------------------------------------------
def test_node_rnn_end_to_end(dev):
    from fet_ode_amd import ecg
    g = load_golden("node_rnn")
    sd = golden_sd(g)
    H, D, K, T = FIX
    m = ecg.NODE_RNN(input_size=D, hidden_size=H, num_classes=2, num_basis=K, solver="rk4")
    m.load_state_dict(sd)
    m = m.to(dev)
    x, y = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["y"]).to(dev)
    with torch.no_grad():
        logits = m(x)
    exp = torch.from_numpy(g["logits"])
    r = rows_rel(logits, exp).max().item()
    print(f"NODE_RNN logits rel {r:.3e}")
    assert r <= 1e-5, r
    out = m.state_dict()
    assert list(out) == list(sd)
    for k in ("enc.odefunc.basis.prev_x", "rnn_cell.input_basis.prev_x", "rnn_cell.hidden_basis.prev_x"):
        e = torch.from_numpy(g["end/" + k])
        assert out[k].shape == e.shape, k
        rr = rows_rel(out[k][:, :, 0, 0], e[:, :, 0, 0]).max().item()
        print(f"end state {k}: {rr:.3e}")
        assert rr <= 1e-5 and bool((out[k] == out[k][:, :, :1, :1]).all()), (k, rr)
    for k, v in sd.items():
        assert out[k].shape == v.shape, k
    m2 = ecg.NODE_RNN(input_size=D, hidden_size=H, num_classes=2, num_basis=K).to(dev)
    m2.load_state_dict(out)                                    # the reference-shaped keys round-trip
    for k, v in m2.state_dict().items():
        assert torch.equal(v, out[k]), k
    # gradients of the cross-entropy loss against the fixture, then one step of the training recipe
    # (train_rnn_node: AdamW lr 1e-3, weight decay 1e-4, clip_grad_norm_ 1.0)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt.zero_grad()
    loss = F.cross_entropy(m(x), y)
    loss.backward()
    for n, p in m.named_parameters():
        e = torch.from_numpy(g["grad/" + n])
        assert p.grad is not None, n
        if not e.any():
            assert not p.grad.any(), n
        else:
            rr = nrel(p.grad, e)
            assert rr <= 2e-4, (n, rr)
    torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt.step()
    for n, p in m.named_parameters():
        assert not torch.equal(p.detach(), before[n]), n
    # a second forward sees the parameters updated in place (the plan cache follows them)
    with torch.no_grad():
        l2 = m(x)
        sd2 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        e2, _ = R.NodeRnn(sd2)(x.cpu())
    assert not torch.equal(l2, logits)
    r2 = rows_rel(l2, e2).max().item()
    print(f"after one step: logits rel {r2:.3e}")
    assert r2 <= 1e-5, r2
