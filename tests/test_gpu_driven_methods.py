"""The one-launch driven solve under euler, midpoint, rk4_classic and the step_size option
on the GPU: the new C entries against the old ones (rk4, bitwise), against themselves (tape, split
launches, row independence, samples per workgroup, the sweep with and without d/dx(t): bitwise), against
the CPU oracle of tests/driven_methods_ref.py (trajectory, end state, every evaluation's taped input and
pre-activation, gradients) and against the per-stage path; the routing behind set_fused_driven_methods;
one NODE_RNN(solver="midpoint") training step.

Bars: tests/test_gpu_driven.py's own.  Trajectories 1e-5 per slice where the oracle's fp32 - fp64 distance
is below 1e-6, elsewhere its envelope (4 x the worst fp32 control + 1e-5 of scale); gradients normwise per
tensor against fp64, max(1e-4, 2 x the per-stage path's error, 2 x the worst fp32 control)."""
import ctypes
import functools
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

import driven_methods_ref as M
import node_rnn_ref as R
import test_gpu_driven as G
from conftest import golden_sd, load_golden

pytestmark = pytest.mark.gpu
SPW = G.SPW
SHAPES = [(8, 1, 3, 2), (8, 2, 3, 5), (24, 3, 12, 5), (64, 1, 10, 4), (64, 4, 16, 3)]
SID = lambda s: "H%d-D%d-K%d-T%d" % s   # noqa: E731
STEP_CASES = [0.0625, 0.05, 0.3]        # divides the knot spacing; does not (mode 2); wider than it (knots skipped)


@contextmanager
def methods_knob(on=True):
    from fet_ode_amd import ecg
    prev = ecg.set_fused_driven_methods(on)
    try:
        yield
    finally:
        ecg.set_fused_driven_methods(prev)


@contextmanager
def knobs(param_grads=False, series=False):
    from fet_ode_amd import ecg
    a, b = ecg.set_fused_driven_param_grads(param_grads), ecg.set_driven_series_grad(series)
    try:
        yield
    finally:
        ecg.set_fused_driven_param_grads(a)
        ecg.set_driven_series_grad(b)


@functools.lru_cache(maxsize=None)
def oracle(H, D, K, T, B, method, step_size=None):
    return M.Oracle(G.case_sd(H, D, K), G.case_x(H, D, K, T, B), method, step_size)


class RawGrid:
    """The four new C entries driven directly: one field, one batch of driving series, one method."""

    def __init__(self, H, D, K, T, x, dev, method, step_size=None):
        from fet_ode_amd import _lib, ecg
        from fet_ode_amd.odeint import FIXED_METHODS, get_schedule
        self.L, self.lib = _lib, _lib.load()
        self.f = G.gpu_field(H, D, K, dev)
        self.plan, self.d, self.keep = ecg._driven_plan(self.f, dev)
        self.code, self.nm = FIXED_METHODS[method], M.N_M[method]
        tc = torch.linspace(0.0, 1.0, steps=T)
        self.sched = get_schedule(tc, step_size, False)
        self.tq, self.coef, self.sel = ecg._driven_grid_arrays(self.sched, self.code, dev)
        self.tg = tc.to(dev)
        self.x = x.to(dev).contiguous()
        self.u = ecg.driven_table(self.tg, self.x, self.tq)
        self.H, self.D, self.In, self.n, self.dev = H, D, H + D, self.sched.n_steps, dev
        assert self.tq.numel() == self.nm * self.n and self.coef.numel() == 4 * self.n

    def solve(self, h0, prev0=None, step0=0, n_steps=None, tape=False):
        n_steps = self.n - step0 if n_steps is None else n_steps
        B = h0.shape[0]
        h0 = h0.to(self.dev).contiguous()
        prev0 = None if prev0 is None else prev0.to(self.dev).contiguous()
        sol = torch.full((n_steps, B, self.H), float("nan"), device=self.dev)
        pout = torch.full((B, self.In), float("nan"), device=self.dev)
        coef = self.coef[4 * step0:]
        args = [ctypes.byref(self.d), self.plan.data_ptr(), self.code, h0.data_ptr(), B, self.u.data_ptr(),
                self.u.shape[0], self.nm * step0, coef.data_ptr(), n_steps, self.L.ptr(prev0), sol.data_ptr(),
                pout.data_ptr()]
        if tape:
            thx = torch.full((self.u.shape[0], B, self.In), float("nan"), device=self.dev)
            tphi = torch.full((self.u.shape[0], B, self.H), float("nan"), device=self.dev)
            self.L.check(self.lib.fetode_driven_grid_tape(*args, thx.data_ptr(), tphi.data_ptr(), None), "grid tape")
            return sol, pout, thx, tphi
        self.L.check(self.lib.fetode_driven_grid(*args, None), "grid")
        return sol, pout

    def sweep(self, prev0, thx, tphi, grad_sol, xg, old=False):
        """adj, grad_h0 (and adj_u) of a full taped solve; old: through fetode_driven_fixed_backward(_x) (rk4)."""
        ne, B = thx.shape[0], thx.shape[1]
        adj = torch.full((ne, B, self.H), float("nan"), device=self.dev)
        gh0 = torch.full((B, self.H), float("nan"), device=self.dev)
        coef = self.coef.view(-1, 4)[:, 0].contiguous() if old else self.coef
        args = [ctypes.byref(self.d), self.plan.data_ptr(), self.code, B, coef.data_ptr(), self.n, self.L.ptr(prev0),
                thx.data_ptr(), tphi.data_ptr(), grad_sol.data_ptr(), adj.data_ptr(), gh0.data_ptr()]
        name = "fetode_driven_%s_backward%s" % ("fixed" if old else "grid", "_x" if xg else "")
        if xg:
            adj_u = torch.full((ne, B, self.D), float("nan"), device=self.dev)
            self.L.check(getattr(self.lib, name)(*args, adj_u.data_ptr(), None), name)
            return adj, gh0, adj_u
        self.L.check(getattr(self.lib, name)(*args, None), name)
        return adj, gh0


def grad_sol(n, B, H, dev, seed=0):
    g = torch.Generator().manual_seed(seed + n + 7 * B + H)
    return torch.randn(n + 1, B, H, generator=g).to(dev)


# ---------------------------------------------------------------------------------------------
# 1. method = rk4: the new entries are the old ones, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_rk4_new_entries_equal_old_bitwise(dev, shape):
    H, D, K, T = shape
    for B in (1, 3, 5):
        x = G.case_x(H, D, K, T, 5)[:B]
        h0 = G.lift(H, D, K, x)
        old, new = G.Raw(H, D, K, T, x, dev), RawGrid(H, D, K, T, x, dev, "rk4")
        assert torch.equal(old.tq, new.tq) and torch.equal(old.dt, new.coef.view(-1, 4)[:, 0])
        gs = grad_sol(T - 1, B, H, dev)
        for v in SPW:
            with G.spw(v):
                a, b = old.solve(h0, tape=True), new.solve(h0, tape=True)
                for i, what in enumerate(("sol", "prev_out", "tape_hx", "tape_phi")):
                    assert torch.isfinite(b[i]).all() and torch.equal(a[i], b[i]), (B, v, what)
                assert all(torch.equal(p, q) for p, q in zip(old.solve(h0), new.solve(h0))), (B, v)
                p0 = torch.zeros(B, H + D, device=dev)
                sa, sb = new.sweep(p0, a[2], a[3], gs, True, old=True), new.sweep(p0, b[2], b[3], gs, True)
                for i, what in enumerate(("adj", "grad_h0", "adj_u")):
                    assert torch.isfinite(sb[i]).all() and torch.equal(sa[i], sb[i]), (B, v, what)
                sa, sb = new.sweep(p0, a[2], a[3], gs, False, old=True), new.sweep(p0, b[2], b[3], gs, False)
                assert torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1]), (B, v)


# ---------------------------------------------------------------------------------------------
# 2. per method: the launches against themselves, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", M.METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_self_consistency_bitwise(dev, shape, method):
    H, D, K, T = shape
    x = G.case_x(H, D, K, T, 5)
    h0 = G.lift(H, D, K, x)
    ref = None
    for v in SPW:
        with G.spw(v):
            raw = RawGrid(H, D, K, T, x, dev, method)
            full, pfull, thx, tphi = raw.solve(h0, tape=True)
            assert all(torch.isfinite(t).all() for t in (full, pfull, thx, tphi)), v
            # taped == untaped; the last taped input is prev_out
            u_full, u_p = raw.solve(h0)
            assert torch.equal(u_full, full) and torch.equal(u_p, pfull) and torch.equal(thx[-1], pfull), v
            # a solve cut in two at eval0 == one launch
            for cut in sorted({1, (T - 1) // 2, T - 2} - {0, T - 1}):
                a, pa = raw.solve(h0, n_steps=cut)
                b, pb = raw.solve(a[-1], pa, step0=cut)
                assert torch.equal(torch.cat([a, b]), full) and torch.equal(pb, pfull), (v, cut)
            # a row alone == the row in the batch (B = 5 and 3: the last workgroup is partly empty)
            for b in range(5):
                one, pone = RawGrid(H, D, K, T, x[b:b + 1], dev, method).solve(h0[b:b + 1])
                assert torch.equal(one[:, 0], full[:, b]) and torch.equal(pone[0], pfull[b]), (v, b)
            three = RawGrid(H, D, K, T, x[:3], dev, method).solve(h0[:3])
            assert torch.equal(three[0], full[:, :3]) and torch.equal(three[1], pfull[:3]), v
            # the sweep: adj and grad_h0 are the same bits with and without d/dx(t)
            gs = grad_sol(T - 1, 5, H, dev)
            p0 = torch.zeros(5, H + D, device=dev)
            adj, gh0, adj_u = raw.sweep(p0, thx, tphi, gs, True)
            adj2, gh02 = raw.sweep(p0, thx, tphi, gs, False)
            assert all(torch.isfinite(t).all() for t in (adj, gh0, adj_u)), v
            assert torch.equal(adj, adj2) and torch.equal(gh0, gh02), v
            out = (full, pfull, thx, tphi, adj, gh0, adj_u)
        # samples per workgroup 1 == 2 == 4
        ref = out if ref is None else ref
        assert all(torch.equal(a, b) for a, b in zip(out, ref)), v


# ---------------------------------------------------------------------------------------------
# 3. per method and shape against the oracle: trajectory, end state, every evaluation's tape
# ---------------------------------------------------------------------------------------------
def check_calls(got_hx, got_phi, orc, b, what):
    """Every evaluation's taped input and pre-activation of sample b against the oracle's recorded calls, in
    call order: 1e-5 per row where the oracle's fp32 - fp64 distance is below 1e-6, the envelope elsewhere."""
    for i, (got, name) in enumerate(((got_hx, "hx"), (got_phi, "phi"))):
        c32, c64 = orc["calls32"][b][i], orc["calls64"][b][i]
        assert got.shape == c32.shape, (what, name, got.shape, c32.shape)
        own, rel = G.rows_rel(c32, c64), G.rows_rel(got, c32)
        well = own < 1e-6
        worst = rel[well].max().item() if well.any() else 0.0
        print(f"{what} {name}: {int(well.sum())}/{len(well)} well-conditioned evaluations, worst rel {worst:.3e}")
        assert worst <= 1e-5, (what, name, worst)
        if not well.all():
            ill = ~well
            G.envelope(got[ill.to(got.device)], [c32[ill]] + [c[i][ill] for c in orc["ctl_calls"][b]], c64[ill],
                       f"{what} {name} (ill-conditioned evaluations)")


@pytest.mark.parametrize("method", M.METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_solve_and_tape_vs_oracle(dev, shape, method):
    H, D, K, T = shape
    B = 3
    orc = oracle(H, D, K, T, B, method)
    x = G.case_x(H, D, K, T, B)
    raw = RawGrid(H, D, K, T, x, dev, method)
    h0 = G.lift(H, D, K, x)
    sol, pout, thx, tphi = raw.solve(h0, tape=True)
    traj = torch.cat([h0.to(dev).unsqueeze(0), sol])
    assert traj.shape == (T, B, H) and thx.shape[0] == M.N_M[method] * (T - 1)
    for b in range(B):
        G.check_traj(traj[:, b], orc, b, f"{method} sample {b}")
        G.check_end(pout[b:b + 1], orc, b, f"{method} sample {b}")
        check_calls(thx[:, b], tphi[:, b], orc, b, f"{method} sample {b}")


# ---------------------------------------------------------------------------------------------
# 4. step_size through odeint, 5. fused against per-stage
# ---------------------------------------------------------------------------------------------
def odeint_run(H, D, K, T, B, dev, method, step_size=None):
    import fet_ode_amd as FA
    from fet_ode_amd import ecg
    x = G.case_x(H, D, K, T, B)
    f = G.gpu_field(H, D, K, dev)
    t_grid = torch.linspace(0.0, 1.0, steps=T).to(dev)
    f.set_interpolator(ecg.LinearInterp1D(t_grid, x.to(dev)))
    f.basis.reset_state()
    f.basis._prev = torch.zeros(B, H + D, device=dev)
    with torch.no_grad():
        traj = FA.odeint(f, G.lift(H, D, K, x).to(dev), t_grid, method=method, options=M.options(step_size))
    return traj, f.basis._prev


@pytest.mark.parametrize("method", ["rk4", "euler"])
@pytest.mark.parametrize("step_size", STEP_CASES)
@pytest.mark.parametrize("shape", [(8, 1, 3, 9), (64, 1, 10, 9)], ids=SID)
def test_step_size_vs_oracle(dev, shape, step_size, method):
    H, D, K, T = shape
    B = 3
    orc = oracle(H, D, K, T, B, method, step_size)
    with methods_knob():
        traj, prev = odeint_run(H, D, K, T, B, dev, method, step_size)
    assert traj.shape == (T, B, H) and prev.shape == (B, H + D)
    for b in range(B):
        G.check_traj(traj[:, b], orc, b, f"{method} step_size {step_size} sample {b}")
        G.check_end(prev[b:b + 1], orc, b, f"{method} step_size {step_size} sample {b}")


@pytest.mark.parametrize("method,step_size", [("euler", None), ("midpoint", None), ("rk4_classic", None),
                                              ("rk4", 0.05)])
@pytest.mark.parametrize("shape", [(8, 1, 3, 9), (64, 1, 10, 6)], ids=SID)
def test_fused_vs_per_stage(dev, shape, method, step_size):
    H, D, K, T = shape
    B = 3
    orc = oracle(H, D, K, T, B, method, step_size)
    with methods_knob(True):
        fused, fp = odeint_run(H, D, K, T, B, dev, method, step_size)
    with methods_knob(False):
        staged, sp = odeint_run(H, D, K, T, B, dev, method, step_size)
    assert not torch.equal(fused, staged)    # two different programs (guards a silent fall-back)
    for b in range(B):
        G.check_traj(fused[:, b], orc, b, f"fused sample {b}")
        G.check_traj(staged[:, b], orc, b, f"per-stage sample {b}")
        well = (G.rows_rel(orc["traj32"][b][:, 0], orc["traj64"][b][:, 0]) < 1e-6).to(dev)
        if well.any():
            r = G.rows_rel(fused[:, b][well], staged[:, b][well]).max().item()
            print(f"fused vs per-stage sample {b}: {r:.3e}")
            assert r <= 1e-5, (b, r)
        G.check_end(fp[b:b + 1], orc, b, "fused")
        G.check_end(sp[b:b + 1], orc, b, "per-stage")


# ---------------------------------------------------------------------------------------------
# 6. gradients
# ---------------------------------------------------------------------------------------------
NAMES = list(R.FERRO) + ["gain", "bias_out", "h0", "x"]


def gpu_grads(H, D, K, x, w, dev, method, step_size):
    import fet_ode_amd as FA
    from fet_ode_amd import ecg
    f = G.gpu_field(H, D, K, dev)
    T = x.shape[1]
    t_grid = torch.linspace(0.0, 1.0, steps=T).to(dev)
    xg = x.to(dev).requires_grad_(True)
    f.set_interpolator(ecg.LinearInterp1D(t_grid, xg))
    f.basis.reset_state()
    f.basis._prev = torch.zeros(x.shape[0], H + D, device=dev)
    h0 = G.lift(H, D, K, x).to(dev).requires_grad_(True)
    traj = FA.odeint(f, h0, t_grid, method=method, options=M.options(step_size))
    (traj * w.to(dev)).sum().backward()
    return [getattr(f.basis, n).grad for n in R.FERRO] + [f.gain.grad, f.bias.grad, h0.grad, xg.grad]


@pytest.mark.parametrize("rows", ["last", "all"])
@pytest.mark.parametrize("method,step_size", [("euler", None), ("midpoint", None), ("rk4_classic", None), ("rk4", 0.05),
                                              ("midpoint", 0.05)])
@pytest.mark.parametrize("shape,B", [((8, 1, 3, 9), 3), ((64, 1, 10, 6), 2)], ids=["H8-B3", "H64-B2"])
def test_gradients(dev, shape, B, method, step_size, rows):
    H, D, K, T = shape
    sd = G.case_sd(H, D, K)
    x = G.case_x(H, D, K, T, B)
    g = torch.Generator().manual_seed(4 + T)
    w = torch.randn(T, B, H, generator=g)
    if rows == "last":
        w[:-1] = 0
    e64 = M.grads(sd, x, w, method, step_size, torch.float64)
    ctl = [M.grads(sd, x, w, method, step_size)] + [M.grads(R.rounded(sd, s), x, w, method, step_size)
                                                    for s in (1, 2, 3)]
    with methods_knob(False):
        staged = gpu_grads(H, D, K, x, w, dev, method, step_size)      # the per-stage path (x through autograd)
    for pg in (False, True):
        with methods_knob(True), knobs(param_grads=pg, series=True):
            got = gpu_grads(H, D, K, x, w, dev, method, step_size)
        for i, n in enumerate(NAMES):
            err, st = G.nrel(got[i], e64[i]), G.nrel(staged[i], e64[i])
            c = max(G.nrel(cg[i], e64[i]) for cg in ctl)
            bar = max(1e-4, 2 * st, 2 * c)
            print(f"{method} step_size {step_size} grad {n} ({rows} rows, fused sums {pg}): gpu {err:.3e}, "
                  f"per-stage {st:.3e}, worst fp32 control {c:.3e}, bar {bar:.3e}")
            assert err <= bar, (n, pg, err, bar)


# ---------------------------------------------------------------------------------------------
# 7. routing
# ---------------------------------------------------------------------------------------------
class Counting:
    """The library with the calls of the grid entries counted."""

    def __init__(self, lib):
        self.lib, self.names = lib, []

    def __getattr__(self, name):
        if name.startswith("fetode_driven_grid"):
            self.names.append(name)
        return getattr(self.lib, name)


def test_routing(dev, monkeypatch):
    import fet_ode_amd as FA
    from fet_ode_amd import _lib, ecg
    cnt = Counting(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: cnt)
    g = load_golden("node_rnn")
    H, D, K, T = G.FIX
    x = torch.from_numpy(g["x"]).to(dev)
    t_grid = torch.linspace(0.0, 1.0, steps=T).to(dev)

    def model(solver="euler"):
        m = ecg.NODE_RNN(input_size=D, hidden_size=H, num_classes=2, num_basis=K, solver=solver)
        m.load_state_dict(golden_sd(g))
        return m.to(dev)

    def field_solve(xs, grad, **kw):
        f = G.gpu_field(H, D, K, dev)
        f.set_interpolator(ecg.LinearInterp1D(t_grid, xs))
        f.basis._prev = torch.zeros(xs.shape[0], H + D, device=dev)
        h0 = G.lift(H, D, K, xs.detach().cpu()).to(dev)
        with torch.enable_grad() if grad else torch.no_grad():
            out = FA.odeint(f, h0, t_grid, **kw)
            if grad:
                out.sum().backward()
                assert f.gain.grad is not None and torch.isfinite(f.gain.grad).all()
        return out.detach()

    res = {}
    for on in (False, True):
        with methods_knob(on):
            cnt.names.clear()
            with torch.no_grad():
                res[on, "model"] = model()(x)
            assert cnt.names == (["fetode_driven_grid"] if on else []), (on, cnt.names)
            cnt.names.clear()
            model()(x).sum().backward()
            assert cnt.names == (["fetode_driven_grid_tape", "fetode_driven_grid_backward"] if on else []), cnt.names
            cnt.names.clear()
            res[on, "step"] = field_solve(x, False, method="rk4", options={"step_size": 0.05})
            assert cnt.names == (["fetode_driven_grid"] if on else []), (on, cnt.names)
            cnt.names.clear()
            field_solve(x, True, method="rk4", options={"step_size": 0.05})
            assert cnt.names == (["fetode_driven_grid_tape", "fetode_driven_grid_backward"] if on else []), cnt.names
            # plain rk4 is the old path's, knob or not
            cnt.names.clear()
            field_solve(x, False, method="rk4")
            assert cnt.names == []
            # a series that requires grad: per stage unless the series-grad knob is on
            xg = x.clone().requires_grad_(True)
            cnt.names.clear()
            with knobs(series=False):
                field_solve(xg, True, method="euler")
            assert cnt.names == [] and xg.grad is not None
            cnt.names.clear()
            with knobs(series=True):
                field_solve(xg, True, method="euler")
            assert cnt.names == (["fetode_driven_grid_tape", "fetode_driven_grid_backward_x"] if on else []), cnt.names
    # knob off is the per-stage path: the same program as with the one-launch solves switched off altogether
    with G.per_stage(), torch.no_grad():
        assert torch.equal(model()(x), res[False, "model"])
        assert torch.equal(field_solve(x, False, method="rk4", options={"step_size": 0.05}), res[False, "step"])
    for k in ("model", "step"):
        assert not torch.equal(res[True, k], res[False, k])
        print(f"routing {k}: fused vs per-stage {G.rows_rel(res[True, k], res[False, k]).max().item():.3e}")


# ---------------------------------------------------------------------------------------------
# 8. one NODE_RNN(solver="midpoint") training step
# ---------------------------------------------------------------------------------------------
def oracle_step_grads(sd, x, y, dtype):
    r = M.NodeRnn(sd, dtype, "midpoint").requires_grad_()
    logits, _ = r(x.to(dtype))
    F.cross_entropy(logits, y).backward()
    return logits.detach(), {n: (p.grad if p.grad is not None else torch.zeros_like(p))
                             for n, p in r.named_params().items()}


def test_node_rnn_midpoint_training_step(dev):
    """train_rnn_node's recipe (AdamW lr 1e-3, weight decay 1e-4, clip_grad_norm_ 1.0), as
    test_node_rnn_end_to_end runs it, with solver="midpoint" on the one-launch path: logits and gradients
    against the fp64 oracle's step, then the logits after the update against the oracle on the updated
    parameters."""
    from fet_ode_amd import ecg
    g = load_golden("node_rnn")
    sd = golden_sd(g)
    H, D, K, T = G.FIX
    xc, yc = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    x, y = xc.to(dev), yc.to(dev)
    l64, g64 = oracle_step_grads(sd, xc, yc, torch.float64)
    ctl = [oracle_step_grads(sd, xc, yc, torch.float32)] + [oracle_step_grads(R.rounded(sd, s), xc, yc, torch.float32)
                                                            for s in (1, 2, 3)]
    with methods_knob():
        m = ecg.NODE_RNN(input_size=D, hidden_size=H, num_classes=2, num_basis=K, solver="midpoint")
        m.load_state_dict(sd)
        m = m.to(dev)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        opt.zero_grad()
        logits = m(x)
        F.cross_entropy(logits, y).backward()
        G.envelope(logits, [c[0] for c in ctl], l64, "midpoint logits")
        for n, p in m.named_parameters():
            e = g64[n]
            assert p.grad is not None, n
            if not e.any():
                assert not p.grad.any(), n
                continue
            err = G.nrel(p.grad, e)
            c = max(G.nrel(cg[1][n], e) for cg in ctl)
            bar = max(1e-4, 2 * c)
            print(f"midpoint step grad {n}: gpu {err:.3e}, worst fp32 control {c:.3e}, bar {bar:.3e}")
            assert err <= bar, (n, err, bar)
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        for n, p in m.named_parameters():
            assert not torch.equal(p.detach(), before[n]), n
        with torch.no_grad():
            l2 = m(x)
    sd2 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        e64, _ = M.NodeRnn(sd2, torch.float64, "midpoint")(xc.double())
        c2 = [M.NodeRnn(s, torch.float32, "midpoint")(xc)[0] for s in [sd2] + [R.rounded(sd2, q) for q in (1, 2, 3)]]
    assert not torch.equal(l2, logits)
    G.envelope(l2, c2, e64, "midpoint logits after one step")
