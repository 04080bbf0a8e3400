"""The gradient to the driving series in the one-launch rk4 solve of the ECG NODE-RNN encoder (DESIGN
§4.21): LinearInterp1D's backward (fetode_driven_table_backward), the sweep that also forms d loss /
d x(t) (fetode_driven_fixed_backward_x) beside the one that does not (bitwise), d loss / d x with h0
detached against tests/driven_xgrad_ref.py, and the routing under ecg.set_driven_series_grad.

Bars.  Table backward: one-hot rows bitwise the host's fp32 (1 - w, w); random rows within the fp32
summation bound (n + 2) 2^-23 sum |contributions| per knot against the fp64 expression, n that knot's
contribution count — on grids with power-of-two spacing, where the fp32 weight w is exact, so that the
bound is the summation's own.  Gradients: the rule of tests/test_gpu_driven.py, normwise
max(1e-4, 2 x the per-stage path's error, 2 x the worst of four fp32 controls) against the fp64 oracle."""
import ctypes
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

import driven_xgrad_ref as XR
import node_rnn_ref as R
import test_gpu_driven as TD
from conftest import golden_sd, load_golden

pytestmark = pytest.mark.gpu
SPW = (1, 2, 4)
SWEEP = [(8, 1, 3, 9, 3), (5, 2, 4, 6, 3), (64, 4, 16, 5, 2)]
GRADS = SWEEP + [(3, 1, 2, 2, 2), (1, 1, 1, 3, 2), (64, 1, 10, 12, 4)]
ids = lambda s: "H%d-D%d-K%d-T%d-B%d" % s   # noqa: E731


@contextmanager
def xgrad(on):
    from fet_ode_amd import ecg
    prev = ecg.set_driven_series_grad(on)
    try:
        yield
    finally:
        ecg.set_driven_series_grad(prev)


# ---------------------------------------------------------------------------------------------
# 1. LinearInterp1D's backward
# ---------------------------------------------------------------------------------------------
def layouts(tq, adj_u, dev):
    """The rows adj_u (B, n, D) at the times tq (B, n) in the dopri5 layout and, where the samples share
    their times, in the rk4 layout too: [(name, args of ecg.driven_series_grad after t_grid)]."""
    B, n, D = adj_u.shape
    out = [("dopri5", (tq.to(dev).contiguous(), n, adj_u.to(dev).contiguous(), B, n, n, 1))]
    if bool((tq == tq[:1]).all()):
        out.append(("rk4", (tq[0].to(dev).contiguous(), 0, adj_u.permute(1, 0, 2).to(dev).contiguous(), B, n, 1, B)))
    return out


def series_grad(t_grid, lay, D, dev, nfev=None):
    from fet_ode_amd import ecg
    tq, tq_sb, au, B, n, sb, se = lay
    return ecg.driven_series_grad(tq, tq_sb, t_grid.to(dev), au, B, n, sb, se, nfev, 0 if nfev is None else 3, D)


@pytest.mark.parametrize("D", [1, 4])
@pytest.mark.parametrize("T", [2, 9])
def test_table_backward_one_hot_bitwise(dev, T, D):
    t_grid = torch.linspace(0.0, 1.0, steps=T)
    # on a knot, inside an interval, t[0], t[-1], outside the grid on both sides
    tq = torch.tensor([t_grid[T // 2].item(), 0.3123, t_grid[0].item(), t_grid[-1].item(), -0.5, 1.5, 0.999999])
    i, w = XR.knot_weights(t_grid, tq)
    n, B = len(tq), 2
    for e in range(n):
        au = torch.zeros(B, n, D)
        au[1, e] = 1.0
        for name, lay in layouts(tq.expand(B, n), au, dev):
            got = series_grad(t_grid, lay, D, dev).cpu()
            exp = torch.zeros(B, T, D)
            exp[1, i[e] - 1], exp[1, i[e]] = 1.0 - w[e], w[e]
            assert got.shape == exp.shape and torch.equal(got, exp), (name, e, got[1, :, 0], exp[1, :, 0])
            assert int((got != 0).sum()) <= 2 * D
    assert i[4] == 1 and w[4] == 0 and i[5] == T - 1 and w[5] == 1      # the clamped queries


@pytest.mark.parametrize("T,D,n", [(9, 4, 40), (5, 1, 300), (2, 2, 7)])
def test_table_backward_random_rows(dev, T, D, n):
    """Random rows against the fp64 expression within the fp32 summation bound per knot; both layouts
    and two runs give the same bits; rows at or beyond nfev are never read."""
    g = torch.Generator().manual_seed(T + 10 * D)
    B = 3
    t_grid = torch.linspace(0.0, 1.0, steps=T)                  # spacing 1/8, 1/4, 1: w is exact in fp32
    tq = (torch.rand(n, generator=g) * 1.4 - 0.2).expand(B, n)
    au = torch.randn(B, n, D, generator=g)
    exp, cnt, mag = XR.table_backward(t_grid, tq, au, [n] * B)
    got = {}
    for name, lay in layouts(tq, au, dev):
        got[name] = series_grad(t_grid, lay, D, dev)
        assert torch.equal(series_grad(t_grid, lay, D, dev), got[name]), name
        err = (got[name].double().cpu() - exp).abs()
        bound = (cnt + 2) * 2.0 ** -23 * mag
        print(f"table backward T={T} D={D} n={n} {name}: worst err / bound {(err / bound.clamp_min(1e-300)).max():.3f}, "
              f"most contributions {int(cnt.max())}")
        assert bool((err <= bound).all()), (name, (err - bound).max().item())
        assert not got[name][(cnt == 0).to(dev)].any()          # a knot nothing touches gets 0
    assert torch.equal(got["rk4"], got["dopri5"])
    assert n < 256 or int(cnt.max()) > 16                       # more than one chunk of evaluations, long sums
    # ragged: per-sample times, rows at or beyond nfev filled with NaN change nothing
    live = [n, n // 3, 0]
    tq2 = (torch.rand(B, n, generator=g) * 1.4 - 0.2)
    exp2, cnt2, mag2 = XR.table_backward(t_grid, tq2, au, live)
    stats = torch.tensor([[v, 0, 0] for v in live], dtype=torch.int32, device=dev)
    name, lay = layouts(tq2, au, dev)[0]
    ref = series_grad(t_grid, lay, D, dev, stats)
    tqn, aun = tq2.clone(), au.clone()
    for b in range(B):
        tqn[b, live[b]:] = float("nan")
        aun[b, live[b]:] = float("nan")
    nan = series_grad(t_grid, layouts(tqn, aun, dev)[0][1], D, dev, stats)
    assert torch.equal(nan, ref) and not ref[2].any() and torch.isfinite(ref).all()
    assert bool(((ref.double().cpu() - exp2).abs() <= (cnt2 + 2) * 2.0 ** -23 * mag2).all())
    big = torch.tensor([[n + 50, 0, 0]] * B, dtype=torch.int32, device=dev)    # nfev is clamped to n_ev
    assert torch.equal(series_grad(t_grid, layouts(tq, au, dev)[0][1], D, dev, big), got["dopri5"])


def test_table_backward_empty_batch_is_a_no_op(dev):
    from fet_ode_amd import _lib
    t_grid = torch.linspace(0.0, 1.0, steps=5).to(dev)
    gx = torch.full((2, 5, 1), 7.0, device=dev)
    z = torch.zeros(8, device=dev)
    for B, n in ((0, 4), (2, 0)):
        rc = _lib.load().fetode_driven_table_backward(z.data_ptr(), 0, t_grid.data_ptr(), 5, z.data_ptr(), B, n, 1, 2,
                                                      None, 0, 1, gx.data_ptr(), None, None)
        assert rc == _lib.FETODE_OK and bool((gx == 7.0).all())


# ---------------------------------------------------------------------------------------------
# 2. the sweep with adj_u beside the sweep without
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SWEEP, ids=ids)
def test_sweep_bitwise_the_plain_sweep(dev, shape):
    """adj and grad_h0 of fetode_driven_fixed_backward_x are the bits of fetode_driven_fixed_backward in
    every samples-per-workgroup variant (B = 3 leaves the last workgroup of spw 2 and 4 partly empty;
    (5, 2, ..) puts inputs 5 and 6 on waves 1 and 2, (64, 4, ..) inputs 64..67 on all four waves);
    adj_u is the same in every variant."""
    H, D, K, T, B = shape
    x = TD.case_x(H, D, K, T, B)
    raw = TD.Raw(H, D, K, T, x, dev)
    gsol = torch.randn(T, B, H, generator=torch.Generator().manual_seed(9)).to(dev)
    ref_u = None
    for v in SPW:
        with TD.spw(v):
            _, _, thx, tphi = raw.solve(TD.lift(H, D, K, x), tape=True)
            outs = []
            for with_u in (False, True):
                adj = torch.full_like(tphi, float("nan"))
                gh0 = torch.full((B, H), float("nan"), device=dev)
                adj_u = torch.full((thx.shape[0], B, D), float("nan"), device=dev)
                args = [ctypes.byref(raw.d), raw.plan.data_ptr(), raw.L.RK4, B, raw.dt.data_ptr(), T - 1, None,
                        thx.data_ptr(), tphi.data_ptr(), gsol.data_ptr(), adj.data_ptr(), gh0.data_ptr()]
                if with_u:
                    raw.L.check(raw.lib.fetode_driven_fixed_backward_x(*args, adj_u.data_ptr(), None), "x")
                else:
                    raw.L.check(raw.lib.fetode_driven_fixed_backward(*args, None), "plain")
                outs.append((adj, gh0, adj_u))
        (a0, g0, _), (a1, g1, u1) = outs
        assert torch.isfinite(a0).all() and torch.equal(a0, a1) and torch.equal(g0, g1), v
        assert torch.isfinite(u1).all() and u1.any(), v
        ref_u = u1 if ref_u is None else ref_u
        assert torch.equal(u1, ref_u), v


# ---------------------------------------------------------------------------------------------
# 3. d loss / d x with h0 detached
# ---------------------------------------------------------------------------------------------
def case_series(shape):
    H, D, K, T, B = shape
    if shape == (8, 1, 3, 9, 3):
        return torch.from_numpy(load_golden("node_rnn")["x"])
    return TD.case_x(H, D, K, T, B, (H, D) == (64, 1))


def weights(shape, rows):
    H, D, K, T, B = shape
    w = torch.randn(T, B, H, generator=torch.Generator().manual_seed(3 + H))
    if rows == "last":
        w[:-1] = 0
    return w


def gpu_run(shape, x, w, dev, h0=None, series_grad=True, param_grad=True, h0_grad=False):
    """FA.odeint(method="rk4") of the field from the reset state with loss = sum(traj * w): the series'
    gradient, the parameters' and h0's, and the name of the trajectory's grad_fn."""
    import fet_ode_amd as FA
    from fet_ode_amd import ecg
    H, D, K, T, B = shape
    f = TD.gpu_field(H, D, K, dev)
    for p in f.parameters():
        p.requires_grad_(param_grad)
    t_grid = torch.linspace(0.0, 1.0, steps=T).to(dev)
    xg = x.to(dev).requires_grad_(series_grad)
    f.set_interpolator(ecg.LinearInterp1D(t_grid, xg))
    f.basis.reset_state()
    f.basis._prev = torch.zeros(B, H + D, device=dev)
    h0 = (TD.lift(H, D, K, x) if h0 is None else h0).to(dev).requires_grad_(h0_grad)
    traj = FA.odeint(f, h0, t_grid, method="rk4")
    (traj * w.to(dev)).sum().backward()
    ps = [getattr(f.basis, n).grad for n in R.FERRO] + [f.gain.grad, f.bias.grad]
    return xg.grad, ps, h0.grad, type(traj.grad_fn).__name__


FUSED = "_DrivenFnBackward"


@pytest.mark.parametrize("rows", ["last", "all"])
@pytest.mark.parametrize("shape", GRADS, ids=ids)
def test_series_gradient_vs_oracle(dev, shape, rows):
    H, D, K, T, B = shape
    sd, x, w = TD.case_sd(H, D, K), case_series(shape), weights(shape, rows)
    e64, ctl = XR.rk4_set(sd, x, w)
    with xgrad(False), TD.per_stage():
        staged, _, _, via = gpu_run(shape, x, w, dev)
    assert via != FUSED
    st, c = TD.nrel(staged, e64), max(TD.nrel(g, e64) for g in ctl)
    bar = max(1e-4, 2 * st, 2 * c)
    for v in SPW:
        with xgrad(True), TD.spw(v):
            got, _, _, via = gpu_run(shape, x, w, dev)
        assert via == FUSED and got.shape == x.shape
        err = TD.nrel(got, e64)
        print(f"d/dx {ids(shape)} ({rows} rows, spw {v}): gpu {err:.3e}, per-stage {st:.3e}, "
              f"worst fp32 control {c:.3e}, bar {bar:.3e}")
        assert err <= bar, (v, err, bar)


def test_node_rnn_series_gradient_through_the_lift(dev):
    """The full d cross_entropy / d x of NODE_RNN (the lift's path included) by the same rule."""
    from fet_ode_amd import ecg
    g = load_golden("node_rnn")
    sd = golden_sd(g)
    H, D, K, T = TD.FIX
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    e64 = XR.node_rnn_xgrad(sd, x, y, torch.float64)
    c = max(TD.nrel(XR.node_rnn_xgrad(sd if s == 0 else R.rounded(sd, s), x, y), e64) for s in (0, 1, 2, 3))

    def run():
        m = ecg.NODE_RNN(input_size=D, hidden_size=H, num_classes=2, num_basis=K, solver="rk4")
        m.load_state_dict(sd)
        m = m.to(dev)
        xg = x.to(dev).requires_grad_(True)
        F.cross_entropy(m(xg), y.to(dev)).backward()
        return xg.grad, [p.grad for p in m.parameters()]

    with xgrad(False):
        staged, pst = run()
    with xgrad(True):
        got, pg = run()
    err, st = TD.nrel(got, e64), TD.nrel(staged, e64)
    bar = max(1e-4, 2 * st, 2 * c)
    print(f"NODE_RNN d/dx: gpu {err:.3e}, per-stage {st:.3e}, worst fp32 control {c:.3e}, bar {bar:.3e}")
    assert err <= bar and not torch.equal(got, staged)           # two different programs
    for a, b in zip(pg, pst):
        assert TD.nrel(a, b) <= 2e-4 if b.any() else not a.any()


# ---------------------------------------------------------------------------------------------
# 4. structure
# ---------------------------------------------------------------------------------------------
def test_parameter_gradients_do_not_see_the_series_gradient(dev):
    shape = (8, 1, 3, 9, 3)
    x, w = case_series(shape), weights(shape, "all")
    with xgrad(True):
        gx, ps, gh, via = gpu_run(shape, x, w, dev, h0_grad=True)
        _, ps0, gh0, via0 = gpu_run(shape, x, w, dev, series_grad=False, h0_grad=True)
    assert via == via0 == FUSED and gx is not None
    assert torch.equal(gh, gh0) and all(torch.equal(a, b) for a, b in zip(ps, ps0))


def test_shared_series_sums_the_rows(dev):
    import fet_ode_amd as FA
    from fet_ode_amd import ecg
    shape = H, D, K, T, B = (8, 1, 3, 9, 3)
    x2 = case_series(shape)[1]
    h0 = torch.randn(B, H, generator=torch.Generator().manual_seed(1))
    w = weights(shape, "all")
    with xgrad(True):
        full, _, _, via = gpu_run(shape, x2.expand(B, T, D).clone(), w, dev, h0=h0)
        f = TD.gpu_field(H, D, K, dev)
        t_grid = torch.linspace(0.0, 1.0, steps=T).to(dev)
        xg = x2.to(dev).requires_grad_(True)
        f.set_interpolator(ecg.LinearInterp1D(t_grid, xg))
        f.basis.reset_state()
        f.basis._prev = torch.zeros(B, H + D, device=dev)
        traj = FA.odeint(f, h0.to(dev), t_grid, method="rk4")
        (traj * w.to(dev)).sum().backward()
    assert via == FUSED and type(traj.grad_fn).__name__ == FUSED and xg.grad.shape == (T, D)
    r = TD.nrel(xg.grad, full.sum(0))
    print(f"shared series: |grad - sum of the rows' gradients| normwise {r:.3e}")
    assert torch.equal(xg.grad, full.sum(0)) or r <= 1e-6


def test_only_the_series_requires_grad(dev):
    shape = (5, 2, 4, 6, 3)
    x, w = case_series(shape), weights(shape, "all")
    with xgrad(True):
        ref, _, _, _ = gpu_run(shape, x, w, dev)
        got, ps, gh, via = gpu_run(shape, x, w, dev, param_grad=False)
    assert via == FUSED and gh is None and all(p is None for p in ps)   # no parameter gradient is allocated
    assert torch.equal(got, ref)


def test_knob_off_is_the_per_stage_path(dev):
    shape = (8, 1, 3, 9, 3)
    x, w = case_series(shape), weights(shape, "last")
    with xgrad(False):
        off, pso, _, via = gpu_run(shape, x, w, dev)
        with TD.per_stage():
            staged, pss, _, _ = gpu_run(shape, x, w, dev)
        # without a series gradient the fused path is taken as before
        _, _, _, via_plain = gpu_run(shape, x, w, dev, series_grad=False)
    assert via != FUSED and via_plain == FUSED
    assert torch.equal(off, staged) and all(torch.equal(a, b) for a, b in zip(pso, pss))
