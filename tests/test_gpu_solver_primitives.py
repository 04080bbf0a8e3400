"""The small kernels every dopri5 / fixed-grid path is built from (include/fetode.h: fetode_lincomb,
fetode_scaled_rms / _sumsq, fetode_interp_fit / _eval, fetode_rk_combine, fetode_axpby) and the
FerroNet elementwise stages (fetode_tanh_bound, fetode_tanh, fetode_nan_clamp and their backward
kernels), called directly through ctypes — not through a solve, where they only ever see n = B D,
kstride == n, a workspace, and a step controller that absorbs a small error.

References: the per-op fp32 restatements and oracle recordings of test_solver_primitives_ref.py
(proved against torch / the oracle on the CPU there); the elementwise kernels must match them bit
for bit.  The two norms are held to the exact sum of the exactly squared fp32 quotients.  Every
output is followed by canary words that must survive, and every kernel also runs on pointers one
element past an allocation's start (no alignment beyond 4 bytes may be assumed)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_solver_primitives_ref import (NAN_CLAMP_PARAMS, SIZES, X_EVAL, assert_bitwise, axpby_ref, combine_cases,
                                        f32, interp_case, lincomb_ref, nan_clamp_inputs, nan_clamp_torch,
                                        oracle_eval, oracle_interp, rand, scaled_q_ref, sumsq_exact,
                                        tanh_backward_ref, tanh_bound_backward_ref)

pytestmark = pytest.mark.gpu

CANARY = -7.0e37     # fp32-representable; never a result of the data used here
PAD = 8
WRAP = 4096 * 256 + 1    # one element past the FerroNet kernels' largest grid: the stride loop wraps


@pytest.fixture(scope="module")
def L(dev):
    from fet_ode_amd import _lib
    return _lib.load()


class Buf:
    """n floats at element `off` of a canary-filled allocation with PAD canaries behind them."""

    def __init__(self, dev, n, off, data=None, dtype=torch.float32):
        self.n, self.off = n, off
        self.all = torch.full((off + n + PAD,), CANARY, device=dev, dtype=dtype)
        self.t = self.all[off:off + n]
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)).reshape(-1))

    @property
    def p(self):
        return self.t.data_ptr()

    def get(self):
        """the n values, after checking that nothing around them was written"""
        a = self.all.cpu().numpy()
        guard = np.concatenate([a[:self.off], a[self.off + self.n:]])
        assert (guard == a.dtype.type(CANARY)).all(), "a kernel wrote outside its output"
        return a[self.off:self.off + self.n]


def _s(dev):
    from fet_ode_amd import _lib
    return _lib.stream_handle(dev)


def _cf(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


# ---- fetode_lincomb ---------------------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_lincomb(dev, L, n, off):
    """m = 1..8, with and without y0, rows packed (kstride == n) and padded (kstride = n + 5, the
    padding poisoned with NaN): bitwise the header's acc = k0 c0; acc = acc + kj cj; y0 + acc, and
    within m 2^-23 sum |k_j c_j| of the oracle's k[..., :m].matmul(c)."""
    y0 = rand(n, 1)
    for m in range(1, 9):
        k = rand(m * n, 10 + m).reshape(m, n)
        c = rand(m, 20 + m, 0.3)
        mm = torch.from_numpy(k).t().contiguous().matmul(torch.from_numpy(c)).numpy().astype(np.float64)
        bound = m * 2.0 ** -23 * (np.abs(k.astype(np.float64)) * np.abs(c.astype(np.float64))[:, None]).sum(0)
        for ks in (n, n + 5):
            kp = np.full((m, ks), np.nan, np.float32)
            kp[:, :n] = k
            kb = Buf(dev, m * ks, off, kp)
            _, cp = _cf(c)
            for with_y0 in (True, False):
                yb = Buf(dev, n, off, y0)
                out = Buf(dev, n, off)
                rc = L.fetode_lincomb(yb.p if with_y0 else None, kb.p, ks, cp, m, out.p, n, _s(dev))
                assert rc == 0
                got = out.get()
                assert_bitwise(got, lincomb_ref(y0 if with_y0 else None, k, c), f"m={m} kstride={ks} y0={with_y0}")
                if not with_y0:
                    assert (np.abs(got.astype(np.float64) - mm) <= bound).all(), f"matmul bound m={m}"


# ---- fetode_interp_fit / fetode_interp_eval ---------------------------------------------------

@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_interp_fit_and_eval(dev, L, n, off):
    """Bitwise O._interp_fit (fed y_mid = y0 + sum_j k_j mid_j formed per-op) and
    O._interp_evaluate at x = 0, 1, 0.3712.., a denormal; the fit at x = 0 is y0 exactly."""
    y0, y1, k, mid, dt = interp_case(n, 100 + n % 97)
    ref = oracle_interp(y0, y1, k, mid, dt)
    _, mp = _cf(mid)
    for ks in (n, n + 5):
        kp = np.full((7, ks), np.nan, np.float32)
        kp[:, :n] = k
        kb, a, b = Buf(dev, 7 * ks, off, kp), Buf(dev, n, off, y0), Buf(dev, n, off, y1)
        co = Buf(dev, 5 * n, off)
        assert L.fetode_interp_fit(a.p, b.p, kb.p, ks, mp, float(dt), co.p, n, _s(dev)) == 0
        got = co.get().reshape(5, n)
        assert_bitwise(got, ref, f"interp_fit kstride={ks}")
        for x in X_EVAL:
            out = Buf(dev, n, off)
            assert L.fetode_interp_eval(co.p, x, out.p, n, _s(dev)) == 0
            r = out.get()
            assert_bitwise(r, oracle_eval(ref, x), f"interp_eval x={x}")
            if x == 0.0:
                assert_bitwise(r, y0, "x = 0 returns y0")


# ---- fetode_rk_combine ------------------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64], ids=["t32", "t64"])
@pytest.mark.parametrize("n", SIZES)
def test_rk_combine(dev, L, n, tdtype, off):
    """Every (method, stage) of the header against what the oracle's own steps feed the field and
    return (rk4_alt_step, rk4_classic_step, midpoint_step, euler_step with a recording func), dt
    formed in the time dtype and rounded to fp32, 0.5 dt, fp32(dt / 6): bitwise."""
    y, cases = combine_cases(n, 300 + n % 89, tdtype)
    yb = Buf(dev, n, off, y)
    for label, method, stage, ks, dt, exp in cases:
        kb = [Buf(dev, n, off, k) for k in ks]
        ptrs = [b.p for b in kb] + [None] * (4 - len(kb))
        out = Buf(dev, n, off)
        assert L.fetode_rk_combine(method, stage, yb.p, *ptrs, float(dt), out.p, n, _s(dev)) == 0
        assert_bitwise(out.get(), exp, label)


# ---- fetode_axpby -----------------------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_axpby(dev, L, n, off):
    """a x + b y as two rounded products and one sum (and a x alone with y = NULL); a, b among
    0, -1 and full-mantissa values."""
    x, y = rand(n, 5), rand(n, 6)
    xb, yb = Buf(dev, n, off, x), Buf(dev, n, off, y)
    full = [float(f32(1.2345678)), float(f32(-0.87654321))]
    for a in [0.0, -1.0] + full:
        for b in [0.0, -1.0] + full:
            for with_y in (True, False):
                out = Buf(dev, n, off)
                assert L.fetode_axpby(n, a, xb.p, b, yb.p if with_y else None, out.p, _s(dev)) == 0
                assert_bitwise(out.get(), axpby_ref(a, x, b, y if with_y else None), f"a={a} b={b} y={with_y}")


# ---- fetode_scaled_rms / fetode_scaled_sumsq --------------------------------------------------

NORM_SIZES = [1, 2047, 2048, 2049, 6145, 1 << 20, (1 << 20) + 1]
RTOL, ATOL = 1e-3, 1e-4


def _ws(dev, L):
    return torch.zeros(L.fetode_scaled_rms_workspace(0) // 8, device=dev, dtype=torch.float64)


def _norms(dev, L, a, sub, y0, y1, ws, off=0):
    """(rms, flag), (sumsq, flag) of one input set"""
    n = len(a)
    bufs = [None if v is None else Buf(dev, n, off, v) for v in (a, sub, y0, y1)]
    p = [None if b is None else b.p for b in bufs]
    wp = None if ws is None else ws.data_ptr()
    o32, o64 = Buf(dev, 2, off), Buf(dev, 2, off, dtype=torch.float64)
    assert L.fetode_scaled_rms(*p, RTOL, ATOL, n, o32.p, wp, _s(dev)) == 0
    assert L.fetode_scaled_sumsq(*p, RTOL, ATOL, n, o64.p, wp, _s(dev)) == 0
    return o32.get(), o64.get()


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("use_ws", [True, False], ids=["ws", "no-ws"])
@pytest.mark.parametrize("n", NORM_SIZES)
def test_scaled_norms(dev, L, n, use_ws):
    """One workgroup, the first grid launch, a ragged last slice, the 512-group cap and a slice
    above 2048 elements; sub / y1 present and NULL in all four combinations.  S = the correctly
    rounded sum of the exact fp64 squares of q = v / (atol32 + rtol32 m) (per-op fp32):
    |sumsq - S| <= 2 n 2^-53 S (an fp64 sum in any order), rms within one fp32 ulp of
    sqrt(fp32(S / n)); the flag is 0 for finite y0.  The oracle's fp32-mean _rms_norm lies within
    its own (n + 4) 2^-24 of the same value (a sanity check of the reference, not the bar)."""
    from oracle import torch_ref as O
    a, sub, y0, y1 = (rand(n, 40 + i) for i in range(4))
    ws = _ws(dev, L) if use_ws else None
    for has_sub in (False, True):
        for has_y1 in (False, True):
            s_, y1_ = (sub if has_sub else None), (y1 if has_y1 else None)
            q = scaled_q_ref(a, s_, y0, y1_, RTOL, ATOL)
            S = sumsq_exact(q)
            (rms, f32flag), (ss, f64flag) = _norms(dev, L, a, s_, y0, y1_, ws, off=int(has_sub))
            assert f32flag == 0.0 and f64flag == 0.0
            assert abs(ss - S) <= 2 * n * 2.0 ** -53 * S, (n, has_sub, has_y1, ss, S)
            want = np.sqrt(np.float32(S / n))
            assert _ulps(rms, want) <= 1, (n, has_sub, has_y1, rms, want)
            orc = float(O._rms_norm(torch.from_numpy(q)))
            assert abs(orc - math.sqrt(S / n)) <= (n + 4) * 2.0 ** -24 * math.sqrt(S / n)
    if use_ws:
        assert ws[-1:].view(torch.int64).item() == 0, "the arrival counter must be zero between calls"


@pytest.mark.parametrize("use_ws", [True, False], ids=["ws", "no-ws"])
@pytest.mark.parametrize("n", [1, 2049, 6145, (1 << 20) + 1])
def test_scaled_norms_nonfinite_flag(dev, L, n, use_ws):
    """out[1] = 1 for one NaN / +inf / -inf in y0 — at element 0, at n - 1, inside the first and
    inside the last slice, one call each — and 0 when only a or y1 holds one (torchdiffeq asserts
    on y0 alone)."""
    a, y0, y1 = rand(n, 1), rand(n, 2), rand(n, 3)
    ws = _ws(dev, L) if use_ws else None
    groups = min(512, (n + 2047) // 2048)
    slice_ = (n + groups - 1) // groups
    spots = sorted({0, n - 1, min(n - 1, slice_ // 2), max(0, n - 1 - slice_ // 3)})
    for pos in spots:
        for bad in (np.nan, np.inf, -np.inf):
            y = y0.copy()
            y[pos] = bad
            (_, fa), (_, fb) = _norms(dev, L, a, None, y, y1, ws)
            assert fa == 1.0 and fb == 1.0, (n, pos, bad)
            for who in ("a", "y1"):
                aa, yy = a.copy(), y1.copy()
                (aa if who == "a" else yy)[pos] = bad
                (_, fa), (_, fb) = _norms(dev, L, aa, None, y0, yy, ws)
                assert fa == 0.0 and fb == 0.0, (n, pos, bad, who)


def test_scaled_norm_workspace_reuse(dev, L):
    """One workspace, one stream: a 512-group call, a 3-group call, a call that raises the flag, then
    a clean call whose flag is 0 again and whose sum owes nothing to the stale partials; the
    arrival counter word is zero at the end."""
    ws = _ws(dev, L)

    def call(n, seed, poison=None):
        a, y0 = rand(n, seed, 3.0), rand(n, seed + 1)
        S = sumsq_exact(scaled_q_ref(a, None, y0, None, RTOL, ATOL))
        if poison is not None:
            y0[poison] = np.nan
        (rms, f1), (ss, f2) = _norms(dev, L, a, None, y0, None, ws)
        return rms, f1, ss, f2, S

    n_big, n3 = 1 << 20, 2 * 2048 + 1
    _, f1, ss, f2, S = call(n_big, 1)
    assert f1 == 0 and f2 == 0 and abs(ss - S) <= 2 * n_big * 2.0 ** -53 * S
    _, f1, ss, f2, S = call(n3, 3)
    assert f1 == 0 and f2 == 0 and abs(ss - S) <= 2 * n3 * 2.0 ** -53 * S
    _, f1, _, f2, _ = call(n3, 5, poison=n3 - 1)
    assert f1 == 1 and f2 == 1
    rms, f1, ss, f2, S = call(n3, 7)
    assert f1 == 0 and f2 == 0, "a raised flag must not outlive its call"
    assert abs(ss - S) <= 2 * n3 * 2.0 ** -53 * S
    assert _ulps(rms, np.sqrt(np.float32(S / n3))) <= 1
    assert ws[-1:].view(torch.int64).item() == 0


def test_scaled_norms_empty(dev, L):
    """n = 0: the sum of squares is two zeros, the RMS (a mean over nothing) is FETODE_EINVAL."""
    from fet_ode_amd import _lib
    o64 = Buf(dev, 2, 0, dtype=torch.float64)
    assert L.fetode_scaled_sumsq(None, None, None, None, RTOL, ATOL, 0, o64.p, None, _s(dev)) == 0
    assert (o64.get() == 0.0).all()
    o32, x = Buf(dev, 2, 0), Buf(dev, 4, 0, np.ones(4, np.float32))
    assert L.fetode_scaled_rms(x.p, None, x.p, None, RTOL, ATOL, 0, o32.p, None, _s(dev)) == _lib.FETODE_EINVAL
    assert (o32.all.cpu().numpy() == f32(CANARY)).all()


# ---- fetode_nan_clamp / _backward -------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("params", NAN_CLAMP_PARAMS, ids=["ref", "inf-inside", "nan-nan"])
@pytest.mark.parametrize("n", SIZES + [WRAP])
def test_nan_clamp(dev, L, n, params, off):
    """NaN, +-inf, +-0, denormals, +-50 and their neighbours, +-1e3 and ordinary values: bitwise
    torch.clamp(torch.nan_to_num(x, nan, posinf, neginf), lo, hi) on the CPU and its autograd —
    with the reference's arguments, with +-inf replaced INSIDE the clamp (the gradient is still 0)
    and with a NaN replacement, which torch.clamp propagates."""
    x, g = nan_clamp_inputs(n, 9), rand(n, 10)
    ro, rg = nan_clamp_torch(x, g, *params)
    xb, gb, out, gx = Buf(dev, n, off, x), Buf(dev, n, off, g), Buf(dev, n, off), Buf(dev, n, off)
    assert L.fetode_nan_clamp(n, *params, xb.p, out.p, _s(dev)) == 0
    assert L.fetode_nan_clamp_backward(n, *params, gb.p, xb.p, gx.p, _s(dev)) == 0
    assert_bitwise(out.get(), ro, "forward")
    assert_bitwise(gx.get(), rg, "backward")


# ---- fetode_tanh_bound / fetode_tanh and their backward kernels --------------------------------

TANH_ULP_BAR = 0.53 + 2.0


def _tanh_inputs(n, hb, seed):
    x = (np.random.default_rng(seed).uniform(-12.0, 12.0, n) * hb).astype(np.float32)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 12.0 * hb, -12.0 * hb, 1e-40, 1e-6 * hb], np.float32)
    m = min(n, len(edge))
    x[:m] = edge[:m]
    if n > len(edge):
        x[-len(edge):] = edge
    return x


def _tanh_ulps(t, arg):
    """max relative error / 2^-23 of t against fp64 tanh of the fp32 argument (normal results)"""
    ref = np.tanh(arg.astype(np.float64))
    ok = np.isfinite(ref) & (np.abs(ref) >= 2.0 ** -126)
    if not ok.any():
        return 0.0
    return float((np.abs(t.astype(np.float64) - ref)[ok] / np.abs(ref)[ok]).max() / 2.0 ** -23)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("hb", [1.0, 3.0, 0.7])
@pytest.mark.parametrize("n", SIZES + [WRAP])
def test_tanh_bound_and_tanh(dev, L, n, hb, off):
    """out == h_bound * t_out bitwise, the same out with t_out = NULL, +-0 -> +-0, +-inf -> +-1,
    NaN -> NaN; both backward kernels bitwise the header's expressions ((g hb) (1 - t^2)) / hb and
    g (1 - y^2), per-op on the kernel's own t / y; the tanh itself within TANH_ULP_BAR of fp64 tanh
    of the fp32 argument (test_tanh_accuracy states the bar)."""
    x, g = _tanh_inputs(n, hb, 11), rand(n, 12)
    xb, gb = Buf(dev, n, off, x), Buf(dev, n, off, g)
    out, t, out2 = Buf(dev, n, off), Buf(dev, n, off), Buf(dev, n, off)
    assert L.fetode_tanh_bound(n, hb, xb.p, out.p, t.p, _s(dev)) == 0
    assert L.fetode_tanh_bound(n, hb, xb.p, out2.p, None, _s(dev)) == 0
    tv, ov = t.get(), out.get()
    assert_bitwise(ov, f32(hb) * tv, "out = hb * t")
    assert_bitwise(out2.get(), ov, "t_out = NULL")
    arg = x / f32(hb)
    m = min(n, 5)
    assert_bitwise(tv[:m], np.array([0.0, -0.0, 1.0, -1.0, np.nan], np.float32)[:m], "edges")
    assert _tanh_ulps(tv, arg) <= TANH_ULP_BAR
    gx = Buf(dev, n, off)
    assert L.fetode_tanh_bound_backward(n, hb, gb.p, t.p, gx.p, _s(dev)) == 0
    assert_bitwise(gx.get(), tanh_bound_backward_ref(g, tv, hb), "tanh_bound backward")
    if hb == 1.0:
        y, gy = Buf(dev, n, off), Buf(dev, n, off)
        assert L.fetode_tanh(n, xb.p, y.p, _s(dev)) == 0
        yv = y.get()
        assert_bitwise(yv[:m], np.array([0.0, -0.0, 1.0, -1.0, np.nan], np.float32)[:m], "edges")
        assert _tanh_ulps(yv, x) <= TANH_ULP_BAR
        assert L.fetode_tanh_backward(n, gb.p, y.p, gy.p, _s(dev)) == 0
        assert_bitwise(gy.get(), tanh_backward_ref(g, yv), "tanh backward")


def test_tanh_bound_rejects_zero_bound(dev, L):
    from fet_ode_amd import _lib
    x, out = Buf(dev, 4, 0, np.ones(4, np.float32)), Buf(dev, 4, 0)
    assert L.fetode_tanh_bound(4, 0.0, x.p, out.p, None, _s(dev)) == _lib.FETODE_EINVAL
    assert (out.all.cpu().numpy() == f32(CANARY)).all()


def test_tanh_accuracy(dev, L, capsys):
    """The device tanh of fetode_tanh / fetode_tanh_bound against fp64 tanh of the fp32 argument over
    2 000 001 points of [-12, 12].  Yardstick: the reference's own arithmetic, torch's CPU fp32 tanh,
    reaches 0.53 ulp (relative error / 2^-23) on the same points; device math functions are specified
    to a couple of ulp, not correctly rounded, so the bar is that plus 2 ulp.
    Measured on the MI355X: 1.169 ulp (this test prints the figure of its run)."""
    n = 2_000_001
    x = np.linspace(-12.0, 12.0, n).astype(np.float32)
    xb, y, o, t = Buf(dev, n, 0, x), Buf(dev, n, 0), Buf(dev, n, 0), Buf(dev, n, 0)
    assert L.fetode_tanh(n, xb.p, y.p, _s(dev)) == 0
    assert L.fetode_tanh_bound(n, 1.0, xb.p, o.p, t.p, _s(dev)) == 0
    yv, tv = y.get(), t.get()
    u = _tanh_ulps(yv, x)
    with capsys.disabled():
        print(f"\nfetode_tanh: max error {u:.3f} ulp over {n} points of [-12, 12] (bar {TANH_ULP_BAR})")
    assert_bitwise(tv, yv, "tanh_bound(h_bound = 1) is tanh")
    assert u <= TANH_ULP_BAR
