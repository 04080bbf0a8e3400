"""Per-op fp32 restatements of the small solver kernels (include/fetode.h: fetode_lincomb,
fetode_interp_fit / _eval, fetode_rk_combine, fetode_axpby, the scaled error of fetode_scaled_rms /
_sumsq, the backward expressions of fetode_tanh_bound / fetode_tanh) in numpy — one ufunc per
operation on float32 arrays, so every product and sum is rounded and nothing is contracted — and
the proof, on the CPU, that each of them is bitwise torch / the oracle (oracle/torch_ref.py).  One
exception, stated where it is proved: torch's CPU tanh' forms 1 - y^2 with a fused multiply-add, the
header's g * (1 - y^2) rounds the square, so the two tanh backward restatements sit one rounding from
torch's autograd (bitwise once that term is fused).

tests/test_gpu_solver_primitives.py imports the helpers below and holds the HIP kernels to them bit
for bit, so this module is what makes those references trustworthy without a GPU."""
import math

import numpy as np
import pytest
import torch

f32 = np.float32
SIZES = [1, 63, 255, 256, 257, 100003]


def rand(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bitwise(got, ref, what=""):
    """equal as bit patterns (so -0 != +0), any NaN equal to any NaN"""
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    same = (bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))
    if not same.all():
        i = int(np.flatnonzero(~same.reshape(-1))[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} differ, first at {i}: "
                             f"{got.reshape(-1)[i]!r} != {ref.reshape(-1)[i]!r}")


# ---- the restatements -----------------------------------------------------------------------

def lincomb_ref(y0, k, c):
    """fetode.h: out = (y0 ? y0 : 0) + sum_j k[j] c[j]: acc = k0 c0; acc = acc + kj cj ...; y0 + acc"""
    acc = k[0] * f32(c[0])
    for j in range(1, len(c)):
        acc = acc + k[j] * f32(c[j])
    return acc if y0 is None else y0 + acc


def interp_fit_ref(y0, y1, k, mid, dt):
    """interp_fit_kernel: [e, d, c, b, a] with y_mid = y0 + k . mid (mid = c_mid * dt, 7 floats)"""
    dt = f32(dt)
    ym = lincomb_ref(y0, k, mid)
    f0, f1 = k[0], k[6]
    a = ((f32(2) * dt) * (f1 - f0) - f32(8) * (y1 + y0)) + f32(16) * ym
    b = ((dt * (f32(5) * f0 - f32(3) * f1) + f32(18) * y0) + f32(14) * y1) - f32(32) * ym
    c = ((dt * (f1 - f32(4) * f0) - f32(11) * y0) - f32(5) * y1) + f32(16) * ym
    return np.stack([y0, dt * f0, c, b, a])


def interp_eval_ref(co, x):
    x = f32(x)
    total = co[0] + x * co[1]
    xp = x
    for j in range(2, 5):
        xp = xp * x
        total = total + xp * co[j]
    return total


def rk_combine_ref(method, stage, y, k1, k2, k3, k4, dt):
    """rk_combine_kernel (method: 0 euler, 1 midpoint, 2 rk4 3/8, 3 classic rk4)"""
    dt, third = f32(dt), f32(1) / f32(3)
    if method == 2:
        if stage == 1:
            return y + (dt * k1) * third
        if stage == 2:
            return y + dt * (k2 - k1 * third)
        if stage == 3:
            return y + dt * ((k1 - k2) + k3)
        return y + (((k1 + f32(3) * (k2 + k3)) + k4) * dt) * f32(0.125)
    if method == 3 and stage == 4:
        return y + dt * (((k1 + f32(2) * k2) + f32(2) * k3) + k4)
    return y + dt * k1


def axpby_ref(a, x, b, y):
    return f32(a) * x if y is None else f32(a) * x + f32(b) * y


def scaled_q_ref(a, sub, y0, y1, rtol, atol):
    """q = (a - sub) / (atol32 + rtol32 max(|y0|, |y1|)), the element the two norms square and sum"""
    v = a if sub is None else a - sub
    m = np.abs(y0) if y1 is None else np.maximum(np.abs(y0), np.abs(y1))
    return v / (f32(atol) + f32(rtol) * m)


def sumsq_exact(q):
    """sum q^2 with every square exact in fp64 (24-bit mantissas) and the sum correctly rounded"""
    return math.fsum((q.astype(np.float64) ** 2).tolist())


def tanh_bound_backward_ref(g, t, hb):
    hb = f32(hb)
    return ((g * hb) * (f32(1) - t * t)) / hb


def tanh_backward_ref(g, y):
    return g * (f32(1) - y * y)


# ---- what the oracle's fixed-grid steps feed the field, and what they return ---------------

def record_step(step_fn, ks, y, dt):
    """Run one oracle step with a `func` that returns the prescribed ks in call order and records
    the stage inputs it is called with.  dt: a 0-dim time tensor (fp32 or fp64).  Returns
    (stage inputs after the first, which is y itself; y + dy)."""
    seen, it = [], iter(ks)

    def func(tt, yy):
        seen.append(yy.clone())
        return next(it)

    t0 = torch.zeros((), dtype=dt.dtype)
    dy = step_fn(func, t0, dt, t0 + dt, y)
    assert torch.equal(seen[0], y)
    return [s.numpy() for s in seen[1:]], (y + dy).numpy()


def step_coefs(dt):
    """the kernel's dt arguments as odeint.Schedule forms them: the time dtype's dt, 0.5 dt and
    dt / 6, each rounded to fp32"""
    d = dt.numpy()
    return f32(d), f32(0.5 * d), f32(d / 6.0)


def combine_cases(n, seed, tdtype):
    """every (method, stage) of fetode_rk_combine with its oracle value:
    (label, method, stage, (k1, k2, k3, k4) or fewer, dt argument, expected) and y"""
    from oracle import torch_ref as O
    y = torch.from_numpy(rand(n, seed))
    ks = [torch.from_numpy(rand(n, seed + 1 + j)) for j in range(4)]
    dt = torch.tensor(0.1234567891234, dtype=tdtype)
    d, hh, h6 = step_coefs(dt)
    kn = [k.numpy() for k in ks]
    out = []
    st, y1 = record_step(O.rk4_alt_step, ks, y, dt)
    for s in range(3):
        out.append((f"rk4 stage {s + 1}", 2, s + 1, kn[:s + 1], d, st[s]))
    out.append(("rk4 stage 4", 2, 4, kn, d, y1))
    st, y1 = record_step(O.rk4_classic_step, ks, y, dt)
    out.append(("classic k2 input", 3, 1, [kn[0]], hh, st[0]))
    out.append(("classic k3 input", 3, 2, [kn[1]], hh, st[1]))
    out.append(("classic k4 input", 3, 3, [kn[2]], d, st[2]))
    out.append(("classic stage 4", 3, 4, kn, h6, y1))
    st, y1 = record_step(O.midpoint_step, ks[:2], y, dt)
    out.append(("midpoint input", 1, 1, [kn[0]], hh, st[0]))
    out.append(("midpoint step", 1, 4, [kn[1]], d, y1))
    st, y1 = record_step(O.euler_step, ks[:1], y, dt)
    out.append(("euler step", 0, 4, [kn[0]], d, y1))
    return y.numpy(), out


X_EVAL = [0.0, 1.0, float(f32(0.3712345)), 1e-40]   # the last one is an fp32 denormal


def interp_case(n, seed):
    """y0, y1, k (7, n), mid (c_mid dt in fp32), dt for fetode_interp_fit"""
    from oracle import torch_ref as O
    dt = f32(0.0371)
    cmid = np.array(O.DOPRI5_C_MID, dtype=np.float64).astype(np.float32)
    return rand(n, seed), rand(n, seed + 1), rand(7 * n, seed + 2).reshape(7, n), cmid * dt, dt


def oracle_interp(y0, y1, k, mid, dt):
    """O._interp_fit fed y_mid = y0 + sum_j k_j mid_j formed per-op; returns (5, n)"""
    from oracle import torch_ref as O
    T = torch.from_numpy
    ym = T(lincomb_ref(y0, k, mid))
    co = O._interp_fit(T(y0), T(y1), ym, T(k[0]), T(k[6]), torch.tensor(float(dt), dtype=torch.float32))
    return np.stack([c.numpy() for c in co])


def oracle_eval(co, x):
    from oracle import torch_ref as O
    one = torch.tensor(1.0, dtype=torch.float64)
    return O._interp_evaluate([torch.from_numpy(c) for c in co], 0 * one, one, torch.tensor(x, dtype=torch.float64)).numpy()


NAN_CLAMP_PARAMS = [(0.0, 1e3, -1e3, -50.0, 50.0), (0.0, 10.0, -10.0, -50.0, 50.0),
                    (math.nan, 1e3, -1e3, -50.0, 50.0)]


def nan_clamp_inputs(n, seed):
    nx = np.nextafter
    edge = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 50.0, -50.0,
                     nx(f32(50), f32(100)), nx(f32(50), f32(0)), nx(f32(-50), f32(-100)), nx(f32(-50), f32(0)),
                     1e3, -1e3, 3.25, -17.5], dtype=np.float32)
    x = rand(n, seed, 40.0)
    m = min(n, len(edge))
    x[:m] = edge[:m]
    if n > len(edge):   # the same edges again at the tail (the last block / the wrapped stride)
        x[-len(edge):] = edge
    return x


def nan_clamp_torch(x, g, nan, posinf, neginf, lo, hi):
    """torch.clamp(torch.nan_to_num(x, ...), lo, hi) on the CPU and its autograd"""
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    out = torch.clamp(torch.nan_to_num(xt, nan=nan, posinf=posinf, neginf=neginf), lo, hi)
    out.backward(torch.from_numpy(g))
    return out.detach().numpy(), xt.grad.numpy()


# ---- the proofs (CPU) -----------------------------------------------------------------------

@pytest.mark.parametrize("m", range(1, 9))
def test_lincomb_ref_is_the_torch_expression(m):
    """bitwise ks[0] c[0] + ks[1] c[1] + ... (then y0 +) in torch, and within the summation bound
    m 2^-23 sum |k_j c_j| of the oracle's k[..., :m].matmul(c)"""
    n = 100003
    k, y0 = rand(m * n, m).reshape(m, n), rand(n, 50 + m)
    c = rand(m, 100 + m, 0.3)
    kt, ct = torch.from_numpy(k), torch.from_numpy(c)
    acc = kt[0] * ct[0]
    for j in range(1, m):
        acc = acc + kt[j] * ct[j]
    assert_bitwise(lincomb_ref(None, k, c), acc.numpy(), "no y0")
    assert_bitwise(lincomb_ref(y0, k, c), (torch.from_numpy(y0) + acc).numpy(), "y0")
    mm = kt.t().contiguous().matmul(ct).numpy()
    bound = m * 2.0 ** -23 * (np.abs(k.astype(np.float64)) * np.abs(c.astype(np.float64))[:, None]).sum(0)
    assert (np.abs(lincomb_ref(None, k, c).astype(np.float64) - mm) <= bound).all()


@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64])
def test_rk_combine_ref_is_the_oracle(tdtype):
    y, cases = combine_cases(100003, 7, tdtype)
    for label, method, stage, ks, dt, exp in cases:
        ks = list(ks) + [None] * (4 - len(ks))
        assert_bitwise(rk_combine_ref(method, stage, y, *ks, dt), exp, label)


def test_interp_ref_is_the_oracle():
    y0, y1, k, mid, dt = interp_case(100003, 11)
    co = interp_fit_ref(y0, y1, k, mid, dt)
    assert_bitwise(co, oracle_interp(y0, y1, k, mid, dt), "interp_fit")
    for x in X_EVAL:
        assert_bitwise(interp_eval_ref(co, x), oracle_eval(co, x), f"interp_eval x={x}")
    assert_bitwise(interp_eval_ref(co, 0.0), y0, "the fit at x = 0 is y0")


def test_axpby_ref_is_torch():
    x, y = torch.from_numpy(rand(100003, 1)), torch.from_numpy(rand(100003, 2))
    for a, b in ((0.0, 1.0), (-1.0, 0.0), (float(f32(1.2345678)), float(f32(-0.87654321)))):
        assert_bitwise(axpby_ref(a, x.numpy(), b, y.numpy()), (a * x + b * y).numpy())
        assert_bitwise(axpby_ref(a, x.numpy(), b, None), (a * x).numpy())


@pytest.mark.parametrize("sub,y1", [(False, False), (True, False), (False, True), (True, True)])
def test_scaled_q_ref_is_the_oracle_expression(sub, y1):
    """the oracle's err / (atol + rtol max(|y0|, |y1|)) with fp64 0-dim tolerances (_dopri5) and
    _select_initial_step's scale; its fp32-mean RMS within (n + 4) 2^-24 of the exact one"""
    from oracle import torch_ref as O
    n, rtol, atol = 6145, 1e-3, 1e-4
    a, s, y0, yb = (rand(n, i) for i in range(4))
    T = torch.from_numpy
    rt, at = torch.as_tensor(rtol, dtype=torch.float64), torch.as_tensor(atol, dtype=torch.float64)
    tol = at + rt * (torch.max(T(y0).abs(), T(yb).abs()) if y1 else torch.abs(T(y0)))
    qt = ((T(a) - T(s)) if sub else T(a)) / tol
    q = scaled_q_ref(a, s if sub else None, y0, yb if y1 else None, rtol, atol)
    assert_bitwise(q, qt.numpy())
    exact = math.sqrt(sumsq_exact(q) / n)
    assert abs(float(O._rms_norm(qt)) - exact) <= (n + 4) * 2.0 ** -24 * exact


def _one_minus_sq_fused(y):
    """fl(1 - y^2) with the square unrounded, as one fused multiply-add forms it (y^2 is exact in fp64)"""
    return (1.0 - y.astype(np.float64) ** 2).astype(np.float32)


def test_tanh_backward_refs_are_torch_autograd():
    """torch's chain for h_bound * tanh(x / h_bound) is mul(h_bound) . tanh' . div(h_bound), the
    header's.  Its CPU tanh' kernel forms 1 - y^2 with ONE rounding (a fused multiply-add), the
    header's g * (1 - y^2) rounds the square too: torch is bitwise the restatement with that one
    term fused, and the per-op restatement the kernels are held to lies within the extra rounding
    of it: |s - s'| <= 3 * 2^-24 for the two forms of 1 - y^2 <= 1, then one rounded product each."""
    x, g = rand(100003, 3, 4.0), rand(100003, 4)
    for hb in (3.0, 0.7):
        xt = torch.from_numpy(x).clone().requires_grad_(True)
        t = torch.tanh(xt / hb)
        (hb * t).backward(torch.from_numpy(g))
        tn = t.detach().numpy()
        assert_bitwise(((g * f32(hb)) * _one_minus_sq_fused(tn)) / f32(hb), xt.grad.numpy(), f"hb={hb}")
        d = np.abs(tanh_bound_backward_ref(g, tn, hb).astype(np.float64) - xt.grad.numpy())
        assert (d <= 7 * 2.0 ** -24 * np.abs(g)).all()   # + the two roundings of (g hb) / hb
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    y = torch.tanh(xt)
    y.backward(torch.from_numpy(g))
    yn = y.detach().numpy()
    assert_bitwise(g * _one_minus_sq_fused(yn), xt.grad.numpy(), "tanh")
    d = np.abs(tanh_backward_ref(g, yn).astype(np.float64) - xt.grad.numpy())
    assert (d <= 5 * 2.0 ** -24 * np.abs(g)).all()


def test_nan_clamp_torch_propagates_a_nan_replacement():
    """what the kernel is held to: with nan = NaN torch.clamp returns NaN (gradient 0)"""
    x = nan_clamp_inputs(64, 0)
    out, gx = nan_clamp_torch(x, np.ones(64, np.float32), *NAN_CLAMP_PARAMS[2])
    assert np.isnan(out[0]) and gx[0] == 0.0
    out, gx = nan_clamp_torch(x, np.ones(64, np.float32), *NAN_CLAMP_PARAMS[1])
    assert out[1] == 10.0 and out[2] == -10.0 and gx[1] == 0.0 and gx[2] == 0.0
