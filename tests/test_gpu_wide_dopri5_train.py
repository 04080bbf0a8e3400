"""MI355X: training through the device-resident dopri5 solve of the wide KAN-FET field — the ETT
forecaster's own training call, odeint(self.dynamics, z0, t_fut, method="dopri5") then
loss.backward() (train_kan_fet_ett.py:192, :312-335) — as one taped forward launch
(fetode_wide_dopri5_tape) and a device reverse sweep without read-backs
(fetode_wide_dopri5_backward), switched on by dopri5.set_resident_wide_training.

Checked: the taped forward is bitwise the untaped resident solve; the tape reproduces every
evaluation; the gradients against the oracle's fp64 autograd under the project's bar
(tests/test_gpu_dopri5_train.py _grad_bar, unchanged) and against autograd through the host-driven
solver (_Dopri5Grad), which runs the same VJP kernels; the tape-overflow re-run; the declines; the
forecaster end to end.  Shapes: the smallest admitted width pairs of tests/test_wide_shape_family.py,
(16, 32, 10) and (48, 16, 12) (D > H, K = 12; neither output width has the MFMA KANLinear VJP, so
the sweep takes the generic one as _Dopri5Grad does), B = 5 (one partial row tile) and B = 70
(across the 64-row tile); and the ETT widths (64, 128, 10), whose output widths take the MFMA
KANLinear VJP."""
import os

import numpy as np
import pytest
import torch

import fet_ode_amd as F
from fet_ode_amd import _lib, ett
from fet_ode_amd.autograd_ops import field_layers, wide_plan
from fet_ode_amd.dopri5 import ResidentSolve, _Dopri5Grad

pytestmark = pytest.mark.gpu

# (D, H, K, B, model seed, z0 scale, horizon, rtol, atol, options)
CASES = {
    "16-32 B5": (16, 32, 10, 5, 48, 0.6, 0.5, 1e-2, 1e-3, None),
    "48-16 B70 first_step": (48, 16, 12, 70, 64, 0.6, 0.5, 1e-2, 1e-3, {"first_step": 0.05}),
    "rejected": (16, 32, 10, 5, 48, 0.6, 0.7, 1e-3, 1e-4, None),
    # the ETT widths: both output widths (128, 64) take the MFMA KANLinear VJP in the sweep
    "64-128 B5": (64, 128, 10, 5, 7, 0.6, 0.3, 1e-2, 1e-3, None),
}


def _pin_field(net, seed):
    """The x 0.1 scaling of the untrained field as the ETT tests / bench do, with the spline weights
    redrawn from a seeded generator: the module's own come from a least-squares fit whose last bits
    differ from one construction to the next (and from process to process), every other tensor is
    reproducible under torch.manual_seed."""
    gen = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("spline_weight"):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.02)
            if n.endswith(("coef", "base_weight", "spline_weight", "logistic_weight")):
                p.mul_(0.1)


def _dyn(D, H, K, seed):
    """ett.KANFETDynamics, reproducible bit for bit in every construction (_pin_field)."""
    torch.manual_seed(seed)
    dyn = ett.KANFETDynamics(D, hidden=H, num_fet_basis=K)
    _pin_field(dyn.net, seed)
    return dyn


def _z0(B, D, scale, seed=3):
    return torch.randn(B, D, generator=torch.Generator().manual_seed(seed)) * scale


def _grid(T):
    return torch.tensor(np.linspace(0, T, 3))


def _weights(B, D, dtype=torch.float32):
    return torch.randn(3, B, D, generator=torch.Generator().manual_seed(0)).to(dtype)


class _switch:
    def __init__(self, on, tape_bytes=None):
        self.on, self.tb = on, tape_bytes

    def __enter__(self):
        self.prev = F.dopri5.set_resident_wide_training(self.on, self.tb)

    def __exit__(self, *exc):
        F.dopri5.set_resident_wide_training(self.prev, 16 << 30)
        return False


_RUNS, _ORACLE = {}, {}


class _rows:
    """FETODE_WIDE_BWD_ROWS for the sweeps inside (read per call by the workspace query and the sweep)."""

    def __init__(self, rows):
        self.rows = rows

    def __enter__(self):
        self.prev = os.environ.get("FETODE_WIDE_BWD_ROWS")
        if self.rows is not None:
            os.environ["FETODE_WIDE_BWD_ROWS"] = str(self.rows)

    def __exit__(self, *exc):
        if self.rows is not None:
            if self.prev is None:
                del os.environ["FETODE_WIDE_BWD_ROWS"]
            else:
                os.environ["FETODE_WIDE_BWD_ROWS"] = self.prev
        return False


def _run(name, dev, resident, rows=None):
    """loss = sum(w * solution): (loss, param grads, y0 grad, attempts, nfev), once per case and path;
    rows: the sweep's chunk row target (None: the default 8192, one chunk at these sizes)."""
    if rows is not None:
        with _rows(rows):
            return _run_once(name, dev, resident)
    if (name, resident) in _RUNS:
        return _RUNS[name, resident]
    _RUNS[name, resident] = _run_once(name, dev, resident)
    return _RUNS[name, resident]


def _run_once(name, dev, resident):
    D, H, K, B, seed, scale, T, rtol, atol, options = CASES[name]
    dyn = _dyn(D, H, K, seed).to(dev)
    y0 = _z0(B, D, scale).to(dev).requires_grad_(True)
    with _switch(resident):
        sol = F.odeint(dyn, y0, _grid(T), rtol=rtol, atol=atol, method="dopri5", options=options)
        s = F.dopri5.dopri5_solve.last
        assert isinstance(s, ResidentSolve if resident else _Dopri5Grad), type(s).__name__
        loss = (_weights(B, D).to(dev) * sol).sum()
        loss.backward()
    att = [(float(a[1]), bool(a[3])) for a in s.attempts]
    grads = {n: p.grad.detach().cpu().clone() for n, p in dyn.net.named_parameters()}
    return loss.item(), grads, y0.grad.cpu(), att, s.nfev


def _oracle(name, dtype, perturb):
    """The same loss through the oracle's autograd: (loss, grads, y0 grad, nfev), once per draw."""
    from oracle import torch_ref as O
    if (name, dtype, perturb) in _ORACLE:
        return _ORACLE[name, dtype, perturb]
    D, H, K, B, seed, scale, T, rtol, atol, options = CASES[name]
    dyn = _dyn(D, H, K, seed)
    sd = {k: v.clone() for k, v in dyn.net.state_dict().items()}
    names = [n for n, _ in dyn.net.named_parameters()]
    if perturb is not None:
        gen = torch.Generator().manual_seed(perturb)
        sd = {k: (v * (1 + 6e-8 * torch.randn(v.shape, generator=gen)) if k in names else v) for k, v in sd.items()}
    ps = {k: v.clone().to(dtype).requires_grad_(k in names) for k, v in sd.items()}
    ref = O.KANFETRef.from_state_dict(ps, 2)
    y0 = _z0(B, D, scale).to(dtype).requires_grad_(True)
    tr = O.Dopri5Trace()
    sol = O.odeint(lambda tt, yy: ref(yy), y0, _grid(T), rtol=rtol, atol=atol, method="dopri5", trace=tr,
                   options=options)
    loss = (_weights(B, D, dtype) * sol).sum()
    gr = torch.autograd.grad(loss, [ps[n] for n in names] + [y0])
    _ORACLE[name, dtype, perturb] = (loss.item(), dict(zip(names, gr[:-1])), gr[-1], tr.nfev, list(tr.attempts))
    return _ORACLE[name, dtype, perturb]


def _apart(d, ea, eh):
    """Two gradients of one fp64 value may lie as far apart as their two distances from it together
    (each within its own error of fp64, on opposite sides); no closer bound follows from both being
    right.  So 'within the larger of 1e-4 and the two paths' own distance from fp64' is
    d <= max(1e-4, ea + eh): a pair beyond it disagrees by more than both errors explain.  (Each
    distance alone as the bound was tried first and is not a property of two correct paths: at the
    forecaster's first iteration the sweep is 1.20e-4 and the host 4.8e-5 from fp64 on
    dynamics.net.layers.0.kan.base_weight and they are 1.28e-4 apart.)"""
    return d > max(1e-4, ea + eh)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


# ---------------------------------------------------------------------------------------------
# 1. forward identity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["16-32 B5", "48-16 B70 first_step"])
def test_taped_forward_is_bitwise_the_resident_solve(dev, name):
    """With the switch on and gradients required: solution, both layers' memory after the solve,
    nfev, attempt count, accept pattern and every (t0, dt, ratio) bitwise fetode_wide_dopri5's under
    no_grad — a first solve and a second one from the carried memory."""
    D, H, K, B, seed, scale, T, rtol, atol, options = CASES[name]
    t = torch.linspace(0.0, 3.0, steps=4)
    kw = dict(rtol=1e-3, atol=1e-4, method="dopri5", options=options)
    a, b = _dyn(D, H, K, seed).to(dev), _dyn(D, H, K, seed).to(dev)
    z0 = _z0(B, D, scale).to(dev)
    prev = F.dopri5.set_wide_resident_dopri5(True, gap=(0, 0))
    try:
        for z in (z0, z0 * 0.9):
            with _switch(True):
                sa = F.odeint(a, z.clone().requires_grad_(True), t, **kw)
                la = F.dopri5.dopri5_solve.last
                assert isinstance(la, ResidentSolve) and sa.requires_grad
            with torch.no_grad():
                sb = F.odeint(b, z, t, **kw)
                lb = F.dopri5.dopri5_solve.last
                assert isinstance(lb, ResidentSolve)
            print(f"taped vs untaped {name}: max |diff| {(sa.detach() - sb).abs().max().item():.3e}, nfev {la.nfev} / "
                  f"{lb.nfev}, attempts {la.n_attempts} / {lb.n_attempts}")
            assert torch.equal(sa.detach(), sb)
            for (_, fa), (_, fb) in zip(field_layers(a.net), field_layers(b.net)):
                assert torch.equal(fa._prev, fb._prev)
            assert la.nfev == lb.nfev and la.n_attempts == lb.n_attempts >= 3
            assert la.attempts == lb.attempts
    finally:
        F.dopri5.set_wide_resident_dopri5(prev, gap=(512, 8192))


# ---------------------------------------------------------------------------------------------
# 2. tape content
# ---------------------------------------------------------------------------------------------
def _layer(kan, fer, x, prev, reinit, dev):
    plan, kd, fd, _ = wide_plan(kan, fer, dev)
    out = torch.empty(x.shape[0], kan.out_features, device=dev)
    by = _lib.ctypes.byref
    _lib.check(_lib.load().fetode_wide_layer_forward(by(kd), by(fd), plan.data_ptr(), x.data_ptr(), x.shape[0],
                                                     _lib.ptr(prev), int(reinit), out.data_ptr(),
                                                     _lib.stream_handle(dev)), "fetode_wide_layer_forward")
    return out


@pytest.mark.parametrize("name", ["16-32 B5", "48-16 B70 first_step"])
def test_tape_reproduces_every_evaluation(dev, name):
    """x_0 = y0 bitwise; for every taped evaluation the two layer forwards of x_e with the memory
    x_{e-1} / h_{e-1} give h_e and k_e within 1e-6 of scale (the bar between the resident and the
    host arithmetic, tests/test_gpu_wide_dopri5.py _compare) — a first solve (first-call rule) and one
    from the carried memory (prev0 / prev1 as saved)."""
    D, H, K, B, seed, scale, T, rtol, atol, options = CASES[name]
    dyn = _dyn(D, H, K, seed).to(dev)
    (k0, f0), (k1, f1) = field_layers(dyn.net)
    z0 = _z0(B, D, scale).to(dev)
    for z in (z0, z0 * 0.9):
        with _switch(True):
            sol = F.odeint(dyn, z.clone().requires_grad_(True), _grid(T), rtol=1e-3, atol=1e-4, method="dopri5",
                           options=options)
        fn = sol.grad_fn
        tape, att, init_rec, *mem = fn.saved_tensors
        cap, n_ev = fn.cap, fn.n_ev
        assert n_ev == F.dopri5.dopri5_solve.last.nfev == (1 if options else 2) + 6 * fn.n_att
        xs = tape[:cap * B * D].view(cap, B, D)
        hs = tape[cap * B * D:cap * B * (D + H)].view(cap, B, H)
        ks = tape[cap * B * (D + H):].view(cap, B, D)
        assert torch.equal(xs[0], z)
        p0, p1 = (mem + [None, None])[:2] if mem else (None, None)
        assert (p0 is None) == (p1 is None) == (z is z0)
        worst = 0.0
        for e in range(n_ev):
            h = _layer(k0, f0, xs[e], p0 if e == 0 else xs[e - 1], e == 0 and p0 is None, dev)
            k = _layer(k1, f1, hs[e], p1 if e == 0 else hs[e - 1], e == 0 and p1 is None, dev)
            for got, want in ((hs[e], h), (ks[e], k)):
                err = (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)
                worst = max(worst, err)
        print(f"tape {name}: {n_ev} evaluations, worst / 1e-6 scale {worst / 1e-6:.3f}")
        assert worst <= 1e-6, worst
        # the memory after the solve is the last evaluation's inputs
        assert torch.equal(f0._prev, xs[n_ev - 1]) and torch.equal(f1._prev, hs[n_ev - 1])


# ---------------------------------------------------------------------------------------------
# 3. gradients against the fp64 oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_gradients_vs_oracle_fp64(dev, name):
    """Per tensor and for y0: <= max(1e-4, 2 x the host path's error, 2 x the worst fp32 control's)
    (_grad_bar of tests/test_gpu_dopri5_train.py, perturbations [None, 1, 2, 3]); nfev the oracle's;
    the loss within 1e-5.  And against _Dopri5Grad, which runs the same VJP kernels: per tensor
    within the larger of 1e-4 and the two paths' own distance from fp64 (_apart).

    "rejected": model seed 48, z0 = 0.6 N(0, 1) (generator seed 3), t = linspace(0, 0.7, 3), rtol 1e-3
    / atol 1e-4, chosen on the CPU from the fp64 oracle alone.  Its trace: 68 evaluations, 11
    attempts; seven accepted steps up to t = 0.545 (error ratios 0.24 .. 0.80), then dt = 0.0815
    REJECTED at ratio 1.155, then dt = 0.0713, 0.0713, 0.0731 accepted (ratios 0.61, 0.52, 0.63) to
    t = 0.7607.  The fp32 oracle and its three re-roundings take the same 68 evaluations.  Asserted
    below: at least one rejected and three accepted attempts, and the fp32 control's nfev."""
    from test_gpu_dopri5_train import _grad_bar
    l64, g64, y64, n64, att64 = _oracle(name, torch.float64, None)
    if name == "rejected":
        acc = [bool(a[3]) for a in att64]
        assert acc.count(False) >= 1 and acc.count(True) >= 3, acc
        assert _oracle(name, torch.float32, None)[3] == n64
    got = _grad_bar(f"wide {name}", lambda resident: _run(name, dev, resident),
                    lambda dtype, pert: _oracle(name, dtype, pert)[:4], 1e-4, 1e-5, [None, 1, 2, 3])
    assert [a[1] for a in got[3]] == [bool(a[3]) for a in att64]
    host = _run(name, dev, False)
    assert host[4] == got[4]
    bad = {}
    for n in list(g64) + ["y0"]:
        a, h, o = (got[2], host[2], y64) if n == "y0" else (got[1][n], host[1][n], g64[n])
        d, ea, eh = _rel(a, h), _rel(a, o), _rel(h, o)
        if _apart(d, ea, eh):
            bad[n] = (d, ea, eh)
    assert not bad, f"(sweep vs host, sweep vs fp64, host vs fp64): {bad}"


# rows target -> attempts per chunk A = max(1, (rows + 3 B) // (6 B)), chunks counted from the last attempt:
#   "rejected" (B = 5, 11 attempts), rows 120: A = 4 -> chunks of 4, 4 and a shorter earliest one of 3
#   "48-16 B70 first_step" (B = 70, 5 attempts), rows 840: A = 2 -> 2, 2, 1;  rows 1: A = 1 -> 5 chunks
#   "64-128 B5" (the MFMA KANLinear VJP), rows 60: A = 2
@pytest.mark.parametrize("name,rows,chunks", [("rejected", 120, [4, 4, 3]), ("48-16 B70 first_step", 840, [2, 2, 1]),
                                              ("48-16 B70 first_step", 1, [1, 1, 1, 1, 1]), ("64-128 B5", 60, None)])
def test_gradients_over_several_chunks(dev, name, rows, chunks):
    """The sweep with a small row target (FETODE_WIDE_BWD_ROWS): several chunks of whole attempts, a
    shorter earliest one, accumulation across chunks — under the same bars as the one-chunk sweep:
    _grad_bar against the fp64 oracle, and per tensor against _Dopri5Grad within the larger of 1e-4
    and either path's own distance from fp64.  Parameter sums that missed a chunk, counted one twice
    or read the wrong planes are off by O(1 / chunks), far beyond either bar.  The chunked gradients
    differ from the one-chunk sweep's by the parameter sums' order only: per tensor under that same
    bar (_apart: the larger of 1e-4 and the two sweeps' own distance from fp64), and y0's, which no chunk boundary
    touches, bitwise."""
    from test_gpu_dopri5_train import _grad_bar
    B = CASES[name][3]
    A = max(1, (rows + 3 * B) // (6 * B))
    l64, g64, y64, n64, att64 = _oracle(name, torch.float64, None)
    n_att = len(att64)
    if chunks is not None:
        want, hi = [], n_att
        while hi > 0:
            want.append(hi - max(0, hi - A))
            hi -= A
        assert want == chunks, (want, n_att, A)
    assert -(-n_att // A) >= 3 or chunks is None
    got = _grad_bar(f"wide {name} rows={rows}", lambda resident: _run(name, dev, resident, rows if resident else None),
                    lambda dtype, pert: _oracle(name, dtype, pert)[:4], 1e-4, 1e-5, [None, 1, 2, 3])
    host, one = _run(name, dev, False), _run(name, dev, True)
    bad = {}
    for n in list(g64) + ["y0"]:
        a, h, o, u = (got[2], host[2], y64, one[2]) if n == "y0" else (got[1][n], host[1][n], g64[n], one[1][n])
        d, ea, eh, du = _rel(a, h), _rel(a, o), _rel(h, o), _rel(a, u)
        if _apart(d, ea, eh) or _apart(du, ea, _rel(u, o)):
            bad[n] = (d, ea, eh, du)
    print(f"chunked {name} rows={rows}: worst vs one chunk {max(_rel(got[1][n], one[1][n]) for n in g64):.2e}")
    assert not bad, f"(chunked vs host, vs fp64, host vs fp64, chunked vs one chunk): {bad}"
    assert torch.equal(got[2], one[2])


def test_rerun_beyond_the_tape_budget_declines(dev):
    """A budget that admits the guessed tape (4 evaluations) but not the solve's: the taped solve
    overflows, the pre-solve memory is restored and the solve is _Dopri5Grad's — solution, memory and
    gradients bitwise those with the switch off; the next call declines before any launch."""
    D, H, K, B, seed, scale, T, rtol, atol, options = CASES["16-32 B5"]
    out = []
    for on in (False, True):
        dyn = _dyn(D, H, K, seed).to(dev)
        budget = None
        if on:
            dyn._fetode_wide_d5tape = (4, 1)
            (k0, f0), (k1, f1) = field_layers(dyn.net)
            e0, e1 = wide_plan(k0, f0, dev), wide_plan(k1, f1, dev)
            by = _lib.ctypes.byref
            budget = 4 * B * (2 * D + H) * 4 + _lib.load().fetode_wide_dopri5_backward_workspace(
                by(e0[1]), by(e0[2]), by(e1[1]), by(e1[2]), B, 1)
        res = []
        for mul in (1.0, 0.9):
            y0 = (_z0(B, D, scale) * mul).to(dev).requires_grad_(True)
            with _switch(on, budget):
                sol = F.odeint(dyn, y0, _grid(T), rtol=rtol, atol=atol, method="dopri5")
                assert isinstance(F.dopri5.dopri5_solve.last, _Dopri5Grad)
                for p in dyn.parameters():
                    p.grad = None
                (_weights(B, D).to(dev) * sol).sum().backward()
            res.append((sol.detach().clone(), [p.grad.clone() for p in dyn.net.parameters()], y0.grad.clone(),
                        [f._prev.clone() for _, f in field_layers(dyn.net)]))
        if on:
            assert dyn._fetode_wide_d5tape[0] > 4
        out.append(res)
    for (s0, g0, y0g, m0), (s1, g1, y1g, m1) in zip(*out):
        assert torch.equal(s0, s1) and torch.equal(y0g, y1g)
        assert all(torch.equal(a, b) for a, b in zip(g0, g1))
        assert all(torch.equal(a, b) for a, b in zip(m0, m1))


def test_second_backward_gives_the_same_gradients(dev):
    D, H, K, B, seed, scale, T, rtol, atol, options = CASES["16-32 B5"]
    dyn = _dyn(D, H, K, seed).to(dev)
    y0 = _z0(B, D, scale).to(dev).requires_grad_(True)
    with _switch(True):
        sol = F.odeint(dyn, y0, _grid(T), rtol=rtol, atol=atol, method="dopri5")
    loss = (_weights(B, D).to(dev) * sol).sum()
    ps = list(dyn.net.parameters()) + [y0]
    g1 = torch.autograd.grad(loss, ps, retain_graph=True)
    g2 = torch.autograd.grad(loss, ps)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert all(torch.isfinite(a).all() and a.any() for a in g1)


# ---------------------------------------------------------------------------------------------
# 4. tape overflow
# ---------------------------------------------------------------------------------------------
def test_tape_overflow_reruns_bitwise(dev):
    """func._fetode_wide_d5tape = (4, 1) is below the solve's evaluations and attempts: the forward
    re-runs from the saved memory with room — solution, memory and gradients bitwise a roomy run's;
    a first solve and one from the carried memory."""
    D, H, K, B, seed, scale, T, rtol, atol, options = CASES["16-32 B5"]
    out = []
    for cap in (None, (4, 1)):
        dyn = _dyn(D, H, K, seed).to(dev)
        res = []
        for mul in (1.0, 0.9):
            if cap is not None:
                dyn._fetode_wide_d5tape = cap
            y0 = (_z0(B, D, scale) * mul).to(dev).requires_grad_(True)
            with _switch(True):
                sol = F.odeint(dyn, y0, _grid(T), rtol=rtol, atol=atol, method="dopri5")
                assert isinstance(F.dopri5.dopri5_solve.last, ResidentSolve)
                assert F.dopri5.dopri5_solve.last.nfev > 4
                for p in dyn.parameters():
                    p.grad = None
                (_weights(B, D).to(dev) * sol).sum().backward()
            res.append((sol.detach().clone(), [p.grad.clone() for p in dyn.net.parameters()], y0.grad.clone(),
                        [f._prev.clone() for _, f in field_layers(dyn.net)]))
        out.append(res)
    for (s0, g0, y0g, m0), (s1, g1, y1g, m1) in zip(*out):
        assert torch.equal(s0, s1) and torch.equal(y0g, y1g)
        assert all(torch.equal(a, b) for a, b in zip(g0, g1))
        assert all(torch.equal(a, b) for a, b in zip(m0, m1))


# ---------------------------------------------------------------------------------------------
# 5. declines
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why", ["off", "D=24", "reversed", "tape_bytes"])
def test_declines_take_host_autograd(dev, why):
    """Switch off (the default), D = 24 (no wide kernel for layer 1), reversed t, tape_bytes = 1: the
    solve is _Dopri5Grad's and the gradients are finite.  options["norm_group"] is declined by
    _scalar_request (it is no scalar option) but has no case here: with it _Dopri5Grad all-reduces
    every norm over the group, which needs an initialised process group."""
    D, H, K, B = (24, 48, 12, 5) if why == "D=24" else (16, 32, 10, 5)
    dyn = _dyn(D, H, K, 48).to(dev)
    y0 = _z0(B, D, 0.6).to(dev).requires_grad_(True)
    t = _grid(0.5)
    if why == "reversed":
        t = t.flip(0)
    with _switch(why != "off", 1 if why == "tape_bytes" else None):
        sol = F.odeint(dyn, y0, t, rtol=1e-2, atol=1e-3, method="dopri5")
        assert isinstance(F.dopri5.dopri5_solve.last, _Dopri5Grad)
        sol.square().sum().backward()
    assert torch.isfinite(y0.grad).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in dyn.net.parameters())


# ---------------------------------------------------------------------------------------------
# 6. forecaster end to end
# ---------------------------------------------------------------------------------------------
def _forecaster_oracle(sd, names, states, xb, yb, t, rtol, atol):
    """The forecaster's loss.backward() through the oracle in fp64 (train_kan_fet_ett.py:155-197 with
    the dopri5 latent solve): {name: gradient}, nfev, and the field's hysteresis states afterwards."""
    import torch.nn.functional as Fn
    from oracle import torch_ref as O
    ps = {k: v.detach().cpu().double().clone().requires_grad_(k in names) for k, v in sd.items()}
    field = O.KANFETRef.from_state_dict({k[len("dynamics.net."):]: v for k, v in ps.items()
                                         if k.startswith("dynamics.net.")}, 2)
    if states is not None:
        field.states = states
    h = Fn.relu(Fn.linear(xb.cpu().double().flatten(1), ps["encoder.1.weight"], ps["encoder.1.bias"]))
    z0 = Fn.linear(h, ps["encoder.3.weight"], ps["encoder.3.bias"])
    tr = O.Dopri5Trace()
    zt = O.odeint(lambda tt, zz: field(zz), z0, t.cpu().double(), rtol=rtol, atol=atol, method="dopri5", trace=tr)
    d = Fn.relu(Fn.linear(zt, ps["decoder.0.weight"], ps["decoder.0.bias"]))
    y = Fn.linear(d, ps["decoder.2.weight"], ps["decoder.2.bias"]).squeeze(-1).transpose(0, 1)
    loss = torch.mean((y - yb.cpu().double()) ** 2)
    gr = torch.autograd.grad(loss, [ps[n] for n in names])
    for st in field.states:
        st.prev_x = st.prev_x.detach()
    return dict(zip(names, gr)), tr.nfev, field.states


def test_forecaster_training_iterations_agree_with_host_autograd(dev):
    """ett forecaster, dopri5, latent 16, hidden 32, B = 5, 8 -> 3: loss.backward() with the switch
    on and off — every parameter gradient (encoder's and head's included) agrees under the bar of
    the sweep-vs-host check above: per tensor within the larger of 1e-4 and the two paths' own
    distance from the fp64 oracle of the same iteration — then clip_grad_norm_(1.0) and one AdamW
    step; a second iteration, from the carried hysteresis memory and the stepped parameters, agrees
    again (the plans follow the parameter versions)."""
    def make(sd=None):
        torch.manual_seed(11)
        m = ett.LatentNeuralODEForecaster(num_features=3, context_len=8, pred_len=3, latent_dim=16, enc_hidden=32,
                                          dec_hidden=32, dyn_hidden=32, solver="dopri5", rtol=1e-2, atol=1e-3)
        _pin_field(m.dynamics.net, 11)   # reproducible in every process
        if sd is not None:
            m.load_state_dict(sd)
        return m.to(dev)

    g = torch.Generator().manual_seed(5)
    xb = torch.randn(5, 8, 3, generator=g).to(dev)
    yb = torch.randn(5, 3, generator=g).to(dev)
    t_fut = torch.linspace(0.0, 2.0, steps=3).to(dev)
    first = make()
    ms = {True: first, False: make({k: v.clone() for k, v in first.state_dict().items()})}
    names = [n for n, _ in first.named_parameters()]
    opt = {k: torch.optim.AdamW(m.parameters(), lr=1e-3) for k, m in ms.items()}
    states = None
    for it in range(2):
        g64, n64, states = _forecaster_oracle(ms[True].state_dict(), names, states, xb, yb, t_fut, 1e-2, 1e-3)
        grads = {}
        for on, m in ms.items():
            opt[on].zero_grad(set_to_none=True)
            with _switch(on):
                loss = torch.nn.functional.mse_loss(m(xb, t_fut), yb)
                assert isinstance(F.dopri5.dopri5_solve.last, ResidentSolve if on else _Dopri5Grad)
                loss.backward()
            grads[on] = (loss.item(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()},
                         F.dopri5.dopri5_solve.last.nfev)
        (l1, g1, n1), (l0, g0, n0) = grads[True], grads[False]
        assert n1 == n0 == n64 and abs(l1 - l0) <= 1e-5 * abs(l0) + 1e-7, (it, n1, n0, n64, l1, l0)
        bad = {}
        for n in names:
            d, ea, eh = _rel(g1[n], g0[n]), _rel(g1[n], g64[n]), _rel(g0[n], g64[n])
            if _apart(d, ea, eh):
                bad[n] = (d, ea, eh)
        print(f"forecaster iteration {it}: nfev {n1}, worst sweep vs host {max(_rel(g1[n], g0[n]) for n in names):.2e}, "
              f"sweep vs fp64 {max(_rel(g1[n], g64[n]) for n in names):.2e}, "
              f"host vs fp64 {max(_rel(g0[n], g64[n]) for n in names):.2e}")
        assert not bad, f"iteration {it} (sweep vs host, sweep vs fp64, host vs fp64): {bad}"
        for on, m in ms.items():
            torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
            opt[on].step()
        # the next iteration compares gradients at ONE set of parameters (AdamW's normalised step turns
        # the paths' 1e-4 gradient difference into different parameters): the sweep model's own step
        with torch.no_grad():
            for p0, p1 in zip(ms[False].parameters(), ms[True].parameters()):
                p0.copy_(p1)
