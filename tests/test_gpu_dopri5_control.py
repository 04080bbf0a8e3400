"""The degenerate branches of the dopri5 step control, on every solver that re-implements it.

The host-driven loop (dopri5.py _Dopri5 / _Dopri5Grad) and the device-resident solvers — the
[2, 10, 2] kernels under both kernel switches, fieldn ([3, 8, 3], K = 6), the wide solve
(32 -> 64 -> 32) and the ECG solve (latent 5, 7 bases), with the reverse sweeps of the first, second
and last — each carry their own copy of misc._select_initial_step and rk_common._optimal_step_size.
The ordinary solves of the other modules never reach:

  (a) a zero field: d1 < 1e-5 -> h0 = 1e-6; d1, d2 <= 1e-15 -> h1 = max(1e-6, h0 1e-3); every
      attempt's error ratio exactly 0 -> dt * ifactor (a sweep that forms er^(-1/5) anyway makes
      inf * 0);
  (b) y0 = 0 exactly: d0 < 1e-5 -> h0 = 1e-6, first step 100 h0;
  (c) training through (a) and (b);
  (d) the per-output-interval max_num_steps count and its status 3;
  (e) non-default safety / ifactor / dfactor;
  (f) min_step / max_step that bind.

Reference: the oracle (oracle/torch_ref.py, torchdiffeq restated, whose options forward
max_num_steps / safety / ifactor / dfactor) in fp32 on the CPU for traces and solutions — under
the bars of tests/test_gpu_dopri5.py's trace tests as stated: the same accept pattern and nfev, dt
within 1e-3, error ratios within 1e-2 (+1e-6), each output slice within 1e-4; a case is admitted
only if the oracle's own fp32 / fp64 / re-rounded runs agree to half of each bar (reference()).  One
loosening against those tests: error ratios under (safety / ifactor)^5 — 5.9e-6 by default, 3.2e-4
with case (e)'s options — are clipped to it before they are compared: below it the controller
ignores the ratio (the factor is capped at ifactor, and dt has its own bar), and such a ratio is
rounding noise of the error estimate's cancelling sum.  Gradients: the oracle's fp64 autograd under
tests/test_gpu_dopri5_train.py's bar (_grad_bar, unchanged).  The oracle has no min_step / max_step,
so (f) pins the resident solvers to the host-driven loop: kernel to kernel only.  Every oracle
solve is computed once per case and shared by the paths."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from conftest import golden_sd, load_golden

pytestmark = pytest.mark.gpu

# (rtol, atol) per field.  From y0 = 0 the first step is 1e-4, where a KAN-FET field's error estimate
# is at rounding level; at rtol 1e-3 its ratio still lies above (safety / ifactor)^5, so that noise
# goes straight into the next dt and the oracle's own fp32 runs differ by more than the trace bars
# (reference() refuses such a case).  The golden KAN-FET and fieldn fields therefore run at looser
# tolerances, where those first ratios fall under the cap and dt grows by exactly x ifactor.
TOL = {"kan": (1e-3, 1e-4), "kanfet": (3e-2, 3e-3), "fieldn": (1e-1, 1e-2), "wide": (1e-3, 1e-4), "ecg": (1e-3, 1e-4)}
H0 = float(np.float32(1e-6))                          # 9.999999974752427e-07
H0_100 = float(np.float32(100) * np.float32(1e-6))    # 9.999999747378752e-05


# ---- the fields ---------------------------------------------------------------------------------

class Field:
    """One vector field: its fp32 state dict (built once), the GPU module and the oracle from it."""
    kind = "kan"          # kan | kanfet | ecg
    zero_keys = ()        # the output layer's tensors: zeroed, the field is exactly 0

    @functools.lru_cache(maxsize=None)
    def sd(self):
        return {k: v.clone() for k, v in self._sd().items()}

    def sd_zero(self):
        sd = {k: v.clone() for k, v in self.sd().items()}
        hit = [k for k in sd if any(k.endswith(z) for z in self.zero_keys)]
        assert hit
        for k in hit:
            sd[k].zero_()
        return sd

    def y0(self, B):
        raise NotImplementedError

    def func(self, m):
        import fet_ode_amd as F
        return F.autonomous(m)

    def gpu_state(self, m):
        return [l.ferro._prev.detach().cpu() for l in m.layers] if self.kind == "kanfet" else []

    def oracle(self, sd):
        from oracle import torch_ref as O
        if self.kind == "kan":
            ref = O.KANRef([O.KANLinearParams.from_state_dict(sd, f"layers.{l}.") for l in range(2)])
        else:
            ref = O.KANFETRef.from_state_dict(sd, 2)
        return ref, (lambda tt, yy: ref(yy))

    def oracle_state(self, ref):
        return [s.prev_x[:, :, 0, 0].clone() for s in ref.states] if self.kind == "kanfet" else []

    def param_names(self):
        return [n for n, _ in self.module().named_parameters()]


class Golden2102(Field):
    """the LV [2, 10, 2] fields with the golden weights (tests/golden/traj_kan*.npz)"""

    def __init__(self, kind):
        self.kind = kind
        self.zero_keys = ("layers.1.base_weight", "layers.1.spline_weight", "layers.1.logistic_weight",
                          "layers.1.kan.base_weight", "layers.1.kan.spline_weight", "layers.1.kan.logistic_weight",
                          "layers.1.ferro.coef")

    def _g(self):
        return load_golden("traj_kanfet" if self.kind == "kanfet" else "traj_kan")

    def _sd(self):
        return golden_sd(self._g())

    def module(self):
        import fet_ode_amd as F
        return (F.KANFET if self.kind == "kanfet" else F.KAN)([2, 10, 2], grid_size=5)

    def y0(self, B):
        return torch.from_numpy(self._g()["y0_B64"])[:B].clone()


class FieldN(Field):
    """KANFET([3, 8, 3], K = 6): no specialised kernel, fieldn's driver and sweep"""
    kind = "kanfet"
    zero_keys = ("layers.1.kan.base_weight", "layers.1.kan.spline_weight", "layers.1.kan.logistic_weight",
                 "layers.1.ferro.coef")

    def module(self):
        import fet_ode_amd as F
        torch.manual_seed(0)
        return F.KANFET([3, 8, 3], grid_size=5, num_fet_basis=6)

    def _sd(self):
        return self.module().state_dict()

    def y0(self, B):
        return 0.5 + 2.0 * torch.rand(B, 3, generator=torch.Generator().manual_seed(7))


class Wide(Field):
    """ett.KANFETDynamics(32, hidden 64, K = 12): the smallest width pair of the wide resident solve"""
    kind = "kanfet"
    zero_keys = ("layers.1.kan.base_weight", "layers.1.kan.spline_weight", "layers.1.kan.logistic_weight",
                 "layers.1.ferro.coef")

    def module(self):
        from fet_ode_amd import ett
        torch.manual_seed(5)
        return ett.KANFETDynamics(32, hidden=64, num_fet_basis=12)

    def _sd(self):
        return self.module().state_dict()

    def func(self, m):
        return m

    def y0(self, B):
        return torch.randn(B, 32, generator=torch.Generator().manual_seed(9)) * 0.4

    def gpu_state(self, m):
        return [l.ferro._prev.detach().cpu() for l in m.net.layers]

    def oracle(self, sd):
        return super().oracle({k[len("net."):]: v for k, v in sd.items() if k.startswith("net.")})


class Ecg(Field):
    """ecg.No_MLP_KANODEFunc(latent 5, 7 bases): the ECG resident solve and sweep"""
    kind = "ecg"
    zero_keys = ("proj.weight", "proj.bias")

    seed = 32   # a seed whose y0 = 0 solve keeps its gate decisions under fp32 re-rounding (reference())

    def module(self):
        from fet_ode_amd import ecg
        torch.manual_seed(self.seed)
        return ecg.No_MLP_KANODEFunc(latent_dim=5, num_basis=7)

    def _sd(self):
        return self.module().state_dict()

    def func(self, m):
        return m

    def y0(self, B):
        return torch.randn(B, 5, generator=torch.Generator().manual_seed(1003)) * 2.0

    def gpu_state(self, m):
        return [m.feat.basis.prev_x.detach().cpu().reshape(-1)]

    def oracle(self, sd):
        from oracle import ecg_ref as E
        ref = E.ECGFieldRef.from_state_dict(sd)
        return ref, ref

    def oracle_state(self, ref):
        return [ref.basis.prev_x.reshape(-1).clone()]


FIELDS = {"kan": Golden2102("kan"), "kanfet": Golden2102("kanfet"), "fieldn": FieldN(), "wide": Wide(), "ecg": Ecg()}

# path -> (field, how the solve is routed)
PATHS = {
    "host-kan": ("kan", "host"), "host-kanfet": ("kanfet", "host"),
    "v4-kan": ("kan", "v4"), "v6-kan": ("kan", "v6"), "v4-kanfet": ("kanfet", "v4"), "v6-kanfet": ("kanfet", "v6"),
    "fieldn": ("fieldn", "resident"), "fieldn-host": ("fieldn", "host"),
    "wide": ("wide", "wide"), "wide-host": ("wide", "wide-host"),
    "ecg": ("ecg", "resident"), "ecg-host": ("ecg", "host"),
}
RESIDENT = [p for p, (_, r) in PATHS.items() if "host" not in r]
HOST_OF = {"v4-kan": "host-kan", "v6-kan": "host-kan", "v4-kanfet": "host-kanfet", "v6-kanfet": "host-kanfet",
           "fieldn": "fieldn-host", "wide": "wide-host", "ecg": "ecg-host"}


@contextlib.contextmanager
def routed(route, kernel_switch, small=False):
    """host: the host-driven loop (small: its [2, 10, 2] evaluations on the small-batch kernel, to
    pair with v6); v4 / v6: the resident [2, 10, 2] solve on the two-per-wave / small-batch kernel;
    wide: the wide resident solve at every batch."""
    from fet_ode_amd import dopri5 as D5
    prev = D5.set_resident_dopri5(route not in ("host", "wide-host"))
    prev_w = D5.set_wide_resident_dopri5(route == "wide", gap=(0, 0))
    try:
        if route in ("v4", "v6", "host"):
            kernel_switch(route == "v6" or (route == "host" and small))
        yield
    finally:
        D5.set_resident_dopri5(prev)
        D5.set_wide_resident_dopri5(prev_w, gap=(512, 8192))


def gpu_solve(path, sd, y0, t, dev, kernel_switch, options=None, module=None, small=False):
    """-> (solution, attempts, nfev, hysteresis state, module); asserts the path taken"""
    import fet_ode_amd as F
    from fet_ode_amd.dopri5 import ResidentSolve
    fld, route = PATHS[path]
    field = FIELDS[fld]
    if module is None:
        module = field.module()
        module.load_state_dict(sd)
        module = module.to(dev)
    with routed(route, kernel_switch, small), torch.no_grad():
        rtol, atol = TOL[fld]
        sol = F.odeint(field.func(module), y0.to(dev), t, method="dopri5", rtol=rtol, atol=atol, options=options)
        s = F.dopri5.dopri5_solve.last
    assert isinstance(s, ResidentSolve) == ("host" not in route), (path, type(s).__name__)
    att = [(float(a[0]), float(a[1]), float(a[2]), bool(a[3])) for a in s.attempts]
    return sol.cpu(), att, s.nfev, field.gpu_state(module), module


_ORACLE = {}


def oracle_solve(fld, case, B, t, options=None, dtype=torch.float32, perturb=None):
    """The oracle's solve of (field, case, B), computed once: solution, trace, hysteresis state.
    case: 'zero' (the zeroed output layer), 'y0zero' (y0 = 0), 'plain'.  dtype / perturb: the
    yardstick draws of reference() — fp64, or fp32 with every parameter scaled by 1 + 6e-8 N(0, 1)
    from generator seed `perturb`, an equally valid fp32 rounding of the same model (as
    tests/test_gpu_dopri5_train.py::_oracle)."""
    from oracle import torch_ref as O
    key = (fld, case, B, tuple(float(v) for v in t), tuple(sorted((options or {}).items())), dtype, perturb)
    if key not in _ORACLE:
        field = FIELDS[fld]
        sd, y0 = case_inputs(fld, case, B)
        if perturb is not None:
            gen, names = torch.Generator().manual_seed(perturb), field.param_names()
            sd = {k: (v * (1 + 6e-8 * torch.randn(v.shape, generator=gen)) if k in names else v) for k, v in sd.items()}
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        ref, f = field.oracle(sd)
        tr = O.Dopri5Trace()
        with torch.no_grad():
            sol = O.odeint(f, y0.to(dtype), t, rtol=TOL[fld][0], atol=TOL[fld][1], method="dopri5", options=options,
                           trace=tr)
        _ORACLE[key] = (sol, tr, field.oracle_state(ref))
    return _ORACLE[key]


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _slice_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm(dim=(1, 2)) / b.norm(dim=(1, 2)).clamp_min(1e-30)).max().item()


def _trace_err(att, exp, floor):
    """largest relative difference of the step sizes and of the error ratios of two attempt logs;
    ratios below `floor` = (safety / ifactor)^5 are clipped to it: under it the step control
    ignores the ratio (the factor is capped at ifactor), and a ratio of 1e-8 is rounding noise of
    the error estimate's cancelling sum"""
    dt = max(abs(a[1] - b[1]) / abs(b[1]) for a, b in zip(att, exp))
    r = max(max(abs(max(a[2], floor) - max(b[2], floor)) - 1e-6, 0.0) / max(b[2], floor) for a, b in zip(att, exp))
    return dt, r


_REFERENCE = {}


def reference(fld, case, B, t, options=None):
    """The fp32 oracle solve a path is compared with, and the proof that the case can carry the
    bars of assert_trace: the oracle itself must hold them with a factor 2 to spare under fp32
    rounding — its fp32 run against its fp64 run and against three fp32 re-roundings of the
    parameters, each with the same accept pattern.  The adaptive control amplifies rounding (dt ~
    ratio^(-1/5), the hysteresis gates); a case where the reference's own arithmetic moves by half a
    bar is no test of a path, and is refused here (choose another grid, tolerance or seed) — the
    bars themselves never widen."""
    key = (fld, case, B, tuple(float(v) for v in t), tuple(sorted((options or {}).items())))
    if key in _REFERENCE:
        return _REFERENCE[key]
    sol, tr, state = oracle_solve(fld, case, B, t, options)
    o = options or {}
    floor = (o.get("safety", 0.9) / o.get("ifactor", 10.0)) ** 5
    yard = {"dt": 0.0, "ratio": 0.0, "sol": 0.0, "state": 0.0}
    for dtype, pert in ((torch.float64, None), (torch.float32, 1), (torch.float32, 2), (torch.float32, 3)):
        s2, tr2, st2 = oracle_solve(fld, case, B, t, options, dtype, pert)
        assert [a[3] for a in tr2.attempts] == [a[3] for a in tr.attempts], \
            f"{key}: the oracle's own accept pattern changes under fp32 rounding ({dtype}, {pert})"
        dt, r = _trace_err(tr.attempts, tr2.attempts, floor)
        yard["dt"], yard["ratio"] = max(yard["dt"], dt), max(yard["ratio"], r)
        yard["sol"] = max(yard["sol"], _slice_err(sol, s2))
        yard["state"] = max([yard["state"]] + [_rel(a, b) for a, b in zip(state, st2)])
    for name, bar in BARS.items():
        assert 2 * yard[name] <= bar, f"{key}: the oracle's own fp32 spread of {name}, {yard[name]:.2e}, is over half the bar"
    _REFERENCE[key] = dict(sol=sol, tr=tr, state=state, yard=yard, floor=floor)
    return _REFERENCE[key]


def case_inputs(fld, case, B):
    field = FIELDS[fld]
    sd = field.sd_zero() if case == "zero" else field.sd()
    y0 = field.y0(B)
    return sd, (torch.zeros_like(y0) if case == "y0zero" else y0)


def per_interval(attempts, t):
    """attempts inside each output interval, as the solvers count them for max_num_steps: the loop
    for output i runs while t[i] > t1 of the last accepted step"""
    counts, t1, i = [0] * (len(t) - 1), float(t[0]), 1
    for t0, dt, _, acc in attempts:
        while i < len(t) and not float(t[i]) > t1:
            i += 1
        counts[i - 1] += 1
        if acc:
            t1 = t0 + dt
    return counts


# dt, error ratio (+1e-6) and output slices: the bars of test_dopri5_kanfet_trace
# (tests/test_gpu_dopri5.py).  The hysteresis memory after the solve is the LAST attempt's last stage
# input, y + dt sum_j beta_j k_j at t0 + dt — past the last output time, so it moves with that
# attempt's dt and gets dt's bar; with dt exact (the zero field) test_zero_field passes the 1e-5 of
# one field evaluation (tests/test_gpu_fieldn.py::test_fieldn_single_eval_and_state).
BARS = {"dt": 1e-3, "ratio": 1e-2, "sol": 1e-4, "state": 1e-3}


def assert_trace(att, nfev, sol, state, R, what, mem_tol=BARS["state"]):
    """Against reference(): the same attempts, accept pattern and nfev, and BARS as stated."""
    exp = R["tr"].attempts
    assert len(att) == len(exp), (what, len(att), len(exp))
    assert [a[3] for a in att] == [a[3] for a in exp], what
    assert nfev == R["tr"].nfev, (what, nfev, R["tr"].nfev)
    dt, r = _trace_err(att, exp, R["floor"])
    assert dt <= BARS["dt"], (what, "dt", dt, R["yard"])
    assert r <= BARS["ratio"], (what, "error ratio", r, R["yard"])
    err = _slice_err(sol, R["sol"])
    assert err <= BARS["sol"], (what, "solution", err, R["yard"])
    if state is not None:
        assert len(state) == len(R["state"])
        for a, b in zip(state, R["state"]):
            assert a.shape == b.shape, (what, a.shape, b.shape)
            assert _rel(a, b) <= mem_tol, (what, "hysteresis memory", _rel(a, b), R["yard"])


def _grid(T, n):
    return torch.tensor(np.linspace(0, T, n))


T_SHORT = _grid(0.5, 3)     # (a): the zero field takes its seven x 10 steps on any of them
# (b), (d), (e), (f): five output times per field.  The smooth fields take the LV horizon; the
# KAN-FET fields short ones (the hysteresis gates make long attempt sequences a matter of fp32
# rounding, as in test_dopri5_kanfet_trace) — the wide field from its random init is stiff.  On
# these grids reference() accepts every case below, and every oracle error ratio stays >= 15 % away
# from 1 (measured on the CPU), so an accept / reject decision never hangs on fp32 rounding.
GRID = {"kan": _grid(2.0, 5), "kanfet": _grid(0.02, 5), "fieldn": _grid(0.2, 5), "wide": _grid(0.005, 5),
        "ecg": _grid(2.0, 5)}


# ---- (a) the zero field -------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("path", [p for p in PATHS if p in RESIDENT or p.startswith("host-")])
def test_zero_field(dev, kernel_switch, path, B):
    """The output layer zeroed, y0 nonzero: first step 1e-6 (both degenerate branches of the
    initial-step selection), every attempt accepted with an error ratio of exactly 0 and dt x 10,
    nfev = 2 + 6 attempts — the oracle's trace with its exact step sizes; the solution is the
    oracle's fp32 one (it is NOT y0: the quartic's rounding moves it by ~2e-7) and the hysteresis
    memory is advanced as the oracle's."""
    fld = PATHS[path][0]
    sd, y0 = case_inputs(fld, "zero", B)
    R = reference(fld, "zero", B, T_SHORT)
    tr = R["tr"]
    assert tr.first_step == H0 and all(a[3] and a[2] == 0.0 for a in tr.attempts) and len(tr.attempts) >= 5
    sol, att, nfev, state, _ = gpu_solve(path, sd, y0, T_SHORT, dev, kernel_switch)
    assert att[0][1] == H0, att[0]
    assert all(a[3] and a[2] == 0.0 for a in att), att
    assert [a[1] for a in att] == [a[1] for a in tr.attempts]          # dt * 10 in fp64, exactly
    assert [a[0] for a in att] == [a[0] for a in tr.attempts]
    assert nfev == 2 + 6 * len(att) == tr.nfev
    assert_trace(att, nfev, sol, state, R, path, mem_tol=1e-5)


# ---- (b) y0 = 0 ---------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("path", [p for p in PATHS if p in RESIDENT or p.startswith("host-")])
def test_zero_state(dev, kernel_switch, path, B):
    """y0 = 0 exactly with the unmodified field: d0 = 0 < 1e-5 -> h0 = 1e-6 and the first step is
    100 h0 (the oracle's, exactly), then the oracle's trace."""
    fld = PATHS[path][0]
    sd, y0 = case_inputs(fld, "y0zero", B)
    t = GRID[fld]
    R = reference(fld, "y0zero", B, t)
    tr = R["tr"]
    assert tr.first_step == H0_100, tr.first_step
    sol, att, nfev, state, _ = gpu_solve(path, sd, y0, t, dev, kernel_switch)
    assert att[0][1] == tr.first_step, (att[0], tr.first_step)
    assert_trace(att, nfev, sol, state, R, path)


# ---- (d) max_num_steps per output interval ------------------------------------------------------

@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("path", [p for p in PATHS if p in RESIDENT or p.startswith("host-")])
def test_max_num_steps_per_interval(dev, kernel_switch, path, B):
    """k = the oracle's largest number of attempts inside one output interval of a solve whose
    total exceeds k (y0 = 0 over 5 output times: most attempts fall into the first interval):
    max_num_steps = k succeeds with the identical trace, so the count restarts at every output time;
    k - 1 raises torchdiffeq's assertion (status 3) on every path, as in the oracle; a fresh solve
    afterwards on the same stream is unaffected."""
    fld = PATHS[path][0]
    T_LONG = GRID[fld]
    sd, y0 = case_inputs(fld, "y0zero", B)
    R = reference(fld, "y0zero", B, T_LONG)
    ref_sol, tr = R["sol"], R["tr"]
    counts = per_interval(tr.attempts, T_LONG)
    k = max(counts)
    assert sum(counts) == len(tr.attempts) > k >= 2, counts
    ref_k, tr_k, _ = oracle_solve(fld, "y0zero", B, T_LONG, options={"max_num_steps": k})
    assert tr_k.attempts == tr.attempts and torch.equal(ref_k, ref_sol)
    with pytest.raises(AssertionError, match="max_num_steps exceeded"):
        oracle_solve(fld, "y0zero", B, T_LONG, options={"max_num_steps": k - 1})
    sol, att, nfev, _, _ = gpu_solve(path, sd, y0, T_LONG, dev, kernel_switch, options={"max_num_steps": k})
    assert_trace(att, nfev, sol, None, R, f"{path} max_num_steps={k}")
    assert per_interval(att, T_LONG) == counts
    with pytest.raises(AssertionError, match="max_num_steps exceeded"):
        gpu_solve(path, sd, y0, T_LONG, dev, kernel_switch, options={"max_num_steps": k - 1})
    sol2, att2, nfev2, _, _ = gpu_solve(path, sd, y0, T_LONG, dev, kernel_switch)
    assert torch.equal(sol2, sol) and att2 == att and nfev2 == nfev


# ---- (e) safety / ifactor / dfactor -------------------------------------------------------------

CTRL = {"safety": 0.8, "ifactor": 4.0, "dfactor": 0.5}
# A smooth field never rejects after growing (the controller aims at ratio safety^5) and a field that
# rejects was not creeping, so each path runs two solves with these options: one from first_step =
# 1e-6 (ratios ~0: the growth is capped at x ifactor, several times) and one from a first step too
# large for the field (rejected attempts: the dfactor branch).  The large first step per field:
BIG_FIRST_STEP = {"kan": 5.0, "kanfet": 0.3, "fieldn": 2.0, "wide": 0.01, "ecg": 5.0}


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("path", [p for p in PATHS if p in RESIDENT or p.startswith("host-")])
def test_safety_ifactor_dfactor(dev, kernel_switch, path, B):
    """safety 0.8, ifactor 4, dfactor 0.5 against the oracle run with the same options.  Asserted on
    the oracle's traces: one holds an attempt whose step would have grown by more than ifactor
    (safety / ratio^(1/5) > 4), the other a rejected attempt; on the solver's: no step grows by more
    than x 4 or shrinks by more than x 0.5."""
    fld = PATHS[path][0]
    t = GRID[fld]
    sd, y0 = case_inputs(fld, "plain", B)
    seen_cap = seen_rej = False
    for fs in (1e-6, BIG_FIRST_STEP[fld]):
        opts = dict(CTRL, first_step=fs)
        R = reference(fld, "plain", B, t, opts)
        tr = R["tr"]
        seen_cap |= any(a[2] == 0 or CTRL["safety"] / a[2] ** 0.2 > CTRL["ifactor"] for a in tr.attempts)
        seen_rej |= any(not a[3] for a in tr.attempts)
        sol, att, nfev, _, _ = gpu_solve(path, sd, y0, t, dev, kernel_switch, options=opts)
        assert nfev == 1 + 6 * len(att)
        assert_trace(att, nfev, sol, None, R, f"{path} first_step={fs}")
        grow = [b[1] / a[1] for a, b in zip(att, att[1:])]
        assert max(grow) <= CTRL["ifactor"] * (1 + 1e-12) and min(grow) >= CTRL["dfactor"] * (1 - 1e-12)
    assert seen_cap, "ifactor never binds in the oracle's traces"
    assert seen_rej, "no rejected attempt in the oracle's traces: dfactor is never used"


# ---- (f) min_step / max_step --------------------------------------------------------------------

# (min_step, max_step) per field, inside the step sizes its y0 = 0 solve takes by itself
STEP_CLAMP = {"kan": (2e-3, 0.11), "kanfet": (2e-3, 4e-3), "fieldn": (2e-3, 0.05), "wide": (5e-4, 2e-3),
              "ecg": (2e-3, 0.11)}


# resident vs host-driven loop: (dt, solution / memory) bars of the existing pins of each pair —
# tests/test_gpu_dopri5.py and test_gpu_fieldn.py (the same fp32 arithmetic, dt to fp64 pow's last
# ulp), test_gpu_wide_dopri5.py, test_gpu_ecg.py (its head's sums are ordered differently).  NOT
# bitwise: none of those tests holds the pairs bit for bit — the norms' fp64 sums run in another
# order on the device, and the device's pow differs from the host's in the last ulp
HOST_BARS = {"kan": (1e-13, 1e-6), "kanfet": (1e-13, 1e-6), "fieldn": (1e-13, 1e-6), "wide": (1e-12, 1e-6),
             "ecg": (1e-5, 1e-5)}


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("path", RESIDENT)
def test_min_max_step_vs_host_loop(dev, kernel_switch, path, B):
    """min_step / max_step clamp the next step after _optimal_step_size.  The oracle (torchdiffeq)
    has no such clamp, so this pin is KERNEL TO KERNEL ONLY: the resident solve against the
    host-driven loop of the same field — the same attempts and nfev, dt to fp64 pow's last ulp, the
    solution and the memory as the existing resident-vs-host tests hold each pair (HOST_BARS:
    relative 1e-6, ECG 1e-5 — not bitwise, which those pairs are not).  Both clamps bind: from y0 = 0 the first step is 1e-4, its x 10 is below
    min_step, so the second logged dt equals min_step, and a later one equals max_step."""
    fld = PATHS[path][0]
    # max_num_steps: should a clamp ever pin dt at a step the field rejects, the solve ends with
    # torchdiffeq's assertion (and this test fails) instead of retrying it 2^31 times
    opts = dict(zip(("min_step", "max_step"), STEP_CLAMP[fld]), max_num_steps=200)
    sd, y0 = case_inputs(fld, "y0zero", B)
    res = gpu_solve(path, sd, y0, GRID[fld], dev, kernel_switch, options=opts)
    host = gpu_solve(HOST_OF[path], sd, y0, GRID[fld], dev, kernel_switch, options=opts, small=path.startswith("v6"))
    (s0, a0, n0, st0, _), (s1, a1, n1, st1, _) = res, host
    dt_tol, tol = HOST_BARS[fld]
    assert n0 == n1 and [a[3] for a in a0] == [a[3] for a in a1]
    np.testing.assert_allclose([a[1] for a in a0], [a[1] for a in a1], rtol=dt_tol)
    assert _slice_err(s0, s1) <= tol
    for a, b in zip(st0, st1):
        assert _rel(a, b) <= tol
    for att in (a0, a1):
        dts = [a[1] for a in att]
        assert dts[0] == H0_100 and opts["min_step"] in dts[1:] and opts["max_step"] in dts, dts
        assert all(opts["min_step"] <= d <= opts["max_step"] for d in dts[1:])


# ---- (c) training through (a) and (b) -----------------------------------------------------------

def _weights(t, B, D, dtype=torch.float32):
    return torch.randn(len(t), B, D, generator=torch.Generator().manual_seed(0)).to(dtype)


def train_gpu(fld, case, B, t, dev, resident):
    """loss = sum(w * solution) through F.odeint and backward, on the taped resident solve + reverse
    sweep (resident) or on _Dopri5Grad: (loss, parameter grads, y0 grad, attempts, nfev)"""
    import fet_ode_amd as F
    from fet_ode_amd.dopri5 import (ResidentSolve, _Dopri5Grad, set_resident_dopri5_training,
                                    set_resident_ecg_training)
    field = FIELDS[fld]
    sd, y0 = case_inputs(fld, case, B)
    m = field.module()
    m.load_state_dict(sd)
    m = m.to(dev)
    y = y0.to(dev).clone().requires_grad_(True)
    prev, prev_ecg = set_resident_dopri5_training(resident), set_resident_ecg_training(resident)
    try:
        sol = F.odeint(field.func(m), y, t, method="dopri5", rtol=TOL[fld][0], atol=TOL[fld][1])
        s = F.dopri5.dopri5_solve.last
        assert isinstance(s, ResidentSolve if resident else _Dopri5Grad), type(s).__name__
        loss = (_weights(t, B, y0.shape[1]).to(dev) * sol).sum()
        loss.backward()
    finally:
        set_resident_dopri5_training(prev)
        set_resident_ecg_training(prev_ecg)
    grads = {n: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu() for n, p in m.named_parameters()}
    att = [(float(a[1]), bool(a[3])) for a in s.attempts]
    return loss.item(), grads, y.grad.cpu(), att, s.nfev


_TRAIN_ORACLE = {}


def train_oracle(fld, case, B, t, dtype, perturb):
    """the same loss through the oracle's autograd (fp64: the reference; fp32, perturb = j: the
    yardstick draws of _grad_bar), once per case: (loss, grads, y0 grad, nfev)"""
    from oracle import torch_ref as O
    key = (fld, case, B, tuple(float(v) for v in t), dtype, perturb)
    if key in _TRAIN_ORACLE:
        return _TRAIN_ORACLE[key]
    field = FIELDS[fld]
    sd, y0 = case_inputs(fld, case, B)
    names = field.param_names()
    if perturb is not None:
        gen = torch.Generator().manual_seed(perturb)
        sd = {k: (v * (1 + 6e-8 * torch.randn(v.shape, generator=gen)) if k in names else v) for k, v in sd.items()}
    ps = {k: v.clone().to(dtype).requires_grad_(k in names) for k, v in sd.items()}
    _, f = field.oracle(ps)
    y = y0.to(dtype).requires_grad_(True)
    tr = O.Dopri5Trace()
    sol = O.odeint(f, y, t, rtol=TOL[fld][0], atol=TOL[fld][1], method="dopri5", trace=tr)
    loss = (_weights(t, B, y0.shape[1], dtype) * sol).sum()
    wrt = [ps[n] for n in names] + [y]
    gr = [torch.zeros_like(p) if g is None else g for g, p in zip(torch.autograd.grad(loss, wrt, allow_unused=True), wrt)]
    _TRAIN_ORACLE[key] = (loss.item(), dict(zip(names, gr[:-1])), gr[-1], tr.nfev)
    return _TRAIN_ORACLE[key]


TRAIN_PATHS = {"host-kan": ("kan", False), "host-kanfet": ("kanfet", False), "sweep-kan": ("kan", True),
               "sweep-kanfet": ("kanfet", True), "sweep-fieldn": ("fieldn", True), "host-ecg": ("ecg", False),
               "sweep-ecg": ("ecg", True)}


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("case", ["zero", "y0zero"])
@pytest.mark.parametrize("path", list(TRAIN_PATHS))
def test_training_through_degenerate_control(dev, path, case, B):
    """loss.backward() through the zero field (every error ratio 0: the sweep must take the
    dt * ifactor branch backwards too, not form er^(-1/5) = inf and multiply it by 0) and through
    y0 = 0 (the h0 = 1e-6 constant carries no gradient), on _Dopri5Grad and on the resident sweeps
    of the [2, 10, 2] fields, of fieldn and of the ECG field (fetode_ecg_dopri5_tape / _backward):
    against the oracle's fp64 autograd under _vs_oracle's bar (tests/test_gpu_dopri5_train.py,
    unchanged: 1e-4 per tensor, or 2x the host path's error, or 2x the reference's own fp32 error;
    the hysteretic fields' yardstick is the worst of four fp32 roundings).  Every gradient is
    finite, and a tensor whose oracle gradient is exactly zero — everything before a zeroed output
    layer — is exactly zero."""
    from test_gpu_dopri5_train import _grad_bar
    fld, resident = TRAIN_PATHS[path]
    kind = FIELDS[fld].kind
    t = T_SHORT if case == "zero" else GRID[fld]
    loss, grads, gy0, att, nfev = _grad_bar(
        f"{path} {case} B={B}", lambda res: train_gpu(fld, case, B, t, dev, res and resident),
        lambda dtype, pert: train_oracle(fld, case, B, t, dtype, pert),
        1e-4, 1e-3 if kind == "kanfet" else 1e-5, [None] if kind == "kan" else [None, 1, 2, 3])
    _, g64, gy64, _ = train_oracle(fld, case, B, t, torch.float64, None)
    assert all(torch.isfinite(g).all() for g in grads.values()) and torch.isfinite(gy0).all()
    zero = sorted(n for n, g in g64.items() if not g.any())
    assert sorted(n for n, g in grads.items() if not g.any()) == zero, "exactly-zero gradients differ from the oracle's"
    if case == "zero":
        assert nfev == 2 + 6 * len(att) and all(a[1] for a in att)
        first = "feat.basis." if kind == "ecg" else "layers.0."
        assert all(n in zero for n in g64 if n.startswith(first)), zero   # nothing reaches the first layer
        assert gy64.any() and gy0.any()
