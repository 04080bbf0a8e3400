"""Where the fused rk4 kernels store their solution rows (fetode_fused4_body.h): a lane carries the
address of the next output row and advances it by the row stride with every output it writes, on the
first output of a step and in the loop over further outputs inside the same step.  A pointer that
falls behind or runs ahead of the output index puts a row one stride off: a neighbour row is
overwritten, a row keeps what the buffer held, or the store leaves the buffer.

Every case solves into a buffer the test owns, through the library's fixed-grid entry point: the
(T, B, 2) solution stands between two guard blocks of one row stride each, guards and solution
pre-filled with a sentinel.  After the solve the guards must still hold the sentinel bit for bit, no
solution element may, and the rows must match the fp32 oracle (oracle/torch_ref.py) at the per-slice
1e-5 that tests/test_gpu_plan_image.py applies to the same grids.

Grids: one output per step; several outputs inside one step; steps with no output; more outputs
than one schedule chunk (SCH = 64), one per step and twenty per step, so that the chunk reload
falls on a step's first output and inside the several-outputs loop.  B = 3 (a half-filled last
wave) and B = 65 (more than one workgroup at either lane map, an odd tail), both lane maps, KAN and
KAN-FET in both gate forms."""
import importlib

import numpy as np
import pytest
import torch

from conftest import fused_ranges, golden_sd, load_golden

REL = 1e-5
SCH = 64
SENTINEL = -12345.678   # no solution value of these short solves (|y| < 10)

LEGS = {
    "two-per-wave": dict(small=0, tpw1=(0, 0), v8=(0, 0)),
    "one-per-wave": dict(small=0, tpw1=(0, 1 << 40), v8=(0, 0)),
}
# steps of 0.1 in the step_size grids.  The horizons stay where tests/test_gpu_plan_image.py keeps
# them (t <= 0.5, for step_size grids t <= 0.4): the KAN-FET field amplifies fp32 rounding along a
# trajectory, and there the oracle's own fp32 solve is about a tenth of the bar from its fp64 solve.
GRIDS = {
    "one-per-step": (torch.tensor(np.linspace(0, 0.5, 6)), None),
    # four outputs inside step 0 (the last on its end), one in step 1, none in step 2's interior but
    # one on its end, an interpolated one in step 3
    "several-per-step": (torch.tensor([0.0, 0.02, 0.05, 0.07, 0.1, 0.13, 0.3, 0.37], dtype=torch.float64), {"step_size": 0.1}),
    # steps 1 and 2 write nothing at all
    "empty-steps": (torch.tensor([0.0, 0.05, 0.31, 0.37], dtype=torch.float64), {"step_size": 0.1}),
    "chunk+1-one-per-step": (torch.tensor(np.linspace(0, 0.5, SCH + 2)), None),
    # 81 outputs, twenty per step: output 65 (the second chunk of 64 starts there) lies inside step 3's loop
    "chunk+1-inside-steps": (torch.tensor(np.linspace(0, 0.4, 81)), {"step_size": 0.1}),
}
KINDS = ["kanfet-factored", "kanfet-unfactored", "kan"]
EC_BIG = 4.5   # gate_slope 10: 10 * log2(e) * 4.5 = 64.9 > 60, the plan drops the factored gate


def _golden(kind):
    return load_golden("traj_kan" if kind == "kan" else "traj_kanfet")


def _sd(kind):
    sd = {k: v.clone() for k, v in golden_sd(_golden(kind)).items()}
    if kind == "kanfet-unfactored":
        sd["layers.0.ferro.Ec"][1, 9, 9] = EC_BIG
    return sd


def _y0(kind, B):
    from oracle import torch_ref as O
    y = torch.from_numpy(_golden(kind)["y0_B64"]).clone()
    if B > y.shape[0]:
        y = torch.cat([y, O.lv_y0(B - y.shape[0], seed=3).to(y.dtype)])
    return y[:B].float().contiguous()


_REF = {}


def _ref_solve(kind, B, grid):
    """The oracle's solve, computed once per case and shared (read-only)."""
    key = (kind, B, grid)
    if key not in _REF:
        from oracle import torch_ref as O
        t, opts = GRIDS[grid]
        if kind == "kan":
            ref = O.KANRef([O.KANLinearParams.from_state_dict(_sd(kind), f"layers.{l}.") for l in range(2)])
        else:
            ref = O.KANFETRef.from_state_dict(_sd(kind), 2)
        with torch.no_grad():
            _REF[key] = O.odeint(lambda tt, yy: ref(yy), _y0(kind, B), t, method="rk4", options=opts)
    return _REF[key]


def _solve_into_guarded_buffer(kind, dev, B, grid, leg):
    """fetode_integrate_fixed with the solution inside a sentinel-filled buffer: (guard before, the
    solution, guard after), each guard one row stride (B * 2 floats)."""
    import fet_ode_amd as F
    from fet_ode_amd import _lib
    OI = importlib.import_module("fet_ode_amd.odeint")
    t, opts = GRIDS[grid]
    m = (F.KAN if kind == "kan" else F.KANFET)([2, 10, 2], grid_size=5)
    m.load_state_dict(_sd(kind))
    m = m.to(dev)
    y0 = _y0(kind, B).to(dev)
    method, _, tp, reversed_ = OI._check_inputs(y0, t, "rk4")
    sched = OI.get_schedule(tp, (opts or {}).get("step_size"), reversed_)
    T, D = sched.T, 2
    with fused_ranges() as fr:
        fr.set(**LEGS[leg])
        field = OI.fused_field(F.autonomous(m))
        assert field is not None
        handle = OI.make_handle(field, B, dev)
        lib = _lib.load()
        assert handle.supported(lib)
        plan = OI.build_plan(field, handle, dev)
        state, mask = OI.pack_state(field, B, dev)
        _, coef, ostep, omode, oslope = sched.device_arrays(dev)
        buf = torch.full(((T + 2) * B * D,), SENTINEL, device=dev, dtype=torch.float32)
        sol = buf[B * D:(T + 1) * B * D].view(T, B, D)
        _lib.check(lib.fetode_integrate_fixed(
            handle.ref, plan.data_ptr(), OI.FIXED_METHODS[method], y0.data_ptr(), B, coef.data_ptr(), sched.n_steps,
            ostep.data_ptr(), omode.data_ptr(), oslope.data_ptr(), T, sol.data_ptr(),
            _lib.ptr(state), mask, None, _lib.stream_handle(dev)), "fetode_integrate_fixed")
        torch.cuda.synchronize()
    buf = buf.cpu()
    return buf[:B * D], buf[B * D:(T + 1) * B * D].view(T, B, D), buf[(T + 1) * B * D:]


def slice_rel_err(a, b):
    a = a.double().reshape(a.shape[0], -1)
    b = b.double().reshape(b.shape[0], -1)
    return ((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)).max().item()


def test_grids_cover_the_output_cases():
    """The schedules are what the docstring says: per step, how many outputs it writes."""
    OI = importlib.import_module("fet_ode_amd.odeint")
    per = {}
    for name, (t, opts) in GRIDS.items():
        s = OI.get_schedule(t, (opts or {}).get("step_size"), False)
        steps = s.out_step[1:s.T].tolist() if hasattr(s.out_step, "tolist") else list(s.out_step[1:s.T])
        per[name] = [steps.count(i) for i in range(s.n_steps)]
        print(name, "outputs per step", per[name], "T", s.T)
    assert set(per["one-per-step"]) == {1}
    assert max(per["several-per-step"]) >= 3
    assert 0 in per["empty-steps"]
    assert set(per["chunk+1-one-per-step"]) == {1} and len(per["chunk+1-one-per-step"]) == SCH + 1
    c = per["chunk+1-inside-steps"]
    assert sum(c) > SCH and max(c) >= 20 and sum(c[:3]) < SCH < sum(c[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("B", [3, 65])
@pytest.mark.parametrize("kind", KINDS)
def test_solution_rows_and_nothing_else(dev, kind, B, leg, grid):
    before, sol, after = _solve_into_guarded_buffer(kind, dev, B, grid, leg)
    ref = _ref_solve(kind, B, grid)
    s = torch.tensor(SENTINEL, dtype=torch.float32)
    unwritten = int((sol == s).sum())
    err = slice_rel_err(sol, ref)
    print(f"{kind} B={B} {leg} {grid}: T={sol.shape[0]}, max slice rel err {err:.3e}, unwritten {unwritten}")
    assert torch.isfinite(ref).all()
    assert bool((before == s).all()) and bool((after == s).all()), "a store outside the solution"
    assert unwritten == 0
    assert err <= REL, err
