"""bench.py's contract: a plain run is the headline only (`--full` holds the rest), the problem's
bits are fixed by the seed, and `--dump-outputs` writes the last timed solve's solution."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import bench

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY_KEYS = {"roofline", "mfma", "train", "strong_proxy", "lv_plain_closure", "lv_dopri5", "ecg", "mnist", "ett",
                  "cpu_baseline", "parity"}


def _args(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_and_dump_are_off_by_default(monkeypatch):
    a = _args(["--gpus", "1", "--steps", "7", "--warmup", "3"], monkeypatch)
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    a = _args(["--full", "--dump-outputs", "d", "--no-ett"], monkeypatch)
    assert a.full and a.dump_outputs == "d" and a.no_ett


def _state_bytes(sd):
    return b"".join(sd[k].contiguous().numpy().tobytes() for k in sorted(sd))


def test_reproducible_init_fixes_the_weights_bits():
    """The fp64 minimum-norm fit rounded once: the same bits whatever sits in memory around it, within
    the LAPACK fit's own wobble (an ulp of the 0.02-sized spline weights: 1e-7 is 50 of them) of the
    plain init, and torch.linalg.lstsq is put back."""
    import fet_ode_amd as F
    orig = torch.linalg.lstsq
    sds = []
    for pad in (0, 3, 17):
        junk = [torch.empty(5 + 7 * pad) for _ in range(pad)]   # shifts the allocations' alignment
        torch.manual_seed(0)
        with bench.reproducible_init():
            sds.append(F.KANFET([2, 10, 2], grid_size=5).state_dict())
        del junk
    assert torch.linalg.lstsq is orig
    assert _state_bytes(sds[0]) == _state_bytes(sds[1]) == _state_bytes(sds[2])
    torch.manual_seed(0)
    plain = F.KANFET([2, 10, 2], grid_size=5).state_dict()
    assert set(plain) == set(sds[0])
    for k, v in plain.items():
        if v.numel():
            assert (v.double() - sds[0][k].double()).abs().max().item() <= 1e-7, k


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_solve(dev, tmp_path):
    """One plain run in a process of its own (K = 3, W = 1, a 20 ms settle loop whose solve count is
    the wall clock's): the line has the headline fields and none of the --full legs, and sol.npy is
    bit for bit solve W + K from the fresh state of the same seed-0 problem built in this process."""
    import fet_ode_amd as F
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--settle-s", "0.02", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert HEADLINE_KEYS <= set(line) and not (FULL_ONLY_KEYS & set(line)), sorted(line)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["ms_per_step"] > 0 and line["clock_settle"]["solves"] >= 10
    assert line["value"] == pytest.approx(bench.STEPS_PER_SOLVE / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert sorted(os.listdir(out)) == ["sol.npy"]
    sol = np.load(out / "sol.npy")
    assert sol.dtype == np.float32 and sol.shape == (bench.T, bench.B, 2) and np.isfinite(sol).all()

    model, _, y0, _, t = bench.make_problem(0, 1, "strong", dev)
    y0d = y0.to(dev)
    with torch.no_grad():
        for _ in range(4):
            here = F.odeint(F.autonomous(model), y0d, t, method="rk4")
    assert np.array_equal(sol, here.cpu().numpy())
    assert np.array_equal(sol[0], y0.numpy())
