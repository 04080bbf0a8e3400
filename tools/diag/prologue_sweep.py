"""Per-launch fixed cost of the bench's rk4 solve (LV KAN-FET): the launch timed at several step
counts with the same dt = 3.5 / 34, fitted as time = a + b n_steps per batch.  The intercept a is
what a launch costs before (and after) its step loop: table staging, lane constants, schedule
chunks, plus the event pair's own overhead.  Uses whatever library FETODE_LIB names; clocks settled
first as tools/diag/fwd_ab.py does.  B = 4096: two trajectories per wave, 1024: one per wave,
512: v8_kernel."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import bench
import fet_ode_amd as F

dev = torch.device("cuda:0")
torch.manual_seed(0)
m = F.KANFET([2, 10, 2], grid_size=5).to(dev)
t35 = torch.tensor(np.linspace(0, 3.5, 35))
with torch.no_grad():
    y4 = bench.lv_y0(4096, 0).to(dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:
        for _ in range(20):
            F.odeint(F.autonomous(m), y4, t35, method="rk4")
        torch.cuda.synchronize()
steps = [int(s) for s in os.environ.get("SWEEP_STEPS", "1,17,34,68").split(",")]
reps = int(os.environ.get("SWEEP_REPS", "200"))
dt = 3.5 / 34
r = {"lib": os.path.basename(os.environ.get("FETODE_LIB", "libfetode.so")), "tag": os.environ.get("AB_TAG", ""),
     "steps": steps, "reps": reps}
for B in [int(b) for b in os.environ.get("AB_B", "4096,1024,512").split(",")]:
    y0 = bench.lv_y0(B, 0).to(dev)
    us = []
    for n in steps:
        t = torch.tensor(dt * np.arange(n + 1))
        us.append(1e3 * bench.kernel_time_ms(m, y0, t, reps=reps))
    b, a = np.polyfit(np.array(steps, dtype=np.float64), np.array(us), 1)
    r[f"B{B}"] = {"us": [round(u, 2) for u in us], "intercept_us": round(float(a), 2), "us_per_step": round(float(b), 3)}
print(json.dumps(r), flush=True)
