"""Training through the ETT forecaster's dopri5 call with dopri5.set_resident_wide_training off
(_Dopri5Grad: host-driven attempts, autograd per stage) and on (fetode_wide_dopri5_tape +
fetode_wide_dopri5_backward), in one process: wall time per iteration, attempts, nfev, and the
two paths' gradient agreement on the first iteration.

CASE=ref   the reference's own iteration (bench.ett_reference_iteration_rate's shapes: B = 64,
           32 -> 8, t_fut 0..7, KAN-FET latent field [64, 128, 64] x 0.1, MSE, clip_grad_norm 1.0,
           AdamW) at rtol REF_RTOL (default 1e-5), atol = rtol / 100
CASE=b2048 the bench's ett.dopri5.train line: B = 2048, 96 -> 24, rtol 1e-3 / atol 1e-4, Adam
ITERS timed iterations per path (default 2) after one warm-up; MODES "0,1" (off, on).
One JSON line per path."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import fet_ode_amd as F  # noqa: E402
import fet_ode_amd.dopri5  # noqa: E402,F401
from fet_ode_amd import ett  # noqa: E402

dev = torch.device("cuda:0")
case = os.environ.get("CASE", "ref")
iters = int(os.environ.get("ITERS", "2"))
modes = [int(v) for v in os.environ.get("MODES", "0,1").split(",")]
if case == "ref":
    rtol = float(os.environ.get("REF_RTOL", "1e-5"))
    atol, B, c, P, tmax = rtol * 1e-2, 64, 32, 8, 7.0
else:
    rtol, atol, B, c, P, tmax = 1e-3, 1e-4, 2048, 96, 24, 23 * 0.05


def make(sd=None):
    torch.manual_seed(0)
    m = ett.LatentNeuralODEForecaster(num_features=7, context_len=c, pred_len=P, latent_dim=64, solver="dopri5",
                                      rtol=rtol, atol=atol)
    if sd is not None:
        m.load_state_dict(sd)
        return m.to(dev)
    with torch.no_grad():
        for n, p_ in m.dynamics.net.named_parameters():
            if n.endswith(("coef", "base_weight", "spline_weight", "logistic_weight")):
                p_.mul_(0.1)
    return m.to(dev)


first = make()
sd0 = {k: v.clone() for k, v in first.state_dict().items()}
g = torch.Generator().manual_seed(4)
series = torch.cumsum(torch.randn(B + c + P, 7, generator=g), 0) * 0.05
ds = ett.EnergyWindowDataset(series, series[:, -1], c, P, device=dev)
xb, yb = ds.batch(torch.arange(B, device=dev))
t_fut = torch.linspace(0.0, tmax, steps=P, device=dev)
grads0 = {}
for mode in modes:
    m = make(sd0)
    opt = (torch.optim.AdamW if case == "ref" else torch.optim.Adam)(m.parameters(), lr=1e-4)
    prev = F.dopri5.set_resident_wide_training(bool(mode))
    rows = []
    try:
        for it in range(iters + 1):
            opt.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = torch.nn.functional.mse_loss(m(xb, t_fut), yb)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            loss.backward()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            s = F.dopri5.dopri5_solve.last
            if it == 0:
                grads0[mode] = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
            if case == "ref":
                torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
            opt.step()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            rows.append(dict(fwd_ms=(t1 - t0) * 1e3, bwd_ms=(t2 - t1) * 1e3, iter_ms=(t3 - t0) * 1e3,
                             attempts=s.n_attempts, nfev=s.nfev, loss=loss.item(), path=type(s).__name__))
    finally:
        F.dopri5.set_resident_wide_training(prev)
    timed = rows[1:]
    print(json.dumps({"case": case, "B": B, "rtol": rtol, "resident_wide_training": bool(mode), "path": rows[0]["path"],
                      "warmup_iter_ms": rows[0]["iter_ms"],
                      "iter_ms": [round(r["iter_ms"], 2) for r in timed], "fwd_ms": [round(r["fwd_ms"], 2) for r in timed],
                      "bwd_ms": [round(r["bwd_ms"], 2) for r in timed], "attempts": [r["attempts"] for r in rows],
                      "nfev": [r["nfev"] for r in rows], "loss": [r["loss"] for r in rows]}), flush=True)
if 0 in grads0 and 1 in grads0:
    rel = {n: ((grads0[1][n].double() - grads0[0][n].double()).norm()
               / grads0[0][n].double().norm().clamp_min(1e-300)).item() for n in grads0[0]}
    worst = max(rel, key=rel.get)
    print(json.dumps({"case": case, "first_iteration_grad_rel_diff_on_vs_off_worst": rel[worst], "tensor": worst,
                      "finite": all(bool(torch.isfinite(v).all()) for v in grads0[1].values())}), flush=True)
