"""One KanFet_NODE training iteration (forward + cross-entropy + backward, HIP events) with the
resident ECG training path switched off (host-driven autograd, _Dopri5Grad) and on (taped resident
solve + resident reverse sweep), in one process, at two workloads:
  * the bench's: synthetic_ecg(200), latent 64, nb 10, rtol 1e-3 / atol 1e-4;
  * the reference trainer's own shape: batch 4, latent_dim = 1.
Usage: python tools/diag/ecg_train_time.py [--warmup 20] [--iters 30]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from fet_ode_amd import dopri5 as D5  # noqa: E402
from fet_ode_amd import ecg  # noqa: E402
from oracle import ecg_ref as E  # noqa: E402


def time_iteration(m, x, y, resident, warmup, iters):
    prev = D5.set_resident_ecg_training(resident)
    try:
        def it():
            m.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(m(x), y)
            loss.backward()
            return loss
        for _ in range(warmup):
            it()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
        ev[0].record()
        for i in range(iters):
            it()
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
        last = m.last_solve
        return ms[len(ms) // 2], ms[0], last.nfev, last.n_attempts, type(last).__name__
    finally:
        D5.set_resident_ecg_training(prev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for label, B, latent in (("bench shape", 200, 64), ("reference trainer shape", 4, 1)):
        torch.manual_seed(0)
        m = ecg.KanFet_NODE(T=96, num_classes=2, latent_dim=latent, num_basis=10, rtol=1e-3, atol=1e-4)
        m = m.to(dev).eval()   # eval: dropout off, so both paths see the same iteration
        x = E.ecg_x(B, seed=1).to(dev)
        y = (torch.arange(B) % 2).to(dev)
        res = {}
        for resident in (False, True):
            res[resident] = time_iteration(m, x, y, resident, max(20, a.warmup), a.iters)
            med, best, nfev, natt, kind = res[resident]
            print(f"{label} (B={B}, latent {latent}) switch {'on ' if resident else 'off'} [{kind}]: "
                  f"median {med:.3f} ms, min {best:.3f} ms per iteration, nfev {nfev}, attempts {natt}", flush=True)
        print(f"{label}: off / on = {res[False][0] / res[True][0]:.2f}x", flush=True)


if __name__ == "__main__":
    main()
