"""The ECG NODE-RNN under dopri5 (T = 96, D = 1, H = 64, K = 12: the reference's own run of the model):
the forward (NODE_RNN logits, no grad) at B = 1, 8 and 256, at the reference main's tolerances
(rtol 1e-2, atol 1e-3) and the constructor defaults (1e-3, 1e-4), with the one-launch solve that
carries a step controller per sample (fetode_driven_dopri5) and with the host-driven per-sample loop
of the same tree (ecg.set_resident_driven_dopri5(False): the code the package had before).  HIP events,
warmed, both paths in one process, alternating; the attempt counts of the batch alongside.
Usage: python tools/diag/driven_dopri5_time.py [--iters 20] [--host-iters 2]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from fet_ode_amd import ecg  # noqa: E402
from oracle import ecg_ref as E  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
    return ms[len(ms) // 2], ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for rtol, atol in ((1e-2, 1e-3), (1e-3, 1e-4)):
        for B in (1, 8, 256):
            torch.manual_seed(0)
            m = ecg.NODE_RNN(input_size=1, hidden_size=64, num_classes=2, num_basis=12, solver="dopri5", rtol=rtol,
                             atol=atol).to(dev)
            x = E.ecg_x(B, seed=1).to(dev)

            def forward():
                with torch.no_grad():
                    return m(x)

            res, out = {}, {}
            for rnd in range(2):                       # alternate the two paths; keep the second round
                for resident in (True, False):
                    prev = ecg.set_resident_driven_dopri5(resident)
                    try:
                        w, n = (5, a.iters) if resident else (1, a.host_iters)
                        res[resident] = timed(forward, w, n)
                        out[resident] = forward()
                        if resident:
                            att = m.enc.last_solve.n_attempts
                            rej = [sum(1 for q in s if not q[3]) for s in m.enc.last_solve.attempts]
                    finally:
                        ecg.set_resident_driven_dopri5(prev)
            # free runs of two fp32 programs: where a sample's error ratio comes near 1 they accept differently
            diff = (out[True] - out[False]).abs().amax(dim=1)
            print(f"rtol {rtol:g} atol {atol:g} B={B:4d}: one launch median {res[True][0]:9.3f} ms (min {res[True][1]:9.3f}), "
                  f"host loop median {res[False][0]:9.3f} ms (min {res[False][1]:9.3f}), host / one launch "
                  f"{res[False][0] / res[True][0]:7.1f}x; attempts per sample {min(att)}-{max(att)} "
                  f"(mean {sum(att) / len(att):.1f}), rejected {min(rej)}-{max(rej)}; |logit difference| per sample "
                  f"median {diff.median().item():.2e}, max {diff.max().item():.2e}", flush=True)


if __name__ == "__main__":
    main()
