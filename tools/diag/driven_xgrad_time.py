"""The ECG NODE-RNN (T = 96, D = 1, H = 64, K = 10) at B = 8 (the reference trainer's batch) and
B = 256 with a driving series that REQUIRES GRAD: one training iteration of the train_rnn_node recipe
(forward + cross-entropy + backward, to the series too, + clip_grad_norm_ 1.0 + AdamW step) under rk4
and under dopri5 at rtol 1e-2 / atol 1e-3 (ecg.set_resident_driven_dopri5_training on), with
ecg.set_driven_series_grad off — what the package did for this input before: the per-stage path (rk4),
the per-sample host loop (dopri5) — and on: the one-launch solves with the series' gradient from the
sweep and fetode_driven_table_backward.  HIP events, warmed, the two knob states in one
process, alternating; the second round is kept.  The slow states run few iterations (the dopri5 host
loop at B = 256 takes seconds per iteration: its first round is its warm-up).
Usage: python tools/diag/driven_xgrad_time.py [--iters 10] [--off-iters 3]"""
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--off-iters", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ptrain = ecg.set_resident_driven_dopri5_training(True)
    try:
        for solver in ("rk4", "dopri5"):
            for B in (8, 256):
                torch.manual_seed(0)
                m = ecg.NODE_RNN(input_size=1, hidden_size=64, num_classes=2, num_basis=10, solver=solver, rtol=1e-2,
                                 atol=1e-3).to(dev)
                opt = torch.optim.AdamW(m.parameters(), lr=0.0, weight_decay=0.0)   # the step is timed, nothing moves
                x = E.ecg_x(B, seed=1).to(dev).requires_grad_(True)
                y = (torch.arange(B) % 2).to(dev)
                last = {}

                def train():
                    opt.zero_grad(set_to_none=True)
                    x.grad = None
                    loss = torch.nn.functional.cross_entropy(m(x), y)
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
                    opt.step()
                    last["loss"], last["gx"] = loss.item(), x.grad

                slow = solver == "dopri5"
                res, out = {}, {}
                for rnd in range(2):                       # alternate the two knob states; keep the second round
                    for on in (True, False):
                        prev = ecg.set_driven_series_grad(on)
                        try:
                            if on:
                                res[on] = timed(train, 2, a.iters)
                            else:
                                res[on] = timed(train, 0 if slow else 1, 1 if slow and B > 8 else a.off_iters)
                            out[on] = (last["loss"], last["gx"].detach().clone())
                        finally:
                            ecg.set_driven_series_grad(prev)
                rel = ((out[True][1] - out[False][1]).norm() / out[False][1].norm()).item()
                for on in (False, True):
                    med, best = res[on]
                    print(f"{solver:6s} B={B:4d} series grad knob {'on ' if on else 'off'}: training iteration median "
                          f"{med:10.3f} ms (min {best:10.3f}), loss {out[on][0]:.6f}", flush=True)
                print(f"{solver:6s} B={B:4d} off / on: {res[False][0] / res[True][0]:.1f}x; d loss / d x on against off, "
                      f"normwise {rel:.3e}", flush=True)
    finally:
        ecg.set_resident_driven_dopri5_training(*ptrain)


if __name__ == "__main__":
    main()
