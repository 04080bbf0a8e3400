"""The ECG NODE-RNN (T = 96, D = 1, H = 64, K = 10) at B = 8 (the reference trainer's batch) and
B = 256 under the fixed-grid configurations plain rk4's one-launch solve declines — solver euler,
midpoint, rk4_classic, and rk4 with step_size = 1/190 (two steps per knot interval) — with
ecg.set_fused_driven_methods off (the per-stage path: what the package does by default) and on (the
one-launch solve of fetode_driven_grid*).  Two legs: the forward without gradients, and one
training iteration of the train_rnn_node recipe (forward + cross-entropy + backward + clip_grad_norm_ 1.0
+ AdamW step).  HIP events, warmed, the two knob states in one process, alternating; the second round is
kept.  The slow state runs few iterations.
Usage: python tools/diag/driven_methods_time.py [--iters 20] [--off-iters 3]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from fet_ode_amd import ecg  # noqa: E402
from oracle import ecg_ref as E  # noqa: E402

CONFIGS = (("euler", None), ("midpoint", None), ("rk4_classic", None), ("rk4", 1.0 / 190.0))


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
    ap.add_argument("--off-iters", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for solver, step_size in CONFIGS:
        name = solver if step_size is None else f"{solver} h=1/190"
        for B in (8, 256):
            torch.manual_seed(0)
            m = ecg.NODE_RNN(input_size=1, hidden_size=64, num_classes=2, num_basis=10, solver=solver).to(dev)
            m.enc.solver_options = None if step_size is None else {"step_size": step_size}
            opt = torch.optim.AdamW(m.parameters(), lr=0.0, weight_decay=0.0)   # the step is timed, nothing moves
            x = E.ecg_x(B, seed=1).to(dev)
            y = (torch.arange(B) % 2).to(dev)
            last = {}

            def forward():
                with torch.no_grad():
                    last["out"] = m(x)

            def train():
                opt.zero_grad(set_to_none=True)
                loss = torch.nn.functional.cross_entropy(m(x), y)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
                opt.step()
                last["out"] = loss.detach()

            for leg, fn in (("forward", forward), ("training iteration", train)):
                res, out = {}, {}
                for rnd in range(2):                       # alternate the two knob states; keep the second round
                    for on in (True, False):
                        prev = ecg.set_fused_driven_methods(on)
                        try:
                            res[on] = timed(fn, 2, a.iters) if on else timed(fn, 1, a.off_iters)
                            out[on] = last["out"].detach().clone()
                        finally:
                            ecg.set_fused_driven_methods(prev)
                rel = ((out[True] - out[False]).norm() / out[False].norm()).item()
                for on in (False, True):
                    med, best = res[on]
                    print(f"{name:16s} B={B:4d} {leg:18s} knob {'on ' if on else 'off'}: median {med:10.3f} ms "
                          f"(min {best:10.3f})", flush=True)
                print(f"{name:16s} B={B:4d} {leg:18s} off / on: {res[False][0] / res[True][0]:.1f}x; "
                      f"{'logits' if leg == 'forward' else 'loss'} on against off, normwise {rel:.3e}", flush=True)


if __name__ == "__main__":
    main()
