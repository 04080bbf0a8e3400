"""The ECG NODE-RNN (T = 96, D = 1, H = 64, K = 10) at B = 8 (the reference trainer's batch) and
B = 256: the forward (NODE_RNN logits, no grad) and one training iteration of the train_rnn_node
recipe (forward + cross-entropy + backward + clip_grad_norm_ 1.0 + AdamW step), with the fused driven
path (fetode_driven_fixed / _tape / _backward) and with the per-stage path of the same tree
(ecg.set_fused_driven(False): kernels the package had before).  HIP events, warmed, both paths in one
process, alternating; the fused path also per forced samples-per-workgroup variant.
Usage: python tools/diag/driven_time.py [--iters 20] [--stage-iters 3]"""
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
    ap.add_argument("--stage-iters", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for B in (8, 256):
        torch.manual_seed(0)
        m = ecg.NODE_RNN(input_size=1, hidden_size=64, num_classes=2, num_basis=10, solver="rk4").to(dev)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
        x = E.ecg_x(B, seed=1).to(dev)
        y = (torch.arange(B) % 2).to(dev)

        def forward():
            with torch.no_grad():
                return m(x)

        def train():
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(m(x), y)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
            opt.step()

        res = {}
        for rnd in range(2):                       # alternate the two paths; keep the second round
            for fused in (True, False):
                prev = ecg.set_fused_driven(fused)
                try:
                    w, n = (5, a.iters) if fused else (1, a.stage_iters)
                    res[fused] = (timed(forward, w, n), timed(train, w, n))
                finally:
                    ecg.set_fused_driven(prev)
        for fused in (True, False):
            (fm, fb), (tm, tb) = res[fused]
            print(f"B={B:4d} {'fused    ' if fused else 'per-stage'}: forward median {fm:9.3f} ms (min {fb:9.3f}), "
                  f"training iteration median {tm:9.3f} ms (min {tb:9.3f})", flush=True)
        print(f"B={B:4d} per-stage / fused: forward {res[False][0][0] / res[True][0][0]:.1f}x, "
              f"training iteration {res[False][1][0] / res[True][1][0]:.1f}x", flush=True)
        for v in (1, 2, 4):
            prev = ecg.set_driven_samples_per_workgroup(v)
            try:
                (fm, fb), (tm, tb) = timed(forward, 3, a.iters), timed(train, 3, a.iters)
            finally:
                ecg.set_driven_samples_per_workgroup(prev)
            print(f"B={B:4d} fused, {v} sample(s) per workgroup: forward median {fm:9.3f} ms, "
                  f"training iteration median {tm:9.3f} ms", flush=True)


if __name__ == "__main__":
    main()
