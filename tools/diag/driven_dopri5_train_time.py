"""Training the ECG NODE-RNN under dopri5 (T = 96, D = 1, H = 64, K = 12: the reference's own run of the
model): one iteration of train_rnn_node's recipe (zero_grad, forward, cross-entropy, backward,
clip_grad_norm_ 1.0, AdamW step) at B = 1, 8 and 256, at the reference main's tolerances (rtol 1e-2,
atol 1e-3) and the constructor defaults (1e-3, 1e-4), through the taped one-launch solve and its reverse
sweep (ecg.set_resident_driven_dopri5_training(True)) and through the per-sample _Dopri5Grad loop of the
same tree (the knob off: the code the package had before).  HIP events, warmed, both paths in one
process, alternating.  The knob-on iteration is split into the model's forward (the taped launch, the
RNN cell, the head), the reverse sweep (fetode_driven_dopri5_backward alone, events around the call)
and the rest of the backward (the parameter sums over the taped rows, the cell's and the head's
backward), plus clip and optimiser step.
Usage: python tools/diag/driven_dopri5_train_time.py [--iters 10] [--host-iters 1] [--step-grad 1]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from fet_ode_amd import _lib, ecg  # noqa: E402
from oracle import ecg_ref as E  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--step-grad", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 256])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    sweep_fn = lib.fetode_driven_dopri5_backward
    sweep_ev = []

    def sweep(*args):   # the sweep alone, between two events on the stream it is launched on
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = sweep_fn(*args)
        e1.record()
        sweep_ev.append((e0, e1))
        return rc

    lib.fetode_driven_dopri5_backward = sweep
    for rtol, atol in ((1e-2, 1e-3), (1e-3, 1e-4)):
        for B in a.sizes:
            torch.manual_seed(0)
            m = ecg.NODE_RNN(input_size=1, hidden_size=64, num_classes=2, num_basis=12, solver="dopri5", rtol=rtol,
                             atol=atol).to(dev)
            opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
            state = {k: v.clone() for k, v in m.state_dict().items()}
            x = E.ecg_x(B, seed=1).to(dev)
            y = (torch.arange(B, device=dev) % 2)

            def iteration():
                """One recipe iteration from the same parameters; the event times of its parts (ms)."""
                m.load_state_dict(state)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                opt.zero_grad()
                ev[0].record()
                loss = F.cross_entropy(m(x), y)
                ev[1].record()
                loss.backward()
                ev[2].record()
                torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
                opt.step()
                ev[3].record()
                torch.cuda.synchronize()
                t = [ev[i].elapsed_time(ev[i + 1]) for i in range(3)]
                sw = sum(e0.elapsed_time(e1) for e0, e1 in sweep_ev)
                sweep_ev.clear()
                return dict(total=sum(t), forward=t[0], sweep=sw, rest=t[1] - sw, step=t[2], loss=loss.item())

            res = {}
            for rnd in range(2):                       # alternate the two paths: a warming round, then the measured one
                for on in (True, False):
                    prev = ecg.set_resident_driven_dopri5_training(on, bool(a.step_grad))
                    try:
                        n = (3 if on else 1) if rnd == 0 else (a.iters if on else a.host_iters)
                        runs = [iteration() for _ in range(n)]
                        res[on] = {k: median([r[k] for r in runs]) for k in runs[0]}
                        if on:
                            att = m.enc.last_solve.n_attempts
                    finally:
                        ecg.set_resident_driven_dopri5_training(*prev)
            r1, r0 = res[True], res[False]
            print(f"rtol {rtol:g} atol {atol:g} B={B:4d} step_grad={a.step_grad}: one launch + sweep median "
                  f"{r1['total']:9.3f} ms = forward {r1['forward']:8.3f} + sweep {r1['sweep']:8.3f} + parameter sums and "
                  f"the rest of backward {r1['rest']:8.3f} + clip and step {r1['step']:7.3f}; _Dopri5Grad loop "
                  f"{r0['total']:10.3f} ms (forward {r0['forward']:10.3f}, backward {r0['sweep'] + r0['rest']:10.3f}), "
                  f"loop / one launch {r0['total'] / r1['total']:7.1f}x; attempts per sample {min(att)}-{max(att)} "
                  f"(mean {sum(att) / len(att):.1f}); loss {r1['loss']:.6f} vs {r0['loss']:.6f}", flush=True)


if __name__ == "__main__":
    main()
