"""The parameter sums of the ECG NODE-RNN's taped solves (T = 96, D = 1, H = 64): one iteration of
train_rnn_node's recipe (zero_grad, forward, cross-entropy, backward, clip_grad_norm_ 1.0, AdamW step) at
B = 1, 8 and 256 under rk4 (K = 10) and under dopri5 (K = 12, the taped one-launch solve, at rtol 1e-2 /
atol 1e-3 and 1e-3 / 1e-4), with ecg.set_fused_driven_param_grads on (fetode_driven_param_grad, DESIGN
§4.20) and off (the generic Ferro backward over every taped row plus two torch reductions: the code the
package had before).  HIP events, warmed, the two legs alternating in one process; next to the iteration
the parameter pass alone, between two events around the one Python function each leg calls for it.
Every configuration runs in a child process of its own under a time limit; the first one that fails or
runs out of time ends the run.
Usage: python tools/diag/driven_param_grad_time.py [--iters 10] [--sizes 1 8 256] [--limit 240]"""
import argparse
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

CONFIGS = [("rk4", 10, 1e-3, 1e-4), ("dopri5", 12, 1e-2, 1e-3), ("dopri5", 12, 1e-3, 1e-4)]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def one(solver, K, rtol, atol, B, iters):
    import torch
    import torch.nn.functional as F

    from fet_ode_amd import ecg
    from oracle import ecg_ref as E
    dev = torch.device("cuda:0")
    pass_ev = []

    def timed(fn):   # the parameter pass alone, between two events on the stream it is launched on
        def call(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args, **kw)
            e1.record()
            pass_ev.append((e0, e1))
            return out
        return call

    ecg.driven_param_grads = timed(ecg.driven_param_grads)
    ecg._driven_param_sums_generic = timed(ecg._driven_param_sums_generic)
    torch.manual_seed(0)
    m = ecg.NODE_RNN(input_size=1, hidden_size=64, num_classes=2, num_basis=K, solver=solver, rtol=rtol,
                     atol=atol).to(dev)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    x = E.ecg_x(B, seed=1).to(dev)
    y = torch.arange(B, device=dev) % 2

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
        assert len(pass_ev) == 1, len(pass_ev)
        ps = pass_ev[0][0].elapsed_time(pass_ev[0][1])
        pass_ev.clear()
        g = torch.cat([p.grad.reshape(-1) for p in m.enc.odefunc.parameters()])
        return dict(total=sum(t), forward=t[0], backward=t[1], param_pass=ps, step=t[2], loss=loss.item()), g

    prev_train = ecg.set_resident_driven_dopri5_training(True, True)
    res, grad = {}, {}
    try:
        for rnd in range(2):                       # alternate the two legs: a warming round, then the measured one
            for on in (True, False):
                prev = ecg.set_fused_driven_param_grads(on)
                try:
                    runs = [iteration() for _ in range(3 if rnd == 0 else iters)]
                    res[on] = {k: median([r[k] for r, _ in runs]) for k in runs[0][0]}
                    grad[on] = runs[-1][1]
                finally:
                    ecg.set_fused_driven_param_grads(prev)
    finally:
        ecg.set_resident_driven_dopri5_training(*prev_train)
    r1, r0 = res[True], res[False]
    rows = ""
    if solver == "dopri5":
        nf = m.enc.last_solve.nfev
        rows = f"; live rows {sum(nf)} of B * max(nfev) = {B * max(nf)}"
    dist = ((grad[True] - grad[False]).norm() / grad[False].norm()).item()
    what = solver if solver == "rk4" else f"{solver} {rtol:g}/{atol:g}"
    print(f"{what:18s} K={K} B={B:4d}: iteration on {r1['total']:9.3f} ms / off {r0['total']:9.3f} ms "
          f"({r0['total'] / r1['total']:6.2f}x); parameter pass on {r1['param_pass']:8.3f} ms / off "
          f"{r0['param_pass']:8.3f} ms ({r0['param_pass'] / r1['param_pass']:7.2f}x); on: forward {r1['forward']:7.3f}, "
          f"backward {r1['backward']:8.3f}, clip and step {r1['step']:6.3f}; off: backward {r0['backward']:8.3f}"
          f"{rows}; field gradients on vs off {dist:.2e}; loss {r1['loss']:.6f} vs {r0['loss']:.6f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 256])
    ap.add_argument("--limit", type=int, default=240, help="seconds a configuration may take")
    ap.add_argument("--one", nargs=5, metavar=("SOLVER", "K", "RTOL", "ATOL", "B"), help="(internal) one configuration")
    a = ap.parse_args()
    if a.one:
        s, K, rtol, atol, B = a.one
        one(s, int(K), float(rtol), float(atol), int(B), a.iters)
        return 0
    for s, K, rtol, atol in CONFIGS:
        for B in a.sizes:
            cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--one", s, str(K), repr(rtol),
                   repr(atol), str(B)]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc:   # a fault, an abort or a hang: nothing more is started
                print(f"{s} K={K} B={B}: exit status {rc}; stopping", flush=True)
                return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
