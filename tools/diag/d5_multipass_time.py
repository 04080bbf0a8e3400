"""The multi-pass mode of the resident LV dopri5 launches (fetode_dopri5_set_multipass) against the
path the same call takes with the switch off, HIP events, median of repeated iterations:
  * B = 8192 and 16384 (beyond one co-resident grid), KAN-FET and KAN [2, 10, 2], t = linspace(0, 1, 11),
    rtol 1e-3 / atol 1e-4: an inference solve and one training iteration (solve + loss.backward());
    switch off = the host-driven loop / host autograd (_Dopri5Grad);
  * B = 4096: the one-grid launches against the same batch forced into passes by the grid limit
    (1024 workgroups: the forward in two passes; 256: the sweep in two, the forward in eight) — the
    cost of the pass structure itself, parking and re-staging.
Usage: python tools/diag/d5_multipass_time.py [--warmup 3] [--iters 9] [--host-iters 3]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fet_ode_amd as F  # noqa: E402
from fet_ode_amd import _lib  # noqa: E402
from fet_ode_amd import dopri5 as D5  # noqa: E402
from oracle import torch_ref as O  # noqa: E402


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


def case(kind, B, t, dev, train, warmup, iters):
    torch.manual_seed(0)
    m = (F.KANFET if kind == "kanfet" else F.KAN)([2, 10, 2], grid_size=5).to(dev)
    f = F.autonomous(m)
    y0 = O.lv_y0(B, 0).to(dev)

    def infer():
        with torch.no_grad():
            F.odeint(f, y0, t, rtol=1e-3, atol=1e-4)

    def iteration():
        m.zero_grad(set_to_none=True)
        F.odeint(f, y0, t, rtol=1e-3, atol=1e-4).square().sum().backward()

    med, best = timed(iteration if train else infer, warmup, iters)
    last = D5.dopri5_solve.last
    return med, best, last.nfev, type(last).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--host-iters", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    t = torch.tensor(np.linspace(0, 1.0, 11))
    mp0, lim0 = lib.fetode_dopri5_set_multipass(-1), lib.fetode_dopri5_set_grid_limit(0)
    try:
        for kind in ("kanfet", "kan"):
            for B in (8192, 16384):
                for train in (False, True):
                    res = {}
                    for on in (True, False):
                        lib.fetode_dopri5_set_multipass(1 if on else 0)
                        res[on] = case(kind, B, t, dev, train, a.warmup if on else 1, a.iters if on else a.host_iters)
                        med, best, nfev, name = res[on]
                        print(f"{kind} B={B} {'train' if train else 'infer'} switch {'on ' if on else 'off'} [{name}]: "
                              f"median {med:.3f} ms, min {best:.3f} ms, nfev {nfev}", flush=True)
                    print(f"{kind} B={B} {'train' if train else 'infer'}: off / on = {res[False][0] / res[True][0]:.1f}x",
                          flush=True)
        lib.fetode_dopri5_set_multipass(1)
        for kind in ("kanfet", "kan"):
            for train in (False, True):
                base = None
                for limit in (0, 1024, 256):
                    lib.fetode_dopri5_set_grid_limit(limit)
                    med, best, nfev, name = case(kind, 4096, t, dev, train, a.warmup, a.iters)
                    base = med if base is None else base
                    print(f"{kind} B=4096 {'train' if train else 'infer'} grid limit {limit:4d}: median {med:.3f} ms, "
                          f"min {best:.3f} ms, nfev {nfev}, x{med / base:.2f} of the one-grid launch", flush=True)
    finally:
        lib.fetode_dopri5_set_multipass(1 if mp0 else 0)
        lib.fetode_dopri5_set_grid_limit(lim0)


if __name__ == "__main__":
    main()
