"""What F.odeint returns and leaves behind on the device-resident dopri5 paths of the LV, ECG and wide
families, written to a directory, for a bitwise A/B of two checkouts of the host glue (dopri5.py):
seeded inputs at the smallest shapes the tests use.
  LV KAN and KAN-FET [2,10,2] at B = 1 and 64, fieldn KANFET([2,16,2], K = 12) at B = 16,
  ECG latent 4 / 10 basis functions at B = 4, wide KANFETDynamics(16, hidden 32) at B = 8 (KANFET([8,16,8])
  is refused: fetode_wide_layer_supported needs in, out >= 16; 16 -> 32 is the smallest pair of the wide tests)
  inference (two solves of one module: the first-call and the steady-state memory): sol, every buffer
  of the module after the solve (the hysteresis memory), nfev, n_attempts and the attempt log
  training: the same plus every parameter gradient and the y0 gradient, once with the module's own
  tape size and once with the tape attribute set below the solve's evaluations and attempts (the re-run)
Every solve must have taken a resident path (dopri5_solve.last is a ResidentSolve), or the tool stops.
Usage: python tools/diag/resident_dump.py --out DIR             (one process per checkout)
       python tools/diag/resident_dump.py --compare DIR_A DIR_B (CPU only: exit status 1 on any difference)"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

from driven_dump import compare  # noqa: E402


def _pin(net, seed):
    """The spline weights redrawn from a seeded generator (the module's own come from a least-squares
    fit whose last bits differ between constructions), every tensor scaled like the untrained ETT field."""
    import torch
    gen = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("spline_weight"):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.02)
            if n.endswith(("coef", "base_weight", "spline_weight", "logistic_weight")):
                p.mul_(0.1)


def cases():
    """name -> (build() -> (odeint's func, the module, the tape's owner), y0, t, rtol, atol, the training
    switch or None, the tape attribute, the small tape)."""
    import torch

    import fet_ode_amd as F
    from fet_ode_amd import dopri5 as D5
    from fet_ode_amd import ecg, ett

    out = {}
    t_lv = torch.tensor(np.linspace(0, 1.0, 6))
    for kind in ("kan", "kanfet"):
        g = dict(np.load(os.path.join(REPO, "tests", "golden", f"traj_{kind}.npz"), allow_pickle=False))

        def build(kind=kind, g=g):
            m = (F.KANFET if kind == "kanfet" else F.KAN)([2, 10, 2], grid_size=5)
            m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")})
            return F.autonomous(m), m, m
        for B in (1, 64):
            out[f"lv_{kind}_B{B}"] = (build, torch.from_numpy(g["y0_B64"])[:B].clone(), t_lv, 1e-3, 1e-4, None,
                                      "_fetode_d5tape", (8, 1))

    def fieldn():
        torch.manual_seed(5)
        m = F.KANFET([2, 16, 2], grid_size=5, num_fet_basis=12)
        _pin(m, 5)
        return F.autonomous(m), m, m
    y0 = 0.5 + 2.0 * torch.rand(16, 2, generator=torch.Generator().manual_seed(3))
    out["fieldn_kanfet16_B16"] = (fieldn, y0, t_lv, 1e-3, 1e-4, None, "_fetode_d5tape", (8, 1))

    def ecg_field():
        torch.manual_seed(11)
        f = ecg.No_MLP_KANODEFunc(latent_dim=4, num_basis=10)
        return f, f, f
    h0 = torch.randn(4, 4, generator=torch.Generator().manual_seed(1011)) * 2.0
    out["ecg_l4_nb10_B4"] = (ecg_field, h0, torch.tensor([0.0, 0.3, 0.7, 1.0], dtype=torch.float64), 1e-3, 1e-4,
                             D5.set_resident_ecg_training, "_fetode_d5tape", (4, 1))

    def wide():
        torch.manual_seed(48)
        dyn = ett.KANFETDynamics(16, hidden=32, num_fet_basis=10)
        _pin(dyn.net, 48)
        return dyn, dyn, dyn
    z0 = torch.randn(8, 16, generator=torch.Generator().manual_seed(3)) * 0.6
    out["wide_16_32_B8"] = (wide, z0, torch.tensor(np.linspace(0, 0.5, 3)), 1e-2, 1e-3,
                            D5.set_resident_wide_training, "_fetode_wide_d5tape", (4, 1))
    return out


def dump(out):
    import torch

    import fet_ode_amd as F
    from fet_ode_amd.dopri5 import ResidentSolve

    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda:0")

    def save(name, mod, sol, **more):
        s = F.dopri5.dopri5_solve.last
        if not isinstance(s, ResidentSolve):
            sys.exit(f"{name}: the solve took {type(s).__name__}, not a resident path")
        arrs = dict(sol=sol, nfev=torch.tensor([s.nfev]), n_attempts=torch.tensor([s.n_attempts]),
                    attempts=torch.tensor([[a[0], a[1], a[2], float(a[3])] for a in s.attempts], dtype=torch.float64))
        arrs.update({"buf/" + n: b for n, b in mod.named_buffers()})
        arrs.update(more)
        np.savez(os.path.join(out, name + ".npz"), **{k: v.detach().cpu().numpy() for k, v in arrs.items()})
        print(f"{name}: nfev {s.nfev}, attempts {s.n_attempts}", flush=True)

    for name, (build, y0, t, rtol, atol, switch, attr, small) in cases().items():
        func, mod, owner = build()
        mod.to(dev)
        with torch.no_grad():
            for call in (0, 1):
                sol = F.odeint(func, y0.to(dev), t, rtol=rtol, atol=atol)
                save(f"{name}_infer{call}", mod, sol)
        w = torch.randn(len(t), *y0.shape, generator=torch.Generator().manual_seed(2)).to(dev)
        for label, tape in (("roomy", None), ("rerun", small)):
            func, mod, owner = build()
            mod.to(dev)
            if tape is not None:
                setattr(owner, attr, tape)
            yg = y0.to(dev).clone().requires_grad_(True)
            prev = switch(True) if switch is not None else None
            try:
                sol = F.odeint(func, yg, t, rtol=rtol, atol=atol)
                save_args = dict(tape_next=torch.tensor(getattr(owner, attr)))
                (w * sol).sum().backward()
            finally:
                if switch is not None:
                    switch(prev)
            grads = {"grad/" + n: p.grad for n, p in mod.named_parameters() if p.grad is not None}
            save(f"{name}_train_{label}", mod, sol, gy0=yg.grad, **save_args, **grads)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--out", metavar="DIR")
    mode.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else dump(a.out))
