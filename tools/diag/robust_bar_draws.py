"""How far do the two count statistics of oracle/parity.py's robust-subset bar spread over equally
valid roundings of the REFERENCE?  CPU only, no GPU code runs.

The bench workload (seed-0 KANFET [2, 10, 2], lv_y0(4096, 0), linspace(0, 3.5, 35)): the reference
fp32 / fp64 solves and the five re-roundings of perturbed_solves(..., 5) (seed 0: three pick the
robust subset, two are the controls) are exactly the legs of
tests/test_gpu_parity.py::test_fused_rk4_kanfet_robust_subset_bench_config.  Each of --draws further
re-roundings (seed --seed, a generator disjoint from seed 0's) then stands in for the GPU solve.
Printed: per stand-in the counts beyond 2e-5 and beyond 1e-5 on the robust subset next to the
controls', the other three parts of the bar, and for m in {1.5, 2, 3} whether every stand-in stays
within m x the worst control's count + 2 (the factor oracle/parity.py robust_parity_parts_ok takes).

  python tools/diag/robust_bar_draws.py [--draws 24] [--seed 1000] [--batch 4096]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=24)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=4096)
    args = ap.parse_args()
    assert args.seed != 0, "seed 0 draws the envelope and the controls"
    import fet_ode_amd as F
    from oracle import parity as P
    from oracle import torch_ref as O
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in F.KANFET([2, 10, 2], grid_size=5).state_dict().items()}
    y0 = O.lv_y0(args.batch, 0)
    t = torch.tensor(np.linspace(0, 3.5, 35))
    with torch.no_grad():
        r32 = O.KANFETRef.from_state_dict(sd, 2)
        e32 = O.odeint(lambda tt, yy: r32(yy), y0, t, method="rk4")
        r64 = O.KANFETRef.from_state_dict(sd, 2).to(torch.float64)
        e64 = O.odeint(lambda tt, yy: r64(yy), y0.double(), t, method="rk4")
    runs = P.perturbed_solves(sd, y0, t, 5)
    rows = []
    for i, sdp in enumerate(P.perturbed_state_dicts(sd, args.draws, seed=args.seed)):
        r = O.KANFETRef.from_state_dict(sdp, 2)
        with torch.no_grad():
            s = O.odeint(lambda tt, yy: r(yy), y0, t, method="rk4")
        st = P.robust_parity(s, e32, e64, runs[:3], runs[3:])
        if i == 0:
            print(f"n_robust {st['n_robust']} of {st['n']}; controls beyond 2e-5 {st['control_n_over_tol_on_robust']}, "
                  f"beyond 1e-5 {st['control_n_over_tol_ref_on_robust']}, max {st['control_max_vs_ref_on_robust']}, "
                  f"well-conditioned spread {st['ref_well_frac_spread']}", flush=True)
        parts = P.robust_parity_parts_ok(st, 1.0)
        rows.append(st)
        print(f"draw {i:2d}: beyond 2e-5 {st['gpu_n_over_tol_on_robust']:3d}  beyond 1e-5 {st['gpu_n_over_tol_ref_on_robust']:3d}  "
              f"max {st['gpu_max_vs_ref_on_robust']:.3e}  frac {st['gpu_frac_within_tol_on_robust']:.4f}  "
              f"well {st['gpu_well_frac']:.4f}  parts(max, frac, well) {parts['max'], parts['frac'], parts['well_frac']}  "
              f"robust_parity_ok {P.robust_parity_ok(st)}  at_tol_ref_ok {P.robust_parity_at_tol_ref_ok(st)}", flush=True)
    print("beyond 2e-5:", sorted(st["gpu_n_over_tol_on_robust"] for st in rows))
    print("beyond 1e-5:", sorted(st["gpu_n_over_tol_ref_on_robust"] for st in rows))
    for m in (1.5, 2, 3):
        ok = [P.robust_parity_parts_ok(st, m) for st in rows]
        print(f"m = {m}: beyond-2e-5 part fails {sum(not o['n_over_tol_gpu'] for o in ok)}, "
              f"beyond-1e-5 part fails {sum(not o['n_over_tol_ref'] for o in ok)} of {len(rows)}")
    for k in ("max", "frac", "well_frac"):
        print(f"part {k}: fails {sum(not P.robust_parity_parts_ok(st)[k] for st in rows)} of {len(rows)}")


if __name__ == "__main__":
    main()
