"""Trajectory-parity statistics for KAN-FET fields (test infrastructure: imported by tests/ and by
bench.py's CPU-reference leg only; nothing here is on the product path).

KAN-FET trajectories are ill-conditioned in fp32: the hysteresis gate amplifies a
1e-7 rounding difference by up to ~1e5 on some trajectories, and WHICH trajectories stay within
1e-5 of fp64 depends on the rounding sequence itself — the reference's own solve re-run with every
parameter moved by a fraction of an ulp (an equally valid fp32 rounding of the same model) keeps a
different subset.  So the strict bar is stated on the ROBUST subset: trajectories that every one of
several equally valid reference roundings keeps within 1e-5 of fp64.  On it the GPU must stay as
close to the reference's fp32 solve as independent re-roundings of the reference itself do
(controls), and the GPU's own well-conditioned fraction must lie within the reference's spread.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import torch_ref as O


def traj_err(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(T, B, D) x2 -> (B,): per trajectory, max over time of ||a_t - b_t|| / ||b_t||."""
    a, b = a.double(), b.double()
    return ((a - b).norm(dim=2) / b.norm(dim=2).clamp_min(1e-30)).max(0).values


def perturbed_state_dicts(sd, n, seed=0, rel=6e-8):
    """n re-roundings of a state dict: every float parameter scaled by (1 + rel * N(0, 1)), the draws
    taken in order from one torch.Generator().manual_seed(seed) (the knot grids stay)."""
    gen = torch.Generator().manual_seed(seed)
    for _ in range(n):
        yield {k: (v * (1 + rel * torch.randn(v.shape, generator=gen)) if v.dtype == torch.float32
                   and "grid" not in k else v) for k, v in sd.items()}


def perturbed_solves(sd, y0, t, n, seed=0, rel=6e-8) -> List[torch.Tensor]:
    """n fp32 reference solves with every float parameter scaled by (1 + rel * N(0, 1))."""
    out = []
    for sdp in perturbed_state_dicts(sd, n, seed, rel):
        r = O.KANFETRef.from_state_dict(sdp, 2)
        with torch.no_grad():
            out.append(O.odeint(lambda tt, yy: r(yy), y0, t, method="rk4"))
    return out


def robust_parity(gpu: torch.Tensor, e32: torch.Tensor, e64: torch.Tensor, envelope: List[torch.Tensor],
                  controls: List[torch.Tensor], tol_ref=1e-5, tol_gpu=2e-5) -> Dict:
    """Statistics of the GPU solve against the reference fp32 solve `e32` on the robust subset
    (e32 and every `envelope` run within `tol_ref` of fp64), next to the same statistics of the
    independent `controls` (re-rounded reference solves not used to pick the subset)."""
    runs = [e32] + list(envelope)
    errs = [traj_err(r, e64) for r in runs]
    robust = torch.stack([e <= tol_ref for e in errs]).all(0)
    g_ref = traj_err(gpu, e32)[robust]
    c_ref = [traj_err(c, e32)[robust] for c in controls]
    fr = [float((e <= tol_ref).double().mean()) for e in errs + [traj_err(c, e64) for c in controls]]
    return {
        "n": int(robust.numel()), "n_robust": int(robust.sum()),
        "gpu_max_vs_ref_on_robust": float(g_ref.max()) if g_ref.numel() else 0.0,
        "gpu_n_over_tol_on_robust": int((g_ref > tol_gpu).sum()),
        # at the north-star bar itself (1e-5 = tol_ref), next to the same count for the controls
        "gpu_n_over_tol_ref_on_robust": int((g_ref > tol_ref).sum()),
        "gpu_frac_within_tol_on_robust": float((g_ref <= tol_gpu).double().mean()) if g_ref.numel() else 1.0,
        "control_max_vs_ref_on_robust": [float(c.max()) if c.numel() else 0.0 for c in c_ref],
        "control_n_over_tol_on_robust": [int((c > tol_gpu).sum()) for c in c_ref],
        "control_n_over_tol_ref_on_robust": [int((c > tol_ref).sum()) for c in c_ref],
        "gpu_well_frac": float((traj_err(gpu, e64) <= tol_ref).double().mean()),
        "ref_well_frac_spread": [min(fr), max(fr)],
        "ref_well_frac": fr[0],
        "tol_ref": tol_ref, "tol_gpu": tol_gpu,
    }


def robust_parity_at_tol_ref_ok(st: Dict) -> bool:
    """The north-star 1e-5 count: on the robust subset no more GPU trajectories leave 1e-5 of the
    reference fp32 solve than the worst independent re-rounding of the reference itself."""
    return st["gpu_n_over_tol_ref_on_robust"] <= max(st["control_n_over_tol_ref_on_robust"] or [0])


def robust_parity_ok(st: Dict) -> bool:
    """The bar: on the robust subset the GPU is no farther from the reference than its own
    re-roundings are (worst case within 1.5x the worst control, no more trajectories beyond
    tol_gpu than the worst control + 2, and >= 97 % of the subset within tol_gpu), and the GPU's
    well-conditioned fraction lies at or above the bottom of the reference's spread."""
    cmax = max(st["control_max_vs_ref_on_robust"] or [0.0])
    cn = max(st["control_n_over_tol_on_robust"] or [0])
    return (st["gpu_max_vs_ref_on_robust"] <= max(1.5 * cmax, st["tol_gpu"])
            and st["gpu_n_over_tol_on_robust"] <= cn + 2
            and st["gpu_frac_within_tol_on_robust"] >= 0.97
            and st["gpu_well_frac"] >= st["ref_well_frac_spread"][0])


def robust_parity_parts_ok(st: Dict, count_factor: float = 1.5) -> Dict[str, bool]:
    """The bar of robust_parity_ok and robust_parity_at_tol_ref_ok part by part, for a solve whose
    rounding sequence differs from the reference's as much as another re-rounding's does (a batch
    cut into shards, each run by another kernel).  The two count parts compare with the worst
    control's count times `count_factor`, + 2: two controls under-sample the spread of those counts
    (tools/diag/robust_bar_draws.py prints it for independent re-roundings), so a
    caller passes the factor measured there.  The other three parts are robust_parity_ok's own."""
    cmax = max(st["control_max_vs_ref_on_robust"] or [0.0])
    cn = max(st["control_n_over_tol_on_robust"] or [0])
    cn_ref = max(st["control_n_over_tol_ref_on_robust"] or [0])
    return {
        "max": st["gpu_max_vs_ref_on_robust"] <= max(1.5 * cmax, st["tol_gpu"]),
        "frac": st["gpu_frac_within_tol_on_robust"] >= 0.97,
        "well_frac": st["gpu_well_frac"] >= st["ref_well_frac_spread"][0],
        "n_over_tol_gpu": st["gpu_n_over_tol_on_robust"] <= count_factor * cn + 2,
        "n_over_tol_ref": st["gpu_n_over_tol_ref_on_robust"] <= count_factor * cn_ref + 2,
    }
