"""Every output of every C entry of the input-driven Ferro field, written to a directory, for a bitwise
A/B of two builds of the library (FETODE_LIB selects it): seeded inputs at the shapes (H, D, K, T) of
tests/test_gpu_driven_methods.py, B = 1, 3, 5, forced 1 / 2 / 4 samples per workgroup.
  fixed and grid (euler, midpoint, rk4, rk4_classic): sol, prev_out, both tapes, adj, grad_h0, adj_u
  dopri5 and dopri5_tape: sol, prev_out, stats, the attempt log, the evaluation log, every tape array
  dopri5_backward and dopri5_backward_x with step_grad 0 and 1: adj, grad_h0, adj_u
  param_grad in both tape layouts (over the fixed-layout tape once per method, at 1 sample per workgroup:
  the tapes and adj it reads are themselves dumped, and compared, in all three variants), table and
  table_backward
Every buffer is filled (NaN, or zeros where a later pass sums it) before the launch that writes it, so
a word the library leaves alone compares equal too.
Usage: python tools/diag/driven_dump.py --out DIR          (one process per library)
       python tools/diag/driven_dump.py --compare DIR_A DIR_B   (CPU only: exit status 1 on any difference)"""
import argparse
import ctypes
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SHAPES = [(8, 1, 3, 2), (8, 2, 3, 5), (24, 3, 12, 5), (64, 1, 10, 4), (64, 4, 16, 3)]
BATCHES = (1, 3, 5)
SPW = (1, 2, 4)
METHODS = ("euler", "midpoint", "rk4", "rk4_classic")
MAX_ATT = 96


def compare(da, db):
    fa, fb = (sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "*.npz"))) for d in (da, db))
    bad = 0 if fa == fb and fa else 1
    if bad:
        print(f"file lists differ or are empty: {len(fa)} against {len(fb)}")
    n_arr = n_word = 0
    for name in sorted(set(fa) & set(fb)):
        a, b = np.load(os.path.join(da, name)), np.load(os.path.join(db, name))
        if sorted(a.files) != sorted(b.files):
            print(f"{name}: keys differ")
            bad += 1
            continue
        for k in a.files:
            va, vb = a[k], b[k]
            n_arr += 1
            n_word += va.size
            # bit patterns: NaN positions (and payloads) and signed zeros count
            same = va.shape == vb.shape and va.dtype == vb.dtype and np.array_equal(
                va.view(np.uint8) if va.size else va, vb.view(np.uint8) if vb.size else vb)
            if not same:
                bad += 1
                nd = int((va != vb).sum()) if va.shape == vb.shape else -1
                print(f"{name}: {k} differs ({nd} of {va.size} values)")
    print(f"{len(fa)} files, {n_arr} arrays, {n_word} values compared: "
          f"{'identical' if not bad else '%d DIFFERENCES' % bad}")
    return 1 if bad else 0


def dump(out):
    import torch
    from fet_ode_amd import _lib, ecg
    from fet_ode_amd.dopri5 import _TABLEAU, _opts_array
    from fet_ode_amd.odeint import FIXED_METHODS, get_schedule

    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    print("library:", _lib.LIB_PATH, flush=True)
    nan = float("nan")
    tab = _TABLEAU.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def full(*shape, v=nan, dtype=torch.float32):
        return torch.full(shape, v, device=dev, dtype=dtype)

    def save(name, **arrs):
        np.savez(os.path.join(out, name + ".npz"), **{k: v.detach().cpu().numpy() for k, v in arrs.items()})

    for H, D, K, T in SHAPES:
        In = H + D
        g = torch.Generator().manual_seed(1000 * H + 100 * D + 10 * K + T)
        f = ecg.InputDrivenKANODEFunc(D, H, K)
        with torch.no_grad():
            for n, (s, o) in dict(k=(2, 0.5), Ec=(2, 0.5), Ps=(1.5, 0.5)).items():
                getattr(f.basis, n).copy_(torch.rand(In, H, K, generator=g) * s + o)
            f.basis.bias.copy_(torch.randn(In, H, K, generator=g) * 0.1)
            f.basis.coef.copy_(torch.randn(In, H, K, generator=g))
            f.gain.copy_(1.0 + 0.2 * torch.randn(H, generator=g))
            f.bias.copy_(0.1 * torch.randn(H, generator=g))
        f = f.to(dev)
        plan, d, keep = ecg._driven_plan(f, dev)
        params = [_lib.f32c(p.detach()) for p in ecg._driven_tensors(f)]
        tc = torch.linspace(0.0, 1.0, steps=T)
        tg = tc.to(dev)
        x_all = torch.randn(5, T, D, generator=g)
        h_all = torch.randn(5, H, generator=g)
        p_all = torch.randn(5, In, generator=g)
        for B in BATCHES:
            tag = f"H{H}_D{D}_K{K}_T{T}_B{B}"
            x, h0, prev0 = (v[:B].to(dev).contiguous() for v in (x_all, h_all, p_all))

            # ---- table and its backward, fixed and grid in every method and samples-per-workgroup variant
            for fam, method in [("fixed", "rk4")] + [("grid", m) for m in METHODS]:
                code = FIXED_METHODS[method]
                if fam == "fixed":
                    _, tq, coef = ecg._driven_grid(tc, dev)
                    n_steps = T - 1
                else:
                    sched = get_schedule(tc, None, False)
                    tq, coef, _ = ecg._driven_grid_arrays(sched, code, dev)
                    n_steps = sched.n_steps
                ne = tq.numel()
                u = ecg.driven_table(tg, x, tq)
                gsol = torch.randn(n_steps + 1, B, H, generator=g).to(dev)
                gu = torch.randn(ne, B, D, generator=g).to(dev)
                save(f"{tag}_{fam}_{method}_table", u=u, gx=ecg.driven_series_grad(tq, 0, tg, gu, B, ne, 1, B, None, 0, D))
                for v in SPW:
                    prev = ecg.set_driven_samples_per_workgroup(v)
                    try:
                        r = {}
                        for tape in (False, True):
                            sol, pout = full(n_steps, B, H), full(B, In)
                            args = [ctypes.byref(d), plan.data_ptr(), code, h0.data_ptr(), B, u.data_ptr(), ne, 0,
                                    coef.data_ptr(), n_steps, prev0.data_ptr(), sol.data_ptr(), pout.data_ptr()]
                            name = f"fetode_driven_{fam}" + ("_tape" if tape else "")
                            if tape:
                                thx, tphi = full(ne, B, In), full(ne, B, H)
                                args += [thx.data_ptr(), tphi.data_ptr()]
                                r.update(tape_hx=thx, tape_phi=tphi)
                            _lib.check(getattr(lib, name)(*args, None), name)
                            r.update({"sol" + "_tape" * tape: sol, "prev_out" + "_tape" * tape: pout})
                        for xg in (False, True):
                            adj, gh0, adj_u = full(ne, B, H), full(B, H), full(ne, B, D)
                            args = [ctypes.byref(d), plan.data_ptr(), code, B, coef.data_ptr(), n_steps, prev0.data_ptr(),
                                    r["tape_hx"].data_ptr(), r["tape_phi"].data_ptr(), gsol.data_ptr(), adj.data_ptr(),
                                    gh0.data_ptr()] + ([adj_u.data_ptr()] if xg else [])
                            name = f"fetode_driven_{fam}_backward" + ("_x" if xg else "")
                            _lib.check(getattr(lib, name)(*args, None), name)
                            r.update({"adj" + "_x" * xg: adj, "grad_h0" + "_x" * xg: gh0})
                            if xg:
                                r["adj_u"] = adj_u
                        if v == 1:   # the parameter sums over the (n_ev, B, .) tape
                            pg = ecg.driven_param_grads(d, params, [True] * 7, B, ne, 1, B, None, 0, prev0, r["tape_hx"],
                                                        r["tape_phi"], r["adj"])
                            r.update({f"pgrad{i}": t for i, t in enumerate(pg)})
                        save(f"{tag}_{fam}_{method}_spw{v}", **r)
                    finally:
                        ecg.set_driven_samples_per_workgroup(prev)

            # ---- dopri5: untaped (with the evaluation log), taped, the sweeps, the sums over the (B, max_ev, .) tape
            for oname, options in (("probe", {}), ("first", {"first_step": 0.05})):
                opts = _opts_array(options)
                optp = opts.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
                rtol, atol, max_ev = 1e-3, 1e-4, 2 + 6 * MAX_ATT
                r = {}
                for tape in (False, True):
                    sol, pout = full(T, B, H), full(B, In)
                    stats, att = full(B, 3, v=-1, dtype=torch.int32), full(B, MAX_ATT, 4, dtype=torch.float64)
                    args = [ctypes.byref(d), plan.data_ptr(), h0.data_ptr(), B, x.data_ptr(), tg.data_ptr(), T, rtol, atol,
                            optp, tab, prev0.data_ptr(), sol.data_ptr(), pout.data_ptr(), stats.data_ptr(), att.data_ptr(),
                            MAX_ATT]
                    if tape:
                        thx, tphi, tt, tsl = full(B, max_ev, In), full(B, max_ev, H), full(B, max_ev), full(B, max_ev, D)
                        init = full(B, 5, dtype=torch.float64)
                        args += [thx.data_ptr(), tphi.data_ptr(), tt.data_ptr(), tsl.data_ptr(), init.data_ptr(), max_ev]
                        name = "fetode_driven_dopri5_tape"
                        r.update(tape_hx=thx, tape_phi=tphi, tape_t=tt, tape_slope=tsl, init_rec=init)
                    else:
                        evlog = full(B, max_ev, 1 + D)
                        args += [evlog.data_ptr(), max_ev]
                        name = "fetode_driven_dopri5"
                        r["evlog"] = evlog
                    _lib.check(getattr(lib, name)(*args, None), name)
                    sfx = "_tape" * tape
                    r.update({"sol" + sfx: sol, "prev_out" + sfx: pout, "stats" + sfx: stats, "att" + sfx: att})
                stats, att = r["stats_tape"], r["att_tape"]
                gsol = torch.randn(T, B, H, generator=g).to(dev)
                for sg in (0, 1):
                    for xg in (False, True):
                        adj, gh0, adj_u = full(B, max_ev, H), full(B, H), full(B, max_ev, D)
                        args = [ctypes.byref(d), plan.data_ptr(), B, tg.data_ptr(), T, rtol, atol, optp, tab,
                                prev0.data_ptr(), stats.data_ptr(), att.data_ptr(), MAX_ATT, r["tape_hx"].data_ptr(),
                                r["tape_phi"].data_ptr(), r["tape_slope"].data_ptr(), r["init_rec"].data_ptr(), max_ev,
                                gsol.data_ptr(), sg, adj.data_ptr(), gh0.data_ptr()] + ([adj_u.data_ptr()] if xg else [])
                        name = "fetode_driven_dopri5_backward" + ("_x" if xg else "")
                        _lib.check(getattr(lib, name)(*args, None), name)
                        k = f"_sg{sg}" + "_x" * xg
                        r.update({"adj" + k: adj, "grad_h0" + k: gh0})
                        if xg:
                            r["adj_u" + k] = adj_u
                nfev = stats[:, 0].tolist()
                ne = min(max(nfev), max_ev)
                if ne > 0 and not bool(stats[:, 2].any()):
                    pg = ecg.driven_param_grads(d, params, [True] * 7, B, ne, max_ev, 1, stats, 3, prev0, r["tape_hx"],
                                                r["tape_phi"], r["adj_sg1"])
                    r.update({f"pgrad{i}": t for i, t in enumerate(pg)})
                    r["gx"] = ecg.driven_series_grad(r["tape_t"], max_ev, tg, r["adj_u_sg1_x"], B, ne, max_ev, 1, stats, 3, D)
                print(f"{tag} dopri5 {oname}: nfev {nfev}, status {stats[:, 2].tolist()}", flush=True)
                save(f"{tag}_dopri5_{oname}", **r)
        torch.cuda.synchronize()
        print(f"shape {(H, D, K, T)} done", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--out", metavar="DIR")
    mode.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else dump(a.out))
