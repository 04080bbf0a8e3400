"""Relative progress of the two waves that share a SIMD in the headline rk4 kernel (B = 4096, 34 steps;
build: make -C fet-ode_amd/csrc progress).
Run: FETODE_LIB=fet-ode_amd/libfetode_progress.so [PHASE_SET=0:0,19:0,0:1] python tools/diag/wave_phase.py
Every wave of the kernel reads s_memtime eight times per solve (entry, tables staged, after steps 1, 9,
17, 25, 34, exit) and stores them with its blockIdx.x, HW_ID and XCC_ID.  Waves are grouped by (XCC, SE,
CU, SIMD); times are compared inside a SIMD only.  Per SIMD pair: the offset of the two waves at every
checkpoint (cycles, ns, evaluation periods: the pair's mean step time / 4), the finish gap and the part
of the solve one wave runs alone, and which static rule tells the two partners apart.
PHASE_SET lists the settings to run one after the other, each skew:prio (fetode_fused_set_wave_skew,
fetode_fused_set_wave_prio); default 0:0, both off."""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import bench
import fet_ode_amd as F
from fet_ode_amd import _lib

CK = ["entry", "staged", "step 1", "step 9", "step 17", "step 25", "step 34", "exit"]
B, ROW = 4096, 16
dev = torch.device("cuda:0")
lib = _lib.load()
lib.fetode_debug_progress_buffer.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
torch.manual_seed(0)
with bench.reproducible_init():
    m = F.KANFET([2, 10, 2], grid_size=5).to(dev)
f = F.autonomous(m)
t = torch.tensor(np.linspace(0, 3.5, 35))
y0 = bench.lv_y0(B, 0).to(dev)
nb = B // 2


def q(x):
    return "mean %9.1f  p10 %9.1f  p50 %9.1f  p90 %9.1f  max %9.1f" % (
        x.mean(), np.percentile(x, 10), np.percentile(x, 50), np.percentile(x, 90), x.max())


def solve_once():
    buf = torch.zeros(nb * ROW, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    _lib.check(lib.fetode_debug_progress_buffer(buf.data_ptr(), nb), "progress buffer")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    F.odeint(f, y0, t, method="rk4")
    e1.record()
    torch.cuda.synchronize()
    _lib.check(lib.fetode_debug_progress_buffer(None, 0), "progress buffer")
    return buf.view(nb, ROW).cpu().numpy(), 1e3 * e0.elapsed_time(e1)


def analyse(rows, us, kus, tag):
    st = rows[:, :8].astype(np.float64)
    blk, hw, xcc = rows[:, 8], rows[:, 9], rows[:, 10]
    slot, simd, cu, sh, se = hw & 15, (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
    assert (blk == np.arange(nb)).all(), "a row was not written: is FETODE_LIB the progress build?"
    key = (((xcc * 8 + se) * 2 + sh) * 16 + cu) * 4 + simd
    order = np.argsort(key, kind="stable")
    uk, cnt = np.unique(key, return_counts=True)
    print(f"--- {tag}: kernel {kus:.1f} us (100 settled launches), this call {us:.1f} us (events); {len(uk)} SIMDs hold waves; waves per SIMD: "
          + ", ".join(f"{c}: {n} SIMDs" for c, n in zip(*np.unique(cnt, return_counts=True))))
    print(f"    placement: {len(np.unique(xcc))} XCC x {len(np.unique(se * 2 + sh))} SE/SH x {len(np.unique(cu))} CU ids x "
          f"{len(np.unique(simd))} SIMDs; wave slots used: {sorted(np.unique(slot).tolist())}")
    pairs = np.array([order[np.searchsorted(key[order], k) + np.arange(2)] for k, c in zip(uk, cnt) if c == 2])
    if len(pairs) == 0:
        print("    no SIMD holds exactly two waves")
        return
    print(f"    pairs analysed: {len(pairs)} of {len(uk)} SIMDs ({100.0 * len(pairs) / len(uk):.1f} %)")
    # leader: the wave that passes the step-34 checkpoint first
    lead_is_0 = st[pairs[:, 0], 6] <= st[pairs[:, 1], 6]
    L = np.where(lead_is_0, pairs[:, 0], pairs[:, 1])
    G = np.where(lead_is_0, pairs[:, 1], pairs[:, 0])
    life = np.maximum(st[L, 7], st[G, 7]) - np.minimum(st[L, 0], st[G, 0])
    ghz = np.median(life) / (kus * 1e3)   # cycles per ns: the pair's lifetime against the kernel's duration
    period = 0.5 * ((st[L, 6] - st[L, 2]) + (st[G, 6] - st[G, 2])) / 33.0 / 4.0
    print(f"    s_memtime rate (median pair lifetime / kernel time) {ghz:.3f} GHz (a lower bound: the kernel time also "
          f"holds dispatch and drain); evaluation period {np.mean(period):.0f} cycles = {np.mean(period) / ghz:.0f} ns")
    print("    offset lagging - leading wave (by the step-34 order), per checkpoint:")
    for k, name in enumerate(CK):
        d = st[G, k] - st[L, k]
        ph = np.abs((d / period + 0.5) % 1.0 - 0.5)   # distance of the offset from a whole number of evaluations
        print(f"      {name:8s} cycles {q(d)}\n               ns     {q(d / ghz)}\n               periods {q(d / period)}"
              f"\n               |offset - nearest whole period| mean {ph.mean():.3f} p50 {np.percentile(ph, 50):.3f} "
              f"(uniform phases: 0.250); pairs within 0.1 period: {100.0 * (ph < 0.1).mean():.1f} %")
    same = 100.0 * np.mean((st[G, 2] >= st[L, 2]) == (st[G, 6] >= st[L, 6]))
    print(f"    the wave ahead after step 1 is the one ahead after step 34 in {same:.1f} % of pairs")
    gap = np.abs(st[G, 7] - st[L, 7])
    print(f"    finish gap: cycles {q(gap)}\n                ns     {q(gap / ghz)}")
    print(f"    share of the pair's lifetime one wave runs alone (start gap + finish gap): "
          f"{100.0 * np.mean((gap + np.abs(st[G, 0] - st[L, 0])) / life):.2f} %")
    stepL, stepG = (st[L, 6] - st[L, 2]) / 33.0, (st[G, 6] - st[G, 2]) / 33.0
    print(f"    mean step time: leading wave {stepL.mean():.0f} cycles, lagging wave {stepG.mean():.0f} cycles "
          f"({100.0 * (stepG.mean() / stepL.mean() - 1.0):+.2f} %)")
    for a_, b_ in ((2, 3), (3, 4), (4, 5), (5, 6)):
        print(f"      steps {CK[a_][5:]:>2s}-{CK[b_][5:]:>2s}: leading {np.mean(st[L, b_] - st[L, a_]):9.0f}  lagging "
              f"{np.mean(st[G, b_] - st[G, a_]):9.0f} cycles")
    print("    static rules (splits: the partners differ in it; lagging: of the split pairs, the wave with the rule true "
          "is the lagging one):")
    rules = [("wave-slot parity", slot & 1), ("blockIdx.x >= gridDim.x / 2", (blk >= nb // 2).astype(np.int64)),
             ("blockIdx.x parity", blk & 1)]
    rules += [(f"blockIdx.x bit {k}", (blk >> k) & 1) for k in range(1, 11)]
    rules += [("later entry stamp", None)]
    for name, r in rules:
        if r is None:
            rl, rg = (st[L, 0] > st[G, 0]).astype(np.int64), (st[G, 0] > st[L, 0]).astype(np.int64)
        else:
            rl, rg = r[L], r[G]
        split = rl != rg
        lag = (rg[split] == 1).mean() if split.any() else float("nan")
        print(f"      {name:30s} splits {100.0 * split.mean():6.2f} %   lagging {100.0 * lag:6.2f} %")
    d_blk = np.abs(blk[L] - blk[G])
    v, c = np.unique(d_blk, return_counts=True)
    top = np.argsort(-c)[:4]
    print("    |blockIdx.x difference| of partners: " + ", ".join(f"{v[i]}: {100.0 * c[i] / len(d_blk):.1f} %" for i in top))


with torch.no_grad():
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:   # clocks settled
        for _ in range(20):
            F.odeint(f, y0, t, method="rk4")
        torch.cuda.synchronize()
    for sk, pr in [[int(x) for x in v.split(":")] for v in os.environ.get("PHASE_SET", "0:0").split(",")]:
        lib.fetode_fused_set_wave_skew(sk)
        lib.fetode_fused_set_wave_prio(pr)
        kus = 1e3 * bench.kernel_time_ms(m, y0, t, reps=100)
        for i in range(int(os.environ.get("PHASE_SOLVES", "3"))):
            rows, us = solve_once()
            analyse(rows, us, kus, f"skew {sk} prio {pr} solve {i}")
