// fetode_bwd.hip — the reverse sweep of the single-launch fixed-grid integrator (training).
//
// What it replaces: loss.backward() through torchdiffeq's fixed-grid solve of a KAN / KAN-FET
// field (train_kanfet_node_predprey.py:254-257), i.e. reverse-mode autograd through every stage
// evaluation (KANLinear.forward efficientkan.py:160-182, FerroelectricBasis.forward
// ferro_class.py:368-420 whose prev_x / branch_sign snapshots are detached, :381-382), the
// rk_common.rk4_alt_step_func stage combines and FixedGridODESolver's output interpolation.
//
// Data flow.  The forward kernel (fetode_fused.hip) records the two layer inputs of every
// evaluation on a "tape" (n_evals, B, D + H); the hysteresis input of evaluation ev is the tape
// row of ev - 1 (ferro_class.py:409), or the state before the solve for ev = 0.  So the sweep
// recomputes nothing but per-input features: one wave owns one trajectory and walks its
// evaluations backwards, carrying the adjoints of y and of the stage derivatives k_j.
//
// Per evaluation (layer 1 then layer 0, lanes = jobs):
//   features   per input: SiLU, SiLU', dense B-spline bases, knot interval/coordinate, the
//              hysteresis gate u = sigmoid(gs(x - prev)); per (input, basis): the logistic sigmoid
//   Ferro      per element (i, o, k): the element's forward quantities and its VJP; parameter
//              gradients are accumulated in three per-element sums A, C, E (see below)
//   KAN edges  per (o, i): base + spline-coefficient sums, d/dx via the plan's cubic tables
//   logistic   per (i, j): the logistic-weight sums and the a / b gradients
//   d out/d x  per-job contributions land in an LDS table and are summed per input in a fixed
//              order (segmented sum + xor shuffles): run-to-run deterministic, no atomics.
// The gradient sums live in VGPRs for the whole sweep (each lane owns fixed slots), are written
// once per block to a partial buffer, reduced over blocks in a fixed order (fp64), and turned
// into parameter gradients by one small kernel:
//   Ferro e = (i,o,k):  A = sum g_o th,  C = sum g_o (1-th^2) sh,  E = sum g_o (1-th^2)(m + Ec dm/dEc),
//                       G_o = sum g_o   ->  dk = coef Ps C, dEc = coef Ps k E, dPs = coef A,
//                       dbias = coef G_o, dcoef = Ps A + bias G_o
//   KAN (o,i):          base = sum g_o SiLU(x_i), spline_c = sum g_o B_c(x_i)
//   logistic (o,i,j):   sum g_o sigmoid_ij;  a_ij, b_ij directly.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "fetode_common.h"
#include "fetode_dopri_ctl.h"

using namespace fetode;

namespace {

#include "fetode_gridsum.h"

#include "fetode_bwd_dev.h"

// ACC = true: the whole reverse sweep in one kernel — adjoints and the parameter-gradient sums (in
// VGPRs, one partial row per wave).  ACC = false: the adjoint sweep only (no sums: 114 VGPRs, four
// waves per SIMD, all B = 4096 trajectories resident at once); it records every evaluation's
// output and hidden adjoints in a.gadj and param_sum_kernel forms the sums in parallel.
// TPW trajectories per wave: lane l serves trajectory tt = l / (64 / TPW) in the per-input phases
// (tape, features, d out/d x sums, adjoint scalars) and owns its job slots for all TPW of them in
// the VJP phases, so the gradient sums do not grow with TPW.  TPW = 2 halves the waves (B = 4096:
// 2 048 waves = every trajectory resident in one round at the sums' 2 waves per SIMD).
template <int D, int H, int K, int NB, int NG, bool FERRO, bool ACC, int TPW>
__global__ __launch_bounds__(64 * kTPB) __attribute__((amdgpu_waves_per_eu(ACC ? FETODE_BWD_WAVES : 4))) void fixed_bwd_kernel(BwdArgs a) {
  using L0 = BL<D, H, K, NB, NG, FERRO>;
  using L1 = BL<H, D, K, NB, NG, FERRO>;
  constexpr int W = D + H, NS = NG - 1 - kSO, HALF = 64 / TPW;
  constexpr int CB = L0::IN * L0::NTMP > L1::IN * L1::NTMP ? L0::IN * L0::NTMP : L1::IN * L1::NTMP;
  static_assert(CB % 2 == 0 && L0::NTMP % 2 == 0 && L1::NTMP % 2 == 0, "8-byte pair stores into the cb table");
  // PF: features are adjoint-free, so they are formed for two evaluations at once (ev on lanes
  // [0, FH) of a trajectory's half, ev - 1 on [FH, HALF)) every other evaluation, into LDS buffers
  // indexed by evaluation parity: the per-input phase's instructions serve twice the lanes.  Only
  // the Ferro sweep with sums pairs them (the others would lose occupancy to the second buffer).
  constexpr bool PF = FERRO && ACC && 2 * W <= HALF;
  constexpr int FH = PF ? HALF / 2 : HALF, NBUF = PF ? 2 : 1;
  static_assert(W <= FH && (TPW == 1 || TPW == 2 || TPW == 4), "one lane per input of each trajectory and evaluation");
  __shared__ BInTab<W, NG, NB> TI;
  __shared__ BTab<L0> T0;
  __shared__ BTab<L1> T1;
  using FB = BFeat<W, NS, NB, PF>;
  __shared__ FB sF[kTPB][NBUF][TPW];
  __shared__ __attribute__((aligned(16))) float s_cb[kTPB][TPW][CB];  // f2 stores (pairs)
  __shared__ float s_g1[kTPB][TPW][D], s_g0[kTPB][TPW][H], s_gx[kTPB][TPW][D];
  __shared__ float s_ak[kTPB][TPW][4][D], s_ay[kTPB][TPW][D], s_ac[kTPB][4][3];

  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tt = lane / HALF, sl = lane % HALF;  // this lane's trajectory in the per-input phases
  const int fb = sl / FH, fsl = sl % FH;          // feature lanes: evaluation ev - fb, input fsl
  TI.stage(a.plan, a.P0, a.P1, D, threadIdx.x, 64 * kTPB);
  T0.stage(a.k0, a.f0, a.plan, a.P0, threadIdx.x, 64 * kTPB);
  T1.stage(a.k1, a.f1, a.plan, a.P1, threadIdx.x, 64 * kTPB);
  BReg<L0> R0;
  BReg<L1> R1;
  if constexpr (ACC) {
    R0.zero();
    R1.zero();
  }
  __syncthreads();  // tables staged; from here on every wave syncs only with itself

  float* cbs = &s_cb[wid][0][0];
  float* g1s = &s_g1[wid][0][0];  // layer-1 output adjoint = d loss / d k_stage
  float* g0s = &s_g0[wid][0][0];  // layer-0 output adjoint = d loss / d h
  float* gxs = &s_gx[wid][0][0];
  float(&ak)[4][D] = s_ak[wid][tt];
  float(&ay)[D] = s_ay[wid][tt];
  float(&acs)[4][3] = s_ac[wid];
  const float gs0 = (float)a.f0.gate_slope, gs1 = (float)a.f1.gate_slope;
  const float gl0 = a.P0.gsl2e, gl1 = a.P1.gsl2e, wc0 = a.P0.wc, wc1 = a.P1.wc;
  const float glane = fsl < D ? gl0 : gl1, wlane = fsl < D ? wc0 : wc1, slane = fsl < D ? gs0 : gs1;  // the feature lane's layer
  const int ns = a.method == FETODE_RK4 || a.method == FETODE_RK4_CLASSIC ? 4 : a.method == FETODE_MIDPOINT ? 2 : 1;
  const int64_t tstride = a.B * W;
  const int n_ev = a.n_steps * ns;

  for (int64_t b0 = ((int64_t)blockIdx.x * kTPB + wid) * TPW; b0 < a.B; b0 += (int64_t)gridDim.x * kTPB * TPW) {
    // this lane's trajectory; a missing partner (B odd) runs on zeros: finite inputs, zero
    // adjoints, exact-zero contributions to every sum
    const int64_t b = b0 + tt;
    const bool live = b < a.B;
    const int64_t bc_ = live ? b : b0;
    // the hysteresis input of evaluation ev is the layer input of ev - 1 (ferro_class.py:409)
    // (any ev < 0 reads the state before the solve: the paired feature lanes of a last pair (0, -1)
    // fill a buffer nothing reads)
    auto tape_at = [&](int ev) -> float {
      if (fsl >= W || !live) return 0.f;
      if (ev >= 0) return a.tape[(int64_t)ev * tstride + b * W + fsl];
      const float v = a.tape[b * W + fsl];  // before evaluation 0: the stored state / reinit rule
      if (fsl < D) return (a.init_mask & 1u) ? v : (FERRO ? a.state0[b * D + fsl] : 0.f);
      return (a.init_mask & 2u) ? v : (FERRO ? a.state0[a.B * D + b * H + (fsl - D)] : 0.f);
    };
    // this feature lane's layer input and hysteresis input, for evaluation ev - fb of the next pair
    float cur = tape_at(n_ev - 1 - fb), prv = tape_at(n_ev - 2 - fb);
    float ay1 = 0.f;  // adjoint of y at the end of the current step (lanes sl < D)
    int jj = a.T - 1;
    for (int s = a.n_steps - 1; s >= 0; --s) {
      float bc[4], ac[4][3];
      step_coefs(a.method, a.step_coef[4 * s], a.step_coef[4 * s + 1], a.step_coef[4 * s + 2], bc, ac);
      // outputs produced in this step (FixedGridODESolver: y at step start, end, or interpolated)
      float ay0x = 0.f;
      for (; jj >= 1 && a.out_step[jj] == s; --jj) {
        if (sl < D) {
          const float g = live ? a.gsol[((int64_t)jj * a.B + bc_) * D + sl] : 0.f;
          const int mode = a.out_mode[jj];
          if (mode == 0) {
            ay0x += g;
          } else if (mode == 1) {
            ay1 += g;
          } else {
            const float slo = a.out_slope[jj];
            ay1 = ffma(slo, g, ay1);
            ay0x = ffma(1.0f - slo, g, ay0x);
          }
        }
      }
      if (sl < D) {
        for (int j = 0; j < ns; ++j) ak[j][sl] = bc[j] * ay1;
        ay[sl] = ay1 + ay0x;
      }
      if (lane == 0) {  // through LDS: the stage index below is a runtime value
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) acs[i][j] = ac[i][j];
      }
      for (int st = ns - 1; st >= 0; --st) {
        const int ev = s * ns + st;
        // table reads are re-issued every evaluation (an opaque zero offset stops the compiler
        // from hoisting ~100 loop-invariant LDS values into VGPRs, which halves occupancy)
        int z = 0;
        asm volatile("" : "+s"(z));
        // features of evaluations ev and ev - 1 (every other evaluation; wave-uniform)
        const bool fstep = !PF || ((n_ev - 1 - ev) & 1) == 0;
        float nx1 = 0.f, nx2 = 0.f;
        FB& FF = sF[wid][PF ? (ev - fb) & 1 : 0][tt];
        if (fstep) {
          if constexpr (PF) {  // prefetch: consumed by the next pair
            nx1 = tape_at(ev - fb - 2);
            nx2 = tape_at(ev - fb - 3);
          } else {  // the next evaluation's layer input is this one's hysteresis input
            nx1 = prv;
            nx2 = tape_at(ev - 2);
          }
          if (fsl < W) {
            FF.x[fsl] = cur;
            FF.pv[fsl] = prv;
          }
        }
        if (sl < D) g1s[tt * D + sl] = ak[st][sl];
        wsync();
        if (fstep) {
          // both layers' inputs on one code path over the combined input index
          if (!(FETODE_EXP_SKIP & 8) && fsl < W) feat_input<W, NG, NB, PF>(FF, TI, fsl, glane, wlane, slane, z);
          if (!(FETODE_EXP_SKIP & 8)) {
            constexpr int NSG = TPW * W * NB, RSG = (NSG + 63) / 64;
#pragma unroll
            for (int pb = 0; pb < NBUF; ++pb) {  // one parity buffer at a time (register pressure)
              FB* Fp = sF[wid][pb];
              float sa[RSG], sb[RSG], sx[RSG];
#pragma unroll
              for (int k = 0; k < RSG; ++k) {  // every round's operands read before any sigmoid
                const int q = lane + 64 * k, qc = q < NSG ? q : 0;
                const int qt = qc / (W * NB), qq = qc % (W * NB);
                const float2 ab = *reinterpret_cast<const float2*>(&TI.lg[2 * qq + z]);  // one 8-byte read
                sa[k] = ab.x;
                sb[k] = ab.y;
                sx[k] = Fp[qt].x[qq / NB];
              }
#pragma unroll
              for (int k = 0; k < RSG; ++k) {
                const int q = lane + 64 * k;
                if (q < NSG) {
                  const int qt = q / (W * NB), qq = q % (W * NB);
                  Fp[qt].sg[qq] = sigm_l2(ffma(sa[k], sx[k], sb[k]));
                }
              }
            }
          }
          wsync();
          cur = nx1;
          prv = nx2;
        }
        FB* Fs = sF[wid][PF ? ev & 1 : 0];
        layer_jobs<L1, D, ACC, TPW, D, CB>(Fs, g1s, T1, TI.rh, R1, cbs, gl1, wc1, gs1, lane, z);
        wsync();
        reduce_gin<L1, TPW, H, CB>(cbs, g0s, lane);  // d loss / d h
        wsync();
        if constexpr (!ACC) {  // this evaluation's adjoints for param_sum_kernel
          if (live) {
            float* gr = a.gadj + ((int64_t)ev * a.B + b) * W;
            if (sl < D) gr[sl] = g1s[tt * D + sl];
            else if (sl < W) gr[sl] = g0s[tt * H + sl - D];
          }
        }
        layer_jobs<L0, 0, ACC, TPW, H, CB>(Fs, g0s, T0, TI.rh, R0, cbs, gl0, wc0, gs0, lane, z);
        wsync();
        reduce_gin<L0, TPW, D, CB>(cbs, gxs, lane);
        wsync();
        if (sl < D) {
          const float ax = gxs[tt * D + sl];
          ay[sl] += ax;
          for (int j = 0; j < st; ++j) ak[j][sl] = ffma(acs[st][j], ax, ak[j][sl]);
        }
        wsync();
      }
      ay1 = sl < D ? ay[sl] : 0.f;
    }
    if (sl < D && live && a.gy0) a.gy0[b * D + sl] = ay1 + a.gsol[b * D + sl];  // solution[0] = y0
    wsync();
  }
  if constexpr (ACC) {
    float* part = a.part + ((int64_t)blockIdx.x * kTPB + wid) * a.nacc;
    R0.template store<TPW>(part, lane);
    R1.template store<TPW>(part + L0::AL.n, lane);
  }
}

// =============================================================================================
// The reverse sweep of the device-resident dopri5 solve: loss.backward() through the reference's
// own training call, odeint(calDeriv, X0, t_learn) with torchdiffeq's default dopri5
// (train_kanfet_node_predprey.py:252-257), i.e. reverse-mode autograd through every evaluation of
// every attempt (rejected ones included), the stage sums, the error norm and the step-size
// control (rk_common._runge_kutta_step / _optimal_step_size, misc._select_initial_step /
// _rms_norm, interp._interp_fit / _interp_evaluate — nothing in torchdiffeq detaches dt).
//
// Tape (fetode_integrate_dopri5_tape): per evaluation its two layer inputs (as the fixed-grid
// tape) and its output k; per attempt (t0, dt, error ratio, accepted); the initial-step scalars.
// Evaluation order: 0 = f(y0), 1 = the initial-step probe (absent with first_step), then six per
// attempt (stages 2..7; stage 7's input is the attempt's y1, its output the next f0).
//
// One wave owns TPW trajectories and walks the evaluations backwards exactly like
// fixed_bwd_kernel (same per-evaluation VJP, gradient sums in VGPRs); the lanes sl < D of a
// trajectory carry its state adjoints.  The adjoint of dt couples the batch (the error ratio is a
// norm over every element), so every attempt ends with one grid-wide fixed-order fp64 sum
// (grid_sum2) of the per-element d/d dt terms — the whole grid is resident.  Per attempt n, in
// reverse, with dt_{n+1}'s adjoint known:
//   control   dt_{n+1} = clamp(dt_n * min(ifactor, max(safety ratio^-1/5, dfactor)))
//             -> adjoint of ratio_n and dt_n's direct part
//   outputs   (accepted) every output t_i in (t0, t1]: the interpolant's coefficient adjoints and
//             d out/d x, x = (t_i - t0s)/(t1s - t0s) -> d/d t0, d/d dt (grid sums)
//   element   interp fit, error ratio (err / tol, tol = atol + rtol max(|y|, |y1|)) and the stage
//             sums -> adjoints of k_1..k_7, y and dt; evaluations 7..2 by VJP
//   carry     y's adjoint and f0's (= k_1's) to the attempt that produced them
// After attempt 0: _select_initial_step's adjoint (one more grid sum, through the probe).
// =============================================================================================

template <int D, int H, int K, int NB, int NG, bool FERRO, int TPW>
__global__ __launch_bounds__(64 * kTPB) __attribute__((amdgpu_waves_per_eu(FETODE_BWD_WAVES))) void dopri_bwd_kernel(DopriBwdArgs da) {
  constexpr bool MP = TPW < 0;   // false, as a value-dependent constant: the MP statements are discarded
#include "fetode_dopri_bwd_body.h"
}

// Parameter-gradient sums of one layer from the recorded adjoints (after fixed_bwd_kernel<ACC =
// false>): every sample (evaluation ev, trajectory b) is independent, so the sums are formed
// element-major — a thread owns fixed jobs of the layer (a Ferro element, a KAN edge, one or two
// logistic (input, basis) pairs) with their sums in a few VGPRs, and walks its block's samples in
// tiles of TS whose per-input features (SiLU, dense B-spline bases, hysteresis gate, logistic
// sigmoids) are computed once per tile into LDS.  The per-sample arithmetic is layer_jobs'; only
// the summation order differs (per block, samples in (ev, b) order; blocks in a fixed order).
// Jobs (256 threads): Ferro element e = tid (E = 200); edge q = tid - E (NE = 20; the i = 0 edge of
// output o also sums G_o); logistic (i, j) jobs tid - E - NE and, if NL exceeds what is left, a
// second one on threads 0.. (L1: 36 + 64 of 100).
// FE = false (after sweep7_kernel, which keeps the Ferro sums itself): the KAN sums only — no
// hysteresis inputs fetched, no Ferro jobs (edges on threads 0.., logistic jobs after them), the
// Ferro slots of the block's row written as zeros.
constexpr int kPsTS = 32;  // samples per tile
template <int D, int H, int K, int NB, int NG, int LAYER, bool FE = true>
__global__ __launch_bounds__(256) void param_sum_kernel(BwdArgs a) {
  using LA = BL<D, H, K, NB, NG, true>;
  using LB = BL<H, D, K, NB, NG, true>;
  using L = typename std::conditional<LAYER == 0, LA, LB>::type;
  constexpr int W = D + H, NS = NG - 1 - kSO, NI = NG - 1, TS = kPsTS;
  constexpr int IN = L::IN, OUT = L::OUT, E = L::E, NE = L::NE, NL = L::NL;
  constexpr int TB = LAYER == 0 ? 0 : D;          // the layer's inputs in a tape row
  constexpr int GB = LAYER == 0 ? D : 0;          // its output adjoints in a gadj row (h | k)
  constexpr int EJ = FE ? E : 0;                   // Ferro jobs of this launch
  constexpr int J1 = 256 - EJ - NE;                // logistic jobs of the first round
  static_assert(EJ + NE <= 256 && NL <= J1 + 64 && (NL <= J1 || NL - J1 <= EJ), "param_sum job map");
  constexpr AccLayout AL = L::AL;
  __shared__ BInTab<W, NG, NB> TI;
  __shared__ BTab<L> Tb;
  __shared__ float sx[TS][IN], sup[TS][IN], ssl[TS][IN], sgo[TS][OUT];
  __shared__ float sbd[TS][IN][NS + 1];            // +1: no bank aliasing between inputs
  __shared__ float ssg[TS][IN * NB];
  const int tid = threadIdx.x;
  const LayerPlan& P = LAYER == 0 ? a.P0 : a.P1;
  TI.stage(a.plan, a.P0, a.P1, D, tid, 256);
  Tb.stage(LAYER == 0 ? a.k0 : a.k1, LAYER == 0 ? a.f0 : a.f1, a.plan, P, tid, 256);
  const float gsl = P.gsl2e, wc = P.wc, gs = (float)(LAYER == 0 ? a.f0.gate_slope : a.f1.gate_slope);
  const uint32_t imask = (a.init_mask >> LAYER) & 1u;
  const int64_t N = (int64_t)a.n_steps * (a.method == FETODE_RK4 || a.method == FETODE_RK4_CLASSIC ? 4
                                          : a.method == FETODE_MIDPOINT ? 2 : 1) * a.B;
  const int64_t n0 = (int64_t)blockIdx.x * N / gridDim.x, n1 = (int64_t)(blockIdx.x + 1) * N / gridDim.x;
  __syncthreads();

  // this thread's jobs and their constants
  const bool fjob = tid < EJ;
  const int e = fjob ? tid : 0, fi = e / (OUT * K), fo = (e % (OUT * K)) / K;
  const float4 fpa = Tb.fpa[e >> 1];
  const float fEc = (e & 1) ? fpa.y : fpa.x, fk2 = (e & 1) ? fpa.w : fpa.z;  // Ec, 2 log2e k
  const bool ejob = tid >= EJ && tid < EJ + NE;
  const int q = ejob ? tid - EJ : 0, eo = q / IN, ei = q % IN;
  const int lq0 = tid - EJ - NE;
  const bool ljob0 = lq0 >= 0 && lq0 < NL;
  const bool ljob1 = NL > J1 && tid < NL - J1;
  const int l0 = ljob0 ? lq0 : 0, l1 = ljob1 ? J1 + tid : 0;
  float A = 0.f, C = 0.f, Ev = 0.f, G = 0.f, base = 0.f, spl[NS];
#pragma unroll
  for (int c = 0; c < NS; ++c) spl[c] = 0.f;
  float lw0[OUT], lw1[OUT], la0 = 0.f, lb0 = 0.f, la1 = 0.f, lb1 = 0.f;
#pragma unroll
  for (int o = 0; o < OUT; ++o) lw0[o] = lw1[o] = 0.f;
  auto logistic = [&](int ql, int s, float* lw, float& la, float& lb) __attribute__((always_inline)) {
    const int i = ql / NB, j = ql % NB;
    const float sg = ssg[s][ql], ds = sg * (1.0f - sg), x = sx[s][i];
    float S = 0.f;
#pragma unroll
    for (int o = 0; o < OUT; ++o) {
      const float go = sgo[s][o];
      S = ffma(go, Tb.kw[o * (IN * L::NFL) + i * L::NFL + 1 + j], S);
      lw[o] = ffma(go, sg, lw[o]);
    }
    const float T = S * ds;
    la = ffma(T, x - Tb.pb[ql], la);
    lb = ffma(-T, Tb.pa[ql], lb);
  };

  // the tile's raw inputs (x, prev, output adjoints) are fetched one tile ahead, into registers,
  // while the current tile's jobs run
  constexpr int KI = (TS * IN + 255) / 256, KO = (TS * OUT + 255) / 256;
  float px[KI], pp[KI], pg[KO];
  auto fetch = [&](int64_t tt) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < KI; ++k) {
      const int it = tid + 256 * k, s = it / IN, i = it % IN;
      const int64_t n = tt + s;
      px[k] = pp[k] = 0.f;
      if (it < TS * IN && n < n1) {
        const int64_t ev = n / a.B;
        px[k] = a.tape[n * W + TB + i];
        if (!FE) continue;  // no hysteresis input without the Ferro jobs
        if (ev > 0) pp[k] = a.tape[(n - a.B) * W + TB + i];
        else if (!imask) pp[k] = a.state0[(LAYER == 0 ? (n % a.B) * D : a.B * D + (n % a.B) * H) + i];
        else pp[k] = px[k];  // the tape_at(-1) rule: first call, dx = 0
      }
    }
#pragma unroll
    for (int k = 0; k < KO; ++k) {
      const int it = tid + 256 * k, s = it / OUT, o = it % OUT;
      pg[k] = (it < TS * OUT && tt + s < n1) ? a.gadj[(tt + s) * W + GB + o] : 0.f;
    }
  };
  fetch(n0);
  for (int64_t t0 = n0; t0 < n1; t0 += TS) {
    // ---- per-tile features (one thread per (sample, input)) ----
#pragma unroll
    for (int k = 0; k < KI; ++k) {
      const int it = tid + 256 * k;
      if (it >= TS * IN) break;
      const int s = it / IN, i = it % IN, t = TB + i;
      const float x = px[k], pv = pp[k];
      // SiLU, interval, dense bases and gate: feat_input's arithmetic
      const float sx_ = sigm_l2(-x * FETODE_LOG2E);
      ssl[s][i] = x * sx_;
      int m = -1;
#pragma unroll
      for (int jj = 0; jj < NG; ++jj) m += (x >= TI.knots[t * NG + jj]) ? 1 : 0;
      const bool fin = __builtin_isfinite(x);
      const bool in = fin && m >= 0 && m < NI;
      const int mc = in ? m : 0;
      const float u = in ? (x - TI.knots[t * NG + mc]) * TI.rh[t * NI + mc] : (fin ? 0.f : __builtin_nanf(""));
      const float fill = fin ? 0.f : __builtin_nanf("");
      float bd[NS];
#pragma unroll
      for (int c = 0; c < NS; ++c) bd[c] = fill;
      if (in) {
#pragma unroll
        for (int r = 0; r <= kSO; ++r) {
          const int c = mc - kSO + r;
          const float4 p = TI.bp[TI.bpi(t, mc) + r];
          const float v = ffma(ffma(ffma(p.w, u, p.z), u, p.y), u, p.x);
#pragma unroll
          for (int cc = 0; cc < NS; ++cc) bd[cc] = cc == c ? v : bd[cc];
        }
      }
#pragma unroll
      for (int c = 0; c < NS; ++c) sbd[s][i][c] = bd[c];
      sx[s][i] = x;
      if (FE) sup[s][i] = sigm_l2(-gsl * (x - pv));
    }
#pragma unroll
    for (int k = 0; k < KO; ++k) {  // the layer's output adjoints
      const int it = tid + 256 * k;
      if (it < TS * OUT) sgo[it / OUT][it % OUT] = pg[k];
    }
    __syncthreads();  // sx of the tile (the logistic sigmoids read it)
    for (int it = tid; it < TS * IN * NB; it += 256) {
      const int s = it / (IN * NB), ql = it % (IN * NB), i = ql / NB;
      const int qq = (TB * NB) + ql;  // combined (t, j) index of the lg table
      ssg[s][ql] = sigm_l2(ffma(TI.lg[2 * qq], sx[s][i] , TI.lg[2 * qq + 1]));
    }
    __syncthreads();
    if (t0 + TS < n1) fetch(t0 + TS);
    // ---- jobs: each thread walks the tile's samples (all TS: samples past the block's range
    // have x = prev = 0 and zero adjoints, so they add exact zeros; unrolled for ILP) ----
    if (fjob) {
#pragma unroll 4
      for (int s = 0; s < TS; ++s) {  // layer_jobs' Ferro element VJP, sums only
        const float x = sx[s][fi], up = sup[s][fi], go = sgo[s][fo];
        const float Ec = fEc;
        const float cn = sigm_l2(gsl * (x + Ec));
        const float omu = 1.0f - up;
        const float mm = ffma(wc, omu * cn, 1.0f);
        const float sh = ffma(Ec, mm, x);
        const float th = ffma(-2.0f, sigm_l2(fk2 * sh), 1.0f);
        const float qv = go * ffma(-th, th, 1.0f);
        A = ffma(go, th, A);
        C = ffma(qv, sh, C);
        const float dcn = gs * cn * (1.0f - cn);
        const float dmdEc = -wc * omu * dcn;
        Ev = ffma(qv, ffma(Ec, dmdEc, mm), Ev);
      }
    }
    if (ejob) {
#pragma unroll 4
      for (int s = 0; s < TS; ++s) {
        const float go = sgo[s][eo];
        base = ffma(go, ssl[s][ei], base);
#pragma unroll
        for (int c = 0; c < NS; ++c) spl[c] = ffma(go, sbd[s][ei][c], spl[c]);
        G += go;  // read only on the i = 0 edge of each output
      }
    }
    if (ljob0) {
#pragma unroll 4
      for (int s = 0; s < TS; ++s) logistic(l0, s, lw0, la0, lb0);
    }
    if (ljob1) {
#pragma unroll 4
      for (int s = 0; s < TS; ++s) logistic(l1, s, lw1, la1, lb1);
    }
    __syncthreads();
  }
  // ---- this block's partial row (the layer's half; the other launch writes the other half) ----
  float* part = a.part + (int64_t)blockIdx.x * a.nacc + (LAYER == 0 ? 0 : LA::AL.n);
  if (!FE) {
    for (int i = tid; i < 3 * E; i += 256) part[AL.oA + i] = 0.f;  // (oA, oC, oE: contiguous)
  }
  if (fjob) {
    part[AL.oA + e] = A;
    part[AL.oC + e] = C;
    part[AL.oE + e] = Ev;
  }
  if (ejob) {
    if (ei == 0) part[AL.oG + eo] = G;
    part[AL.oBase + q] = base;
#pragma unroll
    for (int c = 0; c < NS; ++c) part[AL.oSpl + q * NS + c] = spl[c];
  }
  if (ljob0) {
#pragma unroll
    for (int o = 0; o < OUT; ++o) part[AL.oLw + o * NL + l0] = lw0[o];
    part[AL.oLa + l0] = la0;
    part[AL.oLb + l0] = lb0;
  }
  if (ljob1) {
#pragma unroll
    for (int o = 0; o < OUT; ++o) part[AL.oLw + o * NL + l1] = lw1[o];
    part[AL.oLa + l1] = la1;
    part[AL.oLb + l1] = lb1;
  }
}

// partial rows -> chunk sums (fp64), fixed order
__global__ void part_reduce_kernel(const float* __restrict__ part, int64_t nrows, int nacc, int64_t per,
                                   double* __restrict__ out) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nacc) return;
  const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < nrows ? r0 + per : nrows;
  double s = 0.0;
#pragma unroll 8
  for (int64_t r = r0; r < r1; ++r) s += part[r * nacc + slot];
  out[(int64_t)blockIdx.y * nacc + slot] = s;
}

// chunk sums -> S: four waves per 64 columns each sum a quarter of the chunks (loads issued
// together), then the four partials are added in a fixed order
constexpr int kChunkWaves = 4;
__global__ __launch_bounds__(64 * kChunkWaves) void chunk_sum_kernel(const double* __restrict__ ch, int nch, int nacc,
                                                                     double* __restrict__ S) {
  __shared__ double ps[kChunkWaves][64];
  const int w = threadIdx.x / 64, lane = threadIdx.x % 64, slot = blockIdx.x * 64 + lane;
  const int per = (nch + kChunkWaves - 1) / kChunkWaves, c0 = w * per, c1 = c0 + per < nch ? c0 + per : nch;
  double s = 0.0;
  if (slot < nacc) {
#pragma unroll 8
    for (int c = c0; c < c1; ++c) s += ch[(int64_t)c * nacc + slot];
  }
  ps[w][lane] = s;
  __syncthreads();
  if (w == 0 && slot < nacc) {
    double t = ps[0][lane];
#pragma unroll
    for (int k = 1; k < kChunkWaves; ++k) t += ps[k][lane];
    S[slot] = t;
  }
}

struct ApplyLayer {
  fetode_kanlinear_t kl;
  fetode_ferro_t fl;
  int has_ferro;
  AccLayout AL;
  fetode_kanlinear_grad_t kg;
  fetode_ferro_grad_t fg;
};

__device__ __forceinline__ void put(float* p, int64_t i, double v) {
  if (p) p[i] = (float)v;
}

// work items of one layer in grad_apply_kernel: elements / edges / logistic weights / logistic
// (a, b) pairs, padded to whole waves, then one wave per output for the logistic scalers
__host__ __device__ inline int apply_items(const ApplyLayer& L) {
  const AccLayout& A = L.AL;
  const int out = L.kl.out_features;
  const int n = (A.E + A.NE + out * A.NL + A.NL + 63) / 64 * 64;
  return n + (A.NL && L.kl.logistic_scaler ? 64 * out : 0);
}

// gradient sums of both layers -> parameter gradients (reference parameter layouts); 64-thread
// blocks never straddle a layer (apply_items pads), so the layer choice is wave-uniform
__global__ __launch_bounds__(64) void grad_apply_kernel(const double* __restrict__ S_, ApplyLayer L0_, ApplyLayer L1_,
                                                        int n0) {
  int t = blockIdx.x * 64 + threadIdx.x;
  const bool second = t >= n0;
  const ApplyLayer& L = second ? L1_ : L0_;
  const double* S = S_ + (second ? L0_.AL.n : 0);
  if (second) t -= n0;
  const AccLayout& A = L.AL;
  const int out = L.kl.out_features, NS = A.NS;
  const int nitems = (A.E + A.NE + out * A.NL + A.NL + 63) / 64 * 64;
  if (t >= nitems) {  // logistic scaler of output o: one wave, lanes over the NL weights, fixed-order tree
    const int o = (t - nitems) / 64, lane = (t - nitems) % 64;
    const double sl = L.kl.scale_logistic;
    double g = 0.0;
    for (int q = lane; q < A.NL; q += 64)
      g += 2.0 * S[A.oLw + o * A.NL + q] * (double)L.kl.logistic_weight[(int64_t)o * A.NL + q] * sl;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) g += __shfl_xor(g, m);
    if (lane == 0) put(L.kg.logistic_scaler, o, g);
    return;
  }
  if (t < A.E) {  // Ferro element e = (i, o, k)
    const int K = L.fl.num_basis, o = (t / K) % out;
    const double co = L.fl.coef[t], Ps = L.fl.Ps[t], kk = L.fl.k[t], bi = L.fl.bias[t];
    const double sA = S[A.oA + t], sC = S[A.oC + t], sE = S[A.oE + t], sG = S[A.oG + o];
    put(L.fg.k, t, co * Ps * sC);
    put(L.fg.Ec, t, co * Ps * kk * sE);
    put(L.fg.Ps, t, co * sA);
    put(L.fg.bias, t, co * sG);
    put(L.fg.coef, t, Ps * sA + bi * sG);
    return;
  }
  t -= A.E;
  if (t < A.NE) {  // KAN edge (o, i)
    put(L.kg.base_weight, t, S[A.oBase + t]);
    const double ss = L.kl.spline_scaler ? (double)L.kl.spline_scaler[t] : 1.0;
    double gsc = 0.0;
    for (int c = 0; c < NS; ++c) {
      const double d = S[A.oSpl + t * NS + c];
      put(L.kg.spline_weight, (int64_t)t * NS + c, d * ss);
      gsc += d * (double)L.kl.spline_weight[(int64_t)t * NS + c];
    }
    if (L.kl.spline_scaler) put(L.kg.spline_scaler, t, gsc);
    return;
  }
  t -= A.NE;
  if (A.NL == 0) return;
  if (t < out * A.NL) {  // logistic weight (o, i*NB + j); the basis is 2 sigmoid
    const int o = t / A.NL;
    const double ls = L.kl.logistic_scaler ? (double)L.kl.logistic_scaler[o] : 1.0;
    put(L.kg.logistic_weight, t, 2.0 * S[A.oLw + t] * L.kl.scale_logistic * ls);
    return;
  }
  t -= out * A.NL;
  if (t < A.NL) {
    put(L.kg.logistic_a, t, S[A.oLa + t]);
    put(L.kg.logistic_b, t, S[A.oLb + t]);
  }
}

#include "fetode_sweep7.h"
#include "fetode_kansum.h"

typedef void (*bwd_fn)(BwdArgs);
typedef void (*dopri_bwd_fn)(DopriBwdArgs);
struct BwdEntry {
  int D, H, K, NB, NG;
  bool ferro;
  int tpw;                     // trajectories per wave of fn (and of dopri)
  bwd_fn fn;                   // the one-kernel sweep (sums in VGPRs)
  bwd_fn adj, sum0, sum1;      // the split: adjoint sweep + per-layer parameter sums (or null)
  dopri_bwd_fn dopri;          // the reverse sweep of the resident dopri5 solve
  int dtpw;                    // its trajectories per wave (the whole batch is resident)
  dopri_bwd_fn dopri1;         // the same, one trajectory per wave: half the VJP jobs per lane
                               // (latency) where the batch leaves the grid room (small B)
  bwd_fn fn1;                  // fn at one trajectory per wave (small B), or null
  bwd_fn v7, v7s;              // the lane-group sweep (two trajectories per wave): Ferro sums + the
                               // recorded adjoints (then ks), or every sum in the sweep; or null
  bwd_fn ks;                   // the KAN sums over all samples after v7 (kansum_kernel)
};
// One table row: every kernel of a [D, H, D] shape, each a function of <D, H, K, NB, NG, FERRO> alone.  KK
// is the kernels' element count, TPW the trajectories per wave of the one-kernel sweep; a new kernel
// variant is one member above and one assignment here.
template <int D, int H, int K, int KK, int NB, int NG, bool FERRO, int TPW>
BwdEntry bwd_entry() {
  BwdEntry e{};
  e.D = D, e.H = H, e.K = K, e.NB = NB, e.NG = NG;
  e.ferro = FERRO;
  e.tpw = TPW;
  e.fn = fixed_bwd_kernel<D, H, KK, NB, NG, FERRO, true, TPW>;
  e.dopri = dopri_bwd_kernel<D, H, KK, NB, NG, FERRO, 2>;
  e.dtpw = 2;
  e.dopri1 = dopri_bwd_kernel<D, H, KK, NB, NG, FERRO, 1>;
  if constexpr (TPW > 1) e.fn1 = fixed_bwd_kernel<D, H, KK, NB, NG, FERRO, true, 1>;
  if constexpr (FERRO) {   // the KAN-FET sweep's alternatives
#ifdef FETODE_DIAG   // the split structure (measured slower) lives in the diagnostic build only
    e.adj = fixed_bwd_kernel<D, H, KK, NB, NG, FERRO, false, 1>;
    e.sum0 = param_sum_kernel<D, H, KK, NB, NG, 0>;
    e.sum1 = param_sum_kernel<D, H, KK, NB, NG, 1>;
#endif
    e.v7 = sweep7_kernel<false>;
    e.v7s = sweep7_kernel<true>;
    e.ks = kansum_kernel;
  }
  return e;
}
const BwdEntry kBwd[] = {
    // LV KAN-FET [2,10,2]: one kernel, two trajectories per wave (measured: TPW 1 / 2 / 4 = 1034 / 897 /
    // 1203 us at B = 4096); the split structure as the alternative
    bwd_entry<2, 10, 10, 10, 10, 12, true, 2>(),
    // LV KAN [2,10,2] (126 VGPRs: four waves per SIMD already): the entry's K is 0, the kernels are
    // instantiated at K = 1 (unused without Ferro: their K is 0)
    bwd_entry<2, 10, 0, 1, 10, 12, false, 1>(),
};
// Which path the KAN-FET sweep takes (fetode_backward_set_split; env FETODE_BWD_SPLIT).  Default:
// the one-kernel sweep — measured on MI355X at B = 4096, rk4, 34 steps: one kernel 1.06 ms vs the
// split 0.69 (adjoint sweep) + 0.25 + 0.31 (layer sums) ms (profiles/r02_split_pmc.txt).
int g_bwd_split = -1;
bool use_split(const BwdEntry* e) {
  if (g_bwd_split < 0) g_bwd_split = env_int("FETODE_BWD_SPLIT", 0) != 0;
  return e->adj && g_bwd_split != 0;
}
constexpr int64_t kSumBlocks = 1024;  // param_sum_kernel blocks per layer (= partial rows)
// The lane-group sweep (sweep7_kernel; fetode_backward_set_v7, env FETODE_BWD_V7):
// 0 = off, 1 = where the one-kernel sweep would run two trajectories per wave (the default),
// 2 = at every batch; + 4: the sweep keeps the Ferro sums only and records each evaluation's
// adjoints, kansum_kernel forms the KAN sums over all samples afterwards (measured at B = 4096:
// 386 + 109 us vs 496 us with every sum in the sweep — kansum recomputes the features; kept as
// the alternative).
int g_bwd_v7 = -1;
int g_bwd_tpw = 0;  // fetode_backward_set_tpw
int v7_mode() {
  if (g_bwd_v7 < 0) g_bwd_v7 = (int)env_int("FETODE_BWD_V7", 1);
  return g_bwd_v7;
}
int64_t n_evals_of(int32_t method, int32_t n_steps) {
  return (int64_t)n_steps * (method == FETODE_RK4 || method == FETODE_RK4_CLASSIC ? 4 : method == FETODE_MIDPOINT ? 2 : 1);
}

const BwdEntry* find_bwd(const fetode_field_t* f) {
  if (f->n_layers != 2) return nullptr;
  const fetode_kanlinear_t &k0 = f->kan[0], &k1 = f->kan[1];
  if (k0.spline_order != kSO || k1.spline_order != kSO || k0.grid_size != k1.grid_size ||
      k0.num_logistic != k1.num_logistic || k0.in_features != k1.out_features)
    return nullptr;
  const int NG = k0.grid_size + 2 * kSO + 1;
  for (const BwdEntry& e : kBwd) {
    if (e.D != k0.in_features || e.H != k0.out_features || e.NB != k0.num_logistic || e.NG != NG) continue;
    if (e.ferro != (f->ferro != nullptr)) continue;
    if (f->ferro) {
      if (f->ferro[0].num_basis != e.K || f->ferro[1].num_basis != e.K) continue;
      if (f->ferro[0].branch_sign || f->ferro[1].branch_sign) continue;
    }
    return &e;
  }
  return nullptr;
}

constexpr int64_t kMaxBwdRows = 8192;  // partial rows (one per wave)
constexpr int kChunks = 64;
// one partial row per wave: the grid's waves, a multiple of kTPB
int64_t bwd_rows(int64_t B, int tpw) {
  const int64_t nw = (B + tpw - 1) / tpw;  // waves the trajectories need
  const int64_t w = nw < kMaxBwdRows ? nw : kMaxBwdRows;
  return (w + kTPB - 1) / kTPB * kTPB;
}

void layouts(const fetode_field_t* f, AccLayout* L0, AccLayout* L1) {
  const int NS = f->kan[0].grid_size + kSO;
  const int K = f->ferro ? f->ferro[0].num_basis : 0;
  const bool fe = f->ferro != nullptr;
  *L0 = acc_layout(f->kan[0].in_features, f->kan[0].out_features, K, f->kan[0].num_logistic, NS, fe);
  *L1 = acc_layout(f->kan[1].in_features, f->kan[1].out_features, K, f->kan[1].num_logistic, NS, fe);
}


// gradient sums S -> parameter gradients in the reference layouts (grad_apply_kernel)
int apply_grads(const fetode_field_t* f, const double* S, const AccLayout& AL0, const AccLayout& AL1,
                const fetode_kanlinear_grad_t* kan_grads, const fetode_ferro_grad_t* ferro_grads, hipStream_t s) {
  if (!kan_grads && !ferro_grads) return FETODE_OK;
  ApplyLayer L[2];
  for (int l = 0; l < 2; ++l) {
    memset(&L[l], 0, sizeof(ApplyLayer));
    L[l].kl = f->kan[l];
    if (f->ferro) L[l].fl = f->ferro[l];
    L[l].has_ferro = f->ferro != nullptr;
    L[l].AL = l == 0 ? AL0 : AL1;
    if (kan_grads) L[l].kg = kan_grads[l];
    if (ferro_grads && f->ferro) L[l].fg = ferro_grads[l];
  }
  const int n0 = apply_items(L[0]), n1 = apply_items(L[1]);
  hipLaunchKernelGGL(grad_apply_kernel, dim3((unsigned)((n0 + n1) / 64)), dim3(64), 0, s, S, L[0], L[1], n0);
  LAUNCH_CHECK();
  return FETODE_OK;
}

}  // namespace

extern "C" {

int fetode_backward_set_split(int32_t enable) {
#ifndef FETODE_DIAG
  if (enable > 0) {   // the split sweep is compiled into the diagnostic build only
    set_err(FETODE_EUNSUPPORTED, "the split backward is a diagnostic path (make diag)");
    return -2;
  }
  return 0;
#else
  use_split(&kBwd[0]);  // resolve the env default first
  const int prev = g_bwd_split;
  if (enable >= 0) g_bwd_split = enable != 0;
  return prev;
#endif
}

int fetode_backward_set_v7(int32_t mode) {
  const int prev = v7_mode();
  if (mode >= 0) g_bwd_v7 = mode;
  return prev;
}

int fetode_backward_set_tpw(int32_t tpw) {
  const int prev = g_bwd_tpw;
  if (tpw >= 0 && tpw <= 2) g_bwd_tpw = tpw;
  return prev;
}

int fetode_fused_backward_supported(const fetode_field_t* f) {
  if (validate_field(f) != FETODE_OK) return 0;
  return find_bwd(f) != nullptr || fieldn_shape_supported(f);
}

// the one-kernel sweep at one trajectory per wave while those waves fit one resident round
// (latency-bound small batches: half the VJP jobs per lane), else e->tpw.
// fetode_backward_set_tpw: 0 automatic, 1 / 2 force that shape where the entry has it
int fixed_tpw(const BwdEntry* e, int64_t B) {
  if (!e->fn1) return e->tpw;
  if (g_bwd_tpw == 1) return 1;
  if (g_bwd_tpw == 2) return e->tpw;
  static const bool on = env_int("FETODE_BWD_TPW1", 1) != 0;  // A/B knob
  const int64_t cap = on ? std::max<int64_t>(resident_wgs(e->fn1, 64 * kTPB), 0) * kTPB : 0;  // resident waves
  // measured (tools/diag/bwd_small_time.py, rk4 iteration): B = 512 0.73 vs 0.93 ms, B = 2048 0.79 vs
  // 0.75 ms — one trajectory per wave while at most half the resident waves are needed
  return 2 * B <= cap ? 1 : e->tpw;
}

bool use_v7(const BwdEntry* e, int64_t B) {
  if (!e->v7 || use_split(e)) return false;
  const int m = v7_mode() & 3;
  return m >= 2 || (m == 1 && fixed_tpw(e, B) == 2);
}
bool v7_offload(const BwdEntry* e, int64_t B) { return use_v7(e, B) && (v7_mode() & 4); }
// partial rows of the chosen path: one per wave (the one-kernel and lane-group sweeps) or per
// param_sum block (split)
int64_t sum_rows(const BwdEntry* e, int64_t B, int64_t n_ev) {
  if (use_v7(e, B)) return bwd_rows(B, 2) + (v7_offload(e, B) ? s7::kKsRows : 0);
  if (!use_split(e)) return bwd_rows(B, fixed_tpw(e, B));
  const int64_t tiles = (n_ev * B + kPsTS - 1) / kPsTS;
  return tiles < kSumBlocks ? (tiles > 0 ? tiles : 1) : kSumBlocks;
}

int64_t fetode_integrate_fixed_backward_workspace(const fetode_field_t* f, int32_t method, int32_t n_steps, int64_t B) {
  if (validate_field(f) != FETODE_OK || B <= 0 || n_steps < 0) return -1;
  if (!find_bwd(f)) return fieldn_shape_supported(f) ? fieldn_fixed_backward_workspace(f, method, n_steps, B) : -1;
  const BwdEntry* e = find_bwd(f);
  AccLayout L0, L1;
  layouts(f, &L0, &L1);
  const int64_t nacc = L0.n + L1.n;
  const int64_t n_ev = n_evals_of(method, n_steps);
  const int64_t nrow = sum_rows(e, B, n_ev);
  const int64_t nch = nrow < kChunks ? nrow : kChunks;
  const int64_t adj = use_split(e) || v7_offload(e, B) ? n_ev * B * (f->kan[0].in_features + f->kan[0].out_features) : 0;
  return (int64_t)sizeof(double) * nacc * (nch + 1) + (int64_t)sizeof(float) * (nrow * nacc + adj);
}

int fetode_integrate_fixed_backward(const fetode_field_t* f, const void* plan, int32_t method, int64_t B,
                                    const float* step_coef, int32_t n_steps, const int32_t* out_step,
                                    const int32_t* out_mode, const float* out_slope, int32_t T,
                                    const float* grad_solution, const float* tape, const float* state0,
                                    uint32_t init_mask, float* grad_y0, const fetode_kanlinear_grad_t* kan_grads,
                                    const fetode_ferro_grad_t* ferro_grads, void* workspace, void* stream) {
  int rc = validate_field(f);
  if (rc) return rc;
  const BwdEntry* e = find_bwd(f);
  const bool fieldn = !e && fieldn_shape_supported(f);  // other widths: fetode_fieldn_bwd.hip
  if (!e && !fieldn) return set_err(FETODE_EUNSUPPORTED, "no fused backward kernel for this field shape");
  if (method < FETODE_EULER || method > FETODE_RK4_CLASSIC) return set_err(FETODE_EINVAL, "unknown method %d", method);
  if (B <= 0 || T <= 0) return FETODE_OK;
  if (!plan || !grad_solution || !workspace || (n_steps > 0 && (!tape || !step_coef || !out_step || !out_mode ||
                                                                 !out_slope)) ||
      (f->ferro && !state0 && (init_mask & 3u) != 3u))
    return set_err(FETODE_EINVAL, "null pointer");
  if (fieldn)
    return fieldn_fixed_backward(f, plan, method, B, step_coef, n_steps, out_step, out_mode, out_slope, T,
                                 grad_solution, tape, state0, init_mask, grad_y0, kan_grads, ferro_grads, workspace,
                                 stream);
  hipStream_t s = (hipStream_t)stream;
  AccLayout AL0, AL1;
  layouts(f, &AL0, &AL1);
  const int nacc = AL0.n + AL1.n;
  const bool split = use_split(e);
  const int64_t n_ev = n_evals_of(method, n_steps);
  const int64_t nrow = sum_rows(e, B, n_ev);
  const int64_t nch = nrow < kChunks ? nrow : kChunks;
  double* S = (double*)workspace;
  double* chunks = S + nacc;
  float* part = (float*)(chunks + nch * nacc);
  float* gadj = part + nrow * nacc;  // (n_ev, B, D + H): the split and lane-group (+ kansum) paths

  BwdArgs a;
  memset(&a, 0, sizeof(a));
  a.plan = (const float*)plan;
  field_plans(f, &a.P0, &a.P1);
  a.k0 = f->kan[0];
  a.k1 = f->kan[1];
  if (f->ferro) {
    a.f0 = f->ferro[0];
    a.f1 = f->ferro[1];
  }
  a.method = method;
  a.B = B;
  a.step_coef = step_coef;
  a.n_steps = n_steps;
  a.out_step = out_step;
  a.out_mode = out_mode;
  a.out_slope = out_slope;
  a.T = T;
  a.gsol = grad_solution;
  a.tape = tape;
  a.state0 = state0;
  a.init_mask = f->ferro ? init_mask : 3u;
  a.gy0 = grad_y0;
  a.part = part;
  a.nacc = nacc;
  a.gadj = gadj;
  if (use_v7(e, B)) {   // two trajectories per wave, one partial row per wave
    const bool off = v7_offload(e, B);
    const int64_t nw = bwd_rows(B, 2);
    hipLaunchKernelGGL(off ? e->v7 : e->v7s, dim3((unsigned)(nw / kTPB)), dim3(64 * kTPB), 0, s, a);
    LAUNCH_CHECK();
    if (off) {   // the KAN sums: kKsRows more partial rows (both layers' halves)
      BwdArgs a2 = a;
      a2.part = part + nw * nacc;
      hipLaunchKernelGGL(e->ks, dim3((unsigned)s7::kKsRows, 2), dim3(64 * s7::kKsWaves), 0, s, a2);
      LAUNCH_CHECK();
    }
  } else if (split) {
    // adjoint sweep: one wave per trajectory, every trajectory resident (grid-stride beyond)
    const int64_t blocks = (B + kTPB - 1) / kTPB;
    hipLaunchKernelGGL(e->adj, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(64 * kTPB), 0, s, a);
    LAUNCH_CHECK();
    if (n_ev > 0) {
      hipLaunchKernelGGL(e->sum0, dim3((unsigned)nrow), dim3(256), 0, s, a);
      LAUNCH_CHECK();
      hipLaunchKernelGGL(e->sum1, dim3((unsigned)nrow), dim3(256), 0, s, a);
      LAUNCH_CHECK();
    } else {
      HIP_CHECK_RET(hipMemsetAsync(part, 0, sizeof(float) * nrow * nacc, s));
    }
  } else {
    // (an entry whose own sweep is one trajectory per wave has no fn1)
    hipLaunchKernelGGL((e->fn1 && fixed_tpw(e, B) == 1) ? e->fn1 : e->fn, dim3((unsigned)(nrow / kTPB)), dim3(64 * kTPB),
                       0, s, a);
    LAUNCH_CHECK();
  }
  const int64_t per = (nrow + nch - 1) / nch;
  hipLaunchKernelGGL(part_reduce_kernel, dim3(nblk(nacc, 64), (unsigned)nch), dim3(64), 0, s, part, nrow, nacc, per,
                     chunks);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(chunk_sum_kernel, dim3(nblk(nacc, 64)), dim3(64 * kChunkWaves), 0, s, chunks, (int)nch, nacc, S);
  LAUNCH_CHECK();
  return apply_grads(f, S, AL0, AL1, kan_grads, ferro_grads, s);
}

// ---- reverse sweep of the resident dopri5 solve ----
// every workgroup resident at once (one grid sum per attempt): the occupancy of the kernel
static int64_t dopri_bwd_resident_wgs(const BwdEntry* e, bool one = false) {
  return resident_wgs(one ? e->dopri1 : e->dopri, 64 * kTPB);
}
// fetode_integrate_dopri5_backward_set_shape: 0 automatic, 1 / 2 trajectories per wave
static int g_dopri_bwd_shape = 0;
// one trajectory per wave when that grid is resident (small batches), else e->dtpw
static int dopri_bwd_tpw(const BwdEntry* e, int64_t B) {
  if (g_dopri_bwd_shape == 1 && e->dopri1) return 1;
  if (g_dopri_bwd_shape == 2) return e->dtpw;
  // (as fixed_tpw: while the one-per-wave grid fills at most half of its resident capacity)
  if (e->dopri1 && 2 * ((B + kTPB - 1) / kTPB) <= dopri_bwd_resident_wgs(e, true)) return 1;
  return e->dtpw;
}
static int64_t dopri_bwd_grid(const BwdEntry* e, int64_t B) {
  const int tpw = dopri_bwd_tpw(e, B);
  return (B + kTPB * tpw - 1) / (kTPB * tpw);
}

// multi-pass (fetode_dopri5_set_multipass): the virtual grid is the full-grid shape's, two
// trajectories per wave; taken when that grid exceeds the test limit, or the one-grid launch of the
// batch its co-resident capacity
static int64_t dopri_bwd_mp_vgrid(int64_t B) { return (B + kTPB * 2 - 1) / (kTPB * 2); }
static bool dopri_bwd_mp_forced(int64_t B) {
  const int64_t limit = dp_grid_limit();
  return dp_multipass() && B <= kDpMultipassMaxBatch && limit > 0 && dopri_bwd_mp_vgrid(B) > limit;
}
static bool dopri_bwd_use_mp(const BwdEntry* e, int64_t B) {
  if (!dp_multipass() || B > kDpMultipassMaxBatch) return false;
  if (dopri_bwd_mp_forced(B)) return true;
  const bool one = dopri_bwd_tpw(e, B) == 1;
  const int64_t resident = dopri_bwd_resident_wgs(e, one);
  return resident >= 0 && dopri_bwd_grid(e, B) > resident;
}
// bytes of the one-grid workspace layout for a sweep grid of `grid` workgroups
static int64_t dopri_bwd_ws_bytes(int64_t nacc, int64_t grid) {
  const int64_t nrow = grid * kTPB, nch = nrow < kChunks ? nrow : kChunks;
  const int64_t n = (int64_t)sizeof(unsigned) * kDpBarWords + (int64_t)sizeof(double) * (2 * grid + 4 * kDpGroups) +
                    (int64_t)sizeof(double) * nacc * (nch + 1) + (int64_t)sizeof(float) * nrow * nacc;
  return (n + 7) & ~(int64_t)7;
}

int fetode_integrate_dopri5_backward_set_shape(int tpw) {
  const int prev = g_dopri_bwd_shape;
  if (tpw >= 0 && tpw <= 2) g_dopri_bwd_shape = tpw;
  return prev;
}

int64_t fetode_integrate_dopri5_backward_max_batch(const fetode_field_t* f) {
  if (validate_field(f) != FETODE_OK) return 0;
  const BwdEntry* e = find_bwd(f);
  if (!e && fieldn_shape_supported(f)) return fieldn_dopri5_backward_max_batch(f);
  if (!e || !e->dopri) return 0;
  const int64_t w = dopri_bwd_resident_wgs(e);
  return w > 0 ? w * kTPB * e->dtpw : 0;
}

int64_t fetode_integrate_dopri5_backward_workspace_ev(const fetode_field_t* f, int64_t B, int32_t n_ev) {
  if (validate_field(f) != FETODE_OK || B <= 0 || n_ev < 0) return -1;
  if (!find_bwd(f) && fieldn_shape_supported(f)) return fieldn_dopri5_backward_workspace(f, B, n_ev);
  return fetode_integrate_dopri5_backward_workspace(f, B);
}

int64_t fetode_integrate_dopri5_backward_workspace(const fetode_field_t* f, int64_t B) {
  if (validate_field(f) != FETODE_OK || B <= 0) return -1;
  const BwdEntry* e = find_bwd(f);
  if (!e || !e->dopri) return -1;
  AccLayout L0, L1;
  layouts(f, &L0, &L1);
  const int64_t nacc = L0.n + L1.n, grid = dopri_bwd_grid(e, B), nrow = grid * kTPB;
  const int64_t nch = nrow < kChunks ? nrow : kChunks;
  const int64_t one_grid = (int64_t)sizeof(unsigned) * kDpBarWords + (int64_t)sizeof(double) * (2 * grid + 4 * kDpGroups) +
                           (int64_t)sizeof(double) * nacc * (nch + 1) + (int64_t)sizeof(float) * nrow * nacc;
  if (!dp_multipass() || B > kDpMultipassMaxBatch) return one_grid;
  // multi-pass on: room for either launch — the virtual grid's layout, then the parking area
  const int64_t vgrid = dopri_bwd_mp_vgrid(B);
  const int64_t mp = dopri_bwd_ws_bytes(nacc, vgrid) + dopri_bwd_mp_park_bytes(f->ferro != nullptr, vgrid);
  return one_grid > mp ? one_grid : mp;
}

int fetode_integrate_dopri5_backward(const fetode_field_t* f, const void* plan, int64_t B, const double* t, int32_t T,
                                     double rtol, double atol, const double* opts, const float* tableau,
                                     const float* grad_solution, const float* tape, int32_t n_ev,
                                     const double* attempts, int32_t n_att, const double* init_rec,
                                     const float* state0, uint32_t init_mask, float* grad_y0,
                                     const fetode_kanlinear_grad_t* kan_grads, const fetode_ferro_grad_t* ferro_grads,
                                     void* workspace, int32_t* status, void* stream) {
  int rc = validate_field(f);
  if (rc) return rc;
  const BwdEntry* e = find_bwd(f);
  const bool fieldn = !e && fieldn_shape_supported(f);  // other widths: fetode_fieldn_bwd.hip
  if (!fieldn && (!e || !e->dopri)) return set_err(FETODE_EUNSUPPORTED, "no dopri5 backward kernel for this field shape");
  if (B <= 0 || T <= 0) return FETODE_OK;
  if (!plan || !t || !opts || !tableau || !grad_solution || !tape || !attempts || !init_rec || !workspace ||
      !status || (f->ferro && !state0 && (init_mask & 3u) != 3u))
    return set_err(FETODE_EINVAL, "dopri5 backward: null pointer");
  const int base = dopri_base(opts);
  if (n_att < 0 || n_ev != base + 6 * n_att)
    return set_err(FETODE_EINVAL, "dopri5 backward: %d evaluations do not match %d attempts", n_ev, n_att);
  if (fieldn)
    return fieldn_dopri5_backward(f, plan, B, t, T, rtol, atol, opts, tableau, grad_solution, tape, n_ev, attempts,
                                  n_att, init_rec, state0, init_mask, grad_y0, kan_grads, ferro_grads, workspace, status,
                                  stream);
  const bool mp = dopri_bwd_use_mp(e, B);
  const bool one = !mp && dopri_bwd_tpw(e, B) == 1;
  const int64_t resident = mp ? dopri_bwd_mp_resident_wgs(f->ferro != nullptr) : dopri_bwd_resident_wgs(e, one);
  if (resident <= 0) return set_err(FETODE_EHIP, "dopri5 backward: occupancy query failed");
  // multi-pass: `grid` is the virtual grid (the leaf layout, the slots, the rows of partial sums);
  // the launch takes pgrid <= the co-resident capacity (and the test limit) workgroups
  const int64_t grid = mp ? dopri_bwd_mp_vgrid(B) : dopri_bwd_grid(e, B);
  int64_t pgrid = grid;
  if (mp) {
    pgrid = grid < resident ? grid : resident;
    if (dp_grid_limit() > 0 && pgrid > dp_grid_limit()) pgrid = dp_grid_limit();
  } else if (grid > resident)
    return set_err(FETODE_EUNSUPPORTED, "dopri5 backward: batch %lld needs %lld workgroups, %lld resident",
                   (long long)B, (long long)grid, (long long)resident);
  hipStream_t s = (hipStream_t)stream;
  AccLayout AL0, AL1;
  layouts(f, &AL0, &AL1);
  const int nacc = AL0.n + AL1.n;
  const int64_t nrow = grid * kTPB, nch = nrow < kChunks ? nrow : kChunks;
  unsigned* bar = (unsigned*)workspace;
  double* slot = (double*)((char*)workspace + sizeof(unsigned) * kDpBarWords);
  double* xs = slot + 2 * grid;
  double* S = xs + 4 * kDpGroups;
  double* chunks = S + nacc;
  float* part = (float*)(chunks + nch * nacc);

  DopriBwdArgs d;
  memset(&d, 0, sizeof(d));
  BwdArgs& a = d.b;
  a.plan = (const float*)plan;
  field_plans(f, &a.P0, &a.P1);
  a.k0 = f->kan[0];
  a.k1 = f->kan[1];
  if (f->ferro) {
    a.f0 = f->ferro[0];
    a.f1 = f->ferro[1];
  }
  a.B = B;
  a.T = T;
  a.gsol = grad_solution;
  a.tape = tape;
  a.state0 = state0;
  a.init_mask = f->ferro ? init_mask : 3u;
  a.gy0 = grad_y0;
  a.part = part;
  a.nacc = nacc;
  d.att = attempts;
  d.n_att = n_att;
  d.n_ev = n_ev;
  d.base = base;
  d.t = t;
  d.init_rec = init_rec;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) d.beta[i][j] = tableau[i * 6 + j];
  for (int j = 0; j < 7; ++j) {
    d.cerr[j] = tableau[36 + j];
    d.cmid[j] = tableau[43 + j];
  }
  d.rtol = (float)rtol;
  d.atol = (float)atol;
  dopri_step_from_opts(opts, d.step);
  d.n_el = (double)B * f->kan[0].in_features;
  d.gp.bar = bar;
  d.gp.slot = slot;
  d.gp.xs = xs;
  dp_single_device(d.gp, grid);
  d.gp.mp = mp ? 1 : 0;
  d.gp.park = mp ? (float*)((char*)workspace + dopri_bwd_ws_bytes(nacc, grid)) : nullptr;
  d.status = status;
  HIP_CHECK_RET(hipMemsetAsync(workspace, 0, sizeof(unsigned) * kDpBarWords, s));
  void* args[] = {&d};
  if (mp)
    HIP_CHECK_RET(dopri_bwd_mp_launch(f->ferro != nullptr, &d, pgrid, s));
  else
    HIP_CHECK_RET(resident_launch((const void*)(one ? e->dopri1 : e->dopri), dim3((unsigned)grid), dim3(64 * kTPB), args,
                                  0, s));
  const int64_t per = (nrow + nch - 1) / nch;
  hipLaunchKernelGGL(part_reduce_kernel, dim3(nblk(nacc, 64), (unsigned)nch), dim3(64), 0, s, part, nrow, nacc, per,
                     chunks);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(chunk_sum_kernel, dim3(nblk(nacc, 64)), dim3(64 * kChunkWaves), 0, s, chunks, (int)nch, nacc, S);
  LAUNCH_CHECK();
  return apply_grads(f, S, AL0, AL1, kan_grads, ferro_grads, s);
}

}  // extern "C"
