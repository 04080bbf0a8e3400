// fetode_ecg_bwd.hip — loss.backward() through the device-resident dopri5 solve of the ECG field
// (train_ecg_kan_fet_nn_ode.py:551-572 then :575-617: odeint(self.odefunc, h0, [0, 1], "dopri5")
// followed by loss.backward()): reverse mode through every evaluation of every attempt (rejected
// ones included), the stage sums, the error norm, the step-size control, the initial-step
// selection and the dense output, like autograd through torchdiffeq (which detaches none of them).
//
// Tape (fetode_ecg_dopri5_tape): per evaluation e its input x_e and output k_e, (n_ev, 2, B, D);
// per attempt (t0, dt, error ratio, accepted); the initial-step scalars {d0, d1, d2, h0, h1}.
// Evaluation order: 0 = f(y0), 1 = the initial-step probe (absent with first_step), then six per
// attempt (stages 2..7; stage 7's input is the attempt's y1, its output the next f0).  The
// hysteresis memory of evaluation e is the last batch row of x_{e-1} (the module's prev_x for
// e = 0), so the gate of every element is recomputed from the tape with the forward's expression
// and takes the forward's branch bit for bit; no gradient flows through the gate or the memory
// (train_ecg_kan_fet_nn_ode.py:123, :131-132).
//
// ecg_dopri5_bwd_kernel: ONE resident launch.  A workgroup owns kBwdRows batch rows (a wave per
// row, lane d carries the adjoints of state element d) and walks the evaluations backwards.  Per
// evaluation the VJP needs d/dx only: g_phi = g_k W (thread q sums over the outputs for the four
// rows at once, W read coalesced from L2), sigma'(basis) d basis/dx on the forward's branch, and
// the sum over the bases of an input.  The adjoint of dt couples the batch (the error ratio is a
// norm over every element): one fixed-order fp64 grid sum per attempt, on the forward's bounded
// grid barrier.  The control chain (dt, ratio, t) is carried in fp64.  Every evaluation's output
// adjoint g_k[e] (B, D) goes to a gradient tape.
//
// The parameter gradients are sums over the stacked (evaluation, row) samples and need no order
// between samples: three ordinary launches after the sweep recompute phi from the tape and sum
// head_gw_kernel's / mixer_gparam_kernel's element formulas per workgroup over its tiles of
// samples, then over the workgroups, both in a fixed order (no atomics: run-to-run identical).
#include <algorithm>
#include <cstring>

#include "fetode_common.h"
#include "fetode_dopri_ctl.h"
#include "fetode_ecg_dev.h"

using namespace fetode;

namespace {

constexpr int kBwdThreads = 256;
constexpr int kBwdRows = 4;                      // batch rows per workgroup: one wave each
constexpr int kQPT = kMaxF / kBwdThreads;        // (input, basis) indices per thread: q = tid + 256 c
static_assert(kQPT * kBwdThreads == kMaxF, "every q < kMaxF has an owner");

struct EcgBwdArgs {
  HL L;
  const float* w;      // (D, F) head weight (proj.weight)
  int D, F, Fp;
  const float* prev0;  // (F) prev_x before the solve
  int64_t B;
  const double* t;     // (T) output times
  int T;
  float rtol, atol;
  DopriStep step;  // first_step unused: base says whether it was given
  double n_el;
  DopriTab tab;
  const float* gsol;   // (T, B, D) d loss / d solution
  const float* tape;   // (n_ev, 2, B, D)
  int n_ev, n_att, base;  // base: evaluation index of attempt 0's stage 2 (1 with first_step, else 2)
  const double* att;   // (n_att, 4): t0, dt, error ratio, accepted
  const double* init_rec;  // {d0, d1, d2, h0, h1}
  float* gy0;          // (B, D) nullable
  float* gtape;        // (n_ev, B, D): every evaluation's output adjoint
  double* part;        // (2, gridDim.x, 2) double-buffered partial sums
  unsigned* bar;       // kBarWords, zeroed
  int* status;         // 0, or 4 when a grid barrier timed out
};

__global__ __launch_bounds__(kBwdThreads) void ecg_dopri5_bwd_kernel(EcgBwdArgs a) {
  constexpr int NT = kBwdThreads, R = kBwdRows;
  // dynamic LDS: prm [F] float4 {k, Ec, Ps, bias} | cb (R, Fp): g_basis * d basis / dx per element
  extern __shared__ float4 s_dyn4[];
  __shared__ float xs[R][64];        // the evaluation's inputs
  __shared__ float pvs[64];          // its hysteresis memory per input (evaluations >= 1)
  __shared__ float4 gT[64];          // its output adjoint, [output] -> the four rows
  __shared__ float s_k[8][R][64], s_kb[8][R][64];  // k_1..k_7 of the attempt and their adjoints
  __shared__ double red[NT / 64][2];
  __shared__ double tot[2];
  const int tid = threadIdx.x, d = tid % 64, r = tid / 64;
  const int D = a.D, F = a.F, Fp = a.Fp, nb = a.L.nb;
  float4* prm = s_dyn4;
  float* cb = reinterpret_cast<float*>(prm + F);
  const int64_t b = (int64_t)blockIdx.x * R + r;
  const bool dval = d < D;
  const bool el = dval && b < a.B;  // this thread carries element (b, d)
  const int64_t BD = a.B * D;
  const int64_t bo = el ? b * D + d : 0;
  const int n_ev = a.n_ev, base = a.base;
  const float gs = a.L.gs, bp = a.L.bp;
  for (int q = tid; q < F; q += NT) prm[q] = make_float4(a.L.k[q], a.L.Ec[q], a.L.Ps[q], a.L.bias[q]);
  auto tx = [&](int e) -> float { return a.tape[(int64_t)e * 2 * BD + bo]; };        // input (el lanes)
  auto tk = [&](int e) -> float { return a.tape[((int64_t)e * 2 + 1) * BD + bo]; };  // output (el lanes)
  int phase = 0;
  bool aborted = false;

  // the VJP of evaluation ev for this thread's element: g = d loss / d k_ev -> d loss / d x_ev
  auto vjp = [&](int ev, float g) -> float {
    const float gg = el ? g : 0.f;
    xs[r][d] = el ? tx(ev) : 0.f;
    reinterpret_cast<float*>(gT)[d * R + r] = gg;
    if (tid < D && ev > 0) pvs[tid] = a.tape[(int64_t)(ev - 1) * 2 * BD + (a.B - 1) * D + tid];
    if (el) a.gtape[(int64_t)ev * BD + bo] = gg;
    __syncthreads();
    // g_phi[row, q] = sum_o g[row, o] W[o, q], o ascending (head_gin_kernel's order)
    float acc[kQPT][R];
    int qc[kQPT];
#pragma unroll
    for (int c = 0; c < kQPT; ++c) {
      qc[c] = min(tid + NT * c, F - 1);
#pragma unroll
      for (int r2 = 0; r2 < R; ++r2) acc[c][r2] = 0.f;
    }
#pragma unroll 4
    for (int o = 0; o < D; ++o) {
      const float4 gv = gT[o];
      const float* wr = a.w + (int64_t)o * F;
#pragma unroll
      for (int c = 0; c < kQPT; ++c) {
        const float wv = wr[qc[c]];
        acc[c][0] = __builtin_fmaf(gv.x, wv, acc[c][0]);
        acc[c][1] = __builtin_fmaf(gv.y, wv, acc[c][1]);
        acc[c][2] = __builtin_fmaf(gv.z, wv, acc[c][2]);
        acc[c][3] = __builtin_fmaf(gv.w, wv, acc[c][3]);
      }
    }
#pragma unroll
    for (int c = 0; c < kQPT; ++c) {
      const int q = tid + NT * c;
      if (q < F) {
        const int i = q / nb;
        const float4 pr = prm[q];
        const float pv = ev == 0 ? a.prev0[q] : pvs[i];
#pragma unroll
        for (int r2 = 0; r2 < R; ++r2) {
          const RPoint p = rpoint(pr, gs, bp, xs[r2][i], pv);
          const float gb = acc[c][r2] * (p.phi * (1.0f - p.phi));
          cb[r2 * Fp + q] = gb * p.dx;
        }
      }
    }
    __syncthreads();
    float xb = 0.f;
    if (dval) {
      const float* cr = cb + r * Fp + d * nb;
      for (int j = 0; j < nb; ++j) xb += cr[j];  // mixer_gx_kernel's order
    }
    // no trailing barrier: the next VJP writes xs / gT / pvs (read before the barrier above), then
    // waits before cb is rewritten
    return xb;
  };

  // grid-wide fixed-order sum of two per-thread fp64 values, the same in every workgroup
  // (ecg_dopri5_kernel's global_sum2)
  auto gsum = [&](double v0, double v1, double& s0, double& s1) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      v0 += __shfl_xor(v0, o);
      v1 += __shfl_xor(v1, o);
    }
    if (d == 0) {
      red[r][0] = v0;
      red[r][1] = v1;
    }
    __syncthreads();
    double* slot = a.part + ((int64_t)(phase & 1) * gridDim.x + blockIdx.x) * 2;
    if (tid == 0) {
      double w0 = red[0][0], w1 = red[0][1];
      for (int w = 1; w < NT / 64; ++w) {
        w0 += red[w][0];
        w1 += red[w][1];
      }
      __hip_atomic_store(&slot[0], w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&slot[1], w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (grid_barrier(a.bar, gridDim.x)) aborted = true;
    if (r == 0) {
      double u0 = 0.0, u1 = 0.0;
      for (int g = d; g < (int)gridDim.x; g += 64) {
        const double* o = a.part + ((int64_t)(phase & 1) * gridDim.x + g) * 2;
        u0 += __hip_atomic_load(&o[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u1 += __hip_atomic_load(&o[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        u0 += __shfl_xor(u0, o);
        u1 += __shfl_xor(u1, o);
      }
      if (d == 0) {
        tot[0] = u0;
        tot[1] = u1;
      }
    }
    __syncthreads();
    s0 = tot[0];
    s1 = tot[1];
    ++phase;
  };

  // element adjoints: carried (current y, f0), this attempt's (y, y1, dt32, the outputs' d/d dt and
  // d/d t0 terms), the initial step's (scale, the probe's term of f0)
  float ybc = 0.f, fbc = 0.f, yb0 = 0.f, yb1 = 0.f, dtb32 = 0.f, scb = 0.f, f0bp = 0.f;
  double pd = 0.0, pt = 0.0;
  // the control chain, uniform over the grid, fp64: adjoints of the next dt and of t1s
  double dtbar = 0.0, tbar = 0.0, dtb_base = 0.0, h0b = 0.0, d0b = 0.0, d1b = 0.0;
  float dt32 = 0.f, h0f = 0.f;
  int jj = a.T - 1;  // the last output not yet taken
  bool acc_n = false;
  __syncthreads();

  for (int ev = n_ev - 1; ev >= 0 && !aborted; --ev) {
    const bool in_att = ev >= base;
    const int n = in_att ? (ev - base) / 6 : -1, s = in_att ? 2 + (ev - base) % 6 : 0;
    float kb0 = 0.f;  // output adjoint of evaluations 0 / 1
    // ---------------- before the VJP: this evaluation's output adjoint ----------------
    if (in_att && s == 7) {
      const double t0 = a.att[4 * n], dt = a.att[4 * n + 1];
      const float ratio = (float)a.att[4 * n + 2];
      acc_n = a.att[4 * n + 3] != 0.0;
      int m = n - 1;  // the attempt whose stage 7 produced this attempt's y and f0
      while (m >= 0 && a.att[4 * m + 3] == 0.0) --m;
      const int fe = m >= 0 ? base + 6 * m + 5 : 0;
      const int e2 = base + 6 * n;
      dt32 = (float)dt;
      const double rr = (double)ratio;
      double rbar = 0.0, dtbb = 0.0;
      if (n + 1 < a.n_att)
        dopri_next_dt_adjoint(dtbar, dt, a.att[4 * (n + 1) + 1], rr, a.step.ifactor, a.step.dfactor, a.step.min_step,
                              a.step.max_step, dtbb, rbar);
      dtb_base = dtbb;
      pd = pt = 0.0;
      dtb32 = 0.f;
      float kv[8], kbv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) kv[j] = kbv[j] = 0.f;
      float y = 0.f, y1 = 0.f;
      if (el) {
        y = tx(fe);
        kv[1] = tk(fe);
#pragma unroll
        for (int j = 2; j <= 7; ++j) kv[j] = tk(e2 + j - 2);
        y1 = tx(e2 + 5);
      }
      // err and mid in the forward's op order
      float err = kv[1] * (a.tab.cerr[0] * dt32), midv = kv[1] * (a.tab.cmid[0] * dt32);
#pragma unroll
      for (int j = 2; j <= 7; ++j) {
        err = err + kv[j] * (a.tab.cerr[j - 1] * dt32);
        midv = midv + kv[j] * (a.tab.cmid[j - 1] * dt32);
      }
      float midb = 0.f, fab;
      if (acc_n) {
        yb1 = ybc;
        kbv[7] = fbc;
        yb0 = 0.f;
        fab = 0.f;
        const float fa = kv[1], fbk = kv[7];
        float co[5];  // the forward's interpolant
        dopri_fit(co, y, y1, midv, fa, fbk, dt32);
        float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f, c4 = 0.f;
        const double t1 = t0 + dt, dlt = t1 - t0;
        for (; jj >= 1 && a.t[jj] > t0; --jj) {  // outputs in (t0, t1]: uniform over the grid
          const float x = (float)((a.t[jj] - t0) / dlt);
          const float g = el ? a.gsol[(int64_t)jj * BD + bo] : 0.f;
          const float x2 = x * x, x3 = x2 * x;
          c0 += g;
          c1 += g * x;
          c2 += g * x2;
          c3 += g * x3;
          c4 += g * (x3 * x);
          const float dsdx = co[1] + 2.0f * x * co[2] + 3.0f * x2 * co[3] + 4.0f * x3 * co[4];
          const double xbd = (double)(g * dsdx);
          pt += xbd * (-1.0 / dlt);
          pd += xbd * (-(double)x / dlt);
        }
        yb0 += ((c0 - 11.0f * c2) + 18.0f * c3) - 8.0f * c4;
        yb1 += (-5.0f * c2 + 14.0f * c3) - 8.0f * c4;
        const float ymb = (16.0f * c2 - 32.0f * c3) + 16.0f * c4;
        fab += dt32 * (((c1 - 4.0f * c2) + 5.0f * c3) - 2.0f * c4);
        kbv[7] += dt32 * ((c2 - 3.0f * c3) + 2.0f * c4);
        dtb32 += ((c1 * fa + c2 * (fbk - 4.0f * fa)) + c3 * (5.0f * fa - 3.0f * fbk)) + c4 * (2.0f * (fbk - fa));
        yb0 += ymb;
        midb = ymb;
      } else {
        yb0 = ybc;
        fab = fbc;
        yb1 = 0.f;
      }
      kbv[1] = fab;
      // error ratio = rms(err / tol): d ratio / d qe = qe / (N ratio)
      float errb = 0.f;
      if (el && rbar != 0.0 && ratio > 0.f) {
        const float tol = a.atol + a.rtol * fmaxf(fabsf(y), fabsf(y1));
        const float qe = err / tol;
        const float qb = (float)(rbar * (double)qe / (a.n_el * rr));
        errb = qb / tol;
        const float tolb = -qb * qe / tol, ay = fabsf(y), ay1 = fabsf(y1);
        const float sy = y > 0.f ? 1.f : (y < 0.f ? -1.f : 0.f), sy1 = y1 > 0.f ? 1.f : (y1 < 0.f ? -1.f : 0.f);
        const float wy = ay > ay1 ? 1.f : (ay < ay1 ? 0.f : 0.5f);
        yb0 += tolb * a.rtol * wy * sy;
        yb1 += tolb * a.rtol * (1.f - wy) * sy1;
      }
      float se = 0.f, sm = 0.f;
#pragma unroll
      for (int j = 1; j <= 7; ++j) {
        kbv[j] += errb * (a.tab.cerr[j - 1] * dt32) + midb * (a.tab.cmid[j - 1] * dt32);
        se += a.tab.cerr[j - 1] * kv[j];
        sm += a.tab.cmid[j - 1] * kv[j];
      }
      dtb32 += errb * se + midb * sm;
#pragma unroll
      for (int j = 1; j <= 7; ++j) {
        s_k[j][r][d] = kv[j];
        s_kb[j][r][d] = kbv[j];
      }
    } else if (!in_att && ev == 1) {
      // _select_initial_step (fp32): dt0 = min(100 h0, |h1|)
      const float d1 = (float)a.init_rec[1], d2 = (float)a.init_rec[2];
      const float h0 = (float)a.init_rec[3], h1 = (float)a.init_rec[4];
      h0f = h0;
      const double dtb = dtbar;
      double h1b = 0.0;
      h0b = 0.0;
      const float a100 = 100.0f * h0, ah1 = fabsf(h1), sh1 = h1 < 0.f ? -1.f : 1.f;
      if (a100 < ah1) h0b = 100.0 * dtb;
      else if (ah1 < a100) h1b = dtb * sh1;
      else {
        h0b = 50.0 * dtb;
        h1b = 0.5 * dtb * sh1;
      }
      double d2b = 0.0, d1b_ = 0.0;
      if (d1 <= 1e-15f && d2 <= 1e-15f) {  // h1 = max(1e-6, h0 1e-3)
        const float v = h0 * 1e-3f;
        if (v > 1e-6f) h0b += 1e-3 * h1b;
        else if (v == 1e-6f) h0b += 0.5e-3 * h1b;
      } else {  // h1 = (0.01 / max(d1, d2)) ** (1/5)
        const bool take2 = d2 > d1;
        const double mx = take2 ? d2 : d1;
        const double mxb = -(h1b * 0.2 * (double)h1) / mx;
        if (take2) d2b += mxb;
        else d1b_ += mxb;
      }
      // d2 = |rms((f1 - f0) / scale) / h0|
      const double r2 = (double)d2 * h0, r2b = d2b / h0;
      h0b = h0b - d2b * d2 / h0;
      d1b = d1b_;
      float f1b = 0.f;
      f0bp = scb = 0.f;
      if (el && r2 > 0.0) {
        const float y = tx(0), f0 = tk(0), f1 = tk(1);
        const float scale = a.atol + a.rtol * fabsf(y);
        const float q2 = (f1 - f0) / scale;
        const float q2b = (float)(r2b * (double)q2 / (a.n_el * r2));
        f1b = q2b / scale;
        f0bp = -q2b / scale;
        scb = -q2b * q2 / scale;
      }
      kb0 = f1b;
      d0b = 0.0;
    } else if (ev == 0) {
      if (base == 2) {  // the rest of _select_initial_step: d0 = rms(y0 / scale), d1 = rms(f0 / scale)
        const float d0 = (float)a.init_rec[0], d1 = (float)a.init_rec[1];
        if (el) {
          const float y = tx(0), f0 = tk(0);
          const float scale = a.atol + a.rtol * fabsf(y);
          const float q0 = y / scale, q1 = f0 / scale;
          const float q0b = d0 > 0.f ? (float)(d0b * (double)q0 / (a.n_el * d0)) : 0.f;
          const float q1b = d1 > 0.f ? (float)(d1b * (double)q1 / (a.n_el * d1)) : 0.f;
          const float sc = scb - q0b * q0 / scale - q1b * q1 / scale;
          const float sy = y > 0.f ? 1.f : (y < 0.f ? -1.f : 0.f);
          ybc += q0b / scale + sc * a.rtol * sy;
          fbc += q1b / scale;
        }
      }
      kb0 = el ? fbc : 0.f;
    }
    const float xb = vjp(ev, in_att ? s_kb[s][r][d] : kb0);
    // ---------------- after the VJP: the input adjoint ----------------
    if (in_att) {
      const float X = xb + (s == 7 ? yb1 : 0.f);  // stage 7's input IS y1
      yb0 += X;
      float sb = 0.f;
      for (int j = 1; j < s; ++j) {  // tableau row s - 2
        const float c = a.tab.beta[s - 2][j - 1];
        s_kb[j][r][d] += (c * dt32) * X;
        sb += c * s_k[j][r][d];
      }
      dtb32 += X * sb;
      if (s == 2) {  // attempt n done: the carries, and the grid sum of its d/d dt and d/d t0 terms
        ybc = el ? yb0 : 0.f;
        fbc = el ? s_kb[1][r][d] : 0.f;
        double S0, S1;
        gsum(el ? pd + (double)dtb32 : 0.0, el ? pt : 0.0, S0, S1);
        dtbar = dtb_base + (acc_n ? tbar : 0.0) + S0;
        tbar = tbar + S1;
      }
    } else if (ev == 1) {  // the probe: input y0 + h0 f0
      const float f0 = el ? tk(0) : 0.f;
      if (el) {
        ybc += xb;
        fbc += xb * h0f + f0bp;
      }
      double S0, S1;
      gsum(el ? (double)(xb * f0) : 0.0, 0.0, S0, S1);
      h0b = h0b + S0;
      dopri_h0_adjoint(h0b, h0f, (float)a.init_rec[0], (float)a.init_rec[1], d0b, d1b);
    } else {  // evaluation 0: f(y0)
      if (el) {
        ybc += xb;
        if (a.gy0) a.gy0[bo] = ybc + a.gsol[bo];  // solution[0] = y0
      }
    }
  }
  if (blockIdx.x == 0 && tid == 0)
    a.status[0] =
        (aborted || __hip_atomic_load(a.bar + 64 * 9 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ? 4 : 0;
}

// ---------------------------------------------------------------------------------------------
// Parameter gradients over the N = n_ev * B samples (evaluation e = n / B, row n % B), in tiles of
// kTS samples dealt round-robin to the workgroups.
// ---------------------------------------------------------------------------------------------
constexpr int kTS = 16;        // samples per tile
constexpr int kOG = 16;        // head outputs per workgroup of the head kernel
constexpr int kHeadBlocks = 64;    // most sample groups of the head kernel
constexpr int kBasisBlocks = 256;  // ... of the basis kernel

struct EcgParamArgs {
  HL L;
  const float* w;      // (D, F)
  int D, F, Fp;
  const float* prev0;  // (F)
  int64_t B, N;        // N = n_ev * B samples
  const float* tape;   // (n_ev, 2, B, D)
  const float* gtape;  // (n_ev, B, D)
  float* part;         // the kernel's per-workgroup sums
  float* part_b;       // head kernel: the head bias' sums
};

// input and hysteresis memory of sample n's input i (the memory of evaluation 0 is per basis: prev0[q])
__device__ __forceinline__ void sample_x(const EcgParamArgs& a, int64_t n, int i, int q, float& x, float& pv) {
  const int64_t e = n / a.B, row = n - e * a.B, BD = a.B * a.D;
  x = a.tape[e * 2 * BD + row * a.D + i];
  pv = e == 0 ? a.prev0[q] : a.tape[(e - 1) * 2 * BD + (a.B - 1) * a.D + i];
}

// d loss / d W[o, q] = sum_n g[n, o] phi[n, q], d loss / d b[o] = sum_n g[n, o] (head_gw_kernel's
// element formulas): workgroup (x, y) sums outputs 16 y .. 16 y + 15 over the tiles x, x + gridDim.x, ...;
// thread tid owns q = tid + 256 c.  part (gridDim.x, D, F), part_b (gridDim.x, D).
__global__ __launch_bounds__(256) void ecg_head_grad_kernel(EcgParamArgs a) {
  extern __shared__ float s_phi[];       // (kTS, Fp)
  __shared__ float4 s_g[kTS][kOG / 4];   // the tile's output adjoints of this workgroup's outputs
  const int tid = threadIdx.x, F = a.F, Fp = a.Fp, D = a.D, nb = a.L.nb;
  const int o0 = blockIdx.y * kOG;
  const float gs = a.L.gs, bp = a.L.bp;
  float acc[kQPT][kOG];
#pragma unroll
  for (int c = 0; c < kQPT; ++c)
#pragma unroll
    for (int o = 0; o < kOG; ++o) acc[c][o] = 0.f;
  float accb = 0.f;
  const int64_t ntiles = (a.N + kTS - 1) / kTS;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t n0 = tile * kTS;
    for (int idx = tid; idx < kTS * F; idx += 256) {
      const int sm = idx / F, q = idx - sm * F;
      float v = 0.f;
      if (n0 + sm < a.N) {
        float x, pv;
        sample_x(a, n0 + sm, q / nb, q, x, pv);
        v = rpoint(make_float4(a.L.k[q], a.L.Ec[q], a.L.Ps[q], a.L.bias[q]), gs, bp, x, pv).phi;
      }
      s_phi[sm * Fp + q] = v;
    }
    if (tid < kTS * kOG) {
      const int sm = tid / kOG, o = o0 + tid % kOG;
      reinterpret_cast<float*>(s_g)[tid] = (n0 + sm < a.N && o < D) ? a.gtape[(n0 + sm) * D + o] : 0.f;
    }
    __syncthreads();
#pragma unroll 2
    for (int sm = 0; sm < kTS; ++sm) {
      float gv[kOG];
#pragma unroll
      for (int o4 = 0; o4 < kOG / 4; ++o4) {
        const float4 g4 = s_g[sm][o4];
        gv[4 * o4] = g4.x;
        gv[4 * o4 + 1] = g4.y;
        gv[4 * o4 + 2] = g4.z;
        gv[4 * o4 + 3] = g4.w;
      }
#pragma unroll
      for (int c = 0; c < kQPT; ++c) {
        const float p = s_phi[sm * Fp + min(tid + 256 * c, F - 1)];
#pragma unroll
        for (int o = 0; o < kOG; ++o) acc[c][o] = __builtin_fmaf(gv[o], p, acc[c][o]);
      }
      if (tid < kOG) accb += reinterpret_cast<const float*>(s_g[sm])[tid];
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < kQPT; ++c) {
    const int q = tid + 256 * c;
    if (q < F)
#pragma unroll
      for (int o = 0; o < kOG; ++o)
        if (o0 + o < D) a.part[((int64_t)blockIdx.x * D + o0 + o) * F + q] = acc[c][o];
  }
  if (tid < kOG && o0 + tid < D) a.part_b[(int64_t)blockIdx.x * D + o0 + tid] = accb;
}

// d loss / d (k, Ec, Ps, bias)[q] = sum_n g_basis[n, q] d basis / d (.) (mixer_gparam_kernel's element
// formulas), g_phi recomputed from the gradient tape: workgroup x sums the tiles x, x + gridDim.x, ...;
// thread tid owns q = tid + 256 c.  part (gridDim.x, 4, F).
__global__ __launch_bounds__(256) void ecg_basis_grad_kernel(EcgParamArgs a) {
  __shared__ float4 s_g[64][kTS / 4];  // [output][sample]
  __shared__ float s_x[kTS][64], s_pv[kTS][64];
  __shared__ int s_e0[kTS];            // the sample belongs to evaluation 0 (memory per basis: prev0)
  const int tid = threadIdx.x, F = a.F, D = a.D, nb = a.L.nb;
  const float gs = a.L.gs, bp = a.L.bp;
  float sk[kQPT], sE[kQPT], sP[kQPT], sb[kQPT];
  int qc[kQPT];
  float4 pr[kQPT];
#pragma unroll
  for (int c = 0; c < kQPT; ++c) {
    sk[c] = sE[c] = sP[c] = sb[c] = 0.f;
    qc[c] = min(tid + 256 * c, F - 1);
    pr[c] = make_float4(a.L.k[qc[c]], a.L.Ec[qc[c]], a.L.Ps[qc[c]], a.L.bias[qc[c]]);
  }
  const int64_t ntiles = (a.N + kTS - 1) / kTS;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t n0 = tile * kTS;
    for (int idx = tid; idx < kTS * 64; idx += 256) {
      const int sm = idx / 64, i = idx % 64;
      const bool ok = n0 + sm < a.N && i < D;
      float x = 0.f, pv = 0.f;
      if (ok) sample_x(a, n0 + sm, i, 0, x, pv);
      s_x[sm][i] = x;
      s_pv[sm][i] = pv;
      reinterpret_cast<float*>(s_g)[i * kTS + sm] = ok ? a.gtape[(n0 + sm) * D + i] : 0.f;
      if (i == 0) s_e0[sm] = (n0 + sm < a.N && (n0 + sm) / a.B == 0) ? 1 : 0;
    }
    __syncthreads();
    float gp[kQPT][kTS];
#pragma unroll
    for (int c = 0; c < kQPT; ++c)
#pragma unroll
      for (int sm = 0; sm < kTS; ++sm) gp[c][sm] = 0.f;
#pragma unroll 2
    for (int o = 0; o < D; ++o) {
      float gv[kTS];
#pragma unroll
      for (int s4 = 0; s4 < kTS / 4; ++s4) {
        const float4 g4 = s_g[o][s4];
        gv[4 * s4] = g4.x;
        gv[4 * s4 + 1] = g4.y;
        gv[4 * s4 + 2] = g4.z;
        gv[4 * s4 + 3] = g4.w;
      }
#pragma unroll
      for (int c = 0; c < kQPT; ++c) {
        const float wv = a.w[(int64_t)o * F + qc[c]];
#pragma unroll
        for (int sm = 0; sm < kTS; ++sm) gp[c][sm] = __builtin_fmaf(gv[sm], wv, gp[c][sm]);
      }
    }
#pragma unroll
    for (int c = 0; c < kQPT; ++c) {
      const int i = qc[c] / nb;
#pragma unroll
      for (int sm = 0; sm < kTS; ++sm) {
        const float pv = s_e0[sm] ? a.prev0[qc[c]] : s_pv[sm][i];
        const RPoint p = rpoint(pr[c], gs, bp, s_x[sm][i], pv);
        const float gb = gp[c][sm] * (p.phi * (1.0f - p.phi));  // 0 for the samples past N
        sk[c] = __builtin_fmaf(gb, p.dk, sk[c]);
        sE[c] = __builtin_fmaf(gb, p.dEc, sE[c]);
        sP[c] = __builtin_fmaf(gb, p.dPs, sP[c]);
        sb[c] += gb;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < kQPT; ++c) {
    const int q = tid + 256 * c;
    if (q < F) {
      float* o = a.part + (int64_t)blockIdx.x * 4 * F + q;
      o[0] = sk[c];
      o[F] = sE[c];
      o[2 * F] = sP[c];
      o[3 * F] = sb[c];
    }
  }
}

// out[i] = sum over the workgroups g (ascending) of part[g * stride + i]: up to six outputs in one launch
struct PsumJobs {
  const float* part[6];
  float* out[6];
  int n[6], stride[6], G[6];
};
__global__ __launch_bounds__(256) void ecg_psum_kernel(PsumJobs j) {
  const int k = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (!j.out[k] || i >= j.n[k]) return;
  const float* p = j.part[k] + i;
  float acc = 0.f;
  for (int g = 0; g < j.G[k]; ++g) acc += p[(int64_t)g * j.stride[k]];
  j.out[k][i] = acc;
}

int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }

// workspace: barrier words | grid-sum slots | gradient tape | head sums | head-bias sums | basis sums
struct WsLayout {
  int64_t part, gtape, pw, pb, pp, end;
};
WsLayout ws_layout(int64_t B, int D, int F, int64_t n_ev) {
  WsLayout l;
  const int64_t grid = (B + kBwdRows - 1) / kBwdRows;
  l.part = align16((int64_t)sizeof(unsigned) * kBarWords);
  l.gtape = align16(l.part + (int64_t)sizeof(double) * 2 * 2 * grid);
  l.pw = align16(l.gtape + (int64_t)sizeof(float) * n_ev * B * D);
  l.pb = align16(l.pw + (int64_t)sizeof(float) * kHeadBlocks * D * F);
  l.pp = align16(l.pb + (int64_t)sizeof(float) * kHeadBlocks * D);
  l.end = align16(l.pp + (int64_t)sizeof(float) * kBasisBlocks * 4 * F);
  return l;
}

size_t bwd_lds(int F) { return sizeof(float) * (size_t)(4 * F + kBwdRows * ((F + 3) & ~3)); }

// the most workgroups of the sweep that are resident at once (0: none, < 0: no device)
int64_t bwd_max_grid(int F) {
  const int n_cu = device_cus();
  const int per_cu = n_cu > 0 ? occupancy_per_cu(reinterpret_cast<const void*>(ecg_dopri5_bwd_kernel), kBwdThreads, bwd_lds(F)) : -1;
  if (per_cu < 0) return -1;
  // one workgroup per CU below the API's answer when it admits several (it can be one too high)
  return (int64_t)(per_cu > 1 ? per_cu - 1 : per_cu) * n_cu;
}

int check_shape(const fetode_hlogistic_t* layer, const char* what) {
  int rc = check_layer(layer);
  if (rc) return rc;
  if (layer->in_dim > 64)
    return set_err(FETODE_EUNSUPPORTED, "%s: in_dim %d > 64", what, layer->in_dim);
  const int F = layer->in_dim * layer->num_basis;
  if (F > kMaxF) return set_err(FETODE_EUNSUPPORTED, "%s: in*num_basis=%d > %d", what, F, kMaxF);
  return FETODE_OK;
}

}  // namespace

extern "C" {

int64_t fetode_ecg_dopri5_backward_max_batch(const fetode_hlogistic_t* layer) {
  const int rc = check_shape(layer, "ecg dopri5 backward");
  if (rc) return rc == FETODE_EUNSUPPORTED ? 0 : -1;
  const int64_t g = bwd_max_grid(layer->in_dim * layer->num_basis);
  return g < 0 ? -1 : g * kBwdRows;
}

int64_t fetode_ecg_dopri5_backward_workspace(const fetode_hlogistic_t* layer, int64_t B, int32_t n_ev) {
  if (check_shape(layer, "ecg dopri5 backward") || B <= 0 || n_ev <= 0) return -1;
  return ws_layout(B, layer->in_dim, layer->in_dim * layer->num_basis, n_ev).end;
}

int fetode_ecg_dopri5_backward(const fetode_hlogistic_t* layer, const float* w, int32_t D, const float* prev,
                               int64_t B, const double* t, int32_t T, double rtol, double atol, const double* opts,
                               const float* tableau, const float* grad_solution, const float* tape, int32_t n_ev,
                               const double* attempts, int32_t n_att, const double* init_rec, float* grad_y0,
                               float* gw, float* gbias_head, float* gk, float* gEc, float* gPs, float* gbias,
                               void* workspace, int32_t* status, void* stream) {
  int rc = check_layer(layer);
  if (rc) return rc;
  if (B <= 0 || T <= 0) return FETODE_OK;
  if (!w || !prev || !t || !opts || !tableau || !grad_solution || !tape || !attempts || !init_rec || !workspace ||
      !status)
    return set_err(FETODE_EINVAL, "ecg dopri5 backward: null pointer");
  if (D != layer->in_dim) return set_err(FETODE_EINVAL, "ecg dopri5 backward: state dim %d (must equal in_dim)", D);
  rc = check_shape(layer, "ecg dopri5 backward");
  if (rc) return rc;
  const int F = layer->in_dim * layer->num_basis;
  const int base = dopri_base(opts);
  if (n_att < 0 || (int64_t)n_ev != (int64_t)base + 6 * (int64_t)n_att)
    return set_err(FETODE_EINVAL, "ecg dopri5 backward: %d evaluations do not match %d attempts (expected %lld)", n_ev,
                   n_att, (long long)base + 6 * (long long)n_att);
  const int64_t grid = (B + kBwdRows - 1) / kBwdRows;
  const int64_t max_grid = bwd_max_grid(F);
  if (max_grid < 0) return set_err(FETODE_EHIP, "ecg dopri5 backward: no device");
  if (grid > max_grid)
    return set_err(FETODE_EUNSUPPORTED, "ecg dopri5 backward: batch %lld does not fit one resident grid", (long long)B);
  const WsLayout wl = ws_layout(B, D, F, n_ev);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  EcgBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.L = to_dev(layer);
  a.w = w;
  a.D = D;
  a.F = F;
  a.Fp = (F + 3) & ~3;
  a.prev0 = prev;
  a.B = B;
  a.t = t;
  a.T = T;
  a.rtol = (float)rtol;
  a.atol = (float)atol;
  dopri_step_from_opts(opts, a.step);
  a.n_el = (double)(B * D);
  memcpy(&a.tab, tableau, sizeof(DopriTab));
  a.gsol = grad_solution;
  a.tape = tape;
  a.n_ev = n_ev;
  a.n_att = n_att;
  a.base = base;
  a.att = attempts;
  a.init_rec = init_rec;
  a.gy0 = grad_y0;
  a.gtape = (float*)(ws + wl.gtape);
  a.part = (double*)(ws + wl.part);
  a.bar = (unsigned*)ws;
  a.status = status;
  HIP_CHECK_RET(hipMemsetAsync(workspace, 0, (size_t)wl.part, s));
  void* args[] = {&a};
  HIP_CHECK_RET(resident_launch(reinterpret_cast<const void*>(ecg_dopri5_bwd_kernel), dim3((unsigned)grid),
                                dim3(kBwdThreads), args, bwd_lds(F), s));
  // the parameter sums over the stacked samples
  EcgParamArgs p;
  memset(&p, 0, sizeof(p));
  p.L = a.L;
  p.w = w;
  p.D = D;
  p.F = F;
  p.Fp = a.Fp;
  p.prev0 = prev;
  p.B = B;
  p.N = (int64_t)n_ev * B;
  p.tape = tape;
  p.gtape = a.gtape;
  const int64_t ntiles = (p.N + kTS - 1) / kTS;
  PsumJobs j;
  memset(&j, 0, sizeof(j));
  int max_n = 0;
  if (gw || gbias_head) {
    const int G = (int)std::min<int64_t>(ntiles, kHeadBlocks);
    p.part = (float*)(ws + wl.pw);
    p.part_b = (float*)(ws + wl.pb);
    hipLaunchKernelGGL(ecg_head_grad_kernel, dim3(G, (D + kOG - 1) / kOG), dim3(256), sizeof(float) * kTS * p.Fp, s, p);
    LAUNCH_CHECK();
    j.part[0] = p.part, j.out[0] = gw, j.n[0] = D * F, j.stride[0] = D * F, j.G[0] = G;
    j.part[1] = p.part_b, j.out[1] = gbias_head, j.n[1] = D, j.stride[1] = D, j.G[1] = G;
    max_n = D * F;
  }
  if (gk || gEc || gPs || gbias) {
    const int G = (int)std::min<int64_t>(ntiles, kBasisBlocks);
    p.part = (float*)(ws + wl.pp);
    p.part_b = nullptr;
    hipLaunchKernelGGL(ecg_basis_grad_kernel, dim3(G), dim3(256), 0, s, p);
    LAUNCH_CHECK();
    float* outs[4] = {gk, gEc, gPs, gbias};
    for (int k = 0; k < 4; ++k)
      j.part[2 + k] = p.part + (int64_t)k * F, j.out[2 + k] = outs[k], j.n[2 + k] = F, j.stride[2 + k] = 4 * F,
                 j.G[2 + k] = G;
    max_n = std::max(max_n, F);
  }
  if (max_n) {
    hipLaunchKernelGGL(ecg_psum_kernel, dim3(nblk(max_n, 256), 6), dim3(256), 0, s, j);
    LAUNCH_CHECK();
  }
  return FETODE_OK;
}

}  // extern "C"
