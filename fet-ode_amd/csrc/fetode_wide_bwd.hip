// fetode_wide_bwd.hip — loss.backward() through the device-resident dopri5 solve of the two-layer
// wide KAN-FET field (train_kan_fet_ett.py:192 then :312-335: odeint(self.dynamics, z0, t_fut,
// method="dopri5") followed by loss.backward()): reverse mode through every evaluation of every
// attempt (rejected ones included), the stage sums, the error norm, the step-size control, the
// initial-step selection and the dense output, like autograd through torchdiffeq (which detaches
// none of them).  The adjoint algebra is fetode_ecg_bwd.hip's (ecg_dopri5_bwd_kernel), the control
// chain fetode_dopri_ctl.h's, carried in fp64.
//
// Tape (fetode_wide_dopri5_tape): three planes x (cap, B, D), h (cap, B, H), k (cap, B, D): the
// layer-0 input, the hidden and the output of evaluation e; (t0, dt, error ratio, accepted) per
// attempt; the initial-step scalars {d0, d1, d2, h0, h1}.  Evaluation order: 0 = f(y0), 1 = the
// initial-step probe (absent with first_step), then six per attempt (stages 2..7; stage 7's input
// is the attempt's y1, its output the next f0).  The hysteresis memory of evaluation e is x_{e-1}
// for layer 0 and h_{e-1} for layer 1 (prev0 / prev1, or the first-call rule, for e = 0); no
// gradient flows through the memory (ferro_class.py:381-382).
//
// The sweep is an ordinary sequence of launches on the caller's stream: no persistent kernel, no
// grid barrier, no spin, no host synchronisation.  Per attempt, latest first:
//   wb_ctl_kernel    one workgroup: finishes the later attempt's fp64 partials (its d/d dt and
//                    d/d t0 sums) and advances the control adjoints (dt, ratio, t) to this attempt
//   wb_head_kernel   per element: seeds the adjoints of k_1..k_7 and of y / y1 from the accepted
//                    step's dense-output rows of gsol, the error norm and the carried f0 / y adjoints
//   stages 7..2      d/dx of the evaluation through the wide VJPs (layer 1 then layer 0, x and prev
//                    straight from the tape, no parameter outputs), then wb_stage_kernel: the
//                    input adjoint into the attempt's y adjoint and, times beta_sj dt, into the
//                    adjoints of k_j (j < s), and per-workgroup fp64 partials of <gx_s, sum_j beta_sj k_j>
// then the initial step (probe and f(y0)) the same way.  No atomics: every sum runs in a fixed
// order (element -> workgroup: xor tree per wave, waves in order; workgroups: strided per thread,
// then the same tree), so two runs give the same bits.
//
// Parameter gradients are sums over the stacked (evaluation, row) samples.  The sweep keeps the
// output adjoints gk (C, B, D) and hidden adjoints gh (C, B, H) of a chunk of C = 6 A consecutive
// evaluations (A whole attempts, C B near FETODE_WIDE_BWD_ROWS = 8192 rows, where the wide VJPs
// were tuned) and, once the chunk's first attempt is done, calls each layer's VJPs ONCE over the
// chunk's C B rows (x: the chunk's tape planes, prev: the same planes shifted by one evaluation).
// Summation order: chunks are counted from the LAST attempt backwards (the earliest chunk may be
// shorter) and accumulate latest first, each in its VJP kernel's fixed order over the stacked rows;
// then the probe evaluation and evaluation 0 (its own first-call rule) as calls of their own.
#include <algorithm>
#include <cstring>

#include "fetode_common.h"
#include "fetode_dopri_ctl.h"
#include "fetode_ecg_dev.h"

using namespace fetode;

namespace {

constexpr int kWbT = 256;     // threads of the element kernels
constexpr int kWbSlots = 7;   // partial slots: stages 2..7, then the head's

// the uniform state of the sweep (device memory; written by wb_ctl_kernel / wb_init_ctl_kernel)
struct WbCtl {
  double dtbar, tbar;      // adjoints of the next attempt's dt and t0
  double dtb_base, rbar;   // this attempt: the next dt's part for dt, the error ratio's adjoint
  double t0, dt, ratio;
  double h0b, d0b, d1b, r2, r2b;  // the initial step's
  int acc, fe, j_lo, j_hi, jj, pad;
};

struct WbArgs {
  int64_t n;  // B * D
  float rtol, atol;
  double n_el;
  DopriTab tab;
  DopriStep step;
  const double* t;
  int T;
  const float* gsol;  // (T, B, D)
  const float* tx;    // tape planes x / k (cap, B, D)
  const float* tk;
  const double* att;
  int n_att, base;
  const double* init_rec;
  WbCtl* ctl;
  double* part;  // (kWbSlots, nwg, 2)
  int nwg;
  float *Y0, *Y1, *F, *GX, *SCB, *F0BP;  // (B, D) planes: y / y1 / f0 adjoints, the VJP's d/dx, the initial step's
  float* gy0;
};

__device__ __forceinline__ double wb_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the workgroup's sums of two per-thread values (xor tree per wave, waves in order) -> part[slot][wg]
__device__ __forceinline__ void wb_put_partial(const WbArgs& a, int slot, double v0, double v1) {
  __shared__ double red[kWbT / 64][2];
  v0 = wb_wave_sum(v0);
  v1 = wb_wave_sum(v1);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = v0;
    red[threadIdx.x >> 6][1] = v1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double w0 = red[0][0], w1 = red[0][1];
    for (int w = 1; w < kWbT / 64; ++w) {
      w0 += red[w][0];
      w1 += red[w][1];
    }
    double* o = a.part + ((int64_t)slot * a.nwg + blockIdx.x) * 2;
    o[0] = w0;
    o[1] = w1;
  }
}

// one workgroup: the sums over slots [0, nslot) x workgroups of the partials, in a fixed order
__device__ __forceinline__ void wb_finish(const WbArgs& a, int nslot, double& s0, double& s1) {
  __shared__ double red[kWbT / 64][2];
  __shared__ double tot[2];
  double v0 = 0.0, v1 = 0.0;
  for (int sl = 0; sl < nslot; ++sl)
    for (int g = threadIdx.x; g < a.nwg; g += kWbT) {
      const double* o = a.part + ((int64_t)sl * a.nwg + g) * 2;
      v0 += o[0];
      v1 += o[1];
    }
  v0 = wb_wave_sum(v0);
  v1 = wb_wave_sum(v1);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = v0;
    red[threadIdx.x >> 6][1] = v1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double w0 = red[0][0], w1 = red[0][1];
    for (int w = 1; w < kWbT / 64; ++w) {
      w0 += red[w][0];
      w1 += red[w][1];
    }
    tot[0] = w0;
    tot[1] = w1;
  }
  __syncthreads();
  s0 = tot[0];
  s1 = tot[1];
}

// Attempt n's control (n = -1: the initial step's).  Finishes attempt n + 1's partials first.
__global__ __launch_bounds__(kWbT) void wb_ctl_kernel(WbArgs a, int n) {
  double S0 = 0.0, S1 = 0.0;
  const bool later = n + 1 < a.n_att;
  if (later) wb_finish(a, kWbSlots, S0, S1);
  if (threadIdx.x != 0) return;
  WbCtl c = *a.ctl;
  if (later) {
    c.dtbar = c.dtb_base + (c.acc ? c.tbar : 0.0) + S0;
    c.tbar = c.tbar + S1;
  } else {
    c.dtbar = c.tbar = 0.0;
    c.jj = a.T - 1;  // the last output not yet taken
  }
  if (n >= 0) {
    const double t0 = a.att[4 * n], dt = a.att[4 * n + 1];
    const double rr = (double)(float)a.att[4 * n + 2];
    c.acc = a.att[4 * n + 3] != 0.0;
    int m = n - 1;  // the attempt whose stage 7 produced this attempt's y and f0
    while (m >= 0 && a.att[4 * m + 3] == 0.0) --m;
    c.fe = m >= 0 ? a.base + 6 * m + 5 : 0;
    double rbar = 0.0, dtbb = 0.0;
    if (later)
      dopri_next_dt_adjoint(c.dtbar, dt, a.att[4 * (n + 1) + 1], rr, a.step.ifactor, a.step.dfactor, a.step.min_step,
                            a.step.max_step, dtbb, rbar);
    c.dtb_base = dtbb;
    c.rbar = rbar;
    c.t0 = t0;
    c.dt = dt;
    c.ratio = rr;
    c.j_hi = c.jj;
    if (c.acc)
      while (c.jj >= 1 && a.t[c.jj] > t0) --c.jj;  // outputs in (t0, t1]
    c.j_lo = c.jj + 1;
  } else if (a.base == 2) {  // dt_0 = _select_initial_step's min(100 h0, |h1|)
    dopri_dt0_adjoint(c.dtbar, (float)a.init_rec[1], (float)a.init_rec[2], (float)a.init_rec[3],
                      (float)a.init_rec[4], c.h0b, c.d1b, c.r2, c.r2b);
    c.d0b = 0.0;
  }
  *a.ctl = c;
}

// after the probe's VJP: h0b takes the sum of xb f0, then back to d0 and d1
__global__ __launch_bounds__(kWbT) void wb_init_ctl_kernel(WbArgs a) {
  double S0, S1;
  wb_finish(a, 1, S0, S1);
  if (threadIdx.x != 0) return;
  WbCtl c = *a.ctl;
  c.h0b = c.h0b + S0;
  dopri_h0_adjoint(c.h0b, (float)a.init_rec[3], (float)a.init_rec[0], (float)a.init_rec[1], c.d0b, c.d1b);
  *a.ctl = c;
}

// The attempt's head: the adjoints of k_1 (F), k_2..k_7 (kb: six planes, evaluation e2 + j - 2) and
// of y (Y0) / y1 (Y1), from the carried adjoints (Y0 = y's, F = f0's), the accepted step's output
// rows and the error ratio.  Partial slot 6: the outputs' d/d dt (+ the fit's and the norm's dt
// terms) and d/d t0 sums.
__global__ __launch_bounds__(kWbT) void wb_head_kernel(WbArgs a, int e2, float* __restrict__ kb) {
  const int64_t i = (int64_t)blockIdx.x * kWbT + threadIdx.x, n = a.n;
  const WbCtl& c = *a.ctl;
  const bool el = i < n;
  double pd = 0.0, pt = 0.0;
  if (el) {
    const int fe = c.fe;
    const bool acc = c.acc != 0;
    const double t0 = c.t0, dt = c.dt, rr = c.ratio, rbar = c.rbar;
    const float dt32 = (float)dt, ratio = (float)rr;
    const float ybc = a.Y0[i], fbc = a.F[i];
    float kv[8], kbv[8];
    kv[0] = kbv[0] = 0.f;
#pragma unroll
    for (int j = 1; j < 8; ++j) kbv[j] = 0.f;
    const float y = a.tx[(int64_t)fe * n + i];
    kv[1] = a.tk[(int64_t)fe * n + i];
#pragma unroll
    for (int j = 2; j <= 7; ++j) kv[j] = a.tk[(int64_t)(e2 + j - 2) * n + i];
    const float y1 = a.tx[(int64_t)(e2 + 5) * n + i];
    // err and mid in the forward's op order
    float err = kv[1] * (a.tab.cerr[0] * dt32), midv = kv[1] * (a.tab.cmid[0] * dt32);
#pragma unroll
    for (int j = 2; j <= 7; ++j) {
      err = err + kv[j] * (a.tab.cerr[j - 1] * dt32);
      midv = midv + kv[j] * (a.tab.cmid[j - 1] * dt32);
    }
    float midb = 0.f, fab, yb0, yb1, dtb32 = 0.f;
    if (acc) {
      yb1 = ybc;
      kbv[7] = fbc;
      yb0 = 0.f;
      fab = 0.f;
      const float fa = kv[1], fbk = kv[7];
      float co[5];  // the forward's interpolant
      dopri_fit(co, y, y1, midv, fa, fbk, dt32);
      float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f, c4 = 0.f;
      const double t1 = t0 + dt, dlt = t1 - t0;
      for (int jj = c.j_hi; jj >= c.j_lo; --jj) {
        const float x = (float)((a.t[jj] - t0) / dlt);
        const float g = a.gsol[(int64_t)jj * n + i];
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
    if (rbar != 0.0 && ratio > 0.f) {
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
    a.Y0[i] = yb0;
    a.Y1[i] = yb1;
    a.F[i] = kbv[1];
#pragma unroll
    for (int j = 2; j <= 7; ++j) kb[(int64_t)(j - 2) * n + i] = kbv[j];
    pd += (double)dtb32;
  }
  wb_put_partial(a, kWbSlots - 1, pd, pt);
}

// After the VJP of stage s (evaluation e2 + s - 2, d/dx in GX): X = gx (+ y1's adjoint at stage 7,
// whose input IS y1) into y's adjoint and, times beta dt, into the adjoints of k_j, j < s; partial
// slot s - 2: <X, sum_j beta_sj k_j> (the stage input's d/d dt).
__global__ __launch_bounds__(kWbT) void wb_stage_kernel(WbArgs a, int s, int e2, float* __restrict__ kb) {
  const int64_t i = (int64_t)blockIdx.x * kWbT + threadIdx.x, n = a.n;
  const WbCtl& c = *a.ctl;
  double pd = 0.0;
  if (i < n) {
    const float dt32 = (float)c.dt;
    const float X = a.GX[i] + (s == 7 ? a.Y1[i] : 0.f);
    a.Y0[i] += X;
    float sb = 0.f;
    for (int j = 1; j < s; ++j) {  // tableau row s - 2
      const float cf = a.tab.beta[s - 2][j - 1];
      float* kbj = j == 1 ? a.F + i : kb + (int64_t)(j - 2) * n + i;
      *kbj += (cf * dt32) * X;
      const float kj = j == 1 ? a.tk[(int64_t)c.fe * n + i] : a.tk[(int64_t)(e2 + j - 2) * n + i];
      sb += cf * kj;
    }
    pd = (double)(X * sb);
  }
  wb_put_partial(a, s - 2, pd, 0.0);
}

// The probe's output adjoint (g1, evaluation 1) from d2 = |rms((f1 - f0) / scale) / h0|, and the
// terms it leaves for f0 (F0BP) and the scale (SCB)
__global__ __launch_bounds__(kWbT) void wb_probe_head_kernel(WbArgs a, float* __restrict__ g1) {
  const int64_t i = (int64_t)blockIdx.x * kWbT + threadIdx.x, n = a.n;
  if (i >= n) return;
  const WbCtl& c = *a.ctl;
  float f1b = 0.f, f0bp = 0.f, scb = 0.f;
  if (c.r2 > 0.0) {
    const float y = a.tx[i], f0 = a.tk[i], f1 = a.tk[n + i];
    const float scale = a.atol + a.rtol * fabsf(y);
    const float q2 = (f1 - f0) / scale;
    const float q2b = (float)(c.r2b * (double)q2 / (a.n_el * c.r2));
    f1b = q2b / scale;
    f0bp = -q2b / scale;
    scb = -q2b * q2 / scale;
  }
  g1[i] = f1b;
  a.F0BP[i] = f0bp;
  a.SCB[i] = scb;
}

// after the probe's VJP (input y0 + h0 f0): partial slot 0 = <xb, f0>
__global__ __launch_bounds__(kWbT) void wb_probe_tail_kernel(WbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kWbT + threadIdx.x, n = a.n;
  double pd = 0.0;
  if (i < n) {
    const float xb = a.GX[i], f0 = a.tk[i], h0 = (float)a.init_rec[3];
    a.Y0[i] += xb;
    a.F[i] += xb * h0 + a.F0BP[i];
    pd = (double)(xb * f0);
  }
  wb_put_partial(a, 0, pd, 0.0);
}

// evaluation 0's output adjoint g0 = f0's adjoint, after the rest of _select_initial_step
// (d0 = rms(y0 / scale), d1 = rms(f0 / scale)) when the step was selected
__global__ __launch_bounds__(kWbT) void wb_f0_head_kernel(WbArgs a, float* __restrict__ g0) {
  const int64_t i = (int64_t)blockIdx.x * kWbT + threadIdx.x, n = a.n;
  if (i >= n) return;
  float fbc = a.F[i];
  if (a.base == 2) {
    const WbCtl& c = *a.ctl;
    const float d0 = (float)a.init_rec[0], d1 = (float)a.init_rec[1];
    const float y = a.tx[i], f0 = a.tk[i];
    const float scale = a.atol + a.rtol * fabsf(y);
    const float q0 = y / scale, q1 = f0 / scale;
    const float q0b = d0 > 0.f ? (float)(c.d0b * (double)q0 / (a.n_el * d0)) : 0.f;
    const float q1b = d1 > 0.f ? (float)(c.d1b * (double)q1 / (a.n_el * d1)) : 0.f;
    const float sc = a.SCB[i] - q0b * q0 / scale - q1b * q1 / scale;
    const float sy = y > 0.f ? 1.f : (y < 0.f ? -1.f : 0.f);
    a.Y0[i] += q0b / scale + sc * a.rtol * sy;
    fbc += q1b / scale;
  }
  g0[i] = fbc;
}

// grad_y0 = y's adjoint + evaluation 0's d/dx + gsol[0] (solution[0] = y0)
__global__ __launch_bounds__(kWbT) void wb_gy0_kernel(WbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kWbT + threadIdx.x;
  if (i < a.n) a.gy0[i] = (a.Y0[i] + a.GX[i]) + a.gsol[i];
}

int64_t al256(int64_t v) { return (v + 255) & ~int64_t(255); }

// attempts per chunk: 6 A B rows near FETODE_WIDE_BWD_ROWS
int64_t wb_chunk_attempts(int64_t B, int64_t n_att) {
  // read per call (the workspace query and the sweep of one backward see the same value)
  const int64_t rows = std::max<int64_t>(env_int("FETODE_WIDE_BWD_ROWS", 8192), 1);
  const int64_t A = std::max<int64_t>(1, (rows + 3 * B) / (6 * B));
  return std::max<int64_t>(1, std::min(A, n_att));
}

struct WbLayout {
  int64_t ctl, part, planes, gk, gh, vjp, vjp_bytes, end;
  int64_t C;  // evaluations per chunk
};
bool wb_layout(const fetode_kanlinear_t* kan0, const fetode_ferro_t* fer0, const fetode_kanlinear_t* kan1,
               const fetode_ferro_t* fer1, int64_t B, int64_t n_att, WbLayout& l) {
  const int D = kan0->in_features, H = kan0->out_features;
  const int64_t n = B * D, nwg = (n + kWbT - 1) / kWbT;
  l.C = 6 * wb_chunk_attempts(B, n_att);
  // the VJPs run over B rows (d/dx), a whole chunk's and the earliest (shorter) chunk's
  const int64_t A = l.C / 6, rem = n_att % A;
  const int64_t rows[3] = {B, l.C * B, (rem ? 6 * rem : l.C) * B};
  int64_t v = 0;
  const fetode_kanlinear_t* ks[2] = {kan0, kan1};
  const fetode_ferro_t* fs[2] = {fer0, fer1};
  for (int q = 0; q < 2; ++q)
    for (int r = 0; r < 3; ++r) {
      const int64_t f = fetode_ferro_backward_wide_workspace(fs[q], rows[r]);
      if (f < 0) return false;
      int64_t k = fetode_kanlinear_backward_wide_workspace(ks[q], fs[q], rows[r]);
      if (k < 0) k = fetode_kanlinear_backward_workspace(ks[q]);  // other output widths: the generic VJP
      if (k < 0) return false;
      v = std::max({v, f, k});
    }
  l.ctl = 0;
  l.part = al256((int64_t)sizeof(WbCtl));
  l.planes = al256(l.part + (int64_t)sizeof(double) * 2 * kWbSlots * nwg);
  l.gk = al256(l.planes + (int64_t)sizeof(float) * 6 * n);
  l.gh = al256(l.gk + (int64_t)sizeof(float) * l.C * n);
  l.vjp = al256(l.gh + (int64_t)sizeof(float) * l.C * B * H);
  l.vjp_bytes = v;
  l.end = al256(l.vjp + v + 256);
  return true;
}

bool wb_shape_ok(const fetode_kanlinear_t* kan0, const fetode_ferro_t* fer0, const fetode_kanlinear_t* kan1,
                 const fetode_ferro_t* fer1) {
  if (!kan0 || !fer0 || !kan1 || !fer1) return false;
  if (!fetode_wide_layer_supported(kan0, fer0) || !fetode_wide_layer_supported(kan1, fer1)) return false;
  return kan1->in_features == kan0->out_features && kan1->out_features == kan0->in_features;
}

}  // namespace

extern "C" {

int64_t fetode_wide_dopri5_backward_workspace(const fetode_kanlinear_t* kan0, const fetode_ferro_t* fer0,
                                              const fetode_kanlinear_t* kan1, const fetode_ferro_t* fer1, int64_t B,
                                              int32_t n_att) {
  if (!wb_shape_ok(kan0, fer0, kan1, fer1) || B <= 0 || n_att < 0) return -1;
  WbLayout l;
  if (!wb_layout(kan0, fer0, kan1, fer1, B, n_att, l)) return -1;
  return l.end;
}

int fetode_wide_dopri5_backward(const fetode_kanlinear_t* kan0, const fetode_ferro_t* fer0, const void* plan0,
                                const fetode_kanlinear_t* kan1, const fetode_ferro_t* fer1, const void* plan1,
                                int64_t B, const float* prev0, const float* prev1, uint32_t reinit_mask,
                                const double* t, int32_t T, double rtol, double atol, const double* opts,
                                const float* tableau, const float* grad_solution, const float* tape, int64_t tape_cap,
                                int32_t n_ev, const double* attempts, int32_t n_att, const double* init_rec,
                                float* grad_y0, const fetode_kanlinear_grad_t* kan_grad0,
                                const fetode_ferro_grad_t* ferro_grad0, const fetode_kanlinear_grad_t* kan_grad1,
                                const fetode_ferro_grad_t* ferro_grad1, void* workspace, void* stream) {
  if (!wb_shape_ok(kan0, fer0, kan1, fer1))
    return set_err(FETODE_EUNSUPPORTED, "wide dopri5 backward: needs two wide KAN-FET layers D -> H -> D");
  if (B <= 0 || T <= 0) return FETODE_OK;
  if (!plan0 || !plan1 || !t || !opts || !tableau || !grad_solution || !tape || !attempts || !init_rec || !workspace)
    return set_err(FETODE_EINVAL, "wide dopri5 backward: null pointer");
  const int re0 = (reinit_mask & 1u) ? 1 : 0, re1 = (reinit_mask & 2u) ? 1 : 0;
  if ((!re0 && !prev0) || (!re1 && !prev1)) return set_err(FETODE_EINVAL, "wide dopri5 backward: null hysteresis state");
  const int base = dopri_base(opts);
  if (n_att < 0 || (int64_t)n_ev != (int64_t)base + 6 * (int64_t)n_att)
    return set_err(FETODE_EINVAL, "wide dopri5 backward: %d evaluations do not match %d attempts (expected %lld)", n_ev,
                   n_att, (long long)base + 6 * (long long)n_att);
  if ((int64_t)n_ev > tape_cap) return set_err(FETODE_EINVAL, "wide dopri5 backward: the tape holds %lld of %d evaluations",
                                                (long long)tape_cap, n_ev);
  const int D = kan0->in_features, H = kan0->out_features;
  const int64_t n = B * D, nh = B * H;
  WbLayout wl;
  if (!wb_layout(kan0, fer0, kan1, fer1, B, n_att, wl))
    return set_err(FETODE_EUNSUPPORTED, "wide dopri5 backward: a layer has no VJP kernel");
  if ((n + kWbT - 1) / kWbT > 0x7fffffff) return set_err(FETODE_EINVAL, "wide dopri5 backward: batch too large");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const float* tx = tape;
  const float* th = tape + tape_cap * n;
  const float* tk = th + tape_cap * nh;
  WbArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.rtol = (float)rtol;
  a.atol = (float)atol;
  a.n_el = (double)n;
  memcpy(&a.tab, tableau, sizeof(DopriTab));
  dopri_step_from_opts(opts, a.step);
  a.t = t;
  a.T = T;
  a.gsol = grad_solution;
  a.tx = tx;
  a.tk = tk;
  a.att = attempts;
  a.n_att = n_att;
  a.base = base;
  a.init_rec = init_rec;
  a.ctl = (WbCtl*)(ws + wl.ctl);
  a.part = (double*)(ws + wl.part);
  a.nwg = (int)((n + kWbT - 1) / kWbT);
  float* pl = (float*)(ws + wl.planes);
  a.Y0 = pl;
  a.Y1 = pl + n;
  a.F = pl + 2 * n;
  a.GX = pl + 3 * n;
  a.SCB = pl + 4 * n;
  a.F0BP = pl + 5 * n;
  a.gy0 = grad_y0;
  float* gk = (float*)(ws + wl.gk);
  float* gh = (float*)(ws + wl.gh);
  void* vws = ws + wl.vjp;
  // control words, partials and the adjoint planes start at zero
  HIP_CHECK_RET(hipMemsetAsync(workspace, 0, (size_t)wl.gk, s));
  const dim3 eg((unsigned)a.nwg), et(kWbT);
  const bool kw0 = fetode_kanlinear_backward_wide_workspace(kan0, fer0, B) >= 0;
  const bool kw1 = fetode_kanlinear_backward_wide_workspace(kan1, fer1, B) >= 0;

  // one layer's VJP over `rows` stacked rows: d/dx (gx, written) and / or the parameter sums
  auto layer_vjp = [&](int l, const float* x, const float* prev, int reinit, int64_t rows, const float* g, float* gx,
                       const fetode_kanlinear_grad_t* kg, const fetode_ferro_grad_t* fg, int accumulate) -> int {
    const fetode_kanlinear_t* kan = l ? kan1 : kan0;
    const fetode_ferro_t* fer = l ? fer1 : fer0;
    const void* plan = l ? plan1 : plan0;
    int rc = FETODE_OK;
    if (gx || fg)
      rc = fetode_ferro_backward_wide(fer, plan, x, rows, reinit ? nullptr : prev, reinit, g, gx, fg, gx ? 0 : accumulate,
                                      vws, stream);
    if (rc) return rc;
    if (!gx && !kg) return FETODE_OK;
    // d/dx: the Ferro part wrote gx, the KAN part adds to it; parameter sums: `accumulate`
    if (gx && kg) return set_err(FETODE_EINVAL, "wide dopri5 backward: d/dx and parameter passes are separate calls");
    if (l ? kw1 : kw0) return fetode_kanlinear_backward_wide(kan, fer, plan, x, rows, g, gx, kg, gx ? 1 : accumulate, vws, stream);
    return fetode_kanlinear_backward(kan, x, rows, g, gx, kg, vws, gx ? 1 : accumulate, stream);
  };
  // evaluation e's d/dx: g (B, D) -> ghp (B, H) -> GX (B, D)
  auto eval_vjp = [&](int64_t e, const float* g, float* ghp) -> int {
    const int first = e == 0;
    int rc = layer_vjp(1, th + e * nh, first ? prev1 : th + (e - 1) * nh, first ? re1 : 0, B, g, ghp, nullptr, nullptr, 0);
    if (rc) return rc;
    return layer_vjp(0, tx + e * n, first ? prev0 : tx + (e - 1) * n, first ? re0 : 0, B, ghp, a.GX, nullptr, nullptr, 0);
  };
  // the parameter sums of evaluations [e, e + ne): stacked rows, the memory one evaluation back
  int accumulate = 0;
  const bool want1 = kan_grad1 || ferro_grad1, want0 = kan_grad0 || ferro_grad0;
  auto param_pass = [&](int64_t e, int64_t ne, const float* g, const float* ghp) -> int {
    const int first = e == 0;
    int rc = FETODE_OK;
    if (want1)
      rc = layer_vjp(1, th + e * nh, first ? prev1 : th + (e - 1) * nh, first ? re1 : 0, ne * B, g, nullptr, kan_grad1,
                     ferro_grad1, accumulate);
    if (!rc && want0)
      rc = layer_vjp(0, tx + e * n, first ? prev0 : tx + (e - 1) * n, first ? re0 : 0, ne * B, ghp, nullptr, kan_grad0,
                     ferro_grad0, accumulate);
    accumulate = 1;
    return rc;
  };

  const int64_t A = wl.C / 6;
  int rc;
  for (int64_t hi = n_att; hi > 0; hi -= A) {  // chunks of A attempts, counted from the last
    const int64_t lo = std::max<int64_t>(0, hi - A);
    const int64_t e_lo = base + 6 * lo;
    for (int64_t na = hi - 1; na >= lo; --na) {
      const int e2 = (int)(base + 6 * na);
      float* kb = gk + (e2 - e_lo) * n;
      hipLaunchKernelGGL(wb_ctl_kernel, dim3(1), et, 0, s, a, (int)na);
      LAUNCH_CHECK();
      hipLaunchKernelGGL(wb_head_kernel, eg, et, 0, s, a, e2, kb);
      LAUNCH_CHECK();
      for (int st = 7; st >= 2; --st) {
        const int64_t e = e2 + st - 2;
        if ((rc = eval_vjp(e, gk + (e - e_lo) * n, gh + (e - e_lo) * nh))) return rc;
        hipLaunchKernelGGL(wb_stage_kernel, eg, et, 0, s, a, st, e2, kb);
        LAUNCH_CHECK();
      }
    }
    if ((rc = param_pass(e_lo, 6 * (hi - lo), gk, gh))) return rc;
  }
  // the initial step: attempt 0's partials -> dt_0's adjoint, the probe, f(y0)
  hipLaunchKernelGGL(wb_ctl_kernel, dim3(1), et, 0, s, a, -1);
  LAUNCH_CHECK();
  if (base == 2) {
    hipLaunchKernelGGL(wb_probe_head_kernel, eg, et, 0, s, a, gk);
    LAUNCH_CHECK();
    if ((rc = eval_vjp(1, gk, gh))) return rc;
    hipLaunchKernelGGL(wb_probe_tail_kernel, eg, et, 0, s, a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(wb_init_ctl_kernel, dim3(1), et, 0, s, a);
    LAUNCH_CHECK();
    if ((rc = param_pass(1, 1, gk, gh))) return rc;
  }
  hipLaunchKernelGGL(wb_f0_head_kernel, eg, et, 0, s, a, gk);
  LAUNCH_CHECK();
  if ((rc = eval_vjp(0, gk, gh))) return rc;
  if ((rc = param_pass(0, 1, gk, gh))) return rc;
  if (grad_y0) {
    hipLaunchKernelGGL(wb_gy0_kernel, eg, et, 0, s, a);
    LAUNCH_CHECK();
  }
  return FETODE_OK;
}

}  // extern "C"
