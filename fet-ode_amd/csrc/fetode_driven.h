// fetode_driven.h — the input-driven Ferro field of the ECG NODE-RNN encoder
// (compare_noise_ecg.py:875-907):   dh/dt = tanh(Ferro_{(H+D)->H}(cat[h, x(t)])) * gain + bias.
// Plan layout, launch arguments and the host's dispatch helpers shared by the driven kernel files
// (the device arithmetic: fetode_driven_dev.h).
#pragma once
#include <stdint.h>

#include "fetode_common.h"

namespace fetode {

// admitted family (fetode_driven_supported): D = in_dim - out_dim
constexpr int kDrvHMax = 64;    // one lane per output
constexpr int kDrvDMax = 4;
constexpr int kDrvKMax = 16;
constexpr int kDrvInMax = kDrvHMax + kDrvDMax;
constexpr int kDrvThreads = 256;  // four waves: lane -> output o, wave -> inputs i = wave (mod 4)

// evaluations per step of the four fixed-grid methods as a shift (1, 2, 4, 4); -1: not a fixed-grid method
constexpr int drv_nm_log2(int method) { return method == 0 ? 0 : method == 1 ? 1 : (method == 2 || method == 3) ? 2 : -1; }

// Plan (floats): In*K*H elements of 4 constants, element (i, k, o) at ((i*K + k)*H + o)*4 so that
// the 64 lanes of a wave (o) read consecutive 16-byte words:
//   .x  gate_slope*log2e*Ec     .y  2*log2e*k     .z  2*log2e*k*Ec     .w  coef*Ps
// then fconst[H] = sum_i (sum_k bias*coef), gain[H], bias[H].
constexpr int64_t drv_plan_elems(int In, int H, int K) { return (int64_t)In * K * H; }
constexpr int64_t drv_plan_floats(int In, int H, int K) { return 4 * drv_plan_elems(In, H, K) + 3 * (int64_t)H; }

struct DrivenArgs {
  const float* plan;
  const float* h0;       // (B, H)
  const float* u;        // (n_eval, B, D) driving table
  const float* dt;       // (n_steps) fp32 step sizes of the steps this launch takes; the GRID kernels:
                         // (n_steps, 4) rows of dt, fp32(dt / 2), fp32(dt / 6), 0 (Schedule.step_coef)
  const float* prev0;    // (B, H+D) hysteresis input before the first evaluation, null: zeros
  float* sol;            // (n_steps, B, H) the state after every step
  float* prev_out;       // (B, H+D) nullable: the last evaluation's input
  float* tape_hx;        // (n_eval, B, H+D) taped kernels only
  float* tape_phi;       // (n_eval, B, H)
  int64_t B;
  int64_t eval0;         // first evaluation (row of u / the tape) of this launch
  int32_t H, D, K, n_steps;
  float gs, gsl2e, wc;   // gate_slope, gate_slope*log2e, -2(1-alpha)
  int32_t method, nm_log2;   // the GRID kernels only: FETODE_EULER.., log2 of the evaluations per step
};

struct DrivenAdjArgs {
  const float* plan;
  const float* dt;        // (n_steps); the GRID kernels: (n_steps, 4) as in DrivenArgs
  const float* prev0;     // (B, H+D) nullable
  const float* tape_hx;   // (4 n_steps, B, H+D); the GRID kernels: n_m n_steps rows here and below
  const float* tape_phi;  // (4 n_steps, B, H)
  const float* grad_sol;  // (n_steps + 1, B, H): d loss / d every trajectory row, row 0 = h0
  float* adj;             // (4 n_steps, B, H): d loss / d every evaluation's output
  float* grad_h0;         // (B, H)
  float* adj_u;           // (4 n_steps, B, D): d loss / d every evaluation's x(t); the XG kernels only
  int64_t B;
  int32_t H, D, K, n_steps;
  float gs, gsl2e, wc;
  int32_t method, nm_log2;   // the GRID kernels only
};

// The field constants every driven argument struct carries (H, D, K, gs, gsl2e, wc), from the basis.
template <class Args>
inline void drv_fill_field(Args& a, const fetode_ferro_t* fl) {
  a.H = fl->out_dim;
  a.D = fl->in_dim - fl->out_dim;
  a.K = fl->num_basis;
  a.gs = (float)fl->gate_slope;
  a.gsl2e = (float)fl->gate_slope * FETODE_LOG2E;
  a.wc = (float)(-2.0 * (1.0 - fl->alpha));
}

// Dispatch (the named tables of DESIGN §4.16): a row holds a kernel's three K instantiations, K = 10 and
// K = 12 at compile time and the run-time K; rows per samples-per-workgroup S = 1, 2, 4 make a DrvSRows.
// A new driven kernel builds its row(s) where it is defined and launches through drv_launch.
template <class... A>
struct DrvKRow {
  void (*k10)(A...);
  void (*k12)(A...);
  void (*kany)(A...);
};
template <class... A>
struct DrvSRows {
  DrvKRow<A...> s1, s2, s4;
  const DrvKRow<A...>& at(int spw) const { return spw == 1 ? s1 : (spw == 2 ? s2 : s4); }
};
template <class... A>
inline void drv_launch(const DrvKRow<A...>& r, int K, dim3 grid, int threads, hipStream_t st, const A&... a) {
  hipLaunchKernelGGL(K == 10 ? r.k10 : (K == 12 ? r.k12 : r.kany), grid, dim3(threads), 0, st, a...);
}

}  // namespace fetode
