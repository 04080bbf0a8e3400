// fetode_driven_dopri5.hip — the input-driven Ferro field of the ECG NODE-RNN encoder under
// torchdiffeq's dopri5, the whole batch in one launch with ONE STEP CONTROLLER PER SAMPLE
// (compare_noise_ecg.py:2164-2180: train_rnn_node(..., batch_size=1, solver="dopri5")):
//     dh/dt = tanh(Ferro_{(H+D)->H}(cat[h, x(t)])) * gain + bias
// The reference solves one sample at a time, so every sample has its own error norm over its own H
// elements, its own step sequence and its own attempt log; a workgroup owns a sample from h0 to the
// end and runs that sample's control loop, so no workgroup waits on another one (no grid barrier, no
// exchange, no co-residency limit).  The field is not autonomous: the stage times decide x(t), which
// the kernel interpolates from the sample's own (T, D) series at every evaluation time.
//   evaluation   fetode_driven_dev.h's gate, element loop and meeting (the functions driven_fixed_kernel
//                calls) at one sample per workgroup: the plan of
//                fetode_driven_plan_build, lane -> output o, wave w -> inputs i = w (mod 4), the gate
//                against the previous evaluation's input (prev <- hx in call order, rejected and probe
//                evaluations included), the fixed-order meeting of the four partial sums in LDS
//   control      fetode_dopri_ctl.h in the call order of dopri5.py _Dopri5.integrate; wave 0 holds the
//                state (one lane per element) and decides; the other waves learn through LDS, ahead of a
//                barrier every thread reaches, whether another phase follows
//   tape         the training path's instantiation records every evaluation for the reverse sweep of
//                fetode_driven_dopri5_bwd.hip; the kernel body lives in fetode_driven_dopri5_body.h and
//                is included once per kernel signature, the tape's statements as preprocessor blocks
#include <string.h>

#include "fetode_dopri_ctl.h"
#include "fetode_driven_dev.h"

using namespace fetode;

namespace {

struct DrivenDopriArgs {
  const float* plan;
  const float* h0;      // (B, H)
  const float* x;       // (B, T, D) driving series
  const float* tg;      // (T) fp32 grid: the interpolator's knots and the output times
  const float* prev0;   // (B, H+D) hysteresis input before the first evaluation, null: zeros
  float* sol;           // (T, B, H), row 0 = h0
  float* prev_out;      // (B, H+D) nullable: the last evaluation's input
  int32_t* stats;       // (B, 3) nfev, attempts, status
  double* att;          // (B, max_att, 4) attempt log
  float* evlog;         // (B, max_ev, 1+D) EVLOG kernels only: every evaluation's time and x(t)
  int32_t H, D, K, T, max_att, max_ev, max_steps;
  float gs, gsl2e, wc;  // gate_slope, gate_slope*log2e, -2(1-alpha)
  float rtol, atol;
  DopriStep step;
  float beta[6][6], cerr[7], cmid[7];  // torchdiffeq's tableau rounded to fp32 (dopri5.py _TABLEAU)
  float alpha[6];
};

// the training tape of a sample's solve (TAPE kernels only), rows in call order: f0, the probe, then six
// evaluations per attempt, rejected ones included; rows at or beyond the sample's nfev are zeroed
struct DrivenDopriTape {
  float* hx;         // (B, max_ev, H+D) every evaluation's input row
  float* phi;        // (B, max_ev, H) its pre-activation
  float* tq;         // (B, max_ev) its time
  float* slope;      // (B, max_ev, D) d x(t) / dt of the interval used, 0 where the clamp cut the query
  double* init_rec;  // (B, 5) d0, d1, d2, h0, h1 of the initial-step selection (zeros with first_step)
  int32_t max_ev;
};

// phases of a sample's solve; every thread follows them, wave 0 announces through s_nq how many
// evaluations the next one has (0: the solve is over)
enum { kPhaseF0 = 0, kPhaseProbe = 1, kPhaseAttempt = 2 };

template <int KT, bool EVLOG>
__global__ __launch_bounds__(kDrvThreads) void driven_dopri5_kernel(DrivenDopriArgs a) {
#include "fetode_driven_dopri5_body.h"
}

// the taped solve of the training path: the same body, the tape in a second argument so that the
// untaped kernels keep their argument block
template <int KT>
__global__ __launch_bounds__(kDrvThreads) void driven_dopri5_tape_kernel(DrivenDopriArgs a, DrivenDopriTape tp) {
  constexpr bool EVLOG = false;
#define FETODE_DRIVEN_TAPE
#include "fetode_driven_dopri5_body.h"
#undef FETODE_DRIVEN_TAPE
}

// the kernel tables (fetode_driven.h): [EVLOG] and the taped row
const DrvKRow<DrivenDopriArgs> kDopri5[2] = {
    {driven_dopri5_kernel<10, false>, driven_dopri5_kernel<12, false>, driven_dopri5_kernel<0, false>},
    {driven_dopri5_kernel<10, true>, driven_dopri5_kernel<12, true>, driven_dopri5_kernel<0, true>}};
const DrvKRow<DrivenDopriArgs, DrivenDopriTape> kDopri5Tape = {
    driven_dopri5_tape_kernel<10>, driven_dopri5_tape_kernel<12>, driven_dopri5_tape_kernel<0>};

// steps counted per output interval beyond which only the geometric shrink of a rejected step bounds
// the loop (DESIGN §4.18 "Termination")
constexpr int kDrvBoundedSteps = 1 << 20;

// what the untaped and the taped entry share: the checks, the argument block and the launch
int driven_dopri5(const fetode_ferro_t* basis, const void* plan, const float* h0, int64_t B, const float* x,
                  const float* t_grid, int32_t T, double rtol, double atol, const double* opts, const float* tableau,
                  const float* prev0, float* sol, float* prev_out, int32_t* stats, double* attempts,
                  int32_t max_attempts, float* evlog, int32_t max_ev, const DrivenDopriTape* tape, void* stream) {
  if (!fetode_driven_supported(basis)) return set_err(FETODE_EUNSUPPORTED, "driven: shape outside the admitted family");
  if (B < 0 || T < 2 || max_attempts < 0 || max_ev < 0)
    return set_err(FETODE_EINVAL, "driven dopri5: bad sizes (B=%lld, T=%d, max_attempts=%d, max_ev=%d)", (long long)B, T,
                   max_attempts, max_ev);
  if (B == 0) return FETODE_OK;
  if (!plan || !h0 || !x || !t_grid || !opts || !tableau || !sol || !stats || (max_attempts > 0 && !attempts))
    return set_err(FETODE_EINVAL, "driven dopri5: null pointer");
  if (tape && (!tape->hx || !tape->phi || !tape->tq || !tape->slope || !tape->init_rec || !attempts))
    return set_err(FETODE_EINVAL, "driven dopri5 tape: null pointer");
  if (B > 0x7fffffff) return set_err(FETODE_EUNSUPPORTED, "driven dopri5: batch too large");
  DrivenDopriArgs a{};
  a.max_steps = dopri_step_from_opts(opts, a.step);
  // a rejected step shrinks by max(safety, dfactor) at least, down to the underflow of dt; a floor on
  // dt or factors of 1 and more take that bound away, and then max_num_steps has to be one
  const bool shrinks = a.step.safety < 1.0 && a.step.dfactor < 1.0 && !(a.step.min_step > 0.0);
  if (!shrinks && a.max_steps > kDrvBoundedSteps)
    return set_err(FETODE_EUNSUPPORTED, "driven dopri5: min_step / safety / dfactor leave rejected steps unbounded; "
                                        "set max_num_steps <= %d", kDrvBoundedSteps);
  a.plan = (const float*)plan;
  a.h0 = h0; a.x = x; a.tg = t_grid; a.prev0 = prev0; a.sol = sol; a.prev_out = prev_out;
  a.stats = stats; a.att = attempts; a.evlog = evlog;
  drv_fill_field(a, basis);
  a.T = T;
  a.max_att = attempts ? max_attempts : 0;
  a.max_ev = evlog ? max_ev : 0;
  a.rtol = (float)rtol; a.atol = (float)atol;
  memcpy(a.beta, tableau, sizeof(a.beta));
  memcpy(a.cerr, tableau + 36, sizeof(a.cerr));
  memcpy(a.cmid, tableau + 43, sizeof(a.cmid));
  // torchdiffeq's alpha (dopri5.py _A) rounded to fp32 like the rest of the tableau
  const double alpha[6] = {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
  for (int i = 0; i < 6; ++i) a.alpha[i] = (float)alpha[i];
  const dim3 grid((unsigned)B);
  if (tape) drv_launch(kDopri5Tape, a.K, grid, kDrvThreads, (hipStream_t)stream, a, *tape);
  else drv_launch(kDopri5[evlog != nullptr], a.K, grid, kDrvThreads, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return FETODE_OK;
}

}  // namespace

extern "C" {

int fetode_driven_dopri5(const fetode_ferro_t* basis, const void* plan, const float* h0, int64_t B, const float* x,
                         const float* t_grid, int32_t T, double rtol, double atol, const double* opts,
                         const float* tableau, const float* prev0, float* sol, float* prev_out, int32_t* stats,
                         double* attempts, int32_t max_attempts, float* evlog, int32_t max_ev, void* stream) {
  return driven_dopri5(basis, plan, h0, B, x, t_grid, T, rtol, atol, opts, tableau, prev0, sol, prev_out, stats,
                       attempts, max_attempts, evlog, max_ev, nullptr, stream);
}

int fetode_driven_dopri5_tape(const fetode_ferro_t* basis, const void* plan, const float* h0, int64_t B, const float* x,
                              const float* t_grid, int32_t T, double rtol, double atol, const double* opts,
                              const float* tableau, const float* prev0, float* sol, float* prev_out, int32_t* stats,
                              double* attempts, int32_t max_attempts, float* tape_hx, float* tape_phi, float* tape_t,
                              float* tape_slope, double* init_rec, int32_t max_ev, void* stream) {
  if (max_ev < 1) return set_err(FETODE_EINVAL, "driven dopri5 tape: max_ev=%d", max_ev);
  const DrivenDopriTape tp{tape_hx, tape_phi, tape_t, tape_slope, init_rec, max_ev};
  return driven_dopri5(basis, plan, h0, B, x, t_grid, T, rtol, atol, opts, tableau, prev0, sol, prev_out, stats,
                       attempts, max_attempts, nullptr, 0, &tp, stream);
}

}  // extern "C"
