// fetode_dopri_ctl.h — the dopri5 step control of every device-resident solver and of their
// reverse sweeps, stated once: torchdiffeq's misc._select_initial_step, rk_common.
// _optimal_step_size, interp._interp_fit / _interp_evaluate and the attempt log, in the op order
// of the host-driven loop (fet-ode_amd/dopri5.py _Dopri5 with fetode_scaled_rms / fetode_interp_*).
// Plain functions of scalars: how the sums are formed, who writes, the stage loop and each
// driver's control flow stay in the kernels.  Built with -ffp-contract=off; the expression trees
// below ARE the contract (a resident solve agrees with the host loop and the oracle through them),
// so a change here is a change of every solver at once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fetode {

// options["first_step" .. "max_step"] as the kernels take them (first_step <= 0: select it)
struct DopriStep {
  double first_step, safety, ifactor, dfactor, min_step, max_step;
};

// opts = {first_step, safety, ifactor, dfactor, min_step, max_step, max_num_steps} (dopri5.py
// _opts_array); returns max_num_steps as the int the kernels count to (2^31 - 1 and inf included)
inline int dopri_step_from_opts(const double* opts, DopriStep& s) {
  s = DopriStep{opts[0], opts[1], opts[2], opts[3], opts[4], opts[5]};
  return opts[6] > 2e9 ? 2000000000 : (int)opts[6];
}
// evaluation index of attempt 0's stage 2 on the tape: 0 = f(y0), 1 = the initial-step probe
// (absent with first_step)
inline int dopri_base(const double* opts) { return opts[0] > 0.0 ? 1 : 2; }

// ---- misc._select_initial_step in fp32 (dopri5.py select_initial_step) ----
// s0, s1: the sums of (y0 / scale)^2 and (f0 / scale)^2 over the n_el elements
__device__ __forceinline__ float dopri_h0(double s0, double s1, double n_el, float& d0, float& d1) {
  d0 = fabsf(sqrtf((float)(s0 / n_el)));
  d1 = fabsf(sqrtf((float)(s1 / n_el)));
  const float h0 = (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : (0.01f * d0) / d1;
  return fabsf(h0);
}
// s2: the sum of ((f(y0 + h0 f0) - f0) / scale)^2.  The fp64 pow is rounded once to fp32, so host
// and device agree
__device__ __forceinline__ double dopri_dt0(double s2, double n_el, float h0, float d1, float& d2, float& h1) {
  const float d2v = fabsf(sqrtf((float)(s2 / n_el)) / h0);
  float h1v;
  if (d1 <= 1e-15f && d2v <= 1e-15f) h1v = fmaxf(1e-6f, h0 * 1e-3f);
  else h1v = (float)pow((double)(0.01f / fmaxf(d1, d2v)), (double)0.2f);
  d2 = d2v;
  h1 = h1v;
  return (double)fminf(100.0f * h0, fabsf(h1v));
}
// the scalars the reverse sweep differentiates dt0 through
__device__ __forceinline__ void dopri_init_record(double* init_rec, float d0, float d1, float d2, float h0, float h1) {
  init_rec[0] = d0;
  init_rec[1] = d1;
  init_rec[2] = d2;
  init_rec[3] = h0;
  init_rec[4] = h1;
}

// ---- one attempt ----
// the step is too small to advance t0 (status 2)
__device__ __forceinline__ bool dopri_underflow(double t0, double dt) { return !(t0 + dt > t0); }
// s: the sum of (err / tol)^2
__device__ __forceinline__ float dopri_ratio(double s, double n_el) { return sqrtf((float)(s / n_el)); }
__device__ __forceinline__ bool dopri_accept(float ratio) { return ratio <= 1.0f; }
// the attempt log (max_att, 4): t0, dt, error ratio, accepted.  One thread of the grid calls this
__device__ __forceinline__ void dopri_log_attempt(double* att, int n_att, int max_att, double t0, double dt,
                                                  float ratio, bool accept) {
  if (n_att < max_att) {
    double* o = att + (int64_t)n_att * 4;
    o[0] = t0;
    o[1] = dt;
    o[2] = (double)ratio;
    o[3] = accept ? 1.0 : 0.0;
  }
}
// rk_common._optimal_step_size in fp64 (dopri5.py optimal_step), then the min / max step clamp
__device__ __forceinline__ double dopri_next_dt(double dt, float ratio, const DopriStep& p) {
  const double rr = (double)ratio;
  double nxt;
  if (rr == 0.0) {
    nxt = dt * p.ifactor;
  } else {
    const double dfac = rr < 1.0 ? 1.0 : p.dfactor;
    const double factor = __builtin_isnan(rr) ? rr : fmin(p.ifactor, fmax(p.safety / pow(rr, 1.0 / 5.0), dfac));
    nxt = dt * factor;
  }
  return __builtin_isnan(nxt) ? nxt : fmin(fmax(nxt, p.min_step), p.max_step);
}

// ---- dense output: interp._interp_fit / _interp_evaluate (fetode_interp_fit's op order) ----
// T: float, or a vector of floats (one state dim per component); mid is the step's c_mid sum
template <class T>
__device__ __forceinline__ void dopri_fit(T co[5], T y, T y1, T mid, T f0, T k7, float dt32) {
  const T ym = y + mid, fa = f0, fb6 = k7;
  co[4] = ((2.0f * dt32) * (fb6 - fa) - 8.0f * (y1 + y)) + 16.0f * ym;
  co[3] = ((dt32 * (5.0f * fa - 3.0f * fb6) + 18.0f * y) + 14.0f * y1) - 32.0f * ym;
  co[2] = ((dt32 * (fb6 - 4.0f * fa) - 11.0f * y) - 5.0f * y1) + 16.0f * ym;
  co[1] = dt32 * fa;
  co[0] = y;
}
// xq = (t - t0) / (t1 - t0) of the accepted step
template <class T>
__device__ __forceinline__ T dopri_eval(const T co[5], float xq) {
  T total = co[0] + xq * co[1];
  float xp = xq;
#pragma unroll
  for (int j = 2; j < 5; ++j) {
    xp = xp * xq;
    total = total + xp * co[j];
  }
  return total;
}

// ---- the reverse sweeps' adjoint of the control chain ----
// dt_{n+1} = clamp(dt * min(ifactor, max(safety ratio^-1/5, dfac))).  The factor the forward took
// is dt_{n+1} / dt_n from the attempt log (dtn1: the next attempt's dt), so no pow here: the middle
// term was taken unless the factor sits on a bound (or the clamp did), and its derivative is
// -factor / (5 ratio).  dtbar: the adjoint of dt_{n+1}; added to what the caller zeroed: dtbb, its part
// for dt_n, and rbar, the error ratio's adjoint.  The last attempt's next dt feeds nothing (no call)
// (the options by reference: a sweep that keeps them in LDS reads each where the rule needs it)
__device__ __forceinline__ void dopri_next_dt_adjoint(double dtbar, double dt, double dtn1, double rr,
                                                      const double& ifactor, const double& dfactor,
                                                      const double& min_step, const double& max_step, double& dtbb,
                                                      double& rbar) {
  const bool clamped = (min_step > 0.0 && dtn1 == min_step) || dtn1 == max_step;
  if (!clamped) {
    const double fac = dtn1 / dt;
    dtbb = dtbar * fac;
    if (rr > 0.0) {
      const double dfac = rr < 1.0 ? 1.0 : dfactor;
      const bool bound = fabs(fac - ifactor) <= 1e-12 * ifactor || fabs(fac - dfac) <= 1e-12 * dfac;
      if (!bound) rbar = dtbar * dt * (-0.2 * fac / rr);
    }
  }
}
// dt0 = min(100 h0, |h1|) back to h0 (h0b), d1 (d1b) and r2 = d2 h0 = rms((f1 - f0) / scale)
// (r2b), from the init_rec scalars; dtb: dt0's adjoint.  Ties split evenly; Python's max keeps d1
__device__ __forceinline__ void dopri_dt0_adjoint(double dtb, float d1, float d2, float h0, float h1, double& h0b,
                                                  double& d1b, double& r2, double& r2b) {
  double h1b = 0.0;
  h0b = 0.0;
  const float a100 = 100.0f * h0, ah1 = fabsf(h1), sh1 = h1 < 0.f ? -1.f : 1.f;
  if (a100 < ah1) h0b = 100.0 * dtb;
  else if (ah1 < a100) h1b = dtb * sh1;
  else {
    h0b = 50.0 * dtb;
    h1b = 0.5 * dtb * sh1;
  }
  double d2b = 0.0;
  d1b = 0.0;
  if (d1 <= 1e-15f && d2 <= 1e-15f) {  // h1 = max(1e-6, h0 1e-3)
    const float v = h0 * 1e-3f;
    if (v > 1e-6f) h0b += 1e-3 * h1b;
    else if (v == 1e-6f) h0b += 0.5e-3 * h1b;
  } else {  // h1 = (0.01 / max(d1, d2)) ** (1/5)
    const bool take2 = d2 > d1;
    const double mx = take2 ? d2 : d1, base = 0.01 / mx;
    const double mxb = -(h1b * 0.2 * (double)h1 / base) * base / mx;
    if (take2) d2b += mxb;
    else d1b += mxb;
  }
  // d2 = |r2 / h0|
  r2 = (double)d2 * h0;
  r2b = d2b / h0;
  h0b = h0b - d2b * d2 / h0;
}
// h0 = |0.01 d0 / d1| (unless either is below 1e-5) back to d0 and d1; h0b has taken the probe's
// sum of xb f0
__device__ __forceinline__ void dopri_h0_adjoint(double h0b, float h0, float d0, float d1, double& d0b, double& d1b) {
  if (!(d0 < 1e-5f || d1 < 1e-5f)) {
    d0b = h0b * 0.01 / d1;
    d1b = d1b - h0b * (double)h0 / d1;
  }
}

}  // namespace fetode
