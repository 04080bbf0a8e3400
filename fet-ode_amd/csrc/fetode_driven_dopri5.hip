// fetode_driven_dopri5.hip — the input-driven Ferro field of the ECG NODE-RNN encoder under
// torchdiffeq's dopri5, the whole batch in one launch with ONE STEP CONTROLLER PER SAMPLE
// (compare_noise_ecg.py:2164-2180: train_rnn_node(..., batch_size=1, solver="dopri5")):
//     dh/dt = tanh(Ferro_{(H+D)->H}(cat[h, x(t)])) * gain + bias
// The reference solves one sample at a time, so every sample has its own error norm over its own H
// elements, its own step sequence and its own attempt log; a workgroup owns a sample from h0 to the
// end and runs that sample's control loop, so no workgroup waits on another one (no grid barrier, no
// exchange, no co-residency limit).  The field is not autonomous: the stage times decide x(t), which
// the kernel interpolates from the sample's own (T, D) series at every evaluation time.
//   evaluation   driven_fixed_kernel's arithmetic at one sample per workgroup: the plan of
//                fetode_driven_plan_build, lane -> output o, wave w -> inputs i = w (mod 4), the gate
//                against the previous evaluation's input (prev <- hx in call order, rejected and probe
//                evaluations included), the fixed-order meeting of the four partial sums in LDS
//   control      fetode_dopri_ctl.h in the call order of dopri5.py _Dopri5.integrate; wave 0 holds the
//                state (one lane per element) and decides; the other waves learn through LDS, ahead of a
//                barrier every thread reaches, whether another phase follows
#include <string.h>

#include "fetode_common.h"
#include "fetode_dopri_ctl.h"
#include "fetode_driven.h"

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

// the butterfly gives every lane the same bits: each level adds the same two values on both sides
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// phases of a sample's solve; every thread follows them, wave 0 announces through s_nq how many
// evaluations the next one has (0: the solve is over)
enum { kPhaseF0 = 0, kPhaseProbe = 1, kPhaseAttempt = 2 };

template <int KT, bool EVLOG>
__global__ __launch_bounds__(kDrvThreads) void driven_dopri5_kernel(DrivenDopriArgs a) {
  __shared__ float xs[kDrvInMax], gxs[kDrvInMax], vs[kDrvInMax];
  __shared__ float part[4][64];
  __shared__ float s_beta[6][6], s_cerr[7], s_cmid[7], s_alpha[6];
  __shared__ float s_tq[6], us[6][kDrvDMax];  // the phase's evaluation times and x(t) at each
  __shared__ int s_nq;
  const int H = a.H, D = a.D, In = H + D, K = KT > 0 ? KT : a.K, T = a.T;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.x;  // grid = B
  const float4* __restrict__ el = reinterpret_cast<const float4*>(a.plan);
  const float* __restrict__ tail = a.plan + 4 * drv_plan_elems(In, H, K);
  const float* __restrict__ tg = a.tg;
  const float* __restrict__ xb = a.x + b * (int64_t)T * D;
  const bool w0 = wv == 0, own = w0 && lane < H;  // own: holds element `lane` of the state
  const int dd = tid - 64;
  const bool drv = dd >= 0 && dd < D;              // publishes driving input dd
  const float gs = a.gs, gsl2e = a.gsl2e, wc = a.wc;
  float fcon = 0.f, gain = 0.f, bias = 0.f;
  if (own) {
    fcon = tail[lane];
    gain = tail[H + lane];
    bias = tail[2 * H + lane];
  }
  // input i of the next evaluation: value, its gate against the previous evaluation's input
  // (prev <- hx, call order) and the per-input factors of the element loop
  auto publish = [&](int i, float xn, float xo) {
    const float up = 1.0f / (1.0f + expf(-(gs * (xn - xo))));
    xs[i] = xn;
    gxs[i] = gsl2e * xn;
    vs[i] = wc * (1.0f - up);
  };
  // LinearInterp1D (compare_noise_ecg.py:861-872) as driven_table_kernel states it; the left
  // searchsorted of an increasing grid by bisection (every index stays inside [0, T - 1])
  auto interp = [&](float t, int d) -> float {
    const float lo = tg[0], hi = tg[T - 1];
    t = t < lo ? lo : (t > hi ? hi : t);
    int l = 0, r = T;
    while (l < r) {
      const int m = (l + r) >> 1;
      if (tg[m] < t) l = m + 1;
      else r = m;
    }
    const int i = l < 1 ? 1 : (l > T - 1 ? T - 1 : l);
    const float t0 = tg[i - 1], t1 = tg[i];
    const float x0 = xb[(int64_t)(i - 1) * D + d], x1 = xb[(int64_t)i * D + d];
    const float w = (t - t0) / ((t1 - t0) + 1e-12f);
    return (1.0f - w) * x0 + w * x1;
  };
  int nfev = 0;
  // x(t) at the n evaluation times of the phase that starts (wave 1, one lane per time and input);
  // the first time's values are the next evaluation's driving inputs
  auto drive = [&](int n, bool first) {
    if (dd >= 0 && dd < n * D) {
      const int s = dd / D, d = dd - s * D;
      const float tq = s_tq[s];
      const float v = interp(tq, d);
      us[s][d] = v;
      if (EVLOG) {
        const int64_t e = (int64_t)nfev + s;
        if (e < a.max_ev) {
          float* o = a.evlog + (b * a.max_ev + e) * (1 + D);
          if (d == 0) o[0] = tq;
          o[1 + d] = v;
        }
      }
      if (s == 0) publish(H + d, v, first ? (a.prev0 ? a.prev0[b * In + H + d] : 0.f) : xs[H + d]);
    }
  };
  // one evaluation of the published input; wave 0 receives f (lanes >= H: 0)
  auto eval = [&]() -> float {
    __syncthreads();  // this evaluation's inputs are published
    float acc = 0.f;
    if (lane < H) {
      for (int i = wv; i < In; i += 4) {
        const float x = xs[i], gx = gxs[i], v = vs[i];
        float ai = 0.f;
        const float4* __restrict__ p = el + (int64_t)i * K * H + lane;
#pragma unroll KT > 0 ? KT : 1
        for (int k = 0; k < K; ++k) {
          const float4 c = p[(int64_t)k * H];
          const float cn = rcp(1.0f + ex2(gx + c.x));               // sigma(gs(-x - Ec))
          const float m = ffma(v, cn, 1.0f);
          const float z = ffma(c.z, m, c.y * x);                    // 2 log2e k (x + Ec m)
          const float th = ffma(rcp(1.0f + ex2(z)), -2.0f, 1.0f);   // tanh(k (x + Ec m))
          ai = ffma(c.w, th, ai);
        }
        acc += ai;
      }
    }
    part[wv][lane] = acc;
    __syncthreads();  // partial sums are in; nobody reads this evaluation's inputs any more
    ++nfev;
    float f = 0.f;
    if (w0) {
      const float phi = ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) + fcon;
      f = tanhf(phi) * gain + bias;
    }
    return f;
  };

  // ---- wave 0: the sample's solver state (one lane per element; the scalars agree on every lane) ----
  const double n_el = (double)H;
  const float rtol = a.rtol, atol = a.atol;
  float y = 0.f, f0 = 0.f, yi = 0.f, err = 0.f, mid = 0.f, dt32 = 0.f;
  float A[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float co[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  float h0p = 0.f, d1p = 0.f, scale = 1.f;  // the initial-step selection
  double dt = 0.0, t0 = 0.0, t1 = 0.0, t0s = 0.0, t1s = 0.0;
  int i_out = 1, n_steps = 0, n_att = 0, status = 0;

  // after f0, the probe and every attempt: the output rows the accepted step reaches, then the next
  // attempt's checks (the host loop's assertions, in its order), evaluation times and first input — or
  // the end.  Nothing is published at the end: xs keeps the last evaluation's input for prev_out
  auto begin_attempt = [&]() {
    int n = 6;
    while (i_out < T && !((double)tg[i_out] > t1s)) {
      const float total = dopri_eval(co, (float)(((double)tg[i_out] - t0s) / (t1s - t0s)));
      if (own) a.sol[((int64_t)i_out * gridDim.x + b) * H + lane] = total;
      ++i_out;
      n_steps = 0;
    }
    if (i_out >= T) n = 0;
    else if (n_steps >= a.max_steps) status = 3;
    else if (dopri_underflow(t1s, dt)) status = 2;
    else if (__ballot(own && !__builtin_isfinite(y)) != 0) status = 1;
    if (status) n = 0;
    if (n) {
      t0 = t1s;
      dt32 = (float)dt;
      t1 = t0 + dt;
      if (lane < 6) {
        const float al = s_alpha[lane];
        s_tq[lane] = al == 1.0f ? (float)t1 : (float)t0 + al * dt32;
      }
      // rk_common._runge_kutta_step in fetode_lincomb's op order, accumulated as the stages arrive:
      // A[i] is stage s+1+i's sum k0*b0 + k1*b1 + ... (the same left-to-right sums)
#pragma unroll
      for (int i = 0; i < 6; ++i) A[i] = f0 * (s_beta[i][0] * dt32);
      err = f0 * (s_cerr[0] * dt32);
      mid = f0 * (s_cmid[0] * dt32);
      yi = y + A[0];
      if (own) publish(lane, yi, xs[lane]);
    }
    if (lane == 0) s_nq = n;
  };

  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = 0; j < 6; ++j) s_beta[i][j] = a.beta[i][j];
      s_alpha[i] = a.alpha[i];
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      s_cerr[i] = a.cerr[i];
      s_cmid[i] = a.cmid[i];
    }
    s_tq[0] = tg[0];
    s_nq = 1;
  }
  if (w0) {
    y = own ? a.h0[b * H + lane] : 0.f;
    co[0] = y;
    t0s = t1s = (double)tg[0];
    if (own) {
      a.sol[b * H + lane] = y;
      publish(lane, y, a.prev0 ? a.prev0[b * In + lane] : 0.f);
    }
  }

  int phase = kPhaseF0;
  for (;;) {
    __syncthreads();  // wave 0's announcement: s_nq, s_tq and its part of the first input
    const int n = s_nq;
    if (n == 0) break;  // every thread reads the same word: the four waves leave together
    drive(n, phase == kPhaseF0);
    if (phase == kPhaseF0) {
      const float f = eval();
      phase = a.step.first_step > 0.0 ? kPhaseAttempt : kPhaseProbe;
      if (w0) {
        f0 = f;
        if (phase == kPhaseAttempt) {
          dt = a.step.first_step;
          begin_attempt();
        } else {  // misc._select_initial_step: the probe f(t0 + h0, y0 + h0 f0)
          scale = atol + rtol * fabsf(y);
          const float q0 = y / scale, q1 = f0 / scale;
          const double s0 = wave_sum_d(own ? (double)q0 * q0 : 0.0);
          const double s1 = wave_sum_d(own ? (double)q1 * q1 : 0.0);
          float d0;
          h0p = dopri_h0(s0, s1, n_el, d0, d1p);
          if (own) publish(lane, y + f0 * h0p, xs[lane]);
          if (lane == 0) {
            s_tq[0] = (float)(t0s + (double)h0p);
            s_nq = 1;
          }
        }
      }
    } else if (phase == kPhaseProbe) {
      const float f1 = eval();
      phase = kPhaseAttempt;
      if (w0) {
        const float q2 = (f1 - f0) / scale;
        const double s2 = wave_sum_d(own ? (double)q2 * q2 : 0.0);
        float d2, h1;
        dt = dopri_dt0(s2, n_el, h0p, d1p, d2, h1);
        begin_attempt();
      }
    } else {
      float kn = 0.f;
#pragma unroll 1
      for (int s = 0; s < 6; ++s) {
        kn = eval();
        if (w0) {
          const int j = s + 1, jc = j < 5 ? j : 5;
#pragma unroll
          for (int i = 0; i < 5; ++i) {
            const int r = j + i < 5 ? j + i : 5;
            A[i] = (j + i <= 5) ? A[i + 1] + kn * (s_beta[r][jc] * dt32) : 0.f;
          }
          err = err + kn * (s_cerr[j] * dt32);
          mid = mid + kn * (s_cmid[j] * dt32);
          if (s < 5) {
            yi = y + A[0];
            if (own) publish(lane, yi, xs[lane]);
          }
        }
        if (drv && s < 5) publish(H + dd, us[s + 1][dd], xs[H + dd]);
      }
      if (w0) {
        const float y1 = yi;
        const float tol = atol + rtol * fmaxf(fabsf(y), fabsf(y1));
        const float qe = err / tol;
        const double ss = wave_sum_d(own ? (double)qe * qe : 0.0);
        const float ratio = dopri_ratio(ss, n_el);
        const bool accept = dopri_accept(ratio);
        if (lane == 0) dopri_log_attempt(a.att + b * (int64_t)a.max_att * 4, n_att, a.max_att, t0, dt, ratio, accept);
        ++n_att;
        if (!__builtin_isfinite(ratio)) {
          status = 1;
        } else {
          if (accept) {
            dopri_fit(co, y, y1, mid, f0, kn, dt32);
            y = y1;
            f0 = kn;
            t0s = t0;
            t1s = t1;
          } else {
            t0s = t0;
          }
          dt = dopri_next_dt(dt, ratio, a.step);
          ++n_steps;
        }
        begin_attempt();
      }
    }
  }
  // prev <- the last evaluation's input (the end publishes nothing)
  if (a.prev_out && tid < In) a.prev_out[b * In + tid] = xs[tid];
  if (tid == 0) {
    a.stats[b * 3 + 0] = nfev;
    a.stats[b * 3 + 1] = n_att;
    a.stats[b * 3 + 2] = status;
  }
}

template <bool EVLOG>
void launch_dopri5(int K, int64_t B, hipStream_t st, const DrivenDopriArgs& a) {
  const dim3 g((unsigned)B), t(kDrvThreads);
  if (K == 10) hipLaunchKernelGGL((driven_dopri5_kernel<10, EVLOG>), g, t, 0, st, a);
  else if (K == 12) hipLaunchKernelGGL((driven_dopri5_kernel<12, EVLOG>), g, t, 0, st, a);
  else hipLaunchKernelGGL((driven_dopri5_kernel<0, EVLOG>), g, t, 0, st, a);
}

// steps counted per output interval beyond which only the geometric shrink of a rejected step bounds
// the loop (DESIGN §4.18 "Termination")
constexpr int kDrvBoundedSteps = 1 << 20;

}  // namespace

extern "C" {

int fetode_driven_dopri5(const fetode_ferro_t* basis, const void* plan, const float* h0, int64_t B, const float* x,
                         const float* t_grid, int32_t T, double rtol, double atol, const double* opts,
                         const float* tableau, const float* prev0, float* sol, float* prev_out, int32_t* stats,
                         double* attempts, int32_t max_attempts, float* evlog, int32_t max_ev, void* stream) {
  if (!fetode_driven_supported(basis)) return set_err(FETODE_EUNSUPPORTED, "driven: shape outside the admitted family");
  if (B < 0 || T < 2 || max_attempts < 0 || max_ev < 0)
    return set_err(FETODE_EINVAL, "driven dopri5: bad sizes (B=%lld, T=%d, max_attempts=%d, max_ev=%d)", (long long)B, T,
                   max_attempts, max_ev);
  if (B == 0) return FETODE_OK;
  if (!plan || !h0 || !x || !t_grid || !opts || !tableau || !sol || !stats || (max_attempts > 0 && !attempts))
    return set_err(FETODE_EINVAL, "driven dopri5: null pointer");
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
  a.H = basis->out_dim; a.D = basis->in_dim - basis->out_dim; a.K = basis->num_basis; a.T = T;
  a.max_att = attempts ? max_attempts : 0;
  a.max_ev = evlog ? max_ev : 0;
  a.gs = (float)basis->gate_slope; a.gsl2e = (float)basis->gate_slope * FETODE_LOG2E;
  a.wc = (float)(-2.0 * (1.0 - basis->alpha));
  a.rtol = (float)rtol; a.atol = (float)atol;
  memcpy(a.beta, tableau, sizeof(a.beta));
  memcpy(a.cerr, tableau + 36, sizeof(a.cerr));
  memcpy(a.cmid, tableau + 43, sizeof(a.cmid));
  // torchdiffeq's alpha (dopri5.py _A) rounded to fp32 like the rest of the tableau
  const double alpha[6] = {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
  for (int i = 0; i < 6; ++i) a.alpha[i] = (float)alpha[i];
  if (evlog) launch_dopri5<true>(a.K, B, (hipStream_t)stream, a);
  else launch_dopri5<false>(a.K, B, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return FETODE_OK;
}

}  // extern "C"
