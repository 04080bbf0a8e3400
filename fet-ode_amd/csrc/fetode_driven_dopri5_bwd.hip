// fetode_driven_dopri5_bwd.hip — loss.backward() through the one-launch dopri5 solve of the
// input-driven Ferro field (fetode_driven_dopri5_tape): reverse mode through every evaluation of every
// attempt of a sample (rejected ones included), the stage sums, the error ratio, the step-size control,
// the initial-step selection and the dense output, like autograd through torchdiffeq run on that
// sample alone.  The field is driven by x(t), so — unlike the autonomous fields of fetode_ecg_bwd.hip —
// an evaluation's TIME carries an adjoint: tau_e = sum_d hxbar[H + d] * slope_d(tau_e), with the slope
// of the interpolated series from the tape (0 where the clamp cut the query), and it reaches the step
// size and the step's start through the stage-time expressions of the forward:
//     fp32(t0) + alpha_s dt32  ->  t0bar += tau, dtbar += alpha_s tau      (alpha_s != 1)
//     fp32(t0 + dt)            ->  t0bar += tau, dtbar += tau
//     the probe at t0 + h0     ->  h0bar += tau              (t[0] and the output times are constants)
// One step controller per sample, so nothing couples the batch: a workgroup of four waves owns a sample
// and walks that sample's evaluations backwards from its own status words; no workgroup waits on
// another one.  Wave 0 holds the element adjoints (one lane per element) and the fp64 control scalars
// (equal on all its lanes, sums by the forward's butterfly); the four waves share the evaluation's VJP
// by drv_elem_vjp (fetode_driven_dev.h) in driven_adj_kernel's loop and mapping (lane -> output, wave
// w -> inputs i = w (mod 4), one wave sum per input), over the H state inputs, and over the D driving
// inputs too when the step-size gradient is on or adj_u is asked for (fetode_driven_dopri5_backward_x:
// d loss / d x(t) of every evaluation, which fetode_driven_table_backward takes to the series' knots).
// step_grad = 0 freezes the step sequence: every dt, t0 and stage time is a constant, so there is no
// control chain and no time adjoint, and a rejected attempt contributes exactly nothing.
// Written: adj (B, max_ev, H) = d loss / d every evaluation's output (rows at or beyond nfev: zeros),
// grad_h0 (B, H) and, where given, adj_u (B, max_ev, D) (zeros likewise).  The parameter sums are formed from adj and the tape by the caller
// (fetode_driven_param_grad, fetode_driven_pgrad.hip, or the generic Ferro backward).
#include <string.h>

#include "fetode_dopri_ctl.h"
#include "fetode_driven_dev.h"

using namespace fetode;

namespace {

struct DrivenDopriAdjArgs {
  const float* plan;
  const float* tg;        // (T) fp32 output times
  const float* prev0;     // (B, H+D) nullable: the hysteresis input before the first evaluation
  const int32_t* stats;   // (B, 3) nfev, attempts, status of the forward
  const double* att;      // (B, max_att, 4) attempt log
  const double* init_rec; // (B, 5) d0, d1, d2, h0, h1
  const float* tape_hx;   // (B, max_ev, H+D)
  const float* tape_phi;  // (B, max_ev, H)
  const float* tape_sl;   // (B, max_ev, D)
  const float* gsol;      // (T, B, H) d loss / d solution
  float* adj;             // (B, max_ev, H)
  float* grad_h0;         // (B, H)
  float* adj_u;           // (B, max_ev, D) nullable: d loss / d every evaluation's x(t)
  int32_t H, D, K, T, max_att, max_ev, base, step_grad;
  float gs, gsl2e, wc;
  float rtol, atol;
  double ifactor, dfactor, min_step, max_step;
  float beta[6][6], cerr[7], cmid[7], alpha[6];
};

template <int KT>
__global__ __launch_bounds__(kDrvThreads) void driven_dopri5_adj_kernel(DrivenDopriAdjArgs a) {
  __shared__ float xs[kDrvInMax], gxs[kDrvInMax], vs[kDrvInMax], us[kDrvInMax];
  __shared__ float gph[64], gout[kDrvInMax];
  __shared__ float s_k[8][64], s_kb[8][64];  // k_1..k_7 of the attempt and their adjoints (wave 0, lane's own column)
  __shared__ float s_beta[6][6], s_cerr[7], s_cmid[7], s_alpha[6];
  const int H = a.H, D = a.D, In = H + D, K = KT > 0 ? KT : a.K, T = a.T;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.x, B = gridDim.x;  // grid = B
  const int max_ev = a.max_ev, base = a.base;
  const bool sg = a.step_grad != 0;
  const bool w0 = wv == 0, own = w0 && lane < H;
  // the sample's own counts, held to the capacities passed in: a sample that failed, or whose log or
  // tape does not hold all of its solve, writes zeros and leaves (every thread reads the same words)
  const int nfev = a.stats[b * 3 + 0], n_att = a.stats[b * 3 + 1], status = a.stats[b * 3 + 2];
  const bool ok = status == 0 && n_att >= 1 && n_att <= a.max_att && nfev <= max_ev &&
                  (int64_t)nfev == (int64_t)base + 6 * (int64_t)n_att;
  const int n_ev = ok ? nfev : 0;
  float* __restrict__ adjb = a.adj + b * (int64_t)max_ev * H;
  for (int64_t i = (int64_t)n_ev * H + tid; i < (int64_t)max_ev * H; i += kDrvThreads) adjb[i] = 0.f;
  float* __restrict__ adjub = a.adj_u ? a.adj_u + b * (int64_t)max_ev * D : nullptr;
  if (adjub)
    for (int64_t i = (int64_t)n_ev * D + tid; i < (int64_t)max_ev * D; i += kDrvThreads) adjub[i] = 0.f;
  if (!ok) {
    if (tid < H) a.grad_h0[b * H + tid] = 0.f;
    return;
  }
  const float4* __restrict__ el = reinterpret_cast<const float4*>(a.plan);
  const float* __restrict__ tail = a.plan + 4 * drv_plan_elems(In, H, K);
  const float* __restrict__ thx = a.tape_hx + b * (int64_t)max_ev * In;
  const float* __restrict__ tphi = a.tape_phi + b * (int64_t)max_ev * H;
  const float* __restrict__ tsl = a.tape_sl + b * (int64_t)max_ev * D;
  const double* __restrict__ att = a.att + b * (int64_t)a.max_att * 4;
  const double* __restrict__ irec = a.init_rec + b * 5;
  const float* __restrict__ tg = a.tg;
  const float gs = a.gs, gsl2e = a.gsl2e, wc = a.wc;
  const float rtol = a.rtol, atol = a.atol;
  const double n_el = (double)H;
  const float gain = own ? tail[H + lane] : 0.f, bias = own ? tail[2 * H + lane] : 0.f;
  const int nI = (sg || adjub) ? In : H;  // inputs that carry an adjoint
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
  }
  if (w0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s_k[j][lane] = s_kb[j][lane] = 0.f;
  }
  // element `lane` of evaluation e's input and output (own lanes), the output by the forward's expression
  auto tx = [&](int e) -> float { return thx[(int64_t)e * In + lane]; };
  auto tk = [&](int e) -> float { return tanhf(tphi[(int64_t)e * H + lane]) * gain + bias; };

  // wave 0's element adjoints: carried (current y, f0), this attempt's (y, y1, dt32, the outputs'
  // d/d dt and d/d t0 terms), the initial step's (scale, the probe's term of f0)
  float ybc = 0.f, fbc = 0.f, yb0 = 0.f, yb1 = 0.f, dtb32 = 0.f, scb = 0.f, f0bp = 0.f;
  double pd = 0.0, pt = 0.0;
  // the control chain of the sample, fp64, equal on wave 0's lanes: adjoints of the next dt and of t1s,
  // the attempt's time adjoints towards dt and t0
  double dtbar = 0.0, tbar = 0.0, dtb_base = 0.0, h0b = 0.0, d0b = 0.0, d1b = 0.0, tq_d = 0.0, tq_t = 0.0;
  float dt32 = 0.f, h0f = 0.f;
  int jj = T - 1;  // the last output not yet taken
  bool acc_n = false;
  __syncthreads();  // the tableau is in LDS

  for (int ev = n_ev - 1; ev >= 0; --ev) {
    const bool in_att = ev >= base;
    const int n = in_att ? (ev - base) / 6 : -1, s = in_att ? 2 + (ev - base) % 6 : 0;
    // ---------------- before the VJP: this evaluation's output adjoint (wave 0) ----------------
    if (w0) {
      float ae = 0.f;
      if (in_att && s == 7) {
        const double t0 = att[4 * n], dt = att[4 * n + 1];
        const float ratio = (float)att[4 * n + 2];
        acc_n = att[4 * n + 3] != 0.0;
        int m = n - 1;  // the attempt whose stage 7 produced this attempt's y and f0
        while (m >= 0 && att[4 * m + 3] == 0.0) --m;
        const int fe = m >= 0 ? base + 6 * m + 5 : 0;
        const int e2 = base + 6 * n;
        dt32 = (float)dt;
        const double rr = (double)ratio;
        double rbar = 0.0, dtbb = 0.0;
        if (sg && n + 1 < n_att)
          dopri_next_dt_adjoint(dtbar, dt, att[4 * (n + 1) + 1], rr, a.ifactor, a.dfactor, a.min_step, a.max_step, dtbb,
                                rbar);
        dtb_base = dtbb;
        pd = pt = tq_d = tq_t = 0.0;
        dtb32 = 0.f;
        float kv[8], kbv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) kv[j] = kbv[j] = 0.f;
        float y = 0.f, y1 = 0.f;
        if (own) {
          y = tx(fe);
          kv[1] = tk(fe);
#pragma unroll
          for (int j = 2; j <= 7; ++j) kv[j] = tk(e2 + j - 2);
          y1 = tx(e2 + 5);
        }
        // err and mid in the forward's op order
        float err = kv[1] * (s_cerr[0] * dt32), midv = kv[1] * (s_cmid[0] * dt32);
#pragma unroll
        for (int j = 2; j <= 7; ++j) {
          err = err + kv[j] * (s_cerr[j - 1] * dt32);
          midv = midv + kv[j] * (s_cmid[j - 1] * dt32);
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
          for (; jj >= 1 && (double)tg[jj] > t0; --jj) {  // outputs in (t0, t1]
            const float x = (float)(((double)tg[jj] - t0) / dlt);
            const float g = own ? a.gsol[((int64_t)jj * B + b) * H + lane] : 0.f;
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
        if (own && rbar != 0.0 && ratio > 0.f) {
          const float tol = atol + rtol * fmaxf(fabsf(y), fabsf(y1));
          const float qe = err / tol;
          const float qb = (float)(rbar * (double)qe / (n_el * rr));
          errb = qb / tol;
          const float tolb = -qb * qe / tol, ay = fabsf(y), ay1 = fabsf(y1);
          const float sy = y > 0.f ? 1.f : (y < 0.f ? -1.f : 0.f), sy1 = y1 > 0.f ? 1.f : (y1 < 0.f ? -1.f : 0.f);
          const float wy = ay > ay1 ? 1.f : (ay < ay1 ? 0.f : 0.5f);
          yb0 += tolb * rtol * wy * sy;
          yb1 += tolb * rtol * (1.f - wy) * sy1;
        }
        float se = 0.f, sm = 0.f;
#pragma unroll
        for (int j = 1; j <= 7; ++j) {
          kbv[j] += errb * (s_cerr[j - 1] * dt32) + midb * (s_cmid[j - 1] * dt32);
          se += s_cerr[j - 1] * kv[j];
          sm += s_cmid[j - 1] * kv[j];
        }
        dtb32 += errb * se + midb * sm;
#pragma unroll
        for (int j = 1; j <= 7; ++j) {
          s_k[j][lane] = kv[j];
          s_kb[j][lane] = kbv[j];
        }
      } else if (!in_att && ev == 1) {
        // _select_initial_step (fp32): dt0 = min(100 h0, |h1|) back to h0, d1 and the probe
        f0bp = scb = 0.f;
        h0b = d0b = d1b = 0.0;
        h0f = 0.f;
        if (sg) {
          const float d1 = (float)irec[1], d2 = (float)irec[2], h1 = (float)irec[4];
          h0f = (float)irec[3];
          double r2 = 0.0, r2b = 0.0;
          dopri_dt0_adjoint(dtbar, d1, d2, h0f, h1, h0b, d1b, r2, r2b);
          if (own && r2 > 0.0) {
            const float y = tx(0), f0 = tk(0), f1 = tk(1);
            const float scale = atol + rtol * fabsf(y);
            const float q2 = (f1 - f0) / scale;
            const float q2b = (float)(r2b * (double)q2 / (n_el * r2));
            ae = q2b / scale;
            f0bp = -q2b / scale;
            scb = -q2b * q2 / scale;
          }
        }
      } else if (ev == 0) {
        if (sg && base == 2) {  // the rest of _select_initial_step: d0 = rms(y0 / scale), d1 = rms(f0 / scale)
          const float d0 = (float)irec[0], d1 = (float)irec[1];
          if (own) {
            const float y = tx(0), f0 = tk(0);
            const float scale = atol + rtol * fabsf(y);
            const float q0 = y / scale, q1 = f0 / scale;
            const float q0b = d0 > 0.f ? (float)(d0b * (double)q0 / (n_el * d0)) : 0.f;
            const float q1b = d1 > 0.f ? (float)(d1b * (double)q1 / (n_el * d1)) : 0.f;
            const float sc = scb - q0b * q0 / scale - q1b * q1 / scale;
            const float sy = y > 0.f ? 1.f : (y < 0.f ? -1.f : 0.f);
            ybc += q0b / scale + sc * rtol * sy;
            fbc += q1b / scale;
          }
        }
        ae = own ? fbc : 0.f;
      }
      if (in_att) ae = s_kb[s][lane];
      float g = 0.f;
      if (own) {
        adjb[(int64_t)ev * H + lane] = ae;
        const float t = tanhf(tphi[(int64_t)ev * H + lane]);
        g = (ae * gain) * (1.0f - t * t);
      }
      gph[lane] = g;
    }
    // ---------------- the evaluation's VJP: d loss / d its input ----------------
    if (tid < In) {
      const float xv = thx[(int64_t)ev * In + tid];
      const float pv = ev > 0 ? thx[(int64_t)(ev - 1) * In + tid] : (a.prev0 ? a.prev0[b * In + tid] : 0.f);
      const DrvGate g = drv_gate(gs, gsl2e, wc, xv, pv);
      xs[tid] = g.x;
      gxs[tid] = g.gx;
      vs[tid] = g.v;
      us[tid] = g.u;
    }
    __syncthreads();
    const float gp = gph[lane];
    for (int i = wv; i < nI; i += 4) {
      float d = 0.f;
      if (lane < H) {
        const float x = xs[i], v = vs[i], gx = gxs[i], u = us[i];
        const float4* __restrict__ p = el + (int64_t)i * K * H + lane;
#pragma unroll KT > 0 ? KT : 1
        for (int k = 0; k < K; ++k) d = drv_elem_vjp(p[(int64_t)k * H], x, gx, v, u, gs, d);
      }
      const float r = wave_sum(d * gp);
      if (lane == 0) gout[i] = r * (0.5f / FETODE_LOG2E);  // c.y, c.z carry 2 log2e
    }
    __syncthreads();
    if (adjub && tid >= 64 && tid < 64 + D) adjub[(int64_t)ev * D + (tid - 64)] = gout[H + (tid - 64)];
    // ---------------- after the VJP: the input adjoint (wave 0) ----------------
    if (w0) {
      const float xb = own ? gout[lane] : 0.f;
      double tau = 0.0;  // the evaluation time's adjoint
      if (sg) {
        for (int d = 0; d < D; ++d) tau += (double)gout[H + d] * (double)tsl[(int64_t)ev * D + d];
      }
      if (in_att) {
        const float X = xb + (s == 7 ? yb1 : 0.f);  // stage 7's input IS y1
        yb0 += X;
        float sb = 0.f;
        for (int j = 1; j < s; ++j) {  // tableau row s - 2
          const float c = s_beta[s - 2][j - 1];
          s_kb[j][lane] += (c * dt32) * X;
          sb += c * s_k[j][lane];
        }
        dtb32 += X * sb;
        const float al = s_alpha[s - 2];  // the stage time: fp32(t0 + dt) where alpha is 1, else fp32(t0) + alpha dt32
        tq_t += tau;
        tq_d += (al == 1.0f ? 1.0 : (double)al) * tau;
        if (s == 2) {  // attempt n done: the carries, and the sample's d/d dt and d/d t0 sums
          ybc = own ? yb0 : 0.f;
          fbc = own ? s_kb[1][lane] : 0.f;
          if (sg) {
            const double S0 = wave_sum_d(own ? pd + (double)dtb32 : 0.0) + tq_d;
            const double S1 = wave_sum_d(own ? pt : 0.0) + tq_t;
            dtbar = dtb_base + (acc_n ? tbar : 0.0) + S0;
            tbar = tbar + S1;
          }
        }
      } else if (ev == 1) {  // the probe: input y0 + h0 f0 at t0 + h0
        const float f0 = own ? tk(0) : 0.f;
        if (own) {
          ybc += xb;
          fbc += xb * h0f + f0bp;
        }
        if (sg) {
          const double S0 = wave_sum_d(own ? (double)(xb * f0) : 0.0);
          h0b = h0b + S0 + tau;
          dopri_h0_adjoint(h0b, h0f, (float)irec[0], (float)irec[1], d0b, d1b);
        }
      } else {  // evaluation 0: f(y0) at t[0]
        if (own) {
          ybc += xb;
          a.grad_h0[b * H + lane] = ybc + a.gsol[b * H + lane];  // solution[0] = y0
        }
      }
    }
  }
}

const DrvKRow<DrivenDopriAdjArgs> kDopri5Adj = {driven_dopri5_adj_kernel<10>, driven_dopri5_adj_kernel<12>,
                                                driven_dopri5_adj_kernel<0>};

int driven_dopri5_backward(const fetode_ferro_t* basis, const void* plan, int64_t B, const float* t_grid, int32_t T,
                           double rtol, double atol, const double* opts, const float* tableau, const float* prev0,
                           const int32_t* stats, const double* attempts, int32_t max_attempts, const float* tape_hx,
                           const float* tape_phi, const float* tape_slope, const double* init_rec, int32_t max_ev,
                           const float* grad_sol, int32_t step_grad, float* adj, float* grad_h0, float* adj_u, bool xg,
                           void* stream) {
  if (!fetode_driven_supported(basis)) return set_err(FETODE_EUNSUPPORTED, "driven: shape outside the admitted family");
  if (B < 0 || T < 2 || max_attempts < 1 || max_ev < 1)
    return set_err(FETODE_EINVAL, "driven dopri5 backward: bad sizes (B=%lld, T=%d, max_attempts=%d, max_ev=%d)",
                   (long long)B, T, max_attempts, max_ev);
  if (B == 0) return FETODE_OK;
  if (!plan || !t_grid || !opts || !tableau || !stats || !attempts || !tape_hx || !tape_phi || !tape_slope ||
      !init_rec || !grad_sol || !adj || !grad_h0 || (xg && !adj_u))
    return set_err(FETODE_EINVAL, "driven dopri5 backward: null pointer");
  if (B > 0x7fffffff) return set_err(FETODE_EUNSUPPORTED, "driven dopri5: batch too large");
  DrivenDopriAdjArgs a{};
  DopriStep step;
  dopri_step_from_opts(opts, step);
  a.plan = (const float*)plan;
  a.tg = t_grid; a.prev0 = prev0; a.stats = stats; a.att = attempts; a.init_rec = init_rec;
  a.tape_hx = tape_hx; a.tape_phi = tape_phi; a.tape_sl = tape_slope; a.gsol = grad_sol;
  a.adj = adj; a.grad_h0 = grad_h0; a.adj_u = adj_u;
  drv_fill_field(a, basis);
  a.T = T;
  a.max_att = max_attempts; a.max_ev = max_ev; a.base = dopri_base(opts); a.step_grad = step_grad ? 1 : 0;
  a.rtol = (float)rtol; a.atol = (float)atol;
  a.ifactor = step.ifactor; a.dfactor = step.dfactor; a.min_step = step.min_step; a.max_step = step.max_step;
  memcpy(a.beta, tableau, sizeof(a.beta));
  memcpy(a.cerr, tableau + 36, sizeof(a.cerr));
  memcpy(a.cmid, tableau + 43, sizeof(a.cmid));
  const double alpha[6] = {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};  // as the forward rounds them
  for (int i = 0; i < 6; ++i) a.alpha[i] = (float)alpha[i];
  drv_launch(kDopri5Adj, a.K, dim3((unsigned)B), kDrvThreads, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return FETODE_OK;
}

}  // namespace

extern "C" {

int fetode_driven_dopri5_backward(const fetode_ferro_t* basis, const void* plan, int64_t B, const float* t_grid,
                                  int32_t T, double rtol, double atol, const double* opts, const float* tableau,
                                  const float* prev0, const int32_t* stats, const double* attempts,
                                  int32_t max_attempts, const float* tape_hx, const float* tape_phi,
                                  const float* tape_slope, const double* init_rec, int32_t max_ev,
                                  const float* grad_sol, int32_t step_grad, float* adj, float* grad_h0, void* stream) {
  return driven_dopri5_backward(basis, plan, B, t_grid, T, rtol, atol, opts, tableau, prev0, stats, attempts,
                                max_attempts, tape_hx, tape_phi, tape_slope, init_rec, max_ev, grad_sol, step_grad, adj,
                                grad_h0, nullptr, false, stream);
}

int fetode_driven_dopri5_backward_x(const fetode_ferro_t* basis, const void* plan, int64_t B, const float* t_grid,
                                    int32_t T, double rtol, double atol, const double* opts, const float* tableau,
                                    const float* prev0, const int32_t* stats, const double* attempts,
                                    int32_t max_attempts, const float* tape_hx, const float* tape_phi,
                                    const float* tape_slope, const double* init_rec, int32_t max_ev,
                                    const float* grad_sol, int32_t step_grad, float* adj, float* grad_h0,
                                    float* adj_u, void* stream) {
  return driven_dopri5_backward(basis, plan, B, t_grid, T, rtol, atol, opts, tableau, prev0, stats, attempts,
                                max_attempts, tape_hx, tape_phi, tape_slope, init_rec, max_ev, grad_sol, step_grad, adj,
                                grad_h0, adj_u, true, stream);
}

}  // extern "C"
