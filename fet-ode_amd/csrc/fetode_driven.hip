// fetode_driven.hip — the input-driven Ferro field of the ECG NODE-RNN encoder, solved in one launch
// (compare_noise_ecg.py:848-946: LinearInterp1D, InputDrivenKANODEFunc, OneODEEncoder):
//     dh/dt = tanh(Ferro_{(H+D)->H}(cat[h, x(t)])) * gain + bias          (torchdiffeq rk4, 3/8 rule)
//   driven_table_kernel   x(t) at every evaluation time, the reference's fp32 expression (:861-872)
//   driven_plan_kernel    per-element constants + sum bias*coef per output, one launch
//   driven_fixed_kernel   the whole fixed-grid solve; a workgroup owns its samples from h0 to the end
//                         (GRID: euler, midpoint, rk4 and rk4_classic on a per-step coefficient array,
//                         the fetode_driven_grid entries)
//   driven_adj_kernel     the reverse sweep along the chain of evaluations (d/dh; with XG also d/dx(t)
//                         of every evaluation; the parameter sums over the taped rows:
//                         fetode_driven_pgrad.hip or the generic Ferro backward)
//   driven_table_bwd_kernel  d/dx(t) of every evaluation back to the series' knots (LinearInterp1D's
//                         backward), a gather in ascending evaluation order
// The reference resets the hysteresis state before every sample's solve, so the samples are
// independent: sample b carries its own driving row and its own prev.  branch_sign stays 1, so
//     m = 1 - 2(1-alpha)(1-u) sigma(gs(-x-Ec)),   u = sigma(gs(x - prev))       (DESIGN §3 "Algebra").
// Mapping: 256 threads = 4 waves; lane -> output o (lanes >= H idle), wave w -> inputs i = w (mod 4).
// Every lane sums the K bases of one input first, then its inputs; the four waves'
// partial sums meet in LDS in a fixed order.  No workgroup waits on another one.  The gate, the element
// loop, the meeting, the VJP and the interpolator's locate step are fetode_driven_dev.h's functions, shared
// with the dopri5 kernels; the kernels here hold the solver around them.
#include "fetode_driven_dev.h"

using namespace fetode;

namespace {

constexpr float kThird = 1.0f / 3.0f;

// ---------------------------------------------------------------------------------------------
// driving table: u[e][b][d] = LinearInterp1D(t_grid, x[b])(tq[e])
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void driven_table_kernel(const float* __restrict__ tq, int64_t n_eval,
                                                          const float* __restrict__ tg, int T,
                                                          const float* __restrict__ x, int64_t B, int D,
                                                          float* __restrict__ u) {
  const int64_t n = n_eval * B * D;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(idx % D);
    const int64_t b = (idx / D) % B, e = idx / ((int64_t)D * B);
    const float lo = tg[0], hi = tg[T - 1];
    float w;
    const int i = drv_locate(tg, T, lo, hi, tq[e], w);
    const float x0 = x[(b * T + (i - 1)) * D + d], x1 = x[(b * T + i) * D + d];
    u[idx] = (1.0f - w) * x0 + w * x1;
  }
}

// ---------------------------------------------------------------------------------------------
// driving table, backward: grad_x[b][j][d] = sum over sample b's live evaluations e, in ascending e,
// of adj_u[b][e][d] times the weight the forward gave knot j at the evaluation's time
// ---------------------------------------------------------------------------------------------
constexpr int kTbThreads = 256;

struct DrivenTbArgs {
  const float* tq;        // the time of row (b, e) at tq[b * tq_stride_b + e]
  const float* tg;        // (T) knots
  const float* adj_u;     // row (b, e) at (b * stride_b + e * stride_e) * D
  const int32_t* nfev;    // nullable: every row e < n_ev is live
  float* gx;              // (B, T, D)
  int64_t B, n_ev, tq_stride_b, stride_b, stride_e, nfev_stride;
  int32_t T, D;
};

// Workgroup (b, chunk of 256 outputs): thread -> output (j, d) of sample b.  The sample's evaluations
// are taken 256 at a time: every thread locates one of them in the grid (drv_locate, the forward's fp32
// expression) into LDS, then every
// thread walks the 256 (interval, weight) pairs in order and adds the ones that name its knot.  The
// order is ascending e whatever the strides are: the same bits for the same rows in either layout.
__global__ __launch_bounds__(kTbThreads) void driven_table_bwd_kernel(DrivenTbArgs a) {
  __shared__ int si[kTbThreads];
  __shared__ float sw[kTbThreads];
  const int tid = threadIdx.x, T = a.T, D = a.D;
  const int64_t b = blockIdx.x;   // grid.x = B
  const int64_t o = (int64_t)blockIdx.y * kTbThreads + tid;
  const bool act = o < (int64_t)T * D;
  const int j = act ? (int)(o / D) : 0, d = act ? (int)(o - (int64_t)j * D) : 0;
  int64_t nl = a.n_ev;            // the live rows of sample b: min(nfev, n_ev), 0 for a count <= 0
  if (a.nfev) {
    const int64_t n = a.nfev[b * a.nfev_stride];
    nl = n < 0 ? 0 : (n > a.n_ev ? a.n_ev : n);
  }
  const float* __restrict__ tg = a.tg;
  const float lo = tg[0], hi = tg[T - 1];
  float acc = 0.f;
  for (int64_t e0 = 0; e0 < nl; e0 += kTbThreads) {   // nl is uniform: every thread reaches every barrier
    const int64_t e = e0 + tid;
    if (e < nl) {
      float w;
      si[tid] = drv_locate(tg, T, lo, hi, a.tq[b * a.tq_stride_b + e], w);
      sw[tid] = w;
    }
    __syncthreads();
    const int n = nl - e0 < kTbThreads ? (int)(nl - e0) : kTbThreads;
    if (act) {
      for (int q = 0; q < n; ++q) {
        const int i = si[q];
        if (i == j || i - 1 == j) {   // 1 <= i <= T - 1: at most one of the two
          const float w = sw[q];
          const float g = a.adj_u[(b * a.stride_b + (e0 + q) * a.stride_e) * D + d];
          acc = acc + (i == j ? w : 1.0f - w) * g;
        }
      }
    }
    __syncthreads();
  }
  if (act) a.gx[(b * T + j) * D + d] = acc;
}

// ---------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void driven_plan_kernel(fetode_ferro_t fl, const float* __restrict__ gain,
                                                         const float* __restrict__ bias, float* __restrict__ plan) {
  const int In = fl.in_dim, H = fl.out_dim, K = fl.num_basis;
  const int64_t ne = drv_plan_elems(In, H, K);
  const float gsl2e = (float)fl.gate_slope * FETODE_LOG2E;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t p = t; p < ne; p += (int64_t)gridDim.x * blockDim.x) {
    const int o = (int)(p % H), k = (int)((p / H) % K), i = (int)(p / ((int64_t)H * K));
    const int e = (i * H + o) * K + k;
    const float Ec = fl.Ec[e], kk = fl.k[e];
    const float k2 = 2.0f * FETODE_LOG2E * kk;
    reinterpret_cast<float4*>(plan)[p] = make_float4(gsl2e * Ec, k2, k2 * Ec, fl.coef[e] * fl.Ps[e]);
  }
  if (t < H) {
    const int o = (int)t;
    float acc = 0.f;
    for (int i = 0; i < In; ++i) {
      float acc_i = 0.f;
      for (int k = 0; k < K; ++k) {
        const int e = (i * H + o) * K + k;
        acc_i += fl.bias[e] * fl.coef[e];
      }
      acc += acc_i;
    }
    float* tail = plan + 4 * ne;
    tail[o] = acc;
    tail[H + o] = gain[o];
    tail[2 * H + o] = bias[o];
  }
}

// ---------------------------------------------------------------------------------------------
// forward solve
// ---------------------------------------------------------------------------------------------
// GRID: the four fixed-grid methods (a.method, uniform per launch) with n_m = 1 << a.nm_log2
// evaluations per step and the coefficients of step s at a.dt[4 s ..] (dt, fp32(dt / 2), fp32(dt / 6));
// the combines follow rk_combine_kernel's op order as _per_stage_fixed calls it.  GRID off is the
// rk4 (3/8) kernel of fetode_driven_fixed: the method folds at compile time.
template <int S, int KT, bool TAPE, bool GRID = false>
__global__ __launch_bounds__(kDrvThreads) void driven_fixed_kernel(DrivenArgs a) {
  __shared__ float xs[S][kDrvInMax], gxs[S][kDrvInMax], vs[S][kDrvInMax];
  __shared__ float part[4][S][64];
  const int H = a.H, D = a.D, In = H + D, K = KT > 0 ? KT : a.K;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t B = a.B, b0 = (int64_t)blockIdx.x * S;
  const float4* __restrict__ el = reinterpret_cast<const float4*>(a.plan);
  const float* __restrict__ tail = a.plan + 4 * drv_plan_elems(In, H, K);
  const bool own = wv == 0 && lane < H;               // holds h and the stage slopes of output `lane`
  const int ds = (tid - 64) / D, dd = (tid - 64) - ds * D;
  const bool drv = tid >= 64 && tid < 64 + S * D;     // publishes driving input dd of sample ds
  const float gs = a.gs, gsl2e = a.gsl2e, wc = a.wc;
  float fcon = 0.f, gain = 0.f, bias = 0.f;
  if (own) {
    fcon = tail[lane];
    gain = tail[H + lane];
    bias = tail[2 * H + lane];
  }
  // input i of sample s for the next evaluation: value, its gate against the previous evaluation's
  // input (prev <- hx, call order) and the per-input factors of the element loop
  auto publish = [&](int s, int i, float xn, float xo) {
    const DrvGate g = drv_gate(gs, gsl2e, wc, xn, xo);
    xs[s][i] = g.x;
    gxs[s][i] = g.gx;
    vs[s][i] = g.v;
  };
  float h[S], k1[S], k2[S], k3[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    h[s] = k1[s] = k2[s] = k3[s] = 0.f;
    const int64_t b = b0 + s;
    if (own) {
      const bool live = b < B;
      h[s] = live ? a.h0[b * H + lane] : 0.f;
      publish(s, lane, h[s], (live && a.prev0) ? a.prev0[b * In + lane] : 0.f);
    }
  }
  if (drv) {
    const int64_t b = b0 + ds;
    const bool live = b < B;
    publish(ds, H + dd, live ? a.u[(a.eval0 * B + b) * D + dd] : 0.f,
            (live && a.prev0) ? a.prev0[b * In + H + dd] : 0.f);
  }
  const int method = GRID ? a.method : FETODE_RK4;
  const int sh = GRID ? a.nm_log2 : 2, fin = (1 << sh) - 1;   // a step's last evaluation
  const int n_eval = a.n_steps << sh;
  for (int e = 0; e < n_eval; ++e) {
    const int st = e & fin, step = e >> sh;   // e % n_m, e / n_m
    const int64_t ge = a.eval0 + e;
    __syncthreads();  // this evaluation's inputs are published
    if (TAPE) {
      for (int idx = tid; idx < S * In; idx += kDrvThreads) {
        const int s = idx / In, i = idx - s * In;
        if (b0 + s < B) a.tape_hx[(ge * B + b0 + s) * In + i] = xs[s][i];
      }
    }
    float acc[S];
    drv_eval_partial<S, KT>(el, H, In, K, lane, wv, xs, gxs, vs, acc);
#pragma unroll
    for (int s = 0; s < S; ++s) part[wv][s][lane] = acc[s];
    __syncthreads();  // partial sums are in; nobody reads this evaluation's inputs any more
    const bool last = e == n_eval - 1;
    if (own) {
      const float dt = a.dt[GRID ? 4 * (int64_t)step : (int64_t)step];
      float hh = 0.f, h6 = 0.f;
      if (GRID) {
        hh = a.dt[4 * (int64_t)step + 1];
        h6 = a.dt[4 * (int64_t)step + 2];
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int64_t b = b0 + s;
        const bool live = b < B;
        const float phi = drv_eval_meet<S>(part, s, lane, fcon);
        if (TAPE && live) a.tape_phi[(ge * B + b) * H + lane] = phi;
        const float f = tanhf(phi) * gain + bias;
        float xn;  // torchdiffeq rk4_alt_step_func, its op order
        if (GRID && method != FETODE_RK4) {
          // euler y + dt k1; midpoint y + hh k1 | y + dt k2; classic y + hh k1 | y + hh k2 | y + dt k3 |
          // y + h6 (((k1 + 2 k2) + 2 k3) + k4)
          if (st < fin) {
            if (st == 0) k1[s] = f;
            else if (st == 1) k2[s] = f;
            else k3[s] = f;
            xn = h[s] + (st == 2 ? dt : hh) * f;
          } else {
            if (method == FETODE_RK4_CLASSIC) xn = h[s] + h6 * (((k1[s] + 2.0f * k2[s]) + 2.0f * k3[s]) + f);
            else xn = h[s] + dt * f;
            h[s] = xn;
            if (live) a.sol[((int64_t)step * B + b) * H + lane] = xn;
          }
        } else if (st == 0) {
          k1[s] = f;
          xn = h[s] + (dt * f) * kThird;
        } else if (st == 1) {
          k2[s] = f;
          xn = h[s] + dt * (f - k1[s] * kThird);
        } else if (st == 2) {
          k3[s] = f;
          xn = h[s] + dt * ((k1[s] - k2[s]) + f);
        } else {
          xn = h[s] + (((k1[s] + 3.0f * (k2[s] + k3[s])) + f) * dt) * 0.125f;
          h[s] = xn;
          if (live) a.sol[((int64_t)step * B + b) * H + lane] = xn;
        }
        if (!last) publish(s, lane, xn, xs[s][lane]);
      }
    }
    if (drv && !last) {
      const int64_t b = b0 + ds;
      publish(ds, H + dd, b < B ? a.u[((ge + 1) * B + b) * D + dd] : 0.f, xs[ds][H + dd]);
    }
  }
  // prev <- the last evaluation's input (still in xs: the last evaluation publishes nothing)
  if (a.prev_out && n_eval > 0) {
    for (int idx = tid; idx < S * In; idx += kDrvThreads) {
      const int s = idx / In, i = idx - s * In;
      if (b0 + s < B) a.prev_out[(b0 + s) * In + i] = xs[s][i];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// reverse sweep: adjoints of every evaluation's output and of h0; the gate reads prev detached
// ---------------------------------------------------------------------------------------------
// XG: the D driving inputs carry an adjoint too; adj_u (one row per evaluation, B, D) receives it.
// The h inputs' arithmetic is the same either way, so adj and grad_h0 are the same bits.
// GRID: as in driven_fixed_kernel; the adjoints of the three other combines are written beside them.
template <int S, int KT, bool XG, bool GRID = false>
__global__ __launch_bounds__(kDrvThreads) void driven_adj_kernel(DrivenAdjArgs a) {
  constexpr int NI = XG ? kDrvInMax : kDrvHMax;
  __shared__ float xs[S][NI], gxs[S][NI], vs[S][NI], us[S][NI];
  __shared__ float gph[S][64], gout[S][NI];
  const int H = a.H, D = a.D, In = H + D, K = KT > 0 ? KT : a.K;
  const int nI = XG ? In : H;   // inputs that carry an adjoint
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t B = a.B, b0 = (int64_t)blockIdx.x * S;
  const float4* __restrict__ el = reinterpret_cast<const float4*>(a.plan);
  const float* __restrict__ tail = a.plan + 4 * drv_plan_elems(In, H, K);
  const bool own = wv == 0 && lane < H;
  const float gs = a.gs, gsl2e = a.gsl2e, wc = a.wc;
  const float gain = own ? tail[H + lane] : 0.f;
  const int n_steps = a.n_steps;
  float lam[S], ay[S], ak1[S], ak2[S], ak3[S], ak4[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int64_t b = b0 + s;
    lam[s] = (own && b < B) ? a.grad_sol[((int64_t)n_steps * B + b) * H + lane] : 0.f;
    ay[s] = ak1[s] = ak2[s] = ak3[s] = ak4[s] = 0.f;
  }
  const int method = GRID ? a.method : FETODE_RK4;
  const int sh = GRID ? a.nm_log2 : 2, fin = (1 << sh) - 1;
  const bool alt = GRID && method != FETODE_RK4;
  for (int e = (n_steps << sh) - 1; e >= 0; --e) {
    const int st = e & fin, step = e >> sh;
    const float dt = a.dt[GRID ? 4 * (int64_t)step : (int64_t)step];
    float hh = 0.f, h6 = 0.f;
    if (GRID) {
      hh = a.dt[4 * (int64_t)step + 1];
      h6 = a.dt[4 * (int64_t)step + 2];
    }
    if (own) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int64_t b = b0 + s;
        const bool live = b < B;
        if (GRID) {
          // rk4 as below; classic y1 = y + h6 (((k1 + 2 k2) + 2 k3) + k4); midpoint y1 = y + dt k2; euler
          // y1 = y + dt k1.  Selects of values under the run-time method (ak3, ak4: read by the 4-stage rules)
          const bool top = st == fin, cl = method == FETODE_RK4_CLASSIC;
          const float w8 = (lam[s] * dt) * 0.125f, c6 = h6 * lam[s], cd = dt * lam[s];
          const float n1 = alt ? (cl ? c6 : (method == FETODE_MIDPOINT ? 0.f : cd)) : w8;
          const float n2 = alt ? (cl ? 2.0f * c6 : cd) : 3.0f * w8;
          const float n3 = alt ? 2.0f * c6 : 3.0f * w8;
          const float n4 = alt ? c6 : w8;
          ay[s] = top ? lam[s] : ay[s];
          ak1[s] = top ? n1 : ak1[s];
          ak2[s] = top ? n2 : ak2[s];
          ak3[s] = top ? n3 : ak3[s];
          ak4[s] = top ? n4 : ak4[s];
        } else if (st == 3) {  // y1 = y + ((k1 + 3 (k2 + k3)) + k4) dt / 8
          ay[s] = lam[s];
          ak1[s] = ak4[s] = (lam[s] * dt) * 0.125f;
          ak2[s] = ak3[s] = 3.0f * ((lam[s] * dt) * 0.125f);
        }
        float ae = ak1[s];   // plain selects of values: no pointer select over the register arrays
        if (st == 1) ae = ak2[s];
        if (st == 2) ae = ak3[s];
        if (st == 3) ae = ak4[s];
        float g = 0.f;
        if (live) {
          a.adj[((int64_t)e * B + b) * H + lane] = ae;
          const float t = tanhf(a.tape_phi[((int64_t)e * B + b) * H + lane]);
          g = (ae * gain) * (1.0f - t * t);
        }
        gph[s][lane] = g;
      }
    } else if (wv == 0) {
#pragma unroll
      for (int s = 0; s < S; ++s) gph[s][lane] = 0.f;
    }
    for (int idx = tid; idx < S * nI; idx += kDrvThreads) {
      const int s = idx / nI, i = idx - s * nI;
      const int64_t b = b0 + s;
      float xv = 0.f, pv = 0.f;
      if (b < B) {
        xv = a.tape_hx[((int64_t)e * B + b) * In + i];
        pv = e > 0 ? a.tape_hx[((int64_t)(e - 1) * B + b) * In + i] : (a.prev0 ? a.prev0[b * In + i] : 0.f);
      }
      const DrvGate g = drv_gate(gs, gsl2e, wc, xv, pv);
      xs[s][i] = g.x;
      gxs[s][i] = g.gx;
      vs[s][i] = g.v;
      us[s][i] = g.u;
    }
    __syncthreads();
    float gp[S];
#pragma unroll
    for (int s = 0; s < S; ++s) gp[s] = gph[s][lane];
    for (int i = wv; i < nI; i += 4) {   // XG off: only the h inputs carry an adjoint
      float d[S];
#pragma unroll
      for (int s = 0; s < S; ++s) d[s] = 0.f;
      if (lane < H) {
        const float4* __restrict__ p = el + (int64_t)i * K * H + lane;
#pragma unroll KT > 0 ? KT : 1
        for (int k = 0; k < K; ++k) {
          const float4 c = p[(int64_t)k * H];
#pragma unroll
          for (int s = 0; s < S; ++s) d[s] = drv_elem_vjp(c, xs[s][i], gxs[s][i], vs[s][i], us[s][i], gs, d[s]);
        }
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const float r = wave_sum(d[s] * gp[s]);
        if (lane == 0) gout[s][i] = r * (0.5f / FETODE_LOG2E);   // c.y, c.z carry 2 log2e
      }
    }
    __syncthreads();
    if (XG) {
      for (int idx = tid; idx < S * D; idx += kDrvThreads) {
        const int s = idx / D, dd = idx - s * D;
        if (b0 + s < B) a.adj_u[((int64_t)e * B + b0 + s) * D + dd] = gout[s][H + dd];
      }
    }
    if (own) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const float g = gout[s][lane];
        ay[s] += g;
        if (GRID) {
          // rk4: the three inputs below; the others: input y + c k_st, c = dt at the classic rule's last
          // stage, else hh.  u_j: this evaluation's input holds k_j with weight c_j (selects of values)
          const float dt3 = dt * kThird;
          const float c1 = alt ? hh : (st == 3 ? dt : (st == 2 ? -dt3 : dt3));
          const float c2 = alt ? hh : (st == 3 ? -dt : dt);
          const float c3 = dt;
          const bool u1 = alt ? st == 1 : st >= 1, u2 = alt ? st == 2 : st >= 2, u3 = st == 3;
          ak1[s] = u1 ? ak1[s] + c1 * g : ak1[s];
          ak2[s] = u2 ? ak2[s] + c2 * g : ak2[s];
          ak3[s] = u3 ? ak3[s] + c3 * g : ak3[s];
          const int64_t b = b0 + s;   // st == 0: input y, the step is done
          const float gs0 = (st == 0 && b < B) ? a.grad_sol[((int64_t)step * B + b) * H + lane] : 0.f;
          lam[s] = st == 0 ? ay[s] + gs0 : lam[s];
        } else if (st == 3) {  // input y + dt ((k1 - k2) + k3)
          ak1[s] += dt * g;
          ak2[s] -= dt * g;
          ak3[s] += dt * g;
        } else if (st == 2) {  // input y + dt (k2 - k1 / 3)
          ak2[s] += dt * g;
          ak1[s] -= (dt * kThird) * g;
        } else if (st == 1) {  // input y + (dt k1) / 3
          ak1[s] += (dt * kThird) * g;
        } else {               // input y: the step is done
          const int64_t b = b0 + s;
          lam[s] = ay[s] + (b < B ? a.grad_sol[((int64_t)step * B + b) * H + lane] : 0.f);
        }
      }
    }
  }
  if (own) {
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (b0 + s < B) a.grad_h0[(b0 + s) * H + lane] = lam[s];
  }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
int g_spw = 0;  // forced samples per workgroup (0: by batch size)

bool drv_shape_ok(const fetode_ferro_t* fl) {
  if (!fl || fl->branch_sign) return false;
  const int D = fl->in_dim - fl->out_dim;
  return fl->out_dim >= 1 && fl->out_dim <= kDrvHMax && D >= 1 && D <= kDrvDMax && fl->num_basis >= 1 &&
         fl->num_basis <= kDrvKMax;
}

// Measured (profiles/driven_spw_sweep.log, forward at H = 64, K = 10, T = 96): a workgroup's time grows
// in proportion to its samples, so sharing a parameter read pays only once every CU holds two
// workgroups: one sample per workgroup up to B = 512, two up to 1024, four beyond.
int choose_spw(int64_t B) {
  if (g_spw) return g_spw;
  return B <= 512 ? 1 : (B <= 1024 ? 2 : 4);
}

// the kernel tables (fetode_driven.h): rows by samples per workgroup, tables by [TAPE or XG][GRID]
template <int S, bool TAPE, bool GRID>
constexpr DrvKRow<DrivenArgs> fixed_row() {
  return {driven_fixed_kernel<S, 10, TAPE, GRID>, driven_fixed_kernel<S, 12, TAPE, GRID>,
          driven_fixed_kernel<S, 0, TAPE, GRID>};
}
template <bool TAPE, bool GRID>
constexpr DrvSRows<DrivenArgs> fixed_rows() {
  return {fixed_row<1, TAPE, GRID>(), fixed_row<2, TAPE, GRID>(), fixed_row<4, TAPE, GRID>()};
}
template <int S, bool XG, bool GRID>
constexpr DrvKRow<DrivenAdjArgs> adj_row() {
  return {driven_adj_kernel<S, 10, XG, GRID>, driven_adj_kernel<S, 12, XG, GRID>, driven_adj_kernel<S, 0, XG, GRID>};
}
template <bool XG, bool GRID>
constexpr DrvSRows<DrivenAdjArgs> adj_rows() {
  return {adj_row<1, XG, GRID>(), adj_row<2, XG, GRID>(), adj_row<4, XG, GRID>()};
}
const DrvSRows<DrivenArgs> kFixed[2][2] = {{fixed_rows<false, false>(), fixed_rows<false, true>()},
                                           {fixed_rows<true, false>(), fixed_rows<true, true>()}};
const DrvSRows<DrivenAdjArgs> kAdj[2][2] = {{adj_rows<false, false>(), adj_rows<false, true>()},
                                            {adj_rows<true, false>(), adj_rows<true, true>()}};

// What a solve or sweep entry decides first, and the launch shape.  grd: the fetode_driven_grid entries
// (the four fixed-grid methods on a (n_steps, 4) coefficient array) instead of the fetode_driven_fixed
// ones (rk4, 3/8 rule, on dt); each family keeps its own order of status decisions (pinned by
// tests/test_driven_host.py and tests/test_driven_methods_host.py).  Here: shape, method, then the grid
// entries' 2^31 limits.
int driven_admit(bool grd, const fetode_ferro_t* fl, int32_t method, int64_t B, int32_t n_steps, int* spw,
                 int64_t* grid) {
  const char* who = grd ? "driven grid" : "driven";
  if (!drv_shape_ok(fl)) return set_err(FETODE_EUNSUPPORTED, "%s: shape outside the admitted family", who);
  if (!grd && method != FETODE_RK4) return set_err(FETODE_EUNSUPPORTED, "driven: only rk4 (3/8 rule) is fused");
  if (grd && drv_nm_log2(method) < 0)
    return set_err(FETODE_EUNSUPPORTED, "driven grid: method %d is not euler, midpoint, rk4 or rk4_classic", method);
  // the launch shape; a B <= 0 gets a harmless one here and is refused or accepted as empty by the caller
  *spw = choose_spw(B > 0 ? B : 1);
  *grid = B > 0 ? (B + *spw - 1) / *spw : 0;
  if (grd && (*grid > 0x7fffffff || (n_steps > 0 && ((int64_t)n_steps << drv_nm_log2(method)) > 0x7fffffff)))
    return set_err(FETODE_EUNSUPPORTED, "driven grid: batch or evaluation count beyond 2^31 - 1");
  return FETODE_OK;
}

// fixed: sizes, then OK when empty, then null pointers; grid: OK when empty, then the table's rows, then
// null pointers.  Every status is decided before a launch.
int driven_solve(bool grd, const fetode_ferro_t* fl, const void* plan, int32_t method, const float* h0, int64_t B,
                 const float* u, int64_t n_eval, int64_t eval0, const float* dt, int32_t n_steps, const float* prev0,
                 float* sol, float* prev_out, float* tape_hx, float* tape_phi, bool tape, void* stream) {
  const char* who = grd ? "driven grid" : "driven";
  int spw = 1;
  int64_t grid = 0;
  const int rc = driven_admit(grd, fl, method, B, n_steps, &spw, &grid);
  if (rc != FETODE_OK) return rc;
  const int sh = grd ? drv_nm_log2(method) : 2;
  const bool empty = B <= 0 || n_steps <= 0;
  const bool rows = eval0 < 0 || eval0 + (int64_t)n_steps * (1 << sh) > n_eval;
  // fixed: bad sizes are refused before an empty solve is accepted
  const bool sizes = !grd && (B < 0 || n_steps < 0 || rows);
  // grid: an empty solve is accepted first (driven_admit has held B and the evaluation count below 2^31)
  const bool grid_rows = grd && !empty && rows;
  if (sizes || grid_rows)
    return set_err(FETODE_EINVAL, "%s: evaluations %lld + %d * %d exceed the table's %lld rows", who, (long long)eval0,
                   1 << sh, n_steps, (long long)n_eval);
  if (empty) return FETODE_OK;
  if (!plan || !h0 || !u || !dt || !sol || (tape && (!tape_hx || !tape_phi)))
    return set_err(FETODE_EINVAL, "%s: null pointer", who);
  // fixed only: the grid entries were refused for this in driven_admit, before their empty and row checks
  if (grid > 0x7fffffff) return set_err(FETODE_EUNSUPPORTED, "driven: batch too large");
  DrivenArgs a{};
  a.plan = (const float*)plan;
  a.h0 = h0; a.u = u; a.dt = dt; a.prev0 = prev0; a.sol = sol; a.prev_out = prev_out;
  a.tape_hx = tape_hx; a.tape_phi = tape_phi;
  a.B = B; a.eval0 = eval0; a.n_steps = n_steps;
  drv_fill_field(a, fl);
  if (grd) {
    a.method = method;
    a.nm_log2 = sh;
  }
  drv_launch(kFixed[tape][grd].at(spw), a.K, dim3((unsigned)grid), kDrvThreads, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return FETODE_OK;
}

// fixed: sizes, then OK for an empty batch (no steps: grad_h0 = grad_sol[0] is still written), then null
// pointers; grid: OK when empty, then null pointers.
int driven_backward(bool grd, const fetode_ferro_t* basis, const void* plan, int32_t method, int64_t B, const float* dt,
                    int32_t n_steps, const float* prev0, const float* tape_hx, const float* tape_phi,
                    const float* grad_sol, float* adj, float* grad_h0, float* adj_u, bool xg, void* stream) {
  int spw = 1;
  int64_t grid = 0;
  const int rc = driven_admit(grd, basis, method, B, n_steps, &spw, &grid);
  if (rc != FETODE_OK) return rc;
  if (!grd && (B < 0 || n_steps < 0)) return set_err(FETODE_EINVAL, "driven backward: bad sizes");
  if (grd ? (B <= 0 || n_steps <= 0) : B == 0) return FETODE_OK;
  if (!plan || !dt || !tape_hx || !tape_phi || !grad_sol || !adj || !grad_h0 || (xg && !adj_u))
    return set_err(FETODE_EINVAL, "%s backward: null pointer", grd ? "driven grid" : "driven");
  // fixed only, as in driven_solve
  if (grid > 0x7fffffff) return set_err(FETODE_EUNSUPPORTED, "driven: batch too large");
  DrivenAdjArgs a{};
  a.plan = (const float*)plan;
  a.dt = dt; a.prev0 = prev0; a.tape_hx = tape_hx; a.tape_phi = tape_phi; a.grad_sol = grad_sol;
  a.adj = adj; a.grad_h0 = grad_h0; a.adj_u = adj_u;
  a.B = B; a.n_steps = n_steps;
  drv_fill_field(a, basis);
  if (grd) {
    a.method = method;
    a.nm_log2 = drv_nm_log2(method);
  }
  drv_launch(kAdj[xg][grd].at(spw), a.K, dim3((unsigned)grid), kDrvThreads, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return FETODE_OK;
}

}  // namespace

extern "C" {

int fetode_driven_supported(const fetode_ferro_t* basis) { return drv_shape_ok(basis) ? 1 : 0; }

int fetode_driven_set_spw(int spw) {
  const int prev = g_spw;
  if (spw == 0 || spw == 1 || spw == 2 || spw == 4) g_spw = spw;
  return prev;
}

int64_t fetode_driven_plan_bytes(const fetode_ferro_t* basis) {
  if (!drv_shape_ok(basis)) {
    set_err(FETODE_EUNSUPPORTED, "driven: shape outside the admitted family");
    return -1;
  }
  return (int64_t)sizeof(float) * drv_plan_floats(basis->in_dim, basis->out_dim, basis->num_basis);
}

int fetode_driven_plan_build(const fetode_ferro_t* basis, const float* gain, const float* bias, void* plan,
                             void* stream) {
  if (!drv_shape_ok(basis)) return set_err(FETODE_EUNSUPPORTED, "driven: shape outside the admitted family");
  if (!basis->k || !basis->Ec || !basis->Ps || !basis->bias || !basis->coef || !gain || !bias || !plan)
    return set_err(FETODE_EINVAL, "driven plan: null pointer");
  const int64_t ne = drv_plan_elems(basis->in_dim, basis->out_dim, basis->num_basis);
  hipLaunchKernelGGL(driven_plan_kernel, dim3(nblk(ne, 256)), dim3(256), 0, (hipStream_t)stream, *basis, gain, bias,
                     (float*)plan);
  LAUNCH_CHECK();
  return FETODE_OK;
}

int fetode_driven_table(const float* tq, int64_t n_eval, const float* t_grid, int32_t T, const float* x, int64_t B,
                        int32_t D, float* u, void* stream) {
  if (n_eval < 0 || B < 0 || T < 2 || D < 1) return set_err(FETODE_EINVAL, "driven table: bad sizes");
  const int64_t n = n_eval * B * D;
  if (n == 0) return FETODE_OK;
  if (!tq || !t_grid || !x || !u) return set_err(FETODE_EINVAL, "driven table: null pointer");
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(driven_table_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     (hipStream_t)stream, tq, n_eval, t_grid, T, x, B, D, u);
  LAUNCH_CHECK();
  return FETODE_OK;
}

int fetode_driven_fixed(const fetode_ferro_t* basis, const void* plan, int32_t method, const float* h0, int64_t B,
                        const float* u, int64_t n_eval, int64_t eval0, const float* dt, int32_t n_steps,
                        const float* prev0, float* sol, float* prev_out, void* stream) {
  return driven_solve(false, basis, plan, method, h0, B, u, n_eval, eval0, dt, n_steps, prev0, sol, prev_out, nullptr,
                      nullptr, false, stream);
}

int fetode_driven_fixed_tape(const fetode_ferro_t* basis, const void* plan, int32_t method, const float* h0, int64_t B,
                             const float* u, int64_t n_eval, int64_t eval0, const float* dt, int32_t n_steps,
                             const float* prev0, float* sol, float* prev_out, float* tape_hx, float* tape_phi,
                             void* stream) {
  return driven_solve(false, basis, plan, method, h0, B, u, n_eval, eval0, dt, n_steps, prev0, sol, prev_out, tape_hx,
                      tape_phi, true, stream);
}

int fetode_driven_fixed_backward(const fetode_ferro_t* basis, const void* plan, int32_t method, int64_t B,
                                 const float* dt, int32_t n_steps, const float* prev0, const float* tape_hx,
                                 const float* tape_phi, const float* grad_sol, float* adj, float* grad_h0,
                                 void* stream) {
  return driven_backward(false, basis, plan, method, B, dt, n_steps, prev0, tape_hx, tape_phi, grad_sol, adj, grad_h0, nullptr,
                         false, stream);
}

int fetode_driven_fixed_backward_x(const fetode_ferro_t* basis, const void* plan, int32_t method, int64_t B,
                                   const float* dt, int32_t n_steps, const float* prev0, const float* tape_hx,
                                   const float* tape_phi, const float* grad_sol, float* adj, float* grad_h0,
                                   float* adj_u, void* stream) {
  return driven_backward(false, basis, plan, method, B, dt, n_steps, prev0, tape_hx, tape_phi, grad_sol, adj, grad_h0, adj_u,
                         true, stream);
}

int fetode_driven_grid(const fetode_ferro_t* basis, const void* plan, int32_t method, const float* h0, int64_t B,
                       const float* u, int64_t n_eval, int64_t eval0, const float* coef, int32_t n_steps,
                       const float* prev0, float* sol, float* prev_out, void* stream) {
  return driven_solve(true, basis, plan, method, h0, B, u, n_eval, eval0, coef, n_steps, prev0, sol, prev_out, nullptr,
                     nullptr, false, stream);
}

int fetode_driven_grid_tape(const fetode_ferro_t* basis, const void* plan, int32_t method, const float* h0, int64_t B,
                            const float* u, int64_t n_eval, int64_t eval0, const float* coef, int32_t n_steps,
                            const float* prev0, float* sol, float* prev_out, float* tape_hx, float* tape_phi,
                            void* stream) {
  return driven_solve(true, basis, plan, method, h0, B, u, n_eval, eval0, coef, n_steps, prev0, sol, prev_out, tape_hx,
                     tape_phi, true, stream);
}

int fetode_driven_grid_backward(const fetode_ferro_t* basis, const void* plan, int32_t method, int64_t B,
                                const float* coef, int32_t n_steps, const float* prev0, const float* tape_hx,
                                const float* tape_phi, const float* grad_sol, float* adj, float* grad_h0,
                                void* stream) {
  return driven_backward(true, basis, plan, method, B, coef, n_steps, prev0, tape_hx, tape_phi, grad_sol, adj, grad_h0,
                              nullptr, false, stream);
}

int fetode_driven_grid_backward_x(const fetode_ferro_t* basis, const void* plan, int32_t method, int64_t B,
                                  const float* coef, int32_t n_steps, const float* prev0, const float* tape_hx,
                                  const float* tape_phi, const float* grad_sol, float* adj, float* grad_h0,
                                  float* adj_u, void* stream) {
  return driven_backward(true, basis, plan, method, B, coef, n_steps, prev0, tape_hx, tape_phi, grad_sol, adj, grad_h0,
                              adj_u, true, stream);
}

int64_t fetode_driven_table_backward_workspace(int64_t B, int64_t n_ev) {
  (void)B;
  (void)n_ev;
  return 0;  // the gather keeps its (interval, weight) pairs in LDS
}

int fetode_driven_table_backward(const float* tq, int64_t tq_stride_b, const float* t_grid, int32_t T,
                                 const float* adj_u, int64_t B, int64_t n_ev, int64_t stride_b, int64_t stride_e,
                                 const int32_t* nfev, int64_t nfev_stride, int32_t D, float* grad_x, void* workspace,
                                 void* stream) {
  (void)workspace;
  if (T < 2 || D < 1) return set_err(FETODE_EINVAL, "driven table backward: bad sizes (T=%d, D=%d)", T, D);
  if (B <= 0 || n_ev <= 0) return FETODE_OK;
  if (!tq || !t_grid || !adj_u || !grad_x) return set_err(FETODE_EINVAL, "driven table backward: null pointer");
  if (tq_stride_b < 0 || stride_b < 1 || stride_e < 1 || (nfev && nfev_stride < 1))
    return set_err(FETODE_EINVAL, "driven table backward: strides must be positive (tq_stride_b: not negative)");
  const int64_t chunks = ((int64_t)T * D + kTbThreads - 1) / kTbThreads;
  if (B > 0x7fffffff || chunks > 65535) return set_err(FETODE_EUNSUPPORTED, "driven table backward: too large");
  DrivenTbArgs a{};
  a.tq = tq; a.tg = t_grid; a.adj_u = adj_u; a.nfev = nfev; a.gx = grad_x;
  a.B = B; a.n_ev = n_ev; a.tq_stride_b = tq_stride_b; a.stride_b = stride_b; a.stride_e = stride_e;
  a.nfev_stride = nfev_stride; a.T = T; a.D = D;
  hipLaunchKernelGGL(driven_table_bwd_kernel, dim3((unsigned)B, (unsigned)chunks), dim3(kTbThreads), 0,
                     (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return FETODE_OK;
}

}  // extern "C"
