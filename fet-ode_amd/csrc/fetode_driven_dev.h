// fetode_driven_dev.h — the device arithmetic of the input-driven Ferro field
//     dh/dt = tanh(Ferro_{(H+D)->H}(cat[h, x(t)])) * gain + bias
// written once for every kernel of the family (fetode_driven.hip, fetode_driven_dopri5_body.h,
// fetode_driven_dopri5_bwd.hip, fetode_driven_pgrad.hip): the gate, an evaluation's element loop and the
// meeting of its partial sums, the evaluation's VJP, the interpolator's locate step and the wave sums.
// The bitwise tests between the solvers hold because these are the same statements, not copies kept in
// step; a new variant of the field includes this header.
// Mapping of every function here: 256 threads = 4 waves, lane -> output o (lanes >= H idle), wave wv ->
// inputs i = wv (mod 4), S samples per workgroup.  None of them holds a barrier: those stay at the callers.
#pragma once
#include "fetode_common.h"
#include "fetode_driven.h"

namespace fetode {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// the butterfly gives every lane the same bits: each level adds the same two values on both sides
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// An input of an evaluation as the element loops read it: the value, its gate u = sigma(gs(x - prev))
// against the previous evaluation's input (prev <- hx, call order) and the per-input factors
// gx = gs log2e x, v = -2(1-alpha)(1-u).
struct DrvGate {
  float x, gx, v, u;
};
__device__ __forceinline__ DrvGate drv_gate(float gs, float gsl2e, float wc, float x, float prev) {
  const float up = 1.0f / (1.0f + expf(-(gs * (x - prev))));
  return {x, gsl2e * x, wc * (1.0f - up), up};
}

// One element (i, k, o) of the plan on one input: th = tanh(k (x + Ec m)), m = 1 + v cn,
// cn = sigma(gs(-x - Ec)) (the VJP reads it too).
__device__ __forceinline__ float drv_elem(const float4 c, float x, float gx, float v, float& cn) {
  cn = rcp(1.0f + ex2(gx + c.x));
  const float m = ffma(v, cn, 1.0f);
  const float z = ffma(c.z, m, c.y * x);               // 2 log2e k (x + Ec m)
  return ffma(rcp(1.0f + ex2(z)), -2.0f, 1.0f);
}

// A wave's partial sums of one evaluation of S samples: every lane sums the K bases of one input first,
// then its inputs i = wv, wv + 4, ....  KT > 0: K at compile time.
template <int S, int KT>
__device__ __forceinline__ void drv_eval_partial(const float4* el, int H, int In, int K, int lane, int wv,
                                                 const float (&xs)[S][kDrvInMax], const float (&gxs)[S][kDrvInMax],
                                                 const float (&vs)[S][kDrvInMax], float (&acc)[S]) {
#pragma unroll
  for (int s = 0; s < S; ++s) acc[s] = 0.f;
  if (lane < H) {
    for (int i = wv; i < In; i += 4) {
      float x[S], gx[S], v[S], ai[S];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        x[s] = xs[s][i];
        gx[s] = gxs[s][i];
        v[s] = vs[s][i];
        ai[s] = 0.f;
      }
      const float4* __restrict__ p = el + (int64_t)i * K * H + lane;
#pragma unroll KT > 0 ? KT : 1
      for (int k = 0; k < K; ++k) {
        const float4 c = p[(int64_t)k * H];
#pragma unroll
        for (int s = 0; s < S; ++s) {
          float cn;
          ai[s] = ffma(c.w, drv_elem(c, x[s], gx[s], v[s], cn), ai[s]);
        }
      }
#pragma unroll
      for (int s = 0; s < S; ++s) acc[s] += ai[s];
    }
  }
}

// The four waves' partial sums of output `lane` of sample s meet in a fixed order: the pre-activation phi.
template <int S>
__device__ __forceinline__ float drv_eval_meet(const float (&part)[4][S][64], int s, int lane, float fcon) {
  return ((part[0][s][lane] + part[1][s][lane]) + (part[2][s][lane] + part[3][s][lane])) + fcon;
}

// The VJP term of one element: d + d(coef Ps th)/dx, the gate's x differentiated (u its gate), prev
// detached; c.y and c.z carry 2 log2e, which the sweeps take out of the wave's sum.  The loop over the inputs stays
// at the two sweeps (driven_adj_kernel, driven_dopri5_adj_kernel): as one inlined function it changed
// the S = 2 and 4 sweeps' register allocation.
__device__ __forceinline__ float drv_elem_vjp(const float4 c, float x, float gx, float v, float u, float gs, float d) {
  float cn;
  const float th = drv_elem(c, x, gx, v, cn);
  // d m / d x = -wc gs cn (1 - u) ((1 - cn) + u)
  const float dm = -(v * gs) * (cn * ((1.0f - cn) + u));
  return ffma(c.w * ffma(-th, th, 1.0f), ffma(c.z, dm, c.y), d);
}

// LinearInterp1D's locate step (compare_noise_ecg.py:861-872) in its fp32 expression: the query clamped
// to [lo, hi] = [tg[0], tg[T - 1]], searchsorted left as the count #{grid < t}, .clamp(1, T - 1); returns
// the interval's right knot i, and through w the weight of knot i (1 - w: of knot i - 1).
__device__ __forceinline__ int drv_locate(const float* __restrict__ tg, int T, float lo, float hi, float t, float& w) {
  t = t < lo ? lo : (t > hi ? hi : t);                 // torch.clamp(t, t[0], t[-1])
  int i = 0;                                           // searchsorted, left: #{grid < t}
  for (int j = 0; j < T; ++j) i += tg[j] < t ? 1 : 0;
  i = i < 1 ? 1 : (i > T - 1 ? T - 1 : i);             // .clamp(1, T - 1)
  const float t0 = tg[i - 1], t1 = tg[i];
  w = (t - t0) / ((t1 - t0) + 1e-12f);
  return i;
}

}  // namespace fetode
