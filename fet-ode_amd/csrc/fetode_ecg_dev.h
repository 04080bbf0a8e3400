// fetode_ecg_dev.h — device pieces shared by the ECG field's kernels (fetode_ecg.hip: the mixer,
// its VJP and the resident dopri5 solve; fetode_ecg_bwd.hip: the solve's resident reverse sweep):
// the hysteretic logistic element (train_ecg_kan_fet_nn_ode.py:110-121) with its derivatives, the
// head's summation order, and the bounded XCD-hierarchical grid barrier.
#pragma once
#include "fetode_common.h"

namespace {

struct HL {  // device copy of fetode_hlogistic_t
  int in, nb;
  const float *k, *Ec, *Ps, *bias;
  float gs, bp;
};

__device__ __forceinline__ float ref_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }
__device__ __forceinline__ float fast_sigmoid(float z) { return fetode::rcp(1.0f + fetode::ex2(-z * FETODE_LOG2E)); }

// The head's fp32 summation order, shared by every kernel that evaluates it: q in [0, F) splits
// into kHeadParts = 32 consecutive parts of head_part(F) (a multiple of 4) indices; each part P_p
// is an FMA chain from 0 in increasing q; groups of four add as S_w = (P_4w + P_4w+1) +
// (P_4w+2 + P_4w+3), and the eight S_w add left to right.  (The resident dopri5 gives each wave
// one group, a quarter-wave per part, and combines a group with two lane shuffles.)
constexpr int kHeadParts = 32;
constexpr int kHeadGroups = kHeadParts / 4;
__host__ __device__ __forceinline__ int head_part(int F) { return (((F + 3) & ~3) + 4 * kHeadParts - 1) / (4 * kHeadParts) * 4; }

// the reference's up / down / gate for element (i, j) at input x (train_ecg_kan_fet_nn_ode.py:110-121)
struct HPoint {
  float su, sd, bs, basis;
};
__device__ __forceinline__ HPoint hpoint(const HL& L, float x, float pv, int q) {
  HPoint p;
  const float k = L.k[q], Ec = L.Ec[q], Ps = L.Ps[q];
  p.su = 1.0f / (1.0f + expf(-k * (x - Ec)));
  p.sd = 1.0f / (1.0f + expf(-k * (x + Ec)));
  const float up = Ps * p.su * 2.0f - Ps;
  const float down = Ps * p.sd * 2.0f - Ps;
  const float g = ref_sigmoid(L.gs * (x - pv));
  p.bs = g > L.bp ? 1.0f : 0.0f;
  p.basis = p.bs * up + (1.0f - p.bs) * down + L.bias[q];
  return p;
}

// derivative pieces of element (b, i, j): d basis / d (x, k, Ec, Ps), gb = d loss / d basis
struct HGrad {
  float gb, dx, dk, dEc, dPs;
};
__device__ __forceinline__ HGrad hgrad(const HL& L, float x, float pv, int q, float gphi, float phi, int act_sigmoid) {
  const HPoint p = hpoint(L, x, pv, q);
  HGrad r;
  r.gb = act_sigmoid ? gphi * (phi * (1.0f - phi)) : gphi;
  const float k = L.k[q], Ec = L.Ec[q], Ps = L.Ps[q];
  const float cu = p.bs * 2.0f * Ps * p.su * (1.0f - p.su);          // d up / d z_up    (z = k (x - Ec))
  const float cd = (1.0f - p.bs) * 2.0f * Ps * p.sd * (1.0f - p.sd);  // d down / d z_down (z = k (x + Ec))
  r.dx = (cu + cd) * k;
  r.dk = cu * (x - Ec) + cd * (x + Ec);
  r.dEc = (cd - cu) * k;
  r.dPs = p.bs * (2.0f * p.su - 1.0f) + (1.0f - p.bs) * (2.0f * p.sd - 1.0f);
  return r;
}

// One element of the RESIDENT solve's evaluation, as ecg_dopri5_kernel rounds it: the smooth
// logistics on v_exp / v_rcp, the hard gate in the reference's rounding (expf, IEEE division) — the
// branch is the forward's bit for bit given the same x and prev.  phi = sigmoid(basis); the d's are
// hgrad's formulas on these values.
struct RPoint {
  float phi, dx, dk, dEc, dPs;
};
__device__ __forceinline__ RPoint rpoint(float4 pr, float gs, float bp, float x, float pv) {
  const float k = pr.x, Ec = pr.y, Ps = pr.z;
  const float su = fast_sigmoid(k * (x - Ec));
  const float sd = fast_sigmoid(k * (x + Ec));
  const float up = Ps * su * 2.0f - Ps;
  const float down = Ps * sd * 2.0f - Ps;
  const float bs = ref_sigmoid(gs * (x - pv)) > bp ? 1.0f : 0.0f;
  RPoint r;
  r.phi = fast_sigmoid(bs * up + (1.0f - bs) * down + pr.w);
  const float cu = bs * 2.0f * Ps * su * (1.0f - su);
  const float cd = (1.0f - bs) * 2.0f * Ps * sd * (1.0f - sd);
  r.dx = (cu + cd) * k;
  r.dk = cu * (x - Ec) + cd * (x + Ec);
  r.dEc = (cd - cu) * k;
  r.dPs = bs * (2.0f * su - 1.0f) + (1.0f - bs) * (2.0f * sd - 1.0f);
  return r;
}

inline int check_layer(const fetode_hlogistic_t* l) {
  if (!l || l->in_dim <= 0 || l->num_basis <= 0) return ::fetode::set_err(FETODE_EINVAL, "hlogistic: bad dims");
  if (!l->k || !l->Ec || !l->Ps || !l->bias) return ::fetode::set_err(FETODE_EINVAL, "hlogistic: null parameter");
  return FETODE_OK;
}

inline HL to_dev(const fetode_hlogistic_t* l) {
  HL L;
  L.in = l->in_dim;
  L.nb = l->num_basis;
  L.k = l->k;
  L.Ec = l->Ec;
  L.Ps = l->Ps;
  L.bias = l->bias;
  // gate_slope * dx with gate_slope a Python float: torch scales an fp32 tensor by it in fp32
  L.gs = (float)l->gate_slope;
  L.bp = (float)l->breaking_point;
  return L;
}

constexpr int kMaxF = 768;  // in * num_basis (in <= 64, num_basis <= 12)

struct DopriTab {
  float beta[6][6];  // torchdiffeq Dopri5 tableau rounded to fp32 (tableau.to(y0.dtype))
  float cerr[7];
  float cmid[7];
};

// Grid barrier, XCD-hierarchical (MI355X_MICROARCH.md "barrier-xcd"): workgroup i runs on XCD
// i % 8, so each XCD's workgroups arrive on their own counter (256 B apart); the last arriver of an
// XCD arrives on the top counter, the last of those bumps the generation every workgroup polls.
// The only data shared across workgroups (the partial slots) moves through agent-scope atomics,
// coherent across the XCDs' L2s by themselves, so the ordering needed is a vector-memory wait
// before arriving and after the poll — not agent-scope fences, which would also write back and
// invalidate the whole L2 (buffer_wbl2 / buffer_inv sc1) at every barrier (fetode_fused.hip
// dp_order).  Counters reset themselves; the words are zeroed once per launch.
constexpr int kBarWords = 64 * 10;  // 8 XCD counters, top counter, generation (256 B each)
// Every spin is bounded (MI355X_MICROARCH.md: a stranded workgroup must not hang the device): after
// 2^20 polls (about a second) the barrier gives up and raises the abort word 64*9+1.  Once that word
// is set every barrier returns at once (entering or spinning) and reports it: the solver then stops
// (status 4) instead of running on with counters that were never reset.
constexpr unsigned kSpinLimit = 1u << 20;
__device__ bool grid_barrier(unsigned* bar, unsigned nblk) {
  __shared__ int s_abort;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned x = blockIdx.x & 7u;
    const unsigned nx = (nblk + 7u - x) / 8u, nxcd = nblk < 8u ? nblk : 8u;
    unsigned* cnt = bar + 64 * x;
    unsigned* top = bar + 64 * 8;
    unsigned* gen = bar + 64 * 9;
    unsigned* abort_word = gen + 1;
    int ab = __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    if (!ab) {
      const unsigned g = __hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the slot stores have landed
      if (__hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nx - 1u) {
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // reset lands before the release
        if (__hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nxcd - 1u) {
          __hip_atomic_store(top, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __hip_atomic_fetch_add(gen, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      unsigned spins = 0;
      while (__hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g) {
        __builtin_amdgcn_s_sleep(1);
        if (__hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
          ab = 1;
          break;
        }
        if (++spins == kSpinLimit) {
          __hip_atomic_store(abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ab = 1;
          break;
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_abort = ab;
  }
  __syncthreads();
  return s_abort != 0;
}

}  // namespace
