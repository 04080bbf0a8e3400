// fetode_bwd_dev.h — the device building blocks of the reverse sweeps (layer shapes, LDS tables,
// per-lane gradient sums, the per-evaluation VJP jobs) and the sweeps' kernel arguments, shared by
// fetode_bwd.hip and fetode_bwd_mp.hip.  Device code; included inside each file's anonymous
// namespace, after fetode_gridsum.h.
#pragma once
constexpr int kSO = 3;  // spline order of the fused kernels (efficientkan default)
// FETODE_EXP_SKIP (phase-cost attribution: 1 Ferro, 2 edges, 4 logistic, 8 features, 16 d/dx
// reductions compiled out — results are wrong when set) exists only in the diagnostic build
// (make diag EXTRA=-DFETODE_EXP_SKIP=n); the product library is always built with 0.
#if defined(FETODE_EXP_SKIP) && !defined(FETODE_DIAG)
#error "FETODE_EXP_SKIP is a diagnostic knob: build it with make diag"
#endif
#ifndef FETODE_EXP_SKIP
#define FETODE_EXP_SKIP 0
#endif

typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pfma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 splat(float v) { return f2{v, v}; }
__device__ __forceinline__ f2 ex2x2(f2 v) { return f2{ex2(v.x), ex2(v.y)}; }
__device__ __forceinline__ f2 rcpx2(f2 v) { return f2{rcp(v.x), rcp(v.y)}; }

constexpr int pow2_floor(int v) {
  int p = 1;
  while (p * 2 <= v) p *= 2;
  return p;
}

// Layout of one layer's gradient sums in a partial row (host and device agree on it).
struct AccLayout {
  int E, NE, NL, NS, NTM;
  int oA, oC, oE, oG, oBase, oSpl, oLw, oLa, oLb, n;
};
__host__ __device__ constexpr AccLayout acc_layout(int in, int out, int K, int NB, int NS, bool ferro) {
  AccLayout L{};
  L.E = ferro ? in * out * K : 0;
  L.NE = in * out;
  L.NL = in * NB;
  L.NS = NS;
  L.NTM = (ferro ? out * K : 0) + out + NB;
  L.oA = 0;
  L.oC = L.E;
  L.oE = 2 * L.E;
  L.oG = 3 * L.E;
  L.oBase = L.oG + (ferro ? out : 0);
  L.oSpl = L.oBase + L.NE;
  L.oLw = L.oSpl + L.NE * NS;
  L.oLa = L.oLw + out * L.NL;
  L.oLb = L.oLa + L.NL;
  L.n = L.oLb + L.NL;
  return L;
}

template <int IN_, int OUT_, int K_, int NB_, int NG_, bool FERRO_>
struct BL {  // compile-time shape of one layer
  static constexpr int IN = IN_, OUT = OUT_, K = FERRO_ ? K_ : 0, NB = NB_, NG = NG_;
  static constexpr bool FERRO = FERRO_;
  static constexpr int NI = NG - 1, NS = NG - 1 - kSO, NFL = 1 + NB;
  static constexpr AccLayout AL = acc_layout(IN, OUT, K, NB, NS, FERRO);
  static constexpr int E = AL.E, NE = AL.NE, NL = AL.NL, NTM = AL.NTM;
  static constexpr int RF = (E + 63) / 64, RE = (NE + 63) / 64, RL = (NL + 63) / 64;
  static constexpr int RF1 = RF > 0 ? RF : 1, RL1 = RL > 0 ? RL : 1;
  static constexpr int EP = E / 2, RP = (EP + 63) / 64, RP1 = RP > 0 ? RP : 1;  // Ferro element pairs (k, k+1)
  static_assert(K % 2 == 0, "Ferro elements are walked in (k, k+1) pairs");
  static constexpr int LPI = pow2_floor(64 / IN);  // lanes per input in the d/dx segmented sum
  // cb row pitch: NTM rounded up to LPI mod 32, so the LPI-lane groups of one half-wave read
  // distinct LDS banks in reduce_gin (a pitch of 32 put all ten inputs of layer 1 on banks 0-3)
  // (extra padding of 4 / 12 / 16 floats measured within 1 %: the pitch is not a lever)
  static constexpr int NTMP = LPI >= 32 ? NTM : NTM + ((LPI - NTM % 32) % 32 + 32) % 32;
  static_assert(IN <= 64 && OUT <= 64, "layer widths up to 64");
  static_assert(NS >= 1, "grid too small for cubic splines");
};

// Per-block LDS tables of the whole field.  Per-INPUT tables are laid out over the combined input
// index t in [0, W): t < D are layer-0 inputs, t >= D layer-1 inputs (same knot count), so the
// feature phase is one code path for both layers.
template <int W, int NG, int NB>
struct BInTab {
  static constexpr int NI = NG - 1;
  // basis B_{m-3+r} on interval m as a cubic in u: [t][m][r] (power basis); one float4 of
  // padding per input so that lanes gathering different inputs' rows spread over the LDS banks
  static constexpr int BPS = NI * 4 + 1;
  float4 bp[W * BPS];
  __device__ static int bpi(int t, int m) { return t * BPS + m * 4; }
  float knots[W * NG];
  float rh[W * NI];       // 1/(g[m+1] - g[m])
  __attribute__((aligned(8))) float lg[NB > 0 ? 2 * W * NB : 1];  // (-a log2e, a b log2e) per (t, j)

  __device__ void stage(const float* __restrict__ plan, const LayerPlan& P0, const LayerPlan& P1, int D, int tid,
                        int nt) {
    for (int q = tid; q < W * NG; q += nt) {
      const int t = q / NG, j = q % NG;
      knots[q] = t < D ? plan[P0.knots + t * NG + j] : plan[P1.knots + (t - D) * NG + j];
    }
    for (int q = tid; q < W * NI; q += nt) {
      const int t = q / NI, m = q % NI;
      rh[q] = t < D ? plan[P0.rh + t * NI + m] : plan[P1.rh + (t - D) * NI + m];
    }
    for (int q = tid; q < 2 * W * NB; q += nt)
      lg[q] = q < 2 * D * NB ? plan[P0.lg + q] : plan[P1.lg + (q - 2 * D * NB)];
    // basis polynomials: Cox-de Boor (efficientkan.py:117-131) restricted to interval m, in
    // fp64 at u = 0, 1/3, 2/3, 1, converted to the power basis (exact for cubics)
    for (int q = tid; q < W * NI; q += nt) {
      const int t = q / NI, m = q % NI;
      const float* g = t < D ? plan + P0.knots + t * NG : plan + P1.knots + (t - D) * NG;
      const double h = (double)g[m + 1] - g[m];
      double v[4][kSO + 2];
      for (int s = 0; s < 4; ++s) {
        const double x = g[m] + h * (s / 3.0);
        double* N = v[s];
        for (int r = 0; r < kSO + 2; ++r) N[r] = 0.0;
        N[kSO] = 1.0;
        for (int k = 1; k <= kSO; ++k) {
          double M[kSO + 2];
          for (int r = 0; r < kSO + 2; ++r) M[r] = 0.0;
          for (int r = kSO - k; r <= kSO; ++r) {
            const int j = m - kSO + r;
            if (j >= 0 && j <= NG - 2 - k) {
              const double left = (x - g[j]) / ((double)g[j + k] - g[j]) * N[r];
              const double right = ((double)g[j + k + 1] - x) / ((double)g[j + k + 1] - g[j + 1]) * N[r + 1];
              M[r] = left + right;
            }
          }
          for (int r = 0; r < kSO + 2; ++r) N[r] = M[r];
        }
      }
      for (int r = 0; r <= kSO; ++r) {
        const double a0 = v[0][r], a1 = v[1][r], a2 = v[2][r], a3 = v[3][r];
        bp[bpi(t, m) + r] = make_float4((float)a0, (float)((-11.0 * a0 + 18.0 * a1 - 9.0 * a2 + 2.0 * a3) / 2.0),
                                    (float)(9.0 * (2.0 * a0 - 5.0 * a1 + 4.0 * a2 - a3) / 2.0),
                                    (float)(9.0 * (-a0 + 3.0 * a1 - 3.0 * a2 + a3) / 2.0));
      }
    }
  }
};

template <class L>
struct BTab {  // per-block LDS copy of one layer's edge tables
  // spline edge (o, i) as a cubic in u per interval (NI + 1 rows: the last is the zero row), rows
  // of one edge padded to SPS float4s (lanes gather different edges: spread over the banks)
  static constexpr int SPS = L::NI + 2;
  float4 sp[L::OUT * L::IN * SPS];
  float kw[L::OUT * L::IN * L::NFL];        // SiLU weight, 2 * scaled logistic weights
  float pa[L::NL > 0 ? L::NL : 1], pb[L::NL > 0 ? L::NL : 1];
  // Ferro element pair p = elements (2p, 2p + 1) = (i, o, k..k+1):
  //   fpa = (Ec, Ec', 2 log2e k, 2 log2e k'),  fpb = (coef Ps k, coef' Ps' k', gs log2e Ec, gs log2e Ec')
  float4 fpa[L::EP > 0 ? L::EP : 1], fpb[L::EP > 0 ? L::EP : 1];

  __device__ void stage(const fetode_kanlinear_t& kl, const fetode_ferro_t& fl, const float* __restrict__ plan,
                        const LayerPlan& P, int tid, int nt) {
    const float gl = L::FERRO ? P.gsl2e : 0.f, k2 = 2.0f * FETODE_LOG2E;
    for (int p = tid; p < L::EP; p += nt) {
      const int e = 2 * p;
      fpa[p] = make_float4(fl.Ec[e], fl.Ec[e + 1], k2 * fl.k[e], k2 * fl.k[e + 1]);
      fpb[p] = make_float4((fl.coef[e] * fl.Ps[e]) * fl.k[e], (fl.coef[e + 1] * fl.Ps[e + 1]) * fl.k[e + 1],
                           gl * fl.Ec[e], gl * fl.Ec[e + 1]);
    }
    const float4* src = reinterpret_cast<const float4*>(plan + P.sp);
    for (int q = tid; q < L::OUT * L::IN * (L::NI + 1); q += nt) sp[q / (L::NI + 1) * SPS + q % (L::NI + 1)] = src[q];
    for (int q = tid; q < L::OUT * L::IN * L::NFL; q += nt) kw[q] = plan[P.kw + q];
    for (int q = tid; q < L::NL; q += nt) {
      pa[q] = kl.logistic_a[q];
      pb[q] = kl.logistic_b[q];
    }
  }
};

template <int W, int NS, int NB, bool WIN = false>
struct BFeat {  // per-wave LDS features of both layers' inputs, combined index t
  // dense B-spline row of input t at bd[t * BDP + BD0 + c].  WIN: the interval's four bases are
  // written at c = m - 3 .. m into a filled row, so the rows carry kSO guard floats on either side
  // (BD0 keeps the data 16-byte aligned; BDP = 4 mod 8 spreads the inputs over the banks); without
  // WIN (the adjoint-only sweep, whose 4 waves per SIMD leave no LDS for guards) the row is dense
  static constexpr bool WINDOW = WIN;
  static constexpr int BD0 = WIN ? 4 : 0;
  static constexpr int BDP0 = (BD0 + NS + kSO + 3) / 4 * 4;
  static constexpr int BDP = !WIN ? NS : BDP0 % 8 == 0 ? BDP0 + 4 : BDP0;
  __device__ static int bdi(int t, int c) { return t * BDP + BD0 + c; }
  float4 g4[W];  // Ferro per-input terms: x, gate up, wo = wc (1 - up), -ln2 wo
  float x[W], pv[W], silu[W], dsilu[W], u[W], rhm[W];  // rhm: 1 / (knot step) of x's interval
  int m[W];
  __attribute__((aligned(16))) float bd[W * BDP];
  float sg[NB > 0 ? W * NB : 1];
};

template <class L>
struct BReg {  // per-lane register slice of one layer: its gradient sums
  f2 A[L::RP1], C[L::RP1], Ev[L::RP1];  // element pairs
  float G;
  float base[L::RE], spl[L::RE][L::NS];
  float lw[L::RL1][L::OUT], la[L::RL1], lb[L::RL1];

  __device__ void zero() {
#pragma unroll
    for (int r = 0; r < L::RP1; ++r) A[r] = C[r] = Ev[r] = splat(0.f);
    G = 0.f;
#pragma unroll
    for (int r = 0; r < L::RE; ++r) {
      base[r] = 0.f;
#pragma unroll
      for (int c = 0; c < L::NS; ++c) spl[r][c] = 0.f;
    }
#pragma unroll
    for (int r = 0; r < L::RL1; ++r) {
      la[r] = lb[r] = 0.f;
#pragma unroll
      for (int o = 0; o < L::OUT; ++o) lw[r][o] = 0.f;
    }
  }

  // the raw registers of this lane, word w at p[64 w] (the multi-pass sweep parks a virtual wave's
  // sums between two grid sums: NW words per lane, lane-contiguous)
  static constexpr int NW = 6 * L::RP1 + 1 + L::RE * (1 + L::NS) + L::RL1 * (L::OUT + 2);
  __device__ __forceinline__ void park(float* __restrict__ p) const {
    int w = 0;
#pragma unroll
    for (int r = 0; r < L::RP1; ++r) {
      p[64 * w++] = A[r].x;
      p[64 * w++] = A[r].y;
      p[64 * w++] = C[r].x;
      p[64 * w++] = C[r].y;
      p[64 * w++] = Ev[r].x;
      p[64 * w++] = Ev[r].y;
    }
    p[64 * w++] = G;
#pragma unroll
    for (int r = 0; r < L::RE; ++r) {
      p[64 * w++] = base[r];
#pragma unroll
      for (int c = 0; c < L::NS; ++c) p[64 * w++] = spl[r][c];
    }
#pragma unroll
    for (int r = 0; r < L::RL1; ++r) {
#pragma unroll
      for (int o = 0; o < L::OUT; ++o) p[64 * w++] = lw[r][o];
      p[64 * w++] = la[r];
      p[64 * w++] = lb[r];
    }
  }
  __device__ __forceinline__ void unpark(const float* __restrict__ p) {
    int w = 0;
#pragma unroll
    for (int r = 0; r < L::RP1; ++r) {
      A[r].x = p[64 * w++];
      A[r].y = p[64 * w++];
      C[r].x = p[64 * w++];
      C[r].y = p[64 * w++];
      Ev[r].x = p[64 * w++];
      Ev[r].y = p[64 * w++];
    }
    G = p[64 * w++];
#pragma unroll
    for (int r = 0; r < L::RE; ++r) {
      base[r] = p[64 * w++];
#pragma unroll
      for (int c = 0; c < L::NS; ++c) spl[r][c] = p[64 * w++];
    }
#pragma unroll
    for (int r = 0; r < L::RL1; ++r) {
#pragma unroll
      for (int o = 0; o < L::OUT; ++o) lw[r][o] = p[64 * w++];
      la[r] = p[64 * w++];
      lb[r] = p[64 * w++];
    }
  }

  // TPW > 1: job sets that fit in 64 / TPW lanes ran once per trajectory on lanes tt * LPT + job
  // (layer_jobs), so their sums are combined here, trajectories in order
  template <int TPW>
  __device__ void store(float* __restrict__ part, int lane) {
    constexpr AccLayout AL = L::AL;
    constexpr int LPT = 64 / TPW;
    auto comb = [&](float v) {
      float t = v;
#pragma unroll
      for (int k = 1; k < TPW; ++k) t += __shfl(v, lane + k * LPT);
      return t;
    };
    if constexpr (TPW > 1 && L::NE <= LPT) {
      base[0] = comb(base[0]);
#pragma unroll
      for (int c = 0; c < L::NS; ++c) spl[0][c] = comb(spl[0][c]);
    }
    if constexpr (TPW > 1 && L::NL <= LPT) {
#pragma unroll
      for (int o = 0; o < L::OUT; ++o) lw[0][o] = comb(lw[0][o]);
      la[0] = comb(la[0]);
      lb[0] = comb(lb[0]);
    }
#pragma unroll
    for (int r = 0; r < L::RP; ++r) {
      const int e = 2 * (lane + 64 * r);
      if (e < L::E) {
        part[AL.oA + e] = A[r].x;
        part[AL.oA + e + 1] = A[r].y;
        part[AL.oC + e] = C[r].x;
        part[AL.oC + e + 1] = C[r].y;
        part[AL.oE + e] = Ev[r].x;
        part[AL.oE + e + 1] = Ev[r].y;
      }
    }
    if (L::FERRO && lane < L::OUT) part[AL.oG + lane] = G;
#pragma unroll
    for (int r = 0; r < L::RE; ++r) {
      const int q = lane + 64 * r;
      if (q < L::NE) {
        part[AL.oBase + q] = base[r];
#pragma unroll
        for (int c = 0; c < L::NS; ++c) part[AL.oSpl + q * L::NS + c] = spl[r][c];
      }
    }
#pragma unroll
    for (int r = 0; r < L::RL; ++r) {
      const int q = lane + 64 * r;
      if (q < L::NL) {
#pragma unroll
        for (int o = 0; o < L::OUT; ++o) part[AL.oLw + o * L::NL + q] = lw[r][o];
        part[AL.oLa + q] = la[r];
        part[AL.oLb + q] = lb[r];
      }
    }
  }
};

__device__ __forceinline__ float sigm_l2(float zl) { return rcp(1.0f + ex2(zl)); }  // 1/(1+2^zl)

// The lanes of one wave exchange data only through that wave's private LDS region.  DS
// instructions of one wave execute in issue order, so a compiler barrier plus a wait for the
// wave's own LDS traffic replaces the workgroup barrier (global loads in flight — the tape
// prefetch — are not waited for).
__device__ __forceinline__ void wsync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// sum over aligned groups of G lanes (G a power of two <= 32), result on every lane of the group
template <int G>
__device__ __forceinline__ float group_sum(float v) {
  if constexpr (G >= 2) v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  if constexpr (G >= 4) v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  if constexpr (G == 8) v += __shfl_xor(v, 4);
  if constexpr (G >= 16) {  // row_ror 4 then 8: every lane of the 16-lane row holds the row sum
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x124, 0xF, 0xF, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));
  }
  if constexpr (G >= 32) v += __shfl_xor(v, 16);
  static_assert(G <= 32, "group up to 32 lanes");
  return v;
}

// features of combined input t (one lane): SiLU, SiLU', knot interval, u, dense bases, gate
template <int W, int NG, int NB, bool WIN>
__device__ __forceinline__ void feat_input(BFeat<W, NG - 1 - kSO, NB, WIN>& F, const BInTab<W, NG, NB>& Tb, int t,
                                           float gsl2e, float wc, float gs, int z) {
  constexpr int NI = NG - 1, NS = NG - 1 - kSO;
  const float x = F.x[t];
  const float sx = sigm_l2(-x * FETODE_LOG2E);
  F.silu[t] = x * sx;
  F.dsilu[t] = sx * ffma(x, 1.0f - sx, 1.0f);
  const float* g = &Tb.knots[t * NG + z];
  int m = -1;
  if constexpr (NG % 4 == 0) {  // the row as float4s: every knot read issued at once
    const float4* g4 = reinterpret_cast<const float4*>(g);
#pragma unroll
    for (int j = 0; j < NG / 4; ++j) {
      const float4 v = g4[j];
      m += ((x >= v.x) ? 1 : 0) + ((x >= v.y) ? 1 : 0) + ((x >= v.z) ? 1 : 0) + ((x >= v.w) ? 1 : 0);
    }
  } else {
#pragma unroll
    for (int j = 0; j < NG; ++j) m += (x >= g[j]) ? 1 : 0;
  }
  const bool fin = __builtin_isfinite(x);
  const bool in = fin && m >= 0 && m < NI;
  const int mc = in ? m : 0;
  const float rhm = Tb.rh[t * NI + mc + z];
  const float u = in ? (x - g[mc]) * rhm : (fin ? 0.f : __builtin_nanf(""));
  F.rhm[t] = rhm;
  F.m[t] = in ? m : NI;
  F.u[t] = u;
  using FB = BFeat<W, NS, NB, WIN>;
  float* bd = &F.bd[FB::bdi(t, 0)];
  // non-finite x: NaN bases like the reference's (x - g)/d * 0; outside the grid: all zero
  const float fill = fin ? 0.f : __builtin_nanf("");
  // the interval's four basis cubics, all reads issued before any use
  const float4* bp = &Tb.bp[Tb.bpi(t, mc) + z];
  float4 p[kSO + 1];
#pragma unroll
  for (int r = 0; r <= kSO; ++r) p[r] = bp[r];
  float v[kSO + 1];
#pragma unroll
  for (int r = 0; r <= kSO; ++r) v[r] = ffma(ffma(ffma(p[r].w, u, p[r].z), u, p[r].y), u, p[r].x);
  // dense row through the LDS window: the row filled, then bases m - 3 .. m written over it (one
  // wave's LDS writes land in issue order; c outside [0, NS) falls in the guards, and off the grid
  // mc = 0 puts the fill over c = 0 again)
  if constexpr (WIN) {
    if constexpr (NS % 4 == 0) {
#pragma unroll
      for (int c = 0; c < NS; c += 4) *reinterpret_cast<float4*>(&bd[c]) = make_float4(fill, fill, fill, fill);
    } else {
#pragma unroll
      for (int c = 0; c < NS; ++c) bd[c] = fill;
    }
#pragma unroll
    for (int r = 0; r <= kSO; ++r) bd[mc - kSO + r] = in ? v[r] : fill;
  } else {  // formed in registers (select chains) and written once
#pragma unroll
    for (int c = 0; c < NS; ++c) {
      float b = fill;
#pragma unroll
      for (int r = 0; r <= kSO; ++r) b = (in && c == mc - kSO + r) ? v[r] : b;
      bd[c] = b;
    }
  }
  const float up = sigm_l2(-gsl2e * (x - F.pv[t]));
  const float wo = wc * (1.0f - up);
  F.g4[t] = make_float4(x, up, wo, -0.69314718f * wo);
}

// the VJP jobs of one layer (inputs at combined offset TB) for one evaluation of each of the
// wave's TPW trajectories (Fs[tt], gouts + tt * GS, cbs + tt * CBS): gradient sums into R (the
// lane's job slots, summed over the trajectories in order), d out/d x contributions into
// cb[i * NTMP + t]
template <class L, int TB, bool ACC, int TPW, int GS, int CBS, class FT>
__device__ __forceinline__ void layer_jobs(const FT* Fs, const float* __restrict__ gouts, const BTab<L>& Tb,
                                           const float* __restrict__ rhs, BReg<L>& R, float* __restrict__ cbs,
                                           float gsl2e, float wc, float gs, int lane, int z) {
  if constexpr (L::FERRO && !(FETODE_EXP_SKIP & 1)) {
    // element pairs (k, k+1) of one (i, o) on packed-fp32 ops; with wo = wc (1 - up), c' = c (1 - c):
    //   c = sigmoid(gs(-x - Ec)), m = 1 + wo c, sh = x + Ec m, th = tanh(k sh), q = g (1 - th^2)
    //   A += g th, C += q sh, E += q (m + Ec dm/dEc) with Ec dm/dEc = (-gs Ec) wo c'
    //   d out/d x = q coef Ps k (1 + Ec dm/dx) with dm/dx = -gs wo (up c + c');
    //   (-gs Ec) wo is formed once per pair as (gs log2e Ec)(-ln2 wo)
#pragma unroll
    for (int tt = 0; tt < TPW; ++tt)  // trajectories in turn, each one's rounds interleaved
#pragma unroll
    for (int r = 0; r < L::RP; ++r) {
      const int p = lane + 64 * r;
      if (p < L::EP) {
        const FT& F = Fs[tt];
        const float* gout = gouts + tt * GS;
        float* cb = cbs + tt * CBS;
        const int e = 2 * p, i = e / (L::OUT * L::K), ok_ = e % (L::OUT * L::K);
        const int o = ok_ / L::K;
        const float4 g = F.g4[TB + i];
        const float go = gout[o];
        const float4 fa = Tb.fpa[p + z], fb = Tb.fpb[p + z];
        const f2 Ec = f2{fa.x, fa.y}, k2 = f2{fa.z, fa.w}, cPk = f2{fb.x, fb.y}, Eg2 = f2{fb.z, fb.w};
        const f2 x = splat(g.x), wo = splat(g.z), gv = splat(go);
        const f2 cn = rcpx2(ex2x2(pfma(x, splat(gsl2e), Eg2)) + splat(1.0f));  // sigmoid(gs(-x - Ec))
        const f2 mm = pfma(wo, cn, splat(1.0f));                           // branch_mom, branch_sign = 1
        const f2 sh = pfma(Ec, mm, x);                                     // shifted_x
        const f2 th = pfma(splat(-2.0f), rcpx2(ex2x2(k2 * sh) + splat(1.0f)), splat(1.0f));  // tanh(k sh)
        const f2 q = gv * pfma(-th, th, splat(1.0f));
        const f2 dcn = pfma(-cn, cn, cn);
        const f2 ew = Eg2 * splat(g.w);  // (-gs Ec) wo
        if constexpr (ACC) {
          R.A[r] = pfma(gv, th, R.A[r]);
          R.C[r] = pfma(q, sh, R.C[r]);
          R.Ev[r] = pfma(q, pfma(ew, dcn, mm), R.Ev[r]);
        }
        // Ec dm/dx = ew (up c + c')
        *reinterpret_cast<f2*>(&cb[i * L::NTMP + ok_]) = (q * cPk) * pfma(ew, pfma(splat(g.y), cn, dcn), splat(1.0f));
      }
    }
    if constexpr (ACC)
      if (lane < L::OUT)
#pragma unroll
        for (int tt = 0; tt < TPW; ++tt) R.G += gouts[tt * GS + lane];
  }
  // KAN edges (and below, logistic pairs): when one trajectory's jobs fit in 64 / TPW lanes, every
  // trajectory's jobs run in ONE round (lane = tt * 64 / TPW + job); the lane sums of one job are
  // combined across trajectories once, at store
  auto edge = [&](int tt, int q, int r) __attribute__((always_inline)) {
    {
      const FT& F = Fs[tt];
      float* cb = cbs + tt * CBS;
      const int o = q / L::IN, i = q % L::IN;
      const float go = gouts[tt * GS + o];
      if constexpr (ACC) {
        R.base[r] = ffma(go, F.silu[TB + i], R.base[r]);
#pragma unroll
        for (int c = 0; c < L::NS; ++c) R.spl[r][c] = ffma(go, F.bd[FT::bdi(TB + i, c)], R.spl[r][c]);
      }
      const int m = F.m[TB + i];
      const float u = F.u[TB + i];
      // (o, i, interval), q = o*IN + i; off the grid m = NI reads the zero row, so dsdx is 0 there
      // (u = 0) and NaN for non-finite inputs (u = NaN): the reference's NaN bases, branch-free
      const float4 cf = Tb.sp[q * BTab<L>::SPS + m + z];
      const float dsdx = ffma(u, ffma(3.0f * u, cf.w, 2.0f * cf.z), cf.y) * F.rhm[TB + i];
      const float wb = Tb.kw[o * (L::IN * L::NFL) + i * L::NFL + z];
      cb[i * L::NTMP + L::OUT * L::K + o] = go * ffma(wb, F.dsilu[TB + i], dsdx);
    }
  };
  constexpr int LPT = 64 / TPW;
  if constexpr (FETODE_EXP_SKIP & 2) {
  } else if constexpr (L::NE <= LPT) {
    if (lane % LPT < L::NE) edge(lane / LPT, lane % LPT, 0);
  } else {
#pragma unroll 1
    for (int tt = 0; tt < TPW; ++tt)
#pragma unroll
    for (int r = 0; r < L::RE; ++r)
      if (lane + 64 * r < L::NE) edge(tt, lane + 64 * r, r);
  }
  auto logi = [&](int tt, int q, int r) __attribute__((always_inline)) {
    {
      const FT& F = Fs[tt];
      const float* gout = gouts + tt * GS;
      float* cb = cbs + tt * CBS;
      const int i = q / L::NB, j = q % L::NB;
      const float s = F.sg[TB * L::NB + q], ds = s * (1.0f - s), x = F.x[TB + i];
      float S = 0.f;
#pragma unroll
      for (int o = 0; o < L::OUT; ++o) {
        const float go = gout[o];
        S = ffma(go, Tb.kw[o * (L::IN * L::NFL) + i * L::NFL + 1 + j + z], S);
        if constexpr (ACC) R.lw[r][o] = ffma(go, s, R.lw[r][o]);
      }
      const float T = S * ds;  // kw holds 2 * scaled logistic weight: d(2 sigmoid) folded in
      const float pa = Tb.pa[q + z];
      if constexpr (ACC) {
        R.la[r] = ffma(T, x - Tb.pb[q + z], R.la[r]);
        R.lb[r] = ffma(-T, pa, R.lb[r]);
      }
      cb[i * L::NTMP + L::OUT * L::K + L::OUT + j] = T * pa;
    }
  };
  if constexpr (FETODE_EXP_SKIP & 4) {
  } else if constexpr (L::NL <= LPT) {
    if (lane % LPT < L::NL) logi(lane / LPT, lane % LPT, 0);
  } else {
#pragma unroll 1
    for (int tt = 0; tt < TPW; ++tt)
#pragma unroll
    for (int r = 0; r < L::RL; ++r)
      if (lane + 64 * r < L::NL) logi(tt, lane + 64 * r, r);
  }
}

// gin[i] = sum_t cb[i * NTMP + t], fixed order: LPI lanes per input, each summing a contiguous
// run of float4 chunks, then a DPP tree; with TPW trajectories per wave each takes 64 / TPW lanes
// (cbs + tt * CBS -> gins + tt * GS)
template <class L, int TPW, int GS, int CBS>
__device__ __forceinline__ void reduce_gin(const float* __restrict__ cbs, float* gins, int lane) {
  if constexpr (FETODE_EXP_SKIP & 16) return;
  constexpr int HALF = 64 / TPW;
  constexpr int LPI0 = pow2_floor(HALF / L::IN);
  constexpr int LPI = LPI0 > 32 ? 32 : (L::LPI < LPI0 ? L::LPI : LPI0);
  constexpr int C4 = (L::NTM + 4 * LPI - 1) / (4 * LPI);  // float4 chunks per lane
  static_assert(L::NTM % 4 == 0 && L::NTMP % 4 == 0 && CBS % 4 == 0, "float4 rows of the cb table");
  const int tt = lane / HALF, sl = lane % HALF;
  const int i = sl / LPI, sub = sl % LPI;
  const float4* cb = reinterpret_cast<const float4*>(cbs + tt * CBS + i * L::NTMP);
  float s = 0.f;
  if (i < L::IN) {
#pragma unroll
    for (int k = 0; k < C4; ++k) {
      const int c = sub * C4 + k;
      if (4 * c < L::NTM) {
        const float4 v = cb[c];
        s += (v.x + v.y) + (v.z + v.w);
      }
    }
  }
  s = group_sum<LPI>(s);
  if (i < L::IN && sub == 0) gins[tt * GS + i] = s;
}

struct BwdArgs {
  const float* plan;
  LayerPlan P0, P1;
  fetode_kanlinear_t k0, k1;
  fetode_ferro_t f0, f1;
  int32_t method;
  int64_t B;
  const float* step_coef;
  int32_t n_steps;
  const int32_t* out_step;
  const int32_t* out_mode;
  const float* out_slope;
  int32_t T;
  const float* gsol;    // (T, B, D)
  const float* tape;    // (n_evals, B, D + H)
  const float* state0;  // hysteresis state before the solve (include/fetode.h layout)
  uint32_t init_mask;
  float* gy0;           // (B, D) or null
  float* part;          // (rows, nacc)
  int32_t nacc;
  float* gadj;          // (n_evals, B, D + H): d loss / d k (D) and d loss / d h (H) per evaluation
};

// stage-combine coefficients of one step in the forward's fp32 arithmetic (odeint.py
// _combine_coefs): y1 = y + sum_j bc[j] k_j,  X_st = y + sum_{j<st} ac[st][j] k_j
__device__ __forceinline__ void step_coefs(int method, float dt, float hh, float h6, float bc[4], float ac[4][3]) {
  const float third = 1.0f / 3.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bc[i] = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) ac[i][j] = 0.f;
  }
  if (method == FETODE_RK4) {  // rk_common.rk4_alt_step_func (3/8 rule)
    bc[0] = dt * 0.125f;
    bc[1] = 3.0f * dt * 0.125f;
    bc[2] = 3.0f * dt * 0.125f;
    bc[3] = dt * 0.125f;
    ac[1][0] = dt * third;
    ac[2][0] = -dt * third;
    ac[2][1] = dt;
    ac[3][0] = dt;
    ac[3][1] = -dt;
    ac[3][2] = dt;
  } else if (method == FETODE_RK4_CLASSIC) {  // train_kan_fet_ett.py:72-75
    bc[0] = h6;
    bc[1] = 2.0f * h6;
    bc[2] = 2.0f * h6;
    bc[3] = h6;
    ac[1][0] = hh;
    ac[2][1] = hh;
    ac[3][2] = dt;
  } else if (method == FETODE_MIDPOINT) {
    bc[1] = dt;
    ac[1][0] = hh;
  } else {
    bc[0] = dt;
  }
}

constexpr int kTPB = 4;  // trajectories (waves) per workgroup, sharing one copy of the tables
#ifndef FETODE_BWD_WAVES
#define FETODE_BWD_WAVES 2  // minimum waves per SIMD the register allocation must allow
#endif

struct DopriBwdArgs {
  BwdArgs b;            // plan, layers, B, T, gsol, tape ((n_ev, B, 2 D + H): inputs, output), state0, ...
  const double* att;    // (n_att, 4): t0, dt, error ratio, accepted
  int32_t n_att, n_ev, base;  // base: evaluation index of attempt 0's stage 2 (1 with first_step, else 2)
  const double* t;      // (T) output times, fp64
  const double* init_rec;  // {d0, d1, d2, h0, h1}
  float beta[6][6], cerr[7], cmid[7];
  float rtol, atol;
  DopriStep step;  // first_step unused: base says whether it was given
  double n_el;
  DopriParams gp;       // the grid-sum words and leaf layout (single device)
  int32_t* status;      // 0, or 4 when a grid sum timed out
};

// a wave-uniform value computed on the VALU (or read from LDS) into SGPRs: it stays live across
// the evaluations' VJPs without holding VGPRs
__device__ __forceinline__ float unif(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, v)));
}
__device__ __forceinline__ double uni(double v) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

// bytes of the sweep's per-element carried adjoints (ElSt) in the multi-pass parking area
constexpr int kMpElBytes = 48;
