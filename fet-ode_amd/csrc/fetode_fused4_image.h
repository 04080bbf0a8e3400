// fetode_fused4_image.h — the lane-ordered plan image of the specialised [2, H, 2] kernels
// (fetode_fused4_body.h), and the ONE definition of their lane map.
//
// The classic plan sections (LayerPlan, fetode_common.h) are ordered by parameter; the body's lanes
// used to gather their constants from them one dword at a time.  The image block, appended to the
// plan after the last layer's `end` when the field has a fused kernel, holds the same values in the
// order the kernel consumes them, so its prologue is one burst of 16-byte loads:
//
//   float 0, 1            the two factored-gate guard words (LayerPlan::flag of layer 0 and 1); 2, 3: zero
//   OFS_LDS ..            the LDS image: the bytes of the kernel's table struct
//                         sp0 | sp1 | kr0 | kr1 | c0 | c1 (cubic tables by edge with their SPR row pitch,
//                         (knot, 1/width) rows, per-output constants), zero-padded to a multiple of 16 B
//   OFS_L3 ..             the lane image of the two-trajectories-per-wave kernels (NLG = 3 lanes per
//                         hidden unit, 32 lanes: both half-waves read the same image)
//   OFS_L6 ..             the lane image of the one-trajectory-per-wave kernels (NLG = 6, 64 lanes)
//
// A lane image is slot-major: float4 j of lane l is float4 (j * L + l) of the image, so one wave-wide
// 16-byte load covers one contiguous stretch.  A lane's float slots, in order (S_* below):
//   NPL0 x 8   layer-0 Ferro pair r:  gec(h=0), gec(h=1), k2(0), k2(1), k2Ec(0), k2Ec(1), CPs2(0), CPs2(1)
//   NSL0 x 4   layer-0 single:        gec, k2, k2Ec, CPs2
//   FPL0       layer-0 feature weights of the lane's chunk
//   NPL1 x 8   layer-1 pair r (k = gl + NLG r), h = output d
//   NSL1 x 4   layer-1 single (K - 1, d = cc0)
//   RF1 x 4    layer-1 feature round r (job j = gl + NLG r): -a log2e, a b log2e, weight of output 0, of output 1
//   4          layer-0 feature job c1 of input `row`: -a log2e, a b log2e, knot c1, pad
//   KT (-> 4)  knots KT cc0 .. KT cc0 + KT - 1 of hidden input o0
// gec is stored raw (the kernel applies exp2 when the gate is factored).  Slots with no source are
// pads: 0, or +inf for knots.  Constants that are no plan values (the SiLU / gate / exp job
// coefficients, the job predicates, the integer lane constants) stay lane arithmetic in the kernel.
//
// Host and device: the writer (fused_image_kernel, fetode_fused.hip), the reader (the body's
// prologue, which takes the slot positions from here) and the map test (tests/test_plan_image_map.py)
// include this header; nothing else defines the map.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FETODE_IMG_HD __host__ __device__
#else
#define FETODE_IMG_HD
#endif

namespace fetode {

// Ferro element split of one layer's output over a lane group: NPAIR element pairs (i, k), (i, k+1)
// over `lanes` lanes.  When the remainder of pairs is at most half a round, the full rounds stay
// pairs (NPL per lane) and the leftover pairs' elements go one per lane (NSL = 1: a single-element
// round costs about half a pair round); otherwise one more pair round (NSL = 0).
template <int NPAIR, int LANES>
struct FerroSplit {
  static constexpr int REM = NPAIR % LANES;
  static constexpr bool SPLIT = REM > 0 && 2 * REM <= LANES;
  static constexpr int NPL = SPLIT ? NPAIR / LANES : (NPAIR + LANES - 1) / LANES;
  static constexpr int NSL = SPLIT ? 1 : 0;
};

// where an image float comes from: plan[ofs] (src) or the constant `pad`
struct ImgSrc {
  bool src;
  int64_t ofs;
  float pad;
};
FETODE_IMG_HD inline ImgSrc img_from(int64_t ofs) { return ImgSrc{true, ofs, 0.f}; }
FETODE_IMG_HD inline ImgSrc img_pad(float v) { return ImgSrc{false, 0, v}; }

// the table struct of the kernel (LDS image), K = 0: KAN (no Ferro layer)
template <int H, int NG>
struct Fused4Tables {
  static constexpr int D = 2, NI = NG - 1;
  // edge cubic tables by interval, one row of NI + 1 float4 per edge padded to SPR: at a pitch of 12
  // float4 the rows of units 4 apart (layer 1) / of the same parity (layer 0) start on the same
  // 16-byte slot of the bank row and the lanes' interval reads collide (35 % of the kernel's LDS
  // cycles were conflicts, profiles/r06_lds_bench_nores.txt)
  static constexpr int SPR = NI + 2, SPE = (NI + 1) * 4;
  static constexpr int SPT0 = H * D * SPR * 4, SPT1 = D * H * SPR * 4;
  static constexpr int KR0 = D * (NI + 1), KR1 = H * SPR;   // (knot, 1/width) pairs
  // float offsets of the members
  static constexpr int O_SP0 = 0, O_SP1 = O_SP0 + SPT0, O_KR0 = O_SP1 + SPT1, O_KR1 = O_KR0 + 2 * KR0;
  static constexpr int O_C0 = O_KR1 + 2 * KR1, O_C1 = O_C0 + H, O_END = O_C1 + D;
  static constexpr int NF = (O_END + 3) & ~3;   // floats, a multiple of 16 B

  // float w of the LDS image; P0 / P1: the layers' LayerPlan (any struct with its offset members)
  template <class LP>
  static FETODE_IMG_HD ImgSrc src(const LP& P0, const LP& P1, int w) {
    if (w < O_KR0) {   // cubic tables: edge e's row of NI + 1 float4, then the pitch pad
      const bool l1 = w >= O_SP1;
      const int v = l1 ? w - O_SP1 : w, e = v / (SPR * 4), rr = v % (SPR * 4);
      if (rr >= SPE) return img_pad(0.f);
      return img_from((l1 ? P1.sp : P0.sp) + (int64_t)e * SPE + rr);
    }
    if (w < O_C0) {    // (knot, 1/width) by (input, interval); the zero row NI (and layer 1's pitch pad)
      const bool l1 = w >= O_KR1;
      const int v = l1 ? w - O_KR1 : w - O_KR0, i = v / 2, c = v % 2;
      const int pitch = l1 ? SPR : NI + 1, in = i / pitch, m = i % pitch;
      if (m >= NI) return img_pad(0.f);
      const LP& P = l1 ? P1 : P0;
      return img_from(c == 0 ? P.knots + (int64_t)in * NG + m : P.rh + (int64_t)in * NI + m);
    }
    if (w < O_C1) return img_from(P0.fconst + (w - O_C0));
    if (w < O_END) return img_from(P1.fconst + (w - O_C1));
    return img_pad(0.f);
  }
};

// the lane image of one variant: NLG = 3 (two trajectories per wave) or 6 (one per wave)
template <int H, int K, int NB, int NG, int NLG>
struct Fused4Lanes {
  static_assert(NLG == 3 || NLG == 6, "lanes per hidden unit");
  static constexpr bool FERRO = K > 0;
  static constexpr int D = 2, NI = NG - 1, NFL = 1 + NB, NFP = (NFL + 1) & ~1;
  static constexpr int KP = K / 2 > 0 ? K / 2 : 1;
  using FS0 = FerroSplit<D * KP, NLG>;
  static constexpr int REM0 = FS0::REM;
  static constexpr bool SPLIT1 = NLG == 3 && K % NLG == 1;   // one k left: two singles (d = 0, 1)
  static constexpr int NPL0 = FERRO ? FS0::NPL : 0, NSL0 = FERRO ? FS0::NSL : 0;
  static constexpr int NPL1 = FERRO ? (SPLIT1 ? K / NLG : (K + NLG - 1) / NLG) : 0;
  static constexpr int NSL1 = (FERRO && SPLIT1) ? 1 : 0;
  static constexpr int FPL0 = ((D * NFP + NLG - 1) / NLG + 3) & ~3;
  static constexpr int RF1 = (NFL + NLG - 1) / NLG;   // feature rounds of a hidden input (SiLU + NB)
  static constexpr int KT = (NG + 2) / 3;             // knots per group lane
  static constexpr int L = NLG == 3 ? 32 : 64;        // lanes of the image
  // float slots of a lane
  static constexpr int S_P0 = 0, S_S0 = S_P0 + 8 * NPL0, S_FW0 = S_S0 + 4 * NSL0, S_P1 = S_FW0 + FPL0;
  static constexpr int S_S1 = S_P1 + 8 * NPL1, S_F1 = S_S1 + 4 * NSL1, S_X = S_F1 + 4 * RF1, S_HK = S_X + 4;
  static constexpr int NSLOT = S_HK + ((KT + 3) & ~3);
  static constexpr int NV4 = NSLOT / 4;               // float4 per lane
  static constexpr int NF = NV4 * L * 4;              // floats of the image
  static_assert(NSLOT % 4 == 0, "lane slots fill whole float4s");

  // float offset of lane l's slot s within the image (slot-major float4s)
  static FETODE_IMG_HD int at(int l, int s) { return ((s / 4) * L + l) * 4 + s % 4; }

  template <class LP>
  static FETODE_IMG_HD int64_t ferro(const LP& P, int which) {
    return which == 0 ? P.fe_GEc : which == 1 ? P.fe_k2 : which == 2 ? P.fe_k2Ec : P.fe_CPs2;
  }

  // slot s of lane l
  template <class LP>
  static FETODE_IMG_HD ImgSrc src(const LP& P0, const LP& P1, int l, int s) {
    const int hh = l >> 5, lane = l & 31, row = lane >> 4, c1 = lane & 15;
    const int q = c1, o0 = row * 5 + q / 3, cc0 = q % 3;
    const bool act0 = q < 15 && o0 < H;
    const int gl = NLG == 3 ? cc0 : cc0 + 3 * hh;   // lane within the hidden unit's group
    if (s < S_S0) {          // layer-0 pair r: elements (o0, i, 2 (P % KP) + h), P = gl NPL0 + r
      const int r = (s - S_P0) / 8, e = (s - S_P0) % 8, which = e / 2, h = e % 2;
      const int P = gl * NPL0 + r;
      if (!(act0 && P < D * KP)) return img_pad(0.f);
      return img_from(ferro(P0, which) + (int64_t)o0 * (D * K) + (P / KP) * K + (P % KP) * 2 + h);
    }
    if (s < S_FW0) {         // layer-0 single: element gl % 2 of leftover pair NPL0 NLG + gl / 2
      const int which = s - S_S0;
      const int Pl = NPL0 * NLG + gl / 2;
      if (!(act0 && gl < 2 * REM0)) return img_pad(0.f);
      return img_from(ferro(P0, which) + (int64_t)o0 * (D * K) + (Pl / KP) * K + (Pl % KP) * 2 + gl % 2);
    }
    if (s < S_P1) {          // layer-0 feature weights: chunk float qq = gl FPL0 + f of (input, feature)
      const int qq = gl * FPL0 + (s - S_FW0), i = qq / NFP, ff = qq % NFP;
      if (!(act0 && i < D && ff < NFL)) return img_pad(0.f);
      return img_from(P0.kw + (int64_t)o0 * (D * NFL) + i * NFL + ff);
    }
    if (s < S_S1) {          // layer-1 pair r: elements (o0, d = h, k = gl + NLG r)
      const int r = (s - S_P1) / 8, e = (s - S_P1) % 8, which = e / 2, d = e % 2;
      const int k = gl + NLG * r;
      if (!(act0 && k < K)) return img_pad(0.f);
      return img_from(ferro(P1, which) + (int64_t)d * (H * K) + o0 * K + k);
    }
    if (s < S_F1) {          // layer-1 single: element (o0, d = cc0, K - 1)
      const int which = s - S_S1;
      if (!(act0 && cc0 < D)) return img_pad(0.f);
      return img_from(ferro(P1, which) + (int64_t)cc0 * (H * K) + o0 * K + (K - 1));
    }
    if (s < S_X) {           // layer-1 feature round r: job j = gl + NLG r (logistic j < NB, SiLU j == NB)
      const int r = (s - S_F1) / 4, e = (s - S_F1) % 4;
      const int j = gl + NLG * r;
      if (!(act0 && j < NFL)) return img_pad(0.f);
      if (e < 2) return j < NB ? img_from(P1.lg + 2 * (o0 * NB + j) + e) : img_pad(0.f);
      const int ff = j < NB ? 1 + j : 0;   // kw feature index: SiLU 0, logistic j at 1 + j
      return img_from(P1.kw + (int64_t)(e - 2) * (H * NFL) + o0 * NFL + ff);
    }
    if (s < S_HK) {          // layer-0 feature job c1 of input `row`, and the row's knot c1
      const int e = s - S_X;
      if (e < 2) return c1 < NB ? img_from(P0.lg + 2 * (row * NB + c1) + e) : img_pad(0.f);
      if (e == 2) return c1 < NG ? img_from(P0.knots + row * NG + c1) : img_pad(__builtin_inff());
      return img_pad(0.f);
    }
    const int t = s - S_HK, kk = KT * cc0 + t;   // knots of hidden input o0
    if (!(act0 && t < KT && kk < NG)) return img_pad(__builtin_inff());
    return img_from(P1.knots + (int64_t)o0 * NG + kk);
  }
};

// the whole block
template <int H, int K, int NB, int NG>
struct Fused4Block {
  using TAB = Fused4Tables<H, NG>;
  using L3 = Fused4Lanes<H, K, NB, NG, 3>;
  using L6 = Fused4Lanes<H, K, NB, NG, 6>;
  static constexpr int OFS_LDS = 4, OFS_L3 = OFS_LDS + TAB::NF, OFS_L6 = OFS_L3 + L3::NF;
  static constexpr int NF = OFS_L6 + L6::NF;   // floats, a multiple of 4

  template <class LP>
  static FETODE_IMG_HD ImgSrc src(const LP& P0, const LP& P1, int w) {
    if (w < OFS_LDS) return w == 0 ? img_from(P0.flag) : w == 1 ? img_from(P1.flag) : img_pad(0.f);
    if (w < OFS_L3) return TAB::src(P0, P1, w - OFS_LDS);
    const bool six = w >= OFS_L6;
    const int v = six ? w - OFS_L6 : w - OFS_L3, L = six ? 64 : 32;
    const int f4 = v / 4, c = v % 4, j = f4 / L, l = f4 % L;
    return six ? L6::src(P0, P1, l, 4 * j + c) : L3::src(P0, P1, l, 4 * j + c);
  }
};

}  // namespace fetode
