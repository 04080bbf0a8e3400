// Host-only check of the fused kernels' lane map (fet-ode_amd/csrc/fetode_fused4_image.h), built and
// run by tests/test_plan_image_map.py with -fsanitize=address,undefined.
//
// For both fields (KAN-FET K = 10, KAN) and both variants (3 / 6 lanes per hidden unit) every plan
// value a lane group consumes must be the source of EXACTLY ONE slot of its owning group, and every
// other slot must be a pad with the documented value (0; +inf for knots).  The expected sets are
// formed here from the classic plan layout alone, not from the header.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "fetode_fused4_image.h"

using namespace fetode;

namespace {

// the classic plan sections (fetode_common.hip layer_plan), restated
struct LP {
  int in, out, K, NB, NG, NI, NFL;
  int64_t fe_GEc, fe_k2, fe_k2Ec, fe_CPs2, fconst, kw, lg, knots, rh, sp, flag, end;
};
LP layer(int in, int out, int K, int NB, int NG, int64_t base) {
  LP p{};
  p.in = in; p.out = out; p.K = K; p.NB = NB; p.NG = NG; p.NI = NG - 1; p.NFL = 1 + NB;
  const int64_t NE = (int64_t)in * out * K;
  int64_t o = base;
  p.fe_GEc = o; o += NE;
  p.fe_k2 = o; o += NE;
  p.fe_k2Ec = o; o += NE;
  p.fe_CPs2 = o; o += NE;
  p.fconst = o; o += out;
  p.kw = o; o += (int64_t)out * in * p.NFL;
  p.lg = o; o += (int64_t)in * NB * 2;
  p.knots = o; o += (int64_t)in * NG;
  p.rh = o; o += (int64_t)in * p.NI;
  o = (o + 3) & ~int64_t(3);
  p.sp = o; o += (int64_t)out * in * (p.NI + 1) * 4;
  p.flag = o; o += 1;
  p.end = (o + 3) & ~int64_t(3);
  return p;
}

int g_fail = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (++g_fail <= 20) {                            \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                      \
        std::printf("\n");                             \
      }                                                \
    }                                                  \
  } while (0)

typedef std::map<int64_t, int> Count;

// got == want, every entry exactly once
void same(const Count& got, const Count& want, const char* what, int id) {
  for (const auto& kv : want) {
    const auto it = got.find(kv.first);
    CHECK(it != got.end() && it->second == 1, "%s %d: plan[%lld] is the source of %d slots", what, id,
          (long long)kv.first, it == got.end() ? 0 : it->second);
  }
  for (const auto& kv : got) CHECK(want.count(kv.first), "%s %d: unexpected source plan[%lld]", what, id, (long long)kv.first);
}

template <int H, int K, int NB, int NG, int NLG>
void check_lanes(const LP& P0, const LP& P1) {
  using IMG = Fused4Lanes<H, K, NB, NG, NLG>;
  constexpr int D = 2, NFL = 1 + NB;
  static_assert(IMG::NSLOT % 4 == 0 && IMG::NF == IMG::NSLOT * IMG::L, "image size");
  // `at` is a bijection of (lane, slot) onto the image's floats
  {
    std::vector<int> hit(IMG::NF, 0);
    for (int l = 0; l < IMG::L; ++l)
      for (int s = 0; s < IMG::NSLOT; ++s) {
        const int w = IMG::at(l, s);
        CHECK(w >= 0 && w < IMG::NF, "at(%d, %d) = %d out of the image", l, s, w);
        if (w >= 0 && w < IMG::NF) ++hit[w];
      }
    for (int w = 0; w < IMG::NF; ++w) CHECK(hit[w] == 1, "image float %d addressed %d times", w, hit[w]);
  }
  // group sections (Ferro elements, feature weights, layer-1 feature jobs), per hidden unit: its 3
  // lanes, or its 3 + 3 lanes of both half-waves
  std::vector<Count> grp(H);
  // the knots of a hidden input, per (half-wave, hidden unit): every half counts the interval itself
  std::vector<Count> knt((IMG::L / 32) * H);
  // layer-0 feature jobs, per (half-wave, input row)
  std::vector<Count> rowc(IMG::L / 16);
  for (int l = 0; l < IMG::L; ++l) {
    const int lane = l & 31, row = lane >> 4, c1 = lane & 15, o0 = row * 5 + c1 / 3;
    const bool act = c1 < 15 && o0 < H;
    for (int s = 0; s < IMG::NSLOT; ++s) {
      const ImgSrc r = IMG::src(P0, P1, l, s);
      const bool xsec = s >= IMG::S_X && s < IMG::S_HK;
      if (r.src) {
        if (xsec) ++rowc[l >> 4][r.ofs];
        else {
          CHECK(act, "lane %d slot %d: an inactive lane has a source", l, s);
          if (act && s >= IMG::S_HK) ++knt[(l >> 5) * H + o0][r.ofs];
          else if (act) ++grp[o0][r.ofs];
        }
      } else {
        const bool knot = s >= IMG::S_HK || s == IMG::S_X + 2;
        if (knot) CHECK(std::isinf(r.pad) && r.pad > 0, "lane %d slot %d: knot pad %g, not +inf", l, s, r.pad);
        else CHECK(r.pad == 0.f && !std::signbit(r.pad), "lane %d slot %d: pad %g, not 0", l, s, r.pad);
      }
    }
  }
  for (int o = 0; o < H; ++o) {
    Count want;
    const int64_t fe0[4] = {P0.fe_GEc, P0.fe_k2, P0.fe_k2Ec, P0.fe_CPs2};
    const int64_t fe1[4] = {P1.fe_GEc, P1.fe_k2, P1.fe_k2Ec, P1.fe_CPs2};
    for (int sec = 0; sec < 4; ++sec) {
      for (int i = 0; i < D; ++i)   // layer-0 Ferro element (o, i, k)
        for (int k = 0; k < K; ++k) want[fe0[sec] + (int64_t)o * (D * K) + i * K + k] = 1;
      for (int d = 0; d < D; ++d)   // layer-1 element (output d, input o, k)
        for (int k = 0; k < K; ++k) want[fe1[sec] + (int64_t)d * (H * K) + o * K + k] = 1;
    }
    for (int i = 0; i < D; ++i)     // layer-0 feature weights kw(o, i, ff)
      for (int ff = 0; ff < NFL; ++ff) want[P0.kw + (int64_t)o * (D * NFL) + i * NFL + ff] = 1;
    for (int j = 0; j < NFL; ++j) { // layer-1 feature jobs of hidden unit o: logistic j < NB, SiLU j == NB
      if (j < NB) {
        want[P1.lg + 2 * (o * NB + j)] = 1;
        want[P1.lg + 2 * (o * NB + j) + 1] = 1;
      }
      const int ff = j < NB ? 1 + j : 0;
      for (int d = 0; d < D; ++d) want[P1.kw + (int64_t)d * (H * NFL) + o * NFL + ff] = 1;
    }
    same(grp[o], want, NLG == 3 ? "3-lane group of unit" : "6-lane group of unit", o);
    Count wk;
    for (int kk = 0; kk < NG; ++kk) wk[P1.knots + (int64_t)o * NG + kk] = 1;   // knots of hidden input o
    for (int h = 0; h < IMG::L / 32; ++h) same(knt[h * H + o], wk, "knots of unit", o);
  }
  for (int hr = 0; hr < IMG::L / 16; ++hr) {   // every half-wave holds both input rows
    const int row = hr & 1;
    Count want;
    for (int j = 0; j < NB; ++j) {
      want[P0.lg + 2 * (row * NB + j)] = 1;
      want[P0.lg + 2 * (row * NB + j) + 1] = 1;
    }
    for (int c = 0; c < NG; ++c) want[P0.knots + row * NG + c] = 1;
    same(rowc[hr], want, "layer-0 job row", hr);
  }
}

template <int H, int K, int NB, int NG>
void check_field(const char* name) {
  const LP P0 = layer(2, H, K, NB, NG, 0), P1 = layer(H, 2, K, NB, NG, P0.end);
  using BLK = Fused4Block<H, K, NB, NG>;
  using TAB = typename BLK::TAB;
  constexpr int D = 2, NI = NG - 1;
  check_lanes<H, K, NB, NG, 3>(P0, P1);
  check_lanes<H, K, NB, NG, 6>(P0, P1);
  // the LDS image: every table value once, zero pads
  Count got, want;
  for (int w = 0; w < TAB::NF; ++w) {
    const ImgSrc r = TAB::src(P0, P1, w);
    if (r.src) ++got[r.ofs];
    else CHECK(r.pad == 0.f, "table float %d: pad %g", w, r.pad);
  }
  for (int e = 0; e < H * D * (NI + 1) * 4; ++e) want[P0.sp + e] = want[P1.sp + e] = 1;
  for (int i = 0; i < D; ++i)
    for (int m = 0; m < NI; ++m) want[P0.knots + i * NG + m] = want[P0.rh + i * NI + m] = 1;
  for (int i = 0; i < H; ++i)
    for (int m = 0; m < NI; ++m) want[P1.knots + i * NG + m] = want[P1.rh + i * NI + m] = 1;
  for (int o = 0; o < H; ++o) want[P0.fconst + o] = 1;
  for (int o = 0; o < D; ++o) want[P1.fconst + o] = 1;
  same(got, want, "LDS image", 0);
  // table geometry the kernel's interval reads rely on: row e of a cubic table at pitch SPR float4,
  // interval m < NI + 1 at float4 m of the row; (knot, 1/width) of (input, interval)
  for (int e = 0; e < H * D; ++e)
    for (int m = 0; m <= NI; ++m)
      for (int c = 0; c < 4; ++c) {
        const ImgSrc r0 = TAB::src(P0, P1, TAB::O_SP0 + (e * TAB::SPR + m) * 4 + c);
        const ImgSrc r1 = TAB::src(P0, P1, TAB::O_SP1 + (e * TAB::SPR + m) * 4 + c);
        CHECK(r0.src && r0.ofs == P0.sp + ((int64_t)e * (NI + 1) + m) * 4 + c, "sp0 edge %d interval %d", e, m);
        CHECK(r1.src && r1.ofs == P1.sp + ((int64_t)e * (NI + 1) + m) * 4 + c, "sp1 edge %d interval %d", e, m);
      }
  for (int i = 0; i < H; ++i)
    for (int m = 0; m < NI; ++m) {
      const ImgSrc a = TAB::src(P0, P1, TAB::O_KR1 + 2 * (i * TAB::SPR + m)), b = TAB::src(P0, P1, TAB::O_KR1 + 2 * (i * TAB::SPR + m) + 1);
      CHECK(a.src && a.ofs == P1.knots + i * NG + m && b.src && b.ofs == P1.rh + i * NI + m, "kr1 (%d, %d)", i, m);
      if (i < D) {
        const ImgSrc c = TAB::src(P0, P1, TAB::O_KR0 + 2 * (i * (NI + 1) + m)), d = TAB::src(P0, P1, TAB::O_KR0 + 2 * (i * (NI + 1) + m) + 1);
        CHECK(c.src && c.ofs == P0.knots + i * NG + m && d.src && d.ofs == P0.rh + i * NI + m, "kr0 (%d, %d)", i, m);
      }
    }
  // the block: guard words, then the three images back to back, each float routed to its image
  static_assert(BLK::OFS_LDS % 4 == 0 && BLK::OFS_L3 % 4 == 0 && BLK::OFS_L6 % 4 == 0 && BLK::NF % 4 == 0, "16-byte parts");
  const ImgSrc f0 = BLK::src(P0, P1, 0), f1 = BLK::src(P0, P1, 1);
  CHECK(f0.src && f0.ofs == P0.flag && f1.src && f1.ofs == P1.flag, "guard words");
  for (int w = 2; w < BLK::OFS_LDS; ++w) CHECK(!BLK::src(P0, P1, w).src && BLK::src(P0, P1, w).pad == 0.f, "header pad");
  int n_src = 0;
  for (int w = 0; w < BLK::NF; ++w) {
    const ImgSrc r = BLK::src(P0, P1, w);
    CHECK(!r.src || (r.ofs >= 0 && r.ofs < P1.end), "block float %d: source %lld outside the plan", w, (long long)r.ofs);
    n_src += r.src;
  }
  for (int l = 0; l < 32; ++l)
    for (int s = 0; s < BLK::L3::NSLOT; ++s) {
      const ImgSrc a = BLK::src(P0, P1, BLK::OFS_L3 + BLK::L3::at(l, s)), b = BLK::L3::src(P0, P1, l, s);
      CHECK(a.src == b.src && a.ofs == b.ofs && (a.pad == b.pad), "block routing, 3-lane image (%d, %d)", l, s);
    }
  for (int l = 0; l < 64; ++l)
    for (int s = 0; s < BLK::L6::NSLOT; ++s) {
      const ImgSrc a = BLK::src(P0, P1, BLK::OFS_L6 + BLK::L6::at(l, s)), b = BLK::L6::src(P0, P1, l, s);
      CHECK(a.src == b.src && a.ofs == b.ofs && (a.pad == b.pad), "block routing, 6-lane image (%d, %d)", l, s);
    }
  std::printf("%s: block %d floats (tables %d, lane images %d + %d), %d sourced, failures so far %d\n", name, BLK::NF,
              TAB::NF, BLK::L3::NF, BLK::L6::NF, n_src, g_fail);
}

}  // namespace

int main() {
  check_field<10, 10, 10, 12>("KAN-FET [2,10,2] K=10");
  check_field<10, 0, 10, 12>("KAN [2,10,2]");
  if (g_fail) std::printf("%d checks failed\n", g_fail);
  return g_fail ? 1 : 0;
}
