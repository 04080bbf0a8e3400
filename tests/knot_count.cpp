// Host-only check of the fused kernels' two-level knot count (fet-ode_amd/csrc/fetode_knot_count.h),
// built and run by tests/test_knot_count.py with -fsanitize=address,undefined.
//
// On sorted (non-decreasing) sets of four knots the two-level count must equal the linear count,
// the definition, for every probe: each knot itself, its two neighbouring floats, +-0, +-inf, NaN,
// denormals, the extremes of the format and a sweep across the set.  The sets cover uniform and
// uneven spacing, repeated knots, knots at +-0 and in the denormals, and +inf padding.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "fetode_knot_count.h"

using namespace fetode;

namespace {

int g_fail = 0, g_checks = 0;

void probe(const float* kn, float x, int set) {
  const int lin = knot_count_linear<4>(x, kn);
  const int two = knot_count4_sorted(x, kn);
  const int used = knot_count<4>(x, kn);   // what the kernels call (the host form of it)
  ++g_checks;
  if (lin != two || lin != used) {
    if (++g_fail <= 20)
      std::printf("FAIL set %d {%a, %a, %a, %a} x = %a: linear %d, two-level %d, knot_count %d\n", set, kn[0],
                  kn[1], kn[2], kn[3], x, lin, two, used);
  }
}

}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float dmin = std::numeric_limits<float>::denorm_min();
  const float fmin = std::numeric_limits<float>::min();
  const float fmax = std::numeric_limits<float>::max();
  const std::vector<std::vector<float>> sets = {
      {-2.2f, -1.8f, -1.4f, -1.0f},          // the default grid's first lane
      {-0.6f, -0.2f, 0.2f, 0.6f},            // ... second lane (straddles zero)
      {1.0f, 1.4f, 1.8f, 2.2f},              // ... third lane
      {-3.0f, -0.001f, 0.5f, 1000.0f},       // uneven
      {0.25f, 0.25f, 0.25f, 0.25f},          // all repeated
      {-1.0f, -1.0f, 2.0f, 2.0f},            // repeated pairs
      {-1.0f, 0.5f, 0.5f, 0.5f},             // repeated across the split
      {-1.0f, -1.0f, -1.0f, 3.0f},
      {-0.0f, 0.0f, 0.0f, 1.0f},             // signed zeros as knots
      {-1.0f, -0.0f, 0.0f, 1.0f},
      {-dmin, 0.0f, dmin, 2 * dmin},         // denormal knots
      {-fmin, -dmin, dmin, fmin},
      {1.0f, 2.0f, 3.0f, inf},               // +inf padding, one to four pads
      {1.0f, 2.0f, inf, inf},
      {1.0f, inf, inf, inf},
      {inf, inf, inf, inf},
      {-fmax, -1.0f, 1.0f, fmax},            // the format's extremes
      {1.0f, std::nextafter(1.0f, 2.0f), std::nextafter(std::nextafter(1.0f, 2.0f), 2.0f), 1.000001f},  // adjacent floats
  };
  int si = 0;
  for (const auto& s : sets) {
    const float* kn = s.data();
    for (int t = 0; t + 1 < 4; ++t)
      if (!(kn[t] <= kn[t + 1])) {
        std::printf("FAIL set %d is not sorted\n", si);
        return 2;
      }
    std::vector<float> xs = {0.0f, -0.0f, inf, -inf, nan, -nan, dmin, -dmin, 3 * dmin, fmin, -fmin, fmax, -fmax};
    for (int t = 0; t < 4; ++t) {
      xs.push_back(kn[t]);
      xs.push_back(std::nextafter(kn[t], -inf));
      xs.push_back(std::nextafter(kn[t], inf));
    }
    // a sweep across the finite part of the set and a little beyond
    float lo = kn[0], hi = kn[0];
    for (int t = 0; t < 4; ++t)
      if (std::isfinite(kn[t])) hi = kn[t];
    if (std::isfinite(lo) && std::isfinite(hi)) {
      const double span = (double)hi - (double)lo, pad = span > 0 ? 0.25 * span : 1.0;
      for (int i = 0; i <= 400; ++i) xs.push_back((float)(lo - pad + (span + 2 * pad) * i / 400.0));
    }
    for (float x : xs) probe(kn, x, si);
    ++si;
  }
  // the documented edge values on a plain set: NaN and -inf count none, +inf counts all
  const float k[4] = {-1.0f, 0.0f, 1.0f, 2.0f};
  if (knot_count4_sorted(nan, k) != 0 || knot_count4_sorted(-inf, k) != 0 || knot_count4_sorted(inf, k) != 4 ||
      knot_count4_sorted(1.0f, k) != 3 || knot_count4_sorted(std::nextafter(1.0f, 0.0f), k) != 2) {
    std::printf("FAIL edge values\n");
    ++g_fail;
  }
  std::printf("knot_count: %d sorted sets, %d probes, %d failures\n", si, g_checks, g_fail);
  return g_fail ? 1 : 0;
}
