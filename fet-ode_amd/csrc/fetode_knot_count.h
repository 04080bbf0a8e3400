// fetode_knot_count.h — how many of a lane's N knots are <= x: the lane's share of a hidden value's
// knot interval in the fused [2, 10, 2] kernels (fetode_fused4_body.h: the interval is the sum of
// the shares of a hidden unit's three lanes, minus one).
//
// knot_count_linear is the definition: one compare per knot.  knot_count is what the kernels use:
// for N == 4 a two-level search (x >= k[2] first, then k[3] or k[0], and k[1]), which equals the
// linear count whenever the knots are non-decreasing — what a count-based interval assumes anyway.
// Every comparison is an ordered >=, so a NaN x counts 0, -inf counts 0 (no knot is -inf) and +inf
// counts every knot, +inf pads included, in both forms.
//
// The header also compiles for the host (tests/knot_count.cpp compares the two forms there).
#pragma once

#if defined(__HIPCC__)
#define FETODE_KC_HD __host__ __device__ __forceinline__
#else
#define FETODE_KC_HD inline
#endif

namespace fetode {

template <int N>
FETODE_KC_HD int knot_count_linear(float x, const float* kn) {
  int cnt = 0;
  for (int t = 0; t < N; ++t) cnt += x >= kn[t] ? 1 : 0;
  return cnt;
}

// N == 4, knots non-decreasing.  Upper half (x >= k[2]): k[0], k[1] and k[2] count, k[3] decides:
// 2 + (x >= k[3]) + (x >= k[1]), the last one being true there.  Lower half: (x >= k[0]) + (x >= k[1]).
FETODE_KC_HD int knot_count4_sorted(float x, const float* kn) {
  const bool up = x >= kn[2];
  const float t = up ? kn[3] : kn[0];
  return (up ? 2 : 0) + (x >= t ? 1 : 0) + (x >= kn[1] ? 1 : 0);
}

template <int N>
FETODE_KC_HD int knot_count(float x, const float* kn) {
#if defined(__HIP_DEVICE_COMPILE__)
  // compare + carry-in add per term (plain C++ selects cost a v_cndmask and an add each)
  int cnt;
  if constexpr (N == 4) {
    float t;
    asm("v_cmp_ge_f32 vcc, %2, %3\n\tv_cndmask_b32_e32 %1, %4, %5, vcc\n\tv_cndmask_b32_e64 %0, 0, 2, vcc"
        : "=&v"(cnt), "=&v"(t)
        : "v"(x), "v"(kn[2]), "v"(kn[0]), "v"(kn[3])
        : "vcc");
    asm("v_cmp_ge_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" : "+v"(cnt) : "v"(x), "v"(t) : "vcc");
    asm("v_cmp_ge_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" : "+v"(cnt) : "v"(x), "v"(kn[1]) : "vcc");
  } else {
    cnt = 0;
#pragma unroll
    for (int t = 0; t < N; ++t)
      asm("v_cmp_ge_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" : "+v"(cnt) : "v"(x), "v"(kn[t]) : "vcc");
  }
  return cnt;
#else
  if constexpr (N == 4) return knot_count4_sorted(x, kn);
  else return knot_count_linear<N>(x, kn);
#endif
}

}  // namespace fetode
