// fetode_bwd_mp.hip — the multi-pass reverse sweep of the device-resident dopri5 solve
// (fetode_dopri5_set_multipass): dopri_bwd_kernel's body (fetode_dopri_bwd_body.h, MP) on a grid no
// larger than the co-resident capacity, each workgroup serving several virtual workgroups between
// two grid sums.  A translation unit of its own: instantiated next to the one-grid kernels it
// changed the inlining (and so the register allocation) of theirs.
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "fetode_common.h"
#include "fetode_dopri_ctl.h"

using namespace fetode;

namespace {

#include "fetode_gridsum.h"

#include "fetode_bwd_dev.h"

// The full-grid shape, two trajectories per wave.  One wave per SIMD allowed for KAN-FET: at two the
// register allocation (the gradient sums, 64 VGPRs, stay live across every VJP) needs scratch; the
// launch is sized by the occupancy reached, fewer resident waves only mean more passes.
template <int D, int H, int K, int NB, int NG, bool FERRO>
__global__ __launch_bounds__(64 * kTPB) __attribute__((amdgpu_waves_per_eu(FERRO ? 1 : 2))) void dopri_bwd_mp_kernel(DopriBwdArgs da) {
  constexpr bool MP = D > 0;     // true, as a value-dependent constant (the body's `if constexpr (MP)`)
  constexpr int TPW = 2;
#include "fetode_dopri_bwd_body.h"
}

typedef void (*dopri_bwd_fn)(DopriBwdArgs);
// LV KAN-FET [2,10,2] K = 10 / LV KAN [2,10,2] (fetode_bwd.hip kBwd)
const dopri_bwd_fn kMpFn[2] = {dopri_bwd_mp_kernel<2, 10, 10, 10, 12, true>, dopri_bwd_mp_kernel<2, 10, 1, 10, 12, false>};
constexpr int kMpWords[2] = {BReg<BL<2, 10, 10, 10, 12, true>>::NW + BReg<BL<10, 2, 10, 10, 12, true>>::NW,
                             BReg<BL<2, 10, 1, 10, 12, false>>::NW + BReg<BL<10, 2, 1, 10, 12, false>>::NW};

}  // namespace

namespace fetode {

int64_t dopri_bwd_mp_resident_wgs(bool ferro) { return resident_wgs(kMpFn[ferro ? 0 : 1], 64 * kTPB); }

// the parking area of `vgrid` virtual workgroups: per virtual wave its 2 x 2 element records and
// its gradient-sum registers, lane-contiguous
int64_t dopri_bwd_mp_park_bytes(bool ferro, int64_t vgrid) {
  const int64_t nvw = vgrid * kTPB;
  return nvw * 2 * 2 * kMpElBytes + nvw * (int64_t)kMpWords[ferro ? 0 : 1] * 64 * (int64_t)sizeof(float);
}

hipError_t dopri_bwd_mp_launch(bool ferro, void* dopri_bwd_args, int64_t grid, hipStream_t s) {
  void* args[] = {dopri_bwd_args};
  return resident_launch((const void*)kMpFn[ferro ? 0 : 1], dim3((unsigned)grid), dim3(64 * kTPB), args, 0, s);
}

}  // namespace fetode
