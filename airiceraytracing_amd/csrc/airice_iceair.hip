// airice_iceair.hip -- the ice-to-air direct ray (IceRayTracing::GetDirectRayPar_Air,
// IceRayTracing.cc:2411) for a batch on gfx950: iceair_kernel, one (Tx depth, distance, Rx height)
// triple per lane.  The solve itself is airice_iceair.hpp, the same text the host route compiles.
//
// Like iceray_kernel it is latency-bound on dependent log / sqrt / asin / tan chains (one false
// position, 10 residual evaluations on average and 200 at most), so it wants resident waves: no
// LDS, no atomics, each column stored as soon as it is final.  Column c of triple i is
// out[c*ld + i]: a wave's store of one column is one contiguous 512-byte run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "airice.h"
#include "airice_iceair.hpp"
#include "airice_internal.h"

namespace airice {

namespace {

constexpr int kIceAirBlock = 256;

struct ColumnOut {
  double* base;  // &out[i]
  size_t ld;
  __device__ void put(int c, double x) { base[(size_t)c * ld] = x; }
};

__global__ __launch_bounds__(kIceAirBlock) void iceair_kernel(
    iceray::IceModel model, const double* __restrict__ z0, const double* __restrict__ x1,
    const double* __restrict__ h, size_t n, double* __restrict__ out, size_t ld,
    uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * kIceAirBlock + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = iceair::solve_triple(model, z0[i], x1[i], h[i], ColumnOut{out + i, ld});
  if (status != nullptr) status[i] = st;
}

}  // namespace

int launch_iceair(const double model[3], const double* z0, const double* x1, const double* h,
                  size_t n, double* out, size_t ld, uint8_t* status, hipStream_t st) {
  const iceray::IceModel m = {model[0], model[1], model[2]};
  const size_t blocks = (n + kIceAirBlock - 1) / kIceAirBlock;
  return bracket_launch(LC_ICEAIR, KT_ICEAIR, st, [&] {
    hipLaunchKernelGGL(iceair_kernel, dim3((unsigned)blocks), dim3(kIceAirBlock), 0, st, m, z0, x1,
                       h, n, out, ld, status);
  });
}

}  // namespace airice
