// airice_iceray.hip -- the in-ice ray solver (IceRayTracing::IceRayTracing, IceRayTracing.cc:1745)
// for a batch on gfx950: iceray_kernel, one (Tx, Rx) pair per lane.  The solver itself is
// airice_iceray.hpp, the same text the host route compiles.
//
// The kernel is latency-bound on dependent log / sqrt / divide chains (10 to a few hundred
// residual evaluations per pair), so what it needs is resident waves: no LDS, no atomics, and no
// 32-double output row held in registers -- each ray's columns are stored as soon as that ray is
// final.  Column c of pair i is out[c*ld + i], so a wave's store of one column is one contiguous
// 512-byte run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "airice.h"
#include "airice_iceray.hpp"
#include "airice_internal.h"

namespace airice {

namespace {

constexpr int kIceRayBlock = 256;

struct ColumnOut {
  double* base;  // &out[i]
  size_t ld;
  __device__ void put(int c, double x) { base[(size_t)c * ld] = x; }
};

// Three waves per SIMD is what the solver's live state admits without scratch (a
// bound of 4 spills 40 registers); stated so the allocator stays within the 168-register step.
__global__ __launch_bounds__(kIceRayBlock, 3) void iceray_kernel(
    iceray::IceModel model, const double* __restrict__ z0, const double* __restrict__ x1,
    const double* __restrict__ z1, size_t n, double* __restrict__ out, size_t ld,
    uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * kIceRayBlock + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = iceray::solve_pair(model, z0[i], x1[i], z1[i], ColumnOut{out + i, ld});
  if (status != nullptr) status[i] = st;
}

}  // namespace

int launch_iceray(const double model[3], const double* z0, const double* x1, const double* z1,
                  size_t n, double* out, size_t ld, uint8_t* status, hipStream_t st) {
  const iceray::IceModel m = {model[0], model[1], model[2]};
  const size_t blocks = (n + kIceRayBlock - 1) / kIceRayBlock;
  return bracket_launch(LC_ICERAY, KT_ICERAY, st, [&] {
    hipLaunchKernelGGL(iceray_kernel, dim3((unsigned)blocks), dim3(kIceRayBlock), 0, st, m, z0, x1,
                       z1, n, out, ld, status);
  });
}

}  // namespace airice
