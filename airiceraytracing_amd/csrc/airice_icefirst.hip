// airice_icefirst.hip -- the first-arriving ray between 3-D points (IceRayTracing::DirectRayTracer,
// IceRayTracing.cc:2502) for a batch on gfx950, as three launches over a caller's work buffer:
//
//   icefirst_geom_kernel    one pair per lane: (z0, x1, z1) = (zT, sqrt(dx^2 + dy^2), zR) into the
//                           work buffer.  Elementwise pairs read 48 B and write 24 B; cross pairs
//                           (pair t*n_rx + r) read each emitter once per wave row from cache.
//   iceray_kernel           airice_iceray.hip's, unchanged, over those triples: 32 columns per
//                           pair into the work buffer
//   icefirst_select_kernel  one pair per lane: the reference's choice among D, Ra0 and Ra1.  It
//                           reads the status column, up to three receive angles and times and the
//                           winner's three values (40-88 B) and x1, writes 64 B + a status byte.
//
// Both kernels here are memory-bound and tiny beside the solve; blocks of 256, no LDS, no atomics.
// Work buffer, in doubles, n = pairs:  z0 [n] | x1 [n] | z1 [n] | rays [32 n] (column stride n).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "airice.h"
#include "airice_icefirst.hpp"
#include "airice_internal.h"

namespace airice {

namespace {

constexpr int kIceFirstBlock = 256;

__global__ __launch_bounds__(kIceFirstBlock) void icefirst_geom_kernel(
    const double* __restrict__ tx_x, const double* __restrict__ tx_y,
    const double* __restrict__ tx_z, const double* __restrict__ rx_x,
    const double* __restrict__ rx_y, const double* __restrict__ rx_z, size_t n_rx, int cross,
    size_t n, double* __restrict__ z0, double* __restrict__ x1, double* __restrict__ z1) {
  const size_t i = (size_t)blockIdx.x * kIceFirstBlock + threadIdx.x;
  if (i >= n) return;
  const size_t t = cross ? i / n_rx : i;
  const size_t r = cross ? i - t * n_rx : i;
  z0[i] = tx_z[t];
  x1[i] = icefirst::horizontal_distance(tx_x[t], tx_y[t], rx_x[r], rx_y[r]);
  z1[i] = rx_z[r];
}

__global__ __launch_bounds__(kIceFirstBlock) void icefirst_select_kernel(
    const double* __restrict__ rays, size_t ld_rays, const double* __restrict__ x1, size_t n,
    double* __restrict__ out, size_t ld, uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * kIceFirstBlock + threadIdx.x;
  if (i >= n) return;
  const double* row = rays + i;
  double* o = out + i;
  const uint8_t st = icefirst::select_first(
      [row, ld_rays](int c) { return row[(size_t)c * ld_rays]; }, x1[i],
      [o, ld](int c, double v) { o[(size_t)c * ld] = v; });
  if (status != nullptr) status[i] = st;
}

}  // namespace

int launch_icefirst_select(const double* rays, size_t ld_rays, const double* x1, size_t n,
                           double* out, size_t ld, uint8_t* status, hipStream_t st) {
  const dim3 grid((unsigned)((n + kIceFirstBlock - 1) / kIceFirstBlock)), block(kIceFirstBlock);
  return bracket_launch(LC_ICEFIRST_SELECT, KT_ICEFIRST_SELECT, st, [&] {
    hipLaunchKernelGGL(icefirst_select_kernel, grid, block, 0, st, rays, ld_rays, x1, n, out, ld,
                       status);
  });
}

int launch_icefirst(const double model[3], const double* tx_x, const double* tx_y,
                    const double* tx_z, const double* rx_x, const double* rx_y,
                    const double* rx_z, size_t n_rx, bool cross, size_t n, double* work,
                    double* out, size_t ld, uint8_t* status, hipStream_t st) {
  double* z0 = work;
  double* x1 = work + n;
  double* z1 = work + 2 * n;
  double* rays = work + 3 * n;
  const dim3 grid((unsigned)((n + kIceFirstBlock - 1) / kIceFirstBlock)), block(kIceFirstBlock);
  if (int rc = bracket_launch(LC_ICEFIRST_GEOM, KT_ICEFIRST_GEOM, st, [&] {
        hipLaunchKernelGGL(icefirst_geom_kernel, grid, block, 0, st, tx_x, tx_y, tx_z, rx_x, rx_y,
                           rx_z, n_rx, cross ? 1 : 0, n, z0, x1, z1);
      }))
    return rc;
  if (int rc = launch_iceray(model, z0, x1, z1, n, rays, n, nullptr, st)) return rc;
  return launch_icefirst_select(rays, n, x1, n, out, ld, status, st);
}

}  // namespace airice
