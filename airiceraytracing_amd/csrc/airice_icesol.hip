// airice_icesol.hip -- IceRayTracing::GetRayTracingSolutions and GetFocusingFactor
// (IceRayTracing.cc:2907, 3218) for a batch on gfx950: icesol_kernel, one (Tx, Rx) pair per lane,
// over the columns iceray_kernel wrote for the batch (and, for the focusing factors, for the
// receivers 1 cm lower).  The lane's function is airice_icesol.hpp, the same text the host route
// compiles.
//
// The rows are column-major on both sides: column c of pair i is rays[c*ld_rays + i] and
// out[c*ld + i], so a wave's read or store of one column is one contiguous 512-byte run (a chosen
// ray's columns: up to four runs, one per ray the wave's lanes chose).  No LDS, no atomics; the
// live state is the two chosen rays and one leg's sum, and each output column is stored as soon
// as it is final.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "airice.h"
#include "airice_icesol.hpp"
#include "airice_internal.h"

namespace airice {

namespace {

constexpr int kIceSolBlock = 256;

struct ColumnIn {
  const double* base;  // &rays[i]
  size_t ld;
  __device__ double operator()(int c) const { return base[(size_t)c * ld]; }
};
struct ColumnOut {
  double* base;  // &out[i]
  size_t ld;
  __device__ void put(int c, double x) { base[(size_t)c * ld] = x; }
};

// Four waves per SIMD (at most 128 registers): DESIGN.md §9 has what the compiler took.
__global__ __launch_bounds__(kIceSolBlock, 4) void icesol_kernel(
    iceray::IceModel model, icesol::Medium medium, const double* __restrict__ z0,
    const double* __restrict__ x1, const double* __restrict__ z1,
    const double* __restrict__ rays, size_t ld_rays, const double* __restrict__ rays_lower,
    size_t ld_lower, size_t n, double* __restrict__ out, size_t ld,
    uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * kIceSolBlock + threadIdx.x;
  if (i >= n) return;
  const bool have_lower = rays_lower != nullptr;
  const uint8_t st = icesol::solve_pair(
      model, medium, z0[i], x1[i], z1[i], ColumnIn{rays + i, ld_rays}, have_lower,
      ColumnIn{have_lower ? rays_lower + i : rays + i, have_lower ? ld_lower : ld_rays},
      ColumnOut{out + i, ld});
  if (status != nullptr) status[i] = st;
}

}  // namespace

int launch_icesol(const double model[3], double a0, double frequency_ghz, const double* z0,
                  const double* x1, const double* z1, const double* rays, size_t ld_rays,
                  const double* rays_lower, size_t ld_lower, size_t n, double* out, size_t ld,
                  uint8_t* status, hipStream_t st) {
  const iceray::IceModel m = {model[0], model[1], model[2]};
  const icesol::Medium q = icesol::make_medium(a0, frequency_ghz);  // uniform over the batch
  const size_t blocks = (n + kIceSolBlock - 1) / kIceSolBlock;
  return bracket_launch(LC_ICESOL, KT_ICESOL, st, [&] {
    hipLaunchKernelGGL(icesol_kernel, dim3((unsigned)blocks), dim3(kIceSolBlock), 0, st, m, q, z0,
                       x1, z1, rays, ld_rays, rays_lower, ld_lower, n, out, ld, status);
  });
}

}  // namespace airice
