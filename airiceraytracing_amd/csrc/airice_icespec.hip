// airice_icespec.hip -- the ice attenuation of n pairs' two rays at F frequencies in ONE launch on
// gfx950: icesol_spectrum_kernel, over the solver's rows (iceray_kernel) and the two type columns
// icesol_kernel wrote for the same pairs.  The lane functions are airice_icespec.hpp, the text the
// host route compiles.
//
// A block owns `pairs` consecutive pairs (256 / min(F, 256) of them, at most kSpecMaxPairs) and
// runs two phases around one barrier:
//   A  lanes = nodes: record r = 96 p + 24 leg + node of the block goes to LDS, written once; the
//      log of the turning depth, the expm1 and the square roots are paid here, once per pair.
//   B  lanes = (pair, bin): item = F p + k; the lane forms its bin's three coefficients from
//      d_freq_ghz[k], walks its pair's 96 records -- every lane of a pair reads the same LDS
//      address, a broadcast -- with one exp each into one sum per leg, and stores two doubles at
//      att[(2 i + slot) ld_f + k]: consecutive lanes, consecutive bins.
// A leg that is empty (no such ray, a direct ray's second leg) is flagged in phase A and not walked
// in phase B.  Items beyond 256 (F > 256) are further passes of phase B over the same records.
// LDS: 1,552 bytes per pair (the records and the four legs' flags), at most 24.25 KiB a block.
// No atomics, no scratch, no register array indexed at run time.  DESIGN.md §12 has the
// measurements.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "airice.h"
#include "airice_icespec.hpp"
#include "airice_internal.h"

namespace airice {

namespace {

constexpr int kSpecBlock = 256;
constexpr int kSpecMaxPairs = 16;
constexpr size_t kSpecPairBytes =
    sizeof(icespec::Node) * icespec::kRecords + icespec::kLegs * sizeof(int);
constexpr int kSpecHas = 1, kSpecEmpty = 2;  // a leg's flags: its slot holds a ray; nothing to walk

struct ColumnIn {
  const double* base;  // &rays[i]
  size_t ld;
  __device__ double operator()(int c) const { return base[(size_t)c * ld]; }
};

__global__ __launch_bounds__(kSpecBlock) void icesol_spectrum_kernel(
    iceray::IceModel model, double a0, const double* __restrict__ z0,
    const double* __restrict__ z1, const double* __restrict__ rays, size_t ld_rays,
    const double* __restrict__ sol, size_t ld_sol, size_t n, const double* __restrict__ freq,
    unsigned n_freq, unsigned pairs, double* __restrict__ att, size_t ld_f) {
  extern __shared__ double2 spec_lds[];  // pairs x 96 records, then pairs x 4 flags
  icespec::Node* rec = reinterpret_cast<icespec::Node*>(spec_lds);
  int* flag = reinterpret_cast<int*>(rec + (size_t)pairs * icespec::kRecords);

  const size_t first = (size_t)blockIdx.x * pairs;
  const unsigned here = n - first < pairs ? (unsigned)(n - first) : pairs;

  // ---- A: the block's records
  for (unsigned r = threadIdx.x; r < here * icespec::kRecords; r += kSpecBlock) {
    const unsigned p = r / icespec::kRecords, in_pair = r - p * icespec::kRecords;
    const int k = (int)(in_pair / icespec::kNodes), j = (int)(in_pair - k * icespec::kNodes);
    const size_t i = first + p;
    const ColumnIn ray{rays + i, ld_rays};
    icespec::Node v;
    int f = kSpecHas;
    if (!(ray(iceray::kColStatus) < (double)iceray::kNonFinite)) {  // the solver ran no search
      v.t = v.g = iceray::quiet_nan();
    } else {
      const icespec::SlotRay s =
          icespec::slot_ray(ray, sol[(size_t)(icesol::kColType + (k >> 1)) * ld_sol + i]);
      const icespec::Panel panel =
          icespec::leg_panel(model, icespec::pair_leg(k, s, z0[i], z1[i]));
      v = icespec::node_record(model, panel, j);
      f = (s.has ? kSpecHas : 0) | (panel.hw == 0.0 ? kSpecEmpty : 0);
    }
    rec[r] = v;
    if (j == 0) flag[icespec::kLegs * p + k] = f;
  }
  __syncthreads();

  // ---- B: one (pair, bin) per lane and pass
  const unsigned items = here * n_freq;
  for (unsigned item = threadIdx.x; item < items; item += kSpecBlock) {
    const unsigned p = item / n_freq, k = item - p * n_freq;
    const icespec::Coeffs c = icespec::spectrum_coeffs(freq[k]);
    const icespec::Node* r = rec + p * icespec::kRecords;
    const int* f = flag + icespec::kLegs * p;
    double* o = att + 2 * (first + p) * ld_f + k;
    const double leg0 = icespec::leg_sum(c, r, (f[0] & kSpecEmpty) != 0);
    const double leg1 = icespec::leg_sum(c, r + icespec::kNodes, (f[1] & kSpecEmpty) != 0);
    o[0] = icespec::attenuation(a0, (f[0] & kSpecHas) != 0, leg0, leg1);
    const double leg2 = icespec::leg_sum(c, r + 2 * icespec::kNodes, (f[2] & kSpecEmpty) != 0);
    const double leg3 = icespec::leg_sum(c, r + 3 * icespec::kNodes, (f[3] & kSpecEmpty) != 0);
    o[ld_f] = icespec::attenuation(a0, (f[2] & kSpecHas) != 0, leg2, leg3);
  }
}

}  // namespace

unsigned icespec_pairs_per_block(size_t n_freq) {
  const size_t lanes = n_freq < (size_t)kSpecBlock ? n_freq : (size_t)kSpecBlock;
  const size_t pairs = (size_t)kSpecBlock / lanes;
  return (unsigned)(pairs < (size_t)kSpecMaxPairs ? pairs : (size_t)kSpecMaxPairs);
}

int launch_icespec(const double model[3], double a0, const double* z0, const double* z1,
                   const double* rays, size_t ld_rays, const double* sol, size_t ld_sol, size_t n,
                   const double* freq, size_t n_freq, double* att, size_t ld_f, hipStream_t st) {
  const iceray::IceModel m = {model[0], model[1], model[2]};
  const unsigned pairs = icespec_pairs_per_block(n_freq);
  const size_t blocks = (n + pairs - 1) / pairs;
  return bracket_launch(LC_ICESPEC, KT_ICESPEC, st, [&] {
    hipLaunchKernelGGL(icesol_spectrum_kernel, dim3((unsigned)blocks), dim3(kSpecBlock),
                       kSpecPairBytes * pairs, st, m, a0, z0, z1, rays, ld_rays, sol, ld_sol, n,
                       freq, (unsigned)n_freq, pairs, att, ld_f);
  });
}

}  // namespace airice
