// airice_icepath.hip -- the in-ice ray-path samplers (IceRayTracing::GetFull*RayPath,
// IceRayTracing.cc:1257-1712) for a batch on gfx950, mapped as ray_consts_kernel /
// ray_paths_kernel of airice_path.hip are.  The sampler itself is airice_icepath.hpp, the same
// text the host route compiles.
//
//  icepath_consts_kernel : one lane per (pair, kind) segment, s = 4 i + r.  Reads the solver's row
//                          (L from column 19 + r, zmax from 23 / 24, the status from 29) and the
//                          pair's (z0, x1, z1); writes the segment's record (flip, the leg-1 and
//                          total counts, F(z0), the surface or apex term, sqrt(A^2 - L^2),
//                          (L / C) / sqrt(A^2 - L^2)) and its count.
//  icepath_kernel        : one lane per sample slot, one host-built tile (<= 256 consecutive slots
//                          of one segment) per block.  The segment index is block-uniform, so the
//                          record comes through uniform loads and each wave stores 64 consecutive
//                          x and z.  Per sample one exp, one log, one sqrt and, on a refracted
//                          ray, one expm1.  A lane at or past the segment's count exits without
//                          storing; the consts kernel zeroes a count above the segment's capacity,
//                          so no store lands outside [offsets[s], offsets[s + 1]).
//
// The capacities are host bookkeeping (airice_icepath_plan): the direct and reflected counts depend
// on the depths alone, a refracted ray's is bounded without its turning depth, so the launch is
// stream-ordered behind the solver with no copy back.  No LDS, no atomics, 64-bit indices.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "airice.h"
#include "airice_hostcall.hpp"
#include "airice_icepath.hpp"
#include "airice_internal.h"

namespace airice {

namespace {

constexpr int kIcePathBlock = 256;
constexpr int kIceConstsBlock = 64;

// Workspace (d_work of airice_icepath_launch), in this order: the 4 n + 1 offsets and the tile
// list (host-planned, uploaded by the launch), then the 4 n records icepath_consts_kernel writes.
struct SegRecord {
  icepath::Segment s;
  long long base;  // offsets[s]: the segment's first slot in x / z
};
// One block of icepath_kernel: slots [tile * 256, (tile + 1) * 256) of segment `seg`.  A segment
// of capacity c has ceil(c / 256) tiles.
struct SegTile {
  int seg, tile;
};
static_assert(sizeof(SegRecord) % 16 == 0, "workspace alignment");

__global__ __launch_bounds__(kIceConstsBlock) void icepath_consts_kernel(
    iceray::IceModel model, const double* __restrict__ z0, const double* __restrict__ x1,
    const double* __restrict__ z1, const double* __restrict__ rays, size_t ld, size_t n, int mask,
    const int64_t* __restrict__ offsets, SegRecord* __restrict__ recs,
    int64_t* __restrict__ count) {
  const size_t s = (size_t)blockIdx.x * kIceConstsBlock + threadIdx.x;
  if (s >= 4 * n) return;
  const size_t i = s >> 2;
  const int r = (int)(s & 3);
  const double sv = rays[(size_t)iceray::kColStatus * ld + i];
  const int st = (sv >= 0.0 && sv < 256.0) ? (int)sv : iceray::kNonFinite;
  const double L = rays[(size_t)(19 + r) * ld + i];
  const double zmax = r >= 2 ? rays[(size_t)(21 + r) * ld + i] : 0.0;
  SegRecord R;
  R.s = icepath::make_segment(model, r, z0[i], x1[i], z1[i], L, zmax);
  R.base = offsets[s];
  const bool take = ((mask >> r) & 1) && ((st >> r) & 1) && !(st & iceray::kNonFinite);
  if (!take || R.s.count > offsets[s + 1] - R.base) R.s.count = 0;
  recs[s] = R;
  count[s] = R.s.count;
}

__global__ __launch_bounds__(kIcePathBlock) void icepath_kernel(
    iceray::IceModel model, const SegRecord* __restrict__ recs, const SegTile* __restrict__ tiles,
    double* __restrict__ xs, double* __restrict__ zs) {
  const SegTile t = tiles[blockIdx.x];
  const SegRecord& R = recs[t.seg];
  const long long k = (long long)t.tile * kIcePathBlock + threadIdx.x;
  if (k >= R.s.count) return;
  double x, z;
  icepath::sample(model, R.s, k, x, z);
  xs[R.base + k] = x;
  zs[R.base + k] = z;
}

size_t round16(size_t b) { return (b + 15) / 16 * 16; }

size_t icepath_work_bytes(size_t n, long long tiles) {
  return round16((4 * n + 1) * sizeof(int64_t)) + round16((size_t)tiles * sizeof(SegTile)) +
         4 * n * sizeof(SegRecord);
}

constexpr size_t kMaxPairs = (size_t)1 << 29;  // 4 n segments in an int
int too_many_pairs(size_t n) {
  if (n < kMaxPairs) return AIRICE_OK;
  set_error("icepath: %zu pairs exceed one launch", n);
  return AIRICE_EINVAL;
}

// The host plan: the capacity of every segment, the running offsets and the tile count.
int plan_icepath(const double* z0, const double* z1, const uint8_t* status, size_t n, int mask,
                 int64_t* offsets, long long* tiles_out) {
  if (int rc = too_many_pairs(n)) return rc;
  long long total = 0, tiles = 0;
  offsets[0] = 0;
  for (size_t i = 0; i < n; ++i) {
    const int st = status != nullptr ? status[i] : 15;
    const bool row = !(st & iceray::kNonFinite);
    const long long d = icepath::count_direct(z0[i], z1[i]);
    const long long r = icepath::count_reflected(z0[i], z1[i]);
    const long long a = icepath::bound_refracted(z0[i], z1[i]);
    const long long caps[4] = {d, r, a, a};
    for (int k = 0; k < 4; ++k) {
      const bool take = row && ((mask >> k) & 1) && ((st >> k) & 1);
      const long long c = take ? caps[k] : 0;
      total += c;  // c <= 200,004, 4 n < 2^31: no overflow
      tiles += (c + kIcePathBlock - 1) / kIcePathBlock;
      offsets[4 * i + k + 1] = total;
    }
  }
  if (tiles > 0x7fffffffLL) {
    set_error("icepath: %lld sample tiles exceed one launch", tiles);
    return AIRICE_EINVAL;
  }
  *tiles_out = tiles;
  return AIRICE_OK;
}

}  // namespace

}  // namespace airice

using namespace airice;

extern "C" {

int airice_icepath_plan(const double* z0, const double* z1, const uint8_t* status, size_t n,
                        int ray_mask, int64_t* offsets, size_t* work_bytes) {
  if (int rc = null_argument("icepath plan", {{"offsets", offsets}})) return rc;
  if (n > 0)
    if (int rc = null_argument("icepath plan", {{"z0", z0}, {"z1", z1}})) return rc;
  long long tiles = 0;
  if (int rc = plan_icepath(z0, z1, status, n, ray_mask, offsets, &tiles)) return rc;
  if (work_bytes != nullptr) *work_bytes = icepath_work_bytes(n, tiles);
  return AIRICE_OK;
}

int airice_icepath_launch(const double* model3, const double* d_z0, const double* d_x1,
                          const double* d_z1, const double* d_rays, size_t ld_rays,
                          const double* z0, const double* z1, const uint8_t* status, size_t n,
                          int ray_mask, const int64_t* offsets, void* d_work, size_t work_bytes,
                          int64_t* d_count, double* d_x, double* d_z, size_t cap, void* stream) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("icepath", {{"d_z0", d_z0}, {"d_x1", d_x1}, {"d_z1", d_z1},
                                         {"d_rays", d_rays}, {"z0", z0}, {"z1", z1},
                                         {"offsets", offsets}, {"d_work", d_work},
                                         {"d_count", d_count}, {"d_x", d_x}, {"d_z", d_z}}))
    return rc;
  if (int rc = short_stride("icepath", "ld_rays", ld_rays, n)) return rc;
  if ((reinterpret_cast<uintptr_t>(d_work) & 15) != 0) {
    set_error("icepath: d_work is not 16-byte aligned");
    return AIRICE_EINVAL;
  }
  if (int rc = too_many_pairs(n)) return rc;
  std::vector<int64_t> planned(4 * n + 1);
  long long tiles = 0;
  if (int rc = plan_icepath(z0, z1, status, n, ray_mask, planned.data(), &tiles)) return rc;
  for (size_t s = 0; s <= 4 * n; ++s)
    if (offsets[s] != planned[s]) {
      set_error("icepath: offsets[%zu] = %lld is not the plan of these pairs (%lld)", s,
                (long long)offsets[s], (long long)planned[s]);
      return AIRICE_EINVAL;
    }
  const long long total = planned[4 * n];
  if ((unsigned long long)total > cap) {
    set_error("icepath: cap of %zu samples, the plan holds %lld", cap, total);
    return AIRICE_EINVAL;
  }
  const size_t need = icepath_work_bytes(n, tiles);
  if (work_bytes < need) {
    set_error("icepath: work_bytes of %zu bytes, need %zu", work_bytes, need);
    return AIRICE_EINVAL;
  }
  if (total == 0) return AIRICE_OK;
  const hipStream_t st = (hipStream_t)stream;
  const size_t off_bytes = round16((4 * n + 1) * sizeof(int64_t));
  const size_t tile_bytes = round16((size_t)tiles * sizeof(SegTile));
  char* w = static_cast<char*>(d_work);
  int64_t* d_off = reinterpret_cast<int64_t*>(w);
  SegTile* d_tiles = reinterpret_cast<SegTile*>(w + off_bytes);
  SegRecord* d_recs = reinterpret_cast<SegRecord*>(w + off_bytes + tile_bytes);
  std::vector<SegTile> tl;
  tl.reserve((size_t)tiles);
  for (size_t s = 0; s < 4 * n; ++s) {
    const long long c = planned[s + 1] - planned[s];
    for (long long t = 0; t * kIcePathBlock < c; ++t) tl.push_back(SegTile{(int)s, (int)t});
  }
  // (a copy from pageable memory returns once the source has been read)
  HIP_TRY(hipMemcpyAsync(d_off, planned.data(), (4 * n + 1) * sizeof(int64_t),
                         hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_tiles, tl.data(), tl.size() * sizeof(SegTile), hipMemcpyHostToDevice,
                         st));
  const double* m3 = ice_model_or_default(model3);
  const iceray::IceModel m = {m3[0], m3[1], m3[2]};
  const unsigned cgrid = (unsigned)((4 * n + kIceConstsBlock - 1) / kIceConstsBlock);
  const int rc = bracket_launch(LC_ICEPATH_CONSTS, KT_ICEPATH_CONSTS, st, [&] {
    hipLaunchKernelGGL(icepath_consts_kernel, dim3(cgrid), dim3(kIceConstsBlock), 0, st, m, d_z0,
                       d_x1, d_z1, d_rays, ld_rays, n, ray_mask, d_off, d_recs, d_count);
  });
  if (rc) return rc;
  return bracket_launch(LC_ICEPATH, KT_ICEPATH, st, [&] {
    hipLaunchKernelGGL(icepath_kernel, dim3((unsigned)tiles), dim3(kIcePathBlock), 0, st, m,
                       d_recs, d_tiles, d_x, d_z);
  });
}

int airice_icepath_host(const double* model3, const double* z0, const double* x1, const double* z1,
                        const double* rays, size_t ld_rays, const uint8_t* status, size_t n,
                        int ray_mask, const int64_t* offsets, int64_t* count, double* x, double* z,
                        size_t cap) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("icepath", {{"z0", z0}, {"x1", x1}, {"z1", z1}, {"rays", rays},
                                         {"offsets", offsets}, {"count", count}, {"x", x},
                                         {"z", z}}))
    return rc;
  if (int rc = short_stride("icepath", "ld_rays", ld_rays, n)) return rc;
  if (int rc = too_many_pairs(n)) return rc;
  std::vector<int64_t> planned(4 * n + 1);
  long long tiles = 0;
  if (int rc = plan_icepath(z0, z1, status, n, ray_mask, planned.data(), &tiles)) return rc;
  const size_t total = (size_t)planned[4 * n];
  if (total > cap) {
    set_error("icepath: cap of %zu samples, the plan holds %zu", cap, total);
    return AIRICE_EINVAL;
  }
  constexpr int kF = AIRICE_ICERAY_FIELDS;
  const size_t work_bytes = icepath_work_bytes(n, tiles);
  DevBuffer work, vals;  // vals: z0, x1, z1, the 32 solver columns, x, z, then the counts
  HIP_TRY(work.alloc(work_bytes));
  HIP_TRY(vals.alloc(sizeof(double) * ((3 + kF) * n + 2 * total) + sizeof(int64_t) * 4 * n));
  double* d_in = static_cast<double*>(vals.p);
  double* d_rays = d_in + 3 * n;
  double* dx = d_rays + (size_t)kF * n;
  double* dz = dx + total;
  int64_t* d_count = reinterpret_cast<int64_t*>(dz + total);
  HIP_TRY(hipMemcpy(d_in, z0, sizeof(double) * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_in + n, x1, sizeof(double) * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_in + 2 * n, z1, sizeof(double) * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy2D(d_rays, sizeof(double) * n, rays, sizeof(double) * ld_rays,
                      sizeof(double) * n, (size_t)kF, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_count, 0, sizeof(int64_t) * 4 * n));  // a plan of no samples launches nothing
  if (int rc = airice_icepath_launch(model3, d_in, d_in + n, d_in + 2 * n, d_rays, n, z0, z1,
                                     status, n, ray_mask, offsets, work.p, work_bytes, d_count, dx,
                                     dz, total, nullptr))
    return rc;
  // the copies back are on the null stream, like the launch: they wait for the kernels
  HIP_TRY(hipMemcpy(count, d_count, sizeof(int64_t) * 4 * n, hipMemcpyDeviceToHost));
  if (total > 0) {
    HIP_TRY(hipMemcpy(x, dx, sizeof(double) * total, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(z, dz, sizeof(double) * total, hipMemcpyDeviceToHost));
  }
  return AIRICE_OK;
}

}  // extern "C"
