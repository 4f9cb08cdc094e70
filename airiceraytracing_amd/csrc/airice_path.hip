// airice_path.hip -- SingleRayAirIceRefraction (BASELINE cfg1) on gfx950: the forward trace of
// one launch angle with the RayTracingFunctions numerics, and the x(z) ray-path sampler that
// writes RayPathinAirnIce.txt (SingleRayAirIceRefraction.C:33-299).
//
//  single_ray_kernel : one lane.  Layer loop (.C:100-154: GetLayerHitPointPar for the Tx layer,
//                      the same L below, RayTracingFunctions.cc:399-514 / :349-369), the ice leg
//                      (GetIcePropagationPar, RayTracingFunctions.cc:661-679, positive depth),
//                      and the per-layer constants of the sampler: fDnfR at each layer's start
//                      height and the running x offset (LastRefracted_x, .C:285).
//  path_kernel       : one lane per path sample (1 m steps, ~17k for cfg1): its layer from
//                      the host-computed sample ranges, then one fDnfR (.C:254-258, 293-297).
//  ray_consts_kernel : the batch (airice_ray_paths_launch): one lane per ray, the same per-ray
//                      constants (the __device__ ray_consts both kernels call) and the summary
//                      columns.
//  ray_paths_kernel  : one lane per sample of the whole batch, one host-built tile (<= 256
//                      consecutive samples of one ray) per block, the same per-sample evaluation
//                      (the __device__ path_sample both kernels call).
//
// The sample count and each layer's start/stop heights are integer/height bookkeeping of the
// reference's own loops (.C:226-299) and are done on the host so the output can be sized; every
// refractive-index / ray quantity is computed on the device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "airice.h"
#include "airice_internal.h"

namespace airice {

namespace {

constexpr double kSpeedC = 299792458.0;  // RayTracingFunctions.h spedc
constexpr int kPathBlock = 256;
constexpr int kConstsBlock = 64;

struct PathPlan {
  int top;           // MaxLayers - SkipLayersAbove - 1 (first air layer of the trace, .C:100)
  int bot;           // SkipLayersBelow
  int nl;            // path layers = MaxLayers - SkipLayersAbove - SkipLayersBelow (.C:226)
  int pad_;
  double txh, ice, depth, launch;
  double start[kMaxLayers], stop[kMaxLayers];  // path layer il: LayerStart/StopHeight
  long long first[kMaxLayers + 1];             // first sample of path layer il; first[nl] = n_air
  long long n_ice;
};

// Device copy of the sampler constants (written by single_ray_kernel, read by path_kernel).
struct PathConsts {
  double summary[AIRICE_SINGLE_RAY_FIELDS];
  double L;
  double fstart[kMaxLayers];  // fDnfR(-LayerStartHeight, ...) of path layer il
  double off[kMaxLayers];     // LastRefracted_x entering path layer il
  double off_ice;             // LastRefracted_x after the air layers
  double fice0;               // fDnfR(0, A_ice, B_ice, C_ice, L)
};

// fDnfR (RayTracingFunctions.cc:293-302), pow(y,2) == y*y.
__device__ __forceinline__ double fDnfR(double x, double A, double B, double C, double L) {
  const double y = A + B * exp(C * x);
  return (L / C) * (1.0 / sqrt(A * A - L * L)) *
         (C * x - log(A * (A + B * exp(C * x)) - L * L + sqrt(A * A - L * L) * sqrt(y * y - L * L)));
}

__device__ __forceinline__ double B_air(const DevMedium& M, double z) {
  return sel5(M.B, air_layer(M, fabs(z)));
}
__device__ __forceinline__ double C_air(const DevMedium& M, double z) {  // +C (GetC_air)
  return -sel5(M.negC, air_layer(M, fabs(z)));
}
__device__ __forceinline__ double nz_air(const DevMedium& M, double z) {
  const double zabs = fabs(z);
  return M.A_air + B_air(M, zabs) * exp(-C_air(M, zabs) * zabs);
}
__device__ __forceinline__ double nz_ice(const DevMedium& M, double z) {
  z = fabs(z);
  return M.A_ice + M.B_ice * exp(M.negC_ice * z);
}

// GetRayOpticalPath (RayTracingFunctions.cc:349-369): the horizontal distance of a segment.
__device__ __forceinline__ double ray_path(const DevMedium& M, double A, double Rx, double Tx,
                                           double L, bool air) {
  double x1;
  if (air) {
    x1 = +fDnfR(Rx, A, B_air(M, Rx), -C_air(M, Rx), L) - fDnfR(Tx, A, B_air(M, Tx), -C_air(M, Tx), L);
    x1 *= -1;
  } else {
    x1 = +fDnfR(Rx, A, M.B_ice, M.negC_ice, L) - fDnfR(Tx, A, M.B_ice, M.negC_ice, L);
  }
  return x1;
}

// ftimeD, ice variant (RayTracingFunctions.cc:339-341)
__device__ __forceinline__ double ftimeD_ice(const DevMedium& M, double x, double A, double C,
                                             double L) {
  const double n = nz_ice(M, x);
  const double n2 = n * n;
  return (1.0 / (kSpeedC * C * sqrt(n2 - L * L))) *
         (n2 - L * L +
          (C * x - log(A * n - L * L + sqrt(A * A - L * L) * sqrt(n2 - L * L))) *
              (A * A * sqrt(n2 - L * L)) / sqrt(A * A - L * L) +
          A * sqrt(n2 - L * L) * log(n + sqrt(n2 - L * L)));
}

// The per-ray constants: the air layer loop (.C:100-154), the ice leg and the sampler constants
// of one ray, written to *out.  Shared by single_ray_kernel (P a kernel argument) and
// ray_consts_kernel (P a record of the batch's workspace).
__device__ __forceinline__ void ray_consts(const DevMedium& M, const PathPlan& P, double launch,
                                           PathConsts* __restrict__ out) {
  const double r2d = M.r2d;
  double thd_air = 0.0, start_angle = 0.0, L = 0.0;
  // the air layer loop (.C:100-154)
  for (int il = P.top; il > P.bot - 1; --il) {
    const double start_h = (il == P.top) ? P.txh : M.atm[il + 1] - 0.00001;
    const double start_n = nz_air(M, start_h);
    // (both loaded, then chosen: a choice between the two addresses would tie the plan and the
    // medium together and keep single_ray_kernel's argument copies of both in scratch)
    const double ice_h = P.ice, atm_h = M.atm[il];
    const double stop_h = (il == P.bot) ? ice_h : atm_h;
    if (il == P.top) {
      // GetLayerHitPointPar (RayTracingFunctions.cc:399-514), air
      const double inc = (180 - launch) * M.d2r;
      const double nzRx = nz_air(M, stop_h), nzTx = nz_air(M, start_h);
      const double lang = asin((start_n / nzTx) * sin(inc));
      const double recv = asin((nz_air(M, start_h) * sin(lang)) / nz_air(M, stop_h));
      L = nzRx * sin(recv);
      thd_air += ray_path(M, M.A_air, stop_h, start_h, L, true);
      start_angle = recv * r2d;
    } else {
      const double rec = asin(L / nz_air(M, stop_h)) * r2d;
      thd_air += ray_path(M, M.A_air, stop_h, start_h, L, true);
      start_angle = rec;
    }
  }
  // GetIcePropagationPar (RayTracingFunctions.cc:661-679)
  const double thd_ice = ray_path(M, M.A_ice, P.depth, 0.0, L, false);
  const double recv_ice = asin(L / nz_ice(M, P.depth)) * r2d;
  const double t_ice = +ftimeD_ice(M, P.depth, M.A_ice, M.negC_ice, L) -
                       ftimeD_ice(M, 0.0, M.A_ice, M.negC_ice, L);
  out->summary[0] = thd_air;
  out->summary[1] = L;
  out->summary[2] = start_angle;
  out->summary[3] = thd_ice;
  out->summary[4] = recv_ice;
  out->summary[5] = t_ice;
  out->L = L;
  // sampler constants (.C:226-299): layerLs[il] == L for every layer, LvalueIce == L
  double last_x = 0.0;
  for (int il = 0; il < P.nl; ++il) {
    const double s = P.start[il];
    const double fs = fDnfR(-(s), M.A_air, B_air(M, -(s)), C_air(M, -(s)), L);
    out->fstart[il] = fs;
    out->off[il] = last_x;
    if (P.first[il + 1] > P.first[il]) {  // the layer's last sample sits at its stop height
      const double i = P.stop[il];
      last_x = fDnfR(-i, M.A_air, B_air(M, -i), C_air(M, -i), L) - fs + last_x;
    }
  }
  out->off_ice = last_x;
  out->fice0 = fDnfR(0, M.A_ice, M.B_ice, -M.negC_ice, L);
}

// Path sample k (0 <= k < n_air + n_ice) of one ray: its layer from the plan's sample ranges,
// then one fDnfR (.C:254-258, 293-297).  Shared by path_kernel and ray_paths_kernel.
__device__ __forceinline__ void path_sample(const DevMedium& M, const PathPlan& P,
                                            const PathConsts* __restrict__ c, long long k,
                                            double& x, double& z) {
  const long long n_air = P.first[P.nl];
  const double L = c->L;
  if (k < n_air) {
    int il = 0;
#pragma unroll
    for (int l = 1; l < kMaxLayers; ++l)
      if (l < P.nl && k >= P.first[l]) il = l;
    // i = LayerStartHeight - j equals the reference's repeated i = i - 1 (each step is exact)
    double i = P.start[il] - (double)(k - P.first[il]);
    if (i < P.stop[il]) i = P.stop[il];
    x = fDnfR(-i, M.A_air, B_air(M, -i), C_air(M, -i), L) - c->fstart[il] + c->off[il];
    z = i;
  } else {
    const int i = -(int)(k - n_air);
    x = c->off_ice - fDnfR((double)i, M.A_ice, M.B_ice, -M.negC_ice, L) + c->fice0;
    z = (double)i + P.ice;
  }
}

__global__ void single_ray_kernel(DevMedium M, PathPlan P, PathConsts* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  ray_consts(M, P, P.launch, out);
}

__global__ __launch_bounds__(kPathBlock) void path_kernel(DevMedium M, PathPlan P,
                                                           const PathConsts* __restrict__ c,
                                                           double* __restrict__ xs,
                                                           double* __restrict__ zs) {
  const long long k = (long long)blockIdx.x * kPathBlock + threadIdx.x;
  if (k >= P.first[P.nl] + P.n_ice) return;
  double x, z;
  path_sample(M, P, c, k, x, z);
  xs[k] = x;
  zs[k] = z;
}

// ---- the batch: n rays that share the ice height and the antenna depth ---------------------
// Workspace (d_work of airice_ray_paths_launch), in this order: n RayRecord (host-planned,
// uploaded by the launch), the tile list (uploaded too), n PathConsts (written by
// ray_consts_kernel).
struct RayRecord {
  PathPlan P;      // P.launch is unused: the launch angle is read from the device column
  long long base;  // offsets[i]: first sample of the ray in x / z
  long long pad_;
};
// One block of ray_paths_kernel: samples [tile * kPathBlock, (tile + 1) * kPathBlock) of ray
// `ray`, cut at the ray's end.  A ray of c samples has ceil(c / kPathBlock) tiles.
struct PathTile {
  int ray, tile;
};
static_assert(sizeof(RayRecord) % 16 == 0 && sizeof(PathConsts) % 8 == 0, "workspace alignment");

// One lane per ray: what single_ray_kernel does for its one ray, plus the summary columns.
__global__ __launch_bounds__(kConstsBlock) void ray_consts_kernel(
    DevMedium M, const RayRecord* __restrict__ recs, const double* __restrict__ launch, size_t n,
    PathConsts* __restrict__ consts, double* __restrict__ summary, size_t ld) {
  const size_t i = (size_t)blockIdx.x * kConstsBlock + threadIdx.x;
  if (i >= n) return;
  PathConsts* c = consts + i;
  ray_consts(M, recs[i].P, launch[i], c);
#pragma unroll
  for (int f = 0; f < AIRICE_SINGLE_RAY_FIELDS; ++f) summary[(size_t)f * ld + i] = c->summary[f];
}

// One lane per sample of the whole batch, one tile per block: the ray index is block-uniform, so
// its record and constants come through uniform loads and each wave stores 64 consecutive x / z.
__global__ __launch_bounds__(kPathBlock) void ray_paths_kernel(
    DevMedium M, const RayRecord* __restrict__ recs, const PathTile* __restrict__ tiles,
    const PathConsts* __restrict__ consts, double* __restrict__ xs, double* __restrict__ zs) {
  const PathTile t = tiles[blockIdx.x];
  const RayRecord& R = recs[t.ray];
  const long long k = (long long)t.tile * kPathBlock + threadIdx.x;
  if (k >= R.P.first[R.P.nl] + R.P.n_ice) return;
  double x, z;
  path_sample(M, R.P, consts + t.ray, k, x, z);
  xs[R.base + k] = x;
  zs[R.base + k] = z;
}

// Layer-skip scans (.C:60-86; RayTracingFunctions.cc:534-558)
int skip_above(const airice_medium* m, double txh) {
  int skip = 0;
  for (int il = m->max_layers; il > -1; il--) {
    // ATMLAY[il-1] is read only when the first test holds (txh < ATMLAY[0]/100 = 0 at il = 0)
    if (txh < m->atmlay_cm[il] / 100 && (il - 1 >= 0 ? txh >= m->atmlay_cm[il - 1] / 100 : false))
      il = -100;
    if (il > -1) skip++;
  }
  return skip;
}

int skip_below(const airice_medium* m, double ice) {
  int skip = 0;
  for (int il = 0; il < m->max_layers; il++) {
    if (ice >= m->atmlay_cm[il] / 100 && ice < m->atmlay_cm[il + 1] / 100) il = 100;
    if (il < m->max_layers) skip++;
  }
  return skip;
}

constexpr long long kMaxSamples = 1LL << 31;

int make_plan(const airice_medium* m, double depth, double launch, double txh, double ice,
              PathPlan* P, airice_single_ray_info* info) {
  std::memset(P, 0, sizeof(*P));
  P->txh = txh;
  P->ice = ice;
  P->depth = depth;
  P->launch = launch;
  const int sa = skip_above(m, txh), sb = skip_below(m, ice);
  P->top = m->max_layers - sa - 1;
  P->bot = sb;
  P->nl = m->max_layers - sa - sb;
  if (P->nl < 0) P->nl = 0;
  if (P->nl > kMaxLayers || P->top >= kMaxLayers) {
    set_error("single ray: %d path layers", P->nl);
    return AIRICE_EINVAL;
  }
  // sample ranges of the path loops (.C:226-299)
  long long n = 0;
  double last_height = 0;
  for (int il = 0; il < P->nl; ++il) {
    const double start = (il == 0) ? txh : last_height - 0.00001;
    const double stop = (il == P->nl - 1) ? ice : m->atmlay_cm[P->nl - il - 1] / 100;
    P->start[il] = start;
    P->stop[il] = stop;
    P->first[il] = n;
    // samples i = start, start-1, ... while i > stop-1, the last one clamped up to stop
    // (start - k is exact: every iterate is a multiple of ulp(start) no larger than start, so
    // the count is the number of k >= 0 with start - k > stop - 1, found with the loop's test)
    long long cnt = 0;
    if (start > stop - 1) {
      const double guess = std::floor(start - (stop - 1));
      if (!(guess < (double)kMaxSamples)) {
        set_error("single ray: path layer of %g samples", guess);
        return AIRICE_EINVAL;
      }
      cnt = (long long)guess;
      while (cnt > 0 && !(start - (double)(cnt - 1) > stop - 1)) --cnt;
      while (start - (double)cnt > stop - 1) ++cnt;
      last_height = (start - (double)(cnt - 1) < stop) ? stop : start - (double)(cnt - 1);
    }
    n += cnt;
  }
  for (int il = P->nl; il <= kMaxLayers; ++il) P->first[il] = n;
  // ice samples: for (int i = 0; i > -(depth+1); i--)
  const double lim = depth + 1;
  P->n_ice = (lim > 0) ? (long long)std::ceil(lim) : 0;
  if (!(P->n_ice < kMaxSamples) || !(n + P->n_ice < kMaxSamples)) {
    set_error("single ray: too many path samples");
    return AIRICE_EINVAL;
  }
  if (info != nullptr) {
    info->skip_above = sa;
    info->skip_below = sb;
    info->n_layers = P->nl;
    info->pad_ = 0;
    info->n_air = n;
    info->n_ice = P->n_ice;
  }
  return AIRICE_OK;
}

}  // namespace

int plan_single_ray(const airice_medium* m, double depth, double launch, double txh, double ice,
                    airice_single_ray_info* info) {
  PathPlan P;
  return make_plan(m, depth, launch, txh, ice, &P, info);
}

static_assert(sizeof(PathConsts) <= sizeof(double) * AIRICE_SINGLE_RAY_WORK,
              "AIRICE_SINGLE_RAY_WORK too small");

int launch_single_ray(const DevMedium& M, const airice_medium* m, double depth, double launch,
                      double txh, double ice, double* d_work, double* d_x, double* d_z,
                      size_t cap, hipStream_t st) {
  PathPlan P;
  int rc = make_plan(m, depth, launch, txh, ice, &P, nullptr);
  if (rc) return rc;
  const long long n = P.first[P.nl] + P.n_ice;
  if ((d_x != nullptr || d_z != nullptr) && (size_t)n > cap) {
    set_error("single ray: %lld path samples exceed capacity %zu", n, cap);
    return AIRICE_EINVAL;
  }
  PathConsts* c = reinterpret_cast<PathConsts*>(d_work);  // summary[] first
  rc = bracket_launch(LC_SINGLE_RAY, kNoTimer, st, [&] {
    hipLaunchKernelGGL(single_ray_kernel, dim3(1), dim3(64), 0, st, M, P, c);
  });
  if (rc || d_x == nullptr || d_z == nullptr || n <= 0) return rc;
  const unsigned grid = (unsigned)((n + kPathBlock - 1) / kPathBlock);
  return bracket_launch(LC_PATH, kNoTimer, st, [&] {
    hipLaunchKernelGGL(path_kernel, dim3(grid), dim3(kPathBlock), 0, st, M, P, c, d_x, d_z);
  });
}

namespace {

size_t round16(size_t b) { return (b + 15) / 16 * 16; }

// Workspace bytes of a batch of n rays with `tiles` tiles (layout: RayRecord above).
size_t batch_work_bytes(size_t n, long long tiles) {
  return n * sizeof(RayRecord) + round16((size_t)tiles * sizeof(PathTile)) +
         n * sizeof(PathConsts);
}

// The host plan of the batch: make_plan per ray (the sample count depends on txh, ice and depth
// only), the running sample offsets and the tile count.  recs / offsets are optional outputs.
int plan_batch(const airice_medium* m, double depth, double ice, const double* txh, size_t n,
               RayRecord* recs, int64_t* offsets, long long* tiles_out) {
  long long total = 0, tiles = 0;
  if (offsets != nullptr) offsets[0] = 0;
  for (size_t i = 0; i < n; ++i) {
    RayRecord local;
    RayRecord* R = recs != nullptr ? recs + i : &local;
    if (int rc = make_plan(m, depth, 0.0, txh[i], ice, &R->P, nullptr)) {
      const std::string why = airice_last_error();
      set_error("ray paths: ray %zu (Tx height %.17g m) rejected: %s", i, txh[i], why.c_str());
      return rc;
    }
    const long long cnt = R->P.first[R->P.nl] + R->P.n_ice;
    R->base = total;
    R->pad_ = 0;
    total += cnt;  // cnt < 2^31 (make_plan), n < 2^32: no overflow
    tiles += (cnt + kPathBlock - 1) / kPathBlock;
    if (offsets != nullptr) offsets[i + 1] = total;
  }
  if (tiles > 0x7fffffffLL) {
    set_error("ray paths: %lld sample tiles exceed one launch", tiles);
    return AIRICE_EINVAL;
  }
  *tiles_out = tiles;
  return AIRICE_OK;
}

}  // namespace

int plan_ray_paths(const airice_medium* m, double depth, double ice, const double* txh, size_t n,
                   int64_t* offsets, size_t* work_bytes) {
  if (n >= (1ull << 31)) {
    set_error("ray paths: %zu rays exceed one launch", n);
    return AIRICE_EINVAL;
  }
  long long tiles = 0;
  if (int rc = plan_batch(m, depth, ice, txh, n, nullptr, offsets, &tiles)) return rc;
  if (work_bytes != nullptr) *work_bytes = batch_work_bytes(n, tiles);
  return AIRICE_OK;
}

int launch_ray_paths(const DevMedium& M, const airice_medium* m, double depth, double ice,
                     const double* d_launch, const double* txh, size_t n, const int64_t* offsets,
                     void* d_work, size_t work_bytes, double* d_summary, size_t ld, double* d_x,
                     double* d_z, size_t cap, hipStream_t st) {
  if (n >= (1ull << 31)) {
    set_error("ray paths: %zu rays exceed one launch", n);
    return AIRICE_EINVAL;
  }
  const bool path = d_x != nullptr;
  // the staging image of the workspace's uploaded part: records, then tiles
  std::vector<RayRecord> recs(n);
  long long tiles = 0;
  std::vector<int64_t> planned(n + 1);
  if (int rc = plan_batch(m, depth, ice, txh, n, recs.data(), planned.data(), &tiles)) return rc;
  for (size_t i = 0; i <= n; ++i)
    if (offsets[i] != planned[i]) {
      set_error("ray paths: offsets[%zu] = %lld is not the plan of these rays (%lld)", i,
                (long long)offsets[i], (long long)planned[i]);
      return AIRICE_EINVAL;
    }
  const long long total = offsets[n];
  if (path && (unsigned long long)total > cap) {
    set_error("ray paths: %lld path samples exceed capacity %zu", total, cap);
    return AIRICE_EINVAL;
  }
  const size_t need = batch_work_bytes(n, tiles);
  if (work_bytes < need) {
    set_error("ray paths: workspace of %zu bytes, need %zu", work_bytes, need);
    return AIRICE_EINVAL;
  }
  const size_t rec_bytes = n * sizeof(RayRecord);
  const size_t tile_bytes = round16((size_t)tiles * sizeof(PathTile));
  char* w = static_cast<char*>(d_work);
  RayRecord* d_recs = reinterpret_cast<RayRecord*>(w);
  PathTile* d_tiles = reinterpret_cast<PathTile*>(w + rec_bytes);
  PathConsts* d_consts = reinterpret_cast<PathConsts*>(w + rec_bytes + tile_bytes);
  // (a copy from pageable memory returns once the source has been read)
  if (hipError_t e = hipMemcpyAsync(d_recs, recs.data(), rec_bytes, hipMemcpyHostToDevice, st)) {
    set_error("ray paths: record upload failed: %s", hipGetErrorString(e));
    return AIRICE_EHIP;
  }
  const bool sample = path && total > 0;
  if (sample) {
    std::vector<PathTile> tl;
    tl.reserve((size_t)tiles);
    for (size_t i = 0; i < n; ++i) {
      const long long cnt = offsets[i + 1] - offsets[i];
      for (long long t = 0; t * kPathBlock < cnt; ++t) tl.push_back(PathTile{(int)i, (int)t});
    }
    if (hipError_t e = hipMemcpyAsync(d_tiles, tl.data(), tl.size() * sizeof(PathTile),
                                      hipMemcpyHostToDevice, st)) {
      set_error("ray paths: tile upload failed: %s", hipGetErrorString(e));
      return AIRICE_EHIP;
    }
  }
  const unsigned cgrid = (unsigned)((n + kConstsBlock - 1) / kConstsBlock);
  const int rc = bracket_launch(LC_RAY_CONSTS, KT_RAY_CONSTS, st, [&] {
    hipLaunchKernelGGL(ray_consts_kernel, dim3(cgrid), dim3(kConstsBlock), 0, st, M, d_recs,
                       d_launch, n, d_consts, d_summary, ld);
  });
  if (rc || !sample) return rc;
  return bracket_launch(LC_RAY_PATHS, KT_RAY_PATHS, st, [&] {
    hipLaunchKernelGGL(ray_paths_kernel, dim3((unsigned)tiles), dim3(kPathBlock), 0, st, M, d_recs,
                       d_tiles, d_consts, d_x, d_z);
  });
}

}  // namespace airice
