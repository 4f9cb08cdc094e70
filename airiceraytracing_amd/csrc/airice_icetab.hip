// airice_icetab.hip -- the in-ice interpolation tables on gfx950 (IceRayTracing::MakeTable and
// GetInterpolatedValue, IceRayTracing.cc:2614-2905): three kernels and the entry points that launch
// them.  The rules -- layout, pack, interpolation -- are airice_icetab.hpp, the same text the host
// entries compile.
//
//   icetab_points_kernel  one grid position per lane, all antennas in one launch: the position's
//                         (zT, xT, zR) and (zT, xT, zR - 0.01) as the 2P rows iceray_kernel reads,
//                         and the image's header.  The descriptors travel as a kernel argument.
//   icetab_pack_kernel    one position per lane: 18 solution columns and the status byte in, one
//                         128-byte record out (eight 16-byte stores).
//   icetab_lookup_kernel  one query per lane: the antenna's descriptor (four 16-byte loads), the
//                         cell, the four corner records (seven 16-byte loads each, two parameters
//                         at a time), 13 column stores and the status byte.  No LDS, no atomics.
//
// A build is icetab_points_kernel, iceray_kernel over 2P rows, icesol_kernel over P, and
// icetab_pack_kernel: four launches whatever the number of antennas.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "airice.h"
#include "airice_hostcall.hpp"
#include "airice_icetab.hpp"
#include "airice_internal.h"

namespace airice {

namespace {

constexpr int kIceTabBlock = 256;
constexpr int kIceTabMaxBuild = AIRICE_ICETAB_MAX_BUILD;

// The antennas of one build: antenna a holds positions [begin[a], begin[a+1]) of the P.
struct BuildMap {
  int n_ant;
  long long begin[kIceTabMaxBuild + 1];
  double desc[kIceTabMaxBuild][icetab::kDesc];
};

__global__ __launch_bounds__(kIceTabBlock) void icetab_points_kernel(
    BuildMap map, double* __restrict__ image, size_t header, double* __restrict__ in, size_t P) {
  const size_t p = (size_t)blockIdx.x * kIceTabBlock + threadIdx.x;
  if (p < header) {
    const size_t a = p / icetab::kDesc, f = p % icetab::kDesc;
    image[p] = a < (size_t)map.n_ant ? map.desc[a][f] : 0.0;
  }
  if (p >= P) return;
  int a = 0;
  for (int j = 1; j < map.n_ant; ++j) a += (long long)p >= map.begin[j];
  const double* d = map.desc[a];
  const long long local = (long long)p - map.begin[a];
  const long long nz = (long long)d[icetab::kNz];
  const int ix = (int)(local / nz), iz = (int)(local - (long long)ix * nz);
  const double zT = icetab::grid_position(d[icetab::kZStart], d[icetab::kZStep], iz);
  const double xT = icetab::grid_position(d[icetab::kXStart], d[icetab::kXStep], ix);
  const double zR = d[icetab::kRxDepth];
  // GetRayTracingSolutions(zR, xT, zT, ...) (.cc:2662): z0 = zT, x1 = xT, z1 = zR; the second P
  // rows are GetFocusingFactor's receiver 1 cm lower (.cc:3257)
  in[p] = zT;
  in[P + p] = zT;
  in[2 * P + p] = xT;
  in[3 * P + p] = xT;
  in[4 * P + p] = zR;
  in[5 * P + p] = zR - 0.01;
}

__global__ __launch_bounds__(kIceTabBlock) void icetab_pack_kernel(
    const double* __restrict__ sol, const uint8_t* __restrict__ status, size_t P,
    double* __restrict__ records) {
  const size_t p = (size_t)blockIdx.x * kIceTabBlock + threadIdx.x;
  if (p >= P) return;
  double rec[icetab::kRecord];
  const double* s = sol + p;
  icetab::pack_record([s, P](int c) { return s[(size_t)c * P]; }, status[p],
                      [&rec](int c, double v) { rec[c] = v; });
  double2* dst = reinterpret_cast<double2*>(records + p * icetab::kRecord);
#pragma unroll
  for (int k = 0; k < icetab::kRecord / 2; ++k) dst[k] = make_double2(rec[2 * k], rec[2 * k + 1]);
}

__global__ __launch_bounds__(kIceTabBlock) void icetab_lookup_kernel(
    const double* __restrict__ image, size_t n_ant, const int32_t* __restrict__ ant,
    const double* __restrict__ x, const double* __restrict__ z, size_t n,
    double* __restrict__ out, size_t ld, uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * kIceTabBlock + threadIdx.x;
  if (i >= n) return;
  const long long a = ant != nullptr ? (long long)ant[i] : 0;
  const bool ant_ok = a >= 0 && (unsigned long long)a < n_ant;
  icetab::Cell cell;
  bool used = false;
  if (ant_ok) {
    const double2* dp = reinterpret_cast<const double2*>(image + (size_t)a * icetab::kDesc);
    double desc[icetab::kDesc];
#pragma unroll
    for (int k = 0; k < icetab::kDesc / 2; ++k) {
      const double2 v = dp[k];
      desc[2 * k] = v.x;
      desc[2 * k + 1] = v.y;
    }
    used = icetab::find_cell(desc, x[i], z[i], &cell);
  }
  double* o = out + i;
  if (!used) {
#pragma unroll
    for (int c = 0; c < icetab::kParams; ++c) o[(size_t)c * ld] = icetab::kMissing;
    if (status != nullptr) status[i] = ant_ok ? 0 : (uint8_t)icetab::kBadAntenna;
    return;
  }
  size_t off[4];
  icetab::corner_offsets(cell, off);
  const double2* r11 = reinterpret_cast<const double2*>(image + off[0]);
  const double2* r12 = reinterpret_cast<const double2*>(image + off[1]);
  const double2* r21 = reinterpret_cast<const double2*>(image + off[2]);
  const double2* r22 = reinterpret_cast<const double2*>(image + off[3]);
  bool idw = false;
#pragma unroll
  for (int k = 0; k < (icetab::kParams + 1) / 2; ++k) {
    const double2 f11 = r11[k], f12 = r12[k], f21 = r21[k], f22 = r22[k];
    o[(size_t)(2 * k) * ld] = icetab::interpolate(cell, f11.x, f12.x, f21.x, f22.x, &idw);
    if (2 * k + 1 < icetab::kParams)
      o[(size_t)(2 * k + 1) * ld] = icetab::interpolate(cell, f11.y, f12.y, f21.y, f22.y, &idw);
  }
  if (status != nullptr) status[i] = (uint8_t)(icetab::kCell | (idw ? icetab::kIdw : 0));
}

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
int misaligned_image(const char* who, const void* image) {
  if (!misaligned(image, AIRICE_ICETAB_ALIGN)) return AIRICE_OK;
  set_error("%s: image is not %d-byte aligned", who, AIRICE_ICETAB_ALIGN);
  return AIRICE_EINVAL;
}

// The checks a build shares with the sizing of its work buffer: the descriptors' grids and their
// first_record fields (as airice_icetab_layout leaves them); *positions = P.
int check_descs(const char* who, const double* descs, size_t n_ant, size_t* positions) {
  if (int rc = null_argument(who, {{"descs", descs}})) return rc;
  if (n_ant == 0 || n_ant > (size_t)kIceTabMaxBuild) {
    set_error("%s: n_ant = %zu is outside 1..%d", who, n_ant, kIceTabMaxBuild);
    return AIRICE_EINVAL;
  }
  size_t P = 0;
  const size_t first = icetab::header_doubles(n_ant) / icetab::kRecord;
  for (size_t a = 0; a < n_ant; ++a) {
    const double* d = descs + a * icetab::kDesc;
    if (const char* bad = icetab::bad_grid(d)) {
      set_error("%s: antenna %zu: %s", who, a, bad);
      return AIRICE_EINVAL;
    }
    if (d[icetab::kFirst] != (double)(first + P)) {
      set_error("%s: antenna %zu: first_record is not what airice_icetab_layout sets", who, a);
      return AIRICE_EINVAL;
    }
    P += (size_t)d[icetab::kNx] * (size_t)d[icetab::kNz];
    if (P >= ((size_t)1 << 30)) {
      set_error("%s: more than 2^30 positions", who);
      return AIRICE_EINVAL;
    }
  }
  *positions = P;
  return AIRICE_OK;
}

// What a build checks of its image and values, on either route; *positions = P.
int check_build(const void* image, const double* model, const double* descs, size_t n_ant,
                double a0, double frequency_ghz, size_t* positions) {
  if (int rc = check_descs("icetab build", descs, n_ant, positions)) return rc;
  if (int rc = misaligned_image("icetab build", image)) return rc;
  if (const char* bad = icesol_bad_value(model, a0, frequency_ghz)) {
    set_error("icetab build: %s", bad);
    return AIRICE_EINVAL;
  }
  return AIRICE_OK;
}

// in (6 P) | rays (32 x 2 P) | solutions (18 x P) | status (P bytes)
size_t work_bytes_for(size_t P) {
  return sizeof(double) * (6 + 2 * AIRICE_ICERAY_FIELDS + AIRICE_ICESOL_FIELDS) * P + P;
}

}  // namespace

}  // namespace airice

using namespace airice;

extern "C" {

int airice_icetab_work_bytes(const double* descs, size_t n_ant, size_t* bytes) {
  if (int rc = null_argument("icetab work", {{"bytes", bytes}})) return rc;
  size_t P = 0;
  if (int rc = check_descs("icetab work", descs, n_ant, &P)) return rc;
  *bytes = work_bytes_for(P);
  return AIRICE_OK;
}

int airice_icetab_build_launch(const double* model3, double* d_image, const double* descs,
                               size_t n_ant, double a0, double frequency_ghz, void* d_work,
                               size_t work_bytes, void* stream) {
  if (int rc = null_argument("icetab build", {{"image", d_image}, {"work", d_work}})) return rc;
  const double* model = ice_model_or_default(model3);
  size_t P = 0;
  if (int rc = check_build(d_image, model, descs, n_ant, a0, frequency_ghz, &P)) return rc;
  if (misaligned(d_work, 16)) {
    set_error("icetab build: work is not 16-byte aligned");
    return AIRICE_EINVAL;
  }
  if (work_bytes < work_bytes_for(P)) {
    set_error("icetab build: work_bytes (%zu) < %zu", work_bytes, work_bytes_for(P));
    return AIRICE_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  BuildMap map;
  std::memset(&map, 0, sizeof(map));
  map.n_ant = (int)n_ant;
  for (size_t a = 0; a < n_ant; ++a) {
    const double* d = descs + a * icetab::kDesc;
    std::memcpy(map.desc[a], d, sizeof(double) * icetab::kDesc);
    map.begin[a + 1] = map.begin[a] + (long long)d[icetab::kNx] * (long long)d[icetab::kNz];
  }
  const size_t header = icetab::header_doubles(n_ant);
  double* in = static_cast<double*>(d_work);
  double* rays = in + 6 * P;
  double* sol = rays + (size_t)AIRICE_ICERAY_FIELDS * 2 * P;
  uint8_t* status = reinterpret_cast<uint8_t*>(sol + (size_t)AIRICE_ICESOL_FIELDS * P);
  const size_t threads = P > header ? P : header;
  const unsigned blocks = (unsigned)((threads + kIceTabBlock - 1) / kIceTabBlock);
  int rc = bracket_launch(LC_ICETAB_POINTS, KT_ICETAB_POINTS, st, [&] {
    hipLaunchKernelGGL(icetab_points_kernel, dim3(blocks), dim3(kIceTabBlock), 0, st, map, d_image,
                       header, in, P);
  });
  if (rc) return rc;
  rc = airice_iceray_launch(model, in, in + 2 * P, in + 4 * P, 2 * P, rays, 2 * P, nullptr, st);
  if (rc) return rc;
  rc = airice_icesol_launch(model, in, in + 2 * P, in + 4 * P, rays, 2 * P, rays + P, 2 * P, P, a0,
                            frequency_ghz, sol, P, status, st);
  if (rc) return rc;
  return bracket_launch(LC_ICETAB_PACK, KT_ICETAB_PACK, st, [&] {
    hipLaunchKernelGGL(icetab_pack_kernel, dim3((unsigned)((P + kIceTabBlock - 1) / kIceTabBlock)),
                       dim3(kIceTabBlock), 0, st, sol, status, P, d_image + header);
  });
}

int airice_icetab_build_host(const double* model3, double* h_image, const double* descs,
                             size_t n_ant, double a0, double frequency_ghz) {
  if (int rc = null_argument("icetab build", {{"image", h_image}})) return rc;
  const double* model = ice_model_or_default(model3);
  size_t P = 0;
  if (int rc = check_build(h_image, model, descs, n_ant, a0, frequency_ghz, &P)) return rc;
  const size_t image_bytes = sizeof(double) * (icetab::header_doubles(n_ant) + icetab::kRecord * P);
  const size_t work = work_bytes_for(P);
  DevBuffer dimage, dwork;
  HIP_TRY(dimage.alloc(image_bytes));
  HIP_TRY(dwork.alloc(work));
  const int rc = airice_icetab_build_launch(model, static_cast<double*>(dimage.p), descs, n_ant, a0,
                                            frequency_ghz, dwork.p, work, nullptr);
  if (rc) return rc;
  // the copy-back is on the null stream, like the launches: it waits for the kernels
  HIP_TRY(hipMemcpy(h_image, dimage.p, image_bytes, hipMemcpyDeviceToHost));
  return AIRICE_OK;
}

int airice_icetab_lookup_launch(const double* d_image, size_t n_ant, const int32_t* d_ant,
                                const double* d_x, const double* d_z, size_t n, double* d_out,
                                size_t ld, uint8_t* d_status, void* stream) {
  if (n == 0) return AIRICE_OK;
  const char* who = "icetab lookup";
  if (int rc = null_argument(who, {{"image", d_image}, {"x", d_x}, {"z", d_z}, {"out", d_out}}))
    return rc;
  if (int rc = misaligned_image(who, d_image)) return rc;
  if (n_ant == 0) {
    set_error("icetab lookup: n_ant = 0");
    return AIRICE_EINVAL;
  }
  if (int rc = short_stride(who, "ld", ld, n)) return rc;
  if (int rc = exceeds_one_launch(who, n, kIceTabBlock)) return rc;
  hipStream_t st = (hipStream_t)stream;
  return bracket_launch(LC_ICETAB_LOOKUP, KT_ICETAB_LOOKUP, st, [&] {
    hipLaunchKernelGGL(icetab_lookup_kernel, dim3((unsigned)((n + kIceTabBlock - 1) / kIceTabBlock)),
                       dim3(kIceTabBlock), 0, st, d_image, n_ant, d_ant, d_x, d_z, n, d_out, ld,
                       d_status);
  });
}

}  // extern "C"
