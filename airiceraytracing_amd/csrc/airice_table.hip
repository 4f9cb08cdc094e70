// airice_table.hip -- the forward-ray kernels of libairice.so (gfx950), their per-grid caches
// and their stream-ordered launchers.
//
// Forward ray (GetRayTracingSolutions, MultiRayAirIceRefraction.cc:1796-2017; airice_ray.hpp):
//  table_kernel         : one lane per (TxHeight, launch angle) ray of MakeRayTracingTable
//                         (.cc:2079-2122), writes the 11 float table columns (.cc:2101-2111) and,
//                         optionally, the 18 doubles of dummy[] for parity checks.
//  table_multi_kernel   : the same block body for several antennas' tables in one grid.
//  rowconst_kernel, angle_sines_kernel : fill the per-grid caches of the table launch.
//  air_part_kernel      : the air part (ray_air_part) of every ray of a table launch, written to
//                         the launch's air record; later builds of that launch, for any antenna
//                         depth, run table_kernel's warm instantiation: record in, ice part
//                         (ray_ice_part) only.
//  rays_kernel          : the same ray for arbitrary (angle, height) lists.
//  scalar_ray_kernel    : one ray (n = 1) spread over a wave.
//  table_firn_kernel, table_multi_firn_kernel, rays_firn_kernel : the table (cold and warm), the
//                         multi-antenna table and the rays in a two-layer firn (ray_ice_part_firn).
// Launchers: launch_table, launch_table_multi, launch_rays; rays_host is the one-query host route.
// The caches (row_cache, angle_cache, air_cache: GridCache; the multi-antenna launch's constant
// sets: ConstSetCache) have their policy in airice_gridcache.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "airice.h"
#include "airice_device.hpp"
#include "airice_internal.h"
#include "airice_ray.hpp"
#include "airice_gridcache.hpp"

namespace airice {

// Table launch shape: 256-thread blocks at 8 waves/SIMD (64 VGPRs), measured best of 64 / 128 /
// 256 / 512 threads, 7 / 8 waves and 1 / 2 rays per lane.
#ifndef AIRICE_TABLE_BLOCK
#define AIRICE_TABLE_BLOCK 256
#endif
constexpr int kTableBlock = AIRICE_TABLE_BLOCK;  // (A/B builds: -DAIRICE_TABLE_BLOCK=...)
constexpr int kTableWaves = 8;
// table stores take an SGPR column base and a 32-bit lane byte offset (global_store saddr form):
// launches are split at 2^30 rays so that 4 k < 2^32
constexpr long long kMaxLaunchRays = 1LL << 30;
// table launches of fewer rays store their columns at agent scope (table_ray's SC1)
constexpr long long kAgentStoreRays = 1LL << 24;
// (the warm table launch, whose air part comes from the air record, keeps that rule: cfg2 13.2 us
// at agent scope against 16.1-16.3 us with plain stores)

struct TableArgs {
  double start_h, stop_h, step_h;
  double start_a, stop_a, step_a;
  double inv_asteps;  // 1.0 / asteps (row of ray k without an integer division)
  int hsteps, asteps;
  int row0, in_ice;
  int n;              // rays of this launch (< 2^31; launch_table splits larger grids)
  int rows_per_block; // LDS rows a block's set of rays may span
  int half;           // rays per set (R = 2: ceil(n / 2); R = 1: n)
  size_t ld;
  const struct RowConst* rc;  // the grid's row constants (all hsteps rows, computed once per
                              // medium and grid: row_consts_cached), or nullptr
  const double* vs;           // sin of the start angle of every column (angle_sines_cached), or
                              // nullptr
  unsigned char* air;         // the launch's air record (air_part_cached): written by
                              // air_part_kernel, read by the warm table_kernel; else nullptr
};

// The air record of a launch of n rays: 32 B per ray in two planes of 16-byte entries, so that a
// lane moves its ray with two 16-byte accesses (global_load / global_store_dwordx4), each of them
// contiguous over the wave.  Plane d, double2[n]: {vinc, thd_air} (table column 1 is
// (float)(thd_air + thd_ice), so thd_air keeps its 53 bits).  Plane f, float4[n], 16 n bytes behind
// it (16-byte aligned for every n): table columns {3, 8, 6, 7} -- (float)(t_air c), (float)geo_air
// and the Fresnel coefficients, which read vinc and the ice height's indices only -- as the floats
// the table stores.  Keeping the two Fresnel floats costs 8 B per ray of traffic and saves their
// ~40 FP64 operations, two square roots and two quotients: cfg2 12.0 against 13.2 us.
// Both planes are addressed as a wave-uniform base plus the lane's 32-bit byte offset 16 k (the
// global_load / global_store saddr form, as table_columns): a record therefore stays below 2^32
// bytes -- air_part_cached refuses a larger one (the launch then runs the cold kernel), whatever
// airice_air_cache_limits allows; there is no 64-bit path.
__host__ __device__ __forceinline__ size_t air_record_bytes(size_t n) { return 32 * n; }
constexpr size_t kAirRecordMaxBytes = (size_t)1 << 32;  // exclusive
struct AirRecord {
  double2* d;  // this ray's {vinc, thd_air}
  float4* f;   // this ray's {col3, col8, col6, col7}
};
__device__ __forceinline__ AirRecord air_record(unsigned char* base, size_t n, int k) {
  const uint32_t off = (uint32_t)k * 16u;
  return AirRecord{reinterpret_cast<double2*>(base + off),
                   reinterpret_cast<float4*>(base + 16 * n + off)};
}

// Debug timeline (AIRICE_TABLE_TRACE=<file>, tools/wave_timeline.py): per wave, the 100 MHz
// s_memrealtime at entry and exit plus HW_ID / XCC_ID.  Not part of the API.
struct WaveTrace {
  unsigned long long t0, t1;
  unsigned long long c0, c1;  // s_memtime (shader clock) at entry and exit: the in-kernel clock
  unsigned hw_id, xcc_id;
};

// Tx height of grid row ihei (.cc:2080, 2089-2091; separate mul and add, no contraction).
__device__ __forceinline__ double row_height(const TableArgs& G, int ihei) {
  double H = G.start_h - G.step_h * ihei;
  if (H != G.stop_h && ihei == G.hsteps - 1) H = G.stop_h;
  return H;
}

// Row (within the launch) of ray k: the double quotient k / asteps is within 1 of the integer
// one for k < 2^31, then fixed up.
__device__ __forceinline__ int ray_row(const TableArgs& G, int k) {
  int r = (int)((double)k * G.inv_asteps);
  if (r * G.asteps > k) --r;
  if ((r + 1) * G.asteps <= k) ++r;
  return r;
}

// One table entry: ray k of the launch (row r, row-major over TxH rows x launch angles).
// Launch angle of column iang of the grid (.cc:2085, 2092-2094).
__device__ __forceinline__ double table_angle(const TableArgs& G, int iang) {
  double th = G.start_a + G.step_a * iang;
  if (iang == G.asteps - 1) th = G.stop_a;
  return th;
}

// The 11 AllTableAllAntData columns of ray k (.cc:2101-2111): the column base is wave-uniform, the
// lane's byte offset fits 32 bits (k < 2^30 per launch).
// (non-temporal stores: cfg2 28.9 -> 29.9 us, same bits)
// SC1: the column stores at agent scope (global_store ... sc1), for launches short enough that
// the lines they leave dirty in the XCDs' L2s are a visible part of the launch: cfg2 28.9-29.2
// -> 27.8-28.2 us, the same table (without any table store the kernel takes 25.6 us); at cfg4
// size plain stores are faster (20.8 against 21.9 ms per build)
// COLS: the columns this call stores (bit c: column c); the other arguments are ignored.
constexpr unsigned kAllColumns = 0x7FFu;
template <bool SC1, unsigned COLS = kAllColumns>
__device__ __forceinline__ void table_columns(float* __restrict__ table, size_t ld, int k, float c0,
                                              float c1, float c2, float c3, float c4, float c5,
                                              float c6, float c7, float c8, float c9, float c10) {
  char* tb = reinterpret_cast<char*>(table);
  const size_t ldb = ld * sizeof(float);
  const uint32_t off = (uint32_t)k * 4u;
  auto st = [&](int c, float v) {
    if (!((COLS >> c) & 1u)) return;
    float* p = reinterpret_cast<float*>(tb + c * ldb + off);
    if constexpr (SC1)
      st_agent(p, v);
    else
      *p = v;
  };
  st(0, c0);
  st(1, c1);
  st(2, c2);
  st(3, c3);
  st(4, c4);
  st(5, c5);
  st(6, c6);
  st(7, c7);
  st(8, c8);
  st(9, c9);
  st(10, c10);
}

template <bool A1, bool SC1>
__device__ __forceinline__ void table_ray(const DevMedium& M, const IceConsts& I,
                                          const TableArgs& G, const RowConst& rc, int r, int k,
                                          float* __restrict__ table, double* __restrict__ full,
                                          const double* tab, int top_hi,
                                          const FirnLeg* F = nullptr) {
  const int iang = k - r * G.asteps;
  const double th = table_angle(G, iang);
  double d[18];
  // the start-angle sine of every grid column, formed once per angle grid (angle_sines_kernel);
  // launches captured into a graph before their grid was cached form it here
  double vs;
  if (G.vs != nullptr)
    vs = G.vs[iang];
  else
    vs = sin_start((180 - th) * M.d2r);
  ray_solution_row<A1>(M, I, rc, th, G.in_ice != 0, d, full != nullptr, tab, top_hi, &vs, F);
  const size_t ld = G.ld;
  table_columns<SC1>(table, ld, k, (float)d[1], (float)d[2], (float)d[7], (float)d[6],
                     (float)d[11], (float)d[3], (float)d[14], (float)d[15], (float)d[16],
                     (float)d[17], (float)d[13]);
  if (full != nullptr) {
#pragma unroll
    for (int c = 0; c < 18; ++c) full[c * ld + k] = d[c];
  }
}

// The air part of table ray k alone, written to the launch's air record (air_part_kernel): the
// expressions of table_ray and ray_solution_row up to the ice surface, then the two float columns
// as the table stores them.
template <bool A1>
__device__ __forceinline__ void table_ray_air(const DevMedium& M, const IceConsts& I,
                                              const TableArgs& G, const RowConst& rc, int r, int k,
                                              const double* tab, int top_hi) {
  const int iang = k - r * G.asteps;
  double vs;
  if (G.vs != nullptr)
    vs = G.vs[iang];
  else
    vs = sin_start((180 - table_angle(G, iang)) * M.d2r);
  const AirPart a = ray_air_part<A1>(M, I, rc, vs, tab, top_hi);
  double tS, tP;
  fresnel_from_sine(I.n_air_ice, I.n_ice0, I.n_ratio, a.vinc, tS, tP);
  const AirRecord R = air_record(G.air, (size_t)G.n, k);
  *R.d = double2{a.vinc, a.thd_air};
  *R.f = float4{(float)(a.t_air * kSpeedC), (float)a.geo_air, (float)tS, (float)tP};
}

// Table ray k from its air record (the warm table_kernel).  rd, rf: the ray's two record entries,
// loaded by the caller ahead of the block's barrier; H, th: the row's Tx height (RowConst::H) and
// the column's launch angle.
// Seven of the eleven columns need nothing from the ice segment -- 0 = H, 4 = th, 5 = thd_air and
// the record's own floats 3, 8, 6, 7 (t_air, geo_air and the Fresnel coefficients enter no other
// column) -- so they are stored as soon as the record is there, and travel to memory while the
// wave traces the ice segment; columns 1, 2, 9 and 10 follow it.  The values and their
// conversions are those of one table_columns call behind ray_ice_part (d[1] = H, d[11] = th,
// d[3] = thd_air).  The scheduling barrier keeps the early stores ahead of the segment's
// arithmetic.  log_ratio2's special-value branch (log_ratio_ieee: an exec-masked global load of
// the log table and a vmcnt(0)) then also waits for the wave's early stores; only rays with NaN or
// zero radicands take it, none of them in a grid like cfg2.
constexpr unsigned kWarmEarlyColumns = 0x1F9u;                          // 0, 3, 4, 5, 6, 7, 8
constexpr unsigned kWarmLateColumns = kAllColumns & ~kWarmEarlyColumns;  // 1, 2, 9, 10
template <bool SC1, bool FIRN = false>
__device__ __forceinline__ void table_ray_warm(const DevMedium& M, const IceConsts& I,
                                               const TableArgs& G, int k, double H, double th,
                                               const double2 rd, const float4 rf,
                                               float* __restrict__ table, const double* tab,
                                               const FirnLeg* F = nullptr) {
  const double vinc = rd.x, thd_air = rd.y;
  table_columns<SC1, kWarmEarlyColumns>(table, G.ld, k, (float)H, 0.f, 0.f, rf.x, (float)th,
                                        (float)thd_air, rf.z, rf.w, rf.y, 0.f, 0.f);
  __builtin_amdgcn_sched_barrier(0);
  double d[18];
  if constexpr (FIRN)
    ray_ice_part_firn<false>(M, I, *F, H, th, G.in_ice != 0, vinc, thd_air, 0.0, 0.0, 0.0, d, tab);
  else
    ray_ice_part<false>(M, I, H, th, G.in_ice != 0, vinc, thd_air, 0.0, 0.0, 0.0, d, tab);
  table_columns<SC1, kWarmLateColumns>(table, G.ld, k, 0.f, (float)d[2], (float)d[7], 0.f, 0.f,
                                       0.f, 0.f, 0.f, 0.f, (float)d[17], (float)d[13]);
}

// Table launch: one ray per lane, ray k = block * 256 + threadIdx.x (each wave's column store one
// contiguous 256 B segment).  The block first stages the Tx-height-only constants of the (few) rows
// it spans into LDS -- copied from the grid's row-constant cache, or, when the launch has none, one
// lane per row computes them, so the exp / layer scans / top-layer folding run once per row
// instead of once per wave -- then every lane traces its ray.
// (Measured and rejected, DESIGN.md §5: persistent grid-stride and atomic-chunk schedules -- the
// loop around the inlined ray body raises register pressure to 160 VGPRs, or 330 B/lane of scratch
// when capped at 64, and runs 2.7x / 7x slower -- and two rays per lane.)
// The work of one table block (kTableBlock rays of one antenna's grid), shared by the single- and
// the multi-antenna kernels.
// MODE: kTableFull traces whole rays; kTableAir traces the air part only and writes the launch's
// air record (no table); kTableWarm reads the air record and traces the ice part only -- it needs
// neither the rows' constants (the Tx height comes from row_height) nor the start sines.
// FIRN, F: the lower leg of a layered firn (the *_firn kernels); else F is nullptr and every use of
// it folds away.
enum { kTableFull = 0, kTableAir = 1, kTableWarm = 2 };
template <bool TRACE, bool A1, bool SC1, int MODE = kTableFull, bool FIRN = false>
__device__ __forceinline__ void table_block(const DevMedium& M, const IceConsts& I,
                                            const TableArgs& G, float* __restrict__ table,
                                            double* __restrict__ full,
                                            WaveTrace* __restrict__ trace, unsigned block,
                                            const FirnLeg* F = nullptr) {
  constexpr int BS = kTableBlock;
  extern __shared__ __align__(16) unsigned char smem[];
  RowConst* rows = reinterpret_cast<RowConst*>(smem);
  // the log table (16 B x 2^kLogTableBits) staged in LDS: 16-byte entries, (1 << kLogTableBits) / BS per thread
  __shared__ __align__(16) double s_logtab[1 << kLogTableBits][2];
  if constexpr (MODE == kTableWarm) {
    // One round trip to memory ahead of the arithmetic: the thread's log-table entries and,
    // behind them, its ray's two record entries are all in flight before the first wait; the
    // ray's row, height and angle (kernel-argument fields only) are formed under them.  The LDS
    // write then waits for the log-table entries alone (they were issued first), the record is
    // awaited after the barrier.
    // (The log table stays in LDS.  Read from global memory instead -- no staging, no barrier --
    // the two lookups of a ray are vector loads behind its early stores and wait for them: on a
    // par with this form at 256 and at 64 threads, behind it at 128; without the early stores it
    // was the faster of the two.  DESIGN.md §5.)
    constexpr int NT = ((1 << kLogTableBits) + BS - 1) / BS;
    const int k = (int)block * BS + (int)threadIdx.x;
    const bool live = k < G.n;
    constexpr bool whole = (1 << kLogTableBits) % BS == 0;  // every thread stages NT entries
    double2 e[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const unsigned t = threadIdx.x + j * BS;
      if (whole || t < (1u << kLogTableBits))
        e[j] = *reinterpret_cast<const double2*>(&kLogTable[t][0]);
    }
    __builtin_amdgcn_sched_barrier(0);
    // unconditional loads (a lane past the end re-reads the last ray's entries; n >= 1): no
    // exec-masked block, so the wait ahead of the LDS write can count past them
    const AirRecord R = air_record(G.air, (size_t)G.n, min(k, G.n - 1));
    const double2 rd = *R.d;
    const float4 rf = *R.f;
    const int r = ray_row(G, k);
    const double th = table_angle(G, k - r * G.asteps);
    const double H = row_height(G, G.row0 + r);
    // formed here, ahead of the barrier, and with them the kernel-argument fields the ice segment
    // reads (one scalar round trip under the vector loads instead of one behind the barrier)
    formed_here_v(th, H);
    formed_here_s(I.iceseg, I.n_ratio, M.A_ice, M.r2d, G.ld, table);
    if constexpr (FIRN) formed_here_s(*F);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const unsigned t = threadIdx.x + j * BS;
      if (whole || t < (1u << kLogTableBits)) *reinterpret_cast<double2*>(&s_logtab[t][0]) = e[j];
    }
    __syncthreads();
    if (live) table_ray_warm<SC1, FIRN>(M, I, G, k, H, th, rd, rf, table, &s_logtab[0][0], F);
    return;
  }
#pragma unroll
  for (unsigned t = threadIdx.x; t < (1u << kLogTableBits); t += BS) {
    s_logtab[t][0] = kLogTable[t][0];
    s_logtab[t][1] = kLogTable[t][1];
  }
  const unsigned wave = block * (BS / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (TRACE && lane == 0) {
    trace[wave].t0 = __builtin_amdgcn_s_memrealtime();
    trace[wave].c0 = __builtin_amdgcn_s_memtime();
  }
  const int k0 = (int)block * BS;
  const int ke = min(k0 + BS, G.n);  // end of this block's rays
  const int r0 = k0 < ke ? ray_row(G, k0) : 0;
  {
    const int nrows = k0 < ke ? ray_row(G, ke - 1) - r0 + 1 : 0;
    for (int t = threadIdx.x; t < nrows; t += BS)
      rows[t] = G.rc != nullptr ? G.rc[G.row0 + r0 + t]
                                : row_const(M, I, row_height(G, G.row0 + r0 + t));
  }
  __syncthreads();
  const int k = k0 + (int)threadIdx.x;
  if constexpr (MODE == kTableAir) {
    if (k0 < G.n) {
      const int top_hi = __builtin_amdgcn_readfirstlane(rows[0].top);
      __builtin_assume(top_hi >= 0);
      if (k < G.n) {
        const int r = ray_row(G, k);
        table_ray_air<A1>(M, I, G, rows[r - r0], r, k, &s_logtab[0][0], top_hi);
      }
    }
    return;
  }
  if (k0 < G.n) {  // block-uniform
    // the block's first row has the highest Tx, so its Tx layer bounds every lane's (top_layer is
    // monotone in the height)
    const int top_hi = __builtin_amdgcn_readfirstlane(rows[0].top);
    __builtin_assume(top_hi >= 0);
    if (k < G.n) {
      const int r = ray_row(G, k);
      table_ray<A1, SC1>(M, I, G, rows[r - r0], r, k, table, full, &s_logtab[0][0], top_hi, F);
    }
  }
  if (TRACE && lane == 0) {
    trace[wave].t1 = __builtin_amdgcn_s_memrealtime();
    trace[wave].c1 = __builtin_amdgcn_s_memtime();
    trace[wave].hw_id = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));  // HW_ID
    trace[wave].xcc_id = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11));
  }
}

// waves_per_eu(8): 64 VGPRs at 8 waves/SIMD, measured on par or slightly ahead of 67 VGPRs at 7.
// WARM: the launch has its air record (G.air, air_part_cached): the ice part only.
template <bool TRACE, bool A1, bool SC1, bool WARM = false>
__global__ __launch_bounds__(kTableBlock) __attribute__((amdgpu_waves_per_eu(kTableWaves, kTableWaves))) void table_kernel(
                                                   DevMedium M, IceConsts I, TableArgs G,
                                                   float* __restrict__ table,
                                                   double* __restrict__ full,
                                                   WaveTrace* __restrict__ trace) {
  table_block<TRACE, A1, SC1, WARM ? kTableWarm : kTableFull>(M, I, G, table, full, trace,
                                                              blockIdx.x);
}

// Fills a launch's air record (air_part_cached): the table block's prologue and the air part of
// every ray, one ray per lane, no table store.
template <bool A1>
__global__ __launch_bounds__(kTableBlock) __attribute__((amdgpu_waves_per_eu(kTableWaves, kTableWaves))) void air_part_kernel(
    DevMedium M, IceConsts I, TableArgs G) {
  table_block<false, A1, false, kTableAir>(M, I, G, nullptr, nullptr, nullptr, blockIdx.x);
}

// Several antennas' tables in one grid (airice_table_launch_multi): the blocks of antenna a are
// [begin[a], begin[a+1]); its per-antenna constants (IceConsts, TableArgs: antenna depth, stop
// height) come from global memory, read with scalar loads since the index is block-uniform.
// One launch ramp and one drain for all antennas instead of one per table.
constexpr int kMaxAntennas = 32;
struct MultiMap {
  int n_ant;
  int begin[kMaxAntennas + 1];
  float* table[kMaxAntennas];
};

template <bool A1, bool SC1>
__global__ __launch_bounds__(kTableBlock) __attribute__((amdgpu_waves_per_eu(kTableWaves, kTableWaves))) void table_multi_kernel(
    DevMedium M, const IceConsts* __restrict__ Iv, const TableArgs* __restrict__ Gv, MultiMap map) {
  int a = 0;
  for (int j = 1; j < map.n_ant; ++j) a += (int)blockIdx.x >= map.begin[j];
  a = __builtin_amdgcn_readfirstlane(a);
  table_block<false, A1, SC1>(M, Iv[a], Gv[a], map.table[a], nullptr, nullptr,
                         blockIdx.x - (unsigned)map.begin[a]);
}

// The table kernels in a two-layer firn: the same block bodies with the lower leg's
// constants F beside IceConsts (per antenna in the multi-antenna launch; F.below is block-uniform,
// so one launch mixes antennas above and below the boundary).  The air part kernel is shared: it
// reads nothing of the ice below the surface.
template <bool A1, bool SC1, bool WARM = false>
__global__ __launch_bounds__(kTableBlock) __attribute__((amdgpu_waves_per_eu(kTableWaves, kTableWaves))) void table_firn_kernel(
    DevMedium M, IceConsts I, FirnLeg F, TableArgs G, float* __restrict__ table,
    double* __restrict__ full) {
  table_block<false, A1, SC1, WARM ? kTableWarm : kTableFull, true>(M, I, G, table, full, nullptr,
                                                                    blockIdx.x, &F);
}

template <bool A1, bool SC1>
__global__ __launch_bounds__(kTableBlock) __attribute__((amdgpu_waves_per_eu(kTableWaves, kTableWaves))) void table_multi_firn_kernel(
    DevMedium M, const IceConsts* __restrict__ Iv, const FirnLeg* __restrict__ Fv,
    const TableArgs* __restrict__ Gv, MultiMap map) {
  int a = 0;
  for (int j = 1; j < map.n_ant; ++j) a += (int)blockIdx.x >= map.begin[j];
  a = __builtin_amdgcn_readfirstlane(a);
  table_block<false, A1, SC1, kTableFull, true>(M, Iv[a], Gv[a], map.table[a], nullptr, nullptr,
                                                blockIdx.x - (unsigned)map.begin[a], &Fv[a]);
}

// Row constants of a whole grid (row_consts_cached): one row per lane, the table block's own
// row_const on the same heights, so the cached values are the bits the block would compute.
__global__ __launch_bounds__(256) void rowconst_kernel(DevMedium M, IceConsts I, TableArgs G,
                                                       RowConst* __restrict__ out) {
  const int r = (int)(blockIdx.x * 256 + threadIdx.x);
  if (r < G.hsteps) out[r] = row_const(M, I, row_height(G, r));
}

// Start-angle sines of a grid's columns (angle_sines_cached): the table ray's own expression.
__global__ __launch_bounds__(256) void angle_sines_kernel(DevMedium M, TableArgs G,
                                                          double* __restrict__ out) {
  const int a = (int)(blockIdx.x * 256 + threadIdx.x);
  if (a < G.asteps) out[a] = sin_start((180 - table_angle(G, a)) * M.d2r);
}

// One forward ray spread over a wave (the one-query GetRayTracingSolutions call): the running
// sine chain is cheap, so every lane walks it and knows the input sine of each segment; lane 0
// then traces the Tx-layer segment, lanes 1-3 the lower layers (top-1, top-2, top-3 while >= bot),
// lane 4 the segment in the ice, all at once, while the angle outputs and the Fresnel
// coefficients (functions of the chain's sines only) run beside them on every lane; the sums are
// formed in ray_solution_row's order from the lanes' values.  The same operations on the same
// values as ray_solution (hence the same bits), with the ~1,000-deep one-lane chain cut to about
// one segment.
__device__ __forceinline__ void ray_solution_wave(const DevMedium& M, const IceConsts& I,
                                                  double theta, double H, bool in_ice, double* d,
                                                  const double* tab) {
  const int lane = (int)(threadIdx.x & 63);
  const RowConst rc = row_const(M, I, H);
  const int top = rc.top, bot = I.bot;
  const bool any = rc.any != 0;
  const double A2 = M.A_air * M.A_air, A2i = M.A_ice * M.A_ice;
  // the chain: input sine of every segment, and the sine after the air layers
  double v = sin_start((180 - theta) * M.d2r);
  double sin_in[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  bool on[5] = {false, false, false, false, false};
  if (any) {
    sin_in[0] = sin_asin(v);
    on[0] = true;
    v = sin_asin(rc.seg.ratio * sin_in[0]);
  }
#pragma unroll
  for (int j = 1; j <= 3; ++j) {
    const int il = top - j;
    if (il >= bot && il >= 0) {
      sin_in[j] = v;
      on[j] = true;
      v = sin_asin(sel_lower_ratio(I, il) * v);
    }
  }
  const double vinc = any ? v : 0.0;
  const double u_ice = sin_asin(I.n_ratio * vinc);
  sin_in[4] = u_ice;
  on[4] = in_ice;
  // this lane's segment
  const int j = lane < 5 ? lane : 0;
  SegConst S = rc.seg;
  double sj = sin_in[0];
#pragma unroll
  for (int q = 1; q <= 4; ++q) {
    const bool me = j == q;
    sj = me ? sin_in[q] : sj;
  }
  const int il = top - j;
#pragma unroll
  for (int l = 0; l < kMaxLayers; ++l) {
    const bool me = j >= 1 && j <= 3 && il == l;
    const SegConst& c = I.lower[l];
    S = SegConst{me ? c.Tn : S.Tn,       me ? c.Ty2 : S.Ty2,     me ? c.TAy : S.TAy,
                 me ? c.Rn : S.Rn,       me ? c.Ry2 : S.Ry2,     me ? c.RAy : S.RAy,
                 me ? c.ratio : S.ratio, me ? c.invC : S.invC,   me ? c.invCc : S.invCc,
                 me ? c.dCx : S.dCx,     me ? c.dACx : S.dACx};
  }
  {
    const bool me = j == 4;
    const SegConst& c = I.iceseg;
    S = SegConst{me ? c.Tn : S.Tn,       me ? c.Ty2 : S.Ty2,     me ? c.TAy : S.TAy,
                 me ? c.Rn : S.Rn,       me ? c.Ry2 : S.Ry2,     me ? c.RAy : S.RAy,
                 me ? c.ratio : S.ratio, me ? c.invC : S.invC,   me ? c.invCc : S.invCc,
                 me ? c.dCx : S.dCx,     me ? c.dACx : S.dACx};
  }
  const bool air = j != 4;
  double v_unused;
  const Segment sg = segment_const(S, air ? M.A_air : M.A_ice, air ? A2 : A2i, sj, air, v_unused,
                                   tab);
  // outputs that are functions of the chain's sines (every lane; lane 0 writes)
  const double inc = any ? k_asin(vinc) * M.r2d : 0.0;
  const double recv_ice = k_asin(sin_asin(I.iceseg.ratio * u_ice)) * M.r2d;
  double tS, tP;
  fresnel_from_sine(I.n_air_ice, I.n_ice0, I.n_ratio, vinc, tS, tP);
  double thd_air = 0.0, t_air = 0.0, geo_air = 0.0;
#pragma unroll
  for (int q = 0; q <= 3; ++q) {
    const double a = __shfl(sg.thd, q), b = __shfl(sg.t, q), c = __shfl(sg.geo, q);
    if (on[q]) {
      thd_air += a;
      t_air += b;
      geo_air += c;
    }
  }
  double thd_ice = 0.0, t_ice = 0.0, geo_ice = 0.0;
  {
    const double a = __shfl(sg.thd, 4), b = __shfl(sg.t, 4), c = __shfl(sg.geo, 4);
    if (on[4]) {
      thd_ice += a;
      t_ice += b;
      geo_ice += c;
    }
  }
  if (lane != 0) return;
  d[0] = 0;
  d[1] = H;
  d[2] = thd_air + thd_ice;
  d[3] = thd_air;
  d[4] = thd_ice;
  d[5] = (t_ice + t_air) * kSpeedC;
  d[6] = t_air * kSpeedC;
  d[7] = t_ice * kSpeedC;
  d[8] = (t_ice + t_air) * 1e9;
  d[9] = t_air * 1e9;
  d[10] = t_ice * 1e9;
  d[11] = theta;
  d[12] = inc;
  d[13] = in_ice ? recv_ice : 0.0;
  d[14] = tS;
  d[15] = tP;
  d[16] = geo_air;
  d[17] = geo_ice;
}

// One-ray launch (n = 1): one wave, ray_solution_wave, lane 0 writes dummy[0..17].
__global__ __launch_bounds__(64) void scalar_ray_kernel(DevMedium M, IceConsts I,
                                                        const double* __restrict__ launch,
                                                        const double* __restrict__ txh, int in_ice,
                                                        double* __restrict__ out, size_t ld,
                                                        Signal sig) {
  prefetch_kernargs<sizeof(DevMedium) + sizeof(IceConsts)>();
  const bool inl = sig.n_in >= 2;  // the inputs in the kernel arguments
  double d[18];
  ray_solution_wave(M, I, inl ? sig.in[0] : launch[0], inl ? sig.in[1] : txh[0], in_ice != 0, d,
                    &kLogTable[0][0]);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int c = 0; c < 18; ++c) out[c * ld] = d[c];
  signal_done(sig);
}

__global__ __launch_bounds__(kBlock) void rays_kernel(DevMedium M, IceConsts I,
                                                      const double* __restrict__ launch,
                                                      const double* __restrict__ txh, int in_ice,
                                                      long long n, double* __restrict__ out,
                                                      size_t ld, Signal sig) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  double d[18];
  const bool inl = sig.n_in >= 2;  // one-ray call: its inputs in the kernel arguments
  ray_solution(M, I, inl ? sig.in[0] : launch[k], inl ? sig.in[1] : txh[k], in_ice != 0, d);
#pragma unroll
  for (int c = 0; c < 18; ++c) out[c * ld + k] = d[c];
  if (k == 0) signal_done(sig);  // armed for one-ray calls only
}

// rays_kernel in a two-layer firn; also the one-ray launch (on one lane).
__global__ __launch_bounds__(kBlock) void rays_firn_kernel(DevMedium M, IceConsts I, FirnLeg F,
                                                           const double* __restrict__ launch,
                                                           const double* __restrict__ txh,
                                                           int in_ice, long long n,
                                                           double* __restrict__ out, size_t ld) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  double d[18];
  ray_solution(M, I, launch[k], txh[k], in_ice != 0, d, true, &F);
#pragma unroll
  for (int c = 0; c < 18; ++c) out[c * ld + k] = d[c];
}

static_assert(kMaxAntennas < (int)kCacheSets, "a multi-antenna launch never evicts its own entries");

static GridCache& row_cache() {
  static GridCache c;
  return c;
}
static GridCache& angle_cache() {
  static GridCache c;
  return c;
}

// The row constants of a grid.  row_const reads the medium, the heights and, of the ice constants,
// only the lowest air layer (bot) and the Tx-layer stop ends (topend): the key holds exactly those,
// so tables of one grid for antennas at different depths in the ice share one entry.
// Rays of a launch from which a grid's caches are filled at its first use: forming the rows and
// sines in the kernel costs ~2-5 ps per ray (cfg2: +2 us, 1.07x; cfg4 at 8.7e8 rays: +4.3 ms,
// 1.21x), the two fill kernels ~10-20 us.
constexpr long long kFillFirstRays = 1LL << 22;

static int row_consts_cached(const DevMedium& M, const IceConsts& I, const TableArgs& A,
                             hipStream_t st, bool fill_first, const RowConst** out) {
  const double gk[3] = {A.start_h, A.stop_h, A.step_h};
  std::vector<unsigned char> key(sizeof(M) + sizeof(I.bot) + sizeof(I.topend) + sizeof(gk) +
                                 sizeof(A.hsteps));
  unsigned char* kp = key.data();
  std::memcpy(kp, &M, sizeof(M));
  kp += sizeof(M);
  std::memcpy(kp, &I.bot, sizeof(I.bot));
  kp += sizeof(I.bot);
  std::memcpy(kp, I.topend, sizeof(I.topend));
  kp += sizeof(I.topend);
  std::memcpy(kp, gk, sizeof(gk));
  kp += sizeof(gk);
  std::memcpy(kp, &A.hsteps, sizeof(A.hsteps));
  auto fill = [&](void* p, hipStream_t s) {
    hipLaunchKernelGGL(rowconst_kernel, dim3((unsigned)((A.hsteps + 255) / 256)), dim3(256), 0, s,
                       M, I, A, static_cast<RowConst*>(p));
  };
  const void* p = nullptr;
  const int rc = row_cache().get(key, sizeof(RowConst) * (size_t)std::max(A.hsteps, 1), st, fill,
                                 fill_first, &p);
  *out = static_cast<const RowConst*>(p);
  return rc;
}

// The start-angle sines of an angle grid (the degree-to-radian factor and the angle grid).
static int angle_sines_cached(const DevMedium& M, const TableArgs& A, hipStream_t st,
                              bool fill_first, const double** out) {
  const double k5[5] = {M.d2r, A.start_a, A.stop_a, A.step_a, (double)A.asteps};
  std::vector<unsigned char> key(sizeof(k5));
  std::memcpy(key.data(), k5, sizeof(k5));
  auto fill = [&](void* p, hipStream_t s) {
    hipLaunchKernelGGL(angle_sines_kernel, dim3((unsigned)((A.asteps + 255) / 256)), dim3(256), 0,
                       s, M, A, static_cast<double*>(p));
  };
  const void* p = nullptr;
  const int rc = angle_cache().get(key, sizeof(double) * (size_t)std::max(A.asteps, 1), st, fill,
                                   fill_first, &p);
  *out = static_cast<const double*>(p);
  return rc;
}

// The air part of every ray of one launch (AirRecord; air_part_kernel), kept across launches: it
// reads the medium, the ice height's air-side constants, the row's Tx height and the column's
// launch angle, but not the antenna, so from the second table of one grid on -- one table per
// antenna depth, RunMultiRayCode.C:29-52 -- a build traces the ice segment only (the warm
// table_kernel).  Same entry life cycle as the two caches above, never filled at first use.  The
// key is the bytes of everything ray_air_part, row_const and the Fresnel coefficients read -- the
// medium, I.bot, I.lower, I.topend, the two indices at the ice surface and their ratio, the height
// grid, the angle grid -- and the launch's row range, so a row slab keeps its own rays; the
// antenna depth (I.iceseg, I.ice_rx) and in_ice are not in it.
// A record is 32 B per ray, so this cache has byte limits instead of an entry count alone: no
// record above kAirEntryBytes (cfg4-sized launches are never cached), kAirTotalBytes per device.
// AIRICE_AIR_CACHE_MB=<n> sets the per-device total (and caps the entry limit at it), 0 turns the
// cache off; airice_air_cache_limits sets both in-process.
constexpr size_t kAirEntryBytes = (size_t)320 << 20;  // the reference's default grid: 8.73e6 rays, 279 MB
constexpr size_t kAirTotalBytes = (size_t)640 << 20;
static GridCache& air_cache() {
  static GridCache c = [] {
    GridCache g;
    size_t entry = kAirEntryBytes, total = kAirTotalBytes;
    if (const char* e = getenv("AIRICE_AIR_CACHE_MB")) {
      char* end = nullptr;
      const long long mb = strtoll(e, &end, 10);
      if (end != e && mb >= 0) {
        total = (size_t)mb << 20;
        entry = std::min(entry, total);
      }
    }
    (void)g.set_limits(entry, total);
    return g;
  }();
  return c;
}

template <bool A1>
static void launch_air_part(const DevMedium& M, const IceConsts& I, const TableArgs& A,
                            hipStream_t s) {
  const unsigned blocks = (unsigned)((A.n + kTableBlock - 1) / kTableBlock);
  hipLaunchKernelGGL(air_part_kernel<A1>, dim3(blocks), dim3(kTableBlock),
                     sizeof(RowConst) * (size_t)A.rows_per_block, s, M, I, A);
}

// A: the launch's arguments with row0, n and the row / sine caches set.  rows: its row count.
static int air_part_cached(const DevMedium& M, const IceConsts& I, const TableArgs& A, int rows,
                           hipStream_t st, unsigned char** out) {
  *out = nullptr;
  const size_t bytes = air_record_bytes((size_t)A.n);
  // (kAirRecordMaxBytes: the kernels address a record with 32-bit lane offsets, AirRecord)
  if (bytes == 0 || bytes >= kAirRecordMaxBytes || bytes > air_cache().entry_cap() ||
      bytes > air_cache().total_cap())
    return AIRICE_OK;  // before the key is built: a launch that is never cached pays nothing
  const double gk[6] = {A.start_h, A.stop_h, A.step_h, A.start_a, A.stop_a, A.step_a};
  const int ik[4] = {A.hsteps, A.asteps, A.row0, rows};
  const double fk[3] = {I.n_air_ice, I.n_ice0, I.n_ratio};
  std::vector<unsigned char> key(sizeof(M) + sizeof(I.bot) + sizeof(I.lower) + sizeof(I.topend) +
                                 sizeof(fk) + sizeof(gk) + sizeof(ik));
  unsigned char* kp = key.data();
  auto put = [&kp](const void* p, size_t n) {
    std::memcpy(kp, p, n);
    kp += n;
  };
  put(&M, sizeof(M));
  put(&I.bot, sizeof(I.bot));
  put(I.lower, sizeof(I.lower));
  put(I.topend, sizeof(I.topend));
  put(fk, sizeof(fk));
  put(gk, sizeof(gk));
  put(ik, sizeof(ik));
  auto fill = [&](void* p, hipStream_t s) {
    TableArgs F = A;
    F.air = static_cast<unsigned char*>(p);
    count_launch(LC_AIR_PART);
    if (M.A_air == 1.0)
      launch_air_part<true>(M, I, F, s);
    else
      launch_air_part<false>(M, I, F, s);
  };
  const void* p = nullptr;
  const int rc = air_cache().get(key, bytes, st, fill, false, &p);
  *out = static_cast<unsigned char*>(const_cast<void*>(p));
  return rc;
}

void air_cache_stats(long long out[6]) {
  std::lock_guard<std::mutex> lock(grid_cache_mutex());
  int k = 0, f = 0, p = 0;
  size_t b = 0;
  air_cache().stats(&k, &f, &p, &b);
  auto lim = [](size_t v) { return v > (size_t)INT64_MAX ? (long long)INT64_MAX : (long long)v; };
  out[0] = k;
  out[1] = f;
  out[2] = p;
  out[3] = (long long)b;
  out[4] = lim(air_cache().entry_cap());
  out[5] = lim(air_cache().total_cap());
}

int air_cache_limits(long long entry_bytes, long long total_bytes) {
  std::lock_guard<std::mutex> lock(grid_cache_mutex());
  GridCache& c = air_cache();
  return c.set_limits(entry_bytes < 0 ? c.entry_cap() : (size_t)entry_bytes,
                      total_bytes < 0 ? c.total_cap() : (size_t)total_bytes);
}

void table_cache_stats(int out[6]) {
  std::lock_guard<std::mutex> lock(grid_cache_mutex());
  row_cache().stats(&out[0], &out[1], &out[2]);
  angle_cache().stats(&out[3], &out[4], &out[5]);
}

// Rows a block's kTableBlock rays can touch, for the LDS row constants.
static inline int table_rows_per_block(int angle_steps) {
  return std::min(kTableBlock, (kTableBlock - 1) / angle_steps + 2);
}

// The grid's part of a table launch's arguments; the launcher adds row0, n, half and the caches
// (rc, vs).  Written in place over zeroed bytes, padding included: launch_table_multi compares
// the packed arguments of its antenna sets bytewise.
static void table_args(TableArgs& A, const airice_grid& g, size_t ld, int rows_per_block) {
  std::memset(&A, 0, sizeof(A));
  A.start_h = g.start_height;
  A.stop_h = g.stop_height;
  A.step_h = g.height_step;
  A.start_a = g.start_angle;
  A.stop_a = g.stop_angle;
  A.step_a = g.angle_step;
  A.inv_asteps = 1.0 / (double)g.angle_steps;
  A.hsteps = g.height_steps;
  A.asteps = g.angle_steps;
  A.in_ice = g.in_ice;
  A.rows_per_block = rows_per_block;
  A.ld = ld;
}

int launch_table(const DevMedium& M, const IceConsts& I, const airice_grid* g, int row_begin,
                 int row_count, float* d_table, double* d_full, size_t ld, hipStream_t st,
                 const FirnLeg* F) {
  if (row_count <= 0 || g->angle_steps <= 0) return AIRICE_OK;
  TableArgs A;
  table_args(A, *g, ld, table_rows_per_block(g->angle_steps));
  std::unique_lock<std::mutex> rs_lock(grid_cache_mutex());  // held until the launches are enqueued
  const bool fill_first = (long long)row_count * g->angle_steps >= kFillFirstRays;
  if (int rc = row_consts_cached(M, I, A, st, fill_first, &A.rc)) return rc;
  if (int rc = angle_sines_cached(M, A, st, fill_first, &A.vs)) return rc;
  static const char* trace_env = getenv("AIRICE_TABLE_TRACE");
  const char* trace_path = F != nullptr ? nullptr : trace_env;  // the timeline has no layered form
  // ray indices are 32-bit inside a launch: grids of kMaxLaunchRays or more go in row slabs
  const int max_rows = (int)std::max<long long>(1, (kMaxLaunchRays - 2 * kTableBlock) / g->angle_steps);
  // a plain build (11 columns, one launch) of a launch seen before reads its rays' air part from
  // the air record and traces the ice segment only
  if (d_full == nullptr && trace_path == nullptr && row_count <= max_rows) {
    A.row0 = row_begin;
    A.n = row_count * g->angle_steps;
    if (int rc = air_part_cached(M, I, A, row_count, st, &A.air)) return rc;
  }
  for (int done = 0; done < row_count;) {
    const int rows = std::min(max_rows, row_count - done);
    const size_t off = (size_t)done * (size_t)g->angle_steps;
    A.row0 = row_begin + done;
    A.n = rows * g->angle_steps;
    float* tab = d_table + off;
    double* full = d_full ? d_full + off : nullptr;
    done += rows;
    A.half = A.n;
    const size_t lds = sizeof(RowConst) * (size_t)A.rows_per_block;
    const unsigned blocks = (unsigned)((A.n + kTableBlock - 1) / kTableBlock);
    if (trace_path == nullptr) {
      ktimer_begin(KT_TABLE, st);
      count_launch(LC_TABLE);
      const bool sc1 = A.n < kAgentStoreRays;
      auto kern = M.A_air == 1.0
                      ? (sc1 ? table_kernel<false, true, true> : table_kernel<false, true, false>)
                      : (sc1 ? table_kernel<false, false, true> : table_kernel<false, false, false>);
      if (A.air != nullptr)
        kern = sc1 ? table_kernel<false, false, true, true> : table_kernel<false, false, false, true>;
      if (F != nullptr) {
        const bool a1 = M.A_air == 1.0;
        auto fkern = a1 ? (sc1 ? table_firn_kernel<true, true> : table_firn_kernel<true, false>)
                        : (sc1 ? table_firn_kernel<false, true> : table_firn_kernel<false, false>);
        if (A.air != nullptr)
          fkern = sc1 ? table_firn_kernel<false, true, true> : table_firn_kernel<false, false, true>;
        hipLaunchKernelGGL(fkern, dim3(blocks), dim3(kTableBlock), A.air != nullptr ? 0 : lds, st,
                           M, I, *F, A, tab, full);
      } else {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(kTableBlock), A.air != nullptr ? 0 : lds, st,
                           M, I, A, tab, full, nullptr);
      }
      ktimer_end(KT_TABLE, st);
      if (hipGetLastError() != hipSuccess) return AIRICE_EHIP;
      continue;
    }
    // debug timeline (tools/wave_timeline.py): synchronous, one record per wave appended
    const long long nw = (long long)blocks * (kTableBlock / 64);
    WaveTrace* dtr = nullptr;
    if (hipMalloc(&dtr, sizeof(WaveTrace) * nw) != hipSuccess) return AIRICE_EHIP;
    hipLaunchKernelGGL((table_kernel<true, false, true>), dim3(blocks), dim3(kTableBlock), lds, st, M, I,
                       A, tab, full, dtr);
    std::vector<WaveTrace> h(nw);
    if (hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpy(h.data(), dtr, sizeof(WaveTrace) * nw, hipMemcpyDeviceToHost) != hipSuccess)
      return AIRICE_EHIP;
    (void)hipFree(dtr);
    if (FILE* f = fopen(trace_path, "ab")) {
      fwrite(h.data(), sizeof(WaveTrace), nw, f);
      fclose(f);
    }
  }
  return launch_ok();
}

// Several antennas' whole tables in one launch of table_multi_kernel.  Ih[a], grids[a]: antenna
// a's constants and grid (the rows it holds: grids[a].table_rows); tables[a] its output, column
// stride lds[a].  The per-antenna constants live in a device buffer per distinct set, kept for
// repeated launches of the same set (bench steps, repeated builds).
// Fh (nullable): antenna a's lower firn leg; the launch then runs table_multi_firn_kernel.
int launch_table_multi(const DevMedium& M, const IceConsts* Ih, const airice_grid* grids, int n,
                       float* const* tables, const size_t* lds, hipStream_t st,
                       const FirnLeg* Fh) {
  if (n <= 0) return AIRICE_OK;
  if (n > kMaxAntennas) {
    set_error("at most %d antennas per multi-antenna launch", kMaxAntennas);
    return AIRICE_EINVAL;
  }
  std::vector<TableArgs> Ah(n);
  std::unique_lock<std::mutex> rs_lock(grid_cache_mutex());  // held until the launch is enqueued
  MultiMap map;
  std::memset(&map, 0, sizeof(map));
  map.n_ant = n;
  long long blocks = 0;
  const int rpb = [&] {
    int r = 2;
    for (int a = 0; a < n; ++a)
      r = std::max(r, table_rows_per_block(grids[a].angle_steps));
    return r;
  }();
  for (int a = 0; a < n; ++a) {
    const airice_grid* g = &grids[a];
    TableArgs& A = Ah[a];
    table_args(A, *g, lds[a], rpb);
    const bool fill_first = (long long)g->table_rows * g->angle_steps >= kFillFirstRays;
    if (int rc = row_consts_cached(M, Ih[a], A, st, fill_first, &A.rc)) return rc;
    if (int rc = angle_sines_cached(M, A, st, fill_first, &A.vs)) return rc;
    const long long rays = (long long)g->table_rows * g->angle_steps;
    if (rays >= kMaxLaunchRays - 2 * kTableBlock || lds[a] < (size_t)rays) {
      set_error("antenna %d: %lld rays (ld %zu) do not fit one multi-antenna launch", a, rays,
                lds[a]);
      return AIRICE_EINVAL;
    }
    A.n = (int)rays;
    A.half = A.n;
    map.begin[a] = (int)blocks;
    map.table[a] = tables[a];
    blocks += (rays + kTableBlock - 1) / kTableBlock;
  }
  map.begin[n] = (int)blocks;
  if (blocks == 0) return AIRICE_OK;
  // the device copy of the per-antenna constants (ConstSetCache; the lock is held)
  static ConstSetCache const_sets;
  const size_t bytes_i = sizeof(IceConsts) * n, bytes_ia = bytes_i + sizeof(TableArgs) * n;
  const size_t bytes = bytes_ia + (Fh != nullptr ? sizeof(FirnLeg) * n : 0);
  std::vector<unsigned char> packed(bytes);
  std::memcpy(packed.data(), Ih, bytes_i);
  std::memcpy(packed.data() + bytes_i, Ah.data(), sizeof(TableArgs) * n);
  if (Fh != nullptr) std::memcpy(packed.data() + bytes_ia, Fh, sizeof(FirnLeg) * n);
  void* dconst = nullptr;
  if (int rc = const_sets.get(packed, stream_capturing(st), &dconst)) {
    if (rc == AIRICE_EINVAL)
      set_error("multi-antenna table launch under graph capture: run one uncaptured launch of the "
                "same antenna set (twice: the grid caches fill on a grid's second launch) first");
    return rc;
  }
  const size_t lds_bytes = sizeof(RowConst) * (size_t)rpb;
  const bool sc1 = (long long)blocks * kTableBlock < kAgentStoreRays;
  auto multi = M.A_air == 1.0 ? (sc1 ? table_multi_kernel<true, true> : table_multi_kernel<true, false>)
                              : (sc1 ? table_multi_kernel<false, true> : table_multi_kernel<false, false>);
  if (Fh != nullptr) {
    auto fmulti = M.A_air == 1.0
                      ? (sc1 ? table_multi_firn_kernel<true, true> : table_multi_firn_kernel<true, false>)
                      : (sc1 ? table_multi_firn_kernel<false, true> : table_multi_firn_kernel<false, false>);
    unsigned char* dc = static_cast<unsigned char*>(dconst);
    return bracket_launch(LC_TABLE, KT_TABLE, st, [&] {
      hipLaunchKernelGGL(fmulti, dim3((unsigned)blocks), dim3(kTableBlock), lds_bytes, st, M,
                         reinterpret_cast<const IceConsts*>(dc),
                         reinterpret_cast<const FirnLeg*>(dc + bytes_ia),
                         reinterpret_cast<const TableArgs*>(dc + bytes_i), map);
    });
  }
  return bracket_launch(LC_TABLE, KT_TABLE, st, [&] {
    hipLaunchKernelGGL(multi, dim3((unsigned)blocks), dim3(kTableBlock), lds_bytes, st, M,
                       static_cast<const IceConsts*>(dconst),
                       reinterpret_cast<const TableArgs*>(static_cast<unsigned char*>(dconst) +
                                                          bytes_i),
                       map);
  });
}

int launch_rays(const DevMedium& M, const IceConsts& I, const double* launch, const double* txh,
                int in_ice, size_t n, double* out, size_t ld, hipStream_t st, const FirnLeg* F) {
  if (n == 0) return AIRICE_OK;
  if (F != nullptr)  // a layered firn: rays_firn_kernel for every n (one ray: one lane)
    return bracket_launch(LC_RAYS, kNoTimer, st, [&] {
      hipLaunchKernelGGL(rays_firn_kernel, dim3(grid_for((long long)n)), dim3(kBlock), 0, st, M, I,
                         *F, launch, txh, in_ice, (long long)n, out, ld);
    });
  if (n == 1)  // one ray: spread over a wave (ray_solution_wave)
    return bracket_launch(LC_SCALAR_RAY, kNoTimer, st, [&] {
      hipLaunchKernelGGL(scalar_ray_kernel, dim3(1), dim3(64), 0, st, M, I, launch, txh, in_ice,
                         out, ld, take_scalar_signal());
    });
  return bracket_launch(LC_RAYS, kNoTimer, st, [&] {
    hipLaunchKernelGGL(rays_kernel, dim3(grid_for((long long)n)), dim3(kBlock), 0, st, M, I, launch,
                       txh, in_ice, (long long)n, out, ld, Signal{});
  });
}

// The one-query GetRayTracingSolutions on the host (airice_rays_host): ray_solution compiled for
// the CPU from the same source as rays_kernel -- the same operation sequence, with the host's
// correctly rounded sqrt and quotients in place of the device's v_rsq/v_rcp iterations (within
// ~1 ulp of them).  A one-ray launch costs a kernel dispatch and a completion wait (~8 us); the
// host ray takes ~1 us.
void rays_host(const DevMedium& M, const IceConsts& I, const double* launch, const double* txh,
               int in_ice, size_t n, double* out, size_t ld, const FirnLeg* F) {
  if (F != nullptr) return rays_host_firn(M, I, *F, launch, txh, in_ice, n, out, ld);
  for (size_t k = 0; k < n; ++k) {
    double d[18];
    ray_solution(M, I, launch[k], txh[k], in_ice != 0, d);
    for (int c = 0; c < 18; ++c) out[c * ld + k] = d[c];
  }
}

}  // namespace airice
