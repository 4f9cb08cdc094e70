// airice_internal.h -- host-side internals shared by the runtime and the launchers.
//
// The kernels live in airice_table.hip (forward ray: table, rays), airice_solve.hip (minimizer),
// airice_lookup.hip (the lookup's pack kernels), airice_path.hip, airice_rtf.hip and the in-ice
// units (airice_iceray.hip, airice_icesol.hip, airice_icespec.hip, airice_icetab.hip,
// airice_icepath.hip, airice_iceair.hip, airice_icefirst.hip); each opens with its own inventory.
// Data layout in HBM: structure-of-arrays, column c of item i at out[c*ld + i], so each
// wave's store of one column is one contiguous 256 B (f32) / 512 B (f64) segment.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>

#include "airice.h"
#include "airice_device.hpp"
#include "airice_host.h"

// Library-internal names that are new to a header: kept out of libairice.so's dynamic symbols.
#define AIRICE_LOCAL __attribute__((visibility("hidden")))

namespace airice {

// Launch-shape constants and launcher helpers shared by the kernel units.
constexpr int kBlock = 256;
constexpr int kRootsWaves = 4;  // 127 VGPRs: 4 waves/SIMD (5 and 6 spill and run slower)
inline unsigned grid_for(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }
inline int launch_ok() { return hipGetLastError() == hipSuccess ? AIRICE_OK : AIRICE_EHIP; }
// AIRICE_BISECT_EXACT=1 (debug / validation): the root finder evaluates every bisection midpoint
// (airice_solve.hip).
AIRICE_LOCAL int bisect_exact();

// The host folds (airice_fold.cpp).
// Kernel-argument medium for one variant (pi) built from the parsed medium; the
// layer-boundary endpoints are evaluated here, on the host, once.
int build_dev_medium(const airice_medium* m, int variant, DevMedium* out);
// Batch-uniform ice endpoints: ice height ice_h (m) and antenna depth rx_depth (m, >= 0).
void build_ice_consts(const DevMedium& M, double ice_h, double rx_depth, IceConsts* out);

Endpoint host_air_endpoint(const DevMedium& M, double x);
Endpoint host_ice_endpoint(const DevMedium& M, double x);
// Two-layer firn (airice_firn).  firn_check: the argument check of the *_firn entry
// points (sets the error, AIRICE_EINVAL).  The upper leg is the one-layer fold of
// firn_layer_medium(m, f, 0) with the antenna depth clipped to the boundary (firn_clip_depth);
// build_firn_leg folds the lower leg from that medium's DevMedium and the unclipped depth
// rx_depth (m, >= 0 in the ice).  rays_host_firn: rays_host's loop over the layered ray.
AIRICE_LOCAL int firn_check(const char* who, const airice_firn* f);
AIRICE_LOCAL airice_medium firn_layer_medium(const airice_medium& m, const airice_firn& f,
                                             int layer);
AIRICE_LOCAL double firn_clip_depth(const airice_firn& f, double rx_depth);
AIRICE_LOCAL void build_firn_leg(const DevMedium& M, const airice_firn& f, double rx_depth,
                                 FirnLeg* out);
AIRICE_LOCAL void rays_host_firn(const DevMedium& M, const IceConsts& I, const FirnLeg& F,
                                 const double* launch, const double* txh, int in_ice, size_t n,
                                 double* out, size_t ld);

// F / Fh (nullable, here and in launch_rays / rays_host): the lower leg of a two-layer firn
// (build_firn_leg); M and I then describe the upper layer and the layered kernels run.
int launch_table(const DevMedium& M, const IceConsts& I, const airice_grid* g, int row_begin,
                 int row_count, float* d_table, double* d_full, size_t ld, hipStream_t st,
                 const FirnLeg* F = nullptr);
int launch_table_multi(const DevMedium& M, const IceConsts* Ih, const airice_grid* grids, int n,
                       float* const* tables, const size_t* lds, hipStream_t st,
                       const FirnLeg* Fh = nullptr);
// entries of the table launch's per-grid caches (airice_table_cache_stats)
void table_cache_stats(int out[6]);
// the air-record cache of the table launch (airice_air_cache_stats / airice_air_cache_limits):
// keys, filled, pinned, bytes held on the current device, then the entry and total byte limits
void air_cache_stats(long long out[6]);
int air_cache_limits(long long entry_bytes, long long total_bytes);
int launch_rays(const DevMedium& M, const IceConsts& I, const double* launch, const double* txh,
                int in_ice, size_t n, double* out, size_t ld, hipStream_t st,
                const FirnLeg* F = nullptr);
void rays_host(const DevMedium& M, const IceConsts& I, const double* launch, const double* txh,
               int in_ice, size_t n, double* out, size_t ld, const FirnLeg* F = nullptr);
// one query of the minimizer entry points on the host (airice_solve.hip: solve_one_host_t)
int solve_host_one(const DevMedium& M, const IceConsts& I, int variant, const double* in,
                   bool has_thr, double* out, uint8_t* status);
int hdtip_host_one(const DevMedium& M, const IceConsts& I, double ice_cm, const double* in,
                   double* out9, uint8_t* ok);
int trace_host_one(const DevMedium& M, const IceConsts& I, const double* in, double* out10);
int lookup_fallback_host_one(const DevMedium& M, const IceConsts& I, double ice_cm,
                             const double* in, double* out9, uint8_t* ok, const uint8_t* flags);
int launch_solve(const DevMedium& M, const IceConsts& I, int variant, const double* txh,
                 const double* dist, const double* depth, const double* thr, size_t n,
                 double* out, size_t ld, uint8_t* status, hipStream_t st);
int launch_hdtip(const DevMedium& M, const IceConsts& I, const double* src, const double* dist,
                 const double* depth, double ice_cm, size_t n, double* out, size_t ld,
                 uint8_t* ok, hipStream_t st);
// Stream-ordered scratch from a library-owned pool that keeps freed blocks (hipFreeAsync).
hipError_t scratch_alloc(void** p, size_t bytes, hipStream_t st);
// Batch size from which the minimizer groups the queries of source `in` batch-wide
// (AIRICE_GROUP_MIN overrides it; 0 when a source never groups by default).
size_t group_min_batch(int in);
// Table lookup: lookup_kernel, each AIRICE_LOOKUP_FALLBACK lane solving its minimizer fallback
// in place (airice_solve.hip; the pack kernels: airice_lookup.hip).
int launch_lookup(const DevMedium& M, const IceConsts& I, const airice_lookup_table* t,
                  const double* src, const double* dist, const double* depth, double ice_cm,
                  size_t n, double* out, size_t ld, uint8_t* ok, uint8_t* flags, hipStream_t st);
// The same for n_ant antennas x n_src sources in ONE launch (lookup_multi_kernel): the tables'
// descriptions and each antenna's (table, Rx depth) are uploaded into d_work
// (lookup_multi_work_bytes), no allocation.  The caller has validated every argument.
size_t lookup_multi_work_bytes(size_t n_tables, size_t n_ant);
int launch_lookup_multi(const DevMedium& M, const IceConsts& I, const airice_lookup_table* tables,
                        int n_tables, const int32_t* antenna_table, const double* antenna_depth_cm,
                        size_t n_ant, const double* src, const double* dist, size_t ld_dist,
                        double ice_cm, size_t n_src, double* out, size_t ld, uint8_t* ok,
                        uint8_t* flags, void* d_work, hipStream_t st);
int launch_lookup_pack(const airice_lookup_table* t, float* entries, hipStream_t st);
// the lookup's fallback for one query on the device (batches solve theirs in lookup_kernel)
int launch_lookup_fallback(const DevMedium& M, const IceConsts& I, const double* src,
                           const double* dist, const double* depth, double ice_cm, double* out,
                           size_t ld, uint8_t* ok, const uint8_t* flags, hipStream_t st);
// SingleRayAirIceRefraction (airice_path.hip).  d_work: AIRICE_SINGLE_RAY_WORK doubles.
int plan_single_ray(const airice_medium* m, double depth, double launch, double txh, double ice,
                    airice_single_ray_info* info);
int launch_single_ray(const DevMedium& M, const airice_medium* m, double depth, double launch,
                      double txh, double ice, double* d_work, double* d_x, double* d_z,
                      size_t cap, hipStream_t st);
// The batch of the same sampler: n rays sharing depth and ice, per-ray Tx height (host) and
// launch angle (device).  The plan is host-only; the launch uploads the per-ray plans and the
// tile list into d_work (work_bytes from the plan) and makes no allocation.
int plan_ray_paths(const airice_medium* m, double depth, double ice, const double* txh, size_t n,
                   int64_t* offsets, size_t* work_bytes);
int launch_ray_paths(const DevMedium& M, const airice_medium* m, double depth, double ice,
                     const double* d_launch, const double* txh, size_t n, const int64_t* offsets,
                     void* d_work, size_t work_bytes, double* d_summary, size_t ld, double* d_x,
                     double* d_z, size_t cap, hipStream_t st);
// RayTracingFunctions:: scalar layer (airice_rtf.hip): one call, one lane, d_out >= outputs
int rtf_outputs(int op, int max_layers);
int rtf_host(const DevMedium& M, int op, const double* args, size_t n_args, double* out);
// one-query calls on the host (airice_runtime.cpp): the mode, and per-thread cached folds
bool scalar_on_host();
int set_scalar_mode(int mode);
int folded_medium(const airice_medium* m, int variant, const DevMedium** out);
int folded_ice(const airice_medium* m, int variant, double ice_h, double rx_depth,
               const DevMedium** M, const IceConsts** I);
int launch_rtf(const DevMedium& M, int op, const double* args, size_t n_args, double* d_out,
               hipStream_t st);
int launch_trace(const DevMedium& M, const IceConsts& I, const double* depth, const double* ice,
                 const double* txh, const double* dist, size_t n, double* out10, hipStream_t st);
// The Air2IceRayTracing.C Brent solve, batched (airice_rtf.hip): air2ice_kernel, one query per
// lane, 16 columns of stride ld and a status byte (nullable); air2ice_host_one is the lane's
// function on the calling thread (in: txh, dist, ice, depth).
int launch_air2ice(const DevMedium& M, const double* txh, const double* dist, const double* ice,
                   const double* depth, size_t n, double* out, size_t ld, uint8_t* status,
                   hipStream_t st);
void air2ice_host_one(const DevMedium& M, const double in[4], double* out16, uint8_t* status);
// The in-ice solver, batched (airice_iceray.hip): iceray_kernel, one (z0, x1, z1) pair per lane,
// AIRICE_ICERAY_FIELDS columns of stride ld and a status byte (nullable); model = {A, B, C}.  The
// lane's function on the calling thread is iceray_host_one (airice_host.h).
int launch_iceray(const double model[3], const double* z0, const double* x1, const double* z1,
                  size_t n, double* out, size_t ld, uint8_t* status, hipStream_t st);
// GetRayTracingSolutions / GetFocusingFactor over the solver's rows (airice_icesol.hip):
// icesol_kernel, one pair per lane, AIRICE_ICESOL_FIELDS columns of stride ld and a status byte
// (nullable); rays_lower nullable (no focusing).  The lane's function on the calling thread is
// icesol_host_one (airice_host.h).
int launch_icesol(const double model[3], double a0, double frequency_ghz, const double* z0,
                  const double* x1, const double* z1, const double* rays, size_t ld_rays,
                  const double* rays_lower, size_t ld_lower, size_t n, double* out, size_t ld,
                  uint8_t* status, hipStream_t st);
// The two chosen rays' attenuation at n_freq frequencies (airice_icespec.hip):
// icesol_spectrum_kernel, icespec_pairs_per_block(n_freq) pairs per block, over the solver's rows
// and the type columns of launch_icesol's output; att[(2 i + slot) ld_f + k].  The pair's function
// on the calling thread is icespec_host_one (airice_host.h).
AIRICE_LOCAL unsigned icespec_pairs_per_block(size_t n_freq);
AIRICE_LOCAL int launch_icespec(const double model[3], double a0, const double* z0,
                                const double* z1, const double* rays, size_t ld_rays,
                                const double* sol, size_t ld_sol, size_t n, const double* freq,
                                size_t n_freq, double* att, size_t ld_f, hipStream_t st);
// The ice-to-air direct ray, batched (airice_iceair.hip): iceair_kernel, one (z0, x1, h) triple per
// lane, AIRICE_ICEAIR_FIELDS columns of stride ld and a status byte (nullable).  The lane's
// function on the calling thread is iceair_host_one (airice_host.h).
AIRICE_LOCAL int launch_iceair(const double model[3], const double* z0, const double* x1,
                               const double* h, size_t n, double* out, size_t ld, uint8_t* status,
                               hipStream_t st);
// The first-arriving ray of n (emitter, antenna) pairs (airice_icefirst.hip): icefirst_geom_kernel,
// iceray_kernel and icefirst_select_kernel over work (icefirst::kWorkDoubles doubles per pair);
// cross: pair t*n_rx + r, else pair i = (tx i, rx i).  AIRICE_ICEFIRST_FIELDS columns of stride ld
// and a status byte (nullable).  One pair on the calling thread is icefirst_host_one.
AIRICE_LOCAL int launch_icefirst(const double model[3], const double* tx_x, const double* tx_y,
                                 const double* tx_z, const double* rx_x, const double* rx_y,
                                 const double* rx_z, size_t n_rx, bool cross, size_t n,
                                 double* work, double* out, size_t ld, uint8_t* status,
                                 hipStream_t st);

// The last of those launches on its own: the choice over rows launch_iceray wrote (stride ld_rays).
AIRICE_LOCAL int launch_icefirst_select(const double* rays, size_t ld_rays, const double* x1,
                                        size_t n, double* out, size_t ld, uint8_t* status,
                                        hipStream_t st);

static_assert(kMaxParsedLayers == kMaxLayers, "parse and kernels agree on the layer count");

// One-query calls of the scalar drop-ins (the C++ MultiRayAirIceRefraction:: / RayTracingFunctions::
// functions, Py_TraceIceToAir, airice_rtf_eval): a pinned, device-mapped staging block per device
// that the host fills with the inputs and the kernels read and write in place (no copies), and a
// library-owned non-blocking stream; a call is its launches plus one wait.
// The slot of the current device (hipGetDevice) is created on first use and locked for the call.
// A call made of ONE kernel launch arms the slot's completion flag first (arm()); the launcher
// of that kernel takes the signal (take_scalar_signal) and passes it to the kernel, which stores
// the sequence number after its outputs (signal_done); sync() then spins on the pinned flag
// instead of synchronising the stream (launch + wait 7.8 us instead of 11-12 us).
struct ScalarSlot {
  double* h = nullptr;  // host view
  double* d = nullptr;  // device view of the same memory
  hipStream_t st = nullptr;
  unsigned* flag_h = nullptr;  // completion flag: host view
  unsigned* flag_d = nullptr;  //                  device view
  unsigned seq = 0;
};
constexpr size_t kScalarSlotDoubles = 512;
class ScalarCall {
 public:
  ScalarCall();  // on failure ok() is false and airice_last_error() says why
  ~ScalarCall();
  bool ok() const { return slot_ != nullptr; }
  ScalarSlot& slot() { return *slot_; }
  // Arms the completion signal for the next launch on this thread (the call's only kernel);
  // in[0 .. n_in-1] (n_in <= 4): the query inputs in the launcher's order, passed inline.
  void arm(const double* in = nullptr, int n_in = 0);
  // Waits for the call: on the flag when the armed signal was taken by a launcher (falling back
  // to the stream after a bounded spin), else on the slot's stream; AIRICE_OK or AIRICE_EHIP.
  int sync();
 private:
  ScalarSlot* slot_ = nullptr;
  void* lock_ = nullptr;
  bool armed_ = false;
};
// The armed signal of this thread (cleared by taking it); Signal{} when none is armed.
Signal take_scalar_signal();
// One query of a minimizer entry point, from an airice_medium and host values: on the host (the
// cached folds, then the *_host_one above) when scalar_on_host(), else on the device through the
// scalar slot.  The outputs are the entry point's columns with ld = 1.
// Air2IceRayTracing (in: txh, dist, depth, straight angle -- read when has_thr; status: optional).
int solve_one(const airice_medium* m, int variant, double ice_h, const double in[4], bool has_thr,
              double* out, uint8_t* status);
// GetHorizontalDistanceToIntersectionPoint (in: src, dist, depth in cm).
int hdtip_one(const airice_medium* m, double ice_cm, const double in[3], double out9[9],
              uint8_t* ok);
// TraceIceToAir (in: depth, ice, txh, dist).
int trace_one(const airice_medium* m, const double in[4], double out10[10]);
// The table lookup's minimizer fallback for a query that lk_query flagged one-sided
// (.cc:1418-1420): out9 / *ok as the batch lookup.
int lookup_fallback_one(const airice_medium* m, double src_cm, double dist_cm, double depth_cm,
                        double ice_cm, bool good, int flags, double out9[9], bool* ok);

// Kernel timing for the bench (airice_kernel_timing): when enabled, launches of the kernels
// below are bracketed by a hipEvent pair on their stream.  Off by default: one relaxed load.
enum KTimerId {
  KT_TABLE = 0,
  KT_ROOTS,
  KT_GROUP,
  KT_OUT,
  KT_LOOKUP,
  KT_RAY_CONSTS,
  KT_RAY_PATHS,
  KT_LOOKUP_MULTI,
  KT_AIR2ICE,
  KT_ICERAY,
  KT_ICESOL,
  KT_ICETAB_POINTS,
  KT_ICETAB_PACK,
  KT_ICETAB_LOOKUP,
  KT_ICEPATH_CONSTS,
  KT_ICEPATH,
  KT_ICESPEC,
  KT_ICEAIR,
  KT_ICEFIRST_GEOM,
  KT_ICEFIRST_SELECT,
  KT_COUNT
};
extern std::atomic<bool> g_ktimer_on;
void ktimer_record(int id, bool begin, hipStream_t st);
inline void ktimer_begin(int id, hipStream_t st) {
  if (g_ktimer_on.load(std::memory_order_relaxed)) ktimer_record(id, true, st);
}
inline void ktimer_end(int id, hipStream_t st) {
  if (g_ktimer_on.load(std::memory_order_relaxed)) ktimer_record(id, false, st);
}

// Launch counters (airice_launch_count), always on: one relaxed increment per launch, so a test
// can assert that the kernel it means to check ran (a host route cannot pass for a device test).
enum LaunchId {
  LC_TABLE = 0,     // table_kernel (single- and multi-antenna)
  LC_RAYS,          // rays_kernel
  LC_SCALAR_RAY,    // scalar_ray_kernel (one-query GetRayTracingSolutions)
  LC_ROOTS,         // roots_kernel / roots_sorted_kernel (batched root finder)
  LC_SCALAR_SOLVE,  // scalar_solve_kernel (one-query minimizer entry points)
  LC_OUT,           // the batch stage-2 kernels: solve_out / hdtip_out / trace_out (launch_entry)
  LC_LOOKUP,        // lookup_kernel
  LC_RTF,           // rtf_kernel (ray layer, GSL-Brent search)
  LC_SINGLE_RAY,    // single_ray_kernel
  LC_PATH,          // path_kernel
  LC_RAY_CONSTS,    // ray_consts_kernel
  LC_RAY_PATHS,     // ray_paths_kernel
  LC_LOOKUP_MULTI,  // lookup_multi_kernel
  LC_AIR2ICE,       // air2ice_kernel (batched GSL-Brent point-to-point solve)
  LC_AIR_PART,      // air_part_kernel (fills a table launch's air record)
  LC_ICERAY,        // iceray_kernel (batched in-ice direct / reflected / refracted solve)
  LC_ICESOL,        // icesol_kernel (the two rays a receiver sees, attenuation, focusing)
  LC_ICETAB_POINTS, // icetab_points_kernel (an in-ice table build's positions and header)
  LC_ICETAB_PACK,   // icetab_pack_kernel (one record per position)
  LC_ICETAB_LOOKUP, // icetab_lookup_kernel (the in-ice table read)
  LC_ICEPATH_CONSTS, // icepath_consts_kernel (an in-ice path batch's per-ray records)
  LC_ICEPATH,       // icepath_kernel (the in-ice ray-path samples)
  LC_ICESPEC,       // icesol_spectrum_kernel (the two rays' attenuation over a frequency grid)
  LC_ICEAIR,        // iceair_kernel (batched ice-to-air direct ray)
  LC_ICEFIRST_GEOM, // icefirst_geom_kernel (a first-arrival batch's (z0, x1, z1) triples)
  LC_ICEFIRST_SELECT, // icefirst_select_kernel (the first-arriving ray of each pair)
  LC_COUNT
};
extern std::atomic<long long> g_launches[LC_COUNT];
inline void count_launch(int id) { g_launches[id].fetch_add(1, std::memory_order_relaxed); }

// One kernel launch in its bracket: counted (lc), timed when the bench asks (kt; kNoTimer for a
// kernel without a timer), and its launch error read before the timer's end event is recorded.
// launch() issues the one hipLaunchKernelGGL on st.
constexpr int kNoTimer = -1;
template <class Launch>
inline int bracket_launch(int lc, int kt, hipStream_t st, Launch launch) {
  count_launch(lc);
  if (kt != kNoTimer) ktimer_begin(kt, st);
  launch();
  const hipError_t e = hipGetLastError();
  if (kt != kNoTimer) ktimer_end(kt, st);
  if (e == hipSuccess) return AIRICE_OK;
  set_error("kernel launch failed: %s", hipGetErrorString(e));
  return AIRICE_EHIP;
}

}  // namespace airice
