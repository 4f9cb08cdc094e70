// airice_solve.hip -- the minimizer kernels of libairice.so (gfx950), their stream-ordered
// launchers and the one-query host route, written over airice_minimizer.hpp (the root finder,
// EntryPoint<OUT>, stage2_out).
//
//  roots_kernel<IN>     : stage 1, one lane per query: bracket set-up, the 0.05-degree probe,
//                         GSL-bisection replay (tolerance 1e-9, 40 iterations) over a THD-only
//                         evaluator; each 1,024-query block sorted by straight-line angle in LDS.
//  group_count_kernel<IN>, group_scatter_kernel<IN>, roots_sorted_kernel<IN> : stage 1 of large
//                         trace batches, grouped across the whole batch first.
//  solve_out_kernel<V>, hdtip_out_kernel, trace_out_kernel : stage 2 of a batch, one full
//                         evaluation at the parked root, then the entry point's stores.
//  scalar_solve_kernel<IN, OUT> : one query (n = 1), both stages in one launch on one wave.
//  lookup_kernel        : the table lookup (.cc:1305-1462, airice_lookup.hpp); a lane that needs
//                         the reference's minimizer fallback solves it in place.
//  lookup_multi_kernel  : the same lookup for many antennas x many sources in one launch, one
//                         antenna per block, its table's description read through scalar loads.
//                         (Both sit here, not in airice_lookup.hip: they inline the root finder,
//                         and compiled in a unit without the other minimizer kernels their
//                         instruction order changes.)
// Launchers: launch_solve, launch_hdtip, launch_trace, launch_lookup_fallback (over launch_roots
// and launch_entry), launch_lookup, launch_lookup_multi; the host route: solve_one_host_t and the
// four *_host_one functions.
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
#include "airice_lookup.hpp"
#include "airice_device.hpp"
#include "airice_internal.h"
#include "airice_lean.hpp"
#include "airice_minimizer.hpp"

namespace airice {

#ifndef AIRICE_OUT_WAVES
#define AIRICE_OUT_WAVES 1
#endif
constexpr int kOutWaves = AIRICE_OUT_WAVES;  // stage-2 kernels: minimum waves per SIMD (1: no cap)
// trace_out_kernel held to 8 waves/SIMD: 64 VGPRs without scratch (94 uncapped, 5 waves), cfg5
// 1e7 trace calls 2.059-2.064 against 2.074-2.100 ms, same outputs (profiles/r06_ab/stage2_waves_ab.log);
// solve_out / hdtip_out capped at 5-8 waves measured within noise or slower (8: spills), uncapped
#ifndef AIRICE_TRACE_OUT_WAVES
#define AIRICE_TRACE_OUT_WAVES 8
#endif
constexpr int kTraceOutWaves = AIRICE_TRACE_OUT_WAVES;

// Debug/validation switch: AIRICE_BISECT_EXACT=1 makes the root finder evaluate f at every
// bisection midpoint instead of predicting the signs the guards determine (same roots).
int bisect_exact() {
  const char* e = getenv("AIRICE_BISECT_EXACT");
  return (e != nullptr && e[0] == '1') ? 1 : 0;
}

// Lanes of a wave run until its slowest query is solved, and the number of f-evaluations
// follows the geometry (near-horizontal queries probe and need more secant steps).  So the block
// first groups its queries by straight-line angle (a 24-bucket counting sort in LDS) and each
// lane then solves the query of its slot: waves hold similar queries (per-wave maximum 10.3 ->
// ~8.2 evaluations on cfg3, 0.52 -> 0.45 ms per 1e6 solves).  Every query is still solved on its
// own and written by its index.
// (round 5, six alternating A/B rounds of the cfg3 solve call, same outputs: 16 buckets median
// 0.2377 ms, 24 buckets 0.2351, 64 buckets 0.2362; 8 angle classes x the layers spanned 0.241)
constexpr int kSortBuckets = 24;
// 1024 queries per block: larger groups sort better, and a 16-wave block runs at 4 waves/SIMD
// (128 VGPRs) -- measured faster than 256 (3 waves, no spills), 512 and 768; and (round 5) than
// 512- and 256-thread blocks that each sort the whole 1,024-query chunk (a deterministic ballot
// sort) and solve their half / quarter of it: the same waves at a finer dispatch grain, 0.263 /
// 0.307 against 0.244 ms per call (the duplicated keying costs more than the block tail saves).
constexpr int kRootsBlock = 1024;
// batch-wide grouping: trace (IN_TRACE) batches of at least kGroupMin queries are sorted across
// the whole batch and solved in kSortedBlock-thread blocks (roots_sorted_kernel; group_min_batch:
// the other sources stay block-local, AIRICE_GROUP_MIN in the environment overrides it)
constexpr long long kGroupMin = 65536;

constexpr int kGroupAngles = 8;   // straight-line-angle classes (16 measured +0.4 %)
// the classes within each angle class are the number of air layers the path spans (0-3+): a wave
// then runs only the middle-layer segments its own queries have
constexpr int kGroupHeights = 4;
// The sort key is roots_kernel's straight-line-angle bucket, b = floor((thR - 90) * B / 90) with
// thR = 180 - atan(x) deg, x = D / (H - ice - depth), evaluated without the atan: b >= j exactly
// when x <= tan(90 deg * (1 - j / B)), so b counts the host-computed thresholds x lies below.
// (The key only orders the work; results do not depend on it.)
struct GroupKey {
  double t[kGroupAngles];  // t[j - 1] = tan(90 deg * (1 - j / B)), j = 1 .. B-1
};

template <int IN>
__device__ __forceinline__ int query_bucket(const DevMedium& M, const QueryArgs& Q, long long k,
                                            const GroupKey& K) {
  double thR_unused;
  const Geometry g = load_query<IN>(M, Q, k, thR_unused);
  const double den = g.H - g.ice - g.depth;
  int b = 0;
  if (!(den > 0)) {
    b = den < 0 ? kGroupAngles - 1 : 0;  // thR > 180 (clamped) / 90 or NaN
  } else {
#pragma unroll
    for (int j = 0; j < kGroupAngles - 1; ++j) b += (g.D <= K.t[j] * den) ? 1 : 0;
  }
  const int span = top_layer(M, g.H) - bottom_layer(M, g.ice);
  return b * kGroupHeights + (span < 0 ? 0 : (span > 3 ? 3 : span));
}

template <int IN>
__global__ __launch_bounds__(kRootsBlock, kRootsWaves) void roots_kernel(DevMedium M, IceConsts I,
                                                                         QueryArgs Q, Park park) {
  static_assert(solves_every_lane(IN), "IN_CM100 lanes are masked: use lookup_kernel");
  __shared__ int s_count[kSortBuckets + 1];
  __shared__ int s_slot[kRootsBlock];
  __shared__ double s_q[6][kRootsBlock];  // the sorted queries' geometry and straight-line angle
  const long long k0 = (long long)blockIdx.x * kRootsBlock;
  const long long kt = k0 + threadIdx.x;
  // the log table in LDS (one 16-byte entry per thread), as in table_kernel: every evaluation's
  // log ratios read it instead of global memory
  __shared__ __align__(16) double s_logtab[1 << kLogTableBits][2];
  for (unsigned t = threadIdx.x; t < (1u << kLogTableBits); t += kRootsBlock) {
    s_logtab[t][0] = kLogTable[t][0];
    s_logtab[t][1] = kLogTable[t][1];
  }
  if (threadIdx.x <= kSortBuckets) s_count[threadIdx.x] = 0;
  // the batch's ice end, once per block (IN_TRACE queries carry their own ice height)
  __shared__ IceAirPre s_ice;
  constexpr bool kIcePre = IN != IN_TRACE;
  if (kIcePre && threadIdx.x == 0) {
    const double ice = IN == IN_M ? Q.ice : Q.ice / 100;  // load_query's ice before the shift
    s_ice.x = ice;
    s_ice.bot = bottom_layer(M, ice);
    s_ice.s = air_slim(M, ice, s_ice.n);
  }
  // bucket of this lane's own query (unused lanes last); its inputs are read while the log table
  // is staged
  int bucket = kSortBuckets;
  Geometry g0{};
  double thR0 = 0.0;
  if (kt < Q.n) {
    g0 = load_query<IN>(M, Q, kt, thR0);
    const double b = (thR0 - 90.0) * (kSortBuckets / 90.0);
    bucket = (b >= 0.0 && b < kSortBuckets) ? (int)b : ((b >= kSortBuckets) ? kSortBuckets - 1 : 0);
  }
  __syncthreads();
  const int rank = atomicAdd(&s_count[bucket], 1);
  __syncthreads();
  // the first slot of the lane's bucket: the sizes of the buckets below it (independent LDS reads)
  int slot = rank;
#pragma unroll
  for (int b = 0; b < kSortBuckets; ++b) slot += b < bucket ? s_count[b] : 0;
  // the query moves to its slot through LDS: index, geometry and angle (no second global read)
  s_slot[slot] = threadIdx.x;
  s_q[0][slot] = g0.H;
  s_q[1][slot] = g0.D;
  s_q[2][slot] = g0.ice;
  s_q[3][slot] = g0.depth;
  s_q[4][slot] = g0.depth_pos;
  s_q[5][slot] = thR0;
  __syncthreads();
  const long long k = k0 + s_slot[threadIdx.x];
  if (k >= Q.n) return;
  Geometry g;
  g.H = s_q[0][threadIdx.x];
  g.D = s_q[1][threadIdx.x];
  g.ice = s_q[2][threadIdx.x];
  g.depth = s_q[3][threadIdx.x];
  g.depth_pos = s_q[4][threadIdx.x];
  const double thR = s_q[5][threadIdx.x];
  const SolveResult r = solve_root(M, I, g, thR, park.exact != 0, &s_logtab[0][0],
                                   kIcePre ? &s_ice : nullptr);
  st_agent(park.root + k * park.stride, r.root);
  st_agent(park.status + k * park.stride, (double)r.status);
  if (park.stats != nullptr) {
    park.stats[3 * k] = r.n_eval;
    park.stats[3 * k + 1] = r.n_est;
    park.stats[3 * k + 2] = r.n_inside;
  }
}

// ---------------------------------------------------------------------------
// Batch-wide grouping (large batches).  roots_kernel above sorts inside each 1024-query block, so
// a CU -- which holds one such block at 128 VGPRs -- waits for the block's slowest wave before
// the next block can start.  Here the whole batch is first grouped by the same straight-line
// angle key (counting sort: keys + histogram, then a scatter), and roots_sorted_kernel solves the
// queries in that order in small blocks that the CU replaces independently.  Each query is still
// solved on its own and written by its index: results are identical either way.
// ---------------------------------------------------------------------------
constexpr int kGroupBuckets = kGroupAngles * kGroupHeights;
constexpr int kGroupItems = 2;  // queries per thread in the sort passes
constexpr int kGroupThreads = 1024;  // threads per block of the sort passes
constexpr int kGroupChunk = kGroupThreads * kGroupItems;  // queries per block and round
constexpr int kGroupBlocks = 512;                     // blocks of the sort passes (at most)
constexpr int kSortedBlock = 256;

// Pass 1: the key of every query and each block's bucket counts, bucket-major:
// cnt[b * nblocks + block] (no global atomics: thousands of blocks adding into a few counters
// serialise on them).  Both passes use at most kGroupBlocks blocks of kGroupThreads threads
// (8 waves/SIMD when the batch fills them), each block taking `rounds` chunks in turn.
template <int IN>
__global__ __launch_bounds__(kGroupThreads) void group_count_kernel(DevMedium M, QueryArgs Q,
                                                                    GroupKey K, int rounds,
                                                                    int8_t* __restrict__ key,
                                                                    int* __restrict__ cnt) {
  __shared__ int s_c[kGroupBuckets];
  if (threadIdx.x < kGroupBuckets) s_c[threadIdx.x] = 0;
  __syncthreads();
  for (int rr = 0; rr < rounds; ++rr) {
    const long long k0 = ((long long)blockIdx.x * rounds + rr) * kGroupChunk + threadIdx.x;
#pragma unroll
    for (int i = 0; i < kGroupItems; ++i) {
      const long long k = k0 + i * kGroupThreads;
      if (k < Q.n) {
        const int b = query_bucket<IN>(M, Q, k, K);
        key[k] = (int8_t)b;
        if (b >= 0) atomicAdd(&s_c[b], 1);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kGroupBuckets) cnt[threadIdx.x * gridDim.x + blockIdx.x] = s_c[threadIdx.x];
}

// Pass 2: perm[position] = query index, positions grouped by bucket.  Each block first derives
// its own first position per bucket from all blocks' counts (bucket b's earlier buckets in full,
// plus bucket b of the blocks before it): kLanesPerBucket lanes per bucket sum strided slices of
// cnt[] and a tree in LDS adds them up, so no separate scan pass is needed.  A block's queries
// of one bucket take consecutive positions.
static_assert(kGroupThreads % kGroupBuckets == 0, "lanes per bucket");
constexpr int kLanesPerBucket = kGroupThreads / kGroupBuckets;
static_assert((kLanesPerBucket & (kLanesPerBucket - 1)) == 0, "power-of-two lanes per bucket");
template <int IN>
__global__ __launch_bounds__(kGroupThreads) void group_scatter_kernel(
    QueryArgs Q, const int8_t* __restrict__ key, long long n, int rounds,
    const int* __restrict__ cnt, int* __restrict__ grouped, int* __restrict__ inv,
    QueryRec* __restrict__ recs) {
  __shared__ int s_tot[kGroupBuckets][kLanesPerBucket], s_pre[kGroupBuckets][kLanesPerBucket];
  __shared__ int s_base[kGroupBuckets];
  const int nb = gridDim.x, blk = blockIdx.x;
  // this block's first-round keys, loaded before the prefix work so their latency overlaps it
  int b0[kGroupItems];
  const long long kb = (long long)blk * rounds * kGroupChunk + threadIdx.x;
#pragma unroll
  for (int i = 0; i < kGroupItems; ++i)
    b0[i] = kb + i * kGroupThreads < n ? (int)key[kb + i * kGroupThreads] : -1;
  const int bb = threadIdx.x / kLanesPerBucket, l = threadIdx.x % kLanesPerBucket;
  {
    const int* c = cnt + (long long)bb * nb;
    int tot = 0, pre = 0;
#pragma unroll 4
    for (int j = l; j < nb; j += kLanesPerBucket) {
      const int v = c[j];
      tot += v;
      pre += j < blk ? v : 0;
    }
    s_tot[bb][l] = tot;
    s_pre[bb][l] = pre;
  }
  __syncthreads();
#pragma unroll
  for (int h = kLanesPerBucket / 2; h > 0; h >>= 1) {
    if (l < h) {
      s_tot[bb][l] += s_tot[bb][l + h];
      s_pre[bb][l] += s_pre[bb][l + h];
    }
    __syncthreads();
  }
  if (threadIdx.x < kGroupBuckets) {
    int base = s_pre[threadIdx.x][0];
    for (int b = 0; b < (int)threadIdx.x; ++b) base += s_tot[b][0];
    s_base[threadIdx.x] = base;
    if (blk == 0 && threadIdx.x == kGroupBuckets - 1)  // number of queries with a bucket
      *grouped = base + s_tot[kGroupBuckets - 1][0];
  }
  __syncthreads();
  for (int rr = 0; rr < rounds; ++rr) {
    const long long k0 = ((long long)blk * rounds + rr) * kGroupChunk + threadIdx.x;
#pragma unroll
    for (int i = 0; i < kGroupItems; ++i) {
      const long long k = k0 + i * kGroupThreads;
      const int b = rr == 0 ? b0[i] : (k < n ? (int)key[k] : -1);
      if (b >= 0) {
        // the query's inputs move to its sorted position (one 32-byte record), so the root finder
        // reads them contiguously; inv[k] tells stage 2 where the query's result is parked
        const int pos = atomicAdd(&s_base[b], 1);
        const bool has_d = IN == IN_TRACE || (IN == IN_M && Q.d != nullptr);
        recs[pos] = QueryRec{Q.a[k], Q.b[k], Q.c[k], has_d ? Q.d[k] : 0.0};
        inv[k] = pos;
      }
    }
  }
}

template <int IN>
__global__ __launch_bounds__(kSortedBlock, kRootsWaves) void roots_sorted_kernel(
    DevMedium M, IceConsts I, QueryArgs Q, Park park, const QueryRec* __restrict__ recs,
    double2* __restrict__ sorted_park, const int* __restrict__ grouped) {
  __shared__ __align__(16) double s_logtab[1 << kLogTableBits][2];
  for (int t = threadIdx.x; t < (1 << kLogTableBits); t += kSortedBlock) {
    s_logtab[t][0] = kLogTable[t][0];
    s_logtab[t][1] = kLogTable[t][1];
  }
  __syncthreads();
  const long long ks = (long long)blockIdx.x * kSortedBlock + threadIdx.x;
  static_assert(solves_every_lane(IN), "IN_CM100 lanes are masked: use lookup_kernel");
  if (ks >= *grouped) return;  // past the queries with a bucket
  double thR;
  const Geometry g = load_rec<IN>(M, Q, recs[ks], thR);
  const SolveResult r = solve_root(M, I, g, thR, park.exact != 0, &s_logtab[0][0]);
  sorted_park[ks] = make_double2(r.root, (double)r.status);
}

// The stage-2 kernels read the log table from LDS like the solve.
__device__ __forceinline__ void stage_log_table(double (*s)[2]) {
  for (unsigned t = threadIdx.x; t < (1u << kLogTableBits); t += kBlock) {
    s[t][0] = kLogTable[t][0];
    s[t][1] = kLogTable[t][1];
  }
  __syncthreads();
}

// Where stage 1 of entry point OUT parks, as its launcher passes it to the stage-1 kernels.
template <int OUT>
static Park park_of(double* out, size_t ld) {
  using E = EntryPoint<OUT>;
  // (the stride: from query 0's slot to query 1's)
  return Park{E::root(out, ld, 0), E::status(out, ld, 0), E::root(out, ld, 1) - E::root(out, ld, 0),
              bisect_exact(), nullptr};
}

// The batch stage-2 kernels: one query per lane, the log table read from LDS like the solve.
template <int OUT>
__device__ __forceinline__ void out_block(const DevMedium& M, const IceConsts& I,
                                          const QueryArgs& Q, double* __restrict__ out, size_t ld,
                                          uint8_t* __restrict__ flag, const SortedPark& sp) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  __shared__ __align__(16) double s_logtab[1 << kLogTableBits][2];
  stage_log_table(s_logtab);
  if (k >= Q.n) return;
  stage2_out<OUT, AT_PARKED>(M, I, Q, out, ld, flag, k, &s_logtab[0][0], WaveRoot{0.0, 0}, sp);
}

// occupancy of the stage-2 kernel: the compiler's choice (104 VGPRs, 4 waves/SIMD; held to 5-6
// waves it takes 80 VGPRs and runs within noise, at 8 it spills and runs slower: round 6)
template <int VARIANT>
__global__ __launch_bounds__(kBlock, kOutWaves) void solve_out_kernel(DevMedium M, IceConsts I, QueryArgs Q,
                                                           double* __restrict__ out, size_t ld,
                                                           uint8_t* __restrict__ status,
                                                           SortedPark sp) {
  out_block<VARIANT == AIRICE_VARIANT_MULTIRAY ? OUT_SOLVE_MR : OUT_SOLVE_PY>(M, I, Q, out, ld,
                                                                              status, sp);
}

__global__ __launch_bounds__(kBlock, kOutWaves) void hdtip_out_kernel(DevMedium M, IceConsts I, QueryArgs Q,
                                                           double* __restrict__ out, size_t ld,
                                                           uint8_t* __restrict__ ok, SortedPark sp) {
  out_block<OUT_HDTIP>(M, I, Q, out, ld, ok, sp);
}

__global__ __launch_bounds__(kBlock, kTraceOutWaves) void trace_out_kernel(DevMedium M, IceConsts I, QueryArgs Q,
                                                           double* __restrict__ out10,
                                                           SortedPark sp) {
  out_block<OUT_TRACE>(M, I, Q, out10, 0, nullptr, sp);
}

// One query, both stages in one launch (the scalar C++ / ctypes entry points): one wave finds the
// root with the evaluation spread over its lanes, then runs stage 2 of the entry point (OUT) with
// its evaluation spread the same way.  Bit-identical to the two batch kernels.
// (IN is EntryPoint<OUT>::in; of park only the exact flag is used: the root goes to stage 2
// directly)
template <int IN, int OUT>
__global__ __launch_bounds__(64) void scalar_solve_kernel(DevMedium M, IceConsts I, QueryArgs Q,
                                                          Park park, double* out, size_t ld,
                                                          uint8_t* flag, Signal sig) {
  static_assert(IN == EntryPoint<OUT>::in, "the entry point fixes its query source");
  prefetch_kernargs<sizeof(DevMedium) + sizeof(IceConsts)>();
  // one wave and a handful of logarithms per evaluation: the log table is read from global
  // memory (L1 / L2 after the first call) instead of being staged in LDS first
  const double* tab = &kLogTable[0][0];
  if (IN == IN_CM100 && !(Q.mask[0] & AIRICE_LOOKUP_FALLBACK)) {
    if (threadIdx.x == 0) signal_done(sig);
    return;
  }
  double thR;
  const Geometry g = load_query<IN>(M, Q, 0, thR,
                                    sig.n_in >= ((IN == IN_TRACE || (IN == IN_M && Q.d != nullptr)) ? 4 : 3)
                                        ? &sig
                                        : nullptr);
  const SolveResult r = solve_root<true>(M, I, g, thR, park.exact != 0, tab);
  // every lane runs stage 2 (its evaluation spread over the wave); lane 0 writes
  stage2_out<OUT, AT_WAVE>(M, I, Q, out, ld, flag, 0, tab, WaveRoot{r.root, r.status, g});
  if (threadIdx.x != 0) return;
  signal_done(sig);
}

// One query of a minimizer entry point on the host (AIRICE_SCALAR_HOST, the default of the
// one-query C++ / ctypes drop-ins): the root finder and stage 2 compiled for the CPU from the same
// source as the batch kernels (the host's correctly rounded sqrt and quotients in place of the
// device iterations).  The root is the GSL bisection's, decided by the signs of f at its
// midpoints, so it is the device's; the outputs at it agree to an ulp or so.
// Q: the query at index 0 (host pointers); out, ld, flag: as the entry point's launcher takes them.
template <int OUT>
static int solve_one_host_t(const DevMedium& M, const IceConsts& I, const QueryArgs& Q,
                            double* out, size_t ld, uint8_t* flag) {
  constexpr int IN = EntryPoint<OUT>::in;
  const double* tab = &kLogTable[0][0];
  if (IN == IN_CM100 && !(Q.mask[0] & AIRICE_LOOKUP_FALLBACK)) return AIRICE_OK;
  double thR;
  const Geometry g = load_query<IN>(M, Q, 0, thR);
  const SolveResult r = solve_root<false>(M, I, g, thR, bisect_exact() != 0, tab);
  stage2_out<OUT, AT_DIRECT>(M, I, Q, out, ld, flag, 0, tab, WaveRoot{r.root, r.status, g});
  return AIRICE_OK;
}

// Air2IceRayTracing, one query (in: txh, dist, depth [, straight angle]): out17 / out15 with
// ld = 1, status bits.
int solve_host_one(const DevMedium& M, const IceConsts& I, int variant, const double* in,
                   bool has_thr, double* out, uint8_t* status) {
  const QueryArgs Q{in, in + 1, in + 2, has_thr ? in + 3 : nullptr, I.ice_h, 1};
  return variant == AIRICE_VARIANT_PYWRAPPER
             ? solve_one_host_t<OUT_SOLVE_PY>(M, I, Q, out, 1, status)
             : solve_one_host_t<OUT_SOLVE_MR>(M, I, Q, out, 1, status);
}

// GetHorizontalDistanceToIntersectionPoint, one query (in: src, dist, depth in cm).
int hdtip_host_one(const DevMedium& M, const IceConsts& I, double ice_cm, const double* in,
                   double* out9, uint8_t* ok) {
  return solve_one_host_t<OUT_HDTIP>(M, I, QueryArgs{in, in + 1, in + 2, nullptr, ice_cm, 1}, out9,
                                     1, ok);
}

// TraceIceToAir, one query (in: depth, ice, txh, dist).
int trace_host_one(const DevMedium& M, const IceConsts& I, const double* in, double* out10) {
  return solve_one_host_t<OUT_TRACE>(M, I, QueryArgs{in, in + 1, in + 2, in + 3, 0.0, 1}, out10, 0,
                                     nullptr);
}

// The table lookup's minimizer fallback for one flagged query (in: src, dist, depth in cm; ok and
// flags as the lookup left them).
int lookup_fallback_host_one(const DevMedium& M, const IceConsts& I, double ice_cm,
                             const double* in, double* out9, uint8_t* ok, const uint8_t* flags) {
  const QueryArgs Q{in, in + 1, in + 2, nullptr, fallback_ice_arg(ice_cm), 1, flags};
  return solve_one_host_t<OUT_FALLBACK>(M, I, Q, out9, 1, ok);
}

// ---------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------
static inline dim3 roots_grid(size_t n) {
  return dim3((unsigned)((n + kRootsBlock - 1) / kRootsBlock));
}

// Stream-ordered scratch for the grouping passes: a library-owned pool per device whose release
// threshold keeps freed blocks for reuse (the default pool returns them at every synchronisation,
// and re-growing it made each launch wait on the host).
hipError_t scratch_alloc(void** p, size_t bytes, hipStream_t st) {
  static std::mutex mu;
  static std::vector<hipMemPool_t> pools;
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev)) return e;
  hipMemPool_t pool = nullptr;
  {
    std::lock_guard<std::mutex> lock(mu);
    if ((int)pools.size() <= dev) pools.resize(dev + 1, nullptr);
    if (pools[dev] == nullptr) {
      hipMemPoolProps props{};
      props.allocType = hipMemAllocationTypePinned;
      props.location.type = hipMemLocationTypeDevice;
      props.location.id = dev;
      if (hipError_t e = hipMemPoolCreate(&pools[dev], &props)) return e;
      uint64_t keep = UINT64_MAX;
      (void)hipMemPoolSetAttribute(pools[dev], hipMemPoolAttrReleaseThreshold, &keep);
    }
    pool = pools[dev];
  }
  return hipMallocFromPoolAsync(p, bytes, pool, st);
}

static const GroupKey& group_thresholds() {
  static const GroupKey K = [] {
    GroupKey k{};
    for (int j = 1; j < kGroupAngles; ++j)
      k.t[j - 1] = tan(M_PI / 2 * (1.0 - (double)j / kGroupAngles));
    return k;
  }();
  return K;
}

// Measured with the slope-placed guards (round 4): cfg3 (IN_M, 1e6) 0.241 ms per call
// block-local against 0.276 ms grouped -- four to five evaluations per query leave the 1,024-query
// blocks' angle sort as good as the batch-wide one, and the grouping passes and the stage-2 gather
// cost more -- while cfg5 (IN_TRACE, 1e7, Tx up to 20 km, per-query ice) takes 2.23 ms grouped
// against 2.53 block-local.  So the batch-wide grouping is the default of the trace source only;
// AIRICE_GROUP_MIN overrides it for every source (0: never group).
size_t group_min_batch(int in) {
  static const char* env = getenv("AIRICE_GROUP_MIN");
  static const long long v = env ? atoll(env) : -1;
  if (v >= 0) return (size_t)v;
  return in == IN_TRACE ? (size_t)kGroupMin : 0;
}

// Stage 1 of every minimizer launch: roots_kernel (block-local grouping) for small batches and
// debug statistics, the batch-wide grouping otherwise (stream-ordered scratch, scratch_alloc).
// A grouped launch returns the sorted parking (sp) its stage-2 kernel reads, and the scratch
// block (ws) to release after that kernel (RootsScratch).
template <int IN>
static int launch_roots(const DevMedium& M, const IceConsts& I, const QueryArgs& Q,
                        const Park& park, size_t n, hipStream_t st, SortedPark& sp, void*& ws) {
  static_assert(solves_every_lane(IN), "IN_CM100 lanes are masked: use launch_lookup_fallback");
  sp = SortedPark{nullptr, nullptr};
  ws = nullptr;
  const size_t group_min = group_min_batch(IN);
  if (group_min == 0 || n < group_min ||
      park.stats != nullptr || n >= (1ull << 31)) {
    return bracket_launch(LC_ROOTS, KT_ROOTS, st, [&] {
      hipLaunchKernelGGL((roots_kernel<IN>), roots_grid(n), dim3(kRootsBlock), 0, st, M, I, Q, park);
    });
  }
  const GroupKey& thresholds = group_thresholds();
  // at most kGroupBlocks blocks in the two passes (each scatter block reads every block's
  // counts); larger batches give each block several chunks
  const size_t chunks = (n + kGroupChunk - 1) / kGroupChunk;
  const int rounds = (int)((chunks + kGroupBlocks - 1) / kGroupBlocks);
  const unsigned nb = (unsigned)((chunks + rounds - 1) / rounds);
  const size_t m = (size_t)kGroupBuckets * nb;
  // scratch: sorted query records (32 B), sorted (root, status) (16 B), inv (4 B) and key (1 B)
  // per query, then the bucket counts and the grouped count
  const size_t ws_bytes = (sizeof(QueryRec) + sizeof(double2) + sizeof(int) + 1) * n +
                          sizeof(int) * (m + 1);
  if (scratch_alloc(&ws, ws_bytes, st) != hipSuccess) return AIRICE_EHIP;
  QueryRec* recs = static_cast<QueryRec*>(ws);
  double2* sorted = reinterpret_cast<double2*>(recs + n);
  int* inv = reinterpret_cast<int*>(sorted + n);
  int* cnt = inv + n;
  int* grouped = cnt + m;
  int8_t* key = reinterpret_cast<int8_t*>(grouped + 1);
  ktimer_begin(KT_GROUP, st);
  hipLaunchKernelGGL(group_count_kernel<IN>, dim3(nb), dim3(kGroupThreads), 0, st, M, Q,
                     thresholds, rounds, key, cnt);
  hipLaunchKernelGGL(group_scatter_kernel<IN>, dim3(nb), dim3(kGroupThreads), 0, st, Q, key,
                     (long long)n, rounds, cnt, grouped, inv, recs);
  ktimer_end(KT_GROUP, st);
  const unsigned sorted_blocks = (unsigned)((n + kSortedBlock - 1) / kSortedBlock);
  ktimer_begin(KT_ROOTS, st);
  count_launch(LC_ROOTS);
  hipLaunchKernelGGL(roots_sorted_kernel<IN>, dim3(sorted_blocks), dim3(kSortedBlock), 0, st, M, I,
                     Q, park, recs, sorted, grouped);
  ktimer_end(KT_ROOTS, st);
  sp = SortedPark{sorted, inv};
  return launch_ok();
}

// A grouped launch's scratch block, released stream-ordered after its stage-2 kernel
// (release()), or on any early return by the destructor.
struct RootsScratch {
  void* ws = nullptr;
  hipStream_t st;
  explicit RootsScratch(hipStream_t s) : st(s) {}
  RootsScratch(const RootsScratch&) = delete;
  RootsScratch& operator=(const RootsScratch&) = delete;
  ~RootsScratch() {
    if (ws != nullptr) (void)hipFreeAsync(ws, st);
  }
  int release() {
    void* p = ws;
    ws = nullptr;
    if (p != nullptr && hipFreeAsync(p, st) != hipSuccess) return AIRICE_EHIP;
    return AIRICE_OK;
  }
};

// One query of entry point OUT on the device: scalar_solve_kernel, which takes the armed signal
// of a one-query call (take_scalar_signal).
template <int OUT>
static int launch_one_wave(const DevMedium& M, const IceConsts& I, const QueryArgs& Q,
                           const Park& park, double* out, size_t ld, uint8_t* flag,
                           hipStream_t st) {
  return bracket_launch(LC_SCALAR_SOLVE, kNoTimer, st, [&] {
    hipLaunchKernelGGL((scalar_solve_kernel<EntryPoint<OUT>::in, OUT>), dim3(1), dim3(64), 0, st, M,
                       I, Q, park, out, ld, flag, take_scalar_signal());
  });
}

// A minimizer launch of entry point OUT on one stream.  One query takes the one-wave kernel
// (never a statistics run: its counts come from roots_kernel).  A batch takes the two stages:
// launch_roots, then between() (launch_solve's statistics dump; non-zero ends the launch), then
// the stage-2 kernel, which stage2(grid, block, sp) enqueues, and the release of a grouped
// launch's scratch behind it.
template <int OUT, class Stage2, class Between>
static int launch_entry(const DevMedium& M, const IceConsts& I, const QueryArgs& Q,
                        const Park& park, double* out, size_t ld, uint8_t* flag, hipStream_t st,
                        Stage2 stage2, Between between) {
  if (Q.n == 1 && park.stats == nullptr)
    return launch_one_wave<OUT>(M, I, Q, park, out, ld, flag, st);
  SortedPark sp;
  RootsScratch scr(st);
  if (int rc = launch_roots<EntryPoint<OUT>::in>(M, I, Q, park, (size_t)Q.n, st, sp, scr.ws))
    return rc;
  if (int rc = between()) return rc;
  const int rc = bracket_launch(LC_OUT, KT_OUT, st,
                                [&] { stage2(dim3(grid_for(Q.n)), dim3(kBlock), sp); });
  if (int rf = scr.release()) return rf;
  return rc;
}
static int no_hook() { return AIRICE_OK; }  // between(), for the launchers without one

int launch_solve(const DevMedium& M, const IceConsts& I, int variant, const double* txh,
                 const double* dist, const double* depth, const double* thr, size_t n,
                 double* out, size_t ld, uint8_t* status, hipStream_t st) {
  if (n == 0) return AIRICE_OK;
  const QueryArgs Q{txh, dist, depth, thr, I.ice_h, (long long)n};
  Park park = park_of<OUT_SOLVE_MR>(out, ld);  // (both variants park alike)
  static const char* stats_path = getenv("AIRICE_SOLVE_STATS");
  if (stats_path != nullptr && hipMalloc(&park.stats, sizeof(int) * kStatsInts * n) != hipSuccess)
    return AIRICE_EHIP;
  auto dump_stats = [&] {  // debug: append the per-query counts (synchronous)
    if (park.stats == nullptr) return AIRICE_OK;
    std::vector<int> h(kStatsInts * n);
    if (hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpy(h.data(), park.stats, sizeof(int) * kStatsInts * n, hipMemcpyDeviceToHost) != hipSuccess)
      return AIRICE_EHIP;
    (void)hipFree(park.stats);
    if (FILE* f = fopen(stats_path, "ab")) {
      fwrite(h.data(), sizeof(int), kStatsInts * n, f);
      fclose(f);
    }
    return AIRICE_OK;
  };
  const bool mr = variant == AIRICE_VARIANT_MULTIRAY;
  auto kernel = mr ? solve_out_kernel<AIRICE_VARIANT_MULTIRAY>
                   : solve_out_kernel<AIRICE_VARIANT_PYWRAPPER>;
  auto stage2 = [&](dim3 grid, dim3 block, const SortedPark& sp) {
    hipLaunchKernelGGL(kernel, grid, block, 0, st, M, I, Q, out, ld, status, sp);
  };
  return mr ? launch_entry<OUT_SOLVE_MR>(M, I, Q, park, out, ld, status, st, stage2, dump_stats)
            : launch_entry<OUT_SOLVE_PY>(M, I, Q, park, out, ld, status, st, stage2, dump_stats);
}

int launch_hdtip(const DevMedium& M, const IceConsts& I, const double* src, const double* dist,
                 const double* depth, double ice_cm, size_t n, double* out, size_t ld,
                 uint8_t* ok, hipStream_t st) {
  if (n == 0) return AIRICE_OK;
  const QueryArgs Q{src, dist, depth, nullptr, ice_cm, (long long)n};
  return launch_entry<OUT_HDTIP>(
      M, I, Q, park_of<OUT_HDTIP>(out, ld), out, ld, ok, st,
      [&](dim3 grid, dim3 block, const SortedPark& sp) {
        hipLaunchKernelGGL(hdtip_out_kernel, grid, block, 0, st, M, I, Q, out, ld, ok, sp);
      },
      no_hook);
}

// The table lookup's minimizer fallback for one query (the one-query device call; a batch solves
// its fallback lanes inside lookup_kernel).
int launch_lookup_fallback(const DevMedium& M, const IceConsts& I, const double* src,
                           const double* dist, const double* depth, double ice_cm, double* out,
                           size_t ld, uint8_t* ok, const uint8_t* flags, hipStream_t st) {
  const QueryArgs Q{src, dist, depth, nullptr, fallback_ice_arg(ice_cm), 1, flags};
  return launch_one_wave<OUT_FALLBACK>(M, I, Q, park_of<OUT_FALLBACK>(out, ld), out, ld, ok, st);
}

int launch_trace(const DevMedium& M, const IceConsts& I, const double* depth, const double* ice,
                 const double* txh, const double* dist, size_t n, double* out10, hipStream_t st) {
  if (n == 0) return AIRICE_OK;
  const QueryArgs Q{depth, ice, txh, dist, 0.0, (long long)n};
  return launch_entry<OUT_TRACE>(
      M, I, Q, park_of<OUT_TRACE>(out10, 0), out10, 0, nullptr, st,
      [&](dim3 grid, dim3 block, const SortedPark& sp) {
        hipLaunchKernelGGL(trace_out_kernel, grid, block, 0, st, M, I, Q, out10, sp);
      },
      no_hook);
}

// GetHorizontalDistanceToIntersectionPoint_Table (.cc:1305-1462) for a batch, one query per lane:
// lk_query (airice_lookup.hpp: row records, the THD window in LDS, pair records), and a lane whose
// query hits the one-sided case runs the reference's minimizer fallback (.cc:1418-1420: the root
// finder and its stage 2 with the root in registers) in place while the other waves go on with
// their lookups.  (Round 5: a separate fallback pass after the lookup launch -- 4,096-query
// chunks, flagged lanes listed in LDS -- waited for the whole launch and then for one solve's
// latency: 100.8-101.8 against 93.1-93.5 us per 1e6 random queries, same outputs.)
// 128 VGPRs (the root finder's cap, 4 waves/SIMD as the lookup alone at 97).
// One lane's query of the two lookup kernels.  Q: the lane's own source height, distance and Rx
// depth at index 0 (cm), Q.ice the fallback's ice argument; k: the query's slot in out / ok /
// flags; win: the lane's column of the block's LDS window.
__device__ __forceinline__ void lookup_lane(LkTable T, const DevMedium& M, const IceConsts& I,
                                            const QueryArgs& Q, double* __restrict__ out,
                                            size_t ld, uint8_t* __restrict__ ok,
                                            uint8_t* __restrict__ flags, long long k, int exact,
                                            float* win) {
  if (T.ang != nullptr && *reinterpret_cast<const int*>(T.ang + (lk_angles_ok_offset(T.n, T.asteps) -
                                                                  lk_angles_offset(T.n, T.asteps))) == 0)
    T.ang = nullptr;
  int fl = 0;
  double o[9];
  bool good = false;
  const bool fb = lk_query(T, Q.a[0] / 100, Q.b[0] / 100, M.d2r, o, &good, fl, win);
  if (!fb) {
#pragma unroll
    for (int c = 0; c < 9; ++c) __builtin_nontemporal_store(o[c], out + c * ld + k);
  }
  ok[k] = good ? 1 : 0;
  flags[k] = (uint8_t)fl;
  if (fb) {
    double thR;
    const Geometry g = load_query<IN_CM100>(M, Q, 0, thR);
    const SolveResult r = solve_root(M, I, g, thR, exact != 0, &kLogTable[0][0]);
    stage2_out<OUT_FALLBACK, AT_DIRECT>(M, I, Q, out, ld, ok, k, &kLogTable[0][0],
                                        WaveRoot{r.root, r.status, g});
  }
}

__global__ __launch_bounds__(kLkBlock, kRootsWaves) void lookup_kernel(
    LkTable T, DevMedium M, IceConsts I, QueryArgs Q, double* __restrict__ out, size_t ld,
    uint8_t* __restrict__ ok, uint8_t* __restrict__ flags, int exact) {
  const long long k = (long long)blockIdx.x * kLkBlock + threadIdx.x;
  if (k >= Q.n) return;
  __shared__ float s_win[kLkWindow][kLkBlock];
  const QueryArgs q{Q.a + k, Q.b + k, Q.c + k, nullptr, Q.ice, 1, nullptr};
  lookup_lane(T, M, I, q, out, ld, ok, flags, k, exact, &s_win[0][threadIdx.x]);
}

// The same lookup for n_ant antennas x n_src sources in one launch: every lane of a block works
// for one antenna (blockIdx.y, .z), so the antenna's record and its table's description are
// block-uniform and come through scalar loads from the workspace the launcher filled (tabs: the
// distinct tables, ants: each antenna's table and Rx depth).  Lane i of antenna a reads src[i] and
// dist[a * ld_dist + i] and writes slot a * n_src + i: lookup_lane, the bits of one lookup_kernel
// launch per antenna.
struct LkAntenna {
  double depth_cm;
  int table;
  int pad_;
};
// LkTable as the kernel reads it from the workspace: the same layout with the pointers typed as
// global memory.  (A pointer that is read from memory is generic to the compiler -- flat loads,
// which wait on the LDS counter too; typed like this the gathers are global loads as in
// lookup_kernel, whose pointers are kernel arguments.)
typedef const __attribute__((address_space(1))) float* LkGlobalPtr;
struct LkTableDev {
  LkGlobalPtr col[AIRICE_TABLE_COLUMNS];
  LkGlobalPtr e;
  long long n;
  double stop_h, step_h;
  int hsteps, asteps;
  long long rows;
  LkGlobalPtr ang;
};
static_assert(sizeof(LkTableDev) == sizeof(LkTable) &&
                  offsetof(LkTableDev, ang) == offsetof(LkTable, ang) &&
                  offsetof(LkTableDev, n) == offsetof(LkTable, n),
              "the launcher uploads LkTable images");

__global__ __launch_bounds__(kLkBlock, kRootsWaves) void lookup_multi_kernel(
    const LkTableDev* __restrict__ tabs, const LkAntenna* __restrict__ ants, int n_ant, DevMedium M,
    IceConsts I, const double* __restrict__ src, const double* __restrict__ dist, size_t ld_dist,
    double ice, long long n_src, double* __restrict__ out, size_t ld, uint8_t* __restrict__ ok,
    uint8_t* __restrict__ flags, int exact) {
  const long long a = (long long)blockIdx.z * gridDim.y + blockIdx.y;
  const long long i = (long long)blockIdx.x * kLkBlock + threadIdx.x;
  if (a >= n_ant || i >= n_src) return;
  const LkAntenna* A = ants + a;
  __shared__ float s_win[kLkWindow][kLkBlock];
  const QueryArgs q{src + i, dist + a * ld_dist + i, &A->depth_cm, nullptr, ice, 1, nullptr};
  const LkTableDev* Tp = tabs + A->table;
  LkTable T;
#pragma unroll
  for (int c = 0; c < AIRICE_TABLE_COLUMNS; ++c) T.col[c] = (const float*)Tp->col[c];
  T.e = (const float*)Tp->e;
  T.n = Tp->n;
  T.stop_h = Tp->stop_h;
  T.step_h = Tp->step_h;
  T.hsteps = Tp->hsteps;
  T.asteps = Tp->asteps;
  T.rows = Tp->rows;
  T.ang = (const float*)Tp->ang;
  lookup_lane(T, M, I, q, out, ld, ok, flags, a * n_src + i, exact,
              &s_win[0][threadIdx.x]);
}

int launch_lookup(const DevMedium& M, const IceConsts& I, const airice_lookup_table* t,
                  const double* src, const double* dist, const double* depth, double ice_cm,
                  size_t n, double* out, size_t ld, uint8_t* ok, uint8_t* flags, hipStream_t st) {
  if (n == 0) return AIRICE_OK;
  const LkTable T = lk_table(t);
  const QueryArgs Q{src, dist, depth, nullptr, fallback_ice_arg(ice_cm), (long long)n, flags};
  const unsigned grid = (unsigned)((n + kLkBlock - 1) / kLkBlock);
  return bracket_launch(LC_LOOKUP, KT_LOOKUP, st, [&] {
    hipLaunchKernelGGL(lookup_kernel, dim3(grid), dim3(kLkBlock), 0, st, T, M, I, Q, out, ld, ok,
                       flags, bisect_exact());
  });
}

size_t lookup_multi_work_bytes(size_t n_tables, size_t n_ant) {
  return (n_tables * sizeof(LkTable) + n_ant * sizeof(LkAntenna) + 15) / 16 * 16;
}

int launch_lookup_multi(const DevMedium& M, const IceConsts& I, const airice_lookup_table* tables,
                        int n_tables, const int32_t* antenna_table, const double* antenna_depth_cm,
                        size_t n_ant, const double* src, const double* dist, size_t ld_dist,
                        double ice_cm, size_t n_src, double* out, size_t ld, uint8_t* ok,
                        uint8_t* flags, void* d_work, hipStream_t st) {
  if (n_ant == 0 || n_src == 0) return AIRICE_OK;
  // the staging image of the workspace: the tables' descriptions, then the antennas' records
  const size_t tab_bytes = (size_t)n_tables * sizeof(LkTable);
  std::vector<char> img(tab_bytes + n_ant * sizeof(LkAntenna));
  LkTable* ht = reinterpret_cast<LkTable*>(img.data());
  LkAntenna* ha = reinterpret_cast<LkAntenna*>(img.data() + tab_bytes);
  for (int t = 0; t < n_tables; ++t) ht[t] = lk_table(tables + t);
  for (size_t a = 0; a < n_ant; ++a) ha[a] = LkAntenna{antenna_depth_cm[a], antenna_table[a], 0};
  // (a copy from pageable memory returns once the source has been read)
  if (hipError_t e = hipMemcpyAsync(d_work, img.data(), img.size(), hipMemcpyHostToDevice, st)) {
    set_error("lookup multi: workspace upload failed: %s", hipGetErrorString(e));
    return AIRICE_EHIP;
  }
  const LkTableDev* d_tabs = static_cast<const LkTableDev*>(d_work);
  const LkAntenna* d_ants =
      reinterpret_cast<const LkAntenna*>(static_cast<const char*>(d_work) + tab_bytes);
  constexpr size_t kMaxY = 65535;
  const unsigned gy = (unsigned)(n_ant < kMaxY ? n_ant : kMaxY);
  const dim3 grid((unsigned)((n_src + kLkBlock - 1) / kLkBlock), gy,
                  (unsigned)((n_ant + gy - 1) / gy));
  return bracket_launch(LC_LOOKUP_MULTI, KT_LOOKUP_MULTI, st, [&] {
    hipLaunchKernelGGL(lookup_multi_kernel, grid, dim3(kLkBlock), 0, st, d_tabs, d_ants, (int)n_ant,
                       M, I, src, dist, ld_dist, fallback_ice_arg(ice_cm), (long long)n_src, out,
                       ld, ok, flags, bisect_exact());
  });
}
}  // namespace airice
