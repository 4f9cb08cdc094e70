// airice_runtime.cpp -- host runtime of libairice.so: GDAS atmosphere ingestion,
// medium/grid set-up, device bookkeeping and the C-ABI entry points (include/airice.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <fstream>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

#include "airice.h"
#include "airice_hostcall.hpp"
#include "airice_icefirst.hpp"
#include "airice_internal.h"

namespace airice {

// ---- one-query calls on the host ---------------------------------------------------------
// Where the one-query ray and ray-layer calls run (airice_scalar_mode): AIRICE_SCALAR_HOST (the
// default) or AIRICE_SCALAR_DEVICE (the one-wave kernels through the scalar slot); the environment
// variable AIRICE_SCALAR=device sets the initial mode.
static std::atomic<int> g_scalar_mode{-1};
int set_scalar_mode(int mode) {
  int prev = g_scalar_mode.load();
  if (prev < 0) prev = scalar_on_host() ? AIRICE_SCALAR_HOST : AIRICE_SCALAR_DEVICE;
  if (mode == AIRICE_SCALAR_HOST || mode == AIRICE_SCALAR_DEVICE) g_scalar_mode.store(mode);
  return prev;
}
bool scalar_on_host() {
  int v = g_scalar_mode.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("AIRICE_SCALAR");
    v = (e != nullptr && std::strcmp(e, "device") == 0) ? AIRICE_SCALAR_DEVICE : AIRICE_SCALAR_HOST;
    int expect = -1;
    g_scalar_mode.compare_exchange_strong(expect, v);
    v = g_scalar_mode.load();
  }
  return v == AIRICE_SCALAR_HOST;
}

// The host folds of the last medium (and ice height / antenna depth) a thread's one-query calls
// used: a repeated call with the same medium skips build_dev_medium / build_ice_consts (~20
// exponentials).  Keyed by the medium's bytes (the namespace data a drop-in call folds in).
namespace {
struct FoldCache {
  airice_medium key{};
  int variant = -1;
  DevMedium M{};
  bool have_i = false;
  double ice = 0, rx = 0;
  IceConsts I{};
};
thread_local FoldCache t_fold;
}  // namespace

int folded_medium(const airice_medium* m, int variant, const DevMedium** out) {
  if (m == nullptr) {  // as build_dev_medium: the C-ABI's error contract, not a crash
    set_error("null medium");
    return AIRICE_EINVAL;
  }
  FoldCache& c = t_fold;
  if (c.variant != variant || std::memcmp(&c.key, m, sizeof(*m)) != 0) {
    c.variant = -1;
    c.have_i = false;
    if (int rc = build_dev_medium(m, variant, &c.M)) return rc;
    c.key = *m;
    c.variant = variant;
  }
  *out = &c.M;
  return AIRICE_OK;
}

int folded_ice(const airice_medium* m, int variant, double ice_h, double rx_depth,
               const DevMedium** M, const IceConsts** I) {
  if (int rc = folded_medium(m, variant, M)) return rc;
  FoldCache& c = t_fold;
  if (!c.have_i || c.ice != ice_h || c.rx != rx_depth ||
      (std::signbit(c.ice) != std::signbit(ice_h)) || (std::signbit(c.rx) != std::signbit(rx_depth))) {
    build_ice_consts(c.M, ice_h, rx_depth, &c.I);
    c.ice = ice_h;
    c.rx = rx_depth;
    c.have_i = true;
  }
  *I = &c.I;
  return AIRICE_OK;
}

// ---- kernel timer (bench only) ---------------------------------------------------------
std::atomic<bool> g_ktimer_on{false};
static std::mutex g_kt_mu;
static constexpr size_t kKtMaxPairs = 1 << 16;  // closed pairs kept per kernel until a reset
struct KtPair {
  hipEvent_t a = nullptr, b = nullptr;
};
static std::vector<KtPair> g_kt_done[KT_COUNT];   // closed pairs
static KtPair g_kt_open[KT_COUNT];                // pair whose end is pending
static const char* const kKtNames[KT_COUNT] = {"table_kernel",      "roots_kernel",
                                               "group_passes",      "out_kernel",
                                               "lookup_kernel",     "ray_consts_kernel",
                                               "ray_paths_kernel",  "lookup_multi_kernel",
                                               "air2ice_kernel",    "iceray_kernel",
                                               "icesol_kernel",     "icetab_points_kernel",
                                               "icetab_pack_kernel", "icetab_lookup_kernel",
                                               "icepath_consts_kernel", "icepath_kernel",
                                               "icesol_spectrum_kernel", "iceair_kernel",
                                               "icefirst_geom_kernel",
                                               "icefirst_select_kernel"};
static_assert(sizeof(kKtNames) / sizeof(kKtNames[0]) == KT_COUNT, "one name per timer");

std::atomic<long long> g_launches[LC_COUNT];
static const char* const kLcNames[LC_COUNT] = {
    "table_kernel",        "rays_kernel",  "scalar_ray_kernel", "roots_kernel",
    "scalar_solve_kernel", "out_kernel",   "lookup_kernel",     "rtf_kernel",
    "single_ray_kernel",   "path_kernel",  "ray_consts_kernel", "ray_paths_kernel",
    "lookup_multi_kernel", "air2ice_kernel", "air_part_kernel", "iceray_kernel",
    "icesol_kernel", "icetab_points_kernel", "icetab_pack_kernel", "icetab_lookup_kernel",
    "icepath_consts_kernel", "icepath_kernel", "icesol_spectrum_kernel", "iceair_kernel",
    "icefirst_geom_kernel", "icefirst_select_kernel"};
static_assert(sizeof(kLcNames) / sizeof(kLcNames[0]) == LC_COUNT, "one name per counter");

// AIRICE_LAUNCH_REPORT=1: the counts go to stderr when the library unloads (the CLI tests read
// them from a child process).
namespace {
struct LaunchReport {
  ~LaunchReport() {
    const char* e = getenv("AIRICE_LAUNCH_REPORT");
    if (e == nullptr || *e == '\0' || *e == '0') return;
    fprintf(stderr, "airice launches:");
    for (int i = 0; i < LC_COUNT; ++i)
      fprintf(stderr, " %s=%lld", kLcNames[i], g_launches[i].load(std::memory_order_relaxed));
    fprintf(stderr, "\n");
  }
} g_launch_report;
}  // namespace

void ktimer_record(int id, bool begin, hipStream_t st) {
  std::lock_guard<std::mutex> lock(g_kt_mu);
  if (begin) {
    if (g_kt_open[id].a != nullptr) {  // a begin whose launch failed before its end: drop it
      (void)hipEventDestroy(g_kt_open[id].a);
      (void)hipEventDestroy(g_kt_open[id].b);
      g_kt_open[id] = KtPair();
    }
    if (g_kt_done[id].size() >= kKtMaxPairs) return;  // bounded: time no more until a reset
    KtPair p;
    if (hipEventCreate(&p.a) != hipSuccess) return;
    if (hipEventCreate(&p.b) != hipSuccess) {
      (void)hipEventDestroy(p.a);
      return;
    }
    (void)hipEventRecord(p.a, st);
    g_kt_open[id] = p;
  } else if (g_kt_open[id].a != nullptr) {
    (void)hipEventRecord(g_kt_open[id].b, st);
    g_kt_done[id].push_back(g_kt_open[id]);
    g_kt_open[id] = KtPair();
  }
}

// ---- scalar slots ------------------------------------------------------------------------
namespace {
struct SlotEntry {
  std::mutex mu;
  ScalarSlot slot;
};
std::mutex g_slots_mu;
std::vector<SlotEntry*> g_slots;  // by device ordinal; never freed (process lifetime)
thread_local Signal t_signal{};
}  // namespace

Signal take_scalar_signal() {
  const Signal s = t_signal;
  t_signal = Signal{};
  return s;
}

ScalarCall::ScalarCall() {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess || dev < 0) {
    set_error("scalar call: hipGetDevice failed: %s", hipGetErrorString(e));
    return;
  }
  SlotEntry* ent = nullptr;
  {
    std::lock_guard<std::mutex> g(g_slots_mu);
    if (g_slots.size() <= (size_t)dev) g_slots.resize(dev + 1, nullptr);
    if (g_slots[dev] == nullptr) g_slots[dev] = new SlotEntry();
    ent = g_slots[dev];
  }
  auto* lk = new std::unique_lock<std::mutex>(ent->mu);
  ScalarSlot& sl = ent->slot;
  if (sl.h == nullptr) {
    void* h = nullptr;
    void* d = nullptr;
    hipStream_t st = nullptr;
    // the flag sits in the slot's last 128-byte line, away from the inputs and outputs
    if ((e = hipHostMalloc(&h, sizeof(double) * (kScalarSlotDoubles + 16), hipHostMallocMapped)) !=
            hipSuccess ||
        (e = hipHostGetDevicePointer(&d, h, 0)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) != hipSuccess) {
      set_error("scalar call: pinned staging set-up failed: %s", hipGetErrorString(e));
      if (h != nullptr) (void)hipHostFree(h);
      delete lk;
      return;
    }
    sl.h = static_cast<double*>(h);
    sl.d = static_cast<double*>(d);
    sl.st = st;
    sl.flag_h = reinterpret_cast<unsigned*>(sl.h + kScalarSlotDoubles);
    sl.flag_d = reinterpret_cast<unsigned*>(sl.d + kScalarSlotDoubles);
    __atomic_store_n(sl.flag_h, 0u, __ATOMIC_RELEASE);
  }
  slot_ = &sl;
  lock_ = lk;
}

ScalarCall::~ScalarCall() {
  if (armed_) t_signal = Signal{};  // never leave a signal armed past the call
  delete static_cast<std::unique_lock<std::mutex>*>(lock_);
}

void ScalarCall::arm(const double* in, int n_in) {
  if (++slot_->seq == 0) slot_->seq = 1;  // 0 is the flag's initial value
  Signal s{};
  s.flag = slot_->flag_d;
  s.seq = slot_->seq;
  s.n_in = in != nullptr ? std::min(n_in, 4) : 0;
  for (int i = 0; i < s.n_in; ++i) s.in[i] = in[i];
  t_signal = s;
  armed_ = true;
}

int ScalarCall::sync() {
  if (armed_) {
    armed_ = false;
    const bool taken = t_signal.flag == nullptr;
    t_signal = Signal{};
    if (taken) {
      // the kernel's outputs are visible once the flag holds seq; a launch that has not
      // signalled after ~2 ms (first-use code loading, a fault) is waited for on its stream
      const unsigned want = slot_->seq;
      const auto t0 = std::chrono::steady_clock::now();
      for (unsigned spins = 0;; ++spins) {
        if (__atomic_load_n(slot_->flag_h, __ATOMIC_ACQUIRE) == want) {
          // the outputs are complete.  The slot stream's sticky error state is polled every
          // 64th call: hipStreamQuery costs ~6 us, as much as the rest of the wait.  (Launch
          // errors are checked where each kernel is launched; a memory fault aborts the
          // process from the HSA queue handler.)
          hipError_t q = hipSuccess;
          if ((slot_->seq & 63) == 0) {
            q = hipStreamQuery(slot_->st);
            if (q == hipErrorNotReady) q = hipSuccess;
          }
          if (q == hipSuccess) return AIRICE_OK;
          set_error("scalar call: %s", hipGetErrorString(q));
          return AIRICE_EHIP;
        }
        if ((spins & 255) == 255 &&
            std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(2000))
          break;
      }
    }
  }
  const hipError_t e = hipStreamSynchronize(slot_->st);
  if (e != hipSuccess) {
    set_error("scalar call: %s", hipGetErrorString(e));
    return AIRICE_EHIP;
  }
  return AIRICE_OK;
}

// ---- one query of a minimizer entry point -----------------------------------------------------
// Each *_one below runs its query on the host (the cached folds and the entry point's host route)
// when scalar_on_host(), else on the device through the scalar slot (slot_call), as one launch
// that takes the slot's signal with the query's inputs inline.
int solve_one(const airice_medium* m, int variant, double ice_h, const double in[4], bool has_thr,
              double* out, uint8_t* status) {
  if (scalar_on_host()) {
    const DevMedium* M = nullptr;
    const IceConsts* I = nullptr;
    if (int rc = folded_ice(m, variant, ice_h, 0.0, &M, &I)) return rc;
    return solve_host_one(*M, *I, variant, in, has_thr, out, status);
  }
  const int fields = variant == AIRICE_VARIANT_PYWRAPPER ? AIRICE_PYSOLVE_FIELDS : AIRICE_SOLVE_FIELDS;
  return slot_call(in, 4, 0, out, fields, status, status != nullptr ? 1 : 0, has_thr ? 4 : 3,
                   [&](const SlotArgs& s) {
                     return airice_solve_launch(m, variant, ice_h, s.in, s.in + 1, s.in + 2,
                                                has_thr ? s.in + 3 : nullptr, 1, s.out, 1,
                                                status != nullptr ? s.flag : nullptr, s.st);
                   });
}

int hdtip_one(const airice_medium* m, double ice_cm, const double in[3], double out9[9],
              uint8_t* ok) {
  if (scalar_on_host()) {
    const DevMedium* M = nullptr;
    const IceConsts* I = nullptr;
    if (int rc = folded_ice(m, AIRICE_VARIANT_MULTIRAY, ice_cm / 100, 0.0, &M, &I)) return rc;
    return hdtip_host_one(*M, *I, ice_cm, in, out9, ok);
  }
  return slot_call(in, 3, 0, out9, 9, ok, 1, 3, [&](const SlotArgs& s) {
    return airice_hdtip_launch(m, s.in, s.in + 1, s.in + 2, ice_cm, 1, s.out, 1, s.flag, s.st);
  });
}

int trace_one(const airice_medium* m, const double in[4], double out10[10]) {
  if (scalar_on_host()) {
    const DevMedium* M = nullptr;
    const IceConsts* I = nullptr;
    if (int rc = folded_ice(m, AIRICE_VARIANT_PYWRAPPER, 0.0, 0.0, &M, &I)) return rc;
    return trace_host_one(*M, *I, in, out10);
  }
  return slot_call(in, 4, 0, out10, 10, nullptr, 0, 4, [&](const SlotArgs& s) {
    return airice_trace_ice_to_air_launch(m, s.in, s.in + 1, s.in + 2, s.in + 3, 1, s.out, s.st);
  });
}

int lookup_fallback_one(const airice_medium* m, double src_cm, double dist_cm, double depth_cm,
                        double ice_cm, bool good, int flags, double out9[9], bool* ok) {
  const double in[3] = {src_cm, dist_cm, depth_cm};
  uint8_t fb[2] = {(uint8_t)(good ? 1 : 0), (uint8_t)flags};  // the ok byte, the lookup's flags
  int rc;
  if (scalar_on_host()) {
    const DevMedium* M = nullptr;
    const IceConsts* I = nullptr;
    if ((rc = folded_ice(m, AIRICE_VARIANT_MULTIRAY, ice_cm / 100, 0.0, &M, &I))) return rc;
    rc = lookup_fallback_host_one(*M, *I, ice_cm, in, out9, &fb[0], &fb[1]);
  } else {
    rc = slot_call(in, 3, 0, out9, 9, fb, 2, 0, [&](const SlotArgs& s) {
      DevMedium M;
      IceConsts I;  // as airice_table_lookup_launch
      if (int rm = launch_folds(m, AIRICE_VARIANT_MULTIRAY, ice_cm / 100, 0.0, &M, &I)) return rm;
      return launch_lookup_fallback(M, I, s.in, s.in + 1, s.in + 2, ice_cm, s.out, 1, s.flag,
                                    s.flag + 1, s.st);
    });
  }
  if (rc == AIRICE_OK) *ok = fb[0] != 0;
  return rc;
}

}  // namespace airice

using namespace airice;

extern "C" int airice_table_cache_stats(int out[6]) {
  if (out == nullptr) {
    set_error("airice_table_cache_stats: out is null");
    return AIRICE_EINVAL;
  }
  table_cache_stats(out);
  return AIRICE_OK;
}

extern "C" int airice_air_cache_stats(int64_t out[6]) {
  if (out == nullptr) {
    set_error("airice_air_cache_stats: out is null");
    return AIRICE_EINVAL;
  }
  long long v[6];
  air_cache_stats(v);
  for (int i = 0; i < 6; ++i) out[i] = (int64_t)v[i];
  return AIRICE_OK;
}

extern "C" int airice_air_cache_limits(int64_t entry_bytes, int64_t total_bytes) {
  const int rc = air_cache_limits((long long)entry_bytes, (long long)total_bytes);
  if (rc != AIRICE_OK) set_error("airice_air_cache_limits: freeing a cached air record failed");
  return rc;
}

extern "C" int airice_kernel_timing(int on) {
  g_ktimer_on.store(on != 0, std::memory_order_relaxed);
  return AIRICE_OK;
}

extern "C" int airice_launch_count(const char* name, int64_t* count, int reset) {
  for (int i = 0; i < LC_COUNT; ++i)
    if (name != nullptr && std::strcmp(name, kLcNames[i]) == 0) {
      const long long v = reset ? g_launches[i].exchange(0) : g_launches[i].load();
      if (count) *count = (int64_t)v;
      return AIRICE_OK;
    }
  set_error("unknown counted kernel '%s'", name ? name : "(null)");
  return AIRICE_EINVAL;
}

extern "C" int airice_kernel_time(const char* name, double* total_ms, int64_t* launches,
                                  int reset) {
  int id = -1;
  for (int i = 0; i < KT_COUNT; ++i)
    if (name != nullptr && std::strcmp(name, kKtNames[i]) == 0) id = i;
  if (id < 0) {
    set_error("unknown timed kernel '%s'", name ? name : "(null)");
    return AIRICE_EINVAL;
  }
  std::lock_guard<std::mutex> lock(g_kt_mu);
  double sum = 0;
  for (KtPair& p : g_kt_done[id]) {
    float ms = 0;
    if (hipEventSynchronize(p.b) != hipSuccess || hipEventElapsedTime(&ms, p.a, p.b) != hipSuccess) {
      set_error("kernel timer: event query failed");
      return AIRICE_EHIP;
    }
    sum += ms;
  }
  if (total_ms) *total_ms = sum;
  if (launches) *launches = (int64_t)g_kt_done[id].size();
  if (reset) {
    for (KtPair& p : g_kt_done[id]) {
      (void)hipEventDestroy(p.a);
      (void)hipEventDestroy(p.b);
    }
    g_kt_done[id].clear();
  }
  return AIRICE_OK;
}

extern "C" {

// The folds of a call in a two-layer firn (f checked by bad_firn): M and I from the upper layer's
// medium with the antenna depth clipped to the boundary, the lower leg F, and whether the call
// takes the layered kernels at all -- an antenna at or above the boundary or in the air takes the
// one-layer kernels with M and I (*Fp = nullptr).
static int firn_folds(const airice_medium& m, const airice_firn& f, double ice_h, double rx_depth,
                      int in_ice, DevMedium* M, IceConsts* I, FirnLeg* F, const FirnLeg** Fp) {
  const airice_medium up = firn_layer_medium(m, f, 0);
  if (int rc = launch_folds(&up, AIRICE_VARIANT_MULTIRAY, ice_h, firn_clip_depth(f, rx_depth), M, I))
    return rc;
  build_firn_leg(*M, f, rx_depth, F);
  *Fp = (in_ice != 0 && F->below != 0) ? F : nullptr;
  return AIRICE_OK;
}

// The checks and folds of a table call; table: its (required) 11-column table, by name.
// f (nullable): the call's firn, with F and Fp as firn_folds.
static int table_prepare(const airice_medium* m, const airice_grid* g, int32_t row_begin,
                         int32_t row_count, NamedArg table, size_t ld, DevMedium* M, IceConsts* I,
                         const airice_firn* f = nullptr, FirnLeg* F = nullptr,
                         const FirnLeg** Fp = nullptr) {
  if (g == nullptr || row_begin < 0 || row_count < 0 ||
      (int64_t)row_begin + row_count > g->height_steps) {
    set_error("row range [%d,+%d) outside grid of %d rows", row_begin, row_count,
              g ? g->height_steps : -1);
    return AIRICE_EINVAL;
  }
  if (int rc = short_stride("table", "ld", ld, (size_t)row_count * (size_t)g->angle_steps))
    return rc;
  if (int rc = null_argument("table", {{"m", m}, table})) return rc;
  if (f != nullptr)
    return firn_folds(*m, *f, g->stop_height, -g->depth_m, g->in_ice, M, I, F, Fp);
  return launch_folds(m, AIRICE_VARIANT_MULTIRAY, g->stop_height, -g->depth_m, M, I);
}

// rows of [row_begin, row_begin+row_count) the table holds (the reference skips Tx <= 0, .cc:2082)
static int32_t kept_rows(const airice_grid* g, int32_t row_begin, int32_t row_count) {
  return std::max<int32_t>(0, std::min<int32_t>(row_count, g->table_rows - row_begin));
}

// The table and ray entry points, one body each for the one-layer call (f == nullptr) and its
// *_firn namesake.
static int table_launch(const airice_medium* m, const airice_firn* f, const airice_grid* g,
                        int32_t row_begin, int32_t row_count, float* d_table, double* d_full,
                        size_t ld, void* stream) {
  DevMedium M;
  IceConsts I;
  FirnLeg F;
  const FirnLeg* Fp = nullptr;
  int rc = table_prepare(m, g, row_begin, row_count, {"d_table", d_table}, ld, &M, &I, f, &F, &Fp);
  if (rc) return rc;
  rc = launch_table(M, I, g, row_begin, kept_rows(g, row_begin, row_count), d_table, d_full, ld,
                    (hipStream_t)stream, Fp);
  if (rc) set_error("table launch failed: %s", hipGetErrorString(hipGetLastError()));
  return rc;
}

int airice_table_launch(const airice_medium* m, const airice_grid* g, int32_t row_begin,
                        int32_t row_count, float* d_table, double* d_full, size_t ld,
                        void* stream) {
  return table_launch(m, nullptr, g, row_begin, row_count, d_table, d_full, ld, stream);
}

int airice_table_launch_firn(const airice_medium* m, const airice_firn* f, const airice_grid* g,
                             int32_t row_begin, int32_t row_count, float* d_table, double* d_full,
                             size_t ld, void* stream) {
  if (int rc = bad_firn("table", f)) return rc;
  return table_launch(m, f, g, row_begin, row_count, d_table, d_full, ld, stream);
}

static int table_launch_multi(const airice_medium* m, const airice_firn* f,
                              const airice_grid* grids, int32_t n_grids, float* const* d_tables,
                              const size_t* lds, void* stream) {
  if (n_grids < 0) {
    set_error("table multi: n_grids = %d", n_grids);
    return AIRICE_EINVAL;
  }
  if (n_grids == 0) return AIRICE_OK;
  if (int rc = null_argument("table multi", {{"m", m}, {"grids", grids}, {"d_tables", d_tables},
                                             {"lds", lds}}))
    return rc;
  DevMedium M;
  const airice_medium up = f != nullptr ? firn_layer_medium(*m, *f, 0) : *m;
  int rc = build_dev_medium(&up, AIRICE_VARIANT_MULTIRAY, &M);
  if (rc) return rc;
  std::vector<IceConsts> I(n_grids);
  std::vector<FirnLeg> F(f != nullptr ? n_grids : 0);
  bool layered = false;  // an antenna below the boundary: the layered kernel
  for (int a = 0; a < n_grids; ++a) {
    const airice_grid& g = grids[a];
    if (g.angle_steps != grids[0].angle_steps || g.angle_steps < 1 || d_tables[a] == nullptr) {
      set_error("multi-antenna launch: antenna %d has another angle grid or no table", a);
      return AIRICE_EINVAL;
    }
    if (f == nullptr) {
      build_ice_consts(M, g.stop_height, -g.depth_m, &I[a]);
      continue;
    }
    build_ice_consts(M, g.stop_height, firn_clip_depth(*f, -g.depth_m), &I[a]);
    build_firn_leg(M, *f, -g.depth_m, &F[a]);
    layered = layered || (g.in_ice != 0 && F[a].below != 0);
  }
  rc = launch_table_multi(M, I.data(), grids, n_grids, d_tables, lds, (hipStream_t)stream,
                          layered ? F.data() : nullptr);
  if (rc && rc != AIRICE_EINVAL)
    set_error("multi-antenna table launch failed: %s", hipGetErrorString(hipGetLastError()));
  return rc;
}

int airice_table_launch_multi(const airice_medium* m, const airice_grid* grids, int32_t n_grids,
                              float* const* d_tables, const size_t* lds, void* stream) {
  return table_launch_multi(m, nullptr, grids, n_grids, d_tables, lds, stream);
}

int airice_table_launch_multi_firn(const airice_medium* m, const airice_firn* f,
                                   const airice_grid* grids, int32_t n_grids,
                                   float* const* d_tables, const size_t* lds, void* stream) {
  if (int rc = bad_firn("table multi", f)) return rc;
  return table_launch_multi(m, f, grids, n_grids, d_tables, lds, stream);
}

static int table_host(const airice_medium* m, const airice_firn* f, const airice_grid* g,
                      int32_t row_begin, int32_t row_count, float* h_table, double* h_full,
                      size_t ld) {
  DevMedium M;
  IceConsts I;
  FirnLeg F;
  const FirnLeg* Fp = nullptr;
  int rc = table_prepare(m, g, row_begin, row_count, {"h_table", h_table}, ld, &M, &I, f, &F, &Fp);
  if (rc) return rc;
  DevBuffer dt, df;
  HIP_TRY(dt.alloc(sizeof(float) * 11 * ld));
  if (h_full) HIP_TRY(df.alloc(sizeof(double) * 18 * ld));
  const int32_t rows = kept_rows(g, row_begin, row_count);
  if (rows < row_count) {  // entries of skipped rows come back as NaN (0xFF bytes)
    HIP_TRY(hipMemset(dt.p, 0xFF, sizeof(float) * 11 * ld));
    if (h_full) HIP_TRY(hipMemset(df.p, 0xFF, sizeof(double) * 18 * ld));
  }
  rc = launch_table(M, I, g, row_begin, rows, static_cast<float*>(dt.p),
                    static_cast<double*>(df.p), ld, nullptr, Fp);
  if (rc == AIRICE_OK) {
    HIP_TRY(hipMemcpy(h_table, dt.p, sizeof(float) * 11 * ld, hipMemcpyDeviceToHost));
    if (h_full) HIP_TRY(hipMemcpy(h_full, df.p, sizeof(double) * 18 * ld, hipMemcpyDeviceToHost));
  }
  return rc;
}

int airice_table_host(const airice_medium* m, const airice_grid* g, int32_t row_begin,
                      int32_t row_count, float* h_table, double* h_full, size_t ld) {
  return table_host(m, nullptr, g, row_begin, row_count, h_table, h_full, ld);
}

int airice_table_host_firn(const airice_medium* m, const airice_firn* f, const airice_grid* g,
                           int32_t row_begin, int32_t row_count, float* h_table, double* h_full,
                           size_t ld) {
  if (int rc = bad_firn("table", f)) return rc;
  return table_host(m, f, g, row_begin, row_count, h_table, h_full, ld);
}

int airice_rays_host(const airice_medium* m, const double* launch_deg, const double* txh,
                     double ice_h_m, double depth_m, int32_t in_ice, size_t n, double* out,
                     size_t ld) {
  if (int rc = null_argument("rays", {{"m", m}, {"out", out}})) return rc;
  if (n > 0)
    if (int rc = null_argument("rays", {{"launch_deg", launch_deg}, {"txh", txh}})) return rc;
  if (int rc = short_stride("rays", "ld", ld, n)) return rc;
  const DevMedium* M = nullptr;
  const IceConsts* I = nullptr;
  if (int rc = airice::folded_ice(m, AIRICE_VARIANT_MULTIRAY, ice_h_m, -depth_m, &M, &I)) return rc;
  airice::rays_host(*M, *I, launch_deg, txh, in_ice, n, out, ld);
  return AIRICE_OK;
}

int airice_rays_host_firn(const airice_medium* m, const airice_firn* f, const double* launch_deg,
                          const double* txh, double ice_h_m, double depth_m, int32_t in_ice,
                          size_t n, double* out, size_t ld) {
  if (int rc = bad_firn("rays", f)) return rc;
  if (int rc = null_argument("rays", {{"m", m}, {"out", out}})) return rc;
  if (n > 0)
    if (int rc = null_argument("rays", {{"launch_deg", launch_deg}, {"txh", txh}})) return rc;
  if (int rc = short_stride("rays", "ld", ld, n)) return rc;
  DevMedium M;
  IceConsts I;
  FirnLeg F;
  const FirnLeg* Fp = nullptr;
  if (int rc = firn_folds(*m, *f, ice_h_m, -depth_m, in_ice, &M, &I, &F, &Fp)) return rc;
  airice::rays_host(M, I, launch_deg, txh, in_ice, n, out, ld, Fp);
  return AIRICE_OK;
}

int airice_scalar_mode(int mode) { return airice::set_scalar_mode(mode); }

int airice_rays_launch(const airice_medium* m, const double* d_launch, const double* d_txh,
                       double ice_h_m, double depth_m, int32_t in_ice, size_t n, double* d_out,
                       size_t ld, void* stream) {
  if (n > 0)
    if (int rc = null_argument("rays", {{"m", m}, {"d_launch", d_launch}, {"d_txh", d_txh},
                                        {"d_out", d_out}}))
      return rc;
  if (int rc = short_stride("rays", "ld", ld, n)) return rc;
  DevMedium M;
  IceConsts I;
  if (int rc = launch_folds(m, AIRICE_VARIANT_MULTIRAY, ice_h_m, -depth_m, &M, &I)) return rc;
  return launch_rays(M, I, d_launch, d_txh, in_ice, n, d_out, ld, (hipStream_t)stream);
}

int airice_rays_launch_firn(const airice_medium* m, const airice_firn* f, const double* d_launch,
                            const double* d_txh, double ice_h_m, double depth_m, int32_t in_ice,
                            size_t n, double* d_out, size_t ld, void* stream) {
  if (int rc = bad_firn("rays", f)) return rc;
  if (int rc = null_argument("rays", {{"m", m}})) return rc;
  if (n > 0)
    if (int rc = null_argument("rays", {{"d_launch", d_launch}, {"d_txh", d_txh},
                                        {"d_out", d_out}}))
      return rc;
  if (int rc = short_stride("rays", "ld", ld, n)) return rc;
  DevMedium M;
  IceConsts I;
  FirnLeg F;
  const FirnLeg* Fp = nullptr;
  if (int rc = firn_folds(*m, *f, ice_h_m, -depth_m, in_ice, &M, &I, &F, &Fp)) return rc;
  return launch_rays(M, I, d_launch, d_txh, in_ice, n, d_out, ld, (hipStream_t)stream, Fp);
}

int airice_solve_launch(const airice_medium* m, int variant, double ice_h_m, const double* d_txh,
                        const double* d_dist, const double* d_depth,
                        const double* d_straight_angle, size_t n, double* d_out, size_t ld,
                        uint8_t* d_status, void* stream) {
  if (int rc = bad_variant("solve", variant)) return rc;
  if (n > 0)
    if (int rc = null_argument("solve", {{"m", m}, {"d_txh", d_txh}, {"d_dist", d_dist},
                                         {"d_depth", d_depth}, {"d_out", d_out}}))
      return rc;
  if (int rc = short_stride("solve", "ld", ld, n)) return rc;
  DevMedium M;
  IceConsts I;
  if (int rc = launch_folds(m, variant, ice_h_m, 0.0, &M, &I)) return rc;
  return launch_solve(M, I, variant, d_txh, d_dist, d_depth, d_straight_angle, n, d_out, ld,
                      d_status, (hipStream_t)stream);
}

int airice_solve_host(const airice_medium* m, int variant, double ice_h_m, const double* txh,
                      const double* dist, const double* depth, const double* straight_angle,
                      size_t n, double* out, size_t ld, uint8_t* status) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("solve", {{"m", m}, {"txh", txh}, {"dist", dist}, {"depth", depth},
                                       {"out", out}}))
    return rc;
  if (int rc = bad_variant("solve", variant)) return rc;
  if (int rc = short_stride("solve", "ld", ld, n)) return rc;
  const int fields = variant == AIRICE_VARIANT_PYWRAPPER ? AIRICE_PYSOLVE_FIELDS : AIRICE_SOLVE_FIELDS;
  const bool has_thr = straight_angle != nullptr;
  if (n == 1) {  // one query: where airice_scalar_mode says
    const double in[4] = {txh[0], dist[0], depth[0], has_thr ? straight_angle[0] : 0.0};
    double o[AIRICE_SOLVE_FIELDS];
    uint8_t st = 0;
    if (int rc = airice::solve_one(m, variant, ice_h_m, in, has_thr, o, &st)) return rc;
    scatter_one(o, fields, st, out, ld, status);
    return AIRICE_OK;
  }
  const double* cols[4] = {txh, dist, depth, straight_angle};
  return staged_call(cols, has_thr ? 4 : 3, n, 0, fields, out, ld, status, [&](const Staged& s) {
    return airice_solve_launch(m, variant, ice_h_m, s.col(0), s.col(1), s.col(2),
                               has_thr ? s.col(3) : nullptr, n, s.out, n, s.status, nullptr);
  });
}

int airice_hdtip_launch(const airice_medium* m, const double* d_src_cm, const double* d_dist_cm,
                        const double* d_depth_cm, double ice_cm, size_t n, double* d_out,
                        size_t ld, uint8_t* d_ok, void* stream) {
  if (n > 0)
    if (int rc = null_argument("hdtip", {{"m", m}, {"d_src_cm", d_src_cm}, {"d_dist_cm", d_dist_cm},
                                         {"d_depth_cm", d_depth_cm}, {"d_out", d_out},
                                         {"d_ok", d_ok}}))
      return rc;
  if (int rc = short_stride("hdtip", "ld", ld, n)) return rc;
  DevMedium M;
  IceConsts I;
  if (int rc = launch_folds(m, AIRICE_VARIANT_MULTIRAY, ice_cm / 100, 0.0, &M, &I)) return rc;
  return launch_hdtip(M, I, d_src_cm, d_dist_cm, d_depth_cm, ice_cm, n, d_out, ld, d_ok,
                      (hipStream_t)stream);
}

int airice_table_lookup_launch(const airice_medium* m, const airice_lookup_table* t,
                               const double* d_src_cm, const double* d_dist_cm,
                               const double* d_depth_cm, double ice_cm, size_t n, double* d_out,
                               size_t ld, uint8_t* d_ok, uint8_t* d_flags, void* stream) {
  const char* who = "lookup";
  if (int rc = null_argument(who, {{"m", m}, {"t", t}})) return rc;
  if (n > 0)
    if (int rc = null_argument(who, {{"d_src_cm", d_src_cm}, {"d_dist_cm", d_dist_cm},
                                     {"d_depth_cm", d_depth_cm}, {"d_out", d_out}, {"d_ok", d_ok},
                                     {"d_flags", d_flags}}))
      return rc;
  if (int rc = short_stride(who, "ld", ld, n)) return rc;
  if (int rc = bad_lookup_table(who, t)) return rc;
  DevMedium M;
  IceConsts I;
  int rc = launch_folds(m, AIRICE_VARIANT_MULTIRAY, ice_cm / 100, 0.0, &M, &I);
  if (rc) return rc;
  return launch_lookup(M, I, t, d_src_cm, d_dist_cm, d_depth_cm, ice_cm, n, d_out, ld, d_ok,
                       d_flags, (hipStream_t)stream);
}

size_t airice_table_lookup_multi_work_bytes(int32_t n_tables, int32_t n_ant) {
  if (n_tables < 1 || n_tables > AIRICE_LOOKUP_MAX_TABLES || n_ant < 0) return 0;
  return airice::lookup_multi_work_bytes((size_t)n_tables, (size_t)n_ant);
}

int airice_table_lookup_launch_multi(const airice_medium* m, const airice_lookup_table* tables,
                                     int32_t n_tables, const int32_t* antenna_table,
                                     const double* antenna_depth_cm, int32_t n_ant,
                                     const double* d_src_cm, const double* d_dist_cm,
                                     size_t ld_dist, double ice_cm, size_t n_src, double* d_out,
                                     size_t ld, uint8_t* d_ok, uint8_t* d_flags, void* d_work,
                                     size_t work_bytes, void* stream) {
  const char* who = "lookup multi";
  if (n_tables < 1 || n_tables > AIRICE_LOOKUP_MAX_TABLES) {
    set_error("lookup multi: n_tables = %d outside 1..%d", n_tables, AIRICE_LOOKUP_MAX_TABLES);
    return AIRICE_EINVAL;
  }
  if (n_ant < 0) {
    set_error("lookup multi: n_ant = %d", n_ant);
    return AIRICE_EINVAL;
  }
  const bool work = n_ant > 0 && n_src > 0;
  if (int rc = null_argument(who, {{"m", m}, {"tables", tables}})) return rc;
  if (n_ant > 0)
    if (int rc = null_argument(who, {{"antenna_table", antenna_table},
                                     {"antenna_depth_cm", antenna_depth_cm}}))
      return rc;
  if (work)
    if (int rc = null_argument(who, {{"d_src_cm", d_src_cm}, {"d_dist_cm", d_dist_cm},
                                     {"d_out", d_out}, {"d_ok", d_ok}, {"d_flags", d_flags},
                                     {"d_work", d_work}}))
      return rc;
  for (int32_t i = 0; i < n_tables; ++i)
    if (int rc = bad_lookup_table(who, tables + i, i)) return rc;
  for (int32_t a = 0; a < n_ant; ++a)
    if (antenna_table[a] < 0 || antenna_table[a] >= n_tables) {
      set_error("lookup multi: antenna_table[%d] = %d outside [0, %d)", a, antenna_table[a],
                n_tables);
      return AIRICE_EINVAL;
    }
  if (ld_dist < n_src) {
    set_error("lookup multi: ld_dist (%zu) < n_src (%zu)", ld_dist, n_src);
    return AIRICE_EINVAL;
  }
  if (n_src >= (1ull << 32)) {
    set_error("lookup multi: n_src = %zu exceeds one launch", n_src);
    return AIRICE_EINVAL;
  }
  if (ld < (size_t)n_ant * n_src) {
    set_error("lookup multi: ld (%zu) < n_ant*n_src (%zu)", ld, (size_t)n_ant * n_src);
    return AIRICE_EINVAL;
  }
  if (!work) return AIRICE_OK;
  const size_t need = airice::lookup_multi_work_bytes((size_t)n_tables, (size_t)n_ant);
  if (work_bytes < need || (reinterpret_cast<uintptr_t>(d_work) & 15) != 0) {
    set_error("lookup multi: workspace of %zu bytes (16-byte aligned), need %zu "
              "(airice_table_lookup_multi_work_bytes)", work_bytes, need);
    return AIRICE_EINVAL;
  }
  DevMedium M;
  IceConsts I;  // as airice_table_lookup_launch
  int rc = launch_folds(m, AIRICE_VARIANT_MULTIRAY, ice_cm / 100, 0.0, &M, &I);
  if (rc) return rc;
  return launch_lookup_multi(M, I, tables, n_tables, antenna_table, antenna_depth_cm,
                             (size_t)n_ant, d_src_cm, d_dist_cm, ld_dist, ice_cm, n_src, d_out, ld,
                             d_ok, d_flags, d_work, (hipStream_t)stream);
}

size_t airice_lookup_pack_floats(size_t n_entries, int32_t total_angle_steps) {
  if (n_entries < 1 || total_angle_steps < 1) return 0;
  return AIRICE_LOOKUP_PACK_FLOATS(n_entries, total_angle_steps);
}

int airice_lookup_pack(const airice_lookup_table* t, float* d_entries, size_t capacity_floats,
                       void* stream) {
  if (int rc = null_argument("lookup pack", {{"t", t}, {"d_entries", d_entries}})) return rc;
  if (int rc = null_argument("lookup pack", {{"table", t->table}})) return rc;
  if (t->ld < t->n_entries || (reinterpret_cast<uintptr_t>(d_entries) & 15) != 0) {
    set_error("ld < n_entries or entries not 16-byte aligned");
    return AIRICE_EINVAL;
  }
  if (t->n_entries < 1 || t->total_angle_steps < 1) {  // the row records divide by the row length
    set_error("lookup pack: n_entries (%zu) and total_angle_steps (%d) must be >= 1",
              t->n_entries, t->total_angle_steps);
    return AIRICE_EINVAL;
  }
  const size_t need = AIRICE_LOOKUP_PACK_FLOATS(t->n_entries, t->total_angle_steps);
  if (capacity_floats < need) {
    set_error("lookup pack: %zu floats given, pack format 2 needs %zu "
              "(AIRICE_LOOKUP_PACK_FLOATS / airice_lookup_pack_floats)", capacity_floats, need);
    return AIRICE_EINVAL;
  }
  const int rc = launch_lookup_pack(t, d_entries, (hipStream_t)stream);
  if (rc) set_error("lookup pack failed: %s", hipGetErrorString(hipGetLastError()));
  return rc;
}

int airice_single_ray_plan(const airice_medium* m, double antenna_depth_m, double launch_deg,
                           double txh_m, double ice_m, airice_single_ray_info* info) {
  if (int rc = null_argument("single ray", {{"m", m}, {"info", info}})) return rc;
  return plan_single_ray(m, antenna_depth_m, launch_deg, txh_m, ice_m, info);
}

int airice_single_ray_launch(const airice_medium* m, double antenna_depth_m, double launch_deg,
                             double txh_m, double ice_m, double* d_summary, double* d_x,
                             double* d_z, size_t cap, void* stream) {
  if (int rc = null_argument("single ray", {{"m", m}, {"d_summary", d_summary}})) return rc;
  if ((d_x == nullptr) != (d_z == nullptr)) {
    set_error("single ray: d_x/d_z both or neither");
    return AIRICE_EINVAL;
  }
  DevMedium M;
  int rc = build_dev_medium(m, AIRICE_VARIANT_MULTIRAY, &M);  // RayTracingFunctions pi (.h:26)
  if (rc) return rc;
  return launch_single_ray(M, m, antenna_depth_m, launch_deg, txh_m, ice_m, d_summary, d_x, d_z,
                           cap, (hipStream_t)stream);
}

double airice_nz_air(const airice_medium* m, double z) {
  DevMedium M;
  if (build_dev_medium(m, AIRICE_VARIANT_MULTIRAY, &M) != AIRICE_OK) return NAN;
  return host_air_endpoint(M, std::fabs(z)).n;
}

double airice_nz_firn(const airice_medium* m, const airice_firn* f, double z) {
  if (m == nullptr || f == nullptr) return std::nan("");
  const int l = std::fabs(z) <= f->boundary_m ? 0 : 1;
  return m->A_ice + f->B[l] * std::exp(-f->C[l] * std::fabs(z));
}

double airice_nz_ice(const airice_medium* m, double z) {
  DevMedium M;
  if (build_dev_medium(m, AIRICE_VARIANT_MULTIRAY, &M) != AIRICE_OK) return NAN;
  return host_ice_endpoint(M, std::fabs(z)).n;
}

int airice_rtf_outputs(int op, int max_layers) { return airice::rtf_outputs(op, max_layers); }

int airice_rtf_eval(const airice_medium* m, int op, const double* args, size_t n_args, double* out,
                    size_t n_out) {
  return airice_rtf_eval_variant(m, AIRICE_VARIANT_MULTIRAY, op, args, n_args, out, n_out);
}

int airice_rtf_eval_variant(const airice_medium* m, int variant, int op, const double* args,
                            size_t n_args, double* out, size_t n_out) {
  if (int rc = null_argument("rtf", {{"m", m}, {"out", out}})) return rc;
  if (n_args > 0)
    if (int rc = null_argument("rtf", {{"args", args}})) return rc;
  if (int rc = bad_variant("rtf", variant)) return rc;
  const DevMedium* M = nullptr;
  if (int rc = airice::folded_medium(m, variant, &M)) return rc;
  const int need = airice::rtf_outputs(op, M->ml);
  if (need < 0) {
    set_error("unknown RayTracingFunctions op %d", op);
    return AIRICE_EINVAL;
  }
  if (n_out < (size_t)need || n_args > 8) {
    set_error("rtf op %d: %zu outputs (need %d), %zu args (max 8)", op, n_out, need, n_args);
    return AIRICE_EINVAL;
  }
  if (airice::scalar_on_host()) return airice::rtf_host(*M, op, args, n_args, out);
  // the inputs travel in the kernel arguments; the kernel writes its outputs into the slot
  const DevMedium Md = *M;  // the launch's own copy: the fold cache is the thread's
  return slot_call(nullptr, 0, 0, out, need, nullptr, 0, 0, [&](const SlotArgs& s) {
    return airice::launch_rtf(Md, op, args, n_args, s.out, s.st);
  });
}

int airice_air2ice_launch(const airice_medium* m, const double* d_txh, const double* d_dist,
                          const double* d_ice, const double* d_depth, size_t n, double* d_out,
                          size_t ld, uint8_t* d_status, void* stream) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("air2ice", {{"m", m}, {"txh", d_txh}, {"dist", d_dist}, {"ice", d_ice},
                                         {"depth", d_depth}, {"out", d_out}}))
    return rc;
  if (int rc = short_stride("air2ice", "ld", ld, n)) return rc;
  if (int rc = exceeds_one_launch("air2ice", n)) return rc;
  DevMedium M;
  int rc = build_dev_medium(m, AIRICE_VARIANT_MULTIRAY, &M);  // RayTracingFunctions pi (.h:26)
  if (rc) return rc;
  return airice::launch_air2ice(M, d_txh, d_dist, d_ice, d_depth, n, d_out, ld, d_status,
                                (hipStream_t)stream);
}

int airice_air2ice_host(const airice_medium* m, const double* txh, const double* dist,
                        const double* ice, const double* depth, size_t n, double* out, size_t ld,
                        uint8_t* status) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("air2ice", {{"m", m}, {"txh", txh}, {"dist", dist}, {"ice", ice},
                                         {"depth", depth}, {"out", out}}))
    return rc;
  if (int rc = short_stride("air2ice", "ld", ld, n)) return rc;
  constexpr int kF = AIRICE_RTF_AIR2ICE_FIELDS;
  if (n == 1) {  // one query: where airice_scalar_mode says
    const double in[4] = {txh[0], dist[0], ice[0], depth[0]};
    double o[kF];
    uint8_t st = 0;
    if (airice::scalar_on_host()) {
      const DevMedium* M = nullptr;
      if (int rc = airice::folded_medium(m, AIRICE_VARIANT_MULTIRAY, &M)) return rc;
      airice::air2ice_host_one(*M, in, o, &st);
    } else if (int rc = slot_call(in, 4, 0, o, kF, &st, 1, kNoSignal, [&](const SlotArgs& s) {
                 return airice_air2ice_launch(m, s.in, s.in + 1, s.in + 2, s.in + 3, 1, s.out, 1,
                                              s.flag, s.st);
               })) {
      return rc;
    }
    scatter_one(o, kF, st, out, ld, status);
    return AIRICE_OK;
  }
  const double* cols[4] = {txh, dist, ice, depth};
  return staged_call(cols, 4, n, 0, kF, out, ld, status, [&](const Staged& s) {
    return airice_air2ice_launch(m, s.col(0), s.col(1), s.col(2), s.col(3), n, s.out, n, s.status,
                                 nullptr);
  });
}

// ---- the in-ice solver (IceRayTracing::IceRayTracing), batched ---------------------------------
int airice_iceray_launch(const double* model3, const double* d_z0, const double* d_x1,
                         const double* d_z1, size_t n, double* d_out, size_t ld,
                         uint8_t* d_status, void* stream) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("iceray", {{"z0", d_z0}, {"x1", d_x1}, {"z1", d_z1}, {"out", d_out}}))
    return rc;
  if (int rc = short_stride("iceray", "ld", ld, n)) return rc;
  if (int rc = exceeds_one_launch("iceray", n)) return rc;
  return airice::launch_iceray(ice_model_or_default(model3), d_z0, d_x1, d_z1, n, d_out, ld,
                               d_status, (hipStream_t)stream);
}

int airice_iceray_host(const double* model3, const double* z0, const double* x1, const double* z1,
                       size_t n, double* out, size_t ld, uint8_t* status) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("iceray", {{"z0", z0}, {"x1", x1}, {"z1", z1}, {"out", out}}))
    return rc;
  if (int rc = short_stride("iceray", "ld", ld, n)) return rc;
  constexpr int kF = AIRICE_ICERAY_FIELDS;
  if (n == 1) {  // one pair: where airice_scalar_mode says
    const double in[3] = {z0[0], x1[0], z1[0]};
    double o[kF];
    uint8_t st = 0;
    if (airice::scalar_on_host()) {
      airice::iceray_host_one(ice_model_or_default(model3), in, o, &st);
    } else if (int rc = slot_call(in, 3, 0, o, kF, &st, 1, kNoSignal, [&](const SlotArgs& s) {
                 return airice_iceray_launch(model3, s.in, s.in + 1, s.in + 2, 1, s.out, 1, s.flag,
                                             s.st);
               })) {
      return rc;
    }
    scatter_one(o, kF, st, out, ld, status);
    return AIRICE_OK;
  }
  const double* cols[3] = {z0, x1, z1};
  return staged_call(cols, 3, n, 0, kF, out, ld, status, [&](const Staged& s) {
    return airice_iceray_launch(model3, s.col(0), s.col(1), s.col(2), n, s.out, n, s.status,
                                nullptr);
  });
}

// ---- the ice-to-air direct ray (IceRayTracing::GetDirectRayPar_Air), batched --------------------
int airice_iceair_launch(const double* model3, const double* d_z0, const double* d_x1,
                         const double* d_h, size_t n, double* d_out, size_t ld, uint8_t* d_status,
                         void* stream) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("iceair", {{"z0", d_z0}, {"x1", d_x1}, {"h", d_h}, {"out", d_out}}))
    return rc;
  if (int rc = short_stride("iceair", "ld", ld, n)) return rc;
  if (int rc = exceeds_one_launch("iceair", n)) return rc;
  return airice::launch_iceair(ice_model_or_default(model3), d_z0, d_x1, d_h, n, d_out, ld,
                               d_status, (hipStream_t)stream);
}

int airice_iceair_host(const double* model3, const double* z0, const double* x1, const double* h,
                       size_t n, double* out, size_t ld, uint8_t* status) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("iceair", {{"z0", z0}, {"x1", x1}, {"h", h}, {"out", out}}))
    return rc;
  if (int rc = short_stride("iceair", "ld", ld, n)) return rc;
  constexpr int kF = AIRICE_ICEAIR_FIELDS;
  if (n == 1) {  // one triple: where airice_scalar_mode says
    const double in[3] = {z0[0], x1[0], h[0]};
    double o[kF];
    uint8_t st = 0;
    if (airice::scalar_on_host()) {
      airice::iceair_host_one(ice_model_or_default(model3), in, o, &st);
    } else if (int rc = slot_call(in, 3, 0, o, kF, &st, 1, kNoSignal, [&](const SlotArgs& s) {
                 return airice_iceair_launch(model3, s.in, s.in + 1, s.in + 2, 1, s.out, 1, s.flag,
                                             s.st);
               })) {
      return rc;
    }
    scatter_one(o, kF, st, out, ld, status);
    return AIRICE_OK;
  }
  const double* cols[3] = {z0, x1, h};
  return staged_call(cols, 3, n, 0, kF, out, ld, status, [&](const Staged& s) {
    return airice_iceair_launch(model3, s.col(0), s.col(1), s.col(2), n, s.out, n, s.status,
                                nullptr);
  });
}

// ---- the first-arriving ray between 3-D points (IceRayTracing::DirectRayTracer), batched --------
size_t airice_icefirst_work_bytes(size_t n_pairs) {
  return sizeof(double) * (size_t)airice::icefirst::kWorkDoubles * n_pairs;
}

// The pairs of a first-arrival call, or what is wrong with its pairing and counts.
static int icefirst_pairs(size_t n_tx, size_t n_rx, int pairing, size_t* n_pairs) {
  if (pairing != AIRICE_PAIRS_ELEMENTWISE && pairing != AIRICE_PAIRS_CROSS) {
    set_error("icefirst: unknown pairing %d", pairing);
    return AIRICE_EINVAL;
  }
  if (pairing == AIRICE_PAIRS_ELEMENTWISE && n_tx != n_rx) {
    set_error("icefirst: n_tx (%zu) != n_rx (%zu) with AIRICE_PAIRS_ELEMENTWISE", n_tx, n_rx);
    return AIRICE_EINVAL;
  }
  if (pairing == AIRICE_PAIRS_CROSS && n_rx != 0 && n_tx > ((size_t)1 << 46) / n_rx) {
    set_error("icefirst: n_tx (%zu) x n_rx (%zu) exceeds one launch", n_tx, n_rx);
    return AIRICE_EINVAL;
  }
  *n_pairs = pairing == AIRICE_PAIRS_CROSS ? n_tx * n_rx : n_tx;
  return AIRICE_OK;
}

int airice_icefirst_launch(const double* model3, const double* d_tx_x, const double* d_tx_y,
                           const double* d_tx_z, size_t n_tx, const double* d_rx_x,
                           const double* d_rx_y, const double* d_rx_z, size_t n_rx, int pairing,
                           void* d_work, size_t work_bytes, double* d_out, size_t ld,
                           uint8_t* d_status, void* stream) {
  size_t n = 0;
  if (int rc = icefirst_pairs(n_tx, n_rx, pairing, &n)) return rc;
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("icefirst", {{"tx_x", d_tx_x}, {"tx_y", d_tx_y}, {"tx_z", d_tx_z},
                                          {"rx_x", d_rx_x}, {"rx_y", d_rx_y}, {"rx_z", d_rx_z},
                                          {"work", d_work}, {"out", d_out}}))
    return rc;
  if (int rc = short_stride("icefirst", "ld", ld, n)) return rc;
  if (int rc = exceeds_one_launch("icefirst", n)) return rc;
  if (work_bytes < airice_icefirst_work_bytes(n)) {
    set_error("icefirst: work_bytes (%zu) < airice_icefirst_work_bytes(%zu) = %zu", work_bytes, n,
              airice_icefirst_work_bytes(n));
    return AIRICE_EINVAL;
  }
  return airice::launch_icefirst(ice_model_or_default(model3), d_tx_x, d_tx_y, d_tx_z, d_rx_x,
                                 d_rx_y, d_rx_z, n_rx, pairing == AIRICE_PAIRS_CROSS, n,
                                 static_cast<double*>(d_work), d_out, ld, d_status,
                                 (hipStream_t)stream);
}

int airice_icefirst_select_launch(const double* d_rays, size_t ld_rays, const double* d_x1,
                                  size_t n, double* d_out, size_t ld, uint8_t* d_status,
                                  void* stream) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("icefirst select", {{"rays", d_rays}, {"x1", d_x1}, {"out", d_out}}))
    return rc;
  if (int rc = short_stride("icefirst select", "ld_rays", ld_rays, n)) return rc;
  if (int rc = short_stride("icefirst select", "ld", ld, n)) return rc;
  if (int rc = exceeds_one_launch("icefirst select", n)) return rc;
  return airice::launch_icefirst_select(d_rays, ld_rays, d_x1, n, d_out, ld, d_status,
                                        (hipStream_t)stream);
}

int airice_icefirst_host(const double* model3, const double* tx_x, const double* tx_y,
                         const double* tx_z, size_t n_tx, const double* rx_x, const double* rx_y,
                         const double* rx_z, size_t n_rx, int pairing, double* out, size_t ld,
                         uint8_t* status) {
  size_t n = 0;
  if (int rc = icefirst_pairs(n_tx, n_rx, pairing, &n)) return rc;
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("icefirst", {{"tx_x", tx_x}, {"tx_y", tx_y}, {"tx_z", tx_z},
                                          {"rx_x", rx_x}, {"rx_y", rx_y}, {"rx_z", rx_z},
                                          {"out", out}}))
    return rc;
  if (int rc = short_stride("icefirst", "ld", ld, n)) return rc;
  constexpr int kF = AIRICE_ICEFIRST_FIELDS, kW = airice::icefirst::kWorkDoubles;
  if (n == 1) {  // one pair: where airice_scalar_mode says
    const double in[6] = {tx_x[0], tx_y[0], tx_z[0], rx_x[0], rx_y[0], rx_z[0]};
    double o[kF];
    uint8_t st = 0;
    if (airice::scalar_on_host()) {
      airice::icefirst_host_one(ice_model_or_default(model3), in, o, &st);
    } else if (int rc = slot_call(in, 6, kW, o, kF, &st, 1, kNoSignal,  // three launches
                                  [&](const SlotArgs& s) {
                                    return airice_icefirst_launch(
                                        model3, s.in, s.in + 1, s.in + 2, 1, s.in + 3, s.in + 4,
                                        s.in + 5, 1, AIRICE_PAIRS_ELEMENTWISE, s.scratch,
                                        sizeof(double) * kW, s.out, 1, s.flag, s.st);
                                  })) {
      return rc;
    }
    scatter_one(o, kF, st, out, ld, status);
    return AIRICE_OK;
  }
  // six input columns of stride n: an emitter column holds n_tx values, an antenna column n_rx
  const double* cols[6] = {tx_x, tx_y, tx_z, rx_x, rx_y, rx_z};
  const size_t lens[6] = {n_tx, n_tx, n_tx, n_rx, n_rx, n_rx};
  return staged_call(cols, lens, 6, n, (size_t)kW * n, kF, out, ld, status, [&](const Staged& s) {
    return airice_icefirst_launch(model3, s.col(0), s.col(1), s.col(2), n_tx, s.col(3), s.col(4),
                                  s.col(5), n_rx, pairing, s.scratch, sizeof(double) * kW * n,
                                  s.out, n, s.status, nullptr);
  });
}

// ---- GetRayTracingSolutions / GetFocusingFactor over the solver's rows --------------------------
// What is wrong with the values of an icesol call (set as the error), or false.
static bool icesol_refuses(const double* model3, double a0, double frequency_ghz) {
  const char* bad = airice::icesol_bad_value(ice_model_or_default(model3), a0, frequency_ghz);
  if (bad != nullptr) set_error("icesol: %s", bad);
  return bad != nullptr;
}

int airice_icesol_launch(const double* model3, const double* d_z0, const double* d_x1,
                         const double* d_z1, const double* d_rays, size_t ld_rays,
                         const double* d_rays_lower, size_t ld_lower, size_t n, double a0,
                         double frequency_ghz, double* d_out, size_t ld, uint8_t* d_status,
                         void* stream) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("icesol", {{"z0", d_z0}, {"x1", d_x1}, {"z1", d_z1}, {"out", d_out},
                                        {"rays", d_rays}}))
    return rc;
  if (int rc = short_stride("icesol", "ld", ld, n)) return rc;
  if (int rc = short_stride("icesol", "ld_rays", ld_rays, n)) return rc;
  if (d_rays_lower != nullptr)
    if (int rc = short_stride("icesol", "ld_lower", ld_lower, n)) return rc;
  if (icesol_refuses(model3, a0, frequency_ghz)) return AIRICE_EINVAL;
  if (int rc = exceeds_one_launch("icesol", n)) return rc;
  return airice::launch_icesol(ice_model_or_default(model3), a0, frequency_ghz, d_z0, d_x1, d_z1,
                               d_rays, ld_rays, d_rays_lower, ld_lower, n, d_out, ld, d_status,
                               (hipStream_t)stream);
}

// The launches of one icesol call on device arrays of stride n: the solver's rows for the
// receiver into rays, for the receiver 1 cm lower (z1_lower; null: no focusing) into rays + 32 n,
// then the solutions.
static int icesol_launches(const double* model3, const double* z0, const double* x1,
                           const double* z1, const double* z1_lower, double* rays, size_t n,
                           double a0, double frequency_ghz, double* out, uint8_t* status,
                           hipStream_t st) {
  double* lower = z1_lower != nullptr ? rays + (size_t)AIRICE_ICERAY_FIELDS * n : nullptr;
  int rc = airice_iceray_launch(model3, z0, x1, z1, n, rays, n, nullptr, st);
  if (rc == AIRICE_OK && lower != nullptr)
    rc = airice_iceray_launch(model3, z0, x1, z1_lower, n, lower, n, nullptr, st);
  if (rc == AIRICE_OK)
    rc = airice_icesol_launch(model3, z0, x1, z1, rays, n, lower, n, n, a0, frequency_ghz, out, n,
                              status, st);
  return rc;
}

int airice_icesol_host(const double* model3, const double* z0, const double* x1, const double* z1,
                       size_t n, double a0, double frequency_ghz, int focusing, double* out,
                       size_t ld, uint8_t* status) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("icesol", {{"z0", z0}, {"x1", x1}, {"z1", z1}, {"out", out}}))
    return rc;
  if (int rc = short_stride("icesol", "ld", ld, n)) return rc;
  if (icesol_refuses(model3, a0, frequency_ghz)) return AIRICE_EINVAL;
  constexpr int kF = AIRICE_ICESOL_FIELDS, kR = AIRICE_ICERAY_FIELDS;
  const bool focus = focusing != 0;
  if (n == 1) {  // one pair: where airice_scalar_mode says
    const double in[4] = {z0[0], x1[0], z1[0], z1[0] - 0.01};
    double o[kF];
    uint8_t st = 0;
    if (airice::scalar_on_host()) {
      airice::icesol_host_one(ice_model_or_default(model3), in, a0, frequency_ghz, focus, o, &st);
    } else if (int rc = slot_call(in, 4, 2 * kR, o, kF, &st, 1, kNoSignal,  // up to three launches
                                  [&](const SlotArgs& s) {
                                    return icesol_launches(model3, s.in, s.in + 1, s.in + 2,
                                                           focus ? s.in + 3 : nullptr, s.scratch, 1,
                                                           a0, frequency_ghz, s.out, s.flag, s.st);
                                  })) {
      return rc;
    }
    scatter_one(o, kF, st, out, ld, status);
    return AIRICE_OK;
  }
  // the fourth input column is the receiver 1 cm lower (GetFocusingFactor), formed here
  std::vector<double> lower;
  if (focus) {
    lower = std::vector<double>(z1, z1 + n);
    for (double& v : lower) v = v - 0.01;
  }
  const double* cols[4] = {z0, x1, z1, lower.data()};
  return staged_call(cols, focus ? 4 : 3, n, (focus ? 2 : 1) * (size_t)kR * n, kF, out, ld, status,
                     [&](const Staged& s) {
                       return icesol_launches(model3, s.col(0), s.col(1), s.col(2),
                                              focus ? s.col(3) : nullptr, s.scratch, n, a0,
                                              frequency_ghz, s.out, s.status, nullptr);
                     });
}

// ---- the two rays' attenuation over a frequency grid ---------------------------------------------
// What is wrong with the values and sizes of a spectrum call (set as the error), or AIRICE_OK.
static int icespec_refuses(const double* model3, double a0, size_t n_freq, size_t ld_f) {
  if (n_freq == 0) {
    set_error("icespec: n_freq is 0");
    return AIRICE_EINVAL;
  }
  if (int rc = short_stride("icespec", "ld_f", ld_f, n_freq)) return rc;
  if (n_freq > ((size_t)1 << 27)) {  // 16 pairs x n_freq items in 32 bits
    set_error("icespec: n_freq = %zu exceeds one launch", n_freq);
    return AIRICE_EINVAL;
  }
  if (const char* bad = airice::icespec_bad_value(ice_model_or_default(model3), a0)) {
    set_error("icespec: %s", bad);
    return AIRICE_EINVAL;
  }
  return AIRICE_OK;
}

int airice_icesol_spectrum_launch(const double* model3, const double* d_z0, const double* d_z1,
                                  const double* d_rays, size_t ld_rays, const double* d_sol,
                                  size_t ld_sol, size_t n, double a0, const double* d_freq_ghz,
                                  size_t n_freq, double* d_att, size_t ld_f, void* stream) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("icespec", {{"z0", d_z0}, {"z1", d_z1}, {"rays", d_rays},
                                         {"sol", d_sol}, {"freq_ghz", d_freq_ghz},
                                         {"att", d_att}}))
    return rc;
  if (int rc = icespec_refuses(model3, a0, n_freq, ld_f)) return rc;
  if (int rc = short_stride("icespec", "ld_rays", ld_rays, n)) return rc;
  if (int rc = short_stride("icespec", "ld_sol", ld_sol, n)) return rc;
  if (int rc = exceeds_one_launch("icespec", n, airice::icespec_pairs_per_block(n_freq)))
    return rc;
  return airice::launch_icespec(ice_model_or_default(model3), a0, d_z0, d_z1, d_rays, ld_rays,
                                d_sol, ld_sol, n, d_freq_ghz, n_freq, d_att, ld_f,
                                (hipStream_t)stream);
}

int airice_icesol_spectrum_host(const double* model3, const double* z0, const double* x1,
                                const double* z1, size_t n, double a0, const double* freq_ghz,
                                size_t n_freq, double* sol_out, size_t ld, uint8_t* status,
                                double* att_out, size_t ld_f) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("icespec", {{"z0", z0}, {"x1", x1}, {"z1", z1},
                                         {"freq_ghz", freq_ghz}, {"sol_out", sol_out},
                                         {"att_out", att_out}}))
    return rc;
  if (int rc = icespec_refuses(model3, a0, n_freq, ld_f)) return rc;
  if (int rc = short_stride("icespec", "ld", ld, n)) return rc;
  constexpr int kF = AIRICE_ICESOL_FIELDS, kR = AIRICE_ICERAY_FIELDS;
  if (n == 1 && airice::scalar_on_host()) {  // one pair on the calling thread
    const double in[3] = {z0[0], x1[0], z1[0]};
    double o[kF];
    uint8_t st = 0;
    airice::icespec_host_one(ice_model_or_default(model3), in, a0, freq_ghz, n_freq, o, &st,
                             att_out, att_out + ld_f);
    scatter_one(o, kF, st, sol_out, ld, status);
    return AIRICE_OK;
  }
  // The staged block's scratch: the solver's rows, the frequencies, the spectra.  The solutions
  // are at freq_ghz[0], which -- like every bin -- is not refused: a bad one gives NaN columns.
  if (int rc = exceeds_one_launch("icespec", n)) return rc;
  const size_t n_rays = (size_t)kR * n, n_att = 2 * n * n_freq;
  const double* cols[3] = {z0, x1, z1};
  return staged_call(cols, 3, n, n_rays + n_freq + n_att, kF, sol_out, ld, status,
                     [&](const Staged& s) -> int {
    double* rays = s.scratch;
    double* freq = rays + n_rays;
    double* att = freq + n_freq;
    HIP_TRY(hipMemcpy(freq, freq_ghz, sizeof(double) * n_freq, hipMemcpyHostToDevice));
    int rc = airice_iceray_launch(model3, s.col(0), s.col(1), s.col(2), n, rays, n, nullptr,
                                  nullptr);
    if (rc == AIRICE_OK)
      rc = airice::launch_icesol(ice_model_or_default(model3), a0, freq_ghz[0], s.col(0),
                                 s.col(1), s.col(2), rays, n, nullptr, 0, n, s.out, n, s.status,
                                 nullptr);
    if (rc == AIRICE_OK)
      rc = airice_icesol_spectrum_launch(model3, s.col(0), s.col(2), rays, n, s.out, n, n, a0,
                                         freq, n_freq, att, n_freq, nullptr);
    if (rc) return rc;
    // the copy waits for the kernels: the call's one synchronisation
    HIP_TRY(hipMemcpy2D(att_out, sizeof(double) * ld_f, att, sizeof(double) * n_freq,
                        sizeof(double) * n_freq, 2 * n, hipMemcpyDeviceToHost));
    return AIRICE_OK;
  });
}

int airice_single_ray_host(const airice_medium* m, double antenna_depth_m, double launch_deg,
                           double txh_m, double ice_m, double* summary, double* x, double* z,
                           size_t cap) {
  if (int rc = null_argument("single ray", {{"summary", summary}})) return rc;
  airice_single_ray_info info;
  int rc = airice_single_ray_plan(m, antenna_depth_m, launch_deg, txh_m, ice_m, &info);
  if (rc) return rc;
  const size_t n = (size_t)(info.n_air + info.n_ice);
  const bool path = x != nullptr && z != nullptr;
  if (path && n > cap) {
    set_error("single ray: %zu path samples exceed capacity %zu", n, cap);
    return AIRICE_EINVAL;
  }
  DevBuffer buf;
  const size_t words = AIRICE_SINGLE_RAY_WORK + (path ? 2 * n : 0);
  HIP_TRY(buf.alloc(sizeof(double) * words));
  double* d = static_cast<double*>(buf.p);
  double* dx = path ? d + AIRICE_SINGLE_RAY_WORK : nullptr;
  double* dz = path ? dx + n : nullptr;
  rc = airice_single_ray_launch(m, antenna_depth_m, launch_deg, txh_m, ice_m, d, dx, dz, n, nullptr);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(summary, d, sizeof(double) * AIRICE_SINGLE_RAY_FIELDS, hipMemcpyDeviceToHost));
  if (path && n > 0) {
    HIP_TRY(hipMemcpy(x, dx, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(z, dz, sizeof(double) * n, hipMemcpyDeviceToHost));
  }
  return AIRICE_OK;
}

int airice_ray_paths_plan(const airice_medium* m, double antenna_depth_m, double ice_m,
                          const double* txh_m, size_t n, int64_t* offsets, size_t* work_bytes) {
  if (int rc = null_argument("ray paths", {{"m", m}, {"offsets", offsets}})) return rc;
  if (n > 0)
    if (int rc = null_argument("ray paths", {{"txh_m", txh_m}})) return rc;
  return plan_ray_paths(m, antenna_depth_m, ice_m, txh_m, n, offsets, work_bytes);
}

// x and z of a ray-paths call are given together or not at all.
static int ray_paths_xz(const void* x, const void* z) {
  if ((x == nullptr) == (z == nullptr)) return AIRICE_OK;
  set_error("ray paths: x / z both or neither");
  return AIRICE_EINVAL;
}

int airice_ray_paths_launch(const airice_medium* m, double antenna_depth_m, double ice_m,
                            const double* d_launch_deg, const double* txh_m, size_t n,
                            const int64_t* offsets, void* d_work, size_t work_bytes,
                            double* d_summary, size_t ld, double* d_x, double* d_z, size_t cap,
                            void* stream) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("ray paths", {{"m", m}, {"d_launch_deg", d_launch_deg},
                                           {"txh_m", txh_m}, {"offsets", offsets},
                                           {"d_work", d_work}, {"d_summary", d_summary}}))
    return rc;
  if (int rc = ray_paths_xz(d_x, d_z)) return rc;
  if (int rc = short_stride("ray paths", "ld", ld, n)) return rc;
  DevMedium M;
  int rc = build_dev_medium(m, AIRICE_VARIANT_MULTIRAY, &M);  // RayTracingFunctions pi (.h:26)
  if (rc) return rc;
  return launch_ray_paths(M, m, antenna_depth_m, ice_m, d_launch_deg, txh_m, n, offsets, d_work,
                          work_bytes, d_summary, ld, d_x, d_z, cap, (hipStream_t)stream);
}

int airice_ray_paths_host(const airice_medium* m, double antenna_depth_m, double ice_m,
                          const double* launch_deg, const double* txh_m, size_t n,
                          const int64_t* offsets, double* summary, size_t ld, double* x, double* z,
                          size_t cap) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("ray paths", {{"m", m}, {"launch_deg", launch_deg}, {"txh_m", txh_m},
                                           {"offsets", offsets}, {"summary", summary}}))
    return rc;
  if (int rc = ray_paths_xz(x, z)) return rc;
  if (int rc = short_stride("ray paths", "ld", ld, n)) return rc;
  std::vector<int64_t> planned(n + 1);
  size_t work_bytes = 0;
  int rc = plan_ray_paths(m, antenna_depth_m, ice_m, txh_m, n, planned.data(), &work_bytes);
  if (rc) return rc;
  const bool path = x != nullptr;
  const size_t total = path ? (size_t)planned[n] : 0;
  if (path && total > cap) {
    set_error("ray paths: %zu path samples exceed capacity %zu", total, cap);
    return AIRICE_EINVAL;
  }
  DevBuffer work, vals;  // vals: launch angles, summary columns, x, z
  HIP_TRY(work.alloc(work_bytes));
  HIP_TRY(vals.alloc(sizeof(double) * (n * (1 + AIRICE_SINGLE_RAY_FIELDS) + 2 * total)));
  double* d_launch = static_cast<double*>(vals.p);
  double* d_sum = d_launch + n;
  double* dx = path ? d_sum + n * AIRICE_SINGLE_RAY_FIELDS : nullptr;
  double* dz = path ? dx + total : nullptr;
  HIP_TRY(hipMemcpy(d_launch, launch_deg, sizeof(double) * n, hipMemcpyHostToDevice));
  rc = airice_ray_paths_launch(m, antenna_depth_m, ice_m, d_launch, txh_m, n, offsets, work.p,
                               work_bytes, d_sum, n, dx, dz, total, nullptr);
  if (rc) return rc;
  for (int f = 0; f < AIRICE_SINGLE_RAY_FIELDS; ++f)
    HIP_TRY(hipMemcpy(summary + (size_t)f * ld, d_sum + (size_t)f * n, sizeof(double) * n,
                      hipMemcpyDeviceToHost));
  if (total > 0) {
    HIP_TRY(hipMemcpy(x, dx, sizeof(double) * total, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(z, dz, sizeof(double) * total, hipMemcpyDeviceToHost));
  }
  return AIRICE_OK;
}

int airice_trace_ice_to_air_launch(const airice_medium* m, const double* d_depth,
                                   const double* d_ice, const double* d_txh, const double* d_dist,
                                   size_t n, double* d_out10, void* stream) {
  if (n > 0)
    if (int rc = null_argument("trace", {{"m", m}, {"d_depth", d_depth}, {"d_ice", d_ice},
                                         {"d_txh", d_txh}, {"d_dist", d_dist},
                                         {"d_out10", d_out10}}))
      return rc;
  DevMedium M;
  IceConsts I;
  if (int rc = launch_folds(m, AIRICE_VARIANT_PYWRAPPER, 0.0, 0.0, &M, &I)) return rc;
  return launch_trace(M, I, d_depth, d_ice, d_txh, d_dist, n, d_out10, (hipStream_t)stream);
}

int airice_trace_ice_to_air_host(const airice_medium* m, const double* depth, const double* ice,
                                 const double* txh, const double* dist, size_t n, double* out10) {
  if (n == 0) return AIRICE_OK;
  if (int rc = null_argument("trace", {{"m", m}, {"depth", depth}, {"ice", ice}, {"txh", txh},
                                       {"dist", dist}, {"out10", out10}}))
    return rc;
  if (n == 1) {  // one query: where airice_scalar_mode says
    const double in[4] = {depth[0], ice[0], txh[0], dist[0]};
    return airice::trace_one(m, in, out10);
  }
  const double* cols[4] = {depth, ice, txh, dist};
  return staged_call(cols, 4, n, 0, 10, out10, n, nullptr, [&](const Staged& s) {
    return airice_trace_ice_to_air_launch(m, s.col(0), s.col(1), s.col(2), s.col(3), n, s.out,
                                          nullptr);
  });
}

int airice_device_count(int* count) {
  HIP_TRY(hipGetDeviceCount(count));
  return AIRICE_OK;
}
int airice_set_device(int device) {
  HIP_TRY(hipSetDevice(device));
  return AIRICE_OK;
}
int airice_malloc(void** ptr, size_t bytes) {
  HIP_TRY(hipMalloc(ptr, bytes));
  return AIRICE_OK;
}
int airice_free(void* ptr) {
  HIP_TRY(hipFree(ptr));
  return AIRICE_OK;
}
int airice_memcpy_h2d(void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return AIRICE_OK;
}
int airice_memcpy_d2h(void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return AIRICE_OK;
}
int airice_table_to_host(const float* d_table, size_t d_ld, size_t n_rays, float* h_table,
                         size_t h_ld, void* stream) {
  if (n_rays == 0) return AIRICE_OK;
  if (d_table == nullptr || h_table == nullptr || d_ld < n_rays || h_ld < n_rays) {
    set_error("table_to_host: null table or column stride < n_rays");
    return AIRICE_EINVAL;
  }
  const hipStream_t st = (hipStream_t)stream;
  if (d_ld == n_rays && h_ld == n_rays) {  // both tables dense: one copy
    HIP_TRY(hipMemcpyAsync(h_table, d_table, sizeof(float) * n_rays * AIRICE_TABLE_COLUMNS,
                           hipMemcpyDeviceToHost, st));
    return AIRICE_OK;
  }
  // One copy per column.  (A 2D copy with the host table's pitch fails with "invalid argument"
  // when the host rows are a slab of a larger table -- the multi-GPU host assembly, where each
  // rank page-locks only its own rows of each column -- and each column is a contiguous range.)
  for (int c = 0; c < AIRICE_TABLE_COLUMNS; ++c)
    HIP_TRY(hipMemcpyAsync(h_table + (size_t)c * h_ld, d_table + (size_t)c * d_ld,
                           sizeof(float) * n_rays, hipMemcpyDeviceToHost, st));
  return AIRICE_OK;
}
int airice_host_register(void* ptr, size_t bytes) {
  if (ptr == nullptr || bytes == 0) {
    set_error("host_register: empty range");
    return AIRICE_EINVAL;
  }
  HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterPortable));
  return AIRICE_OK;
}
int airice_host_unregister(void* ptr) {
  HIP_TRY(hipHostUnregister(ptr));
  return AIRICE_OK;
}
int airice_synchronize(void) {
  HIP_TRY(hipDeviceSynchronize());
  return AIRICE_OK;
}

}  // extern "C"
