// airice_gridcache.hpp -- the device-buffer caches of the table launchers (airice_table.hip):
// GridCache (per-grid buffers a fill kernel writes) and ConstSetCache (the multi-antenna launch's
// constant sets).  Host-only cache policy: no kernels, nothing a kernel reads.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <vector>

#include "airice.h"
#include "airice_internal.h"

namespace airice {

// Per-grid device caches of the table launch: the row constants of every Tx-height row
// (RowConst, 104 B; rowconst_kernel) and the start-angle sine of every grid column (8 B;
// angle_sines_kernel).  Both are O(rows + columns) work that every block of a launch would
// otherwise redo for the rows and columns it touches.
//
// Life of an entry (GridCache::get):
//  - the FIRST launch that needs a key records the key only and forms its rows / sines in the
//    kernel (rc / vs = nullptr): a grid built once -- one table per antenna, RunMultiRayCode.C's
//    pattern -- pays no fill kernel, no allocation and no synchronisation;
//  - the SECOND launch with the key allocates the buffer, enqueues the fill kernel on its own
//    stream ahead of its table kernel (stream order makes the buffer complete for it) and records
//    an event behind the fill; no host synchronisation;
//  - later launches use the buffer: on the filling stream directly, on another stream once the
//    event has completed (hipEventQuery) or behind a hipStreamWaitEvent on it;
//  - a launch being captured into a graph uses an entry only if its fill is already known to be
//    complete, and pins it: a pinned buffer is never evicted (its address lives in the graph's
//    kernel arguments).  Otherwise the captured launch forms its rows / sines in the kernel.  No
//    allocation, query or fill happens under capture.
// A buffer is written once and never overwritten.  At most kCacheSets unpinned entries per device;
// the least recently used is freed with hipFree, which waits for the kernels still reading it.
// The caller holds grid_cache_mutex() from the lookup until its launches are enqueued, so no other
// thread can evict a buffer in between; a multi-antenna launch touches at most kMaxAntennas
// (< kCacheSets) entries, so its own are never the least recently used.
// (inline: one mutex however many units include this header)
AIRICE_LOCAL inline std::mutex& grid_cache_mutex() {
  static std::mutex mu;
  return mu;
}
// A stream that is being captured into a graph (no allocation, query or synchronisation then).
AIRICE_LOCAL inline bool stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}
constexpr size_t kCacheSets = 64;

class GridCache {
 public:
  // fill(buffer, stream): enqueue the kernel that writes the whole buffer.  fill_first: fill at
  // the key's first use already (large launches, where forming the values in the kernel costs
  // more than the fill kernel).
  template <class Fill>
  int get(const std::vector<unsigned char>& key, size_t bytes, hipStream_t st, Fill fill,
          bool fill_first, const void** out) {
    *out = nullptr;
    // a buffer above the byte limits is never cached: no key, no entry (set_limits)
    if (bytes > entry_cap_ || bytes > total_cap_) return AIRICE_OK;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return AIRICE_EHIP;
    if (per_dev_.size() <= (size_t)dev) per_dev_.resize(dev + 1);
    Dev& D = per_dev_[dev];
    Entry* c = nullptr;
    for (Entry& e : D.entries)
      if (e.key == key) c = &e;
    if (stream_capturing(st)) {
      if (c != nullptr && c->dev != nullptr && c->ready) {
        c->pinned = true;
        c->used = ++D.tick;
        *out = c->dev;
      }
      return AIRICE_OK;  // otherwise the captured kernel forms the values itself
    }
    if (c == nullptr) {  // first use: remember the key, the kernel forms the values
      if (int rc = make_room(D)) return rc;
      Entry e;
      e.key = key;
      e.used = ++D.tick;
      D.entries.push_back(std::move(e));
      if (!fill_first) return AIRICE_OK;
      c = &D.entries.back();
    }
    c->used = ++D.tick;
    if (c->dev == nullptr) {  // second use: fill, stream-ordered ahead of this launch
      // under a byte budget: free least recently used unpinned buffers first; when the pinned
      // ones leave no room the launch goes uncached
      bool fits = false;
      if (int rc = trim(D, bytes, c, &fits)) return rc;
      if (!fits) return AIRICE_OK;
      void* p = nullptr;
      if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return AIRICE_EHIP;
      fill(p, st);
      hipEvent_t ev = nullptr;
      if (hipGetLastError() != hipSuccess ||
          hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess ||
          hipEventRecord(ev, st) != hipSuccess) {
        if (ev != nullptr) (void)hipEventDestroy(ev);
        (void)hipFree(p);
        return AIRICE_EHIP;
      }
      c->dev = p;
      c->bytes = bytes;
      c->ev = ev;
      c->origin = st;
      *out = p;
      return AIRICE_OK;
    }
    if (!c->ready) {
      const hipError_t q = hipEventQuery(c->ev);
      if (q == hipSuccess) {
        c->ready = true;
      } else if (q != hipErrorNotReady) {
        return AIRICE_EHIP;
      } else if (st != c->origin && hipStreamWaitEvent(st, c->ev, 0) != hipSuccess) {
        return AIRICE_EHIP;
      }
    }
    *out = c->dev;
    return AIRICE_OK;
  }

  // entries of the current device (tests: airice_table_cache_stats)
  void stats(int* keys, int* filled, int* pinned, size_t* bytes = nullptr) {
    int dev = 0;
    *keys = *filled = *pinned = 0;
    if (bytes != nullptr) *bytes = 0;
    if (hipGetDevice(&dev) != hipSuccess || per_dev_.size() <= (size_t)dev) return;
    for (const Entry& e : per_dev_[dev].entries) {
      ++*keys;
      *filled += e.dev != nullptr;
      *pinned += e.pinned;
      if (bytes != nullptr) *bytes += e.bytes;
    }
  }

  // Byte limits (the air record's cache; the row and sine caches have none): a buffer larger than
  // entry_cap is never cached, and the buffers of one device hold at most total_cap bytes --
  // least recently used unpinned buffers are freed to make room, their keys stay.  Lowering the
  // total frees down to it at once, on every device; a total of 0 (the cache switched off) also
  // forgets the keys of all unpinned entries.
  int set_limits(size_t entry_cap, size_t total_cap) {
    entry_cap_ = entry_cap;
    total_cap_ = total_cap;
    for (Dev& D : per_dev_) {
      bool fits = false;
      if (int rc = trim(D, 0, nullptr, &fits)) return rc;
      if (total_cap == 0)
        D.entries.erase(std::remove_if(D.entries.begin(), D.entries.end(),
                                       [](const Entry& e) { return !e.pinned; }),
                        D.entries.end());
    }
    return AIRICE_OK;
  }
  size_t entry_cap() const { return entry_cap_; }
  size_t total_cap() const { return total_cap_; }

 private:
  struct Entry {
    std::vector<unsigned char> key;
    void* dev = nullptr;        // nullptr: seen once, not filled
    hipEvent_t ev = nullptr;    // recorded behind the fill kernel
    hipStream_t origin = nullptr;
    bool ready = false;         // the fill is known complete
    bool pinned = false;        // handed to a captured launch: never evicted
    unsigned long long used = 0;
    size_t bytes = 0;           // of the buffer
  };
  struct Dev {
    std::vector<Entry> entries;
    unsigned long long tick = 0;
  };
  // evict the least recently used unpinned entry when kCacheSets unpinned entries exist
  static int make_room(Dev& D) {
    size_t unpinned = 0, old = D.entries.size();
    for (size_t k = 0; k < D.entries.size(); ++k) {
      if (D.entries[k].pinned) continue;
      ++unpinned;
      if (old == D.entries.size() || D.entries[k].used < D.entries[old].used) old = k;
    }
    if (unpinned < kCacheSets) return AIRICE_OK;
    Entry& e = D.entries[old];
    if (e.dev != nullptr && hipFree(e.dev) != hipSuccess) return AIRICE_EHIP;
    if (e.ev != nullptr) (void)hipEventDestroy(e.ev);
    D.entries.erase(D.entries.begin() + (long)old);
    return AIRICE_OK;
  }
  // Frees least recently used unpinned buffers of D (not keep's) until `need` more bytes fit
  // under total_cap_; an entry whose buffer is freed is back to "seen once".  hipFree waits for
  // the kernels still reading the buffer.
  int trim(Dev& D, size_t need, const Entry* keep, bool* fits) {
    for (;;) {
      size_t held = 0;
      Entry* old = nullptr;
      for (Entry& e : D.entries) {
        held += e.bytes;
        if (e.dev == nullptr || e.pinned || &e == keep) continue;
        if (old == nullptr || e.used < old->used) old = &e;
      }
      *fits = need <= total_cap_ && held <= total_cap_ - need;
      if (*fits || total_cap_ == SIZE_MAX || old == nullptr) return AIRICE_OK;
      if (hipFree(old->dev) != hipSuccess) return AIRICE_EHIP;
      if (old->ev != nullptr) (void)hipEventDestroy(old->ev);
      old->dev = nullptr;
      old->ev = nullptr;
      old->origin = nullptr;
      old->ready = false;
      old->bytes = 0;
    }
  }
  std::vector<Dev> per_dev_;
  size_t entry_cap_ = SIZE_MAX, total_cap_ = SIZE_MAX;
};

// Device copies of the per-antenna constants of a multi-antenna table launch, one immutable
// buffer per distinct constant set (up to kConstSets unpinned per device, least recently used
// evicted).  A buffer is written once, by a synchronous copy before any launch reads it, and
// never overwritten; eviction frees it with hipFree, which waits for the kernels still reading
// it, on any stream.  Under graph capture (no allocation or copy allowed) a launch needs its set
// to be resident already -- one uncaptured launch of the same antenna set first -- and pins it: a
// pinned set is never evicted, since the graph keeps its address.
// Not a GridCache: a set is complete after its first (synchronous) use, a GridCache entry only
// after a second launch and a completed event.
// No lock of its own: the caller holds grid_cache_mutex() from the lookup until its launch is
// enqueued, so no other thread can evict the buffer in between.
class AIRICE_LOCAL ConstSetCache {
 public:
  // packed: the launch's constant set (taken over when it is new).  capturing: the launch is
  // being captured into a graph.  AIRICE_OK and *dev_ptr, AIRICE_EHIP, or AIRICE_EINVAL when a
  // captured launch finds no resident set (the caller words the error).
  int get(std::vector<unsigned char>& packed, bool capturing, void** dev_ptr) {
    *dev_ptr = nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return AIRICE_EHIP;
    if (caches_.size() <= (size_t)dev) caches_.resize(dev + 1);
    std::vector<ConstSet>& sets = caches_[dev];
    ConstSet* c = nullptr;
    for (ConstSet& e : sets)
      if (e.host == packed) c = &e;
    if (c == nullptr && capturing) return AIRICE_EINVAL;
    if (c == nullptr) {
      size_t unpinned = 0, old = sets.size();
      for (size_t k = 0; k < sets.size(); ++k) {
        if (sets[k].pinned) continue;
        ++unpinned;
        if (old == sets.size() || sets[k].used < sets[old].used) old = k;
      }
      if (unpinned >= kConstSets) {  // evict the least recently used unpinned set
        if (hipFree(sets[old].dev) != hipSuccess) return AIRICE_EHIP;
        sets.erase(sets.begin() + (long)old);
      }
      ConstSet e;
      if (hipMalloc(&e.dev, packed.size()) != hipSuccess) return AIRICE_EHIP;
      if (hipMemcpy(e.dev, packed.data(), packed.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(e.dev);
        return AIRICE_EHIP;
      }
      e.host = std::move(packed);
      sets.push_back(std::move(e));
      c = &sets.back();
    }
    c->used = ++tick_;
    if (capturing) c->pinned = true;
    *dev_ptr = c->dev;
    return AIRICE_OK;
  }

 private:
  struct ConstSet {
    std::vector<unsigned char> host;
    void* dev = nullptr;
    unsigned long long used = 0;
    bool pinned = false;
  };
  static constexpr size_t kConstSets = 8;
  std::vector<std::vector<ConstSet>> caches_;  // per device
  unsigned long long tick_ = 0;
};

}  // namespace airice
