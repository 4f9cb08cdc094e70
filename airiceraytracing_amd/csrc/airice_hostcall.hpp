// airice_hostcall.hpp -- the host glue of the C-ABI entries, written once (airice_runtime.cpp and
// airice_icetab.hip include it; every name is private to the including unit):
//
//   checks     the argument-check vocabulary: each sets the error and returns AIRICE_EINVAL
//   folds      launch_folds: the kernel-argument medium and ice constants through the thread's cache
//   staged     staged_call: the batch route of a *_host entry through one device block
//   slot       slot_call: the one-query route through the device's scalar slot
//
// A new entry states only what is particular to it: its columns, its kernel and its nullable
// arguments.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "airice.h"
#include "airice_iceray.hpp"
#include "airice_internal.h"

#define HIP_TRY(expr)                                                          \
  do {                                                                         \
    hipError_t e_ = (expr);                                                    \
    if (e_ != hipSuccess) {                                                    \
      airice::set_error("%s failed: %s", #expr, hipGetErrorString(e_));        \
      return AIRICE_EHIP;                                                      \
    }                                                                          \
  } while (0)

namespace airice {
namespace {

// Device buffer freed on every exit path of the *_host entry points.
struct DevBuffer {
  void* p = nullptr;
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
  ~DevBuffer() {
    if (p != nullptr) (void)hipFree(p);
  }
};

// ---- checks ----------------------------------------------------------------------------------
struct NamedArg {
  const char* name;
  const void* p;
};
// The first null pointer among an entry's required arguments, by name.
inline int null_argument(const char* who, std::initializer_list<NamedArg> required) {
  for (const NamedArg& a : required)
    if (a.p == nullptr) {
      set_error("%s: null argument (%s)", who, a.name);
      return AIRICE_EINVAL;
    }
  return AIRICE_OK;
}
inline int short_stride(const char* who, const char* ld_name, size_t ld, size_t n) {
  if (ld >= n) return AIRICE_OK;
  set_error("%s: %s (%zu) < n (%zu)", who, ld_name, ld, n);
  return AIRICE_EINVAL;
}
// One item per lane, blocks of `block` lanes, a 31-bit grid.
inline int exceeds_one_launch(const char* who, size_t n, size_t block = 256) {
  if (n <= (size_t)0x7fffffff * block) return AIRICE_OK;
  set_error("%s: n = %zu exceeds one launch", who, n);
  return AIRICE_EINVAL;
}
inline int bad_variant(const char* who, int variant) {
  if (variant == AIRICE_VARIANT_MULTIRAY || variant == AIRICE_VARIANT_PYWRAPPER) return AIRICE_OK;
  set_error("%s: unknown variant %d", who, variant);
  return AIRICE_EINVAL;
}
// A lookup table's description as the lookup kernels need it; index >= 0 names tables[index].
inline int bad_lookup_table(const char* who, const airice_lookup_table* t, int index = -1) {
  char where[32] = "";
  if (index >= 0) snprintf(where, sizeof(where), "tables[%d]", index);
  if (t == nullptr || t->table == nullptr) {
    set_error("%s: null argument (%s%stable)", who, where, index >= 0 ? "." : "");
    return AIRICE_EINVAL;
  }
  if (t->n_entries == 0 || t->ld < t->n_entries || t->total_angle_steps < 1 ||
      t->total_height_steps < 1 || !(t->height_step > 0) ||
      (reinterpret_cast<uintptr_t>(t->entries) & 15) != 0) {
    set_error("%s: invalid lookup table description%s%s%s", who, index >= 0 ? " (" : "", where,
              index >= 0 ? ")" : "");
    return AIRICE_EINVAL;
  }
  return AIRICE_OK;
}

// The firn of a *_firn entry point: non-null, every field finite, boundary_m > 0, C[l] > 0.
inline int bad_firn(const char* who, const airice_firn* f) { return firn_check(who, f); }

// model3, or IceRayTracing's default {A, B, C} (airice_iceray.hpp) when it is null.
inline const double* ice_model_or_default(const double* model3) {
  static const double kDefault[3] = {iceray::kDefaultModel.A, iceray::kDefaultModel.B,
                                     iceray::kDefaultModel.C};
  return model3 != nullptr ? model3 : kDefault;
}

// ---- folds -----------------------------------------------------------------------------------
// The launch constants are a pure function of the medium, the variant, the ice height and the
// antenna depth: repeated launches reuse the thread's folds (folded_ice) instead of re-deriving
// ~20 host exp()s.  Copies, because the cache is the thread's and its next user overwrites it.
inline int launch_folds(const airice_medium* m, int variant, double ice_h,
                                  double rx_depth, DevMedium* M, IceConsts* I) {
  const DevMedium* Mc = nullptr;
  const IceConsts* Ic = nullptr;
  if (int rc = folded_ice(m, variant, ice_h, rx_depth, &Mc, &Ic)) return rc;
  *M = *Mc;
  *I = *Ic;
  return AIRICE_OK;
}

// ---- staged: the batch route of a *_host entry -------------------------------------------------
// One device block:  in (k x n) | scratch | out (fields x n) | status (n bytes).
struct Staged {
  size_t n;
  double* in;       // column j of the inputs at col(j)
  double* scratch;  // scratch_doubles, uninitialised
  double* out;      // `fields` dense columns (stride n)
  uint8_t* status;
  double* col(size_t j) const { return in + j * n; }
};
// Uploads the k input columns cols[0 .. k-1] (n doubles each), runs launch(const Staged&) -- its
// kernels go on the null stream -- and copies the outputs into the caller's columns of stride ld
// (the padding [n, ld) of a column is left alone) and the status bytes into status (nullable).
// lens (nullable): column j holds lens[j] <= n doubles, the rest of its n is left uninitialised.
template <class Launch>
int staged_call(const double* const* cols, const size_t* lens, size_t k, size_t n,
                size_t scratch_doubles, int fields, double* out, size_t ld, uint8_t* status,
                Launch launch) {
  DevBuffer buf;
  HIP_TRY(buf.alloc(sizeof(double) * ((k + (size_t)fields) * n + scratch_doubles) + n));
  Staged s;
  s.n = n;
  s.in = static_cast<double*>(buf.p);
  s.scratch = s.in + k * n;
  s.out = s.scratch + scratch_doubles;
  s.status = reinterpret_cast<uint8_t*>(s.out + (size_t)fields * n);
  for (size_t j = 0; j < k; ++j)
    HIP_TRY(hipMemcpy(s.col(j), cols[j], sizeof(double) * (lens != nullptr ? lens[j] : n),
                      hipMemcpyHostToDevice));
  if (int rc = launch(s)) return rc;
  // the copy-back is on the null stream, like the launches: it waits for the kernels
  HIP_TRY(hipMemcpy2D(out, sizeof(double) * ld, s.out, sizeof(double) * n, sizeof(double) * n,
                      (size_t)fields, hipMemcpyDeviceToHost));
  if (status != nullptr) HIP_TRY(hipMemcpy(status, s.status, n, hipMemcpyDeviceToHost));
  return AIRICE_OK;
}
template <class Launch>
int staged_call(const double* const* cols, size_t k, size_t n, size_t scratch_doubles, int fields,
                double* out, size_t ld, uint8_t* status, Launch launch) {
  return staged_call(cols, nullptr, k, n, scratch_doubles, fields, out, ld, status, launch);
}

// The n == 1 form of the same hand-over: one value per column, and the status byte.
inline void scatter_one(const double* o, int fields, uint8_t st, double* out, size_t ld,
                                  uint8_t* status) {
  for (int c = 0; c < fields; ++c) out[(size_t)c * ld] = o[c];
  if (status != nullptr) status[0] = st;
}

// ---- slot: one query through the device's scalar slot -------------------------------------------
// The device views of a call's part of the slot, and the slot's stream.
struct SlotArgs {
  const double* in;
  double* scratch;
  double* out;
  uint8_t* flag;
  hipStream_t st;
};
constexpr int kNoSignal = -1;
// The slot holds, in doubles: the n_in inputs, then n_scratch of scratch, then -- each on a 64-byte
// boundary -- the n_out outputs (ld = 1) and the n_flag flag bytes.  in -> slot, launch(const SlotArgs&),
// the wait, slot -> out and flag (flag bytes are read and written: in/out of the kernels).
// signal: kNoSignal, or -- for a call made of exactly ONE launch whose launcher takes the signal
// (take_scalar_signal) -- how many of the inputs also travel in the kernel arguments (0..4).
template <class Launch>
int slot_call(const double* in, int n_in, int n_scratch, double* out, int n_out, uint8_t* flag,
              int n_flag, int signal, Launch launch) {
  const int o_out = (n_in + n_scratch + 7) & ~7, o_flag = (o_out + n_out + 7) & ~7;
  if (o_flag * sizeof(double) + (size_t)n_flag > kScalarSlotDoubles * sizeof(double)) {
    set_error("scalar call: %d + %d + %d doubles and %d bytes exceed the slot", n_in, n_scratch,
              n_out, n_flag);
    return AIRICE_EINVAL;
  }
  ScalarCall call;
  if (!call.ok()) return AIRICE_EHIP;
  ScalarSlot& s = call.slot();
  std::copy(in, in + n_in, s.h);
  uint8_t* flag_h = reinterpret_cast<uint8_t*>(s.h + o_flag);
  std::copy(flag, flag + n_flag, flag_h);
  if (signal != kNoSignal) call.arm(s.h, signal);
  int rc = launch(SlotArgs{s.d, s.d + n_in, s.d + o_out, reinterpret_cast<uint8_t*>(s.d + o_flag),
                           s.st});
  if (rc == AIRICE_OK) rc = call.sync();
  if (rc) return rc;
  std::copy(s.h + o_out, s.h + o_out + n_out, out);
  std::copy(flag_h, flag_h + n_flag, flag);
  return AIRICE_OK;
}

}  // namespace
}  // namespace airice
