// airice_fold.cpp -- the host folds of the kernel-argument constants: the medium (DevMedium), the
// ice height's and antenna's constants (IceConsts), and the two-layer firn (its argument check,
// its upper-layer medium, the lower leg's FirnLeg and the layered host ray route).  Host arithmetic
// only, no HIP call, so the same file also builds into a sanitizer program of its own
// (tests/cpp/firn_driver.cpp, `make firn_driver_asan`).
#include <cmath>
#include <cstring>

#include "airice.h"
#include "airice_host.h"
#include "airice_internal.h"
#include "airice_ray.hpp"

namespace airice {

static int host_air_layer(const DevMedium& M, double zabs) {
  int which = 0;
  for (int l = 0; l < M.ml - 1; ++l) {
    if (zabs < M.atm[l + 1] && zabs >= M.atm[l]) {
      which = l;
      break;
    }
  }
  if (zabs >= M.atm[M.ml - 1]) which = M.ml - 1;
  return which;
}

Endpoint host_air_endpoint(const DevMedium& M, double x) {
  const double zabs = std::fabs(x);
  const int l = host_air_layer(M, zabs);
  const double C = M.negC[l];
  const double e_abs = std::exp(C * zabs);
  const double e_x = x >= 0.0 ? e_abs : std::exp(C * x);
  return make_endpoint(M.A_air, M.B[l], C, x, e_abs, e_x);
}

Endpoint host_ice_endpoint(const DevMedium& M, double x) {
  const double zabs = std::fabs(x);
  const double e_abs = std::exp(M.negC_ice * zabs);
  const double e_x = x >= 0.0 ? e_abs : std::exp(M.negC_ice * x);
  return make_endpoint(M.A_ice, M.B_ice, M.negC_ice, x, e_abs, e_x);
}

int build_dev_medium(const airice_medium* m, int variant, DevMedium* out) {
  if (m == nullptr || out == nullptr) {
    set_error("null medium");
    return AIRICE_EINVAL;
  }
  if (m->max_layers < 1 || m->max_layers > kMaxLayers) {
    set_error("medium not initialised (max_layers=%d)", m->max_layers);
    return AIRICE_EINVAL;
  }
  DevMedium& M = *out;
  std::memset(&M, 0, sizeof(M));
  const double pi = variant_pi(variant);
  for (int i = 0; i < 5; ++i) {
    M.atm[i] = m->atmlay_cm[i] / 100;
    M.B[i] = m->B_air[i];
    M.negC[i] = -m->C_air[i];
  }
  M.A_air = m->A_air;
  M.A_ice = m->A_ice;
  M.B_ice = m->B_ice;
  M.negC_ice = -m->C_ice;
  M.d2r = pi / 180.0;
  M.r2d = 180 / pi;
  M.ml = m->max_layers;
  if (variant == AIRICE_VARIANT_PYWRAPPER && m->constant_air_index) {
    // UseConstantRefractiveIndex (pythonwrapper AirIceRayTracing.cc:173-238): GetB_air = 0,
    // GetC_air = 1e-9 in every layer; Getnz_air = A_const, which A_air + 0*exp() reproduces
    // exactly while A_const == A_air (both 1.00, .h:69-72)
    if (m->A_const != m->A_air) {
      set_error("constant air index: A_const (%g) != A_air (%g) is not supported", m->A_const,
                m->A_air);
      return AIRICE_EINVAL;
    }
    for (int i = 0; i < 5; ++i) {
      M.B[i] = 0;
      M.negC[i] = -1e-9;
    }
    M.const_air = 1;
  }
  for (int l = 0; l < kMaxLayers; ++l) {
    M.start[l] = host_air_endpoint(M, M.atm[l + 1] - 0.00001);
    M.stop[l] = host_air_endpoint(M, M.atm[l]);
  }
  return AIRICE_OK;
}

void build_ice_consts(const DevMedium& M, double ice_h, double rx_depth, IceConsts* out) {
  std::memset(out, 0, sizeof(*out));
  out->ice_h = ice_h;
  out->ice_air = host_air_endpoint(M, ice_h);
  out->ice0 = host_ice_endpoint(M, 0.0);
  out->ice_rx = host_ice_endpoint(M, rx_depth);
  out->n_air_ice = out->ice_air.n;
  out->n_ice0 = out->ice0.n;
  out->n_ratio = out->n_air_ice / out->n_ice0;
  // lowest air layer: SkipLayersBelow scan (.cc:1815-1825)
  int bot = 0;
  for (int il = 0; il < M.ml; ++il) {
    if (ice_h >= M.atm[il] && ice_h < M.atm[il + 1]) break;
    ++bot;
  }
  out->bot = bot;
  for (int l = 0; l < kMaxLayers; ++l) {
    const Endpoint& T = M.start[l];
    Endpoint R = (l == bot) ? out->ice_air : M.stop[l];
    out->topend[l] = make_topend(R);
    if (R.x == T.x) R = T;  // zero-length segment: the same function of the same x
    out->lower[l] = make_segconst(T, R);
  }
  Endpoint rx = out->ice_rx;
  if (rx.x == out->ice0.x) rx = out->ice0;
  out->iceseg = make_segconst(out->ice0, rx);
}

// ---- two-layer firn ---------------------------------------------------------
int firn_check(const char* who, const airice_firn* f) {
  if (f == nullptr) {
    set_error("%s: null argument (firn)", who);
    return AIRICE_EINVAL;
  }
  if (!std::isfinite(f->boundary_m) || !(f->boundary_m > 0)) {
    set_error("%s: firn boundary_m (%g) must be finite and > 0", who, f->boundary_m);
    return AIRICE_EINVAL;
  }
  for (int l = 0; l < 2; ++l)
    if (!std::isfinite(f->B[l]) || !std::isfinite(f->C[l]) || !(f->C[l] > 0)) {
      set_error("%s: firn layer %d: B (%g) must be finite, C (%g) finite and > 0", who, l,
                f->B[l], f->C[l]);
      return AIRICE_EINVAL;
    }
  return AIRICE_OK;
}

airice_medium firn_layer_medium(const airice_medium& m, const airice_firn& f, int layer) {
  airice_medium u = m;
  u.B_ice = f.B[layer];
  u.C_ice = f.C[layer];
  return u;
}

double firn_clip_depth(const airice_firn& f, double rx_depth) {
  return rx_depth > f.boundary_m ? f.boundary_m : rx_depth;
}

void build_firn_leg(const DevMedium& M, const airice_firn& f, double rx_depth, FirnLeg* out) {
  std::memset(out, 0, sizeof(*out));
  DevMedium L = M;  // host_ice_endpoint reads A_ice, B_ice and negC_ice only
  L.B_ice = f.B[1];
  L.negC_ice = -f.C[1];
  const Endpoint T = host_ice_endpoint(L, f.boundary_m);
  out->below = rx_depth > f.boundary_m;
  // an antenna at or above the boundary has no lower leg: a zero-length segment, never traced
  out->seg = make_segconst(T, out->below ? host_ice_endpoint(L, rx_depth) : T);
  out->ratio_b = host_ice_endpoint(M, f.boundary_m).n / T.n;
}

void rays_host_firn(const DevMedium& M, const IceConsts& I, const FirnLeg& F, const double* launch,
                    const double* txh, int in_ice, size_t n, double* out, size_t ld) {
  for (size_t k = 0; k < n; ++k) {
    double d[18];
    ray_solution(M, I, launch[k], txh[k], in_ice != 0, d, true, &F);
    for (int c = 0; c < 18; ++c) out[c * ld + k] = d[c];
  }
}

}  // namespace airice
