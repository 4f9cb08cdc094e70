// firn_driver.cpp -- the host code of the two-layer firn (airice_fold.cpp: firn_check, the upper
// layer's medium, build_firn_leg, rays_host_firn) as a stand-alone program; `make firn_driver_asan`
// builds it with the host compiler under ASan + UBSan (no device code, no HIP call).
//
// It traces a fan of rays through the Summit firn from a hand-made four-layer atmosphere and
// checks what needs no reference: every invalid firn is refused, an antenna 1 um below the
// boundary continues the upper layer's ray, two equal layers add up to the one-layer ray, and the
// results are finite.  Prints "firn_driver ok" and returns 0, else says what failed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "airice.h"
#include "airice_internal.h"
#include "airice_ray.hpp"

using namespace airice;

static int g_failed = 0;
#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                   \
    }                                                               \
  } while (0)

static airice_medium test_medium() {
  airice_medium m;
  std::memset(&m, 0, sizeof(m));
  const double atm[5] = {0.0, 4.0e5, 1.0e6, 4.0e6, 1.5e7};  // cm
  const double B[5] = {3.1e-4, 2.9e-4, 2.6e-4, 2.2e-4, 2.2e-4};
  const double C[5] = {1.1e-4, 1.2e-4, 1.35e-4, 1.5e-4, 1.5e-4};
  for (int i = 0; i < 5; ++i) {
    m.atmlay_cm[i] = atm[i];
    m.B_air[i] = B[i];
    m.C_air[i] = C[i];
  }
  m.max_layers = 4;
  m.A_air = 1.0;
  m.A_ice = 1.775;
  m.B_ice = -0.43;
  m.C_ice = 0.0132;
  m.pi = 3.1415927;
  m.A_const = 1.0;
  return m;
}

// the rays of one antenna depth (m, negative) in firn f; one-layer when f is null
static std::vector<double> trace(const airice_medium& m, const airice_firn* f, double ice_h,
                                 double depth_m, const std::vector<double>& launch,
                                 const std::vector<double>& txh) {
  const size_t n = launch.size();
  std::vector<double> out(18 * n, -1.0);
  DevMedium M;
  IceConsts I;
  const airice_medium up = f != nullptr ? firn_layer_medium(m, *f, 0) : m;
  EXPECT(build_dev_medium(&up, AIRICE_VARIANT_MULTIRAY, &M) == AIRICE_OK);
  if (f == nullptr) {
    build_ice_consts(M, ice_h, -depth_m, &I);
    for (size_t k = 0; k < n; ++k) {
      double d[18];
      ray_solution(M, I, launch[k], txh[k], true, d);
      for (int c = 0; c < 18; ++c) out[c * n + k] = d[c];
    }
    return out;
  }
  build_ice_consts(M, ice_h, firn_clip_depth(*f, -depth_m), &I);
  FirnLeg F;
  build_firn_leg(M, *f, -depth_m, &F);
  EXPECT(F.below == (-depth_m > f->boundary_m));
  rays_host_firn(M, I, F, launch.data(), txh.data(), 1, n, out.data(), n);
  return out;
}

static double rel(double a, double b) {
  return std::fabs(a - b) / std::fmax(std::fabs(b), 1e-6);
}

int main() {
  const airice_firn summit = AIRICE_FIRN_SUMMIT;
  EXPECT(firn_check("driver", &summit) == AIRICE_OK);
  EXPECT(firn_check("driver", nullptr) == AIRICE_EINVAL);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double inf = std::numeric_limits<double>::infinity();
  for (double bad : {0.0, -14.9, nan, inf}) {
    airice_firn f = summit;
    f.boundary_m = bad;
    EXPECT(firn_check("driver", &f) == AIRICE_EINVAL);
  }
  for (int l = 0; l < 2; ++l) {
    for (double bad : {nan, inf, -inf}) {
      airice_firn f = summit;
      f.B[l] = bad;
      EXPECT(firn_check("driver", &f) == AIRICE_EINVAL);
    }
    for (double bad : {0.0, -0.02, nan, inf}) {
      airice_firn f = summit;
      f.C[l] = bad;
      EXPECT(firn_check("driver", &f) == AIRICE_EINVAL);
    }
  }
  EXPECT(std::strstr(airice_last_error(), "firn") != nullptr);

  const airice_medium m = test_medium();
  const double ice_h = 3216.0;
  std::vector<double> launch, txh;
  for (int i = 0; i < 300; ++i) {
    launch.push_back(100.0 + 80.0 * i / 299.0);
    txh.push_back(ice_h + 1.0 + 300.0 * i);
  }
  const size_t n = launch.size();
  const int ice_cols[5] = {4, 7, 10, 13, 17};

  // finite, and the ice leg grows with the depth
  const std::vector<double> at100 = trace(m, &summit, ice_h, -100.0, launch, txh);
  const std::vector<double> at200 = trace(m, &summit, ice_h, -200.0, launch, txh);
  for (size_t k = 0; k < n; ++k) {
    for (int c = 0; c < 18; ++c) EXPECT(std::isfinite(at100[c * n + k]));
    EXPECT(at200[7 * n + k] > at100[7 * n + k]);
    EXPECT(at200[17 * n + k] > at100[17 * n + k]);
  }
  // 1 um below the boundary: the upper layer's ray to the boundary plus 1 um of path
  const std::vector<double> below = trace(m, &summit, ice_h, -(summit.boundary_m + 1e-6), launch, txh);
  const std::vector<double> at_b = trace(m, &summit, ice_h, -summit.boundary_m, launch, txh);
  for (size_t k = 0; k < n; ++k) {
    EXPECT(std::fabs(below[7 * n + k] - at_b[7 * n + k]) < 1e-5);
    EXPECT(std::fabs(below[17 * n + k] - at_b[17 * n + k]) < 1e-5);
    EXPECT(std::fabs(below[4 * n + k] - at_b[4 * n + k]) < 1e-5);
  }
  // at the boundary the layered call is the one-layer ray of the upper model, bit for bit
  const airice_medium up = firn_layer_medium(m, summit, 0);
  const std::vector<double> one_b = trace(up, nullptr, ice_h, -summit.boundary_m, launch, txh);
  EXPECT(std::memcmp(at_b.data(), one_b.data(), sizeof(double) * at_b.size()) == 0);
  // equal layers: the two legs add up to the one-layer ray
  const airice_firn equal = {14.9, {m.B_ice, m.B_ice}, {m.C_ice, m.C_ice}};
  const std::vector<double> two = trace(m, &equal, ice_h, -150.0, launch, txh);
  const std::vector<double> one = trace(m, nullptr, ice_h, -150.0, launch, txh);
  double worst = 0;
  for (size_t k = 0; k < n; ++k)
    for (int c : ice_cols) worst = std::fmax(worst, rel(two[c * n + k], one[c * n + k]));
  EXPECT(worst <= 1e-9);
  std::printf("equal layers: max rel %.3e\n", worst);
  // no rays at all
  rays_host_firn(DevMedium{}, IceConsts{}, FirnLeg{}, nullptr, nullptr, 1, 0, nullptr, 0);

  if (g_failed) {
    std::printf("firn_driver: %d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("firn_driver ok\n");
  return 0;
}
