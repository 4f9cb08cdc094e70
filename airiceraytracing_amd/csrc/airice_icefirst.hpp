// airice_icefirst.hpp -- the reference's first-arriving ray between two 3-D points
// (IceRayTracing::DirectRayTracer, IceRayTracing.cc:2502-2612): the geometry it forms for the
// solver and the choice it makes among the solver's rays, written once for the device
// (icefirst_geom_kernel, icefirst_select_kernel; airice_icefirst.hip) and the host
// (icefirst_host_one, airice_host.cpp; the drop-in's DirectRayTracer).  The solve between the two
// is airice_iceray.hpp's solve_pair, untouched.
#pragma once
#include "airice_iceray.hpp"

namespace airice {
namespace icefirst {

constexpr int kFields = 8;  // AIRICE_ICEFIRST_FIELDS
constexpr int kColLang = 0, kColRang = 1, kColPath = 2, kColTimeC = 3, kColTime = 4;
constexpr int kColType = 5, kColX1 = 6, kColStatus = 7;
constexpr int kWorkDoubles = 3 + iceray::kColumns;  // per pair: z0, x1, z1, the solver's row
constexpr double kNoRay = -1000.0;

// x1 = sqrt(pow(xT - xR, 2) + pow(yT - yR, 2)) (.cc:2511): two products, one sum and the correctly
// rounded root, each rounded on its own -- no fused multiply-add -- so that it is numpy's
// np.sqrt(dx*dx + dy*dy) bit for bit.  (pow(d, 2) is d*d exactly.)
AIRICE_IR_HD inline double horizontal_distance(double xT, double yT, double xR, double yR) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dx = xT - xR, dy = yT - yR;
  const double dx2 = dx * dx, dy2 = dy * dy;
  return sqrt(dx2 + dy2);
}

// The choice (.cc:2537-2598) over one row of the solver: ray(c) reads its column c.  Candidates in
// the order D, Ra0, Ra1 -- those whose receive-angle column (8, 10, 11) is not -1000; the reflected
// ray is never one.  MinValueBin starts at 0 and min at 1e9, and a candidate takes over only when
// its time*c is < min: the first candidate stands unless a later one is strictly earlier, and also
// when no time*c is below 1e9.  No candidate: the five values are -1000.  A row the solver flagged
// non-finite is NaN in the five values with type 0.  put(column, value) receives the kFields
// columns; returns the solver's status byte.
template <class Ray, class Put>
AIRICE_IR_HD inline uint8_t select_first(Ray&& ray, double x1, Put&& put) {
  const uint8_t status = (uint8_t)ray(iceray::kColStatus);
  put(kColX1, x1);
  put(kColStatus, (double)status);
  if (status & iceray::kNonFinite) {
    for (int c = kColLang; c <= kColTime; c++) put(c, iceray::quiet_nan());
    put(kColType, 0.0);
    return status;
  }
  int winner = -1;
  double min = 1e9, winner_tc = 0;
  AIRICE_IR_NOUNROLL
  for (int k = 0; k < 3; k++) {
    const int r = k == 0 ? 0 : k + 1;  // the solver's ray: 0 D, 2 Ra0, 3 Ra1
    if (!(ray(8 + r) != kNoRay)) continue;
    const double tc = ray(4 + r) * iceray::kSpeedC;
    if (winner < 0 || tc < min) {
      if (tc < min) min = tc;
      winner = r;
      winner_tc = tc;
    }
  }
  if (winner < 0) {
    for (int c = kColLang; c <= kColTime; c++) put(c, kNoRay);
    put(kColType, 0.0);
    return status;
  }
  put(kColLang, ray(0 + winner));
  put(kColRang, ray(8 + winner));
  put(kColPath, ray(25 + winner));
  put(kColTimeC, winner_tc);
  put(kColTime, ray(4 + winner));
  put(kColType, (double)(winner + 1));  // icesol's codes: 1 D, 3 Ra0, 4 Ra1
  return status;
}

}  // namespace icefirst
}  // namespace airice
