// airice_iceair.hpp -- the reference's ice-to-air direct ray (IceRayTracing.cc:2358-2500: fDa_Air,
// GetDirectRayPar_Air): from a transmitter at depth z0 in the firn to a receiver x1 metres away
// and h metres ABOVE the surface, refracting in the ice and straight in the air at n = 1.  Written
// once for the device (iceair_kernel, airice_iceair.hip) and the host (iceair_host_one,
// airice_host.cpp; the drop-in's fDa_Air / GetDirectRayPar_Air, compat_iceray.cpp).
//
// The model, fDnfR_L, ftimeD and fpathD are airice_iceray.hpp's.  The false-position search is a
// SECOND COPY of that header's falsepos (the same GSL semantics, statement by statement), taking
// the residual as a functor: iceray's is tied to its Pair and its three residuals, and changing it
// would change the text every existing in-ice kernel compiles.
// TransitionBoundary is 0 as there: none of its branches is carried.
#pragma once
#include "airice_iceray.hpp"

namespace airice {
namespace iceair {

using iceray::IceModel;
using iceray::Root;

constexpr int kFields = 10;  // AIRICE_ICEAIR_FIELDS
constexpr int kColRang = 0, kColLang = 1, kColTime = 2, kColL = 3, kColCheckzero = 4;
constexpr int kColStatus = 5, kColEvals = 6, kColIters = 7, kColPhysTime = 8, kColPath = 9;
constexpr int kAccepted = 1;     // status: |checkzero| <= 0.5
constexpr int kNonFinite = 128;  // status: a NaN or infinite input

// One (Tx depth, distance, Rx height) triple: what fDa_Air reads that does not depend on L, and the
// count of residual evaluations.
struct Triple {
  IceModel m;
  double z0, x1, h;
  double n0, ns;  // Getnz(z0), Getnz(1e-7)
  int evals;
};

AIRICE_IR_HD inline Triple make_triple(const IceModel& m, double z0, double x1, double h) {
  Triple t;
  t.m = m;
  t.z0 = z0;
  t.x1 = x1;
  t.h = h;
  t.n0 = iceray::nz(m, z0);
  t.ns = iceray::nz(m, iceray::kSurface);
  t.evals = 0;
  return t;
}

// fDa_Air (.cc:2358-2408) at L = x: the ice leg from z0 up to the surface (-1e-7), the air leg
// h tan(asin(L / 1)), minus the distance.  A NaN air term (L > 1, where asin has no value) is 1e9,
// which keeps the residual finite on (1, n(1e-7)]; the NaN rule on the ice term is commented out in
// the reference and stays out.
AIRICE_IR_HD inline double residual(Triple& t, double x) {
  t.evals++;
  const double nz_air = 1;
  const double angle_in_air = asin(x / nz_air);
  double x1_air = t.h * tan(angle_in_air);
  const double d = iceray::fDnfR_L(t.m, x, t.m.C, -iceray::kSurface, t.ns) -
                   iceray::fDnfR_L(t.m, x, t.m.C, t.z0, t.n0);
  if (iceray::is_nan(x1_air)) x1_air = 1e9;
  return d + x1_air - t.x1;
}

// FindFunctionRoot (.cc:261-300) over gsl_root_fsolver_falsepos: iceray::falsepos with f(x) for
// residual(p, kind, x) and not one statement else changed -- the end values kept even when they do
// not straddle, GSL's comparison orientation, SAFE_FUNC_CALL (a non-finite trial value ends the
// step before any update; the search then ends with the reference's count, 100), a non-finite end
// value ends it at the bracket midpoint, x_lo > x_hi gives NaN, and the value at a root the step
// just evaluated is reused.  Stop: |f| < 1e-6 or 100 iterations.
template <class F>
AIRICE_IR_HD inline Root falsepos(F&& f, double x_lo, double x_hi) {
  Root R;
  R.iters = 0;
  if (x_lo > x_hi) {
    R.r = R.fr = iceray::quiet_nan();
    return R;
  }
  double root = 0.5 * (x_lo + x_hi);
  double f_lower = 0, f_upper = 0;
  bool set_ok = true;
  AIRICE_IR_NOUNROLL
  for (int k = 0; k < 2 && set_ok; k++) {  // the set call: f at the two ends
    const double v = f(k == 0 ? x_lo : x_hi);
    if (k == 0) f_lower = v;
    else f_upper = v;
    set_ok = iceray::is_finite(v);
  }
  double fr = 0;
  bool have_fr = false;
  int iter = 0;
  for (;;) {
    bool stuck = !set_ok;
    if (set_ok) {
      iter++;
      const double x_left = x_lo, x_right = x_hi;
      const double fl = f_lower, fu = f_upper;
      if (fl == 0.0) {
        root = x_left;
        x_hi = x_left;
        fr = fl;
        have_fr = true;
      } else if (fu == 0.0) {
        root = x_right;
        x_lo = x_right;
        fr = fu;
        have_fr = true;
      } else {
        const double x_linear = x_right - (fu * (x_left - x_right) / (fl - fu));
        const double f_linear = f(x_linear);
        if (!iceray::is_finite(f_linear)) {
          stuck = true;
        } else if (f_linear == 0.0) {
          root = x_linear;
          x_lo = x_linear;
          x_hi = x_linear;
          fr = f_linear;
          have_fr = true;
        } else {
          double w;
          root = x_linear;
          fr = f_linear;
          have_fr = true;
          if ((fl > 0.0 && f_linear < 0.0) || (fl < 0.0 && f_linear > 0.0)) {
            x_hi = x_linear;
            f_upper = f_linear;
            w = x_linear - x_left;
          } else {
            x_lo = x_linear;
            f_lower = f_linear;
            w = x_right - x_linear;
          }
          if (!(w < 0.5 * (x_right - x_left))) {  // the linear step shrank it by less than half
            const double x_bisect = 0.5 * (x_left + x_right);
            const double f_bisect = f(x_bisect);
            if (!iceray::is_finite(f_bisect)) {
              // the step returns here: the linear update stays
            } else if ((fl > 0.0 && f_bisect < 0.0) || (fl < 0.0 && f_bisect > 0.0)) {
              x_hi = x_bisect;
              f_upper = f_bisect;
              if (root > x_bisect) {
                root = 0.5 * (x_left + x_bisect);
                have_fr = false;
              }
            } else {
              x_lo = x_bisect;
              f_lower = f_bisect;
              if (root < x_bisect) {
                root = 0.5 * (x_bisect + x_right);
                have_fr = false;
              }
            }
          }
        }
      }
    }
    if (!have_fr) {
      fr = f(root);
      have_fr = true;
    }
    if (fabs(fr) < 1e-6) break;  // gsl_root_test_residual
    if (stuck) iter = 100;
    if (iter >= 100) break;
  }
  R.r = root;
  R.fr = fr;
  R.iters = iter;
  return R;
}

// GetDirectRayPar_Air (.cc:2411-2500) for one triple: out.put(column, value) receives each of the
// kFields columns as soon as it is final; returns the status byte.
//   0-4  the reference's output[0..4]: receive angle in air (deg; -1000 when |checkzero| > 0.5),
//        launch angle (deg), time (s), L, checkzero
//   5-7  status as a double, residual evaluations, false-position iterations
//   8-9  extensions: the physical time and the geometric path
// The ice leg's time is ftimeD(-z0) - ftimeD(1e-7) at -C in the reference: here the (z, +C) form,
// its exact negative, taken the other way round, as iceray's direct ray (the same bits).  The
// receive angle in ice is asin(L / n(1e-7)) where the reference takes atan of a gsl_deriv_central
// slope (DESIGN.md §8's analytic angles); its two NaN fallbacks stay as written -- degrees used as
// radians -- and can fire only for a NaN L.  The reference's time adds the air leg's HORIZONTAL
// distance over c (.cc:2483-2486): column 2 keeps that; column 8 has the air leg's length,
// h / cos(air angle), over c, column 9 the path with the same leg.
// One more departure, of the kind of §8's third: the air angle's tangent and cosine are taken from
// its sine, which is L (Snell), as L / sqrt((1 - L)(1 + L)) and sqrt((1 - L)(1 + L)).  The
// reference's tan(asin(n sin(asin(L / n)))) goes through a rounded angle next to 90 degrees and
// loses 1 / (1 - L^2) ulps at a grazing exit: up to 1e-8 of the time in the test draw, ten times
// the project's parity bound between two libms, and 27 times the physics bound.
// Column 0 is that rounded angle in degrees, where the loss is below 1e-11 relative.
template <class Out>
AIRICE_IR_HD inline uint8_t solve_triple(const IceModel& m, double z0, double x1, double h,
                                         Out&& out) {
  if (!(iceray::is_finite(z0) && iceray::is_finite(x1) && iceray::is_finite(h))) {
    for (int c = 0; c <= kColCheckzero; c++) out.put(c, iceray::quiet_nan());
    out.put(kColStatus, (double)kNonFinite);
    out.put(kColEvals, 0.0);
    out.put(kColIters, 0.0);
    out.put(kColPhysTime, iceray::quiet_nan());
    out.put(kColPath, iceray::quiet_nan());
    return (uint8_t)kNonFinite;
  }
  Triple t = make_triple(m, z0, x1, h);
  double hi = t.ns;  // min_element({Getnz(1e-7), Getnz(z0)})
  if (t.n0 < hi) hi = t.n0;
  const Root S = falsepos([&t](double x) { return residual(t, x); }, 1e-7, hi);
  const double L = S.r, cz = S.fr;
  const double lang = asin(L / t.n0) * iceray::kDeg;
  const int status = fabs(cz) <= 0.5 ? kAccepted : 0;
  out.put(kColLang, lang);
  out.put(kColL, L);
  out.put(kColCheckzero, cz);
  out.put(kColStatus, (double)status);
  out.put(kColEvals, (double)t.evals);
  out.put(kColIters, (double)S.iters);

  const double zs = -iceray::kSurface;
  const double time_ice = iceray::ftimeD(m, zs, m.C, t.ns, L) - iceray::ftimeD(m, z0, m.C, t.n0, L);
  double rang = asin(L / t.ns);  // radians, as the reference's atan(result)
  if (h == z0 && iceray::is_nan(rang)) rang = 180 - lang;  // .cc:2473-2480, as written
  if (h != z0 && iceray::is_nan(rang)) rang = 90;
  const double air_angle = asin(t.ns * sin(rang));
  out.put(kColRang, fabs(cz) > 0.5 ? -1000.0 : air_angle * iceray::kDeg);
  const double cos_air = sqrt((1 - L) * (1 + L));  // of the angle whose sine is L
  const double air_horizontal = (L / cos_air) * h;  // tan(air angle) h
  out.put(kColTime, time_ice + air_horizontal / iceray::kSpeedC);
  out.put(kColPhysTime, time_ice + h / (iceray::kSpeedC * cos_air));
  const double path_ice =
      iceray::fpathD_q(m, zs, m.C, exp(m.C * zs), t.ns, t.ns * t.ns - L * L, L) -
      iceray::fpathD_q(m, z0, m.C, exp(m.C * z0), t.n0, t.n0 * t.n0 - L * L, L);
  out.put(kColPath, path_ice + h / cos_air);
  return (uint8_t)status;
}

}  // namespace iceair
}  // namespace airice
