// airice_iceray.hpp -- the in-ice ray solver of the reference (IceRayTracing.cc: the direct,
// reflected and refracted rays between a transmitter and a receiver that are both in the firn),
// written once for the device (iceray_kernel, airice_iceray.hip) and the host (iceray_host_one,
// airice_host.cpp; the IceRayTracing:: drop-in, compat_iceray.cpp).
//
// IceRayTracing::TransitionBoundary is a constexpr 0 (.hh:55): GetB / GetC are the model's B and C
// at every depth and every `TransitionBoundary != 0` branch of the reference is dead; none is
// carried here.  What is restated: Getnz (.cc:56), fDnfR_L (.cc:368), ftimeD (.cc:382), fpathD
// (.cc:395), the residuals fDa / fRa / fRaa (.cc:411, 471, 543), FindFunctionRoot over GSL's
// false-position solver (.cc:261, roots/falsepos.c), FindFunctionRootFDF over GSL's Newton solver
// with gsl_deriv_central slopes (.cc:222, roots/newton.c, deriv/deriv.c), GetDirectRayPar (.cc:626),
// GetReflectedRayPar (.cc:745), GetRefractedRayPar (.cc:923) and IceRayTracing (.cc:1745).
// The three departures (closed-form turning depth, analytic angles, the index below a turning
// depth without cancellation) are in DESIGN.md §8.
//
// Shape: the nine searches a pair can need (direct, reflected, the refracted ray's first false
// position and Newton tries, its five second-root attempts) and the four rays' closing
// arithmetic are rows of ONE loop (run_stages), so the false-position solver, the Newton solver
// and the ray's time / path legs each exist once in the kernel, and the lanes of a wave meet
// again at every row whatever their pairs needed.
#pragma once
#include <math.h>

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AIRICE_IR_HD __host__ __device__
#else
#define AIRICE_IR_HD
#endif
#if defined(__clang__)
#define AIRICE_IR_NOUNROLL _Pragma("nounroll")
#elif defined(__GNUC__)
#define AIRICE_IR_NOUNROLL _Pragma("GCC unroll 1")
#else
#define AIRICE_IR_NOUNROLL
#endif

namespace airice {
namespace iceray {

constexpr double kPi = 3.14159265359;        // IceRayTracing.hh:47
constexpr double kSpeedC = 299792458.0;      // c_light_ms, .hh:49
constexpr double kDeg = 180.0 / kPi;         // the reference's (180.0/pi)
constexpr double kSurface = 1e-7;            // the depth the reference takes for the surface
constexpr double kNoTurn = -1000.0;          // zmax_of: the reference's bracket holds no root
constexpr int kFields = 29;                  // IceRayTracing's output[0..28] (.cc:1862-1902)
constexpr int kColumns = 32;                 // + status, f evaluations, direct-search iterations
constexpr int kColStatus = 29, kColEvals = 30, kColIters = 31;
constexpr int kNonFinite = 128;              // status: a NaN or infinite input (bits 0-3: rays)

struct IceModel {
  double A, B, C;  // n(z) = A + B exp(-C |z|); SetA / SetB / SetC
};
constexpr IceModel kDefaultModel = {1.78, -0.43, 0.0132};  // .hh:52-54

AIRICE_IR_HD inline bool is_nan(double x) { return x != x; }
AIRICE_IR_HD inline bool is_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }
AIRICE_IR_HD inline double quiet_nan() { return 0.0 * HUGE_VAL; }

// Getnz (.cc:56-59)
AIRICE_IR_HD inline double nz(const IceModel& m, double z) {
  z = fabs(z);
  return m.A + m.B * exp(-m.C * z);
}

// GetZmax (.cc:346-353): the depth at which n(z) = L.  The reference searches
// A + B e^{-Cz} - L on [0, 5000] by false position to 1e-6 inside every fRaa; the root is
// ln(B / (L - A)) / C.  Where that bracket holds no root (L >= A or L <= A + B) the value returned
// makes fRaa take its `zmax <= 0` branch (1e9) and the ray fail the zmax test of .cc:1083.
AIRICE_IR_HD inline double zmax_of(const IceModel& m, double L) {
  if (L >= m.A || L <= m.A + m.B) return kNoTurn;
  return log(m.B / (L - m.A)) / m.C;
}

// fDnfR_L (.cc:368-379) at depth parameter Z with index n = Getnz(Z): x is the L parameter
AIRICE_IR_HD inline double fDnfR_L(const IceModel& m, double x, double Cp, double Z, double n) {
  return (x / Cp) * (1.0 / sqrt(m.A * m.A - x * x)) *
         (Cp * Z - log(m.A * n - x * x + sqrt(m.A * m.A - x * x) * sqrt(n * n - x * x)));
}

// The index just below a refracted ray's turning depth, n(zmax + 1e-7) - L, where n(zmax) = L:
// (L - A) expm1(-C 1e-7), with no cancellation.  The reference forms n(zmax + 1e-7) and then
// n^2 - L^2, a difference of two numbers that agree to 1e-10: the rounding of exp and log then
// decides the seventh digit of sqrt(n^2 - L^2), and with it the tenth digit of the root L and the
// eighth of a short leg's time (the third departure of DESIGN.md §8).
AIRICE_IR_HD inline double top_gap(const IceModel& m, double L) {
  return (L - m.A) * expm1(-m.C * 1e-7);
}

// ftimeD (.cc:382-392) with n = Getnz(x) and q2 = n^2 - L^2
AIRICE_IR_HD inline double ftimeD_q(const IceModel& m, double x, double Cp, double n, double q2,
                                    double L, double speedc) {
  const double q = sqrt(q2), sA = sqrt(m.A * m.A - L * L);
  return (1.0 / (speedc * Cp * q)) *
         (q2 + (Cp * x - log(m.A * n - L * L + sA * q)) * (m.A * m.A * q) / sA +
          m.A * q * log(n + q));
}
AIRICE_IR_HD inline double ftimeD(const IceModel& m, double x, double Cp, double n, double L,
                                  double speedc = kSpeedC) {
  return ftimeD_q(m, x, Cp, n, n * n - L * L, L, speedc);
}

// fpathD (.cc:395-408) with e = exp(C x), nx = A + B e and q2 = nx^2 - L^2 (which the reference
// writes out as A^2 + 2 A B e + B^2 exp(2 C x) - L^2)
AIRICE_IR_HD inline double fpathD_q(const IceModel& m, double x, double Cp, double e, double nx,
                                    double q2, double L) {
  const double A = m.A, B = m.B;
  const double sA = sqrt(A * A - L * L);
  const double q = sqrt(q2 / (nx * nx));
  return (log(nx * (q + 1)) -
          (A * log(A * sA * q + B * sA * e * q + A * A + A * B * e - L * L)) / sA +
          (A * Cp * x) / sA) / Cp;
}
AIRICE_IR_HD inline double fpathD(const IceModel& m, double x, double Cp, double L) {
  const double A = m.A, B = m.B;
  const double e = exp(Cp * x), e2 = exp(2 * Cp * x);
  return fpathD_q(m, x, Cp, e, A + B * e, A * A + 2 * A * B * e + B * B * e2 - L * L, L);
}

// One (Tx, Rx) pair with the Tx below the Rx (the reference's flip applied): what its residuals
// read that does not depend on L, and the count of residual evaluations.
struct Pair {
  IceModel m;
  double z0, z1, x1;   // z0 <= z1 unless one is NaN
  double n0, n1, ns;   // Getnz(z0), Getnz(z1), Getnz(1e-7)
  int evals;
};

AIRICE_IR_HD inline Pair make_ray_pair(const IceModel& m, double z0, double x1, double z1,
                                       bool* flip) {
  Pair p;
  p.m = m;
  *flip = false;
  if (z0 > z1) {  // .cc:631-637
    const double dsw = z0;
    z0 = z1;
    z1 = dsw;
    *flip = true;
  }
  p.z0 = z0;
  p.z1 = z1;
  p.x1 = x1;
  p.n0 = nz(m, z0);
  p.n1 = nz(m, z1);
  p.ns = nz(m, kSurface);
  p.evals = 0;
  return p;
}

enum Residual { kFDa = 0, kFRa = 1, kFRaa = 2 };

// fDa (.cc:411-452), fRa (.cc:471-524) and fRaa (.cc:543-607) at L = x.  A^2 - L^2 and its root
// are taken once; the two end terms are shared by the three residuals.
AIRICE_IR_HD inline double residual(Pair& p, int kind, double x) {
  const IceModel& m = p.m;
  p.evals++;
  double zt = kSurface, nt = p.ns;
  const double L2 = x * x;
  double qt2 = nt * nt - L2;  // n^2 - L^2 at the top of the ray
  if (kind == kFRaa) {
    zt = zmax_of(m, x) + 1e-7;
    if (!(zt > 0)) return 1e9;
    const double gap = top_gap(m, x);
    nt = x + gap;
    qt2 = gap * (nt + x);
  }
  const double s = sqrt(m.A * m.A - L2);
  const double lg0 = log(m.A * p.n0 - L2 + s * sqrt(p.n0 * p.n0 - L2));
  const double lg1 = log(m.A * p.n1 - L2 + s * sqrt(p.n1 * p.n1 - L2));
  if (kind == kFDa) {
    const double pre = (x / m.C) * (1.0 / s);
    const double d01 = pre * (m.C * p.z1 - lg1) - pre * (m.C * p.z0 - lg0);
    return d01 - p.x1;
  }
  const double nC = -m.C;
  const double pre = (x / nC) * (1.0 / s);
  const double t0 = pre * (nC * -p.z0 - lg0);
  const double t1 = pre * (nC * -p.z1 - lg1);
  const double lgt = log(m.A * nt - L2 + s * sqrt(qt2));
  const double ts = pre * (nC * zt - lgt);
  double d01 = t1 - t0;
  double d0s = ts - t0;
  if (kind == kFRaa) {  // .cc:596-601
    if (is_nan(d01)) d01 = 1e9;
    if (is_nan(d0s)) d0s = 1e9;
  }
  return d01 - 2 * d0s - p.x1;
}

struct Root {
  double r, fr;  // the root estimate and the residual there
  int iters;
};

// FindFunctionRoot (.cc:261-300): gsl_root_fsolver_falsepos with the error handler off, iterated
// until |f(r)| < 1e-6 or 100 iterations.  GSL 2.x semantics (roots/falsepos.c, roots.h):
//   - the end values are stored even when they do not straddle zero (the set call's error is
//     ignored and the reference iterates anyway);
//   - every comparison keeps GSL's orientation, so a NaN takes the branch it takes in C;
//   - a non-finite value at a trial point makes the step return before it updates anything
//     (SAFE_FUNC_CALL).  After such a linear step nothing has changed, the remaining iterations
//     would repeat it, and the loop ends here with the count the reference reaches (100);
//   - a non-finite END value makes the set call return before it stores the values, and the
//     reference then iterates on uninitialised state; here the search ends at the bracket
//     midpoint, the root estimate the set call left.  x_lo > x_hi leaves the reference's solver
//     without a function (it would dereference null); here the root is NaN.
// Where r is the point the step just evaluated its value is reused, not computed again.
AIRICE_IR_HD inline Root falsepos(Pair& p, int kind, double x_lo, double x_hi) {
  Root R;
  R.iters = 0;
  if (x_lo > x_hi) {
    R.r = R.fr = quiet_nan();
    return R;
  }
  double root = 0.5 * (x_lo + x_hi);
  double f_lower = 0, f_upper = 0;
  bool set_ok = true;
  AIRICE_IR_NOUNROLL
  for (int k = 0; k < 2 && set_ok; k++) {  // the set call: f at the two ends
    const double v = residual(p, kind, k == 0 ? x_lo : x_hi);
    if (k == 0) f_lower = v;
    else f_upper = v;
    set_ok = is_finite(v);
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
        const double f_linear = residual(p, kind, x_linear);
        if (!is_finite(f_linear)) {
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
            const double f_bisect = residual(p, kind, x_bisect);
            if (!is_finite(f_bisect)) {
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
      fr = residual(p, kind, root);
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

// gsl_deriv_central (deriv/deriv.c): the 5-point rule (x-h, x-h/2, x+h/2, x+h) at h, and once more
// at the step that its own error estimate calls optimal, kept when it is consistent with the
// first.
AIRICE_IR_HD inline double deriv_central(Pair& p, int kind, double x, double h) {
  const double kEps = 2.2204460492503131e-16;  // GSL_DBL_EPSILON
  double r_0 = 0, error = 0;
  AIRICE_IR_NOUNROLL
  for (int pass = 0; pass < 2; pass++) {
    double fm1 = 0, fp1 = 0, fmh = 0, fph = 0;
    AIRICE_IR_NOUNROLL
    for (int k = 0; k < 4; k++) {  // GSL's order: x-h, x+h, x-h/2, x+h/2
      const double dx = k < 2 ? h : h / 2;
      const double v = residual(p, kind, (k & 1) ? x + dx : x - dx);
      if (k == 0) fm1 = v;
      else if (k == 1) fp1 = v;
      else if (k == 2) fmh = v;
      else fph = v;
    }
    const double r3 = 0.5 * (fp1 - fm1);
    const double r5 = (4.0 / 3.0) * (fph - fmh) - (1.0 / 3.0) * r3;
    const double e3 = (fabs(fp1) + fabs(fm1)) * kEps;
    const double e5 = 2.0 * (fabs(fph) + fabs(fmh)) * kEps + e3;
    const double a3 = fabs(r3 / h), a5 = fabs(r5 / h);
    const double dy = (a3 > a5 ? a3 : a5) * (fabs(x) / h) * kEps;  // GSL_MAX
    const double r = r5 / h;
    const double trunc = fabs((r5 - r3) / h);
    const double round = fabs(e5 / h) + dy;
    if (pass == 0) {
      r_0 = r;
      error = round + trunc;
      if (!(round < trunc && (round > 0 && trunc > 0))) break;
      h = h * pow(round / (2.0 * trunc), 1.0 / 3.0);
    } else if (round + trunc < error && fabs(r - r_0) < 4.0 * error) {
      r_0 = r;
    }
  }
  return r_0;
}

// FindFunctionRootFDF (.cc:222-258): gsl_root_fdfsolver_newton (roots/newton.c) from the bracket
// midpoint, slopes by gsl_deriv_central(h = 1e-8) (fRaa_df, .cc:609-618), at most 100 steps,
// stopped by gsl_root_test_delta(x, x0, 0, 1e-6).  A zero slope leaves the root where it is
// (GSL_EZERODIV), which the delta test reads as converged.  A NaN root stays NaN through all
// 100 steps of the reference; the loop ends at the first.
AIRICE_IR_HD inline Root newton(Pair& p, int kind, double x_lo, double x_hi) {
  Root R;
  double x = (x_lo + x_hi) / 2, x0 = x;
  double f;
  int iter = 0;
  for (;;) {
    // f and its slope at x: the set call's when iter == 0, else the step's
    f = residual(p, kind, x);
    if (is_nan(x)) break;
    const double df = deriv_central(p, kind, x, 1e-8);
    if (iter > 0) {
      const double tolerance = 0.0 + 1e-6 * fabs(x);
      if (fabs(x - x0) < tolerance || x == x0) break;
      if (iter >= 100) break;
    }
    iter++;
    x0 = x;
    if (df == 0.0) break;  // the root stays: x == x0, converged
    x = x - (f / df);
  }
  R.r = x;
  R.fr = f;
  R.iters = iter;
  return R;
}

// One ray as the reference's *RayPar functions return it: receive and launch angle (deg), time,
// L, checkzero, the two legs' times, aux (the reflected ray's incidence angle at the surface, a
// refracted ray's turning depth), geometric path and its two legs.
struct RayOut {
  double rang, lang, time, L, checkzero, time1, time2, aux, path, path1, path2;
};
enum RayKind { kDirect = 0, kReflected = 1, kRefracted = 2 };

// The closing arithmetic of GetDirectRayPar (.cc:661-739), GetReflectedRayPar (.cc:780-917) and
// one turn of GetRefractedRayPar's loop (.cc:1075-1195) at the L the search found.
// Times and paths are differences of ftimeD / fpathD at z0, z1 and -- reflected, refracted -- the
// top of the ray (the surface, the turning depth).  The reference evaluates the direct ray's at
// (-z, -C) and the others' at (z, C); the two forms are exact negatives of each other (the signs
// cancel in C*z and flip the outer quotient), so one form serves, with the direct difference
// taken the other way round: the same bits.
// Angles: asin(L / n(z1)) where the reference takes atan of gsl_deriv_central(fDnfR) at the Rx
// (.cc:708, 869, 1182), asin(L / n(1e-7)) for the incidence angle (.cc:890); its NaN fallbacks
// (180 - launch angle at equal depths, else 90) stay as written.
AIRICE_IR_HD inline RayOut finish_ray(const Pair& p, bool flip, int kind, double L, double lang,
                                      double cz, double zm) {
  const IceModel& m = p.m;
  RayOut o;
  if (is_nan(cz)) cz = -1000;
  if (kind == kRefracted && (zm == 1e-7 || zm <= 0)) cz = -1000;  // .cc:1083
  double ta = 0, sa = 0, tb = 0, sb = 0, tt = 0, st = 0;
  // .cc:1095: a refracted ray's legs only when its turning point is above the Tx or the Rx
  if (kind != kRefracted || (p.z0 < -zm || zm < -p.z1)) {
    // the top of a refracted ray whose zm is the turning depth of its L (zmax_of found one):
    // top_gap.  (A ray the searches never set -- L = 0 with zm = 10 or -1000 -- and an L outside
    // (A + B, A) keep the reference's form.)
    const bool turning = kind == kRefracted && L > m.A + m.B && L < m.A;
    AIRICE_IR_NOUNROLL
    // a time or a path per turn: the two together hold enough live values to cost the kernel
    // its third wave
    for (int kk = (kind == kDirect ? 2 : 0); kk < 6; kk++) {
      const int k = kk >> 1;
      double z, n, e, q2;
      if (k == 0 && turning) {
        const double gap = top_gap(m, L);
        z = -zm;
        n = L + gap;
        e = (n - m.A) / m.B;
        q2 = gap * (n + L);
      } else {
        if (k == 0) {
          z = kind == kReflected ? -1e-7 : -zm;
          n = kind == kReflected ? p.ns : nz(m, zm);
        } else {
          z = k == 1 ? p.z0 : p.z1;
          n = k == 1 ? p.n0 : p.n1;
        }
        e = exp(m.C * z);
        q2 = n * n - L * L;
      }
      const double v = (kk & 1) ? fpathD_q(m, z, m.C, e, n, q2, L)
                                : ftimeD_q(m, z, m.C, n, q2, L, kSpeedC);
      if (kk == 0) tt = v;
      else if (kk == 1) st = v;
      else if (kk == 2) ta = v;
      else if (kk == 3) sa = v;
      else if (kk == 4) tb = v;
      else sb = v;
    }
  }
  double time1 = 0, time2 = 0, path1 = 0, path2 = 0;
  if (kind == kDirect) {
    o.time = tb - ta;
    o.path = sb - sa;
  } else {
    time1 = tt - ta;
    time2 = tt - tb;
    path1 = st - sa;
    path2 = st - sb;
    o.time = time1 + time2;
    o.path = path1 + path2;
    if (flip) {
      double t;
      t = time2, time2 = time1, time1 = t;
      t = path2, path2 = path1, path1 = t;
    }
  }
  double rang = asin(L / p.n1) * kDeg;
  if (kind != kDirect) rang = 180 - rang;
  if (p.z1 == p.z0 && is_nan(rang)) rang = 180 - lang;
  if (kind != kDirect && p.z1 != p.z0 && is_nan(rang)) rang = 90;
  o.aux = kind == kReflected ? asin(L / p.ns) * kDeg : zm;
  o.rang = flip ? 180 - lang : rang;
  o.lang = flip ? 180 - rang : lang;
  o.L = L;
  o.checkzero = cz;
  o.time1 = time1;
  o.time2 = time2;
  o.path1 = path1;
  o.path2 = path2;
  return o;
}

// What one ray's search leaves for the next (IceRayTracing's locals, .cc:1766-1789; the arguments
// of GetRefractedRayPar): the direct and reflected rays' checkzero, the reflected ray's angles as
// GetReflectedRayPar returns them, the direct search's iteration count.
struct SearchState {
  double czD, czR, LangR, RangR;
  int itersD;
};

// Rows first..last of the solve, emit(ray, RayOut) as each ray (0 D, 1 R, 2 Ra0, 3 Ra1) is final:
//   0      GetDirectRayPar: false position of fDa on [1e-7, min(n(z1), n(z0))]
//   1      GetReflectedRayPar: false position of fRa on [1e-7, min(n(z1), n(z0), n(1e-7))]
//   2      the refracted ray (.cc:978-987): false position of fRaa on [lower, min(n(z0), n(z1))],
//          lower = n(z0) sin 64 deg, or the reflected ray's L when that is above the upper limit;
//          with gate, only when the direct or the reflected ray failed (.cc:1806)
//   3      Newton on the same bracket when |checkzero| > 0.5 (.cc:989-994)
//   4..8   the second refracted root (.cc:1000-1045), only when the first is accepted and both D
//          and R failed; each row only while the last one is not an accepted root distinct from
//          the first (row 4 always): false position on [l0 - 0.23, l0 - 0.023], on
//          [l0 - 0.15, l0 - 0.023], on [l0 + 0.005, upper] (or [l0 - 0.1, l0 - 0.01] when that is
//          empty), then Newton from the middle of [l0 - 0.23, l0 - 0.023] and of
//          [l0 - 0.1, l0 - 0.023], taken only when |root| < A.  (The reference runs the first
//          Newton twice with the same arguments; once here.)
//   9, 10  the same-root test, the swap by launch angle (.cc:1047-1066), and the two refracted
//          rays' closing arithmetic
template <class Emit>
AIRICE_IR_HD inline void run_stages(Pair& p, bool flip, int first, int last, bool gate,
                                    SearchState& s, Emit&& emit) {
  const IceModel& m = p.m;
  double l0 = 0, lang0 = 0, cz0 = -1000, zm0 = 10;  // .cc:945-959
  double l1 = 0, lang1 = 0, cz1 = -1000, zm1 = 10;
  double up = 0, lower = 0;
  bool second = false;
  for (int stage = first; stage <= last; stage++) {
    bool search = false, use_newton = false;
    int kind = kFDa, finish = -1;
    double lo = 1e-7, hi = p.n1;
    if (stage <= 1) {  // min_element({Getnz(z1), Getnz(z0)[, Getnz(1e-7)]})
      search = true;
      kind = stage == 0 ? kFDa : kFRa;
      if (p.n0 < hi) hi = p.n0;
      if (stage == 1 && p.ns < hi) hi = p.ns;
      finish = stage;
    } else if (stage <= 3) {
      if (stage == 2) {
        if (gate && !(fabs(s.czR) > 0.5 || fabs(s.czD) > 0.5)) break;
        double LangR = s.LangR;
        if (flip) LangR = 180 - s.RangR;  // .cc:937-941
        up = p.n0;  // min_element({Getnz(z0), Getnz(z1)})
        if (p.n1 < up) up = p.n1;
        lower = p.n0 * sin(64.0 * (kPi / 180.0));
        if (lower > up) lower = p.n0 * sin(LangR * (kPi / 180.0));
      }
      kind = kFRaa;
      lo = lower;
      hi = up;
      use_newton = stage == 3;
      search = stage == 2 || fabs(cz0) > 0.5;
    } else if (stage <= 8) {
      if (stage == 4) {
        if (l0 < 0) cz0 = -1000;
        second = fabs(cz0) < 0.5 && fabs(s.czD) > 0.5 && fabs(s.czR) > 0.5;
        if (!second) {  // .cc:1068-1073
          l1 = 0;
          lang1 = 0;
          cz1 = -1000;
          zm1 = -1000;
        }
      }
      const int row = stage - 4;
      const bool retry = fabs(cz1) > 0.5 || is_nan(cz1) || fabs(l1 - l0) < 1e-4;
      kind = kFRaa;
      search = second && (row == 0 || retry);
      use_newton = row >= 3;
      lo = l0 - (row == 1 ? 0.15 : (row == 4 ? 0.1 : 0.23));
      hi = l0 - 0.023;
      if (row == 2) {
        if (l0 + 0.005 < up) {
          lo = l0 + 0.005;
          hi = up;
        } else {
          lo = l0 - 0.1;
          hi = l0 - 0.01;
        }
      }
    } else {
      if (stage == 9 && second) {
        if (l1 < 0) cz1 = -1000;
        if (fabs(cz1) < 0.5 && fabs(cz0) < 0.5 && fabs(l1 - l0) < 1e-4) cz1 = -1000;
        if (is_nan(lang0)) lang0 = 0;
        if (is_nan(lang1)) lang1 = 0;
        if (lang1 < lang0 && fabs(cz0) < 0.5 && fabs(cz1) < 0.5) {  // order by launch angle
          double t;
          t = l0, l0 = l1, l1 = t;
          t = lang0, lang0 = lang1, lang1 = t;
          t = cz0, cz0 = cz1, cz1 = t;
          t = zm0, zm0 = zm1, zm1 = t;
        }
      }
      finish = stage - 7;
    }

    double fL = 0, fLang = 0, fCz = 0, fZm = 0;
    if (search) {
      const Root S = use_newton ? newton(p, kind, lo, hi) : falsepos(p, kind, lo, hi);
      const double lang = asin(S.r / p.n0) * kDeg;
      if (stage <= 1) {
        fL = S.r;
        fLang = lang;
        fCz = S.fr;
        if (stage == 0) s.itersD = S.iters;
      } else if (stage <= 3) {
        l0 = S.r;
        lang0 = lang;
        cz0 = S.fr;
        zm0 = zmax_of(m, S.r) + 1e-7;
      } else if (!use_newton || fabs(S.r) < m.A) {
        l1 = S.r;
        lang1 = lang;
        cz1 = S.fr;
        zm1 = zmax_of(m, S.r) + 1e-7;
      }
    }
    if (finish >= 0) {
      if (finish == 2) fL = l0, fLang = lang0, fCz = cz0, fZm = zm0;
      if (finish == 3) fL = l1, fLang = lang1, fCz = cz1, fZm = zm1;
      const RayOut o = finish_ray(p, flip, finish < 2 ? finish : kRefracted, fL, fLang, fCz, fZm);
      if (finish == 0) s.czD = o.checkzero;
      if (finish == 1) {
        s.czR = o.checkzero;
        s.LangR = o.lang;
        s.RangR = o.rang;
      }
      emit(finish, o);
    }
  }
}

// IceRayTracing (.cc:1745-1919) for one pair: out.put(column, value) receives the reference's
// output[0..28] in its order -- each ray's columns as soon as that ray is final -- then column 29
// (the status byte as a double), 30 (residual evaluations) and 31 (false-position iterations of
// the direct search).  Columns 12-17, which the reference leaves as uninitialised heap when their
// ray failed, are 0.0.  Returns the status byte: bit k set when ray k (D, R, Ra0, Ra1) is accepted
// (|checkzero| < 0.5); bit 7 alone for a non-finite input, whose 29 ray columns are NaN and for
// which no search runs.
template <class Out>
AIRICE_IR_HD inline uint8_t solve_pair(const IceModel& m, double z0, double x1, double z1,
                                       Out&& out) {
  if (!(is_finite(z0) && is_finite(x1) && is_finite(z1))) {
    for (int c = 0; c < kFields; c++) out.put(c, quiet_nan());
    out.put(kColStatus, (double)kNonFinite);
    out.put(kColEvals, 0.0);
    out.put(kColIters, 0.0);
    return (uint8_t)kNonFinite;
  }
  bool flip;
  Pair p = make_ray_pair(m, z0, x1, z1, &flip);
  SearchState s = {0, 0, 0, 0, 0};
  int status = 0, emitted = 0;
  run_stages(p, flip, 0, 10, true, s, [&](int ray, const RayOut& r) {
    emitted = ray + 1;
    // the second refracted solution is taken only when both D and R failed (.cc:1817), its
    // path always (.cc:1832)
    if (ray == 3 && !(fabs(s.czR) > 0.5 && fabs(s.czD) > 0.5)) {
      out.put(3, 0.0);
      out.put(7, 0.0);
      out.put(11, -1000.0);
      out.put(16, 0.0);
      out.put(17, 0.0);
      out.put(22, 0.0);
      out.put(24, 0.0);
      out.put(28, r.path);
      return;
    }
    const bool ok = fabs(r.checkzero) < 0.5;
    if (ok) status |= 1 << ray;
    out.put(0 + ray, r.lang);
    out.put(4 + ray, r.time);
    out.put(8 + ray, fabs(r.checkzero) > 0.5 ? -1000.0 : r.rang);  // .cc:1905-1916
    out.put(19 + ray, r.L);
    out.put(25 + ray, r.path);
    if (ray >= 1) {
      out.put(10 + 2 * ray, ok ? r.time1 : 0.0);
      out.put(11 + 2 * ray, ok ? r.time2 : 0.0);
    }
    if (ray == 1) out.put(18, r.aux);
    if (ray >= 2) out.put(21 + ray, r.aux);
  });
  if (emitted < 4) {  // no refracted search (.cc:1792-1803)
    AIRICE_IR_NOUNROLL
    for (int ray = 2; ray < 4; ray++) {
      out.put(0 + ray, 0.0);
      out.put(4 + ray, 0.0);
      out.put(8 + ray, -1000.0);
      out.put(10 + 2 * ray, 0.0);
      out.put(11 + 2 * ray, 0.0);
      out.put(19 + ray, 0.0);
      out.put(21 + ray, 0.0);
      out.put(25 + ray, 0.0);
    }
  }
  out.put(kColStatus, (double)status);
  out.put(kColEvals, (double)p.evals);
  out.put(kColIters, (double)s.itersD);
  return (uint8_t)status;
}

// out.put for a plain array of kColumns doubles
struct ArrayOut {
  double* v;
  AIRICE_IR_HD void put(int c, double x) { v[c] = x; }
};

}  // namespace iceray
}  // namespace airice
