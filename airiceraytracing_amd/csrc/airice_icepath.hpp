// airice_icepath.hpp -- the in-ice ray-path samplers of the reference (IceRayTracing.cc:
// GetFullDirectRayPath :1257, GetFullReflectedRayPath :1363, GetFullRefractedRayPath :1533),
// written once for the device (icepath_consts_kernel / icepath_kernel, airice_icepath.hip) and the
// host (airice_icepath_one_host, airice_host.cpp; the IceRayTracing::GetFull* drop-in,
// compat_iceray.cpp).
//
// One ray is (kind, z0, x1, z1, L, zmax): kind one of D, R, Ra0, Ra1 (index 0..3, the bit
// positions of AIRICE_ICERAY_D / _R / _RA0 / _RA1), zmax read by Ra only.  TransitionBoundary is
// the constexpr 0 of this project, so only the reference's `else` branches are restated; h = 0.5 m.
// The reference's flip applies: z0 > z1 swaps the depths and emits x1 - xn.  With
// F(z) = fDnfR(z; A, B, +C, L) the samples, in the reference's order, are
//   D    zn_k = z1 - 0.5 k while zn_k >= z0, xn = F(zn) - F(z0); then the closing sample at z0
//   R    leg 1: zn_k = z1 + 0.5 k while zn_k <= 0, xn = 2 F(-1e-7) - F(zn) - F(z0) (the reference's
//        distancez0z1 - 2 distancez0surface, which it writes in the -C convention);
//        leg 2: zn_k = -1e-7 - 0.5 k while zn_k >= z0, xn = F(zn) - F(z0); then the closing sample
//   Ra   as R with -zmax in place of the surface: leg 1 while zn_k <= -zmax, leg 2 from -zmax
// Three departures: a downward leg's depth is fl(start - 0.5 k), rounded once,
// where the reference chains zn = zn - h; no sample is dropped (q^2 = n^2 - L^2 is clamped at 0
// where the reference skips a NaN); on Ra legs n(z) - L is formed without cancellation.
#pragma once
#include "airice_iceray.hpp"

namespace airice {
namespace icepath {

constexpr double kStep = 0.5;            // the reference's h
constexpr double kDeepest = -50000.0;    // its dmax (100000) steps of h: no depth below this
constexpr int kKinds = 4;                // D, R, Ra0, Ra1

// The number of k >= 0 with fl(start - 0.5 k) >= stop: the predicate is monotone in k (rounding
// is), so the closed form is corrected by testing the predicate itself at its edge.
AIRICE_IR_HD inline long long count_down(double start, double stop) {
  if (!(start >= stop)) return 0;
  long long c = (long long)floor((start - stop) * 2.0) + 1;
  while (c > 0 && !(start - kStep * (double)(c - 1) >= stop)) --c;
  while (start - kStep * (double)c >= stop) ++c;
  return c;
}
// The number of k >= 0 with fl(start + 0.5 k) <= stop.
AIRICE_IR_HD inline long long count_up(double start, double stop) {
  if (!(start <= stop)) return 0;
  long long c = (long long)floor((stop - start) * 2.0) + 1;
  while (c > 0 && !(start + kStep * (double)(c - 1) <= stop)) --c;
  while (start + kStep * (double)c <= stop) ++c;
  return c;
}

// A pair the samplers take: both depths finite, in the ice and within the reference's dmax steps.
AIRICE_IR_HD inline bool depths_ok(double z0, double z1) {
  return z0 <= 0.0 && z0 >= kDeepest && z1 <= 0.0 && z1 >= kDeepest;
}

// The sample counts that need no L: the direct and the reflected ray's, from the depths alone.
AIRICE_IR_HD inline long long count_direct(double z0, double z1) {
  if (!depths_ok(z0, z1)) return 0;
  const double lo = z0 > z1 ? z1 : z0, hi = z0 > z1 ? z0 : z1;
  return count_down(hi, lo) + 1;
}
AIRICE_IR_HD inline long long count_reflected(double z0, double z1) {
  if (!depths_ok(z0, z1)) return 0;
  const double lo = z0 > z1 ? z1 : z0, hi = z0 > z1 ? z0 : z1;
  return count_up(hi, 0.0) + count_down(-iceray::kSurface, lo) + 1;
}
// What a refracted ray's count cannot exceed, whatever its turning depth zmax >= 0:
// count_reflected + 1.  Leg 1: {k : z1 + 0.5 k <= -zmax} is a subset of {k : z1 + 0.5 k <= 0}.
// Leg 2: -zmax <= 0 and rounding is monotone, so fl(-zmax - 0.5 k) <= -0.5 k and the leg holds at
// most #{k >= 0 : -0.5 k >= z0} = floor(-2 z0) + 1 samples; the reflected ray's second leg has
// fl(-1e-7 - 0.5 k) >= -0.5 (k + 1) (a representable number below its argument), so it holds at
// least #{j >= 1 : -0.5 j >= z0} = floor(-2 z0) samples: one fewer at the most.
AIRICE_IR_HD inline long long bound_refracted(double z0, double z1) {
  if (!depths_ok(z0, z1)) return 0;
  return count_reflected(z0, z1) + 1;
}

// One ray, ready to be sampled: what a sample needs that does not depend on its index.
struct Segment {
  double z0, z1, x1;  // the reference's flip applied: z0 <= z1
  double top;         // where leg 1 ends and leg 2 starts: -1e-7 (R), -zmax (Ra); unused by D
  double L, zt;       // zt: the turning depth of L, where n = L (Ra; see sample_F)
  double sA, pre;     // sqrt(A^2 - L^2), (L / C) (1 / sA)
  double F0, Ftop2;   // F(z0), 2 F(top)
  long long n1, count;  // samples of leg 1, of the whole ray (count 0: nothing to emit)
  int kind, flip;
};

// F(z) = fDnfR(z; A, B, +C, L) (.cc:356-365) with q^2 = n(z)^2 - L^2 clamped at 0.  On a refracted
// ray (turning) n(z) - L = (L - A) expm1(-C (|z| - zt)) -- exact where n(zt) = L, with no
// cancellation -- and q^2 = (n - L)(n + L): the top_gap of airice_iceray.hpp at every sample.
AIRICE_IR_HD inline double sample_F(const iceray::IceModel& m, const Segment& s, bool turning,
                                    double z) {
  const double n = m.A + m.B * exp(-m.C * fabs(z));
  double q2;
  if (turning) q2 = (s.L - m.A) * expm1(-m.C * (fabs(z) - s.zt)) * (n + s.L);
  else q2 = n * n - s.L * s.L;
  if (!(q2 > 0.0)) q2 = 0.0;
  return s.pre * (m.C * z - log(m.A * n - s.L * s.L + s.sA * sqrt(q2)));
}

// Whether the segment's ray is sampled in the refracted form: a refracted kind whose L has a
// turning depth (every accepted refracted ray's has).
AIRICE_IR_HD inline bool is_turning(const iceray::IceModel& m, int kind, double L) {
  return kind >= 2 && L > m.A + m.B && L < m.A;
}

// The segment of ray `kind` (0 D, 1 R, 2 Ra0, 3 Ra1) between (0, z0) and (x1, z1).  zmax as the
// solver reports it (columns 23-24: the turning depth of L plus the 1e-7 the reference keeps its
// rays below it) or the turning depth itself; the index is formed about the turning depth of L,
// so the apex sample zn = -zmax has q = 0 exactly in the second case and the solver's
// sqrt((n - L)(n + L)) at its 1e-7 in the first.  count 0: a non-finite input, a depth above 0 or
// below -50,000 m, or a refracted ray without a zmax >= 0.
AIRICE_IR_HD inline Segment make_segment(const iceray::IceModel& m, int kind, double z0, double x1,
                                         double z1, double L, double zmax) {
  Segment s;
  s.kind = kind;
  s.flip = 0;
  if (z0 > z1) {  // .cc:1262-1266
    const double dsw = z0;
    z0 = z1;
    z1 = dsw;
    s.flip = 1;
  }
  s.z0 = z0;
  s.z1 = z1;
  s.x1 = x1;
  s.L = L;
  s.top = kind == 1 ? -iceray::kSurface : -zmax;
  s.zt = 0.0;
  s.sA = s.pre = s.F0 = s.Ftop2 = 0.0;
  s.n1 = s.count = 0;
  const bool finite = iceray::is_finite(x1) && iceray::is_finite(L);
  if (!depths_ok(z0, z1) || !finite || (kind >= 2 && !(zmax >= 0.0 && zmax <= -kDeepest)))
    return s;
  long long n2;
  if (kind == 0) {
    n2 = count_down(z1, z0);
  } else {
    s.n1 = count_up(z1, kind == 1 ? 0.0 : s.top);
    n2 = count_down(s.top, z0);
  }
  s.count = s.n1 + n2 + 1;
  const bool turning = is_turning(m, kind, L);
  if (turning) s.zt = log(m.B / (L - m.A)) / m.C;  // iceray::zmax_of
  s.sA = sqrt(m.A * m.A - L * L);
  s.pre = (L / m.C) * (1.0 / s.sA);
  s.F0 = sample_F(m, s, turning, z0);
  if (kind != 0) s.Ftop2 = 2 * sample_F(m, s, turning, s.top);
  return s;
}

// Sample k (0 <= k < s.count) of the segment, in the reference's order.
AIRICE_IR_HD inline void sample(const iceray::IceModel& m, const Segment& s, long long k, double& x,
                                double& z) {
  const bool turning = is_turning(m, s.kind, s.L);
  double zn;
  const bool leg1 = k < s.n1;
  if (leg1) zn = s.z1 + kStep * (double)k;
  else if (k == s.count - 1) zn = s.z0;
  else zn = (s.kind == 0 ? s.z1 : s.top) - kStep * (double)(k - s.n1);
  const double F = sample_F(m, s, turning, zn);
  const double xn = leg1 ? s.Ftop2 - F - s.F0 : F - s.F0;
  x = s.flip ? s.x1 - xn : xn;
  z = zn;
}

}  // namespace icepath
}  // namespace airice
