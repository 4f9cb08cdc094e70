// airice_icesol.hpp -- what a user of the reference's in-ice tracer calls: the two rays a receiver
// sees with their ice attenuation (IceRayTracing::GetRayTracingSolutions, IceRayTracing.cc:2907)
// and their focusing factors (GetFocusingFactor, .cc:3218), computed from the 32 columns the
// in-ice solver (airice_iceray.hpp) leaves for a pair.  Written once for the device
// (icesol_kernel, airice_icesol.hip) and the host (icesol_host_one, airice_host.cpp; the
// IceRayTracing:: drop-in, compat_iceray.cpp).
//
// Restated: GetIceTemperature (.cc:137), GetIceAttenuationLength (.cc:144), the attenuation of a
// ray's legs (AttenuationIntegrand, IntegrateOverLAttn, GetTotalAttenuation*, .cc:166-219), the
// choice and ordering of GetRayTracingSolutions (.cc:2943-3200) and the focusing formula
// (.cc:3239-3291).  The departures -- a fixed 24-node Gauss-Legendre rule in s = sqrt(z - zv)
// where the reference calls QAGS in z, a refracted leg that ends at the turning point of its own
// L, NaN where the reference's integrand is NaN -- are in DESIGN.md §9.
//
// Shape: the choice comes first (it reads only the four receive angles), so the attenuation is
// integrated for the two chosen rays alone -- at most four legs, which are rows of ONE loop over
// ONE copy of the integrand.  No workspace, no subdivision: every lane of a wave runs the same 24
// nodes per row.
#pragma once
#include "airice_iceray.hpp"

namespace airice {
namespace icesol {

using iceray::IceModel;
using iceray::quiet_nan;

constexpr int kFields = 18;  // AIRICE_ICESOL_FIELDS
constexpr int kColTime = 0, kColPath = 2, kColLaunch = 4, kColReceive = 6, kColIgnore = 8,
              kColIncidence = 10, kColAtt = 12, kColType = 14, kColFocus = 16;
constexpr int kSlot0 = 1, kSlot1 = 2, kStraight = 4, kFocus0 = 8, kFocus1 = 16, kNonFinite = 128;
constexpr double kNoRay = -1000.0;       // the receive angle of a ray that does not exist
constexpr double kSurfaceAtt = 0.000001; // the depth a reflected leg ends at (.cc:212)
constexpr double kLowerRx = 0.01;        // GetFocusingFactor's second receiver (.cc:3257)

// GetIceTemperature (.cc:137-141): the cubic in |z|, in Horner form
AIRICE_IR_HD inline double ice_temperature(double z) {
  const double d = fabs(z);
  return ((1.83415e-09 * d + -1.59061e-08) * d + 0.00267687) * d + -51.0696;
}

// GetIceAttenuationLength (.cc:144-163) as written
AIRICE_IR_HD inline double attenuation_length(double z, double frequency) {
  const double t = ice_temperature(z);
  const double f0 = 0.0001, f2 = 3.16;
  const double w0 = log(f0), w1 = 0.0, w2 = log(f2), w = log(frequency);
  const double b0 = -6.74890 + t * (0.026709 - t * 0.000884);
  const double b1 = -6.22121 - t * (0.070927 + t * 0.001773);
  const double b2 = -4.09468 - t * (0.002213 + t * 0.000332);
  double a, bb;
  if (frequency < 1.) {
    a = (b1 * w0 - b0 * w1) / (w0 - w1);
    bb = (b1 - b0) / (w1 - w0);
  } else {
    a = (b2 * w1 - b1 * w2) / (w1 - w2);
    bb = (b2 - b1) / (w2 - w1);
  }
  return 1. / exp(a + bb * w);
}

// What a batch's A0 and frequency leave for the integrand.  1 / L_att = exp(a + bb w) with
// a + bb w = bA (w - wB) / (wA - wB) + bB (wA - w) / (wA - wB): the two b of the frequency's
// branch, weighted by where log f lies between the branch's ends.  Each b is a quadratic in the
// temperature t, so the exponent is k0 + t (k1 + t k2) with three numbers that hold for the batch.
struct Medium {
  double a0, k0, k1, k2;
};

inline Medium make_medium(double a0, double frequency) {
  const double w = log(frequency);
  const bool low = frequency < 1.;
  const double wA = low ? log(0.0001) : 0.0, wB = low ? 0.0 : log(3.16);
  const double cA = (w - wB) / (wA - wB), cB = (wA - w) / (wA - wB);
  const double b[3][3] = {{-6.74890, 0.026709, -0.000884},
                          {-6.22121, -0.070927, -0.001773},
                          {-4.09468, -0.002213, -0.000332}};
  const int iA = low ? 0 : 1, iB = iA + 1;
  Medium q;
  q.a0 = a0;
  q.k0 = b[iA][0] * cA + b[iB][0] * cB;
  q.k1 = b[iA][1] * cA + b[iB][1] * cB;
  q.k2 = b[iA][2] * cA + b[iB][2] * cB;
  return q;
}

// The positive nodes and the weights of the 24-point Gauss-Legendre rule on [-1, 1]
constexpr int kGaussHalf = 12;
AIRICE_IR_HD inline double gauss_x(int j) {
  constexpr double x[kGaussHalf] = {
      0.064056892862605626085, 0.19111886747361630916, 0.31504267969616337439,
      0.43379350762604513849,  0.54542147138883953566, 0.64809365193697556925,
      0.74012419157855436424,  0.82000198597390292195, 0.88641552700440103421,
      0.93827455200273275852,  0.9747285559713094982,  0.99518721999702136018};
  return x[j];
}
AIRICE_IR_HD inline double gauss_w(int j) {
  constexpr double w[kGaussHalf] = {
      0.12793819534675215697,  0.12583745634682829612,  0.1216704729278033912,
      0.11550566805372560135,  0.10744427011596563478,  0.09761865210411388827,
      0.086190161531953275917, 0.073346481411080305734, 0.059298584915436780746,
      0.044277438817419806169, 0.028531388628933663181, 0.012341229799987199547};
  return w[j];
}

// One leg of a ray of invariant L: the depths (positive) it runs between, or from za to the
// turning depth of L.
struct Leg {
  double L, za, zb;
  bool turning;
};

// |integral of (1 / L_att(z)) n / sqrt(n^2 - L^2) dz| over each of the n_legs legs, added into
// sum0 (legs 0, 1) or sum1 (legs 2, 3): the legs of a ray are neighbours.  With z = zv + s^2, zv = ln(B / (L - A)) / C the
// depth where n = L (the turning depth of a refracted ray; above the surface for L < A + B):
//   n = A + (L - A) e^{-C s^2},  n - L = (A - L)(-expm1(-C s^2)),
//   dz n / sqrt(n^2 - L^2) = 2 ds n s / sqrt((A - L)(n + L)(-expm1(-C s^2))),
// smooth on [sqrt(za - zv), sqrt(zb - zv)] with the limit s / sqrt(-expm1(-C s^2)) -> 1 / sqrt(C)
// at s = 0.  A leg with an end above zv, or L >= A, is NaN: the reference's integrand is NaN
// there.  Assumes B < 0 < C (the callers check).
template <class LegOf>
AIRICE_IR_HD inline void integrate_legs(const IceModel& m, const Medium& q, int n_legs,
                                        LegOf&& leg_of, double& sum0, double& sum1) {
  AIRICE_IR_NOUNROLL
  for (int k = 0; k < n_legs; k++) {
    const Leg g = leg_of(k);
    const double zv = log(m.B / (g.L - m.A)) / m.C;
    const double sa = sqrt(g.za - zv);
    const double sb = g.turning ? 0.0 : sqrt(g.zb - zv);
    const double mid = 0.5 * (sa + sb), hw = 0.5 * (sb - sa);
    const double AL = m.A - g.L;
    double acc = 0;
    if (hw != 0.0) {
      AIRICE_IR_NOUNROLL
      for (int j = 0; j < 2 * kGaussHalf; j++) {
        const double x = gauss_x(j >> 1);
        const double s = mid + hw * ((j & 1) ? -x : x);
        const double s2 = s * s;
        const double u = -expm1(-m.C * s2);
        const double n = m.A + (g.L - m.A) * (1.0 - u);
        const double t = ice_temperature(zv + s2);
        const double inv_latt = exp(q.k0 + t * (q.k1 + t * q.k2));
        // no node is an end of the panel, so s > 0 here and the limit at s = 0 is never taken
        acc += gauss_w(j >> 1) * (inv_latt * n * sqrt(s2 / (u * (AL * (n + g.L)))));
      }
    }
    const double v = fabs(2.0 * hw * acc);
    if (k >> 1) sum1 += v;
    else sum0 += v;
  }
}

// IntegrateOverLAttn (.cc:179-200) between the limits given
AIRICE_IR_HD inline double attenuation_between(const IceModel& m, const Medium& q, double z0,
                                               double z1, double L) {
  double sum = 0, none = 0;
  integrate_legs(m, q, 1, [&](int) { return Leg{L, z0, z1, false}; }, sum, none);
  return fabs(q.a0 * sum);
}

// The legs of ray `type` (1 D, 2 R, 3 / 4 refracted) between |z0| and |z1|
// (GetTotalAttenuationDirect / Reflected / Refracted, .cc:203-219)
AIRICE_IR_HD inline Leg ray_leg(int type, int leg, double L, double z0, double z1) {
  z0 = fabs(z0);
  z1 = fabs(z1);
  if (type == 1) return Leg{L, z0, z1, false};
  return Leg{L, leg == 0 ? z0 : z1, kSurfaceAtt, type >= 3};
}

// GetTotalAttenuation* of one ray
AIRICE_IR_HD inline double total_attenuation(const IceModel& m, const Medium& q, int type,
                                             double z0, double z1, double L) {
  double sum = 0, none = 0;
  integrate_legs(m, q, type == 1 ? 1 : 2,
                 [&](int k) { return ray_leg(type, k, L, z0, z1); }, sum, none);
  return fabs(q.a0 * sum);
}

// The choice of GetRayTracingSolutions (.cc:3004-3128) on the four receive angles alone: which ray
// (0 D, 1 R, 2 Ra0, 3 Ra1) each of the two slots holds.  Every block of the reference copies a
// ray's values into a slot whole, so the slot's ray says it all; the blocks are in its order.
struct Choice {
  int s0, s1;
};
// v[i] without a register array indexed at run time
AIRICE_IR_HD inline double pick4(const double v[4], int i) {
  return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3];
}
AIRICE_IR_HD inline Choice choose(const double rang[4]) {
  const bool d = rang[0] != kNoRay, r = rang[1] != kNoRay;
  const bool a0 = rang[2] != kNoRay, a1 = rang[3] != kNoRay;
  Choice c = {0, 1};  // .cc:2989-3030
  if (a0 && d) c.s0 = 0, c.s1 = 2;
  if (a0 && r) c.s1 = 1, c.s0 = 2;
  if (a1 && d) c.s0 = 0, c.s1 = 3;
  if (a1 && r) c.s1 = 1, c.s0 = 3;
  if (a1 && a0) c.s1 = 3, c.s0 = 2;
  if (pick4(rang, c.s1) == kNoRay && pick4(rang, c.s0) == kNoRay && a0) c.s0 = 2;
  if (pick4(rang, c.s1) == kNoRay && pick4(rang, c.s0) == kNoRay && a1) c.s1 = 3;
  return c;
}

// The two rays of a receiver after the swap by time and the straight-line rule (.cc:3130-3200),
// without attenuation: all GetFocusingFactor reads of the lower receiver.
struct Chosen {
  double time[2], path[2], lang[2], rang[2];
  int ignore[2], src[2];  // IgnoreCh; the ray (0..3) of each slot, RayType - 1
  bool straight;
};

// ray(c): column c of the solver's row for (z0, x1, z1)
template <class Ray>
AIRICE_IR_HD inline Chosen choose_and_order(const IceModel& m, double z0, double x1, double z1,
                                            Ray&& ray) {
  double rang4[4];
  for (int k = 0; k < 4; k++) rang4[k] = ray(8 + k);
  const Choice c = choose(rang4);
  Chosen o;
  o.src[0] = c.s0;
  o.src[1] = c.s1;
  for (int k = 0; k < 2; k++) {
    const int s = o.src[k];
    o.lang[k] = ray(0 + s);
    o.time[k] = ray(4 + s);
    o.rang[k] = pick4(rang4, s);
    o.path[k] = ray(25 + s);
    o.ignore[k] = o.rang[k] == kNoRay ? 0 : 1;
  }
  if (o.time[0] > o.time[1] && o.rang[0] != kNoRay && o.rang[1] != kNoRay) {  // .cc:3141-3148
    double t;
    int i;
    t = o.lang[0], o.lang[0] = o.lang[1], o.lang[1] = t;
    t = o.rang[0], o.rang[0] = o.rang[1], o.rang[1] = t;
    t = o.time[0], o.time[0] = o.time[1], o.time[1] = t;
    t = o.path[0], o.path[0] = o.path[1], o.path[1] = t;
    i = o.src[0], o.src[0] = o.src[1], o.src[1] = i;
  }
  // equal depths with no time and no path: the straight line (.cc:3190-3200)
  o.straight = z1 == z0 && o.time[0] == 0 && o.path[0] == 0;
  if (o.straight) {
    if (x1 == 0) o.ignore[0] = o.ignore[1] = 0;
    o.path[0] = x1;
    o.time[0] = x1 / (iceray::kSpeedC / iceray::nz(m, z0));
    o.lang[0] = 90.;
    o.rang[0] = 90.;
    o.ignore[0] = 1;
  }
  return o;
}

// One focusing factor (.cc:3271-3283); at and lower are the receiver and the one 1 cm below
AIRICE_IR_HD inline double focusing_factor(const IceModel& m, double z0, double z1,
                                           const Chosen& at, const Chosen& lower, int k) {
  const double pi = iceray::kPi;
  const double nTx = iceray::nz(m, z0), nRx = iceray::nz(m, z1);
  const double recAng = at.rang[k] * (pi / 180), lauAng = at.lang[k] * (pi / 180);
  const double lauAngB = lower.lang[k] * (pi / 180);
  const double recPos = z1, recPosB = z1 - kLowerRx;
  return sqrt(((at.path[k] / (sin(recAng) * fabs((recPosB - recPos) / (lauAngB - lauAng)))) *
               (nTx / nRx)));
}

// GetRayTracingSolutions and -- with a lower row -- GetFocusingFactor for one pair.
// ray(c) / lower(c): column c of the solver's rows for (z0, x1, z1) and (z0, x1, z1 - 0.01);
// out.put(column, value) receives the kFields values, each as soon as it is final.  Returns the
// status byte.  A focusing factor whose condition is not met is 0.0 before the closing rule
// (zR == zT and factor 0 == 0 -> 1, .cc:3289); kFocus0 / kFocus1 say that the condition was met.
template <class Ray, class Lower, class Out>
AIRICE_IR_HD inline uint8_t solve_pair(const IceModel& m, const Medium& q, double z0, double x1,
                                       double z1, Ray&& ray, bool have_lower, Lower&& lower,
                                       Out&& out) {
  if (!(ray(iceray::kColStatus) < (double)iceray::kNonFinite)) {  // the solver ran no search
    for (int c = 0; c < kFields; c++)
      out.put(c, (c >> 1) == (kColIgnore >> 1) || (c >> 1) == (kColType >> 1) ? 0.0 : quiet_nan());
    return (uint8_t)kNonFinite;
  }
  const Chosen at = choose_and_order(m, z0, x1, z1, ray);
  int status = (at.ignore[0] ? kSlot0 : 0) | (at.ignore[1] ? kSlot1 : 0) |
               (at.straight ? kStraight : 0);
  for (int k = 0; k < 2; k++) {
    out.put(kColTime + k, at.time[k]);
    out.put(kColPath + k, at.path[k]);
    out.put(kColLaunch + k, at.lang[k]);
    out.put(kColReceive + k, at.rang[k]);
    out.put(kColIgnore + k, (double)at.ignore[k]);
    out.put(kColType + k, (double)(at.src[k] + 1));
  }
  // IncidenceAngleInIce (.cc:3007-3012), not swapped
  out.put(kColIncidence, 100.0);
  out.put(kColIncidence + 1, ray(8 + 1) == kNoRay ? 100.0 : ray(18));
  if (have_lower) {
    const double zl = z1 - kLowerRx;
    const Chosen lo = choose_and_order(m, z0, x1, zl, lower);
    double f[2] = {0.0, 0.0};
    for (int k = 0; k < 2; k++)
      if (at.rang[k] != kNoRay && lo.rang[k] != kNoRay) {
        f[k] = focusing_factor(m, z0, z1, at, lo, k);
        status |= kFocus0 << k;
      }
    if (z1 == z0 && f[0] == 0) f[0] = 1.;
    out.put(kColFocus, f[0]);
    out.put(kColFocus + 1, f[1]);
  } else {
    out.put(kColFocus, 0.0);
    out.put(kColFocus + 1, 0.0);
  }
  // AttRay = 1 - I of the slot's ray when that ray exists (its receive angle as the solver
  // reported it, .cc:2976-2987), else 0: the two slots' legs in one loop
  const int src0 = at.src[0], src1 = at.src[1];
  const double L0 = ray(19 + src0), L1 = ray(19 + src1);
  const bool has0 = ray(8 + src0) != kNoRay, has1 = ray(8 + src1) != kNoRay;
  double sum0 = 0, sum1 = 0;
  integrate_legs(m, q, 4, [&](int k) {
    const bool second = (k >> 1) != 0;
    const int type = (second ? src1 : src0) + 1;
    Leg g = ray_leg(type, k & 1, second ? L1 : L0, z0, z1);
    // no such ray, or a direct ray's second leg: an empty leg (both ends equal)
    if (!(second ? has1 : has0) || (type == 1 && (k & 1)))
      g.za = g.zb = 0.0, g.L = 0.0, g.turning = false;
    return g;
  }, sum0, sum1);
  out.put(kColAtt, has0 ? 1 - fabs(q.a0 * sum0) : 0.0);
  out.put(kColAtt + 1, has1 ? 1 - fabs(q.a0 * sum1) : 0.0);
  return (uint8_t)status;
}

// out.put for a plain array of kFields doubles
struct ArrayOut {
  double* v;
  AIRICE_IR_HD void put(int c, double x) { v[c] = x; }
};

}  // namespace icesol
}  // namespace airice
