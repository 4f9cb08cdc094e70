// airice_icespec.hpp -- the ice attenuation of a pair's two rays over a GRID of frequencies: what a
// consumer of GetRayTracingSolutions folds into a broadband pulse's spectrum, bin by bin.  Written
// once for the device (icesol_spectrum_kernel, airice_icespec.hip) and the host
// (icespec_host_one, airice_host.cpp; IceRayTracing::GetAttenuationSpectrum, compat_iceray.cpp).
//
// airice_icesol.hpp's integrand is  w_j 2 hw (1 / L_att) n sqrt(s^2 / (u (A - L)(n + L)))  at each
// of the 24 nodes of a leg, and 1 / L_att = exp(k0 + t (k1 + t k2)) is its only factor that knows
// the frequency: t is the node's temperature, the three k come from make_medium.  So a node is a
// record (t, g) -- g everything but 1 / L_att -- that holds for every bin, a bin is three numbers
// that hold for every node, and a spectrum of F bins is 96 records per pair and then F exps per
// record.  The legs are those solve_pair feeds integrate_legs (slot 0's two, then slot 1's two),
// over the slot order icesol_kernel wrote: the choice is read, not made again.  DESIGN.md §12.
#pragma once
#include "airice_icesol.hpp"

namespace airice {
namespace icespec {

using iceray::IceModel;
using iceray::quiet_nan;
using icesol::Leg;

constexpr int kLegs = 4;                          // two per slot
constexpr int kNodes = 2 * icesol::kGaussHalf;    // per leg
constexpr int kRecords = kLegs * kNodes;          // per pair: 96 records, 1,536 bytes

struct alignas(16) Node {  // one 16-byte LDS read
  double t, g;
};
struct Coeffs {
  double k0, k1, k2;
};

// make_medium's three numbers for one bin, in its arithmetic: f < 1 takes the low branch, 1.0 the
// high one.  A frequency that is not finite and positive gives NaN, so its column is NaN wherever
// the ray exists.
AIRICE_IR_HD inline Coeffs spectrum_coeffs(double frequency) {
  if (!(iceray::is_finite(frequency) && frequency > 0)) {
    const double nan = quiet_nan();
    return Coeffs{nan, nan, nan};
  }
  const double w = log(frequency);
  const bool low = frequency < 1.;
  const double wA = low ? log(0.0001) : 0.0, wB = low ? 0.0 : log(3.16);
  const double cA = (w - wB) / (wA - wB), cB = (wA - w) / (wA - wB);
  // the rows b0, b1 (low) or b1, b2 (high) of make_medium's table
  const double a0 = low ? -6.74890 : -6.22121, a1 = low ? 0.026709 : -0.070927,
               a2 = low ? -0.000884 : -0.001773;
  const double b0 = low ? -6.22121 : -4.09468, b1 = low ? -0.070927 : -0.002213,
               b2 = low ? -0.001773 : -0.000332;
  return Coeffs{a0 * cA + b0 * cB, a1 * cA + b1 * cB, a2 * cA + b2 * cB};
}

// The ray a slot holds, from the type column icesol_kernel wrote for it (1 D, 2 R, 3 Ra0, 4 Ra1;
// anything else reads as 1) and the solver's row: `has` is solve_pair's rule.
struct SlotRay {
  int type;
  bool has;
  double L;
};
template <class Ray>
AIRICE_IR_HD inline SlotRay slot_ray(Ray&& ray, double type_column) {
  const int src = type_column >= 2. ? (type_column >= 3. ? (type_column >= 4. ? 3 : 2) : 1) : 0;
  return SlotRay{src + 1, ray(8 + src) != icesol::kNoRay, ray(19 + src)};
}

// Leg k (0..3) of the pair as solve_pair hands it to integrate_legs: no such ray, or a direct
// ray's second leg, is an empty leg.
AIRICE_IR_HD inline Leg pair_leg(int k, const SlotRay& s, double z0, double z1) {
  Leg g = icesol::ray_leg(s.type, k & 1, s.L, z0, z1);
  if (!s.has || (s.type == 1 && (k & 1))) g.za = g.zb = 0.0, g.L = 0.0, g.turning = false;
  return g;
}

// What integrate_legs derives once per leg
struct Panel {
  double zv, mid, hw, L, AL;
};
AIRICE_IR_HD inline Panel leg_panel(const IceModel& m, const Leg& g) {
  const double zv = log(m.B / (g.L - m.A)) / m.C;
  const double sa = sqrt(g.za - zv);
  const double sb = g.turning ? 0.0 : sqrt(g.zb - zv);
  return Panel{zv, 0.5 * (sa + sb), 0.5 * (sb - sa), g.L, m.A - g.L};
}

// Node j (0..23) of a leg: its temperature and integrate_legs' summand without 1 / L_att, the
// panel's 2 hw included.  An empty leg (hw == 0) is g = 0; a leg integrate_legs makes NaN is NaN.
AIRICE_IR_HD inline Node node_record(const IceModel& m, const Panel& p, int j) {
  if (p.hw == 0.0) return Node{0.0, 0.0};
  const double x = icesol::gauss_x(j >> 1);
  const double s = p.mid + p.hw * ((j & 1) ? -x : x);
  const double s2 = s * s;
  const double u = -expm1(-m.C * s2);
  const double n = m.A + (p.L - m.A) * (1.0 - u);
  const double t = icesol::ice_temperature(p.zv + s2);
  const double g =
      (2.0 * p.hw * icesol::gauss_w(j >> 1)) * (n * sqrt(s2 / (u * (p.AL * (n + p.L)))));
  return Node{t, g};
}

// One node's share of one bin's leg sum
AIRICE_IR_HD inline double term(const Coeffs& c, const Node& r) {
  return exp(c.k0 + r.t * (c.k1 + r.t * c.k2)) * r.g;
}

// One bin's sum over a leg's records r[0 .. 23].  An empty leg's records are all g = 0 and add
// nothing, so they are not walked: 0.0 k0 is their sum -- 0.0, and NaN in a bin whose frequency is
// bad, as every term would have been.
AIRICE_IR_HD inline double leg_sum(const Coeffs& c, const Node* r, bool empty) {
  if (empty) return 0.0 * c.k0;
  double acc = 0;
  for (int j = 0; j < kNodes; j++) acc += term(c, r[j]);
  return acc;
}

// AttRay of a slot from its two leg sums: the reference's fabs per leg stays
AIRICE_IR_HD inline double attenuation(double a0, bool has, double leg0, double leg1) {
  return has ? 1 - fabs(a0 * (fabs(leg0) + fabs(leg1))) : 0.0;
}

// One pair on the calling thread: att0[k], att1[k] for the n_freq bins.  ray(c): column c of the
// solver's row; type0 / type1: the pair's two type columns of the icesol output.  A row the solver
// flagged non-finite is NaN in every bin of both slots.
template <class Ray>
inline void spectrum_pair(const IceModel& m, double a0, double z0, double z1, Ray&& ray,
                          double type0, double type1, const double* frequency, size_t n_freq,
                          double* att0, double* att1) {
  if (!(ray(iceray::kColStatus) < (double)iceray::kNonFinite)) {
    for (size_t k = 0; k < n_freq; k++) att0[k] = att1[k] = quiet_nan();
    return;
  }
  Node rec[kRecords];
  const SlotRay slot[2] = {slot_ray(ray, type0), slot_ray(ray, type1)};
  bool empty[kLegs];
  for (int k = 0; k < kLegs; k++) {
    const Panel p = leg_panel(m, pair_leg(k, slot[k >> 1], z0, z1));
    empty[k] = p.hw == 0.0;
    for (int j = 0; j < kNodes; j++) rec[k * kNodes + j] = node_record(m, p, j);
  }
  for (size_t k = 0; k < n_freq; k++) {
    const Coeffs c = spectrum_coeffs(frequency[k]);
    double leg[kLegs];
    for (int l = 0; l < kLegs; l++) leg[l] = leg_sum(c, rec + l * kNodes, empty[l]);
    att0[k] = attenuation(a0, slot[0].has, leg[0], leg[1]);
    att1[k] = attenuation(a0, slot[1].has, leg[2], leg[3]);
  }
}

}  // namespace icespec
}  // namespace airice
