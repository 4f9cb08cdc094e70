// airice_ray.hpp -- the forward ray of GetRayTracingSolutions (MultiRayAirIceRefraction.cc:
// 1796-2017) as __host__ __device__ functions: no kernels, no launchers.
//
// A ray is traced in two parts that meet at the ice surface: ray_air_part (the air layers, from
// the row's constants RowConst and the start sine) and ray_ice_part (the segment in the ice, the
// receive angle, the Fresnel coefficients, the 18 outputs); ray_solution_row is the one followed
// by the other, ray_solution the per-lane form with its own row constants.  The table and ray
// kernels (airice_table.hip) and the host route rays_host are written over them.  The ice part in
// a two-layer firn (the reference's TransitionBoundary != 0 model) is ray_ice_part_firn, DESIGN.md
// §14.  The minimizer's
// stage 2 (airice_minimizer.hpp) takes stop_of, fresnel_from_sine and sin_start from here and
// nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "airice_device.hpp"

namespace airice {

constexpr double kSpeedC = 299792458.0;  // .h:30

// ---------------------------------------------------------------------------
// Forward ray: GetRayTracingSolutions (.cc:1796-2017).  d[] = dummy[0..17].
// The layer loop follows the reference (each layer re-derives L from the incidence angle
// it receives, .cc:1871) with the running sine of identity (2).
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ Endpoint stop_of(const DevMedium& M, int l) {
  Endpoint r = M.stop[0];
  r = pick(l == 1, M.stop[1], r);
  r = pick(l == 2, M.stop[2], r);
  r = pick(l == 3, M.stop[3], r);
  return r;
}

// Fresnel T_S, T_P (.cc:285-337) at the incidence whose sine is v (identity (2):
// sin(asin(v) r2d d2r) = v, cos = sqrt(1 - v^2) on [0, 90] degrees).
// ratio = n1 / n2 (folded on the host, IceConsts::n_ratio).  The two quotients have positive
// denominators (n1, n2 > 0 and ct, sqterm >= 0, never both 0): div_pos.
__host__ __device__ __forceinline__ void fresnel_from_sine(double n1, double n2, double ratio, double v,
                                                  double& tS, double& tP) {
  const double st = v, ct = fast_sqrt(1 - v * v);
  const double a = ratio * st;
  const double sqterm = fast_sqrt(1 - a * a);
  double num = n1 * ct - n2 * sqterm;
  double den = n1 * ct + n2 * sqterm;
  tS = 1 + div_pos(num, den);
  if (__builtin_isnan(tS)) tS = 0;
  num = n1 * sqterm - n2 * ct;
  den = n1 * sqterm + n2 * ct;
  tP = (1 - div_pos(num, den)) * ratio;
  if (__builtin_isnan(tP)) tP = 0;
}

// Stop end of the Tx layer `top`.  Rays of one wave almost always share their Tx layer (a
// wave covers <= 2 table rows), so the entry is read with a wave-uniform (scalar) index;
// a wave that straddles a layer boundary falls back to per-lane selects.
__host__ __device__ __forceinline__ TopEnd topend_of(const IceConsts& I, int top) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int tu = __builtin_amdgcn_readfirstlane(top);
  if (__ballot(top != tu) == 0) return I.topend[tu];
#endif
  TopEnd r = I.topend[0];
#pragma unroll
  for (int l = 1; l < kMaxLayers; ++l) {
    const bool c = (top == l);
    const TopEnd& e = I.topend[l];
    r = TopEnd{c ? e.x : r.x,       c ? e.n : r.n,       c ? e.y2 : r.y2, c ? e.Ay : r.Ay,
               c ? e.invC : r.invC, c ? e.invCc : r.invCc, c ? e.Cx : r.Cx, c ? e.ACx : r.ACx};
  }
  return r;
}

// Everything of a ray that depends on its Tx height only: the Tx layer and the Tx layer's
// segment folded like the lower layers' (Tx endpoint -> the layer's stop end, or the ice).  The
// table computes it once per row into LDS (a block spans few rows); other launches per lane.
struct RowConst {
  SegConst seg;  // Tx endpoint -> stop end of the Tx layer (zero-length case resolved)
  double H;
  int top;       // MaxLayers - SkipLayersAbove - 1
  int any;       // top >= bot: at least one air layer
};

__host__ __device__ __forceinline__ RowConst row_const(const DevMedium& M, const IceConsts& I, double H) {
  RowConst rc;
  rc.H = H;
  rc.top = top_layer(M, H);
  rc.any = rc.top >= I.bot;
  const Endpoint T = air_endpoint(M, H);
  const TopEnd R_ = topend_of(I, rc.top);
  // zero-length (Tx exactly on the layer's lower bound / the ice): reuse the Tx end
  const bool zl = (R_.x == T.x);
  SegConst& s = rc.seg;
  s.Tn = T.n;
  s.Ty2 = T.y2;
  s.TAy = T.Ay;
  s.Rn = zl ? T.n : R_.n;
  s.Ry2 = zl ? T.y2 : R_.y2;
  s.RAy = zl ? T.Ay : R_.Ay;
  s.ratio = T.n / s.Rn;
  s.invC = zl ? T.invC : R_.invC;
  s.invCc = zl ? T.invC * (1.0 / kSpeedC) : R_.invCc;
  s.dCx = zl ? 0.0 : R_.Cx - T.Cx;
  s.dACx = zl ? 0.0 : R_.ACx - T.ACx;
  return rc;
}

// sin(x) for the start angle's radians, x = (180 - theta) pi/180 in [0, pi/2] for every launch
// angle in [90, 180]: odd Taylor polynomial to x^23 (truncation < 2^-59 relative on the range);
// other arguments go to ocml's sin.
__host__ __device__ __forceinline__ double sin_start(double x) {
  if (!(x >= 0.0 && x <= 1.5707963267948966)) return sin(x);
  const double x2 = x * x;
  // (-1)^k / (2k+1)!, k = 11 .. 1, as doubles
  double p = __builtin_fma(x2, -0x1.761b41316381ap-75, kc(0x1.71b8ef6dcf572p-66));  // 1/23!, 1/21!
  p = __builtin_fma(x2, p, kc(-0x1.2f49b46814157p-57));                             // 1/19!
  p = __builtin_fma(x2, p, kc(0x1.952c77030ad4ap-49));                              // 1/17!
  p = __builtin_fma(x2, p, kc(-0x1.ae7f3e733b81fp-41));                             // 1/15!
  p = __builtin_fma(x2, p, kc(0x1.6124613a86d09p-33));                              // 1/13!
  p = __builtin_fma(x2, p, kc(-0x1.ae64567f544e4p-26));                             // 1/11!
  p = __builtin_fma(x2, p, kc(0x1.71de3a556c734p-19));                              // 1/9!
  p = __builtin_fma(x2, p, kc(-0x1.a01a01a01a01ap-13));                             // 1/7!
  p = __builtin_fma(x2, p, kc(0x1.1111111111111p-7));                               // 1/5!
  p = __builtin_fma(x2, p, kc(-0x1.5555555555555p-3));                              // 1/3!
  return __builtin_fma(x * x2, p, x);
}

// I.lower[il].ratio for a lane-varying il (selects)
__host__ __device__ __forceinline__ double sel_lower_ratio(const IceConsts& I, int il) {
  double r = I.lower[0].ratio;
#pragma unroll
  for (int l = 1; l < kMaxLayers; ++l) r = (il == l) ? I.lower[l].ratio : r;
  return r;
}

// A ray is traced in two parts that meet at the ice surface.
// The AIR PART (ray_air_part) reads the medium, the ice height's constants (I.bot, I.lower), the
// row's constants (the Tx height) and the start sine (the launch angle) -- never the antenna depth
// -- so its result is the same for every antenna of one grid: the table launch keeps it per ray
// across launches (air_part_cached).  The ICE PART (ray_ice_part) forms the segment in the ice, the
// receive angle, the Fresnel coefficients and the 18 outputs from it.  ray_solution_row is exactly
// the air part followed by the ice part.
struct AirPart {
  double vinc;     // sine of the incidence on the ice; 0 when the ray crosses no air layer
  double thd_air;  // horizontal distance, time and geometric path summed over the air layers
  double t_air;
  double geo_air;
  double v;        // the running sine itself (dummy[12], want_inc)
  bool any;        // at least one air layer
};

// top_hi >= 0: a wave-uniform upper bound of the lanes' Tx layers (the table block's first row);
// the lower layers then run as one loop over a uniform layer index, their SegConst read with
// scalar loads one layer at a time, instead of one inlined copy per layer.  Same operations in
// the same order either way.
// A1: the launch's A_air is exactly 1 (MultiRayAirIceRefraction.h:99, the table's medium), so
// the products with it are dropped (exact: x * 1.0 == x).
// v: sine of StartAngle (.cc:1863)
template <bool A1 = false>
__host__ __device__ __forceinline__ AirPart ray_air_part(const DevMedium& M, const IceConsts& I,
                                                         const RowConst& rc, double v,
                                                         const double* tab, int top_hi) {
  const int top = rc.top;
  const int bot = I.bot;
  const double Aair = A1 ? 1.0 : M.A_air;
  const double A2 = Aair * Aair;
  double thd_air = 0.0, t_air = 0.0, geo_air = 0.0;
  const bool any = rc.any != 0;
  if (any) {
    // n_layer1 == Getnz_air(StartHeight) == nzTx: Snell into a layer is the identity
    const Segment s = segment_const(rc.seg, Aair, A2, sin_asin(v), true, v, tab);
    thd_air += s.thd;
    t_air += s.t;
    geo_air += s.geo;
  }
  // lower layers: both ends folded on the host (I.lower, scalar reads)
  if (top_hi >= 0) {
#pragma clang loop unroll(disable)
    for (int il = top_hi - 1; il >= bot; --il) {
      if (il < top) {
        // v is a segment's output sine here (already sin_asin'd: sin_asin is idempotent)
        const Segment s = segment_const(I.lower[il], Aair, A2, v, true, v, tab);
        thd_air += s.thd;
        t_air += s.t;
        geo_air += s.geo;
      }
    }
  } else {
#pragma unroll
    for (int il = kMaxLayers - 2; il >= 0; --il) {
      if (il >= top || il < bot) continue;
      const Segment s = segment_const(I.lower[il], Aair, A2, v, true, v, tab);
      thd_air += s.thd;
      t_air += s.t;
      geo_air += s.geo;
    }
  }
  AirPart a;
  a.vinc = any ? v : 0.0;
  // One NaN for the three sums.  An air segment's results are negated (segment_const: * -1), and
  // the compiler may fold that negation into a neighbouring operation differently in every kernel
  // this function is inlined into -- exact for numbers, but it leaves a NaN's sign to the kernel:
  // the 11-column table stored -NaN as geo_air where rays_kernel's double was +NaN.  With the
  // default NaN here the table, the air record and the per-lane rays carry the same bits.
  a.thd_air = __builtin_isnan(thd_air) ? __builtin_nan("") : thd_air;
  a.t_air = __builtin_isnan(t_air) ? __builtin_nan("") : t_air;
  a.geo_air = __builtin_isnan(geo_air) ? __builtin_nan("") : geo_air;
  a.v = v;
  a.any = any;
  return a;
}

// inc: dummy[12], formed by the caller (want_inc) from the air part's running sine.
// FRESNEL = false: d[14], d[15] are left 0 (the warm table launch has them in its air record).
template <bool FRESNEL = true>
__host__ __device__ __forceinline__ void ray_ice_part(const DevMedium& M, const IceConsts& I,
                                                      double H, double theta, bool in_ice,
                                                      double vinc, double thd_air, double t_air,
                                                      double geo_air, double inc, double* d,
                                                      const double* tab) {
  double thd_ice = 0.0, t_ice = 0.0, geo_ice = 0.0, recv_ice = 0.0;
  if (in_ice) {
    // .cc:1897-1922: n_layer1 = Getnz_air(IceLayerHeight), Rx = -AntennaDepth, Tx = 0
    const double A2i = M.A_ice * M.A_ice;
    const double u = sin_asin(I.n_ratio * vinc);
    double v2;
    const Segment s = segment_const(I.iceseg, M.A_ice, A2i, u, false, v2, tab);
    thd_ice += s.thd;
    t_ice += s.t;
    geo_ice += s.geo;
    recv_ice = k_asin(v2) * M.r2d;
  }
  double tS = 0.0, tP = 0.0;
  if constexpr (FRESNEL) fresnel_from_sine(I.n_air_ice, I.n_ice0, I.n_ratio, vinc, tS, tP);
  d[0] = 0;
  d[1] = H;
  d[2] = thd_air + thd_ice;
  d[3] = thd_air;
  d[4] = thd_ice;
  d[5] = (t_ice + t_air) * kSpeedC;
  d[6] = t_air * kSpeedC;
  d[7] = t_ice * kSpeedC;
  d[8] = (t_ice + t_air) * 1e9;
  d[9] = t_air * 1e9;
  d[10] = t_ice * 1e9;
  d[11] = theta;
  d[12] = inc;
  d[13] = recv_ice;
  d[14] = tS;
  d[15] = tP;
  d[16] = geo_air;
  d[17] = geo_ice;
}

// The ice part in a two-layer firn: M and I describe the upper layer, I.iceseg ends
// at the layer boundary when the antenna lies below it (F.below), and F.seg is the leg from the
// boundary to the antenna in the lower layer's model.  L = n sin(theta) is conserved across the
// index step, so the sine entering the lower leg is F.ratio_b times the upper leg's output sine.
// d[4], d[7], d[10], d[17] are the two legs' sums, d[13] is the angle at the antenna; the Fresnel
// coefficients stay those of the surface.  With F.below == 0 these are ray_ice_part's operations.
template <bool FRESNEL = true>
__host__ __device__ __forceinline__ void ray_ice_part_firn(const DevMedium& M, const IceConsts& I,
                                                           const FirnLeg& F, double H, double theta,
                                                           bool in_ice, double vinc, double thd_air,
                                                           double t_air, double geo_air, double inc,
                                                           double* d, const double* tab) {
  double thd_ice = 0.0, t_ice = 0.0, geo_ice = 0.0, recv_ice = 0.0;
  if (in_ice) {
    const double A2i = M.A_ice * M.A_ice;
    const double u = sin_asin(I.n_ratio * vinc);
    double v2;
    const Segment s = segment_const(I.iceseg, M.A_ice, A2i, u, false, v2, tab);
    thd_ice += s.thd;
    t_ice += s.t;
    geo_ice += s.geo;
    if (F.below != 0) {
      const double ub = sin_asin(F.ratio_b * v2);
      const Segment q = segment_const(F.seg, M.A_ice, A2i, ub, false, v2, tab);
      thd_ice += q.thd;
      t_ice += q.t;
      geo_ice += q.geo;
    }
    recv_ice = k_asin(v2) * M.r2d;
  }
  double tS = 0.0, tP = 0.0;
  if constexpr (FRESNEL) fresnel_from_sine(I.n_air_ice, I.n_ice0, I.n_ratio, vinc, tS, tP);
  d[0] = 0;
  d[1] = H;
  d[2] = thd_air + thd_ice;
  d[3] = thd_air;
  d[4] = thd_ice;
  d[5] = (t_ice + t_air) * kSpeedC;
  d[6] = t_air * kSpeedC;
  d[7] = t_ice * kSpeedC;
  d[8] = (t_ice + t_air) * 1e9;
  d[9] = t_air * 1e9;
  d[10] = t_ice * 1e9;
  d[11] = theta;
  d[12] = inc;
  d[13] = recv_ice;
  d[14] = tS;
  d[15] = tP;
  d[16] = geo_air;
  d[17] = geo_ice;
}

// want_inc: dummy[12] (the incidence angle on the ice, one asin) is not a table column
// (.cc:2101-2111), so table launches without the double output skip it.
// v_start: the sine of StartAngle, formed by the caller.
// F: the lower leg of a layered firn (ray_ice_part_firn), nullptr in the one-layer model.
template <bool A1 = false>
__host__ __device__ __forceinline__ void ray_solution_row(const DevMedium& M, const IceConsts& I,
                                                 const RowConst& rc, double theta, bool in_ice,
                                                 double* d, bool want_inc,
                                                 const double* tab = &kLogTable[0][0],
                                                 int top_hi = -1,
                                                 const double* v_start = nullptr,
                                                 const FirnLeg* F = nullptr) {
  // sine of StartAngle (.cc:1863); v_start: the same value, formed by the caller
  const double v = v_start != nullptr ? *v_start : sin_start((180 - theta) * M.d2r);
  const AirPart a = ray_air_part<A1>(M, I, rc, v, tab, top_hi);
  // IncidentAngleonIce = last layer's receive angle; 0 when no air layer (.cc:1832, 1881)
  double inc = 0.0;
  if (want_inc) inc = a.any ? k_asin(a.v) * M.r2d : 0.0;
  if (F != nullptr)
    ray_ice_part_firn(M, I, *F, rc.H, theta, in_ice, a.vinc, a.thd_air, a.t_air, a.geo_air, inc, d,
                      tab);
  else
    ray_ice_part(M, I, rc.H, theta, in_ice, a.vinc, a.thd_air, a.t_air, a.geo_air, inc, d, tab);
}

// Per-lane form (rays, minimizer evaluations): the row constants of its own Tx height.
__host__ __device__ __forceinline__ void ray_solution(const DevMedium& M, const IceConsts& I, double theta,
                                             double H, bool in_ice, double* d,
                                             bool want_inc = true, const FirnLeg* F = nullptr) {
  const RowConst rc = row_const(M, I, H);
  ray_solution_row(M, I, rc, theta, in_ice, d, want_inc, &kLogTable[0][0], -1, nullptr, F);
}

}  // namespace airice
