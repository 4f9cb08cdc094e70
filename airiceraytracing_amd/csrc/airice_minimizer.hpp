// airice_minimizer.hpp -- what one lane needs to solve and store one minimizer query
// (Air2IceRayTracing, MultiRayAirIceRefraction.cc:1464-1616): __host__ __device__ code, no
// kernels, no launchers.
//
// Two stages around one shared root finder (RootSearch / solve_root, also compiled for the host's
// one-query calls): stage 1 finds the launch angle -- bracket set-up, the 0.05-degree probe,
// GSL-bisection replay (tolerance 1e-9, 40 iterations) over a THD-only evaluator -- and stage 2
// (stage2_out) makes one full evaluation at the root (evaluate_root) and the entry point's stores.
// The five entry points -- Air2IceRayTracing in the MultiRay and the pythonwrapper variant,
// GetHorizontalDistanceToIntersectionPoint, the table lookup's fallback, TraceIceToAir -- are each
// described once (EntryPoint<OUT>: query source, park slots, stores).  The batch and one-query
// kernels, their launchers and the host route (airice_solve.hip) and the lookup's fallback lanes
// (lookup_lane, airice_lookup.hip) are written over this header.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "airice.h"
#include "airice_device.hpp"
#include "airice_lean.hpp"
#include "airice_ray.hpp"

namespace airice {

// ints per query of the AIRICE_SOLVE_STATS record: evaluations, secant steps, midpoints (Park::stats)
constexpr int kStatsInts = 3;
// evaluation-free bisection steps of the root finder per loop trip (as compare-and-select)
constexpr int kLeanUnroll = 4;

// ---------------------------------------------------------------------------
// Minimizer: per-query air path (GetAirPropagationPar .cc:661-804 semantics: the first
// layer derives L, the lower layers reuse it, .cc:757-771).
// ---------------------------------------------------------------------------
struct AirPath {
  Endpoint tx;      // Tx height endpoint
  Endpoint iceair;  // air model at the (possibly depth-shifted) ice height
  Endpoint rtop;    // Rx endpoint of the top layer
  int top, bot;
};


__host__ __device__ __forceinline__ AirPath make_air_path(const DevMedium& M, double H, double ice) {
  AirPath P;
  P.top = top_layer(M, H);
  P.bot = bottom_layer(M, ice);
  P.tx = air_endpoint(M, H);
  P.iceair = air_endpoint(M, ice);
  P.rtop = pick(P.top == P.bot, P.iceair, stop_of(M, P.top));
  P.rtop = pick(P.rtop.x == P.tx.x, P.tx, P.rtop);  // zero-length top segment
  return P;
}

// sin of the receive angle of the first layer (GetLayerHitPointPar .cc:562-589).
__host__ __device__ __forceinline__ double first_layer_v2(const DevMedium& M, double n_tx, double n_rtop,
                                                 double theta) {
  const double v1 = sin_start((180 - theta) * M.d2r);
  return sin_asin((n_tx * sin_asin(v1)) / n_rtop);
}

// The four endpoint quantities fDnfR needs (prim_D): a bisection keeps only these in VGPRs.
struct Slim {
  double y2, Ay, Cx, invC;
};

__host__ __device__ __forceinline__ Slim slim(const Endpoint& p) { return Slim{p.y2, p.Ay, p.Cx, p.invC}; }

__host__ __device__ __forceinline__ Slim pick(bool c, const Slim& a, const Slim& b) {
  return Slim{c ? a.y2 : b.y2, c ? a.Ay : b.Ay, c ? a.Cx : b.Cx, c ? a.invC : b.invC};
}

// Slim air endpoint at x >= 0 (Tx heights and ice heights are non-negative; a negative x
// would need y(x) != n(|x|), handled by the full Endpoint path).
__host__ __device__ __forceinline__ Slim air_slim(const DevMedium& M, double x, double& n) {
  const double zabs = fabs(x);
  const int l = air_layer(M, zabs);
  const double B = sel5(M.B, l), C = sel5(M.negC, l);
  const double e_abs = exp(C * zabs);
  n = M.A_air + B * e_abs;
  const double y = (x >= 0.0) ? n : M.A_air + B * exp(C * x);
  return Slim{y * y, M.A_air * y, C * x, 1.0 / C};
}

__host__ __device__ __forceinline__ Slim stop_slim(const DevMedium& M, int l) {
  Slim r = slim(M.stop[0]);
  r = pick(l == 1, slim(M.stop[1]), r);
  r = pick(l == 2, slim(M.stop[2]), r);
  r = pick(l == 3, slim(M.stop[3]), r);
  return r;
}

// Start endpoint of air layer l (scalar reads when l is wave-uniform, as start_slim below).
__host__ __device__ __forceinline__ Endpoint start_endpoint(const DevMedium& M, int l) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int lu = __builtin_amdgcn_readfirstlane(l);
  if (__ballot(l != lu) == 0) return M.start[lu];
#endif
  Endpoint r = M.start[0];
  r = pick(l == 1, M.start[1], r);
  r = pick(l == 2, M.start[2], r);
  r = pick(l == 3, M.start[3], r);
  return r;
}

// Start end of air layer l: a scalar read when l is the same on every lane of the wave (a batch
// with one ice height), per-lane selects otherwise.
__host__ __device__ __forceinline__ Slim start_slim(const DevMedium& M, int l) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int lu = __builtin_amdgcn_readfirstlane(l);
  if (__ballot(l != lu) == 0) return slim(M.start[lu]);
#endif
  Slim r = slim(M.start[0]);
  r = pick(l == 1, slim(M.start[1]), r);
  r = pick(l == 2, slim(M.start[2]), r);
  r = pick(l == 3, slim(M.start[3]), r);
  return r;
}

__host__ __device__ __forceinline__ double stop_n(const DevMedium& M, int l) {
  double r = M.stop[0].n;
  r = (l == 1) ? M.stop[1].n : r;
  r = (l == 2) ? M.stop[2].n : r;
  r = (l == 3) ? M.stop[3].n : r;
  return r;
}


// fDnfR(R) - fDnfR(T) with one logarithm when both ends share C (identity (5)).
// tab: the log table (the roots kernel's LDS copy, else the global one).
__host__ __device__ __forceinline__ double delta_D(const Slim& T, const Slim& R, const RayL& RL,
                                          const double* tab = &kLogTable[0][0]) {
  const double syR = fast_sqrt(R.y2 - RL.LL), syT = fast_sqrt(T.y2 - RL.LL);
  const double d1 = log_ratio(R.Ay - RL.LL + RL.sAL * syR, T.Ay - RL.LL + RL.sAL * syT, tab);
  return (RL.L * R.invC) * RL.rsAL * ((R.Cx - T.Cx) - d1);
}

// Per-query state of the root finder (MinforLAng_params + the air path's endpoints).
struct Query {
  Slim tx, rtop, iceair, rx;
  double n_tx, n_rtop;
  double ratio;  // n_tx / n_rtop: the first layer's Snell step (as the table's SegConst::ratio)
  int top, bot;
  double dist;
  double depth_pos;  // MinforLAng_params.antennadepth (> 0 in ice, 0 in air)
};

// Sum of per-layer horizontal distances in air for launch angle theta (THD only: the time
// and geometric-path terms do not enter f).  Returns L0 through the reference.
__host__ __device__ __forceinline__ double air_thd(const DevMedium& M, const Query& q, double theta,
                                          double& L0, const double* tab) {
  if (q.top < q.bot) {  // no layer: the reference reads unset output slots (UB)
    L0 = __builtin_nan("");
    return 0.0;
  }
  // first_layer_v2 with the per-query ratio and the start-angle polynomial (theta in [90, 180]
  // here; other angles go through ocml's sin inside sin_start)
  const double v1 = sin_start((180 - theta) * M.d2r);
  const double L = q.n_rtop * sin_asin(q.ratio * sin_asin(v1));
  L0 = L;
  const RayL RL = ray_L(M.A_air * M.A_air, L);
  // The reference's layer loop (top -> bot) in three parts with the same summation order: the
  // Tx layer (both ends per query), the layers strictly between (both ends layer bounds: uniform
  // across the wave, read as scalars, no per-lane selects; at most layers 2 and 1), the ice layer
  // (start bound of the lowest layer -> the query's ice endpoint).
  double thd = 0.0;
  {
    double x1 = delta_D(q.tx, q.rtop, RL, tab);
    x1 *= -1;
    thd += x1;
  }
#pragma unroll
  for (int il = kMaxLayers - 2; il >= 1; --il) {
    if (il < q.top && il > q.bot) {
      double x1 = delta_D(slim(M.start[il]), slim(M.stop[il]), RL, tab);
      x1 *= -1;
      thd += x1;
    }
  }
  if (q.top > q.bot) {
    double x1 = delta_D(start_slim(M, q.bot), q.iceair, RL, tab);
    x1 *= -1;
    thd += x1;
  }
  return thd;
}

// delta_D at two ray parameters (two launch angles) on the same segment: the two chains in one
// straight-line block, so each hides the other's latency; every value as delta_D forms it.
__host__ __device__ __forceinline__ void delta_D2(const Slim& T, const Slim& R, const RayL& Ra,
                                         const RayL& Rb, const double* tab, double& xa,
                                         double& xb) {
  const double syRa = fast_sqrt(R.y2 - Ra.LL), syTa = fast_sqrt(T.y2 - Ra.LL);
  const double syRb = fast_sqrt(R.y2 - Rb.LL), syTb = fast_sqrt(T.y2 - Rb.LL);
  double da, db;
  log_ratio2(R.Ay - Ra.LL + Ra.sAL * syRa, T.Ay - Ra.LL + Ra.sAL * syTa,
             R.Ay - Rb.LL + Rb.sAL * syRb, T.Ay - Rb.LL + Rb.sAL * syTb, tab, da, db);
  xa = (Ra.L * R.invC) * Ra.rsAL * ((R.Cx - T.Cx) - da);
  xb = (Rb.L * R.invC) * Rb.rsAL * ((R.Cx - T.Cx) - db);
}

// MinimizeforLaunchAngle's THD in air and in the ice at two angles (the root finder's bracket
// ends f(lo), f(hi)), as air_thd + the ice term of solve_root's evaluation site computes each:
// the same operations in the same order per angle, the two angles' chains interleaved.
__host__ __device__ __forceinline__ void eval_thd2(const DevMedium& M, const IceConsts& I, const Query& q,
                                          double ta, double tb, const double* tab,
                                          double& air_a, double& ice_a, double& air_b,
                                          double& ice_b) {
  double La = __builtin_nan(""), Lb = __builtin_nan("");
  air_a = 0.0;
  air_b = 0.0;
  if (q.top >= q.bot) {
    const double v1a = sin_start((180 - ta) * M.d2r);
    const double v1b = sin_start((180 - tb) * M.d2r);
    La = q.n_rtop * sin_asin(q.ratio * sin_asin(v1a));
    Lb = q.n_rtop * sin_asin(q.ratio * sin_asin(v1b));
    const RayL Ra = ray_L(M.A_air * M.A_air, La), Rb = ray_L(M.A_air * M.A_air, Lb);
    double xa, xb;
    delta_D2(q.tx, q.rtop, Ra, Rb, tab, xa, xb);
    xa *= -1;
    xb *= -1;
    air_a += xa;
    air_b += xb;
#pragma unroll
    for (int il = kMaxLayers - 2; il >= 1; --il) {
      if (il < q.top && il > q.bot) {
        delta_D2(slim(M.start[il]), slim(M.stop[il]), Ra, Rb, tab, xa, xb);
        xa *= -1;
        xb *= -1;
        air_a += xa;
        air_b += xb;
      }
    }
    if (q.top > q.bot) {
      delta_D2(start_slim(M, q.bot), q.iceair, Ra, Rb, tab, xa, xb);
      xa *= -1;
      xb *= -1;
      air_a += xa;
      air_b += xb;
    }
  }
  ice_a = 0;
  ice_b = 0;
  if (q.depth_pos != 0) {
    const RayL Ra = ray_L(M.A_ice * M.A_ice, La), Rb = ray_L(M.A_ice * M.A_ice, Lb);
    double xa, xb;
    delta_D2(slim(I.ice0), q.rx, Ra, Rb, tab, xa, xb);
    ice_a += xa;
    ice_b += xb;
  }
}

// Two evaluations of f spread over a wave, for one-query calls (scalar_solve_kernel): lanes 0-4
// take the Tx layer, layers 2 and 1 (when strictly between), the ice layer and the segment in the
// ice at theta_a, lanes 32-36 the same at theta_b, each with the same delta_D as air_thd, and the
// sums are formed in air_thd's order from the lanes' values -- the same bits as the one-lane
// evaluation, with ~1/4 of its dependent chain.  Every lane holds the same query, so everything
// else stays wave-uniform.
__device__ __forceinline__ void eval_thd_wave(const DevMedium& M, const IceConsts& I,
                                              const Query& q, double theta_a, double theta_b,
                                              const double* tab, double& thd_air_a,
                                              double& thd_ice_a, double& thd_air_b,
                                              double& thd_ice_b) {
  const int lane = (int)(threadIdx.x & 31);
  const double theta = (threadIdx.x & 32) ? theta_b : theta_a;
  const bool air = q.top >= q.bot;
  double L = __builtin_nan("");
  if (air) {
    const double v1 = sin_start((180 - theta) * M.d2r);
    L = q.n_rtop * sin_asin(q.ratio * sin_asin(v1));
  }
  const bool ice = lane == 4;
  const RayL RL = ray_L(ice ? M.A_ice * M.A_ice : M.A_air * M.A_air, L);
  Slim T = q.tx, R = q.rtop;  // lane 0 (and the lanes past 4, whose value is unused)
  T = pick(lane == 1, slim(M.start[2]), T);
  R = pick(lane == 1, slim(M.stop[2]), R);
  T = pick(lane == 2, slim(M.start[1]), T);
  R = pick(lane == 2, slim(M.stop[1]), R);
  T = pick(lane == 3, slim(M.start[0]), T);
  T = pick(lane == 3 && q.bot >= 1, slim(M.start[1]), T);
  T = pick(lane == 3 && q.bot >= 2, slim(M.start[2]), T);
  T = pick(lane == 3 && q.bot >= 3, slim(M.start[3]), T);
  R = pick(lane == 3, q.iceair, R);
  T = pick(ice, slim(I.ice0), T);
  R = pick(ice, q.rx, R);
  const double x = delta_D(T, R, RL, tab);
  auto sums = [&](int l0, double& thd_air, double& thd_ice) {
    const double d0 = __shfl(x, l0), d1 = __shfl(x, l0 + 1), d2 = __shfl(x, l0 + 2),
                 d3 = __shfl(x, l0 + 3), d4 = __shfl(x, l0 + 4);
    thd_air = 0.0;
    if (air) {
      thd_air += -d0;
      if (2 < q.top && 2 > q.bot) thd_air += -d1;
      if (1 < q.top && 1 > q.bot) thd_air += -d2;
      if (q.top > q.bot) thd_air += -d3;
    }
    thd_ice = 0;
    if (q.depth_pos != 0) thd_ice += d4;
  };
  sums(0, thd_air_a, thd_ice_a);
  sums(32, thd_air_b, thd_ice_b);
}

// ---------------------------------------------------------------------------
// Air2IceRayTracing (.cc:1464-1616) in two launches: stage 1 finds the launch angle
// (bracket, probe, bisection) keeping only the slim per-query state live; stage 2 rebuilds
// the full endpoints and evaluates every output at the root.  Splitting keeps the
// register-hungry full evaluation out of the bisection kernel's allocation.  Stage 1 parks
// the root and status in output slots that stage 2 overwrites.
// ---------------------------------------------------------------------------
struct Geometry {
  double H, D, ice, depth;  // after the Rx-in-air shift (.cc:1472-1479)
  double depth_pos;         // MinforLAng_params.antennadepth
};

__host__ __device__ __forceinline__ Geometry shift(double H, double D, double ice, double depth) {
  Geometry g;
  g.H = H;
  g.D = D;
  if (depth >= 0) {
    g.ice = depth + ice;
    g.depth = 0;
    g.depth_pos = 0;
  } else {
    g.ice = ice;
    g.depth = depth;
    g.depth_pos = -depth;
  }
  return g;
}

// What the root finder returns for one query.
struct SolveResult {
  double root;
  int status;
  int n_eval, n_est, n_inside;  // evaluations: all, secant search, bisection midpoints (stats)
};

enum { PH_PROBE = 0, PH_FLO = 1, PH_FHI = 2, PH_EST = 3, PH_G1 = 4, PH_G2 = 5, PH_BISECT = 6,
       PH_DONE = 7 };

// Quotients and the first guess's tangent that only steer the search (the root comes from GSL's
// bisection replay): v_rcp_f64 (~2^-24 relative) and the fast single-precision tangent on the
// device, the plain forms on the host.
__host__ __device__ __forceinline__ double rcp_steer(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcp(x);
#else
  return 1.0 / x;
#endif
}
// isfinite / isnan as each pass has them (ocml's on the device: the kernels' code is unchanged)
__host__ __device__ __forceinline__ bool k_isfinite(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return isfinite(x);
#else
  return std::isfinite(x);
#endif
}
__host__ __device__ __forceinline__ bool k_isnan(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return isnan(x);
#else
  return std::isnan(x);
#endif
}
__host__ __device__ __forceinline__ float tanf_steer(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __tanf(x);
#else
  return std::tan(x);
#endif
}

// The air model at the ice height of a batch whose queries share it (the ice end of every air
// path), formed once per block by the kernel: x the ice height it is for, bot its layer.
struct IceAirPre {
  Slim s;
  double n, x;
  int bot;
};

// The root finder of one query as a state machine with a single evaluation site (RootSearch):
// begin() sets up the bracket and the probe, next_point() runs the evaluation-free bisection
// steps and returns the point to evaluate next, update() takes f there.  solve_root() below drives
// one query to its root.
struct RootSearch {
  Query q;
  double lo, hi;
  double f_lower, f_upper;
  double tau;
  // Sign guards.  f(theta) = D - THD(theta) is monotone in theta wherever it is finite, so
  // between two exactly evaluated points with the same sign and |f| >= tau (far above the
  // evaluation's rounding noise) every point has that sign.  gL / gR: the innermost evaluated
  // points with the sign of f(lo) / f(hi); okL / okR: |f(lo)| / |f(hi)| >= tau, so the guard
  // regions [lo, gL] / [gR, hi] are safe.  A secant search finds the root, two guards straddle
  // it, and the bisection then evaluates f only at midpoints between the guards: the same
  // midpoints, signs and root as evaluating every one (tests/test_gpu_bisect_replay.py checks
  // this bit for bit against AIRICE_BISECT_EXACT=1).
  double gL, fL, gR, fR;  // fL holds f(lo) between PH_FLO and PH_FHI
  // secant search for the root: the first step in u = tan(180 - theta), where THD is close to
  // linear (a straight ray's is exactly H u; single precision is plenty for a first guess), then
  // steps on the last points (x1, f1), (x2, f2) and, from the second search point on, inverse
  // quadratic interpolation through (x0, f0) as well (the secant step plus a curvature term).
  // PH_G1/G2: guards at x2 -/+ dlt, where x2 is the search's last point (it stays put after the
  // search) and dlt lives in x1 (dead once the search ends).
  double x0, f0, x1, f1, x2, f2;
  int phase, status, iter, est, n_eval, n_inside;
  bool root_zero;  // the failed probe reports root 0 (.cc:1500-1509)
  bool okL, okR, exact;

  __host__ __device__ __forceinline__ double& dlt() { return x1; }

  // Air2IceRayTracing's set-up (.cc:1487-1509): the query's endpoints, the bracket [thR - 16, thR]
  // and the 0.05-degree probe.  An uninitialised solver state (non-finite bracket end) is modelled
  // as zeros.
  __host__ __device__ __forceinline__ void begin(const DevMedium& M, const IceConsts& I, const Geometry& g,
                                        double thR, bool exact_,
                                        const IceAirPre* pre = nullptr) {
    status = 0;
    exact = exact_;
    q.depth_pos = g.depth_pos;
    q.dist = g.D;
    q.top = top_layer(M, g.H);
    // the ice end: the block's copy when every lane of the wave has the batch's ice height
    bool have_pre = false;
    if (pre != nullptr) {
#if defined(__HIP_DEVICE_COMPILE__)
      have_pre = __ballot(g.ice != pre->x) == 0;
#else
      have_pre = g.ice == pre->x;
#endif
    }
    double n_ice;
    if (have_pre) {
      q.bot = pre->bot;
      q.iceair = pre->s;
      n_ice = pre->n;
    } else {
      q.bot = bottom_layer(M, g.ice);
      q.iceair = air_slim(M, g.ice, n_ice);
    }
    q.tx = air_slim(M, g.H, q.n_tx);
    // Rx end of the top layer: the ice, or the layer's lower boundary (stop endpoint)
    const bool to_ice = q.top == q.bot;
    q.rtop = pick(to_ice, q.iceair, stop_slim(M, q.top));
    q.n_rtop = to_ice ? n_ice : stop_n(M, q.top);
    const double x_rtop = to_ice ? g.ice : sel5(M.atm, q.top);
    if (x_rtop == g.H) {  // zero-length top segment (see segment())
      q.rtop = q.tx;
      q.n_rtop = q.n_tx;
    }
    q.ratio = q.n_tx / q.n_rtop;
    {
      const double e = exp(M.negC_ice * g.depth_pos);
      const double y = M.A_ice + M.B_ice * e;
      // 1/C of the ice from the host-folded surface endpoint (the same IEEE quotient): a kernel
      // argument, so it occupies no VGPRs across the loop
      q.rx = Slim{y * y, M.A_ice * y, M.negC_ice * g.depth_pos, I.ice0.invC};
    }
    lo = thR - 16;
    hi = thR;
    phase = PH_FLO;
    bool probe_bad = false;  // the probe ended with lo > hi: the reference then reports root 0
    if (M.const_air) lo = 90;  // pythonwrapper constant air index: [90, thR], no probe (.cc:978-980)
    if (!M.const_air && lo < 90.001) {
      lo = 90.001;
      phase = PH_PROBE;
      // While n(Tx) sin(180-lo) exceeds 1 by a margin (1e-6) the ray parameter L > A_air = 1,
      // so sqrt(A^2-L^2) and THD are NaN whatever the rounding: those probe steps need no
      // evaluation (.cc:1496-1509 would reject each of them).
      if (q.top >= q.bot) {
        const double thr = 180 - asin((1 + 1e-6) / q.n_tx) * M.r2d;  // NaN if n(Tx) < 1+1e-6
        // while (lo < thr && !(lo > hi - 0.1)) lo = lo + 0.05, in closed form (airice_lean.hpp)
        bool stepped;
        lo = probe_steps(lo, 0.05, hi - 0.1, thr, true, stepped);
        if (stepped) status |= AIRICE_SOLVE_PROBED;
      } else {
        // no air layer (Tx above the atmosphere, e.g. the table lookup's x100 fallback): THD in
        // air is 0 at every angle, so the probe only stops at lo > hi - 0.1 -- up to ~900 steps
        // whose outcome needs no evaluation, taken in closed form (airice_lean.hpp)
        bool stepped;
        lo = probe_steps(lo, 0.05, hi - 0.1, 0.0, false, stepped);
        if (stepped) status |= AIRICE_SOLVE_PROBED;
        if (hi < 90.001 && hi > 90.00) hi = 90.05;
        phase = PH_FLO;
        if (lo > hi) {
          status |= AIRICE_SOLVE_BAD_BRACKET;
          probe_bad = true;
          phase = PH_DONE;
        }
      }
    } else {
      if (hi < 90.001 && hi > 90.00) hi = 90.05;
      if (lo > hi) {  // gsl_root_fsolver_set: EINVAL, nothing initialised
        status |= AIRICE_SOLVE_BAD_BRACKET;
        phase = PH_DONE;
      }
    }
    // GSL's reported root is 0.5 (lo + hi) of the final bracket on every path (each iterate sets
    // it so, and the exact-zero exits make lo == hi), except the failed probe, which reports 0:
    // the root is formed once at the end instead of being carried through the loop
    root_zero = probe_bad;
    f_lower = 0.0;
    f_upper = 0.0;
    iter = 0;
    tau = 1e-6 + 1e-10 * fabs(g.D);
    okL = false;
    okR = false;
    gL = fL = gR = fR = 0.0;
    x0 = f0 = x1 = f1 = x2 = f2 = 0.0;
    est = 0;
    n_eval = 0;
    n_inside = 0;
  }

  __host__ __device__ __forceinline__ void guard(double x, double f) {
    if (!(fabs(f) >= tau) || !(x > gL && x < gR)) return;
    if ((f < 0.0) == (fL < 0.0)) {
      gL = x;
      fL = f;
    } else {
      gR = x;
      fR = f;
    }
  }

  // gsl_root_test_interval(lo, hi, 0, 1e-9) and the driver's max_iter (.cc:355-371)
  __host__ __device__ __forceinline__ void finish(bool frozen) {
    const double tol = 0.000000001;
    bool cont;
    if (lo > hi) {
      cont = false;
    } else {
      const double min_abs = ((lo > 0.0 && hi > 0.0) || (lo < 0.0 && hi < 0.0))
                                 ? (fabs(lo) < fabs(hi) ? fabs(lo) : fabs(hi))
                                 : 0.0;
      const double tolerance = 0 + tol * min_abs;
      cont = !(fabs(hi - lo) < tolerance);
    }
    if (cont && iter == 40) status |= AIRICE_SOLVE_MAXITER;
    if (frozen || !cont || iter == 40) phase = PH_DONE;
  }

  // gsl_root_fsolver_set's second end, f(hi) (fL holds f(lo)): the bracket state, the guards and
  // the secant search's first guess
  __host__ __device__ __forceinline__ void on_fhi(const DevMedium& M, double f) {
    phase = PH_BISECT;
    if (!k_isfinite(f)) {
      status |= AIRICE_SOLVE_NONFINITE_END;
    } else {
      f_lower = fL;
      f_upper = f;
      if (!exact) {
        gL = lo;
        gR = hi;
        fR = f;
        okL = fabs(fL) >= tau;
        okR = fabs(fR) >= tau;
        if (okL && okR) {
          if ((fL < 0.0) == (fR < 0.0)) {
            gL = hi;  // no sign change: every midpoint has the ends' sign
          } else {
            const float ul = tanf_steer((float)((180 - lo) * M.d2r));
            const float uh = tanf_steer((float)((180 - hi) * M.d2r));
            const float un = uh - (float)fR * ((uh - ul) / (float)(fR - fL));
            x1 = hi;
            f1 = fR;
            x0 = lo;
            f0 = fL;
            x2 = 180 - (double)atanf(un) * M.r2d;  // first guess, evaluated first
            phase = PH_EST;
          }
        }
      }
    }
  }

  // f(lo) and f(hi) in one pass (eval_thd2: two independent chains per lane, ~1.3x the time of one
  // evaluation instead of 2x); a lane that is probing reaches PH_FLO in the loop and evaluates the
  // ends there
  __host__ __device__ __forceinline__ void ends_paired(const DevMedium& M, const IceConsts& I,
                                              const double* tab) {
    if (phase != PH_FLO) return;
    double air_a, ice_a, air_b, ice_b;
    eval_thd2(M, I, q, lo, hi, tab, air_a, ice_a, air_b, ice_b);
    const double fa = (q.dist - (ice_a + air_a));
    ++n_eval;
    if (!k_isfinite(fa)) {
      status |= AIRICE_SOLVE_NONFINITE_END;
      phase = PH_BISECT;
    } else {
      fL = fa;
      ++n_eval;
      on_fhi(M, q.dist - (ice_b + air_b));
    }
  }

  // The evaluation-free bisection steps and the next point to evaluate.  False: the query is done
  // (phase PH_DONE) without another evaluation.
  __host__ __device__ __forceinline__ bool next_point(const DevMedium& M, double& x) {
    const double tol = 0.000000001;
    if (phase == PH_BISECT) {
      // steps that need no evaluation: an exact zero at a bracket end (GSL returns that end),
      // or a midpoint inside a guard region, whose sign is the region's: lo (left) or hi
      // (right) moves to it, as gsl_root_fsolver_iterate would
      if (f_lower == 0.0 || f_upper == 0.0) {
        ++iter;
        const double r0 = (f_lower == 0.0) ? lo : hi;
        lo = r0;
        hi = r0;
        finish(false);
        phase = PH_DONE;  // lo == hi: gsl_root_test_interval converges
        return false;
      }
      if ((okL || okR) && lo > 0.0) {
        // lean run (0 < lo < hi here): the root GSL reports after a step is 0.5 (lo + hi) of the
        // new bracket either way; the interval test reduces to hi - lo < tol lo
        const double gl = okL ? gL : -1.0, gr = okR ? gR : __builtin_inf();
        const double lo0 = lo, hi0 = hi;
        bool done = false;
        // the whole run in closed form when its midpoints are exact (airice_lean.hpp: every
        // bracket the probe did not move), the same lo, hi, steps and exit as the steps below
        LeanRun lr;
        if (lean_closed(lo, hi, iter, gL, gR, okL, okR, tol, lr)) {
          lo = lr.lo;
          hi = lr.hi;
          iter += lr.steps;
          status = lr.maxiter ? (status | AIRICE_SOLVE_MAXITER) : status;
          done = lr.done;
        } else {
          // the steps as selects, four per trip, so that the chain is midpoint -> compare ->
          // select without a divergent exit per step
          bool stop = false;
          while (!stop) {
#pragma unroll
            for (int u = 0; u < kLeanUnroll; ++u) {
              const double xm = (lo + hi) / 2.0;
              const bool inL = xm <= gl, inR = !inL && xm >= gr;
              const bool mv = !stop && (inL || inR);  // otherwise: evaluate this midpoint
              lo = (mv && inL) ? xm : lo;
              hi = (mv && inR) ? xm : hi;
              iter += mv ? 1 : 0;
              const bool cont = !(fabs(hi - lo) < 0 + tol * lo);
              const bool fin = mv && (!cont || iter == 40);
              status = (fin && cont) ? (status | AIRICE_SOLVE_MAXITER) : status;
              done = done || fin;
              stop = stop || !mv || fin;
            }
          }
        }
        if (lo != lo0) f_lower = fL;
        if (hi != hi0) f_upper = fR;
        if (done) {
          phase = PH_DONE;
          return false;
        }
      }
    }
    if (phase == PH_FHI) {
      x = hi;
    } else if (phase == PH_BISECT) {
      x = (lo + hi) / 2.0;
    } else if (phase == PH_EST) {
      // the secant point only steers the search (the root comes from GSL's bisection replay), so
      // its quotient takes v_rcp_f64 (~2^-24 relative) instead of the IEEE division
      x = (est == 0) ? x2 : x2 - f2 * ((x2 - x1) * rcp_steer(f2 - f1));
      // theta(f) through (x0, f0), (x1, f1), (x2, f2) in Newton form, at f = 0: the secant step
      // minus f1 f2 times the second divided difference (the search only steers; a point outside
      // the guards falls back to their midpoint below)
      if (est >= 1) {
        const double d1 = (x2 - x1) * rcp_steer(f2 - f1);
        const double d0 = (x1 - x0) * rcp_steer(f1 - f0);
        x += f1 * f2 * ((d1 - d0) * rcp_steer(f2 - f0));
      }
      if (!(x > gL && x < gR)) x = 0.5 * (gL + gR);  // safeguard: the guards' midpoint
    } else if (phase == PH_G1) {
      x = x2 - dlt();
    } else if (phase == PH_G2) {
      x = x2 + dlt();
    } else {
      x = lo;
    }
    return true;
  }

  // f = D - THD at x, the point next_point() returned.  REUSE_PROBE: a probing lane's last probe
  // evaluation (at x = lo, the point gsl_root_fsolver_set evaluates next) is taken as f(lo).
  template <bool REUSE_PROBE>
  __host__ __device__ __forceinline__ void update(const DevMedium& M, double x, double thd_air,
                                         double thd_ice) {
    ++n_eval;
    n_inside += (phase == PH_BISECT);
    const double f = (q.dist - (thd_ice + thd_air));
    if (phase == PH_PROBE) {
      if ((!k_isnan(thd_air) && thd_air > 0) || lo > hi - 0.1) {
        if (hi < 90.001 && hi > 90.00) hi = 90.05;
        phase = PH_FLO;
        if (lo > hi) {
          status |= AIRICE_SOLVE_BAD_BRACKET;
          root_zero = true;
          phase = PH_DONE;
        } else if (REUSE_PROBE) {
          // this trip evaluated f at x = lo, the point gsl_root_fsolver_set evaluates next
          // (f(lo)): the same point and arithmetic, so its value is PH_FLO's result and the lane
          // goes on to f(hi) one trip earlier
          if (!k_isfinite(f)) {
            status |= AIRICE_SOLVE_NONFINITE_END;
            phase = PH_BISECT;
          } else {
            fL = f;
            phase = PH_FHI;
          }
        }
      } else {
        lo = lo + 0.05;
        status |= AIRICE_SOLVE_PROBED;
      }
    } else if (phase == PH_FLO) {
      if (!k_isfinite(f)) {
        status |= AIRICE_SOLVE_NONFINITE_END;
        phase = PH_BISECT;
      } else {
        fL = f;
        phase = PH_FHI;
      }
    } else if (phase == PH_FHI) {
      on_fhi(M, f);
    } else if (phase == PH_EST) {
      if (est > 0) {
        x0 = x1;
        f0 = f1;
        x1 = x2;
        f1 = f2;
      }
      x2 = x;
      f2 = f;
      ++est;
      if (!k_isfinite(f)) {
        phase = PH_BISECT;
      } else if (fabs(f) < tau) {
        // at the root: guards a few tau either side, scaled by the local secant slope
        const double sl = (x2 - x1) * rcp_steer(f2 - f1);  // dtheta / df
        const double a = (x2 - x1) * (f1 - f0), b = (x1 - x0) * (f2 - f1);  // (before dlt takes x1)
        dlt() = 4.0 * tau * fabs(sl);
        const bool room = dlt() > 0.0 && dlt() < (gR - gL);
        // x1 is a search point near the root (est >= 2), so the secant slope through it is the
        // local one, and f at x2 -+ dlt is f2 -+ 4 tau sign(sl) to first order: |.| >= 3 tau with
        // the root between.  The guards then take those signs without evaluating f there -- when
        // the slope is consistent: the previous secant slope (x0, x1) has the same sign and is
        // within 2x of it (sl (f2 - f1) = x2 - x1 and its twin, compared as products: no
        // quotient, and any NaN fails), so f's curvature cannot have moved the root out of
        // [x2 - dlt, x2 + dlt].  Otherwise, and for the first search point (x1 is the bracket
        // end), both guards are evaluated (a side whose guard already lies at the root needs none).
        const bool consistent = a * b > 0.0 && fabs(a) <= 2.0 * fabs(b) && fabs(b) <= 2.0 * fabs(a);
        if (room && est >= 2 && consistent) {
          const double fm = sl > 0.0 ? -tau : tau;  // f(x2 - dlt)
          guard(x2 - dlt(), fm);
          guard(x2 + dlt(), -fm);
          phase = PH_BISECT;
        } else {
          const bool needL = !(x2 - gL <= 0.0), needR = !(gR - x2 <= 0.0);
          phase = room ? (needL ? PH_G1 : (needR ? PH_G2 : PH_BISECT)) : PH_BISECT;
        }
      } else {
        guard(x, f);
        if (est >= 12) phase = PH_BISECT;
      }
    } else if (phase == PH_G1 || phase == PH_G2) {
      if (k_isfinite(f)) guard(x, f);
      phase = phase == PH_G1 ? PH_G2 : PH_BISECT;
    } else {  // PH_BISECT: gsl_root_fsolver_iterate at a midpoint between the guards
      if (!exact && k_isfinite(f)) guard(x, f);
      ++iter;
      bool frozen = false;
      if (!k_isfinite(f)) {
        // EBADFUNC leaves the state unchanged: every later iterate repeats this one, so the
        // driver ends at max_iter with the same root.
        status |= AIRICE_SOLVE_STALE_MID | AIRICE_SOLVE_MAXITER;
        frozen = true;
      } else if (f == 0.0) {
        lo = x;
        hi = x;
      } else if ((f_lower > 0.0 && f < 0.0) || (f_lower < 0.0 && f > 0.0)) {
        hi = x;
        f_upper = f;
      } else {
        lo = x;
        f_lower = f;
      }
      finish(frozen);
    }
  }

  __host__ __device__ __forceinline__ double root() const { return root_zero ? 0.0 : 0.5 * (lo + hi); }
};

// MinimizeforLaunchAngle's f terms at theta (.cc:873-917): THD in air and in the ice.
__host__ __device__ __forceinline__ void eval_thd(const DevMedium& M, const IceConsts& I, const Query& q,
                                         double theta, const double* tab, double& thd_air,
                                         double& thd_ice) {
  double L;
  thd_air = air_thd(M, q, theta, L, tab);
  thd_ice = 0;
  if (q.depth_pos != 0) {
    const RayL RL = ray_L(M.A_ice * M.A_ice, L);
    thd_ice += delta_D(slim(I.ice0), q.rx, RL, tab);
  }
}

// Root finding of Air2IceRayTracing (.cc:1487-1521): the probe loop, gsl_root_fsolver_set and the
// FindFunctionRoot driver (.cc:340-374) with gsl_root_fsolver_bisection +
// gsl_root_test_interval(lo, hi, 0, 1e-9) semantics, as one per-lane state machine with a single
// evaluation site: lanes that are probing, setting up the bracket or bisecting share each
// evaluation instead of waiting for each other (the probe runs in ~7% of queries).
// WAVE: one query per wave (scalar_solve_kernel), each evaluation spread over the lanes.
template <bool WAVE = false>
__host__ __device__ __forceinline__ SolveResult solve_root(const DevMedium& M, const IceConsts& I,
                                                  const Geometry& g, double thR, bool exact,
                                                  const double* tab,
                                                  const IceAirPre* pre = nullptr) {
  RootSearch s;
  s.begin(M, I, g, thR, exact, pre);
  if constexpr (!WAVE) s.ends_paired(M, I, tab);
  // WAVE: f(lo) and f(hi), and the two guards, are independent pairs of points; the wave evaluates
  // each pair at once and keeps the second value for the next trip (the same points, the same
  // bits, two sequential evaluations fewer)
  bool have_next = false;
  double next_air = 0.0, next_ice = 0.0;
  while (s.phase != PH_DONE) {
    if constexpr (WAVE) {
      // one query per wave: the phase and the counters are the same on every lane; scalar copies
      // let the phase dispatch branch on SCC instead of exec masks
      s.phase = __builtin_amdgcn_readfirstlane(s.phase);
      s.est = __builtin_amdgcn_readfirstlane(s.est);
      s.iter = __builtin_amdgcn_readfirstlane(s.iter);
    }
    double x;
    if (!s.next_point(M, x)) break;
    // the single evaluation site: MinimizeforLaunchAngle (.cc:873-917)
    double thd_air, thd_ice;
    const int ph = s.phase;
    if constexpr (WAVE) {
      if (have_next) {
        thd_air = next_air;
        thd_ice = next_ice;
        have_next = false;
      } else {
        // the point the next trip evaluates when this one is f(lo) (then f(hi)) or the first guard
        // (then always the second: PH_G1 -> PH_G2)
        const bool pair = ph == PH_FLO || ph == PH_G1;
        const double xb = ph == PH_FLO ? s.hi : s.x2 + s.dlt();
        eval_thd_wave(M, I, s.q, x, pair ? xb : x, tab, thd_air, thd_ice, next_air, next_ice);
        have_next = pair;
      }
    } else {
      eval_thd(M, I, s.q, x, tab, thd_air, thd_ice);
    }
    s.template update<!WAVE>(M, x, thd_air, thd_ice);
    // f(hi) is not wanted after all when f(lo) was not finite
    if (WAVE && ph == PH_FLO && s.phase != PH_FHI) have_next = false;
  }
  return SolveResult{s.root(), s.status, s.n_eval, s.est, s.n_inside};
}

struct Solved {
  double launch, thd_air, t_air, geo_air, inc, thd_ice, t_ice, geo_ice, ant;
  double ice_n;  // Getnz_air(IceLayerHeight) after the Rx-in-air shift
  int status;
};

// Outputs at the root (GetAirPropagationPar + GetIcePropagationPar, .cc:1524-1566).
__host__ __device__ __forceinline__ Solved evaluate_root(const DevMedium& M, const IceConsts& I,
                                                const Geometry& g, double x, int status,
                                                const double* tab) {
  Solved S;
  S.status = status;
  S.launch = x;
  const AirPath P = make_air_path(M, g.H, g.ice);
  S.ice_n = P.iceair.n;
  S.thd_air = 0.0;
  S.t_air = 0.0;
  S.geo_air = 0.0;
  S.inc = __builtin_nan("");
  double L0 = __builtin_nan("");
  if (P.top < P.bot) {
    S.status |= AIRICE_SOLVE_NO_AIR_LAYER;
  } else {
    const double v2 = first_layer_v2(M, P.tx.n, P.rtop.n, x);
    L0 = P.rtop.n * v2;
    const double A2 = M.A_air * M.A_air;
    const RayL RL = ray_L(A2, L0);
    // the layer loop top -> bot as in air_thd: Tx layer, layers strictly between (uniform ends),
    // ice layer; same summation order
    auto add = [&](const Segment& sg) {
      S.thd_air += sg.thd;
      S.t_air += sg.t;
      S.geo_air += sg.geo;
    };
    add(segment(P.tx, P.rtop, M.A_air, A2, RL, true, tab));
#pragma unroll
    for (int il = kMaxLayers - 2; il >= 1; --il)
      if (il < P.top && il > P.bot) add(segment(M.start[il], M.stop[il], M.A_air, A2, RL, true, tab));
    if (P.top > P.bot) add(segment(start_endpoint(M, P.bot), P.iceair, M.A_air, A2, RL, true, tab));
    // receive angle of the last layer: asin(v2) for the first layer, asin(L0/n(Stop)) below
    S.inc = k_asin(P.top == P.bot ? v2 : L0 / P.iceair.n) * M.r2d;
  }
  S.thd_ice = 0.0;
  S.t_ice = 0.0;
  S.geo_ice = 0.0;
  S.ant = 0.0;
  if (g.depth < 0) {
    const Endpoint rx = ice_endpoint(M, g.depth_pos);
    const double A2i = M.A_ice * M.A_ice;
    const RayL RL = ray_L(A2i, L0);
    const Segment sg = segment(I.ice0, rx, M.A_ice, A2i, RL, false, tab);
    S.thd_ice = sg.thd;
    S.ant = k_asin(L0 / rx.n) * M.r2d;
    S.t_ice = sg.t;
    S.geo_ice = sg.geo;
  }
  return S;
}

// evaluate_root for one-query calls (scalar_solve_kernel; every lane holds the same query and
// root): the four air segments -- Tx layer, layers 2 and 1, the ice layer -- on lanes 0-3 at once
// (as eval_thd_wave), the segment in the ice beside them on every lane, then every lane forms the
// sums from the lanes' values in evaluate_root's order.  The same bits with about a quarter of
// its dependent chain.
__device__ __forceinline__ Solved evaluate_root_wave(const DevMedium& M, const IceConsts& I,
                                                     const Geometry& g, double x, int status,
                                                     const double* tab) {
  const int lane = (int)(threadIdx.x & 63);
  // branch-free (selects on wave-uniform conditions): one straight block, so the angle chains
  // (asin of the incidence and of the receive angle) overlap the segments
  Solved S;
  S.launch = x;
  const AirPath P = make_air_path(M, g.H, g.ice);
  S.ice_n = P.iceair.n;
  const bool air = !(P.top < P.bot);
  S.status = air ? status : (status | AIRICE_SOLVE_NO_AIR_LAYER);
  const double v2 = first_layer_v2(M, P.tx.n, P.rtop.n, x);
  const double L0 = air ? P.rtop.n * v2 : __builtin_nan("");
  const double inc = k_asin(P.top == P.bot ? v2 : L0 / P.iceair.n) * M.r2d;
  const Endpoint rx = ice_endpoint(M, g.depth_pos);
  const double ant = k_asin(L0 / rx.n) * M.r2d;
  // lanes 0-3: the air segments, with the kernel-uniform A as evaluate_root has it (the same
  // instruction forms, hence also the same NaN bits on rays without a solution)
  const double A2 = M.A_air * M.A_air;
  const RayL RL = ray_L(A2, L0);
  Endpoint T = P.tx, R = P.rtop;  // lane 0 (and the lanes past 3, whose value is unused)
  T = pick(lane == 1, M.start[2], T);
  R = pick(lane == 1, M.stop[2], R);
  T = pick(lane == 2, M.start[1], T);
  R = pick(lane == 2, M.stop[1], R);
  T = pick(lane == 3, start_endpoint(M, P.bot), T);
  R = pick(lane == 3, P.iceair, R);
  const Segment sg = segment(T, R, M.A_air, A2, RL, true, tab);
  // the segment in the ice on every lane, beside the air segments (used when g.depth < 0)
  const double A2i = M.A_ice * M.A_ice;
  const RayL RLi = ray_L(A2i, L0);
  const Segment si = segment(I.ice0, rx, M.A_ice, A2i, RLi, false, tab);
  auto from = [&](int l) { return Segment{__shfl(sg.thd, l), __shfl(sg.t, l), __shfl(sg.geo, l)}; };
  const Segment s0 = from(0), s1 = from(1), s2 = from(2), s3 = from(3);
  double thd = 0.0, t = 0.0, geo = 0.0;
  auto add = [&](bool c, const Segment& a) {
    thd = c ? thd + a.thd : thd;
    t = c ? t + a.t : t;
    geo = c ? geo + a.geo : geo;
  };
  add(air, s0);
  add(air && 2 < P.top && 2 > P.bot, s1);
  add(air && 1 < P.top && 1 > P.bot, s2);
  add(air && P.top > P.bot, s3);
  S.thd_air = thd;
  S.t_air = t;
  S.geo_air = geo;
  S.inc = air ? inc : __builtin_nan("");
  const bool in_ice = g.depth < 0;
  S.thd_ice = in_ice ? si.thd : 0.0;
  S.t_ice = in_ice ? si.t : 0.0;
  S.geo_ice = in_ice ? si.geo : 0.0;
  S.ant = in_ice ? ant : 0.0;
  return S;
}

// The root found by the one-query kernel, handed to its stage-2 body directly (WAVE) instead of
// through the parked output slots.
struct WaveRoot {
  double root;
  int status;
  Geometry g;  // the query, as load_query gave it to the root finder
};

__host__ __device__ __forceinline__ double straight_angle(const DevMedium& M, double H, double D, double ice,
                                                 double depth) {
  double thR = 0;
  if (depth < 0) thR = 180 - (atan(D / (H - ice - depth)) * M.r2d);
  if (depth >= 0) thR = 180 - (atan(D / (H - (ice + depth))) * M.r2d);
  return thR;
}

// Query sources.  IN_M: metres, uniform ice (Air2IceRayTracing batch); IN_CM: centimetres
// (GetHorizontalDistanceToIntersectionPoint, .cc:947-950); IN_TRACE: per-query ice, metres
// (TraceIceToAir).
// IN_CM100: the table lookup's minimizer fallback (.cc:1419), which hands the already-cm
// source/distance/depth over multiplied by 100 again (and the ice height, already in m, x100).
enum { IN_M = 0, IN_CM = 1, IN_TRACE = 2, IN_CM100 = 3 };

struct QueryArgs {
  const double* a;    // IN_M: txh    IN_CM(100): src_cm   IN_TRACE: depth
  const double* b;    //       dist               dist_cm            ice
  const double* c;    //       depth              depth_cm           txh
  const double* d;    //       thR (opt.)         -                  dist
  double ice;         // uniform ice height (m) or ice_cm for IN_CM(100)
  long long n;
  const uint8_t* mask;  // IN_CM100: only lanes with AIRICE_LOOKUP_FALLBACK set
};

// inl: a one-query call whose inputs arrived in the kernel arguments (Signal::in, the same values
// as Q's arrays hold), read from there instead of from host memory.
template <int IN>
__host__ __device__ __forceinline__ Geometry load_query(const DevMedium& M, const QueryArgs& Q, long long k,
                                               double& thR, const Signal* inl = nullptr) {
  const double qa = inl ? inl->in[0] : Q.a[k];
  const double qb = inl ? inl->in[1] : Q.b[k];
  const double qc = inl ? inl->in[2] : Q.c[k];
  double H, D, ice, dep;
  if (IN == IN_M) {
    H = qa;
    D = qb;
    dep = qc;
    ice = Q.ice;
    thR = Q.d != nullptr ? (inl ? inl->in[3] : Q.d[k]) : straight_angle(M, H, D, ice, dep);
  } else if (IN == IN_CM) {
    H = qa / 100;
    D = qb / 100;
    ice = Q.ice / 100;
    dep = qc / 100;
    thR = straight_angle(M, H, D, ice, dep);
  } else if (IN == IN_CM100) {
    H = (qa * 100) / 100;
    D = (qb * 100) / 100;
    ice = Q.ice / 100;
    dep = (qc * 100) / 100;
    thR = straight_angle(M, H, D, ice, dep);
  } else {
    dep = qa;
    ice = qb;
    H = qc;
    D = inl ? inl->in[3] : Q.d[k];
    thR = straight_angle(M, H, D, ice, dep);
  }
  return shift(H, D, ice, dep);
}

// A query's raw inputs as the grouping pass stores them in sorted order (group_scatter_kernel):
// {a, b, c, d} of QueryArgs at the query's index (d: IN_M's thR when given, IN_TRACE's dist).
struct QueryRec {
  double a, b, c, d;
};

// load_query<IN> on a stored record: the same arithmetic on the same values.
template <int IN>
__device__ __forceinline__ Geometry load_rec(const DevMedium& M, const QueryArgs& Q,
                                             const QueryRec& r, double& thR) {
  Signal s{};
  s.n_in = 4;
  s.in[0] = r.a;
  s.in[1] = r.b;
  s.in[2] = r.c;
  s.in[3] = r.d;
  return load_query<IN>(M, Q, 0, thR, &s);
}

// Stage 1's (root, status) of a grouped batch, in sorted order; stage 2 finds query k's record
// at inv[k].  rec == nullptr: the parked output slots (Park) hold them.
struct SortedPark {
  const double2* rec;
  const int* inv;
};

// Where stage 1 parks (root, status) for stage 2.
struct Park {
  double* root;
  double* status;
  long long stride;
  int exact;  // 1: evaluate every bisection midpoint (AIRICE_BISECT_EXACT, validation only)
  int* stats; // debug (AIRICE_SOLVE_STATS): per query {evaluations, secant search, midpoints}
};

// (the table lookup's fallback solves only its flagged lanes: lookup_kernel, not this)
constexpr bool solves_every_lane(int in) { return in != IN_CM100; }

// Stage 1's result of query k for stage 2.
__host__ __device__ __forceinline__ void parked(const SortedPark& sp, const double* root_slot,
                                       const double* status_slot, long long k, double& x, int& st) {
  if (sp.rec != nullptr) {
    const double2 p = sp.rec[sp.inv[k]];
    x = p.x;
    st = (int)p.y;
  } else {
    x = *root_slot;
    st = (int)*status_slot;
  }
}

__host__ __device__ __forceinline__ bool check_solution(double thd, double D) {
  // CheckSolution (.cc:978-983, AirIceRayTracing.cc:916-921)
  bool good = false;
  if ((fabs(thd - D) / D < 0.01 && D <= 100) || (fabs(thd - D) < 1 && D > 100)) good = true;
  if (thd < 0) good = false;
  return good;
}

// ---------------------------------------------------------------------------
// Minimizer entry points.  EntryPoint<OUT> says everything that tells one from another:
//  in            : its query source (IN_*);
//  root, status  : where stage 1 parks query k's (root, status) in the output: the Park a launcher
//                  passes (park_of) and the slots stage 2 reads back;
//  write         : the stores of stage 2 for query k and its flag byte.
// The stage-2 body, the kernels, the launchers and the host route below are written once over it.
// ---------------------------------------------------------------------------
enum { OUT_SOLVE_MR = 0, OUT_SOLVE_PY = 1, OUT_HDTIP = 2, OUT_FALLBACK = 3, OUT_TRACE = 4 };
template <int OUT>
struct EntryPoint;

// Stage-2 output stores of the solve (non-temporal stores measured no faster)
// (agent-scope stores: cfg3 solve call 0.2359-0.2370 -> 0.2352-0.2358 ms with the parked roots
// stored the same way, same outputs; the lookup's non-temporal stores stay: 101.7 against 102.4 us)
__host__ __device__ __forceinline__ void put_out(double* p, double v) { st_agent(p, v); }

// Air2IceRayTracing: dummy[0..16] (MultiRay, .cc:1597-1614) or dummy[0..14] (pythonwrapper,
// AirIceRayTracing.cc:1070-1084), SoA with stride ld; the flag byte takes the status bits.
template <int VARIANT>
struct SolveEntry {
  static constexpr int in = IN_M;
  __host__ __device__ static double* root(double* out, size_t ld, long long k) {
    return out + 10 * ld + k;
  }
  __host__ __device__ static double* status(double* out, size_t, long long k) { return out + k; }
  __host__ __device__ __forceinline__ static void write(const DevMedium& M, const IceConsts& I,
                                                        const QueryArgs&, const Geometry& g,
                                                        const Solved& S, double* __restrict__ out,
                                                        size_t ld, uint8_t* __restrict__ status,
                                                        long long k) {
    const double thd = S.thd_ice + S.thd_air;
    const double tt = S.t_ice + S.t_air;
    put_out(out + 0 * ld + k, g.H);
    put_out(out + 1 * ld + k, thd);
    put_out(out + 2 * ld + k, S.thd_air);
    put_out(out + 3 * ld + k, S.thd_ice);
    put_out(out + 4 * ld + k, tt * kSpeedC);
    put_out(out + 5 * ld + k, S.t_ice * kSpeedC);
    put_out(out + 6 * ld + k, S.t_air * kSpeedC);
    put_out(out + 7 * ld + k, tt);
    put_out(out + 8 * ld + k, S.t_ice);
    put_out(out + 9 * ld + k, S.t_air);
    put_out(out + 10 * ld + k, S.launch);
    if (VARIANT == AIRICE_VARIANT_MULTIRAY) {
      double tS, tP;
      fresnel_from_sine(S.ice_n, I.ice0.n, S.ice_n / I.ice0.n, sin_start(S.inc * M.d2r), tS, tP);
      put_out(out + 11 * ld + k, S.ant);
      put_out(out + 12 * ld + k, tS);
      put_out(out + 13 * ld + k, tP);
      put_out(out + 14 * ld + k, S.geo_air);
      put_out(out + 15 * ld + k, S.geo_ice);
      put_out(out + 16 * ld + k, S.inc);
    } else {
      put_out(out + 11 * ld + k, k_asin((S.ice_n / I.ice0.n) * sin_start(S.inc * M.d2r)) * M.r2d);
      put_out(out + 12 * ld + k, S.ant);
      put_out(out + 13 * ld + k, S.geo_air);
      put_out(out + 14 * ld + k, S.geo_ice);
    }
    if (status != nullptr) status[k] = (uint8_t)S.status;
  }
};
template <>
struct EntryPoint<OUT_SOLVE_MR> : SolveEntry<AIRICE_VARIANT_MULTIRAY> {};
template <>
struct EntryPoint<OUT_SOLVE_PY> : SolveEntry<AIRICE_VARIANT_PYWRAPPER> {};

// The park slots of the two entry points with 9 output columns (cm, rad) and a bool.
struct Out9Slots {
  __host__ __device__ static double* root(double* out9, size_t ld, long long k) {
    return out9 + 4 * ld + k;
  }
  __host__ __device__ static double* status(double* out9, size_t, long long k) { return out9 + k; }
};

// GetHorizontalDistanceToIntersectionPoint (.cc:945-989).
template <>
struct EntryPoint<OUT_HDTIP> : Out9Slots {
  static constexpr int in = IN_CM;
  __host__ __device__ __forceinline__ static void write(const DevMedium& M, const IceConsts& I,
                                                        const QueryArgs&, const Geometry& g,
                                                        const Solved& S, double* __restrict__ out,
                                                        size_t ld, uint8_t* __restrict__ ok,
                                                        long long k) {
    const double thd = S.thd_ice + S.thd_air;
    double tS, tP;
    fresnel_from_sine(S.ice_n, I.ice0.n, S.ice_n / I.ice0.n, sin_start(S.inc * M.d2r), tS, tP);
    out[0 * ld + k] = (S.t_ice * kSpeedC) * 100;
    out[1 * ld + k] = (S.t_air * kSpeedC) * 100;
    out[2 * ld + k] = S.geo_ice * 100;
    out[3 * ld + k] = S.geo_air * 100;
    out[4 * ld + k] = S.launch * M.d2r;
    out[5 * ld + k] = S.thd_air * 100;
    out[6 * ld + k] = tS;
    out[7 * ld + k] = tP;
    out[8 * ld + k] = S.ant * M.d2r;
    ok[k] = check_solution(thd, g.D) ? 1 : 0;
  }
};

// The table lookup's minimizer fallback (.cc:1417-1456): the reference passes its own output
// references to GetHorizontalDistanceToIntersectionPoint in the order (geoIce, geoAir, optIce,
// optAir, ...), so the optical and geometric slots trade places; `ok` arrives holding the
// lookup's checks and is completed with CheckSolBool and launchAngle < 0, then the four zeroed
// slots of .cc:1451-1456.  Only queries flagged AIRICE_LOOKUP_FALLBACK (Q.mask) are solved, and
// their root always reaches stage 2 in registers, so nothing is parked.
template <>
struct EntryPoint<OUT_FALLBACK> : Out9Slots {
  static constexpr int in = IN_CM100;
  __host__ __device__ __forceinline__ static void write(const DevMedium& M, const IceConsts& I,
                                                        const QueryArgs&, const Geometry& g,
                                                        const Solved& S, double* __restrict__ out,
                                                        size_t ld, uint8_t* __restrict__ ok,
                                                        long long k) {
    const double thd = S.thd_ice + S.thd_air;
    double tS, tP;
    fresnel_from_sine(S.ice_n, I.ice0.n, S.ice_n / I.ice0.n, sin_start(S.inc * M.d2r), tS, tP);
    const double launch = S.launch * M.d2r;
    const bool good = ok[k] != 0 && check_solution(thd, g.D) && !(launch < 0);
    out[0 * ld + k] = good ? S.geo_ice * 100 : 0.0;
    out[1 * ld + k] = good ? S.geo_air * 100 : 0.0;
    out[2 * ld + k] = (S.t_ice * kSpeedC) * 100;
    out[3 * ld + k] = (S.t_air * kSpeedC) * 100;
    out[4 * ld + k] = good ? launch : 0.0;
    out[5 * ld + k] = good ? S.thd_air * 100 : 0.0;
    out[6 * ld + k] = tS;
    out[7 * ld + k] = tP;
    out[8 * ld + k] = S.ant * M.d2r;
    ok[k] = good ? 1 : 0;
  }
};

// The pythonwrapper TraceIceToAir (TraceIceToAir.C:5-73): rows of 10, no flag byte, no ld.
template <>
struct EntryPoint<OUT_TRACE> {
  static constexpr int in = IN_TRACE;
  __host__ __device__ static double* root(double* out10, size_t, long long k) {
    return out10 + 10 * k + 5;
  }
  __host__ __device__ static double* status(double* out10, size_t, long long k) {
    return out10 + 10 * k + 9;
  }
  __host__ __device__ __forceinline__ static void write(const DevMedium& M, const IceConsts& I,
                                                        const QueryArgs&, const Geometry& g,
                                                        const Solved& S, double* __restrict__ out10,
                                                        size_t, uint8_t*, long long k) {
    double* o = out10 + 10 * k;
    const double thd = S.thd_ice + S.thd_air;
    const double aoi = k_asin((S.ice_n / I.ice0.n) * sin_start(S.inc * M.d2r)) * M.r2d;
    if (check_solution(thd, g.D)) {
      // swap(launch, received); received = 180 - received (TraceIceToAir.C:33-34)
      o[0] = g.H;
      o[1] = g.D;
      o[2] = S.geo_ice;
      o[3] = S.geo_air;
      o[4] = S.ant;
      o[5] = 180 - S.launch;
      o[6] = S.thd_air;
      o[7] = aoi;
      o[8] = 0;
      o[9] = 0;
    } else {
#pragma unroll
      for (int c = 0; c < 10; ++c) o[c] = -1000;
    }
  }
};

// Stage 2 of every entry point for one query k: one full evaluation at the root, then the entry
// point's stores.  Where the query and its root come from:
//  AT_PARKED : the lane reloads the query and reads the root stage 1 parked (the batch kernels);
//  AT_WAVE   : wr holds them on every lane of the one-query kernel; evaluate_root_wave spreads the
//              evaluation over the wave and lane 0 writes;
//  AT_DIRECT : wr holds them, one lane (lookup_kernel's fallback lanes, the host route).
enum { AT_PARKED = 0, AT_WAVE = 1, AT_DIRECT = 2 };
template <int OUT, int MODE>
__host__ __device__ __forceinline__ void stage2_out(const DevMedium& M, const IceConsts& I,
                                                    const QueryArgs& Q, double* __restrict__ out,
                                                    size_t ld, uint8_t* __restrict__ flag,
                                                    long long k, const double* tab,
                                                    WaveRoot wr = WaveRoot{0.0, 0},
                                                    SortedPark sp = SortedPark{nullptr, nullptr}) {
  using E = EntryPoint<OUT>;
  // (the fallback's callers have looked at the query's flag already: only flagged ones get here)
  static_assert(solves_every_lane(E::in) || MODE != AT_PARKED, "the fallback parks nothing");
  double thR;
  const Geometry g = MODE != AT_PARKED ? wr.g : load_query<E::in>(M, Q, k, thR);
  double x = wr.root;
  int st = wr.status;
  if (MODE == AT_PARKED)
    parked(sp, E::root(out, ld, k), E::status(out, ld, k), k, x, st);
  Solved S;
  if constexpr (MODE == AT_WAVE) {
    S = evaluate_root_wave(M, I, g, x, st, tab);
    if (threadIdx.x != 0) return;
  } else {
    S = evaluate_root(M, I, g, x, st, tab);
  }
  E::write(M, I, Q, g, S, out, ld, flag, k);
}

// QueryArgs::ice of the IN_CM100 source: .cc:1309 turns IceLayerHeight into metres and .cc:1419
// passes IceLayerHeight*100 to the minimizer fallback.
static inline double fallback_ice_arg(double ice_cm) { return (ice_cm / 100) * 100; }

}  // namespace airice
