// compat_iceray.cpp -- the IceRayTracing:: drop-in (include/IceRayTracing.hh): the reference's
// names and signatures over the in-ice solver of airice_iceray.hpp.  Every call here runs on the
// calling thread: IceRayTracing() is the solver's host route (iceray_host_one, the function
// airice_iceray_host runs for n = 1), the *RayPar functions and the (double, void*) functions are
// the same header's pieces; GetRayTracingSolutions and GetFocusingFactor are icesol_host_one (the
// function airice_icesol_host runs for n = 1), the attenuation functions airice_icesol.hpp's.  No HIP here, so this file also builds into the sanitizer driver
// (tests/cpp/iceray_driver.cpp, `make iceray_asan`).
#include <algorithm>
#include <cmath>

#include "IceRayTracing.hh"
#include "airice_host.h"
#include "airice_iceray.hpp"
#include "airice_icesol.hpp"

namespace ir = airice::iceray;
namespace is = airice::icesol;

namespace IceRayTracing {

double A_ice = A_ice_def;
double B_ice = B_ice_def;
double C_ice = C_ice_def;

void SetA(double &A) { A_ice = A; }
void SetB(double &B) { B_ice = B; }
void SetC(double &C) { C_ice = C; }

// TransitionBoundary is 0: one B and one C at every depth (.cc:21-52)
double GetB(double) { return B_ice; }
double GetC(double) { return C_ice; }

static ir::IceModel model() { return ir::IceModel{A_ice, B_ice, C_ice}; }

double Getnz(double z) { return ir::nz(model(), z); }

// Fresnel coefficients of the E field at the surface, from the ice side (.cc:62-132):
// n1 = Getnz(0) (ice), n2 = 1 (air); total internal reflection (NaN) gives r = 1, t = 0.
namespace {
struct Fresnel {
  double n1, n2, cosi, sqterm;
};
Fresnel fresnel(double thetai) {
  Fresnel f;
  f.n1 = Getnz(0);
  f.n2 = 1;
  f.cosi = std::cos(thetai);
  f.sqterm = std::sqrt(1 - std::pow((f.n1 / f.n2) * std::sin(thetai), 2));
  return f;
}
}  // namespace

double Refl_S(double thetai) {
  const Fresnel f = fresnel(thetai);
  const double rS = (f.n1 * f.cosi - f.n2 * f.sqterm) / (f.n1 * f.cosi + f.n2 * f.sqterm);
  return std::isnan(rS) ? 1 : rS;
}
double Trans_S(double thetai) {
  const Fresnel f = fresnel(thetai);
  const double tS = 1 + (f.n1 * f.cosi - f.n2 * f.sqterm) / (f.n1 * f.cosi + f.n2 * f.sqterm);
  return std::isnan(tS) ? 0 : tS;
}
double Refl_P(double thetai) {
  const Fresnel f = fresnel(thetai);
  const double rP = -(f.n1 * f.sqterm - f.n2 * f.cosi) / (f.n1 * f.sqterm + f.n2 * f.cosi);
  return std::isnan(rP) ? 1 : rP;
}
double Trans_P(double thetai) {
  const Fresnel f = fresnel(thetai);
  const double tP =
      (1 - ((f.n1 * f.sqterm - f.n2 * f.cosi) / (f.n1 * f.sqterm + f.n2 * f.cosi))) * (f.n1 / f.n2);
  return std::isnan(tP) ? 0 : tP;
}

double GetZmax(double A, double L) { return ir::zmax_of(ir::IceModel{A, B_ice, C_ice}, L); }

// fDnfR (.cc:356-365): the ray path as a function of depth x at fixed L
double fDnfR(double x, void *params) {
  const fDnfR_params *p = static_cast<const fDnfR_params *>(params);
  return ir::fDnfR_L(ir::IceModel{p->a, p->b, p->c}, p->l, p->c, x, Getnz(x));
}
// fDnfR_L (.cc:368-379): the same as a function of L = x at fixed depth
double fDnfR_L(double x, void *params) {
  const fDnfR_L_params *p = static_cast<const fDnfR_L_params *>(params);
  return ir::fDnfR_L(ir::IceModel{p->a, p->b, p->c}, x, p->c, p->z, Getnz(p->z));
}
double ftimeD(double x, void *params) {
  const ftimeD_params *p = static_cast<const ftimeD_params *>(params);
  return ir::ftimeD(ir::IceModel{p->a, p->b, p->c}, x, p->c, Getnz(x), p->l, p->speedc);
}
double fpathD(double x, void *params) {
  const ftimeD_params *p = static_cast<const ftimeD_params *>(params);
  return ir::fpathD(ir::IceModel{p->a, p->b, p->c}, x, p->c, p->l);
}

// The residuals take the depths as given (the reference's callers flip them first)
static ir::Pair pair_of(const fDanfRa_params *p) {
  ir::Pair q;
  q.m = ir::IceModel{p->a, B_ice, C_ice};
  q.z0 = p->z0;
  q.z1 = p->z1;
  q.x1 = p->x1;
  q.n0 = ir::nz(q.m, p->z0);
  q.n1 = ir::nz(q.m, p->z1);
  q.ns = ir::nz(q.m, ir::kSurface);
  q.evals = 0;
  return q;
}
double fDa(double x, void *params) {
  ir::Pair q = pair_of(static_cast<const fDanfRa_params *>(params));
  return ir::residual(q, ir::kFDa, x);
}
double fRa(double x, void *params) {
  ir::Pair q = pair_of(static_cast<const fDanfRa_params *>(params));
  return ir::residual(q, ir::kFRa, x);
}
double fRaa(double x, void *params) {
  ir::Pair q = pair_of(static_cast<const fDanfRa_params *>(params));
  return ir::residual(q, ir::kFRaa, x);
}

double *GetDirectRayPar(double z0, double x1, double z1) {
  bool flip;
  ir::Pair p = ir::make_ray_pair(model(), z0, x1, z1, &flip);
  ir::SearchState s = {0, 0, 0, 0, 0};
  double *output = new double[6];
  ir::run_stages(p, flip, 0, 0, false, s, [output](int, const ir::RayOut &r) {
    const double v[6] = {r.rang, r.lang, r.time, r.L, r.checkzero, r.path};
    std::copy(v, v + 6, output);
  });
  return output;
}

double *GetReflectedRayPar(double z0, double x1, double z1) {
  bool flip;
  ir::Pair p = ir::make_ray_pair(model(), z0, x1, z1, &flip);
  ir::SearchState s = {0, 0, 0, 0, 0};
  double *output = new double[11];
  ir::run_stages(p, flip, 1, 1, false, s, [output](int, const ir::RayOut &r) {
    const double v[11] = {r.rang,  r.lang, r.time, r.L,     r.checkzero, r.time1,
                          r.time2, r.aux,  r.path, r.path1, r.path2};
    std::copy(v, v + 11, output);
  });
  return output;
}

double *GetRefractedRayPar(double z0, double x1, double z1, double LangR, double RangR,
                           double checkzeroD, double checkzeroR) {
  bool flip;
  ir::Pair p = ir::make_ray_pair(model(), z0, x1, z1, &flip);
  ir::SearchState s = {checkzeroD, checkzeroR, LangR, RangR, 0};
  double *output = new double[22];
  ir::run_stages(p, flip, 2, 10, false, s, [output](int ray, const ir::RayOut &r) {
    const int i = ray - 2;
    const double v[8] = {r.rang, r.lang, r.time, r.L, r.checkzero, r.time1, r.time2, r.aux};
    std::copy(v, v + 8, output + 8 * i);
    const double w[3] = {r.path, r.path1, r.path2};
    std::copy(w, w + 3, output + 16 + 3 * i);
  });
  return output;
}

double *IceRayTracing(double /*x0*/, double z0, double x1, double z1) {
  const double m[3] = {A_ice, B_ice, C_ice};
  const double in[3] = {z0, x1, z1};
  double all[AIRICE_ICERAY_FIELDS];
  airice::iceray_host_one(m, in, all, nullptr);
  double *output = new double[AIRICE_ICERAY_REFERENCE_FIELDS];
  for (int c = 0; c < AIRICE_ICERAY_REFERENCE_FIELDS; c++) output[c] = all[c];
  return output;
}

double GetIceTemperature(double z) { return is::ice_temperature(z); }
double GetIceAttenuationLength(double z, double frequency) {
  return is::attenuation_length(z, frequency);
}

// AttenuationIntegrand (.cc:166-176) as written: params = {A0, frequency, L}
double AttenuationIntegrand(double x, void *params) {
  const double *p = static_cast<const double *>(params);
  return (p[0] / GetIceAttenuationLength(x, p[1])) *
         std::sqrt(1 + std::pow(std::tan(std::asin(p[2] / Getnz(x))), 2));
}

// The integral of it between the limits given, by the solver's fixed rule (no GSL workspace)
double IntegrateOverLAttn(double A0, double Frequency, double z0, double z1, double Lvalue) {
  return is::attenuation_between(model(), is::make_medium(A0, Frequency), z0, z1, Lvalue);
}
double GetTotalAttenuationDirect(double A0, double frequency, double z0, double z1,
                                 double Lvalue) {
  return is::total_attenuation(model(), is::make_medium(A0, frequency), 1, z0, z1, Lvalue);
}
double GetTotalAttenuationReflected(double A0, double frequency, double z0, double z1,
                                    double Lvalue) {
  return is::total_attenuation(model(), is::make_medium(A0, frequency), 2, z0, z1, Lvalue);
}
// zmax is not read: each leg ends at the turning depth of Lvalue itself
double GetTotalAttenuationRefracted(double A0, double frequency, double z0, double z1,
                                    double /*zmax*/, double Lvalue) {
  return is::total_attenuation(model(), is::make_medium(A0, frequency), 3, z0, z1, Lvalue);
}

void GetRayTracingSolutions(double RxDepth, double Distance, double TxDepth, double TimeRay[2],
                            double PathRay[2], double LaunchAngle[2], double RecieveAngle[2],
                            int IgnoreCh[2], double IncidenceAngleInIce[2], double A0,
                            double frequency, double AttRay[2]) {
  const double m[3] = {A_ice, B_ice, C_ice};
  const double in[3] = {TxDepth, Distance, RxDepth};
  double o[AIRICE_ICESOL_FIELDS];
  airice::icesol_host_one(m, in, A0, frequency, false, o, nullptr);
  for (int k = 0; k < 2; k++) {
    TimeRay[k] = o[AIRICE_ICESOL_TIME + k];
    PathRay[k] = o[AIRICE_ICESOL_PATH + k];
    LaunchAngle[k] = o[AIRICE_ICESOL_LAUNCH_ANGLE + k];
    RecieveAngle[k] = o[AIRICE_ICESOL_RECEIVE_ANGLE + k];
    IgnoreCh[k] = (int)o[AIRICE_ICESOL_IGNORE + k];
    IncidenceAngleInIce[k] = o[AIRICE_ICESOL_INCIDENCE + k];
    AttRay[k] = o[AIRICE_ICESOL_ATTENUATION + k];
  }
}

// A factor whose condition is not met stays what the caller left there, as in the reference
void GetFocusingFactor(double zT, double xR, double zR, double focusing[2]) {
  const double m[3] = {A_ice, B_ice, C_ice};
  const double in[3] = {zT, xR, zR};
  double o[AIRICE_ICESOL_FIELDS];
  uint8_t st = 0;
  airice::icesol_host_one(m, in, 1, 0.1, true, o, &st);
  if (st & AIRICE_ICESOL_FOCUS0) focusing[0] = o[AIRICE_ICESOL_FOCUSING];
  if (st & AIRICE_ICESOL_FOCUS1) focusing[1] = o[AIRICE_ICESOL_FOCUSING + 1];
  if (zR == zT && focusing[0] == 0) focusing[0] = 1.;
}

}  // namespace IceRayTracing
