// compat_iceray.cpp -- the IceRayTracing:: drop-in (include/IceRayTracing.hh): the reference's
// names and signatures over the in-ice solver of airice_iceray.hpp.  Every call here runs on the
// calling thread: IceRayTracing() is the solver's host route (iceray_host_one, the function
// airice_iceray_host runs for n = 1), the *RayPar functions and the (double, void*) functions are
// the same header's pieces; GetRayTracingSolutions and GetFocusingFactor are icesol_host_one (the
// function airice_icesol_host runs for n = 1), the attenuation functions airice_icesol.hpp's,
// GetAttenuationSpectrum icespec_host_one (airice_icespec.hpp); the
// GetFull*RayPath samplers and PlotAndStoreRays are airice_icepath.hpp (bit for bit
// airice_icepath_one_host); fDa_Air and GetDirectRayPar_Air are airice_iceair.hpp (iceair_host_one,
// the function airice_iceair_host runs for n = 1), DirectRayTracer icefirst_host_one.  No HIP here, so this file also builds into the sanitizer driver
// (tests/cpp/iceray_driver.cpp, `make iceray_asan`).
// The interpolation tables (SetNumberOfAntennas, MakeTable, GetInterpolatedValue and their
// extensions, at the end) keep one image per antenna in host memory and read it on the calling
// thread with airice_icetab.hpp; only the builds and the batch read go to the device, through
// entry points this file references weakly, so that the host-only sanitizer drivers link without
// them (there MakeTable, MakeTables and GetInterpolatedValuesBatch report AIRICE_EHIP).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "IceRayTracing.hh"
#include "airice_host.h"
#include "airice_iceair.hpp"
#include "airice_icepath.hpp"
#include "airice_iceray.hpp"
#include "airice_icesol.hpp"
#include "airice_icetab.hpp"

// The device entries of the tables: null in a program built without the device runtime.
extern "C" {
int airice_icetab_build_host(const double *, double *, const double *, size_t, double, double)
    __attribute__((weak));
int airice_icetab_lookup_launch(const double *, size_t, const int32_t *, const double *,
                                const double *, size_t, double *, size_t, uint8_t *, void *)
    __attribute__((weak));
int airice_malloc(void **, size_t) __attribute__((weak));
int airice_free(void *) __attribute__((weak));
int airice_memcpy_h2d(void *, const void *, size_t) __attribute__((weak));
int airice_memcpy_d2h(void *, const void *, size_t) __attribute__((weak));
}

namespace ir = airice::iceray;
namespace ia = airice::iceair;
namespace is = airice::icesol;
namespace it = airice::icetab;
namespace ip = airice::icepath;

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

// fDa_Air (.cc:2358-2408): z1 is the receiver's height above the surface
double fDa_Air(double x, void *params) {
  const fDanfRa_params *p = static_cast<const fDanfRa_params *>(params);
  ia::Triple t = ia::make_triple(ir::IceModel{p->a, B_ice, C_ice}, p->z0, p->x1, p->z1);
  return ia::residual(t, x);
}

// GetDirectRayPar_Air (.cc:2411-2500): columns 0-4 of the ice-to-air solve's host route
double *GetDirectRayPar_Air(double z0, double x1, double z1) {
  const double m[3] = {A_ice, B_ice, C_ice};
  const double in[3] = {z0, x1, z1};
  double all[AIRICE_ICEAIR_FIELDS];
  airice::iceair_host_one(m, in, all, nullptr);
  double *output = new double[5];
  std::copy(all, all + 5, output);
  return output;
}

// DirectRayTracer (.cc:2502-2612): columns 0-4 of the first arrival's host route.  Five values:
// the reference allocates four and writes five.
double *DirectRayTracer(double xT, double yT, double zT, double xR, double yR, double zR) {
  const double m[3] = {A_ice, B_ice, C_ice};
  const double in[6] = {xT, yT, zT, xR, yR, zR};
  double all[AIRICE_ICEFIRST_FIELDS];
  airice::icefirst_host_one(m, in, all, nullptr);
  double *output = new double[5];
  std::copy(all, all + 5, output);
  return output;
}

// GetFull*RayPath (.cc:1257-1712): the samples of airice_icepath.hpp appended to the caller's
// vectors (the reference's `using namespace std` vector).
static void append_path(int kind, double z0, double x1, double z1, double L, double zmax,
                        std::vector<double> &x, std::vector<double> &z) {
  const ir::IceModel m = model();
  const ip::Segment s = ip::make_segment(m, kind, z0, x1, z1, L, zmax);
  const size_t at = x.size(), zat = z.size();
  x.resize(at + (size_t)s.count);
  z.resize(zat + (size_t)s.count);
  for (long long k = 0; k < s.count; k++) ip::sample(m, s, k, x[at + (size_t)k], z[zat + (size_t)k]);
}
void GetFullDirectRayPath(double z0, double x1, double z1, double lvalueD, std::vector<double> &x,
                          std::vector<double> &z) {
  append_path(0, z0, x1, z1, lvalueD, 0.0, x, z);
}
void GetFullReflectedRayPath(double z0, double x1, double z1, double lvalueR,
                             std::vector<double> &x, std::vector<double> &z) {
  append_path(1, z0, x1, z1, lvalueR, 0.0, x, z);
}
// raynumber named the reference's (commented-out) text file; both refracted rays sample alike
void GetFullRefractedRayPath(double z0, double x1, double z1, double zmax, double lvalueRa,
                             std::vector<double> &x, std::vector<double> &z, int raynumber) {
  append_path(raynumber == 2 ? 3 : 2, z0, x1, z1, lvalueRa, zmax, x, z);
}
// .cc:1715-1743: the three under its conditions; the vectors are locals there too
void PlotAndStoreRays(double /*x0*/, double z0, double z1, double x1, double zmax[2],
                      double lvalues[4], double checkzeroes[4]) {
  std::vector<double> xD, zD, xR, zR, xRa[2], zRa[2];
  GetFullDirectRayPath(z0, x1, z1, lvalues[0], xD, zD);
  GetFullReflectedRayPath(z0, x1, z1, lvalues[1], xR, zR);
  if ((std::fabs(checkzeroes[1]) > 0.5 || std::fabs(checkzeroes[0]) > 0.5) &&
      std::fabs(checkzeroes[2]) < 0.5) {
    GetFullRefractedRayPath(z0, x1, z1, zmax[0], lvalues[2], xRa[0], zRa[0], 1);
    if (std::fabs(checkzeroes[3]) < 0.5)
      GetFullRefractedRayPath(z0, x1, z1, zmax[1], lvalues[3], xRa[1], zRa[1], 2);
  }
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

// Extension: AttRay of the same two rays at n_freq frequencies, on the calling thread -- the
// function airice_icesol_spectrum_host runs for n = 1 (airice_icespec.hpp)
int GetAttenuationSpectrum(double RxDepth, double Distance, double TxDepth, double A0,
                           const double *frequency, size_t n_freq, double *AttRay0,
                           double *AttRay1) {
  const double m[3] = {A_ice, B_ice, C_ice};
  const char *bad = frequency == nullptr || AttRay0 == nullptr || AttRay1 == nullptr
                        ? "null argument"
                        : n_freq == 0 ? "n_freq is 0" : airice::icespec_bad_value(m, A0);
  if (bad != nullptr) {
    airice::set_error("GetAttenuationSpectrum: %s", bad);
    return AIRICE_EINVAL;
  }
  const double in[3] = {TxDepth, Distance, RxDepth};
  double o[AIRICE_ICESOL_FIELDS];
  airice::icespec_host_one(m, in, A0, frequency, n_freq, o, nullptr, AttRay0, AttRay1);
  return AIRICE_OK;
}

// ---- interpolation tables (.cc:2614-2905, 3212-3216) -------------------------------------------
// One image per antenna (n_ant = 1: a 16-double header, then the records), so MakeTable for one
// antenna touches no other.  Like the reference's namespace statics this state is not reentrant.
namespace {

struct FreeDeleter {
  void operator()(double *p) const { std::free(p); }
};
using ImagePtr = std::unique_ptr<double, FreeDeleter>;

ImagePtr alloc_image(size_t doubles) {
  const size_t bytes = (sizeof(double) * doubles + AIRICE_ICETAB_ALIGN - 1) / AIRICE_ICETAB_ALIGN *
                       AIRICE_ICETAB_ALIGN;
  return ImagePtr(static_cast<double *>(std::aligned_alloc(AIRICE_ICETAB_ALIGN, bytes)));
}

struct AntennaTable {
  ImagePtr image;
  size_t doubles = 0;
};
std::vector<AntennaTable> g_tables;

// The device copy GetInterpolatedValuesBatch reads: the antennas that have a table, joined into
// one image; slot[AntNum] is the antenna's index there (-1: no table).
struct DeviceTables {
  void *image = nullptr;
  size_t n_ant = 0;
  std::vector<int32_t> slot;
  void drop() {
    if (image != nullptr && airice_free != nullptr) (void)airice_free(image);
    image = nullptr;
    n_ant = 0;
    slot.clear();
  }
  ~DeviceTables() { drop(); }
} g_device;

const double *table_of(int AntNum) {
  if (AntNum < 0 || (size_t)AntNum >= g_tables.size()) return nullptr;
  return g_tables[(size_t)AntNum].image.get();
}

// A fresh image for AntNum with the descriptor laid out for one antenna; nullptr on failure.
double *new_table(int AntNum, const double desc8[8]) {
  if (AntNum < 0) {
    airice::set_error("IceRayTracing tables: AntNum = %d", AntNum);
    return nullptr;
  }
  double d[it::kDesc];
  std::copy(desc8, desc8 + it::kDesc, d);
  size_t doubles = 0;
  if (airice_icetab_layout(d, 1, &doubles) != AIRICE_OK) return nullptr;
  ImagePtr image = alloc_image(doubles);
  if (!image) {
    airice::set_error("IceRayTracing tables: out of memory (%zu doubles)", doubles);
    return nullptr;
  }
  std::fill(image.get(), image.get() + it::header_doubles(1), 0.0);
  std::copy(d, d + it::kDesc, image.get());
  if ((size_t)AntNum >= g_tables.size()) g_tables.resize((size_t)AntNum + 1);
  g_device.drop();
  g_tables[(size_t)AntNum].image = std::move(image);
  g_tables[(size_t)AntNum].doubles = doubles;
  return g_tables[(size_t)AntNum].image.get();
}

void drop_table(int AntNum) {
  if (AntNum >= 0 && (size_t)AntNum < g_tables.size()) g_tables[(size_t)AntNum] = AntennaTable();
  g_device.drop();
}

int no_device(const char *who) {
  airice::set_error("IceRayTracing::%s: this program was built without the device runtime", who);
  return AIRICE_EHIP;
}

}  // namespace

void SetNumberOfAntennas(int numberOfAntennas) {
  g_tables.resize(numberOfAntennas > 0 ? (size_t)numberOfAntennas : 0);
  g_device.drop();
}

int MakeTables(double ShowerHitDistance, double ShowerDepth, const double *zR, int n_ant) {
  if (zR == nullptr || n_ant <= 0) {
    airice::set_error("IceRayTracing::MakeTables: null zR or n_ant = %d", n_ant);
    return AIRICE_EINVAL;
  }
  if (airice_icetab_build_host == nullptr) return no_device("MakeTables");
  const double m[3] = {A_ice, B_ice, C_ice};
  for (int a0 = 0; a0 < n_ant; a0 += AIRICE_ICETAB_MAX_BUILD) {  // one build per 32 antennas
    const int na = std::min(n_ant - a0, (int)AIRICE_ICETAB_MAX_BUILD);
    std::vector<double> descs((size_t)na * it::kDesc);
    for (int a = 0; a < na; a++)
      if (int rc = airice_icetab_grid_init(ShowerHitDistance, ShowerDepth, zR[a0 + a],
                                           descs.data() + (size_t)a * it::kDesc))
        return rc;
    size_t doubles = 0;
    if (int rc = airice_icetab_layout(descs.data(), (size_t)na, &doubles)) return rc;
    ImagePtr joint = alloc_image(doubles);
    if (!joint) {
      airice::set_error("IceRayTracing::MakeTables: out of memory (%zu doubles)", doubles);
      return AIRICE_ENOMEM;
    }
    // A0 = 1, frequency = 0.1 GHz (.cc:2652-2653)
    if (int rc = airice_icetab_build_host(m, joint.get(), descs.data(), (size_t)na, 1, 0.1))
      return rc;
    for (int a = 0; a < na; a++) {
      const double *d = descs.data() + (size_t)a * it::kDesc;
      double *image = new_table(a0 + a, d);
      if (image == nullptr) return AIRICE_ENOMEM;
      const size_t records = (size_t)d[it::kNx] * (size_t)d[it::kNz];
      std::copy(joint.get() + (size_t)d[it::kFirst] * it::kRecord,
                joint.get() + ((size_t)d[it::kFirst] + records) * it::kRecord,
                image + it::header_doubles(1));
    }
  }
  return AIRICE_OK;
}

// Replaces AntNum's table; prints no "The table took ... ms to make" (IceRayTracing.hh)
void MakeTable(double ShowerHitDistance, double ShowerDepth, double zR, int AntNum) {
  int rc = AIRICE_OK;
  double desc[it::kDesc];
  double *image = nullptr;
  if (airice_icetab_build_host == nullptr) rc = no_device("MakeTable");
  if (rc == AIRICE_OK) rc = airice_icetab_grid_init(ShowerHitDistance, ShowerDepth, zR, desc);
  if (rc == AIRICE_OK && (image = new_table(AntNum, desc)) == nullptr) rc = AIRICE_EINVAL;
  if (rc == AIRICE_OK) {
    const double m[3] = {A_ice, B_ice, C_ice};
    rc = airice_icetab_build_host(m, image, image, 1, 1, 0.1);
    if (rc != AIRICE_OK) drop_table(AntNum);
  }
  if (rc != AIRICE_OK)
    std::fprintf(stderr, "IceRayTracing::MakeTable: %s\n", airice_last_error());
}

int SetTable(int AntNum, const double desc8[8], const double *values13) {
  if (desc8 == nullptr || values13 == nullptr) {
    airice::set_error("IceRayTracing::SetTable: null argument");
    return AIRICE_EINVAL;
  }
  double *image = new_table(AntNum, desc8);
  if (image == nullptr) return AIRICE_EINVAL;
  const size_t records = (size_t)image[it::kNx] * (size_t)image[it::kNz];
  double *rec = image + it::header_doubles(1);
  for (size_t r = 0; r < records; r++, rec += it::kRecord) {
    for (int c = 0; c < it::kParams; c++) rec[c] = values13[(size_t)c * records + r];
    for (int c = it::kParams; c < it::kRecord; c++) rec[c] = 0.0;
  }
  return AIRICE_OK;
}

double GetInterpolatedValue(double xT, double zT, int rtParameter, int AntNum) {
  const double *image = table_of(AntNum);
  if (image == nullptr || rtParameter < 0 || rtParameter >= it::kParams) return it::kMissing;
  it::Cell cell;
  if (!it::find_cell(image, xT, zT, &cell)) return it::kMissing;
  size_t off[4];
  it::corner_offsets(cell, off);
  bool idw = false;
  return it::interpolate(cell, image[off[0] + rtParameter], image[off[1] + rtParameter],
                         image[off[2] + rtParameter], image[off[3] + rtParameter], &idw);
}

void GetInterpolatedValues(double xT, double zT, int AntNum, double out[13]) {
  const double *image = table_of(AntNum);
  if (image == nullptr) {
    std::fill(out, out + it::kParams, it::kMissing);
    return;
  }
  it::lookup_one(image, 1, 0, xT, zT, [out](int c, double v) { out[c] = v; });
}

int GetInterpolatedValuesBatch(const int *AntNum, const double *xT, const double *zT, size_t n,
                               double *out, size_t ld, uint8_t *status) {
  if (n == 0) return AIRICE_OK;
  if (xT == nullptr || zT == nullptr || out == nullptr || ld < n) {
    airice::set_error("IceRayTracing::GetInterpolatedValuesBatch: null argument or ld < n");
    return AIRICE_EINVAL;
  }
  if (airice_icetab_lookup_launch == nullptr || airice_malloc == nullptr)
    return no_device("GetInterpolatedValuesBatch");
  if (g_device.image == nullptr) {  // join the antennas that have a table and upload them
    std::vector<double> descs;
    std::vector<int32_t> slot(g_tables.size(), -1);
    for (size_t a = 0; a < g_tables.size(); a++)
      if (g_tables[a].image) {
        slot[a] = (int32_t)(descs.size() / it::kDesc);
        descs.insert(descs.end(), g_tables[a].image.get(), g_tables[a].image.get() + it::kDesc);
      }
    const size_t n_ant = descs.size() / it::kDesc;
    if (n_ant == 0) {
      airice::set_error("IceRayTracing::GetInterpolatedValuesBatch: no antenna has a table");
      return AIRICE_EINVAL;
    }
    size_t doubles = 0;
    if (int rc = airice_icetab_layout(descs.data(), n_ant, &doubles)) return rc;
    std::vector<double> joint(doubles, 0.0);
    std::copy(descs.begin(), descs.end(), joint.begin());
    for (size_t a = 0; a < g_tables.size(); a++)
      if (slot[a] >= 0) {
        const double *d = descs.data() + (size_t)slot[a] * it::kDesc;
        std::copy(g_tables[a].image.get() + it::header_doubles(1),
                  g_tables[a].image.get() + g_tables[a].doubles,
                  joint.begin() + (size_t)d[it::kFirst] * it::kRecord);
      }
    void *dev = nullptr;
    if (int rc = airice_malloc(&dev, sizeof(double) * doubles)) return rc;
    if (int rc = airice_memcpy_h2d(dev, joint.data(), sizeof(double) * doubles)) {
      (void)airice_free(dev);
      return rc;
    }
    g_device.image = dev;
    g_device.n_ant = n_ant;
    g_device.slot = slot;
  }
  // queries: ant (4 n, padded) | x | z | out (13 n) | status
  std::vector<int32_t> ant(n);
  for (size_t i = 0; i < n; i++) {
    const int a = AntNum != nullptr ? AntNum[i] : 0;
    const bool known = a >= 0 && (size_t)a < g_device.slot.size() && g_device.slot[(size_t)a] >= 0;
    ant[i] = known ? g_device.slot[(size_t)a] : (int32_t)g_device.n_ant;  // -> BAD_ANTENNA, -1000
  }
  const size_t ant_bytes = (sizeof(int32_t) * n + 15) / 16 * 16;
  const size_t bytes = ant_bytes + sizeof(double) * (2 + it::kParams) * n + n;
  void *block = nullptr;
  if (int rc = airice_malloc(&block, bytes)) return rc;
  char *base = static_cast<char *>(block);
  double *dx = reinterpret_cast<double *>(base + ant_bytes);
  double *dz = dx + n, *dout = dz + n;
  uint8_t *dst = reinterpret_cast<uint8_t *>(dout + (size_t)it::kParams * n);
  int rc = airice_memcpy_h2d(base, ant.data(), sizeof(int32_t) * n);
  if (rc == AIRICE_OK) rc = airice_memcpy_h2d(dx, xT, sizeof(double) * n);
  if (rc == AIRICE_OK) rc = airice_memcpy_h2d(dz, zT, sizeof(double) * n);
  if (rc == AIRICE_OK)
    rc = airice_icetab_lookup_launch(static_cast<const double *>(g_device.image), g_device.n_ant,
                                     reinterpret_cast<const int32_t *>(base), dx, dz, n, dout, n,
                                     dst, nullptr);
  // the copies back are on the null stream, like the launch: they wait for the kernel
  for (int c = 0; c < it::kParams && rc == AIRICE_OK; c++)
    rc = airice_memcpy_d2h(out + (size_t)c * ld, dout + (size_t)c * n, sizeof(double) * n);
  if (rc == AIRICE_OK && status != nullptr) rc = airice_memcpy_d2h(status, dst, n);
  (void)airice_free(block);
  return rc;
}

}  // namespace IceRayTracing
