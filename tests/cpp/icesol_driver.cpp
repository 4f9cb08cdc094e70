// A caller of the IceRayTracing:: drop-in's consumer-facing entries, written the way the
// reference's user code is: GetRayTracingSolutions and GetFocusingFactor per (emitter, antenna)
// pair, and the attenuation functions.  Two builds: tests/cpp/icesol_driver links libairice.so;
// tests/cpp/icesol_driver_asan compiles the drop-in and the host route with it under ASan + UBSan
// (no GPU code, nothing preloaded).
//
//   icesol_driver                    the class rows at A0 = 1, f = 0.1 GHz and a tour
//   icesol_driver rows.bin A0 f      rows of three float64 (z0, x1, z1) from a file
//
// Every value is printed as the 16 hex digits of its bits, so tests/test_icesol_cpu.py compares
// bit for bit: "S <row> <14 words>" GetRayTracingSolutions (time, path, launch, receive, IgnoreCh,
// incidence, attenuation; two each), "F <row> <4 words>" GetFocusingFactor into {0, 0} and into
// {7, 7}, "T <name> <word>" the tour.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "IceRayTracing.hh"

namespace I = IceRayTracing;

static void words(const char* tag, long row, const double* v, int n) {
  std::printf("%s %ld", tag, row);
  for (int i = 0; i < n; i++) {
    uint64_t b;
    std::memcpy(&b, v + i, 8);
    std::printf(" %016llx", (unsigned long long)b);
  }
  std::printf("\n");
}

static void tour_value(const char* name, double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  std::printf("T %s %016llx\n", name, (unsigned long long)b);
}

static void one_row(long row, double z0, double x1, double z1, double a0, double f) {
  double t[2], p[2], la[2], ra[2], inc[2], att[2];
  int ig[2];
  I::GetRayTracingSolutions(z1, x1, z0, t, p, la, ra, ig, inc, a0, f, att);
  const double v[14] = {t[0],  t[1],  p[0],          p[1],          la[0],  la[1],  ra[0],
                        ra[1], (double)ig[0], (double)ig[1], inc[0], inc[1], att[0], att[1]};
  words("S", row, v, 14);
  double fo[4] = {0, 0, 7, 7};
  I::GetFocusingFactor(z0, x1, z1, fo);
  I::GetFocusingFactor(z0, x1, z1, fo + 2);
  words("F", row, fo, 4);
}

static void tour() {
  tour_value("GetIceTemperature(-150)", I::GetIceTemperature(-150.0));
  tour_value("GetIceAttenuationLength(-150,0.3)", I::GetIceAttenuationLength(-150.0, 0.3));
  tour_value("GetIceAttenuationLength(-150,2)", I::GetIceAttenuationLength(-150.0, 2.0));
  double par[3] = {1.0, 0.3, 1.3};
  tour_value("AttenuationIntegrand(150)", I::AttenuationIntegrand(150.0, par));
  tour_value("IntegrateOverLAttn(150,150)", I::IntegrateOverLAttn(1.0, 0.3, 150.0, 150.0, 1.3));
  tour_value("IntegrateOverLAttn(150,40)", I::IntegrateOverLAttn(1.0, 0.3, 150.0, 40.0, 1.3));
  tour_value("IntegrateOverLAttn(40,150)", I::IntegrateOverLAttn(1.0, 0.3, 40.0, 150.0, 1.3));
  tour_value("Direct", I::GetTotalAttenuationDirect(1.0, 0.3, -150.0, -40.0, 1.3));
  tour_value("Reflected", I::GetTotalAttenuationReflected(1.0, 0.3, -150.0, -40.0, 1.3));
  tour_value("Refracted", I::GetTotalAttenuationRefracted(1.0, 0.3, -150.0, -140.0, 99.0, 1.7));
  tour_value("Refracted(L>=A)", I::GetTotalAttenuationRefracted(1.0, 0.3, -150.0, -140.0, 99.0, 1.8));
}

int main(int argc, char** argv) {
  if (argc >= 4) {
    FILE* f = std::fopen(argv[1], "rb");
    if (f == nullptr) {
      std::fprintf(stderr, "icesol_driver: cannot read %s\n", argv[1]);
      return 2;
    }
    const double a0 = std::atof(argv[2]), freq = std::atof(argv[3]);
    double t[3];
    long row = 0;
    while (std::fread(t, sizeof(double), 3, f) == 3) one_row(row++, t[0], t[1], t[2], a0, freq);
    std::fclose(f);
    return 0;
  }
  // the class rows of tests/iceray_cases.py, equal depths 30 cm and 0 m apart, a NaN
  static const double kRows[][3] = {
      {-180, 100, -100},       {-180, 500, -100},      {-1000, 2000, -200},
      {-200, 1000, -150},      {-157.6, 562.74, -90.13}, {-84.62, 570.19, -183.09},
      {-536.68, 994.9, -44.18}, {-100, 50, -100},       {-100, 500, -180},
      {-100, 0.3, -100},       {-100, 0, -100}};
  long row = 0;
  for (const auto& r : kRows) one_row(row++, r[0], r[1], r[2], 1.0, 0.1);
  tour();
  return 0;
}
