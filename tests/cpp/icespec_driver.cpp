// A caller of the attenuation spectrum, written the way a time-domain consumer is: for each
// (emitter, antenna) pair the two rays' AttRay over a list of frequencies in one call.  Two builds:
// tests/cpp/icespec_driver links libairice.so and also calls the C-ABI's host entry (n = 1, which
// runs on the calling thread by default); tests/cpp/icespec_driver_asan compiles the drop-in and
// the host route with it under ASan + UBSan (no GPU code, no device runtime -- the C-ABI entry is
// not linked there and its lines are left out -- and nothing preloaded).
//
//   icespec_driver                   the class rows of tests/iceray_cases.py at A0 = 1 over the
//                                    eight frequencies that straddle the 1 GHz branch
//
// Every value is printed as the 16 hex digits of its bits, so tests/test_icespec_cpu.py compares
// bit for bit: "G <row> <slot> <8 words>" GetAttenuationSpectrum, "H <row> <slot> <8 words>"
// airice_icesol_spectrum_host, "E <code>" the drop-in's answer to n_freq = 0.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "IceRayTracing.hh"

extern "C" int airice_icesol_spectrum_host(const double *, const double *, const double *,
                                           const double *, size_t, double, const double *, size_t,
                                           double *, size_t, uint8_t *, double *, size_t)
    __attribute__((weak));

namespace I = IceRayTracing;

static void words(const char *tag, long row, int slot, const double *v, int n) {
  std::printf("%s %ld %d", tag, row, slot);
  for (int i = 0; i < n; i++) {
    uint64_t b;
    std::memcpy(&b, v + i, 8);
    std::printf(" %016llx", (unsigned long long)b);
  }
  std::printf("\n");
}

int main() {
  static const double kRows[][3] = {
      {-180, 100, -100},        {-180, 500, -100},        {-1000, 2000, -200},
      {-200, 1000, -150},       {-157.6, 562.74, -90.13}, {-84.62, 570.19, -183.09},
      {-536.68, 994.9, -44.18}, {-100, 50, -100},         {-100, 500, -180}};
  static const double kFreq[8] = {0.05, 0.1, 0.5, 0.999999, 1.0, 2.0, 3.16, 5.0};
  long row = 0;
  for (const auto &r : kRows) {
    double a[2][8];
    if (I::GetAttenuationSpectrum(r[2], r[1], r[0], 1.0, kFreq, 8, a[0], a[1]) != AIRICE_OK) {
      std::fprintf(stderr, "icespec_driver: GetAttenuationSpectrum: %s\n", airice_last_error());
      return 2;
    }
    words("G", row, 0, a[0], 8);
    words("G", row, 1, a[1], 8);
    if (airice_icesol_spectrum_host != nullptr) {
      double sol[AIRICE_ICESOL_FIELDS], att[2 * 8];
      uint8_t st = 0;
      const double model[3] = {I::A_ice, I::B_ice, I::C_ice};
      if (airice_icesol_spectrum_host(model, &r[0], &r[1], &r[2], 1, 1.0, kFreq, 8, sol, 1, &st,
                                      att, 8) != AIRICE_OK) {
        std::fprintf(stderr, "icespec_driver: airice_icesol_spectrum_host: %s\n",
                     airice_last_error());
        return 3;
      }
      words("H", row, 0, att, 8);
      words("H", row, 1, att + 8, 8);
    }
    row++;
  }
  double none[1];
  std::printf("E %d\n", I::GetAttenuationSpectrum(-100, 100, -180, 1.0, kFreq, 0, none, none));
  return 0;
}
