// airice_host.h -- host-only internals (airice_host.cpp): no HIP types, so the sanitizer harness
// (tests/cpp/asan_harness.cpp) builds them with a plain host compiler.
#pragma once
#include <string>

#include "airice.h"

namespace airice {

constexpr int kMaxParsedLayers = 4;  // ATMLAY has 5 bounds -> at most 4 air layers (.h:56)

// printf-style message for airice_last_error() (thread-local)
void set_error(const char* fmt, ...);
// pi of a reference namespace: MultiRayAirIceRefraction.h:29 / RayTracingFunctions.h:26
// (3.1415927) or pythonwrapper AirIceRayTracing.h:25 (4*atan(1))
double variant_pi(int variant);
// readATMpar + readnhFromFile + spline + FillInAirRefractiveIndex (.cc:24-213, 920-942) on a
// text image of a GDAS Atmosphere.dat, with the reference's stream semantics
int parse_gdas(const std::string& text, airice_medium* m);
// One (z0, x1, z1) pair of the in-ice solver on the calling thread (airice_iceray.hpp compiled
// for the host): model = {A, B, C}, out32 = the AIRICE_ICERAY_FIELDS values, status nullable.
void iceray_host_one(const double model[3], const double in[3], double* out32, uint8_t* status);
// GetRayTracingSolutions (and, with focusing, GetFocusingFactor) of one pair on the calling thread
// (airice_icesol.hpp compiled for the host): the solver's host route for the receiver -- and for
// the one 1 cm lower -- then the lane function of icesol_kernel.  out18 = the
// AIRICE_ICESOL_FIELDS values, status nullable.
void icesol_host_one(const double model[3], const double in[3], double a0, double frequency_ghz,
                     bool focusing, double* out18, uint8_t* status);
// The argument checks the icesol entries share: nullptr, or what is wrong with a0, the frequency
// or the model (a static string for airice_last_error()).
const char* icesol_bad_value(const double model[3], double a0, double frequency_ghz);
// The same pair's solutions without focusing at frequency[0], then the attenuation of its two rays
// at each of the n_freq frequencies (airice_icespec.hpp compiled for the host): att0 / att1 = slot
// 0 / 1, n_freq values each.  No frequency is refused: a bad one makes its bin NaN.
void icespec_host_one(const double model[3], const double in[3], double a0,
                      const double* frequency_ghz, size_t n_freq, double* out18, uint8_t* status,
                      double* att0, double* att1);
// The value checks the spectrum entries share: a0 and the model, as icesol_bad_value.
const char* icespec_bad_value(const double model[3], double a0);
// One (z0, x1, h) triple of the ice-to-air direct ray on the calling thread (airice_iceair.hpp
// compiled for the host): out10 = the AIRICE_ICEAIR_FIELDS values, status nullable.
void iceair_host_one(const double model[3], const double in[3], double* out10, uint8_t* status);
// The first-arriving ray of one (emitter, antenna) pair on the calling thread
// (airice_icefirst.hpp compiled for the host): in = xT, yT, zT, xR, yR, zR; out8 = the
// AIRICE_ICEFIRST_FIELDS values, status nullable.
void icefirst_host_one(const double model[3], const double in[6], double* out8, uint8_t* status);

}  // namespace airice
