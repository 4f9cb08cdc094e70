// Caller of MultiRayAirIceRefraction::MakeRayTracingTablesLayered (the two-layer firn extension of
// the drop-in), linked against libairice.so: the coarse grid of tests/test_gpu_firn.py through the
// reference's globals, the Summit firn, antennas at -100 m and -5 m.  Writes the first table's 11
// float columns to argv[1] and prints one JSON object; tests/test_gpu_firn.py compares the file with
// airice_table_launch_firn's bits.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "MultiRayAirIceRefraction.h"

std::vector<double> AntennaDepths;
std::vector<int> AntennaTableAlreadyMade;

namespace M = MultiRayAirIceRefraction;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  HeightStepSize = 2000;
  AngleStepSize = 0.7;
  LoopStartAngle = 90.1;
  TotalAngleSteps = (int)std::floor((LoopStopAngle - LoopStartAngle) / AngleStepSize) + 1;
  const airice_firn summit = AIRICE_FIRN_SUMMIT;
  M::A_ice = 1.775;
  const double ice_cm = 321600.0;
  M::MakeRayTracingTablesLayered({-100 * 100., -5 * 100.}, ice_cm, summit);
  // above the boundary the layered table is the one-layer one of (A, B[0], C[0])
  M::B_ice = summit.B[0];
  M::C_ice = summit.C[0];
  M::MakeRayTracingTable(-5 * 100., ice_cm, 2);
  const auto& t = AllTableAllAntData;
  int same = t.size() == 3 && t[1].size() == 11 && t[2].size() == 11;
  for (size_t c = 0; same && c < 11; ++c)
    same = t[1][c].size() == t[2][c].size() &&
           std::memcmp(t[1][c].data(), t[2][c].data(), sizeof(float) * t[1][c].size()) == 0;
  FILE* f = std::fopen(argv[1], "wb");
  if (f == nullptr) return 3;
  for (size_t c = 0; c < 11; ++c) std::fwrite(t[0][c].data(), sizeof(float), t[0][c].size(), f);
  std::fclose(f);
  std::printf("{\"tables\": %zu, \"entries\": %zu, \"angle_steps\": %d, \"height_steps\": %d, "
              "\"shallow_equals_one_layer\": %d}\n",
              t.size(), t[0][0].size(), TotalAngleSteps, TotalHeightSteps, same);
  return 0;
}
