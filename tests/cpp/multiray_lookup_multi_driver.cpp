// Caller of MultiRayAirIceRefraction::TableLookupBatchMulti, linked against libairice.so: three
// antennas, of which antenna 2 remaps to table 0 through the caller's AntennaDepths /
// AntennaTableAlreadyMade (.cc:1348-1352), looked up in one launch and compared bit for bit with
// one TableLookupBatch per antenna.  Prints one JSON object for tests/test_gpu_lookup_multi.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "MultiRayAirIceRefraction.h"

std::vector<double> AntennaDepths;
std::vector<int> AntennaTableAlreadyMade;

namespace M = MultiRayAirIceRefraction;

int main() {
  M::MakeAtmosphere();
  // coarse tables through the reference's globals, antennas 0 and 2 at one depth
  HeightStepSize = 2000;
  AngleStepSize = 5;
  LoopStartAngle = 92;
  TotalAngleSteps = (int)std::floor((LoopStopAngle - LoopStartAngle) / AngleStepSize) + 1;
  AntennaDepths = {-200 * 100., -100 * 100., -200 * 100.};
  for (size_t i = 0; i < AntennaDepths.size(); ++i) {
    bool make = true;
    for (int j : AntennaTableAlreadyMade)
      if (AntennaDepths[i] == AntennaDepths[j]) make = false;
    if (make) {
      M::MakeRayTracingTable(AntennaDepths[i], 3000 * 100., (int)AntennaTableAlreadyMade.size());
      AntennaTableAlreadyMade.push_back((int)i);
    }
  }
  const double q[][2] = {{5000e2, 1000e2},   {20000e2, 15000e2}, {3500e2, 100e2},
                         {99999e2, 30000e2}, {200000e2, 1000e2}, {8000e2, 1e9},
                         {60000e2, 42000e2}, {3000e2, 10e2},     {41000e2, 39000e2}};
  const size_t nq = sizeof(q) / sizeof(q[0]);
  const size_t na = 3;
  const int ants[na] = {0, 1, 2};
  std::vector<double> src(nq), dist(na * nq), out9(9 * na * nq);
  std::vector<char> okm(na * nq);
  for (size_t i = 0; i < nq; ++i) {
    src[i] = q[i][0];
    for (size_t a = 0; a < na; ++a) dist[a * nq + i] = q[i][1] * (1.0 + 0.125 * a);
  }
  M::TableLookupBatchMulti(src.data(), dist.data(), AntennaDepths.data(), 3000 * 100., ants, na, nq,
                           out9.data(), reinterpret_cast<bool*>(okm.data()));
  std::printf("{\"tables\": %zu,\n\"rows\": [\n", AllTableAllAntData.size());
  for (size_t a = 0; a < na; ++a) {
    const int table = a == 1 ? 1 : 0;
    std::vector<double> dep(nq, AntennaDepths[a]), ref9(9 * nq);
    std::vector<char> okb(nq);
    M::TableLookupBatch(src.data(), dist.data() + a * nq, dep.data(), 3000 * 100., table, nq,
                        ref9.data(), reinterpret_cast<bool*>(okb.data()));
    for (size_t i = 0; i < nq; ++i) {
      const bool same = okb[i] == okm[a * nq + i] &&
                        std::memcmp(&ref9[i * 9], &out9[(a * nq + i) * 9], 9 * sizeof(double)) == 0;
      std::printf("[%zu, %zu, %d, %d]%s\n", a, i, okb[i] ? 1 : 0, same ? 1 : 0,
                  (a == na - 1 && i == nq - 1) ? "" : ",");
    }
  }
  std::printf("]}\n");
  return 0;
}
