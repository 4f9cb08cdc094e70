// airice_icetab.hpp -- the in-ice interpolation tables (IceRayTracing::MakeTable,
// IceRayTracing.cc:2614-2724, and GetInterpolatedValue, .cc:2727-2905): the image's layout, the
// rule that packs one position's 18 solution columns into its record, and the interpolation of
// one query.  Written once for the device (airice_icetab.hip) and the host (airice_host.cpp; the
// IceRayTracing:: drop-in, compat_iceray.cpp).
//
// Image: n_ant descriptors of 8 doubles {x_start, z_start, x_step, z_step, nx, nz, first_record,
// rx_depth}, zero-padded to a multiple of 16 doubles, then one record of 16 doubles (128 B, one
// cache line) per grid position; record r is at image + 16 r, antenna a's position (ix, iz) is
// record first_record[a] + ix*nz + iz.  A query reads the four corner records of its cell: four
// cache lines for all 13 parameters, where 13 separate columns would be 26 to 52.
//
// A grid position is start + step*i, a product and then a sum, each rounded (the library is built
// with -ffp-contract=off): the bits the reference keeps in GridPositionXb / GridPositionZb.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "airice_iceray.hpp"

namespace airice {
namespace icetab {

constexpr int kDesc = 8;      // AIRICE_ICETAB_DESC
constexpr int kRecord = 16;   // AIRICE_ICETAB_RECORD
constexpr int kParams = 13;   // AIRICE_ICETAB_PARAMS
constexpr int kSlotStatus = 13;
constexpr int kCell = 1, kIdw = 2, kBadAntenna = 4;  // AIRICE_ICETAB_CELL / _IDW / _BAD_ANTENNA
constexpr double kMissing = -1000.0;
// descriptor fields
constexpr int kXStart = 0, kZStart = 1, kXStep = 2, kZStep = 3, kNx = 4, kNz = 5, kFirst = 6,
              kRxDepth = 7;
// the solution columns the pack reads (AIRICE_ICESOL_*) and its status bits
constexpr int kSolTime = 0, kSolPath = 2, kSolLaunch = 4, kSolReceive = 6, kSolIgnore = 8,
              kSolIncidence = 10, kSolAtt = 12, kSolFocus = 16;
constexpr int kSolFocus0 = 8, kSolFocus1 = 16;

// doubles of the header of n_ant antennas
AIRICE_IR_HD inline size_t header_doubles(size_t n_ant) {
  return (n_ant * kDesc + kRecord - 1) / kRecord * kRecord;
}

AIRICE_IR_HD inline double grid_position(double start, double step, int i) {
  const double off = step * (double)i;
  return start + off;
}

// MakeTable's stores for one position (.cc:2664-2715) from the 18 columns sol(c) and the status
// byte of icesol: put(slot, value) for the 16 slots of the record.  A position the solver flagged
// non-finite has IgnoreCh 0 in both slots and packs as -1000.
template <class Sol, class Put>
AIRICE_IR_HD inline void pack_record(Sol sol, uint8_t status, Put put) {
  double focusing[2] = {1, 1};
  if (status & kSolFocus0) focusing[0] = sol(kSolFocus);
  if (status & kSolFocus1) focusing[1] = sol(kSolFocus + 1);
  if (focusing[0] != focusing[0]) focusing[0] = 1;
  if (focusing[1] != focusing[1]) focusing[1] = 1;
  if (sol(kSolIgnore) != 0) {
    put(0, sol(kSolTime));
    put(1, sol(kSolPath));
    put(2, sol(kSolLaunch));
    put(3, sol(kSolReceive));
    put(4, sol(kSolAtt));
    put(5, focusing[0]);
  } else {
    for (int c = 0; c < 6; ++c) put(c, kMissing);
  }
  if (sol(kSolIgnore + 1) != 0) {
    put(6, sol(kSolTime + 1));
    put(7, sol(kSolPath + 1));
    put(8, sol(kSolLaunch + 1));
    put(9, sol(kSolReceive + 1));
    put(10, sol(kSolAtt + 1));
    put(11, focusing[1]);
    const double inc = sol(kSolIncidence + 1);
    put(12, inc != 100 ? inc : kMissing);
  } else {
    for (int c = 6; c < 13; ++c) put(c, kMissing);
  }
  put(kSlotStatus, (double)status);
  put(14, 0.0);
  put(15, 0.0);
}

// The cell of a query (.cc:2736-2766) and what every parameter of the query shares: the four
// bilinear weights (.cc:2808-2811) and the four inverse squared distances (.cc:2774-2793).
struct Cell {
  double first;  // record of the cell's corner (bx, bz), exact
  double nz;
  double w11, w12, w21, w22;
  double q11, q12, q21, q22;
};

// desc: the antenna's 8 descriptor doubles.  False: no cell, every parameter is -1000.
AIRICE_IR_HD inline bool find_cell(const double* desc, double xT, double zT, Cell* cell) {
  const double x_start = desc[kXStart], z_start = desc[kZStart];
  const double x_step = desc[kXStep], z_step = desc[kZStep];
  const double nxd = desc[kNx], nzd = desc[kNz];
  const double x_stop = grid_position(x_start, x_step, (int)nxd - 1);
  const double z_stop = grid_position(z_start, z_step, (int)nzd - 1);
  if (!(xT >= x_start && xT <= x_stop && zT >= z_start && zT <= z_stop)) return false;
  const double x = xT, y = zT;
  const double bxd = floor((xT - x_start) / x_step);
  const double bzd = floor(fabs(zT - z_start) / z_step);
  // minXbin+1 <= TotalStepsX_O-1 && minZbin+1 <= TotalStepsZ_O-1, compared before the conversion
  // so that no value outside the grid is ever converted or used as an index
  if (!(bxd >= 0 && bzd >= 0 && bxd + 1 <= nxd - 1 && bzd + 1 <= nzd - 1)) return false;
  const int bx = (int)bxd, bz = (int)bzd;
  const double x1 = grid_position(x_start, x_step, bx), y1 = grid_position(z_start, z_step, bz);
  const double x2 = grid_position(x_start, x_step, bx + 1);
  const double y2 = grid_position(z_start, z_step, bz + 1);
  cell->first = desc[kFirst] + (bxd * nzd + bzd);
  cell->nz = nzd;
  cell->w11 = ((x2 - x) * (y2 - y)) / ((x2 - x1) * (y2 - y1));
  cell->w12 = ((x2 - x) * (y - y1)) / ((x2 - x1) * (y2 - y1));
  cell->w21 = ((x - x1) * (y2 - y)) / ((x2 - x1) * (y2 - y1));
  cell->w22 = ((x - x1) * (y - y1)) / ((x2 - x1) * (y2 - y1));
  cell->q11 = (1.0 / ((x1 - x) * (x1 - x) + (y1 - y) * (y1 - y)));
  cell->q12 = (1.0 / ((x1 - x) * (x1 - x) + (y2 - y) * (y2 - y)));
  cell->q21 = (1.0 / ((x2 - x) * (x2 - x) + (y1 - y) * (y1 - y)));
  cell->q22 = (1.0 / ((x2 - x) * (x2 - x) + (y2 - y) * (y2 - y)));
  return true;
}

// One parameter from its four corners (.cc:2769-2814); *idw is set when the inverse-distance
// branch ran.  The reference's test for four missing corners (.cc:2798) reads corners it has
// already zeroed and is never true: such a cell gives 0/0 and so -1000 by the NaN rule.
AIRICE_IR_HD inline double interpolate(const Cell& c, double f11, double f12, double f21,
                                       double f22, bool* idw) {
  if (f11 == kMissing || f12 == kMissing || f21 == kMissing || f22 == kMissing) {
    double sum1 = 0, sum2 = 0;
    if (f11 != kMissing) {
      sum1 += c.q11 * f11;
      sum2 += c.q11;
    }
    if (f12 != kMissing) {
      sum1 += c.q12 * f12;
      sum2 += c.q12;
    }
    if (f21 != kMissing) {
      sum1 += c.q21 * f21;
      sum2 += c.q21;
    }
    if (f22 != kMissing) {
      sum1 += c.q22 * f22;
      sum2 += c.q22;
    }
    double v = sum1 / sum2;
    if (v != v) v = kMissing;
    *idw = true;
    return v;
  }
  return c.w11 * f11 + c.w12 * f12 + c.w21 * f21 + c.w22 * f22;
}

// The records of a cell's corners f11, f12, f21, f22, as offsets in doubles from the image's base
AIRICE_IR_HD inline void corner_offsets(const Cell& c, size_t off[4]) {
  const size_t r = (size_t)c.first, nz = (size_t)c.nz;
  off[0] = r * kRecord;
  off[1] = (r + 1) * kRecord;
  off[2] = (r + nz) * kRecord;
  off[3] = (r + nz + 1) * kRecord;
}

// One query against a host image: all 13 parameters to put(c, value); returns the status byte.
template <class Put>
inline uint8_t lookup_one(const double* image, size_t n_ant, long long ant, double x, double z,
                          Put put) {
  Cell cell;
  const bool ant_ok = ant >= 0 && (unsigned long long)ant < n_ant;
  if (!ant_ok || !find_cell(image + (size_t)ant * kDesc, x, z, &cell)) {
    for (int c = 0; c < kParams; ++c) put(c, kMissing);
    return ant_ok ? 0 : (uint8_t)kBadAntenna;
  }
  size_t off[4];
  corner_offsets(cell, off);
  bool idw = false;
  for (int c = 0; c < kParams; ++c)
    put(c, interpolate(cell, image[off[0] + c], image[off[1] + c], image[off[2] + c],
                       image[off[3] + c], &idw));
  return (uint8_t)(kCell | (idw ? kIdw : 0));
}

// What is wrong with a descriptor's grid (a static string), or nullptr
inline const char* bad_grid(const double* desc) {
  const double nx = desc[kNx], nz = desc[kNz];
  if (!(nx >= 2 && nx <= 2147483647.0 && nx == floor(nx))) return "nx < 2 or not a count";
  if (!(nz >= 2 && nz <= 2147483647.0 && nz == floor(nz))) return "nz < 2 or not a count";
  if (!(iceray::is_finite(desc[kXStep]) && desc[kXStep] > 0))
    return "x_step is not finite and positive";
  if (!(iceray::is_finite(desc[kZStep]) && desc[kZStep] > 0))
    return "z_step is not finite and positive";
  return nullptr;
}

}  // namespace icetab
}  // namespace airice
