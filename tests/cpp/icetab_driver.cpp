// A caller of the IceRayTracing:: drop-in's table workflow, written the way the reference's user
// code is: SetNumberOfAntennas, a table per antenna, GetInterpolatedValue per parameter and point.
// Two builds: tests/cpp/icetab_driver links libairice.so; tests/cpp/icetab_driver_asan compiles
// the drop-in and the host route with it under ASan + UBSan (no GPU code, nothing preloaded).
//
//   icetab_driver                 two small tables installed with SetTable and a fixed sweep of
//                                 queries; runs without a GPU
//   icetab_driver set  file.bin   tables and queries from a file of float64:
//                                 n_ant, then per antenna desc8 and 13 x nx x nz values, then
//                                 n and n x (AntNum, x, z); SetTable; runs without a GPU
//   icetab_driver make file.bin   hit, depth, n_ant, zR[n_ant], n, n x (AntNum, x, z):
//                                 MakeTable per antenna, then also the batch read
//   icetab_driver makes file.bin  the same with one MakeTables call
//
// Every value is printed as the 16 hex digits of its bits: "Q <i> <AntNum x z>" the query,
// "V <i> <13 words>" GetInterpolatedValues, "G <i> <13 words>" 13 calls of GetInterpolatedValue,
// "B <i> <13 words + status>" GetInterpolatedValuesBatch, "T <name> <word>" single cases.
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

static void single(const char* name, double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  std::printf("T %s %016llx\n", name, (unsigned long long)b);
}

struct Query {
  double ant, x, z;
};

static void scalar_reads(const std::vector<Query>& q) {
  for (size_t i = 0; i < q.size(); i++) {
    const double in[3] = {q[i].ant, q[i].x, q[i].z};
    words("Q", (long)i, in, 3);
    double v[13], g[13];
    I::GetInterpolatedValues(q[i].x, q[i].z, (int)q[i].ant, v);
    words("V", (long)i, v, 13);
    for (int c = 0; c < 13; c++) g[c] = I::GetInterpolatedValue(q[i].x, q[i].z, c, (int)q[i].ant);
    words("G", (long)i, g, 13);
  }
}

static bool read_doubles(const char* path, std::vector<double>* out) {
  FILE* f = std::fopen(path, "rb");
  if (f == nullptr) {
    std::fprintf(stderr, "icetab_driver: cannot read %s\n", path);
    return false;
  }
  double v;
  while (std::fread(&v, sizeof(double), 1, f) == 1) out->push_back(v);
  std::fclose(f);
  return true;
}

static std::vector<Query> queries_at(const std::vector<double>& d, size_t at) {
  std::vector<Query> q;
  if (at >= d.size()) return q;
  const size_t n = (size_t)d[at++];
  for (size_t i = 0; i < n && at + 3 <= d.size(); i++, at += 3) q.push_back({d[at], d[at + 1], d[at + 2]});
  return q;
}

// the value of the built-in tables: exact in double, so a test restates it
static double builtin_value(int a, int c, int ix, int iz) { return 100.0 * c + 10.0 * ix + iz + 0.5 * a; }

static int builtin() {
  I::SetNumberOfAntennas(3);  // antenna 2 gets no table
  const double grids[2][6] = {{0.0, -20.0, 0.5, 0.25, 5, 4}, {10.0, -3.5, 0.25, 0.5, 4, 6}};
  for (int a = 0; a < 2; a++) {
    const int nx = (int)grids[a][4], nz = (int)grids[a][5];
    double desc[8];
    if (airice_icetab_grid(grids[a][0], grids[a][1], grids[a][2], grids[a][3], nx, nz, -1.0 - a, desc))
      return 3;
    std::vector<double> v((size_t)13 * nx * nz);
    for (int c = 0; c < 13; c++)
      for (int ix = 0; ix < nx; ix++)
        for (int iz = 0; iz < nz; iz++) {
          double f = builtin_value(a, c, ix, iz);
          if (a == 1 && ix == 1 && iz == 2 && c < 6) f = -1000;
          if (a == 1 && ix == 2 && iz == 3 && c >= 6) f = -1000;
          v[((size_t)c * nx + ix) * nz + iz] = f;
        }
    if (I::SetTable(a, desc, v.data())) return 3;
  }
  std::vector<Query> q;
  for (int a = 0; a < 2; a++)
    for (int i = 0; i < 16; i++)
      for (int j = 0; j < 24; j++)
        q.push_back({(double)a, grids[a][0] - 0.25 + 0.1875 * i, grids[a][1] - 0.125 + 0.15625 * j});
  scalar_reads(q);
  // the documented -1000 cases
  single("rtParameter=-1", I::GetInterpolatedValue(1.0, -19.5, -1, 0));
  single("rtParameter=13", I::GetInterpolatedValue(1.0, -19.5, 13, 0));
  single("AntNum=2(no-table)", I::GetInterpolatedValue(1.0, -19.5, 0, 2));
  single("AntNum=3(beyond)", I::GetInterpolatedValue(1.0, -19.5, 0, 3));
  single("AntNum=-1", I::GetInterpolatedValue(1.0, -19.5, 0, -1));
  single("inside", I::GetInterpolatedValue(1.0, -19.5, 0, 0));
  // SetTable again replaces the table: every value of antenna 0 is now 7
  {
    double desc[8];
    if (airice_icetab_grid(0.0, -20.0, 0.5, 0.25, 5, 4, -1.0, desc)) return 3;
    std::vector<double> v((size_t)13 * 5 * 4, 7.0);
    if (I::SetTable(0, desc, v.data())) return 3;
    single("replaced", I::GetInterpolatedValue(1.0, -19.5, 0, 0));
  }
  I::SetNumberOfAntennas(0);
  single("SetNumberOfAntennas(0)", I::GetInterpolatedValue(1.0, -19.5, 0, 0));
  return 0;
}

static int from_tables(const std::vector<double>& d) {
  size_t at = 0;
  const int n_ant = (int)d[at++];
  I::SetNumberOfAntennas(n_ant);
  for (int a = 0; a < n_ant; a++) {
    const double* desc = &d[at];
    const size_t cells = (size_t)desc[4] * (size_t)desc[5];
    if (I::SetTable(a, desc, &d[at + 8])) {
      std::fprintf(stderr, "icetab_driver: SetTable: %s\n", airice_last_error());
      return 3;
    }
    at += 8 + 13 * cells;
  }
  scalar_reads(queries_at(d, at));
  return 0;
}

static int from_build(const std::vector<double>& d, bool joint) {
  const double hit = d[0], depth = d[1];
  const int n_ant = (int)d[2];
  const double* zR = &d[3];
  I::SetNumberOfAntennas(n_ant);
  if (joint) {
    if (I::MakeTables(hit, depth, zR, n_ant)) {
      std::fprintf(stderr, "icetab_driver: MakeTables: %s\n", airice_last_error());
      return 3;
    }
  } else {
    for (int a = 0; a < n_ant; a++) I::MakeTable(hit, depth, zR[a], a);
  }
  const std::vector<Query> q = queries_at(d, 3 + (size_t)n_ant);
  scalar_reads(q);
  const size_t n = q.size();
  std::vector<int> ant(n);
  std::vector<double> x(n), z(n), out(13 * n);
  std::vector<uint8_t> st(n);
  for (size_t i = 0; i < n; i++) {
    ant[i] = (int)q[i].ant;
    x[i] = q[i].x;
    z[i] = q[i].z;
  }
  if (I::GetInterpolatedValuesBatch(ant.data(), x.data(), z.data(), n, out.data(), n, st.data())) {
    std::fprintf(stderr, "icetab_driver: GetInterpolatedValuesBatch: %s\n", airice_last_error());
    return 3;
  }
  for (size_t i = 0; i < n; i++) {
    double b[14];
    for (int c = 0; c < 13; c++) b[c] = out[(size_t)c * n + i];
    b[13] = (double)st[i];
    words("B", (long)i, b, 14);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return builtin();
  if (argc != 3) {
    std::fprintf(stderr, "usage: icetab_driver [set|make|makes file.bin]\n");
    return 2;
  }
  std::vector<double> d;
  if (!read_doubles(argv[2], &d) || d.size() < 4) return 2;
  if (std::strcmp(argv[1], "set") == 0) return from_tables(d);
  if (std::strcmp(argv[1], "make") == 0) return from_build(d, false);
  if (std::strcmp(argv[1], "makes") == 0) return from_build(d, true);
  std::fprintf(stderr, "icetab_driver: unknown mode %s\n", argv[1]);
  return 2;
}
