// A caller of the ice-to-air ray and of the first-arrival tracer, written the way the reference's
// user code is: include the header, call GetDirectRayPar_Air / fDa_Air / DirectRayTracer, delete[]
// what they return.  Two builds: tests/cpp/iceair_driver links libairice.so;
// tests/cpp/iceair_driver_asan compiles the drop-in and the host routes with it under ASan + UBSan
// (no GPU code, nothing preloaded) -- the delete[] of DirectRayTracer's five doubles is what that
// build checks against the reference's four-element allocation.
//
//   iceair_driver                      the head rows of tests/iceair_cases.py and a few pairs
//   iceair_driver air rows.bin         rows of three float64 (z0, x1, h) from a file
//   iceair_driver first pairs.bin      rows of six float64 (xT, yT, zT, xR, yR, zR)
//   iceair_driver --bench rows.bin T   triples per second of GetDirectRayPar_Air on T threads (JSON)
//
// Every value is printed as the 16 hex digits of its bits, so the tests compare bit for bit:
// "A <row> <5 words>" GetDirectRayPar_Air, "F <row> <1 word>" fDa_Air at the L it reported,
// "T <row> <5 words>" DirectRayTracer.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
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

static void air_row(long row, double z0, double x1, double h) {
  double* a = I::GetDirectRayPar_Air(z0, x1, h);
  words("A", row, a, 5);
  I::fDanfRa_params p = {I::A_ice, z0, x1, h};
  const double f = I::fDa_Air(a[3], &p);
  words("F", row, &f, 1);
  delete[] a;
}

static void first_row(long row, const double* q) {
  double* t = I::DirectRayTracer(q[0], q[1], q[2], q[3], q[4], q[5]);
  words("T", row, t, 5);
  delete[] t;
}

static bool read_rows(const char* path, size_t width, std::vector<double>* rows) {
  FILE* f = std::fopen(path, "rb");
  if (f == nullptr) return false;
  std::vector<double> t(width);
  while (std::fread(t.data(), sizeof(double), width, f) == width)
    rows->insert(rows->end(), t.begin(), t.end());
  std::fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc >= 4 && std::strcmp(argv[1], "--bench") == 0) {
    std::vector<double> rows;
    if (!read_rows(argv[2], 3, &rows) || rows.empty()) {
      std::fprintf(stderr, "iceair_driver: cannot read %s\n", argv[2]);
      return 2;
    }
    const int threads = std::max(1, std::atoi(argv[3]));
    const size_t n = rows.size() / 3;
    std::vector<double> sink(threads, 0.0);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
      pool.emplace_back([&, t] {
        double s = 0;
        for (size_t i = t; i < n; i += threads) {
          double* o = I::GetDirectRayPar_Air(rows[3 * i], rows[3 * i + 1], rows[3 * i + 2]);
          s += o[3];
          delete[] o;
        }
        sink[t] = s;
      });
    for (auto& th : pool) th.join();
    const double sec =
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double s = 0;
    for (double v : sink) s += v;
    std::printf("{\"triples\": %zu, \"threads\": %d, \"seconds\": %.6f, \"triples_per_s\": %.1f, "
                "\"checksum\": %.17g}\n", n, threads, sec, n / sec, s);
    return 0;
  }
  if (argc >= 3) {
    const bool air = std::strcmp(argv[1], "air") == 0;
    if (!air && std::strcmp(argv[1], "first") != 0) {
      std::fprintf(stderr, "iceair_driver: unknown mode %s\n", argv[1]);
      return 2;
    }
    const size_t width = air ? 3 : 6;
    std::vector<double> rows;
    if (!read_rows(argv[2], width, &rows)) {
      std::fprintf(stderr, "iceair_driver: cannot read %s\n", argv[2]);
      return 2;
    }
    for (size_t i = 0; i < rows.size() / width; i++) {
      const double* q = rows.data() + width * i;
      if (air) air_row((long)i, q[0], q[1], q[2]);
      else first_row((long)i, q);
    }
    return 0;
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double inf = std::numeric_limits<double>::infinity();
  // the head rows of tests/iceair_cases.py
  static const double kAir[][3] = {{-100, 10, 500},  {-10, 2500, 5},    {-1000, 300, 1},
                                   {-200, 100, 0.1}, {-200, 100, 3000}, {-200, 1, 50},
                                   {-200, 3000, 50}};
  long row = 0;
  for (const auto& r : kAir) air_row(row++, r[0], r[1], r[2]);
  for (int k = 0; k < 3; k++)
    for (double bad : {nan, inf, -inf}) {
      double q[3] = {-100, 10, 500};
      q[k] = bad;
      air_row(row++, q[0], q[1], q[2]);
    }
  // pairs: D and R, R and Ra0 (D fails), no candidate, two refracted rays, equal depths, NaN
  static const double kPairs[][6] = {
      {0, 0, -180, 60, 80, -100},           {10, -20, -180, 310, 380, -100},
      {0, 0, -200, 600, 800, -150},         {5, 5, -157.6, 342.644, 455.192, -90.13},
      {0, 0, -100, 30, 40, -100},           {0, 0, -100, 0, 0, -50}};
  row = 0;
  for (const auto& q : kPairs) first_row(row++, q);
  const double bad_pair[6] = {0, nan, -100, 30, 40, -50};
  first_row(row++, bad_pair);
  // another ice model, then back
  double A = 1.775, B = -0.5, C = 0.02;
  I::SetA(A);
  I::SetB(B);
  I::SetC(C);
  air_row(1000, -100, 10, 500);
  first_row(1000, kPairs[0]);
  A = I::A_ice_def, B = I::B_ice_def, C = I::C_ice_def;
  I::SetA(A);
  I::SetB(B);
  I::SetC(C);
  return 0;
}
