// An IceRayTracing:: caller written the way the reference's user code is: include the header, call
// IceRayTracing(x0, z0, x1, z1) and the *RayPar functions, delete[] what they return.  Two builds:
// tests/cpp/iceray_driver links libairice.so; tests/cpp/iceray_driver_asan compiles the drop-in and
// the host route with it under ASan + UBSan (no GPU code, nothing preloaded).
//
//   iceray_driver                     the class rows and a tour of the scalar functions
//   iceray_driver rows.bin            rows of three float64 (z0, x1, z1) from a file
//   iceray_driver --bench rows.bin T  pairs per second of IceRayTracing() on T threads (JSON)
//
// Every value is printed as the 16 hex digits of its bits, so tests/test_iceray_cpu.py compares
// bit for bit: "I <row> <29 words>" IceRayTracing, "D" / "R" / "A" the three *RayPar functions
// (6 / 11 / 22 words), "T <name> <words>" the tour.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

static void tour_value(const char* name, double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  std::printf("T %s %016llx\n", name, (unsigned long long)b);
}

static void one_row(long row, double z0, double x1, double z1) {
  double* all = I::IceRayTracing(0.0, z0, x1, z1);
  words("I", row, all, 29);
  delete[] all;
  double* d = I::GetDirectRayPar(z0, x1, z1);
  words("D", row, d, 6);
  double* r = I::GetReflectedRayPar(z0, x1, z1);
  words("R", row, r, 11);
  if (std::fabs(r[4]) > 0.5 || std::fabs(d[4]) > 0.5) {  // as IceRayTracing calls it
    double* a = I::GetRefractedRayPar(z0, x1, z1, r[1], r[0], d[4], r[4]);
    words("A", row, a, 22);
    delete[] a;
  }
  delete[] d;
  delete[] r;
}

static bool read_rows(const char* path, std::vector<double>* rows) {
  FILE* f = std::fopen(path, "rb");
  if (f == nullptr) return false;
  double t[3];
  while (std::fread(t, sizeof(double), 3, f) == 3) rows->insert(rows->end(), t, t + 3);
  std::fclose(f);
  return true;
}

static void tour() {
  tour_value("Getnz(-100)", I::Getnz(-100.0));
  tour_value("GetB(-100)", I::GetB(-100.0));
  tour_value("GetC(-100)", I::GetC(-100.0));
  tour_value("Refl_S(0.3)", I::Refl_S(0.3));
  tour_value("Trans_S(0.3)", I::Trans_S(0.3));
  tour_value("Refl_P(0.3)", I::Refl_P(0.3));
  tour_value("Trans_P(0.3)", I::Trans_P(0.3));
  tour_value("Refl_S(1.2)", I::Refl_S(1.2));  // past the critical angle: r = 1, t = 0
  tour_value("Trans_P(1.2)", I::Trans_P(1.2));
  tour_value("GetZmax(A,1.6)", I::GetZmax(I::A_ice, 1.6));
  tour_value("GetZmax(A,1.9)", I::GetZmax(I::A_ice, 1.9));
  tour_value("GetZmax(A,1.2)", I::GetZmax(I::A_ice, 1.2));
  I::fDanfRa_params q = {I::A_ice, -180.0, 100.0, -100.0};
  tour_value("fDa(1.3)", I::fDa(1.3, &q));
  tour_value("fRa(0.5)", I::fRa(0.5, &q));
  tour_value("fRaa(1.6)", I::fRaa(1.6, &q));
  tour_value("fRaa(1.9)", I::fRaa(1.9, &q));
  I::fDnfR_params a = {I::A_ice, I::GetB(-100.0), -I::GetC(-100.0), 1.3};
  tour_value("fDnfR(100)", I::fDnfR(100.0, &a));
  I::fDnfR_L_params b = {I::A_ice, I::GetB(-100.0), -I::GetC(-100.0), 100.0};
  tour_value("fDnfR_L(1.3)", I::fDnfR_L(1.3, &b));
  I::ftimeD_params c = {I::A_ice, I::GetB(-100.0), -I::GetC(-100.0), I::c_light_ms, 1.3};
  tour_value("ftimeD(100)", I::ftimeD(100.0, &c));
  tour_value("fpathD(100)", I::fpathD(100.0, &c));
  // another ice model, then back
  double A = 1.775, B = -0.45, C = 0.014;
  I::SetA(A);
  I::SetB(B);
  I::SetC(C);
  tour_value("Getnz(-100)'", I::Getnz(-100.0));
  one_row(1000, -180.0, 100.0, -100.0);
  A = I::A_ice_def, B = I::B_ice_def, C = I::C_ice_def;
  I::SetA(A);
  I::SetB(B);
  I::SetC(C);
}

int main(int argc, char** argv) {
  if (argc >= 4 && std::strcmp(argv[1], "--bench") == 0) {
    std::vector<double> rows;
    if (!read_rows(argv[2], &rows) || rows.empty()) {
      std::fprintf(stderr, "iceray_driver: cannot read %s\n", argv[2]);
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
          double* o = I::IceRayTracing(0.0, rows[3 * i], rows[3 * i + 1], rows[3 * i + 2]);
          s += o[19];
          delete[] o;
        }
        sink[t] = s;
      });
    for (auto& th : pool) th.join();
    const double sec =
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double s = 0;
    for (double v : sink) s += v;
    std::printf("{\"pairs\": %zu, \"threads\": %d, \"seconds\": %.6f, \"pairs_per_s\": %.1f, "
                "\"checksum\": %.17g}\n", n, threads, sec, n / sec, s);
    return 0;
  }
  if (argc >= 2) {
    std::vector<double> rows;
    if (!read_rows(argv[1], &rows)) {
      std::fprintf(stderr, "iceray_driver: cannot read %s\n", argv[1]);
      return 2;
    }
    for (size_t i = 0; i < rows.size() / 3; i++)
      one_row((long)i, rows[3 * i], rows[3 * i + 1], rows[3 * i + 2]);
    return 0;
  }
  // the class rows of tests/iceray_cases.py
  static const double kRows[][3] = {
      {-180, 100, -100}, {-180, 500, -100}, {-1000, 2000, -200}, {-200, 1000, -150},
      {-50, 300, -20},   {-100, 50, -100},  {-100, 500, -180}};
  long row = 0;
  for (const auto& r : kRows) one_row(row++, r[0], r[1], r[2]);
  tour();
  return 0;
}
