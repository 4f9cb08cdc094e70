// A caller of the IceRayTracing:: ray-path samplers written the way the reference's user code is:
// solve a pair with IceRayTracing(), then hand each accepted ray's L (and a refracted ray's zmax)
// to GetFullDirectRayPath / GetFullReflectedRayPath / GetFullRefractedRayPath, and all of them to
// PlotAndStoreRays.  Two builds: tests/cpp/icepath_driver links libairice.so;
// tests/cpp/icepath_driver_asan compiles the drop-in and the host route with it under ASan + UBSan
// (no GPU code, nothing preloaded).
//
//   icepath_driver                     a few fixed pairs
//   icepath_driver rows.bin            rows of three float64 (z0, x1, z1) from a file
//   icepath_driver --bench rows.bin T  samples per second of airice_icepath_one_host over the
//                                      accepted rays of the rows, on T threads (JSON)
//
// Every value is printed as the 16 hex digits of its bits, so tests/test_icepath_cpu.py compares
// bit for bit: "X <row> <ray> <words>" and "Z <row> <ray> <words>" the vectors of ray 0..3,
// "P <row>" after PlotAndStoreRays returned.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "IceRayTracing.hh"

namespace I = IceRayTracing;

static void words(const char* tag, long row, int ray, const std::vector<double>& v) {
  std::printf("%s %ld %d", tag, row, ray);
  for (double d : v) {
    uint64_t b;
    std::memcpy(&b, &d, 8);
    std::printf(" %016llx", (unsigned long long)b);
  }
  std::printf("\n");
}

// IceRayTracing's receive angle is -1000 for a ray it did not accept, NaN for a non-finite pair
static bool accepted(const double* all, int ray) {
  return all[8 + ray] != -1000.0 && std::isfinite(all[8 + ray]);
}

static void one_row(long row, double z0, double x1, double z1) {
  double* all = I::IceRayTracing(0.0, z0, x1, z1);
  // a vector the caller already holds is appended to
  std::vector<double> x(1, -1.0), z(1, -2.0);
  for (int ray = 0; ray < 4; ray++) {
    if (!accepted(all, ray)) continue;
    x.resize(1);
    z.resize(1);
    if (ray == 0) I::GetFullDirectRayPath(z0, x1, z1, all[19], x, z);
    if (ray == 1) I::GetFullReflectedRayPath(z0, x1, z1, all[20], x, z);
    if (ray >= 2) I::GetFullRefractedRayPath(z0, x1, z1, all[21 + ray], all[19 + ray], x, z, ray - 1);
    if (x[0] != -1.0 || z[0] != -2.0 || x.size() != z.size()) {
      std::fprintf(stderr, "icepath_driver: row %ld ray %d: the vectors were not appended to\n",
                   row, ray);
      std::exit(3);
    }
    words("X", row, ray, std::vector<double>(x.begin() + 1, x.end()));
    words("Z", row, ray, std::vector<double>(z.begin() + 1, z.end()));
  }
  double zmax[2] = {all[23], all[24]}, lvalues[4], checkzeroes[4];
  for (int ray = 0; ray < 4; ray++) {
    lvalues[ray] = all[19 + ray];
    checkzeroes[ray] = accepted(all, ray) ? 0.0 : -1000.0;
  }
  I::PlotAndStoreRays(0.0, z0, z1, x1, zmax, lvalues, checkzeroes);
  std::printf("P %ld\n", row);
  delete[] all;
}

static bool read_rows(const char* path, std::vector<double>* rows) {
  FILE* f = std::fopen(path, "rb");
  if (f == nullptr) return false;
  double t[3];
  while (std::fread(t, sizeof(double), 3, f) == 3) rows->insert(rows->end(), t, t + 3);
  std::fclose(f);
  return true;
}

struct Ray {
  int kind;
  double z0, x1, z1, L, zmax;
};

static int bench(const char* path, int threads) {
  std::vector<double> rows;
  if (!read_rows(path, &rows) || rows.empty()) {
    std::fprintf(stderr, "icepath_driver: cannot read %s\n", path);
    return 2;
  }
  std::vector<Ray> rays;  // solved outside the timed part
  for (size_t i = 0; i < rows.size() / 3; i++) {
    double* all = I::IceRayTracing(0.0, rows[3 * i], rows[3 * i + 1], rows[3 * i + 2]);
    for (int ray = 0; ray < 4; ray++)
      if (accepted(all, ray))
        rays.push_back(Ray{1 << ray, rows[3 * i], rows[3 * i + 1], rows[3 * i + 2], all[19 + ray],
                           ray >= 2 ? all[21 + ray] : 0.0});
    delete[] all;
  }
  const double model[3] = {I::A_ice, I::B_ice, I::C_ice};
  std::vector<long long> samples(threads, 0);
  std::vector<double> sink(threads, 0.0);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++)
    pool.emplace_back([&, t] {
      std::vector<double> x(1 << 12), z(1 << 12);
      for (size_t i = t; i < rays.size(); i += threads) {
        const Ray& r = rays[i];
        int64_t count = 0;
        int rc = airice_icepath_one_host(model, r.kind, r.z0, r.x1, r.z1, r.L, r.zmax, x.data(),
                                         z.data(), x.size(), &count);
        if (rc != AIRICE_OK && (size_t)count > x.size()) {  // a longer ray: grow and repeat
          x.resize((size_t)count);
          z.resize((size_t)count);
          rc = airice_icepath_one_host(model, r.kind, r.z0, r.x1, r.z1, r.L, r.zmax, x.data(),
                                       z.data(), x.size(), &count);
        }
        if (rc != AIRICE_OK) std::exit(4);
        samples[t] += count;
        if (count > 0) sink[t] += x[0] + z[(size_t)count - 1];
      }
    });
  for (auto& th : pool) th.join();
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  long long total = 0;
  double s = 0;
  for (int t = 0; t < threads; t++) total += samples[t], s += sink[t];
  std::printf("{\"pairs\": %zu, \"rays\": %zu, \"samples\": %lld, \"threads\": %d, "
              "\"seconds\": %.6f, \"samples_per_s\": %.1f, \"checksum\": %.17g}\n",
              rows.size() / 3, rays.size(), total, threads, sec, total / sec, s);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && std::strcmp(argv[1], "--bench") == 0)
    return bench(argv[2], std::max(1, std::atoi(argv[3])));
  if (argc >= 2) {
    std::vector<double> rows;
    if (!read_rows(argv[1], &rows)) {
      std::fprintf(stderr, "icepath_driver: cannot read %s\n", argv[1]);
      return 2;
    }
    for (size_t i = 0; i < rows.size() / 3; i++)
      one_row((long)i, rows[3 * i], rows[3 * i + 1], rows[3 * i + 2]);
    return 0;
  }
  static const double kRows[][3] = {{-180, 100, -100}, {-180, 500, -100}, {-100, 500, -180},
                                    {-157.6, 562.74, -90.13}, {-177, 60, -50}, {-50, 60, -50}};
  long row = 0;
  for (const auto& r : kRows) one_row(row++, r[0], r[1], r[2]);
  return 0;
}
