// Developer tool (tools/opt_timing.py): the reference's diameter loop, OPTEvaluator::CalculateDiameters
// (examples/opt_evaluator.cpp:580-600) -- all V^2 pairs, one maximum per OpenMP thread -- in the arithmetic of
// m3t_hip_vertices_diameter: d2 = (dx*dx + dy*dy) + dz*dz in f32 without contraction, one sqrtf of the maximum.
//   g++ -O2 -fopenmp -ffp-contract=off -o tools/bin/diameter_cpu tools/diameter_cpu.cpp
//   diameter_cpu VERTICES.f32 N      prints "<seconds> <bits of the diameter>"
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const long long n = std::atoll(argv[2]);
  std::vector<float> v(size_t(n) * 3);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) return 1;
  std::fclose(f);
  std::vector<float> x(n), y(n), z(n);
  for (long long i = 0; i < n; ++i) {
    x[i] = v[3 * i];
    y[i] = v[3 * i + 1];
    z[i] = v[3 * i + 2];
  }
  const double t0 = omp_get_wtime();
  float best = 0.0f;
#pragma omp parallel
  {
    float best_thread = 0.0f;
#pragma omp for schedule(static)
    for (long long i = 0; i < n; ++i) {
      const float xi = x[i], yi = y[i], zi = z[i];
      float b = 0.0f;
#pragma omp simd reduction(max : b)
      for (long long j = 0; j < n; ++j) {
        const float dx = xi - x[j], dy = yi - y[j], dz = zi - z[j];
        b = std::max(b, (dx * dx + dy * dy) + dz * dz);
      }
      best_thread = std::max(best_thread, b);
    }
#pragma omp critical
    best = std::max(best, best_thread);
  }
  const float diameter = std::sqrt(best);
  const double seconds = omp_get_wtime() - t0;
  uint32_t bits;
  std::memcpy(&bits, &diameter, 4);
  std::printf("%.9f %u\n", seconds, bits);
  return 0;
}
