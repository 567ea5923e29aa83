// Developer tool: the texture modality's match (texture_modality.cpp:349-377) as a plain C++ loop over the shared
// arithmetic of csrc/m3t_texture.h, OpenMP over the queries: the reference point tools/texture_timing.py prints beside
// the device numbers.  texture_match_cpu <queries.u8> <train.u8> <n_query> <n_train> <bytes> <reps>
// prints "<seconds per match, best of reps> <kept queries>".
#include <omp.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../3dobjecttracking_amd/csrc/m3t_texture.h"

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int nq = std::atoi(argv[3]), nt = std::atoi(argv[4]), bytes = std::atoi(argv[5]), reps = std::atoi(argv[6]);
  const int words = bytes / 8;
  std::vector<unsigned long long> q(size_t(nq) * words), t(size_t(nt) * words);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(q.data(), 8, q.size(), f) != q.size()) return 3;
  std::fclose(f);
  f = std::fopen(argv[2], "rb");
  if (!f || std::fread(t.data(), 8, t.size(), f) != t.size()) return 3;
  std::fclose(f);
  std::vector<int> best(size_t(nq), -1);
  double fastest = 1e30;
  for (int rep = 0; rep < reps; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(static)
    for (int i = 0; i < nq; ++i) {
      m3t_tex_best2 b;
      m3t_tex_best2_init(&b);
      for (int j = 0; j < nt; ++j) {
        int d = 0;
        for (int w = 0; w < words; ++w) d += __builtin_popcountll(q[size_t(i) * words + w] ^ t[size_t(j) * words + w]);
        m3t_tex_best2_update(&b, d, j);
      }
      best[size_t(i)] = m3t_tex_ratio_keeps(&b, 0.7f) ? b.i0 : -1;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (s < fastest) fastest = s;
  }
  long long kept = 0;
  for (int i = 0; i < nq; ++i) kept += best[size_t(i)] >= 0 ? 1 : 0;
  std::printf("%.9f %lld\n", fastest, kept);
  return 0;
}
