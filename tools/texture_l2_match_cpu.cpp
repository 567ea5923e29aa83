// Developer tool: the texture modality's L2 match (texture_modality.cpp:349-377 with cv::NORM_L2) as a plain C++ loop
// over the shared arithmetic of csrc/m3t_texture.h -- the sequential sum, the best two by the shortcut on the sums --
// with OpenMP over the queries: the reference point tools/texture_l2_timing.py prints beside the device numbers.
//   texture_l2_match_cpu <queries.f32> <train.f32> <n_query> <n_train> <floats> <reps>
// prints "<seconds per match, best of reps> <kept queries>".
#include <omp.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../3dobjecttracking_amd/csrc/m3t_texture.h"

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int nq = std::atoi(argv[3]), nt = std::atoi(argv[4]), floats = std::atoi(argv[5]), reps = std::atoi(argv[6]);
  std::vector<float> q(size_t(nq) * floats), t(size_t(nt) * floats);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(q.data(), 4, q.size(), f) != q.size()) return 3;
  std::fclose(f);
  f = std::fopen(argv[2], "rb");
  if (!f || std::fread(t.data(), 4, t.size(), f) != t.size()) return 3;
  std::fclose(f);
  std::vector<int> best(size_t(nq), -1);
  double fastest = 1e30;
  for (int rep = 0; rep < reps; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(static)
    for (int i = 0; i < nq; ++i) {
      m3t_tex_best2s b;
      m3t_tex_best2s_init(&b);
      for (int j = 0; j < nt; ++j)
        m3t_tex_best2s_update(&b, m3t_tex_l2_squared(&q[size_t(i) * floats], &t[size_t(j) * floats], floats), j);
      best[size_t(i)] = m3t_tex_ratio_keeps_l2(&b.b, 0.7f) ? b.b.i0 : -1;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (s < fastest) fastest = s;
  }
  long long kept = 0;
  for (int i = 0; i < nq; ++i) kept += best[size_t(i)] >= 0 ? 1 : 0;
  std::printf("%.9f %lld\n", fastest, kept);
  return 0;
}
