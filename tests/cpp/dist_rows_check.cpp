// Host check of the row pass's item mapping (3dobjecttracking_amd/csrc/m3t_dist_rows.h; region_distribution_rows in
// m3t_kernels.hip runs its loop with these functions): for every part of every split of nl lines, every
// (line, d) of the part's own lines [line_lo, min(line_hi, nl)) -- padded lines below nl included -- is taken exactly
// once, a line's lanes sit in one aligned 16-lane row of one wave with lane d on value d, no lane takes an item outside
// the part, and all lanes of a wave make the same number of trips (the row chains need uniform control flow).
//   dist_rows_check     prints "cases N items M errors E"
#include <cstdio>
#include <vector>

#include "../../3dobjecttracking_amd/csrc/m3t_dist_rows.h"

int main() {
  long cases = 0, items = 0, errors = 0;
  const int parts_list[] = {2, 4, 8, 16}, threads_list[] = {256, 512};
  for (int nl = 1; nl <= 256; ++nl)
    for (int parts : parts_list)
      for (int threads : threads_list)
        for (int dl = 1; dl <= 16; ++dl) {
          const int per_part = (nl + parts - 1) / parts;  // the host's rule (m3t_hip_api.hip)
          for (int part = 0; part < parts; ++part, ++cases) {
            const int lo = part * per_part, hi = lo + per_part, last = m3t_dist_rows_last(hi, nl);
            const int n_own = last > lo ? last - lo : 0;
            std::vector<int> taken(size_t(n_own) * 16, 0), first_tid(size_t(n_own), -1);
            std::vector<int> wave_trips(size_t(threads / 64), -1);
            for (int tid = 0; tid < threads; ++tid) {
              int trips = 0;
              // the kernel's loop
              for (int line = m3t_dist_rows_line(tid, 0, lo, threads); m3t_dist_rows_wave_line(line, tid) < last;
                   line += m3t_dist_rows_per_trip(threads), ++trips) {
                if (line != m3t_dist_rows_line(tid, trips, lo, threads)) ++errors;
                const int d = m3t_dist_rows_lane(tid);
                if (!m3t_dist_rows_active(line, d, last, dl)) continue;
                if (line < lo || line >= last || line >= nl || d < 0 || d >= dl) { ++errors; continue; }  // outside the part
                ++taken[size_t(line - lo) * 16 + d];
                ++items;
                int& t0 = first_tid[size_t(line - lo)];
                if (t0 < 0) t0 = tid - d;  // lane 0 of the row
                if (tid - d != t0 || t0 % 16 != 0 || t0 / 64 != tid / 64 || (tid & 15) != d) ++errors;  // one aligned row
              }
              if (trips > m3t_dist_rows_trips(lo, last, threads)) ++errors;
              int& wt = wave_trips[size_t(tid / 64)];
              if (wt < 0) wt = trips;
              if (wt != trips) ++errors;  // wave-uniform trip count
            }
            for (int l = 0; l < n_own; ++l)
              for (int d = 0; d < 16; ++d)
                if (taken[size_t(l) * 16 + d] != (d < dl ? 1 : 0)) ++errors;
          }
        }
  std::printf("cases %ld items %ld errors %ld\n", cases, items, errors);
  return errors == 0 ? 0 : 1;
}
