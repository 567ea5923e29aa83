// m3t_dist_rows.h -- item mapping of the row pass of tracking_step_split_moments_kernel (m3t_kernels.hip,
// region_distribution_rows): the distribution values of one line sit in one aligned 16-lane row of one wave, lane d of
// the row holding value d, so that a line's area, mean and variance are row-local chains (DPP row_shr:1) and nothing of
// a line crosses a wave.  Row r = tid >> 4 of the workgroup takes, in trip t, the line line_lo + r + (threads / 16) * t
// of the part's lines [line_lo, last), last = min(line_hi, nl): padded lines below nl included (their rows send what
// they hold).  Lanes d >= distribution_length idle.  Compiles for host and device: tests/cpp/dist_rows_check.cpp
// checks the mapping on the host.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define M3T_DIST_ROWS_FN __host__ __device__ __forceinline__
#else
#define M3T_DIST_ROWS_FN inline
#endif

#define M3T_DIST_ROW_LANES 16  // = M3T_MAX_DISTRIBUTION_LENGTH: every legal length fits a row

M3T_DIST_ROWS_FN int m3t_dist_rows_per_trip(int threads) { return threads / M3T_DIST_ROW_LANES; }
// one past the part's last line
M3T_DIST_ROWS_FN int m3t_dist_rows_last(int line_hi, int nl) { return line_hi < nl ? line_hi : nl; }
// trips of the workgroup (0 for a part without lines)
M3T_DIST_ROWS_FN int m3t_dist_rows_trips(int line_lo, int last, int threads) {
  const int rows = m3t_dist_rows_per_trip(threads);
  return last > line_lo ? (last - line_lo + rows - 1) / rows : 0;
}
M3T_DIST_ROWS_FN int m3t_dist_rows_lane(int tid) { return tid & (M3T_DIST_ROW_LANES - 1); }  // d
M3T_DIST_ROWS_FN int m3t_dist_rows_line(int tid, int trip, int line_lo, int threads) {
  return line_lo + tid / M3T_DIST_ROW_LANES + m3t_dist_rows_per_trip(threads) * trip;
}
// the line of the first row of the thread's wave (64 lanes = 4 rows): a wave's trips end when it leaves the part
M3T_DIST_ROWS_FN int m3t_dist_rows_wave_line(int line, int tid) { return line - ((tid & 63) / M3T_DIST_ROW_LANES); }
// whether the lane takes the item (line, d) in this trip
M3T_DIST_ROWS_FN bool m3t_dist_rows_active(int line, int d, int last, int distribution_length) {
  return line < last && d < distribution_length;
}
