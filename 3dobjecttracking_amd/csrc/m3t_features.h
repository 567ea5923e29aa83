// m3t_features.h -- the arithmetic of the built-in texture detector that host and device share.  The detector is the
// project's own (the reference delegates to OpenCV classes; this is none of them): the focused grey image of
// DetectAndComputeCorrKeypoints (texture_modality.cpp:861-868) by an integer bilinear sample, FAST-9 of 16 with a
// sum-of-excess score, a direction out of 30 from the intensity centroid and a 256-test binary descriptor on 5 x 5 box
// sums, steered by integer rotation.  tests/feature_reference.py is the definition; everything here is integer apart
// from the f32 operations of the sample position, which are single correctly rounded operations.  Free of device-only
// constructs so that tests/cpp/feature_check.cpp runs it on the host.
#pragma once
#include <math.h>
#include <stdint.h>

#include "m3t_brief_pattern.h"

#if defined(__HIPCC__)
#define M3T_FEAT_FN __host__ __device__ __forceinline__
#else
#define M3T_FEAT_FN static inline
#endif

#define M3T_TEXTURE_FOCUSED_MAX 512  /* largest side of a focused image: see the LDS of texture_fast_kernel */
#define M3T_FEATURE_BORDER 16        /* a corner is at least this far from every edge of the focused image */
#define M3T_FEATURE_BAND 16          /* rows of the focused image per workgroup of the focus and FAST kernels */
#define M3T_FEATURE_FAST_HALO 4      /* 3 rows of the circle + 1 of the suppression */
#define M3T_FEATURE_MOMENT_RADIUS 15 /* disc of the intensity centroid */
#define M3T_FEATURE_BOX_RADIUS 2     /* 5 x 5 box sums */
#define M3T_FEATURE_DIRECTIONS 30
#define M3T_FEATURE_MAX_SCORE 4080   /* 16 * 255 */
#define M3T_FEATURE_SCORE_BINS 4096

// round(16384 cos(2 pi k / 30)), round(16384 sin(2 pi k / 30))
#define M3T_FEATURE_COS_VALUES                                                                                       \
  16384, 16026, 14968, 13255, 10963, 8192, 5063, 1713, -1713, -5063, -8192, -10963, -13255, -14968, -16026, -16384, \
      -16026, -14968, -13255, -10963, -8192, -5063, -1713, 1713, 5063, 8192, 10963, 13255, 14968, 16026
#define M3T_FEATURE_SIN_VALUES                                                                                      \
  0, 3406, 6664, 9630, 12176, 14189, 15582, 16294, 16294, 15582, 14189, 12176, 9630, 6664, 3406, 0, -3406, -6664, \
      -9630, -12176, -14189, -15582, -16294, -16294, -15582, -14189, -12176, -9630, -6664, -3406
// the Bresenham circle of radius 3, clockwise from the top: {dx, dy} of circle pixel i
#define M3T_FEATURE_CIRCLE_VALUES \
  0, -3, 1, -3, 2, -2, 3, -1, 3, 0, 3, 1, 2, 2, 1, 3, 0, 3, -1, 3, -2, 2, -3, 1, -3, 0, -3, -1, -2, -2, -1, -3

// grey of a BGR8 pixel
M3T_FEAT_FN int m3t_feat_grey(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14; }

// side of the focused image for a side of the region of interest, at least 1
M3T_FEAT_FN int m3t_feat_focused_side(int roi_side, float scale) {
  const int s = (int)((float)roi_side * scale + 0.5f);
  return s < 1 ? 1 : s;
}

// where destination coordinate x of the focused image samples a side of n source pixels: the two source indices and
// the weight of the second out of 2048
M3T_FEAT_FN void m3t_feat_sample_axis(int x, float scale, int n, int* i0, int* i1, int* weight) {
  const float fx = ((float)x + 0.5f) / scale - 0.5f;
  const float f0 = floorf(fx);
  const float a = fx - f0;
  int x0, w;
  if (f0 < 0.0f) {
    x0 = 0;
    w = 0;
  } else if (f0 >= (float)(n - 1)) {
    x0 = n - 1;
    w = 0;
  } else {
    x0 = (int)f0;
    w = (int)(a * 2048.0f + 0.5f);
  }
  *i0 = x0;
  *i1 = x0 + 1 < n - 1 ? x0 + 1 : n - 1;
  *weight = w;
}

// g00: (x0, y0), g01: (x1, y0), g10: (x0, y1), g11: (x1, y1); wx, wy: the weights of x1 and y1 out of 2048
M3T_FEAT_FN int m3t_feat_bilinear(int g00, int g01, int g10, int g11, int wx, int wy) {
  const uint32_t ux = (uint32_t)wx, uy = (uint32_t)wy, vx = 2048u - ux, vy = 2048u - uy;
  const uint32_t sum = vx * vy * (uint32_t)g00 + ux * vy * (uint32_t)g01 + vx * uy * (uint32_t)g10 + ux * uy * (uint32_t)g11;
  return (int)((sum + (1u << 21)) >> 22);
}

// 1 iff the 16-bit circular mask holds a run of nine set bits
M3T_FEAT_FN int m3t_feat_run_of_nine(uint32_t mask16) {
  const uint32_t m = mask16 | (mask16 << 16);
  const uint32_t r2 = m & (m >> 1);
  const uint32_t r4 = r2 & (r2 >> 2);
  const uint32_t r8 = r4 & (r4 >> 4);
  return ((r8 & (m >> 8)) & 0xffffu) != 0u;
}

// FAST-9 of 16 at a pixel of value p with circle values c[16] and threshold t: the score of a corner -- the larger of
// the summed excess of the brighter and of the darker circle pixels, at least 9 -- or 0
M3T_FEAT_FN int m3t_feat_fast_score(int p, const int c[16], int t) {
  uint32_t brighter = 0u, darker = 0u;
  int sum_brighter = 0, sum_darker = 0;
  for (int i = 0; i < 16; ++i) {
    const int up = c[i] - p - t, down = p - c[i] - t;
    if (up > 0) {
      brighter |= 1u << i;
      sum_brighter += up;
    }
    if (down > 0) {
      darker |= 1u << i;
      sum_darker += down;
    }
  }
  if (!m3t_feat_run_of_nine(brighter) && !m3t_feat_run_of_nine(darker)) return 0;
  return sum_brighter > sum_darker ? sum_brighter : sum_darker;
}

// the compass test: a run of nine covers at least two of the circle pixels 0, 4, 8, 12, so a pixel with fewer than two
// of them brighter and fewer than two darker is no corner.  A necessary condition only: skipping on it changes no score.
M3T_FEAT_FN int m3t_feat_compass_may_be_corner(int p, int c0, int c4, int c8, int c12, int t) {
  const int hi = p + t, lo = p - t;
  const int brighter = (c0 > hi) + (c4 > hi) + (c8 > hi) + (c12 > hi);
  const int darker = (c0 < lo) + (c4 < lo) + (c8 < lo) + (c12 < lo);
  return brighter >= 2 || darker >= 2;
}

// direction bin 0 .. 29 of the moments: the largest m10 C[k] + m01 S[k], the lowest k among equals
M3T_FEAT_FN int m3t_feat_direction_bin(int m10, int m01, const int16_t* cos_table, const int16_t* sin_table) {
  int best = 0;
  int64_t best_value = (int64_t)m10 * cos_table[0] + (int64_t)m01 * sin_table[0];
  for (int k = 1; k < M3T_FEATURE_DIRECTIONS; ++k) {
    const int64_t v = (int64_t)m10 * cos_table[k] + (int64_t)m01 * sin_table[k];
    if (v > best_value) {
      best_value = v;
      best = k;
    }
  }
  return best;
}

// a pattern point turned to direction bin k (arithmetic shifts)
M3T_FEAT_FN void m3t_feat_rotate(int x, int y, int c, int s, int* xr, int* yr) {
  *xr = (x * c - y * s + 8192) >> 14;
  *yr = (x * s + y * c + 8192) >> 14;
}

// half the chord of the moment disc at row dy: the largest dx with dx^2 + dy^2 <= 15^2
M3T_FEAT_FN int m3t_feat_disc_half_width(int dy) {
  const int rest = M3T_FEATURE_MOMENT_RADIUS * M3T_FEATURE_MOMENT_RADIUS - dy * dy;
  int w = 0;
  while ((w + 1) * (w + 1) <= rest) ++w;
  return w;
}
