// m3t_texture.h -- the arithmetic of TextureModality (M3T/src/texture_modality.cpp) that host and device share:
// the focused region of interest (:890-931), the Tukey weight (:424-427, 1231-1237), the best-two update and the ratio
// test of the brute-force matcher (:349-367) -- for Hamming-norm descriptors and, further down, for L2-norm ones -- and
// the products of one data point (:407-440).  Free of device-only constructs so that tests/cpp/texture_check.cpp and
// tests/cpp/texture_l2_check.cpp run it on the host.  f32 left to right, no contraction (the library
// and the check are built with -ffp-contract=off), int() truncating.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define M3T_TEX_FN __host__ __device__ __forceinline__
#else
#define M3T_TEX_FN static inline
#endif

#define M3T_TEXTURE_MAX_FEATURES 4096        /* features per frame and points per keyframe */
#define M3T_TEXTURE_MAX_KEYFRAMES 8          /* cap of n_keyframes */
#define M3T_TEXTURE_MAX_DESCRIPTOR_WORDS 16  /* 64 bytes: BRISK, FREAK; ORB has 8 */
#define M3T_TEXTURE_MATCH_THREADS 256        /* query descriptors per pass of texture_match_kernel */
#define M3T_TEXTURE_TRAIN_TILE 128           /* train descriptors per LDS tile: 8 KB at 64 bytes */
#define M3T_TEXTURE_QUERY_TILE 64            /* query descriptors per workgroup of texture_match_tiled_kernel: a lane each */
#define M3T_TEXTURE_ROI_MARGIN 10            /* kRegionOfInterestMargin, texture_modality.h:132 */
#define M3T_TEXTURE_GH_CHUNK 504             /* data points per pass of the g/H chains (a multiple of 24): 54 KB of rows */

M3T_TEX_FN int m3t_tex_f2i(float v) { return (int)v; }

// CalculateScaleAndRegionOfInterest :890-931.  t: translation of body2camera, r: half the body's maximum diameter.
// roi = {x, y, width, height}.  false: z < 1.5 r or an empty rectangle; roi and scale are then left alone.
M3T_TEX_FN bool m3t_tex_region_of_interest(const float t[3], float r, float fu, float fv, float ppu, float ppv, int width,
                                           int height, int focused_image_size, int roi[4], float* scale) {
  const float x = t[0], y = t[1], z = t[2];
  if (z < r * 1.5f) return false;
  const float abs_x = fabsf(x), abs_y = fabsf(y);
  const float x2 = x * x, y2 = y * y, z2 = z * z, r2 = r * r, rz = r * z;
  const float z2_r2 = z2 - r2;
  const float z3_zr2 = z2_r2 * z;
  const float r_u = fu * (abs_x * r2 + rz * sqrtf(z2_r2 + x2)) / z3_zr2;
  const float r_v = fv * (abs_y * r2 + rz * sqrtf(z2_r2 + y2)) / z3_zr2;
  const float center_u = x * fu / z + ppu;
  const float center_v = y * fv / z + ppv;
  const float margin = (float)M3T_TEXTURE_ROI_MARGIN;  // (float - float - int + float: the int converts)
  int u_min = m3t_tex_f2i(center_u - r_u - margin + 0.5f);
  int u_max = m3t_tex_f2i(center_u + r_u + margin + 0.5f);
  int v_min = m3t_tex_f2i(center_v - r_v - margin + 0.5f);
  int v_max = m3t_tex_f2i(center_v + r_v + margin + 0.5f);
  u_min = u_min > 0 ? u_min : 0;
  u_max = u_max < width - 1 ? u_max : width - 1;
  v_min = v_min > 0 ? v_min : 0;
  v_max = v_max < height - 1 ? v_max : height - 1;
  if (u_min >= u_max || v_min >= v_max) return false;
  roi[0] = u_min;
  roi[1] = v_min;
  roi[2] = u_max - u_min;
  roi[3] = v_max - v_min;
  const float du = 2.0f * r_u, dv = 2.0f * r_v;
  *scale = (float)focused_image_size / (du < dv ? dv : du);  // std::max(a, b): a < b ? b : a
  return true;
}

// TukeyNorm :1231-1237.  powf(c, 2) is c * c (the correctly rounded square); the cube is the f32 nearest to the f64
// product.
M3T_TEX_FN float m3t_tex_tukey_norm(float error, float c) {
  const float c2_6 = c * c / 6.0f;
  if (fabsf(error) <= c) {
    const float q = error / c;
    const float t = 1.0f - q * q;
    const double td = (double)t;
    const float cube = (float)((td * td) * td);
    return c2_6 * (1.0f - cube);
  }
  return c2_6;
}
// the weight of a data point :424-427
M3T_TEX_FN float m3t_tex_weight(float error, float squared_error, float c, float variance) {
  float weight = 1.0f / variance;
  if (error > FLT_MIN) weight = (m3t_tex_tukey_norm(error, c) / squared_error) / variance;
  return weight;
}

// The two train descriptors of smallest distance, the lower index first among equals: candidates arrive in ascending
// index, a candidate only displaces an entry it is strictly smaller than (cv::BFMatcher::knnMatch(k = 2)).
struct m3t_tex_best2 {
  int d0, d1;  // distances; INT32_MAX: no entry yet
  int i0;      // train index of the best
};
M3T_TEX_FN void m3t_tex_best2_init(m3t_tex_best2* b) {
  b->d0 = b->d1 = INT32_MAX;
  b->i0 = -1;
}
M3T_TEX_FN void m3t_tex_best2_update(m3t_tex_best2* b, int distance, int index) {
  if (distance < b->d0) {
    b->d1 = b->d0;
    b->d0 = distance;
    b->i0 = index;
  } else if (distance < b->d1) {
    b->d1 = distance;
  }
}
// `later` holds the best two of train descriptors that all follow those of `b` (m3t_texture_tiled.hip: the ranges of the
// four waves): its best is a candidate, then its second, which can at most become the second here, so its index is
// never needed.  An entry that is not there (INT32_MAX) is smaller than nothing and changes nothing.  The result is
// what one pass over both ranges in ascending index gives.
M3T_TEX_FN void m3t_tex_best2_append(m3t_tex_best2* b, const m3t_tex_best2* later) {
  m3t_tex_best2_update(b, later->d0, later->i0);
  m3t_tex_best2_update(b, later->d1, -1);
}
// :364-367: a query becomes a data point iff it has two matches and NOT d0 / d1 >= threshold (0 / 0 = NaN: kept)
M3T_TEX_FN bool m3t_tex_ratio_keeps(const m3t_tex_best2* b, float threshold) {
  if (b->d1 == INT32_MAX) return false;  // knn_match.size() < 2
  return !((float)b->d0 / (float)b->d1 >= threshold);
}

// ---- L2-norm descriptors (SIFT, DAISY: cv::BFMatcher(cv::NORM_L2), :794-796) -------------------------------------------
// A descriptor is D floats, D a multiple of 4 in [4, 256].  The distance is std::sqrt(normL2Sqr(q, t)) of OpenCV's
// batchDistL2_32f with the order of the sum fixed: s = 0, then s = s + (q[k] - t[k]) * (q[k] - t[k]) for k = 0 .. D - 1 in
// ascending order, every operation rounded to f32, no contraction; the distance is sqrtf(s), correctly rounded.
#define M3T_TEXTURE_L2_MIN_FLOATS 4
#define M3T_TEXTURE_L2_MAX_FLOATS 256    /* SIFT: 128; DAISY: (3 * 4 + 1) * 8 = 104, with OpenCV's defaults (3 * 8 + 1) * 8 = 200 */
#define M3T_TEXTURE_L2_QUERY_TILE 64     /* query descriptors per workgroup of texture_match_l2_kernel: a lane each */
#define M3T_TEXTURE_L2_TRAIN_TILE 32     /* train descriptors per LDS tile: a quarter for each of the four waves */
#define M3T_TEXTURE_L2_ROWS 8            /* train rows a thread carries at a time */

M3T_TEX_FN float m3t_tex_l2_squared(const float* q, const float* t, int n_floats) {
  float s = 0.0f;
  for (int k = 0; k < n_floats; ++k) {
    const float e = q[k] - t[k];
    s = s + e * e;
  }
  return s;
}
M3T_TEX_FN float m3t_tex_l2_distance(const float* q, const float* t, int n_floats) {
  return sqrtf(m3t_tex_l2_squared(q, t, n_floats));
}

// The best two of an L2 match.  The comparison is on the distances (the sqrtf values), not on the sums: two sums that
// differ can round to one distance, and then the lower index ranks first.  A NaN distance satisfies no `<` and never
// enters; that leaves NaN free to mark "no entry yet" (+inf is a distance like any other).
struct m3t_tex_best2f {
  float d0, d1;  // distances; NaN: no entry yet
  int i0;        // train index of the best
};
M3T_TEX_FN void m3t_tex_best2f_init(m3t_tex_best2f* b) {
  b->d0 = b->d1 = NAN;
  b->i0 = -1;
}
M3T_TEX_FN void m3t_tex_best2f_update(m3t_tex_best2f* b, float distance, int index) {
  if (distance != distance) return;
  if (b->d0 != b->d0 || distance < b->d0) {
    b->d1 = b->d0;
    b->d0 = distance;
    b->i0 = index;
  } else if (b->d1 != b->d1 || distance < b->d1) {
    b->d1 = distance;
  }
}
// The same update from the sum s, with the square root taken only where it can matter.  s1 is the sum behind d1 (NaN
// while there is no second entry), s0 the sum behind d0.  sqrtf is monotone: s >= s1 gives sqrtf(s) >= d1 >= d0, and
// such a candidate displaces nothing.  Every other candidate (a NaN sum among them) takes the update above.
struct m3t_tex_best2s {
  m3t_tex_best2f b;
  float s0, s1;
};
M3T_TEX_FN void m3t_tex_best2s_init(m3t_tex_best2s* b) {
  m3t_tex_best2f_init(&b->b);
  b->s0 = b->s1 = NAN;
}
M3T_TEX_FN void m3t_tex_best2s_update(m3t_tex_best2s* b, float s, int index) {
  if (s >= b->s1) return;
  const float distance = sqrtf(s);
  if (distance != distance) return;
  if (b->b.d0 != b->b.d0 || distance < b->b.d0) {
    b->b.d1 = b->b.d0;
    b->s1 = b->s0;
    b->b.d0 = distance;
    b->s0 = s;
    b->b.i0 = index;
  } else if (b->b.d1 != b->b.d1 || distance < b->b.d1) {
    b->b.d1 = distance;
    b->s1 = s;
  }
}
// `later` holds the best two of train descriptors that all follow those of `b`: its best is a candidate, then its
// second (which can at most become the second here, so its index is never needed)
M3T_TEX_FN void m3t_tex_best2f_append(m3t_tex_best2f* b, const m3t_tex_best2f* later) {
  m3t_tex_best2f_update(b, later->d0, later->i0);
  m3t_tex_best2f_update(b, later->d1, -1);
}
// :364-367 for an L2 match: two matches and NOT d0 / d1 >= threshold (0 / 0 and inf / inf = NaN: kept)
M3T_TEX_FN bool m3t_tex_ratio_keeps_l2(const m3t_tex_best2f* b, float threshold) {
  if (b->d1 != b->d1) return false;  // knn_match.size() < 2
  return !(b->d0 / b->d1 >= threshold);
}

// What one data point subtracts from gradient_ (out[0 .. 6)) and from the lower triangle of hessian_ (out[6 .. 27),
// column after column: the row order of the library's g/H chains) :407-440.  R: body2camera rotation, column-major;
// (x, y, z): center_f_camera; (cu, cv): center; corr: correspondence_center; cb: center_f_body.
M3T_TEX_FN void m3t_tex_point_products(const float R[9], float fu, float fv, float x, float y, float z, float cu, float cv,
                                       const float corr[2], const float cb[3], float tukey_norm_constant, float variance,
                                       float out[27]) {
  const float z2 = z * z;
  const float d0 = cu - corr[0], d1 = cv - corr[1];
  const float squared_error = d0 * d0 + d1 * d1;
  const float error = sqrtf(squared_error);
  const float weight = m3t_tex_weight(error, squared_error, tukey_norm_constant, variance);
  // dx_dX = [fu / z, 0, -x fu / z2; 0, fv / z, -y fv / z2]
  const float a00 = fu / z, a02 = -x * fu / z2, a11 = fv / z, a12 = -y * fv / z2;
  // dx_dtranslation = dx_dX * R (2 x 3): the products with the two zeros are part of Eigen's sums
  float T0[3], T1[3];
  for (int k = 0; k < 3; ++k) {
    T0[k] = (a00 * R[k * 3 + 0] + 0.0f * R[k * 3 + 1]) + a02 * R[k * 3 + 2];
    T1[k] = (0.0f * R[k * 3 + 0] + a11 * R[k * 3 + 1]) + a12 * R[k * 3 + 2];
  }
  // -dx_dtranslation * skew(cb); skew = [0, -c2, c1; c2, 0, -c0; -c1, c0, 0], its zero products dropped
  const float c0 = cb[0], c1 = cb[1], c2 = cb[2];
  float J0[6], J1[6];
  J0[0] = (-T0[1]) * c2 + (-T0[2]) * (-c1);
  J0[1] = (-T0[0]) * (-c2) + (-T0[2]) * c0;
  J0[2] = (-T0[0]) * c1 + (-T0[1]) * (-c0);
  J1[0] = (-T1[1]) * c2 + (-T1[2]) * (-c1);
  J1[1] = (-T1[0]) * (-c2) + (-T1[2]) * c0;
  J1[2] = (-T1[0]) * c1 + (-T1[1]) * (-c0);
  for (int k = 0; k < 3; ++k) {
    J0[3 + k] = T0[k];
    J1[3 + k] = T1[k];
  }
  const float wd0 = weight * d0, wd1 = weight * d1;
  for (int k = 0; k < 6; ++k) out[k] = wd0 * J0[k] + wd1 * J1[k];
  int row = 6;
  for (int c = 0; c < 6; ++c)
    for (int r = c; r < 6; ++r) out[row++] = (weight * J0[r]) * J0[c] + (weight * J1[r]) * J1[c];
}
