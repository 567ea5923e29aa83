// extern "C" face of m3t_raster.h for tools/raster_stats.py: bounding-box and coverage statistics of a mesh under one
// focused projection (what the rasteriser's work distribution has to cope with)
#include <vector>

#include "../../3dobjecttracking_amd/csrc/m3t_raster.h"

extern "C" {
// out: [0] triangles that survive set-up, [1] sum of box pixels, [2] covered pixels, [3] boxes > 192 px, [4] largest box,
// [5..5+15] histogram of box sizes by power of two (1, 2-3, 4-7, ...), [21..36] the same for covered pixels per triangle
void raster_stats(const float* trans16, const float* vertices, const int* triangles, int n_triangles, int culling, int S,
                  long long* out) {
  RasterM44 trans;
  for (int i = 0; i < 16; ++i) trans.m[i] = trans16[i];
  for (int i = 0; i < 40; ++i) out[i] = 0;
  for (int t = 0; t < n_triangles; ++t) {
    RasterTriangle tri;
    if (!raster_setup(trans, vertices, triangles, t, culling != 0, S, tri)) continue;
    const long long box = (long long)(tri.x1 - tri.x0 + 1) * (tri.y1 - tri.y0 + 1);
    long long covered = 0;
    auto sink = [&](int, int, uint32_t) { ++covered; };
    for (int py = tri.y0; py <= tri.y1; ++py) raster_row(tri, py, tri.x0, tri.x1, 0u, sink);
    out[0] += 1;
    out[1] += box;
    out[2] += covered;
    out[3] += box > 192;
    if (box > out[4]) out[4] = box;
    int b = 0;
    while ((1ll << (b + 1)) <= box && b < 15) ++b;
    out[5 + b] += 1;
    int c = 0;
    while ((1ll << (c + 1)) <= covered && c < 15) ++c;
    if (covered > 0) out[21 + c] += 1;
  }
}
}

// What becomes of every triangle and pixel of one body under one projection, for tests/test_render_edge_cases.py: the
// counters that show a case of tests/render_edges.py reaches the branch it was written for.  The stages are those of
// raster_vertex / raster_setup_snapped in their order; the pixels are judged with raster_pixel's expressions.
// n_slices: the set-up grid's slices (a slice is ceil(n / n_slices) consecutive triangles, walked in trips of 512).
// out: [0] triangles dropped because a vertex has cw <= 0, [1] dropped as out of range (|sx| or |sy| >= 3e7, no vertex
// behind the eye), [2] dropped for zero area, [3] culled, [4] without a pixel centre in the box, [5] survivors,
// [6] boxes > 192 px, [7] the most such boxes in one trip of one slice, [8] covered pixels (drawn), [9] pixels rejected
// because the depth leaves [0, 1], [10] covered pixels where an edge function is exactly 0, [11] / [12] survivors whose
// box is exactly 8 / 9 pixels wide, [13] / [14] boxes of exactly 192 / 193 pixels, [15] the most survivors in one wave
// of a trip, [16] waves of a trip without a survivor that hold triangles, [17] pixel centres on a horizontal edge that
// the fill rule gives to the neighbour (no edge function negative, the zero ones all on edges with ey == 0 that do not
// own their pixels)
extern "C" void raster_edge_stats(const float* trans16, const float* vertices, const int* triangles, int n_triangles,
                                  int culling, int S, int n_slices, long long* out) {
  RasterM44 trans;
  for (int i = 0; i < 16; ++i) trans.m[i] = trans16[i];
  for (int i = 0; i < 24; ++i) out[i] = 0;
  const int per_slice = (n_triangles + n_slices - 1) / n_slices;
  std::vector<long long> big_in_trip, in_wave, survivors_in_wave;
  for (int t = 0; t < n_triangles; ++t) {
    const int slice = t / per_slice, within = t - slice * per_slice;
    const size_t trip = size_t(slice) * size_t((per_slice + 511) / 512) + size_t(within / 512);
    const size_t wave = size_t(slice) * size_t((per_slice + 63) / 64 + 8) + size_t(within / 64);
    if (big_in_trip.size() <= trip) big_in_trip.resize(trip + 1, 0);
    if (in_wave.size() <= wave) {
      in_wave.resize(wave + 1, 0);
      survivors_in_wave.resize(wave + 1, 0);
    }
    ++in_wave[wave];
    double sx[3], sy[3];
    float wz[3];
    bool behind = false, accepted = true;
    for (int k = 0; k < 3; ++k) {
      const float* p = vertices + (size_t)triangles[t * 3 + k] * 3;
      const float cw = ((trans(3, 0) * p[0] + trans(3, 1) * p[1]) + trans(3, 2) * p[2]) + trans(3, 3);
      behind = behind || !(cw > 0.0f);
      accepted = raster_vertex(trans, p, S, &sx[k], &sy[k], &wz[k]) && accepted;
    }
    if (behind) { ++out[0]; continue; }
    if (!accepted) { ++out[1]; continue; }
    const double area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sy[1] - sy[0]) * (sx[2] - sx[0]);
    if (area == 0.0) { ++out[2]; continue; }
    if (area > 0.0 && culling) { ++out[3]; continue; }
    RasterTriangle tri;
    if (!raster_setup_snapped(sx, sy, wz, culling != 0, S, tri)) { ++out[4]; continue; }
    ++out[5];
    ++survivors_in_wave[wave];
    const int width = tri.x1 - tri.x0 + 1;
    const long long box = (long long)width * (tri.y1 - tri.y0 + 1);
    if (box > 192) {
      ++out[6];
      ++big_in_trip[trip];
    }
    out[11] += width == 8;
    out[12] += width == 9;
    out[13] += box == 192;
    out[14] += box == 193;
    for (int py = tri.y0; py <= tri.y1; ++py)
      for (int px = tri.x0; px <= tri.x1; ++px) {
        const double cx = (double)px * 256.0 + 128.0, cy = (double)py * 256.0 + 128.0;
        double e[3];
        bool inside = true, tie = false, negative = false, other_zero = false;
        for (int k = 0; k < 3; ++k) {
          const int k1 = (k + 1) % 3;
          const double ex = tri.ax[k1] - tri.ax[k], ey = tri.ay[k1] - tri.ay[k];
          e[k] = ex * (cy - tri.ay[k]) - ey * (cx - tri.ax[k]);
          const bool owns = ey < 0.0 || (ey == 0.0 && ex > 0.0);
          inside = inside && (e[k] > 0.0 || (e[k] == 0.0 && owns));
          tie = tie || e[k] == 0.0;
          negative = negative || e[k] < 0.0;
          other_zero = other_zero || (e[k] == 0.0 && !owns && ey != 0.0);
        }
        if (!inside) {
          out[17] += !negative && !other_zero;
          continue;
        }
        if (raster_depth_word(tri, e[0], e[1], e[2], 0u) == 0xffffffffu) {
          ++out[9];
        } else {
          ++out[8];
          out[10] += tie;
        }
      }
  }
  for (long long b : big_in_trip) out[7] = b > out[7] ? b : out[7];
  for (size_t w = 0; w < in_wave.size(); ++w) {
    out[15] = survivors_in_wave[w] > out[15] ? survivors_in_wave[w] : out[15];
    out[16] += in_wave[w] > 0 && survivors_in_wave[w] == 0;
  }
}

// The whole rendering of one body list into a z-buffer the way focused_setup_kernel + focused_resolve_kernel do it
// (set-up, survivors, row scan, minimum of the packed words, unpack), for tests/test_raster_scene.py: against the
// oracle's focused renderer on the same scene.  packed: [S * S] words, 0xffffffff = nothing (the caller clears it).
extern "C" void raster_body(const float* trans16, const float* vertices, const int* triangles, int n_triangles, int culling,
                            int S, unsigned low_bits, unsigned* packed) {
  RasterM44 trans;
  for (int i = 0; i < 16; ++i) trans.m[i] = trans16[i];
  std::vector<RasterTriangle> survivors;
  for (int t = 0; t < n_triangles; ++t) {
    RasterTriangle tri;
    if (raster_setup(trans, vertices, triangles, t, culling != 0, S, tri)) survivors.push_back(tri);
  }
  auto sink = [&](int px, int py, uint32_t word) {
    if (word < packed[py * S + px]) packed[py * S + px] = word;
  };
  for (const RasterTriangle& tri : survivors) {
    const int pixels = (tri.x1 - tri.x0 + 1) * (tri.y1 - tri.y0 + 1);
    if (pixels <= 192) {
      for (int py = tri.y0; py <= tri.y1; ++py) raster_row(tri, py, tri.x0, tri.x1, low_bits, sink);
    } else {  // the workgroup path: 32-pixel pieces of the rows
      const int pieces = (tri.x1 - tri.x0 + 32) / 32, total = pieces * (tri.y1 - tri.y0 + 1);
      for (int k = 0; k < total; ++k) {
        const int row = k / pieces, xa = tri.x0 + (k - row * pieces) * 32;
        raster_row(tri, tri.y0 + row, xa, xa + 31 < tri.x1 ? xa + 31 : tri.x1, low_bits, sink);
      }
    }
  }
}
