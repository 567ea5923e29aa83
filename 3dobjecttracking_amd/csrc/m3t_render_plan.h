// m3t_render_plan.h -- how the focused renderers are launched (m3t_render.hip): slices of the triangle lists, bands of
// image rows, the LDS of a resolve workgroup, and whether the two-launch form (z-buffer band in LDS) or the three-launch
// form (z-buffer in memory) runs: the decision apart from the launches.  Plain C++17, no HIP header, no context: the
// library reads the developer overrides with ReadRenderOverrides and passes them in, together with what it learnt of the
// device; tests/cpp/render_plan_check.cpp runs the same code on the host with overrides of its own.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>

namespace m3t_render {

// (m3t_device.h has the same figure as M3T_BLOCK_THREADS; m3t_hip_api.hip asserts that they agree)
constexpr int kBlockThreads = 512;
constexpr size_t kCuLdsBytes = size_t(160) * 1024;
constexpr int kResolvePer = 4;          // survivors a resolve thread looks at per trip (m3t_render_resolve.inc: kPer)
constexpr int kThreeLaunchSlices = 32;  // focused_raster_kernel's grid (M3T_RASTER_SLICES unless the build says otherwise)

// ---- developer overrides -------------------------------------------------------------------------------------------
// M3T_HIP_RASTER_BANDS / M3T_HIP_RASTER_SLICES: numbers (atoi of the text, at least 1), read at every launch.
// M3T_HIP_NO_LDS_RASTER: a flag that counts when the variable exists, whatever it holds; a context looks at it once, at
// its first rendering.
struct RenderOverrides {
  bool bands_set = false, slices_set = false;
  int bands = 0, slices = 0;
  bool no_lds_raster = false;
};
inline RenderOverrides ReadRenderOverrides() {
  RenderOverrides o;
  if (const char* e = std::getenv("M3T_HIP_RASTER_BANDS")) {
    o.bands_set = true;
    o.bands = std::atoi(e);
  }
  if (const char* e = std::getenv("M3T_HIP_RASTER_SLICES")) {
    o.slices_set = true;
    o.slices = std::atoi(e);
  }
  o.no_lds_raster = std::getenv("M3T_HIP_NO_LDS_RASTER") != nullptr;
  return o;
}

// Renderings whose z-buffer band fits the LDS of a CU: set-up + survivor list (slices of the triangle lists per
// renderer), then a workgroup per band of rows that rasterises the survivors in LDS and writes the images.  Larger
// ones: clear + crop, rasterise into a z-buffer in memory, unpack.
struct RenderLaunchShape {
  int slices, bands;
  size_t lds;  // of a resolve workgroup
};
inline RenderLaunchShape RenderShape(int n_pairs, int largest_image_size, const RenderOverrides& overrides) {
  // work spread: ~128 set-up workgroups (slices of the triangle lists) and ~256 resolve workgroups (bands of image
  // rows, at least two rows each) per launch, whatever the number of renderings (measured on the reference's test
  // scene, two pairs of twins, renderer-fed step: 32 bands 0.633 ms, 64: 0.624, 100: 0.611; 64 -> 128 slices: no
  // change, 256: slower)
  // (round 5: at 128 pairs -- the renderer-fed step of 64 objects -- 32 slices per pair were 4096 workgroups of 149
  // VGPRs, one per CU at a time, each paying the projection and the matrix chain for two trips over its triangles:
  // 131 us per set-up launch; 2 slices per pair = one workgroup per CU: 2.33 -> 1.64 ms per step,
  // profiles/r05_render64_knobs.txt)
  RenderLaunchShape s;
  s.slices = std::min(128, std::max(2, 128 / std::max(1, n_pairs)));
  s.bands = std::min(std::max(8, largest_image_size / 2), std::max(8, 256 / std::max(1, n_pairs)));
  if (overrides.bands_set) s.bands = std::max(1, overrides.bands);
  if (overrides.slices_set) s.slices = std::max(1, overrides.slices);
  const size_t band_rows = (size_t(largest_image_size) + s.bands - 1) / s.bands;
  // z-buffer band | prefix sums | wave totals | per-thread counts
  s.lds = band_rows * largest_image_size * 4 + (kBlockThreads + 1 + 16 + kResolvePer * kBlockThreads) * 4;
  return s;
}
// the two-launch form (z-buffer band in LDS) for a rendering of this shape?  lds_form_usable: the device granted the
// resolve kernels 160 KB of dynamic LDS and M3T_HIP_NO_LDS_RASTER was not there when the context looked
inline bool LdsRasterFits(const RenderLaunchShape& shape, int largest_image_size, bool lds_form_usable) {
  return lds_form_usable && largest_image_size > 0 && shape.lds <= kCuLdsBytes;
}

// The rows of band b of a renderer of image size S under a grid of n_bands (m3t_render_resolve.inc): row_lo ..
// row_hi inclusive, row_lo > row_hi for a band past the image's end.
struct BandRows {
  int row_lo, row_hi;
};
inline BandRows RowsOfBand(int image_size, int n_bands, int band) {
  const int band_rows = (image_size + n_bands - 1) / n_bands;
  const int row_lo = band * band_rows;
  return {row_lo, std::min(row_lo + band_rows, image_size) - 1};
}
// the four-pixel stores of the resolve kernel: the band's first pixel and its length are multiples of four
inline bool BandStoresVectors(int image_size, const BandRows& rows) {
  const long long first = (long long)rows.row_lo * image_size, n_out = (long long)(rows.row_hi - rows.row_lo + 1) * image_size;
  return (first & 3) == 0 && (n_out & 3) == 0;
}

}  // namespace m3t_render
