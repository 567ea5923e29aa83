// The launch choice of the focused renderers (3dobjecttracking_amd/csrc/m3t_render_plan.h) on the host.  The expected
// values are written down from the rule: slices = min(128, max(2, 128 / pairs)), bands = min(max(8, S / 2),
// max(8, 256 / pairs)), LDS = ceil(S / bands) * S * 4 + (513 + 16 + 4 * 512) * 4 = ... + 10308 bytes, the two-launch
// form while that is at most 160 KB = 163840 bytes.
//   render_plan_check                                  runs the cases, prints "checks N errors M"
//   render_plan_check --plan PAIRS LARGEST [IMAGE] [--bands N] [--slices N] [--no-lds]
//                                                      prints the plan of such a launch and how its bands cut a renderer
//                                                      of size IMAGE (default LARGEST), one "key value" per line
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../3dobjecttracking_amd/csrc/m3t_render_plan.h"

using namespace m3t_render;

static int g_checks = 0, g_errors = 0;
#define CHECK(cond)                                  \
  do {                                               \
    ++g_checks;                                      \
    if (!(cond)) {                                   \
      ++g_errors;                                    \
      std::printf("line %d: %s\n", __LINE__, #cond); \
    }                                                \
  } while (0)

static RenderOverrides None() { return RenderOverrides(); }
static RenderOverrides Bands(int n) {
  RenderOverrides o;
  o.bands_set = true;
  o.bands = n;
  return o;
}
static RenderOverrides Slices(int n) {
  RenderOverrides o;
  o.slices_set = true;
  o.slices = n;
  return o;
}
static bool Is(int pairs, int S, const RenderOverrides& o, int slices, int bands, size_t lds, bool lds_form) {
  const RenderLaunchShape s = RenderShape(pairs, S, o);
  return s.slices == slices && s.bands == bands && s.lds == lds && LdsRasterFits(s, S, !o.no_lds_raster) == lds_form;
}

struct BandCounts {
  int vector_bands = 0, scalar_bands = 0, one_row_bands = 0, partial_bands = 0, empty_bands = 0, band_rows = 0;
};
static BandCounts Count(int image, int bands) {
  BandCounts c;
  c.band_rows = (image + bands - 1) / bands;
  for (int b = 0; b < bands; ++b) {
    const BandRows r = RowsOfBand(image, bands, b);
    if (r.row_lo > r.row_hi) {
      ++c.empty_bands;
      continue;
    }
    const int rows = r.row_hi - r.row_lo + 1;
    (BandStoresVectors(image, r) ? c.vector_bands : c.scalar_bands) += 1;
    c.one_row_bands += rows == 1;
    c.partial_bands += rows < c.band_rows;
  }
  return c;
}

static void Defaults() {
  // one pair (StartRendering): 128 slices, 256 bands at most, two rows a band at least
  CHECK(Is(1, 8, None(), 128, 8, 1 * 8 * 4 + 10308, true));
  CHECK(Is(1, 9, None(), 128, 8, 2 * 9 * 4 + 10308, true));
  CHECK(Is(1, 13, None(), 128, 8, 2 * 13 * 4 + 10308, true));
  CHECK(Is(1, 64, None(), 128, 32, 2 * 64 * 4 + 10308, true));
  CHECK(Is(1, 200, None(), 128, 100, 2 * 200 * 4 + 10308, true));
  CHECK(Is(1, 333, None(), 128, 166, 3 * 333 * 4 + 10308, true));  // (not "the z-buffer in memory": ~14 KB)
  CHECK(Is(1, 1024, None(), 128, 256, 4 * 1024 * 4 + 10308, true));
  // two pairs (the fixture's tracker: a pair of twins per camera)
  CHECK(Is(2, 8, None(), 64, 8, 32 + 10308, true));
  CHECK(Is(2, 9, None(), 64, 8, 72 + 10308, true));
  CHECK(Is(2, 13, None(), 64, 8, 104 + 10308, true));
  CHECK(Is(2, 64, None(), 64, 32, 512 + 10308, true));
  CHECK(Is(2, 200, None(), 64, 100, 1600 + 10308, true));
  CHECK(Is(2, 333, None(), 64, 128, 3 * 333 * 4 + 10308, true));
  CHECK(Is(2, 1024, None(), 64, 128, 8 * 1024 * 4 + 10308, true));
  // eight pairs
  CHECK(Is(8, 8, None(), 16, 8, 32 + 10308, true));
  CHECK(Is(8, 9, None(), 16, 8, 72 + 10308, true));
  CHECK(Is(8, 13, None(), 16, 8, 104 + 10308, true));
  CHECK(Is(8, 64, None(), 16, 32, 512 + 10308, true));
  CHECK(Is(8, 200, None(), 16, 32, 7 * 200 * 4 + 10308, true));
  CHECK(Is(8, 333, None(), 16, 32, 11 * 333 * 4 + 10308, true));
  CHECK(Is(8, 1024, None(), 16, 32, 32 * 1024 * 4 + 10308, true));
  // 128 pairs (64 objects with twins on two cameras): 2 slices, 8 bands
  CHECK(Is(128, 8, None(), 2, 8, 32 + 10308, true));
  CHECK(Is(128, 9, None(), 2, 8, 72 + 10308, true));
  CHECK(Is(128, 13, None(), 2, 8, 104 + 10308, true));
  CHECK(Is(128, 64, None(), 2, 8, 8 * 64 * 4 + 10308, true));
  CHECK(Is(128, 200, None(), 2, 8, 25 * 200 * 4 + 10308, true));
  CHECK(Is(128, 333, None(), 2, 8, 42 * 333 * 4 + 10308, true));
  CHECK(Is(128, 1024, None(), 2, 8, size_t(128) * 1024 * 4 + 10308, false));  // 512 KB a band: three launches
  // beyond: never fewer than 2 slices and 8 bands; no pairs counts as one
  CHECK(Is(1000, 200, None(), 2, 8, 25 * 200 * 4 + 10308, true));
  CHECK(Is(0, 200, None(), 128, 100, 1600 + 10308, true));
}

static void Overrides() {
  CHECK(Is(1, 13, Bands(4), 128, 4, 4 * 13 * 4 + 10308, true));
  CHECK(Is(1, 64, Bands(1), 128, 1, 64 * 64 * 4 + 10308, true));
  CHECK(Is(1, 200, Bands(0), 128, 1, 200 * 200 * 4 + 10308, false));   // atoi("") = 0 -> 1 band: 160 000 + 10 308
  CHECK(Is(1, 200, Bands(-3), 128, 1, 200 * 200 * 4 + 10308, false));
  CHECK(Is(1, 200, Bands(2), 128, 2, 100 * 200 * 4 + 10308, true));
  CHECK(Is(2, 200, Bands(1000), 64, 1000, 1 * 200 * 4 + 10308, true));  // more bands than rows: the rest is empty
  CHECK(Is(1, 200, Slices(1), 1, 100, 1600 + 10308, true));
  CHECK(Is(1, 200, Slices(3), 3, 100, 1600 + 10308, true));
  CHECK(Is(128, 200, Slices(0), 1, 8, 25 * 200 * 4 + 10308, true));
  CHECK(Is(1, 200, Slices(4096), 4096, 100, 1600 + 10308, true));
  RenderOverrides no_lds;
  no_lds.no_lds_raster = true;
  CHECK(Is(1, 200, no_lds, 128, 100, 1600 + 10308, false));
  CHECK(Is(1, 8, no_lds, 128, 8, 32 + 10308, false));
  RenderOverrides both = Bands(4);
  both.slices_set = true;
  both.slices = 3;
  CHECK(Is(8, 13, both, 3, 4, 4 * 13 * 4 + 10308, true));
}

static void Boundary() {
  // 163840 - 10308 = 153532 bytes of z-buffer band
  CHECK(Is(1, 333, Bands(3), 128, 3, 111 * 333 * 4 + 10308, true));    // 158 160
  CHECK(Is(1, 333, Bands(2), 128, 2, 167 * 333 * 4 + 10308, false));   // 232 752
  CHECK(Is(1, 1024, Bands(28), 128, 28, 37 * 1024 * 4 + 10308, true));   // 161 860
  CHECK(Is(1, 1024, Bands(27), 128, 27, 38 * 1024 * 4 + 10308, false));  // 165 956
  RenderLaunchShape s{128, 8, kCuLdsBytes};
  CHECK(LdsRasterFits(s, 200, true));
  s.lds = kCuLdsBytes + 1;
  CHECK(!LdsRasterFits(s, 200, true));
  s.lds = 1;
  CHECK(!LdsRasterFits(s, 0, true));
  CHECK(!LdsRasterFits(s, 200, false));
  CHECK(kCuLdsBytes == 163840 && kThreeLaunchSlices == 32 && kBlockThreads == 512 && kResolvePer == 4);
}

static void BandGeometry() {
  // S = 8, 8 bands: one row each, 8 pixels from a multiple of 8: all vector stores
  BandCounts c = Count(8, 8);
  CHECK(c.band_rows == 1 && c.vector_bands == 8 && c.scalar_bands == 0 && c.one_row_bands == 8 && c.empty_bands == 0);
  // S = 9, 8 bands of 2 rows (18 pixels): rows 0-1 .. 6-7, row 8 alone, three bands without a row.  Band b starts at
  // pixel 18 b and 18 is no multiple of four: scalar stores throughout
  c = Count(9, 8);
  CHECK(c.band_rows == 2 && c.vector_bands == 0 && c.scalar_bands == 5 && c.one_row_bands == 1 && c.partial_bands == 1 &&
        c.empty_bands == 3);
  // S = 10: 5 bands of 20 pixels (vector), 3 empty
  c = Count(10, 8);
  CHECK(c.band_rows == 2 && c.vector_bands == 5 && c.scalar_bands == 0 && c.partial_bands == 0 && c.empty_bands == 3);
  // S = 13, 8 bands of 2 rows (26 pixels: scalar), row 12 alone, one empty
  c = Count(13, 8);
  CHECK(c.band_rows == 2 && c.vector_bands == 0 && c.scalar_bands == 7 && c.one_row_bands == 1 && c.empty_bands == 1);
  // S = 13, 4 bands of 4 rows (52 pixels: vector), the last one row 12 alone (13 pixels from 156: scalar)
  c = Count(13, 4);
  CHECK(c.band_rows == 4 && c.vector_bands == 3 && c.scalar_bands == 1 && c.one_row_bands == 1 && c.partial_bands == 1 &&
        c.empty_bands == 0);
  c = Count(64, 32);
  CHECK(c.band_rows == 2 && c.vector_bands == 32 && c.scalar_bands == 0 && c.empty_bands == 0);
  c = Count(64, 1);
  CHECK(c.band_rows == 64 && c.vector_bands == 1);
  c = Count(200, 100);
  CHECK(c.band_rows == 2 && c.vector_bands == 100 && c.empty_bands == 0);
  // S = 201, 100 bands of 3 rows: 67 bands, 33 empty; band b starts at 603 b: every fourth band starts at a multiple of
  // four, but its 603 pixels are no multiple of four: scalar
  c = Count(201, 100);
  CHECK(c.band_rows == 3 && c.vector_bands == 0 && c.scalar_bands == 67 && c.empty_bands == 33 && c.partial_bands == 0);
  // S = 333, 166 bands of 3 rows: 111 bands, 55 empty
  c = Count(333, 166);
  CHECK(c.band_rows == 3 && c.vector_bands == 0 && c.scalar_bands == 111 && c.empty_bands == 55);
  c = Count(1024, 256);
  CHECK(c.band_rows == 4 && c.vector_bands == 256 && c.empty_bands == 0);
  // a small renderer in a launch whose grid the largest one decides (S = 8 beside S = 333, two pairs: 128 bands)
  c = Count(8, 128);
  CHECK(c.band_rows == 1 && c.vector_bands == 8 && c.empty_bands == 120);
  const BandRows last = RowsOfBand(9, 8, 7);
  CHECK(last.row_lo == 14 && last.row_hi == 8);
}

// every override as ReadRenderOverrides reads it
static void Environment() {
  unsetenv("M3T_HIP_RASTER_BANDS");
  unsetenv("M3T_HIP_RASTER_SLICES");
  unsetenv("M3T_HIP_NO_LDS_RASTER");
  RenderOverrides o = ReadRenderOverrides();
  CHECK(!o.bands_set && !o.slices_set && !o.no_lds_raster);
  setenv("M3T_HIP_RASTER_BANDS", "4", 1);
  o = ReadRenderOverrides();
  CHECK(o.bands_set && o.bands == 4 && !o.slices_set && !o.no_lds_raster);
  setenv("M3T_HIP_RASTER_BANDS", "", 1);
  o = ReadRenderOverrides();
  CHECK(o.bands_set && o.bands == 0);
  CHECK(RenderShape(1, 64, o).bands == 1);
  unsetenv("M3T_HIP_RASTER_BANDS");
  setenv("M3T_HIP_RASTER_SLICES", "3", 1);
  o = ReadRenderOverrides();
  CHECK(!o.bands_set && o.slices_set && o.slices == 3);
  setenv("M3T_HIP_RASTER_SLICES", "x", 1);
  CHECK(RenderShape(1, 64, ReadRenderOverrides()).slices == 1);
  unsetenv("M3T_HIP_RASTER_SLICES");
  setenv("M3T_HIP_NO_LDS_RASTER", "0", 1);  // a flag: present counts, whatever it holds
  o = ReadRenderOverrides();
  CHECK(o.no_lds_raster && !o.bands_set && !o.slices_set);
  setenv("M3T_HIP_NO_LDS_RASTER", "", 1);
  CHECK(ReadRenderOverrides().no_lds_raster);
  unsetenv("M3T_HIP_NO_LDS_RASTER");
  CHECK(!ReadRenderOverrides().no_lds_raster);
}

static int PrintPlan(int argc, char** argv) {
  int numbers[3] = {0, 0, 0}, n_numbers = 0;
  RenderOverrides o;
  for (int i = 2; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--bands") && i + 1 < argc) {
      o.bands_set = true;
      o.bands = std::atoi(argv[++i]);
    } else if (!std::strcmp(argv[i], "--slices") && i + 1 < argc) {
      o.slices_set = true;
      o.slices = std::atoi(argv[++i]);
    } else if (!std::strcmp(argv[i], "--no-lds")) {
      o.no_lds_raster = true;
    } else if (n_numbers < 3) {
      numbers[n_numbers++] = std::atoi(argv[i]);
    } else {
      return 2;
    }
  }
  if (n_numbers < 2) return 2;
  const int pairs = numbers[0], largest = numbers[1], image = n_numbers == 3 ? numbers[2] : largest;
  const RenderLaunchShape s = RenderShape(pairs, largest, o);
  const bool lds_form = LdsRasterFits(s, largest, !o.no_lds_raster);
  std::printf("form %s\n", lds_form ? "lds" : "three");
  std::printf("slices %d\n", lds_form ? s.slices : kThreeLaunchSlices);
  std::printf("bands %d\n", lds_form ? s.bands : 0);
  std::printf("lds %zu\n", lds_form ? s.lds : size_t(0));
  const BandCounts c = lds_form ? Count(image, s.bands) : BandCounts();
  std::printf("band_rows %d\nvector_bands %d\nscalar_bands %d\none_row_bands %d\npartial_bands %d\nempty_bands %d\n",
              c.band_rows, c.vector_bands, c.scalar_bands, c.one_row_bands, c.partial_bands, c.empty_bands);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--plan")) return PrintPlan(argc, argv);
  Defaults();
  Overrides();
  Boundary();
  BandGeometry();
  Environment();
  std::printf("checks %d errors %d\n", g_checks, g_errors);
  return g_errors ? 1 : 0;
}
