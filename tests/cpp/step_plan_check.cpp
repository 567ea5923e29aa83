// The launch choice of m3t_hip_execute_tracking_step (3dobjecttracking_amd/csrc/m3t_step_plan.h) on the host, with a
// stub in the place of the runtime's occupancy query: one workgroup of 512 threads per CU, two of 256.  The expected
// values are written down from the conditions of the step function the header was taken from and from what the GPU
// tests assert of whole trajectories (tests/test_gpu_benchmark_shape.py: [64, 4, 512, 1]; tests/fused_edges.py).
//   step_plan_check          runs the cases, prints "checks N errors M"
//   step_plan_check --names  prints the name of every StepKernel enumerator, one per line
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../3dobjecttracking_amd/csrc/m3t_step_plan.h"

using namespace m3t_step;

static int g_checks = 0, g_errors = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++g_checks;                                                      \
    if (!(cond)) {                                                   \
      ++g_errors;                                                    \
      std::printf("line %d: %s\n", __LINE__, #cond);                 \
    }                                                                \
  } while (0)

static int g_queries = 0;
static int Resident(StepKernel, int threads, size_t) {
  ++g_queries;
  return threads == 512 ? 1 : (threads == 256 ? 2 : 0);
}
static int NoneResident(StepKernel, int, size_t) { return 0; }

// 200 lines, function_length 8, distribution_length 12, 32 bins: the benchmark's Region-only objects.  Working set
// 4 * (1024 + 31 * 200 + 3 * 200 * 19) = 74496 bytes, count table 4096 + 32^3 * 4 bytes, pair table read from L2.
static RigidStepFacts Region(int n) {
  RigidStepFacts f;
  f.n = n;
  f.compute_cus = 256;
  f.lds_track = 74496;
  f.lds_hist = 4096 + 32768 * 4;
  f.lds_compact = 47 * 1024;
  f.lds_compact_table = 52 * 1024;
  f.table_cap = 1024;
  f.off_hist = -1;
  f.total_floats = 18624;
  f.nl = 200;
  f.np_max = 0;
  f.has_region = true;
  f.regions_allow_moments_first = RegionAllowsMomentsFirst(false, false, false, 1);
  f.n_corr_iterations = 7;
  f.n_update_iterations = 2;
  f.fuse_histogram_possible = f.split_possible = f.compact_possible = true;
  f.compact_fuses_histogram = false;  // (32 bins: the count table does not fit next to the compact kernel's scratch)
  return f;
}
// Region + Depth, 16 bins: the pair table (32 KB) staged in LDS behind the working set, 200 points
static RigidStepFacts RegionDepth(int n) {
  RigidStepFacts f = Region(n);
  f.has_depth = true;
  f.np_max = 200;
  f.off_hist = 18624;
  f.total_floats = 18624 + 8192;
  f.lds_track = size_t(f.total_floats) * 4;
  f.lds_hist = 4096 + 4096 * 4;
  f.lds_compact_table = 0;
  f.compact_fuses_histogram = true;
  return f;
}
static StepOverrides None() { return StepOverrides(); }
static EnvNumber Set(int v) {
  EnvNumber e;
  e.set = true;
  e.value = v;
  return e;
}
static bool Shape(const RigidStepPlan& p, int n, StepKernel k, int parts, int threads, int fused) {
  (void)n;
  return p.kernel == k && (p.split() ? p.parts : 1) == parts && p.threads == threads && int(p.histogram_fused) == fused;
}

static void Headline() {
  for (int n_corr : {1, 7}) {
    RigidStepFacts f = Region(64);
    f.n_corr_iterations = n_corr;
    RigidStepPlan p = PlanRigidStep(f, None(), Resident);
    CHECK(Shape(p, 64, StepKernel::kSplitMoments, 4, 512, 1));
    CHECK(p.moments_first && ReportedStepKernel(p.kernel) == StepKernel::kSplit);
    CHECK(p.lds == 74496 && p.grid(64) == 256);
    StepOverrides o;
    o.no_moments_first = true;
    p = PlanRigidStep(f, o, Resident);
    CHECK(Shape(p, 64, StepKernel::kSplit, 4, 512, 1) && !p.moments_first);
  }
  CHECK(RegionAllowsMomentsFirst(false, false, false, 1));
  const bool off[4] = {RegionAllowsMomentsFirst(true, false, false, 1), RegionAllowsMomentsFirst(false, true, false, 1),
                       RegionAllowsMomentsFirst(false, false, true, 1), RegionAllowsMomentsFirst(false, false, false, 0)};
  for (bool allowed : off) {
    CHECK(!allowed);
    RigidStepFacts f = Region(64);
    f.regions_allow_moments_first = allowed;
    const RigidStepPlan p = PlanRigidStep(f, None(), Resident);
    CHECK(Shape(p, 64, StepKernel::kSplit, 4, 512, 1) && !p.moments_first);
  }
  RigidStepFacts f = Region(64);
  f.n_update_iterations = 0;  // no Newton step that could go first
  CHECK(PlanRigidStep(f, None(), Resident).kernel == StepKernel::kSplit);
}

static void Forced() {
  StepOverrides o;
  o.no_split = true;
  RigidStepPlan p = PlanRigidStep(Region(64), o, Resident);
  CHECK(Shape(p, 64, StepKernel::kPlain, 1, 512, 1) && p.lds == 4096 + 32768 * 4 && p.grid(64) == 64 && !p.moments_first);
  o.threads = Set(256);
  p = PlanRigidStep(Region(64), o, Resident);
  CHECK(Shape(p, 64, StepKernel::kPlain, 1, 256, 0) && p.lds == 74496);
  o = None();
  o.threads = Set(128);  // no multiple of the 256 split lanes
  p = PlanRigidStep(Region(64), o, Resident);
  CHECK(Shape(p, 64, StepKernel::kPlain, 1, 128, 0));
  o.threads = Set(256);  // two workgroups of 256 threads per CU: 64 x 8 fit 256 CUs
  p = PlanRigidStep(Region(64), o, Resident);
  CHECK(Shape(p, 64, StepKernel::kSplitMoments, 8, 256, 1));
  o = None();
  o.no_fused_histogram = true;
  p = PlanRigidStep(Region(64), o, Resident);
  CHECK(Shape(p, 64, StepKernel::kSplitMoments, 4, 512, 0));
  RigidStepFacts f = Region(64);
  f.n_corr_iterations = 64;  // the exchange's tags count searches in six bits
  CHECK(Shape(PlanRigidStep(f, None(), Resident), 64, StepKernel::kPlain, 1, 512, 1));
  f = Region(64);
  f.split_possible = false;
  CHECK(Shape(PlanRigidStep(f, None(), Resident), 64, StepKernel::kPlain, 1, 512, 1));
}

static void Parts() {
  RigidStepPlan p = PlanRigidStep(RegionDepth(21), None(), Resident);
  CHECK(Shape(p, 21, StepKernel::kSplitPair, 8, 512, 1) && p.grid(21) == 24 * 8 && !p.moments_first);
  StepOverrides o;
  o.no_pair = true;
  p = PlanRigidStep(RegionDepth(21), o, Resident);
  CHECK(Shape(p, 21, StepKernel::kSplit, 8, 512, 1) && !p.moments_first);
  CHECK(PlanRigidStep(Region(1), None(), Resident).parts == 8);
  o = None();
  o.split_parts = Set(16);
  CHECK(PlanRigidStep(Region(1), o, Resident).parts == 16);
  o.split_parts = Set(2);
  CHECK(PlanRigidStep(Region(1), o, Resident).parts == 2);
  o.split_parts = Set(0);  // ("" and garbage read as 0: no part count is small enough)
  CHECK(Shape(PlanRigidStep(Region(1), o, Resident), 1, StepKernel::kPlain, 1, 512, 1));
  RigidStepFacts f = Region(1);
  f.split_parts_override = 4;  // m3t_hip_set_object_split(ctx, 4)
  CHECK(PlanRigidStep(f, None(), Resident).parts == 4);
  f.split_parts_override = 16;
  CHECK(PlanRigidStep(f, None(), Resident).parts == 16);
  o.split_parts = Set(2);  // the variable wins
  CHECK(PlanRigidStep(f, o, Resident).parts == 2);
  f = Region(1);
  f.split_enabled = false;  // m3t_hip_set_object_split(ctx, 0)
  CHECK(Shape(PlanRigidStep(f, None(), Resident), 1, StepKernel::kPlain, 1, 512, 1));
  // padded_n * p must not exceed the CUs: 64 x 8 > 256, 64 x 4 = 256; one CU less and only two parts fit
  auto one = [](int) { return 1; };
  CHECK(SplitParts(64, 200, 8, 256, one) == 4);
  CHECK(SplitParts(64, 200, 8, 255, one) == 2);
  CHECK(SplitParts(64, 200, 8, 127, one) == 0);
  CHECK(SplitParts(8, 200, 16, 256, [](int) { return 2; }) == 16);
  CHECK(PlanRigidStep(Region(57), None(), Resident).parts == 4);   // padded to 64
  CHECK(PlanRigidStep(Region(65), None(), Resident).parts == 2);   // padded to 72: 72 x 4 > 256
  CHECK(PlanRigidStep(Region(129), None(), Resident).parts == 0);  // padded to 136: 136 x 2 > 256
  // a part's elements must fit its share of the 256 lanes
  CHECK(SplitParts(8, 256, 16, 256, one) == 16);
  CHECK(SplitParts(8, 257, 16, 256, one) == 0);
  f = RegionDepth(1);
  f.np_max = 300;
  CHECK(Shape(PlanRigidStep(f, None(), Resident), 1, StepKernel::kLdsPair, 1, 512, 1));
  f.has_depth = false;  // (the points of a batch without depth modalities do not count)
  CHECK(PlanRigidStep(f, None(), Resident).parts == 8);
  // the runtime's answer: nothing resident, no split; a negative answer ends the search at once
  CHECK(SplitParts(8, 200, 8, 256, [](int) { return 0; }) == 0);
  CHECK(Shape(PlanRigidStep(Region(64), None(), NoneResident), 64, StepKernel::kPlain, 1, 512, 1));
  int calls = 0;
  CHECK(SplitParts(8, 200, 16, 256, [&calls](int) { ++calls; return -1; }) == 0 && calls == 1);
  // parts the grid cannot hold are never asked about
  g_queries = 0;
  CHECK(PlanRigidStep(Region(64), None(), Resident).parts == 4 && g_queries == 1);
  // the render-fed step's limit of 16, without a fused histogram
  size_t lds = 0;
  CHECK(RigidSplitParts(Region(1), None(), StepKernel::kSplitRender, 512, false, 16, Resident, &lds) == 16 && lds == 74496);
  CHECK(RigidSplitParts(Region(64), None(), StepKernel::kSplitRender, 512, false, 16, Resident, &lds) == 4);
  // a part's LDS: the working set, or its share of the fused histogram's count table where that is larger
  o = None();
  o.split_parts = Set(2);
  CHECK(PlanRigidStep(Region(64), o, Resident).lds == 74496);
  f = Region(64);
  f.total_floats = 10000;
  CHECK(PlanRigidStep(f, o, Resident).lds == 4096 + 32768 * 4 / 2);
}

static void Compact() {
  RigidStepPlan p = PlanRigidStep(RegionDepth(512), None(), Resident);
  CHECK(Shape(p, 512, StepKernel::kCompactWide, 1, 512, 1) && p.compact_wide && !p.compact_table && p.lds == 47 * 1024);
  StepOverrides o;
  o.compact_wide = Set(0);
  p = PlanRigidStep(RegionDepth(512), o, Resident);
  CHECK(Shape(p, 512, StepKernel::kCompact, 1, 256, 1) && !p.compact_wide);
  o = None();
  o.compact = Set(0);
  p = PlanRigidStep(RegionDepth(512), o, Resident);
  CHECK(Shape(p, 512, StepKernel::kLdsPair, 1, 512, 1) && p.lds == size_t(18624 + 8192) * 4);
  o.no_pair = true;
  CHECK(Shape(PlanRigidStep(RegionDepth(512), o, Resident), 512, StepKernel::kLds, 1, 512, 1));
  // from more objects than CUs on; M3T_HIP_COMPACT=1: whenever possible
  o = None();
  o.no_split = true;
  CHECK(PlanRigidStep(RegionDepth(256), o, Resident).kernel == StepKernel::kLdsPair);
  CHECK(PlanRigidStep(RegionDepth(257), o, Resident).kernel == StepKernel::kCompactWide);
  o.compact = Set(1);
  CHECK(Shape(PlanRigidStep(RegionDepth(3), o, Resident), 3, StepKernel::kCompactWide, 1, 512, 1));
  CHECK(PlanRigidStep(RegionDepth(3), o, Resident).grid(3) == 3);
  RigidStepFacts f = RegionDepth(512);
  f.compact_possible = false;
  CHECK(PlanRigidStep(f, o, Resident).kernel == StepKernel::kLdsPair);
  f = RegionDepth(512);
  f.fused_mode = 2;  // line / point state requested: the compact kernels do not write it
  CHECK(PlanRigidStep(f, None(), Resident).kernel == StepKernel::kLdsPair);
  // the wide gap 5/2 CUs < n <= 3 CUs
  CHECK(PlanRigidStep(RegionDepth(640), None(), Resident).kernel == StepKernel::kCompactWide);
  CHECK(Shape(PlanRigidStep(RegionDepth(641), None(), Resident), 641, StepKernel::kCompact, 1, 256, 1));
  CHECK(Shape(PlanRigidStep(RegionDepth(768), None(), Resident), 768, StepKernel::kCompact, 1, 256, 1));
  CHECK(PlanRigidStep(RegionDepth(769), None(), Resident).kernel == StepKernel::kCompactWide);
  o = None();
  o.compact_wide = Set(1);
  CHECK(PlanRigidStep(RegionDepth(700), o, Resident).kernel == StepKernel::kCompactWide);
  // the LDS pair table and its gap 3 CUs < n <= 4 CUs
  p = PlanRigidStep(Region(768), None(), Resident);
  CHECK(Shape(p, 768, StepKernel::kCompactTable, 1, 256, 0) && p.compact_table && p.lds == 52 * 1024);
  CHECK(Shape(PlanRigidStep(Region(769), None(), Resident), 769, StepKernel::kCompact, 1, 256, 0));
  CHECK(PlanRigidStep(Region(1024), None(), Resident).kernel == StepKernel::kCompact);
  CHECK(PlanRigidStep(Region(1025), None(), Resident).kernel == StepKernel::kCompactTable);
  CHECK(PlanRigidStep(Region(4096), None(), Resident).kernel == StepKernel::kCompactTable);
  f = Region(512);
  f.table_overflow = 1024 / 2;
  CHECK(PlanRigidStep(f, None(), Resident).kernel == StepKernel::kCompactTable);
  f.table_overflow = 1024 / 2 + 1;
  p = PlanRigidStep(f, None(), Resident);
  CHECK(p.kernel == StepKernel::kCompact && !p.compact_table && p.lds == 47 * 1024);
  o = None();
  o.compact_table = Set(1);  // (forces nothing)
  CHECK(PlanRigidStep(f, o, Resident).kernel == StepKernel::kCompact);
  CHECK(PlanRigidStep(Region(1024), o, Resident).kernel == StepKernel::kCompact);
  CHECK(PlanRigidStep(Region(512), o, Resident).kernel == StepKernel::kCompactTable);
  o.compact_table = Set(0);
  CHECK(PlanRigidStep(Region(512), o, Resident).kernel == StepKernel::kCompact);
  f = Region(512);
  f.lds_compact_table = 0;
  CHECK(PlanRigidStep(f, None(), Resident).kernel == StepKernel::kCompact);
  f = Region(512);
  f.compact_fuses_histogram = true;  // (<= 16 bins)
  CHECK(Shape(PlanRigidStep(f, None(), Resident), 512, StepKernel::kCompactTable, 1, 256, 1));
  // M3T_HIP_THREADS keeps the compact kernels out, whatever else is set
  o = None();
  o.threads = Set(512);
  CHECK(Shape(PlanRigidStep(Region(768), o, Resident), 768, StepKernel::kPlain, 1, 512, 1));
  o.compact = Set(1);
  CHECK(Shape(PlanRigidStep(RegionDepth(512), o, Resident), 512, StepKernel::kLdsPair, 1, 512, 1));
}

static void RoiAndThreads() {
  // behind rectangles only the guard kernels, never pair, moments, table or wide
  RigidStepFacts f = Region(64);
  f.roi_frames = true;
  RigidStepPlan p = PlanRigidStep(f, None(), Resident);
  CHECK(Shape(p, 64, StepKernel::kSplitGuard, 4, 512, 1) && !p.moments_first);
  f = RegionDepth(21);
  f.roi_frames = true;
  CHECK(Shape(PlanRigidStep(f, None(), Resident), 21, StepKernel::kSplitGuard, 8, 512, 1));
  StepOverrides o;
  o.no_split = true;
  CHECK(Shape(PlanRigidStep(f, o, Resident), 21, StepKernel::kLdsGuard, 1, 512, 1));
  f = Region(64);
  f.roi_frames = true;
  CHECK(Shape(PlanRigidStep(f, o, Resident), 64, StepKernel::kGuard, 1, 512, 1));
  f = Region(768);
  f.roi_frames = true;
  p = PlanRigidStep(f, None(), Resident);
  CHECK(Shape(p, 768, StepKernel::kCompactGuard, 1, 256, 0) && !p.compact_table && !p.compact_wide && p.lds == 47 * 1024);
  f = RegionDepth(512);
  f.roi_frames = true;
  p = PlanRigidStep(f, None(), Resident);
  CHECK(Shape(p, 512, StepKernel::kCompactGuard, 1, 256, 1) && !p.compact_table && !p.compact_wide);
  o = None();
  o.compact_wide = Set(1);
  CHECK(Shape(PlanRigidStep(f, o, Resident), 512, StepKernel::kCompactGuard, 1, 256, 1));
  // 256 threads from two objects per CU on, if two working sets fit the 160 KB of a CU
  for (int cus : {256, 100}) {
    f = Region(2 * cus - 1);
    f.compute_cus = cus;
    f.compact_possible = false;
    f.lds_track = 80 * 1024;
    CHECK(Shape(PlanRigidStep(f, None(), Resident), f.n, StepKernel::kPlain, 1, 512, 1));
    f.n = 2 * cus;
    CHECK(Shape(PlanRigidStep(f, None(), Resident), f.n, StepKernel::kPlain, 1, 256, 0));
    f.lds_track = 80 * 1024 - 4;
    CHECK(Shape(PlanRigidStep(f, None(), Resident), f.n, StepKernel::kPlain, 1, 256, 0));
    f.lds_track = 80 * 1024 + 4;
    CHECK(Shape(PlanRigidStep(f, None(), Resident), f.n, StepKernel::kPlain, 1, 512, 1));
  }
}

static void Overrides() {
  const char* names[] = {"M3T_HIP_THREADS", "M3T_HIP_NO_PAIR", "M3T_HIP_NO_MOMENTS_FIRST", "M3T_HIP_NO_FUSED_HISTOGRAM",
                         "M3T_HIP_NO_SPLIT", "M3T_HIP_SPLIT_PARTS", "M3T_HIP_COMPACT", "M3T_HIP_COMPACT_TABLE",
                         "M3T_HIP_COMPACT_WIDE", "M3T_HIP_NO_SEARCH_FUSION", "M3T_HIP_NO_TREE_SPLIT", "M3T_HIP_TREE_PARTS",
                         "M3T_HIP_NO_TREE_FUSION", "M3T_HIP_NO_TREE_SEGMENTS"};
  for (const char* n : names) unsetenv(n);
  StepOverrides o = ReadStepOverrides();
  CHECK(!o.threads.set && !o.no_pair && !o.no_moments_first && !o.no_fused_histogram && !o.no_split && !o.split_parts.set &&
        !o.compact.set && !o.compact_table.set && !o.compact_wide.set && !o.no_search_fusion && !o.no_tree_split &&
        !o.tree_parts.set && !o.no_tree_fusion && !o.no_tree_segments);
  // flags: presence alone, "" and "0" included; numbers: atoi, "" and garbage 0
  for (const char* text : {"", "0", "1"}) {
    for (const char* n : names) setenv(n, text, 1);
    o = ReadStepOverrides();
    CHECK(o.no_pair && o.no_moments_first && o.no_fused_histogram && o.no_split && o.no_search_fusion && o.no_tree_split &&
          o.no_tree_fusion && o.no_tree_segments);
    const int v = std::atoi(text);
    CHECK(o.threads.set && o.split_parts.set && o.compact.set && o.compact_table.set && o.compact_wide.set && o.tree_parts.set);
    CHECK(o.threads.value == v && o.split_parts.value == v && o.compact.value == v && o.compact_table.value == v &&
          o.compact_wide.value == v && o.tree_parts.value == v);
  }
  for (const char* n : names) unsetenv(n);
  setenv("M3T_HIP_THREADS", "256", 1);
  setenv("M3T_HIP_SPLIT_PARTS", "sixteen", 1);
  setenv("M3T_HIP_COMPACT", "", 1);
  o = ReadStepOverrides();
  CHECK(o.threads.set && o.threads.value == 256 && o.split_parts.set && o.split_parts.value == 0);
  CHECK(o.compact.set && o.compact.value == 0 && !o.no_split && !o.compact_wide.set);
  // "set but empty" M3T_HIP_COMPACT means never, like 0
  CHECK(PlanRigidStep(RegionDepth(512), o, Resident).kernel == StepKernel::kLdsPair);
  for (const char* n : names) unsetenv(n);
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--names") == 0) {
    for (int k = 0; k < int(StepKernel::kCount); ++k) std::printf("%s\n", StepKernelName(StepKernel(k)));
    return 0;
  }
  Headline();
  Forced();
  Parts();
  Compact();
  RoiAndThreads();
  Overrides();
  CHECK(IsTreeStepKernel(StepKernel::kTree) && IsTreeStepKernel(StepKernel::kTreeSplit) &&
        IsTreeStepKernel(StepKernel::kTreeSegmentConstrained) && !IsTreeStepKernel(StepKernel::kSplitRender) &&
        !IsTreeStepKernel(StepKernel::kNone) && !IsTreeStepKernel(StepKernel::kCompactGuard));
  std::printf("checks %d errors %d\n", g_checks, g_errors);
  return g_errors ? 1 : 0;
}
