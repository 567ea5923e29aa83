// m3t_step_plan.h -- which kernel m3t_hip_execute_tracking_step launches, with how many threads, parts and bytes of
// LDS: the decision apart from the launches.  Plain C++17, no HIP header, no context: the library copies what the
// decision reads into RigidStepFacts and passes the occupancy query as a callable; tests/cpp/step_plan_check.cpp runs
// the same code on the host with a stub in its place.  Every measured crossover of the step lives here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>

namespace m3t_step {

// (m3t_device.h has the same figures as M3T_BLOCK_THREADS, ...; m3t_hip_api.hip asserts that they agree)
constexpr int kBlockThreads = 512;
constexpr int kCompactThreads = 256;
constexpr int kSplitLanes = 256;  // workgroups per object x padded elements per part
constexpr int kSplitMaxParts = 16;
constexpr size_t kMiscBytes = 1024 * 4;
constexpr size_t kCuLdsBytes = size_t(160) * 1024;

enum class StepKernel {
  kNone,  // one launch per sub-step
  kPlain, kLds, kPair, kLdsPair, kGuard, kLdsGuard,
  kSplit, kSplitPair, kSplitMoments, kSplitGuard, kSplitRender,
  kCompact, kCompactTable, kCompactWide, kCompactGuard,
  kTree, kTreeConstrained, kTreeSplit, kTreeSegment, kTreeSegmentConstrained,
  kCount
};

inline const char* StepKernelName(StepKernel k) {
  switch (k) {
    case StepKernel::kNone: return "";
    case StepKernel::kPlain: return "tracking_step_kernel";
    case StepKernel::kLds: return "tracking_step_lds_kernel";
    case StepKernel::kPair: return "tracking_step_pair_kernel";
    case StepKernel::kLdsPair: return "tracking_step_lds_pair_kernel";
    case StepKernel::kGuard: return "tracking_step_guard_kernel";
    case StepKernel::kLdsGuard: return "tracking_step_lds_guard_kernel";
    case StepKernel::kSplit: return "tracking_step_split_kernel";
    case StepKernel::kSplitPair: return "tracking_step_split_pair_kernel";
    case StepKernel::kSplitMoments: return "tracking_step_split_moments_kernel";
    case StepKernel::kSplitGuard: return "tracking_step_split_guard_kernel";
    case StepKernel::kSplitRender: return "tracking_step_split_render_kernel";
    case StepKernel::kCompact: return "tracking_step_compact_kernel";
    case StepKernel::kCompactTable: return "tracking_step_compact_table_kernel";
    case StepKernel::kCompactWide: return "tracking_step_compact_wide_kernel";
    case StepKernel::kCompactGuard: return "tracking_step_compact_guard_kernel";
    case StepKernel::kTree: return "tracking_step_tree_kernel";
    case StepKernel::kTreeConstrained: return "tracking_step_tree_constrained_kernel";
    case StepKernel::kTreeSplit: return "tracking_step_tree_split_kernel";
    case StepKernel::kTreeSegment: return "tracking_step_tree_segment_kernel";
    case StepKernel::kTreeSegmentConstrained: return "tracking_step_tree_segment_constrained_kernel";
    case StepKernel::kCount: break;
  }
  return "";
}
// what m3t_hip_get_step_kernel reports: the moments-first instantiation goes by the split kernel's name (only
// m3t_hip_get_step_variant tells them apart)
inline StepKernel ReportedStepKernel(StepKernel k) { return k == StepKernel::kSplitMoments ? StepKernel::kSplit : k; }
inline bool IsTreeStepKernel(StepKernel k) { return k >= StepKernel::kTree && k <= StepKernel::kTreeSegmentConstrained; }

// ---- developer overrides -------------------------------------------------------------------------------------------
// M3T_HIP_* environment variables of the step path, read once at the top of every step (a variable changed between
// two steps of one context takes effect in the next one).  Flags count when the variable exists, whatever it holds;
// numbers are atoi of its text ("" and garbage: 0).
struct EnvNumber {
  bool set = false;
  int value = 0;
};
struct StepOverrides {
  EnvNumber threads;            // M3T_HIP_THREADS: workgroup size of the one-launch rigid step; keeps the compact kernels out
  bool no_pair = false;         // M3T_HIP_NO_PAIR
  bool no_moments_first = false;    // M3T_HIP_NO_MOMENTS_FIRST
  bool no_fused_histogram = false;  // M3T_HIP_NO_FUSED_HISTOGRAM
  bool no_split = false;        // M3T_HIP_NO_SPLIT
  EnvNumber split_parts;        // M3T_HIP_SPLIT_PARTS: the largest part count tried
  EnvNumber compact;            // M3T_HIP_COMPACT=0 / 1: never / whenever possible
  EnvNumber compact_table;      // M3T_HIP_COMPACT_TABLE=0: never (1 forces nothing)
  EnvNumber compact_wide;       // M3T_HIP_COMPACT_WIDE=0 / 1
  bool no_search_fusion = false;  // M3T_HIP_NO_SEARCH_FUSION
  bool no_tree_split = false;     // M3T_HIP_NO_TREE_SPLIT
  EnvNumber tree_parts;           // M3T_HIP_TREE_PARTS
  bool no_tree_fusion = false;    // M3T_HIP_NO_TREE_FUSION
  bool no_tree_segments = false;  // M3T_HIP_NO_TREE_SEGMENTS
};
inline StepOverrides ReadStepOverrides() {
  auto flag = [](const char* name) { return std::getenv(name) != nullptr; };
  auto number = [](const char* name) {
    EnvNumber v;
    if (const char* e = std::getenv(name)) {
      v.set = true;
      v.value = std::atoi(e);
    }
    return v;
  };
  StepOverrides o;
  o.threads = number("M3T_HIP_THREADS");
  o.no_pair = flag("M3T_HIP_NO_PAIR");
  o.no_moments_first = flag("M3T_HIP_NO_MOMENTS_FIRST");
  o.no_fused_histogram = flag("M3T_HIP_NO_FUSED_HISTOGRAM");
  o.no_split = flag("M3T_HIP_NO_SPLIT");
  o.split_parts = number("M3T_HIP_SPLIT_PARTS");
  o.compact = number("M3T_HIP_COMPACT");
  o.compact_table = number("M3T_HIP_COMPACT_TABLE");
  o.compact_wide = number("M3T_HIP_COMPACT_WIDE");
  o.no_search_fusion = flag("M3T_HIP_NO_SEARCH_FUSION");
  o.no_tree_split = flag("M3T_HIP_NO_TREE_SPLIT");
  o.tree_parts = number("M3T_HIP_TREE_PARTS");
  o.no_tree_fusion = flag("M3T_HIP_NO_TREE_FUSION");
  o.no_tree_segments = flag("M3T_HIP_NO_TREE_SEGMENTS");
  return o;
}

// ---- part counts ---------------------------------------------------------------------------------------------------
// How many workgroups per object / tracked link (0: none): the largest power of two <= limit whose parts' elements fit
// their share of the 256 collecting lanes (parts x padded elements per part = 256, split_exchange_state) and whose grid
// -- blocks_per_part x parts workgroups -- is resident all at once, which the in-kernel exchange needs.
// resident_per_cu(p): workgroups of that launch a CU keeps, the caller's own caps applied; < 0: stop looking.
template <class ResidentPerCu>
int SplitParts(int blocks_per_part, int elements, int limit, int compute_cus, ResidentPerCu resident_per_cu) {
  for (int p = kSplitMaxParts; p >= 2; p >>= 1) {
    if (p > limit) continue;
    if ((elements + p - 1) / p > kSplitLanes / p) continue;  // a part's elements fit its share of the lanes
    const int resident = resident_per_cu(p);
    if (resident < 0) break;
    if (resident < 1 || blocks_per_part * p > compute_cus * resident) continue;
    return p;
  }
  return 0;
}

// ---- the one-launch step of rigid objects --------------------------------------------------------------------------
struct RigidStepFacts {
  int n = 0;            // objects (optimizers)
  int compute_cus = 0;  // CUs the tracking launches may count on
  size_t lds_track = 0, lds_hist = 0, lds_compact = 0, lds_compact_table = 0;  // bytes; lds_compact_table 0: not available
  int table_cap = 0;    // mixed bins the LDS pair table holds
  unsigned table_overflow = 0;  // the mapped overflow word as read in front of this step (0: no word yet)
  int off_hist = -1;    // layout.off_hist: >= 0 = the pair table is staged in LDS (tracking_step_lds_kernel)
  int total_floats = 0, nl = 0, np_max = 0;
  bool has_region = false, has_depth = false;
  bool regions_allow_moments_first = false;  // RegionAllowsMomentsFirst of every region modality
  int n_corr_iterations = 0, n_update_iterations = 0, fused_mode = 1;
  bool fuse_histogram_possible = false, split_possible = false, split_enabled = true;
  int split_parts_override = 0;  // m3t_hip_set_object_split(ctx, n > 1)
  bool compact_possible = false, compact_fuses_histogram = false;
  bool roi_frames = false;  // the step reads a slot that holds a rectangle only: the guarded kernels
};
struct RigidStepPlan {
  StepKernel kernel = StepKernel::kNone;
  int threads = 0, parts = 0;  // parts 0: one workgroup per object
  size_t lds = 0;              // dynamic LDS bytes
  bool histogram_fused = false, moments_first = false, compact_table = false, compact_wide = false;
  bool split() const { return parts >= 2; }
  int grid(int n) const { return split() ? (n + 7) / 8 * 8 * parts : n; }
};

// the first Newton step after a search reads no distribution row and the search has no occlusion vote to defer
inline bool RegionAllowsMomentsFirst(bool measure_occlusions, bool model_occlusions, bool use_region_checking,
                                     int n_global_iterations) {
  return !(measure_occlusions || model_occlusions || use_region_checking || n_global_iterations < 1);
}

// tracking_step_split_kernel / _split_render_kernel: how many workgroups per object (0: none) for a batch of f.n.
// resident(kernel, threads, lds): workgroups of that shape a CU keeps resident according to the runtime (0: unknown).
// (default_limit: 8 for the one-launch step -- 16 was not faster there in round 2; 16 for the per-search launches of
// renderer-fed steps, measured 0.643 -> 0.635 ms for one object)
template <class Resident>
int RigidSplitParts(const RigidStepFacts& f, const StepOverrides& o, StepKernel kernel, int threads,
                    bool want_fused_histogram, int default_limit, Resident resident, size_t* lds_out) {
  const size_t lds_tracking = size_t(f.off_hist >= 0 ? f.off_hist : f.total_floats) * 4;
  int limit = f.split_parts_override > 1 ? f.split_parts_override : default_limit;
  if (o.split_parts.set) limit = o.split_parts.value;
  const int elements = std::max(f.nl, f.has_depth ? f.np_max : 1);
  const int padded = (f.n + 7) / 8 * 8;  // grid blocks / p: every XCD gets the blocks of the fullest one
  return SplitParts(padded, elements, limit, f.compute_cus, [&](int p) {
    // (each workgroup counts its share of the histogram bins: that share of the count table; the pair table is
    // read from L2, never staged)
    const size_t lds = want_fused_histogram ? std::max(lds_tracking, kMiscBytes + (f.lds_hist - kMiscBytes) / p) : lds_tracking;
    // 256-thread workgroups (developer override): two are resident per CU if their LDS fits twice
    const int per_cu = (threads == kSplitLanes && lds * 2 <= kCuLdsBytes) ? 2 : 1;
    if (padded * p > f.compute_cus * per_cu) return 0;
    // the exchange needs every workgroup of the grid resident at once: ask the runtime how many of these
    // workgroups (registers, LDS) a CU takes, instead of assuming the LDS arithmetic above is the only limit
    *lds_out = lds;
    // (the query is known to over-report by one block for SGPR-heavy kernels)
    return std::min(int(resident(kernel, threads, lds)), per_cu);
  });
}

template <class Resident>
RigidStepPlan PlanRigidStep(const RigidStepFacts& f, const StepOverrides& o, Resident resident) {
  RigidStepPlan plan;
  const bool roi_frames = f.roi_frames, lds_table = f.off_hist >= 0;
  // From two objects per CU on (and if two working sets fit the CU's LDS) the kernel runs with 256-thread
  // workgroups, two per CU: one object's serial solve overlaps the other's parallel phases and no register is
  // spilled (measured, pose-updates/s: 512 objects 1.11 M vs 0.87 M with 512 threads, 4096: 1.24 M vs 0.91 M;
  // 128-VGPR variants of the 512-thread kernel reached 1.03 M / 1.11 M)
  int threads = kBlockThreads;
  if (f.n >= 2 * f.compute_cus && f.lds_track * 2 <= kCuLdsBytes) threads = kBlockThreads / 2;
  if (o.threads.set) threads = o.threads.value;
  // Batches with region AND depth modalities: the _pair_ kernels (m3t_kernels.hip, PAIR: the two modalities' products
  // side by side, their sums on two waves).
  const bool pair = !roi_frames && f.has_region && f.has_depth && !o.no_pair;
  // Region-only batches whose first Newton step after a search reads no distribution row (n_global_iterations >= 1)
  // and whose searches have no occlusion vote to defer: the split kernel with the moments-first exchange
  // (m3t_kernels.hip, region_distribution_rows).  Every object of the launch must qualify; all others keep
  // tracking_step_split_kernel.
  const bool moments_first = !roi_frames && !pair && !f.has_depth && f.has_region && f.n_update_iterations >= 1 &&
                             !o.no_moments_first && f.regions_allow_moments_first;
  const StepKernel split_kernel = roi_frames ? StepKernel::kSplitGuard
                                             : (pair ? StepKernel::kSplitPair
                                                     : (moments_first ? StepKernel::kSplitMoments : StepKernel::kSplit));
  // One workgroup per CU: the histogram update (CalculateResults) runs at the end of the same launch, its
  // count table taking over the line buffers' LDS.  With two workgroups per CU that table (128 KB at 32 bins)
  // would not fit twice, so large batches keep the separate region_histogram_kernel.
  const bool want_fused_histogram = f.fuse_histogram_possible && !o.no_fused_histogram;
  plan.histogram_fused = want_fused_histogram && threads == kBlockThreads;
  plan.lds = plan.histogram_fused ? std::max(f.lds_track, f.lds_hist) : f.lds_track;
  // Batches that leave CUs idle: several workgroups per object, each on its own CU (all resident at once, which
  // their in-kernel exchange needs; a wait that runs out abandons the object's step, see CheckSplitExchange).
  size_t lds_split = 0;
  if (f.split_possible && f.split_enabled && threads % kSplitLanes == 0 && f.n_corr_iterations < 64 && !o.no_split)
    plan.parts = RigidSplitParts(f, o, split_kernel, threads, want_fused_histogram, 8, resident, &lds_split);
  const bool split = plan.parts >= 2;
  plan.moments_first = split && moments_first;
  // More objects than CUs: the compact kernel (<= 47 KB of LDS, <= 128 VGPRs per object: 3-4 workgroups per CU;
  // measured crossover on 256 CUs: 256 objects 0.249 vs 0.225 ms with one 512-thread workgroup per CU, 384 objects
  // 0.309 vs 0.426 ms).
  const bool compact_can = !split && f.compact_possible && f.fused_mode == 1;
  bool compact = compact_can && f.n > f.compute_cus;
  if (o.compact.set) compact = compact_can && o.compact.value != 0;
  if (o.threads.set) compact = false;
  // Region-only batches with >= 1024-bin histograms: the pair table compacted in LDS (round 6; 4096 objects 1.96 ->
  // 1.78 ms).  While the mixed bins of every object fit the table, that is; histograms that outgrow it by more than
  // half its size (the kernels report it through a mapped word) go back to the kernel that gathers from L2.
  // (Region + Depth batches keep the plain kernel: measured with the table, synth512 0.769 / 0.784 vs 0.778 ms -- their
  // 16-bin pair table is 32 KB and sits in the L1 / L2 anyway, and the depth scan is most of their step)
  bool compact_table = compact && !roi_frames && f.lds_compact_table > 0 && !f.has_depth;
  // (three workgroups per CU instead of four: a batch that is ONE round of the plain kernel but not of this one keeps
  // the plain kernel -- 1024 objects on 256 CUs: 0.556 vs 0.583 ms; 384: 0.314 / 0.290, 512: 0.325 / 0.298, 2048:
  // 1.041 / 0.935, 4096: 1.964 / 1.769)
  if (f.n > 3 * f.compute_cus && f.n <= 4 * f.compute_cus) compact_table = false;
  if (compact_table && f.table_overflow > unsigned(f.table_cap) / 2) compact_table = false;
  if (o.compact_table.set) compact_table = compact_table && o.compact_table.value != 0;
  // Batches with depth modalities: 512-thread workgroups, two per CU (round 6).  Their step is the depth scan -- sixteen
  // lanes per point, 200 points: 12.5 rounds of a 256-thread workgroup, half of that here --, the registers and the LDS
  // per object stay, 16 waves per CU instead of 12.  Measured (Region + Depth, YCB parameters, ms per step, 256 / 512
  // threads): 257 objects 0.732 / 0.577, 512: 0.790 / 0.635, 640: 0.970 / 0.949, 700: 0.986 / 1.058, 768: 0.996 / 1.083,
  // 900: 1.473 / 1.168, 1024: 1.567 / 1.216, 2048: 2.640 / 2.410, 4096: 5.097 / 4.736 -- the 256-thread kernel keeps the
  // batches that are ONE round of its three workgroups per CU but not of two.  Region-only batches: 384 / 512 objects
  // 0.314 / 0.295 and 0.324 / 0.306 ms, behind the LDS pair table's 0.286 / 0.292 -- not taken.
  bool compact_wide = compact && !roi_frames && !compact_table && f.has_depth &&
                      !(2 * f.n > 5 * f.compute_cus && f.n <= 3 * f.compute_cus);
  if (o.compact_wide.set) compact_wide = compact && !roi_frames && !compact_table && o.compact_wide.value != 0;
  plan.compact_table = compact_table;
  plan.compact_wide = compact_wide;
  if (split) {
    plan.kernel = split_kernel;
    plan.threads = threads;
    plan.lds = lds_split;
    plan.histogram_fused = want_fused_histogram;
  } else if (compact) {
    plan.kernel = roi_frames ? StepKernel::kCompactGuard
                             : (compact_table ? StepKernel::kCompactTable
                                              : (compact_wide ? StepKernel::kCompactWide : StepKernel::kCompact));
    plan.threads = compact_wide ? 2 * kCompactThreads : kCompactThreads;
    plan.lds = compact_table ? f.lds_compact_table : f.lds_compact;
    plan.histogram_fused = want_fused_histogram && f.compact_fuses_histogram;
  } else {
    plan.kernel = roi_frames ? (lds_table ? StepKernel::kLdsGuard : StepKernel::kGuard)
                             : (pair ? (lds_table ? StepKernel::kLdsPair : StepKernel::kPair)
                                     : (lds_table ? StepKernel::kLds : StepKernel::kPlain));
    plan.threads = threads;
  }
  return plan;
}

}  // namespace m3t_step
