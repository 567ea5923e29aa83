// m3t_hip_api.hip — host side of libm3t_hip.so: context, device-resident tables,
// .bin model parser and kernel launches behind the C-ABI of include/m3t_hip.h.
// Single translation unit together with the kernels (one hipcc invocation).

#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library is opened with dlopen when a structure spans GPUs

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/m3t_hip.h"
#include "m3t_device.h"
#include "m3t_host_resources.h"
#include "m3t_view_rows.h"
#include "m3t_step_plan.h"
#include "m3t_render_plan.h"
#include "m3t_texture_plan.h"
#include "m3t_call_args.h"
#include "m3t_ingest_plan.h"
#include "m3t_kernels.hip"
#include "m3t_judge.hip"
#include "m3t_opt.hip"
#include "m3t_texture.hip"
#include "m3t_features.hip"
#include "m3t_compact.hip"
#include "m3t_render.hip"
#include "m3t_modelgen.hip"
#include "m3t_links.hip"
#include "m3t_structures.hip"
#include "m3t_ingest.hip"
// the *_list_kernel forms of the texture kernels, behind every other kernel: no existing kernel moves in the code object
#define M3T_TEXTURE_LIST_KERNELS
#include "m3t_texture.hip"
#include "m3t_features.hip"
#undef M3T_TEXTURE_LIST_KERNELS
// the matcher of L2-norm descriptors, behind those again
#include "m3t_texture_l2.hip"
// the tiled form of the Hamming matcher, behind that
#include "m3t_texture_tiled.hip"

static_assert(m3t_step::kBlockThreads == M3T_BLOCK_THREADS && m3t_step::kCompactThreads == M3T_COMPACT_THREADS &&
                  m3t_step::kSplitLanes == M3T_SPLIT_LANES && m3t_step::kSplitMaxParts == M3T_SPLIT_MAX_PARTS &&
                  m3t_step::kMiscBytes == M3T_MISC_FLOATS * 4,
              "m3t_step_plan.h and m3t_device.h disagree");
static_assert(m3t_render::kBlockThreads == M3T_BLOCK_THREADS, "m3t_render_plan.h and m3t_device.h disagree");
static_assert(m3t_texture::kMatchThreads == M3T_TEXTURE_MATCH_THREADS && m3t_texture::kQueryTile == M3T_TEXTURE_QUERY_TILE &&
                  m3t_texture::kMaxFeatures == M3T_TEXTURE_MAX_FEATURES && m3t_texture::kQueryTiles == kTiledQueryTiles &&
                  m3t_texture::kMaxKeyframes == M3T_TEXTURE_MAX_KEYFRAMES && m3t_texture::kBestBytes == 3 * sizeof(uint32_t),
              "m3t_texture_plan.h and m3t_texture.h disagree");

namespace {

thread_local std::string g_create_error;

using m3t_res::CreateMaskedStream;
using m3t_res::DevMem;
using m3t_res::Event;
using m3t_res::EventPair;
using m3t_res::HostBlock;
using m3t_res::kMapped;
using m3t_res::kPinned;
using m3t_res::Stream;
using m3t_res::UploadTable;
// m3t_hip_reset_* / m3t_hip_judge_* / set_features: a call's arguments in mapped blocks, read in place by its launches
using MappedRing = m3t_res::HostRing<4, kMapped>;

struct Model {
  bool region = true;
  int n_views = 0, n_points = 0, point_floats = 0;
  float stride_depth_offset = 0.002f, max_radius_depth_offset = 0.05f, max_extent = 0.0f;
  DevMem points, orientations, extents;
  DevMem points8, orientations4;  // device-only compact copies of the hot fields
  DevMem view_neighbors;          // [n_views][M3T_VIEW_ROW] float4 (closest_view_local), empty for tiny view sets
  std::vector<float> h_orientations;  // host copy: modalities whose models share their view table share the view search
  float box_min[3] = {0, 0, 0}, box_max[3] = {0, 0, 0};  // around the centres of all data points (ROI ingest, m3t_roi.h)
  float box_rho = 0.0f;  // ... which also lie in the ellipsoid of box_rho x the box's half extents (0: a flat box, not used)
};

struct Camera {
  bool is_depth = false;
  m3t_intrinsics intr{};
  float world2camera[16];
  float depth_scale = 0.0f;
  uint32_t pitch = 0;
  size_t frame_bytes = 0;
  int n_slots = 1, current = 0;
  std::vector<bool> has_image;
  std::vector<long> last_read_step;  // per slot: the last streaming step that read it (-1: none)
  std::vector<bool> slot_is_roi;     // per slot: only the trackers' rectangle of the frame was uploaded (m3t_ingest.hip)
  std::vector<Event> slot_copied;  // per slot: behind its last camera_upload_slot_async (m3t_hip_camera_slot_sync); lazily made
  DevMem ring;          // this camera's own frame ring, or empty when it lives in a shared slab
  int slab = -1, slab_index = 0;  // shared slab (m3t_hip_cameras_set_ring): [slot][camera of the group][frame]
  uint8_t* frames = nullptr;      // slot 0 of this camera
  size_t slot_stride = 0;         // bytes from one slot of this camera to the next
  uint8_t* frame(int slot) const { return frames + size_t(slot) * slot_stride; }
  void SetSlots(int n) {  // a new ring: no frames in it, no readers
    n_slots = n;
    current = 0;
    has_image.assign(size_t(n), false);
    last_read_step.assign(size_t(n), -1);
    slot_is_roi.assign(size_t(n), false);
  }
};
struct FrameSlab {  // the frame rings of a group of cameras of equal geometry in one allocation
  DevMem mem;
  std::vector<int> cameras;
  // per ring slot: behind the last batch upload / rectangle pull into it (m3t_hip_camera_slot_sync of any of its
  // cameras).  ONE event per batch-frame: an event per camera cost a 64-camera upload 0.3 ms of host time.
  std::vector<Event> slot_copied;
};

// Asynchronous ingest: frame copies run on streams of their own beside the tracking kernels.  The ledger decides
// (m3t_ingest_plan.h), the methods carry its decisions out; DESIGN.md section 1 ("Frame ingest") states the protocol.
struct Ingest {
  static constexpr int kCopyStreams = m3t_ingest::kCopyStreams;
  Stream copy_stream[kCopyStreams];
  Event copies_done[kCopyStreams], step_done[m3t_ingest::kStepEvents];
  m3t_ingest::Ledger ledger;
  std::vector<void*> registered;  // Register
  bool async() const { return ledger.async; }
  bool untracked() const { return ledger.untracked; }
  void LaunchedUntracked() { ledger.LaunchedUntracked(); }
  hipStream_t CopyStream(int cs) const { return copy_stream[cs].get(); }
  hipError_t Keep(const m3t_ingest::Ledger& before, hipError_t e) {  // a runtime call that fails leaves the ledger as it was
    if (e != hipSuccess) ledger = before;
    return e;
  }
  static hipError_t CreateStreams(int ingest_cus, int cus, Stream (&streams)[kCopyStreams]) {
    hipError_t e = CreateMaskedStream(ingest_cus, cus, &streams[0], true);
    for (int i = 1; i < kCopyStreams && e == hipSuccess; ++i) e = streams[i].Create(hipStreamNonBlocking);
    return e;
  }
  hipError_t EnsureStarted(int ingest_cus, int cus) {
    const m3t_ingest::Ledger before = ledger;
    if (!ledger.Start()) return hipSuccess;
    hipError_t e = CreateStreams(ingest_cus, cus, copy_stream);
    for (auto& ev : copies_done)
      if (e == hipSuccess) e = ev.Ensure(hipEventDisableTiming);
    for (auto& ev : step_done)
      if (e == hipSuccess) e = ev.Ensure(hipEventDisableTiming);
    return Keep(before, e);
  }
  // what a decision of the ledger asks for; cs: the copy stream that waits for a step event (-1: the host does)
  hipError_t Obey(const m3t_ingest::Wait& w, int cs, hipStream_t compute) const {
    if (w.kind == m3t_ingest::Wait::kComputeStream) return hipStreamSynchronize(compute);
    if (w.kind == m3t_ingest::Wait::kNothing) return hipSuccess;
    return cs < 0 ? hipEventSynchronize(step_done[w.event].get()) : hipStreamWaitEvent(copy_stream[cs].get(), step_done[w.event].get(), 0);
  }
  // a copy on copy stream cs overwrites a slot only behind the launches that read it last (step last_read) ...
  hipError_t OrderCopy(int cs, long last_read, hipStream_t compute) {
    const m3t_ingest::Ledger before = ledger;
    return Keep(before, Obey(ledger.OrderCopy(cs, last_read), cs, compute));
  }
  // ... and the host waits for those launches
  hipError_t WaitForReader(long last_read, hipStream_t compute) const { return Obey(ledger.WaitForReader(last_read), -1, compute); }
  // the "slot copied" event of a camera or a slab (made on first use) behind what copy stream cs holds for the slot
  hipError_t SlotCopied(std::vector<Event>* events, int n_slots, int slot, int cs) {
    if (events->size() < size_t(n_slots)) events->resize(size_t(n_slots));
    Event& copied = (*events)[slot];
    hipError_t e = copied.Ensure(hipEventDisableTiming);
    if (e == hipSuccess && (e = hipEventRecord(copied.get(), copy_stream[cs].get())) == hipSuccess) ledger.CopyEnqueued(cs);
    return e;
  }
  // frames enqueued on the copy streams so far become visible to everything launched on `compute` from here on
  hipError_t JoinPendingCopies(hipStream_t compute) {
    const m3t_ingest::Ledger before = ledger;
    hipError_t e = hipSuccess;
    for (unsigned k = 0, pending = ledger.TakePending(); k < kCopyStreams && e == hipSuccess; ++k)
      if ((pending >> k & 1u) && (e = hipEventRecord(copies_done[k].get(), copy_stream[k].get())) == hipSuccess)
        e = hipStreamWaitEvent(compute, copies_done[k].get(), 0);
    return Keep(before, e);
  }
  // Launches on `compute` read the current frames of the cameras listed (ids null: of all of them): a later asynchronous
  // upload into one of these slots waits for exactly them, not for the ones enqueued after them
  hipError_t MarkRead(hipStream_t compute, const std::vector<std::unique_ptr<Camera>>& cameras, const std::vector<int>* ids) {
    const m3t_ingest::Ledger before = ledger;
    const m3t_ingest::ReadMark mark = ledger.MarkRead();
    if (mark.event < 0) return hipSuccess;
    const hipError_t e = Keep(before, hipEventRecord(step_done[mark.event].get(), compute));
    for (size_t i = 0; e == hipSuccess && i < (ids ? ids->size() : cameras.size()); ++i) {
      Camera& c = *cameras[ids ? size_t((*ids)[i]) : i];
      c.last_read_step[c.current] = mark.step;
    }
    return e;
  }
  hipError_t SyncCopies() const {
    hipError_t e = hipSuccess;
    for (auto& cs : copy_stream)
      if (cs && e == hipSuccess) e = hipStreamSynchronize(cs.get());
    return e;
  }
  hipError_t Register(void* ptr, size_t bytes) {
    const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
    if (e == hipSuccess) registered.push_back(ptr);
    return e;
  }
  bool IsRegistered(void* ptr) const { return std::find(registered.begin(), registered.end(), ptr) != registered.end(); }
  hipError_t Unregister(void* ptr) {  // (behind every copy that may still read the buffer)
    hipError_t e = SyncCopies();
    if (e == hipSuccess && (e = hipHostUnregister(ptr)) == hipSuccess) registered.erase(std::find(registered.begin(), registered.end(), ptr));
    return e;
  }
  void ReplaceStreams(Stream (&streams)[kCopyStreams]) {  // (synchronised by the caller: nothing is pending)
    for (int i = 0; i < kCopyStreams; ++i) copy_stream[i] = std::move(streams[i]);
    (void)ledger.TakePending();
  }
  void UnregisterAll() {  // m3t_hip_destroy, behind SyncCopies
    for (void* p : registered) (void)hipHostUnregister(p);
    registered.clear();
  }
};

struct BodyGeometryH {  // body.h:46-60 on the device
  bool set = false;
  DevMem vertices, triangles;
  std::vector<float> h_vertices;  // host copies for model generation
  std::vector<int> h_triangles;
  int n_triangles = 0;
  float geometry2body[16];
  int culling = 1, body_id = 0, region_id = 0;
  float maximum_body_diameter = 0.0f;
};
struct RendererH {  // FocusedBasicDepthRenderer / FocusedSilhouetteRenderer
  bool silhouette = false;
  int geometry = -1, camera = -1, id_type = M3T_ID_TYPE_BODY, image_size = 200;
  float z_min = 0.02f, z_max = 10.0f;
  std::vector<int> referenced;
  DevMem depth, sil, packed, state;
  DevMem survivors, n_survivors;  // focused_setup_kernel -> focused_resolve_kernel (m3t_render.hip)
  int survivor_capacity = 0;
  bool rendered = false;
};
struct SharedHistogramsH {  // a ColorHistograms object used by several RegionModalities
  int n_bins = 16, bitshift = 4;
  float learning_rate_f = 0.2f, learning_rate_b = 0.2f;
  DevMem hist_f, hist_b, hist_norm, counts;
};
struct RegionMod {
  m3t_region_modality_params p{};
  int depth_renderer = -1, silhouette_renderer = -1;
  int shared_histograms = -1;
  int body, camera, depth_camera, model;
  DevMem hist_f, hist_b, hist_norm, occupancy, count_scratch, line_state, gh;
  RegionModDev dev{};
};
struct DepthMod {
  m3t_depth_modality_params p{};
  int depth_renderer = -1, silhouette_renderer = -1;
  int body, camera, model;
  DevMem point_state, gh;
  DepthModDev dev{};
};
struct TextureMod {  // TextureModality behind its feature detector (m3t_texture.hip)
  m3t_texture_modality_params p{};
  int body, camera, depth_camera, silhouette_renderer, depth_renderer = -1;
  DevMem features, keyframe_points, keyframe_descriptors, data_points, state, gh;
  MappedRing uploads;  // set_features: the caller's features cross through page-locked blocks taken in turn
  TextureModDev dev{};
  // the built-in detector (m3t_features.hip), when set_detector has named one: its parameters and its images
  bool builtin = false;
  m3t_texture_detector_params detector{};
  DevMem focused, scores, boxes, detector_header;
  // L2-norm descriptors (m3t_texture_l2.hip): descriptor_bytes / 4 floats a row, and the matcher's best-two scratch
  // (which a Hamming modality has too once its context has resolved to the tiled matcher, m3t_texture_tiled.hip)
  bool l2 = false;
  DevMem best;
};
enum ModalityKind { kRegionModality, kDepthModality, kTextureModality };
struct ModalityRef {
  ModalityKind kind;
  int index;
};
struct Link {
  int body = -1, parent = -1;
  std::vector<int> children, modalities;
  float body2joint[16], joint2parent[16], link2world[16];
  int free_directions[6] = {1, 1, 1, 1, 1, 1};
  int fixed_body2joint_pose = 1;
  bool simple = true;  // free 6-dof root link with identity joint poses and a body
  int optimizer = -1, local_index = -1;
};
struct ConstraintH {
  int link1, link2;
  float body12joint1[16], body22joint2[16];
  int directions[6];
};
struct SoftConstraintH {
  ConstraintH joint;
  float max_distance_rotation, max_distance_translation, standard_deviation_rotation, standard_deviation_translation;
};
struct Optimizer {
  int link;
  float tr, tt;
  std::vector<int> constraints, soft_constraints;
  std::vector<int> order;  // global link ids, depth first (parents before children)
  int dof = 0, n_rows = 0;
  size_t partial_offset = 0;
};

struct Judge {  // m3t_hip_judge_*: the evaluators' judgement of a list of bodies, rows of results in mapped host memory
  std::vector<int> body_ids;
  int n_rows_max = 0, n_rows = 0;
  float thr_t = 0.05f, thr_r = 5.0f * 3.14159265358979323846f / 180.0f;  // rbot_evaluator.h:192-193
  std::vector<int> n_vertices;
  std::vector<std::unique_ptr<DevMem>> vertices;  // per listed body: float4, padded to a multiple of 4
  DevMem d_bodies, d_parts, d_flags, d_partial;
  int n_parts = 0, queries_per_thread = 1;
  bool any_split = false;
  // m3t_hip_judge_set_add_only: the bodies judged as OPTEvaluator::CalculatePoseResults judges, by kernels of their own
  std::vector<char> add_only;                      // per listed body
  std::vector<std::array<float, 12>> geometry2body;  // per listed body, column-major 3 x 4
  DevMem d_add_bodies, d_add_parts, d_add_partial;
  int n_add_bodies = 0, n_add_parts = 0;
  bool any_add_split = false;
  HostBlock rows;               // mapped: [n_rows_max][n_bodies], written by the kernels in place
  std::vector<Event> row_done;  // per row: behind the launches of its call; made on first use
  MappedRing args;  // the ground-truth poses and the region-modality lists of a call, read in place by its launches
  // m3t_hip_judge_set_structures: the structures' groups of listed bodies and a second table of rows
  int n_structures = 0;
  DevMem d_structure_ints, d_structure_thresholds;  // [first group of each structure | first index of each group | indices]
  size_t structure_groups = 0;
  // m3t_hip_judge_set_reset_target: per listed body the body a reset writes (-1: the listed body itself);
  // m3t_hip_judge_set_reset_renderers: a resetting call may run start-modality renderers, decided on the device
  std::vector<int> targets;
  bool reset_renderers = false;
  HostBlock structure_rows;  // mapped: [n_rows_max][n_structures], written by the kernel in place
};

}  // namespace

struct m3t_hip_context {
  int device = 0;
  Stream compute;  // declared before every event and block used on it: destroyed behind them (m3t_hip_destroy)
  hipStream_t stream = nullptr;  // compute.get(), as the launches take it
  hipDeviceProp_t prop{};
  std::string error;
  std::vector<std::unique_ptr<Model>> region_models, depth_models;
  std::vector<std::unique_ptr<Camera>> cameras;
  std::vector<std::unique_ptr<FrameSlab>> slabs;
  std::vector<float> body_poses;  // host mirror [n][16] (valid when !poses_on_device_newer)
  std::vector<std::unique_ptr<RegionMod>> region_mods;
  std::vector<std::unique_ptr<DepthMod>> depth_mods;
  std::vector<std::unique_ptr<TextureMod>> texture_mods;
  std::vector<ModalityRef> modalities;
  std::vector<std::unique_ptr<SharedHistogramsH>> shared_histograms;
  DevMem d_shared_histograms;
  std::vector<std::unique_ptr<BodyGeometryH>> body_geometries;  // parallel to the bodies (may be shorter)
  std::vector<std::vector<int>> renderer_geometries;
  std::vector<std::unique_ptr<RendererH>> renderers;
  DevMem d_renderers, d_render_region, d_render_all;  // RendererDev table; which renderers to run when
  DevMem d_render_region_pairs, d_render_all_pairs;   // the same lists as {renderer, twin or -1} (LaunchRenderers)
  int n_render_region_pairs = 0, n_render_all_pairs = 0;
  int n_render_region = 0, n_render_all = 0;
  int lds_raster = -1;  // focused_resolve_kernel (z-buffer in LDS) usable on this device: -1 not tried yet
  int judge_render_always = -1;  // M3T_HIP_JUDGE_RENDER_ALWAYS (developer switch, tools/occlusion_judge_timing.py): -1 not read yet
  std::vector<Link> links;
  std::vector<ConstraintH> constraints;
  std::vector<SoftConstraintH> soft_constraints;
  std::vector<Optimizer> optimizers;
  bool tree_mode = false;          // any kinematic tree / constraint -> links_* kernels
  bool links_device_newer = false;  // joint poses on the device are ahead of the host mirror
  DevMem d_links, d_constraints, d_soft, d_treeopts, d_work, d_partial;
  DevMem d_link_sums, d_link_first;  // what a structure spread over processes exchanges (links_gather_kernel): [links][42], first link per structure
  DevMem d_link_sums_alt, d_links_alt;  // tracking_step_tree_segment_kernel: the second copies (sums, link table) that take turns
  DevMem d_poses_first;  // ... and the bodies' start poses for a frame of one Newton step
  bool tree_untracked_structure = false;  // some structure has no modality in this context (its bodies live on other ranks)
  size_t link_sums_count = 0;
  // tracking_step_tree_kernel: one workgroup per link that carries modalities
  DevMem d_treesteps, d_tracked_links, d_tree_exchange;
  int n_treesteps = 0;
  bool tree_fused_possible = false;
  bool tree_constrained = false;  // some structure has Constraint / SoftConstraint objects: tracking_step_tree_constrained_kernel
  size_t tree_block_floats = 0;  // LDS of the structure copy (link table, link sums, system, work arrays), largest structure
  unsigned tree_seq = 0;
  size_t partial_count = 0;
  size_t tree_lds = 0;  // bytes of LDS per structure for the link kernels, 0: work arrays in global memory
  bool partial_ready = false;
  // a kinematic structure spread over GPUs: this rank's RCCL communicator (m3t_hip_comm_init_rank) or the host's
  ncclComm_t comm = nullptr;
  long long allreduce_calls = 0;  // ncclAllReduce calls issued since the context was created (m3t_hip_comm_get_allreduce_count)
  bool comm_owned = false;
  // ... or the host's own transport in the collective's place (m3t_hip_comm_set_reduce_callback): MPI, gloo, threads
  m3t_hip_reduce_fn reduce_fn = nullptr;
  void* reduce_user = nullptr;
  bool Distributed() const { return comm != nullptr || reduce_fn != nullptr; }
  int n_corr_iterations = 5, n_update_iterations = 2;
  int fused_mode = 1;
  // device tables
  DevMem d_detectors;   // TextureDetectorDev of the texture modalities with a built-in detector
  // With an L2 texture modality in the context: the Hamming modalities' TextureModDev entries alone (what
  // texture_match_kernel is launched on) and the L2 modalities' TextureL2Dev table.  Without one, texture_match_kernel
  // takes d_texture as it always did.
  DevMem d_texture_hamming, d_texture_l2;
  int n_texture_hamming = 0, n_texture_l2 = 0, l2_keyframes_max = 0;
  size_t lds_texture_l2 = 0;
  // The Hamming matcher's form (m3t_texture_plan.h): the mode (the developer override M3T_HIP_TEXTURE_MATCH, looked at
  // once, when the context is made), the plan in effect, and the table of the Hamming modalities' scratch pointers in
  // the order of the table the matcher runs on.  The plan is made again by UploadTables whenever the tables changed.
  int texture_match_mode = m3t_texture::ReadMatchOverride(), hamming_keyframes_max = 0;
  bool texture_plan_stale = true;
  m3t_texture::MatchPlan texture_plan{};
  DevMem d_texture_best;
  int n_detectors = 0;
  DevMem d_cams, d_region, d_depth, d_texture, d_opts, d_poses, d_scratch_view;
  DevMem d_gh_sources, d_gh_all;  // m3t_hip_modalities_get_gradient_hessian
  int gh_sources_count = -1;
  bool tables_dirty = true, cams_dirty = true, slots_dirty = false, poses_dirty_host = true;
  const CameraDev* cams_active = nullptr;  // the camera table version the kernels read (UploadTables)
  size_t pose_capacity = 0;
  std::vector<RigidOptDev> opt_table;
  bool fused_possible = false;
  bool fused_per_search_possible = false;  // ... if it were not for renderer-fed branches: one launch per correspondence search
  bool fuse_histogram_possible = false;  // ... and the histogram update can ride in the same launch
  // several workgroups per object (tracking_step_split_kernel) for batches that leave most CUs idle
  bool split_possible = false;
  size_t tree_split_lds_attribute = 0;  // the dynamic LDS limit tracking_step_tree_split_kernel was given last
  bool split_enabled = true;  // m3t_hip_set_object_split
  std::map<std::tuple<const void*, int, size_t>, int> occupancy_cache;  // ResidentBlocks
  int ingest_cus = 0;   // m3t_hip_reserve_ingest_cus: CUs kept free of the tracking kernels for the ROI pull kernel
  int compute_cus = 0;  // what the tracking launches may count on (set with the device properties)
  size_t tree_lds_attribute = 0;  // dynamic LDS limit last set on the one-launch tree kernel ...
  const void* tree_lds_kernel = nullptr;  // ... and which of the two it was
  size_t tree_segment_lds_attribute = 0;  // the same for tracking_step_tree_segment_kernel
  const void* tree_segment_lds_kernel = nullptr;
  DevMem d_split;            // [objects][2 slots][parts][32 fields][256 / parts] granules, then one abort word per object
  size_t split_objects = 0;  // capacity of d_split
  unsigned split_seq = 0;    // launch counter inside the granule tags
  int split_parts_override = 0;  // m3t_hip_set_object_split(ctx, n > 1): workgroups per object (0: automatic)
  HostBlock split_abort;  // mapped host word: sequence number of a split step that gave up (MappedWord)
  unsigned split_abort_seen = 0;
  unsigned split_launches = 0;  // never reset (unlike split_seq): the value an aborting launch leaves in the host word
  int last_step_shape[4] = {0, 0, 0, 0};  // m3t_hip_get_step_shape
  bool state_valid = false;  // line/point state + g/H on the device reflect the last step
  TrackLdsLayout layout{};
  // tracking_step_compact_kernel (m3t_compact.hip): the launch shape of batches with two objects per CU and more
  CompactLayout compact{};
  size_t lds_compact = 0;
  CompactLayout compact_table{};  // ... with the pair table compacted in LDS (tracking_step_compact_table_kernel)
  size_t lds_compact_table = 0;   // 0: not available for this context's modalities
  HostBlock table_overflow;  // mapped word: mixed bins that did not fit the LDS table, largest over the workgroups
  bool compact_possible = false;       // every modality fits the kernel's assumptions (UploadTables)
  bool compact_fuses_histogram = false;  // ... and the count table fits next to the scratch block (<= 16 bins)
  // what the last step launched (m3t_step_plan.h): m3t_hip_get_step_variant reports it, m3t_hip_get_step_kernel too
  // except that the split kernel's moments-first instantiation goes by the split kernel's name there
  m3t_step::StepKernel last_step_kernel = m3t_step::StepKernel::kNone;
  // ROI ingest (m3t_ingest.hip): rectangles instead of whole frames
  bool roi_enabled = false;        // m3t_hip_set_roi_ingest
  bool roi_adaptive = false;       // ... with enable = 2: per-body margins from the motion over the last step
  float roi_margin_px = 0.0f;
  bool roi_recorded = false;       // the last step was a fused rigid launch with the ROI tables in place: the next pull may go as rectangles
  int roi_n_poses = 0;             // n_corr_iterations + 2
  int n_roi_items = 0;
  long long roi_pulls = 0;         // batch-frames uploaded as rectangles so far
  long long roi_repeated = 0;      // bodies whose step was repeated on whole frames so far (read with roi_get_status)
  DevMem d_search_poses, d_roi_items, d_roi_item_first, d_roi_all_cam_ids, d_roi_rects, d_roi_pose_snapshot,
         d_roi_motion_peak,  // [reader]: adaptive margins (roi_rect_kernel)
         d_roi_opt_of_region;  // [region modality]: its optimizer's row (region_histogram_kernel behind a guarded step)
  // the camera lists of the batches whose ids are not consecutive (the colour and the depth cameras of Region + Depth
  // objects: two lists), each in device memory of its own -- a slot's repair sources point into them
  static constexpr size_t kRoiScatteredLists = 8;
  std::vector<std::pair<std::vector<int>, std::unique_ptr<DevMem>>> roi_cam_id_lists;
  int roi_rect_slots = 0;          // d_roi_rects: [slot][camera id]
  // Where the whole frames behind the rectangles of a slot are (the repair after a guarded step reads them): one entry
  // per batch upload into the slot, replaced by the next upload of the same cameras.  The host block has to stay what
  // it is until the step that reads the slot is done -- the lifetime rule of every asynchronous upload.
  struct RoiSource {
    std::vector<int> ids;          // the batch's cameras (ring order)
    const int* d_ids = nullptr;    // the same on the device
    const uint8_t* src = nullptr;  // device address of the mapped host block
    size_t camera_stride = 0;
    uint32_t row_step = 0;
  };
  std::vector<std::vector<RoiSource>> roi_sources;  // [slot]
  // three snapshots of the bodies' poses, in turn: taken at the END of every fused rigid step (= the poses the next
  // step starts from, available a whole pull earlier than a snapshot at that step's start), or at a step's start when
  // the previous step's end does not vouch for them (first step, poses set by the host, other launches in between).
  // A rectangle upload reads the newest one and, for adaptive margins, the one before it.
  static constexpr int kRoiSnapshots = 3;
  Event roi_snapshot_done[kRoiSnapshots];
  bool roi_snapshot_valid = false;
  int roi_use = 0;              // the snapshot the next rectangle upload reads: the poses at the start of the step enqueued last
  int roi_prev = -1;            // the snapshot one step before roi_use (-1: none)
  int roi_end_index = 0;        // where the last step's end-of-step snapshot went
  bool roi_end_valid = false;   // ... and whether it still describes the device poses
  // one mapped block of two lists, each [0] count, [1 ..] body ids: steps that left their rectangles (and were
  // repeated), and behind them the bodies whose repeat missed again (no whole frame within reach)
  static constexpr int kRoiMissCapacity = 255;
  HostBlock roi_miss;
  static int* RoiMissList(void* block, bool unrecovered) {  // (block: roi_miss.host or .dev; null before ROI ingest)
    return block ? static_cast<int*>(block) + (unrecovered ? kRoiMissCapacity + 1 : 0) : nullptr;
  }
  int np_max = 0, off_points = 0;
  size_t lds_track = 0, lds_corr = 0, lds_hist = 0, lds_depth = 0;
  bool hist_counts_in_lds = true;
  // optional HIP-event timing of the two per-frame kernels (bench.py roofline leg)
  // pinned staging ring for the camera table: a frame switch is an async 1-2 KB copy, no host sync
  m3t_res::HostRing<8, kPinned> cam_staging;
  MappedRing reset_args;  // m3t_hip_reset_bodies / _structures: the call's lists and poses, read in place by its launches
  std::vector<std::unique_ptr<Judge>> judges;  // m3t_hip_judge_create
  Ingest ingest;  // asynchronous frame uploads and their order against the launches that read the frames
  bool timing = false;        // m3t_hip_set_kernel_timing(1): an event pair around every launch
  bool timing_region = false; // m3t_hip_set_kernel_timing(2): ONE pair around all launches until the query
  EventPair region;
  struct Pending { EventPair events; int which; };
  std::vector<Pending> pending;
  double kernel_ms[2] = {0.0, 0.0};
  int kernel_launches[2] = {0, 0};
};

namespace {

using Ctx = m3t_hip_context;

// RCCL entry points, resolved on first use from the process's librccl.so.1 (the one torch.distributed loaded, if any:
// a communicator and the all-reduce that uses it must come from the same library)
struct Rccl {
  void* handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string error;
  bool Load() {
    if (AllReduce) return true;
    handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!handle) handle = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!handle) { error = std::string("librccl.so.1: ") + dlerror(); return false; }
    GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(dlsym(handle, "ncclGetUniqueId"));
    CommInitRank = reinterpret_cast<decltype(CommInitRank)>(dlsym(handle, "ncclCommInitRank"));
    CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(handle, "ncclCommDestroy"));
    CommCount = reinterpret_cast<decltype(CommCount)>(dlsym(handle, "ncclCommCount"));
    AllReduce = reinterpret_cast<decltype(AllReduce)>(dlsym(handle, "ncclAllReduce"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(handle, "ncclGetErrorString"));
    if (!GetUniqueId || !CommInitRank || !CommDestroy || !AllReduce) { error = "librccl.so.1 lacks the nccl* entry points"; AllReduce = nullptr; return false; }
    return true;
  }
};
Rccl g_rccl;

int Fail(Ctx* c, int code, const std::string& msg) {
  if (c) c->error = msg;
  return code;
}
#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return Fail(ctx, M3T_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));    \
  } while (0)
#define REQUIRE(cond, code, msg) \
  do {                           \
    if (!(cond)) return Fail(ctx, code, msg); \
  } while (0)

// ---- .bin parser: model.cpp:218-284 + region_model.cpp:259-307,346-363 + depth_model.cpp:215-283
bool SkipBodyData(std::ifstream& ifs) {
  uint64_t len = 0;
  ifs.read(reinterpret_cast<char*>(&len), 8);
  if (!ifs || len > (1u << 20)) return false;
  ifs.seekg(std::streamoff(len + 4 + 1 + 1 + 4 + 64), std::ios::cur);
  return bool(ifs);
}
struct HostModel {
  int n_views = 0, n_points = 0;
  float stride = 0, max_radius = 0;
  std::vector<float> points, orientations, extents;
};
bool ParseModelFile(const char* path, bool region, HostModel* m, std::string* err) {
  std::ifstream ifs{path, std::ios::in | std::ios::binary};
  if (!ifs.is_open()) { *err = std::string("Could not open model file ") + path; return false; }
  char type = 0;
  int32_t version = 0, n_divides = 0, n_points = 0, image_size = 0;
  float sphere_radius = 0, max_radius = 0, stride = 0;
  uint8_t use_random_seed = 0;
  ifs.read(&type, 1);
  ifs.read(reinterpret_cast<char*>(&version), 4);
  ifs.read(reinterpret_cast<char*>(&sphere_radius), 4);
  ifs.read(reinterpret_cast<char*>(&n_divides), 4);
  ifs.read(reinterpret_cast<char*>(&n_points), 4);
  ifs.read(reinterpret_cast<char*>(&max_radius), 4);
  ifs.read(reinterpret_cast<char*>(&stride), 4);
  ifs.read(reinterpret_cast<char*>(&use_random_seed), 1);
  ifs.read(reinterpret_cast<char*>(&image_size), 4);
  if (!ifs) { *err = "truncated model header"; return false; }
  if (type != (region ? 'r' : 'd')) { *err = "Wrong model type"; return false; }
  if (version != (region ? 10 : 9)) { *err = "Wrong version id"; return false; }
  if (!SkipBodyData(ifs)) { *err = "bad body data"; return false; }
  uint64_t n_assoc = 0;
  ifs.read(reinterpret_cast<char*>(&n_assoc), 8);
  if (region) {
    for (int g = 0; g < 4; ++g) {
      uint64_t n = 0;
      ifs.read(reinterpret_cast<char*>(&n), 8);
      for (uint64_t i = 0; i < n && ifs; ++i)
        if (!SkipBodyData(ifs)) { *err = "bad associated body data"; return false; }
    }
  } else {
    for (uint64_t i = 0; i < n_assoc && ifs; ++i)
      if (!SkipBodyData(ifs)) { *err = "bad occlusion body data"; return false; }
  }
  uint64_t n_views = 0;
  ifs.read(reinterpret_cast<char*>(&n_views), 8);
  if (!ifs || n_views == 0 || n_views > (1u << 24) || n_points <= 0 || n_points > (1 << 20)) {
    *err = "bad view table";
    return false;
  }
  const int pf = region ? M3T_REGION_POINT_FLOATS : M3T_DEPTH_POINT_FLOATS;
  m->n_views = int(n_views);
  m->n_points = n_points;
  m->stride = stride;
  m->max_radius = max_radius;
  m->points.resize(size_t(n_views) * n_points * pf);
  m->orientations.resize(size_t(n_views) * 3);
  m->extents.resize(n_views);
  for (uint64_t v = 0; v < n_views; ++v) {
    ifs.read(reinterpret_cast<char*>(&m->points[v * n_points * pf]), std::streamsize(size_t(n_points) * pf * 4));
    ifs.read(reinterpret_cast<char*>(&m->orientations[v * 3]), 12);
    ifs.read(reinterpret_cast<char*>(&m->extents[v]), 4);
  }
  if (!ifs) { *err = "truncated view data"; return false; }
  return true;
}

int CreateModel(Ctx* ctx, bool region, int n_views, int n_points, const float* pts, const float* ori,
                const float* ext, float stride, float max_radius) {
  REQUIRE(n_views > 0 && n_points > 0 && pts && ori && ext, M3T_ERR_INVALID_ARGUMENT, "bad model description");
  auto m = std::make_unique<Model>();
  m->region = region;
  m->n_views = n_views;
  m->n_points = n_points;
  m->point_floats = region ? M3T_REGION_POINT_FLOATS : M3T_DEPTH_POINT_FLOATS;
  m->stride_depth_offset = stride;
  m->max_radius_depth_offset = max_radius;
  for (int v = 0; v < n_views; ++v) m->max_extent = std::max(m->max_extent, ext[v]);
  m->h_orientations.assign(ori, ori + size_t(n_views) * 3);
  for (int k = 0; k < 3; ++k) {
    m->box_min[k] = 3.0e38f;
    m->box_max[k] = -3.0e38f;
  }
  for (size_t i = 0; i < size_t(n_views) * n_points; ++i)
    for (int k = 0; k < 3; ++k) {
      m->box_min[k] = std::min(m->box_min[k], pts[i * m->point_floats + k]);
      m->box_max[k] = std::max(m->box_max[k], pts[i * m->point_floats + k]);
    }
  {  // the largest normalised radius of a point about the box's centre (m3t_roi_ellipsoid)
    double mid[3], half[3], worst = 0.0;
    bool flat = false;
    for (int k = 0; k < 3; ++k) {
      mid[k] = 0.5 * (double(m->box_min[k]) + double(m->box_max[k]));
      half[k] = 0.5 * (double(m->box_max[k]) - double(m->box_min[k]));
      flat = flat || !(half[k] > 1e-9);
    }
    for (size_t i = 0; !flat && i < size_t(n_views) * n_points; ++i) {
      double r2 = 0.0;
      for (int k = 0; k < 3; ++k) {
        const double q = (double(pts[i * m->point_floats + k]) - mid[k]) / half[k];
        r2 += q * q;
      }
      worst = std::max(worst, r2);
    }
    m->box_rho = flat ? 0.0f : float(std::sqrt(worst) * (1.0 + 1e-4));
  }
  size_t pb = size_t(n_views) * n_points * m->point_floats * 4;
  HIPCHK(m->points.alloc(pb));
  HIPCHK(m->orientations.alloc(size_t(n_views) * 12));
  HIPCHK(m->extents.alloc(size_t(n_views) * 4));
  HIPCHK(hipMemcpy(m->points.p, pts, pb, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->orientations.p, ori, size_t(n_views) * 12, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->extents.p, ext, size_t(n_views) * 4, hipMemcpyHostToDevice));
  {  // compact, 16-byte aligned copies: 32 B per point instead of 152/144 B, float4 per orientation
    const int pf = m->point_floats;
    std::vector<float> p8(size_t(n_views) * n_points * 8, 0.0f), o4(size_t(n_views) * 4, 0.0f);
    for (size_t i = 0; i < size_t(n_views) * n_points; ++i)
      for (int k = 0; k < (region ? 8 : 6); ++k) p8[i * 8 + k] = pts[i * pf + k];
    for (int v = 0; v < n_views; ++v)
      for (int k = 0; k < 3; ++k) o4[size_t(v) * 4 + k] = ori[size_t(v) * 3 + k];
    HIPCHK(UploadTable(&m->points8, p8));
    HIPCHK(UploadTable(&m->orientations4, o4));
  }
  if (n_views > M3T_VIEW_ROW) {
    const std::vector<float> rows = m3t_view_rows(ori, n_views);  // closest_view_local's table (m3t_view_rows.h)
    HIPCHK(UploadTable(&m->view_neighbors, rows));
  }
  auto& vec = region ? ctx->region_models : ctx->depth_models;
  vec.push_back(std::move(m));
  return int(vec.size()) - 1;
}

int LoadModel(Ctx* ctx, const char* path, bool region) {
  REQUIRE(path, M3T_ERR_INVALID_ARGUMENT, "null path");
  HostModel h;
  std::string err;
  if (!ParseModelFile(path, region, &h, &err)) return Fail(ctx, M3T_ERR_IO, err);
  return CreateModel(ctx, region, h.n_views, h.n_points, h.points.data(), h.orientations.data(), h.extents.data(),
                     h.stride, h.max_radius);
}

int CreateCamera(Ctx* ctx, const m3t_intrinsics* intr, const float* w2c, bool depth, float depth_scale) {
  REQUIRE(intr && w2c && intr->width > 0 && intr->height > 0, M3T_ERR_INVALID_ARGUMENT, "bad camera description");
  auto c = std::make_unique<Camera>();
  c->is_depth = depth;
  c->intr = *intr;
  std::memcpy(c->world2camera, w2c, 64);
  c->depth_scale = depth_scale;
  size_t row = size_t(intr->width) * (depth ? 2 : 3);
  c->pitch = uint32_t((row + 63) / 64 * 64);
  c->frame_bytes = size_t(c->pitch) * intr->height;
  c->SetSlots(1);
  HIPCHK(c->ring.alloc(c->frame_bytes + 64));  // +64: pixels are fetched as one 4-byte load (B,G,R,+1)
  c->frames = c->ring.as<uint8_t>();
  c->slot_stride = c->frame_bytes;
  ctx->cameras.push_back(std::move(c));
  ctx->cams_dirty = true;
  return int(ctx->cameras.size()) - 1;
}

void RoiMarkWholeFrame(Ctx* ctx, int camera, int slot, hipStream_t stream);  // (ROI ingest, below)
void RoiMarkWholeFrames(Ctx* ctx, const int* ids, int n, int slot, hipStream_t stream);

int UploadFrame(Ctx* ctx, int id, int slot, const void* pixels, size_t row_step) {
  REQUIRE(id >= 0 && id < int(ctx->cameras.size()) && pixels, M3T_ERR_INVALID_ARGUMENT, "bad camera id");
  Camera& c = *ctx->cameras[id];
  REQUIRE(slot >= 0 && slot < c.n_slots, M3T_ERR_INVALID_ARGUMENT, "bad frame slot");
  size_t row = size_t(c.intr.width) * (c.is_depth ? 2 : 3);
  REQUIRE(row_step >= row, M3T_ERR_INVALID_ARGUMENT, "row_step smaller than one image row");
  uint8_t* dst = c.frame(slot);
  HIPCHK(hipMemcpy2DAsync(dst, c.pitch, pixels, row_step, row, c.intr.height, hipMemcpyHostToDevice, ctx->stream));
  // the host buffer is only borrowed for the duration of the call
  RoiMarkWholeFrame(ctx, id, slot, ctx->stream);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  c.has_image[slot] = true;
  return M3T_OK;
}

// ---- device tables -----------------------------------------------------------
// Workgroups of `kernel` (threads, dynamic LDS bytes) a CU keeps resident: asked once per (kernel, shape) and kept --
// the per-frame launch decision must not call into the driver (round-3 advisor).  0 = the query failed.
template <typename K>
int ResidentBlocks(Ctx* ctx, K kernel, int threads, size_t lds) {
  const auto key = std::make_tuple(reinterpret_cast<const void*>(kernel), threads, lds);
  auto it = ctx->occupancy_cache.find(key);
  if (it != ctx->occupancy_cache.end()) return it->second;
  int resident = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kernel, threads, lds) != hipSuccess) {
    (void)hipGetLastError();
    resident = 0;
  }
  ctx->occupancy_cache[key] = resident;
  return resident;
}

// A word the kernels write with system scope and the host reads in place: 64 zeroed bytes of mapped host memory,
// allocated on first use.
int MappedWord(Ctx* ctx, HostBlock* word) {
  if (!word->host) HIPCHK(word->Alloc(64, kMapped, true));
  return M3T_OK;
}

// After a synchronisation: did the workgroups of a split object ever give up waiting for each other?  (They
// are all resident by construction; the bounded wait exists so that a surprise cannot hang the device.)
int CheckSplitExchange(Ctx* ctx) {
  // the word lives in mapped host memory: no copy, no synchronisation; the kernel writes it with system scope
  if (!ctx->split_abort.host) return M3T_OK;
  const unsigned value = __atomic_load_n(ctx->split_abort.as<unsigned>(), __ATOMIC_ACQUIRE);
  if (value != ctx->split_abort_seen) {
    ctx->split_abort_seen = value;
    using m3t_step::StepKernel;
    const bool tree = m3t_step::IsTreeStepKernel(ctx->last_step_kernel);
    const bool render = ctx->last_step_kernel == StepKernel::kSplitRender;
    const std::string msg =
        std::string(m3t_step::StepKernelName(tree || render ? ctx->last_step_kernel : StepKernel::kSplit)) +
        ": a workgroup waited in vain for the other workgroups of its " + (tree ? "kinematic structure" : "object") +
        " (is another process or stream using this GPU?); the step was abandoned part-way: workgroups that had "
        "already finished may have written the new pose" + (tree ? "s and joints" : "") +
        " and blended their share of the histogram bins, so the poses and histograms involved are undefined; set the "
        "poses again and call start_modalities.  m3t_hip_set_object_split(ctx, 0) keeps both kernels out: one "
        "workgroup per rigid object, per-sub-step launches for kinematic structures";
    return Fail(ctx, M3T_ERR_DEVICE, msg.c_str());
  }
  return M3T_OK;
}
int SyncPosesToHost(Ctx* ctx) {
  // device is authoritative after any device-side optimisation
  size_t n = ctx->body_poses.size() / 16;
  if (n == 0 || ctx->poses_dirty_host) return M3T_OK;
  HIPCHK(hipMemcpyAsync(ctx->body_poses.data(), ctx->d_poses.p, n * 64, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return CheckSplitExchange(ctx);
}

void ComputeLayout(Ctx* ctx) {
  int nl = 1, ns = 1, bins3 = 0, np = 1;
  bool hist_lds = !ctx->region_mods.empty();
  for (auto& m : ctx->region_mods) {
    nl = std::max(nl, m->p.n_lines_max);
    ns = std::max(ns, std::max(9, m->dev.n_seg));
    int b = m->p.n_histogram_bins;
    bins3 = std::max(bins3, b * b * b);
  }
  for (auto& m : ctx->depth_mods) np = std::max(np, m->p.n_points_max);
  // the LDS-staged pair table must fit next to the line buffers (<= 16 bins: 32 KB)
  if (bins3 * 8 > 32 * 1024) hist_lds = false;
  TrackLdsLayout L{};
  L.nl = nl;
  L.ns = ns;
  int off = 0;
  L.off_misc = off; off += M3T_MISC_FLOATS;
  L.off_state = off; off += LS_FIELDS * nl;
  off = (off + 3) / 4 * 4;
  // chain | seg_f | seg_b live during a correspondence search; the product rows of the g/H sums during the Newton
  // steps between two searches: the same LDS
  const int block = off;
  L.off_chain = off; off += nl * ns;
  L.off_seg_f = off; off += nl * ns;
  L.off_seg_b = off; off += nl * ns;
  L.pitch_r = chain_pitch(nl);
  L.pitch_d = chain_pitch(np);
  L.off_rows_r = block;
  L.off_rows_d = block + (ctx->region_mods.empty() ? 0 : 27 * L.pitch_r);
  const int rows_end = L.off_rows_d + (ctx->depth_mods.empty() ? 0 : 27 * L.pitch_d);
  off = (std::max(off, rows_end) + 3) / 4 * 4;
  ctx->off_points = off;
  ctx->np_max = np;
  int off_with_points = off + (ctx->depth_mods.empty() ? 0 : PS_FIELDS * np);
  if (hist_lds) {
    L.off_hist = (off_with_points + 3) / 4 * 4;
    L.total_floats = L.off_hist + bins3 * 2;
  } else {
    L.off_hist = -1;
    L.total_floats = off_with_points;
  }
  ctx->layout = L;
  ctx->lds_track = size_t(L.total_floats) * 4;
  // the correspondence-only kernel does not need the depth point block
  ctx->lds_corr = ctx->lds_track;
  ctx->lds_depth = size_t(M3T_MISC_FLOATS + (PS_FIELDS * np + 3) / 4 * 4 + 27 * L.pitch_d) * 4;
  size_t counts = size_t(bins3) * 4;
  ctx->hist_counts_in_lds = (M3T_MISC_FLOATS * 4 + counts) <= 160 * 1024;
  ctx->lds_hist = M3T_MISC_FLOATS * 4 + (ctx->hist_counts_in_lds ? counts : 0);
  // the compact carve-up: scratch | line state | factor rows (+ point state | factor rows)
  CompactLayout C{};
  C.nl = nl;
  C.np = np;
  int o = M3T_COMPACT_MISC_FLOATS;
  C.off_state = o; o += ctx->region_mods.empty() ? 0 : CS_FIELDS * nl;
  o = (o + 3) / 4 * 4;
  C.pitch_r = chain_pitch(nl);
  C.off_rows_r = o; o += ctx->region_mods.empty() ? 0 : M3T_COMPACT_ROWS * C.pitch_r;
  o = (o + 3) / 4 * 4;
  C.off_points = o; o += ctx->depth_mods.empty() ? 0 : PS_FIELDS * np;
  o = (o + 3) / 4 * 4;
  C.pitch_d = chain_pitch(np);
  C.off_rows_d = o; o += ctx->depth_mods.empty() ? 0 : M3T_COMPACT_ROWS * C.pitch_d;
  C.total_floats = (o + 3) / 4 * 4;
  // The histogram update rides along in the tail of the launch.  Up to 16 bins per channel the packed count table
  // (one word per bin) fits behind the 1024-float scratch block; with 32 bins the samples' bins go to a 16-bit list
  // and the bins are counted and blended in passes (region_histogram_update<.., LIST>).  Budget: 40 KB per
  // workgroup, so that four stay resident per CU.  (Counting by L2 atomics into a table in HBM instead was measured:
  // 0.77 ms per step for 4096 objects x 8000 samples -- more than the whole separate histogram kernel.)
  ctx->compact_fuses_histogram = false;
  C.tail_list_row = C.tail_pass_bins = C.off_tail_list = C.off_tail_counts = 0;
  const int budget = 40 * 1024 / 4;
  if (bins3 > 0 && M3T_MISC_FLOATS + bins3 <= budget) {
    ctx->compact_fuses_histogram = true;
    C.off_tail_counts = M3T_MISC_FLOATS;
    C.total_floats = std::max(C.total_floats, M3T_MISC_FLOATS + bins3);
  } else if (bins3 > 0 && bins3 <= 32768) {
    float longest = 0.0f;
    for (auto& m : ctx->region_mods) longest = std::max(longest, m->p.max_considered_line_length);
    const int row = int(longest + 0.5f) + 1;
    const int list_words = nl * row;  // two walkers per line, two entries per word
    int pass = bins3;
    while (pass > 256 && M3T_MISC_FLOATS + list_words + pass > budget) pass /= 2;
    if (M3T_MISC_FLOATS + list_words + pass <= budget) {
      ctx->compact_fuses_histogram = true;
      C.tail_list_row = row;
      C.tail_pass_bins = pass;
      C.off_tail_list = M3T_MISC_FLOATS;
      C.off_tail_counts = M3T_MISC_FLOATS + list_words;
      C.total_floats = std::max(C.total_floats, M3T_MISC_FLOATS + list_words + pass);
    }
  }
  ctx->compact = C;
  ctx->lds_compact = size_t(C.total_floats) * 4;
  // tracking_step_compact_table_kernel: the same carve-up with the compacted pair table behind the search's part (the
  // tail's lists and counts lie over it: the table is dead by then).  Region-only batches with histograms of at least
  // 1024 bins; the budget is a third of the CU's LDS (three workgroups per CU instead of four).
  ctx->compact_table = C;
  ctx->compact_table.off_table = 0;
  ctx->lds_compact_table = 0;
  if (bins3 >= 1024 && bins3 % 32 == 0 && bins3 <= 32768 && !ctx->region_mods.empty()) {
    CompactLayout T = C;
    T.off_table = (o + 3) / 4 * 4;  // (o: the end of the search's carve-up)
    T.table_words = bins3 / 32;
    // 52 KB: three workgroups per CU with room for the allocation granule (a third of 160 KB, 54 356 B, does not fit three
    // times: measured, the kernel ran at two workgroups per CU)
    int budget_floats = 52 * 256;
    if (const char* e = std::getenv("M3T_HIP_COMPACT_TABLE_KB")) budget_floats = std::atoi(e) * 256;  // developer override
    const int index_floats = 2 * T.table_words + (T.table_words + 1) / 2;  // bit words, 16-bit ranks
    // (a stored pair takes five bytes: m3t_compact.hip, CompactTable)
    int cap = int((long(budget_floats - T.off_table - index_floats - 12) * 4) / 5) - 3;
    if (const char* e = std::getenv("M3T_HIP_COMPACT_TABLE_CAP")) cap = std::min(cap, std::atoi(e));  // (tests: force the overflow path)
    if (cap >= 64) {
      T.table_cap = std::min(std::min(cap, bins3), 65000);
      T.total_floats = std::max(C.total_floats,
                                (T.off_table + index_floats + (3 + T.table_cap) + (3 + T.table_cap + 3) / 4 + 3) / 4 * 4);
      T.table_overflow = nullptr;  // (set where the kernel is launched: a mapped host word)
      ctx->compact_table = T;
      ctx->lds_compact_table = size_t(T.total_floats) * 4;
    }
  }
}

// the 42-float g/H block of a modality, whatever its kind (Link::CalculateGradientAndHessian sums them, link.cpp:184-193)
float* ModalityGhPointer(Ctx* ctx, const ModalityRef& ref) {
  switch (ref.kind) {
    case kRegionModality: return ctx->region_mods[ref.index]->gh.as<float>();
    case kDepthModality: return ctx->depth_mods[ref.index]->gh.as<float>();
    default: return ctx->texture_mods[ref.index]->gh.as<float>();
  }
}
int ModalityBody(Ctx* ctx, const ModalityRef& ref) {
  switch (ref.kind) {
    case kRegionModality: return ctx->region_mods[ref.index]->body;
    case kDepthModality: return ctx->depth_mods[ref.index]->body;
    default: return ctx->texture_mods[ref.index]->body;
  }
}

void DfsOrder(Ctx* ctx, int link, std::vector<int>* order) {
  order->push_back(link);
  for (int c : ctx->links[link].children) DfsOrder(ctx, c, order);
}

// device -> host mirror of the joint poses (after device-side UpdatePoses)
int PullLinks(Ctx* ctx) {
  if (!ctx->links_device_newer || !ctx->tree_mode) return M3T_OK;
  size_t n = 0;
  for (auto& o : ctx->optimizers) n += o.order.size();
  std::vector<LinkDev> dev(n);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (n) HIPCHK(hipMemcpy(dev.data(), ctx->d_links.p, n * sizeof(LinkDev), hipMemcpyDeviceToHost));
  size_t off = 0;
  for (auto& o : ctx->optimizers)
    for (int lid : o.order) {
      Link& l = ctx->links[lid];
      std::memcpy(l.body2joint, dev[off].body2joint, 64);
      std::memcpy(l.joint2parent, dev[off].joint2parent, 64);
      std::memcpy(l.link2world, dev[off].link2world, 64);
      ++off;
    }
  ctx->links_device_newer = false;
  return M3T_OK;
}

int UploadTreeTables(Ctx* ctx) {
  int r = PullLinks(ctx);
  if (r) return r;
  std::vector<LinkDev> links;
  std::vector<ConstraintDev> cons;
  std::vector<SoftConstraintDev> soft;
  std::vector<TreeOptDev> opts(ctx->optimizers.size());
  std::vector<size_t> link_off(ctx->optimizers.size()), con_off(ctx->optimizers.size()), work_off(ctx->optimizers.size()),
      soft_off(ctx->optimizers.size());
  size_t work_total = 0, partial_total = 0, tree_work_max = 0;
  for (auto& l : ctx->links) { l.optimizer = -1; l.local_index = -1; }
  for (size_t oi = 0; oi < ctx->optimizers.size(); ++oi) {
    Optimizer& o = ctx->optimizers[oi];
    o.order.clear();
    DfsOrder(ctx, o.link, &o.order);
    int dof = 0;
    for (size_t k = 0; k < o.order.size(); ++k) {
      Link& l = ctx->links[o.order[k]];
      REQUIRE(l.optimizer < 0, M3T_ERR_INVALID_ARGUMENT, "a link belongs to two optimizers");
      l.optimizer = int(oi);
      l.local_index = int(k);
    }
    link_off[oi] = links.size();
    for (int lid : o.order) {
      const Link& l = ctx->links[lid];
      LinkDev d{};
      d.body = l.body;
      d.parent = l.parent >= 0 ? ctx->links[l.parent].local_index : -1;
      std::memcpy(d.body2joint, l.body2joint, 64);
      std::memcpy(d.joint2parent, l.joint2parent, 64);
      std::memcpy(d.link2world, l.link2world, 64);
      for (int i = 0; i < 6; ++i) d.free_directions[i] = l.free_directions[i];
      d.fixed_body2joint_pose = l.fixed_body2joint_pose;
      d.first_jacobian_index = dof;  // optimizer.cpp:237-250
      for (int i = 0; i < 6; ++i) dof += l.free_directions[i] ? 1 : 0;
      REQUIRE(int(l.modalities.size()) <= M3T_MAX_LINK_MODALITIES, M3T_ERR_UNSUPPORTED, "too many modalities per link");
      d.n_gh = int(l.modalities.size());
      for (int k = 0; k < d.n_gh; ++k) {
        d.gh[k] = ModalityGhPointer(ctx, ctx->modalities[l.modalities[k]]);
      }
      links.push_back(d);
    }
    o.dof = dof;
    con_off[oi] = cons.size();
    o.n_rows = 0;
    for (int cid : o.constraints) {
      const ConstraintH& c = ctx->constraints[cid];
      REQUIRE(ctx->links[c.link1].optimizer == int(oi) && ctx->links[c.link2].optimizer == int(oi),
              M3T_ERR_INVALID_ARGUMENT, "constraint links must belong to the optimizer's structure");
      ConstraintDev d{};
      d.link1 = ctx->links[c.link1].local_index;
      d.link2 = ctx->links[c.link2].local_index;
      std::memcpy(d.body12joint1, c.body12joint1, 64);
      std::memcpy(d.body22joint2, c.body22joint2, 64);
      d.n = 0;
      for (int i = 0; i < 6; ++i) { d.directions[i] = c.directions[i]; d.n += c.directions[i] ? 1 : 0; }
      o.n_rows += d.n;
      cons.push_back(d);
    }
    soft_off[oi] = soft.size();
    for (int sid : o.soft_constraints) {
      const SoftConstraintH& c = ctx->soft_constraints[sid];
      REQUIRE(ctx->links[c.joint.link1].optimizer == int(oi) && ctx->links[c.joint.link2].optimizer == int(oi),
              M3T_ERR_INVALID_ARGUMENT, "soft constraint links must belong to the optimizer's structure");
      SoftConstraintDev d{};
      d.joint.link1 = ctx->links[c.joint.link1].local_index;
      d.joint.link2 = ctx->links[c.joint.link2].local_index;
      std::memcpy(d.joint.body12joint1, c.joint.body12joint1, 64);
      std::memcpy(d.joint.body22joint2, c.joint.body22joint2, 64);
      for (int i = 0; i < 6; ++i) { d.joint.directions[i] = c.joint.directions[i]; d.joint.n += c.joint.directions[i] ? 1 : 0; }
      d.max_distance_rotation = c.max_distance_rotation;
      d.max_distance_translation = c.max_distance_translation;
      d.standard_deviation_rotation = c.standard_deviation_rotation;
      d.standard_deviation_translation = c.standard_deviation_translation;
      soft.push_back(d);
    }
    work_off[oi] = work_total;
    work_total += tree_work_floats(int(o.order.size()), dof, o.n_rows);
    tree_work_max = std::max(tree_work_max, tree_work_floats(int(o.order.size()), dof, o.n_rows));
    o.partial_offset = partial_total;
    partial_total += size_t(dof) * dof + dof;
  }
  HIPCHK(UploadTable(&ctx->d_links, links));
  HIPCHK(UploadTable(&ctx->d_links_alt, links));
  HIPCHK(UploadTable(&ctx->d_constraints, cons));
  HIPCHK(UploadTable(&ctx->d_soft, soft));
  HIPCHK(ctx->d_work.alloc(std::max<size_t>(1, work_total) * 4));
  // the structures' work arrays live in LDS when the largest fits (one wave per structure, m3t_links.hip)
  ctx->tree_lds = tree_work_max * 4 <= size_t(152) * 1024 ? tree_work_max * 4 : 0;
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(links_project_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, int(ctx->tree_lds)));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(links_solve_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, int(ctx->tree_lds)));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(links_solve_sums_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, int(ctx->tree_lds)));
  {
    std::vector<int> first(std::max<size_t>(1, opts.size()), 0);
    for (size_t oi = 0; oi < opts.size(); ++oi) first[oi] = int(link_off[oi]);
    HIPCHK(UploadTable(&ctx->d_link_first, first));
    ctx->link_sums_count = links.size() * 42;
    HIPCHK(ctx->d_link_sums.alloc(std::max<size_t>(1, ctx->link_sums_count) * 4));
    HIPCHK(hipMemset(ctx->d_link_sums.p, 0, ctx->d_link_sums.bytes));
    HIPCHK(ctx->d_link_sums_alt.alloc(std::max<size_t>(1, ctx->link_sums_count) * 4));
    HIPCHK(hipMemset(ctx->d_link_sums_alt.p, 0, ctx->d_link_sums_alt.bytes));
  }
  HIPCHK(ctx->d_partial.alloc(std::max<size_t>(1, partial_total) * 4));
  HIPCHK(hipMemset(ctx->d_partial.p, 0, ctx->d_partial.bytes));
  ctx->partial_count = partial_total;
  for (size_t oi = 0; oi < opts.size(); ++oi) {
    const Optimizer& o = ctx->optimizers[oi];
    TreeOptDev& d = opts[oi];
    d.n_links = int(o.order.size());
    d.links = ctx->d_links.as<LinkDev>() + link_off[oi];
    d.dof = o.dof;
    d.n_constraints = int(o.constraints.size());
    d.constraints = ctx->d_constraints.as<ConstraintDev>() + con_off[oi];
    d.n_rows = o.n_rows;
    d.n_soft = int(o.soft_constraints.size());
    d.soft = ctx->d_soft.as<SoftConstraintDev>() + soft_off[oi];
    d.tikhonov_rotation = o.tr;
    d.tikhonov_translation = o.tt;
    d.work = ctx->d_work.as<float>() + work_off[oi];
    d.partial = ctx->d_partial.as<float>() + o.partial_offset;
    d.links_alt = ctx->d_links_alt.as<LinkDev>() + link_off[oi];
    d.first_link = int(link_off[oi]);
  }
  // tracking_step_tree_kernel: the links that carry modalities, one workgroup each (at most one region and one
  // depth modality per link, every modality on a link), their exchange buffers, the LDS of a structure's copy
  {
    std::vector<TreeStepDev> steps;
    std::vector<int> tracked;
    std::vector<size_t> tracked_off(opts.size()), exchange_off(opts.size());
    size_t exchange_total = 0, attached = 0;
    bool possible = true;
    ctx->tree_block_floats = 0;
    ctx->tree_untracked_structure = false;
    for (size_t oi = 0; oi < opts.size(); ++oi) {
      const Optimizer& o = ctx->optimizers[oi];
      tracked_off[oi] = tracked.size();
      int n_tracked = 0;
      for (size_t k = 0; k < o.order.size(); ++k) {
        const Link& l = ctx->links[o.order[k]];
        if (l.modalities.empty()) continue;
        TreeStepDev st{};
        st.opt = int(oi);
        st.link = int(k);
        st.tracked = n_tracked++;
        st.region_modality = st.depth_modality = -1;
        st.region_first = 1;
        for (size_t m = 0; m < l.modalities.size(); ++m) {
          const ModalityRef& ref = ctx->modalities[l.modalities[m]];
          ++attached;
          if (ref.kind == kTextureModality) {  // (the one-launch steps do not know texture modalities)
            possible = false;
            continue;
          }
          const bool region = ref.kind == kRegionModality;
          int& slot = region ? st.region_modality : st.depth_modality;
          if (slot >= 0 || l.body < 0) possible = false;  // two of a kind on one link, or a modality without a body
          slot = ref.index;
          if (m == 0) st.region_first = region ? 1 : 0;
        }
        steps.push_back(st);
        tracked.push_back(int(k));
      }
      opts[oi].n_tracked = n_tracked;
      if (n_tracked == 0) ctx->tree_untracked_structure = true;
      exchange_off[oi] = exchange_total;
      exchange_total += size_t(2) * n_tracked * M3T_TREE_GRANULES + 1;  // + the structure's abort word
      const size_t block = (o.order.size() * sizeof(LinkDev) + 3) / 4 + o.order.size() * 42 + size_t(o.dof) * o.dof + o.dof +
                           tree_work_floats(int(o.order.size()), o.dof, o.n_rows);
      ctx->tree_block_floats = std::max(ctx->tree_block_floats, (block + 3) / 4 * 4);
    }
    if (attached != ctx->modalities.size() || steps.empty()) possible = false;
    // what the one-launch step's structure code is laid out for (m3t_links.hip, round 5); larger structures take the
    // per-sub-step launches.  Structures with Constraint / SoftConstraint objects run the kernel that has their code.
    ctx->tree_constrained = false;
    for (size_t oi = 0; oi < opts.size(); ++oi) {
      const Optimizer& o = ctx->optimizers[oi];
      if (int(o.order.size()) > M3T_TREE_FUSED_MAX_LINKS || o.dof + o.n_rows > M3T_TREE_FUSED_MAX_SIZE) possible = false;
      if (!o.constraints.empty() || !o.soft_constraints.empty()) ctx->tree_constrained = true;
    }
    HIPCHK(UploadTable(&ctx->d_treesteps, steps));
    HIPCHK(UploadTable(&ctx->d_tracked_links, tracked));
    HIPCHK(ctx->d_tree_exchange.alloc(std::max<size_t>(1, exchange_total) * 8));
    HIPCHK(hipMemset(ctx->d_tree_exchange.p, 0, ctx->d_tree_exchange.bytes));
    ctx->tree_seq = 0;
    for (size_t oi = 0; oi < opts.size(); ++oi) {
      opts[oi].tracked_links = ctx->d_tracked_links.as<int>() + tracked_off[oi];
      opts[oi].exchange = ctx->d_tree_exchange.as<unsigned long long>() + exchange_off[oi];
    }
    ctx->n_treesteps = int(steps.size());
    ctx->tree_fused_possible = possible;
  }
  HIPCHK(UploadTable(&ctx->d_treeopts, opts));  // (last: its entries point into the tables above)
  return M3T_OK;
}

// A list of renderers as {renderer, twin or -1} pairs.  Twins: two renderers of a list that differ in nothing but the id
// written (focused_setup_kernel) are drawn once.
std::vector<int> RendererPairs(Ctx* ctx, const std::vector<int>& list) {
  auto same_rendering = [&](int a, int b) {
    const RendererH& x = *ctx->renderers[a];
    const RendererH& y = *ctx->renderers[b];
    return x.camera == y.camera && x.geometry == y.geometry && x.image_size == y.image_size && x.z_min == y.z_min &&
           x.z_max == y.z_max && x.referenced == y.referenced;
  };
  std::vector<int> pairs;
  std::vector<char> taken(list.size(), 0);
  for (size_t i = 0; i < list.size(); ++i) {
    if (taken[i]) continue;
    int twin = -1;
    for (size_t j = i + 1; j < list.size() && twin < 0; ++j)
      if (!taken[j] && same_rendering(list[i], list[j])) {
        twin = list[j];
        taken[j] = 1;
      }
    pairs.push_back(list[i]);
    pairs.push_back(twin);
  }
  return pairs;
}

// RendererDev table + the renderer fields of the modality tables + the two "which renderers" lists
// (region modalities' renderers for start / results, all referenced ones for correspondences)
int UploadRendererTables(Ctx* ctx) {
  {  // shared ColorHistograms objects
    std::vector<SharedHistogramsDev> sh(ctx->shared_histograms.size());
    for (size_t i = 0; i < sh.size(); ++i) {
      SharedHistogramsH& h = *ctx->shared_histograms[i];
      sh[i].n_bins = h.n_bins;
      sh[i].learning_rate_f = h.learning_rate_f;
      sh[i].learning_rate_b = h.learning_rate_b;
      sh[i].histogram_f = h.hist_f.as<float>();
      sh[i].histogram_b = h.hist_b.as<float>();
      sh[i].histogram_norm = h.hist_norm.as<float2>();
      sh[i].counts = h.counts.as<unsigned long long>();
    }
    HIPCHK(UploadTable(&ctx->d_shared_histograms, sh));
  }
  const size_t n = ctx->renderers.size();
  std::vector<RendererDev> table(n);
  for (size_t i = 0; i < n; ++i) {
    RendererH& h = *ctx->renderers[i];
    RendererDev& d = table[i];
    std::memset(&d, 0, sizeof(d));
    d.camera = h.camera;
    d.silhouette = h.silhouette ? 1 : 0;
    d.id_type = h.id_type;
    d.image_size = h.image_size;
    d.z_min = h.z_min;
    d.z_max = h.z_max;
    const std::vector<int>& bodies = ctx->renderer_geometries[h.geometry];
    d.n_bodies = int(bodies.size());
    for (int k = 0; k < d.n_bodies; ++k) {
      const BodyGeometryH& g = *ctx->body_geometries[bodies[k]];
      d.body[k] = bodies[k];
      d.vertices[k] = g.vertices.as<float>();
      d.triangles[k] = g.triangles.as<int>();
      d.n_triangles[k] = g.n_triangles;
      std::memcpy(d.geometry2body[k], g.geometry2body, 64);
      d.culling[k] = g.culling;
      d.id[k] = h.id_type == M3T_ID_TYPE_REGION ? g.region_id : g.body_id;
    }
    d.n_referenced = int(h.referenced.size());
    for (int k = 0; k < d.n_referenced; ++k) {
      d.referenced[k] = h.referenced[k];
      d.referenced_diameter[k] = ctx->body_geometries[h.referenced[k]]->maximum_body_diameter;
    }
    d.depth_image = h.depth.as<uint16_t>();
    d.silhouette_image = h.sil.as<uint8_t>();
    d.packed = h.packed.as<uint32_t>();
    d.state = h.state.as<float>();
    int n_triangles = 0;
    for (int k = 0; k < d.n_bodies; ++k) n_triangles += d.n_triangles[k];
    if (h.survivor_capacity < n_triangles || !h.n_survivors.p) {
      HIPCHK(hipStreamSynchronize(ctx->stream));
      HIPCHK(h.survivors.alloc(std::max<size_t>(1, size_t(n_triangles)) * M3T_SURVIVOR_BYTES));
      HIPCHK(h.n_survivors.alloc(64));
      HIPCHK(hipMemset(h.n_survivors.p, 0, 64));
      h.survivor_capacity = n_triangles;
    }
    d.survivors = h.survivors.p;
    d.n_survivors = h.n_survivors.as<int>();
    d.survivor_capacity = h.survivor_capacity;
  }
  HIPCHK(UploadTable(&ctx->d_renderers, table));
  auto slot_of = [&](int renderer, int body) {
    const std::vector<int>& ref = ctx->renderers[renderer]->referenced;
    for (size_t k = 0; k < ref.size(); ++k)
      if (ref[k] == body) return int(k);
    return -1;
  };
  std::vector<char> for_region(n, 0), for_all(n, 0);
  for (auto& m : ctx->region_mods) {
    RegionModDev& d = m->dev;
    d.depth_renderer = d.model_occlusions ? ctx->d_renderers.as<RendererDev>() + m->depth_renderer : nullptr;
    d.silhouette_renderer = d.use_region_checking ? ctx->d_renderers.as<RendererDev>() + m->silhouette_renderer : nullptr;
    d.depth_renderer_slot = d.model_occlusions ? slot_of(m->depth_renderer, m->body) : -1;
    d.silhouette_renderer_slot = d.use_region_checking ? slot_of(m->silhouette_renderer, m->body) : -1;
    if (d.model_occlusions) for_region[m->depth_renderer] = for_all[m->depth_renderer] = 1;
    if (d.use_region_checking) for_region[m->silhouette_renderer] = for_all[m->silhouette_renderer] = 1;
  }
  for (auto& m : ctx->depth_mods) {
    DepthModDev& d = m->dev;
    d.depth_renderer = d.model_occlusions ? ctx->d_renderers.as<RendererDev>() + m->depth_renderer : nullptr;
    d.silhouette_renderer =
        d.use_silhouette_checking ? ctx->d_renderers.as<RendererDev>() + m->silhouette_renderer : nullptr;
    d.depth_renderer_slot = d.model_occlusions ? slot_of(m->depth_renderer, m->body) : -1;
    d.silhouette_renderer_slot = d.use_silhouette_checking ? slot_of(m->silhouette_renderer, m->body) : -1;
    if (d.model_occlusions) for_all[m->depth_renderer] = 1;
    if (d.use_silhouette_checking) for_all[m->silhouette_renderer] = 1;
  }
  for (auto& m : ctx->texture_mods) {  // start_modality_renderer_ptrs / results_renderer_ptrs :516-524
    TextureModDev& d = m->dev;
    d.silhouette_renderer = ctx->d_renderers.as<RendererDev>() + m->silhouette_renderer;
    d.silhouette_renderer_slot = slot_of(m->silhouette_renderer, m->body);
    d.depth_renderer = d.model_occlusions ? ctx->d_renderers.as<RendererDev>() + m->depth_renderer : nullptr;
    d.depth_renderer_slot = d.model_occlusions ? slot_of(m->depth_renderer, m->body) : -1;
    for_region[m->silhouette_renderer] = 1;
    if (d.model_occlusions) for_region[m->depth_renderer] = 1;
  }
  std::vector<int> list_region, list_all;
  for (size_t i = 0; i < n; ++i) {
    if (for_region[i]) list_region.push_back(int(i));
    if (for_all[i]) list_all.push_back(int(i));
  }
  const std::vector<int> pairs_region = RendererPairs(ctx, list_region), pairs_all = RendererPairs(ctx, list_all);
  ctx->n_render_region_pairs = int(pairs_region.size() / 2);
  ctx->n_render_all_pairs = int(pairs_all.size() / 2);
  HIPCHK(UploadTable(&ctx->d_render_region_pairs, pairs_region));
  HIPCHK(UploadTable(&ctx->d_render_all_pairs, pairs_all));
  ctx->n_render_region = int(list_region.size());
  ctx->n_render_all = int(list_all.size());
  HIPCHK(UploadTable(&ctx->d_render_region, list_region));
  HIPCHK(UploadTable(&ctx->d_render_all, list_all));
  return M3T_OK;
}

// Which form a rendering takes and with what grid is decided in m3t_render_plan.h (host-checkable); what this file adds
// is the one thing the plan cannot know: whether this device grants the resolve kernels their LDS.
using m3t_render::RenderLaunchShape;
RenderLaunchShape RenderShape(int n_pairs, int largest_image_size) {
  return m3t_render::RenderShape(n_pairs, largest_image_size, m3t_render::ReadRenderOverrides());
}
// the two-launch form (z-buffer band in LDS) for a rendering of this shape?
bool LdsRasterFits(Ctx* ctx, const RenderLaunchShape& shape, int largest_image_size) {
  if (ctx->lds_raster < 0) {  // once per context (= per device)
    ctx->lds_raster = 1;
    if (m3t_render::ReadRenderOverrides().no_lds_raster) ctx->lds_raster = 0;
    else
      for (const void* kernel : {reinterpret_cast<const void*>(focused_resolve_kernel),
                                 reinterpret_cast<const void*>(focused_resolve_flagged_kernel)})
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(m3t_render::kCuLdsBytes)) != hipSuccess) {
          (void)hipGetLastError();
          ctx->lds_raster = 0;
        }
  }
  return m3t_render::LdsRasterFits(shape, largest_image_size, ctx->lds_raster == 1);
}
int LaunchRenderers(Ctx* ctx, const int* which, int n_which, const int* pairs, int n_pairs, int largest_image_size) {
  if (n_which == 0) return M3T_OK;
  const RenderLaunchShape shape = RenderShape(n_pairs, largest_image_size);
  if (LdsRasterFits(ctx, shape, largest_image_size)) {
    hipLaunchKernelGGL(focused_setup_kernel, dim3(shape.slices, n_pairs), dim3(M3T_BLOCK_THREADS), 0, ctx->stream,
                       ctx->d_renderers.as<RendererDev>(), pairs, ctx->cams_active, ctx->d_poses.as<float>());
    hipLaunchKernelGGL(focused_resolve_kernel, dim3(n_pairs, shape.bands), dim3(M3T_BLOCK_THREADS), shape.lds, ctx->stream,
                       ctx->d_renderers.as<RendererDev>(), pairs);
    HIPCHK(hipGetLastError());
    return M3T_OK;
  }
#ifndef M3T_RASTER_SLICES
#define M3T_RASTER_SLICES m3t_render::kThreeLaunchSlices
#endif
  hipLaunchKernelGGL(focused_clear_kernel, dim3(16, n_which), dim3(M3T_BLOCK_THREADS), 0, ctx->stream,
                     ctx->d_renderers.as<RendererDev>(), which, ctx->cams_active, ctx->d_poses.as<float>());
  hipLaunchKernelGGL(focused_raster_kernel, dim3(M3T_RASTER_SLICES, n_which), dim3(M3T_BLOCK_THREADS), 0, ctx->stream,
                     ctx->d_renderers.as<RendererDev>(), which, ctx->cams_active, ctx->d_poses.as<float>());
  hipLaunchKernelGGL(focused_unpack_kernel, dim3(16, n_which), dim3(M3T_BLOCK_THREADS), 0, ctx->stream,
                     ctx->d_renderers.as<RendererDev>(), which);
  HIPCHK(hipGetLastError());
  return M3T_OK;
}
int LargestRendererImage(Ctx* ctx) {
  int s = 0;
  for (auto& r : ctx->renderers) s = std::max(s, r->image_size);
  return s;
}
int RenderForModalities(Ctx* ctx, bool region_only) {
  for (auto& r : ctx->renderers) r->rendered = true;
  return LaunchRenderers(ctx, region_only ? ctx->d_render_region.as<int>() : ctx->d_render_all.as<int>(),
                         region_only ? ctx->n_render_region : ctx->n_render_all,
                         region_only ? ctx->d_render_region_pairs.as<int>() : ctx->d_render_all_pairs.as<int>(),
                         region_only ? ctx->n_render_region_pairs : ctx->n_render_all_pairs, LargestRendererImage(ctx));
}

// ROI ingest: the readers of every camera (one per modality of a rigid optimizer: which body, which box of model
// points, which reach -- m3t_roi.h) sorted by camera, and where the fused kernels leave their search poses.
// Called while the optimizer table is being rebuilt.
int BuildRoiTables(Ctx* ctx) {
  ctx->n_roi_items = 0;
  ctx->roi_recorded = false;
  ctx->roi_snapshot_valid = false;
  ctx->roi_end_valid = false;
  for (auto& od : ctx->opt_table) od.search_poses = nullptr;
  if (!ctx->roi_enabled || ctx->tree_mode || ctx->opt_table.empty()) return M3T_OK;
  ctx->roi_n_poses = ctx->n_corr_iterations + 2;
  // per object: the poses, then the guard's header (RoiGuardDev: which rows of the reader table are this object's)
  static_assert(sizeof(RoiGuardDev) % 4 == 0, "RoiGuardDev is addressed in floats");
  const size_t per_object = size_t(ctx->roi_n_poses) * 16 + sizeof(RoiGuardDev) / 4;
  HIPCHK(ctx->d_search_poses.alloc(ctx->opt_table.size() * per_object * 4));
  HIPCHK(hipMemset(ctx->d_search_poses.p, 0, ctx->opt_table.size() * per_object * 4));
  ctx->roi_prev = -1;
  std::vector<RoiItemDev> items;
  auto add = [&](int camera, int body, int opt, const Model& model, float reach_px, float reach_m) {
    RoiItemDev it{};
    it.camera = camera;
    it.body = body;
    it.opt = opt;
    for (int k = 0; k < 3; ++k) {
      it.box_min[k] = model.box_min[k];
      it.box_max[k] = model.box_max[k];
    }
    it.reach_px = reach_px;
    it.reach_m = reach_m;
    it.rho = model.box_rho;
    items.push_back(it);
  };
  for (size_t oi = 0; oi < ctx->opt_table.size(); ++oi) {
    RigidOptDev& od = ctx->opt_table[oi];
    od.search_poses = ctx->d_search_poses.as<float>() + oi * per_object;
    if (od.region_modality >= 0) {
      const RegionMod& m = *ctx->region_mods[od.region_modality];
      const Model& model = *ctx->region_models[m.model];
      float reach = m3t_roi_region_histogram_reach(&m.p);
      for (int c = 0; c < ctx->n_corr_iterations; ++c) reach = std::max(reach, m3t_roi_region_line_reach(&m.p, c));
      add(m.camera, od.body, int(oi), model, reach, 0.0f);
      if (m.p.measure_occlusions) {
        float reach_m = 0.0f, reach_px = 0.0f;
        m3t_roi_region_depth_reach(&m.p, &reach_m, &reach_px);
        add(m.depth_camera, od.body, int(oi), model, reach_px, reach_m);
      }
    }
    if (od.depth_modality >= 0) {
      const DepthMod& m = *ctx->depth_mods[od.depth_modality];
      float reach_m = 0.0f, reach_px = 0.0f;
      m3t_roi_depth_reach(&m.p, ctx->cameras[m.camera]->intr.fu, &reach_m, &reach_px);
      add(m.camera, od.body, int(oi), *ctx->depth_models[m.model], reach_px, reach_m);
    }
  }
  std::stable_sort(items.begin(), items.end(), [](const RoiItemDev& a, const RoiItemDev& b) { return a.camera < b.camera; });
  const size_t n_cams = ctx->cameras.size();
  std::vector<int> first(n_cams + 1, 0);
  for (auto& it : items) ++first[size_t(it.camera) + 1];
  for (size_t c = 0; c < n_cams; ++c) first[c + 1] += first[c];
  HIPCHK(UploadTable(&ctx->d_roi_items, items));
  {  // region modality -> its optimizer (region_histogram_kernel behind a guarded step)
    std::vector<int> opt_of(std::max<size_t>(1, ctx->region_mods.size()), -1);
    for (size_t oi = 0; oi < ctx->opt_table.size(); ++oi)
      if (ctx->opt_table[oi].region_modality >= 0) opt_of[size_t(ctx->opt_table[oi].region_modality)] = int(oi);
    HIPCHK(UploadTable(&ctx->d_roi_opt_of_region, opt_of));
  }
  HIPCHK(UploadTable(&ctx->d_roi_item_first, first));
  ctx->n_roi_items = int(items.size());
  // (until a body's motion is known its margin is the caller's)
  HIPCHK(UploadTable(&ctx->d_roi_motion_peak, std::vector<float>(std::max<size_t>(1, items.size()), -1.0f)));
  {  // the guard's headers: every object's readers by their rows in the sorted table
    std::vector<float> blocks(ctx->opt_table.size() * per_object, 0.0f);
    for (size_t j = 0; j < items.size(); ++j) {
      RoiGuardDev* g = reinterpret_cast<RoiGuardDev*>(blocks.data() + size_t(items[j].opt) * per_object + size_t(ctx->roi_n_poses) * 16);
      // (a reader beyond the header's capacity would shrink its camera's upload without any kernel checking it)
      REQUIRE(g->n_items < M3T_ROI_GUARD_ITEMS, M3T_ERR_UNSUPPORTED,
              "ROI ingest: an optimizer has more frame readers than the guard header holds (M3T_ROI_GUARD_ITEMS)");
      g->item[g->n_items++] = int(j);
    }
    HIPCHK(hipMemcpy(ctx->d_search_poses.p, blocks.data(), blocks.size() * 4, hipMemcpyHostToDevice));
  }
  {  // the camera ids in order: a batch of consecutive ids needs no list of its own
    std::vector<int> all(std::max<size_t>(1, n_cams));
    for (size_t c = 0; c < n_cams; ++c) all[c] = int(c);
    HIPCHK(UploadTable(&ctx->d_roi_all_cam_ids, all));
  }
  int slots = 1;
  for (auto& c : ctx->cameras) slots = std::max(slots, c->n_slots);
  ctx->roi_rect_slots = slots;
  ctx->roi_sources.assign(size_t(slots), {});
  HIPCHK(ctx->d_roi_pose_snapshot.alloc(Ctx::kRoiSnapshots * std::max<size_t>(64, ctx->body_poses.size() * 4)));
  for (auto& e : ctx->roi_snapshot_done) HIPCHK(e.Ensure(hipEventDisableTiming));
  {  // what every slot holds now: a whole frame, or (a rectangle from before the rebuild) nothing that can be vouched for
    std::vector<m3t_roi_rect> rects(size_t(slots) * n_cams, m3t_roi_empty());
    for (size_t c = 0; c < n_cams; ++c)
      for (int sl = 0; sl < ctx->cameras[c]->n_slots; ++sl)
        if (!ctx->cameras[c]->slot_is_roi[sl])
          rects[size_t(sl) * n_cams + c] = m3t_roi_rect{0, 0, ctx->cameras[c]->intr.width - 1, ctx->cameras[c]->intr.height - 1};
    HIPCHK(UploadTable(&ctx->d_roi_rects, rects));
  }
  if (!ctx->roi_miss.host) HIPCHK(ctx->roi_miss.Alloc(2 * (Ctx::kRoiMissCapacity + 1) * sizeof(int), kMapped, true));
  return M3T_OK;
}

// whole frames were (or are being, on `stream`) written into the slot of the cameras ids[0 .. n): ONE launch notes
// that in the rectangle table (round 4 launched one single-thread kernel per camera: 64 per batch-frame)
void RoiMarkWholeFrames(Ctx* ctx, const int* ids, int n, int slot, hipStream_t stream) {
  bool consecutive = true;
  for (int i = 0; i < n; ++i) {
    ctx->cameras[ids[i]]->slot_is_roi[slot] = false;
    consecutive = consecutive && ids[i] == ids[0] + i;
  }
  if (slot < int(ctx->roi_sources.size())) {  // the whole frames replace what the rectangles of these cameras came from
    auto& sources = ctx->roi_sources[size_t(slot)];
    for (size_t k = 0; k < sources.size();) {
      bool overlaps = false;
      for (int i = 0; i < n && !overlaps; ++i)
        overlaps = std::find(sources[k].ids.begin(), sources[k].ids.end(), ids[i]) != sources[k].ids.end();
      if (overlaps) sources.erase(sources.begin() + long(k)); else ++k;
    }
  }
  if (!ctx->roi_enabled || ctx->n_roi_items == 0 || slot >= ctx->roi_rect_slots || ctx->tables_dirty) return;
  m3t_roi_rect* rects = ctx->d_roi_rects.as<m3t_roi_rect>() + size_t(slot) * ctx->cameras.size();
  // (a batch is a group of cameras of equal geometry: m3t_hip_cameras_set_ring)
  for (int i = 0; i < n; i += consecutive ? n : 1) {
    const Camera& c = *ctx->cameras[ids[i]];
    hipLaunchKernelGGL(roi_set_rects_kernel, dim3(((consecutive ? n : 1) + 63) / 64), dim3(64), 0, stream, rects, ids[i],
                       consecutive ? n : 1, c.intr.width, c.intr.height);
  }
}
void RoiMarkWholeFrame(Ctx* ctx, int camera, int slot, hipStream_t stream) { RoiMarkWholeFrames(ctx, &camera, 1, slot, stream); }

int UploadTables(Ctx* ctx) {
  HIPCHK(ctx->ingest.JoinPendingCopies(ctx->stream));
  if (ctx->cams_dirty || ctx->tables_dirty || ctx->slots_dirty) {
    // Camera table versions: when every camera has the same number of ring slots, version s holds all cameras
    // looking at slot s, and a frame switch of the whole batch (m3t_hip_cameras_select_slot) only moves the
    // table pointer the kernels receive: nothing is copied between two tracking steps.  Cameras on different
    // slots use the extra version behind them, rebuilt and staged per switch.
    const size_t n_cams = ctx->cameras.size();
    int n_versions = n_cams ? ctx->cameras[0]->n_slots : 0;
    int uniform_slot = n_cams ? ctx->cameras[0]->current : 0;
    for (auto& c : ctx->cameras) {
      if (c->n_slots != n_versions) n_versions = 0;
      if (c->current != uniform_slot) uniform_slot = -1;
    }
    const size_t version_bytes = n_cams * sizeof(CameraDev);
    if (n_versions > 4096 || version_bytes * size_t(n_versions + 1) > (size_t(32) << 20)) n_versions = 0;
    auto fill = [&](CameraDev* out, int slot /* -1: every camera's own current slot */) {
      for (size_t i = 0; i < n_cams; ++i) {
        const Camera& c = *ctx->cameras[i];
        CameraDev& d = out[i];
        d.image = c.frame(slot < 0 ? c.current : slot);
        d.pitch = c.pitch;
        d.width = c.intr.width;
        d.height = c.intr.height;
        d.fu = c.intr.fu; d.fv = c.intr.fv; d.ppu = c.intr.ppu; d.ppv = c.intr.ppv;
        d.depth_scale = c.depth_scale;
        d.slot = slot < 0 ? c.current : slot;
        std::memcpy(d.world2camera, c.world2camera, 64);
      }
    };
    const size_t bytes = version_bytes * size_t(n_versions + 1);
    if (ctx->d_cams.bytes < bytes) {
      HIPCHK(hipStreamSynchronize(ctx->stream));
      HIPCHK(ctx->d_cams.alloc(bytes * 2));
      ctx->cams_dirty = true;
    }
    const bool rebuild = ctx->cams_dirty || ctx->tables_dirty;
    const bool custom = uniform_slot < 0 || n_versions == 0;
    if (n_cams && rebuild && n_versions > 0) {
      // all slot versions at once: rare (set-up, a camera pose change), so a plain blocking copy
      std::vector<CameraDev> all(n_cams * size_t(n_versions));
      for (int v = 0; v < n_versions; ++v) fill(all.data() + size_t(v) * n_cams, v);
      HIPCHK(hipStreamSynchronize(ctx->stream));
      HIPCHK(hipMemcpy(ctx->d_cams.p, all.data(), all.size() * sizeof(CameraDev), hipMemcpyHostToDevice));
    }
    if (n_cams && custom) {
      // one table for cameras on different slots, staged through a small pinned ring: no host sync per switch
      if (ctx->cam_staging.SmallestBlock() < version_bytes) {  // all blocks at once, behind everything that read them
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx->cam_staging.GrowAll(version_bytes));
      }
      void* staged = nullptr;
      int stage = 0;
      HIPCHK(ctx->cam_staging.Acquire(version_bytes, &staged, nullptr, &stage));
      fill(static_cast<CameraDev*>(staged), -1);
      HIPCHK(hipMemcpyAsync(ctx->d_cams.as<uint8_t>() + size_t(n_versions) * version_bytes, staged, version_bytes,
                            hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(ctx->cam_staging.Release(stage, ctx->stream));
    }
    ctx->cams_active = ctx->d_cams.as<CameraDev>() + (custom ? size_t(n_versions) : size_t(uniform_slot)) * n_cams;
    ctx->cams_dirty = false;
    ctx->slots_dirty = false;
  }
  if (ctx->tables_dirty) {
    int rr = UploadRendererTables(ctx);
    if (rr) return rr;
    std::vector<RegionModDev> r(ctx->region_mods.size());
    for (size_t i = 0; i < r.size(); ++i) r[i] = ctx->region_mods[i]->dev;
    std::vector<DepthModDev> d(ctx->depth_mods.size());
    for (size_t i = 0; i < d.size(); ++i) d[i] = ctx->depth_mods[i]->dev;
    HIPCHK(UploadTable(&ctx->d_region, r));
    HIPCHK(UploadTable(&ctx->d_depth, d));
    if (!ctx->texture_mods.empty()) {
      std::vector<TextureModDev> t(ctx->texture_mods.size());
      for (size_t i = 0; i < t.size(); ++i) t[i] = ctx->texture_mods[i]->dev;
      HIPCHK(UploadTable(&ctx->d_texture, t));
    }
    {
      std::vector<TextureModDev> hamming;
      std::vector<TextureL2Dev> l2;
      int words_max = 0;
      ctx->l2_keyframes_max = 0;
      ctx->hamming_keyframes_max = 0;
      ctx->texture_plan_stale = true;
      for (size_t i = 0; i < ctx->texture_mods.size(); ++i) {
        TextureMod& m = *ctx->texture_mods[i];
        if (!m.l2) {
          hamming.push_back(m.dev);
          ctx->hamming_keyframes_max = std::max(ctx->hamming_keyframes_max, m.dev.n_keyframes_max);
          continue;
        }
        TextureL2Dev d{};
        d.modality = int(i);
        d.best = m.best.as<uint32_t>();
        l2.push_back(d);
        words_max = std::max(words_max, m.dev.descriptor_words);
        ctx->l2_keyframes_max = std::max(ctx->l2_keyframes_max, m.dev.n_keyframes_max);
      }
      ctx->n_texture_l2 = int(l2.size());
      ctx->n_texture_hamming = int(hamming.size());
      if (!l2.empty()) {
        HIPCHK(UploadTable(&ctx->d_texture_l2, l2));
        if (!hamming.empty()) HIPCHK(UploadTable(&ctx->d_texture_hamming, hamming));
        ctx->lds_texture_l2 = texture_l2_lds_bytes(words_max);
        // (the attribute belongs to the function, not to this context: the widest descriptor any context can hold)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(texture_match_l2_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   int(texture_l2_lds_bytes(M3T_TEXTURE_L2_MAX_FLOATS))));
      }
    }
    std::vector<TextureDetectorDev> detectors;
    for (size_t i = 0; i < ctx->texture_mods.size(); ++i) {
      TextureMod& m = *ctx->texture_mods[i];
      if (!m.builtin) continue;
      TextureDetectorDev d{};
      d.modality = int(i);
      d.n_features = m.detector.n_features;
      d.fast_threshold = m.detector.fast_threshold;
      d.focused_image_size = m.p.focused_image_size;
      d.radius = 0.5f * ctx->body_geometries[m.body]->maximum_body_diameter;
      d.features = m.features.as<uint32_t>();
      d.focused = m.focused.as<uint8_t>();
      d.scores = m.scores.as<uint16_t>();
      d.boxes = m.boxes.as<uint16_t>();
      d.header = m.detector_header.as<int>();
      detectors.push_back(d);
    }
    ctx->n_detectors = int(detectors.size());
    if (!detectors.empty()) HIPCHK(UploadTable(&ctx->d_detectors, detectors));
    // kinematic structures (m3t_links.hip) as soon as one optimizer is more than a free rigid body
    ctx->tree_mode = !ctx->texture_mods.empty();  // a texture modality: the general path, one launch per sub-step
    for (auto& o : ctx->optimizers) {
      if (!ctx->links[o.link].simple || !ctx->links[o.link].children.empty() || !o.constraints.empty() ||
          !o.soft_constraints.empty())
        ctx->tree_mode = true;
      // a body seen by several cameras carries several modalities of one kind; the rigid table holds one region
      // and one depth modality per body, the link kernels sum any number (Link::CalculateGradientAndHessian,
      // link.cpp:184-193, in the order they were added)
      int n_region = 0, n_depth = 0;
      for (int mid : ctx->links[o.link].modalities) {
        const ModalityKind kind = ctx->modalities[mid].kind;
        if (kind == kTextureModality) ctx->tree_mode = true;  // the link kernels sum its g/H like any other
        else (kind == kRegionModality ? n_region : n_depth) += 1;
      }
      if (n_region > 1 || n_depth > 1) ctx->tree_mode = true;
    }
    if (ctx->tree_mode) {
      int r = UploadTreeTables(ctx);
      if (r) return r;
    }
    // optimizer table
    ctx->opt_table.clear();
    bool depth_table_changed = false;
    ctx->fused_possible = !ctx->optimizers.empty() && !ctx->tree_mode;
    std::vector<char> body_used(ctx->body_poses.size() / 16, 0);
    for (auto& o : ctx->optimizers) {
      if (ctx->tree_mode) break;
      const Link& l = ctx->links[o.link];
      RigidOptDev od{};
      od.body = l.body;
      od.region_modality = -1;
      od.depth_modality = -1;
      od.tikhonov_rotation = o.tr;
      od.tikhonov_translation = o.tt;
      for (int mid : l.modalities) {
        const ModalityRef& ref = ctx->modalities[mid];
        if (ref.kind == kRegionModality) od.region_modality = ref.index;
        else od.depth_modality = ref.index;
      }
      if (od.region_modality >= 0 && od.depth_modality >= 0) {
        const RegionMod& rmod = *ctx->region_mods[od.region_modality];
        DepthMod& dmod = *ctx->depth_mods[od.depth_modality];
        const Model& a = *ctx->region_models[rmod.model];
        const Model& b = *ctx->depth_models[dmod.model];
        const bool shared = a.h_orientations == b.h_orientations &&
                            std::memcmp(ctx->cameras[rmod.camera]->world2camera, ctx->cameras[dmod.camera]->world2camera, 64) == 0;
        if (dmod.dev.view_search_shared != (shared ? 1 : 0)) {
          dmod.dev.view_search_shared = shared ? 1 : 0;
          depth_table_changed = true;
        }
      }
      if (body_used[l.body]) ctx->fused_possible = false;
      body_used[l.body] = 1;
      ctx->opt_table.push_back(od);
    }
    // the fused kernel iterates optimizers; every modality must hang on exactly one of them
    size_t attached = 0;
    for (auto& o : ctx->optimizers) attached += ctx->links[o.link].modalities.size();
    if (attached != ctx->modalities.size()) ctx->fused_possible = false;
    // renderer-fed branches read other bodies' poses between the sub-steps: one launch per sub-step
    ctx->fused_per_search_possible = ctx->fused_possible && ctx->n_render_all > 0;
    if (ctx->n_render_all > 0) ctx->fused_possible = false;
    // the histogram update can ride in the tracking launch when every region modality sits alone on its
    // optimizer, owns its histograms, and the count table fits the LDS
    ctx->fuse_histogram_possible = ctx->fused_possible && !ctx->region_mods.empty();
    for (auto& m : ctx->region_mods)
      if (m->shared_histograms >= 0) ctx->fuse_histogram_possible = false;
    if (depth_table_changed) {
      for (size_t i = 0; i < d.size(); ++i) d[i] = ctx->depth_mods[i]->dev;
      HIPCHK(hipMemcpy(ctx->d_depth.p, d.data(), d.size() * sizeof(DepthModDev), hipMemcpyHostToDevice));
    }
    {
      int r = BuildRoiTables(ctx);  // (sets RigidOptDev::search_poses)
      if (r) return r;
    }
    HIPCHK(UploadTable(&ctx->d_opts, ctx->opt_table));
    ComputeLayout(ctx);
    size_t max_lds = std::max(std::max(ctx->lds_track, ctx->lds_hist), ctx->lds_depth);
    REQUIRE(max_lds <= 160 * 1024, M3T_ERR_UNSUPPORTED,
            "per-object working set exceeds the 160 KB LDS of a CU");
    if (!ctx->hist_counts_in_lds) ctx->fuse_histogram_possible = false;
    // the compact kernel: the reference's default function / distribution lengths, unrolled scales, a thread per line
    ctx->compact_possible = ctx->fused_possible && ctx->lds_compact <= 80 * 1024;
    for (auto& m : ctx->region_mods) {
      if (m->p.function_length != 8 || m->p.distribution_length != 12 || m->p.n_lines_max > M3T_COMPACT_THREADS)
        ctx->compact_possible = false;
      for (int i = 0; i < m->p.n_scales; ++i)
        if (m->p.scales[i] < 1 || m->p.scales[i] > 9) ctx->compact_possible = false;
      // (the LDS pair table is laid out for ONE histogram size, each modality's own table, no shared ColorHistograms)
      if (m->p.n_histogram_bins != ctx->region_mods[0]->p.n_histogram_bins || m->shared_histograms >= 0)
        ctx->lds_compact_table = 0;
    }
    // the split kernel: free rigid bodies with their own histograms (the pair table is read from L2)
    ctx->split_possible = ctx->fused_possible;
    for (auto& m : ctx->region_mods)
      if (m->shared_histograms >= 0 || m->p.n_histogram_bins < 4) ctx->split_possible = false;
    // the dynamic LDS each kernel may be launched with
    auto fn = [](auto* kernel) { return reinterpret_cast<const void*>(kernel); };
    using Kernels = std::vector<const void*>;
    const struct {
      Kernels kernels;
      size_t bytes;
    } lds_groups[] = {
        {{fn(tracking_step_compact_kernel), fn(tracking_step_compact_wide_kernel)}, ctx->lds_compact},
        {ctx->lds_compact_table ? Kernels{fn(tracking_step_compact_table_kernel)} : Kernels{}, ctx->lds_compact_table},
        {{fn(tracking_step_split_kernel), fn(tracking_step_split_moments_kernel), fn(tracking_step_split_render_kernel),
          fn(tracking_step_split_pair_kernel), fn(tracking_step_pair_kernel), fn(tracking_step_lds_pair_kernel),
          fn(tracking_step_kernel), fn(tracking_step_lds_kernel)},
         std::max(ctx->lds_track, ctx->lds_hist)},
        {{fn(region_correspondence_kernel), fn(region_correspondence_lds_kernel), fn(region_gradient_hessian_kernel)},
         ctx->lds_corr},
        {{fn(region_histogram_kernel), fn(region_histogram_list_kernel), fn(region_histogram_flagged_kernel)},
         ctx->lds_hist},
        {{fn(depth_correspondence_kernel), fn(depth_gradient_hessian_kernel)}, ctx->lds_depth},
    };
    for (const auto& group : lds_groups)
      for (const void* kernel : group.kernels)
        HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(group.bytes)));
    ctx->tables_dirty = false;
  }
  if (ctx->texture_plan_stale) {  // the Hamming matcher's form; the tiled one needs its scratch (m3t_texture_plan.h)
    ctx->texture_plan = m3t_texture::PlanMatch(ctx->texture_match_mode, ctx->n_texture_hamming, ctx->hamming_keyframes_max);
    if (ctx->texture_plan.form == m3t_texture::kTiled) {
      std::vector<uint32_t*> best;
      for (auto& m : ctx->texture_mods) {
        if (m->l2) continue;
        if (m->best.bytes < ctx->texture_plan.scratch_bytes) HIPCHK(m->best.alloc(ctx->texture_plan.scratch_bytes));
        best.push_back(m->best.as<uint32_t>());
      }
      HIPCHK(UploadTable(&ctx->d_texture_best, best));
    }
    ctx->texture_plan_stale = false;
  }
  size_t n_bodies = ctx->body_poses.size() / 16;
  if (ctx->pose_capacity < n_bodies) {
    // keep device poses if they are newer than the host mirror
    if (!ctx->poses_dirty_host && ctx->pose_capacity > 0) {
      std::vector<float> tmp(ctx->pose_capacity * 16);
      HIPCHK(hipMemcpy(tmp.data(), ctx->d_poses.p, tmp.size() * 4, hipMemcpyDeviceToHost));
      std::memcpy(ctx->body_poses.data(), tmp.data(), tmp.size() * 4);
    }
    HIPCHK(ctx->d_poses.alloc(std::max<size_t>(1, n_bodies) * 64 * 2));
    ctx->pose_capacity = ctx->d_poses.bytes / 64;
    ctx->poses_dirty_host = true;
  }
  if (ctx->poses_dirty_host && n_bodies) {
    HIPCHK(hipMemcpyAsync(ctx->d_poses.p, ctx->body_poses.data(), n_bodies * 64, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->poses_dirty_host = false;
  }
  return M3T_OK;
}

int CheckImages(Ctx* ctx) {
  for (auto& m : ctx->region_mods) {
    const Camera& c = *ctx->cameras[m->camera];
    REQUIRE(c.has_image[c.current], M3T_ERR_NOT_SET_UP, "Set up color camera first (no image uploaded)");
    if (m->p.measure_occlusions) {
      const Camera& d = *ctx->cameras[m->depth_camera];
      REQUIRE(d.has_image[d.current], M3T_ERR_NOT_SET_UP, "Set up depth camera first (no image uploaded)");
    }
  }
  for (auto& m : ctx->depth_mods) {
    const Camera& d = *ctx->cameras[m->camera];
    REQUIRE(d.has_image[d.current], M3T_ERR_NOT_SET_UP, "Set up depth camera first (no image uploaded)");
  }
  for (auto& m : ctx->texture_mods) {  // (the colour frame is the detector's: the caller's, or the built-in one's)
    if (m->builtin) {
      const Camera& c = *ctx->cameras[m->camera];
      REQUIRE(c.has_image[c.current], M3T_ERR_NOT_SET_UP, "Set up color camera first (no image uploaded)");
    }
    if (!m->p.measure_occlusions) continue;
    const Camera& d = *ctx->cameras[m->depth_camera];
    REQUIRE(d.has_image[d.current], M3T_ERR_NOT_SET_UP, "Set up depth camera first (no image uploaded)");
  }
  return M3T_OK;
}

struct ScopedKernelTimer {
  Ctx* ctx;
  int which;
  EventPair events;
  ScopedKernelTimer(Ctx* c, int w) : ctx(c), which(w) {
    if (ctx->timing_region) ctx->kernel_launches[w] += 1;  // (no event between the launches)
    if (!ctx->timing || events.Ensure(hipEventDefault) != hipSuccess) return;
    (void)hipEventRecord(events.a.get(), ctx->stream);
  }
  ~ScopedKernelTimer() {
    if (!events) return;
    (void)hipEventRecord(events.b.get(), ctx->stream);
    ctx->pending.push_back({std::move(events), which});
  }
};

int LaunchHistogram(Ctx* ctx, int iteration, bool initialize, bool behind_guarded_step = false) {
  int n = int(ctx->region_mods.size());
  if (n == 0) return M3T_OK;
  ScopedKernelTimer timer(ctx, 1);
  const bool guarded = behind_guarded_step && ctx->d_roi_opt_of_region.p != nullptr && !ctx->opt_table.empty();
  hipLaunchKernelGGL(region_histogram_kernel, dim3(n), dim3(M3T_BLOCK_THREADS), ctx->lds_hist, ctx->stream,
                     ctx->d_region.as<RegionModDev>(), ctx->cams_active, ctx->d_poses.as<float>(), iteration,
                     initialize ? 1 : 0, ctx->hist_counts_in_lds ? 1 : 0,
                     guarded ? ctx->d_opts.as<RigidOptDev>() : (const RigidOptDev*)nullptr,
                     guarded ? ctx->d_roi_opt_of_region.as<int>() : (const int*)nullptr, ctx->roi_n_poses);
  if (!ctx->shared_histograms.empty())  // Initialize / UpdateHistograms of the shared objects, tracker.cpp:441-443,513-515
    hipLaunchKernelGGL(shared_histogram_finish_kernel, dim3(unsigned(ctx->shared_histograms.size())),
                       dim3(M3T_BLOCK_THREADS), 0, ctx->stream, ctx->d_shared_histograms.as<SharedHistogramsDev>(),
                       initialize ? 1 : 0);
  HIPCHK(hipGetLastError());
  return M3T_OK;
}

// DetectAndComputeCorrKeypoints (texture_modality.cpp:858-888) of the texture modalities with a built-in detector, on
// the colour camera's current frame at the pose the device holds
int LaunchTextureDetection(Ctx* ctx) {
  const int n = ctx->n_detectors;
  if (n == 0) return M3T_OK;
  const dim3 bands(n, M3T_TEXTURE_FOCUSED_MAX / M3T_FEATURE_BAND);
  const TextureDetectorDev* detectors = ctx->d_detectors.as<TextureDetectorDev>();
  hipLaunchKernelGGL(texture_focus_kernel, bands, dim3(kFeatureThreads), 0, ctx->stream, detectors,
                     ctx->d_texture.as<TextureModDev>(), ctx->cams_active, ctx->d_poses.as<float>());
  hipLaunchKernelGGL(texture_fast_kernel, bands, dim3(kFeatureThreads), 0, ctx->stream, detectors);
  hipLaunchKernelGGL(texture_describe_kernel, dim3(n), dim3(kDescribeThreads), 0, ctx->stream, detectors);
  HIPCHK(hipGetLastError());
  return M3T_OK;
}

// TextureModality::StartModality (decide = false) / CalculateResults (decide = true), behind their renderers
int LaunchTextureKeyframes(Ctx* ctx, bool decide) {
  const int nt = int(ctx->texture_mods.size());
  if (nt == 0) return M3T_OK;
  hipLaunchKernelGGL(texture_keyframe_kernel, dim3(nt), dim3(M3T_TEXTURE_MATCH_THREADS), 0, ctx->stream,
                     ctx->d_texture.as<TextureModDev>(), ctx->cams_active, ctx->d_poses.as<float>(), decide ? 1 : 0);
  HIPCHK(hipGetLastError());
  return M3T_OK;
}

int LaunchCorrespondences(Ctx* ctx, int iteration, int corr_iteration) {
  int nr = int(ctx->region_mods.size()), nd = int(ctx->depth_mods.size());
  if (!ctx->texture_mods.empty()) {
    if (corr_iteration == 0) {  // :334
      const int r = LaunchTextureDetection(ctx);
      if (r) return r;
    }
    const int match = corr_iteration == 0 ? 1 : 0;
    // the Hamming matcher sees the Hamming modalities alone: the whole table, or beside L2 modalities their own one;
    // its form -- one workgroup a modality, or tiled over ring slots and queries with the collect pass behind it, which
    // at corr_iteration > 0 runs alone -- is the plan's (m3t_texture_plan.h, made by UploadTables)
    const m3t_texture::MatchPlan& plan = ctx->texture_plan;
    const TextureModDev* hamming = (ctx->n_texture_l2 == 0 ? ctx->d_texture : ctx->d_texture_hamming).as<TextureModDev>();
    if (plan.form == m3t_texture::kOneWorkgroup) {
      hipLaunchKernelGGL(texture_match_kernel, dim3(plan.match.x, plan.match.y), dim3(M3T_TEXTURE_MATCH_THREADS), 0, ctx->stream,
                         hamming, ctx->cams_active, ctx->d_poses.as<float>(), match);
    } else if (plan.form == m3t_texture::kTiled) {
      uint32_t* const* best = ctx->d_texture_best.as<uint32_t*>();
      if (match)
        hipLaunchKernelGGL(texture_match_tiled_kernel, dim3(plan.match.x, plan.match.y), dim3(M3T_TEXTURE_MATCH_THREADS), 0,
                           ctx->stream, hamming, best);
      hipLaunchKernelGGL(texture_collect_kernel, dim3(plan.collect.x, plan.collect.y), dim3(M3T_TEXTURE_MATCH_THREADS), 0,
                         ctx->stream, hamming, best, ctx->cams_active, ctx->d_poses.as<float>(), match);
    }
    if (ctx->n_texture_l2) {
      // the L2 modalities' match is tiled over keyframes and queries (texture_match_l2_kernel, which finds on the device
      // what it has to do) with the ratio test, the data points and the projection behind it -- at corr_iteration > 0
      // the projection alone
      const TextureL2Dev* l2 = ctx->d_texture_l2.as<TextureL2Dev>();
      if (match)
        hipLaunchKernelGGL(texture_match_l2_kernel, dim3(ctx->n_texture_l2, ctx->l2_keyframes_max * kL2QueryTiles),
                           dim3(M3T_TEXTURE_MATCH_THREADS), ctx->lds_texture_l2, ctx->stream, l2,
                           ctx->d_texture.as<TextureModDev>());
      hipLaunchKernelGGL(texture_collect_l2_kernel, dim3(ctx->n_texture_l2), dim3(M3T_TEXTURE_MATCH_THREADS), 0, ctx->stream,
                         l2, ctx->d_texture.as<TextureModDev>(), ctx->cams_active, ctx->d_poses.as<float>(), match);
    }
    HIPCHK(hipGetLastError());
  }
  if (nr) {
    hipLaunchKernelGGL(ctx->layout.off_hist >= 0 ? region_correspondence_lds_kernel : region_correspondence_kernel,
                       dim3(nr), dim3(M3T_BLOCK_THREADS), ctx->lds_corr, ctx->stream,
                       ctx->d_region.as<RegionModDev>(), ctx->cams_active, ctx->d_poses.as<float>(),
                       ctx->layout, iteration, corr_iteration);
    HIPCHK(hipGetLastError());
  }
  if (nd) {
    hipLaunchKernelGGL(depth_correspondence_kernel, dim3(nd), dim3(M3T_BLOCK_THREADS), ctx->lds_depth, ctx->stream,
                       ctx->d_depth.as<DepthModDev>(), ctx->cams_active, ctx->d_poses.as<float>(),
                       ctx->np_max, iteration, corr_iteration);
    HIPCHK(hipGetLastError());
  }
  return M3T_OK;
}

int LaunchGradientHessian(Ctx* ctx, int corr_iteration, int opt_iteration) {
  int nr = int(ctx->region_mods.size()), nd = int(ctx->depth_mods.size());
  if (const int nt = int(ctx->texture_mods.size())) {
    hipLaunchKernelGGL(texture_gradient_hessian_kernel, dim3(nt), dim3(M3T_TEXTURE_MATCH_THREADS), 0, ctx->stream,
                       ctx->d_texture.as<TextureModDev>(), ctx->cams_active, ctx->d_poses.as<float>(), corr_iteration);
    HIPCHK(hipGetLastError());
  }
  if (nr) {
    hipLaunchKernelGGL(region_gradient_hessian_kernel, dim3(nr), dim3(M3T_BLOCK_THREADS), ctx->lds_corr, ctx->stream,
                       ctx->d_region.as<RegionModDev>(), ctx->cams_active, ctx->d_poses.as<float>(),
                       ctx->layout, corr_iteration, opt_iteration);
    HIPCHK(hipGetLastError());
  }
  if (nd) {
    hipLaunchKernelGGL(depth_gradient_hessian_kernel, dim3(nd), dim3(M3T_BLOCK_THREADS), ctx->lds_depth, ctx->stream,
                       ctx->d_depth.as<DepthModDev>(), ctx->cams_active, ctx->d_poses.as<float>(),
                       ctx->np_max, corr_iteration);
    HIPCHK(hipGetLastError());
  }
  return M3T_OK;
}

int LaunchProject(Ctx* ctx) {
  int n = int(ctx->optimizers.size());
  if (n == 0) return M3T_OK;
  hipLaunchKernelGGL(links_project_kernel, dim3(n), dim3(64), ctx->tree_lds, ctx->stream,
                     ctx->d_treeopts.as<TreeOptDev>(), n, ctx->d_poses.as<float>(), ctx->tree_lds ? 1 : 0);
  HIPCHK(hipGetLastError());
  ctx->partial_ready = true;
  return M3T_OK;
}
int LaunchSolve(Ctx* ctx, bool zero_theta) {
  int n = int(ctx->optimizers.size());
  if (n == 0) return M3T_OK;
  hipLaunchKernelGGL(links_solve_kernel, dim3(n), dim3(64), ctx->tree_lds, ctx->stream,
                     ctx->d_treeopts.as<TreeOptDev>(), n, ctx->d_poses.as<float>(), zero_theta ? 1 : 0,
                     ctx->tree_lds ? 1 : 0);
  HIPCHK(hipGetLastError());
  ctx->links_device_newer = true;
  ctx->partial_ready = false;
  return M3T_OK;
}

// The two halves around the exchange of a structure spread over processes (m3t_links.hip): the link sums of this
// process's modalities, and everything else of Optimizer::CalculateOptimization from the summed link sums
int LaunchGather(Ctx* ctx) {
  int n = int(ctx->optimizers.size());
  if (n == 0) return M3T_OK;
  hipLaunchKernelGGL(links_gather_kernel, dim3(n), dim3(64), 0, ctx->stream, ctx->d_treeopts.as<TreeOptDev>(), n,
                     ctx->d_link_sums.as<float>(), ctx->d_link_first.as<int>());
  HIPCHK(hipGetLastError());
  ctx->partial_ready = true;
  return M3T_OK;
}
int LaunchSolveSums(Ctx* ctx) {
  int n = int(ctx->optimizers.size());
  if (n == 0) return M3T_OK;
  hipLaunchKernelGGL(links_solve_sums_kernel, dim3(n), dim3(64), ctx->tree_lds, ctx->stream,
                     ctx->d_treeopts.as<TreeOptDev>(), n, ctx->d_poses.as<float>(), 0, ctx->tree_lds ? 1 : 0,
                     ctx->d_link_sums.as<float>(), ctx->d_link_first.as<int>());
  HIPCHK(hipGetLastError());
  ctx->links_device_newer = true;
  ctx->partial_ready = false;
  return M3T_OK;
}

// sum of the stacked link sums ([links of all structures][6 + 36]) over the ranks of the communicator: ONE
// ncclAllReduce on the context's stream, in place.  Exact: every link's modalities live on one rank, the others add
// +0.0 (m3t_links.hip, links_gather_kernel)
int AllReducePartial(Ctx* ctx, float* buffer = nullptr) {
  REQUIRE(ctx->partial_ready, M3T_ERR_NOT_SET_UP, "calculate_optimization_begin has to be called first");
  REQUIRE(ctx->Distributed(), M3T_ERR_NOT_SET_UP,
          "no communicator: m3t_hip_comm_init_rank / m3t_hip_comm_set / m3t_hip_comm_set_reduce_callback first");
  if (!buffer) buffer = ctx->d_link_sums.as<float>();
  if (ctx->reduce_fn) {  // the host's transport: leaves the sum over its ranks in the buffer, in stream order
    const int rc = ctx->reduce_fn(ctx->reduce_user, buffer, ctx->link_sums_count, static_cast<void*>(ctx->stream));
    if (rc != 0) return Fail(ctx, M3T_ERR_DEVICE, "the reduce callback failed with code " + std::to_string(rc));
    ++ctx->allreduce_calls;
    return M3T_OK;
  }
  const ncclResult_t rc =
      g_rccl.AllReduce(buffer, buffer, ctx->link_sums_count, ncclFloat, ncclSum, ctx->comm, ctx->stream);
  if (rc != ncclSuccess)
    return Fail(ctx, M3T_ERR_DEVICE,
                std::string("ncclAllReduce: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error"));
  ++ctx->allreduce_calls;
  return M3T_OK;
}

// Optimizer::CalculateOptimization for every optimizer.  With a communicator set the structures span GPUs
// (SURVEY 8e): link sums -> ONE all-reduce of them -> project + solve, on every path that reaches this function
// (m3t_hip_calculate_optimization and the sub-step loop of m3t_hip_execute_tracking_step alike).
int LaunchOptimization(Ctx* ctx) {
  if (ctx->Distributed()) {
    if (!ctx->tree_mode) {  // rigid bodies only: force the general path so that the sums exist
      ctx->tree_mode = true;
      ctx->fused_possible = false;
      int r = UploadTreeTables(ctx);
      if (r) return r;
    }
    int r = LaunchGather(ctx);
    if (r) return r;
    if ((r = AllReducePartial(ctx))) return r;
    return LaunchSolveSums(ctx);
  }
  if (ctx->tree_mode) {
    int r = LaunchProject(ctx);
    if (r) return r;
    return LaunchSolve(ctx, false);
  }
  int n = int(ctx->opt_table.size());
  if (n == 0) return M3T_OK;
  hipLaunchKernelGGL(rigid_optimize_kernel, dim3(n), dim3(64), 0, ctx->stream,
                     ctx->d_opts.as<RigidOptDev>(), n, ctx->d_region.as<RegionModDev>(),
                     ctx->d_depth.as<DepthModDev>(), ctx->d_poses.as<float>());
  HIPCHK(hipGetLastError());
  return M3T_OK;
}

// LDS of one workgroup of tracking_step_tree_kernel: the tracking carve-up (or the histogram update's count table,
// whichever is larger) with the structure block behind it
size_t TreeStepLds(Ctx* ctx, bool fused_histogram) {
  const size_t front = fused_histogram ? std::max(ctx->lds_track, ctx->lds_hist) : ctx->lds_track;
  return (front + 15) / 16 * 16 + ctx->tree_block_floats * 4;
}
// Can this step run as ONE launch of tracking_step_tree_kernel?  Needs: kinematic structures whose modalities sit on
// links (at most one region and one depth modality per link), no renderer-fed branches, no communicator, no shared
// histogram objects, line / point state not requested (fused mode 1), fewer than 63 Newton steps per frame, the
// structure copy next to the tracking carve-up in LDS, and every workgroup of the grid resident at once.
bool TreeStepFused(Ctx* ctx, const m3t_step::StepOverrides& overrides) {
  // (m3t_hip_set_object_split(ctx, 0) = "this context shares its GPU": no launch whose workgroups wait for each other)
  if (!(ctx->tree_mode && ctx->tree_fused_possible && ctx->fused_mode == 1 && !ctx->Distributed() && ctx->n_render_all == 0 &&
        ctx->shared_histograms.empty() && ctx->n_treesteps > 0 && ctx->split_enabled &&
        !overrides.no_tree_fusion))
    return false;
  if (ctx->layout.off_hist >= 0) return false;  // (the LDS-staged pair table belongs to tracking_step_lds_kernel)
  if (ctx->n_corr_iterations * ctx->n_update_iterations >= 63) return false;
  const bool fused_histogram = !ctx->region_mods.empty() && ctx->hist_counts_in_lds;
  const size_t lds = TreeStepLds(ctx, fused_histogram);
  if (lds > size_t(160) * 1024) return false;
  auto kernel = ctx->tree_constrained ? tracking_step_tree_constrained_kernel : tracking_step_tree_kernel;
  if (ctx->tree_lds_attribute != lds || ctx->tree_lds_kernel != reinterpret_cast<const void*>(kernel)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            int(lds)) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    ctx->tree_lds_attribute = lds;
    ctx->tree_lds_kernel = reinterpret_cast<const void*>(kernel);
  }
  int resident = ResidentBlocks(ctx, kernel, M3T_BLOCK_THREADS, lds);
  resident = std::min(resident, int(size_t(160) * 1024 / lds));
  return resident >= 1 && ctx->n_treesteps <= ctx->compute_cus * resident;
}

// A structure spread over processes (a communicator is set): can the step run as ONE launch + ONE all-reduce per
// Newton step (tracking_step_tree_segment_kernel)?  The conditions of the one-launch step, except that no workgroup
// waits for another one inside a launch: no co-residency needed, any grid.
bool TreeStepSegmented(Ctx* ctx, const m3t_step::StepOverrides& overrides) {
  if (!(ctx->tree_mode && ctx->tree_fused_possible && ctx->fused_mode == 1 && ctx->Distributed() && ctx->n_render_all == 0 &&
        ctx->shared_histograms.empty() && ctx->n_treesteps > 0 && !overrides.no_tree_segments))
    return false;
  // a structure's solve is done by the workgroups of its tracked links: one whose modalities all live on other ranks
  // has none here, and still has to be solved from the summed link sums -> the per-sub-step launches (grid = structures)
  if (ctx->tree_untracked_structure) return false;
  if (ctx->layout.off_hist >= 0) return false;
  const bool fused_histogram = !ctx->region_mods.empty() && ctx->hist_counts_in_lds;
  const size_t lds = TreeStepLds(ctx, fused_histogram);
  if (lds > size_t(160) * 1024) return false;
  auto kernel = ctx->tree_constrained ? tracking_step_tree_segment_constrained_kernel : tracking_step_tree_segment_kernel;
  if (ctx->tree_segment_lds_attribute != lds || ctx->tree_segment_lds_kernel != reinterpret_cast<const void*>(kernel)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            int(lds)) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    ctx->tree_segment_lds_attribute = lds;
    ctx->tree_segment_lds_kernel = reinterpret_cast<const void*>(kernel);
  }
  return true;
}

// tracked: the caller's launches read no frames, or it marks them as readers itself (Ingest::MarkRead) -- the launches of
// every other caller are behind no step event, and the next asynchronous upload waits for the whole compute stream
int Prepare(Ctx* ctx, bool need_images, bool tracked = false) {
  if (!tracked) ctx->ingest.LaunchedUntracked();
  if (need_images) {
    int r = CheckImages(ctx);
    if (r) return r;
  }
  return UploadTables(ctx);
}

RegionMod* GetRegion(Ctx* ctx, int id) {
  if (id < 0 || id >= int(ctx->modalities.size()) || ctx->modalities[id].kind != kRegionModality) return nullptr;
  return ctx->region_mods[ctx->modalities[id].index].get();
}
DepthMod* GetDepth(Ctx* ctx, int id) {
  if (id < 0 || id >= int(ctx->modalities.size()) || ctx->modalities[id].kind != kDepthModality) return nullptr;
  return ctx->depth_mods[ctx->modalities[id].index].get();
}
TextureMod* GetTexture(Ctx* ctx, int id) {
  if (id < 0 || id >= int(ctx->modalities.size()) || ctx->modalities[id].kind != kTextureModality) return nullptr;
  return ctx->texture_mods[ctx->modalities[id].index].get();
}

// ---- what the enqueued calls share (m3t_hip_reset_bodies, m3t_hip_reset_structures, m3t_hip_judge_bodies): validate ->
// collect -> BeginEnqueued -> acquire a block of a MappedRing and fill it (m3t_call_args.h) -> launches -> host mirrors
// -> EndEnqueued

// n ids below limit, none of them twice; listed: the mask of those named
int CheckListedIds(Ctx* ctx, const char* entry, const int* ids, int n, int limit, const char* what, std::vector<char>* listed) {
  listed->assign(size_t(limit), 0);
  for (int i = 0; i < n; ++i) {
    REQUIRE(ids[i] >= 0 && ids[i] < limit, M3T_ERR_INVALID_ARGUMENT, std::string(entry) + ": bad " + what + " id");
    REQUIRE(!(*listed)[size_t(ids[i])], M3T_ERR_INVALID_ARGUMENT,
            std::string(entry) + (std::strchr("aeiou", what[0]) ? ": an " : ": a ") + what + " id is listed twice");
    (*listed)[size_t(ids[i])] = 1;
  }
  return M3T_OK;
}
// What the modalities of the listed bodies read: region and texture modalities in table order, their start-modality
// renderers (the region modalities' first) and shared ColorHistograms (each once, in the order met), the cameras of all
// their modalities (as often as read).
struct BodiesRead { std::vector<int> region_ids, renderer_ids, cameras, shared_ids, texture_ids; };
BodiesRead CollectReads(Ctx* ctx, const std::vector<char>& listed) {
  BodiesRead out;
  auto add_once = [](std::vector<int>* v, int id) {
    if (id >= 0 && std::find(v->begin(), v->end(), id) == v->end()) v->push_back(id);
  };
  for (size_t i = 0; i < ctx->region_mods.size(); ++i) {
    const RegionMod& m = *ctx->region_mods[i];
    if (!listed[size_t(m.body)]) continue;
    add_once(&out.shared_ids, m.shared_histograms);
    out.region_ids.push_back(int(i));
    out.cameras.push_back(m.camera);
    if (m.depth_camera >= 0) out.cameras.push_back(m.depth_camera);
    add_once(&out.renderer_ids, m.dev.model_occlusions ? m.depth_renderer : -1);
    add_once(&out.renderer_ids, m.dev.use_region_checking ? m.silhouette_renderer : -1);
  }
  for (auto& m : ctx->depth_mods)
    if (listed[size_t(m->body)]) out.cameras.push_back(m->camera);
  for (size_t i = 0; i < ctx->texture_mods.size(); ++i) {  // start_modality_renderer_ptrs :516-524
    const TextureMod& m = *ctx->texture_mods[i];
    if (!listed[size_t(m.body)]) continue;
    out.texture_ids.push_back(int(i));
    out.cameras.push_back(m.camera);
    if (m.p.measure_occlusions) out.cameras.push_back(m.depth_camera);
    add_once(&out.renderer_ids, m.silhouette_renderer);
    add_once(&out.renderer_ids, m.dev.model_occlusions ? m.depth_renderer : -1);
  }
  return out;
}
// A reset restarts a body's modalities from the host's side of the boundary; the restart of a texture modality that is
// fed by the caller needs the caller's detector on the frame at the new pose (StartModality :315-322), which no enqueued
// call can run.  One with the built-in detector (m3t_features.hip) is restarted on the device -- unless the entry
// restarts none (with_detector_too: m3t_hip_reset_structures).
int RefuseTextureBodies(Ctx* ctx, const std::vector<char>& listed, const char* entry, bool with_detector_too = false) {
  for (auto& m : ctx->texture_mods)
    REQUIRE(!listed[size_t(m->body)] || (m->builtin && !with_detector_too), M3T_ERR_UNSUPPORTED,
            std::string(entry) + ": a listed body has a texture modality (set the pose, set the features of the frame "
            "and call start_modalities)");
  return M3T_OK;
}
// Launches outside the fused step read the current frames of these cameras unguarded: outside the trackers' rectangle a
// slot filled by ROI ingest holds whatever an earlier frame left there, and a body reset between two steps reads its
// histogram pixels away from the rectangle of its old pose.  Refused: the caller uploads the whole frame first (m3t_hip.h).
template <typename Cameras>
int RefuseRoiFrames(Ctx* ctx, const Cameras& cameras, const char* entry) {
  for (int c : cameras)
    REQUIRE(c < 0 || !ctx->cameras[c]->slot_is_roi[ctx->cameras[c]->current], M3T_ERR_UNSUPPORTED,
            std::string(entry) + ": a frame slot the modalities read holds the trackers' rectangle only (ROI ingest); "
            "upload the whole frame into it first (camera_upload_slot)");
  return M3T_OK;
}
// ... for the sub-steps outside the fused step (start_modalities, calculate_correspondences, calculate_results)
int RequireWholeFrames(Ctx* ctx, const char* entry) {
  int r = M3T_OK;
  for (auto& m : ctx->region_mods)
    if ((r = RefuseRoiFrames(ctx, std::array<int, 2>{m->camera, m->depth_camera}, entry))) return r;
  for (auto& m : ctx->depth_mods)
    if ((r = RefuseRoiFrames(ctx, std::array<int, 1>{m->camera}, entry))) return r;
  return M3T_OK;
}
// (tables and poses that were waiting for their upload anyway)  changes_state: not a judgement without reset
int BeginEnqueued(Ctx* ctx, bool changes_state) {
  HIPCHK(hipSetDevice(ctx->device));
  if (changes_state && ctx->poses_dirty_host) ctx->roi_end_valid = false;  // poses set by the host: the last step's end no longer vouches for them
  return Prepare(ctx, changes_state, true);  // reads poses only, or is marked as a reader by EndEnqueued
}
// cameras: whose current frames the call's launches read (null: none)
int EndEnqueued(Ctx* ctx, MappedRing* ring, int slot, const std::vector<int>* cameras) {
  HIPCHK(hipGetLastError());
  HIPCHK(ring->Release(slot, ctx->stream));
  if (cameras) HIPCHK(ctx->ingest.MarkRead(ctx->stream, ctx->cameras, cameras));
  return M3T_OK;
}
// the start-modality renderers of a call, from the two lists in its argument block
int LaunchStartRenderers(Ctx* ctx, const std::vector<int>& renderer_ids, const int* d_ids, const int* d_pairs) {
  if (renderer_ids.empty()) return M3T_OK;
  int largest = 0;
  for (int id : renderer_ids) {
    ctx->renderers[size_t(id)]->rendered = true;
    largest = std::max(largest, ctx->renderers[size_t(id)]->image_size);
  }
  return LaunchRenderers(ctx, d_ids, int(renderer_ids.size()), d_pairs, int(renderer_ids.size()), largest);
}
// The texture items of a call ({detector, texture modality, flag index or -1}: m3t_call_args.h) for these texture
// modalities, all of which have the built-in detector (RefuseTextureBodies).  flag_of: the flag index of a body, or null.
std::vector<int> TextureItems(Ctx* ctx, const std::vector<int>& texture_ids, const std::vector<int>* flag_of) {
  std::vector<int> detector_of(ctx->texture_mods.size(), -1);  // the detector table's order (UploadTables)
  int n_detectors = 0;
  for (size_t i = 0; i < ctx->texture_mods.size(); ++i)
    if (ctx->texture_mods[i]->builtin) detector_of[i] = n_detectors++;
  std::vector<int> items;
  for (int id : texture_ids) {
    items.push_back(detector_of[size_t(id)]);
    items.push_back(id);
    items.push_back(flag_of ? (*flag_of)[size_t(ctx->texture_mods[size_t(id)]->body)] : -1);
  }
  return items;
}
// StartModality (texture_modality.cpp:315-322) of the items of a call's argument block: detection on the colour
// camera's current frame at the pose the device holds, then the keyframe, behind the call's renderers.  flags: the
// judge's (an item runs iff its flag is set), or null (every item runs).
int LaunchTextureRestart(Ctx* ctx, int n_items, const int* d_items, const int* d_flags) {
  if (n_items == 0) return M3T_OK;
  const dim3 bands(n_items, M3T_TEXTURE_FOCUSED_MAX / M3T_FEATURE_BAND);
  const TextureDetectorDev* detectors = ctx->d_detectors.as<TextureDetectorDev>();
  hipLaunchKernelGGL(texture_focus_list_kernel, bands, dim3(kFeatureThreads), 0, ctx->stream, detectors,
                     ctx->d_texture.as<TextureModDev>(), ctx->cams_active, ctx->d_poses.as<float>(), d_items, d_flags);
  hipLaunchKernelGGL(texture_fast_list_kernel, bands, dim3(kFeatureThreads), 0, ctx->stream, detectors, d_items, d_flags);
  hipLaunchKernelGGL(texture_describe_list_kernel, dim3(n_items), dim3(kDescribeThreads), 0, ctx->stream, detectors,
                     d_items, d_flags);
  hipLaunchKernelGGL(texture_keyframe_list_kernel, dim3(n_items), dim3(M3T_TEXTURE_MATCH_THREADS), 0, ctx->stream,
                     ctx->d_texture.as<TextureModDev>(), ctx->cams_active, ctx->d_poses.as<float>(), d_items, d_flags);
  HIPCHK(hipGetLastError());
  return M3T_OK;
}
Judge* GetJudge(Ctx* ctx, int id, const char* entry) {
  if (id >= 0 && id < int(ctx->judges.size())) return ctx->judges[size_t(id)].get();
  Fail(ctx, M3T_ERR_INVALID_ARGUMENT, std::string(entry) + ": bad judge id");
  return nullptr;
}
// xyz as float4, padded to a multiple with copies of vertex 0 (which change no minimum and form pairs of the set only)
std::vector<float> PadVertices(const float* xyz, int n, size_t multiple) {
  const size_t n_padded = (size_t(n) + multiple - 1) / multiple * multiple;
  std::vector<float> padded(n_padded * 4, 0.0f);
  for (size_t i = 0; i < n_padded; ++i) std::memcpy(&padded[4 * i], xyz + 3 * (i < size_t(n) ? i : 0), 12);
  return padded;
}

// The last step that read ring slot `slot` of any of these cameras (-1: none)
long LastRead(Ctx* ctx, const int* ids, int n, int slot) {
  long last_read = -1;
  for (int i = 0; i < n; ++i) last_read = std::max(last_read, ctx->cameras[ids[i]]->last_read_step[slot]);
  return last_read;
}
// Whole frames into ring slot `slot` on copy stream cs -- of one camera, or of n cameras that lie one behind the other
// in a slab and in the host block (rows of row_step bytes): order, transfer, mark ("Frame
// ingest").  copied: the slot-copied events of the camera or the slab.  The arguments have been validated.
int UploadWholeFrames(Ctx* ctx, const int* ids, int n, int slot, const void* src, size_t row_step, int cs,
                      std::vector<Event>* copied) {
  const Camera& c0 = *ctx->cameras[ids[0]];
  const size_t row = size_t(c0.intr.width) * (c0.is_depth ? 2 : 3);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(ctx->ingest.EnsureStarted(ctx->ingest_cus, ctx->prop.multiProcessorCount));
  HIPCHK(ctx->ingest.OrderCopy(cs, LastRead(ctx, ids, n, slot), ctx->stream));
  hipStream_t stream = ctx->ingest.CopyStream(cs);
  if (row_step == c0.pitch)  // contiguous on both sides: one linear DMA transfer
    HIPCHK(hipMemcpyAsync(c0.frame(slot), src, c0.frame_bytes * size_t(n) - (c0.pitch - row), hipMemcpyHostToDevice, stream));
  else
    HIPCHK(hipMemcpy2DAsync(c0.frame(slot), c0.pitch, src, row_step, row, size_t(c0.intr.height) * size_t(n),
                            hipMemcpyHostToDevice, stream));
  for (int i = 0; i < n; ++i) ctx->cameras[ids[i]]->has_image[slot] = true;
  RoiMarkWholeFrames(ctx, ids, n, slot, stream);
  HIPCHK(ctx->ingest.SlotCopied(copied, c0.n_slots, slot, cs));
  return M3T_OK;
}

}  // namespace

#define CHECK_CTX() \
  if (!ctx) return M3T_ERR_INVALID_ARGUMENT

extern "C" {

int m3t_hip_create(m3t_hip_context** out, int device_id) {
  if (!out) return M3T_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_create_error = std::string("no usable HIP device: ") + (e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return M3T_ERR_DEVICE;
  }
  if (device_id < 0 || device_id >= n) {
    g_create_error = "device id out of range";
    return M3T_ERR_INVALID_ARGUMENT;
  }
  auto ctx = std::make_unique<m3t_hip_context>();
  ctx->device = device_id;
  if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipGetDeviceProperties(&ctx->prop, device_id)) != hipSuccess ||
      (e = CreateMaskedStream(0, ctx->prop.multiProcessorCount, &ctx->compute, false)) != hipSuccess) {
    g_create_error = std::string("device initialisation failed: ") + hipGetErrorString(e);
    return M3T_ERR_DEVICE;
  }
  ctx->stream = ctx->compute.get();
  ctx->compute_cus = ctx->prop.multiProcessorCount;
  *out = ctx.release();
  return M3T_OK;
}

void m3t_hip_destroy(m3t_hip_context* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  // nothing is in flight when the members go: the streams drain first, the host buffers are let go behind the copies
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  (void)ctx->ingest.SyncCopies();
  ctx->ingest.UnregisterAll();
  if (ctx->comm && ctx->comm_owned && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(ctx->comm);
  delete ctx;
}

const char* m3t_hip_last_error(m3t_hip_context* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int m3t_hip_device_info(m3t_hip_context* ctx, char* name, size_t cap, int* cus, size_t* mem) {
  CHECK_CTX();
  if (name && cap) {
    std::snprintf(name, cap, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
  }
  if (cus) *cus = ctx->prop.multiProcessorCount;
  if (mem) *mem = ctx->prop.totalGlobalMem;
  return M3T_OK;
}
int m3t_hip_get_stream(m3t_hip_context* ctx, void** s) {
  CHECK_CTX();
  REQUIRE(s, M3T_ERR_INVALID_ARGUMENT, "null out pointer");
  *s = ctx->stream;
  return M3T_OK;
}

// ---- models -------------------------------------------------------------------
int m3t_hip_region_model_create(m3t_hip_context* ctx, const m3t_region_model_desc* d) {
  CHECK_CTX();
  REQUIRE(d, M3T_ERR_INVALID_ARGUMENT, "null desc");
  HIPCHK(hipSetDevice(ctx->device));
  return CreateModel(ctx, true, d->n_views, d->n_points, d->data_points, d->orientations, d->contour_lengths,
                     d->stride_depth_offset, d->max_radius_depth_offset);
}
int m3t_hip_depth_model_create(m3t_hip_context* ctx, const m3t_depth_model_desc* d) {
  CHECK_CTX();
  REQUIRE(d, M3T_ERR_INVALID_ARGUMENT, "null desc");
  HIPCHK(hipSetDevice(ctx->device));
  return CreateModel(ctx, false, d->n_views, d->n_points, d->data_points, d->orientations, d->surface_areas,
                     d->stride_depth_offset, d->max_radius_depth_offset);
}
int m3t_hip_region_model_load(m3t_hip_context* ctx, const char* path) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  return LoadModel(ctx, path, true);
}
int m3t_hip_depth_model_load(m3t_hip_context* ctx, const char* path) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  return LoadModel(ctx, path, false);
}
static int ModelInfo(m3t_hip_context* ctx, bool region, int id, int* nv, int* np, float* me) {
  auto& vec = region ? ctx->region_models : ctx->depth_models;
  REQUIRE(id >= 0 && id < int(vec.size()), M3T_ERR_INVALID_ARGUMENT, "bad model id");
  if (nv) *nv = vec[id]->n_views;
  if (np) *np = vec[id]->n_points;
  if (me) *me = vec[id]->max_extent;
  return M3T_OK;
}
int m3t_hip_region_model_info(m3t_hip_context* ctx, int id, int* nv, int* np, float* me) {
  CHECK_CTX();
  return ModelInfo(ctx, true, id, nv, np, me);
}
int m3t_hip_depth_model_info(m3t_hip_context* ctx, int id, int* nv, int* np, float* me) {
  CHECK_CTX();
  return ModelInfo(ctx, false, id, nv, np, me);
}

}  // extern "C"

// single-block helper kernel for the stand-alone GetClosestView entry point
extern "C" __global__ void __launch_bounds__(M3T_BLOCK_THREADS)
closest_view_kernel(const float4* orientations, int n_views, const float* body2camera, int* out) {
  __shared__ float misc[256];
  const Affine b2c = load_pose(body2camera);
  int v = closest_view((G<v4f>)orientations, n_views, b2c, misc);
  if (threadIdx.x == 0) *out = v;
}

extern "C" {

static int ClosestView(m3t_hip_context* ctx, bool region, int id, const float* pose, int* view) {
  auto& vec = region ? ctx->region_models : ctx->depth_models;
  REQUIRE(id >= 0 && id < int(vec.size()) && pose && view, M3T_ERR_INVALID_ARGUMENT, "bad arguments");
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->d_scratch_view.bytes < 128) HIPCHK(ctx->d_scratch_view.alloc(128));
  float* d_pose = ctx->d_scratch_view.as<float>();
  int* d_out = reinterpret_cast<int*>(d_pose + 16);
  HIPCHK(hipMemcpyAsync(d_pose, pose, 64, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(closest_view_kernel, dim3(1), dim3(M3T_BLOCK_THREADS), 0, ctx->stream,
                     vec[id]->orientations4.as<float4>(), vec[id]->n_views, d_pose, d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(view, d_out, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return M3T_OK;
}
int m3t_hip_region_model_closest_view(m3t_hip_context* ctx, int id, const float pose[16], int* view) {
  CHECK_CTX();
  return ClosestView(ctx, true, id, pose, view);
}
int m3t_hip_depth_model_closest_view(m3t_hip_context* ctx, int id, const float pose[16], int* view) {
  CHECK_CTX();
  return ClosestView(ctx, false, id, pose, view);
}

// ---- cameras --------------------------------------------------------------------
int m3t_hip_color_camera_create(m3t_hip_context* ctx, const m3t_intrinsics* i, const float w2c[16]) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  return CreateCamera(ctx, i, w2c, false, 0.0f);
}
int m3t_hip_depth_camera_create(m3t_hip_context* ctx, const m3t_intrinsics* i, const float w2c[16], float depth_scale) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  return CreateCamera(ctx, i, w2c, true, depth_scale);
}
int m3t_hip_camera_upload(m3t_hip_context* ctx, int id, const void* pixels, size_t row_step) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  REQUIRE(id >= 0 && id < int(ctx->cameras.size()), M3T_ERR_INVALID_ARGUMENT, "bad camera id");
  return UploadFrame(ctx, id, ctx->cameras[id]->current, pixels, row_step);
}
int m3t_hip_camera_set_world2camera_pose(m3t_hip_context* ctx, int id, const float w2c[16]) {
  CHECK_CTX();
  REQUIRE(id >= 0 && id < int(ctx->cameras.size()) && w2c, M3T_ERR_INVALID_ARGUMENT, "bad camera id");
  std::memcpy(ctx->cameras[id]->world2camera, w2c, 64);
  ctx->cams_dirty = true;
  ctx->tables_dirty = true;  // (whether a body's two modalities share their view search depends on the camera poses)
  return M3T_OK;
}
int m3t_hip_camera_set_ring(m3t_hip_context* ctx, int id, int n_slots) {
  CHECK_CTX();
  REQUIRE(id >= 0 && id < int(ctx->cameras.size()) && n_slots >= 1, M3T_ERR_INVALID_ARGUMENT, "bad arguments");
  HIPCHK(hipSetDevice(ctx->device));
  Camera& c = *ctx->cameras[id];
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(c.ring.alloc(c.frame_bytes * size_t(n_slots) + 64));
  c.frames = c.ring.as<uint8_t>();
  c.slot_stride = c.frame_bytes;
  c.slab = -1;
  c.SetSlots(n_slots);
  if (ctx->roi_enabled) ctx->tables_dirty = true;  // (the rectangle table has a row per ring slot)
  ctx->cams_dirty = true;
  return M3T_OK;
}
int m3t_hip_camera_upload_slot(m3t_hip_context* ctx, int id, int slot, const void* pixels, size_t row_step) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  return UploadFrame(ctx, id, slot, pixels, row_step);
}
int m3t_hip_host_register(m3t_hip_context* ctx, void* ptr, size_t bytes) {
  CHECK_CTX();
  REQUIRE(ptr && bytes, M3T_ERR_INVALID_ARGUMENT, "null buffer");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(ctx->ingest.Register(ptr, bytes));
  return M3T_OK;
}
int m3t_hip_host_unregister(m3t_hip_context* ctx, void* ptr) {
  CHECK_CTX();
  REQUIRE(ctx->ingest.IsRegistered(ptr), M3T_ERR_INVALID_ARGUMENT, "buffer was not registered with this context");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(ctx->ingest.Unregister(ptr));
  return M3T_OK;
}
int m3t_hip_camera_upload_slot_async(m3t_hip_context* ctx, int id, int slot, const void* pixels, size_t row_step) {
  CHECK_CTX();
  REQUIRE(id >= 0 && id < int(ctx->cameras.size()) && pixels, M3T_ERR_INVALID_ARGUMENT, "bad camera id");
  Camera& c = *ctx->cameras[id];
  REQUIRE(slot >= 0 && slot < c.n_slots, M3T_ERR_INVALID_ARGUMENT, "bad frame slot");
  REQUIRE(row_step >= size_t(c.intr.width) * (c.is_depth ? 2 : 3), M3T_ERR_INVALID_ARGUMENT, "row_step smaller than one image row");
  return UploadWholeFrames(ctx, &id, 1, slot, pixels, row_step, id % Ingest::kCopyStreams, &c.slot_copied);
}
// Wait until the last upload into (camera, slot) -- camera_upload_slot_async, a batch upload, a rectangle pull -- has
// left its host buffer, and for nothing else: the copies of other cameras and of this camera's other slots stay in
// flight (m3t_hip_ingest_sync waits for all).  A rectangle slot also waits for the step that read it (its repair
// reads the host block once more).
int m3t_hip_camera_slot_sync(m3t_hip_context* ctx, int id, int slot) {
  CHECK_CTX();
  REQUIRE(id >= 0 && id < int(ctx->cameras.size()), M3T_ERR_INVALID_ARGUMENT, "bad camera id");
  Camera& c = *ctx->cameras[id];
  REQUIRE(slot >= 0 && slot < c.n_slots, M3T_ERR_INVALID_ARGUMENT, "bad frame slot");
  HIPCHK(hipSetDevice(ctx->device));
  hipEvent_t slab_copied = nullptr;  // behind the last batch upload / rectangle pull into the slot
  if (c.slab >= 0 && size_t(slot) < ctx->slabs[size_t(c.slab)]->slot_copied.size())
    slab_copied = ctx->slabs[size_t(c.slab)]->slot_copied[slot].get();
  if (c.slot_is_roi[slot]) {
    // a rectangle went into the slot (m3t_hip_cameras_upload_batch_roi_async): the host block is read by the pull and,
    // should a body outrun its rectangle, again by the repair of the step that reads the slot -- both must be over
    if (slab_copied) HIPCHK(hipEventSynchronize(slab_copied));
    else if (ctx->ingest.CopyStream(0)) HIPCHK(hipStreamSynchronize(ctx->ingest.CopyStream(0)));
    HIPCHK(ctx->ingest.WaitForReader(c.last_read_step[slot], ctx->stream));
    return M3T_OK;
  }
  // (a camera may have been fed both ways: its own uploads and batch uploads of its slab; an event that has long
  // completed costs nothing to wait for)
  if (slab_copied) HIPCHK(hipEventSynchronize(slab_copied));
  if (size_t(slot) >= c.slot_copied.size() || !c.slot_copied[slot]) return M3T_OK;  // nothing (else) was enqueued
  HIPCHK(hipEventSynchronize(c.slot_copied[slot].get()));
  return M3T_OK;
}
// One frame ring for a group of cameras of equal geometry: [slot][camera][frame], so that slot s of the whole group is
// one contiguous block of device memory and a batch-frame arrives as ONE transfer (m3t_hip_cameras_upload_batch_async).
int m3t_hip_cameras_set_ring(m3t_hip_context* ctx, const int* ids, int n, int n_slots) {
  CHECK_CTX();
  REQUIRE(ids && n >= 1 && n_slots >= 1, M3T_ERR_INVALID_ARGUMENT, "bad arguments");
  for (int i = 0; i < n; ++i) {
    REQUIRE(ids[i] >= 0 && ids[i] < int(ctx->cameras.size()), M3T_ERR_INVALID_ARGUMENT, "bad camera id");
    const Camera& a = *ctx->cameras[ids[0]];
    const Camera& b = *ctx->cameras[ids[i]];
    // (the row pitch is rounded up to 64 bytes, so equal pitch does not imply equal width: the one-block upload
    // copies every camera's rows with camera 0's row length)
    REQUIRE(a.frame_bytes == b.frame_bytes && a.pitch == b.pitch && a.is_depth == b.is_depth &&
                a.intr.width == b.intr.width && a.intr.height == b.intr.height,
            M3T_ERR_INVALID_ARGUMENT, "the cameras of a shared ring must have the same image geometry (width, height, type)");
    for (int j = 0; j < i; ++j) REQUIRE(ids[j] != ids[i], M3T_ERR_INVALID_ARGUMENT, "camera listed twice");
  }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  auto slab = std::make_unique<FrameSlab>();
  const size_t frame_bytes = ctx->cameras[ids[0]]->frame_bytes;
  HIPCHK(slab->mem.alloc(frame_bytes * size_t(n) * size_t(n_slots) + 64));
  slab->cameras.assign(ids, ids + n);
  const int slab_id = int(ctx->slabs.size());
  for (int i = 0; i < n; ++i) {
    Camera& c = *ctx->cameras[ids[i]];
    c.ring.release();
    c.slab = slab_id;
    c.slab_index = i;
    c.frames = slab->mem.as<uint8_t>() + size_t(i) * frame_bytes;
    c.slot_stride = frame_bytes * size_t(n);
    c.SetSlots(n_slots);
    if (ctx->roi_enabled) ctx->tables_dirty = true;  // (the rectangle table has a row per ring slot)
  }
  ctx->slabs.push_back(std::move(slab));
  ctx->cams_dirty = true;
  return M3T_OK;
}
// The frames of n cameras for one ring slot, frame i at base + i * camera_stride, enqueued from here (what a capture
// process hands over per batch-frame; replaces n blocking cv::Mat hand-overs, loader_camera.cpp:76-98).  Cameras
// that share a ring (m3t_hip_cameras_set_ring, listed in its order) and a host block in the ring's layout
// (camera_stride = height * row_step, row_step = the device pitch) make it ONE linear DMA transfer.
int m3t_hip_cameras_upload_batch_async(m3t_hip_context* ctx, const int* ids, int n, int slot, const void* base,
                                       size_t camera_stride, size_t row_step) {
  CHECK_CTX();
  REQUIRE(ids && n >= 1 && base, M3T_ERR_INVALID_ARGUMENT, "bad arguments");
  bool one_block = true;
  for (int i = 0; i < n; ++i) {
    REQUIRE(ids[i] >= 0 && ids[i] < int(ctx->cameras.size()), M3T_ERR_INVALID_ARGUMENT, "bad camera id");
    const Camera& c = *ctx->cameras[ids[i]];
    REQUIRE(slot >= 0 && slot < c.n_slots, M3T_ERR_INVALID_ARGUMENT, "bad frame slot");
    const Camera& c0 = *ctx->cameras[ids[0]];
    if (c.slab < 0 || c.slab != c0.slab || c.slab_index != c0.slab_index + i) one_block = false;
  }
  const Camera& c0 = *ctx->cameras[ids[0]];
  REQUIRE(row_step >= size_t(c0.intr.width) * (c0.is_depth ? 2 : 3), M3T_ERR_INVALID_ARGUMENT, "row_step smaller than one image row");
  if (!(one_block && camera_stride == size_t(c0.intr.height) * row_step)) {
    for (int i = 0; i < n; ++i) {  // scattered on one side: one transfer per camera, still without a host round trip each
      int r = m3t_hip_camera_upload_slot_async(ctx, ids[i], slot, static_cast<const uint8_t*>(base) + size_t(i) * camera_stride,
                                               row_step);
      if (r) return r;
    }
    return M3T_OK;
  }
  // (also reached from cameras_upload_batch_roi_async whenever rectangles are not possible)
  return UploadWholeFrames(ctx, ids, n, slot, base, row_step, 0, &ctx->slabs[size_t(c0.slab)]->slot_copied);
}
// ROI ingest (m3t_ingest.hip).  enable: the fused rigid launches record the poses their searches run at,
// and m3t_hip_cameras_upload_batch_roi_async may upload rectangles instead of frames; margin_px: how far (in pixels,
// in every direction) the trackers' rectangle may move between the pose it is computed from and the last pose of
// the step that reads the frame, i.e. two frames of motion.
int m3t_hip_set_roi_ingest(m3t_hip_context* ctx, int enable, float margin_px) {
  CHECK_CTX();
  REQUIRE(margin_px >= 0.0f && margin_px < 1.0e6f, M3T_ERR_INVALID_ARGUMENT, "bad margin");
  REQUIRE(enable >= 0 && enable <= 2, M3T_ERR_INVALID_ARGUMENT, "enable: 0 (off), 1 (one margin for all bodies) or 2 (adaptive margins)");
  REQUIRE(enable == 0 || ctx->texture_mods.empty(), M3T_ERR_UNSUPPORTED, "a texture modality and ROI ingest do not go together");
  if ((enable != 0) != ctx->roi_enabled) ctx->tables_dirty = true;
  ctx->roi_enabled = enable != 0;
  ctx->roi_adaptive = enable == 2;
  ctx->roi_margin_px = margin_px;
  return M3T_OK;
}
// Keep n_cus CUs free of the tracking kernels and run the ROI pull kernel there (CU masks on the context's streams).
// Why: the pull kernel's PCIe reads (~2 us each) sit in the memory pipelines of the CUs it runs on; a tracking
// workgroup that shares its CU takes 3-4 x longer, and since an object's workgroups wait for each other so does the
// step.  On CUs of its own the pull costs the step ~14 % (tools/ubench_cumask.hip) and frame k + 1 crosses PCIe while
// step k runs.  n_cus should take the same number of CUs from every shader engine -- on MI355X a multiple of 32
// (8 XCDs x 4 shader engines): 16 leaves the engines unequal and a one-workgroup-per-CU launch 1.5 x slower, 64 gives
// the pull more lanes than PCIe can feed and costs the step more.  0 = off.  The call synchronises and REPLACES the
// context's streams: fetch m3t_hip_get_stream again afterwards.
int m3t_hip_reserve_ingest_cus(m3t_hip_context* ctx, int n_cus) {
  CHECK_CTX();
  REQUIRE(n_cus >= 0 && n_cus <= ctx->prop.multiProcessorCount / 2, M3T_ERR_INVALID_ARGUMENT,
          "n_cus must lie in [0, CUs / 2]");
  // unequal shader engines are not only slow: the hardware deals workgroups to engines, so a launch planned with one
  // workgroup per remaining CU may find two of its workgroups queued behind each other -- and the split / tree launches
  // need all of theirs resident at once
  REQUIRE(n_cus % 32 == 0, M3T_ERR_INVALID_ARGUMENT,
          "n_cus must be a multiple of 32 (one CU from each of the 4 shader engines of each of the 8 XCDs)");
  // the mask layout above (bit i -> XCD i mod 8, the highest bits of an XCD = the last CU of each shader engine) and the
  // multiple-of-32 rule were probed on MI355X in SPX mode (tools/ubench_cumask.hip): on another part or partition mode
  // the split / tree launches, which need all their workgroups resident, could be planned wrong
  REQUIRE(n_cus == 0 || (ctx->prop.multiProcessorCount == 256 && std::strncmp(ctx->prop.gcnArchName, "gfx950", 6) == 0),
          M3T_ERR_UNSUPPORTED, "CU reservation is laid out for MI355X (gfx950, 256 CUs in one partition)");
  if (n_cus == ctx->ingest_cus) return M3T_OK;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx->ingest.SyncCopies());
  // all new streams first, then the swap: a failure leaves the context as it was.  (A stream with a CU mask is a
  // BLOCKING stream: while CUs are reserved, work on the legacy NULL stream -- a plain hipMemcpy, torch's default
  // stream -- synchronises with the compute stream and copy stream 0; keep such work off the device meanwhile, or
  // the pull / step overlap is lost.)
  Stream compute, copies[Ingest::kCopyStreams];
  hipError_t e = CreateMaskedStream(n_cus, ctx->prop.multiProcessorCount, &compute, false);
  if (e == hipSuccess && ctx->ingest.async()) e = Ingest::CreateStreams(n_cus, ctx->prop.multiProcessorCount, copies);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return Fail(ctx, M3T_ERR_UNSUPPORTED, "this device / runtime does not create CU-masked streams");
  }
  ctx->compute = std::move(compute);
  ctx->stream = ctx->compute.get();
  ctx->ingest.ReplaceStreams(copies);
  ctx->ingest_cus = n_cus;
  ctx->compute_cus = ctx->prop.multiProcessorCount - n_cus;
  return M3T_OK;
}
// m3t_hip_cameras_upload_batch_async for the trackers' rectangles only: ONE kernel on the copy stream computes every
// camera's rectangle from the bodies' poses as of the start of the step enqueued last, and pulls its rows out of the
// mapped, page-locked host block.  Whole frames are uploaded instead (same result, more bytes) whenever the
// conditions are not met: ROI ingest off, no recorded step yet, cameras not in one slab in this order, a host block
// that is not registered, or strides that are not multiples of 16 bytes.
int m3t_hip_cameras_upload_batch_roi_async(m3t_hip_context* ctx, const int* ids, int n, int slot, const void* base,
                                           size_t camera_stride, size_t row_step) {
  CHECK_CTX();
  REQUIRE(ids && n >= 1 && base, M3T_ERR_INVALID_ARGUMENT, "bad arguments");
  bool pull = ctx->roi_enabled && ctx->roi_recorded && ctx->roi_snapshot_valid && ctx->n_roi_items > 0 &&
              !ctx->tables_dirty && !ctx->cams_dirty && ctx->ingest.async();
  for (int i = 0; i < n && pull; ++i) {
    if (ids[i] < 0 || ids[i] >= int(ctx->cameras.size())) { pull = false; break; }
    const Camera& c = *ctx->cameras[ids[i]];
    const Camera& c0 = *ctx->cameras[ids[0]];
    if (slot < 0 || slot >= c.n_slots || slot >= ctx->roi_rect_slots) pull = false;
    if (c.slab < 0 || c.slab != c0.slab || c.slab_index != c0.slab_index + i) pull = false;
  }
  const uint8_t* src = nullptr;
  if (pull) {
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, const_cast<void*>(base), 0) != hipSuccess) {
      (void)hipGetLastError();
      pull = false;
    }
    src = static_cast<const uint8_t*>(dev);
  }
  if (pull) {
    const Camera& c0 = *ctx->cameras[ids[0]];
    const size_t row = size_t(c0.intr.width) * (c0.is_depth ? 2 : 3), row16 = (row + 15) / 16 * 16;
    if (reinterpret_cast<uintptr_t>(src) % 16 || camera_stride % 16 || row_step % 16 || c0.pitch % 16 ||
        c0.frame_bytes % 16 || reinterpret_cast<uintptr_t>(c0.frame(slot)) % 16 || row16 > row_step || row16 > c0.pitch)
      pull = false;
  }
  if (!pull) return m3t_hip_cameras_upload_batch_async(ctx, ids, n, slot, base, camera_stride, row_step);
  HIPCHK(hipSetDevice(ctx->device));
  const int cs = 0;
  hipStream_t copy_stream = ctx->ingest.CopyStream(cs);
  bool consecutive = true;
  for (int i = 0; i < n; ++i) consecutive = consecutive && ids[i] == ids[0] + i;
  const int* d_ids = ctx->d_roi_all_cam_ids.as<int>() + ids[0];
  if (!consecutive) {
    // Every scattered batch keeps its own list.  (Until now there was one list for all of them: the depth cameras' batch
    // replaced the colour cameras' list and cleared every slot's repair sources, so a body of Region + Depth objects
    // that left its rectangle was repeated without its colour frame and stayed uncommitted.)
    const std::vector<int> wanted(ids, ids + n);
    const DevMem* list = nullptr;
    for (auto& l : ctx->roi_cam_id_lists)
      if (l.first == wanted) list = l.second.get();
    if (!list) {
      if (ctx->roi_cam_id_lists.size() >= Ctx::kRoiScatteredLists) {  // (rare: camera lists that keep changing)
        HIPCHK(hipStreamSynchronize(copy_stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));  // (a repair may still read an old list)
        for (auto& sources : ctx->roi_sources) sources.clear();
        ctx->roi_cam_id_lists.clear();
      }
      auto mem = std::make_unique<DevMem>();
      HIPCHK(mem->alloc(size_t(n) * sizeof(int)));
      HIPCHK(hipMemcpy(mem->p, ids, size_t(n) * sizeof(int), hipMemcpyHostToDevice));
      list = mem.get();
      ctx->roi_cam_id_lists.emplace_back(wanted, std::move(mem));
    }
    d_ids = list->as<int>();
  }
  HIPCHK(ctx->ingest.OrderCopy(cs, LastRead(ctx, ids, n, slot), ctx->stream));
  HIPCHK(hipStreamWaitEvent(copy_stream, ctx->roi_snapshot_done[ctx->roi_use].get(), 0));  // the poses the rectangles come from
  const bool adaptive = ctx->roi_adaptive && ctx->roi_prev >= 0;
  if (adaptive) HIPCHK(hipStreamWaitEvent(copy_stream, ctx->roi_snapshot_done[ctx->roi_prev].get(), 0));
  const Camera& c0 = *ctx->cameras[ids[0]];
  // the camera table is only read for intrinsics and world2camera here: any slot version will do (the first one)
  m3t_roi_rect* rects = ctx->d_roi_rects.as<m3t_roi_rect>() + size_t(slot) * ctx->cameras.size();
  const size_t snapshot_floats = ctx->d_roi_pose_snapshot.bytes / (4 * Ctx::kRoiSnapshots);
  const float* snapshots = ctx->d_roi_pose_snapshot.as<float>();
  // (without a second snapshot an adaptive upload takes the whole margin)
  hipLaunchKernelGGL(roi_rect_kernel, dim3((n + 63) / 64), dim3(64), 0, copy_stream,
                     ctx->d_roi_items.as<RoiItemDev>(), ctx->d_roi_item_first.as<int>(), d_ids, n,
                     ctx->d_cams.as<CameraDev>(), snapshots + size_t(ctx->roi_use) * snapshot_floats,
                     adaptive ? snapshots + size_t(ctx->roi_prev) * snapshot_floats : (const float*)nullptr,
                     adaptive ? ctx->d_roi_motion_peak.as<float>() : (float*)nullptr, ctx->roi_margin_px,
                     std::min(ctx->roi_margin_px, 4.0f), rects);
  hipLaunchKernelGGL(roi_pull_kernel, dim3((c0.intr.height + 7) / 8, n), dim3(256), 0, copy_stream,
                     d_ids, rects, src, camera_stride, uint32_t(row_step), c0.frame(slot),
                     c0.frame_bytes, c0.pitch, c0.is_depth ? 2 : 3);
  HIPCHK(hipGetLastError());
  ++ctx->roi_pulls;
  for (int i = 0; i < n; ++i) {
    Camera& c = *ctx->cameras[ids[i]];
    c.has_image[slot] = true;
    c.slot_is_roi[slot] = true;
  }
  // m3t_hip_camera_slot_sync waits for THIS pull, not for whatever else the copy stream carries by then
  HIPCHK(ctx->ingest.SlotCopied(&ctx->slabs[size_t(c0.slab)]->slot_copied, c0.n_slots, slot, cs));
  {  // where the whole frames are, should a body outrun its rectangle (the repair of the step that reads this slot)
    auto& sources = ctx->roi_sources[size_t(slot)];
    for (size_t k = 0; k < sources.size();) {
      bool overlaps = false;
      for (int i = 0; i < n && !overlaps; ++i)
        overlaps = std::find(sources[k].ids.begin(), sources[k].ids.end(), ids[i]) != sources[k].ids.end();
      if (overlaps) sources.erase(sources.begin() + long(k)); else ++k;
    }
    Ctx::RoiSource source;
    source.ids.assign(ids, ids + n);
    source.d_ids = d_ids;
    source.src = src;
    source.camera_stride = camera_stride;
    source.row_step = uint32_t(row_step);
    sources.push_back(std::move(source));
  }
  return M3T_OK;
}
// one of the two lists of the mapped miss block, read in place behind the stream and cleared
static int ReadRoiMisses(Ctx* ctx, bool unrecovered, int* bodies, int capacity, int* n) {
  if (!ctx->roi_miss.host) return M3T_OK;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  int* list = Ctx::RoiMissList(ctx->roi_miss.host, unrecovered);
  const int count = __atomic_load_n(&list[0], __ATOMIC_ACQUIRE);
  *n = count;
  for (int i = 0; i < std::min(std::min(count, capacity), int(Ctx::kRoiMissCapacity)); ++i) bodies[i] = list[1 + i];
  std::memset(list, 0, (Ctx::kRoiMissCapacity + 1) * sizeof(int));
  return M3T_OK;
}
// Bodies whose steps since the last call needed pixels outside the rectangle that had been uploaded: up to `capacity`
// body ids, *n = how many there were; the list is cleared.  Such a step is not committed; the library fetched the whole
// frames and repeated it (m3t_hip_execute_tracking_step), so the poses ARE the whole-frame poses -- the list says how
// often the margin was too small.  m3t_hip_roi_get_unrecovered names the ones for which that was not possible.
int m3t_hip_roi_get_status(m3t_hip_context* ctx, int* bodies, int capacity, int* n, long long* n_rectangle_uploads) {
  CHECK_CTX();
  REQUIRE(n && capacity >= 0 && (bodies || capacity == 0), M3T_ERR_INVALID_ARGUMENT, "null output");
  *n = 0;
  if (n_rectangle_uploads) *n_rectangle_uploads = ctx->roi_pulls;
  return ReadRoiMisses(ctx, false, bodies, capacity, n);
}
// Bodies whose step left its rectangle AND whose repeat did too (the whole frames were not within reach: the host
// block of the upload was not recorded for the slot, e.g. after the tables were rebuilt).  Their step was not
// committed: pose, histograms and modality state are those before it.  Re-upload the frame in full
// (m3t_hip_cameras_upload_batch_async) and call m3t_hip_execute_tracking_step again -- the bodies that were committed
// are then stepped a second time, so set their poses back first or accept the extra step.  Cleared by the call.
int m3t_hip_roi_get_unrecovered(m3t_hip_context* ctx, int* bodies, int capacity, int* n) {
  CHECK_CTX();
  REQUIRE(n && capacity >= 0 && (bodies || capacity == 0), M3T_ERR_INVALID_ARGUMENT, "null output");
  *n = 0;
  return ReadRoiMisses(ctx, true, bodies, capacity, n);
}
// Developer read-backs (tests/test_gpu_roi_edges.py): what the ROI kernels left on the device, read behind the copy
// streams and the compute stream.  Nothing is launched and no state of the context changes.
int m3t_hip_roi_get_rectangles(m3t_hip_context* ctx, const int* ids, int n, int slot, int* rects) {
  CHECK_CTX();
  REQUIRE(ids && n >= 1 && rects, M3T_ERR_INVALID_ARGUMENT, "bad arguments");
  REQUIRE(ctx->roi_enabled && ctx->n_roi_items > 0 && !ctx->tables_dirty && ctx->d_roi_rects.p, M3T_ERR_UNSUPPORTED,
          "roi_get_rectangles: no rectangle table (ROI ingest off, or the tables were not built by a step yet)");
  for (int i = 0; i < n; ++i)
    REQUIRE(ids[i] >= 0 && ids[i] < int(ctx->cameras.size()), M3T_ERR_INVALID_ARGUMENT, "bad camera id");
  REQUIRE(slot >= 0 && slot < ctx->roi_rect_slots, M3T_ERR_INVALID_ARGUMENT, "bad frame slot");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(ctx->ingest.SyncCopies());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  static_assert(sizeof(m3t_roi_rect) == 4 * sizeof(int), "a rectangle is x0 y0 x1 y1");
  const m3t_roi_rect* table = ctx->d_roi_rects.as<m3t_roi_rect>() + size_t(slot) * ctx->cameras.size();
  for (int i = 0; i < n; ++i)
    HIPCHK(hipMemcpy(rects + 4 * i, table + ids[i], sizeof(m3t_roi_rect), hipMemcpyDeviceToHost));
  return M3T_OK;
}
int m3t_hip_camera_download_slot(m3t_hip_context* ctx, int id, int slot, void* pixels, size_t row_step) {
  CHECK_CTX();
  REQUIRE(id >= 0 && id < int(ctx->cameras.size()) && pixels, M3T_ERR_INVALID_ARGUMENT, "bad camera id");
  const Camera& c = *ctx->cameras[id];
  REQUIRE(slot >= 0 && slot < c.n_slots, M3T_ERR_INVALID_ARGUMENT, "bad frame slot");
  const size_t row = size_t(c.intr.width) * (c.is_depth ? 2 : 3);
  REQUIRE(row_step >= row, M3T_ERR_INVALID_ARGUMENT, "row_step smaller than one image row");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(ctx->ingest.SyncCopies());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy2D(pixels, row_step, c.frame(slot), c.pitch, row, size_t(c.intr.height), hipMemcpyDeviceToHost));
  return M3T_OK;
}
int m3t_hip_ingest_sync(m3t_hip_context* ctx) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(ctx->ingest.SyncCopies());
  return M3T_OK;
}
int m3t_hip_camera_select_slot(m3t_hip_context* ctx, int id, int slot) {
  CHECK_CTX();
  REQUIRE(id >= 0 && id < int(ctx->cameras.size()), M3T_ERR_INVALID_ARGUMENT, "bad camera id");
  Camera& c = *ctx->cameras[id];
  REQUIRE(slot >= 0 && slot < c.n_slots, M3T_ERR_INVALID_ARGUMENT, "bad frame slot");
  if (c.current != slot) {
    c.current = slot;
    ctx->slots_dirty = true;
  }
  return M3T_OK;
}
int m3t_hip_cameras_select_slot(m3t_hip_context* ctx, int slot) {
  CHECK_CTX();
  // every camera that has a ring: a camera without one keeps its only frame (the cameras of bodies whose modalities
  // live on another rank -- a structure spread over processes -- hold no frames at all; round 5: before, the call
  // failed on them with "bad frame slot", i.e. the N > 1 chain leg of bench.py could not have run)
  for (size_t i = 0; i < ctx->cameras.size(); ++i) {
    if (ctx->cameras[i]->n_slots <= 1 && slot != 0) continue;
    int r = m3t_hip_camera_select_slot(ctx, int(i), slot);
    if (r) return r;
  }
  return M3T_OK;
}

// ---- bodies ---------------------------------------------------------------------
int m3t_hip_body_create(m3t_hip_context* ctx, const float pose[16]) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  int r = SyncPosesToHost(ctx);
  if (r) return r;
  static const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float* src = pose ? pose : ident;
  ctx->body_poses.insert(ctx->body_poses.end(), src, src + 16);
  ctx->poses_dirty_host = true;
  ctx->tables_dirty = true;
  return int(ctx->body_poses.size() / 16) - 1;
}
int m3t_hip_body_set_body2world_pose(m3t_hip_context* ctx, int id, const float pose[16]) {
  CHECK_CTX();
  REQUIRE(id >= 0 && id < int(ctx->body_poses.size() / 16) && pose, M3T_ERR_INVALID_ARGUMENT, "bad body id");
  HIPCHK(hipSetDevice(ctx->device));
  int r = SyncPosesToHost(ctx);
  if (r) return r;
  std::memcpy(&ctx->body_poses[size_t(id) * 16], pose, 64);
  ctx->poses_dirty_host = true;
  return M3T_OK;
}
int m3t_hip_body_get_body2world_pose(m3t_hip_context* ctx, int id, float pose[16]) {
  CHECK_CTX();
  REQUIRE(id >= 0 && id < int(ctx->body_poses.size() / 16) && pose, M3T_ERR_INVALID_ARGUMENT, "bad body id");
  HIPCHK(hipSetDevice(ctx->device));
  int r = SyncPosesToHost(ctx);
  if (r) return r;
  std::memcpy(pose, &ctx->body_poses[size_t(id) * 16], 64);
  return M3T_OK;
}
int m3t_hip_bodies_set_poses(m3t_hip_context* ctx, const float* poses, int n) {
  CHECK_CTX();
  REQUIRE(poses && n >= 0 && n <= int(ctx->body_poses.size() / 16), M3T_ERR_INVALID_ARGUMENT, "bad pose count");
  HIPCHK(hipSetDevice(ctx->device));
  int r = SyncPosesToHost(ctx);
  if (r) return r;
  std::memcpy(ctx->body_poses.data(), poses, size_t(n) * 64);
  ctx->poses_dirty_host = true;
  return M3T_OK;
}
int m3t_hip_bodies_get_poses(m3t_hip_context* ctx, float* poses, int n) {
  CHECK_CTX();
  REQUIRE(poses && n >= 0 && n <= int(ctx->body_poses.size() / 16), M3T_ERR_INVALID_ARGUMENT, "bad pose count");
  HIPCHK(hipSetDevice(ctx->device));
  int r = SyncPosesToHost(ctx);
  if (r) return r;
  std::memcpy(poses, ctx->body_poses.data(), size_t(n) * 64);
  return M3T_OK;
}

// ---- modalities -------------------------------------------------------------------
int m3t_hip_region_modality_create(m3t_hip_context* ctx, const m3t_region_modality_params* p, int body,
                                   int color_camera, int model, int depth_camera) {
  CHECK_CTX();
  REQUIRE(p, M3T_ERR_INVALID_ARGUMENT, "null params");
  REQUIRE(body >= 0 && body < int(ctx->body_poses.size() / 16), M3T_ERR_INVALID_ARGUMENT, "bad body id");
  REQUIRE(color_camera >= 0 && color_camera < int(ctx->cameras.size()) && !ctx->cameras[color_camera]->is_depth,
          M3T_ERR_INVALID_ARGUMENT, "bad color camera id");
  REQUIRE(model >= 0 && model < int(ctx->region_models.size()), M3T_ERR_INVALID_ARGUMENT, "bad region model id");
  REQUIRE(!p->use_region_checking && !p->model_occlusions, M3T_ERR_INVALID_ARGUMENT,
          "switch region checking / modelled occlusions on with their renderer afterwards");
  if (p->measure_occlusions)
    REQUIRE(depth_camera >= 0 && depth_camera < int(ctx->cameras.size()) && ctx->cameras[depth_camera]->is_depth,
            M3T_ERR_INVALID_ARGUMENT, "measure_occlusions needs a depth camera");
  REQUIRE(p->function_length >= 1 && p->function_length <= M3T_MAX_FUNCTION_LENGTH && p->distribution_length >= 2 &&
              p->distribution_length <= M3T_MAX_DISTRIBUTION_LENGTH && p->n_scales >= 1 &&
              p->n_scales <= M3T_MAX_SCALES && p->n_standard_deviations >= 1 &&
              p->n_standard_deviations <= M3T_MAX_SCALES && p->n_lines_max >= 1 && p->n_lines_max <= 1024,
          M3T_ERR_INVALID_ARGUMENT, "bad region modality parameters");
  int bitshift;
  switch (p->n_histogram_bins) {  // color_histograms.cpp:131-158
    case 2: bitshift = 7; break;
    case 4: bitshift = 6; break;
    case 8: bitshift = 5; break;
    case 16: bitshift = 4; break;
    case 32: bitshift = 3; break;
    case 64: bitshift = 2; break;
    default:
      return Fail(ctx, M3T_ERR_INVALID_ARGUMENT, "n_bins has to be of value 2, 4, 8, 16, 32, or 64");
  }
  HIPCHK(hipSetDevice(ctx->device));
  const Model& mdl = *ctx->region_models[model];
  auto m = std::make_unique<RegionMod>();
  m->p = *p;
  m->body = body;
  m->camera = color_camera;
  m->depth_camera = p->measure_occlusions ? depth_camera : -1;
  m->model = model;
  RegionModDev& d = m->dev;
  d.body = body;
  d.camera = color_camera;
  d.depth_camera = m->depth_camera;
  d.points = mdl.points.as<float>();
  d.points8 = mdl.points8.as<float4>();
  d.orientations4 = mdl.orientations4.as<float4>();
  d.extents = mdl.extents.as<float>();
  d.n_views = mdl.n_views;
  d.n_points = mdl.n_points;
  d.max_extent = mdl.max_extent;
  d.n_lines_max = p->n_lines_max;
  d.use_adaptive_coverage = p->use_adaptive_coverage;
  d.reference_contour_length = p->reference_contour_length;
  d.min_continuous_distance = p->min_continuous_distance;
  d.function_length = p->function_length;
  d.distribution_length = p->distribution_length;
  d.n_seg = p->function_length + p->distribution_length - 1;
  // PrecalculateFunctionLookup region_modality.cpp:910-923
  for (int i = 0; i < p->function_length; ++i) {
    float x = float(i) - float(p->function_length - 1) / 2.0f;
    if (p->function_slope == 0.0f)
      d.function_lookup_f[i] = 0.5f - p->function_amplitude * ((0.0f < x) - (x < 0.0f));
    else
      d.function_lookup_f[i] = 0.5f - p->function_amplitude * std::tanh(x / (2.0f * p->function_slope));
    d.function_lookup_b[i] = 1.0f - d.function_lookup_f[i];
  }
  // PrecalculateDistributionVariables region_modality.cpp:925-936
  d.distribution_length_minus_1_half = (float(p->distribution_length) - 1.0f) / 2.0f;
  d.distribution_length_plus_1_half = (float(p->distribution_length) + 1.0f) / 2.0f;
  float mev_laplace = 1.0f / (2.0f * powf(atanhf(2.0f * p->function_amplitude), 2.0f));
  d.min_expected_variance = std::max(mev_laplace, p->function_slope);
  d.learning_rate = p->learning_rate;
  d.n_global_iterations = p->n_global_iterations;
  d.n_scales = p->n_scales;
  d.n_standard_deviations = p->n_standard_deviations;
  for (int i = 0; i < M3T_MAX_SCALES; ++i) {
    d.scales[i] = p->scales[i];
    d.standard_deviations[i] = p->standard_deviations[i];
  }
  for (int i = 0; i < p->n_scales; ++i)
    REQUIRE(p->scales[i] >= 1, M3T_ERR_INVALID_ARGUMENT, "scales must be >= 1");
  d.n_bins = p->n_histogram_bins;
  d.bitshift = bitshift;
  d.learning_rate_f = p->learning_rate_f;
  d.learning_rate_b = p->learning_rate_b;
  d.unconsidered_line_length = p->unconsidered_line_length;
  d.max_considered_line_length = p->max_considered_line_length;
  d.measure_occlusions = p->measure_occlusions;
  d.measured_depth_offset_id = 0;
  if (p->measure_occlusions) {  // PrecalculateModelVariables region_modality.cpp:966-991
    REQUIRE(p->measured_depth_offset_radius <= mdl.max_radius_depth_offset, M3T_ERR_INVALID_ARGUMENT,
            "Measured depth offset radius too large");
    d.measured_depth_offset_id = int(p->measured_depth_offset_radius / mdl.stride_depth_offset + 0.5f);
    REQUIRE(d.measured_depth_offset_id < M3T_N_DEPTH_OFFSETS, M3T_ERR_INVALID_ARGUMENT, "depth offset id out of range");
  }
  d.measured_occlusion_radius = p->measured_occlusion_radius;
  d.measured_occlusion_threshold = p->measured_occlusion_threshold;
  d.n_unoccluded_iterations = p->n_unoccluded_iterations;
  d.min_n_unoccluded_lines = p->min_n_unoccluded_lines;
  d.first_iteration = 0;
  size_t bins3 = size_t(d.n_bins) * d.n_bins * d.n_bins;
  HIPCHK(m->hist_f.alloc(bins3 * 4));
  HIPCHK(m->hist_b.alloc(bins3 * 4));
  HIPCHK(m->hist_norm.alloc(bins3 * 8));
  HIPCHK(m->occupancy.alloc(bins3 / 4));
  HIPCHK(hipMemset(m->occupancy.p, 1, bins3 / 4));  // (the uniform start histograms below: every group is non-zero)
  if (bins3 * 4 + M3T_MISC_FLOATS * 4 > 160 * 1024) HIPCHK(m->count_scratch.alloc(bins3 * 4));
  HIPCHK(m->line_state.alloc(size_t(LS_FIELDS) * d.n_lines_max * 4));
  HIPCHK(m->gh.alloc(48 * 4));  // 42 floats g / H, then (at [44]) the view of the last search (int, -1: none yet)
  HIPCHK(hipMemset(m->line_state.p, 0, m->line_state.bytes));
  HIPCHK(hipMemset(m->gh.p, 0, m->gh.bytes));
  HIPCHK(hipMemset(m->gh.as<int>() + 44, 0xff, 4));
  {  // SetUpHistograms color_histograms.cpp:160-172: uniform 1/n^3
    std::vector<float> u(bins3, 1.0f / float(bins3));
    std::vector<float> nrm(bins3 * 2, 0.5f);
    HIPCHK(hipMemcpy(m->hist_f.p, u.data(), bins3 * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m->hist_b.p, u.data(), bins3 * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m->hist_norm.p, nrm.data(), bins3 * 8, hipMemcpyHostToDevice));
  }
  d.histogram_f = m->hist_f.as<float>();
  d.histogram_b = m->hist_b.as<float>();
  d.histogram_norm = m->hist_norm.as<float2>();
  d.occupancy = m->occupancy.as<uint8_t>();
  d.count_scratch = m->count_scratch.as<uint32_t>();
  d.line_state = m->line_state.as<float>();
  d.gradient_hessian = m->gh.as<float>();
  d.view_neighbors = mdl.view_neighbors.as<float4>();
  d.last_view = m->gh.as<int>() + 44;
  ctx->region_mods.push_back(std::move(m));
  ctx->modalities.push_back({kRegionModality, int(ctx->region_mods.size()) - 1});
  ctx->tables_dirty = true;
  return int(ctx->modalities.size()) - 1;
}

int m3t_hip_depth_modality_create(m3t_hip_context* ctx, const m3t_depth_modality_params* p, int body, int depth_camera,
                                  int model) {
  CHECK_CTX();
  REQUIRE(p, M3T_ERR_INVALID_ARGUMENT, "null params");
  REQUIRE(body >= 0 && body < int(ctx->body_poses.size() / 16), M3T_ERR_INVALID_ARGUMENT, "bad body id");
  REQUIRE(depth_camera >= 0 && depth_camera < int(ctx->cameras.size()) && ctx->cameras[depth_camera]->is_depth,
          M3T_ERR_INVALID_ARGUMENT, "bad depth camera id");
  REQUIRE(model >= 0 && model < int(ctx->depth_models.size()), M3T_ERR_INVALID_ARGUMENT, "bad depth model id");
  REQUIRE(!p->use_silhouette_checking && !p->model_occlusions, M3T_ERR_INVALID_ARGUMENT,
          "switch silhouette checking / modelled occlusions on with their renderer afterwards");
  REQUIRE(p->n_considered_distances >= 1 && p->n_considered_distances <= M3T_MAX_SCALES &&
              p->n_standard_deviations >= 1 && p->n_standard_deviations <= M3T_MAX_SCALES && p->n_points_max >= 1,
          M3T_ERR_INVALID_ARGUMENT, "bad depth modality parameters");
  HIPCHK(hipSetDevice(ctx->device));
  const Model& mdl = *ctx->depth_models[model];
  auto m = std::make_unique<DepthMod>();
  m->p = *p;
  m->body = body;
  m->camera = depth_camera;
  m->model = model;
  DepthModDev& d = m->dev;
  d.body = body;
  d.camera = depth_camera;
  d.points = mdl.points.as<float>();
  d.points8 = mdl.points8.as<float4>();
  d.orientations4 = mdl.orientations4.as<float4>();
  d.extents = mdl.extents.as<float>();
  d.n_views = mdl.n_views;
  d.n_points = mdl.n_points;
  d.max_extent = mdl.max_extent;
  d.stride_depth_offset = mdl.stride_depth_offset;
  d.n_points_max = p->n_points_max;
  d.use_adaptive_coverage = p->use_adaptive_coverage;
  d.use_depth_scaling = p->use_depth_scaling;
  d.reference_surface_area = p->reference_surface_area;
  d.stride_length = p->stride_length;
  d.n_considered_distances = p->n_considered_distances;
  d.n_standard_deviations = p->n_standard_deviations;
  for (int i = 0; i < M3T_MAX_SCALES; ++i) {
    d.considered_distances[i] = p->considered_distances[i];
    d.standard_deviations[i] = p->standard_deviations[i];
  }
  d.measure_occlusions = p->measure_occlusions;
  d.measured_depth_offset_radius = p->measured_depth_offset_radius;
  d.measured_occlusion_radius = p->measured_occlusion_radius;
  d.measured_occlusion_threshold = p->measured_occlusion_threshold;
  d.n_unoccluded_iterations = p->n_unoccluded_iterations;
  d.min_n_unoccluded_points = p->min_n_unoccluded_points;
  d.first_iteration = 0;  // DepthModality never sets first_iteration_ (depth_modality.h:358)
  HIPCHK(m->point_state.alloc(size_t(PS_FIELDS) * d.n_points_max * 4));
  HIPCHK(m->gh.alloc(42 * 4));
  HIPCHK(hipMemset(m->point_state.p, 0, m->point_state.bytes));
  HIPCHK(hipMemset(m->gh.p, 0, m->gh.bytes));
  d.point_state = m->point_state.as<float>();
  d.gradient_hessian = m->gh.as<float>();
  ctx->depth_mods.push_back(std::move(m));
  ctx->modalities.push_back({kDepthModality, int(ctx->depth_mods.size()) - 1});
  ctx->tables_dirty = true;
  return int(ctx->modalities.size()) - 1;
}

static float* ModalityGh(m3t_hip_context* ctx, int id) {
  if (id < 0 || id >= int(ctx->modalities.size())) return nullptr;
  return ModalityGhPointer(ctx, ctx->modalities[id]);
}
int m3t_hip_modality_get_gradient_hessian(m3t_hip_context* ctx, int id, float g[6], float h[36]) {
  CHECK_CTX();
  float* d = ModalityGh(ctx, id);
  REQUIRE(d, M3T_ERR_INVALID_ARGUMENT, "bad modality id");
  REQUIRE(ctx->state_valid, M3T_ERR_NOT_SET_UP,
          "gradient/hessian are not written back in fused mode 1 (use m3t_hip_set_fused_step(ctx, 0 or 2))");
  HIPCHK(hipSetDevice(ctx->device));
  float buf[42];
  HIPCHK(hipMemcpyAsync(buf, d, sizeof(buf), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (g) std::memcpy(g, buf, 24);
  if (h) std::memcpy(h, buf + 6, 144);
  return M3T_OK;
}
}  // extern "C"
// gradient | Hessian of every modality into one contiguous buffer (one read-back per round for an adapter host)
extern "C" __global__ void gather_gradient_hessian_kernel(const float* const* sources, float* out) {
  out[blockIdx.x * 42 + threadIdx.x] = sources[blockIdx.x][threadIdx.x];
}
extern "C" {
int m3t_hip_modalities_get_gradient_hessian(m3t_hip_context* ctx, float* out, int capacity) {
  CHECK_CTX();
  const int n = int(ctx->modalities.size());
  REQUIRE(out && capacity >= n, M3T_ERR_INVALID_ARGUMENT, "the buffer must hold 42 floats per modality");
  REQUIRE(ctx->state_valid, M3T_ERR_NOT_SET_UP,
          "gradient/hessian are not written back in fused mode 1 (use m3t_hip_set_fused_step(ctx, 0 or 2))");
  if (n == 0) return M3T_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->gh_sources_count != n) {
    std::vector<const float*> src(size_t(n), nullptr);
    for (int i = 0; i < n; ++i) src[size_t(i)] = ModalityGh(ctx, i);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(UploadTable(&ctx->d_gh_sources, src));
    HIPCHK(ctx->d_gh_all.alloc(size_t(n) * 42 * sizeof(float)));
    ctx->gh_sources_count = n;
  }
  hipLaunchKernelGGL(gather_gradient_hessian_kernel, dim3(n), dim3(42), 0, ctx->stream,
                     ctx->d_gh_sources.as<const float*>(), ctx->d_gh_all.as<float>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, ctx->d_gh_all.p, size_t(n) * 42 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return M3T_OK;
}
int m3t_hip_modality_set_gradient_hessian(m3t_hip_context* ctx, int id, const float g[6], const float h[36]) {
  CHECK_CTX();
  float* d = ModalityGh(ctx, id);
  REQUIRE(d && g && h, M3T_ERR_INVALID_ARGUMENT, "bad modality id");
  HIPCHK(hipSetDevice(ctx->device));
  float buf[42];
  std::memcpy(buf, g, 24);
  std::memcpy(buf + 6, h, 144);
  HIPCHK(hipMemcpyAsync(d, buf, sizeof(buf), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->state_valid = true;
  return M3T_OK;
}

int m3t_hip_region_modality_get_lines(m3t_hip_context* ctx, int id, m3t_data_line* out, int capacity, int* n) {
  CHECK_CTX();
  RegionMod* m = GetRegion(ctx, id);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad region modality id");
  REQUIRE(ctx->state_valid, M3T_ERR_NOT_SET_UP,
          "line state is not written back in fused mode 1 (use m3t_hip_set_fused_step(ctx, 0 or 2))");
  HIPCHK(hipSetDevice(ctx->device));
  const int nl = m->p.n_lines_max;
  std::vector<float> st(size_t(LS_FIELDS) * nl);
  HIPCHK(hipMemcpyAsync(st.data(), m->line_state.p, st.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  int count = 0;
  for (int l = 0; l < nl; ++l) {
    int flags;
    std::memcpy(&flags, &st[size_t(LS_VALID) * nl + l], 4);
    if (!(flags & 1)) continue;
    if (out && count < capacity) {
      m3t_data_line& o = out[count];
      std::memset(&o, 0, sizeof(o));
      o.center_f_body[0] = st[size_t(LS_CX) * nl + l];
      o.center_f_body[1] = st[size_t(LS_CY) * nl + l];
      o.center_f_body[2] = st[size_t(LS_CZ) * nl + l];
      o.center_u = st[size_t(LS_CENTER_U) * nl + l];
      o.center_v = st[size_t(LS_CENTER_V) * nl + l];
      o.normal_u = st[size_t(LS_NORMAL_U) * nl + l];
      o.normal_v = st[size_t(LS_NORMAL_V) * nl + l];
      o.delta_r = st[size_t(LS_DELTA_R) * nl + l];
      o.normal_component_to_scale = st[size_t(LS_NCTS) * nl + l];
      o.continuous_distance = st[size_t(LS_CONT) * nl + l];
      o.mean = st[size_t(LS_MEAN) * nl + l];
      o.measured_variance = st[size_t(LS_VAR) * nl + l];
      for (int d = 0; d < m->p.distribution_length; ++d) o.distribution[d] = st[size_t(LS_DIST0 + d) * nl + l];
      o.valid = 1;
      o.model_point_index = l;
    }
    ++count;
  }
  if (n) *n = count;
  return M3T_OK;
}

int m3t_hip_depth_modality_get_points(m3t_hip_context* ctx, int id, m3t_data_point* out, int capacity, int* n) {
  CHECK_CTX();
  DepthMod* m = GetDepth(ctx, id);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad depth modality id");
  REQUIRE(ctx->state_valid, M3T_ERR_NOT_SET_UP,
          "point state is not written back in fused mode 1 (use m3t_hip_set_fused_step(ctx, 0 or 2))");
  HIPCHK(hipSetDevice(ctx->device));
  const int np = m->p.n_points_max;
  std::vector<float> st(size_t(PS_FIELDS) * np);
  HIPCHK(hipMemcpyAsync(st.data(), m->point_state.p, st.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  int count = 0;
  for (int i = 0; i < np; ++i) {
    int flags;
    std::memcpy(&flags, &st[size_t(PS_VALID) * np + i], 4);
    if (!(flags & 1)) continue;
    if (out && count < capacity) {
      m3t_data_point& o = out[count];
      std::memset(&o, 0, sizeof(o));
      for (int k = 0; k < 3; ++k) {
        o.center_f_body[k] = st[size_t(PS_CX + k) * np + i];
        o.normal_f_body[k] = st[size_t(PS_NX + k) * np + i];
        o.correspondence_center_f_camera[k] = st[size_t(PS_CORR_X + k) * np + i];
      }
      o.center_u = st[size_t(PS_CENTER_U) * np + i];
      o.center_v = st[size_t(PS_CENTER_V) * np + i];
      o.depth = st[size_t(PS_DEPTH) * np + i];
      o.valid = 1;
      o.model_point_index = i;
    }
    ++count;
  }
  if (n) *n = count;
  return M3T_OK;
}

int m3t_hip_region_modality_get_histograms(m3t_hip_context* ctx, int id, float* f, float* b) {
  CHECK_CTX();
  RegionMod* m = GetRegion(ctx, id);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad region modality id");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const size_t bytes = size_t(m->dev.n_bins) * m->dev.n_bins * m->dev.n_bins * 4;  // private or shared tables
  if (f) HIPCHK(hipMemcpy(f, m->dev.histogram_f, bytes, hipMemcpyDeviceToHost));
  if (b) HIPCHK(hipMemcpy(b, m->dev.histogram_b, bytes, hipMemcpyDeviceToHost));
  return M3T_OK;
}
int m3t_hip_region_modality_set_histograms(m3t_hip_context* ctx, int id, const float* f, const float* b) {
  CHECK_CTX();
  RegionMod* m = GetRegion(ctx, id);
  REQUIRE(m && f && b, M3T_ERR_INVALID_ARGUMENT, "bad region modality id");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  size_t bins3 = size_t(m->dev.n_bins) * m->dev.n_bins * m->dev.n_bins;
  std::vector<float> nrm(bins3 * 2);
  for (size_t i = 0; i < bins3; ++i) {  // MultiplyPixelColorProbability :1585-1593 per bin
    float pf = f[i], pb = b[i];
    if (pf || pb) {
      float sum = pf;
      sum += pb;
      nrm[2 * i] = pf / sum;
      nrm[2 * i + 1] = pb / sum;
    } else {
      nrm[2 * i] = 0.5f;
      nrm[2 * i + 1] = 0.5f;
    }
  }
  HIPCHK(hipMemcpy(m->dev.histogram_f, f, bins3 * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->dev.histogram_b, b, bins3 * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->dev.histogram_norm, nrm.data(), bins3 * 8, hipMemcpyHostToDevice));
  std::vector<uint8_t> occupied(bins3 / 4);
  for (size_t g = 0; g < bins3 / 4; ++g) {
    bool any = false;
    for (size_t k = 4 * g; k < 4 * g + 4; ++k) any = any || f[k] != 0.0f || b[k] != 0.0f;
    occupied[g] = any ? 1 : 0;
  }
  HIPCHK(hipMemcpy(m->dev.occupancy, occupied.data(), occupied.size(), hipMemcpyHostToDevice));
  return M3T_OK;
}

// ---- links / optimizers ---------------------------------------------------------------
static bool IsIdentity(const float* p) {
  if (!p) return true;
  static const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  return std::memcmp(p, ident, 64) == 0;
}
static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// m3t::Link (link.h:67): body may be -1 (pure joint), parent -1 = root
// ---- renderer-fed branches (a14 / f-3) ---------------------------------------------------------------
int m3t_hip_body_set_geometry(m3t_hip_context* ctx, int body, const m3t_body_geometry* g) {
  CHECK_CTX();
  REQUIRE(body >= 0 && body < int(ctx->body_poses.size() / 16) && g && g->vertices && g->triangles &&
              g->n_vertices >= 3 && g->n_triangles >= 1 && g->body_id >= 0 && g->body_id <= 255 &&
              g->region_id >= 0 && g->region_id <= 255,
          M3T_ERR_INVALID_ARGUMENT, "bad body geometry");
  for (int i = 0; i < g->n_triangles * 3; ++i)
    REQUIRE(g->triangles[i] >= 0 && g->triangles[i] < g->n_vertices, M3T_ERR_INVALID_ARGUMENT,
            "triangle index out of range");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (ctx->body_geometries.size() <= size_t(body)) ctx->body_geometries.resize(size_t(body) + 1);
  auto bg = std::make_unique<BodyGeometryH>();
  std::vector<int> tri(size_t(g->n_triangles) * 3);
  for (int t = 0; t < g->n_triangles; ++t)  // body.cpp:227-236
    for (int k = 0; k < 3; ++k)
      tri[size_t(t) * 3 + k] = g->triangles[size_t(t) * 3 + (g->geometry_counterclockwise ? k : 2 - k)];
  HIPCHK(bg->vertices.alloc(size_t(g->n_vertices) * 12));
  HIPCHK(bg->triangles.alloc(tri.size() * 4));
  HIPCHK(hipMemcpy(bg->vertices.p, g->vertices, size_t(g->n_vertices) * 12, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(bg->triangles.p, tri.data(), tri.size() * 4, hipMemcpyHostToDevice));
  bg->n_triangles = g->n_triangles;
  bg->h_vertices.assign(g->vertices, g->vertices + size_t(g->n_vertices) * 3);
  bg->h_triangles = tri;
  std::memcpy(bg->geometry2body, g->geometry2body, 64);
  bg->culling = g->geometry_enable_culling ? 1 : 0;
  bg->body_id = g->body_id;
  bg->region_id = g->region_id;
  float max_radius = 0.0f;  // Body::CalculateMaximumBodyDiameter body.cpp:244-250
  const float* m = g->geometry2body;
  for (int i = 0; i < g->n_vertices; ++i) {
    const float* v = g->vertices + size_t(i) * 3;
    float q[3];
    for (int k = 0; k < 3; ++k) q[k] = m[12 + k] + ((m[k] * v[0] + m[4 + k] * v[1]) + m[8 + k] * v[2]);
    max_radius = std::max(max_radius, std::sqrt(q[0] * q[0] + (q[1] * q[1] + q[2] * q[2])));
  }
  bg->maximum_body_diameter = 2.0f * max_radius;
  bg->set = true;
  ctx->body_geometries[body] = std::move(bg);
  ctx->tables_dirty = true;
  return M3T_OK;
}
static bool HasGeometry(m3t_hip_context* ctx, int body) {
  return body >= 0 && size_t(body) < ctx->body_geometries.size() && ctx->body_geometries[body] &&
         ctx->body_geometries[body]->set;
}
int m3t_hip_renderer_geometry_create(m3t_hip_context* ctx) {
  CHECK_CTX();
  ctx->renderer_geometries.emplace_back();
  return int(ctx->renderer_geometries.size()) - 1;
}
int m3t_hip_renderer_geometry_add_body(m3t_hip_context* ctx, int geometry, int body) {
  CHECK_CTX();
  REQUIRE(geometry >= 0 && geometry < int(ctx->renderer_geometries.size()) && body >= 0 &&
              body < int(ctx->body_poses.size() / 16),
          M3T_ERR_INVALID_ARGUMENT, "bad renderer geometry / body id");
  REQUIRE(HasGeometry(ctx, body), M3T_ERR_NOT_SET_UP, "body has no geometry");
  REQUIRE(ctx->renderer_geometries[geometry].size() < M3T_MAX_RENDERER_BODIES, M3T_ERR_UNSUPPORTED, "too many bodies");
  ctx->renderer_geometries[geometry].push_back(body);
  ctx->tables_dirty = true;
  return M3T_OK;
}
static int CreateRenderer(m3t_hip_context* ctx, bool silhouette, int geometry, int camera, int id_type, int image_size,
                          float z_min, float z_max) {
  CHECK_CTX();
  REQUIRE(geometry >= 0 && geometry < int(ctx->renderer_geometries.size()) && camera >= 0 &&
              camera < int(ctx->cameras.size()) && image_size >= 8 && image_size <= 1024 && z_min > 0.0f &&
              z_max > z_min && (id_type == M3T_ID_TYPE_BODY || id_type == M3T_ID_TYPE_REGION),
          M3T_ERR_INVALID_ARGUMENT, "bad renderer arguments");
  HIPCHK(hipSetDevice(ctx->device));
  auto r = std::make_unique<RendererH>();
  r->silhouette = silhouette;
  r->geometry = geometry;
  r->camera = camera;
  r->id_type = id_type;
  r->image_size = image_size;
  r->z_min = z_min;
  r->z_max = z_max;
  const size_t px = size_t(image_size) * image_size;
  HIPCHK(r->depth.alloc(px * 2));
  HIPCHK(r->sil.alloc(px));
  HIPCHK(r->packed.alloc(px * 4));
  HIPCHK(r->state.alloc(RS_FLOATS * 4));
  HIPCHK(hipMemset(r->state.p, 0, RS_FLOATS * 4));
  ctx->renderers.push_back(std::move(r));
  ctx->tables_dirty = true;
  return int(ctx->renderers.size()) - 1;
}
int m3t_hip_focused_depth_renderer_create(m3t_hip_context* ctx, int geometry, int camera, int image_size, float z_min,
                                          float z_max) {
  return CreateRenderer(ctx, false, geometry, camera, M3T_ID_TYPE_BODY, image_size, z_min, z_max);
}
int m3t_hip_focused_silhouette_renderer_create(m3t_hip_context* ctx, int geometry, int camera, int id_type,
                                               int image_size, float z_min, float z_max) {
  return CreateRenderer(ctx, true, geometry, camera, id_type, image_size, z_min, z_max);
}
int m3t_hip_renderer_add_referenced_body(m3t_hip_context* ctx, int renderer, int body) {
  CHECK_CTX();
  REQUIRE(renderer >= 0 && renderer < int(ctx->renderers.size()) && body >= 0 && body < int(ctx->body_poses.size() / 16),
          M3T_ERR_INVALID_ARGUMENT, "bad renderer / body id");
  REQUIRE(HasGeometry(ctx, body), M3T_ERR_NOT_SET_UP, "body has no geometry");
  RendererH& r = *ctx->renderers[renderer];
  REQUIRE(r.referenced.size() < M3T_MAX_RENDERER_BODIES, M3T_ERR_UNSUPPORTED, "too many referenced bodies");
  r.referenced.push_back(body);
  r.rendered = false;
  ctx->tables_dirty = true;
  return M3T_OK;
}
int m3t_hip_renderer_start_rendering(m3t_hip_context* ctx, int renderer) {
  CHECK_CTX();
  REQUIRE(renderer >= 0 && renderer < int(ctx->renderers.size()), M3T_ERR_INVALID_ARGUMENT, "bad renderer id");
  REQUIRE(!ctx->renderers[renderer]->referenced.empty(), M3T_ERR_NOT_SET_UP, "no referenced body");
  HIPCHK(hipSetDevice(ctx->device));
  int r = Prepare(ctx, false);
  if (r) return r;
  DevMem which;  // freed after the synchronisation below
  const int pair[2] = {renderer, -1};
  HIPCHK(which.alloc(8));
  HIPCHK(hipMemcpy(which.p, pair, 8, hipMemcpyHostToDevice));
  if ((r = LaunchRenderers(ctx, which.as<int>(), 1, which.as<int>(), 1, ctx->renderers[renderer]->image_size))) return r;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->renderers[renderer]->rendered = true;
  return M3T_OK;
}
int m3t_hip_renderer_get_images(m3t_hip_context* ctx, int renderer, uint16_t* depth, uint8_t* silhouette,
                                float info[3], int* n_visible) {
  CHECK_CTX();
  REQUIRE(renderer >= 0 && renderer < int(ctx->renderers.size()), M3T_ERR_INVALID_ARGUMENT, "bad renderer id");
  RendererH& r = *ctx->renderers[renderer];
  REQUIRE(r.rendered, M3T_ERR_NOT_SET_UP, "renderer has not rendered yet");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const size_t px = size_t(r.image_size) * r.image_size;
  if (depth) HIPCHK(hipMemcpy(depth, r.depth.p, px * 2, hipMemcpyDeviceToHost));
  if (silhouette) HIPCHK(hipMemcpy(silhouette, r.sil.p, px, hipMemcpyDeviceToHost));
  float state[RS_FLOATS];
  HIPCHK(hipMemcpy(state, r.state.p, sizeof(state), hipMemcpyDeviceToHost));
  if (info) { info[0] = state[RS_CORNER_U]; info[1] = state[RS_CORNER_V]; info[2] = state[RS_SCALE]; }
  if (n_visible) *n_visible = int(state[RS_N_VISIBLE]);
  return M3T_OK;
}
static int CheckAttach(m3t_hip_context* ctx, int modality, int renderer, bool want_region, bool want_silhouette,
                       int body) {
  REQUIRE(renderer >= 0 && renderer < int(ctx->renderers.size()) &&
              ctx->renderers[renderer]->silhouette == want_silhouette,
          M3T_ERR_INVALID_ARGUMENT, "bad renderer id / kind");
  bool referenced = false;
  for (int b : ctx->renderers[renderer]->referenced) referenced |= b == body;
  REQUIRE(referenced, M3T_ERR_INVALID_ARGUMENT, "the modality's body is not referenced by the renderer");
  return M3T_OK;
}
int m3t_hip_region_modality_model_occlusions(m3t_hip_context* ctx, int modality, int renderer) {
  CHECK_CTX();
  RegionMod* m = GetRegion(ctx, modality);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad region modality id");
  int r = CheckAttach(ctx, modality, renderer, true, false, m->body);
  if (r) return r;
  const Model& mdl = *ctx->region_models[m->model];
  REQUIRE(m->p.modeled_depth_offset_radius <= mdl.max_radius_depth_offset, M3T_ERR_INVALID_ARGUMENT,
          "Modeled depth offset radius too large");
  m->depth_renderer = renderer;
  m->p.model_occlusions = 1;
  m->dev.model_occlusions = 1;
  m->dev.modeled_depth_offset_id = int(m->p.modeled_depth_offset_radius / mdl.stride_depth_offset + 0.5f);
  m->dev.modeled_occlusion_radius = m->p.modeled_occlusion_radius;
  m->dev.modeled_occlusion_threshold = m->p.modeled_occlusion_threshold;
  ctx->tables_dirty = true;
  return M3T_OK;
}
int m3t_hip_region_modality_use_region_checking(m3t_hip_context* ctx, int modality, int renderer) {
  CHECK_CTX();
  RegionMod* m = GetRegion(ctx, modality);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad region modality id");
  int r = CheckAttach(ctx, modality, renderer, true, true, m->body);
  if (r) return r;
  m->silhouette_renderer = renderer;
  m->p.use_region_checking = 1;
  m->dev.use_region_checking = 1;
  m->dev.region_id = ctx->body_geometries[m->body]->region_id;
  ctx->tables_dirty = true;
  return M3T_OK;
}
int m3t_hip_depth_modality_model_occlusions(m3t_hip_context* ctx, int modality, int renderer) {
  CHECK_CTX();
  REQUIRE(modality >= 0 && modality < int(ctx->modalities.size()) && ctx->modalities[modality].kind == kDepthModality,
          M3T_ERR_INVALID_ARGUMENT, "bad depth modality id");
  DepthMod* m = ctx->depth_mods[ctx->modalities[modality].index].get();
  int r = CheckAttach(ctx, modality, renderer, false, false, m->body);
  if (r) return r;
  m->depth_renderer = renderer;
  m->p.model_occlusions = 1;
  m->dev.model_occlusions = 1;
  m->dev.modeled_depth_offset_radius = m->p.modeled_depth_offset_radius;
  m->dev.modeled_occlusion_radius = m->p.modeled_occlusion_radius;
  m->dev.modeled_occlusion_threshold = m->p.modeled_occlusion_threshold;
  ctx->tables_dirty = true;
  return M3T_OK;
}
int m3t_hip_depth_modality_use_silhouette_checking(m3t_hip_context* ctx, int modality, int renderer) {
  CHECK_CTX();
  REQUIRE(modality >= 0 && modality < int(ctx->modalities.size()) && ctx->modalities[modality].kind == kDepthModality,
          M3T_ERR_INVALID_ARGUMENT, "bad depth modality id");
  DepthMod* m = ctx->depth_mods[ctx->modalities[modality].index].get();
  int r = CheckAttach(ctx, modality, renderer, false, true, m->body);
  if (r) return r;
  m->silhouette_renderer = renderer;
  m->p.use_silhouette_checking = 1;
  m->dev.use_silhouette_checking = 1;
  m->dev.body_id = ctx->body_geometries[m->body]->body_id;
  ctx->tables_dirty = true;
  return M3T_OK;
}

// ---- TextureModality behind its feature detector (m3t_texture.hip) --------------------------------------------------
static int CreateTextureModality(m3t_hip_context* ctx, const m3t_texture_modality_params* p, int body, int color_camera,
                                 int silhouette_renderer, int depth_camera, bool l2) {
  CHECK_CTX();
  REQUIRE(p, M3T_ERR_INVALID_ARGUMENT, "null params");
  REQUIRE(body >= 0 && body < int(ctx->body_poses.size() / 16), M3T_ERR_INVALID_ARGUMENT, "bad body id");
  REQUIRE(color_camera >= 0 && color_camera < int(ctx->cameras.size()) && !ctx->cameras[color_camera]->is_depth,
          M3T_ERR_INVALID_ARGUMENT, "bad color camera id");
  if (p->measure_occlusions)
    REQUIRE(depth_camera >= 0 && depth_camera < int(ctx->cameras.size()) && ctx->cameras[depth_camera]->is_depth,
            M3T_ERR_INVALID_ARGUMENT, "measure_occlusions needs a depth camera");
  if (l2)
    REQUIRE(p->descriptor_bytes % 16 == 0 && p->descriptor_bytes >= 4 * M3T_TEXTURE_L2_MIN_FLOATS &&
                p->descriptor_bytes <= 4 * M3T_TEXTURE_L2_MAX_FLOATS,
            M3T_ERR_INVALID_ARGUMENT,
            "descriptor_bytes must be 4 * D for D floats a descriptor, a multiple of 16 in [16, 1024] (SIFT: 512)");
  else
    REQUIRE(p->descriptor_bytes == 32 || p->descriptor_bytes == 64, M3T_ERR_INVALID_ARGUMENT,
            "descriptor_bytes must be 32 (ORB) or 64 (BRISK, FREAK): Hamming-norm descriptors only");
  REQUIRE(p->n_keyframes >= 1 && p->n_keyframes <= M3T_MAX_TEXTURE_KEYFRAMES && p->n_standard_deviations >= 1 &&
              p->n_standard_deviations <= M3T_MAX_SCALES && p->focused_image_size >= 1,
          M3T_ERR_INVALID_ARGUMENT, "bad texture modality parameters");
  REQUIRE(silhouette_renderer >= 0 && silhouette_renderer < int(ctx->renderers.size()), M3T_ERR_INVALID_ARGUMENT,
          "bad renderer id");
  {
    const RendererH& r = *ctx->renderers[silhouette_renderer];
    // (the reference only warns, :59-63; with REGION ids the silhouette test of Reconstruct3DPoint matches nothing)
    REQUIRE(r.silhouette && r.id_type == M3T_ID_TYPE_BODY, M3T_ERR_INVALID_ARGUMENT,
            "the texture modality needs a focused silhouette renderer with id_type BODY");
    REQUIRE(r.camera == color_camera, M3T_ERR_INVALID_ARGUMENT, "the silhouette renderer has to render the color camera's view");
  }
  int r = CheckAttach(ctx, -1, silhouette_renderer, false, true, body);
  if (r) return r;
  REQUIRE(HasGeometry(ctx, body), M3T_ERR_NOT_SET_UP, "the texture modality's body needs its geometry (body_set_geometry)");
  REQUIRE(!ctx->roi_enabled, M3T_ERR_UNSUPPORTED, "a texture modality and ROI ingest do not go together");
  REQUIRE(!ctx->Distributed(), M3T_ERR_UNSUPPORTED,
          "a texture modality and a communicator / reduce callback do not go together");
  HIPCHK(hipSetDevice(ctx->device));
  auto m = std::make_unique<TextureMod>();
  m->p = *p;
  m->body = body;
  m->camera = color_camera;
  m->depth_camera = p->measure_occlusions ? depth_camera : -1;
  m->silhouette_renderer = silhouette_renderer;
  TextureModDev& d = m->dev;
  d.body = body;
  d.camera = color_camera;
  d.depth_camera = m->depth_camera;
  d.descriptor_words = p->descriptor_bytes / 4;
  d.n_keyframes_max = p->n_keyframes;
  d.descriptor_distance_threshold = p->descriptor_distance_threshold;
  d.tukey_norm_constant = p->tukey_norm_constant;
  d.n_standard_deviations = p->n_standard_deviations;
  for (int i = 0; i < M3T_MAX_SCALES; ++i) d.standard_deviations[i] = p->standard_deviations[i];
  d.max_keyframe_rotation_difference = p->max_keyframe_rotation_difference;
  d.max_keyframe_age = p->max_keyframe_age;
  d.measure_occlusions = p->measure_occlusions ? 1 : 0;
  d.measured_occlusion_radius = p->measured_occlusion_radius;
  d.measured_occlusion_threshold = p->measured_occlusion_threshold;
  d.model_occlusions = 0;
  d.body_id = ctx->body_geometries[body]->body_id;
  d.modeled_occlusion_radius = p->modeled_occlusion_radius;
  d.modeled_occlusion_threshold = p->modeled_occlusion_threshold;
  const size_t words = size_t(d.descriptor_words), slots = size_t(p->n_keyframes) * M3T_TEXTURE_MAX_FEATURES;
  HIPCHK(m->features.alloc((TF_HEADER_WORDS + (2 + words) * M3T_TEXTURE_MAX_FEATURES) * 4));
  HIPCHK(m->keyframe_points.alloc(slots * 3 * 4));
  HIPCHK(m->keyframe_descriptors.alloc(slots * words * 4));
  HIPCHK(m->data_points.alloc(slots * TP_FLOATS * 4));
  HIPCHK(m->state.alloc(sizeof(TextureStateDev)));
  HIPCHK(m->gh.alloc(42 * 4));
  if (l2) {
    m->l2 = true;
    HIPCHK(m->best.alloc(slots * 3 * 4));
  }
  HIPCHK(hipMemset(m->features.p, 0, TF_HEADER_WORDS * 4));
  HIPCHK(hipMemset(m->state.p, 0, m->state.bytes));
  HIPCHK(hipMemset(m->gh.p, 0, m->gh.bytes));
  d.features = m->features.as<uint32_t>();
  d.keyframe_points = m->keyframe_points.as<float>();
  d.keyframe_descriptors = m->keyframe_descriptors.as<uint32_t>();
  d.data_points = m->data_points.as<float>();
  d.state = m->state.as<TextureStateDev>();
  d.gradient_hessian = m->gh.as<float>();
  ctx->texture_mods.push_back(std::move(m));
  ctx->modalities.push_back({kTextureModality, int(ctx->texture_mods.size()) - 1});
  ctx->tables_dirty = true;
  return int(ctx->modalities.size()) - 1;
}
int m3t_hip_texture_modality_create(m3t_hip_context* ctx, const m3t_texture_modality_params* p, int body, int color_camera,
                                    int silhouette_renderer, int depth_camera) {
  return CreateTextureModality(ctx, p, body, color_camera, silhouette_renderer, depth_camera, false);
}
int m3t_hip_texture_modality_create_l2(m3t_hip_context* ctx, const m3t_texture_modality_params* p, int body, int color_camera,
                                       int silhouette_renderer, int depth_camera) {
  return CreateTextureModality(ctx, p, body, color_camera, silhouette_renderer, depth_camera, true);
}
int m3t_hip_texture_modality_model_occlusions(m3t_hip_context* ctx, int modality, int renderer) {
  CHECK_CTX();
  TextureMod* m = GetTexture(ctx, modality);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad texture modality id");
  int r = CheckAttach(ctx, modality, renderer, false, false, m->body);
  if (r) return r;
  REQUIRE(ctx->renderers[renderer]->camera == m->camera, M3T_ERR_INVALID_ARGUMENT,
          "the depth renderer has to render the color camera's view");
  m->depth_renderer = renderer;
  m->dev.model_occlusions = 1;
  ctx->tables_dirty = true;
  return M3T_OK;
}
int m3t_hip_texture_modality_get_region_of_interest(m3t_hip_context* ctx, int modality, int roi[4], float* scale, int* valid) {
  CHECK_CTX();
  TextureMod* m = GetTexture(ctx, modality);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad texture modality id");
  REQUIRE(roi && scale && valid, M3T_ERR_INVALID_ARGUMENT, "null output");
  float pose[16];
  int r = m3t_hip_body_get_body2world_pose(ctx, m->body, pose);  // (waits for the stream when the device is ahead)
  if (r) return r;
  const Camera& c = *ctx->cameras[m->camera];
  // translation of world2camera * body2world: L t + t_camera, Transform * Transform as the kernels form it (mul_pose)
  const float* w = c.world2camera;
  float t[3];
  for (int k = 0; k < 3; ++k) t[k] = ((w[k] * pose[12] + w[4 + k] * pose[13]) + w[8 + k] * pose[14]) + w[12 + k];
  const float radius = 0.5f * ctx->body_geometries[m->body]->maximum_body_diameter;
  *valid = m3t_tex_region_of_interest(t, radius, c.intr.fu, c.intr.fv, c.intr.ppu, c.intr.ppv, c.intr.width, c.intr.height,
                                      m->p.focused_image_size, roi, scale)
               ? 1
               : 0;
  return M3T_OK;
}
int m3t_hip_texture_modality_set_features(m3t_hip_context* ctx, int modality, const float* keypoints_xy,
                                          const uint8_t* descriptors, int n) {
  CHECK_CTX();
  TextureMod* m = GetTexture(ctx, modality);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad texture modality id");
  REQUIRE(n >= 0 && n <= M3T_MAX_TEXTURE_FEATURES, M3T_ERR_INVALID_ARGUMENT,
          "set_features: n must be in [0, " + std::to_string(M3T_MAX_TEXTURE_FEATURES) + "]");
  REQUIRE(n == 0 || (keypoints_xy && descriptors), M3T_ERR_INVALID_ARGUMENT, "set_features: null features");
  REQUIRE(!m->builtin, M3T_ERR_UNSUPPORTED,
          "set_features: the modality detects its features itself (texture_modality_set_detector(NULL) hands them back to the caller)");
  HIPCHK(hipSetDevice(ctx->device));
  // one block: {n, 0, 0, 0} | keypoints | descriptors; two copies on the context's stream, behind whatever it holds
  const size_t head_bytes = TF_HEADER_WORDS * 4 + size_t(n) * 8, descriptor_bytes = size_t(n) * m->p.descriptor_bytes;
  void *host = nullptr, *dev = nullptr;
  int slot = 0;
  HIPCHK(m->uploads.Acquire(head_bytes + descriptor_bytes, &host, &dev, &slot));
  uint8_t* block = static_cast<uint8_t*>(host);
  const uint32_t header[TF_HEADER_WORDS] = {uint32_t(n), 0u, 0u, 0u};
  std::memcpy(block, header, sizeof(header));
  if (n) {
    std::memcpy(block + sizeof(header), keypoints_xy, size_t(n) * 8);
    std::memcpy(block + head_bytes, descriptors, descriptor_bytes);
  }
  uint8_t* target = m->features.as<uint8_t>();
  HIPCHK(hipMemcpyAsync(target, block, head_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (n)
    HIPCHK(hipMemcpyAsync(target + (TF_HEADER_WORDS + 2 * M3T_TEXTURE_MAX_FEATURES) * 4, block + head_bytes, descriptor_bytes,
                          hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(m->uploads.Release(slot, ctx->stream));
  ctx->ingest.LaunchedUntracked();  // (copies on the compute stream behind no step event)
  return M3T_OK;
}
int m3t_hip_texture_modality_set_detector(m3t_hip_context* ctx, int modality, const m3t_texture_detector_params* p) {
  CHECK_CTX();
  TextureMod* m = GetTexture(ctx, modality);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad texture modality id");
  if (!p) {  // back to the caller's features (the images stay allocated: a later set_detector finds them)
    if (m->builtin) ctx->tables_dirty = true;
    m->builtin = false;
    return M3T_OK;
  }
  REQUIRE(!m->l2, M3T_ERR_UNSUPPORTED,
          "set_detector: the built-in detector writes 32-byte binary descriptors, the modality matches rows of floats with the L2 norm");
  REQUIRE(p->type == M3T_TEXTURE_DETECTOR_BUILTIN, M3T_ERR_INVALID_ARGUMENT, "set_detector: unknown detector type");
  REQUIRE(p->n_features >= 1 && p->n_features <= M3T_MAX_TEXTURE_FEATURES, M3T_ERR_INVALID_ARGUMENT,
          "set_detector: n_features must be in [1, " + std::to_string(M3T_MAX_TEXTURE_FEATURES) + "]");
  REQUIRE(p->fast_threshold >= 0 && p->fast_threshold <= 255, M3T_ERR_INVALID_ARGUMENT,
          "set_detector: fast_threshold must be in [0, 255]");
  REQUIRE(m->p.descriptor_bytes == 32, M3T_ERR_UNSUPPORTED, "set_detector: the built-in detector writes 32-byte descriptors");
  REQUIRE(m->p.focused_image_size <= M3T_TEXTURE_FOCUSED_MAX, M3T_ERR_UNSUPPORTED,
          "set_detector: focused_image_size must not exceed " + std::to_string(M3T_TEXTURE_FOCUSED_MAX));
  HIPCHK(hipSetDevice(ctx->device));
  if (!m->focused.p) {
    const size_t pixels = size_t(M3T_TEXTURE_FOCUSED_MAX) * M3T_TEXTURE_FOCUSED_MAX;
    HIPCHK(m->focused.alloc(pixels));
    HIPCHK(m->scores.alloc(pixels * 2));
    HIPCHK(m->boxes.alloc(pixels * 2));
    HIPCHK(m->detector_header.alloc(DH_WORDS * 4));
    HIPCHK(hipMemset(m->detector_header.p, 0, DH_WORDS * 4));
  }
  m->detector = *p;
  m->builtin = true;
  ctx->tables_dirty = true;
  return M3T_OK;
}
// what the last detection left (synchronous; for tests and for a caller who wants to look)
static int ReadDetectorHeader(Ctx* ctx, TextureMod* m, int header[DH_WORDS]) {
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(header, m->detector_header.p, DH_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return M3T_OK;
}
int m3t_hip_texture_modality_get_features(m3t_hip_context* ctx, int modality, float* keypoints_xy, uint8_t* descriptors,
                                          int capacity, int* n_features) {
  CHECK_CTX();
  TextureMod* m = GetTexture(ctx, modality);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad texture modality id");
  REQUIRE(n_features && capacity >= 0 && ((keypoints_xy && descriptors) || capacity == 0), M3T_ERR_INVALID_ARGUMENT,
          "bad output buffer");
  HIPCHK(hipSetDevice(ctx->device));
  uint32_t header[TF_HEADER_WORDS];
  HIPCHK(hipMemcpyAsync(header, m->features.p, sizeof(header), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *n_features = int(header[0]);
  const int n = std::min(int(header[0]), capacity);
  if (n > 0) {
    const uint8_t* block = m->features.as<uint8_t>();
    HIPCHK(hipMemcpy(keypoints_xy, block + TF_HEADER_WORDS * 4, size_t(n) * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(descriptors, block + (TF_HEADER_WORDS + 2 * M3T_TEXTURE_MAX_FEATURES) * 4,
                     size_t(n) * m->p.descriptor_bytes, hipMemcpyDeviceToHost));
  }
  return M3T_OK;
}
int m3t_hip_texture_modality_get_focused_image(m3t_hip_context* ctx, int modality, uint8_t* pixels, int capacity, int* width,
                                               int* height) {
  CHECK_CTX();
  TextureMod* m = GetTexture(ctx, modality);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad texture modality id");
  REQUIRE(width && height && capacity >= 0 && (pixels || capacity == 0), M3T_ERR_INVALID_ARGUMENT, "bad output buffer");
  REQUIRE(m->detector_header.p, M3T_ERR_NOT_SET_UP, "get_focused_image: the modality has had no built-in detector");
  int header[DH_WORDS];
  int r = ReadDetectorHeader(ctx, m, header);
  if (r) return r;
  *width = header[DH_WIDTH];
  *height = header[DH_HEIGHT];
  const size_t bytes = size_t(header[DH_WIDTH]) * size_t(header[DH_HEIGHT]);
  if (pixels && bytes > 0) {
    REQUIRE(size_t(capacity) >= bytes, M3T_ERR_INVALID_ARGUMENT,
            "get_focused_image: the focused image has " + std::to_string(bytes) + " pixels");
    HIPCHK(hipMemcpy(pixels, m->focused.p, bytes, hipMemcpyDeviceToHost));
  }
  return M3T_OK;
}
int m3t_hip_texture_modality_get_points(m3t_hip_context* ctx, int modality, m3t_texture_data_point* out, int capacity,
                                        int* n_points) {
  CHECK_CTX();
  TextureMod* m = GetTexture(ctx, modality);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad texture modality id");
  REQUIRE(n_points && capacity >= 0 && (out || capacity == 0), M3T_ERR_INVALID_ARGUMENT, "bad output buffer");
  static_assert(sizeof(m3t_texture_data_point) == TP_FLOATS * 4, "the kernels write m3t_texture_data_point rows");
  HIPCHK(hipSetDevice(ctx->device));
  TextureStateDev st;
  HIPCHK(hipMemcpyAsync(&st, m->state.p, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *n_points = st.n_data_points;
  const int n = std::min(st.n_data_points, capacity);
  if (n > 0) HIPCHK(hipMemcpy(out, m->data_points.p, size_t(n) * sizeof(m3t_texture_data_point), hipMemcpyDeviceToHost));
  return M3T_OK;
}
int m3t_hip_texture_modality_get_keyframes(m3t_hip_context* ctx, int modality, int* n_keyframes, int* keyframe_age,
                                           int* counts, float* points_xyz, int capacity_points) {
  CHECK_CTX();
  TextureMod* m = GetTexture(ctx, modality);
  REQUIRE(m, M3T_ERR_INVALID_ARGUMENT, "bad texture modality id");
  HIPCHK(hipSetDevice(ctx->device));
  TextureStateDev st;
  HIPCHK(hipMemcpyAsync(&st, m->state.p, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  int total = 0;
  for (int k = 0; k < st.n_keyframes; ++k) total += st.counts[(st.head + k) % m->p.n_keyframes];
  REQUIRE(!points_xyz || capacity_points >= total, M3T_ERR_INVALID_ARGUMENT,
          "get_keyframes: the keyframes hold " + std::to_string(total) + " points");
  if (n_keyframes) *n_keyframes = st.n_keyframes;
  if (keyframe_age) *keyframe_age = st.keyframe_age;
  size_t at = 0;
  for (int k = 0; k < M3T_MAX_TEXTURE_KEYFRAMES; ++k) {
    const int slot = (st.head + k) % m->p.n_keyframes;
    const int count = k < st.n_keyframes ? st.counts[slot] : 0;
    if (counts) counts[k] = count;
    if (points_xyz && count > 0)
      HIPCHK(hipMemcpy(points_xyz + at * 3, m->keyframe_points.as<float>() + size_t(slot) * M3T_TEXTURE_MAX_FEATURES * 3,
                       size_t(count) * 12, hipMemcpyDeviceToHost));
    at += size_t(count);
  }
  return M3T_OK;
}

// ---- model generation (f-1) ---------------------------------------------------------------------------
// groups (RegionModel::AddAssociatedBody region_model.cpp:365-388): 0 fixed, 1 movable, 2 fixed same-region,
// 3 movable same-region; for the depth model 0 = occlusion bodies (DepthModel::AddOcclusionBody depth_model.cpp:61-70)
static int GenerateModel(m3t_hip_context* ctx, bool region, int body, const m3t_model_generation_params* p,
                         const std::vector<int> (&groups)[4] = {}) {
  CHECK_CTX();
  REQUIRE(p && p->sphere_radius > 0.0f && p->n_divides >= 0 && p->n_divides <= 6 && p->n_points >= 1 &&
              p->image_size >= 64 && p->image_size <= 4096 && p->stride_depth_offset > 0.0f &&
              p->max_radius_depth_offset >= 0.0f &&
              int(p->max_radius_depth_offset / p->stride_depth_offset + 1.0f) <= M3T_N_DEPTH_OFFSETS,
          M3T_ERR_INVALID_ARGUMENT, "bad model generation parameters");
  REQUIRE(HasGeometry(ctx, body), M3T_ERR_NOT_SET_UP, "body has no geometry");
  for (auto& grp : groups)
    for (int b : grp) REQUIRE(HasGeometry(ctx, b) && b != body, M3T_ERR_NOT_SET_UP, "associated body has no geometry");
  HIPCHK(hipSetDevice(ctx->device));
  using namespace modelgen;
  const BodyGeometryH& g = *ctx->body_geometries[body];
  const int S = p->image_size;
  const float d = g.maximum_body_diameter, radius = p->sphere_radius;
  REQUIRE(0.5f * d < radius, M3T_ERR_INVALID_ARGUMENT, "sphere radius smaller than the body");
  // Model::SetUpRenderer model.cpp:120-153: intrinsics from the main body
  const float fu = 0.5f * float(S - 20) / tanf(asinf(0.5f * d / radius));
  const float pp = float(S) / 2.0f;
  // the renderers of one view: which bodies are drawn, in which order, with which id.  Renderers that draw the same
  // bodies share one rasterisation; their silhouette images differ only in the ids.
  constexpr uint8_t M = 255, B = 0, D = 120;  // kMainBodyID, kBackgroundID, kDifferentBodyID
  struct Draw { int body; uint8_t id; };
  struct Renderer { std::vector<Draw> draws; };
  auto draws = [&](std::initializer_list<std::pair<const std::vector<int>*, uint8_t>> parts, uint8_t main_id) {
    Renderer r;
    r.draws.push_back({body, main_id});
    for (auto& part : parts)
      for (int b : *part.first) r.draws.push_back({b, part.second});
    return r;
  };
  const std::vector<int>&fixed = groups[0], &movable = groups[1], &fixed_same = groups[2], &movable_same = groups[3];
  const bool any_associated = !fixed.empty() || !movable.empty() || !fixed_same.empty() || !movable_same.empty();
  enum { R_MAIN = 0, R_OCCLUSION, R_SAME_REGION, R_FOREGROUND, R_BACKGROUND, N_RENDERERS };
  Renderer renderers[N_RENDERERS];
  bool used[N_RENDERERS] = {true, false, false, false, false};
  if (region) {  // region_model.cpp:207-213, 417-463
    renderers[R_MAIN] = draws({{&fixed, D}}, M);
    if (!movable.empty()) {
      renderers[R_OCCLUSION] = draws({{&fixed, B}, {&movable, M}}, B);
      used[R_OCCLUSION] = true;
    }
    if (!fixed_same.empty() || !movable_same.empty()) {
      renderers[R_SAME_REGION] = draws({{&fixed, B}, {&fixed_same, M}, {&movable_same, M}}, B);
      used[R_SAME_REGION] = true;
    }
    if (!movable.empty() || !fixed_same.empty() || !movable_same.empty()) {
      renderers[R_FOREGROUND] = draws({{&fixed, B}, {&movable, B}, {&fixed_same, M}}, M);
      renderers[R_BACKGROUND] = draws({{&fixed, B}, {&fixed_same, M}, {&movable_same, M}}, M);
      used[R_FOREGROUND] = used[R_BACKGROUND] = true;
    }
  } else {  // depth_model.cpp:165-177: the main (normal) renderer draws the body alone
    renderers[R_MAIN] = draws({}, M);
    if (!fixed.empty()) {
      renderers[R_OCCLUSION] = draws({{&fixed, B}}, M);
      used[R_OCCLUSION] = true;
    }
  }
  for (auto& r : renderers) REQUIRE(r.draws.size() <= 64, M3T_ERR_UNSUPPORTED, "more than 63 associated bodies");
  // clip range of a renderer: widened to every body it draws (Model::AddBodiesToRenderer model.cpp:164-192)
  auto clip_range = [&](const Renderer& r, float* z_min, float* z_max) {
    *z_min = radius - d * 0.5f;
    *z_max = radius + d * 0.5f;
    for (const Draw& dr : r.draws) {
      const float db = ctx->body_geometries[dr.body]->maximum_body_diameter;
      *z_min = std::min(*z_min, radius - db * 0.5f);
      *z_max = std::max(*z_max, radius + db * 0.5f);
    }
  };
  auto projection = [&](float z_min, float z_max) {
    P4 P;
    for (float& f : P.m) f = 0.0f;  // FullRenderer::CalculateProjectionMatrix renderer.cpp:257-264
    P(0, 0) = 2.0f * fu / float(S);
    P(0, 2) = 2.0f * (pp + 0.5f) / float(S) - 1.0f;
    P(1, 1) = 2.0f * fu / float(S);
    P(1, 2) = 2.0f * (pp + 0.5f) / float(S) - 1.0f;
    P(2, 2) = (z_max + z_min) / (z_max - z_min);
    P(2, 3) = -2.0f * z_max * z_min / (z_max - z_min);
    P(3, 2) = 1.0f;
    return P;
  };
  {
    float z_min, z_max;
    for (int r = 0; r < N_RENDERERS; ++r)
      if (used[r]) {
        clip_range(renderers[r], &z_min, &z_max);
        REQUIRE(z_min >= radius * 0.2f, M3T_ERR_INVALID_ARGUMENT,  // kMinimumClipSpaceRatio model.h:59
                "z_min too small for the model's sphere radius");
      }
  }
  P4 g2b;
  std::memcpy(g2b.m, g.geometry2body, 64);
  const std::vector<P4> poses = GeodesicPoses(p->n_divides, radius);
  const int n_views = int(poses.size());
  const int pf = region ? M3T_REGION_POINT_FLOATS : M3T_DEPTH_POINT_FLOATS;
  std::vector<float> points(size_t(n_views) * p->n_points * pf), orientations(size_t(n_views) * 3), extents(n_views);
  const size_t px = size_t(S) * S;
  const int batch = int(std::max<size_t>(1, std::min<size_t>(16, (size_t(768) << 20) / (px * 8))));
  DevMem d_z, d_trans, d_depth, d_tri, d_body;
  HIPCHK(d_z.alloc(size_t(batch) * px * 8));
  HIPCHK(d_trans.alloc(size_t(batch) * 64));
  HIPCHK(d_depth.alloc(size_t(batch) * px * 2));
  if (!region) HIPCHK(d_tri.alloc(size_t(batch) * px * 4));
  if (any_associated) HIPCHK(d_body.alloc(size_t(batch) * px));
  std::vector<uint16_t> h_depth(size_t(batch) * px);
  std::vector<int> h_tri(region ? 0 : size_t(batch) * px);
  std::vector<uint8_t> h_body(any_associated ? size_t(batch) * px : 0);
  std::vector<uint8_t> h_ids[N_RENDERERS];  // silhouette images of the renderers in use (only with associated bodies)
  if (any_associated)
    for (int r = 0; r < N_RENDERERS; ++r)
      if (used[r]) h_ids[r].resize(size_t(batch) * px);
  std::vector<P4> trans(batch), geometry2camera(batch);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float main_z_min, main_z_max;
  clip_range(renderers[R_MAIN], &main_z_min, &main_z_max);
  for (int first = 0; first < n_views; first += batch) {
    const int n = std::min(batch, n_views - first);
    for (int k = 0; k < n; ++k) geometry2camera[k] = MulAffine(InverseAffine(poses[first + k]), g2b);  // body at the identity pose
    for (int r = 0; r < N_RENDERERS; ++r) {
      if (!used[r]) continue;
      if (r == R_BACKGROUND && used[R_SAME_REGION]) continue;  // same bodies as the same-region renderer: ids only
      if (!any_associated && r != R_MAIN) continue;
      float z_min, z_max;
      clip_range(renderers[r], &z_min, &z_max);
      const P4 P = projection(z_min, z_max);
      HIPCHK(hipMemsetAsync(d_z.p, 0xff, size_t(n) * px * 8, ctx->stream));
      for (size_t order = 0; order < renderers[r].draws.size(); ++order) {
        const BodyGeometryH& bg = *ctx->body_geometries[renderers[r].draws[order].body];
        P4 bg2b;
        std::memcpy(bg2b.m, bg.geometry2body, 64);
        for (int k = 0; k < n; ++k) trans[k] = MulGeneral(P, MulAffine(InverseAffine(poses[first + k]), bg2b));
        HIPCHK(hipMemcpyAsync(d_trans.p, trans.data(), size_t(n) * 64, hipMemcpyHostToDevice, ctx->stream));
        ModelRenderDev job{};
        job.vertices = bg.vertices.as<float>();
        job.triangles = bg.triangles.as<int>();
        job.n_triangles = bg.n_triangles;
        job.culling = bg.culling;
        job.image_size = S;
        job.order = int(order);
        job.trans = d_trans.as<float>();
        job.z_buffer = d_z.as<unsigned long long>();
        const int slices = std::max(1, std::min(64, (bg.n_triangles + M3T_BLOCK_THREADS - 1) / M3T_BLOCK_THREADS));
        hipLaunchKernelGGL(model_render_kernel, dim3(slices, n), dim3(M3T_BLOCK_THREADS), 0, ctx->stream, job);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));  // `trans` is reused by the next body
      }
      const bool is_main = r == R_MAIN;
      hipLaunchKernelGGL(model_unpack_kernel, dim3(1024), dim3(M3T_BLOCK_THREADS), 0, ctx->stream,
                         d_z.as<unsigned long long>(), size_t(n) * px, is_main ? d_depth.as<uint16_t>() : nullptr,
                         (is_main && !region) ? d_tri.as<int>() : static_cast<int*>(nullptr),
                         any_associated ? d_body.as<uint8_t>() : static_cast<uint8_t*>(nullptr));
      HIPCHK(hipGetLastError());
      if (is_main) {
        HIPCHK(hipMemcpyAsync(h_depth.data(), d_depth.p, size_t(n) * px * 2, hipMemcpyDeviceToHost, ctx->stream));
        if (!region) HIPCHK(hipMemcpyAsync(h_tri.data(), d_tri.p, size_t(n) * px * 4, hipMemcpyDeviceToHost, ctx->stream));
      }
      if (any_associated) HIPCHK(hipMemcpyAsync(h_body.data(), d_body.p, size_t(n) * px, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      if (any_associated) {  // draw order -> id, for this renderer and the one that shares its bodies
        auto to_ids = [&](int which) {
          uint8_t lut[256];
          for (int i = 0; i < 256; ++i) lut[i] = 0;
          for (size_t o = 0; o < renderers[which].draws.size(); ++o) lut[o] = renderers[which].draws[o].id;
          for (size_t i = 0; i < size_t(n) * px; ++i) h_ids[which][i] = lut[h_body[i]];
        };
        to_ids(r);
        if (r == R_SAME_REGION && used[R_BACKGROUND]) to_ids(R_BACKGROUND);
      }
    }
    std::vector<std::thread> workers;
    for (int k = 0; k < n; ++k)
      workers.emplace_back([&, k]() {
        View v;
        v.S = S;
        v.fu = fu;
        v.pp = pp;
        v.term_a = main_z_max * main_z_min * 65535.0f / (main_z_max - main_z_min);  // renderer.cpp:475-478
        v.term_b = main_z_max * 65535.0f / (main_z_max - main_z_min);
        v.depth = h_depth.data() + size_t(k) * px;
        v.triangle = region ? nullptr : h_tri.data() + size_t(k) * px;
        if (any_associated) {
          auto image = [&](int which) { return used[which] ? h_ids[which].data() + size_t(k) * px : nullptr; };
          if (region) v.main_id = image(R_MAIN);
          v.occlusion = image(R_OCCLUSION);
          v.same_region = image(R_SAME_REGION);
          v.foreground = image(R_FOREGROUND);
          v.background = image(R_BACKGROUND);
        }
        const int view = first + k;
        const P4& c2b = poses[view];
        float* out = points.data() + size_t(view) * p->n_points * pf;
        if (region)
          RegionViewData(v, c2b, radius, p->n_points, p->max_radius_depth_offset, p->stride_depth_offset, out,
                         &extents[view]);
        else
          DepthViewData(v, c2b, geometry2camera[k], g.h_vertices, g.h_triangles, radius, p->n_points,
                        p->max_radius_depth_offset, p->stride_depth_offset, out, &extents[view]);
        for (int c = 0; c < 3; ++c) orientations[size_t(view) * 3 + c] = c2b(c, 2);
      });
    for (auto& w : workers) w.join();
  }
  return CreateModel(ctx, region, n_views, p->n_points, points.data(), orientations.data(), extents.data(),
                     p->stride_depth_offset, p->max_radius_depth_offset);
}
int m3t_hip_region_model_generate(m3t_hip_context* ctx, int body, const m3t_model_generation_params* p) {
  return GenerateModel(ctx, true, body, p);
}
int m3t_hip_depth_model_generate(m3t_hip_context* ctx, int body, const m3t_model_generation_params* p) {
  return GenerateModel(ctx, false, body, p);
}
int m3t_hip_region_model_generate_associated(m3t_hip_context* ctx, int body, const m3t_model_generation_params* p, int n,
                                             const int* body_ids, const int* movable, const int* same_region) {
  CHECK_CTX();
  REQUIRE(n >= 0 && (n == 0 || (body_ids && movable && same_region)), M3T_ERR_INVALID_ARGUMENT, "bad associated bodies");
  std::vector<int> groups[4];
  for (int i = 0; i < n; ++i) groups[(movable[i] ? 1 : 0) + (same_region[i] ? 2 : 0)].push_back(body_ids[i]);
  return GenerateModel(ctx, true, body, p, groups);
}
int m3t_hip_depth_model_generate_occluded(m3t_hip_context* ctx, int body, const m3t_model_generation_params* p, int n,
                                          const int* body_ids) {
  CHECK_CTX();
  REQUIRE(n >= 0 && (n == 0 || body_ids), M3T_ERR_INVALID_ARGUMENT, "bad occlusion bodies");
  std::vector<int> groups[4];
  groups[0].assign(body_ids, body_ids + n);
  return GenerateModel(ctx, false, body, p, groups);
}
static int GetViews(m3t_hip_context* ctx, bool region, int id, float* points, float* orientations, float* extents) {
  CHECK_CTX();
  auto& models = region ? ctx->region_models : ctx->depth_models;
  REQUIRE(id >= 0 && id < int(models.size()), M3T_ERR_INVALID_ARGUMENT, "bad model id");
  HIPCHK(hipSetDevice(ctx->device));
  const Model& m = *models[id];
  if (points) HIPCHK(hipMemcpy(points, m.points.p, size_t(m.n_views) * m.n_points * m.point_floats * 4, hipMemcpyDeviceToHost));
  if (orientations) HIPCHK(hipMemcpy(orientations, m.orientations.p, size_t(m.n_views) * 12, hipMemcpyDeviceToHost));
  if (extents) HIPCHK(hipMemcpy(extents, m.extents.p, size_t(m.n_views) * 4, hipMemcpyDeviceToHost));
  return M3T_OK;
}
int m3t_hip_region_model_get_views(m3t_hip_context* ctx, int id, float* points, float* orientations, float* extents) {
  return GetViews(ctx, true, id, points, orientations, extents);
}
int m3t_hip_depth_model_get_views(m3t_hip_context* ctx, int id, float* points, float* orientations, float* extents) {
  return GetViews(ctx, false, id, points, orientations, extents);
}

int m3t_hip_link_create(m3t_hip_context* ctx, int body, int parent, const float body2joint[16],
                        const float joint2parent[16], const int free_directions[6], int fixed_body2joint_pose) {
  CHECK_CTX();
  REQUIRE(body >= -1 && body < int(ctx->body_poses.size() / 16), M3T_ERR_INVALID_ARGUMENT, "bad body id");
  REQUIRE(parent >= -1 && parent < int(ctx->links.size()), M3T_ERR_INVALID_ARGUMENT, "bad parent link id");
  HIPCHK(hipSetDevice(ctx->device));
  int r = PullLinks(ctx);
  if (r) return r;
  Link l;
  l.body = body;
  l.parent = parent;
  std::memcpy(l.body2joint, body2joint ? body2joint : kIdentity, 64);
  std::memcpy(l.joint2parent, joint2parent ? joint2parent : kIdentity, 64);
  if (body >= 0) {
    r = SyncPosesToHost(ctx);
    if (r) return r;
    std::memcpy(l.link2world, &ctx->body_poses[size_t(body) * 16], 64);
  } else {
    std::memcpy(l.link2world, kIdentity, 64);
  }
  bool all_free = true;
  if (free_directions)
    for (int i = 0; i < 6; ++i) {
      l.free_directions[i] = free_directions[i] != 0;
      all_free &= free_directions[i] != 0;
    }
  l.fixed_body2joint_pose = fixed_body2joint_pose != 0;
  l.simple = body >= 0 && parent < 0 && IsIdentity(body2joint) && IsIdentity(joint2parent) && all_free;
  ctx->links.push_back(l);
  int id = int(ctx->links.size()) - 1;
  if (parent >= 0) ctx->links[parent].children.push_back(id);
  ctx->tables_dirty = true;
  return id;
}
int m3t_hip_link_add_modality(m3t_hip_context* ctx, int link, int modality) {
  CHECK_CTX();
  REQUIRE(link >= 0 && link < int(ctx->links.size()) && modality >= 0 && modality < int(ctx->modalities.size()),
          M3T_ERR_INVALID_ARGUMENT, "bad ids");
  const ModalityRef& ref = ctx->modalities[modality];
  int mbody = ModalityBody(ctx, ref);
  REQUIRE(mbody == ctx->links[link].body, M3T_ERR_INVALID_ARGUMENT, "modality and link refer to different bodies");
  ctx->links[link].modalities.push_back(modality);
  ctx->tables_dirty = true;
  return M3T_OK;
}
int m3t_hip_optimizer_create(m3t_hip_context* ctx, int root_link, float tr, float tt) {
  CHECK_CTX();
  REQUIRE(root_link >= 0 && root_link < int(ctx->links.size()), M3T_ERR_INVALID_ARGUMENT, "bad root link");
  Optimizer o;
  o.link = root_link;
  o.tr = tr;
  o.tt = tt;
  ctx->optimizers.push_back(o);
  ctx->tables_dirty = true;
  return int(ctx->optimizers.size()) - 1;
}
int m3t_hip_optimizer_create_rigid(m3t_hip_context* ctx, int body, int n, const int* mids, float tr, float tt) {
  CHECK_CTX();
  REQUIRE(body >= 0, M3T_ERR_INVALID_ARGUMENT, "bad body id");
  int link = m3t_hip_link_create(ctx, body, -1, nullptr, nullptr, nullptr, 1);
  if (link < 0) return link;
  for (int i = 0; i < n; ++i) {
    int r = m3t_hip_link_add_modality(ctx, link, mids[i]);
    if (r < 0) return r;
  }
  return m3t_hip_optimizer_create(ctx, link, tr, tt);
}
// m3t::Constraint (constraint.h): hard constraint between two links of one structure
int m3t_hip_constraint_create(m3t_hip_context* ctx, int optimizer, int link1, int link2, const float b1[16],
                              const float b2[16], const int dirs[6]) {
  CHECK_CTX();
  REQUIRE(optimizer >= 0 && optimizer < int(ctx->optimizers.size()) && link1 >= 0 && link2 >= 0 &&
              link1 < int(ctx->links.size()) && link2 < int(ctx->links.size()) && dirs,
          M3T_ERR_INVALID_ARGUMENT, "bad constraint arguments");
  ConstraintH c;
  c.link1 = link1;
  c.link2 = link2;
  std::memcpy(c.body12joint1, b1 ? b1 : kIdentity, 64);
  std::memcpy(c.body22joint2, b2 ? b2 : kIdentity, 64);
  for (int i = 0; i < 6; ++i) c.directions[i] = dirs[i] != 0;
  ctx->constraints.push_back(c);
  ctx->optimizers[optimizer].constraints.push_back(int(ctx->constraints.size()) - 1);
  ctx->tables_dirty = true;
  return int(ctx->constraints.size()) - 1;
}
int m3t_hip_color_histograms_create(m3t_hip_context* ctx, int n_bins, float learning_rate_f, float learning_rate_b) {
  CHECK_CTX();
  int bitshift;
  switch (n_bins) {  // color_histograms.cpp:131-158
    case 2: bitshift = 7; break;
    case 4: bitshift = 6; break;
    case 8: bitshift = 5; break;
    case 16: bitshift = 4; break;
    case 32: bitshift = 3; break;
    case 64: bitshift = 2; break;
    default: return Fail(ctx, M3T_ERR_INVALID_ARGUMENT, "n_bins has to be of value 2, 4, 8, 16, 32, or 64");
  }
  HIPCHK(hipSetDevice(ctx->device));
  auto h = std::make_unique<SharedHistogramsH>();
  h->n_bins = n_bins;
  h->bitshift = bitshift;
  h->learning_rate_f = learning_rate_f;
  h->learning_rate_b = learning_rate_b;
  const size_t bins3 = size_t(n_bins) * n_bins * n_bins;
  HIPCHK(h->hist_f.alloc(bins3 * 4));
  HIPCHK(h->hist_b.alloc(bins3 * 4));
  HIPCHK(h->hist_norm.alloc(bins3 * 8));
  HIPCHK(h->counts.alloc(bins3 * 8));
  HIPCHK(hipMemset(h->counts.p, 0, bins3 * 8));
  std::vector<float> u(bins3, 1.0f / float(bins3)), nrm(bins3 * 2, 0.5f);  // SetUpHistograms color_histograms.cpp:160-172
  HIPCHK(hipMemcpy(h->hist_f.p, u.data(), bins3 * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->hist_b.p, u.data(), bins3 * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->hist_norm.p, nrm.data(), bins3 * 8, hipMemcpyHostToDevice));
  ctx->shared_histograms.push_back(std::move(h));
  ctx->tables_dirty = true;
  return int(ctx->shared_histograms.size()) - 1;
}
int m3t_hip_region_modality_use_shared_color_histograms(m3t_hip_context* ctx, int modality, int histograms) {
  CHECK_CTX();
  RegionMod* m = GetRegion(ctx, modality);
  REQUIRE(m && histograms >= 0 && histograms < int(ctx->shared_histograms.size()), M3T_ERR_INVALID_ARGUMENT,
          "bad modality / histograms id");
  const SharedHistogramsH& h = *ctx->shared_histograms[histograms];
  m->shared_histograms = histograms;
  m->dev.n_bins = h.n_bins;
  m->dev.bitshift = h.bitshift;
  m->dev.learning_rate_f = h.learning_rate_f;
  m->dev.learning_rate_b = h.learning_rate_b;
  m->dev.histogram_f = h.hist_f.as<float>();
  m->dev.histogram_b = h.hist_b.as<float>();
  m->dev.histogram_norm = h.hist_norm.as<float2>();
  m->dev.shared_counts = h.counts.as<unsigned long long>();
  ctx->tables_dirty = true;
  return M3T_OK;
}
int m3t_hip_soft_constraint_create(m3t_hip_context* ctx, int optimizer, int link1, int link2, const float b1[16],
                                   const float b2[16], const int dirs[6], float max_distance_rotation,
                                   float max_distance_translation, float standard_deviation_rotation,
                                   float standard_deviation_translation) {
  CHECK_CTX();
  REQUIRE(optimizer >= 0 && optimizer < int(ctx->optimizers.size()) && link1 >= 0 && link2 >= 0 &&
              link1 < int(ctx->links.size()) && link2 < int(ctx->links.size()) && dirs,
          M3T_ERR_INVALID_ARGUMENT, "bad soft constraint arguments");
  REQUIRE(standard_deviation_rotation > 0.0f && standard_deviation_translation > 0.0f, M3T_ERR_INVALID_ARGUMENT,
          "standard deviations must be positive");
  SoftConstraintH c{};
  c.joint.link1 = link1;
  c.joint.link2 = link2;
  std::memcpy(c.joint.body12joint1, b1 ? b1 : kIdentity, 64);
  std::memcpy(c.joint.body22joint2, b2 ? b2 : kIdentity, 64);
  for (int i = 0; i < 6; ++i) c.joint.directions[i] = dirs[i] != 0;
  c.max_distance_rotation = max_distance_rotation;
  c.max_distance_translation = max_distance_translation;
  c.standard_deviation_rotation = standard_deviation_rotation;
  c.standard_deviation_translation = standard_deviation_translation;
  ctx->soft_constraints.push_back(c);
  ctx->optimizers[optimizer].soft_constraints.push_back(int(ctx->soft_constraints.size()) - 1);
  ctx->tables_dirty = true;
  return int(ctx->soft_constraints.size()) - 1;
}
int m3t_hip_link_get_link2world_pose(m3t_hip_context* ctx, int link, float pose[16]) {
  CHECK_CTX();
  REQUIRE(link >= 0 && link < int(ctx->links.size()) && pose, M3T_ERR_INVALID_ARGUMENT, "bad link id");
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->links[link].body >= 0) return m3t_hip_body_get_body2world_pose(ctx, ctx->links[link].body, pose);
  int r = PullLinks(ctx);
  if (r) return r;
  std::memcpy(pose, ctx->links[link].link2world, 64);
  return M3T_OK;
}
int m3t_hip_link_set_link2world_pose(m3t_hip_context* ctx, int link, const float pose[16]) {
  CHECK_CTX();
  REQUIRE(link >= 0 && link < int(ctx->links.size()) && pose, M3T_ERR_INVALID_ARGUMENT, "bad link id");
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->links[link].body >= 0) return m3t_hip_body_set_body2world_pose(ctx, ctx->links[link].body, pose);
  int r = PullLinks(ctx);
  if (r) return r;
  std::memcpy(ctx->links[link].link2world, pose, 64);
  ctx->tables_dirty = true;
  return M3T_OK;
}
int m3t_hip_link_set_joint_poses(m3t_hip_context* ctx, int link, const float body2joint[16],
                                 const float joint2parent[16]) {
  CHECK_CTX();
  REQUIRE(link >= 0 && link < int(ctx->links.size()), M3T_ERR_INVALID_ARGUMENT, "bad link id");
  HIPCHK(hipSetDevice(ctx->device));
  int r = PullLinks(ctx);
  if (r) return r;
  Link& l = ctx->links[link];
  if (body2joint) std::memcpy(l.body2joint, body2joint, 64);
  if (joint2parent) std::memcpy(l.joint2parent, joint2parent, 64);
  if (!IsIdentity(l.body2joint) || !IsIdentity(l.joint2parent)) l.simple = false;
  ctx->tables_dirty = true;
  return M3T_OK;
}
int m3t_hip_link_get_joint_poses(m3t_hip_context* ctx, int link, float body2joint[16], float joint2parent[16]) {
  CHECK_CTX();
  REQUIRE(link >= 0 && link < int(ctx->links.size()), M3T_ERR_INVALID_ARGUMENT, "bad link id");
  HIPCHK(hipSetDevice(ctx->device));
  int r = PullLinks(ctx);
  if (r) return r;
  if (body2joint) std::memcpy(body2joint, ctx->links[link].body2joint, 64);
  if (joint2parent) std::memcpy(joint2parent, ctx->links[link].joint2parent, 64);
  return M3T_OK;
}

// ---- tracker sub-steps -------------------------------------------------------------------
int m3t_hip_tracker_set_iterations(m3t_hip_context* ctx, int n_corr, int n_update) {
  CHECK_CTX();
  REQUIRE(n_corr >= 0 && n_update >= 0, M3T_ERR_INVALID_ARGUMENT, "bad iteration counts");
  if (ctx->roi_enabled && n_corr != ctx->n_corr_iterations) ctx->tables_dirty = true;  // (the search-pose slots per object)
  ctx->n_corr_iterations = n_corr;
  ctx->n_update_iterations = n_update;
  return M3T_OK;
}
int m3t_hip_set_fused_step(m3t_hip_context* ctx, int mode) {
  CHECK_CTX();
  REQUIRE(mode >= 0 && mode <= 2, M3T_ERR_INVALID_ARGUMENT, "mode must be 0, 1 or 2");
  ctx->fused_mode = mode;
  return M3T_OK;
}

int m3t_hip_set_object_split(m3t_hip_context* ctx, int enable) {
  CHECK_CTX();
  REQUIRE(enable >= 0 && enable <= M3T_SPLIT_MAX_PARTS, M3T_ERR_INVALID_ARGUMENT, "0 (off), 1 (automatic) or the largest number of workgroups per object (2..16)");
  ctx->split_enabled = enable != 0;
  ctx->split_parts_override = enable > 1 ? enable : 0;
  return M3T_OK;
}

int m3t_hip_start_modalities(m3t_hip_context* ctx, int iteration) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  int r = RequireWholeFrames(ctx, "start_modalities");
  if (r) return r;
  for (auto& m : ctx->region_mods) {  // RegionModality::StartModality :378
    if (m->dev.first_iteration != iteration) {
      m->dev.first_iteration = iteration;
      ctx->tables_dirty = true;
    }
  }
  if ((r = Prepare(ctx, true))) return r;
  if (ctx->table_overflow.host) {  // new histograms: the LDS pair table gets its chance again
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *ctx->table_overflow.as<volatile unsigned>() = 0u;
  }
  if ((r = RenderForModalities(ctx, true))) return r;  // start_modality_renderer_ptrs tracker.cpp:430-436
  if ((r = LaunchTextureDetection(ctx))) return r;  // StartModality :319
  if ((r = LaunchTextureKeyframes(ctx, false))) return r;
  return LaunchHistogram(ctx, iteration, true);
}
// RBOTEvaluator::ResetBody (rbot_evaluator.cpp:334-342) for n bodies of the batch: their poses, the start-modality
// renderers their modalities read, StartModality of their texture modalities (built-in detector only) and of their
// region modalities, in the order of m3t_hip_start_modalities -- enqueued behind whatever the stream
// holds, without reading poses back, waiting for the stream or uploading a table again (m3t_hip.h).
int m3t_hip_reset_bodies(m3t_hip_context* ctx, const int* body_ids, const float* body2world_poses, int n, int iteration) {
  CHECK_CTX();
  REQUIRE(n >= 0, M3T_ERR_INVALID_ARGUMENT, "reset_bodies: n must not be negative");
  if (n == 0) return M3T_OK;
  REQUIRE(body_ids, M3T_ERR_INVALID_ARGUMENT, "reset_bodies: null body ids");
  std::vector<char> listed;
  int r = CheckListedIds(ctx, "reset_bodies", body_ids, n, int(ctx->body_poses.size() / 16), "body", &listed);
  if (r) return r;
  for (auto& l : ctx->links)
    REQUIRE(l.body < 0 || !listed[l.body] || (l.parent < 0 && l.children.empty()), M3T_ERR_UNSUPPORTED,
            "reset_bodies: a listed body belongs to a structure of more than one link (set the poses of the "
            "structure and call start_modalities)");
  if ((r = RefuseTextureBodies(ctx, listed, "reset_bodies"))) return r;
  const BodiesRead reads = CollectReads(ctx, listed);
  REQUIRE(reads.shared_ids.empty(), M3T_ERR_UNSUPPORTED,
          "reset_bodies: a region modality of a listed body uses shared ColorHistograms (call start_modalities)");
  if ((r = RefuseRoiFrames(ctx, reads.cameras, "reset_bodies")) || (r = BeginEnqueued(ctx, true))) return r;
  const int n_region = int(reads.region_ids.size());
  // (a call that lists no texture modality fills the block of ResetBodiesArgs, byte for byte as before)
  const std::vector<int> texture_items = TextureItems(ctx, reads.texture_ids, nullptr);
  const m3t_args::ResetBodiesTextureArgs texture_args(size_t(n), reads.region_ids.size(), reads.renderer_ids.size(),
                                                      body2world_poses != nullptr, reads.texture_ids.size());
  const m3t_args::ResetBodiesArgs args(size_t(n), reads.region_ids.size(), reads.renderer_ids.size(), body2world_poses != nullptr);
  void *host = nullptr, *dev = nullptr;
  int slot = 0;
  HIPCHK(ctx->reset_args.Acquire(texture_items.empty() ? args.bytes : texture_args.bytes, &host, &dev, &slot));
  m3t_args::PutInts(host, texture_args.texture_items, texture_items.data());
  m3t_args::PutInts(host, args.body_ids, body_ids);
  m3t_args::PutInts(host, args.region_ids, reads.region_ids.data());
  m3t_args::PutRenderers(host, args.renderer_ids, args.renderer_pairs, reads.renderer_ids.data());
  m3t_args::PutPoses(host, args.poses, body2world_poses);
  const int* d_region_ids = args.region_ids.in<int>(dev);
  const int items = std::max(body2world_poses ? n * 16 : 0, n_region);
  if (items > 0)
    hipLaunchKernelGGL(reset_bodies_scatter_kernel, dim3((items + 255) / 256), dim3(256), 0, ctx->stream,
                       ctx->d_poses.as<float>(), args.body_ids.in<int>(dev),
                       body2world_poses ? args.poses.in<float>(dev) : (const float*)nullptr, n,
                       ctx->d_region.as<RegionModDev>(), d_region_ids, n_region, iteration);
  // the host mirrors follow (the poses' only where the host copy counts: the device stays authoritative)
  if (body2world_poses) {
    for (int i = 0; i < n; ++i) std::memcpy(&ctx->body_poses[size_t(body_ids[i]) * 16], body2world_poses + size_t(i) * 16, 64);
    ctx->roi_end_valid = false;  // the next step's rectangles start from a snapshot of these poses
  }
  for (int id : reads.region_ids) ctx->region_mods[id]->dev.first_iteration = iteration;
  if ((r = LaunchStartRenderers(ctx, reads.renderer_ids, args.renderer_ids.in<int>(dev), args.renderer_pairs.in<int>(dev))))
    return r;
  if ((r = LaunchTextureRestart(ctx, int(reads.texture_ids.size()), texture_args.texture_items.in<int>(dev), nullptr)))
    return r;
  if (n_region) {
    ScopedKernelTimer timer(ctx, 1);
    hipLaunchKernelGGL(region_histogram_list_kernel, dim3(unsigned(n_region)), dim3(M3T_BLOCK_THREADS), ctx->lds_hist,
                       ctx->stream, ctx->d_region.as<RegionModDev>(), d_region_ids, ctx->cams_active,
                       ctx->d_poses.as<float>(), ctx->hist_counts_in_lds ? 1 : 0);
  }
  return EndEnqueued(ctx, &ctx->reset_args, slot, &reads.cameras);
}
// RTBEvaluator::SetBodyAndJointPoses (rtb_evaluator.cpp:809-858) + Tracker::StartModalities (tracker.cpp:430-445) for n
// kinematic structures of the batch and for no other: the bodies' poses, the joints that follow from them, the
// start-modality renderers, StartModality of the structures' region modalities, shared ColorHistograms included --
// enqueued like reset_bodies (m3t_hip.h; kernels in m3t_structures.hip).
int m3t_hip_reset_structures(m3t_hip_context* ctx, const int* optimizer_ids, int n, const float* body2world_poses, int mode,
                             int iteration) {
  CHECK_CTX();
  REQUIRE(n >= 0, M3T_ERR_INVALID_ARGUMENT, "reset_structures: n must not be negative");
  if (n == 0) return M3T_OK;
  REQUIRE(optimizer_ids && body2world_poses, M3T_ERR_INVALID_ARGUMENT, "reset_structures: null optimizer ids or poses");
  REQUIRE(mode == 0 || mode == 1, M3T_ERR_INVALID_ARGUMENT, "reset_structures: mode must be 0 (independent / projected) or 1 (constrained)");
  std::vector<char> opt_listed, listed(ctx->body_poses.size() / 16, 0);
  int r = CheckListedIds(ctx, "reset_structures", optimizer_ids, n, int(ctx->optimizers.size()), "optimizer", &opt_listed);
  if (r) return r;
  REQUIRE(!ctx->Distributed(), M3T_ERR_UNSUPPORTED,
          "reset_structures: the context's structures are spread over ranks (a communicator or a reduce callback is set)");
  // the structures' links in table order (depth first, parents before children) and what each of them takes
  std::vector<StructureResetDev> structures;
  std::vector<StructureLinkResetDev> entries;
  std::vector<int> pose_body;  // body of pose k of the call
  std::vector<int> local(ctx->links.size(), -1);
  for (int i = 0; i < n; ++i) {
    const Optimizer& o = ctx->optimizers[size_t(optimizer_ids[i])];
    std::vector<int> order;
    DfsOrder(ctx, o.link, &order);
    const Link& root = ctx->links[size_t(o.link)];
    REQUIRE(mode == 0 || (root.body < 0 && !root.children.empty()), M3T_ERR_INVALID_ARGUMENT,
            "reset_structures: mode 1 (constrained) needs a root link without a body that has children");
    structures.push_back(StructureResetDev{optimizer_ids[i], int(entries.size()), int(order.size())});
    std::vector<int> pose_of(order.size(), -1);
    for (size_t k = 0; k < order.size(); ++k) {
      const Link& l = ctx->links[size_t(order[k])];
      local[size_t(order[k])] = int(k);
      StructureLinkResetDev e{l.body, -1, -1};
      if (mode == 1 && k == 0) {  // :846-858: the root's link2world and joint poses stay
        entries.push_back(e);
        continue;
      }
      REQUIRE(l.body >= 0, M3T_ERR_UNSUPPORTED,
              "reset_structures: a link without a body (the reference dereferences its body_ptr)");
      REQUIRE(!listed[size_t(l.body)], M3T_ERR_INVALID_ARGUMENT, "reset_structures: a body belongs to two listed links");
      REQUIRE(order.size() == 1 || !l.modalities.empty(), M3T_ERR_UNSUPPORTED,
              "reset_structures: a body of the structure has no modality in this context (the structure's ownership "
              "is partial: its other modalities live on another rank)");
      listed[size_t(l.body)] = 1;
      e.pose = pose_of[k] = int(pose_body.size());
      pose_body.push_back(l.body);
      if (k > 0) {
        const int parent = local[size_t(l.parent)];
        e.joint = (mode == 1 && parent == 0) ? -2 : pose_of[size_t(parent)];
      }
      entries.push_back(e);
    }
  }
  if ((r = RefuseTextureBodies(ctx, listed, "reset_structures", true))) return r;
  const BodiesRead reads = CollectReads(ctx, listed);
  for (auto& m : ctx->region_mods)
    REQUIRE(m->shared_histograms < 0 || listed[size_t(m->body)] ||
                std::find(reads.shared_ids.begin(), reads.shared_ids.end(), m->shared_histograms) == reads.shared_ids.end(),
            M3T_ERR_UNSUPPORTED,
            "reset_structures: shared ColorHistograms of a listed structure are also used by a modality of a structure "
            "that is not listed (the reference defines no result for that)");
  if ((r = RefuseRoiFrames(ctx, reads.cameras, "reset_structures")) || (r = BeginEnqueued(ctx, true))) return r;
  if (!ctx->tree_mode)
    for (auto& s : structures) s.opt = -1;  // free rigid bodies only: there is no link table, the poses are all
  static_assert(sizeof(StructureResetDev) == 12 && sizeof(StructureLinkResetDev) == 12, "lists of ints");
  const int n_region = int(reads.region_ids.size());
  const m3t_args::ResetStructuresArgs args(structures.size(), entries.size(), reads.region_ids.size(),
                                           reads.renderer_ids.size(), pose_body.size());
  void *host = nullptr, *dev = nullptr;
  int slot = 0;
  HIPCHK(ctx->reset_args.Acquire(args.bytes, &host, &dev, &slot));
  m3t_args::PutInts(host, args.structures, structures.data());
  m3t_args::PutInts(host, args.links, entries.data());
  m3t_args::PutInts(host, args.region_ids, reads.region_ids.data());
  m3t_args::PutRenderers(host, args.renderer_ids, args.renderer_pairs, reads.renderer_ids.data());
  m3t_args::PutPoses(host, args.poses, body2world_poses);
  const int* d_region_ids = args.region_ids.in<int>(dev);
  hipLaunchKernelGGL(reset_structures_kernel, dim3(unsigned(structures.size())), dim3(64), 0, ctx->stream,
                     ctx->tree_mode ? ctx->d_treeopts.as<TreeOptDev>() : (const TreeOptDev*)nullptr, ctx->d_poses.as<float>(),
                     args.structures.in<const StructureResetDev>(dev), args.links.in<const StructureLinkResetDev>(dev),
                     args.poses.in<const float>(dev), ctx->d_region.as<RegionModDev>(), d_region_ids, n_region, iteration);
  // the host mirrors follow: the bodies' poses; the joints stay the device's (PullLinks fetches them when asked)
  for (size_t k = 0; k < pose_body.size(); ++k)
    std::memcpy(&ctx->body_poses[size_t(pose_body[k]) * 16], body2world_poses + k * 16, 64);
  if (ctx->tree_mode) ctx->links_device_newer = true;
  ctx->roi_end_valid = false;  // the next step's rectangles start from a snapshot of these poses
  for (int id : reads.region_ids) ctx->region_mods[size_t(id)]->dev.first_iteration = iteration;
  if ((r = LaunchStartRenderers(ctx, reads.renderer_ids, args.renderer_ids.in<int>(dev), args.renderer_pairs.in<int>(dev))))
    return r;
  if (n_region) {
    ScopedKernelTimer timer(ctx, 1);
    hipLaunchKernelGGL(structures_histogram_list_kernel, dim3(unsigned(n_region)), dim3(M3T_BLOCK_THREADS), ctx->lds_hist,
                       ctx->stream, ctx->d_region.as<RegionModDev>(), d_region_ids, ctx->cams_active,
                       ctx->d_poses.as<float>(), ctx->hist_counts_in_lds ? 1 : 0);
    for (int id : reads.shared_ids)  // InitializeHistograms of the shared objects these modalities added their samples to (tracker.cpp:441-443)
      hipLaunchKernelGGL(shared_histogram_finish_kernel, dim3(1), dim3(M3T_BLOCK_THREADS), 0, ctx->stream,
                         ctx->d_shared_histograms.as<SharedHistogramsDev>() + id, 1);
  }
  return EndEnqueued(ctx, &ctx->reset_args, slot, &reads.cameras);
}
// ---- the evaluators' judgement on the device (m3t_judge.hip) ---------------------------------------------------------
}  // extern "C"
namespace {
// The launch shape of a judge: which workgroup searches which query range of which body.  Follows the batch: one query
// per thread while that leaves no more than a few workgroups per CU, four per thread beyond.  (Create / set_vertices
// only: waits for the stream, since earlier calls may still read the tables.)
int BuildJudgeTables(Ctx* ctx, Judge* j) {
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int n = int(j->body_ids.size());
  long chunks = 0;
  for (int i = 0; i < n; ++i)
    if (!j->add_only[size_t(i)])
      chunks += std::max(1, (j->n_vertices[size_t(i)] + M3T_JUDGE_SPLIT_QUERIES - 1) / M3T_JUDGE_SPLIT_QUERIES);
  j->queries_per_thread = chunks > 4L * std::max(1, ctx->prop.multiProcessorCount) ? 4 : 1;
  const int q = j->queries_per_thread * M3T_JUDGE_THREADS;
  std::vector<JudgeBodyDev> bodies(static_cast<size_t>(n));
  std::vector<JudgePartDev> parts;
  std::vector<JudgeAddBodyDev> add_bodies;
  std::vector<JudgePartDev> add_parts;
  j->any_split = j->any_add_split = false;
  for (int i = 0; i < n; ++i) {
    JudgeBodyDev& b = bodies[size_t(i)];
    b.vertices = j->vertices[size_t(i)] ? j->vertices[size_t(i)]->as<float4>() : nullptr;
    b.body = j->body_ids[size_t(i)];
    b.target = j->targets[size_t(i)] >= 0 ? j->targets[size_t(i)] : b.body;
    b.n_vertices = j->n_vertices[size_t(i)];
    b.first_part = int(parts.size());
    if (j->add_only[size_t(i)]) {  // no workgroup of judge_bodies_kernel, nothing for judge_finish_kernel
      b.n_parts = 1;
      JudgeAddBodyDev a;
      a.vertices = b.vertices;
      a.index = i;
      a.body = b.body;
      a.target = b.target;
      a.n_vertices = b.n_vertices;
      a.first_part = int(add_parts.size());
      a.n_parts = std::max(1, (a.n_vertices + M3T_JUDGE_ADD_SPLIT - 1) / M3T_JUDGE_ADD_SPLIT);
      std::memcpy(a.geometry2body, j->geometry2body[size_t(i)].data(), sizeof(a.geometry2body));
      j->any_add_split = j->any_add_split || a.n_parts > 1;
      for (int p = 0; p < a.n_parts; ++p) add_parts.push_back(JudgePartDev{int(add_bodies.size()), p});
      add_bodies.push_back(a);
      continue;
    }
    b.n_parts = std::max(1, (b.n_vertices + q - 1) / q);
    j->any_split = j->any_split || b.n_parts > 1;
    for (int p = 0; p < b.n_parts; ++p) parts.push_back(JudgePartDev{i, p});
  }
  j->n_parts = int(parts.size());
  j->n_add_bodies = int(add_bodies.size());
  j->n_add_parts = int(add_parts.size());
  HIPCHK(UploadTable(&j->d_bodies, bodies));
  HIPCHK(UploadTable(&j->d_parts, parts));
  HIPCHK(j->d_partial.alloc(std::max<size_t>(1, parts.size()) * 2 * sizeof(double)));
  HIPCHK(j->d_flags.alloc(size_t(n) * sizeof(int)));
  if (!add_bodies.empty()) {
    HIPCHK(UploadTable(&j->d_add_bodies, add_bodies));
    HIPCHK(UploadTable(&j->d_add_parts, add_parts));
    HIPCHK(j->d_add_partial.alloc(add_parts.size() * sizeof(double)));
  }
  HIPCHK(hipMemset(j->d_flags.p, 0, size_t(n) * sizeof(int)));
  return M3T_OK;
}
}  // namespace
extern "C" {

int m3t_hip_judge_create(m3t_hip_context* ctx, const int* body_ids, int n_bodies, int n_rows_max, int* judge) {
  CHECK_CTX();
  REQUIRE(body_ids && judge && n_bodies >= 1 && n_rows_max >= 1, M3T_ERR_INVALID_ARGUMENT,
          "judge_create: needs body ids, at least one body and one row");
  REQUIRE(size_t(n_bodies) * size_t(n_rows_max) <= (size_t(1) << 23), M3T_ERR_INVALID_ARGUMENT,
          "judge_create: more than 2^23 results (n_bodies x n_rows_max)");
  std::vector<char> listed;
  int r = CheckListedIds(ctx, "judge_create", body_ids, n_bodies, int(ctx->body_poses.size() / 16), "body", &listed);
  if (r) return r;
  HIPCHK(hipSetDevice(ctx->device));
  auto j = std::make_unique<Judge>();
  j->body_ids.assign(body_ids, body_ids + n_bodies);
  j->n_rows_max = n_rows_max;
  j->n_vertices.assign(size_t(n_bodies), 0);
  j->vertices.resize(size_t(n_bodies));
  j->add_only.assign(size_t(n_bodies), 0);
  j->targets.assign(size_t(n_bodies), -1);
  j->geometry2body.resize(size_t(n_bodies));
  j->row_done.resize(size_t(n_rows_max));
  HIPCHK(j->rows.Alloc(size_t(n_bodies) * size_t(n_rows_max) * sizeof(m3t_body_judgement), kMapped, true));
  if ((r = BuildJudgeTables(ctx, j.get()))) return r;
  ctx->judges.push_back(std::move(j));
  *judge = int(ctx->judges.size()) - 1;
  return M3T_OK;
}
int m3t_hip_judge_set_thresholds(m3t_hip_context* ctx, int judge, float translation_error_threshold,
                                 float rotation_error_threshold) {
  CHECK_CTX();
  Judge* j = GetJudge(ctx, judge, "judge_set_thresholds");
  if (!j) return M3T_ERR_INVALID_ARGUMENT;
  j->thr_t = translation_error_threshold;
  j->thr_r = rotation_error_threshold;
  return M3T_OK;
}
int m3t_hip_judge_set_vertices(m3t_hip_context* ctx, int judge, int index, const float* xyz, int n_vertices) {
  CHECK_CTX();
  Judge* j = GetJudge(ctx, judge, "judge_set_vertices");
  if (!j) return M3T_ERR_INVALID_ARGUMENT;
  REQUIRE(index >= 0 && index < int(j->body_ids.size()), M3T_ERR_INVALID_ARGUMENT, "judge_set_vertices: bad body index");
  REQUIRE(xyz && n_vertices >= 1 && n_vertices <= (1 << 18), M3T_ERR_INVALID_ARGUMENT,
          "judge_set_vertices: 1 to 2^18 vertices");
  HIPCHK(hipSetDevice(ctx->device));
  const std::vector<float> padded = PadVertices(xyz, n_vertices, 4);
  HIPCHK(hipStreamSynchronize(ctx->stream));  // earlier calls may still search the old vertices
  auto mem = std::make_unique<DevMem>();
  HIPCHK(UploadTable(mem.get(), padded));
  j->vertices[size_t(index)] = std::move(mem);
  j->n_vertices[size_t(index)] = n_vertices;
  return BuildJudgeTables(ctx, j);
}
// CalculatePoseResults of the listed bodies against these ground-truth poses into the next row and, with
// reset_iteration >= 0, ResetBody of those the device finds lost -- enqueued behind whatever the stream holds (m3t_hip.h).
int m3t_hip_judge_bodies(m3t_hip_context* ctx, int judge, const float* gt_body2world_poses, int reset_iteration, int* row) {
  CHECK_CTX();
  Judge* j = GetJudge(ctx, judge, "judge_bodies");
  if (!j) return M3T_ERR_INVALID_ARGUMENT;
  REQUIRE(gt_body2world_poses, M3T_ERR_INVALID_ARGUMENT, "judge_bodies: null ground-truth poses");
  REQUIRE(j->n_rows < j->n_rows_max, M3T_ERR_INVALID_ARGUMENT,
          "judge_bodies: the row table is full (judge_read, then judge_clear)");
  const int n = int(j->body_ids.size());
  const bool reset = reset_iteration >= 0;
  int r = M3T_OK;
  BodiesRead reads;
  std::vector<int> region_ids, region_body_index, region_first(size_t(n) + 1, 0);  // the modalities grouped by listed body
  std::vector<int> render_pairs, reader_first, readers;  // judge_set_reset_renderers: what the device may render, and for whom
  std::vector<int> texture_items;  // the texture modalities of the bodies a reset writes, flagged by their judge entry
  RenderLaunchShape render_shape{};
  if (ctx->judge_render_always < 0)  // once per context, like the other developer knobs
    ctx->judge_render_always = std::getenv("M3T_HIP_JUDGE_RENDER_ALWAYS") ? 1 : 0;
  const bool render_always = ctx->judge_render_always == 1;  // every pair is rendered, lost reader or not
  if (reset) {  // the host cannot follow a reset the device decides: only what needs no host mirror
    // (the bodies a reset writes -- the reset targets, by default the listed bodies themselves -- are "listed" below)
    std::vector<int> index_of(ctx->body_poses.size() / 16, -1);
    std::vector<char> listed(index_of.size(), 0);  // (the same as a mask: what CollectReads takes)
    for (int i = 0; i < n; ++i) {
      const int written = j->targets[size_t(i)] >= 0 ? j->targets[size_t(i)] : j->body_ids[size_t(i)];
      index_of[size_t(written)] = i;
      listed[size_t(written)] = 1;
    }
    for (auto& l : ctx->links)
      REQUIRE(l.body < 0 || !listed[size_t(l.body)] || (l.parent < 0 && l.children.empty()), M3T_ERR_UNSUPPORTED,
              "judge_bodies: a listed body belongs to a structure of more than one link (judge with "
              "reset_iteration < 0 and reset the structure from the host)");
    if ((r = RefuseTextureBodies(ctx, listed, "judge_bodies"))) return r;
    reads = CollectReads(ctx, listed);
    std::vector<std::vector<int>> of_body(static_cast<size_t>(n));
    for (int id : reads.region_ids) {
      const RegionMod& m = *ctx->region_mods[size_t(id)];
      REQUIRE(m.shared_histograms < 0, M3T_ERR_UNSUPPORTED,
              "judge_bodies: a region modality of a listed body uses shared ColorHistograms (call start_modalities)");
      REQUIRE(m.dev.first_iteration == reset_iteration, M3T_ERR_INVALID_ARGUMENT,
              "judge_bodies: first_iteration of a listed body's region modality differs from reset_iteration (the "
              "host could not follow a change the device decides; start_modalities(reset_iteration) first)");
      REQUIRE(j->reset_renderers ||
                  (!(m.dev.model_occlusions && m.depth_renderer >= 0) && !(m.dev.use_region_checking && m.silhouette_renderer >= 0)),
              M3T_ERR_UNSUPPORTED,
              "judge_bodies: a region modality of a listed body reads a start-modality renderer (judge with "
              "reset_iteration < 0 and call reset_bodies)");
      of_body[size_t(index_of[size_t(m.body)])].push_back(id);
    }
    // (a texture modality's silhouette renderer is a start-modality renderer, :516-524)
    REQUIRE(j->reset_renderers || reads.texture_ids.empty(), M3T_ERR_UNSUPPORTED,
            "judge_bodies: a texture modality of a listed body reads a start-modality renderer (judge_set_reset_renderers "
            "first, or judge with reset_iteration < 0 and call reset_bodies)");
    if ((r = RefuseRoiFrames(ctx, reads.cameras, "judge_bodies"))) return r;
    texture_items = TextureItems(ctx, reads.texture_ids, &index_of);
    for (int i = 0; i < n; ++i) {
      for (int id : of_body[size_t(i)]) {
        region_ids.push_back(id);
        region_body_index.push_back(i);
      }
      region_first[size_t(i) + 1] = int(region_ids.size());
    }
    if (j->reset_renderers && !reads.renderer_ids.empty()) {
      // the renderers as reset_bodies would list them for ALL the targets, paired with their twins; per pair the
      // entries of the judge whose target reads one of the two
      HIPCHK(hipSetDevice(ctx->device));
      render_pairs = RendererPairs(ctx, reads.renderer_ids);
      const int n_pairs = int(render_pairs.size() / 2);
      int largest = 0;
      for (int id : reads.renderer_ids) largest = std::max(largest, ctx->renderers[size_t(id)]->image_size);
      render_shape = RenderShape(n_pairs, largest);
      REQUIRE(LdsRasterFits(ctx, render_shape, largest), M3T_ERR_UNSUPPORTED,
              "judge_bodies: a start-modality renderer of image size " + std::to_string(largest) +
                  " needs the three-launch form (its z-buffer band does not fit the LDS, or the LDS form is switched "
                  "off): a device-decided run covers the two-launch form only (judge with reset_iteration < 0 and call "
                  "reset_bodies)");
      reader_first.push_back(0);
      for (int p = 0; p < n_pairs; ++p) {
        std::vector<char> reads_pair(static_cast<size_t>(n), 0);
        for (int id : reads.region_ids) {
          const RegionMod& m = *ctx->region_mods[size_t(id)];
          for (int renderer : {m.dev.model_occlusions ? m.depth_renderer : -1, m.dev.use_region_checking ? m.silhouette_renderer : -1})
            if (renderer >= 0 && (renderer == render_pairs[size_t(2 * p)] || renderer == render_pairs[size_t(2 * p + 1)]))
              reads_pair[size_t(index_of[size_t(m.body)])] = 1;
        }
        for (int id : reads.texture_ids) {
          const TextureMod& m = *ctx->texture_mods[size_t(id)];
          for (int renderer : {m.silhouette_renderer, m.dev.model_occlusions ? m.depth_renderer : -1})
            if (renderer >= 0 && (renderer == render_pairs[size_t(2 * p)] || renderer == render_pairs[size_t(2 * p + 1)]))
              reads_pair[size_t(index_of[size_t(m.body)])] = 1;
        }
        for (int i = 0; i < n; ++i)
          if (reads_pair[size_t(i)]) readers.push_back(i);
        reader_first.push_back(int(readers.size()));
      }
    }
  }
  if ((r = BeginEnqueued(ctx, reset))) return r;
  const size_t n_region = region_ids.size();
  const size_t n_pairs = render_pairs.size() / 2;
  // (a judge without judge_set_reset_renderers fills the block of JudgeBodiesArgs, a call that restarts no texture
  // modality that of JudgeBodiesRenderArgs, byte for byte as before)
  const size_t n_texture = texture_items.size() / 3;
  const m3t_args::JudgeBodiesTextureArgs texture_args(size_t(n), n_region, n_pairs, readers.size(), n_texture);
  const m3t_args::JudgeBodiesRenderArgs render_args(size_t(n), n_region, n_pairs, readers.size());
  const m3t_args::JudgeBodiesArgs plain_args(size_t(n), n_region);
  const m3t_args::JudgeBodiesArgs& args = plain_args;
  void *host = nullptr, *dev = nullptr;
  int slot = 0;
  HIPCHK(j->args.Acquire(n_texture ? texture_args.bytes : n_pairs ? render_args.bytes : plain_args.bytes, &host, &dev, &slot));
  m3t_args::PutPoses(host, args.gt_poses, gt_body2world_poses);
  m3t_args::PutInts(host, args.region_ids, region_ids.data());
  m3t_args::PutInts(host, args.region_body, region_body_index.data());
  m3t_args::PutInts(host, args.region_first, region_first.data());
  if (n_pairs) {  // behind the four lists, which sit where JudgeBodiesArgs puts them
    m3t_args::PutInts(host, render_args.renderer_pairs, render_pairs.data());
    m3t_args::PutInts(host, render_args.reader_first, reader_first.data());
    m3t_args::PutInts(host, render_args.readers, readers.data());
  }
  if (n_texture) m3t_args::PutInts(host, texture_args.texture_items, texture_items.data());  // (n_pairs > 0: behind the seven)
  const float* d_gt = args.gt_poses.in<float>(dev);
  const int *d_region_ids = args.region_ids.in<int>(dev), *d_region_body = args.region_body.in<int>(dev),
            *d_region_first = args.region_first.in<int>(dev);
  const int row_index = j->n_rows;
  m3t_body_judgement* d_row = j->rows.dev_as<m3t_body_judgement>() + size_t(row_index) * size_t(n);
  HIPCHK(j->row_done[size_t(row_index)].Ensure(hipEventDisableTiming));
  if (j->n_add_parts > 0) {  // the ADD-only bodies: workgroups of their own (m3t_opt.hip)
    hipLaunchKernelGGL(judge_add_only_kernel, dim3(unsigned(j->n_add_parts)), dim3(M3T_JUDGE_THREADS), 0, ctx->stream,
                       ctx->d_poses.as<float>(), j->d_add_bodies.as<JudgeAddBodyDev>(), j->d_add_parts.as<JudgePartDev>(),
                       d_gt, j->thr_t, j->thr_r, reset_iteration, ctx->d_region.as<RegionModDev>(), d_region_ids,
                       d_region_first, j->d_flags.as<int>(), d_row, j->d_add_partial.as<double>());
    if (j->any_add_split)
      hipLaunchKernelGGL(judge_add_only_finish_kernel, dim3(unsigned(j->n_add_bodies)), dim3(64), 0, ctx->stream,
                         ctx->d_poses.as<float>(), j->d_add_bodies.as<JudgeAddBodyDev>(), d_gt, reset_iteration,
                         ctx->d_region.as<RegionModDev>(), d_region_ids, d_region_first, j->d_flags.as<int>(), d_row,
                         j->d_add_partial.as<double>());
  }
  if (j->n_parts > 0)
  hipLaunchKernelGGL(j->queries_per_thread == 4 ? judge_bodies_x4_kernel : judge_bodies_kernel, dim3(unsigned(j->n_parts)),
                     dim3(M3T_JUDGE_THREADS), 0, ctx->stream, ctx->d_poses.as<float>(), j->d_bodies.as<JudgeBodyDev>(),
                     j->d_parts.as<JudgePartDev>(), d_gt, j->thr_t, j->thr_r, reset_iteration,
                     ctx->d_region.as<RegionModDev>(), d_region_ids, d_region_first, j->d_flags.as<int>(), d_row,
                     j->d_partial.as<double>());
  if (j->any_split)
    hipLaunchKernelGGL(judge_finish_kernel, dim3(unsigned(n)), dim3(64), 0, ctx->stream, ctx->d_poses.as<float>(),
                       j->d_bodies.as<JudgeBodyDev>(), d_gt, reset_iteration, ctx->d_region.as<RegionModDev>(),
                       d_region_ids, d_region_first, j->d_flags.as<int>(), d_row, j->d_partial.as<double>());
  if (n_pairs) {  // the start-modality renderers some lost body reads, with the poses after all of the call's resets
    const int* d_pairs = render_args.renderer_pairs.in<int>(dev);
    const int *d_reader_first = render_args.reader_first.in<int>(dev), *d_readers = render_args.readers.in<int>(dev);
    hipLaunchKernelGGL(focused_setup_flagged_kernel, dim3(unsigned(render_shape.slices), unsigned(n_pairs)),
                       dim3(M3T_BLOCK_THREADS), 0, ctx->stream, ctx->d_renderers.as<RendererDev>(), d_pairs,
                       ctx->cams_active, ctx->d_poses.as<float>(), j->d_flags.as<int>(), d_reader_first, d_readers,
                       render_always ? 1 : 0);
    hipLaunchKernelGGL(focused_resolve_flagged_kernel, dim3(unsigned(n_pairs), unsigned(render_shape.bands)),
                       dim3(M3T_BLOCK_THREADS), render_shape.lds, ctx->stream, ctx->d_renderers.as<RendererDev>(), d_pairs,
                       j->d_flags.as<int>(), d_reader_first, d_readers, render_always ? 1 : 0);
  }
  if ((r = LaunchTextureRestart(ctx, int(n_texture), texture_args.texture_items.in<int>(dev), j->d_flags.as<int>()))) return r;
  if (n_region) {
    ScopedKernelTimer timer(ctx, 1);
    hipLaunchKernelGGL(region_histogram_flagged_kernel, dim3(unsigned(n_region)), dim3(M3T_BLOCK_THREADS), ctx->lds_hist,
                       ctx->stream, ctx->d_region.as<RegionModDev>(), d_region_ids, d_region_body, j->d_flags.as<int>(),
                       ctx->cams_active, ctx->d_poses.as<float>(), ctx->hist_counts_in_lds ? 1 : 0);
  }
  if (j->n_structures > 0) {  // RTBEvaluator::CalculatePoseResults' combination of the row, behind the per-body results
    const int* d_structure_ints = j->d_structure_ints.as<int>();
    hipLaunchKernelGGL(judge_structures_kernel, dim3(unsigned(j->n_structures + 63) / 64), dim3(64), 0, ctx->stream, d_row,
                       d_structure_ints, d_structure_ints + j->n_structures + 1,
                       d_structure_ints + j->n_structures + 1 + j->structure_groups + 1,
                       j->d_structure_thresholds.as<float>(), j->n_structures,
                       j->structure_rows.dev_as<m3t_structure_judgement>() + size_t(row_index) * size_t(j->n_structures));
  }
  if ((r = EndEnqueued(ctx, &j->args, slot, reset ? &reads.cameras : nullptr))) return r;
  HIPCHK(hipEventRecord(j->row_done[size_t(row_index)].get(), ctx->stream));
  if (reset) ctx->roi_end_valid = false;  // the host's mirror does not vouch for these bodies' poses any more
  ++j->n_rows;
  if (row) *row = row_index;
  return M3T_OK;
}
// A resetting judge_bodies call of this judge may run the start-modality renderers of the bodies it resets, decided on
// the device (m3t_hip.h).  Off: the call refuses such bodies, as it always did.
int m3t_hip_judge_set_reset_renderers(m3t_hip_context* ctx, int judge, int enable) {
  CHECK_CTX();
  Judge* j = GetJudge(ctx, judge, "judge_set_reset_renderers");
  if (!j) return M3T_ERR_INVALID_ARGUMENT;
  j->reset_renderers = enable != 0;
  return M3T_OK;
}
// Entry `index` of the judge resets body_id instead of its listed body when it is found lost (-1: its listed body again;
// m3t_hip.h).  Waits for the stream and uploads: outside the frame loop, like judge_set_vertices.
int m3t_hip_judge_set_reset_target(m3t_hip_context* ctx, int judge, int index, int body_id) {
  CHECK_CTX();
  Judge* j = GetJudge(ctx, judge, "judge_set_reset_target");
  if (!j) return M3T_ERR_INVALID_ARGUMENT;
  const int n = int(j->body_ids.size());
  REQUIRE(index >= 0 && index < n, M3T_ERR_INVALID_ARGUMENT, "judge_set_reset_target: bad body index");
  REQUIRE(body_id >= -1 && body_id < int(ctx->body_poses.size() / 16), M3T_ERR_INVALID_ARGUMENT,
          "judge_set_reset_target: bad body id");
  REQUIRE(j->n_rows == 0, M3T_ERR_INVALID_ARGUMENT,
          "judge_set_reset_target: rows have been judged already (judge_clear first)");
  const int target = body_id == j->body_ids[size_t(index)] ? -1 : body_id;
  for (int k = 0; k < n && target >= 0; ++k) {
    if (k == index) continue;
    // (a listed body is read by its own entry's workgroups while another entry's reset would write it)
    REQUIRE(j->body_ids[size_t(k)] != target, M3T_ERR_INVALID_ARGUMENT,
            "judge_set_reset_target: the body is the listed body of another entry of the judge (it would be written by "
            "two entries, or written by one while the other reads its pose)");
    REQUIRE(j->targets[size_t(k)] != target, M3T_ERR_INVALID_ARGUMENT,
            "judge_set_reset_target: the body would be written by two entries of the judge");
  }
  HIPCHK(hipSetDevice(ctx->device));
  const int before = j->targets[size_t(index)];
  j->targets[size_t(index)] = target;
  const int r = BuildJudgeTables(ctx, j);
  if (r) j->targets[size_t(index)] = before;  // (a failed upload: the next upload is of the old table again)
  return r;
}
int m3t_hip_judge_read(m3t_hip_context* ctx, int judge, int first_row, int n_rows, m3t_body_judgement* out) {
  CHECK_CTX();
  Judge* j = GetJudge(ctx, judge, "judge_read");
  if (!j) return M3T_ERR_INVALID_ARGUMENT;
  REQUIRE(first_row >= 0 && n_rows >= 0 && first_row <= j->n_rows && n_rows <= j->n_rows - first_row,
          M3T_ERR_INVALID_ARGUMENT, "judge_read: rows that have not been judged");
  if (n_rows == 0) return M3T_OK;
  REQUIRE(out, M3T_ERR_INVALID_ARGUMENT, "judge_read: null output");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipEventSynchronize(j->row_done[size_t(first_row + n_rows - 1)].get()));  // rows complete in order
  const size_t n = j->body_ids.size();
  std::memcpy(out, j->rows.as<m3t_body_judgement>() + size_t(first_row) * n, size_t(n_rows) * n * sizeof(m3t_body_judgement));
  return M3T_OK;
}
// RTBEvaluator's ids_combined_bodies_ of n_structures structures: structure s holds the groups
// [structure_first_group[s], structure_first_group[s + 1]), group g the listed bodies
// listed_body_indices[group_first_index[g] .. group_first_index[g + 1]) (indices into the judge's list of bodies).
// Waits for the stream and uploads: outside the frame loop, like judge_set_vertices.
int m3t_hip_judge_set_structures(m3t_hip_context* ctx, int judge, int n_structures, const int* structure_first_group,
                                 const int* group_first_index, const int* listed_body_indices,
                                 const float* error_thresholds) {
  CHECK_CTX();
  Judge* j = GetJudge(ctx, judge, "judge_set_structures");
  if (!j) return M3T_ERR_INVALID_ARGUMENT;
  REQUIRE(n_structures >= 1 && structure_first_group && group_first_index && listed_body_indices && error_thresholds,
          M3T_ERR_INVALID_ARGUMENT, "judge_set_structures: needs at least one structure and all four lists");
  REQUIRE(size_t(n_structures) * size_t(j->n_rows_max) <= (size_t(1) << 23), M3T_ERR_INVALID_ARGUMENT,
          "judge_set_structures: more than 2^23 results (n_structures x n_rows_max)");
  REQUIRE(j->n_rows == 0, M3T_ERR_INVALID_ARGUMENT, "judge_set_structures: rows have been judged already (judge_clear first)");
  REQUIRE(structure_first_group[0] == 0, M3T_ERR_INVALID_ARGUMENT, "judge_set_structures: the first group is group 0");
  for (int s = 0; s < n_structures; ++s)
    REQUIRE(structure_first_group[s + 1] > structure_first_group[s], M3T_ERR_INVALID_ARGUMENT,
            "judge_set_structures: a structure without a group");
  const int n_groups = structure_first_group[n_structures];
  REQUIRE(group_first_index[0] == 0, M3T_ERR_INVALID_ARGUMENT, "judge_set_structures: the first index is index 0");
  for (int g = 0; g < n_groups; ++g)
    REQUIRE(group_first_index[g + 1] > group_first_index[g], M3T_ERR_INVALID_ARGUMENT,
            "judge_set_structures: a group without a body");
  const int n_listed = group_first_index[n_groups];
  for (int i = 0; i < n_listed; ++i) {
    REQUIRE(listed_body_indices[i] >= 0 && listed_body_indices[i] < int(j->body_ids.size()), M3T_ERR_INVALID_ARGUMENT,
            "judge_set_structures: an index outside the judge's list of bodies");
    REQUIRE(j->n_vertices[size_t(listed_body_indices[i])] > 0, M3T_ERR_INVALID_ARGUMENT,
            "judge_set_structures: a body of a group has no evaluation vertices (judge_set_vertices first)");
  }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));  // earlier calls may still read the old lists
  std::vector<int> ints;
  ints.insert(ints.end(), structure_first_group, structure_first_group + n_structures + 1);
  ints.insert(ints.end(), group_first_index, group_first_index + n_groups + 1);
  ints.insert(ints.end(), listed_body_indices, listed_body_indices + n_listed);
  HIPCHK(UploadTable(&j->d_structure_ints, ints));
  HIPCHK(j->d_structure_thresholds.alloc(size_t(n_structures) * 4));
  HIPCHK(hipMemcpy(j->d_structure_thresholds.p, error_thresholds, size_t(n_structures) * 4, hipMemcpyHostToDevice));
  j->n_structures = 0;
  HIPCHK(j->structure_rows.Alloc(size_t(n_structures) * size_t(j->n_rows_max) * sizeof(m3t_structure_judgement),
                                 kMapped, true));
  j->n_structures = n_structures;
  j->structure_groups = size_t(n_groups);
  return M3T_OK;
}
int m3t_hip_judge_read_structures(m3t_hip_context* ctx, int judge, int first_row, int n_rows, m3t_structure_judgement* out) {
  CHECK_CTX();
  Judge* j = GetJudge(ctx, judge, "judge_read_structures");
  if (!j) return M3T_ERR_INVALID_ARGUMENT;
  REQUIRE(j->n_structures > 0, M3T_ERR_INVALID_ARGUMENT, "judge_read_structures: judge_set_structures first");
  REQUIRE(first_row >= 0 && n_rows >= 0 && first_row <= j->n_rows && n_rows <= j->n_rows - first_row,
          M3T_ERR_INVALID_ARGUMENT, "judge_read_structures: rows that have not been judged");
  if (n_rows == 0) return M3T_OK;
  REQUIRE(out, M3T_ERR_INVALID_ARGUMENT, "judge_read_structures: null output");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipEventSynchronize(j->row_done[size_t(first_row + n_rows - 1)].get()));  // rows complete in order
  const size_t n = size_t(j->n_structures);
  std::memcpy(out, j->structure_rows.as<m3t_structure_judgement>() + size_t(first_row) * n, size_t(n_rows) * n * sizeof(m3t_structure_judgement));
  return M3T_OK;
}
// OPTEvaluator::CalculatePoseResults for listed body `index` from now on (m3t_hip.h).  Waits for the stream and uploads:
// outside the frame loop, like judge_set_vertices.
int m3t_hip_judge_set_add_only(m3t_hip_context* ctx, int judge, int index, const float* geometry2body_pose) {
  CHECK_CTX();
  Judge* j = GetJudge(ctx, judge, "judge_set_add_only");
  if (!j) return M3T_ERR_INVALID_ARGUMENT;
  REQUIRE(index >= 0 && index < int(j->body_ids.size()), M3T_ERR_INVALID_ARGUMENT, "judge_set_add_only: bad body index");
  REQUIRE(j->n_rows == 0, M3T_ERR_INVALID_ARGUMENT, "judge_set_add_only: rows have been judged already (judge_clear first)");
  std::array<float, 12> g = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
  if (geometry2body_pose) {
    for (int i = 0; i < 16; ++i)
      REQUIRE(std::isfinite(geometry2body_pose[i]), M3T_ERR_INVALID_ARGUMENT,
              "judge_set_add_only: a non-finite entry in geometry2body_pose");
    for (int c = 0; c < 4; ++c)
      for (int r = 0; r < 3; ++r) g[size_t(3 * c + r)] = geometry2body_pose[4 * c + r];
  }
  HIPCHK(hipSetDevice(ctx->device));
  j->add_only[size_t(index)] = 1;
  j->geometry2body[size_t(index)] = g;
  return BuildJudgeTables(ctx, j);
}
// OPTEvaluator::CalculateDiameters (opt_evaluator.cpp:580-600) of one vertex set (m3t_hip.h).  Waits for the stream,
// uploads and waits for the result: outside the frame loop.  Touches nothing of the tracking state.
int m3t_hip_vertices_diameter(m3t_hip_context* ctx, const float* xyz, int n_vertices, float* diameter) {
  CHECK_CTX();
  REQUIRE(n_vertices >= 1 && n_vertices <= (1 << 20), M3T_ERR_INVALID_ARGUMENT, "vertices_diameter: 1 to 2^20 vertices");
  REQUIRE(xyz && diameter, M3T_ERR_INVALID_ARGUMENT, "vertices_diameter: null vertices or result");
  for (size_t i = 0; i < size_t(n_vertices) * 3; ++i)  // fmaxf would drop a NaN silently
    REQUIRE(std::isfinite(xyz[i]), M3T_ERR_INVALID_ARGUMENT, "vertices_diameter: a non-finite coordinate");
  if (n_vertices == 1) {
    *diameter = 0.0f;
    return M3T_OK;
  }
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n_tiles = (size_t(n_vertices) + M3T_DIAMETER_TILE - 1) / M3T_DIAMETER_TILE;
  const std::vector<float> padded = PadVertices(xyz, n_vertices, M3T_DIAMETER_TILE);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  DevMem vertices, max_bits;
  HIPCHK(UploadTable(&vertices, padded));
  HIPCHK(max_bits.alloc(sizeof(unsigned int)));
  HIPCHK(hipMemset(max_bits.p, 0, sizeof(unsigned int)));
  for (size_t first = 0; first < n_tiles; first += M3T_DIAMETER_ROW_TILES_PER_LAUNCH) {
    ScopedKernelTimer timer(ctx, 1);
    const size_t rows = std::min<size_t>(M3T_DIAMETER_ROW_TILES_PER_LAUNCH, n_tiles - first);
    hipLaunchKernelGGL(vertices_diameter_kernel, dim3(unsigned(n_tiles), unsigned(rows)), dim3(M3T_DIAMETER_THREADS), 0,
                       ctx->stream, vertices.as<float4>(), int(first), max_bits.as<unsigned int>());
  }
  HIPCHK(hipGetLastError());
  float d2 = 0.0f;
  HIPCHK(hipMemcpyAsync(&d2, max_bits.p, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *diameter = sqrtf(d2);
  return M3T_OK;
}
int m3t_hip_judge_clear(m3t_hip_context* ctx, int judge) {
  CHECK_CTX();
  Judge* j = GetJudge(ctx, judge, "judge_clear");
  if (!j) return M3T_ERR_INVALID_ARGUMENT;
  j->n_rows = 0;
  return M3T_OK;
}
int m3t_hip_calculate_correspondences(m3t_hip_context* ctx, int iteration, int corr_iteration) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  int r = RequireWholeFrames(ctx, "calculate_correspondences");
  if (r) return r;
  r = Prepare(ctx, true);
  if (r) return r;
  ctx->state_valid = true;
  if ((r = RenderForModalities(ctx, false))) return r;  // correspondence_renderer_ptrs tracker.cpp:447-452
  return LaunchCorrespondences(ctx, iteration, corr_iteration);
}
int m3t_hip_calculate_gradient_and_hessian(m3t_hip_context* ctx, int, int corr_iteration, int opt_iteration) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  int r = Prepare(ctx, false);
  if (r) return r;
  REQUIRE(ctx->state_valid, M3T_ERR_NOT_SET_UP, "CalculateCorrespondences has to be called first");
  return LaunchGradientHessian(ctx, corr_iteration, opt_iteration);
}
int m3t_hip_calculate_optimization(m3t_hip_context* ctx, int, int, int) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  int r = Prepare(ctx, false);
  if (r) return r;
  return LaunchOptimization(ctx);  // (with a communicator: link sums, ONE all-reduce, project + solve)
}
// Optimizer::CalculateOptimization split at the multi-GPU exchange point: *partial is a
// DEVICE pointer to `count` floats (the 6 + 36 gradient / Hessian sums of every link of every structure, zero for
// links whose modalities live in another process); sum it over the ranks that hold bodies of the structures (one
// RCCL all-reduce on the context stream), then call _end.
int m3t_hip_calculate_optimization_begin(m3t_hip_context* ctx, float** partial, size_t* count) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  int r = Prepare(ctx, false);
  if (r) return r;
  if (!ctx->tree_mode) {  // rigid bodies only: force the general path so that the sums exist
    ctx->tree_mode = true;
    ctx->fused_possible = false;
    r = UploadTreeTables(ctx);
    if (r) return r;
  }
  r = LaunchGather(ctx);
  if (r) return r;
  if (partial) *partial = ctx->d_link_sums.as<float>();
  if (count) *count = ctx->link_sums_count;
  return M3T_OK;
}
int m3t_hip_calculate_optimization_end(m3t_hip_context* ctx) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  REQUIRE(ctx->partial_ready, M3T_ERR_NOT_SET_UP, "calculate_optimization_begin has to be called first");
  return LaunchSolveSums(ctx);
}
// ---- RCCL: the one collective of the path (a kinematic structure spread over GPUs) ----
#define RCCLCHK(expr)                                                                                      \
  do {                                                                                                     \
    ncclResult_t _r = (expr);                                                                              \
    if (_r != ncclSuccess)                                                                                 \
      return Fail(ctx, M3T_ERR_DEVICE, std::string(#expr) + ": " +                                         \
                                           (g_rccl.GetErrorString ? g_rccl.GetErrorString(_r) : "RCCL error")); \
  } while (0)
int m3t_hip_comm_get_unique_id(m3t_hip_context* ctx, void* id, size_t bytes) {
  CHECK_CTX();
  REQUIRE(id && bytes >= sizeof(ncclUniqueId), M3T_ERR_INVALID_ARGUMENT, "the id buffer must hold 128 bytes");
  REQUIRE(g_rccl.Load(), M3T_ERR_DEVICE, g_rccl.error);
  ncclUniqueId u;
  RCCLCHK(g_rccl.GetUniqueId(&u));
  std::memcpy(id, &u, sizeof(u));
  return M3T_OK;
}
int m3t_hip_comm_init_rank(m3t_hip_context* ctx, const void* id, size_t bytes, int n_ranks, int rank) {
  CHECK_CTX();
  REQUIRE(id && bytes >= sizeof(ncclUniqueId) && n_ranks >= 1 && rank >= 0 && rank < n_ranks, M3T_ERR_INVALID_ARGUMENT,
          "bad communicator description");
  REQUIRE(ctx->texture_mods.empty(), M3T_ERR_UNSUPPORTED, "a texture modality and a communicator / reduce callback do not go together");
  REQUIRE(g_rccl.Load(), M3T_ERR_DEVICE, g_rccl.error);
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->comm && ctx->comm_owned) RCCLCHK(g_rccl.CommDestroy(ctx->comm));
  ctx->comm = nullptr;
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  ncclComm_t comm = nullptr;
  RCCLCHK(g_rccl.CommInitRank(&comm, n_ranks, u, rank));
  ctx->comm = comm;
  ctx->comm_owned = true;
  // (soft constraints need no care here: every rank adds them AFTER the all-reduce of the link sums, as one process
  // does -- links_solve_sums_kernel)
  return M3T_OK;
}
int m3t_hip_comm_set(m3t_hip_context* ctx, void* nccl_comm) {
  CHECK_CTX();
  REQUIRE(nccl_comm == nullptr || ctx->texture_mods.empty(), M3T_ERR_UNSUPPORTED, "a texture modality and a communicator / reduce callback do not go together");
  REQUIRE(nccl_comm == nullptr || g_rccl.Load(), M3T_ERR_DEVICE, g_rccl.error);
  if (ctx->comm && ctx->comm_owned) RCCLCHK(g_rccl.CommDestroy(ctx->comm));
  ctx->comm = static_cast<ncclComm_t>(nccl_comm);
  ctx->comm_owned = false;
  return M3T_OK;
}
int m3t_hip_comm_destroy(m3t_hip_context* ctx) {
  CHECK_CTX();
  if (ctx->comm && ctx->comm_owned) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    RCCLCHK(g_rccl.CommDestroy(ctx->comm));
  }
  ctx->comm = nullptr;
  ctx->comm_owned = false;
  return M3T_OK;
}
// The host's own transport in the collective's place: fn(user, device buffer, count, hipStream_t) is called wherever
// ncclAllReduce would be, and has to leave the sum over the host's ranks in the buffer, ordered on that stream (it may
// synchronise the stream and do the sum on the host).  While it is set the context takes the distributed paths exactly
// as with a communicator.  NULL takes it out again.
int m3t_hip_comm_set_reduce_callback(m3t_hip_context* ctx, m3t_hip_reduce_fn fn, void* user) {
  CHECK_CTX();
  REQUIRE(fn == nullptr || ctx->texture_mods.empty(), M3T_ERR_UNSUPPORTED, "a texture modality and a communicator / reduce callback do not go together");
  ctx->reduce_fn = fn;
  ctx->reduce_user = fn ? user : nullptr;
  return M3T_OK;
}
// sum of the stacked link sums of all structures over the ranks of the communicator: ONE ncclAllReduce on the
// context's stream, in place (Link::CalculateGradientAndHessian link.cpp:184-193 is the sum being distributed)
int m3t_hip_calculate_optimization_allreduce(m3t_hip_context* ctx) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  return AllReducePartial(ctx);
}
// Tracker::CalculateConsistentPoses tracker.cpp:423 -> Optimizer::CalculateConsistentPoses optimizer.cpp:135
int m3t_hip_calculate_consistent_poses(m3t_hip_context* ctx) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  int r = Prepare(ctx, false);
  if (r) return r;
  if (!ctx->tree_mode) return M3T_OK;  // T * [I | 0] == T exactly for a free rigid body
  return LaunchSolve(ctx, true);
}
int m3t_hip_calculate_results(m3t_hip_context* ctx, int iteration) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  int r = RequireWholeFrames(ctx, "calculate_results");
  if (r) return r;
  r = Prepare(ctx, true);
  if (r) return r;
  if ((r = RenderForModalities(ctx, true))) return r;  // results_renderer_ptrs tracker.cpp:503-509
  if ((r = LaunchTextureKeyframes(ctx, true))) return r;
  return LaunchHistogram(ctx, iteration, false);
}

}  // extern "C"
namespace {
// ---- the tracking step: its launch choice is m3t_step_plan.h, one function per path below ---------------------------
using m3t_step::StepKernel;
using m3t_step::StepOverrides;

// What a path launched; m3t_hip_execute_tracking_step stores it into the context.
struct StepReport {
  StepKernel kernel = StepKernel::kNone;
  int shape[4] = {0, 0, 0, 0};  // objects or tracked links, workgroups per each, threads, histogram update in the launch
  bool histogram_fused = false;
  bool state_valid = false;         // line/point state + g/H on the device reflect the step
  bool links_device_newer = false;  // the step wrote the joints
  void Launched(StepKernel k, int n, int parts, int threads, bool fused_histogram) {
    kernel = k;
    shape[0] = n, shape[1] = parts, shape[2] = threads, shape[3] = fused_histogram ? 1 : 0;
    histogram_fused = fused_histogram;
  }
};

// ResidentBlocks of the kernels whose workgroups wait for each other (the plan asks by name)
int ResidentStepBlocks(Ctx* ctx, StepKernel kernel, int threads, size_t lds) {
  switch (kernel) {
    case StepKernel::kSplit: return ResidentBlocks(ctx, tracking_step_split_kernel, threads, lds);
    case StepKernel::kSplitPair: return ResidentBlocks(ctx, tracking_step_split_pair_kernel, threads, lds);
    case StepKernel::kSplitMoments: return ResidentBlocks(ctx, tracking_step_split_moments_kernel, threads, lds);
    case StepKernel::kSplitGuard: return ResidentBlocks(ctx, tracking_step_split_guard_kernel, threads, lds);
    case StepKernel::kSplitRender: return ResidentBlocks(ctx, tracking_step_split_render_kernel, threads, lds);
    default: return 0;
  }
}

// what the plan reads of the context (the table-overflow word: StepRigidFused)
m3t_step::RigidStepFacts RigidFacts(Ctx* ctx, bool roi_frames) {
  m3t_step::RigidStepFacts f;
  f.n = int(ctx->opt_table.size());
  f.compute_cus = ctx->compute_cus;
  f.lds_track = ctx->lds_track;
  f.lds_hist = ctx->lds_hist;
  f.lds_compact = ctx->lds_compact;
  f.lds_compact_table = ctx->lds_compact_table;
  f.table_cap = ctx->compact_table.table_cap;
  f.off_hist = ctx->layout.off_hist;
  f.total_floats = ctx->layout.total_floats;
  f.nl = ctx->layout.nl;
  f.np_max = ctx->np_max;
  f.has_region = !ctx->region_mods.empty();
  f.has_depth = !ctx->depth_mods.empty();
  f.regions_allow_moments_first = true;
  for (auto& m : ctx->region_mods)
    f.regions_allow_moments_first = f.regions_allow_moments_first &&
                                    m3t_step::RegionAllowsMomentsFirst(m->dev.measure_occlusions, m->dev.model_occlusions,
                                                                       m->dev.use_region_checking, m->dev.n_global_iterations);
  f.n_corr_iterations = ctx->n_corr_iterations;
  f.n_update_iterations = ctx->n_update_iterations;
  f.fused_mode = ctx->fused_mode;
  f.fuse_histogram_possible = ctx->fuse_histogram_possible;
  f.split_possible = ctx->split_possible;
  f.split_enabled = ctx->split_enabled;
  f.split_parts_override = ctx->split_parts_override;
  f.compact_possible = ctx->compact_possible;
  f.compact_fuses_histogram = ctx->compact_fuses_histogram;
  f.roi_frames = roi_frames;
  return f;
}

// The launches.  The step kernels of rigid objects share their first 13 arguments, the compact ones 10, the kinematic
// structures' 11; what follows (SplitParams, RoiGuardArgs, the first search of a per-search launch, ...) is the caller's.
template <typename K, typename... Tail>
void LaunchRigid(Ctx* ctx, K kernel, int grid, int threads, size_t lds, int iteration, int n_corr_iterations,
                 bool histogram_fused, Tail... tail) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, ctx->stream, ctx->d_opts.as<RigidOptDev>(),
                     ctx->d_region.as<RegionModDev>(), ctx->d_depth.as<DepthModDev>(), ctx->cams_active,
                     ctx->d_poses.as<float>(), ctx->layout, ctx->off_points, ctx->np_max, iteration, n_corr_iterations,
                     ctx->n_update_iterations, ctx->fused_mode == 2 ? 1 : 0, histogram_fused ? 1 : 0, tail...);
}
template <typename K, typename... Tail>
void LaunchCompact(Ctx* ctx, K kernel, int grid, int threads, size_t lds, const CompactLayout& layout, int iteration,
                   bool histogram_fused, Tail... tail) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, ctx->stream, ctx->d_opts.as<RigidOptDev>(),
                     ctx->d_region.as<RegionModDev>(), ctx->d_depth.as<DepthModDev>(), ctx->cams_active,
                     ctx->d_poses.as<float>(), layout, iteration, ctx->n_corr_iterations, ctx->n_update_iterations,
                     histogram_fused ? 1 : 0, tail...);
}
template <typename K, typename... Tail>
void LaunchTree(Ctx* ctx, K kernel, int grid, size_t lds, int iteration, Tail... tail) {
  const int off_tree = int((lds / 4 - ctx->tree_block_floats));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(M3T_BLOCK_THREADS), lds, ctx->stream, ctx->d_treesteps.as<TreeStepDev>(),
                     ctx->d_treeopts.as<TreeOptDev>(), ctx->d_region.as<RegionModDev>(), ctx->d_depth.as<DepthModDev>(),
                     ctx->cams_active, ctx->d_poses.as<float>(), ctx->layout, ctx->off_points, ctx->np_max, off_tree,
                     iteration, tail...);
}

// the exchange buffers and the per-launch descriptor of a split launch
int PrepareSplit(Ctx* ctx, int n, int parts, SplitParams* out) {
  const size_t per_object = size_t(2) * M3T_SPLIT_LANES * 32;  // granules
  int r = MappedWord(ctx, &ctx->split_abort);
  if (r) return r;
  if (ctx->split_objects < size_t(n) || ctx->split_seq >= (1u << 26) - 1) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->split_objects < size_t(n)) {
      HIPCHK(ctx->d_split.alloc(size_t(n) * per_object * sizeof(unsigned long long) + size_t(n) * sizeof(unsigned)));
      ctx->split_objects = size_t(n);
    }
    HIPCHK(hipMemset(ctx->d_split.p, 0, ctx->d_split.bytes));
    ctx->split_seq = 0;
  }
  ++ctx->split_seq;
  SplitParams sp{};
  sp.granules = ctx->d_split.as<unsigned long long>();
  sp.object_abort = reinterpret_cast<unsigned*>(sp.granules + ctx->split_objects * per_object);
  sp.host_abort = ctx->split_abort.dev_as<unsigned>();
  sp.seq = ctx->split_seq;
  if (++ctx->split_launches == 0) ctx->split_launches = 1;  // (0 = the word's initial value)
  sp.abort_id = ctx->split_launches;
  sp.n_objects = n;
  sp.n_parts = parts;
  sp.lshift = 0;
  while ((parts << sp.lshift) < M3T_SPLIT_LANES) ++sp.lshift;
  sp.per_part_lines = (ctx->layout.nl + parts - 1) / parts;
  sp.per_part_points = (ctx->np_max + parts - 1) / parts;
  *out = sp;
  return M3T_OK;
}

// Rigid objects, the whole loop nest in one launch (m3t_step_plan.h: PlanRigidStep says which).
int StepRigidFused(Ctx* ctx, int iteration, const StepOverrides& overrides, bool roi_frames, StepReport* report) {
  const int n = int(ctx->opt_table.size());
  ScopedKernelTimer timer(ctx, 0);
  m3t_step::RigidStepFacts facts = RigidFacts(ctx, roi_frames);
  if (ctx->table_overflow.host) facts.table_overflow = *ctx->table_overflow.as<volatile unsigned>();
  const m3t_step::RigidStepPlan plan = m3t_step::PlanRigidStep(
      facts, overrides, [ctx](StepKernel k, int threads, size_t lds) { return ResidentStepBlocks(ctx, k, threads, lds); });
  int r = M3T_OK;
  if (plan.compact_table) {
    if ((r = MappedWord(ctx, &ctx->table_overflow))) return r;
    ctx->compact_table.table_overflow = ctx->table_overflow.dev_as<unsigned>();
  }
  report->kernel = plan.kernel;
  // a step that reads rectangles runs the guarded kernels (m3t_kernels.hip, roi_guard_outside): an object whose poses
  // leave what was uploaded is not committed but flagged; roi_repair_kernel then fetches the whole frames of the
  // flagged objects' cameras and the step is launched again for the flagged objects alone
  RoiGuardArgs guard{};
  if (roi_frames) {
    guard.items = ctx->d_roi_items.as<RoiItemDev>();
    guard.rects = ctx->d_roi_rects.as<m3t_roi_rect>();
    guard.n_cams = int(ctx->cameras.size());
    guard.n_rect_slots = ctx->roi_rect_slots;
    guard.n_poses = ctx->roi_n_poses;
    guard.mode = 1;
    guard.misses = Ctx::RoiMissList(ctx->roi_miss.dev, false);
    guard.miss_capacity = int(Ctx::kRoiMissCapacity);
    guard.unrecovered = Ctx::RoiMissList(ctx->roi_miss.dev, true);
  }
  const int grid = plan.grid(n), threads = plan.threads, n_corr = ctx->n_corr_iterations;
  const size_t lds = plan.lds;
  const bool fused = plan.histogram_fused;
  // pass 0: the step; passes 1 (repair) and 2 (the flagged objects again, on whole frames) only behind rectangles
  for (int pass = 0; pass < (roi_frames ? 2 : 1); ++pass) {
    if (pass == 1) {
      for (size_t sl = 0; sl < ctx->roi_sources.size(); ++sl)
        for (const Ctx::RoiSource& source : ctx->roi_sources[sl]) {
          const Camera& c0 = *ctx->cameras[source.ids[0]];
          if (c0.current != int(sl) || !c0.slot_is_roi[sl]) continue;  // (this step reads another slot of these cameras)
          m3t_roi_rect* rects = ctx->d_roi_rects.as<m3t_roi_rect>() + sl * ctx->cameras.size();
          hipLaunchKernelGGL(roi_repair_kernel, dim3((c0.intr.height + 7) / 8, unsigned(source.ids.size())), dim3(256), 0,
                             ctx->stream, source.d_ids, ctx->d_roi_items.as<RoiItemDev>(), ctx->d_roi_item_first.as<int>(),
                             ctx->d_opts.as<RigidOptDev>(), ctx->roi_n_poses, rects, source.src, source.camera_stride,
                             source.row_step, c0.frame(int(sl)), c0.frame_bytes, c0.pitch, c0.intr.width, c0.intr.height,
                             c0.is_depth ? 2 : 3);
        }
      guard.mode = 2;
    }
    SplitParams sp{};
    if (plan.split() && (r = PrepareSplit(ctx, n, plan.parts, &sp))) return r;
    switch (plan.kernel) {
      case StepKernel::kCompactGuard:
        LaunchCompact(ctx, tracking_step_compact_guard_kernel, grid, threads, lds, ctx->compact, iteration, fused, guard);
        break;
      case StepKernel::kCompactTable:
        LaunchCompact(ctx, tracking_step_compact_table_kernel, grid, threads, lds, ctx->compact_table, iteration, fused);
        break;
      case StepKernel::kCompactWide:
        LaunchCompact(ctx, tracking_step_compact_wide_kernel, grid, threads, lds, ctx->compact, iteration, fused);
        break;
      case StepKernel::kCompact:
        LaunchCompact(ctx, tracking_step_compact_kernel, grid, threads, lds, ctx->compact, iteration, fused);
        break;
      case StepKernel::kSplitGuard:
        LaunchRigid(ctx, tracking_step_split_guard_kernel, grid, threads, lds, iteration, n_corr, fused, sp, guard);
        break;
      case StepKernel::kSplitPair:
        LaunchRigid(ctx, tracking_step_split_pair_kernel, grid, threads, lds, iteration, n_corr, fused, sp);
        break;
      case StepKernel::kSplitMoments:
        LaunchRigid(ctx, tracking_step_split_moments_kernel, grid, threads, lds, iteration, n_corr, fused, sp);
        break;
      case StepKernel::kSplit:
        LaunchRigid(ctx, tracking_step_split_kernel, grid, threads, lds, iteration, n_corr, fused, sp);
        break;
      case StepKernel::kLdsGuard:
        LaunchRigid(ctx, tracking_step_lds_guard_kernel, grid, threads, lds, iteration, n_corr, fused, guard);
        break;
      case StepKernel::kGuard:
        LaunchRigid(ctx, tracking_step_guard_kernel, grid, threads, lds, iteration, n_corr, fused, guard);
        break;
      case StepKernel::kLdsPair:
        LaunchRigid(ctx, tracking_step_lds_pair_kernel, grid, threads, lds, iteration, n_corr, fused, 0);
        break;
      case StepKernel::kPair:
        LaunchRigid(ctx, tracking_step_pair_kernel, grid, threads, lds, iteration, n_corr, fused, 0);
        break;
      case StepKernel::kLds:
        LaunchRigid(ctx, tracking_step_lds_kernel, grid, threads, lds, iteration, n_corr, fused, 0);
        break;
      case StepKernel::kPlain:
        LaunchRigid(ctx, tracking_step_kernel, grid, threads, lds, iteration, n_corr, fused, 0);
        break;
      default:
        return Fail(ctx, M3T_ERR_DEVICE, std::string("no launch for the planned kernel ") + m3t_step::StepKernelName(plan.kernel));
    }
    HIPCHK(hipGetLastError());
  }
  // (where the repair fetched a whole frame only the device's rectangle table knows it: for the host the slot keeps
  // counting as a rectangle slot -- conservative -- until the next upload into it)
  report->Launched(plan.kernel, n, plan.split() ? plan.parts : 1, threads, fused);
  report->state_valid = ctx->fused_mode == 2;
  return M3T_OK;
}

// Renderer-fed branches (modelled occlusions, region / silhouette checking): the focused renderings are redrawn
// before every correspondence search from the bodies' current poses (correspondence_renderer_ptrs,
// tracker.cpp:447-452), so the loop nest runs one search per launch -- the renderers, then ONE launch for the
// search and its Newton steps of all objects -- instead of one launch per sub-step: 4 instead of 11 per search.
int StepPerSearch(Ctx* ctx, int iteration, const StepOverrides& overrides, StepReport* report) {
  ScopedKernelTimer timer(ctx, 0);
  const int n = int(ctx->opt_table.size());
  // a batch that leaves CUs idle: several workgroups per object here too (tracking_step_split_render_kernel: the
  // split kernel with the renderer-fed branches compiled in, one search per launch)
  int parts = 0, r = M3T_OK;
  size_t lds_split = 0;
  bool shared = false;
  for (auto& m : ctx->region_mods) shared = shared || m->shared_histograms >= 0 || m->p.n_histogram_bins < 4;
  if (!shared && ctx->split_enabled && ctx->n_corr_iterations < 64 && !overrides.no_split)
    parts = m3t_step::RigidSplitParts(
        RigidFacts(ctx, false), overrides, StepKernel::kSplitRender, M3T_BLOCK_THREADS, false, 16,
        [ctx](StepKernel k, int threads, size_t lds) { return ResidentStepBlocks(ctx, k, threads, lds); }, &lds_split);
  const bool lds_table = ctx->layout.off_hist >= 0;
  for (int c = 0; c < ctx->n_corr_iterations; ++c) {
    if ((r = RenderForModalities(ctx, false))) return r;
    if (parts >= 2) {
      SplitParams sp{};
      if ((r = PrepareSplit(ctx, n, parts, &sp))) return r;
      hipLaunchKernelGGL(tracking_step_split_render_kernel, dim3((n + 7) / 8 * 8 * parts), dim3(M3T_BLOCK_THREADS),
                         lds_split, ctx->stream, ctx->d_opts.as<RigidOptDev>(), ctx->d_region.as<RegionModDev>(),
                         ctx->d_depth.as<DepthModDev>(), ctx->cams_active, ctx->d_poses.as<float>(), ctx->layout,
                         ctx->off_points, ctx->np_max, iteration, ctx->n_update_iterations,
                         ctx->fused_mode == 2 ? 1 : 0, c, sp);
    } else if (lds_table) {
      LaunchRigid(ctx, tracking_step_lds_kernel, n, M3T_BLOCK_THREADS, ctx->lds_track, iteration, 1, false, c);
    } else {
      LaunchRigid(ctx, tracking_step_kernel, n, M3T_BLOCK_THREADS, ctx->lds_track, iteration, 1, false, c);
    }
  }
  HIPCHK(hipGetLastError());
  report->Launched(parts >= 2 ? StepKernel::kSplitRender : (lds_table ? StepKernel::kLds : StepKernel::kPlain), n,
                   parts >= 2 ? parts : 1, M3T_BLOCK_THREADS, false);
  report->state_valid = ctx->fused_mode == 2;
  return M3T_OK;
}

// kinematic structures: the whole loop nest in one launch, one workgroup per link that carries modalities
int StepTreeFused(Ctx* ctx, int iteration, const StepOverrides& overrides, StepReport* report) {
  ScopedKernelTimer timer(ctx, 0);
  const bool want_fused_histogram = !ctx->region_mods.empty() && ctx->hist_counts_in_lds && ctx->shared_histograms.empty() &&
                                    !overrides.no_fused_histogram;
  const size_t lds = TreeStepLds(ctx, want_fused_histogram);
  int r = MappedWord(ctx, &ctx->split_abort);
  if (r) return r;
  if (ctx->tree_seq >= (1u << 26) - 1) {  // the tags restart: clear them first
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemset(ctx->d_tree_exchange.p, 0, ctx->d_tree_exchange.bytes));
    ctx->tree_seq = 0;
  }
  TreeStepParams xp{};
  xp.seq = ++ctx->tree_seq;
  if (++ctx->split_launches == 0) ctx->split_launches = 1;
  xp.abort_id = ctx->split_launches;
  xp.host_abort = ctx->split_abort.dev_as<unsigned>();
  // Structures that leave CUs idle (the 8-body chain: 8 workgroups on 256 CUs): several workgroups per tracked link
  // (tracking_step_tree_split_kernel; open structures only -- the constrained kernel keeps one).  The parts of a link
  // exchange their lines' results, so all workgroups must be resident: checked like the split kernel's launch.
  int tree_parts = 0;
  if (!ctx->tree_constrained && ctx->n_corr_iterations < 64 && !overrides.no_tree_split) {
    bool can = true;
    for (auto& m : ctx->region_mods) can = can && m->shared_histograms < 0 && m->p.n_histogram_bins >= 4;
    const int elements = std::max(ctx->layout.nl, ctx->depth_mods.empty() ? 1 : ctx->np_max);
    // (the 8-body chain, ms per step: 1 part 0.3046, 2: 0.2939, 4: 0.2756, 8: 0.2649; profiles/r05_chain8_parts.txt)
    const int limit = overrides.tree_parts.set ? overrides.tree_parts.value : 8;
    if (can)
      tree_parts = m3t_step::SplitParts(ctx->n_treesteps, elements, limit, ctx->compute_cus, [ctx, lds](int) {
        if (ctx->tree_split_lds_attribute != lds) {
          if (hipFuncSetAttribute(reinterpret_cast<const void*>(tracking_step_tree_split_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
          }
          ctx->tree_split_lds_attribute = lds;
        }
        const int resident = ResidentBlocks(ctx, tracking_step_tree_split_kernel, M3T_BLOCK_THREADS, lds);
        return std::min(resident, int(size_t(160) * 1024 / lds));
      });
  }
  const int fuse = want_fused_histogram ? 1 : 0, n_corr = ctx->n_corr_iterations, n_update = ctx->n_update_iterations;
  StepKernel kernel = ctx->tree_constrained ? StepKernel::kTreeConstrained : StepKernel::kTree;
  if (tree_parts >= 2) {
    SplitParams sp{};
    if ((r = PrepareSplit(ctx, ctx->n_treesteps, tree_parts, &sp))) return r;
    kernel = StepKernel::kTreeSplit;
    LaunchTree(ctx, tracking_step_tree_split_kernel, ctx->n_treesteps * tree_parts, lds, iteration, n_corr, n_update, fuse, xp, sp);
  } else if (ctx->tree_constrained) {
    LaunchTree(ctx, tracking_step_tree_constrained_kernel, ctx->n_treesteps, lds, iteration, n_corr, n_update, fuse, xp);
  } else {
    LaunchTree(ctx, tracking_step_tree_kernel, ctx->n_treesteps, lds, iteration, n_corr, n_update, fuse, xp);
  }
  HIPCHK(hipGetLastError());
  report->Launched(kernel, ctx->n_treesteps, tree_parts >= 2 ? tree_parts : 1, M3T_BLOCK_THREADS, want_fused_histogram);
  report->links_device_newer = true;
  report->state_valid = false;
  return M3T_OK;
}

// kinematic structures spread over processes: one launch and one all-reduce (of the link sums) per Newton step,
// a last launch for the last solve, the bodies and the histogram update (m3t_links.hip, tree_segment_body)
int StepTreeSegmented(Ctx* ctx, int iteration, const StepOverrides& overrides, StepReport* report) {
  ScopedKernelTimer timer(ctx, 0);
  const bool want_fused_histogram = !ctx->region_mods.empty() && ctx->hist_counts_in_lds && ctx->shared_histograms.empty() &&
                                    !overrides.no_fused_histogram;
  const size_t lds = TreeStepLds(ctx, want_fused_histogram);
  float* sums[2] = {ctx->d_link_sums.as<float>(), ctx->d_link_sums_alt.as<float>()};
  const int n_newton = ctx->n_corr_iterations * ctx->n_update_iterations;
  // launch k reads the link table launch k - 1 wrote: the primary table at k <= 1 (launch 0 solves nothing and writes
  // nothing), then alternately; launch k >= 1 writes the other one.  The last launch (k = n_newton) must leave the
  // joints in the primary table, the one the rest of the library reads: an odd n_newton ends in the second one and
  // is copied over.
  // FIRST (the links take their bodies' poses) and FINAL (the bodies take their links') meet in one launch only when
  // the frame has a single Newton step: a workgroup that starts late would then seed from poses a faster one has
  // already written back, so that launch seeds from a snapshot taken in front of the loop
  const float* first_poses = ctx->d_poses.as<float>();
  if (n_newton == 1) {
    if (ctx->d_poses_first.bytes < ctx->d_poses.bytes) HIPCHK(ctx->d_poses_first.alloc(ctx->d_poses.bytes));
    HIPCHK(hipMemcpyAsync(ctx->d_poses_first.p, ctx->d_poses.p, ctx->body_poses.size() * 4, hipMemcpyDeviceToDevice,
                          ctx->stream));
    first_poses = ctx->d_poses_first.as<float>();
  }
  for (int k = 0; k <= n_newton; ++k) {
    TreeSegmentParams sp{};
    const int c = k / std::max(ctx->n_update_iterations, 1), u = k % std::max(ctx->n_update_iterations, 1);
    const bool last = k == n_newton;
    int flags = 0;
    if (k <= 1) flags |= TSEG_FIRST;  // (nothing has written the bodies' link2world yet: launch 0 solves nothing)
    if (k > 0) flags |= TSEG_SOLVE;
    if (!last) {
      flags |= TSEG_SUMS;
      if (u == 0) flags |= TSEG_SEARCH | (ctx->n_update_iterations > 1 ? TSEG_STORE_STATE : 0);
      else flags |= TSEG_LOAD_STATE;
    } else {
      flags |= TSEG_FINAL;
    }
    const bool read_alt = k >= 2 && (k % 2 == 0);
    const bool write_alt = k >= 1 && (k % 2 == 1);
    if (read_alt) flags |= TSEG_LINKS_FROM_ALT;
    if (write_alt) flags |= TSEG_LINKS_TO_ALT;
    sp.flags = flags;
    sp.corr_iteration = last ? 0 : c;
    sp.opt_iteration = last ? 0 : u;
    sp.sums_in = sums[(k + 1) & 1];  // what launch k - 1 wrote and the all-reduce summed
    sp.sums_out = sums[k & 1];
    sp.first_poses = first_poses;
    const int fuse = (last && want_fused_histogram) ? 1 : 0;
    if (ctx->tree_constrained)
      LaunchTree(ctx, tracking_step_tree_segment_constrained_kernel, ctx->n_treesteps, lds, iteration, fuse, sp);
    else
      LaunchTree(ctx, tracking_step_tree_segment_kernel, ctx->n_treesteps, lds, iteration, fuse, sp);
    HIPCHK(hipGetLastError());
    if (!last) {
      ctx->partial_ready = true;
      int r = AllReducePartial(ctx, sums[k & 1]);
      if (r) return r;
      ctx->partial_ready = false;
    }
  }
  if (n_newton >= 1 && (n_newton % 2 == 1))  // the last launch wrote the second table
    HIPCHK(hipMemcpyAsync(ctx->d_links.p, ctx->d_links_alt.p, ctx->d_links.bytes, hipMemcpyDeviceToDevice, ctx->stream));
  report->Launched(ctx->tree_constrained ? StepKernel::kTreeSegmentConstrained : StepKernel::kTreeSegment, ctx->n_treesteps, 1,
                   M3T_BLOCK_THREADS, want_fused_histogram);
  report->links_device_newer = true;
  report->state_valid = false;
  return M3T_OK;
}

// Tracker::ExecuteTrackingStep tracker.cpp:344-364, one launch per sub-step
int StepSubSteps(Ctx* ctx, int iteration, StepReport* report) {
  report->kernel = StepKernel::kNone;
  int r = M3T_OK;
  for (int c = 0; c < ctx->n_corr_iterations; ++c) {
    if ((r = RenderForModalities(ctx, false))) return r;
    if ((r = LaunchCorrespondences(ctx, iteration, c))) return r;
    for (int u = 0; u < ctx->n_update_iterations; ++u) {
      if ((r = LaunchGradientHessian(ctx, c, u))) return r;
      if ((r = LaunchOptimization(ctx))) return r;
    }
  }
  report->state_valid = true;
  return M3T_OK;
}
}  // namespace
extern "C" {

int m3t_hip_execute_tracking_step(m3t_hip_context* ctx, int iteration) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  const StepOverrides overrides = m3t_step::ReadStepOverrides();  // every step: tests change them between two steps
  const bool host_poses_before = ctx->poses_dirty_host;  // (Prepare uploads them)
  int r = Prepare(ctx, true, true);  // a whole step is marked as a reader below
  if (r) return r;
  if ((r = CheckSplitExchange(ctx))) return r;  // an earlier step that was abandoned on the device
  const bool rigid_fused = ctx->fused_mode >= 1 && ctx->fused_possible && !ctx->Distributed();
  bool roi_frames = false;  // does this step read a slot that holds a rectangle only
  for (auto& cam : ctx->cameras) roi_frames = roi_frames || cam->slot_is_roi[cam->current];
  REQUIRE(!roi_frames || (rigid_fused && ctx->n_roi_items > 0), M3T_ERR_UNSUPPORTED,
          "a frame slot holds the trackers' rectangle only (ROI ingest): that needs the fused step of rigid objects");
  const bool roi_active = ctx->roi_enabled && ctx->n_roi_items > 0 && rigid_fused;
  float* const roi_snapshots = ctx->d_roi_pose_snapshot.as<float>();
  const size_t roi_snapshot_floats = ctx->d_roi_pose_snapshot.bytes / (4 * Ctx::kRoiSnapshots);
  if (roi_active) {
    // the poses the NEXT frame's rectangles are computed from (m3t_hip_cameras_upload_batch_roi_async, copy stream):
    // the poses this step starts from.  The previous step's end-of-step snapshot holds exactly those -- and was ready
    // before this step had to wait for its own frame, so the next pull can follow the current one at once -- unless
    // something else touched the poses in between.  The snapshot before that one (adaptive margins) is the start of
    // the previous step.
    if (ctx->roi_end_valid && !host_poses_before && !ctx->ingest.untracked()) {
      ctx->roi_prev = ctx->roi_use;
      ctx->roi_use = ctx->roi_end_index;
    } else {
      ctx->roi_prev = -1;
      ctx->roi_use = 0;
      HIPCHK(hipMemcpyAsync(roi_snapshots, ctx->d_poses.p, ctx->body_poses.size() * 4, hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK(hipEventRecord(ctx->roi_snapshot_done[0].get(), ctx->stream));
    }
    ctx->roi_snapshot_valid = true;
  }
  ctx->roi_end_valid = false;
  ctx->roi_recorded = roi_active;
  // the paths (m3t_step_plan.h; DESIGN.md section 5 has the table)
  StepReport report;
  std::memcpy(report.shape, ctx->last_step_shape, sizeof(report.shape));  // (the per-sub-step path has no shape of its own)
  report.state_valid = ctx->state_valid;
  if (rigid_fused)  // (a communicator: the structures span GPUs)
    r = StepRigidFused(ctx, iteration, overrides, roi_frames, &report);
  else if (ctx->fused_mode >= 1 && ctx->fused_per_search_possible && !ctx->Distributed() && !ctx->tree_mode &&
           !overrides.no_search_fusion)
    r = StepPerSearch(ctx, iteration, overrides, &report);
  else if (TreeStepFused(ctx, overrides))
    r = StepTreeFused(ctx, iteration, overrides, &report);
  else if (TreeStepSegmented(ctx, overrides))
    r = StepTreeSegmented(ctx, iteration, overrides, &report);
  else
    r = StepSubSteps(ctx, iteration, &report);
  ctx->last_step_kernel = report.kernel;
  std::memcpy(ctx->last_step_shape, report.shape, sizeof(report.shape));
  ctx->state_valid = report.state_valid;
  if (report.links_device_newer) ctx->links_device_newer = true;
  if (r) return r;
  if (!report.histogram_fused) {
    if ((r = RenderForModalities(ctx, true))) return r;
    if ((r = LaunchTextureKeyframes(ctx, true))) return r;
    if ((r = LaunchHistogram(ctx, iteration, false, roi_frames))) return r;
  }
  if (roi_active) {  // the poses the step ends on = the poses the next one starts from
    // (the third buffer: a rectangle upload that is still to run on the copy stream reads roi_use and roi_prev)
    ctx->roi_end_index = 0;
    while (ctx->roi_end_index == ctx->roi_use || ctx->roi_end_index == ctx->roi_prev) ++ctx->roi_end_index;
    HIPCHK(hipMemcpyAsync(roi_snapshots + size_t(ctx->roi_end_index) * roi_snapshot_floats, ctx->d_poses.p,
                          ctx->body_poses.size() * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipEventRecord(ctx->roi_snapshot_done[ctx->roi_end_index].get(), ctx->stream));
    ctx->roi_end_valid = true;
  }
  HIPCHK(ctx->ingest.MarkRead(ctx->stream, ctx->cameras, nullptr));  // the current slot of every camera
  return M3T_OK;
}
// Refiner::RefinePoses src/refiner.cpp:76-117 (one launch per sub-step)
int m3t_hip_refine_poses(m3t_hip_context* ctx, int n_corr_iterations, int n_update_iterations) {
  CHECK_CTX();
  REQUIRE(n_corr_iterations >= 0 && n_update_iterations >= 0, M3T_ERR_INVALID_ARGUMENT, "bad iteration counts");
  int r = m3t_hip_calculate_consistent_poses(ctx);
  if (r) return r;
  for (int c = 0; c < n_corr_iterations; ++c) {
    if ((r = m3t_hip_start_modalities(ctx, 0))) return r;  // StartModality(0, corr_iteration)
    if ((r = m3t_hip_calculate_correspondences(ctx, 0, c))) return r;
    for (int u = 0; u < n_update_iterations; ++u) {
      if ((r = m3t_hip_calculate_gradient_and_hessian(ctx, 0, c, u))) return r;
      if ((r = m3t_hip_calculate_optimization(ctx, 0, c, u))) return r;
    }
  }
  return M3T_OK;
}
int m3t_hip_execute_tracking_cycle(m3t_hip_context* ctx, int iteration) {
  return m3t_hip_execute_tracking_step(ctx, iteration);
}
int m3t_hip_set_kernel_timing(m3t_hip_context* ctx, int enable) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->pending.clear();
  ctx->timing = enable == 1;
  ctx->timing_region = enable == 2;
  ctx->kernel_ms[0] = ctx->kernel_ms[1] = 0.0;
  ctx->kernel_launches[0] = ctx->kernel_launches[1] = 0;
  if (ctx->timing_region) {  // the stream is idle (synchronised above): the region starts here
    HIPCHK(ctx->region.Ensure(hipEventDefault));
    HIPCHK(hipEventRecord(ctx->region.a.get(), ctx->stream));
  }
  return M3T_OK;
}
int m3t_hip_get_step_shape(m3t_hip_context* ctx, int shape[4]) {
  CHECK_CTX();
  REQUIRE(shape, M3T_ERR_INVALID_ARGUMENT, "null output");
  std::memcpy(shape, ctx->last_step_shape, sizeof(ctx->last_step_shape));
  return M3T_OK;
}
int m3t_hip_debug_log_checksum(m3t_hip_context* ctx, unsigned first_bits, unsigned last_bits,
                               unsigned long long out[3]) {
  CHECK_CTX();
  REQUIRE(out && first_bits <= last_bits, M3T_ERR_INVALID_ARGUMENT, "bad range");
  HIPCHK(hipSetDevice(ctx->device));
  DevMem sums;  // (a failure leaves through its destructor, which waits for the device)
  HIPCHK(sums.alloc(24));
  unsigned long long* d = sums.as<unsigned long long>();
  HIPCHK(hipMemsetAsync(d, 0, 24, ctx->stream));
  hipLaunchKernelGGL(log_checksum_kernel, dim3(ctx->prop.multiProcessorCount * 8), dim3(256), 0, ctx->stream,
                     first_bits, last_bits, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d, 24, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return M3T_OK;
}
int m3t_hip_comm_get_allreduce_count(m3t_hip_context* ctx, long long* count) {
  CHECK_CTX();
  REQUIRE(count, M3T_ERR_INVALID_ARGUMENT, "null output");
  *count = ctx->allreduce_calls;
  return M3T_OK;
}
int m3t_hip_comm_get_rank_count(m3t_hip_context* ctx, int* n_ranks) {
  CHECK_CTX();
  REQUIRE(n_ranks, M3T_ERR_INVALID_ARGUMENT, "null output");
  *n_ranks = 0;
  if (!ctx->comm) return M3T_OK;
  REQUIRE(g_rccl.Load() && g_rccl.CommCount, M3T_ERR_UNSUPPORTED, "ncclCommCount is not available in the loaded librccl");
  const ncclResult_t rc = g_rccl.CommCount(ctx->comm, n_ranks);
  if (rc != ncclSuccess)
    return Fail(ctx, M3T_ERR_DEVICE,
                std::string("ncclCommCount: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error"));
  return M3T_OK;
}
int m3t_hip_get_step_kernel(m3t_hip_context* ctx, char* name, size_t capacity) {
  CHECK_CTX();
  REQUIRE(name && capacity > 0, M3T_ERR_INVALID_ARGUMENT, "null output");
  std::snprintf(name, capacity, "%s", m3t_step::StepKernelName(m3t_step::ReportedStepKernel(ctx->last_step_kernel)));
  return M3T_OK;
}
int m3t_hip_get_step_variant(m3t_hip_context* ctx, char* name, size_t capacity) {
  CHECK_CTX();
  REQUIRE(name && capacity > 0, M3T_ERR_INVALID_ARGUMENT, "null output");
  std::snprintf(name, capacity, "%s", m3t_step::StepKernelName(ctx->last_step_kernel));
  return M3T_OK;
}
int m3t_hip_get_kernel_timing(m3t_hip_context* ctx, float total_ms[2], int launches[2]) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->timing_region) {  // device time from the enabling call to here, all of it booked on the tracking launches
    HIPCHK(hipEventRecord(ctx->region.b.get(), ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, ctx->region.a.get(), ctx->region.b.get()));
    if (total_ms) { total_ms[0] = ms; total_ms[1] = 0.0f; }
    if (launches) { launches[0] = ctx->kernel_launches[0]; launches[1] = ctx->kernel_launches[1]; }
    return M3T_OK;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (auto& p : ctx->pending) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, p.events.a.get(), p.events.b.get()) == hipSuccess) {
      ctx->kernel_ms[p.which] += ms;
      ctx->kernel_launches[p.which] += 1;
    }
  }
  ctx->pending.clear();
  if (total_ms) { total_ms[0] = float(ctx->kernel_ms[0]); total_ms[1] = float(ctx->kernel_ms[1]); }
  if (launches) { launches[0] = ctx->kernel_launches[0]; launches[1] = ctx->kernel_launches[1]; }
  return M3T_OK;
}
#ifdef M3T_PHASE_TIMING
int m3t_hip_debug_phase_rows(void) { return M3T_PHASE_ROWS; }  // how many values m3t_hip_debug_phase_cycles writes
int m3t_hip_debug_phase_cycles(m3t_hip_context* ctx, unsigned long long* out, int reset) {
  CHECK_CTX();
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_cycles), M3T_PHASE_ROWS * sizeof(unsigned long long)));
  if (reset) {
    unsigned long long z[M3T_PHASE_ROWS] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z, sizeof(z)));
  }
  return M3T_OK;
}
int m3t_hip_debug_exchange_times(m3t_hip_context* ctx, unsigned long long* out768) {
  CHECK_CTX();
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpyFromSymbol(out768, HIP_SYMBOL(g_exchange_times), 768 * sizeof(unsigned long long)));
  return M3T_OK;
}
#endif
int m3t_hip_sync(m3t_hip_context* ctx) {
  CHECK_CTX();
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return CheckSplitExchange(ctx);
}

}  // extern "C"
