// m3t_structures.hip -- the RTB evaluator's two per-frame operations for the kinematic structures of a batch
// (examples/rtb_evaluator.cpp): RTBEvaluator::SetBodyAndJointPoses (:809-858) + Tracker::StartModalities for the
// listed structures alone (m3t_hip_reset_structures) and RTBEvaluator::CalculatePoseResults' combination of the
// per-body errors (:930-989, m3t_hip_judge_set_structures).  Included by m3t_hip_api.hip behind m3t_links.hip and
// m3t_judge.hip (same translation unit: LinkDev / TreeOptDev, the pose helpers, region_histogram_update and
// shared_histogram_finish are the ones of the tracking kernels).
//
// Device state that follows the joint poses and outlives a step (what a reset would have to refresh): none beyond the
// link table itself.  The tree kernels rebuild their constants (tree_tables), adjoints and Jacobians (tree_kinematics,
// tree_kin_adjoints) from the link table at the start of every launch, in LDS or in the structure's work array;
// links_project_kernel hands its Jacobians to links_solve_kernel through the work array, but both are launched by one
// calculate_optimization call.  The second link table (links_alt) is read by a segment launch only after the launch in
// front of it, of the same frame, has written it (k >= 2 reads what k - 1 wrote): nothing of it survives a frame.  The
// exchange granules carry sums, tagged with the launch number.  So the reset writes the primary link table and the
// bodies' poses, nothing else.

struct StructureResetDev {  // one listed structure of a m3t_hip_reset_structures call
  int opt;          // row of the TreeOptDev table, or -1: a context of free rigid bodies (there is no link table)
  int first_entry;  // its links in the call's entry list, in table order (depth first, parents before children)
  int n_links;
};
struct StructureLinkResetDev {  // one link of it
  int body;   // body id or -1
  int pose;   // index of the body's new pose in the call's poses, -1: the link stays (the body-less root of mode 1)
  int joint;  // >= 0: joint2parent from this pose index (the parent body's new pose); -1: joint2parent stays;
              // -2: joint2parent = the new pose bit for bit (:853, a child of the root in mode 1)
};

extern "C" {

// m3t_hip_reset_structures, first launch: one workgroup per listed structure, a lane per link in table order.  Every
// link's new joint follows from the call's poses alone (its own, its parent body's) and from its body2joint as the
// table holds it -- the value tracking has left there for a link with fixed_body2joint_pose == 0 --, so no lane waits
// for another.  :836-838, left to right: (parent world2body * body2world) * body2joint^-1.
// Also first_iteration of the listed region modalities (RegionModality::StartModality :378).
__global__ void __launch_bounds__(64)
reset_structures_kernel(const TreeOptDev* opts, float* body_poses, const StructureResetDev* structures,
                        const StructureLinkResetDev* entries, const float* poses, RegionModDev* mods,
                        const int* region_ids, int n_region, int iteration) {
  const StructureResetDev s = structures[blockIdx.x];
  LinkDev* links = s.opt >= 0 ? opts[s.opt].links : nullptr;
  for (int li = threadIdx.x; li < s.n_links; li += blockDim.x) {
    const StructureLinkResetDev e = entries[s.first_entry + li];
    if (e.pose < 0) continue;
    const float* p = poses + 16 * e.pose;
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = p[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) body_poses[16 * e.body + i] = v[i];
    if (!links) continue;
    LinkDev& l = links[li];
#pragma unroll
    for (int i = 0; i < 16; ++i) l.link2world[i] = v[i];
    if (e.joint >= 0) {
      const Affine parent2world = load_pose(poses + 16 * e.joint);
      const Affine joint2parent =
          mul_pose(mul_pose(inverse_pose(parent2world), load_pose(v)), inverse_pose(load_pose(l.body2joint)));
      float out[16];
      affine_to_array(joint2parent, out);
#pragma unroll
      for (int i = 0; i < 16; ++i) l.joint2parent[i] = out[i];
    } else if (e.joint == -2) {
#pragma unroll
      for (int i = 0; i < 16; ++i) l.joint2parent[i] = v[i];
    }
  }
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_region; r += gridDim.x * blockDim.x)
    mods[region_ids[r]].first_iteration = iteration;
}

// m3t_hip_reset_structures, second launch: StartModality (:375-388) of the region modalities region_ids[0 .. gridDim.x),
// one workgroup each -- region_histogram_list_kernel's body, with the branch of region_histogram_kernel for a modality
// on shared ColorHistograms (it only adds its samples to the shared object's counts, which are zero between calls:
// shared_histogram_finish ends with ClearMemory).
__global__ void __launch_bounds__(M3T_BLOCK_THREADS)
structures_histogram_list_kernel(const RegionModDev* mods, const int* region_ids, const CameraDev* cams,
                                 const float* body_poses, int counts_in_lds) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  CRegion& m = *(CRegion*)(mods + region_ids[blockIdx.x]);
  CCam& cam = *(CCam*)(cams + m.camera);
  CCam* dcam = m.measure_occlusions ? (CCam*)(cams + m.depth_camera) : nullptr;
  const Affine b2w = load_pose(body_poses + 16 * m.body);
  const Affine b2c = mul_pose(load_pose(cam.world2camera), b2w);
  Affine b2dc = b2c;
  if (dcam) b2dc = mul_pose(load_pose(dcam->world2camera), b2w);
  const bool handle_occlusions = m.n_unoccluded_iterations == 0;
  float* misc = lds;
  if (m.shared_counts) {
    region_histogram_update<true>(m, cam, dcam, b2c, b2dc, handle_occlusions, true,
                                  (__attribute__((address_space(1))) unsigned long long*)m.shared_counts, misc);
    return;
  }
  if (counts_in_lds) {
    region_histogram_update(m, cam, dcam, b2c, b2dc, handle_occlusions, true,
                            (__attribute__((address_space(3))) uint32_t*)(lds + M3T_MISC_FLOATS), misc);
  } else {
    region_histogram_update(m, cam, dcam, b2c, b2dc, handle_occlusions, true,
                            (__attribute__((address_space(1))) uint32_t*)m.count_scratch, misc);
  }
}

// (... then ColorHistograms::InitializeHistograms of the shared objects those modalities use: shared_histogram_finish_kernel,
// one workgroup launched on each object's row of the table.)

// Behind the per-body judgement of a judge_bodies call: one lane per structure combines the row's ADD / ADD-S errors
// as RTBEvaluator::CalculatePoseResults does (:935-988), in f32, op by op: per group the members' errors summed left
// to right in listed order and divided by their number, per structure 1 - min(err / threshold, 1) summed over its
// groups and divided by their number; *_curve_zeros: the leading curve entries the reference sets to 0.
__global__ void __launch_bounds__(64)
judge_structures_kernel(const m3t_body_judgement* row, const int* structure_first_group, const int* group_first_index,
                        const int* listed, const float* thresholds, int n_structures, m3t_structure_judgement* out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_structures) return;
  const float threshold = thresholds[s];
  float add_auc = 0.0f, adds_auc = 0.0f;
  const int g0 = structure_first_group[s], g1 = structure_first_group[s + 1];
  for (int g = g0; g < g1; ++g) {
    float add = 0.0f, adds = 0.0f;
    const int i0 = group_first_index[g], i1 = group_first_index[g + 1];
    for (int i = i0; i < i1; ++i) {
      add += row[listed[i]].add_error;
      adds += row[listed[i]].adds_error;
    }
    add /= float(i1 - i0);
    adds /= float(i1 - i0);
    add_auc += 1.0f - fminf(add / threshold, 1.0f);
    adds_auc += 1.0f - fminf(adds / threshold, 1.0f);
  }
  add_auc /= float(g1 - g0);
  adds_auc /= float(g1 - g0);
  const float threshold_step = 1.0f / 100.0f;  // :21-24
  int add_zeros = 0, adds_zeros = 0;
  while (add_zeros < 100 && !(add_auc < threshold_step * (0.5f + float(add_zeros)))) ++add_zeros;
  while (adds_zeros < 100 && !(adds_auc < threshold_step * (0.5f + float(adds_zeros)))) ++adds_zeros;
  m3t_structure_judgement r;
  r.add_auc = add_auc;
  r.adds_auc = adds_auc;
  r.add_curve_zeros = add_zeros;
  r.adds_curve_zeros = adds_zeros;
  out[s] = r;
}

}  // extern "C"
