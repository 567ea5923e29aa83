// m3t_judge.hip -- the evaluators' judgement on the device (m3t_hip_judge_*): RBOTEvaluator::CalculatePoseResults
// (rbot_evaluator.cpp:416-433), YCBEvaluator::CalculatePoseResults (ycb_evaluator.cpp:803-848) and, for a body the
// device finds lost, RBOTEvaluator::ResetBody (:334-342).  Included by m3t_hip_api.hip behind m3t_kernels.hip (same
// translation unit: region_histogram_update and the pose helpers are the ones of the tracking kernels).

#define M3T_JUDGE_THREADS 256
// T: evaluation vertices (float4 targets) per LDS tile of the nearest-vertex search.  16 KB per workgroup: eight
// workgroups of 256 threads (the wave-slot limit of a CU) take 128 KB of its 160 KB.
#define M3T_JUDGE_TILE 1024
// queries per workgroup: 256 (one per thread) while the batch leaves CUs idle, 1024 (four per thread, every target
// read from LDS serves four distances) once the workgroups of one-per-thread would queue up several deep
#define M3T_JUDGE_SPLIT_QUERIES 256
#define M3T_JUDGE_SPLIT_QUERIES_LARGE 1024

struct JudgeBodyDev {        // one listed body
  const float4* vertices;    // evaluation vertices (x, y, z, 0), padded to a multiple of 4 with copies of vertex 0
  int body;                  // body id
  int n_vertices;            // 0: pose errors only
  int first_part, n_parts;   // its workgroups in the launch / its rows of the partial sums
  int target;                // the body a reset writes (m3t_hip_judge_set_reset_target; by default `body`)
};
struct JudgePartDev {
  int index, part;           // listed body, query range [part * Q, (part + 1) * Q)
};

namespace {

// ResetBody's words: the ground truth over the pose, first_iteration of the body's region modalities (threads 0 .. 15
// and 16 ..; the pose has been read by everyone who needs it)
__device__ __forceinline__ void judge_reset_body(float* body_poses, int body, const float* gt, RegionModDev* mods,
                                                 const int* region_ids, int region_begin, int region_end,
                                                 int reset_iteration) {
  const int tid = threadIdx.x;
  if (tid < 16) body_poses[16 * body + tid] = gt[tid];
  for (int r = region_begin + tid - 16; tid >= 16 && r < region_end; r += blockDim.x - 16)
    mods[region_ids[r]].first_iteration = reset_iteration;
}

}  // namespace

extern "C" {

// One workgroup per (listed body, query range).  Part 0 judges the pose (thread 0: the reference's scalar arithmetic,
// op by op) and, for a body in one part, performs the reset; every part sums its share of ADD / ADD-S.
// K: queries per thread.
extern "C++" template <int K>
__device__ __forceinline__ void judge_bodies_body(float* body_poses, const JudgeBodyDev* bodies, const JudgePartDev* parts,
                                                  const float* gt_poses, float thr_t, float thr_r, int reset_iteration,
                                                  RegionModDev* mods, const int* region_ids, const int* region_first,
                                                  int* flags, m3t_body_judgement* row, double* partial) {
  __shared__ __attribute__((aligned(16))) float4 tile[M3T_JUDGE_TILE];
  double* sum_add = reinterpret_cast<double*>(tile);  // the tree of the sums, once the last tile has been searched
  double* sum_adds = sum_add + M3T_JUDGE_THREADS;
  __shared__ float s_pose[16], s_gt[16], s_delta[12];
  __shared__ int s_reset;
  const int tid = threadIdx.x;
  const JudgePartDev wp = parts[blockIdx.x];
  const JudgeBodyDev b = bodies[wp.index];
  if (tid < 16) {
    s_pose[tid] = body_poses[16 * b.body + tid];
    s_gt[tid] = gt_poses[16 * wp.index + tid];
  }
  __syncthreads();
  if (wp.part == 0 && tid == 0) {
    const float* p = s_pose;
    const float* g = s_gt;
    const float dx = p[12] - g[12], dy = p[13] - g[13], dz = p[14] - g[14];
    const float t_err = sqrtf((dx * dx + dy * dy) + dz * dz);
    float d[3];
    for (int j = 0; j < 3; ++j) d[j] = (p[4 * j] * g[4 * j] + p[4 * j + 1] * g[4 * j + 1]) + p[4 * j + 2] * g[4 * j + 2];
    const float tr = (d[0] + d[1]) + d[2];
    const float c = (tr - 1.0f) * 0.5f;
    const float r_err = float(acos(double(c)));
    const bool lost = t_err > thr_t || r_err > thr_r;  // a NaN error is "not lost", as in the reference
    const int reset = (lost && reset_iteration >= 0) ? 1 : 0;
    m3t_body_judgement& out = row[wp.index];
    out.translation_error = t_err;
    out.rotation_error = r_err;
    out.rotation_cosine = c;
    out.tracking_success = lost ? 0.0f : 1.0f;
    if (b.n_vertices == 0) {
      out.add_error = 0.0f;
      out.adds_error = 0.0f;
    }
    out.was_reset = reset;
    out.reserved = 0;
    flags[wp.index] = reset;
    s_reset = reset;
  }
  if (b.n_vertices > 0) {
    // delta = body2world^-1 * gt: rigid inverse [R^T | -R^T t] and the product in f64, rounded to f32
    if (tid < 12) {
      const int r = tid % 3, c = tid / 3;
      const double i0 = double(s_pose[4 * r]), i1 = double(s_pose[4 * r + 1]), i2 = double(s_pose[4 * r + 2]);
      const double i3 = -((i0 * double(s_pose[12]) + i1 * double(s_pose[13])) + i2 * double(s_pose[14]));
      const double v = ((i0 * double(s_gt[4 * c]) + i1 * double(s_gt[4 * c + 1])) + i2 * double(s_gt[4 * c + 2])) +
                       i3 * double(s_gt[4 * c + 3]);
      s_delta[tid] = float(v);  // [c * 3 + r]
    }
    __syncthreads();
    const int n = b.n_vertices;
    const int n_padded = (n + 3) & ~3;
    const int q0 = wp.part * (K * M3T_JUDGE_THREADS);
    float qx[K], qy[K], qz[K], best[K];
    double add = 0.0, adds = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int q = q0 + k * M3T_JUDGE_THREADS + tid;
      const float4 v = b.vertices[q < n ? q : 0];
      qx[k] = ((s_delta[0] * v.x + s_delta[3] * v.y) + s_delta[6] * v.z) + s_delta[9];
      qy[k] = ((s_delta[1] * v.x + s_delta[4] * v.y) + s_delta[7] * v.z) + s_delta[10];
      qz[k] = ((s_delta[2] * v.x + s_delta[5] * v.y) + s_delta[8] * v.z) + s_delta[11];
      best[k] = 3.402823466e38f;
      const float ex = v.x - qx[k], ey = v.y - qy[k], ez = v.z - qz[k];
      if (q < n) add += double(sqrtf((ex * ex + ey * ey) + ez * ez));
    }
    for (int t0 = 0; t0 < n_padded; t0 += M3T_JUDGE_TILE) {
      const int m = min(M3T_JUDGE_TILE, n_padded - t0);  // a multiple of 4
      __syncthreads();
      for (int i = tid; i < m; i += M3T_JUDGE_THREADS) tile[i] = b.vertices[t0 + i];
      __syncthreads();
      for (int i = 0; i < m; i += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 t = tile[i + u];  // the same address in every lane
          asm volatile("" ::"v"(t.w));   // (w counts as read: one ds_read_b128, not the narrower ds_read_b96)
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const float ex = t.x - qx[k], ey = t.y - qy[k], ez = t.z - qz[k];
            best[k] = fminf(best[k], (ex * ex + ey * ey) + ez * ez);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (q0 + k * M3T_JUDGE_THREADS + tid < n) adds += double(sqrtf(best[k]));
    // fixed order: per thread over its strided vertices (above), then this tree
    __syncthreads();
    sum_add[tid] = add;
    sum_adds[tid] = adds;
    __syncthreads();
    for (int s = M3T_JUDGE_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) {
        sum_add[tid] += sum_add[tid + s];
        sum_adds[tid] += sum_adds[tid + s];
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (b.n_parts == 1) {
        row[wp.index].add_error = float(sum_add[0] / double(n));
        row[wp.index].adds_error = float(sum_adds[0] / double(n));
      } else {
        partial[2 * (b.first_part + wp.part)] = sum_add[0];
        partial[2 * (b.first_part + wp.part) + 1] = sum_adds[0];
      }
    }
  } else {
    __syncthreads();
  }
  // a body in one part: its workgroup is the only reader of the pose (a split body: judge_finish_kernel); a reset
  // target other than the body is no listed body of the judge: nobody in this launch reads its pose
  if (b.n_parts == 1 && s_reset)
    judge_reset_body(body_poses, b.target, s_gt, mods, region_ids, region_first[wp.index], region_first[wp.index + 1],
                     reset_iteration);
}

__global__ void __launch_bounds__(M3T_JUDGE_THREADS)
judge_bodies_kernel(float* body_poses, const JudgeBodyDev* bodies, const JudgePartDev* parts, const float* gt_poses,
                    float thr_t, float thr_r, int reset_iteration, RegionModDev* mods, const int* region_ids,
                    const int* region_first, int* flags, m3t_body_judgement* row, double* partial) {
  judge_bodies_body<1>(body_poses, bodies, parts, gt_poses, thr_t, thr_r, reset_iteration, mods, region_ids,
                       region_first, flags, row, partial);
}
__global__ void __launch_bounds__(M3T_JUDGE_THREADS)
judge_bodies_x4_kernel(float* body_poses, const JudgeBodyDev* bodies, const JudgePartDev* parts, const float* gt_poses,
                       float thr_t, float thr_r, int reset_iteration, RegionModDev* mods, const int* region_ids,
                       const int* region_first, int* flags, m3t_body_judgement* row, double* partial) {
  judge_bodies_body<4>(body_poses, bodies, parts, gt_poses, thr_t, thr_r, reset_iteration, mods, region_ids,
                       region_first, flags, row, partial);
}

// Behind judge_bodies_kernel when a body is split over workgroups: one workgroup per listed body adds the partial sums
// in range order and performs the reset of a split body (every reader of its pose has finished).
__global__ void __launch_bounds__(64)
judge_finish_kernel(float* body_poses, const JudgeBodyDev* bodies, const float* gt_poses, int reset_iteration,
                    RegionModDev* mods, const int* region_ids, const int* region_first, const int* flags,
                    m3t_body_judgement* row, const double* partial) {
  const JudgeBodyDev b = bodies[blockIdx.x];
  if (b.n_parts == 1) return;
  if (threadIdx.x == 0) {
    double add = 0.0, adds = 0.0;
    for (int p = 0; p < b.n_parts; ++p) {
      add += partial[2 * (b.first_part + p)];
      adds += partial[2 * (b.first_part + p) + 1];
    }
    row[blockIdx.x].add_error = float(add / double(b.n_vertices));
    row[blockIdx.x].adds_error = float(adds / double(b.n_vertices));
  }
  if (flags[blockIdx.x])
    judge_reset_body(body_poses, b.target, gt_poses + 16 * blockIdx.x, mods, region_ids, region_first[blockIdx.x],
                     region_first[blockIdx.x + 1], reset_iteration);
}

// Behind the judge when the call may reset: StartModality (:375-388) of the region modalities of the listed bodies,
// one workgroup each -- region_histogram_list_kernel's body for the bodies the judge flagged, nothing for the others.
__global__ void __launch_bounds__(M3T_BLOCK_THREADS)
region_histogram_flagged_kernel(const RegionModDev* mods, const int* region_ids, const int* region_body_index,
                                const int* flags, const CameraDev* cams, const float* body_poses, int counts_in_lds) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (flags[region_body_index[blockIdx.x]] == 0) return;
  CRegion& m = *(CRegion*)(mods + region_ids[blockIdx.x]);
  CCam& cam = *(CCam*)(cams + m.camera);
  CCam* dcam = m.measure_occlusions ? (CCam*)(cams + m.depth_camera) : nullptr;
  const Affine b2w = load_pose(body_poses + 16 * m.body);
  const Affine b2c = mul_pose(load_pose(cam.world2camera), b2w);
  Affine b2dc = b2c;
  if (dcam) b2dc = mul_pose(load_pose(dcam->world2camera), b2w);
  const bool handle_occlusions = m.n_unoccluded_iterations == 0;
  float* misc = lds;
  if (counts_in_lds) {
    region_histogram_update(m, cam, dcam, b2c, b2dc, handle_occlusions, true,
                            (__attribute__((address_space(3))) uint32_t*)(lds + M3T_MISC_FLOATS), misc);
  } else {
    region_histogram_update(m, cam, dcam, b2c, b2dc, handle_occlusions, true,
                            (__attribute__((address_space(1))) uint32_t*)m.count_scratch, misc);
  }
}

}  // extern "C"
