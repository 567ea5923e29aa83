// m3t_opt.hip -- the OPT evaluator's two costs on the device: OPTEvaluator::CalculateDiameters
// (examples/opt_evaluator.cpp:580-600, m3t_hip_vertices_diameter) and OPTEvaluator::CalculatePoseResults (:462-488,
// the ADD-only bodies of a judge, m3t_hip_judge_set_add_only).  Included by m3t_hip_api.hip behind m3t_judge.hip (same
// translation unit: JudgePartDev, judge_reset_body and the constants of the judge).

// ---- ADD-only bodies of a judge ---------------------------------------------------------------------------------------
// vertices per workgroup (four per thread, the four float4 loads in flight together).  1024: the 2^18 vertices of the
// largest body judge_set_vertices takes become 256 workgroups, one per CU of the chip, and their 256 partial sums are
// still a short serial chain for the finish launch; a body of the evaluators' usual 1 000 reduced vertices stays in one
// workgroup, which writes its row itself (no finish launch, no partial sums).
#define M3T_JUDGE_ADD_SPLIT 1024
#define M3T_JUDGE_ADD_PER_THREAD (M3T_JUDGE_ADD_SPLIT / M3T_JUDGE_THREADS)
static_assert(M3T_JUDGE_ADD_SPLIT % M3T_JUDGE_THREADS == 0, "whole vertices per thread");

struct JudgeAddBodyDev {     // one ADD-only body
  const float4* vertices;    // the judge's evaluation vertices of the body (JudgeBodyDev::vertices)
  int index;                 // listed body: its row entry, ground truth, flag and regions
  int body;                  // body id
  int n_vertices;            // 0: pose errors only
  int first_part, n_parts;   // its workgroups in the launch / its partial sums
  int target;                // the body a reset writes (JudgeBodyDev::target)
  float geometry2body[12];   // column-major 3 x 4: [c * 3 + r]
};

// ---- diameter ---------------------------------------------------------------------------------------------------------
#define M3T_DIAMETER_THREADS 256
// row vertices per thread, in registers (two packed pairs)
#define M3T_DIAMETER_ROWS 4
// T: column vertices (float4) per LDS tile = row vertices per workgroup.  16 KB per workgroup, as the judge's tile.
#define M3T_DIAMETER_TILE 1024
static_assert(M3T_DIAMETER_TILE == M3T_DIAMETER_THREADS * M3T_DIAMETER_ROWS, "one tile of rows per workgroup");
// rows of tiles per launch: a call over 1 << 20 vertices (1024 rows of tiles) is four launches, none of which holds the
// device for longer than a 2^18-vertex call's few times over
#define M3T_DIAMETER_ROW_TILES_PER_LAUNCH 256

typedef float m3t_float2 __attribute__((ext_vector_type(2)));

extern "C" {

// One workgroup per (ADD-only body, range of M3T_JUDGE_ADD_SPLIT vertices).  Part 0 judges the pose (thread 0: the
// scalar arithmetic of judge_bodies_kernel, op by op) and, for a body in one part, writes add_error and performs the
// reset; a split body leaves its partial sums to judge_add_only_finish_kernel.  No nearest-vertex search, no tile.
__global__ void __launch_bounds__(M3T_JUDGE_THREADS)
judge_add_only_kernel(float* body_poses, const JudgeAddBodyDev* bodies, const JudgePartDev* parts, const float* gt_poses,
                      float thr_t, float thr_r, int reset_iteration, RegionModDev* mods, const int* region_ids,
                      const int* region_first, int* flags, m3t_body_judgement* row, double* partial) {
  __shared__ double sum_add[M3T_JUDGE_THREADS];
  __shared__ double s_a[12];
  __shared__ float s_pose[16], s_gt[16], s_delta[12], s_g[12];
  __shared__ int s_reset;
  const int tid = threadIdx.x;
  const JudgePartDev wp = parts[blockIdx.x];
  const JudgeAddBodyDev& b = bodies[wp.index];
  const int index = b.index, n = b.n_vertices, n_parts = b.n_parts;
  if (tid < 16) {
    s_pose[tid] = body_poses[16 * b.body + tid];
    s_gt[tid] = gt_poses[16 * index + tid];
  }
  if (tid >= 32 && tid < 44) s_g[tid - 32] = b.geometry2body[tid - 32];
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
    m3t_body_judgement& out = row[index];
    out.translation_error = t_err;
    out.rotation_error = r_err;
    out.rotation_cosine = c;
    out.tracking_success = lost ? 0.0f : 1.0f;
    if (n == 0) out.add_error = 0.0f;
    out.adds_error = 0.0f;  // never searched
    out.was_reset = reset;
    out.reserved = 0;
    flags[index] = reset;
    s_reset = reset;
  }
  if (n > 0) {
    // delta = (body2world * geometry2body)^-1 * gt * geometry2body in f64, left to right, rounded to f32 once.
    // a = body2world * geometry2body (bottom rows (0, 0, 0, 1) implied)
    if (tid < 12) {
      const int r = tid % 3, c = tid / 3;
      double v = (double(s_pose[r]) * double(s_g[3 * c]) + double(s_pose[4 + r]) * double(s_g[3 * c + 1])) +
                 double(s_pose[8 + r]) * double(s_g[3 * c + 2]);
      if (c == 3) v += double(s_pose[12 + r]);
      s_a[tid] = v;  // [c * 3 + r]
    }
    __syncthreads();
    if (tid < 12) {
      const int r = tid % 3, c = tid / 3;
      // row r of a^-1 = [R^T | -R^T t], then times gt as judge_bodies_kernel multiplies (its bottom row as stored)
      const double i0 = s_a[3 * r], i1 = s_a[3 * r + 1], i2 = s_a[3 * r + 2];
      const double i3 = -((i0 * s_a[9] + i1 * s_a[10]) + i2 * s_a[11]);
      double m[4];
      for (int k = 0; k < 4; ++k)
        m[k] = ((i0 * double(s_gt[4 * k]) + i1 * double(s_gt[4 * k + 1])) + i2 * double(s_gt[4 * k + 2])) +
               i3 * double(s_gt[4 * k + 3]);
      double v = (m[0] * double(s_g[3 * c]) + m[1] * double(s_g[3 * c + 1])) + m[2] * double(s_g[3 * c + 2]);
      if (c == 3) v += m[3];
      s_delta[tid] = float(v);  // [c * 3 + r]
    }
    __syncthreads();
    const int q0 = wp.part * M3T_JUDGE_ADD_SPLIT;
    float4 v[M3T_JUDGE_ADD_PER_THREAD];
#pragma unroll
    for (int k = 0; k < M3T_JUDGE_ADD_PER_THREAD; ++k) {
      const int q = q0 + k * M3T_JUDGE_THREADS + tid;
      v[k] = b.vertices[q < n ? q : 0];
    }
    double add = 0.0;
#pragma unroll
    for (int k = 0; k < M3T_JUDGE_ADD_PER_THREAD; ++k) {
      const float qx = ((s_delta[0] * v[k].x + s_delta[3] * v[k].y) + s_delta[6] * v[k].z) + s_delta[9];
      const float qy = ((s_delta[1] * v[k].x + s_delta[4] * v[k].y) + s_delta[7] * v[k].z) + s_delta[10];
      const float qz = ((s_delta[2] * v[k].x + s_delta[5] * v[k].y) + s_delta[8] * v[k].z) + s_delta[11];
      const float ex = v[k].x - qx, ey = v[k].y - qy, ez = v[k].z - qz;
      if (q0 + k * M3T_JUDGE_THREADS + tid < n) add += double(sqrtf((ex * ex + ey * ey) + ez * ez));
    }
    // fixed order: per thread over its strided vertices (above), then this tree, then the parts in range order
    sum_add[tid] = add;
    __syncthreads();
    for (int s = M3T_JUDGE_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) sum_add[tid] += sum_add[tid + s];
      __syncthreads();
    }
    if (tid == 0) {
      if (n_parts == 1) {
        row[index].add_error = float(sum_add[0] / double(n));
      } else {
        partial[b.first_part + wp.part] = sum_add[0];
      }
    }
  } else {
    __syncthreads();
  }
  // a body in one part: its workgroup is the only reader of the pose (a split body: judge_add_only_finish_kernel)
  if (n_parts == 1 && s_reset)
    judge_reset_body(body_poses, b.target, s_gt, mods, region_ids, region_first[index], region_first[index + 1],
                     reset_iteration);
}

// judge_finish_kernel's twin behind judge_add_only_kernel when an ADD-only body is split: one workgroup per ADD-only
// body adds its partial sums in range order and performs its reset (every reader of its pose has finished).
__global__ void __launch_bounds__(64)
judge_add_only_finish_kernel(float* body_poses, const JudgeAddBodyDev* bodies, const float* gt_poses, int reset_iteration,
                             RegionModDev* mods, const int* region_ids, const int* region_first, const int* flags,
                             m3t_body_judgement* row, const double* partial) {
  const JudgeAddBodyDev& b = bodies[blockIdx.x];
  if (b.n_parts == 1) return;
  const int index = b.index;
  if (threadIdx.x == 0) {
    double add = 0.0;
    for (int p = 0; p < b.n_parts; ++p) add += partial[b.first_part + p];
    row[index].add_error = float(add / double(b.n_vertices));
  }
  if (flags[index])
    judge_reset_body(body_poses, b.target, gt_poses + 16 * index, mods, region_ids, region_first[index],
                     region_first[index + 1], reset_iteration);
}

// The maximum of d2 = (dx*dx + dy*dy) + dz*dz over the pairs of two tiles of vertices: workgroup (x, y) takes the row
// tile first_row_tile + y and the column tile x, and only tile pairs on or above the diagonal work (d2 is symmetric).
// `vertices` is padded to a multiple of the tile with copies of vertex 0, so every pair it forms is a pair of the set.
// Four rows per thread as two packed pairs (v_pk_add_f32 / v_pk_mul_f32 round as their scalar forms do), the columns
// through LDS at the same address in every lane.  The running maximum may merge rows: a maximum is exact in any order.
// Non-negative floats order like their bit patterns, so the workgroups combine with an integer atomic maximum.
__global__ void __launch_bounds__(M3T_DIAMETER_THREADS)
vertices_diameter_kernel(const float4* vertices, int first_row_tile, unsigned int* max_bits) {
  __shared__ __attribute__((aligned(16))) float4 tile[M3T_DIAMETER_TILE];
  __shared__ float s_wave[M3T_DIAMETER_THREADS / 64];
  const int row_tile = first_row_tile + int(blockIdx.y), col_tile = int(blockIdx.x);
  if (col_tile < row_tile) return;
  const int tid = threadIdx.x;
  const float4* rows = vertices + size_t(row_tile) * M3T_DIAMETER_TILE;
  const float4* cols = vertices + size_t(col_tile) * M3T_DIAMETER_TILE;
  m3t_float2 x[M3T_DIAMETER_ROWS / 2], y[M3T_DIAMETER_ROWS / 2], z[M3T_DIAMETER_ROWS / 2];
#pragma unroll
  for (int k = 0; k < M3T_DIAMETER_ROWS / 2; ++k) {
    const float4 a = rows[(2 * k) * M3T_DIAMETER_THREADS + tid], b = rows[(2 * k + 1) * M3T_DIAMETER_THREADS + tid];
    x[k] = m3t_float2{a.x, b.x};
    y[k] = m3t_float2{a.y, b.y};
    z[k] = m3t_float2{a.z, b.z};
  }
  for (int i = tid; i < M3T_DIAMETER_TILE; i += M3T_DIAMETER_THREADS) tile[i] = cols[i];
  __syncthreads();
  float best = 0.0f;
  for (int i = 0; i < M3T_DIAMETER_TILE; i += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4 t = tile[i + u];  // the same address in every lane
      asm volatile("" ::"v"(t.w));   // (w counts as read: one ds_read_b128, not the narrower ds_read_b96)
      const m3t_float2 tx = {t.x, t.x}, ty = {t.y, t.y}, tz = {t.z, t.z};
#pragma unroll
      for (int k = 0; k < M3T_DIAMETER_ROWS / 2; ++k) {
        const m3t_float2 dx = x[k] - tx, dy = y[k] - ty, dz = z[k] - tz;
        const m3t_float2 d2 = (dx * dx + dy * dy) + dz * dz;
        best = fmaxf(fmaxf(best, d2.x), d2.y);
      }
    }
  }
  for (int s = 32; s > 0; s >>= 1) best = fmaxf(best, __shfl_xor(best, s, 64));
  if ((tid & 63) == 0) s_wave[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < M3T_DIAMETER_THREADS / 64; ++w) best = fmaxf(best, s_wave[w]);
    atomicMax(max_bits, __float_as_uint(best));
  }
}

}  // extern "C"
