// m3t_texture.hip -- TextureModality (M3T/src/texture_modality.cpp) behind the feature detector: keyframe
// reconstruction with the two occlusion tests (:933-1127), the brute-force 2-nearest-neighbour Hamming match with the
// ratio test (:349-377), the projection of the data points (:380-385), the Tukey-weighted g/H (:397-444) and the keyframe
// renewal rule (:456-472).  Included by m3t_hip_api.hip behind m3t_kernels.hip (same translation unit: the pose math,
// the renderer reads, occlusion_window_clear and the g/H chains).  One workgroup per texture modality in every kernel.

// The file is included twice by m3t_hip_api.hip: the second time, with M3T_TEXTURE_LIST_KERNELS defined, it yields
// texture_keyframe_list_kernel alone (at its end) -- behind every other kernel of the library, so that no existing kernel
// moves in the code object.
#ifndef M3T_TEXTURE_LIST_KERNELS

typedef const __attribute__((address_space(4))) TextureModDev CTexture;
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4u* LdsTile;

// exclusive prefix of `keep` over the workgroup's threads in thread order, and the workgroup's total: a wave ballot and
// a prefix over the waves' counts (no atomic decides an order).  wave_counts: one word per wave; two barriers.
__device__ __forceinline__ int texture_stable_rank(bool keep, int* wave_counts, int* total) {
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave, n_waves = (int)blockDim.x / kWave;
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) wave_counts[wave] = __popcll(mask);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < n_waves; ++w) {
    const int c = wave_counts[w];
    before += w < wave ? c : 0;
    all += c;
  }
  __syncthreads();  // wave_counts may be written again
  *total = all;
  return before + __popcll(mask & ((1ull << lane) - 1ull));
}

// orientation of ComputeKeyframeData :988-990 / CalculateResults :460-462: rotation().inverse() * normalized(translation),
// rotation() taken as linear() (the view direction of the region and depth modalities, with Eigen's normalized() for t = 0)
__device__ __forceinline__ void texture_orientation(const Affine& b2c, float o[3]) {
  if (!view_direction(b2c, o[0], o[1], o[2])) o[0] = o[1] = o[2] = 0.0f;
}

extern "C" {

// ComputeKeyframeData :933-992 for every texture modality.  decide = 0: StartModality (:315-322).  decide = 1:
// CalculateResults (:456-472) -- the age is counted and the renewal decided here, behind a block-uniform test.
// (The body lives in m3t_texture_keyframe.inc: the list kernel below includes the same text behind its test, and this
// kernel compiles to what it always was.)
__global__ void __launch_bounds__(M3T_TEXTURE_MATCH_THREADS)
texture_keyframe_kernel(const TextureModDev* mods, const CameraDev* cams, const float* body_poses, int decide) {
  const unsigned modality_index = blockIdx.x;
#include "m3t_texture_keyframe.inc"
}

}  // extern "C"

// The match of one keyframe against the current features: every thread owns one query descriptor (W dwords in
// registers), the train descriptors pass through LDS in tiles of ascending index (every lane reads the same address: a
// broadcast, 16 bytes at a time), the best two are kept with a strict `<`, so the lower train index ranks first among
// equal distances.  Survivors of the ratio test are appended in query order.
template <int W>
__device__ __forceinline__ int texture_match_keyframe(CTexture& m, int slot, int n_query, int n_train, int first,
                                                      LdsTile tile, int* wave_counts) {
  const int tid = threadIdx.x;
  G<uint32_t> features = as_global(m.features);
  G<float> xy = (G<float>)(features + TF_HEADER_WORDS);
  G<v4u> train = (G<v4u>)(features + TF_HEADER_WORDS + 2 * M3T_TEXTURE_MAX_FEATURES);
  G<v4u> query = (G<v4u>)(as_global(m.keyframe_descriptors) + (size_t)slot * M3T_TEXTURE_MAX_FEATURES * W);
  G<float> points = as_global(m.keyframe_points) + (size_t)slot * M3T_TEXTURE_MAX_FEATURES * 3;
  GW<float> out = as_global_w(m.data_points);
  constexpr int Q = W / 4;  // 16-byte pieces of a descriptor
  int n_out = first;
  for (int base = 0; base < n_query; base += M3T_TEXTURE_MATCH_THREADS) {
    const int q = base + tid;
    const bool have = q < n_query;
    v4u mine[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) mine[k] = query[(size_t)(have ? q : 0) * Q + k];
    m3t_tex_best2 best;
    m3t_tex_best2_init(&best);
    for (int t0 = 0; t0 < n_train; t0 += M3T_TEXTURE_TRAIN_TILE) {
      const int nt = n_train - t0 < M3T_TEXTURE_TRAIN_TILE ? n_train - t0 : M3T_TEXTURE_TRAIN_TILE;
      __syncthreads();  // the previous tile has been read
      for (int k = tid; k < nt * Q; k += M3T_TEXTURE_MATCH_THREADS) tile[k] = train[(size_t)t0 * Q + k];
      __syncthreads();
      for (int t = 0; t < nt; ++t) {
        int distance = 0;
#pragma unroll
        for (int k = 0; k < Q; ++k) {
          const v4u other = tile[t * Q + k];
          distance += __popc(mine[k].x ^ other.x) + __popc(mine[k].y ^ other.y) + __popc(mine[k].z ^ other.z) +
                      __popc(mine[k].w ^ other.w);
        }
        m3t_tex_best2_update(&best, distance, t0 + t);
      }
    }
    const bool keep = have && m3t_tex_ratio_keeps(&best, m.descriptor_distance_threshold);
    int total;
    const int rank = texture_stable_rank(keep, wave_counts, &total);
    if (keep) {
      GW<float> p = out + (size_t)(n_out + rank) * TP_FLOATS;
      p[TP_BODY] = points[3 * q];
      p[TP_BODY + 1] = points[3 * q + 1];
      p[TP_BODY + 2] = points[3 * q + 2];
      p[TP_CORRESPONDENCE] = xy[2 * best.i0];
      p[TP_CORRESPONDENCE + 1] = xy[2 * best.i0 + 1];
    }
    n_out += total;
  }
  return n_out;
}

extern "C" {

// CalculateCorrespondences :324-387.  match = 1 (corr_iteration == 0): the data points are rebuilt from the keyframes in
// order, with a running count, so their order is the reference's; then, at every corr_iteration, the projection :380-385.
__global__ void __launch_bounds__(M3T_TEXTURE_MATCH_THREADS)
texture_match_kernel(const TextureModDev* mods, const CameraDev* cams, const float* body_poses, int match) {
  __shared__ v4u s_tile[M3T_TEXTURE_TRAIN_TILE * M3T_TEXTURE_MAX_DESCRIPTOR_WORDS / 4];
  __shared__ int s_wave_counts[M3T_TEXTURE_MATCH_THREADS / kWave];
  CTexture& m = *(CTexture*)(mods + blockIdx.x);
  CCam& cam = *(CCam*)(cams + m.camera);
  TextureStateDev* st = m.state;
  const int tid = threadIdx.x;
  int n_points = st->n_data_points;
  if (match) {
    const int n_train = (int)as_global(m.features)[0];
    const int head = st->head, held = st->n_keyframes;
    n_points = 0;
    for (int k = 0; k < held; ++k) {
      const int slot = (head + k) % m.n_keyframes_max;
      const int n_query = st->counts[slot];
      if (n_query == 0 || n_train == 0) continue;  // :351
      n_points = m.descriptor_words == 8
                     ? texture_match_keyframe<8>(m, slot, n_query, n_train, n_points, (LdsTile)s_tile, s_wave_counts)
                     : texture_match_keyframe<16>(m, slot, n_query, n_train, n_points, (LdsTile)s_tile, s_wave_counts);
    }
    __syncthreads();  // every thread has read the old count
    if (tid == 0) st->n_data_points = n_points;
  }
  const Affine b2c = mul_pose(load_pose(cam.world2camera), load_pose(body_poses + 16 * m.body));
  GW<float> points = as_global_w(m.data_points);
  for (int i = tid; i < n_points; i += M3T_TEXTURE_MATCH_THREADS) {
    GW<float> p = points + (size_t)i * TP_FLOATS;
    float x, y, z;
    apply_pose(b2c, p[TP_BODY], p[TP_BODY + 1], p[TP_BODY + 2], x, y, z);
    p[TP_CAMERA] = x;
    p[TP_CAMERA + 1] = y;
    p[TP_CAMERA + 2] = z;
    p[TP_CENTER] = x * cam.fu / z + cam.ppu;
    p[TP_CENTER + 1] = y * cam.fv / z + cam.ppv;
  }
}

// CalculateGradientAndHessian :397-444: a thread per data point forms its 27 products (m3t_texture.h) into rows in LDS,
// M3T_TEXTURE_GH_CHUNK points at a time; the first 42 lanes carry the sequential f32 sums of the reference over the
// chunks with the chain walk of the region and depth modalities.
__global__ void __launch_bounds__(M3T_TEXTURE_MATCH_THREADS)
texture_gradient_hessian_kernel(const TextureModDev* mods, const CameraDev* cams, const float* body_poses,
                                int corr_iteration) {
  constexpr int kPitch = M3T_TEXTURE_GH_CHUNK + 4;
  static_assert(M3T_TEXTURE_GH_CHUNK % kChainBlock == 0 && ((kPitch / 4) & 1) == 1, "chain_slots / chain_pitch of a chunk");
  __shared__ __attribute__((aligned(16))) float rows[27 * kPitch];
  CTexture& m = *(CTexture*)(mods + blockIdx.x);
  CCam& cam = *(CCam*)(cams + m.camera);
  const int tid = threadIdx.x;
  const int n_points = m.state->n_data_points;
  const Affine b2c = mul_pose(load_pose(cam.world2camera), load_pose(body_poses + 16 * m.body));
  const float standard_deviation = last_valid(m.standard_deviations, m.n_standard_deviations, corr_iteration);
  const float variance = standard_deviation * standard_deviation;  // powf(sd, 2.0f) :855
  const float tukey_norm_constant = m.tukey_norm_constant;
  GW<float> points = as_global_w(m.data_points);
  float sum = 0.0f;
  for (int base = 0; base < n_points; base += M3T_TEXTURE_GH_CHUNK) {
    const int count = n_points - base < M3T_TEXTURE_GH_CHUNK ? n_points - base : M3T_TEXTURE_GH_CHUNK;
    const int slots = chain_slots(count);
    for (int i = tid; i < slots; i += M3T_TEXTURE_MATCH_THREADS) {
      float out[27];
      if (i < count) {
        GW<float> p = points + (size_t)(base + i) * TP_FLOATS;
        const float cb[3] = {p[TP_BODY], p[TP_BODY + 1], p[TP_BODY + 2]};
        const float corr[2] = {p[TP_CORRESPONDENCE], p[TP_CORRESPONDENCE + 1]};
        float x, y, z;
        apply_pose(b2c, cb[0], cb[1], cb[2], x, y, z);
        const float cu = x * cam.fu / z + cam.ppu, cv = y * cam.fv / z + cam.ppv;
        p[TP_CAMERA] = x;
        p[TP_CAMERA + 1] = y;
        p[TP_CAMERA + 2] = z;
        p[TP_CENTER] = cu;
        p[TP_CENTER + 1] = cv;
        m3t_tex_point_products(b2c.l, cam.fu, cam.fv, x, y, z, cu, cv, corr, cb, tukey_norm_constant, variance, out);
      } else {
#pragma unroll
        for (int k = 0; k < 27; ++k) out[k] = 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 27; ++k) rows[k * kPitch + i] = out[k];
    }
    __syncthreads();
    if (tid < 42) sum = chain_walk<6>((LdsV4)(rows + gh_lane_row(tid) * kPitch), slots / 4, sum);
    __syncthreads();
  }
  if (tid < 42) m.gradient_hessian[tid] = sum;
}

}  // extern "C"

#else  // M3T_TEXTURE_LIST_KERNELS

// Item `item` of an enqueued call's texture items ({detector, texture modality, flag index or -1}, three ints each) is
// skipped iff the call has flags and the item's flag is 0 (m3t_features.hip, "StartModality ... an enqueued call lists")
__device__ __forceinline__ bool texture_item_skipped(const int* items, const int* flags, int item) {
  return flags != nullptr && !flags[items[3 * item + 2]];
}

extern "C" {

// StartModality (:315-322, decide = 0) of the texture modalities an enqueued call lists, behind their renderers and
// their detection: the item is blockIdx.x, skipped as in the list kernels of m3t_features.hip.
__global__ void __launch_bounds__(M3T_TEXTURE_MATCH_THREADS)
texture_keyframe_list_kernel(const TextureModDev* mods, const CameraDev* cams, const float* body_poses, const int* items,
                             const int* flags) {
  if (texture_item_skipped(items, flags, (int)blockIdx.x)) return;  // block-uniform
  const int modality_index = items[3 * blockIdx.x + 1];
  constexpr int decide = 0;
#include "m3t_texture_keyframe.inc"
}

}  // extern "C"

#endif  // M3T_TEXTURE_LIST_KERNELS
