// m3t_texture_tiled.hip -- the brute-force 2-nearest-neighbour Hamming match of TextureModality (texture_modality.cpp:
// 349-377) in the tiled form of m3t_texture_l2.hip: texture_match_tiled_kernel finds the best two train descriptors of
// every keyframe descriptor on a (modality, ring slot x query tile) grid, texture_collect_kernel applies the ratio test,
// compacts the survivors in keyframe-then-query order and projects the data points (:380-385).  Distance, best-two rule,
// the join of two ranges and the ratio test: m3t_texture.h; the grids: m3t_texture_plan.h.  texture_match_kernel
// (m3t_texture.hip) is the same computation in one workgroup per modality; both give the same bits.  Included by
// m3t_hip_api.hip behind every other kernel of the library, so that no existing kernel moves in the code object.

typedef const __attribute__((address_space(4))) uint32_t* TextureUniformWords;

constexpr int kTiledWaves = M3T_TEXTURE_MATCH_THREADS / kWave;
constexpr int kTiledQueryTiles = M3T_TEXTURE_MAX_FEATURES / M3T_TEXTURE_QUERY_TILE;  // per ring slot
static_assert(M3T_TEXTURE_QUERY_TILE == kWave, "a lane per query descriptor");

// The best two of the tile's queries (a lane each, its W dwords in registers) over this wave's range of the train
// descriptors, joined over the waves in range order and written to the scratch.  The train rows are wave-uniform: the
// row index is the same in every lane and the rows are read through the constant address space, so a row arrives in
// scalar registers by scalar loads and costs no LDS traffic, no staging pass and no fence within the wave (the feature
// block is written by earlier launches only).
template <int W>
__device__ __forceinline__ void texture_match_tile(CTexture& m, GW<uint32_t> found, int slot, int q0, int n_query,
                                                   m3t_tex_best2 (*s_best)[M3T_TEXTURE_QUERY_TILE]) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  TextureUniformWords features = (TextureUniformWords)m.features;
  const int n_train = (int)features[0];
  TextureUniformWords train = features + TF_HEADER_WORDS + 2 * M3T_TEXTURE_MAX_FEATURES;
  constexpr int Q = W / 4;  // 16-byte pieces of a descriptor
  const int nq = n_query - q0 < M3T_TEXTURE_QUERY_TILE ? n_query - q0 : M3T_TEXTURE_QUERY_TILE;
  const int q = q0 + (lane < nq ? lane : 0);  // (lanes past nq carry the tile's first query; nothing of theirs is written out)
  G<v4u> query = (G<v4u>)(as_global(m.keyframe_descriptors) + ((size_t)slot * M3T_TEXTURE_MAX_FEATURES + q) * W);
  v4u mine[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) mine[k] = query[k];
  const int range = (n_train + kTiledWaves - 1) / kTiledWaves;
  const int t_begin = wave * range < n_train ? wave * range : n_train;
  const int t_end = t_begin + range < n_train ? t_begin + range : n_train;
  m3t_tex_best2 best;
  m3t_tex_best2_init(&best);
#pragma unroll 4
  for (int t = t_begin; t < t_end; ++t) {
    TextureUniformWords row = train + (size_t)t * W;
    int distance = 0;
#pragma unroll
    for (int k = 0; k < Q; ++k)
      distance += __popc(mine[k].x ^ row[4 * k]) + __popc(mine[k].y ^ row[4 * k + 1]) + __popc(mine[k].z ^ row[4 * k + 2]) +
                  __popc(mine[k].w ^ row[4 * k + 3]);
    m3t_tex_best2_update(&best, distance, t);
  }
  if (wave > 0) s_best[wave - 1][lane] = best;
  __syncthreads();
  if (wave == 0 && lane < nq) {
    for (int w = 0; w < kTiledWaves - 1; ++w) {
      const m3t_tex_best2 later = s_best[w][lane];
      m3t_tex_best2_append(&best, &later);
    }
    GW<uint32_t> out = found + ((size_t)slot * M3T_TEXTURE_MAX_FEATURES + q0 + lane) * 3;
    out[0] = (uint32_t)best.d0;
    out[1] = (uint32_t)best.d1;
    out[2] = (uint32_t)best.i0;
  }
}

extern "C" {

// blockIdx.x: the Hamming modality (mods holds those alone); blockIdx.y: ring slot * kTiledQueryTiles + query tile.
// best[blockIdx.x]: the modality's scratch, [n_keyframes_max][4096][3] = {d0, d1, i0} of every keyframe descriptor.
// What there is to do is read from the modality's state on the device: the grid is sized for the most there can be.
__global__ void __launch_bounds__(M3T_TEXTURE_MATCH_THREADS)
texture_match_tiled_kernel(const TextureModDev* mods, uint32_t* const* best) {
  __shared__ m3t_tex_best2 s_best[kTiledWaves - 1][M3T_TEXTURE_QUERY_TILE];
  CTexture& m = *(CTexture*)(mods + blockIdx.x);
  const int slot = (int)blockIdx.y / kTiledQueryTiles, q0 = ((int)blockIdx.y % kTiledQueryTiles) * M3T_TEXTURE_QUERY_TILE;
  if (slot >= m.n_keyframes_max) return;  // block-uniform, as is the next
  const TextureStateDev* st = m.state;
  const int n_query = st->counts[slot];
  const int position = (slot - st->head + m.n_keyframes_max) % m.n_keyframes_max;
  if (position >= st->n_keyframes || q0 >= n_query) return;  // a slot that holds no keyframe, a tile beyond its count
  GW<uint32_t> found = as_global_w(best[blockIdx.x]);
  if (m.descriptor_words == 8)
    texture_match_tile<8>(m, found, slot, q0, n_query, s_best);
  else
    texture_match_tile<16>(m, found, slot, q0, n_query, s_best);
}

// CalculateCorrespondences :324-387 behind texture_match_tiled_kernel, one workgroup per Hamming modality: the tail of
// texture_match_kernel.  match = 1 (corr_iteration == 0): the ratio test on what the match kernel left and the data
// points, keyframe after keyframe and query after query with a running count (texture_stable_rank: no atomic decides an
// order); then, at every corr_iteration, the projection :380-385.
__global__ void __launch_bounds__(M3T_TEXTURE_MATCH_THREADS)
texture_collect_kernel(const TextureModDev* mods, uint32_t* const* best, const CameraDev* cams, const float* body_poses,
                       int match) {
  __shared__ int s_wave_counts[M3T_TEXTURE_MATCH_THREADS / kWave];
  CTexture& m = *(CTexture*)(mods + blockIdx.x);
  CCam& cam = *(CCam*)(cams + m.camera);
  TextureStateDev* st = m.state;
  const int tid = threadIdx.x;
  int n_points = st->n_data_points;
  GW<float> points = as_global_w(m.data_points);
  if (match) {
    G<uint32_t> features = as_global(m.features);
    G<float> xy = (G<float>)(features + TF_HEADER_WORDS);
    const int n_train = (int)features[0];
    const int head = st->head, held = st->n_keyframes;
    G<uint32_t> all_found = as_global((const uint32_t*)best[blockIdx.x]);
    n_points = 0;
    for (int k = 0; k < held; ++k) {
      const int slot = (head + k) % m.n_keyframes_max;
      const int n_query = st->counts[slot];
      if (n_query == 0 || n_train == 0) continue;  // :351
      G<uint32_t> found = all_found + (size_t)slot * M3T_TEXTURE_MAX_FEATURES * 3;
      G<float> body = as_global(m.keyframe_points) + (size_t)slot * M3T_TEXTURE_MAX_FEATURES * 3;
      for (int base = 0; base < n_query; base += M3T_TEXTURE_MATCH_THREADS) {
        const int q = base + tid;
        const bool have = q < n_query;
        m3t_tex_best2 b;
        m3t_tex_best2_init(&b);
        if (have) {
          b.d0 = (int)found[3 * q];
          b.d1 = (int)found[3 * q + 1];
          b.i0 = (int)found[3 * q + 2];
        }
        const bool keep = have && m3t_tex_ratio_keeps(&b, m.descriptor_distance_threshold);
        int total;
        const int rank = texture_stable_rank(keep, s_wave_counts, &total);
        if (keep) {
          GW<float> p = points + (size_t)(n_points + rank) * TP_FLOATS;
          p[TP_BODY] = body[3 * q];
          p[TP_BODY + 1] = body[3 * q + 1];
          p[TP_BODY + 2] = body[3 * q + 2];
          p[TP_CORRESPONDENCE] = xy[2 * b.i0];
          p[TP_CORRESPONDENCE + 1] = xy[2 * b.i0 + 1];
        }
        n_points += total;
      }
    }
    __syncthreads();  // every thread has read the old count; the points are written
    if (tid == 0) st->n_data_points = n_points;
  }
  const Affine b2c = mul_pose(load_pose(cam.world2camera), load_pose(body_poses + 16 * m.body));
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

}  // extern "C"
