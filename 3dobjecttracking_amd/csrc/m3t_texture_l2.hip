// m3t_texture_l2.hip -- the brute-force 2-nearest-neighbour match of TextureModality (texture_modality.cpp:349-377) for
// L2-norm descriptors (SIFT, DAISY: cv::BFMatcher(cv::NORM_L2), :794-796), in the tiled form: texture_match_l2_kernel
// finds the best two train descriptors of every keyframe descriptor on a (modality, ring slot x query tile) grid,
// texture_collect_l2_kernel applies the ratio test, compacts the survivors in keyframe-then-query order and projects
// the data points (:380-385).  Distance, best-two rule and ratio test: m3t_texture.h.  Included by m3t_hip_api.hip behind
// every other kernel of the library, so that no existing kernel moves in the code object.

typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4f* LdsV4f;

constexpr int kL2QueryPitch = M3T_TEXTURE_L2_QUERY_TILE + 1;  // 16-byte pieces: the transposing writes spread over the banks
constexpr int kL2Waves = M3T_TEXTURE_MATCH_THREADS / kWave;
constexpr int kL2QueryTiles = M3T_TEXTURE_MAX_FEATURES / M3T_TEXTURE_L2_QUERY_TILE;  // per ring slot
static_assert(M3T_TEXTURE_L2_QUERY_TILE == kWave, "a lane per query descriptor");
static_assert(M3T_TEXTURE_L2_TRAIN_TILE == kL2Waves * M3T_TEXTURE_L2_ROWS, "every wave carries its own rows of a tile");

// dynamic LDS of texture_match_l2_kernel for descriptors of n_floats: the query tile, transposed, and the train rows
__host__ __device__ constexpr size_t texture_l2_lds_bytes(int n_floats) {
  return size_t(n_floats / 4) * (kL2QueryPitch + M3T_TEXTURE_L2_TRAIN_TILE) * 16;
}

// A wave's LDS accesses reach LDS in program order, so the lanes of one wave see each other's writes without a
// barrier; what is needed is that the compiler keeps the accesses on their side of this point.
__device__ __forceinline__ void texture_l2_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

extern "C" {

// blockIdx.x: the L2 modality; blockIdx.y: ring slot * kL2QueryTiles + query tile.  A lane owns one keyframe descriptor
// (its floats in LDS, [piece][query], so that a wave reads a piece of all its queries in one conflict-free pass).  The
// train descriptors are split into four contiguous ranges of ascending index, one per wave; a wave passes its range
// through LDS M3T_TEXTURE_L2_ROWS rows at a time and every lane carries that many sums, each one the sequential chain
// of m3t_tex_l2_squared (the rows are wave-uniform: every lane reads the same address, a broadcast).  The waves' best
// two are joined in range order, which is ascending train index.
__global__ void __launch_bounds__(M3T_TEXTURE_MATCH_THREADS)
texture_match_l2_kernel(const TextureL2Dev* l2, const TextureModDev* mods) {
  extern __shared__ __attribute__((aligned(16))) float lds_l2[];
  __shared__ m3t_tex_best2f s_best[kL2Waves - 1][M3T_TEXTURE_L2_QUERY_TILE];
  const TextureL2Dev& l = l2[blockIdx.x];
  CTexture& m = *(CTexture*)(mods + l.modality);
  const int slot = (int)blockIdx.y / kL2QueryTiles, q0 = ((int)blockIdx.y % kL2QueryTiles) * M3T_TEXTURE_L2_QUERY_TILE;
  if (slot >= m.n_keyframes_max) return;  // block-uniform, as is the next
  const TextureStateDev* st = m.state;
  const int n_query = st->counts[slot];
  const int position = (slot - st->head + m.n_keyframes_max) % m.n_keyframes_max;
  if (position >= st->n_keyframes || q0 >= n_query) return;  // a slot that holds no keyframe, a tile beyond its count
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int pieces = m.descriptor_words / 4;  // 16-byte pieces of a descriptor
  G<uint32_t> features = as_global(m.features);
  const int n_train = (int)features[0];
  G<v4f> train = (G<v4f>)(features + TF_HEADER_WORDS + 2 * M3T_TEXTURE_MAX_FEATURES);
  G<v4f> query = (G<v4f>)(as_global(m.keyframe_descriptors) + ((size_t)slot * M3T_TEXTURE_MAX_FEATURES + q0) * m.descriptor_words);
  LdsV4f s_query = (LdsV4f)lds_l2;
  LdsV4f s_rows = s_query + pieces * kL2QueryPitch + wave * M3T_TEXTURE_L2_ROWS * pieces;
  const int nq = n_query - q0 < M3T_TEXTURE_L2_QUERY_TILE ? n_query - q0 : M3T_TEXTURE_L2_QUERY_TILE;
  for (int i = tid; i < nq * pieces; i += M3T_TEXTURE_MATCH_THREADS) s_query[(i % pieces) * kL2QueryPitch + i / pieces] = query[i];
  // (lanes past nq run on what LDS holds; nothing of theirs is written out)
  __syncthreads();  // the query tile, which every wave reads; the train rows below are each wave's own
  const int range = (((n_train + kL2Waves - 1) / kL2Waves) + M3T_TEXTURE_L2_ROWS - 1) / M3T_TEXTURE_L2_ROWS * M3T_TEXTURE_L2_ROWS;
  m3t_tex_best2s best;
  m3t_tex_best2s_init(&best);
  for (int offset = 0; offset < range; offset += M3T_TEXTURE_L2_ROWS) {
    const int t0 = wave * range + offset;
    int nt = n_train - t0;
    nt = nt < 0 ? 0 : nt > M3T_TEXTURE_L2_ROWS ? M3T_TEXTURE_L2_ROWS : nt;
    texture_l2_wave_sync();  // the previous rows have been read
    for (int i = lane; i < nt * pieces; i += kWave) s_rows[i] = train[(size_t)t0 * pieces + i];
    texture_l2_wave_sync();  // the rows are written
    float s[M3T_TEXTURE_L2_ROWS];
#pragma unroll
    for (int r = 0; r < M3T_TEXTURE_L2_ROWS; ++r) s[r] = 0.0f;
    for (int k = 0; k < pieces; ++k) {
      const v4f mine = s_query[k * kL2QueryPitch + lane];
#pragma unroll
      for (int r = 0; r < M3T_TEXTURE_L2_ROWS; ++r) {  // (rows past nt: stale LDS, never looked at)
        const v4f other = s_rows[r * pieces + k];
        const float e0 = mine.x - other.x, e1 = mine.y - other.y, e2 = mine.z - other.z, e3 = mine.w - other.w;
        s[r] = s[r] + e0 * e0;
        s[r] = s[r] + e1 * e1;
        s[r] = s[r] + e2 * e2;
        s[r] = s[r] + e3 * e3;
      }
    }
#pragma unroll
    for (int r = 0; r < M3T_TEXTURE_L2_ROWS; ++r)
      if (r < nt) m3t_tex_best2s_update(&best, s[r], t0 + r);
  }
  if (wave > 0) s_best[wave - 1][lane] = best.b;
  __syncthreads();
  if (wave == 0 && lane < nq) {
    for (int w = 0; w < kL2Waves - 1; ++w) {
      const m3t_tex_best2f later = s_best[w][lane];
      m3t_tex_best2f_append(&best.b, &later);
    }
    GW<uint32_t> out = as_global_w(l.best) + ((size_t)slot * M3T_TEXTURE_MAX_FEATURES + q0 + lane) * 3;
    out[0] = __float_as_uint(best.b.d0);
    out[1] = __float_as_uint(best.b.d1);
    out[2] = (uint32_t)best.b.i0;
  }
}

// CalculateCorrespondences :324-387 behind texture_match_l2_kernel, one workgroup per L2 modality.  match = 1
// (corr_iteration == 0): the ratio test on what the match kernel left and the data points, keyframe after keyframe and
// query after query with a running count (texture_stable_rank: no atomic decides an order); then, at every
// corr_iteration, the projection :380-385.
__global__ void __launch_bounds__(M3T_TEXTURE_MATCH_THREADS)
texture_collect_l2_kernel(const TextureL2Dev* l2, const TextureModDev* mods, const CameraDev* cams, const float* body_poses,
                          int match) {
  __shared__ int s_wave_counts[M3T_TEXTURE_MATCH_THREADS / kWave];
  const TextureL2Dev& l = l2[blockIdx.x];
  CTexture& m = *(CTexture*)(mods + l.modality);
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
    n_points = 0;
    for (int k = 0; k < held; ++k) {
      const int slot = (head + k) % m.n_keyframes_max;
      const int n_query = st->counts[slot];
      if (n_query == 0 || n_train == 0) continue;  // :351
      G<uint32_t> found = as_global(l.best) + (size_t)slot * M3T_TEXTURE_MAX_FEATURES * 3;
      G<float> body = as_global(m.keyframe_points) + (size_t)slot * M3T_TEXTURE_MAX_FEATURES * 3;
      for (int base = 0; base < n_query; base += M3T_TEXTURE_MATCH_THREADS) {
        const int q = base + tid;
        const bool have = q < n_query;
        m3t_tex_best2f best;
        m3t_tex_best2f_init(&best);
        if (have) {
          best.d0 = __uint_as_float(found[3 * q]);
          best.d1 = __uint_as_float(found[3 * q + 1]);
          best.i0 = (int)found[3 * q + 2];
        }
        const bool keep = have && m3t_tex_ratio_keeps_l2(&best, m.descriptor_distance_threshold);
        int total;
        const int rank = texture_stable_rank(keep, s_wave_counts, &total);
        if (keep) {
          GW<float> p = points + (size_t)(n_points + rank) * TP_FLOATS;
          p[TP_BODY] = body[3 * q];
          p[TP_BODY + 1] = body[3 * q + 1];
          p[TP_BODY + 2] = body[3 * q + 2];
          p[TP_CORRESPONDENCE] = xy[2 * best.i0];
          p[TP_CORRESPONDENCE + 1] = xy[2 * best.i0 + 1];
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
