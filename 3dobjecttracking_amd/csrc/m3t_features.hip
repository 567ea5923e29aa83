// m3t_features.hip -- the built-in feature detector of TextureModality: what DetectAndComputeCorrKeypoints
// (M3T/src/texture_modality.cpp:858-888) asks of OpenCV, as a detector of the project's own (m3t_features.h;
// tests/feature_reference.py is its definition).  Three kernels on the context's stream, no host read between them:
//   texture_focus_kernel     (detector, row band)  region of interest from the device pose, grey + bilinear sample
//   texture_fast_kernel      (detector, row band)  FAST-9 score, 3 x 3 suppression, 5 x 5 box sums
//   texture_describe_kernel  (detector)            the n best corners in raster order, direction, descriptor, keypoints
// Included by m3t_hip_api.hip behind m3t_texture.hip (same translation unit).

typedef const __attribute__((address_space(4))) TextureDetectorDev CDetector;

__constant__ int16_t k_feature_cos[M3T_FEATURE_DIRECTIONS] = {M3T_FEATURE_COS_VALUES};
__constant__ int16_t k_feature_sin[M3T_FEATURE_DIRECTIONS] = {M3T_FEATURE_SIN_VALUES};
__constant__ int8_t k_feature_pattern[M3T_BRIEF_TESTS * 4] = {M3T_BRIEF_PATTERN_VALUES};

constexpr int kFeatureThreads = 256;           // focus and FAST kernels
constexpr int kDescribeThreads = 1024;         // one workgroup per detector
constexpr int kFastRows = M3T_FEATURE_BAND + 2 * M3T_FEATURE_FAST_HALO;  // image rows of a band in LDS
constexpr int kScoreRows = M3T_FEATURE_BAND + 2;                         // score rows of a band in LDS

extern "C" {

__global__ void __launch_bounds__(kFeatureThreads)
texture_focus_kernel(const TextureDetectorDev* detectors, const TextureModDev* mods, const CameraDev* cams,
                     const float* body_poses) {
  CDetector& d = *(CDetector*)(detectors + blockIdx.x);
  CTexture& m = *(CTexture*)(mods + d.modality);
  CCam& cam = *(CCam*)(cams + m.camera);
  const int tid = threadIdx.x;
  const Affine b2c = mul_pose(load_pose(cam.world2camera), load_pose(body_poses + 16 * m.body));
  int roi[4] = {0, 0, 0, 0};
  float scale = 0.0f;
  bool valid = m3t_tex_region_of_interest(b2c.t, d.radius, cam.fu, cam.fv, cam.ppu, cam.ppv, cam.width, cam.height,
                                          d.focused_image_size, roi, &scale);
  int fw = 0, fh = 0;
  if (valid) {
    fw = m3t_feat_focused_side(roi[2], scale);
    fh = m3t_feat_focused_side(roi[3], scale);
    if (fw > M3T_TEXTURE_FOCUSED_MAX || fh > M3T_TEXTURE_FOCUSED_MAX) valid = false;
  }
  if (blockIdx.y == 0 && tid == 0) {
    GW<int> h = as_global_w(d.header);
    h[DH_VALID] = valid ? 1 : 0;
    h[DH_WIDTH] = valid ? fw : 0;
    h[DH_HEIGHT] = valid ? fh : 0;
    h[DH_ROI] = roi[0];
    h[DH_ROI + 1] = roi[1];
    h[DH_ROI + 2] = roi[2];
    h[DH_ROI + 3] = roi[3];
    h[DH_SCALE] = __float_as_int(scale);
    if (!valid) {  // no features for this frame
      h[DH_N] = 0;
      as_global_w(d.features)[0] = 0u;
    }
  }
  if (!valid) return;
  const int y_begin = (int)blockIdx.y * M3T_FEATURE_BAND;
  const int y_end = y_begin + M3T_FEATURE_BAND < fh ? y_begin + M3T_FEATURE_BAND : fh;
  G<uint8_t> image = as_global(cam.image);
  GW<uint8_t> out = as_global_w(d.focused);
  for (int y = y_begin; y < y_end; ++y) {
    int y0, y1, wy;
    m3t_feat_sample_axis(y, scale, roi[3], &y0, &y1, &wy);
    G<uint8_t> row0 = image + (size_t)(roi[1] + y0) * cam.pitch + (size_t)roi[0] * 3;
    G<uint8_t> row1 = image + (size_t)(roi[1] + y1) * cam.pitch + (size_t)roi[0] * 3;
    for (int x = tid; x < fw; x += kFeatureThreads) {
      int x0, x1, wx;
      m3t_feat_sample_axis(x, scale, roi[2], &x0, &x1, &wx);
      const int g00 = m3t_feat_grey(row0[3 * x0], row0[3 * x0 + 1], row0[3 * x0 + 2]);
      const int g01 = m3t_feat_grey(row0[3 * x1], row0[3 * x1 + 1], row0[3 * x1 + 2]);
      const int g10 = m3t_feat_grey(row1[3 * x0], row1[3 * x0 + 1], row1[3 * x0 + 2]);
      const int g11 = m3t_feat_grey(row1[3 * x1], row1[3 * x1 + 1], row1[3 * x1 + 2]);
      out[(size_t)y * fw + x] = (uint8_t)m3t_feat_bilinear(g00, g01, g10, g11, wx, wy);
    }
  }
}

// A band of M3T_FEATURE_BAND rows with a halo of 4 (3 for the circle, 1 for the suppression) in LDS: 24 rows of 512
// bytes, and the scores of the band with a halo of 1: 18 rows of 512 u16 -- 30 KB.
__global__ void __launch_bounds__(kFeatureThreads)
texture_fast_kernel(const TextureDetectorDev* detectors) {
  __shared__ uint8_t s_image[kFastRows * M3T_TEXTURE_FOCUSED_MAX];
  __shared__ uint16_t s_score[kScoreRows * M3T_TEXTURE_FOCUSED_MAX];
  CDetector& d = *(CDetector*)(detectors + blockIdx.x);
  G<int> h = as_global((const int*)d.header);
  const int fw = h[DH_WIDTH], fh = h[DH_HEIGHT];
  const int y_begin = (int)blockIdx.y * M3T_FEATURE_BAND;
  if (!h[DH_VALID] || y_begin >= fh) return;
  const int tid = threadIdx.x;
  const int threshold = d.fast_threshold;
  constexpr int P = M3T_TEXTURE_FOCUSED_MAX;
  G<uint8_t> image = as_global((const uint8_t*)d.focused);
  for (int r = 0; r < kFastRows; ++r) {
    const int y = y_begin - M3T_FEATURE_FAST_HALO + r;
    const bool inside = y >= 0 && y < fh;
    for (int x = tid; x < fw; x += kFeatureThreads) s_image[r * P + x] = inside ? image[(size_t)y * fw + x] : (uint8_t)0;
  }
  __syncthreads();
  const int8_t circle[32] = {M3T_FEATURE_CIRCLE_VALUES};
  for (int r = 0; r < kScoreRows; ++r) {
    const int y = y_begin - 1 + r;
    const bool row_ok = y >= M3T_FEATURE_BORDER && y < fh - M3T_FEATURE_BORDER;
    const uint8_t* center = s_image + (r + M3T_FEATURE_FAST_HALO - 1) * P;
    for (int x = tid; x < fw; x += kFeatureThreads) {
      int score = 0;
      if (row_ok && x >= M3T_FEATURE_BORDER && x < fw - M3T_FEATURE_BORDER) {
        const int p = center[x];
        if (m3t_feat_compass_may_be_corner(p, center[x - 3 * P], center[x + 3], center[x + 3 * P], center[x - 3], threshold)) {
          int c[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) c[i] = center[x + circle[2 * i] + circle[2 * i + 1] * P];
          score = m3t_feat_fast_score(p, c, threshold);
        }
      }
      s_score[r * P + x] = (uint16_t)score;
    }
  }
  __syncthreads();
  GW<uint16_t> scores = as_global_w(d.scores);
  GW<uint16_t> boxes = as_global_w(d.boxes);
  const int y_end = y_begin + M3T_FEATURE_BAND < fh ? y_begin + M3T_FEATURE_BAND : fh;
  for (int y = y_begin; y < y_end; ++y) {
    const uint16_t* row = s_score + (y - y_begin + 1) * P;
    const uint8_t* center = s_image + (y - y_begin + M3T_FEATURE_FAST_HALO) * P;
    const bool box_row = y >= M3T_FEATURE_BOX_RADIUS && y < fh - M3T_FEATURE_BOX_RADIUS;
    for (int x = tid; x < fw; x += kFeatureThreads) {
      int s = row[x];
      if (s > 0) {  // (a corner is at least M3T_FEATURE_BORDER from the edges: its eight neighbours exist)
        const bool greatest = s > row[x - 1] && s > row[x + 1] && s > row[x - P - 1] && s > row[x - P] &&
                              s > row[x - P + 1] && s > row[x + P - 1] && s > row[x + P] && s > row[x + P + 1];
        if (!greatest) s = 0;
      }
      scores[(size_t)y * fw + x] = (uint16_t)s;
      int box = 0;
      if (box_row && x >= M3T_FEATURE_BOX_RADIUS && x < fw - M3T_FEATURE_BOX_RADIUS) {
#pragma unroll
        for (int dy = -M3T_FEATURE_BOX_RADIUS; dy <= M3T_FEATURE_BOX_RADIUS; ++dy)
#pragma unroll
          for (int dx = -M3T_FEATURE_BOX_RADIUS; dx <= M3T_FEATURE_BOX_RADIUS; ++dx) box += center[x + dy * P + dx];
      }
      boxes[(size_t)y * fw + x] = (uint16_t)box;
    }
  }
}

// Selection (score descending, raster index ascending; output in raster order), direction and descriptor.  LDS: the
// score histogram (4096 words), the kept corners' raster indices (4096 words) and a few words per wave: 33 KB.
// Every wave owns a contiguous piece of the raster, so the raster order of the output is a ballot within the wave and a
// prefix over the waves' counts; no atomic decides an order (the histogram's atomics only count).
__global__ void __launch_bounds__(kDescribeThreads)
texture_describe_kernel(const TextureDetectorDev* detectors) {
  constexpr int kWaves = kDescribeThreads / kWave;
  __shared__ int s_hist[M3T_FEATURE_SCORE_BINS];
  __shared__ int s_kept[M3T_TEXTURE_MAX_FEATURES];
  __shared__ int s_above[kWaves], s_at[kWaves];
  __shared__ int s_cut, s_quota;
  CDetector& d = *(CDetector*)(detectors + blockIdx.x);
  G<int> h = as_global((const int*)d.header);
  if (!h[DH_VALID]) return;  // (the focus kernel has set n = 0)
  const int fw = h[DH_WIDTH], fh = h[DH_HEIGHT];
  const int n_pixels = fw * fh;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int n_features = d.n_features;
  G<uint16_t> scores = as_global((const uint16_t*)d.scores);
  for (int i = tid; i < M3T_FEATURE_SCORE_BINS; i += kDescribeThreads) s_hist[i] = 0;
  __syncthreads();
#pragma unroll 8
  for (int i = tid; i < n_pixels; i += kDescribeThreads) {
    const int s = scores[i];
    if (s > 0) atomicAdd(&s_hist[s], 1);
  }
  __syncthreads();
  // the cut: the score c with fewer than n_features corners above it and at least n_features at or above it; 0 when
  // there are no more corners than n_features (then all are kept).  Lane l of wave 0 owns the 64 bins below 4096 - 64 l.
  if (wave == 0) {
    const int top = M3T_FEATURE_SCORE_BINS - 1 - kWave * lane;
    int mine = 0;
    for (int k = 0; k < kWave; ++k) mine += s_hist[top - k];
    int inclusive = mine;
#pragma unroll
    for (int step = 1; step < kWave; step <<= 1) {
      const int other = __shfl_up(inclusive, step);
      if (lane >= step) inclusive += other;
    }
    const int total = __shfl(inclusive, kWave - 1);
    if (lane == 0 && total <= n_features) {
      s_cut = 0;
      s_quota = 0;
    }
    if (total > n_features && inclusive >= n_features && inclusive - mine < n_features) {  // one lane
      int above = inclusive - mine, cut = top;
      for (int k = 0; k < kWave; ++k) {
        const int c = s_hist[top - k];
        if (above + c >= n_features) {
          cut = top - k;
          break;
        }
        above += c;
      }
      s_cut = cut;
      s_quota = n_features - above;
    }
  }
  __syncthreads();
  const int cut = s_cut, quota = s_quota;
  // the piece of the raster of this wave, a multiple of 64 pixels
  const int piece = ((n_pixels + kWaves - 1) / kWaves + kWave - 1) / kWave * kWave;
  const int begin = wave * piece;
  const int end = begin + piece < n_pixels ? begin + piece : n_pixels;
  // (kBatch chunks of 64 pixels per trip: their loads are in flight together, the ballots follow in raster order)
  constexpr int kBatch = 4;
  int n_above = 0, n_at = 0;
  for (int base = begin; base < end; base += kBatch * kWave) {
    int s[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int i = base + j * kWave + lane;
      s[j] = i < end ? (int)scores[i] : 0;
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      n_above += __popcll(__ballot(s[j] > cut));
      n_at += __popcll(__ballot(cut > 0 && s[j] == cut));
    }
  }
  if (lane == 0) {
    s_above[wave] = n_above;
    s_at[wave] = n_at;
  }
  __syncthreads();
  int at_before = 0, out_before = 0, n_out = 0;
  {
    int at_seen = 0;
    for (int w = 0; w < kWaves; ++w) {
      int kept_at = quota - at_seen;
      kept_at = kept_at < 0 ? 0 : (kept_at < s_at[w] ? kept_at : s_at[w]);
      if (w == wave) {
        at_before = at_seen;
        out_before = n_out;
      }
      n_out += s_above[w] + kept_at;
      at_seen += s_at[w];
    }
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int base = begin; base < end; base += kBatch * kWave) {
    int s[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int i = base + j * kWave + lane;
      s[j] = i < end ? (int)scores[i] : 0;
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const bool at = cut > 0 && s[j] == cut;
      const unsigned long long at_mask = __ballot(at);
      const bool keep = s[j] > cut || (at && at_before + __popcll(at_mask & below) < quota);
      const unsigned long long keep_mask = __ballot(keep);
      if (keep) {
        const int slot = out_before + __popcll(keep_mask & below);
        if (slot < M3T_TEXTURE_MAX_FEATURES) s_kept[slot] = base + j * kWave + lane;
      }
      at_before += __popcll(at_mask);
      out_before += __popcll(keep_mask);
    }
  }
  __syncthreads();
  if (n_out > M3T_TEXTURE_MAX_FEATURES) n_out = M3T_TEXTURE_MAX_FEATURES;  // (n_features <= 4096: cannot happen)
  // direction and descriptor: a keypoint per 16-lane row
  const int row = tid >> 4, sub = tid & 15;
  const float scale = __int_as_float(h[DH_SCALE]);
  const float roi_x = (float)h[DH_ROI], roi_y = (float)h[DH_ROI + 1];
  G<uint8_t> image = as_global((const uint8_t*)d.focused);
  G<uint16_t> boxes = as_global((const uint16_t*)d.boxes);
  GW<uint32_t> features = as_global_w(d.features);
  GW<float> xy = (GW<float>)(features + TF_HEADER_WORDS);
  GW<uint16_t> descriptors = (GW<uint16_t>)(features + TF_HEADER_WORDS + 2 * M3T_TEXTURE_MAX_FEATURES);
  for (int k = row; k < n_out; k += kDescribeThreads / 16) {
    const int index = s_kept[k];
    const int y = index / fw, x = index - y * fw;
    // the disc row by row: lane `sub` takes the columns sub - 15 and sub + 1 (-15 .. 16; 16 lies outside the disc but
    // inside the image, a corner being 16 from the edges), loads first, the disc test on the loaded values
    int m10 = 0, m01 = 0;
    const int dx0 = sub - M3T_FEATURE_MOMENT_RADIUS, dx1 = sub + 1;
    G<uint8_t> centre = image + (size_t)y * fw + x;
#pragma unroll 8
    for (int dy = -M3T_FEATURE_MOMENT_RADIUS; dy <= M3T_FEATURE_MOMENT_RADIUS; ++dy) {
      const int rest = M3T_FEATURE_MOMENT_RADIUS * M3T_FEATURE_MOMENT_RADIUS - dy * dy;
      const int v0 = centre[dy * fw + dx0], v1 = centre[dy * fw + dx1];
      const int w0 = dx0 * dx0 <= rest ? v0 : 0, w1 = dx1 * dx1 <= rest ? v1 : 0;
      m10 += dx0 * w0 + dx1 * w1;
      m01 += dy * (w0 + w1);
    }
#pragma unroll
    for (int step = 8; step >= 1; step >>= 1) {
      m10 += __shfl_xor(m10, step, 16);
      m01 += __shfl_xor(m01, step, 16);
    }
    const int bin = m3t_feat_direction_bin(m10, m01, k_feature_cos, k_feature_sin);
    const int c = k_feature_cos[bin], s = k_feature_sin[bin];
    uint32_t bits = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int8_t* t = k_feature_pattern + (sub * 16 + j) * 4;
      int ax, ay, bx, by;
      m3t_feat_rotate(t[0], t[1], c, s, &ax, &ay);
      m3t_feat_rotate(t[2], t[3], c, s, &bx, &by);
      const int a = boxes[(size_t)(y + ay) * fw + (x + ax)], b = boxes[(size_t)(y + by) * fw + (x + bx)];
      bits |= (a < b ? 1u : 0u) << j;
    }
    descriptors[(size_t)k * 16 + sub] = (uint16_t)bits;  // 32 bytes per keypoint, test 8 i + j in bit j of byte i
    if (sub == 0) {
      xy[2 * k] = roi_x + (float)x / scale;
      xy[2 * k + 1] = roi_y + (float)y / scale;
    }
  }
  if (tid == 0) {
    features[0] = (uint32_t)n_out;
    as_global_w(d.header)[DH_N] = n_out;
  }
}

}  // extern "C"
