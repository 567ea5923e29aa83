// m3t_features_fast.inc -- the body of texture_fast_kernel and texture_fast_list_kernel (m3t_features.hip), included into
// both: detectors is the kernel's parameter, detector_index names the detector, the row band is blockIdx.y.
  __shared__ uint8_t s_image[kFastRows * M3T_TEXTURE_FOCUSED_MAX];
  __shared__ uint16_t s_score[kScoreRows * M3T_TEXTURE_FOCUSED_MAX];
  CDetector& d = *(CDetector*)(detectors + detector_index);
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
