// m3t_features_describe.inc -- the body of texture_describe_kernel and texture_describe_list_kernel (m3t_features.hip),
// included into both: detectors is the kernel's parameter, detector_index names the detector.
  constexpr int kWaves = kDescribeThreads / kWave;
  __shared__ int s_hist[M3T_FEATURE_SCORE_BINS];
  __shared__ int s_kept[M3T_TEXTURE_MAX_FEATURES];
  __shared__ int s_above[kWaves], s_at[kWaves];
  __shared__ int s_cut, s_quota;
  CDetector& d = *(CDetector*)(detectors + detector_index);
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
