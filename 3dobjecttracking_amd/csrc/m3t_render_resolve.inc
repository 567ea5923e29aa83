// m3t_render_resolve.inc -- the body of focused_resolve_kernel and focused_resolve_flagged_kernel (m3t_render.hip),
// included into both: renderers and which (pairs {renderer, twin or -1}) are the kernel's parameters, the pair is
// blockIdx.x, the band blockIdx.y.
  extern __shared__ uint32_t lds_z[];  // [band rows * S] packed words, then first_item[threads + 1], wave_total[16]
  // Every survivor's rows inside the band are cut into pieces of kPiece pixels; the pieces of ALL survivors of a trip
  // are numbered through (block-wide prefix sum) and dealt out evenly: a covered pixel costs ~30 f64 operations, and a
  // thread that finished a 100-pixel box by itself kept its whole wave waiting (measured: 54 us per resolve).
  constexpr int kPiece = 8, kPer = 4;  // survivors a thread looks at per trip: one trip up to 2048 survivors
  // grid: (renderer pairs, bands) -- workgroup b runs on XCD b mod 8, so with the pair as the fast index the bands of a
  // pair share an XCD (whenever the number of pairs is a multiple of 8) and its survivor list is fetched into ONE L2:
  // round 5, 128 pairs x 8 bands -- with the band as the fast index each of the eight L2s read all 12 MB of lists
  const RendererDev& r = renderers[which[2 * blockIdx.x]];
  const int twin = which[2 * blockIdx.x + 1];  // a renderer whose rendering is this one (focused_setup_kernel), or -1
  const int S = r.image_size;
  const int n_bands = (int)gridDim.y;
  const int band_rows = (S + n_bands - 1) / n_bands;
  const int row_lo = (int)blockIdx.y * band_rows, row_hi = min(row_lo + band_rows, S) - 1;  // inclusive
  const int n_px = band_rows * S;
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & (kWave - 1), wave = tid / kWave;
  int* first_item = reinterpret_cast<int*>(lds_z + n_px);  // [nt + 1]: pieces before thread t's survivors
  int* wave_total = first_item + nt + 1;                   // [16]
  int* own_count = wave_total + 16;                        // [kPer][nt]: pieces of thread t's j-th survivor
  for (int i = tid; i < n_px; i += nt) lds_z[i] = 0xffffffffu;
  const int n = min(__hip_atomic_load(r.n_survivors, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), r.survivor_capacity);
  const RasterSurvivor* list = static_cast<const RasterSurvivor*>(r.survivors);
  auto sink = [S, row_lo](int px, int py, uint32_t word) { atomicMin(&lds_z[(py - row_lo) * S + px], word); };
  for (int base = 0; base < n && row_lo <= row_hi; base += nt * kPer) {  // block-uniform trip count
    int mine = 0, cnt[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int i = base + j * nt + tid;
      cnt[j] = 0;
      if (i < n) {
        const RasterTriangle& tri = list[i].tri;
        const int ya = max(tri.y0, row_lo), yb = min(tri.y1, row_hi);
        if (ya <= yb) cnt[j] = ((tri.x1 - tri.x0 + kPiece) / kPiece) * (yb - ya + 1);
      }
      mine += cnt[j];
    }
    // inclusive prefix sum over the wave (DPP: row_shr 1 2 4 8, row_bcast 15 / 31), then over the waves
    int incl = mine;
    incl += dpp_zero_i<0x111, 0xf>(incl);
    incl += dpp_zero_i<0x112, 0xf>(incl);
    incl += dpp_zero_i<0x114, 0xf>(incl);
    incl += dpp_zero_i<0x118, 0xf>(incl);
    incl += dpp_zero_i<0x142, 0xa>(incl);
    incl += dpp_zero_i<0x143, 0xc>(incl);
    __syncthreads();  // (the previous trip's pieces are done with the tables; the first time: the cleared z-buffer)
    if (lane == kWave - 1) wave_total[wave] = incl;
#pragma unroll
    for (int j = 0; j < kPer; ++j) own_count[j * nt + tid] = cnt[j];
    __syncthreads();
    int before = 0;
    for (int wv = 0; wv < wave; ++wv) before += wave_total[wv];
    first_item[tid] = before + incl - mine;
    if (tid == nt - 1) first_item[nt] = before + incl;
    __syncthreads();
    const int total = first_item[nt];
    for (int k = tid; k < total; k += nt) {
      int lo = 0, hi = nt - 1;  // the last thread whose first piece is <= k (threads without pieces repeat the value:
      while (lo < hi) {         // the last of equals is the one that owns the piece)
        const int mid = (lo + hi + 1) >> 1;
        if (first_item[mid] <= k) lo = mid; else hi = mid - 1;
      }
      int local = k - first_item[lo], j = 0;
      while (j < kPer - 1 && local >= own_count[j * nt + lo]) { local -= own_count[j * nt + lo]; ++j; }
      const RasterSurvivor& sv = list[base + j * nt + lo];
      const int ya = max(sv.tri.y0, row_lo);
      const int pieces = (sv.tri.x1 - sv.tri.x0 + kPiece) / kPiece;
      const int row = local / pieces, xa = sv.tri.x0 + (local - row * pieces) * kPiece;
      raster_row(sv.tri, ya + row, xa, min(xa + kPiece - 1, sv.tri.x1), sv.low_bits, sink);
    }
  }
  __syncthreads();
  const int n_out = (row_hi - row_lo + 1) * S;
  // four pixels per thread and store where the band allows it (its first pixel and its length multiples of four: the
  // images are DevMem blocks): one 8-byte and one 4-byte store instead of four 2-byte and four 1-byte ones -- the
  // output of 128 pairs cost 10.7 of the launch's 69 us (round 5, probe builds)
  const RendererDev* t = twin >= 0 ? &renderers[twin] : nullptr;  // the same rendering with the twin's id byte: the
  const size_t first = (size_t)row_lo * S;                        // winner's draw order sits in bits 8..15
  auto depth_of = [](uint32_t v) { return v == 0xffffffffu ? (uint32_t)65535 : v >> 16; };
  auto id_of = [](uint32_t v) { return v == 0xffffffffu ? 0u : (v & 0xffu); };
  auto twin_id_of = [t](uint32_t v) { return (v == 0xffffffffu || !t->silhouette) ? 0u : (uint32_t)(uint8_t)t->id[(v >> 8) & 0xffu]; };
  if ((first & 3) == 0 && (n_out & 3) == 0) {
    for (int i = tid * 4; i < n_out; i += nt * 4) {
      const uint32_t v0 = lds_z[i], v1 = lds_z[i + 1], v2 = lds_z[i + 2], v3 = lds_z[i + 3];
      const uint2 d = make_uint2(depth_of(v0) | depth_of(v1) << 16, depth_of(v2) | depth_of(v3) << 16);
      *reinterpret_cast<uint2*>(r.depth_image + first + i) = d;
      *reinterpret_cast<uint32_t*>(r.silhouette_image + first + i) =
          id_of(v0) | id_of(v1) << 8 | id_of(v2) << 16 | id_of(v3) << 24;
      if (t) {
        *reinterpret_cast<uint2*>(t->depth_image + first + i) = d;
        *reinterpret_cast<uint32_t*>(t->silhouette_image + first + i) =
            twin_id_of(v0) | twin_id_of(v1) << 8 | twin_id_of(v2) << 16 | twin_id_of(v3) << 24;
      }
    }
  } else {
    for (int i = tid; i < n_out; i += nt) {
      const uint32_t v = lds_z[i];
      r.depth_image[first + i] = (uint16_t)depth_of(v);
      r.silhouette_image[first + i] = (uint8_t)id_of(v);
      if (t) {
        t->depth_image[first + i] = (uint16_t)depth_of(v);
        t->silhouette_image[first + i] = (uint8_t)twin_id_of(v);
      }
    }
  }
  // every band has read the count by now once it says it is done: the last one clears the list for the next rendering
  if (tid == 0) {
    if (atomicAdd(r.n_survivors + 1, 1) == n_bands - 1) {
      __hip_atomic_store(r.n_survivors, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(r.n_survivors + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
