// m3t_render_setup.inc -- the body of focused_setup_kernel and focused_setup_flagged_kernel (m3t_render.hip), included
// into both: renderers, which (pairs {renderer, twin or -1}), cams and body_poses are the kernel's parameters, the pair
// is blockIdx.y, the slice blockIdx.x.
  const RendererDev& r = renderers[which[2 * blockIdx.y]];
  const int twin = which[2 * blockIdx.y + 1];
  const CameraDev& cam = cams[r.camera];
  const FocusedProjection f = focused_projection(r, cam, body_poses);
  if (threadIdx.x == 0 && blockIdx.x == 0) {  // the crop, for the modalities that read the rendering
    for (int w = 0; w < (twin >= 0 ? 2 : 1); ++w) {
      float* state = w == 0 ? r.state : renderers[twin].state;
      state[RS_CORNER_U] = f.corner_u;
      state[RS_CORNER_V] = f.corner_v;
      state[RS_SCALE] = f.scale;
      state[RS_TERM_A] = r.z_max * r.z_min * 65535.0f / (r.z_max - r.z_min);  // renderer.cpp:567-570
      state[RS_TERM_B] = r.z_max * 65535.0f / (r.z_max - r.z_min);
      state[RS_N_VISIBLE] = (float)f.n_visible;
      for (int k = 0; k < M3T_MAX_RENDERER_BODIES; ++k)
        state[RS_VISIBLE0 + k] = (f.visible_mask >> k & 1u) ? 1.0f : 0.0f;
    }
  }
  if (f.n_visible == 0) return;  // block-uniform
  const int S = r.image_size;
  RasterSurvivor* list = static_cast<RasterSurvivor*>(r.survivors);
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & (kWave - 1);
  for (int order = 0; order < r.n_bodies; ++order) {
    const M44 trans = mul44(f.P, mul44(load44(cam.world2camera),
                                       mul44(load44(body_poses + 16 * r.body[order]), load44(r.geometry2body[order]))));
    const uint32_t low_bits = ((uint32_t)order << 8) | (r.silhouette ? (uint32_t)r.id[order] : 0u);
    const float* vertices = r.vertices[order];
    const int* triangles = r.triangles[order];
    const bool culling = r.culling[order] != 0;
    const int per_slice = (r.n_triangles[order] + gridDim.x - 1) / gridDim.x;
    const int t_begin = blockIdx.x * per_slice;
    const int t_end = min(t_begin + per_slice, r.n_triangles[order]);
    // A slice is tens of trips long at 128 pairs and a trip is two dependent loads (indices, then the vertices they
    // name -- the meshes of 64 objects do not stay in L2) in front of ~400 instructions, at two waves per SIMD: the
    // loads run two trips ahead -- the indices of trip i + 2 and the vertices of trip i + 1 are on their way while
    // trip i is set up (round 5, 128 pairs x 2 slices: 49.5 -> 45 us with the indices alone -> 41.4 us).  Measured
    // and not kept, all with identical images: the body's vertices snapped once into an LDS table and the triangles
    // set up from it (a third of the instructions, 41.9 us: the trips are chains of dependent f64 operations at two
    // waves per SIMD, not instruction issue), two triangles per thread and trip on top of that (41.8), the list
    // append's atomic answered one trip later (57: registers), a 128-VGPR build with two workgroups per CU (46.9)
    int idx1[3] = {0, 0, 0}, idx2[3] = {0, 0, 0};
    float xyz1[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) xyz1[k] = 0.0f;
    auto load_indices = [&](int t, int (&index)[3]) {
      if (t < t_end) {
#pragma unroll
        for (int k = 0; k < 3; ++k) index[k] = triangles[t * 3 + k];
      }
    };
    auto load_vertices = [&](int t, const int (&index)[3], float (&xyz)[9]) {
      if (t < t_end) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float* p = vertices + (size_t)index[k] * 3;
          xyz[3 * k] = p[0]; xyz[3 * k + 1] = p[1]; xyz[3 * k + 2] = p[2];
        }
      }
    };
    load_indices(t_begin + tid, idx1);
    load_indices(t_begin + nt + tid, idx2);
    load_vertices(t_begin + tid, idx1, xyz1);
    for (int base = t_begin; base < t_end; base += nt) {
      const int t = base + tid;
      float xyz[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) xyz[k] = xyz1[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) idx1[k] = idx2[k];
      load_vertices(t + nt, idx1, xyz1);
      load_indices(t + 2 * nt, idx2);
      RasterSurvivor sv;
      const bool ok = t < t_end && raster_setup_vertices(trans, xyz, culling, S, sv.tri);
      // one atomic per wave: the lanes with a survivor take consecutive entries
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(ok);
      if (mask == 0) continue;  // wave-uniform
      int first = 0;
      if (lane == 0) first = atomicAdd(r.n_survivors, __builtin_popcountll(mask));
      first = __builtin_amdgcn_readfirstlane(first);
      if (ok) {
        const int at = first + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (at < r.survivor_capacity) {
          sv.low_bits = low_bits;
          sv.pad = 0;
          list[at] = sv;
        }
      }
    }
  }
