// m3t_texture_keyframe.inc -- the body of texture_keyframe_kernel and texture_keyframe_list_kernel (m3t_texture.hip),
// included into both: mods, cams, body_poses and decide are the kernel's parameters (decide a constant 0 in the list
// kernel), modality_index names the texture modality.
  __shared__ int s_go, s_slot, s_modeled;
  __shared__ int s_wave_counts[M3T_TEXTURE_MATCH_THREADS / kWave];
  CTexture& m = *(CTexture*)(mods + modality_index);
  CCam& cam = *(CCam*)(cams + m.camera);
  TextureStateDev* st = m.state;
  const int tid = threadIdx.x;
  const Affine b2c = mul_pose(load_pose(cam.world2camera), load_pose(body_poses + 16 * m.body));
  if (tid == 0) {
    int go = 1;
    int head = st->head, held = st->n_keyframes;
    if (decide) {
      float o[3];
      texture_orientation(b2c, o);
      const float dot = (o[0] * st->orientation_last_keyframe[0] + o[1] * st->orientation_last_keyframe[1]) +
                        o[2] * st->orientation_last_keyframe[2];
      const float rotation_difference = float(acos(double(dot)));
      const int age = st->keyframe_age + 1;
      st->keyframe_age = age;
      go = (rotation_difference > m.max_keyframe_rotation_difference || age > m.max_keyframe_age) ? 1 : 0;
    }
    if (go) {
      if (held >= m.n_keyframes_max) {  // pop_front
        head = (head + 1) % m.n_keyframes_max;
        held -= 1;
        st->head = head;
        st->n_keyframes = held;
      }
      if (!renderer_body_visible(m.silhouette_renderer, m.silhouette_renderer_slot)) go = 0;  // :945
    }
    s_go = go;
    s_slot = (head + held) % m.n_keyframes_max;
    s_modeled = (m.model_occlusions && renderer_body_visible(m.depth_renderer, m.depth_renderer_slot)) ? 1 : 0;
  }
  __syncthreads();
  if (!s_go) return;
  const int slot = s_slot;
  const bool modeled = s_modeled != 0;
  const Affine c2b = inverse_pose(b2c);
  const RendererDev& sr = *m.silhouette_renderer;
  const FocusedCrop crop = renderer_crop(sr);
  G<uint32_t> features = as_global(m.features);
  const int n = (int)features[0];
  const int words = m.descriptor_words;
  G<float> xy = (G<float>)(features + TF_HEADER_WORDS);
  G<uint32_t> descriptors = features + TF_HEADER_WORDS + 2 * M3T_TEXTURE_MAX_FEATURES;
  GW<float> points = as_global_w(m.keyframe_points) + (size_t)slot * M3T_TEXTURE_MAX_FEATURES * 3;
  GW<uint32_t> kept = as_global_w(m.keyframe_descriptors) + (size_t)slot * M3T_TEXTURE_MAX_FEATURES * words;
  int count = 0;
  for (int base = 0; base < n; base += M3T_TEXTURE_MATCH_THREADS) {
    const int i = base + tid;
    bool keep = false;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (i < n) {
      // Reconstruct3DPoint :994-1023
      const float cx = xy[2 * i], cy = xy[2 * i + 1];
      const int u = f2i((cx - crop.corner_u) * crop.scale + 0.5f);
      const int v = f2i((cy - crop.corner_v) * crop.scale + 0.5f);
      if (u >= 0 && u <= crop.image_size - 1 && v >= 0 && v <= crop.image_size - 1 &&
          (int)as_global(sr.silhouette_image)[(size_t)v * crop.image_size + u] == m.body_id) {
        const unsigned short value = as_global(sr.depth_image)[(size_t)v * crop.image_size + u];
        const float depth = renderer_depth(sr, value);
        apply_pose(c2b, depth * (cx - cam.ppu) / cam.fu, depth * (cy - cam.ppv) / cam.fv, depth, px, py, pz);
        keep = true;
        if (m.measure_occlusions) {  // IsPointUnoccludedMeasured :1035-1081
          CCam& dcam = *(CCam*)(cams + m.depth_camera);
          const Affine b2dc = mul_pose(load_pose(dcam.world2camera), load_pose(body_poses + 16 * m.body));
          float x, y, z;
          apply_pose(b2dc, px, py, pz, x, y, z);
          const float center_u = x * dcam.fu / z + dcam.ppu;
          const float center_v = y * dcam.fv / z + dcam.ppv;
          const float meter_to_pixel = dcam.fu / z;
          const float diameter = 2.0f * m.measured_occlusion_radius * meter_to_pixel;
          // (a negative or NaN diameter -- a point behind the depth camera -- has no window: the reference divides by a
          // stride of zero there; the point is kept)
          if (diameter >= 0.0f)
            keep = occlusion_window_clear(dcam, center_u, center_v, diameter, z, 0.0f, m.measured_occlusion_threshold);
        }
        if (keep && modeled) {  // IsPointUnoccludedModeled :1083-1127
          const RendererDev& dr = *m.depth_renderer;
          float x, y, z;
          apply_pose(b2c, px, py, pz, x, y, z);
          const float meter_to_pixel = (cam.fu / z) * dr.state[RS_SCALE];
          const float diameter = 2.0f * m.modeled_occlusion_radius * meter_to_pixel;
          const float center_u = x * cam.fu / z + cam.ppu;
          const float center_v = y * cam.fv / z + cam.ppv;
          if (diameter >= 0.0f) {
            const unsigned short min_value = modeled_window_min(dr, center_u, center_v, diameter);
            keep = renderer_depth(dr, min_value) > z - m.modeled_occlusion_threshold;
          }
        }
      }
    }
    int total;
    const int rank = texture_stable_rank(keep, s_wave_counts, &total);
    if (keep) {
      const int at = count + rank;
      points[3 * at] = px;
      points[3 * at + 1] = py;
      points[3 * at + 2] = pz;
      for (int w = 0; w < words; ++w) kept[(size_t)at * words + w] = descriptors[(size_t)i * words + w];
    }
    count += total;
  }
  if (tid == 0) {
    float o[3];
    texture_orientation(b2c, o);
    st->counts[slot] = count;
    st->n_keyframes = st->n_keyframes + 1;
    st->orientation_last_keyframe[0] = o[0];
    st->orientation_last_keyframe[1] = o[1];
    st->orientation_last_keyframe[2] = o[2];
    st->keyframe_age = 0;
  }
