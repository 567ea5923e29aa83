// m3t_features_focus.inc -- the body of texture_focus_kernel and texture_focus_list_kernel (m3t_features.hip), included
// into both: detectors, mods, cams and body_poses are the kernel's parameters, detector_index names the detector, the
// row band is blockIdx.y.
  CDetector& d = *(CDetector*)(detectors + detector_index);
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
