// m3t_render.hip — FocusedBasicDepthRenderer / FocusedSilhouetteRenderer for the renderer-fed
// branches: the square crop around the referenced bodies
// (FocusedRenderer::CalculateProjectionMatrix renderer.cpp:348-405) rasterised with OpenGL's
// rules: pixel centres at integer image coordinates (renderer.cpp:396-404), window coordinates
// snapped to 1/256 pixel, top-left fill rule, 16-bit depth, GL_LESS in draw order
// (basic_depth_renderer.cpp:45-84, silhouette_renderer.cpp:54-100).  Three launches per set of
// renderers: clear + crop, rasterise (the triangle lists split over 32 workgroups per renderer; the
// z-buffer holds packed (depth16 << 16 | draw order << 8 | id) words that triangles reach with
// atomicMin, so the result does not depend on the order), unpack.  Included by m3t_hip_api.hip after
// m3t_kernels.hip.
#ifndef M3T_RENDER_HIP_
#define M3T_RENDER_HIP_

#include "m3t_raster.h"

namespace {

using M44 = RasterM44;
__device__ M44 mul44(const M44& a, const M44& b) {
  M44 o;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r)
      o(r, c) = ((a(r, 0) * b(0, c) + a(r, 1) * b(1, c)) + a(r, 2) * b(2, c)) + a(r, 3) * b(3, c);
  return o;
}
__device__ M44 load44(const float* p) {
  M44 o;
  for (int i = 0; i < 16; ++i) o.m[i] = p[i];
  return o;
}
__device__ __forceinline__ long long floor_div256(long long a) { return a >> 8; }  // arithmetic shift = floor

}  // namespace

// FocusedRenderer::CalculateProjectionMatrix renderer.cpp:348-405 (identical arithmetic in every thread that
// needs it); returns the number of visible referenced bodies
struct FocusedProjection {
  float corner_u, corner_v, scale;
  unsigned visible_mask;
  int n_visible;
  M44 P;
};
__device__ FocusedProjection focused_projection(const RendererDev& r, const CameraDev& cam, const float* body_poses) {
  FocusedProjection f;
  const Affine w2c = load_pose(cam.world2camera);
  float u_min = 3.402823466e+38f, u_max = 1.175494351e-38f, v_min = 3.402823466e+38f, v_max = 1.175494351e-38f;
  f.n_visible = 0;
  f.visible_mask = 0;
  for (int k = 0; k < r.n_referenced; ++k) {
    const float* b2w = body_poses + 16 * r.referenced[k];
    float rr = 0.5f * r.referenced_diameter[k];
    float x, y, z;
    apply_pose(w2c, b2w[12], b2w[13], b2w[14], x, y, z);
    if (z < rr * 1.5f || z - rr < r.z_min || z + rr > r.z_max) continue;
    float abs_x = fabsf(x), abs_y = fabsf(y);
    float x2 = x * x, y2 = y * y, z2 = z * z, r2 = rr * rr;
    float rz = rr * z;
    float z2_r2 = z2 - r2;
    float z3_zr2 = z2_r2 * z;
    float r_u = cam.fu * (abs_x * r2 + rz * sqrtf(z2_r2 + x2)) / z3_zr2;
    float r_v = cam.fv * (abs_y * r2 + rz * sqrtf(z2_r2 + y2)) / z3_zr2;
    float center_u = x * cam.fu / z + cam.ppu;
    float center_v = y * cam.fv / z + cam.ppv;
    float u_min_body = center_u - r_u, u_max_body = center_u + r_u;
    float v_min_body = center_v - r_v, v_max_body = center_v + r_v;
    if (u_min_body > (float)cam.width || u_max_body < 0.0f || v_min_body > (float)cam.height || v_max_body < 0.0f)
      continue;
    u_min = fminf(u_min, u_min_body);
    u_max = fmaxf(u_max, u_max_body);
    v_min = fminf(v_min, v_min_body);
    v_max = fmaxf(v_max, v_max_body);
    f.visible_mask |= 1u << k;
    ++f.n_visible;
  }
  f.corner_u = 0.0f;
  f.corner_v = 0.0f;
  f.scale = 1.0f;
  for (int i = 0; i < 16; ++i) f.P.m[i] = 0.0f;
  if (f.n_visible > 0) {
    const int S = r.image_size;
    const float d = fmaxf(u_max - u_min, v_max - v_min) * 1.05f;  // kImageSizeSafetyMargin
    f.corner_u = 0.5f * (u_min + u_max - d);
    f.corner_v = 0.5f * (v_min + v_max - d);
    f.scale = (float)S / d;
    const float ppu_scaled = (cam.ppu - f.corner_u) * f.scale;
    const float ppv_scaled = (cam.ppv - f.corner_v) * f.scale;
    f.P(0, 0) = 2.0f * cam.fu / d;
    f.P(0, 2) = 2.0f * (ppu_scaled + 0.5f) / (float)S - 1.0f;
    f.P(1, 1) = 2.0f * cam.fv / d;
    f.P(1, 2) = 2.0f * (ppv_scaled + 0.5f) / (float)S - 1.0f;
    f.P(2, 2) = (r.z_max + r.z_min) / (r.z_max - r.z_min);
    f.P(2, 3) = -2.0f * r.z_max * r.z_min / (r.z_max - r.z_min);
    f.P(3, 2) = 1.0f;
  }
  return f;
}

extern "C" {

// 1/3: clear the packed z-buffer, publish the crop (grid: 16 x renderers)
__global__ void __launch_bounds__(M3T_BLOCK_THREADS)
focused_clear_kernel(const RendererDev* renderers, const int* which, const CameraDev* cams, const float* body_poses) {
  const RendererDev& r = renderers[which[blockIdx.y]];
  const int n_px = r.image_size * r.image_size;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_px; i += gridDim.x * blockDim.x) r.packed[i] = 0xffffffffu;
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const FocusedProjection f = focused_projection(r, cams[r.camera], body_poses);
    r.state[RS_CORNER_U] = f.corner_u;
    r.state[RS_CORNER_V] = f.corner_v;
    r.state[RS_SCALE] = f.scale;
    r.state[RS_TERM_A] = r.z_max * r.z_min * 65535.0f / (r.z_max - r.z_min);  // renderer.cpp:567-570
    r.state[RS_TERM_B] = r.z_max * 65535.0f / (r.z_max - r.z_min);
    r.state[RS_N_VISIBLE] = (float)f.n_visible;
    for (int k = 0; k < M3T_MAX_RENDERER_BODIES; ++k)
      r.state[RS_VISIBLE0 + k] = (f.visible_mask >> k & 1u) ? 1.0f : 0.0f;
  }
}

// 2/3: rasterise (grid: slices x renderers; a slice is a contiguous part of every body's triangle list).
// A triangle with a small bounding box is finished by the thread that owns it, row after row (raster_row: three
// additions per pixel, and a row is left behind its covered span -- the slivers of a finely tessellated body have
// boxes that are mostly empty); larger ones are queued in LDS and rasterised by the whole workgroup, a thread taking
// 32-pixel pieces of rows.
__global__ void __launch_bounds__(M3T_BLOCK_THREADS)
focused_raster_kernel(const RendererDev* renderers, const int* which, const CameraDev* cams, const float* body_poses) {
  constexpr int kQueue = 64, kPiece = 32;
  __shared__ RasterTriangle queue[kQueue];
  __shared__ int n_queued;
  const RendererDev& r = renderers[which[blockIdx.y]];
  const CameraDev& cam = cams[r.camera];
  const FocusedProjection f = focused_projection(r, cam, body_poses);
  if (f.n_visible == 0) return;  // block-uniform
  const int S = r.image_size;
  uint32_t* z_buffer = r.packed;
  auto sink = [z_buffer, S](int px, int py, uint32_t word) { atomicMin(&z_buffer[py * S + px], word); };
  const int tid = threadIdx.x, nt = blockDim.x;
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
    for (int base = t_begin; base < t_end; base += nt) {  // block-uniform trip count
      if (tid == 0) n_queued = 0;
      __syncthreads();
      const int t = base + tid;
      RasterTriangle tri;
      if (t < t_end && raster_setup(trans, vertices, triangles, t, culling, S, tri)) {
        const int pixels = (tri.x1 - tri.x0 + 1) * (tri.y1 - tri.y0 + 1);
        int slot = kQueue;
        if (pixels > 192) slot = atomicAdd(&n_queued, 1);
        if (slot < kQueue) {
          queue[slot] = tri;
        } else {
          for (int py = tri.y0; py <= tri.y1; ++py) raster_row(tri, py, tri.x0, tri.x1, low_bits, sink);
        }
      }
      __syncthreads();
      const int nq = min(n_queued, kQueue);
      for (int q = 0; q < nq; ++q) {
        const RasterTriangle big = queue[q];
        const int pieces = (big.x1 - big.x0 + kPiece) / kPiece, total = pieces * (big.y1 - big.y0 + 1);
        for (int i = tid; i < total; i += nt) {
          const int row = i / pieces, xa = big.x0 + (i - row * pieces) * kPiece;
          raster_row(big, big.y0 + row, xa, min(xa + kPiece - 1, big.x1), low_bits, sink);
        }
      }
      __syncthreads();
    }
  }
}

// ---- the two-launch form, used when the z-buffer of a rendering fits the LDS of a CU (image_size <= 200) ----
// Of a finely tessellated body most triangles never reach a pixel (tools/raster_stats.py: 1 000 - 1 300 of 20 950 on
// the probe scene; the rest face away or lie outside the crop), and the survivors' boxes hold ~55 000 pixels in all:
// little work, spread thin.  focused_setup_kernel (grid: slices x renderers) does the set-up and APPENDS the survivors
// to a list; focused_resolve_kernel (a workgroup per band of rows of every renderer) clears its band of the z-buffer in
// LDS, rasterises the list into it with LDS atomics, and writes the depth and id images: no clear launch, no global
// atomics, no unpack launch.  The words and their minimum are those of the three-launch form.
struct RasterSurvivor {
  RasterTriangle tri;
  uint32_t low_bits, pad;
};
static_assert(sizeof(RasterSurvivor) == M3T_SURVIVOR_BYTES, "M3T_SURVIVOR_BYTES");

// which: pairs {renderer, twin or -1}.  A twin is a second renderer of the same camera, geometry, referenced bodies,
// depth range and image size (a FocusedBasicDepthRenderer and a FocusedSilhouetteRenderer of one camera, say): its
// rendering is this one -- the z-buffer word orders by depth and draw order, the id byte follows from the draw order --
// so one set-up and one rasterisation serve both; the resolve kernel writes the twin's images with the twin's ids.
// (The two kernels' bodies live in m3t_render_setup.inc / m3t_render_resolve.inc: the flagged kernels below include the
// same text behind their test, and these two compile to what they always were.)
__global__ void __launch_bounds__(M3T_BLOCK_THREADS)
focused_setup_kernel(const RendererDev* renderers, const int* which, const CameraDev* cams, const float* body_poses) {
#include "m3t_render_setup.inc"
}

// grid: (bands, renderers).  A workgroup owns a band of image rows: its z-buffer band lives in LDS, it looks at every
// survivor and rasterises the rows that fall into its band (round 4: ONE workgroup per renderer took 166 us for the
// probe scene's ~1 200 survivors, the three-launch form 98 us).  The workgroup that finishes last resets the counters.
__global__ void __launch_bounds__(M3T_BLOCK_THREADS)
focused_resolve_kernel(const RendererDev* renderers, const int* which) {
#include "m3t_render_resolve.inc"
}

// ---- the two-launch form behind a judgement that may reset (m3t_hip_judge_set_reset_renderers) ----
// Pair p of `which` is rendered iff the judge flagged one of its readers: the entries readers[reader_first[p] ..
// reader_first[p + 1]) of the judge's list, those whose reset target has a region modality that reads the renderer or
// its twin.  The test is block-uniform and both kernels form it from the same words -- the judge kernels wrote the
// flags before the first of them and nobody writes them in between -- so a pair is set up and resolved or neither:
// the resolve kernel's "last workgroup resets the counters" finds the counters it expects.  A skipped pair stores
// nothing.  always != 0 (a developer switch of the host): every pair runs.
__device__ __forceinline__ bool focused_pair_flagged(const int* flags, const int* reader_first, const int* readers, int p) {
  const int begin = reader_first[p], end = reader_first[p + 1];
  for (int k = begin; k < end; ++k)
    if (flags[readers[k]] != 0) return true;
  return false;
}
__global__ void __launch_bounds__(M3T_BLOCK_THREADS)
focused_setup_flagged_kernel(const RendererDev* renderers, const int* which, const CameraDev* cams, const float* body_poses,
                             const int* flags, const int* reader_first, const int* readers, int always) {
  if (!always && !focused_pair_flagged(flags, reader_first, readers, (int)blockIdx.y)) return;  // block-uniform
#include "m3t_render_setup.inc"
}
__global__ void __launch_bounds__(M3T_BLOCK_THREADS)
focused_resolve_flagged_kernel(const RendererDev* renderers, const int* which, const int* flags, const int* reader_first,
                               const int* readers, int always) {
  if (!always && !focused_pair_flagged(flags, reader_first, readers, (int)blockIdx.x)) return;  // block-uniform
#include "m3t_render_resolve.inc"
}

// 3/3: unpack into the u16 depth image and the u8 id image (grid: 16 x renderers)
__global__ void __launch_bounds__(M3T_BLOCK_THREADS)
focused_unpack_kernel(const RendererDev* renderers, const int* which) {
  const RendererDev& r = renderers[which[blockIdx.y]];
  const int n_px = r.image_size * r.image_size;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_px; i += gridDim.x * blockDim.x) {
    const uint32_t v = r.packed[i];
    r.depth_image[i] = v == 0xffffffffu ? (uint16_t)65535 : (uint16_t)(v >> 16);
    r.silhouette_image[i] = v == 0xffffffffu ? (uint8_t)0 : (uint8_t)(v & 0xffu);
  }
}

}  // extern "C"
#endif  // M3T_RENDER_HIP_
