// m3t_call_args.h -- the argument block of an enqueued call (m3t_hip_reset_bodies, m3t_hip_reset_structures,
// m3t_hip_judge_bodies): lists of ints and of 4 x 4 poses, one behind the other in one block of mapped host memory that
// the call's launches read in place.  A block is laid out ONCE, segment after segment; its segments address it as the
// host fills it and as the device reads it.  Plain C++17, no HIP header: tests/cpp/call_args_check.cpp checks it.
#pragma once

#include <cstddef>
#include <cstring>

namespace m3t_args {

constexpr size_t kPoseBytes = 64;
constexpr size_t kPoseAlign = 16;  // a list of poses starts at a multiple of this

struct Segment {
  size_t offset = 0, count = 0;  // bytes from the start of the block; ints or poses
  template <typename T>
  T* in(void* block) const { return reinterpret_cast<T*>(static_cast<char*>(block) + offset); }
};

struct Layout {  // appends segments: every offset of a block comes from here
  size_t bytes = 0;
  Segment Ints(size_t n) {
    const Segment s{bytes, n};
    bytes += n * sizeof(int);
    return s;
  }
  Segment Poses(size_t n) {
    bytes = (bytes + kPoseAlign - 1) / kPoseAlign * kPoseAlign;
    const Segment s{bytes, n};
    bytes += n * kPoseBytes;
    return s;
  }
};

inline void PutInts(void* block, const Segment& s, const void* ints) {
  if (s.count) std::memcpy(s.in<int>(block), ints, s.count * sizeof(int));
}
inline void PutPoses(void* block, const Segment& s, const float* poses) {
  if (s.count) std::memcpy(s.in<float>(block), poses, s.count * kPoseBytes);
}
// [renderer ids][{renderer, -1} pairs]: the two lists a launch of the renderers takes
inline void PutRenderers(void* block, const Segment& ids, const Segment& pairs, const int* renderers) {
  for (size_t k = 0; k < ids.count; ++k) {
    ids.in<int>(block)[k] = pairs.in<int>(block)[2 * k] = renderers[k];
    pairs.in<int>(block)[2 * k + 1] = -1;
  }
}

// The three calls' blocks.  (Members are initialised in the order they are declared in: that order IS the layout.)
// [body ids][region modality ids][renderer ids][pairs], then the poses -- none when the call sets no poses
struct ResetBodiesArgs : Layout {
  Segment body_ids, region_ids, renderer_ids, renderer_pairs, poses;
  ResetBodiesArgs(size_t n, size_t n_region, size_t n_render, bool with_poses)
      : body_ids(Ints(n)), region_ids(Ints(n_region)), renderer_ids(Ints(n_render)), renderer_pairs(Ints(2 * n_render)),
        poses(Poses(with_poses ? n : 0)) {}
};
// [structures][links] (three ints each) [region modality ids][renderer ids][pairs], then the poses
struct ResetStructuresArgs : Layout {
  Segment structures, links, region_ids, renderer_ids, renderer_pairs, poses;
  ResetStructuresArgs(size_t n_structures, size_t n_links, size_t n_region, size_t n_render, size_t n_poses)
      : structures(Ints(3 * n_structures)), links(Ints(3 * n_links)), region_ids(Ints(n_region)),
        renderer_ids(Ints(n_render)), renderer_pairs(Ints(2 * n_render)), poses(Poses(n_poses)) {}
};
// [ground-truth poses][region modality ids][the listed body of each][first region of each body, n + 1]
struct JudgeBodiesArgs : Layout {
  Segment gt_poses, region_ids, region_body, region_first;
  JudgeBodiesArgs(size_t n, size_t n_region)
      : gt_poses(Poses(n)), region_ids(Ints(n_region)), region_body(Ints(n_region)), region_first(Ints(n + 1)) {}
};

// judge_bodies of a judge that may run start-modality renderers (m3t_hip_judge_set_reset_renderers): the four lists of
// JudgeBodiesArgs where JudgeBodiesArgs puts them, then [{renderer, twin or -1} pairs][first reader of each pair,
// n_pairs + 1][readers: indices into the judge's list]
struct JudgeBodiesRenderArgs : Layout {
  Segment gt_poses, region_ids, region_body, region_first, renderer_pairs, reader_first, readers;
  JudgeBodiesRenderArgs(size_t n, size_t n_region, size_t n_pairs, size_t n_readers)
      : gt_poses(Poses(n)), region_ids(Ints(n_region)), region_body(Ints(n_region)), region_first(Ints(n + 1)),
        renderer_pairs(Ints(2 * n_pairs)), reader_first(Ints(n_pairs + 1)), readers(Ints(n_readers)) {}
};

// The two calls that may restart texture modalities with a built-in detector (m3t_features.hip): the block of
// ResetBodiesArgs / JudgeBodiesRenderArgs, segment for segment where that layout puts it, then [texture items: {detector,
// texture modality, flag index or -1}, three ints each].  A call that lists no texture modality fills the old block.
struct ResetBodiesTextureArgs : Layout {
  Segment body_ids, region_ids, renderer_ids, renderer_pairs, poses, texture_items;
  ResetBodiesTextureArgs(size_t n, size_t n_region, size_t n_render, bool with_poses, size_t n_texture)
      : body_ids(Ints(n)), region_ids(Ints(n_region)), renderer_ids(Ints(n_render)), renderer_pairs(Ints(2 * n_render)),
        poses(Poses(with_poses ? n : 0)), texture_items(Ints(3 * n_texture)) {}
};
struct JudgeBodiesTextureArgs : Layout {
  Segment gt_poses, region_ids, region_body, region_first, renderer_pairs, reader_first, readers, texture_items;
  JudgeBodiesTextureArgs(size_t n, size_t n_region, size_t n_pairs, size_t n_readers, size_t n_texture)
      : gt_poses(Poses(n)), region_ids(Ints(n_region)), region_body(Ints(n_region)), region_first(Ints(n + 1)),
        renderer_pairs(Ints(2 * n_pairs)), reader_first(Ints(n_pairs + 1)), readers(Ints(n_readers)),
        texture_items(Ints(3 * n_texture)) {}
};

}  // namespace m3t_args
