// The argument blocks of the two enqueued calls that may restart texture modalities
// (3dobjecttracking_amd/csrc/m3t_call_args.h: ResetBodiesTextureArgs, JudgeBodiesTextureArgs) on the host: blocks
// filled in ordinary memory of exactly the size the layout asks for, compared with offsets, sizes and contents written
// down from the layouts the calls' kernels read --
//   reset_bodies  [body ids n][region ids][renderer ids][{renderer, -1} pairs], poses at the next multiple of 16 bytes
//                 and only when the call has poses, then [texture items: {detector, texture modality, flag or -1}]
//   judge_bodies  [ground-truth poses n x 64 bytes][region ids][listed body of each][first region of each body, n + 1]
//                 [{renderer, twin or -1} pairs][first reader of each pair, n_pairs + 1][readers], then [texture items]
// -- and not from the header; with no texture item a block has the size and the bytes of ResetBodiesArgs /
// JudgeBodiesRenderArgs.  Prints "checks N errors M".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../3dobjecttracking_amd/csrc/m3t_call_args.h"

using namespace m3t_args;

static int g_checks = 0, g_errors = 0;
#define CHECK(cond)                                  \
  do {                                               \
    ++g_checks;                                      \
    if (!(cond)) {                                   \
      ++g_errors;                                    \
      std::printf("line %d: %s\n", __LINE__, #cond); \
    }                                                \
  } while (0)

static const unsigned char kUntouched = 0xAB;  // what a byte no segment covers keeps

static std::vector<float> Poses(size_t n, float base) {
  std::vector<float> p(n * 16);
  for (size_t i = 0; i < p.size(); ++i) p[i] = base + float(i);
  return p;
}
struct Expected {
  std::vector<unsigned char> bytes;
  explicit Expected(size_t n) : bytes(n, kUntouched) {}
  void Ints(size_t first_int, std::vector<int> v) { std::memcpy(&bytes[first_int * 4], v.data(), v.size() * 4); }
  void Floats(size_t first_byte, const std::vector<float>& v) { std::memcpy(&bytes[first_byte], v.data(), v.size() * 4); }
  bool Equals(const std::vector<unsigned char>& block) const { return block == bytes; }
};

static std::vector<unsigned char> FillReset(const ResetBodiesTextureArgs& a, const int* ids, const int* regions,
                                            const int* renderers, const float* poses, const int* items) {
  std::vector<unsigned char> block(a.bytes, kUntouched);
  PutInts(block.data(), a.body_ids, ids);
  PutInts(block.data(), a.region_ids, regions);
  PutRenderers(block.data(), a.renderer_ids, a.renderer_pairs, renderers);
  PutPoses(block.data(), a.poses, poses);
  PutInts(block.data(), a.texture_items, items);
  return block;
}

static void ResetBodiesTexture() {
  {  // one texture-only body with a pose: 1 + 0 + 1 + 2 = 4 ints, the pose at 16, the item at 80: 92 bytes
    const ResetBodiesTextureArgs a(1, 0, 1, true, 1);
    CHECK(a.body_ids.offset == 0 && a.region_ids.offset == 4 && a.renderer_ids.offset == 4 && a.renderer_pairs.offset == 8);
    CHECK(a.poses.offset == 16 && a.poses.count == 1);
    CHECK(a.texture_items.offset == 80 && a.texture_items.count == 3);
    CHECK(a.bytes == 92);
    const int ids[] = {7}, renderers[] = {3}, items[] = {0, 2, -1};
    const std::vector<float> poses = Poses(1, 100.0f);
    Expected e(92);
    e.Ints(0, {7, 3, 3, -1});
    e.Floats(16, poses);
    e.Ints(20, {0, 2, -1});
    CHECK(e.Equals(FillReset(a, ids, nullptr, renderers, poses.data(), items)));
  }
  {  // n = 2, 2 region ids, 3 renderers, poses, 2 items: 2 + 2 + 3 + 6 = 13 ints = 52 bytes, poses at 64, items at 192
    const ResetBodiesTextureArgs a(2, 2, 3, true, 2);
    CHECK(a.region_ids.offset == 8 && a.renderer_ids.offset == 16 && a.renderer_pairs.offset == 28);
    CHECK(a.poses.offset == 64);
    CHECK(a.texture_items.offset == 192 && a.texture_items.count == 6);
    CHECK(a.bytes == 216);
    const int ids[] = {4, 1}, regions[] = {1, 4}, renderers[] = {2, 8, 9}, items[] = {1, 1, -1, 3, 4, -1};
    const std::vector<float> poses = Poses(2, 200.0f);
    Expected e(216);
    e.Ints(0, {4, 1, 1, 4, 2, 8, 9, 2, -1, 8, -1, 9, -1});
    e.Floats(64, poses);
    e.Ints(48, {1, 1, -1, 3, 4, -1});
    std::vector<unsigned char> block = FillReset(a, ids, regions, renderers, poses.data(), items);
    CHECK(e.Equals(block));
    CHECK(block[52] == kUntouched && block[63] == kUntouched);  // the padding in front of the poses
    CHECK(a.texture_items.in<int>(block.data())[3] == 3 && a.texture_items.in<int>(block.data())[5] == -1);
  }
  {  // without poses (poses = NULL): 3 + 0 + 1 + 2 = 6 ints; the pose list is empty but aligns: items at 32, 68 bytes
    const ResetBodiesTextureArgs a(3, 0, 1, false, 3);
    CHECK(a.poses.offset == 32 && a.poses.count == 0);
    CHECK(a.texture_items.offset == 32 && a.texture_items.count == 9);
    CHECK(a.bytes == 68);
    const int ids[] = {0, 1, 2}, renderers[] = {5}, items[] = {0, 0, -1, 1, 1, -1, 2, 2, -1};
    Expected e(68);
    e.Ints(0, {0, 1, 2, 5, 5, -1});
    e.Ints(8, {0, 0, -1, 1, 1, -1, 2, 2, -1});
    CHECK(e.Equals(FillReset(a, ids, nullptr, renderers, nullptr, items)));
  }
  // no texture item: the size, the segments and the bytes of ResetBodiesArgs
  for (int with_poses = 0; with_poses < 2; ++with_poses)
    for (size_t n = 1; n <= 5; ++n)
      for (size_t n_render = 0; n_render <= 2; ++n_render) {
        const size_t n_region = n - 1;
        const ResetBodiesTextureArgs a(n, n_region, n_render, with_poses != 0, 0);
        const ResetBodiesArgs old(n, n_region, n_render, with_poses != 0);
        CHECK(a.bytes == old.bytes && a.texture_items.count == 0 && a.texture_items.offset == old.bytes);
        CHECK(a.body_ids.offset == old.body_ids.offset && a.region_ids.offset == old.region_ids.offset &&
              a.renderer_ids.offset == old.renderer_ids.offset && a.renderer_pairs.offset == old.renderer_pairs.offset &&
              a.poses.offset == old.poses.offset && a.poses.count == old.poses.count);
        const int ids[] = {9, 8, 7, 6, 5}, regions[] = {1, 2, 3, 4}, renderers[] = {6, 2};
        const std::vector<float> poses = Poses(n, 300.0f);
        std::vector<unsigned char> before(old.bytes, kUntouched);
        PutInts(before.data(), old.body_ids, ids);
        PutInts(before.data(), old.region_ids, regions);
        PutRenderers(before.data(), old.renderer_ids, old.renderer_pairs, renderers);
        PutPoses(before.data(), old.poses, poses.data());
        CHECK(FillReset(a, ids, regions, renderers, poses.data(), nullptr) == before);
      }
}

static std::vector<unsigned char> FillJudge(const JudgeBodiesTextureArgs& a, const float* gt, const int* regions,
                                            const int* region_body, const int* region_first, const int* pairs,
                                            const int* reader_first, const int* readers, const int* items) {
  std::vector<unsigned char> block(a.bytes, kUntouched);
  PutPoses(block.data(), a.gt_poses, gt);
  PutInts(block.data(), a.region_ids, regions);
  PutInts(block.data(), a.region_body, region_body);
  PutInts(block.data(), a.region_first, region_first);
  PutInts(block.data(), a.renderer_pairs, pairs);
  PutInts(block.data(), a.reader_first, reader_first);
  PutInts(block.data(), a.readers, readers);
  PutInts(block.data(), a.texture_items, items);
  return block;
}

static void JudgeBodiesTexture() {
  {  // three texture-only bodies, a pair each: poses 192 bytes, first 4 ints, pairs 6, reader_first 4, readers 3, items 9
    const JudgeBodiesTextureArgs a(3, 0, 3, 3, 3);
    CHECK(a.gt_poses.offset == 0 && a.region_ids.offset == 192 && a.region_body.offset == 192 && a.region_first.offset == 192);
    CHECK(a.renderer_pairs.offset == 208 && a.reader_first.offset == 232 && a.readers.offset == 248);
    CHECK(a.texture_items.offset == 260 && a.texture_items.count == 9);
    CHECK(a.bytes == 296);
    const std::vector<float> gt = Poses(3, 400.0f);
    const int first[] = {0, 0, 0, 0}, pairs[] = {0, -1, 1, -1, 2, -1}, reader_first[] = {0, 1, 2, 3}, readers[] = {0, 1, 2};
    const int items[] = {0, 0, 0, 1, 1, 1, 2, 2, 2};
    Expected e(296);
    e.Floats(0, gt);
    e.Ints(48, {0, 0, 0, 0, 0, -1, 1, -1, 2, -1, 0, 1, 2, 3, 0, 1, 2, 0, 0, 0, 1, 1, 1, 2, 2, 2});
    CHECK(e.Equals(FillJudge(a, gt.data(), nullptr, nullptr, first, pairs, reader_first, readers, items)));
  }
  {  // two bodies with a region modality each, one pair of twins read by both, one texture item flagged by entry 1
    const JudgeBodiesTextureArgs a(2, 2, 1, 2, 1);
    CHECK(a.region_ids.offset == 128 && a.region_body.offset == 136 && a.region_first.offset == 144);
    CHECK(a.renderer_pairs.offset == 156 && a.reader_first.offset == 164 && a.readers.offset == 172);
    CHECK(a.texture_items.offset == 180 && a.bytes == 192);
    const std::vector<float> gt = Poses(2, 500.0f);
    const int regions[] = {3, 5}, region_body[] = {0, 1}, first[] = {0, 1, 2}, pairs[] = {4, 7}, reader_first[] = {0, 2};
    const int readers[] = {0, 1}, items[] = {2, 6, 1};
    Expected e(192);
    e.Floats(0, gt);
    e.Ints(32, {3, 5, 0, 1, 0, 1, 2, 4, 7, 0, 2, 0, 1, 2, 6, 1});
    CHECK(e.Equals(FillJudge(a, gt.data(), regions, region_body, first, pairs, reader_first, readers, items)));
  }
  // no texture item: the size, the segments and the bytes of JudgeBodiesRenderArgs
  for (size_t n = 1; n <= 4; ++n)
    for (size_t n_pairs = 0; n_pairs <= 2; ++n_pairs) {
      const size_t n_region = n - 1, n_readers = n_pairs ? n_pairs + 1 : 0;
      const JudgeBodiesTextureArgs a(n, n_region, n_pairs, n_readers, 0);
      const JudgeBodiesRenderArgs old(n, n_region, n_pairs, n_readers);
      CHECK(a.bytes == old.bytes && a.texture_items.count == 0 && a.texture_items.offset == old.bytes);
      CHECK(a.gt_poses.offset == old.gt_poses.offset && a.region_ids.offset == old.region_ids.offset &&
            a.region_body.offset == old.region_body.offset && a.region_first.offset == old.region_first.offset &&
            a.renderer_pairs.offset == old.renderer_pairs.offset && a.reader_first.offset == old.reader_first.offset &&
            a.readers.offset == old.readers.offset);
      const std::vector<float> gt = Poses(n, 600.0f);
      const int regions[] = {2, 4, 6}, region_body[] = {0, 1, 2}, first[] = {0, 1, 2, 3, 3}, pairs[] = {1, 3, 5, -1};
      const int reader_first[] = {0, 2, 3}, readers[] = {0, 1, 2};
      std::vector<unsigned char> before(old.bytes, kUntouched);
      PutPoses(before.data(), old.gt_poses, gt.data());
      PutInts(before.data(), old.region_ids, regions);
      PutInts(before.data(), old.region_body, region_body);
      PutInts(before.data(), old.region_first, first);
      PutInts(before.data(), old.renderer_pairs, pairs);
      PutInts(before.data(), old.reader_first, reader_first);
      PutInts(before.data(), old.readers, readers);
      CHECK(FillJudge(a, gt.data(), regions, region_body, first, pairs, reader_first, readers, nullptr) == before);
    }
}

int main() {
  ResetBodiesTexture();
  JudgeBodiesTexture();
  std::printf("checks %d errors %d\n", g_checks, g_errors);
  return g_errors == 0 ? 0 : 1;
}
