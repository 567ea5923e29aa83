// The argument blocks of the enqueued calls (3dobjecttracking_amd/csrc/m3t_call_args.h) on the host: blocks filled in
// ordinary memory of exactly the size the layout asks for, compared with offsets, sizes and contents written down from
// the three layouts the calls' kernels read --
//   reset_bodies      [body ids n][region ids][renderer ids][{renderer, -1} pairs], poses at the next multiple of 16
//                     bytes and only when the call has poses
//   reset_structures  [structures x 3 ints][links x 3 ints][region ids][renderer ids][pairs], poses likewise
//   judge_bodies      [ground-truth poses n x 64 bytes][region ids][listed body of each][first region of each body, n + 1]
// -- and not from the header.  Prints "checks N errors M".
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

// pose k of a call: 16 floats that name their pose and their place
static std::vector<float> Poses(size_t n, float base) {
  std::vector<float> p(n * 16);
  for (size_t i = 0; i < p.size(); ++i) p[i] = base + float(i);
  return p;
}
// the block as written down: ints at int positions, floats at byte positions, everything else untouched
struct Expected {
  std::vector<unsigned char> bytes;
  explicit Expected(size_t n) : bytes(n, kUntouched) {}
  void Ints(size_t first_int, std::vector<int> v) { std::memcpy(&bytes[first_int * 4], v.data(), v.size() * 4); }
  void Floats(size_t first_byte, const std::vector<float>& v) { std::memcpy(&bytes[first_byte], v.data(), v.size() * 4); }
  bool Equals(const std::vector<unsigned char>& block) const { return block == bytes; }
};

static void ResetBodies() {
  {  // n = 1 with poses, no region modality, no renderer: 1 int, poses at 16, 80 bytes
    const ResetBodiesArgs a(1, 0, 0, true);
    CHECK(a.body_ids.offset == 0 && a.region_ids.offset == 4 && a.renderer_ids.offset == 4 && a.renderer_pairs.offset == 4);
    CHECK(a.poses.offset == 16);
    CHECK(a.bytes == 80);
    std::vector<unsigned char> block(a.bytes, kUntouched);
    const int ids[] = {7};
    const std::vector<float> poses = Poses(1, 100.0f);
    PutInts(block.data(), a.body_ids, ids);
    PutInts(block.data(), a.region_ids, nullptr);
    PutRenderers(block.data(), a.renderer_ids, a.renderer_pairs, nullptr);
    PutPoses(block.data(), a.poses, poses.data());
    Expected e(80);
    e.Ints(0, {7});
    e.Floats(16, poses);
    CHECK(e.Equals(block));
  }
  {  // n = 4, 4 region ids, no renderer: 8 ints, poses at 32 without padding
    const ResetBodiesArgs a(4, 4, 0, true);
    CHECK(a.region_ids.offset == 16 && a.region_ids.count == 4);
    CHECK(a.poses.offset == 32);
    CHECK(a.bytes == 32 + 4 * 64);
    std::vector<unsigned char> block(a.bytes, kUntouched);
    const int ids[] = {3, 0, 2, 1}, regions[] = {0, 1, 2, 3};
    const std::vector<float> poses = Poses(4, 200.0f);
    PutInts(block.data(), a.body_ids, ids);
    PutInts(block.data(), a.region_ids, regions);
    PutRenderers(block.data(), a.renderer_ids, a.renderer_pairs, nullptr);
    PutPoses(block.data(), a.poses, poses.data());
    Expected e(288);
    e.Ints(0, {3, 0, 2, 1, 0, 1, 2, 3});
    e.Floats(32, poses);
    CHECK(e.Equals(block));
  }
  {  // n = 3, 2 region ids, 1 renderer: 3 + 2 + 1 + 2 = 8 ints, the pair at ints 6 and 7
    const ResetBodiesArgs a(3, 2, 1, true);
    CHECK(a.region_ids.offset == 12 && a.renderer_ids.offset == 20 && a.renderer_pairs.offset == 24);
    CHECK(a.renderer_ids.count == 1 && a.renderer_pairs.count == 2);
    CHECK(a.poses.offset == 32);
    CHECK(a.bytes == 32 + 3 * 64);
    std::vector<unsigned char> block(a.bytes, kUntouched);
    const int ids[] = {5, 6, 9}, regions[] = {4, 8}, renderers[] = {11};
    const std::vector<float> poses = Poses(3, 300.0f);
    PutInts(block.data(), a.body_ids, ids);
    PutInts(block.data(), a.region_ids, regions);
    PutRenderers(block.data(), a.renderer_ids, a.renderer_pairs, renderers);
    PutPoses(block.data(), a.poses, poses.data());
    Expected e(224);
    e.Ints(0, {5, 6, 9, 4, 8, 11, 11, -1});
    e.Floats(32, poses);
    CHECK(e.Equals(block));
    CHECK(a.renderer_pairs.in<int>(block.data())[0] == 11 && a.renderer_pairs.in<int>(block.data())[1] == -1);
  }
  {  // n = 5, 5 region ids, 2 renderers: 5 + 5 + 2 + 4 = 16 ints, poses at 64
    const ResetBodiesArgs a(5, 5, 2, true);
    CHECK(a.renderer_ids.offset == 40 && a.renderer_pairs.offset == 48);
    CHECK(a.poses.offset == 64);
    CHECK(a.bytes == 64 + 5 * 64);
    std::vector<unsigned char> block(a.bytes, kUntouched);
    const int ids[] = {0, 1, 2, 3, 4}, regions[] = {10, 11, 12, 13, 14}, renderers[] = {2, 0};
    const std::vector<float> poses = Poses(5, 400.0f);
    PutInts(block.data(), a.body_ids, ids);
    PutInts(block.data(), a.region_ids, regions);
    PutRenderers(block.data(), a.renderer_ids, a.renderer_pairs, renderers);
    PutPoses(block.data(), a.poses, poses.data());
    Expected e(384);
    e.Ints(0, {0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 2, 0, 2, -1, 0, -1});
    e.Floats(64, poses);
    CHECK(e.Equals(block));
  }
  {  // without poses: no pose segment, the block ends where the poses would begin (3 + 3 + 1 + 2 = 9 ints -> 48)
    const ResetBodiesArgs a(3, 3, 1, false);
    CHECK(a.poses.offset == 48 && a.poses.count == 0);
    CHECK(a.bytes == 48);
    std::vector<unsigned char> block(a.bytes, kUntouched);
    const int ids[] = {2, 1, 0}, regions[] = {0, 1, 2}, renderers[] = {6};
    PutInts(block.data(), a.body_ids, ids);
    PutInts(block.data(), a.region_ids, regions);
    PutRenderers(block.data(), a.renderer_ids, a.renderer_pairs, renderers);
    PutPoses(block.data(), a.poses, nullptr);
    Expected e(48);
    e.Ints(0, {2, 1, 0, 0, 1, 2, 6, 6, -1});
    CHECK(e.Equals(block));
    const ResetBodiesArgs one(1, 0, 0, false);  // ... and the smallest call
    CHECK(one.poses.offset == 16 && one.bytes == 16);
  }
}

static void ResetStructures() {
  // two structures of 1 and 3 links in mode 0 (every link takes a pose: 4 poses), 3 region ids, 1 renderer:
  // 2 x 3 | 4 x 3 | 3 | 1 | 2 ints = 24 ints, poses at 96
  struct Three {
    int a, b, c;
  };
  const Three structures[] = {{0, 0, 1}, {1, 1, 3}};                          // {optimizer, first link entry, links}
  const Three links[] = {{4, 0, -1}, {5, 1, -1}, {6, 2, 1}, {7, 3, 1}};       // {body, pose, pose of the parent}
  const int regions[] = {4, 5, 7}, renderers[] = {3};
  const ResetStructuresArgs a(2, 4, 3, 1, 4);
  CHECK(a.structures.offset == 0);
  CHECK(a.links.offset == 6 * 4);
  CHECK(a.region_ids.offset == 18 * 4);
  CHECK(a.renderer_ids.offset == 21 * 4);
  CHECK(a.renderer_pairs.offset == 22 * 4);
  CHECK(a.poses.offset == 96 && a.poses.count == 4);
  CHECK(a.bytes == 96 + 4 * 64);
  std::vector<unsigned char> block(a.bytes, kUntouched);
  const std::vector<float> poses = Poses(4, 500.0f);
  PutInts(block.data(), a.structures, structures);
  PutInts(block.data(), a.links, links);
  PutInts(block.data(), a.region_ids, regions);
  PutRenderers(block.data(), a.renderer_ids, a.renderer_pairs, renderers);
  PutPoses(block.data(), a.poses, poses.data());
  Expected e(352);
  e.Ints(0, {0, 0, 1, 1, 1, 3, 4, 0, -1, 5, 1, -1, 6, 2, 1, 7, 3, 1, 4, 5, 7, 3, 3, -1});
  e.Floats(96, poses);
  CHECK(e.Equals(block));
  // one structure of one link, nothing else: 6 ints -> poses at 32 (8 bytes the launches never read)
  const ResetStructuresArgs b(1, 1, 0, 0, 1);
  CHECK(b.links.offset == 12 && b.region_ids.offset == 24 && b.poses.offset == 32 && b.bytes == 96);
}

static void JudgeBodies() {
  {  // n = 2 without reset: no region modality, the poses first, then only the n + 1 firsts
    const JudgeBodiesArgs a(2, 0);
    CHECK(a.gt_poses.offset == 0 && a.gt_poses.count == 2);
    CHECK(a.region_ids.offset == 128 && a.region_body.offset == 128 && a.region_first.offset == 128);
    CHECK(a.bytes == 128 + 3 * 4);
    std::vector<unsigned char> block(a.bytes, kUntouched);
    const std::vector<float> poses = Poses(2, 600.0f);
    const int first[] = {0, 0, 0};
    PutPoses(block.data(), a.gt_poses, poses.data());
    PutInts(block.data(), a.region_ids, nullptr);
    PutInts(block.data(), a.region_body, nullptr);
    PutInts(block.data(), a.region_first, first);
    Expected e(140);
    e.Floats(0, poses);
    e.Ints(32, {0, 0, 0});
    CHECK(e.Equals(block));
  }
  {  // n = 2, regions {1, 2} of body 0 and {0} of body 1
    const JudgeBodiesArgs a(2, 3);
    CHECK(a.region_ids.offset == 128 && a.region_body.offset == 140 && a.region_first.offset == 152);
    CHECK(a.bytes == 128 + (3 + 3 + 3) * 4);
    std::vector<unsigned char> block(a.bytes, kUntouched);
    const std::vector<float> poses = Poses(2, 700.0f);
    const int ids[] = {1, 2, 0}, body[] = {0, 0, 1}, first[] = {0, 2, 3};
    PutPoses(block.data(), a.gt_poses, poses.data());
    PutInts(block.data(), a.region_ids, ids);
    PutInts(block.data(), a.region_body, body);
    PutInts(block.data(), a.region_first, first);
    Expected e(164);
    e.Floats(0, poses);
    e.Ints(32, {1, 2, 0, 0, 0, 1, 0, 2, 3});
    CHECK(e.Equals(block));
  }
}

int main() {
  // the rule every pose list follows, at each residue of the int count
  for (size_t ints = 0; ints <= 9; ++ints) {
    Layout l;
    l.Ints(ints);
    const Segment p = l.Poses(2);
    const size_t want[] = {0, 16, 16, 16, 16, 32, 32, 32, 32, 48};
    CHECK(p.offset == want[ints] && p.offset % 16 == 0 && p.offset >= ints * 4 && p.offset < ints * 4 + 16);
    CHECK(l.bytes == want[ints] + 128);
  }
  ResetBodies();
  ResetStructures();
  JudgeBodies();
  std::printf("checks %d errors %d\n", g_checks, g_errors);
  return g_errors ? 1 : 0;
}
