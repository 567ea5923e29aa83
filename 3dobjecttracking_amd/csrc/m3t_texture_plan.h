// m3t_texture_plan.h -- how the Hamming match of the texture modalities is launched: in one workgroup per modality
// (texture_match_kernel, m3t_texture.hip) or tiled over ring slots and query tiles with a collect pass behind it
// (texture_match_tiled_kernel + texture_collect_kernel, m3t_texture_tiled.hip): the decision apart from the launches.
// Plain C++17, no HIP header, no context: LaunchCorrespondences launches from what PlanMatch returns,
// tests/cpp/texture_tiled_check.cpp runs the same code on the host.  Both forms give the same bits; the plan decides
// time and memory only.  It depends on what the host knows -- the mode (a developer override), the number of Hamming
// modalities, the largest n_keyframes among them -- and on nothing the device decides (how many keyframes are held, how many points each has).
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace m3t_texture {

// (m3t_texture.h has the same figures as M3T_TEXTURE_*; m3t_hip_api.hip asserts that they agree)
constexpr int kMatchThreads = 256;
constexpr int kQueryTile = 64;
constexpr int kMaxFeatures = 4096;
constexpr int kQueryTiles = kMaxFeatures / kQueryTile;  // per ring slot
constexpr int kMaxKeyframes = 8;
constexpr size_t kBestBytes = 12;  // {d0, d1, i0} per ring entry

enum MatchMode { kAuto = 0, kOneWorkgroup = 1, kTiled = 2 };

// ---- developer override -------------------------------------------------------------------------------------------
// M3T_HIP_TEXTURE_MATCH: "one" (the one-workgroup matcher), "tiled" or "auto"; a context looks at it once, when it is
// made.  No variable, an empty one and any other text are AUTO.
inline MatchMode ParseMatchMode(const char* text) {
  if (text == nullptr) return kAuto;
  if (std::strcmp(text, "one") == 0) return kOneWorkgroup;
  if (std::strcmp(text, "tiled") == 0) return kTiled;
  return kAuto;
}
inline MatchMode ReadMatchOverride() { return ParseMatchMode(std::getenv("M3T_HIP_TEXTURE_MATCH")); }

// What AUTO stands for.  Measured (profiles/r17_texture_match_tiled.txt): the tiled form is the
// faster one at every size that was timed -- 300 x 300 x 32 bytes with one modality and one keyframe, where its second
// launch weighs most, included (25 against 73 us) -- so no size threshold stands between the two.
constexpr MatchMode kAutoForm = kTiled;

struct Grid {
  int x, y;
};
struct MatchPlan {
  int form;              // 0: nothing to match (no Hamming modality); else kOneWorkgroup or kTiled
  Grid match;            // texture_match_kernel (one workgroup form) or texture_match_tiled_kernel
  Grid collect;          // texture_collect_kernel; {0, 0} in the one-workgroup form, which collects itself
  size_t scratch_bytes;  // best-two scratch per Hamming modality; 0 in the one-workgroup form
};

// n_hamming: the Hamming modalities of the context (L2 ones have a matcher of their own and do not count);
// keyframes_max: the largest n_keyframes among them.  A bad mode plans like AUTO.
inline MatchPlan PlanMatch(int mode, int n_hamming, int keyframes_max) {
  MatchPlan plan{0, {0, 0}, {0, 0}, 0};
  if (n_hamming <= 0) return plan;
  const int slots = keyframes_max < 1 ? 1 : keyframes_max > kMaxKeyframes ? kMaxKeyframes : keyframes_max;
  plan.form = mode == kTiled ? kTiled : mode == kOneWorkgroup ? kOneWorkgroup : kAutoForm;
  if (plan.form == kOneWorkgroup) {
    plan.match = {n_hamming, 1};
    return plan;
  }
  plan.match = {n_hamming, slots * kQueryTiles};
  plan.collect = {n_hamming, 1};
  plan.scratch_bytes = size_t(slots) * kMaxFeatures * kBestBytes;
  return plan;
}

}  // namespace m3t_texture
