// texture_tiled_check.cpp -- what the tiled Hamming matcher (csrc/m3t_texture_tiled.hip) shares with the host, on the
// host: m3t_tex_best2_append (m3t_texture.h) against one sequential pass of m3t_tex_best2_update over every split of
// every short sequence of distances, and the launch plan (m3t_texture_plan.h) for every mode.  Stand-alone:
//   g++ -std=c++17 -ffp-contract=off -o texture_tiled_check texture_tiled_check.cpp && ./texture_tiled_check
// prints "checks N errors M" and returns M != 0.
#include <cstdio>
#include <vector>

#include "../../3dobjecttracking_amd/csrc/m3t_texture.h"
#include "../../3dobjecttracking_amd/csrc/m3t_texture_plan.h"

static int g_checks = 0, g_errors = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    ++g_checks;                                                 \
    if (!(cond)) {                                              \
      ++g_errors;                                               \
      std::printf("line %d: %s\n", __LINE__, #cond);            \
    }                                                           \
  } while (0)

static bool Same(const m3t_tex_best2& a, const m3t_tex_best2& b) {
  // (the index of an absent best is -1 on both sides: init and no update)
  return a.d0 == b.d0 && a.d1 == b.d1 && a.i0 == b.i0;
}
// the best two of d[begin .. end) fed in ascending index
static m3t_tex_best2 Pass(const std::vector<int>& d, int begin, int end) {
  m3t_tex_best2 b;
  m3t_tex_best2_init(&b);
  for (int i = begin; i < end; ++i) m3t_tex_best2_update(&b, d[size_t(i)], i);
  return b;
}
// the ranges [cut[k], cut[k + 1]) joined in order
static m3t_tex_best2 Joined(const std::vector<int>& d, const std::vector<int>& cut) {
  m3t_tex_best2 b = Pass(d, cut[0], cut[1]);
  for (size_t k = 1; k + 1 < cut.size(); ++k) {
    const m3t_tex_best2 later = Pass(d, cut[k], cut[k + 1]);
    m3t_tex_best2_append(&b, &later);
  }
  return b;
}

static void CheckAppend() {
  for (int n = 0; n <= 6; ++n) {
    int n_sequences = 1;
    for (int i = 0; i < n; ++i) n_sequences *= 3;
    for (int code = 0; code < n_sequences; ++code) {
      std::vector<int> d(static_cast<size_t>(n));
      for (int i = 0, c = code; i < n; ++i, c /= 3) d[size_t(i)] = c % 3;  // distances out of {0, 1, 2}: ties of every kind
      const m3t_tex_best2 whole = Pass(d, 0, n);
      for (int a = 0; a <= n; ++a) {  // every two-way split, the empty and the one-entry sides among them
        CHECK(Same(Joined(d, {0, a, n}), whole));
        for (int b = a; b <= n; ++b)  // every four-way split (the four waves), empty ranges among them
          for (int c = b; c <= n; ++c) CHECK(Same(Joined(d, {0, a, b, c, n}), whole));
      }
    }
  }
  // written down: the lower index wins a tie across the join, and 0 / 0 stays 0 / 0
  const std::vector<int> tie = {5, 0, 0, 7};
  const m3t_tex_best2 j = Joined(tie, {0, 2, 4});
  CHECK(j.d0 == 0 && j.d1 == 0 && j.i0 == 1);
  const std::vector<int> later_best = {4, 3, 1, 2};
  const m3t_tex_best2 k = Joined(later_best, {0, 2, 4});
  CHECK(k.d0 == 1 && k.d1 == 2 && k.i0 == 2);
  m3t_tex_best2 none, other;
  m3t_tex_best2_init(&none);
  m3t_tex_best2_init(&other);
  m3t_tex_best2_append(&none, &other);
  CHECK(none.d0 == INT32_MAX && none.d1 == INT32_MAX && none.i0 == -1);
  CHECK(!m3t_tex_ratio_keeps(&none, 0.75f));
}

static void CheckPlan() {
  using namespace m3t_texture;
  CHECK(kAuto == 0 && kOneWorkgroup == 1 && kTiled == 2);
  CHECK(ParseMatchMode(nullptr) == kAuto && ParseMatchMode("") == kAuto && ParseMatchMode("auto") == kAuto);
  CHECK(ParseMatchMode("one") == kOneWorkgroup && ParseMatchMode("tiled") == kTiled);
  CHECK(ParseMatchMode("ONE") == kAuto && ParseMatchMode("one ") == kAuto && ParseMatchMode("2") == kAuto);
  CHECK(kMatchThreads == M3T_TEXTURE_MATCH_THREADS && kQueryTile == M3T_TEXTURE_QUERY_TILE);
  CHECK(kMaxFeatures == M3T_TEXTURE_MAX_FEATURES && kMaxKeyframes == M3T_TEXTURE_MAX_KEYFRAMES);
  CHECK(kQueryTiles == 64 && kBestBytes == sizeof(m3t_tex_best2));
  CHECK(kAutoForm == kOneWorkgroup || kAutoForm == kTiled);
  for (int mode = kAuto; mode <= kTiled; ++mode) {
    const int form = mode == kAuto ? int(kAutoForm) : mode;
    for (int keyframes : {1, 8}) {
      // no Hamming modality (an empty context, or L2 modalities alone): nothing is launched, nothing allocated
      const MatchPlan none = PlanMatch(mode, 0, keyframes);
      CHECK(none.form == 0 && none.match.x == 0 && none.match.y == 0 && none.collect.x == 0 && none.collect.y == 0 &&
            none.scratch_bytes == 0);
      for (int n : {1, 64}) {
        const MatchPlan p = PlanMatch(mode, n, keyframes);
        CHECK(p.form == form);
        CHECK(p.match.x == n);
        if (form == kOneWorkgroup) {
          CHECK(p.match.y == 1 && p.collect.x == 0 && p.collect.y == 0 && p.scratch_bytes == 0);
        } else {
          CHECK(p.match.y == keyframes * 64);  // ring slots x tiles of 64 queries out of 4096
          CHECK(p.collect.x == n && p.collect.y == 1);
          CHECK(p.scratch_bytes == size_t(keyframes) * 4096 * 12);
          CHECK(p.match.y <= 65535);  // the y dimension of a grid
        }
      }
    }
  }
  // the L2 modalities of a context do not count: with none but L2 ones the Hamming plan is empty in every mode (above);
  // beside L2 ones the Hamming modalities alone size the grid
  CHECK(PlanMatch(kTiled, 2, 3).match.x == 2 && PlanMatch(kTiled, 2, 3).match.y == 3 * 64);
  // n_keyframes outside [1, 8] cannot come from a modality that was created; the plan stays inside the scratch's cap
  CHECK(PlanMatch(kTiled, 1, 0).match.y == 64 && PlanMatch(kTiled, 1, 9).match.y == 8 * 64);
}

int main() {
  CheckAppend();
  CheckPlan();
  std::printf("checks %d errors %d\n", g_checks, g_errors);
  return g_errors != 0;
}
