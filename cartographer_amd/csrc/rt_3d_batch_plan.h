// The host's plan of one cmx_rt3d_match_grid_batch call (rt_3d_batch.hip): the search window of
// every match (what BuildSearchSpace of rt_3d.hip computes before it fills its tables -- it asks
// the function below), the route every match takes and how the matches of the segmented route are
// cut into launch sets.  Plain C++17 without HIP types or CMX_REQUIRE, pinned on the host by
// tests/test_rt3d_batch_plan.py (tests/native/rt3d_batch_plan_check.cc).
//
// Segmented route.  One thread per candidate, a block of 64 threads = 64 translations of one
// rotation (Rt3DScoreKernel's wavefront): a match of T translations and R rotations takes
// R * ceil(T / 64) consecutive blocks of the score launch, and the same blocks of the collect
// launch.  A set of launches is cut (CutSets) where
//   * its blocks would pass 2^31 - 1 (block indices are 32-bit ints, and a launch takes no more),
//   * its candidates would pass kRt3DSetCandidates: every candidate keeps an unweighted and a
//     weighted f32 score, 8 bytes, so 2^25 candidates are the 256 MB a set may hold in scratch,
//   * its upload block (tables and staged clouds) would pass kRt3DSetStagedBytes, 64 MB of pinned
//     memory.
// A match that exceeds a bound alone is a set of its own.
#ifndef CMX_RT_3D_BATCH_PLAN_H_
#define CMX_RT_3D_BATCH_PLAN_H_
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "../../include/cartographer_mi355x.h"
#include "cmx_batch.h"

namespace cmx {

constexpr int kRt3DBatchLanes = 64;                       // candidates (translations) per block
constexpr long long kRt3DSetBlocks = 0x7fffffffll;
constexpr long long kRt3DSetCandidates = 1ll << 25;
constexpr long long kRt3DSetStagedBytes = 64ll << 20;
// Most work (candidates x points) of a match on the segmented route.  Measured, not reasoned: the
// route sweep of profiles/rt3d_batch_timing.json ("In batches") has single matches
// of growing work on both routes on one MI355X.  The segmented route is 3.3x faster at 4.3e7
// (42 875 candidates x 1000 points: 0.24 against 0.79 ms) and 1.4x slower at 3.5e8 (x 8192 points:
// 1.67 against 1.20 ms); 2^25 is the largest power of two not above the last size at which it was
// not slower.
constexpr long long kRt3DSegmentedMaxWork = 1ll << 25;

enum Rt3DBatchRoute { kRt3DRouteSegmented = 0, kRt3DRouteSingle = 1 };

// GenerateExhaustiveSearchTransforms' window (SM3/real_time_correlative_scan_matcher_3d.cc:55-75)
// in steps; `unsupported`: the limit of this library it exceeds, or null.
struct Rt3DWindow {
  int L = 0, A = 0;                  // linear / angular window in steps
  float step = 0.f;                  // angular step
  long long T = 0, R = 0, num_candidates = 0;
  const char* unsupported = nullptr;
};

// max(3 resolution, the largest point norm), in the reference's order of operations.
inline float Rt3DScanRange(float resolution, const float* xyz, int n) {
  float max_scan_range = 3.f * resolution;
  for (int i = 0; i < n; ++i) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const float norm = std::sqrt((x * x + y * y) + z * z);
    max_scan_range = std::max(norm, max_scan_range);
  }
  return max_scan_range;
}

inline Rt3DWindow Rt3DWindowOf(const cmx_rt_options& options, float resolution,
                               float max_scan_range) {
  Rt3DWindow W;
  W.L = static_cast<int>(std::lround(options.linear_search_window / resolution));
  const float kSafetyMargin = 1.f - 1e-3f;
  W.step = kSafetyMargin * std::acos(1.f - (resolution * (resolution * 1.f)) /
                                               (2.f * (max_scan_range * (max_scan_range * 1.f))));
  W.A = static_cast<int>(std::lround(options.angular_search_window / W.step));
  if (!(W.L >= 0 && W.L < 512 && W.A >= 0 && W.A < 64)) {
    W.unsupported = "unsupported search window";
    return W;
  }
  const long long side_t = 2 * W.L + 1, side_r = 2 * W.A + 1;
  W.T = side_t * side_t * side_t;
  W.R = side_r * side_r * side_r;
  W.num_candidates = W.T * W.R;
  if (!(W.num_candidates < (1ll << 31))) W.unsupported = "search window too large";
  return W;
}

inline long long Rt3DBatchBlocks(const Rt3DWindow& W) {
  return W.R * BlocksOf(W.T, kRt3DBatchLanes);
}
// What a match adds to its set's upload block at most: descriptor and head, rotation (16) +
// angle (4) per rotation, translation (16), its cloud (a cloud shared by pointer is staged once
// and counted with every match that names it).
inline long long Rt3DBatchStagedBytes(const Rt3DWindow& W, int num_points) {
  return 512 + 20 * W.R + 16 * W.T + 12ll * num_points;
}

struct Rt3DMatchInput {
  Rt3DWindow window;               // supported
  int num_points = 0;
  bool finite = true;              // no coordinate of the cloud is NaN or infinite
  bool brick_in_reach = true;      // the grid's brick can be read through 32-bit byte offsets
};

struct Rt3DMatchPlan {
  int route = kRt3DRouteSingle;
  int set = -1;                    // segmented route: its launch set,
  int slot = -1;                   // its descriptor among all of the call's (sets back to back),
  int first_block = 0, blocks = 0; // and its blocks in either launch of the set
};

struct Rt3DBatchPlan {
  std::vector<Rt3DMatchPlan> matches;
  std::vector<LaunchSet> sets;     // total[0] blocks, [1] candidates, [2] staged bytes
  std::vector<int> match_of_slot;
  std::vector<int> singles;        // in list order
};

struct Rt3DBatchBounds {
  long long blocks = kRt3DSetBlocks, candidates = kRt3DSetCandidates,
            staged_bytes = kRt3DSetStagedBytes, max_work = kRt3DSegmentedMaxWork;
};

// route_switch: the debug switch rt3d_batch_route (0 by size, 1 every finite cloud segmented,
// 2 every match single).
inline int Rt3DRouteOf(const Rt3DMatchInput& in, int route_switch, long long max_work) {
  if (route_switch == 2 || !in.finite || !in.brick_in_reach) return kRt3DRouteSingle;
  if (route_switch == 1) return kRt3DRouteSegmented;
  return in.window.num_candidates * in.num_points <= max_work ? kRt3DRouteSegmented
                                                              : kRt3DRouteSingle;
}

inline Rt3DBatchPlan PlanRt3DBatch(const Rt3DMatchInput* in, int num, int route_switch,
                                   const Rt3DBatchBounds& bounds = Rt3DBatchBounds()) {
  Rt3DBatchPlan plan;
  plan.matches.resize(num);
  std::vector<int> segmented;
  for (int k = 0; k < num; ++k) {
    plan.matches[k].route = Rt3DRouteOf(in[k], route_switch, bounds.max_work);
    if (plan.matches[k].route == kRt3DRouteSegmented) segmented.push_back(k);
    else plan.singles.push_back(k);
  }
  const std::vector<int> one_round(segmented.size(), 0);
  const long long bound[3] = {bounds.blocks, bounds.candidates, bounds.staged_bytes};
  plan.match_of_slot.resize(segmented.size());
  plan.sets = CutSets(
      one_round, 1 << 30, bound,
      [&](int s, long long* add) {
        const Rt3DMatchInput& I = in[segmented[s]];
        add[0] = Rt3DBatchBlocks(I.window);
        add[1] = I.window.num_candidates;
        add[2] = Rt3DBatchStagedBytes(I.window, I.num_points);
      },
      [&](int s, int slot, const long long* first) {
        Rt3DMatchPlan& P = plan.matches[segmented[s]];
        P.slot = slot;
        P.first_block = static_cast<int>(first[0]);
        P.blocks = static_cast<int>(Rt3DBatchBlocks(in[segmented[s]].window));
        plan.match_of_slot[slot] = segmented[s];
      });
  for (size_t s = 0; s < plan.sets.size(); ++s)
    for (int slot = plan.sets[s].begin; slot < plan.sets[s].end; ++slot)
      plan.matches[plan.match_of_slot[slot]].set = static_cast<int>(s);
  return plan;
}

}  // namespace cmx
#endif  // CMX_RT_3D_BATCH_PLAN_H_
