// The host's plan of one cmx_ceres2d_match_grid_batch call (ceres_2d.hip): the checks of the
// job list that need no grid, and the layout of the call's one upload block -- the problem array
// followed by one slot per distinct host cloud.  Plain C++17 without HIP types or CMX_REQUIRE (a
// failure goes to a callback, the call site words the error), pinned on the host by
// tests/test_ceres2d_batch_plan.py (tests/native/ceres2d_batch_plan_check.cc).
//
// A job is one workgroup of the one launch, whatever its kind (Ceres2DJobKernel branches on the
// kind, uniformly across the workgroup): the number of launches does not depend on the list.
// Host clouds are staged once per distinct pointer, in first-seen order; a resident cloud and
// the empty cloud of a TSDF job are read where they lie (nowhere) and take no slot.
#ifndef CMX_CERES_2D_BATCH_PLAN_H_
#define CMX_CERES_2D_BATCH_PLAN_H_
#include <stddef.h>

#include <unordered_map>
#include <vector>

#include "cmx_batch.h"

namespace cmx {

constexpr int kCeres2DMaxPoints = 1 << 24;
constexpr int kCeres2DBatchLaunches = 1;
enum Ceres2DKind { kCeres2DProbabilityGrid = 0, kCeres2DTsdf = 1 };

// What the plan reads of a job: its kind, where its cloud comes from and how many points it has
// (a resident cloud's own count).
struct Ceres2DJobShape {
  int kind = kCeres2DProbabilityGrid;
  const float* host_xyz = nullptr;   // the job's point_cloud_xyz: an identity, never read here
  bool resident = false;             // the job names an uploaded cloud
  int num_points = 0;
};

// The argument checks of cmx_ceres2d_match_grid_batch that the shapes decide: fail(job, what) for
// the first that does not hold, and false.
template <class Fail>
bool CheckCeres2DJobShapes(const Ceres2DJobShape* shapes, int num, Fail&& fail) {
  std::unordered_map<const float*, int> count_of;
  for (int k = 0; k < num; ++k) {
    const Ceres2DJobShape& S = shapes[k];
    const auto bad = [&](const char* what) { fail(k, what); return false; };
    if (S.kind != kCeres2DProbabilityGrid && S.kind != kCeres2DTsdf) return bad("unknown grid kind");
    const bool tsdf = S.kind == kCeres2DTsdf;
    if (S.resident && S.host_xyz) return bad("both point_cloud_xyz and cloud are set");
    // A TSDF takes an empty cloud (the functor fails on it: FAILURE, as in the single call).
    if (S.num_points < (tsdf ? 0 : 1) || S.num_points > kCeres2DMaxPoints)
      return bad(tsdf ? "the point count must be 0 .. 2^24" : "the point count must be 1 .. 2^24");
    if (!S.resident && !S.host_xyz && S.num_points > 0)
      return bad("neither point_cloud_xyz nor cloud is set");
    if (!S.resident && S.host_xyz && S.num_points > 0) {
      const auto [at, fresh] = count_of.emplace(S.host_xyz, S.num_points);
      if (!fresh && at->second != S.num_points)
        return bad("point_cloud_xyz is the cloud of an earlier job with another point count");
    }
  }
  return true;
}

struct Ceres2DJobPlan {
  int kind = kCeres2DProbabilityGrid;
  int cloud_slot = -1;               // a host cloud with points: which of the call's distinct clouds
  size_t cloud_at = 0;               // ... and its byte offset in the upload block
};

struct Ceres2DCloudSlot {
  const float* host_xyz = nullptr;
  int num_points = 0;
  size_t at = 0;
};

struct Ceres2DBatchPlan {
  std::vector<Ceres2DJobPlan> jobs;          // in list order
  std::vector<Ceres2DCloudSlot> clouds;      // in first-seen order
  size_t problem_bytes = 0;                  // the problem array, to a 256-byte boundary
  size_t total_bytes = 0;                    // of the upload block
  int num_launches = kCeres2DBatchLaunches;
};

// `shapes` have passed CheckCeres2DJobShapes; problem_size: the bytes of one problem descriptor.
inline Ceres2DBatchPlan PlanCeres2DBatch(const Ceres2DJobShape* shapes, int num,
                                         size_t problem_size) {
  Ceres2DBatchPlan plan;
  plan.jobs.resize(num);
  BlockLayout layout;
  layout.Add<char>(problem_size * static_cast<size_t>(num));
  plan.problem_bytes = layout.bytes;
  std::unordered_map<const float*, int> slot_of;
  for (int k = 0; k < num; ++k) {
    const Ceres2DJobShape& S = shapes[k];
    Ceres2DJobPlan& P = plan.jobs[k];
    P.kind = S.kind;
    if (S.resident || S.num_points == 0) continue;
    const auto [at, fresh] = slot_of.emplace(S.host_xyz, static_cast<int>(plan.clouds.size()));
    if (fresh) {
      const BlockRegion<float> region = layout.Add<float>(3 * static_cast<size_t>(S.num_points));
      plan.clouds.push_back(Ceres2DCloudSlot{S.host_xyz, S.num_points, region.at});
    }
    P.cloud_slot = at->second;
    P.cloud_at = plan.clouds[P.cloud_slot].at;
  }
  plan.total_bytes = layout.bytes;
  return plan;
}

}  // namespace cmx
#endif  // CMX_CERES_2D_BATCH_PLAN_H_
