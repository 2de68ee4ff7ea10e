// FastCorrelativeScanMatcher2D on gfx950: lists of (node, submap) pairs, every pair with a cloud
// of its own -- the burst of PoseGraph2D::ComputeConstraintsForNode when a submap finishes
// (mapping/internal/2d/pose_graph_2d.cc:383-393: every old node against the new submap).
//
// Every search kernel and the front end take the cloud and its point count as launch-wide
// arguments (the fused front end sizes its LDS from that count), so pairs of different clouds do
// not share launches.  What this unit does instead is host-side: the pairs are grouped by
// (cloud, branch_and_bound_depth) -- a group is exactly what MatchBatch takes, so the pairs of one
// node share that node's launches as in cmx_fast2d_match_batch -- and several groups run as
// independent MatchBatch calls over the host pool, each on a workspace and stream of its own:
// the mechanism batches of 32 and more full-submap searches already use (fast_2d_match.hip).
// No kernel lives here.
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "fast_2d_internal.h"

namespace cmx {
namespace {

// The cloud of one pair: a host array (uploaded by the call) or a resident cmx_cloud.
struct PairCloud {
  const float* host = nullptr;
  const cmx_cloud* resident = nullptr;
  int n = 0;
  const void* key() const { return resident ? static_cast<const void*>(resident) : host; }
};

struct Group {
  PairCloud cloud;
  std::vector<int> pairs;                 // indices into the call's list, ascending
  std::vector<const cmx_fast2d*> handles;
  std::vector<cmx_pose2d> initial, poses;
  std::vector<int32_t> full, found;
  std::vector<float> min_scores, scores;
  cmx_match_stats stats{};
};

void MatchPairs(const cmx_fast2d* const* matchers, int num_pairs, const cmx_pose2d* initial,
                const int32_t* full, const float* min_scores, const std::vector<PairCloud>& clouds,
                int32_t* found, float* scores, cmx_pose2d* poses, cmx_match_stats* stats) {
  CMX_REQUIRE(matchers && full && min_scores && found && scores && poses, "null argument");
  // Everything that can be refused is refused here, in pair order, before anything is launched.
  std::map<const void*, int> points_of;
  int device = 0;
  for (int p = 0; p < num_pairs; ++p) {
    CMX_REQUIRE(matchers[p] != nullptr && matchers[p]->impl, "null matcher handle (pair %d)", p);
    if (p == 0) device = matchers[0]->impl->device();
    CMX_REQUIRE(matchers[p]->impl->device() == device,
                "the matchers of a call must live on one device (pair %d)", p);
    const PairCloud& c = clouds[p];
    CMX_REQUIRE(c.key() != nullptr, "the point cloud of pair %d is null", p);
    CMX_REQUIRE(c.n >= 1, "empty point cloud (pair %d)", p);
    CMX_REQUIRE(c.n <= (1 << 24), "point cloud too large (pair %d)", p);
    CMX_REQUIRE(!c.resident || c.resident->device == device,
                "cloud and matcher are on different devices (pair %d)", p);
    CMX_REQUIRE(full[p] != 0 || initial != nullptr,
                "initial_pose_estimates required for windowed searches (pair %d)", p);
    const auto seen = points_of.emplace(c.key(), c.n);
    CMX_REQUIRE(seen.first->second == c.n,
                "pair %d names a cloud of an earlier pair with another num_points (%d, there %d)",
                p, c.n, seen.first->second);
  }
  // Groups by (cloud, depth), in the order their first pairs appear.
  std::vector<Group> groups;
  std::map<std::pair<const void*, int>, int> group_of;
  for (int p = 0; p < num_pairs; ++p) {
    const auto key = std::make_pair(clouds[p].key(), matchers[p]->impl->depth());
    auto it = group_of.find(key);
    if (it == group_of.end()) {
      it = group_of.emplace(key, static_cast<int>(groups.size())).first;
      groups.emplace_back();
      groups.back().cloud = clouds[p];
    }
    Group& g = groups[it->second];
    g.pairs.push_back(p);
    g.handles.push_back(matchers[p]);
    g.initial.push_back(initial ? initial[p] : cmx_pose2d{0., 0., 0.});
    g.full.push_back(full[p]);
    g.min_scores.push_back(min_scores[p]);
  }
  const int num_groups = static_cast<int>(groups.size());
  for (Group& g : groups) {
    g.found.assign(g.pairs.size(), 0);
    g.scores.assign(g.pairs.size(), 0.f);
    g.poses.assign(g.pairs.size(), cmx_pose2d{0., 0., 0.});
  }
  // A host cloud goes up once per distinct pointer.  One that a single group names is uploaded by
  // that group's MatchBatch, on the group's stream; one that groups of several depths name goes
  // up here, once, and those groups read it as a resident cloud.
  std::map<const float*, int> groups_of_host;
  for (const Group& g : groups)
    if (g.cloud.host) ++groups_of_host[g.cloud.host];
  std::unique_ptr<WorkspaceLease> upload_ws;
  std::vector<std::unique_ptr<cmx_cloud>> uploaded;
  {
    const auto padded = [](int n) { return (3 * static_cast<size_t>(n) + 63) & ~size_t(63); };
    size_t floats = 0;
    for (const auto& kv : groups_of_host)
      if (kv.second > 1) floats += padded(points_of[kv.first]);
    if (floats) {
      upload_ws.reset(new WorkspaceLease(device));
      Workspace& ws = **upload_ws;
      float* base = ws.dev[0].ReserveAs<float>(floats);
      std::map<const float*, const cmx_cloud*> resident_of;
      size_t at = 0;
      for (const auto& kv : groups_of_host) {
        if (kv.second <= 1) continue;
        const int n = points_of[kv.first];
        CMX_HIP(hipMemcpyAsync(base + at, kv.first, 3 * sizeof(float) * n, hipMemcpyHostToDevice,
                               ws.stream));
        std::unique_ptr<cmx_cloud> c(new cmx_cloud);
        c->device = device;
        c->num_points = n;
        c->xyz = base + at;
        c->max_range_xy = MaxRangeXY(kv.first, n);
        resident_of[kv.first] = c.get();
        uploaded.push_back(std::move(c));
        at += padded(n);
      }
      CMX_HIP(hipStreamSynchronize(ws.stream));
      for (Group& g : groups) {
        const auto it = g.cloud.host ? resident_of.find(g.cloud.host) : resident_of.end();
        if (it == resident_of.end()) continue;
        g.cloud.resident = it->second;
        g.cloud.host = nullptr;
      }
    }
  }
  const auto run = [&](int k, bool allow_fanout) {
    Group& g = groups[k];
    MatchBatch(g.handles.data(), static_cast<int>(g.pairs.size()), g.initial.data(), false,
               g.cloud.host, g.cloud.resident, g.cloud.n, 0.f, g.found.data(), g.scores.data(),
               g.poses.data(), &g.stats, g.full.data(), g.min_scores.data(), allow_fanout);
  };
  if (num_groups == 1) {
    // The equivalent cmx_fast2d_match_batch, launch for launch.
    run(0, /*allow_fanout=*/true);
  } else if (OverrideStream(device) != nullptr) {
    // The override is the calling thread's: the groups one after the other on that stream.  The
    // first group to fail is the one with the lowest pair index (groups are in that order).
    for (int k = 0; k < num_groups; ++k) run(k, /*allow_fanout=*/false);
  } else {
    // Independent searches over the host pool.  A group runs inside the pool, so it does not fan
    // out again; an error is kept with the text its thread left (the last error is per thread).
    std::vector<cmx_status> status(num_groups, CMX_OK);
    std::vector<std::string> message(num_groups);
    ParallelFor(num_groups, 2, [&](int k) {
      status[k] = Guard([&] { run(k, /*allow_fanout=*/false); });
      if (status[k] != CMX_OK) message[k] = LastError();
    });
    for (int k = 0; k < num_groups; ++k) {
      if (status[k] == CMX_OK) continue;
      SetLastError("%s", message[k].c_str());
      throw HipError{status[k]};
    }
  }
  cmx_match_stats total{};
  for (const Group& g : groups) {
    for (size_t k = 0; k < g.pairs.size(); ++k) {
      const int p = g.pairs[k];
      found[p] = g.found[k];
      if (!g.found[k]) continue;        // (as the single calls: score and pose are left alone)
      scores[p] = g.scores[k];
      poses[p] = g.poses[k];
    }
    AddMatchStats(g.stats, &total);
  }
  if (stats) *stats = total;
}

}  // namespace
}  // namespace cmx

using cmx::Guard;

extern "C" {

cmx_status cmx_fast2d_match_pairs(const cmx_fast2d* const* matchers, int32_t num_pairs,
                                  const cmx_pose2d* initial_pose_estimates,
                                  const int32_t* match_full_submap, const float* min_scores,
                                  const float* const* point_clouds_xyz, const int32_t* num_points,
                                  int32_t* found, float* scores, cmx_pose2d* pose_estimates,
                                  cmx_match_stats* stats) {
  return Guard([&] {
    // (a matcher handle cannot exist without a device: say so, whatever the arguments are)
    if (cmx_device_count() <= 0) cmx::UseDevice(0);
    CMX_REQUIRE(num_pairs >= 1, "num_pairs must be at least 1");
    CMX_REQUIRE(point_clouds_xyz && num_points, "null argument");
    std::vector<cmx::PairCloud> clouds(num_pairs);
    for (int p = 0; p < num_pairs; ++p) {
      clouds[p].host = point_clouds_xyz[p];
      clouds[p].n = num_points[p];
    }
    cmx::MatchPairs(matchers, num_pairs, initial_pose_estimates, match_full_submap, min_scores,
                    clouds, found, scores, pose_estimates, stats);
  });
}

cmx_status cmx_fast2d_match_pairs_resident(const cmx_fast2d* const* matchers, int32_t num_pairs,
                                           const cmx_pose2d* initial_pose_estimates,
                                           const int32_t* match_full_submap,
                                           const float* min_scores,
                                           const cmx_cloud* const* clouds, int32_t* found,
                                           float* scores, cmx_pose2d* pose_estimates,
                                           cmx_match_stats* stats) {
  return Guard([&] {
    if (cmx_device_count() <= 0) cmx::UseDevice(0);
    CMX_REQUIRE(num_pairs >= 1, "num_pairs must be at least 1");
    CMX_REQUIRE(clouds, "null argument");
    std::vector<cmx::PairCloud> list(num_pairs);
    for (int p = 0; p < num_pairs; ++p) {
      list[p].resident = clouds[p];
      list[p].n = clouds[p] ? clouds[p]->num_points : 0;
    }
    cmx::MatchPairs(matchers, num_pairs, initial_pose_estimates, match_full_submap, min_scores,
                    list, found, scores, pose_estimates, stats);
  });
}

}  // extern "C"
