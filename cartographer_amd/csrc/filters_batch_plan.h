// The host's plan of one cmx_filter_batch call (filters_batch.hip), and the sizes of the
// one-workgroup filter that the plan and the kernels (filters_small_device.h) have in common.
// Plain C++17 without HIP types or CMX_REQUIRE (a failure goes to a callback, the call site words
// the error), pinned on the host by tests/test_abi_filter_batch.py
// (tests/native/filter_batch_plan_check.cc).
//
// A call is a forest of depth two at most: roots filter host clouds, a chained job filters the
// output of a root.  Roots of up to kSmallCloud points and their children are batched: the roots
// are stage 0, the children stage 1, and a stage is at most two launches -- dynamic LDS is per
// launch and sized for the largest N in it, and with 1024 threads a compute unit holds two
// workgroups, so the only line that changes occupancy is N <= 2048 against N = 4096.  Families
// whose staged clouds or result slots would pass `byte_bound` together go out as consecutive
// sets (CutSets), a family never split.  A larger root and its children run single.
#ifndef CMX_FILTERS_BATCH_PLAN_H_
#define CMX_FILTERS_BATCH_PLAN_H_
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

#include "../../include/cartographer_mi355x.h"
#include "cmx_batch.h"

namespace cmx {

constexpr int kSmallCloud = 4096;         // most points of a cloud one workgroup filters
constexpr int kSmallThreads = 1024;
constexpr int kFilterMaxPoints = 1 << 26;
constexpr int kTwoPerUnitN = 2048;        // the largest N of which a compute unit holds two workgroups
constexpr long long kFilterSetBytes = 32ll << 20;   // staged clouds / result slots of one set

// The filter's arrays for N = the cloud's size rounded up to a power of two (SmallFilterLds),
// (N = 4096: 128 KB of arrays + the kernel's 20 KB active list and result flags: under the 160 KB)
CMX_BATCH_HD size_t SmallFilterLdsBytes(int N) {
  return static_cast<size_t>(N) * (8 + 4 + 5 * 4) + 64 * 4 + 64;
}
// ... and the dynamic LDS of a launch: behind them the active list and the best result's flags.
CMX_BATCH_HD size_t SmallFilterLaunchLds(int N) {
  return SmallFilterLdsBytes(N) + static_cast<size_t>(N) * 5 + 64;
}
inline int SmallFilterN(int n) {
  int N = 64;
  while (N < n) N <<= 1;
  return N;
}

// The argument checks of cmx_filter_batch that name a job: fail(job, what) for the first that
// does not hold, and false.
template <class Fail>
bool CheckFilterJobs(const cmx_filter_job* jobs, int num, Fail&& fail) {
  std::vector<char> used(num, 0);
  std::unordered_map<const float*, int> count_of;
  for (int k = 0; k < num; ++k) {
    const cmx_filter_job& J = jobs[k];
    const auto bad = [&](const char* what) { fail(k, what); return false; };
    if (J.mode != CMX_FILTER_VOXEL && J.mode != CMX_FILTER_ADAPTIVE) return bad("unknown mode");
    if (!(J.length > 0.f)) return bad("length must be > 0");
    if (J.num_points < 0 || J.num_points > kFilterMaxPoints) return bad("bad num_points");
    if (J.input_job < 0) {
      if (J.input_job != -1) return bad("input_job must be -1 or the index of an earlier job");
      if (J.num_points > 0 && !J.point_cloud_xyz) return bad("null point_cloud_xyz");
      if (J.num_points > 0) {
        const auto [at, fresh] = count_of.emplace(J.point_cloud_xyz, J.num_points);
        if (!fresh && at->second != J.num_points)
          return bad("point_cloud_xyz is the cloud of an earlier job with another num_points");
      }
    } else {
      if (J.point_cloud_xyz || J.num_points != 0)
        return bad("a chained job takes no point_cloud_xyz and no num_points");
      if (J.input_job >= k) return bad("input_job must be an earlier job");
      if (jobs[J.input_job].input_job != -1) return bad("input_job must not be a chained job");
      used[J.input_job] = 1;
    }
  }
  for (int k = 0; k < num; ++k)
    if (!jobs[k].kept_indices && !jobs[k].filtered_xyz && !used[k]) {
      fail(k, "no output pointer and no job chained on it");
      return false;
    }
  return true;
}

struct FilterJobPlan {
  int root = 0;            // the job itself, or the job it is chained on
  int set = -1;            // set of launches; -1: takes no workgroup (runs single, or has no input)
  int stage = 0;           // 0: a root, 1: chained
  int launch = -1;         // of its stage: 0 (N <= 2048) or 1 (N = 4096)
  int slot = -1;           // its descriptor in the table of its set
  int N = 0;               // the LDS carve: a root's points rounded up to a power of two, at least 64;
                           // a chained job takes its root's
  long long lds_bytes = 0;
  int cloud_slot = -1;     // a root with points: its cloud among the distinct clouds of the call
  bool single = false;     // through the multi-launch path: a root above kSmallCloud and its children
  bool batched = false;    // takes a workgroup: a root of 1 .. kSmallCloud points and its children
};

struct FilterLaunchPlan {
  int first = 0, count = 0;   // descriptors of the set's table
  int N = 0;                  // the largest of them
};

struct FilterSetPlan {
  std::vector<int> jobs;               // by slot
  FilterLaunchPlan launch[2][2];       // [stage][launch]
  long long staged_floats = 0;         // the distinct clouds of its roots
};

struct FilterBatchPlan {
  std::vector<FilterJobPlan> jobs;
  std::vector<std::vector<int>> children;   // by job
  std::vector<FilterSetPlan> sets;
  std::vector<int> single_roots;
  int num_launches = 0;
  long long staged_bytes = 0;
};

// What a family adds to the pinned result block of its set.
inline long long FilterResultBytes(const cmx_filter_job& J, int root_points) {
  long long bytes = 0;
  if (J.kept_indices) bytes += static_cast<long long>(Align256(4 * static_cast<size_t>(root_points)));
  if (J.filtered_xyz) bytes += static_cast<long long>(Align256(12 * static_cast<size_t>(root_points)));
  return bytes;
}

// `jobs` have passed CheckFilterJobs.
inline FilterBatchPlan PlanFilterBatch(const cmx_filter_job* jobs, int num, long long byte_bound) {
  FilterBatchPlan plan;
  plan.jobs.resize(num);
  plan.children.resize(num);
  std::unordered_map<const float*, int> slot_of_cloud;
  std::vector<int> batched;                // roots that take a workgroup, in list order
  for (int k = 0; k < num; ++k) {
    const cmx_filter_job& J = jobs[k];
    FilterJobPlan& P = plan.jobs[k];
    if (J.input_job >= 0) {
      const FilterJobPlan& R = plan.jobs[J.input_job];
      plan.children[J.input_job].push_back(k);
      P.root = J.input_job;
      P.stage = 1;
      P.single = R.single;
      P.batched = R.batched;
      if (P.batched) { P.N = R.N; P.lds_bytes = R.lds_bytes; P.launch = R.launch; }
      continue;
    }
    P.root = k;
    if (J.num_points == 0) continue;
    P.cloud_slot =
        slot_of_cloud.emplace(J.point_cloud_xyz, static_cast<int>(slot_of_cloud.size())).first->second;
    if (J.num_points > kSmallCloud) {
      P.single = true;
      plan.single_roots.push_back(k);
      continue;
    }
    P.batched = true;
    P.N = SmallFilterN(J.num_points);
    P.lds_bytes = static_cast<long long>(SmallFilterLaunchLds(P.N));
    P.launch = P.N <= kTwoPerUnitN ? 0 : 1;
    batched.push_back(k);
  }
  // One round: the families in list order, a set cut where the staged clouds or the result slots
  // would pass the bound.
  const std::vector<int> one_round(batched.size(), 0);
  const long long bound[3] = {byte_bound, byte_bound, 1ll << 30};
  const std::vector<LaunchSet> cuts = CutSets(
      one_round, 1 << 30, bound,
      [&](int b, long long* add) {
        const int r = batched[b];
        const int n = jobs[r].num_points;
        add[0] = 12ll * n;
        add[1] = 256 + FilterResultBytes(jobs[r], n);
        for (int c : plan.children[r]) add[1] += 256 + FilterResultBytes(jobs[c], n);
        add[2] = 1 + static_cast<long long>(plan.children[r].size());
      },
      [](int, int, const long long*) {});
  for (const LaunchSet& cut : cuts) {
    FilterSetPlan set;
    const int s = static_cast<int>(plan.sets.size());
    StagedArrays clouds(3);
    for (int b = cut.begin; b < cut.end; ++b)
      clouds.Add(batched[b], jobs[batched[b]].point_cloud_xyz, jobs[batched[b]].num_points,
                 [](int, int, int) {});
    set.staged_floats = static_cast<long long>(clouds.floats());
    for (int stage = 0; stage < 2; ++stage) {
      for (int launch = 0; launch < 2; ++launch) {
        FilterLaunchPlan& L = set.launch[stage][launch];
        L.first = static_cast<int>(set.jobs.size());
        const auto take = [&](int k) {
          FilterJobPlan& P = plan.jobs[k];
          if (!P.batched || P.launch != launch) return;
          P.set = s;
          P.slot = static_cast<int>(set.jobs.size());
          set.jobs.push_back(k);
          L.N = std::max(L.N, P.N);
        };
        for (int b = cut.begin; b < cut.end; ++b) {
          if (stage == 0) {
            take(batched[b]);
          } else {
            for (int c : plan.children[batched[b]]) take(c);
          }
        }
        L.count = static_cast<int>(set.jobs.size()) - L.first;
        if (L.count > 0) ++plan.num_launches;
      }
    }
    plan.staged_bytes += 4 * set.staged_floats;
    plan.sets.push_back(std::move(set));
  }
  return plan;
}

}  // namespace cmx
#endif  // CMX_FILTERS_BATCH_PLAN_H_
