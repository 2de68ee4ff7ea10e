// The host's plan of one cmx_compute_histogram_batch call (histogram_batch.hip), and the sizes
// of the one-workgroup histogram that the plan and the kernel (histogram_batch_device.h) have in
// common.  Plain C++17 without HIP types or CMX_REQUIRE (a failure goes to a callback, the call
// site words the error), pinned on the host by tests/test_histogram_batch_plan.py
// (tests/native/histogram_batch_plan_check.cc).
//
// A job without points is done by the host (zeros).  A cloud of 1 .. kSmallCloud finite points
// takes one workgroup.  A larger cloud, or one with a non-finite coordinate, runs single.  The
// batched jobs of a call go out in sets (CutSets: the staged clouds and the result block of a
// set bounded by `byte_bound`), a set in one launch per class of N: dynamic LDS is per launch
// and sized for the largest N in it, so only the lines of N at which a compute unit holds
// another number of workgroups are worth a launch of their own.
#ifndef CMX_HISTOGRAM_BATCH_PLAN_H_
#define CMX_HISTOGRAM_BATCH_PLAN_H_
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>

#include "../../include/cartographer_mi355x.h"
#include "cmx_batch.h"
#include "filters_batch_plan.h"      // kSmallCloud, kSmallThreads, SmallFilterN

namespace cmx {

constexpr int kHistogramMaxPoints = 1 << 24;
constexpr int kHistogramMaxSize = 8192;
constexpr long long kHistogramSetBytes = 32ll << 20;   // staged clouds / result block of one set
constexpr long long kLdsPerUnit = 160 * 1024;          // of a gfx950 compute unit
// Workgroups of kSmallThreads a compute unit holds by the kernel's registers: 16 wavefronts are
// four per SIMD, a SIMD has 512 vector registers per lane, and the kernel takes 92, more than
// the 64 that eight wavefronts would leave each (the two 32-register banks of ChainSumLds alone
// are 64; DESIGN.md 5.6 has the compiler's figures).
constexpr int kHistogramWorkgroupsByRegisters = 1;

// The kernel's arrays for N = the cloud's size rounded up to a power of two (HistogramLds,
// histogram_batch_device.h): 64-bit sort keys, two pairs of coordinate rows, slice of every
// point, first point and end of the kept points of every slice; 64 wave totals and 64 bytes.
CMX_BATCH_HD size_t HistogramLdsBytes(int N) {
  return static_cast<size_t>(N) * (8 + 4 * 4 + 3 * 4) + 64 * 4 + 64;
}
inline int HistogramN(int n) { return SmallFilterN(n); }

// Workgroups of carve N that a compute unit holds, and the launch class of N: 0 for the
// smallest carves, one more behind every N at which that number changes.
inline int HistogramWorkgroupsPerUnit(int N) {
  const long long by_lds = kLdsPerUnit / static_cast<long long>(HistogramLdsBytes(N));
  return static_cast<int>(std::min<long long>(kHistogramWorkgroupsByRegisters, by_lds));
}
inline int HistogramLaunchClass(int N) {
  int cls = 0;
  for (int M = 64; M < N; M <<= 1)
    if (HistogramWorkgroupsPerUnit(M) != HistogramWorkgroupsPerUnit(2 * M)) ++cls;
  return cls;
}

inline bool CloudIsFinite(const float* xyz, int n) {
  // (an exponent of all ones is an infinity or a NaN; no branch in the loop, so it vectorises)
  uint32_t non_finite = 0;
  for (size_t i = 0; i < 3 * static_cast<size_t>(n); ++i) {
    uint32_t bits;
    memcpy(&bits, xyz + i, 4);
    non_finite |= (bits & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
  }
  return non_finite == 0;
}

// The argument checks of cmx_compute_histogram_batch that name a job: fail(job, what) for the
// first that does not hold, and false.
template <class Fail>
bool CheckHistogramJobs(const cmx_histogram_job* jobs, int num, Fail&& fail) {
  std::unordered_map<const float*, int> count_of;
  for (int k = 0; k < num; ++k) {
    const cmx_histogram_job& J = jobs[k];
    const auto bad = [&](const char* what) { fail(k, what); return false; };
    if (J.num_points < 0 || J.num_points > kHistogramMaxPoints) return bad("bad num_points");
    if (J.histogram_size < 1 || J.histogram_size > kHistogramMaxSize)
      return bad("histogram_size must be 1 .. 8192");
    if (!J.histogram) return bad("null histogram");
    if (J.num_points > 0 && !J.point_cloud_xyz) return bad("null point_cloud_xyz");
    if (J.num_points > 0) {
      const auto [at, fresh] = count_of.emplace(J.point_cloud_xyz, J.num_points);
      if (!fresh && at->second != J.num_points)
        return bad("point_cloud_xyz is the cloud of an earlier job with another num_points");
    }
  }
  return true;
}

enum HistogramRoute { kHistogramNone = 0, kHistogramBatched = 1, kHistogramSingle = 2 };

struct HistogramJobPlan {
  int route = kHistogramNone;
  int set = -1;            // batched: its set of launches
  int launch = -1;         // of its set
  int slot = -1;           // its descriptor in the table of its set
  int N = 0;               // the LDS carve: its points rounded up to a power of two, at least 64
  long long lds_bytes = 0;
  int cloud_slot = -1;     // with points: its cloud among the distinct clouds of the call
};

struct HistogramLaunchPlan {
  int first = 0, count = 0;   // descriptors of the set's table
  int N = 0;                  // the largest of them
  int cls = 0;
};

struct HistogramSetPlan {
  std::vector<int> jobs;                      // by slot
  std::vector<HistogramLaunchPlan> launches;  // those with jobs, classes ascending
  long long staged_floats = 0;                // the distinct clouds of its jobs
  long long result_bytes = 0;
};

struct HistogramBatchPlan {
  std::vector<HistogramJobPlan> jobs;
  std::vector<HistogramSetPlan> sets;
  std::vector<int> single_jobs;
  int num_launches = 0;
  long long staged_bytes = 0;
};

// What a job adds to the pinned result block of its set.
inline long long HistogramResultBytes(const cmx_histogram_job& J) {
  return static_cast<long long>(Align256(4 * static_cast<size_t>(J.histogram_size)));
}

// `jobs` have passed CheckHistogramJobs.  finite(k): whether the cloud of job k (1 ..
// kSmallCloud points) has finite coordinates only; asked once per distinct cloud.
template <class Finite>
HistogramBatchPlan PlanHistogramBatch(const cmx_histogram_job* jobs, int num, long long byte_bound,
                                      Finite&& finite) {
  HistogramBatchPlan plan;
  plan.jobs.resize(num);
  std::unordered_map<const float*, int> slot_of_cloud;
  std::vector<char> finite_of_slot;
  std::vector<int> batched;                // in list order
  for (int k = 0; k < num; ++k) {
    const cmx_histogram_job& J = jobs[k];
    HistogramJobPlan& P = plan.jobs[k];
    if (J.num_points == 0) continue;
    const auto [at, fresh] =
        slot_of_cloud.emplace(J.point_cloud_xyz, static_cast<int>(slot_of_cloud.size()));
    P.cloud_slot = at->second;
    if (fresh) finite_of_slot.push_back(J.num_points <= kSmallCloud && finite(k) ? 1 : 0);
    if (!finite_of_slot[P.cloud_slot]) {
      P.route = kHistogramSingle;
      plan.single_jobs.push_back(k);
      continue;
    }
    P.route = kHistogramBatched;
    P.N = HistogramN(J.num_points);
    P.lds_bytes = static_cast<long long>(HistogramLdsBytes(P.N));
    batched.push_back(k);
  }
  // One round: the jobs in list order, a set cut where the staged clouds (every job's counted:
  // an upper bound where jobs share one) or the result block would pass the bound.
  const std::vector<int> one_round(batched.size(), 0);
  const long long bound[3] = {byte_bound, byte_bound, 1ll << 30};
  const std::vector<LaunchSet> cuts = CutSets(
      one_round, 1 << 30, bound,
      [&](int b, long long* add) {
        add[0] = 12ll * jobs[batched[b]].num_points;
        add[1] = HistogramResultBytes(jobs[batched[b]]);
        add[2] = 1;
      },
      [](int, int, const long long*) {});
  for (const LaunchSet& cut : cuts) {
    HistogramSetPlan set;
    const int s = static_cast<int>(plan.sets.size());
    StagedArrays clouds(3);
    int classes = 0;
    for (int b = cut.begin; b < cut.end; ++b) {
      const int k = batched[b];
      clouds.Add(k, jobs[k].point_cloud_xyz, jobs[k].num_points, [](int, int, int) {});
      set.result_bytes += HistogramResultBytes(jobs[k]);
      classes = std::max(classes, HistogramLaunchClass(plan.jobs[k].N) + 1);
    }
    set.staged_floats = static_cast<long long>(clouds.floats());
    for (int cls = 0; cls < classes; ++cls) {
      HistogramLaunchPlan L;
      L.first = static_cast<int>(set.jobs.size());
      L.cls = cls;
      for (int b = cut.begin; b < cut.end; ++b) {
        HistogramJobPlan& P = plan.jobs[batched[b]];
        if (HistogramLaunchClass(P.N) != cls) continue;
        P.set = s;
        P.launch = static_cast<int>(set.launches.size());
        P.slot = static_cast<int>(set.jobs.size());
        set.jobs.push_back(batched[b]);
        L.N = std::max(L.N, P.N);
      }
      L.count = static_cast<int>(set.jobs.size()) - L.first;
      if (L.count == 0) continue;
      set.launches.push_back(L);
      ++plan.num_launches;
    }
    plan.staged_bytes += 4 * set.staged_floats;
    plan.sets.push_back(std::move(set));
  }
  return plan;
}

}  // namespace cmx
#endif  // CMX_HISTOGRAM_BATCH_PLAN_H_
