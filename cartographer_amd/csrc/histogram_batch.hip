// cmx_compute_histogram_batch: RotationalScanMatcher::ComputeHistogram for many clouds in one
// call -- the histogram LocalTrajectoryBuilder3D::InsertIntoSubmap computes for every inserted
// node, for a fleet -- bit for bit the single call of filters.hip on the same inputs.
//
// One workgroup per job.  The single call is three radix sorts, a scan and six kernels per cloud
// with the host reading the number of slices in between; a node's voxel-filtered cloud is a few
// thousand points, and for those every step fits one workgroup's LDS
// (histogram_batch_device.h).  A set of jobs is one upload block (descriptors | distinct clouds),
// one launch per class of N (histogram_batch_plan.h), histograms stored straight into a pinned
// result block, one synchronisation, then a memcpy to every caller's array.
//
// A cloud above kSmallCloud points, or with a non-finite coordinate, goes through
// cmx_compute_histogram inside the call.
#include <chrono>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/cartographer_mi355x_debug.h"
#include "cmx_batch.h"
#include "cmx_common.h"
#include "histogram_batch_device.h"
#include "histogram_batch_plan.h"
#include "histogram_common.h"

namespace cmx {
namespace {

// Offsets in bytes.
struct HistogramJobDesc {
  long long cloud_at;       // in the upload block
  long long histogram_at;   // in the pinned result block
  int n, N;
  int histogram_size;
  int reserved;
};

__global__ void __launch_bounds__(kSmallThreads)
HistogramBatchKernel(const HistogramJobDesc* __restrict__ descs, const char* __restrict__ staged,
                     char* __restrict__ results, float min_distance_sq, float max_distance_sq) {
  extern __shared__ __attribute__((aligned(16))) unsigned char histogram_smem[];
  const HistogramJobDesc& D = descs[blockIdx.x];
  const int N = D.N;
  const int n = min(max(D.n, 0), N);       // (the carve holds N points)
  HistogramWorkgroup(histogram_smem, reinterpret_cast<const float*>(staged + D.cloud_at), n, N,
                     D.histogram_size, min_distance_sq, max_distance_sq,
                     reinterpret_cast<float*>(results + D.histogram_at));
}

void CheckJobs(const cmx_histogram_job* jobs, int num) {
  CMX_REQUIRE(num >= 1, "num_jobs %d < 1", num);
  CMX_REQUIRE(jobs != nullptr, "null jobs");
  CheckHistogramJobs(jobs, num,
                     [](int job, const char* what) { CMX_REQUIRE(false, "job %d: %s", job, what); });
}

long long SetBytes() {
  return Debug().histogram_batch_set_kb > 0 ? 1024ll * Debug().histogram_batch_set_kb
                                            : kHistogramSetBytes;
}

// The plan of a call.  Its routes need to know which clouds are finite: every distinct cloud of
// up to kSmallCloud points is scanned once, ahead of the plan, by the pool's threads.
HistogramBatchPlan Plan(const cmx_histogram_job* jobs, int num) {
  std::unordered_map<const float*, int> first_job;
  std::vector<int> scans;
  for (int k = 0; k < num; ++k)
    if (jobs[k].num_points >= 1 && jobs[k].num_points <= kSmallCloud &&
        first_job.emplace(jobs[k].point_cloud_xyz, k).second)
      scans.push_back(k);
  std::vector<char> finite(num, 0);
  ParallelFor(static_cast<int>(scans.size()), 8, [&](int s) {
    const cmx_histogram_job& J = jobs[scans[s]];
    finite[scans[s]] = CloudIsFinite(J.point_cloud_xyz, J.num_points) ? 1 : 0;
  });
  return PlanHistogramBatch(jobs, num, SetBytes(), [&](int k) { return finite[k] != 0; });
}

struct HostTimes {
  double prepare_us = 0, issue_us = 0, wait_us = 0, copy_us = 0;
};

// One set: staging, its launches, one synchronisation, the histograms handed out.
void RunSet(const cmx_histogram_job* jobs, const HistogramBatchPlan& plan,
            const HistogramSetPlan& set, int device, HostTimes* times) {
  using Clock = std::chrono::steady_clock;
  const auto since = [](Clock::time_point t) {
    return std::chrono::duration<double, std::micro>(Clock::now() - t).count();
  };
  Clock::time_point lap = Clock::now();
  const int num = static_cast<int>(set.jobs.size());
  WorkspaceLease ws(device);
  hipStream_t stream = ws->stream;
  StagedArrays clouds(3);
  for (int k : set.jobs) clouds.Add(k, jobs[k].point_cloud_xyz, jobs[k].num_points, [](int, int, int) {});

  // One upload block: descriptors (launch after launch) | clouds.  The pinned result block: per
  // job its histogram.
  BlockLayout block, results;
  const auto descs_in = block.Add<HistogramJobDesc>(num);
  const auto points_in = block.Add<float>(clouds.floats());
  std::vector<HistogramJobDesc> descs(num);
  for (int slot = 0; slot < num; ++slot) {
    const cmx_histogram_job& J = jobs[set.jobs[slot]];
    HistogramJobDesc& D = descs[slot];
    D.cloud_at = static_cast<long long>(points_in.at + sizeof(float) * clouds.OffsetOf(J.point_cloud_xyz));
    D.histogram_at = static_cast<long long>(results.Add<float>(J.histogram_size).at);
    D.n = J.num_points;
    D.N = plan.jobs[set.jobs[slot]].N;
    D.histogram_size = J.histogram_size;
    D.reserved = 0;
  }
  char* h_block = static_cast<char*>(ws->pinned[0].Reserve(block.bytes));
  char* d_block = static_cast<char*>(ws->dev[0].Reserve(block.bytes));
  char* h_results = static_cast<char*>(ws->pinned[1].Reserve(results.bytes));
  std::memcpy(descs_in(h_block), descs.data(), sizeof(HistogramJobDesc) * num);
  // Every distinct cloud once (the pool's threads: a copy is memory bound).
  clouds.CopyTo(points_in(h_block), [](int n, const std::function<void(int)>& copy) {
    ParallelFor(n, 8, copy);
  });
  times->prepare_us += since(lap);
  lap = Clock::now();

  OptInLds(reinterpret_cast<const void*>(HistogramBatchKernel), device, 160 * 1024 - 256);
  SmallCopyAsync(d_block, h_block, block.bytes, /*to_device=*/true, stream);
  for (const HistogramLaunchPlan& L : set.launches)
    HistogramBatchKernel<<<L.count, kSmallThreads, HistogramLdsBytes(L.N), stream>>>(
        descs_in(d_block) + L.first, d_block, h_results, HistogramMinDistanceSq(),
        HistogramMaxDistanceSq());
  CMX_HIP(hipGetLastError());
  times->issue_us += since(lap);
  lap = Clock::now();
  CMX_HIP(hipStreamSynchronize(stream));
  times->wait_us += since(lap);
  lap = Clock::now();

  ParallelFor(num, 16, [&](int slot) {
    const cmx_histogram_job& J = jobs[set.jobs[slot]];
    std::memcpy(J.histogram, h_results + descs[slot].histogram_at,
                4 * static_cast<size_t>(J.histogram_size));
  });
  times->copy_us += since(lap);
}

void HistogramBatch(const cmx_histogram_job* jobs, int num, int device) {
  using Clock = std::chrono::steady_clock;
  // Every argument check before the device is touched, and before a histogram is written.
  CheckJobs(jobs, num);
  const Clock::time_point begin = Clock::now();
  const HistogramBatchPlan plan = Plan(jobs, num);
  HostTimes times;
  times.prepare_us = std::chrono::duration<double, std::micro>(Clock::now() - begin).count();
  UseDevice(device);
  for (int k = 0; k < num; ++k)
    if (plan.jobs[k].route == kHistogramNone)
      std::memset(jobs[k].histogram, 0, 4 * static_cast<size_t>(jobs[k].histogram_size));
  for (const HistogramSetPlan& set : plan.sets) RunSet(jobs, plan, set, device, &times);
  for (int k : plan.single_jobs) {
    const cmx_histogram_job& J = jobs[k];
    const cmx_status status =
        cmx_compute_histogram(J.point_cloud_xyz, J.num_points, J.histogram_size, device, J.histogram);
    if (status != CMX_OK) throw HipError{status};      // (cmx_last_error is the single call's)
  }
  if (Debug().host_trace)
    fprintf(stderr,
            "[cmx host] histogram_batch jobs=%d sets=%d launches=%d single=%d prepare=%.0f "
            "issue=%.0f wait=%.0f copy=%.0f\n",
            num, static_cast<int>(plan.sets.size()), plan.num_launches,
            static_cast<int>(plan.single_jobs.size()), times.prepare_us, times.issue_us,
            times.wait_us, times.copy_us);
}

}  // namespace
}  // namespace cmx

extern "C" cmx_status cmx_compute_histogram_batch(const cmx_histogram_job* jobs, int32_t num_jobs,
                                                  int32_t device) {
  return cmx::Guard([&] { cmx::HistogramBatch(jobs, num_jobs, device); });
}

extern "C" cmx_status cmx_debug_histogram_batch_plan(const cmx_histogram_job* jobs,
                                                     int32_t num_jobs,
                                                     cmx_debug_histogram_job_plan* job_plans,
                                                     cmx_debug_histogram_call_plan* call_plan) {
  using namespace cmx;
  return Guard([&] {
    CheckJobs(jobs, num_jobs);
    CMX_REQUIRE(job_plans && call_plan, "null argument");
    const HistogramBatchPlan plan = Plan(jobs, num_jobs);
    for (int k = 0; k < num_jobs; ++k) {
      const HistogramJobPlan& P = plan.jobs[k];
      job_plans[k] = cmx_debug_histogram_job_plan{P.route, P.set, P.launch, P.slot,
                                                  P.N,     P.cloud_slot, P.lds_bytes};
    }
    *call_plan = cmx_debug_histogram_call_plan{plan.staged_bytes, plan.num_launches,
                                               static_cast<int32_t>(plan.sets.size())};
  });
}
