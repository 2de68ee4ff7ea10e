// cmx_filter_batch: sensor::VoxelFilter / AdaptiveVoxelFilter for many clouds in one call, and a
// filter's output handed to the next filter on the device -- the chain of LocalTrajectoryBuilder2D
// (VoxelFilter, then AdaptiveVoxelFilter on its output) and of LocalTrajectoryBuilder3D
// (VoxelFilter, then a high- and a low-resolution AdaptiveVoxelFilter on its output), for one
// robot or a fleet -- bit for bit the single calls of filters.hip on the same inputs.
//
// One workgroup per job.  The single call's kernel is one workgroup for one cloud: one of 256
// compute units works, and every call is an upload, a launch and a synchronisation.  Here the same
// device code (filters_small_device.h) runs as blockIdx.x-th job of a descriptor table: all roots
// (jobs on host clouds) in a first stage of launches, all chained jobs in a second on the same
// stream.  A root with children also leaves its kept points and their number in device memory;
// a child reads its n0 there, so the host reads nothing between the stages and synchronises once,
// at the end.  A child's LDS carve is its root's N: its input cannot be larger.
//
// Dynamic LDS is per launch and sized for the largest N in it; a stage is cut into the two
// launches that differ in occupancy (filters_batch_plan.h).  Every distinct host cloud is staged
// once (StagedArrays); results are stored straight into pinned host memory, every job in slots of
// its own.  Sets (CutSets) bound the staging and the result block of a call.
//
// A root above kSmallCloud points, and its children, go through the single calls one after the
// other (their multi-launch path searches with the host between the launches).
#include <chrono>
#include <cstring>
#include <vector>

#include "../../include/cartographer_mi355x_debug.h"
#include "cmx_batch.h"
#include "cmx_common.h"
#include "filters_batch_plan.h"
#include "filters_small_device.h"

namespace cmx {
namespace {

// Offsets in bytes; -1: none.
struct FilterJobDesc {
  long long input_at;       // a root: its cloud in the staged clouds; a child: its parent's points
                            // in the device outputs
  long long count_from;     // a child: its parent's count in the device outputs; a root: -1
  int n0;                   // a root: its points
  int N;
  int mode;
  float length, min_num_points, max_range;
  long long count_at, indices_at, points_at;   // in the pinned result block
  long long device_at;      // in the device outputs: the count, the points 256 bytes behind it
};

// (8 waves per SIMD = two workgroups per compute unit: without the bound the compiler takes 106
// scalar registers, which admit six waves per SIMD, one workgroup; with it 78, a few scalars kept
// in vector lanes, no scratch)
__global__ void __launch_bounds__(kSmallThreads, 8)
FilterBatchKernel(const FilterJobDesc* __restrict__ descs, const char* __restrict__ staged,
                  char* __restrict__ results, char* device_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char batch_smem[];
  const FilterJobDesc& D = descs[blockIdx.x];
  const bool chained = D.count_from >= 0;
  const float* xyz = reinterpret_cast<const float*>((chained ? device_out : staged) + D.input_at);
  int n0 = chained ? *reinterpret_cast<const int*>(device_out + D.count_from) : D.n0;
  n0 = min(max(n0, 0), D.N);       // (the carve holds N points whatever the parent left)
  SmallFilterResult out;
  out.count = reinterpret_cast<int*>(results + D.count_at);
  out.indices = D.indices_at >= 0 ? reinterpret_cast<int*>(results + D.indices_at) : nullptr;
  out.points = D.points_at >= 0 ? reinterpret_cast<float*>(results + D.points_at) : nullptr;
  out.device_count = D.device_at >= 0 ? reinterpret_cast<int*>(device_out + D.device_at) : nullptr;
  out.device_points =
      D.device_at >= 0 ? reinterpret_cast<float*>(device_out + D.device_at + 256) : nullptr;
  SmallFilterWorkgroup(batch_smem, xyz, n0, D.N, D.mode, D.length, D.min_num_points, D.max_range,
                       out);
}

void CheckJobs(const cmx_filter_job* jobs, int num) {
  CMX_REQUIRE(num >= 1, "num_jobs %d < 1", num);
  CMX_REQUIRE(jobs != nullptr, "null jobs");
  CheckFilterJobs(jobs, num,
                  [](int job, const char* what) { CMX_REQUIRE(false, "job %d: %s", job, what); });
}

long long SetBytes() {
  return Debug().filter_batch_set_kb > 0 ? 1024ll * Debug().filter_batch_set_kb : kFilterSetBytes;
}

struct HostTimes {
  double prepare_us = 0, issue_us = 0, wait_us = 0, copy_us = 0;
};

// One set: staging, the launches of both stages, one synchronisation, the results handed out.
void RunSet(const cmx_filter_job* jobs, const FilterBatchPlan& plan, const FilterSetPlan& set,
            int device, int32_t* num_filtered, HostTimes* times) {
  using Clock = std::chrono::steady_clock;
  const auto since = [](Clock::time_point t) {
    return std::chrono::duration<double, std::micro>(Clock::now() - t).count();
  };
  Clock::time_point lap = Clock::now();
  const int num = static_cast<int>(set.jobs.size());
  WorkspaceLease ws(device);
  hipStream_t stream = ws->stream;
  StagedArrays clouds(3);
  for (int k : set.jobs)
    if (jobs[k].input_job < 0)
      clouds.Add(k, jobs[k].point_cloud_xyz, jobs[k].num_points, [](int, int, int) {});

  // One upload block: descriptors (launch after launch) | clouds.
  BlockLayout block;
  const auto descs_in = block.Add<FilterJobDesc>(num);
  const auto points_in = block.Add<float>(clouds.floats());
  // The pinned result block: counts | per job its indices and points, where it wants them.
  // The device outputs: per root with children its count and, 256 bytes on, its points.
  BlockLayout results, device_out;
  const auto counts_out = results.Add<int>(num);
  std::vector<FilterJobDesc> descs(num);
  for (int slot = 0; slot < num; ++slot) {
    const int k = set.jobs[slot];
    const cmx_filter_job& J = jobs[k];
    const FilterJobPlan& P = plan.jobs[k];
    const size_t room = static_cast<size_t>(jobs[P.root].num_points);
    FilterJobDesc& D = descs[slot];
    D.N = P.N;
    D.mode = J.mode;
    D.length = J.length;
    D.min_num_points = J.min_num_points;
    D.max_range = J.max_range;
    D.count_at = static_cast<long long>(counts_out.at + sizeof(int) * slot);
    D.indices_at = J.kept_indices ? static_cast<long long>(results.Add<int>(room).at) : -1;
    D.points_at = J.filtered_xyz ? static_cast<long long>(results.Add<float>(3 * room).at) : -1;
    D.device_at = -1;
    if (J.input_job < 0) {
      D.input_at = static_cast<long long>(
          points_in.at + sizeof(float) * clouds.OffsetOf(J.point_cloud_xyz));
      D.count_from = -1;
      D.n0 = J.num_points;
      if (!plan.children[k].empty()) {
        D.device_at = static_cast<long long>(device_out.Add<char>(256).at);
        device_out.Add<float>(3 * room);
      }
    } else {
      // (stage 1 follows stage 0 in slot order: the parent's descriptor is complete)
      const FilterJobDesc& parent = descs[plan.jobs[J.input_job].slot];
      D.input_at = parent.device_at + 256;
      D.count_from = parent.device_at;
      D.n0 = 0;
    }
  }
  char* h_block = static_cast<char*>(ws->pinned[0].Reserve(block.bytes));
  char* d_block = static_cast<char*>(ws->dev[0].Reserve(block.bytes));
  char* h_results = static_cast<char*>(ws->pinned[1].Reserve(results.bytes));
  char* d_out = static_cast<char*>(ws->dev[1].Reserve(device_out.bytes + 256));
  std::memcpy(descs_in(h_block), descs.data(), sizeof(FilterJobDesc) * num);
  // Every distinct cloud once (the pool's threads: a copy is memory bound).
  clouds.CopyTo(points_in(h_block), [](int n, const std::function<void(int)>& copy) {
    ParallelFor(n, 8, copy);
  });
  times->prepare_us += since(lap);
  lap = Clock::now();

  OptInLds(reinterpret_cast<const void*>(FilterBatchKernel), device, 160 * 1024 - 256);
  SmallCopyAsync(d_block, h_block, block.bytes, /*to_device=*/true, stream);
  for (int stage = 0; stage < 2; ++stage) {
    for (int launch = 0; launch < 2; ++launch) {
      const FilterLaunchPlan& L = set.launch[stage][launch];
      if (L.count == 0) continue;
      FilterBatchKernel<<<L.count, kSmallThreads, SmallFilterLaunchLds(L.N), stream>>>(
          descs_in(d_block) + L.first, d_block, h_results, d_out);
    }
  }
  CMX_HIP(hipGetLastError());
  times->issue_us += since(lap);
  lap = Clock::now();
  CMX_HIP(hipStreamSynchronize(stream));
  times->wait_us += since(lap);
  lap = Clock::now();

  const int* counts = counts_out(h_results);
  for (int slot = 0; slot < num; ++slot) {
    const int k = set.jobs[slot];
    CMX_REQUIRE(counts[slot] >= 0 && counts[slot] <= jobs[plan.jobs[k].root].num_points,
                "job %d: internal error: filter count %d of %d", k, counts[slot],
                jobs[plan.jobs[k].root].num_points);
  }
  ParallelFor(num, 8, [&](int slot) {
    const cmx_filter_job& J = jobs[set.jobs[slot]];
    const size_t kept = static_cast<size_t>(counts[slot]);
    if (J.kept_indices) std::memcpy(J.kept_indices, h_results + descs[slot].indices_at, 4 * kept);
    if (J.filtered_xyz) std::memcpy(J.filtered_xyz, h_results + descs[slot].points_at, 12 * kept);
    num_filtered[set.jobs[slot]] = counts[slot];
  });
  times->copy_us += since(lap);
}

void Rethrow(cmx_status status) {
  if (status != CMX_OK) throw HipError{status};      // (cmx_last_error is the single call's)
}

// One job by the single calls: both outputs where the job asks for both (the points are the
// input's at the kept indices).  `points` (room for n) receives the kept points if not null.
int RunSingleJob(const cmx_filter_job& J, const float* xyz, int n, int device, float* points) {
  if (n == 0) return 0;
  int32_t kept = 0;
  std::vector<int32_t> own_indices;
  int32_t* indices = J.kept_indices;
  const bool gather = (J.filtered_xyz != nullptr) + (points != nullptr) + (indices != nullptr) > 1;
  if (gather && !indices) {
    own_indices.resize(n);
    indices = own_indices.data();
  }
  float* direct = J.filtered_xyz ? J.filtered_xyz : points;
  if (J.mode == CMX_FILTER_VOXEL) {
    Rethrow(indices ? cmx_voxel_filter_indices(xyz, n, J.length, device, indices, &kept)
                    : cmx_voxel_filter(xyz, n, J.length, device, direct, &kept));
  } else {
    Rethrow(indices ? cmx_adaptive_voxel_filter_indices(xyz, n, J.length, J.min_num_points,
                                                        J.max_range, device, indices, &kept)
                    : cmx_adaptive_voxel_filter(xyz, n, J.length, J.min_num_points, J.max_range,
                                                device, direct, &kept));
  }
  if (indices) {
    for (float* to : {J.filtered_xyz, points}) {
      if (!to) continue;
      for (int i = 0; i < kept; ++i)
        std::memcpy(to + 3 * static_cast<size_t>(i), xyz + 3 * static_cast<size_t>(indices[i]), 12);
    }
  }
  return kept;
}

void FilterBatch(const cmx_filter_job* jobs, int num, int device, int32_t* num_filtered) {
  using Clock = std::chrono::steady_clock;
  // Every argument check before the device is touched.
  CheckJobs(jobs, num);
  CMX_REQUIRE(num_filtered != nullptr, "null num_filtered");
  const Clock::time_point begin = Clock::now();
  const FilterBatchPlan plan = PlanFilterBatch(jobs, num, SetBytes());
  HostTimes times;
  times.prepare_us = std::chrono::duration<double, std::micro>(Clock::now() - begin).count();
  UseDevice(device);
  for (int k = 0; k < num; ++k) num_filtered[k] = 0;
  for (const FilterSetPlan& set : plan.sets) RunSet(jobs, plan, set, device, num_filtered, &times);
  for (int r : plan.single_roots) {
    const cmx_filter_job& R = jobs[r];
    std::vector<float> kept_points;
    if (!plan.children[r].empty() && !R.filtered_xyz)
      kept_points.resize(3 * static_cast<size_t>(R.num_points));
    num_filtered[r] = RunSingleJob(R, R.point_cloud_xyz, R.num_points, device,
                                   kept_points.empty() ? nullptr : kept_points.data());
    const float* parent_points = R.filtered_xyz ? R.filtered_xyz : kept_points.data();
    for (int c : plan.children[r])
      num_filtered[c] = RunSingleJob(jobs[c], parent_points, num_filtered[r], device, nullptr);
  }
  if (Debug().host_trace)
    fprintf(stderr,
            "[cmx host] filter_batch jobs=%d sets=%d launches=%d single=%d prepare=%.0f issue=%.0f "
            "wait=%.0f copy=%.0f\n",
            num, static_cast<int>(plan.sets.size()), plan.num_launches,
            static_cast<int>(plan.single_roots.size()), times.prepare_us, times.issue_us,
            times.wait_us, times.copy_us);
}

}  // namespace
}  // namespace cmx

extern "C" cmx_status cmx_filter_batch(const cmx_filter_job* jobs, int32_t num_jobs, int32_t device,
                                       int32_t* num_filtered) {
  return cmx::Guard([&] { cmx::FilterBatch(jobs, num_jobs, device, num_filtered); });
}

extern "C" cmx_status cmx_debug_filter_batch_plan(const cmx_filter_job* jobs, int32_t num_jobs,
                                                  cmx_debug_filter_job_plan* job_plans,
                                                  cmx_debug_filter_call_plan* call_plan) {
  using namespace cmx;
  return Guard([&] {
    CheckJobs(jobs, num_jobs);
    CMX_REQUIRE(job_plans && call_plan, "null argument");
    const FilterBatchPlan plan = PlanFilterBatch(jobs, num_jobs, SetBytes());
    for (int k = 0; k < num_jobs; ++k) {
      const FilterJobPlan& P = plan.jobs[k];
      const bool runs = P.batched;
      job_plans[k] = cmx_debug_filter_job_plan{
          runs ? P.set : -1, P.stage,     runs ? P.launch : -1, runs ? P.N : 0,
          runs ? P.lds_bytes : 0, P.cloud_slot, P.single ? 1 : 0};
    }
    *call_plan = cmx_debug_filter_call_plan{plan.staged_bytes, plan.num_launches,
                                            static_cast<int32_t>(plan.sets.size())};
  });
}
