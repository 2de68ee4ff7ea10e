// FastCorrelativeScanMatcher2D on gfx950: a match from end to end (MatchBatch), the exact
// resolution of ties and the C ABI.  The work itself lives in units of its own:
//   fast_2d_stack.hip    precomputation-grid stack construction
//   fast_2d_coarse.hip   scan preparation, lowest-resolution scoring
//   fast_2d.hip          the batched branch and bound: its driver, over fast_2d_seed.hip (dive,
//                        filter), fast_2d_queue.hip and fast_2d_levels.hip (the two strategies)
// Lists of (node, submap) pairs, each with its own cloud, are split into MatchBatch calls by
// fast_2d_pairs.hip.
// (shared declarations: fast_2d_internal.h, shared device helpers: fast_2d_device.h).
//
// Reference behaviour being replaced:
//   SM2/fast_correlative_scan_matcher_2d.cc:91-186   PrecomputationGrid2D / Stack
//   SM2/correlative_scan_matcher_2d.cc:73-127        ShrinkToFit / GenerateRotatedScans / DiscretizeScans
//   SM2/fast_correlative_scan_matcher_2d.cc:227-378  MatchWithSearchParameters, ScoreCandidates, BranchAndBound
// (SM2 = cartographer/mapping/internal/2d/scan_matching).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "../../include/cartographer_mi355x_debug.h"
#include "fast_2d_internal.h"

namespace cmx {

float MaxRangeXY(const float* xyz, int n) {
  float m = 0.f;
  for (int i = 0; i < n; ++i) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1];
    m = std::max(m, std::sqrt(x * x + y * y));
  }
  return m;
}

namespace {

// Exact tie resolution.  When several leaves share the best score the
// reference returns the one its depth-first search meets first, and at the top
// level that order is whatever std::sort (libstdc++ introsort, unstable) makes
// of equal-score candidates (SM2/fast_...2d.cc:331-332).  The host repeats that
// very sort on the lowest-resolution scores (same initial order, same
// comparator) and ranks the tied leaves by (sorted position of their
// lowest-resolution ancestor, sibling ranks down the tree).  Only runs when the
// device reported a tie.
struct ScoreIndex {
  float score;
  int index;
  bool operator>(const ScoreIndex& other) const { return score > other.score; }
};

// The device keeps the lowest-resolution candidates of scan s at [s * coarse_stride, ...);
// the reference's generation order (scan, x, y) is the dense concatenation.  Host-side
// views for the rare paths that need that order (tie replay, depth 1, introspection).
struct CoarseLayout {
  std::vector<int2> dims;   // [S]
  std::vector<int> off;     // [S + 1] dense prefix
  int Dense(const Fast2DProblem& P, int strided) const {
    return off[strided / P.coarse_stride] + strided % P.coarse_stride;
  }
};
CoarseLayout DownloadLayout(const Fast2DProblem& P) {
  CoarseLayout L;
  const int S = P.num_scans;
  L.dims.resize(S);
  L.off.resize(S + 1);
  CMX_HIP(hipMemcpy(L.dims.data(), P.coarse_dims, S * sizeof(int2), hipMemcpyDeviceToHost));
  L.off[0] = 0;
  for (int s = 0; s < S; ++s) L.off[s + 1] = L.off[s] + L.dims[s].x * L.dims[s].y;
  return L;
}
template <typename T>
std::vector<T> DownloadDense(const Fast2DProblem& P, const CoarseLayout& L, const T* device) {
  const int S = P.num_scans;
  std::vector<T> strided(static_cast<size_t>(S) * P.coarse_stride);
  CMX_HIP(hipMemcpy(strided.data(), device, strided.size() * sizeof(T), hipMemcpyDeviceToHost));
  std::vector<T> dense(L.off[S]);
  for (int s = 0; s < S; ++s)
    std::copy_n(strided.begin() + static_cast<size_t>(s) * P.coarse_stride,
                L.off[s + 1] - L.off[s], dense.begin() + L.off[s]);
  return dense;
}

void ResolveTies(Workspace& ws, const PreparedBatch& batch, BatchResult* result) {
  std::vector<BestLeaf>* best = &result->best;
  const std::vector<ProblemState>& states = result->states;
  bool any = false;
  for (const BestLeaf& b : *best) any |= (b.found && b.ties > 1);
  if (!any) return;
  // All recorded leaves.
  std::vector<Node2D> leaves;
  for (int sub = 0; sub < kSubLists; ++sub) {
    const int count = std::min(result->leaf_counts[sub], result->leaf_sub_capacity);
    if (count <= 0) continue;
    const size_t old = leaves.size();
    leaves.resize(old + count);
    CMX_HIP(hipMemcpy(leaves.data() + old,
                      result->d_leaves + static_cast<size_t>(sub) * result->leaf_sub_capacity,
                      count * sizeof(Node2D), hipMemcpyDeviceToHost));
  }
  for (int p = 0; p < batch.num_problems; ++p) {
    BestLeaf& b = (*best)[p];
    if (!b.found || b.ties <= 1) continue;
    unsigned best_bits;
    std::memcpy(&best_bits, &b.score, sizeof(float));
    // The dive and the search record the same leaf twice; only distinct leaves tie.
    std::vector<const Node2D*> tied;
    for (const Node2D& nd : leaves) {
      unsigned bits;
      std::memcpy(&bits, &nd.score, sizeof(float));
      if ((nd.problem & 0xffffff) != p || bits != best_bits) continue;
      bool duplicate = false;
      for (const Node2D* t : tied)
        duplicate |= (t->scan == nd.scan && t->dx == nd.dx && t->dy == nd.dy);
      if (!duplicate) tied.push_back(&nd);
      if (tied.size() > 4096) break;   // degenerate input: plenty of ties, stop deduplicating
    }
    if (tied.size() <= 1) continue;
    const Fast2DProblem& P = batch.h_problems[p];
    RescoreExact(ws, batch, p);
    const CoarseLayout layout = DownloadLayout(P);
    const std::vector<float> scores = DownloadDense(P, layout, P.coarse_score);
    const int total = static_cast<int>(scores.size());
    CMX_REQUIRE(total == states[p].coarse_total, "internal error: candidate layout mismatch");
    std::vector<ScoreIndex> sorted(total);
    for (int c = 0; c < total; ++c) sorted[c] = {scores[c], c};
    std::sort(sorted.begin(), sorted.end(), std::greater<ScoreIndex>());
    std::vector<int> position(total);
    for (int i = 0; i < total; ++i) position[sorted[i].index] = i;
    bool have = false;
    unsigned long long best_key = 0;
    for (const Node2D& nd : leaves) {
      unsigned bits;
      std::memcpy(&bits, &nd.score, sizeof(float));
      if ((nd.problem & 0xffffff) != p || bits != best_bits) continue;
      const unsigned long long key =
          (static_cast<unsigned long long>(position[layout.Dense(P, nd.coarse_index)]) << 32) |
          nd.path;
      if (!have || key < best_key) {
        have = true;
        best_key = key;
        b.scan = nd.scan; b.dx = nd.dx; b.dy = nd.dy;
      }
    }
  }
}

// depth == 1: BranchAndBound returns candidates[0] of the std::sort-ed
// lowest-resolution candidates (SM2/fast_...2d.cc:340-343); replay that sort.
void ResolveDepthOne(const PreparedBatch& batch, std::vector<BestLeaf>* best,
                     const std::vector<ProblemState>& states) {
  for (int p = 0; p < batch.num_problems; ++p) {
    BestLeaf& b = (*best)[p];
    const Fast2DProblem& P = batch.h_problems[p];
    if (states[p].error || states[p].coarse_total <= 0) continue;
    const CoarseLayout layout = DownloadLayout(P);
    const std::vector<float> scores = DownloadDense(P, layout, P.coarse_score);
    const int total = static_cast<int>(scores.size());
    std::vector<ScoreIndex> sorted(total);
    for (int c = 0; c < total; ++c) sorted[c] = {scores[c], c};
    std::sort(sorted.begin(), sorted.end(), std::greater<ScoreIndex>());
    const int S = P.num_scans;
    const std::vector<int>& off = layout.off;
    const std::vector<int2>& dims = layout.dims;
    std::vector<int4> bounds(S);
    CMX_HIP(hipMemcpy(bounds.data(), P.bounds, S * sizeof(int4), hipMemcpyDeviceToHost));
    const int c = sorted[0].index;
    const int s = static_cast<int>(std::upper_bound(off.begin(), off.end(), c) - off.begin()) - 1;
    const int local = c - off[s];
    b = BestLeaf{};
    b.score = sorted[0].score;
    b.found = b.score > P.min_score;
    b.scan = s;
    b.dx = bounds[s].x + local / dims[s].y;    // depth 1: step 1, x outer / y inner
    b.dy = bounds[s].z + local % dims[s].y;
    b.ties = 1;
  }
}

void CheckProblemErrors(const BatchResult& r) {
  for (const ProblemState& st : r.states) {
    CMX_REQUIRE(st.error != 1, "scan cell indices exceed the int16 range supported on device");
    CMX_REQUIRE(st.error != 2, "internal error: lowest-resolution candidate capacity exceeded");
    CMX_REQUIRE(st.error != 3, "internal error: a group bound of the fused front end lies below one of its rotations' sums");
  }
}

// (debug switch host_trace: where a caller's wall clock goes -- tools only)
std::atomic<long long> g_host_calls{0}, g_host_total_ns{0}, g_host_waited_ns{0};

}  // namespace

void AddMatchStats(const cmx_match_stats& part, cmx_match_stats* total) {
  total->candidates_scored += part.candidates_scored;
  total->coarse_candidates += part.coarse_candidates;
  total->nodes_expanded += part.nodes_expanded;
  total->num_scans += part.num_scans;
  total->device_ms += part.device_ms;                      // (sums over concurrent searches)
  total->dominant_kernel_ms += part.dominant_kernel_ms;
  total->expansion_ms += part.expansion_ms;
  total->expansion_launches += part.expansion_launches;
  total->expansion_nodes += part.expansion_nodes;
  total->expansion_lookups += part.expansion_lookups;
}

void MatchBatch(const cmx_fast2d* const* handles, int num, const cmx_pose2d* initial,
                bool full_submap, const float* host_xyz, const cmx_cloud* cloud, int n,
                float min_score, int32_t* found, float* scores, cmx_pose2d* poses,
                cmx_match_stats* stats, const int32_t* full_flags, const float* min_scores,
                bool allow_fanout) {
  CMX_REQUIRE(handles != nullptr && num >= 1, "no matchers given");
  CMX_REQUIRE(num < (1 << 24), "too many matchers in one batch");
  CMX_REQUIRE(found != nullptr && scores != nullptr && poses != nullptr,
              "score / pose_estimate outputs must not be null");   // CHECK at :232-233
  CMX_REQUIRE(n >= 1, "empty point cloud");
  CMX_REQUIRE(n <= (1 << 24), "point cloud too large");
  std::vector<const Fast2DMatcher*> matchers(num);
  for (int p = 0; p < num; ++p) {
    CMX_REQUIRE(handles[p] != nullptr && handles[p]->impl, "null matcher handle");
    matchers[p] = handles[p]->impl.get();
    CMX_REQUIRE(matchers[p]->device() == matchers[0]->device(),
                "all matchers of a batch must live on the same device");
    // (the tree search walks the batch level by level; refused here, before anything is launched)
    CMX_REQUIRE(matchers[p]->depth() == matchers[0]->depth(),
                "all matchers of a batch must share branch_and_bound_depth");
  }
  const int device = matchers[0]->device();
  // Large batches (from 32 problems on; debug switch fast2d_fanout: 1 never, N > 1 from N on) as
  // INDEPENDENT searches over the host pool: every problem the single-search chain (front end, dive,
  // filter, work-queue tree) on a workspace and stream of its own, sixteen in flight on sixteen
  // hardware queues, instead of the level-synchronous launches over the whole batch -- 64 submaps
  // 6.6 against 9.8 ms, 128: 11.8 against 17.9, 16: the same (profiles/r06g_fanout.txt; with the
  // runtime's four queues of until round 6 it lost: 1.69 against 1.42 ms for 16).  Same results: a
  // problem's search does not depend on its neighbours in the batch.  A caller that finds the
  // pool busy (another batch of the process) runs its problems one after the other itself.
  const int fanout_from = Debug().fast2d_fanout == 0 ? 32 : Debug().fast2d_fanout == 1 ? (1 << 30)
                                                                                       : Debug().fast2d_fanout;
  // (full-submap searches only: a windowed search is a few launches' worth of work, and a batch of
  // them is cheaper in the batch's few launches than in five launches each)
  bool all_full = true;
  for (int p = 0; p < num && all_full; ++p) all_full = full_flags ? full_flags[p] != 0 : full_submap;
  if (allow_fanout && num >= fanout_from && all_full && OverrideStream(device) == nullptr) {
    std::vector<cmx_match_stats> part(num);
    ParallelFor(num, 2, [&](int p) {
      MatchBatch(handles + p, 1, initial ? initial + p : nullptr, full_submap, host_xyz, cloud, n,
                 min_scores ? min_scores[p] : min_score, found + p, scores + p, poses + p, &part[p],
                 full_flags ? full_flags + p : nullptr, nullptr, /*allow_fanout=*/false);
    });
    cmx_match_stats total{};
    for (const cmx_match_stats& st : part) AddMatchStats(st, &total);
    if (stats) *stats = total;
    return;
  }
  const auto t_call = std::chrono::steady_clock::now();
  g_host_wait_ns = 0;
  WorkspaceLease ws(device);
  const float* d_xyz;
  float max_range;
  if (cloud) {
    CMX_REQUIRE(cloud->device == device, "cloud and matcher are on different devices");
    d_xyz = cloud->xyz;
    max_range = cloud->max_range_xy;
  } else {
    CMX_REQUIRE(host_xyz != nullptr, "point cloud is null");
    float* buf = ws->dev[0].ReserveAs<float>(3 * static_cast<size_t>(n));
    CMX_HIP(hipMemcpyAsync(buf, host_xyz, 3 * sizeof(float) * n, hipMemcpyHostToDevice,
                           ws->stream));
    d_xyz = buf;
    max_range = MaxRangeXY(host_xyz, n);
  }
  RecordEvent(ws->ev_begin, ws->stream);
  PreparedBatch batch;
  StageTrace trace(ws->stream);
  batch.trace = &trace;
  ReserveSearchScratch(*ws, num, &batch);
  PrepareAndScoreCoarse(*ws, matchers.data(), num, initial, full_submap, d_xyz, n, max_range,
                        min_score, &batch, full_flags, min_scores);
  BatchResult result;
  RunBranchAndBound(*ws, batch, &result);
  if (matchers[0]->depth() > 1) {
    ResolveTies(*ws, batch, &result);
  } else {
    ResolveDepthOne(batch, &result.best, result.states);
  }
  if (Debug().host_trace) {
    g_host_total_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(
                           std::chrono::steady_clock::now() - t_call).count();
    g_host_waited_ns += g_host_wait_ns;
    const long long calls = ++g_host_calls;
    if (calls % 2000 == 0)
      fprintf(stderr, "[cmx host] fast2d: %lld calls, mean %.1f us per call, of which %.1f us in the final synchronisation\n",
              calls, g_host_total_ns.load() * 1e-3 / calls, g_host_waited_ns.load() * 1e-3 / calls);
  }
  trace.Report();
  if (batch.d_timeline)
    ReportTimeline("PrepScoreFusedKernel", batch.d_timeline, batch.timeline_blocks, ws->stream);
  if (trace.enabled()) {
    for (int p = 0; p < std::min(num, 4); ++p) {
      unsigned long long ex = 0;
      for (int k = 0; k < kStatShards; ++k) ex += result.states[p].expanded_shard[k];
      fprintf(stderr, "[cmx trace] problem %d: coarse %d expanded %llu found %d ties %d\n", p,
              result.states[p].coarse_total, ex, result.best[p].found, result.best[p].ties);
    }
  }
  CheckProblemErrors(result);
  cmx_match_stats total{};
  for (int p = 0; p < num; ++p) {
    const BestLeaf& b = result.best[p];
    const HostSearch& h = batch.search[p];
    const bool ok = b.found && b.score > (min_scores ? min_scores[p] : min_score);
    found[p] = ok ? 1 : 0;
    if (ok) {
      // Candidate2D (SM2/correlative_scan_matcher_2d.h:74-84) and the pose
      // composition of :254-259.
      const double res = matchers[p]->limits().resolution;
      const double cx = -b.dy * res, cy = -b.dx * res;
      const double orientation = (b.scan - h.num_angular) * h.step;
      scores[p] = b.score;
      poses[p].x = batch.initial[p].x + cx;
      poses[p].y = batch.initial[p].y + cy;
      poses[p].theta = batch.initial[p].theta + orientation;
    }
    total.candidates_scored += result.states[p].coarse_total;
    total.coarse_candidates += result.states[p].coarse_total;
    for (int k = 0; k < kStatShards; ++k) {
      total.candidates_scored += result.states[p].scored_shard[k];
      total.nodes_expanded += result.states[p].expanded_shard[k];
    }
    total.num_scans += h.num_scans;
  }
  total.device_ms = result.device_ms;
  total.dominant_kernel_ms = result.dominant_ms;
  total.expansion_ms = result.expansion_ms;
  total.expansion_launches = result.expansion_launches;
  total.expansion_nodes = result.expansion_nodes;
  total.expansion_lookups = result.expansion_lookups;
  if (stats) *stats = total;
}

}  // namespace cmx

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using cmx::Guard;

extern "C" {

cmx_status cmx_fast2d_match(const cmx_fast2d* matcher, const cmx_pose2d* initial_pose_estimate,
                            const float* point_cloud_xyz, int32_t num_points, float min_score,
                            int32_t* found, float* score, cmx_pose2d* pose_estimate,
                            cmx_match_stats* stats) {
  return Guard([&] {
    CMX_REQUIRE(matcher && initial_pose_estimate, "null argument");
    cmx::MatchBatch(&matcher, 1, initial_pose_estimate, false, point_cloud_xyz, nullptr,
                    num_points, min_score, found, score, pose_estimate, stats);
  });
}

cmx_status cmx_fast2d_match_full_submap(const cmx_fast2d* matcher, const float* point_cloud_xyz,
                                        int32_t num_points, float min_score, int32_t* found,
                                        float* score, cmx_pose2d* pose_estimate,
                                        cmx_match_stats* stats) {
  return Guard([&] {
    CMX_REQUIRE(matcher, "null argument");
    cmx::MatchBatch(&matcher, 1, nullptr, true, point_cloud_xyz, nullptr, num_points, min_score,
                    found, score, pose_estimate, stats);
  });
}

cmx_status cmx_fast2d_match_full_submap_batch(const cmx_fast2d* const* matchers,
                                              int32_t num_matchers, const float* point_cloud_xyz,
                                              int32_t num_points, float min_score,
                                              int32_t* found, float* scores,
                                              cmx_pose2d* pose_estimates, cmx_match_stats* stats) {
  return Guard([&] {
    cmx::MatchBatch(matchers, num_matchers, nullptr, true, point_cloud_xyz, nullptr, num_points,
                    min_score, found, scores, pose_estimates, stats);
  });
}

cmx_status cmx_cloud_upload(const float* point_cloud_xyz, int32_t num_points, int32_t device,
                            cmx_cloud** out) {
  return Guard([&] {
    CMX_REQUIRE(point_cloud_xyz && out && num_points >= 1, "invalid point cloud");
    *out = nullptr;
    cmx::UseDevice(device);
    std::unique_ptr<cmx_cloud> c(new cmx_cloud);
    c->device = device;
    c->num_points = num_points;
    c->host_xyz.assign(point_cloud_xyz, point_cloud_xyz + 3 * static_cast<size_t>(num_points));
    c->max_range_xy = cmx::MaxRangeXY(point_cloud_xyz, num_points);
    float m = 0.f;
    for (int i = 0; i < num_points; ++i) {
      const float x = point_cloud_xyz[3 * i], y = point_cloud_xyz[3 * i + 1],
                  z = point_cloud_xyz[3 * i + 2];
      m = std::max(m, std::sqrt(x * x + y * y + z * z));
    }
    c->max_range_xyz = m;
    {
      double best = 0.;
      for (int i = 0; i < num_points; ++i) {
        const double x = point_cloud_xyz[3 * i], y = point_cloud_xyz[3 * i + 1];
        best = std::max(best, x * x + y * y);
      }
      for (int i = 0; i < num_points && c->far_points.size() <= 64; ++i) {
        const double x = point_cloud_xyz[3 * i], y = point_cloud_xyz[3 * i + 1];
        if (x * x + y * y >= best * (1. - 1e-4)) c->far_points.push_back(i);
      }
      if (c->far_points.size() > 64) c->far_points.clear();
    }
    CMX_HIP(hipMalloc(&c->xyz, 3 * sizeof(float) * num_points));
    hipError_t err = hipMemcpy(c->xyz, point_cloud_xyz, 3 * sizeof(float) * num_points,
                               hipMemcpyHostToDevice);
    if (err != hipSuccess) {
      (void)hipFree(c->xyz);
      c->xyz = nullptr;
      CMX_HIP(err);
    }
    *out = c.release();
  });
}

void cmx_cloud_destroy(cmx_cloud* cloud) {
  if (!cloud) return;
  if (cloud->xyz) {
    (void)hipSetDevice(cloud->device);
    (void)hipFree(cloud->xyz);
  }
  delete cloud;
}

cmx_status cmx_fast2d_match_full_submap_batch_resident(
    const cmx_fast2d* const* matchers, int32_t num_matchers, const cmx_cloud* cloud,
    float min_score, int32_t* found, float* scores, cmx_pose2d* pose_estimates,
    cmx_match_stats* stats) {
  return Guard([&] {
    CMX_REQUIRE(cloud != nullptr, "null cloud");
    cmx::MatchBatch(matchers, num_matchers, nullptr, true, nullptr, cloud, cloud->num_points,
                    min_score, found, scores, pose_estimates, stats);
  });
}

cmx_status cmx_fast2d_match_batch(const cmx_fast2d* const* matchers, int32_t num_matchers,
                                  const cmx_pose2d* initial_pose_estimates,
                                  const int32_t* match_full_submap, const float* min_scores,
                                  const float* point_cloud_xyz, int32_t num_points, int32_t* found,
                                  float* scores, cmx_pose2d* pose_estimates,
                                  cmx_match_stats* stats) {
  return Guard([&] {
    CMX_REQUIRE(match_full_submap != nullptr && min_scores != nullptr, "null argument");
    bool any_windowed = false;
    for (int p = 0; p < num_matchers; ++p) any_windowed |= match_full_submap[p] == 0;
    CMX_REQUIRE(!any_windowed || initial_pose_estimates != nullptr,
                "initial_pose_estimates required for windowed searches");
    cmx::MatchBatch(matchers, num_matchers, initial_pose_estimates, false, point_cloud_xyz, nullptr,
                    num_points, 0.f, found, scores, pose_estimates, stats, match_full_submap,
                    min_scores);
  });
}

cmx_status cmx_fast2d_debug_prepare(const cmx_fast2d* matcher,
                                    const cmx_pose2d* initial_pose_estimate,
                                    const float* point_cloud_xyz, int32_t num_points,
                                    int32_t full_submap, int32_t* num_scans,
                                    double* angular_step, int32_t* discrete_xy,
                                    int64_t discrete_capacity, int32_t* bounds,
                                    int64_t bounds_capacity, int32_t* coarse_sums,
                                    int64_t sums_capacity, int64_t* num_coarse) {
  return Guard([&] {
    CMX_REQUIRE(matcher && matcher->impl && point_cloud_xyz && num_points >= 1, "bad argument");
    CMX_REQUIRE(full_submap || initial_pose_estimate, "initial pose required");
    const cmx::Fast2DMatcher* m = matcher->impl.get();
    cmx::WorkspaceLease ws(m->device());
    const int n = num_points;
    float* d_xyz = ws->dev[0].ReserveAs<float>(3 * static_cast<size_t>(n));
    CMX_HIP(hipMemcpyAsync(d_xyz, point_cloud_xyz, 3 * sizeof(float) * n, hipMemcpyHostToDevice,
                           ws->stream));
    cmx::RecordEvent(ws->ev_begin, ws->stream);
    cmx::PreparedBatch batch;
    batch.write_all_discrete = true;
    cmx::PrepareAndScoreCoarse(*ws, &m, 1, initial_pose_estimate, full_submap != 0, d_xyz, n,
                               cmx::MaxRangeXY(point_cloud_xyz, n), 0.f, &batch);
    CMX_HIP(hipStreamSynchronize(ws->stream));
    const cmx::Fast2DProblem& P = batch.h_problems[0];
    cmx::ProblemState st;
    CMX_HIP(hipMemcpy(&st, batch.d_states, sizeof(st), hipMemcpyDeviceToHost));
    CMX_REQUIRE(st.error == 0, "device preparation error %d", st.error);
    const int S = P.num_scans;
    const cmx::CoarseLayout layout = cmx::DownloadLayout(P);
    st.coarse_total = layout.off[S];
    if (num_scans) *num_scans = S;
    if (angular_step) *angular_step = batch.search[0].step;
    if (num_coarse) *num_coarse = st.coarse_total;
    if (discrete_xy) {
      CMX_REQUIRE(discrete_capacity >= 2ll * S * n, "discrete_xy capacity too small");
      std::vector<uint32_t> packed(static_cast<size_t>(S) * n);
      CMX_HIP(hipMemcpy(packed.data(), P.discrete, packed.size() * sizeof(uint32_t),
                        hipMemcpyDeviceToHost));
      for (size_t i = 0; i < packed.size(); ++i) {
        discrete_xy[2 * i] = static_cast<short>(packed[i] & 0xffffu);
        discrete_xy[2 * i + 1] = static_cast<short>(packed[i] >> 16);
      }
    }
    if (bounds) {
      CMX_REQUIRE(bounds_capacity >= 4ll * S, "bounds capacity too small");
      std::vector<int4> b(S);
      CMX_HIP(hipMemcpy(b.data(), P.bounds, S * sizeof(int4), hipMemcpyDeviceToHost));
      for (int s = 0; s < S; ++s) {
        bounds[4 * s] = b[s].x; bounds[4 * s + 1] = b[s].y;
        bounds[4 * s + 2] = b[s].z; bounds[4 * s + 3] = b[s].w;
      }
    }
    if (coarse_sums) {
      CMX_REQUIRE(sums_capacity >= st.coarse_total, "coarse_sums capacity too small");
      const std::vector<int> dense = cmx::DownloadDense(P, layout, P.coarse_sum);
      std::copy(dense.begin(), dense.end(), coarse_sums);
    }
  });
}

cmx_status cmx_debug_fast2d_plan(const cmx_fast2d* const* matchers,
                                 const cmx_grid2d_limits* limits,
                                 const cmx_fast2d_options* options, int32_t num_matchers,
                                 const int32_t* match_full_submap, int32_t num_points,
                                 float max_range_xy, cmx_debug_fast2d_problem_plan* problems,
                                 cmx_debug_fast2d_launch_plan* launch) {
  return Guard([&] {
    CMX_REQUIRE(num_matchers >= 1 && num_points >= 1 && problems && launch, "bad argument");
    CMX_REQUIRE(matchers || (limits && options), "matchers, or limits and options");
    std::vector<cmx::PlanMatcher> views(num_matchers);
    for (int p = 0; p < num_matchers; ++p) {
      if (matchers) {
        CMX_REQUIRE(matchers[p] && matchers[p]->impl, "null matcher handle");
        views[p] = cmx::PlanMatcherOf(*matchers[p]->impl);
      } else {
        // (what cmx_fast2d_create requires of them)
        CMX_REQUIRE(options[p].branch_and_bound_depth >= 1 &&
                        options[p].branch_and_bound_depth <= cmx::kMaxDepth,
                    "branch_and_bound_depth %d outside [1,%d]", options[p].branch_and_bound_depth,
                    cmx::kMaxDepth);
        CMX_REQUIRE(limits[p].resolution > 0. && limits[p].num_x_cells >= 1 &&
                        limits[p].num_y_cells >= 1 && limits[p].num_x_cells <= 16384 &&
                        limits[p].num_y_cells <= 16384, "unsupported grid limits");
        views[p] = cmx::PlanMatcherOf(options[p], limits[p]);
      }
    }
    const cmx::FrontEndPlan plan = cmx::PlanFrontEnd(views.data(), num_matchers, match_full_submap,
                                                     false, num_points, max_range_xy, false);
    for (int p = 0; p < num_matchers; ++p) {
      const cmx::ProblemPlan& Q = plan.problems[p];
      cmx_debug_fast2d_problem_plan& out = problems[p];
      out = cmx_debug_fast2d_problem_plan{};
      out.use_planes = Q.use_planes ? 1 : 0;
      out.plane_stride = views[p].planes ? views[p].plane_stride : 0;
      out.use_fused = Q.use_fused ? 1 : 0;
      out.group = Q.group;
      out.num_scans = Q.search.num_scans;
      out.acc = Q.acc;
    }
    *launch = cmx_debug_fast2d_launch_plan{};
    launch->fused_lds = static_cast<int64_t>(plan.fused_lds);
    launch->fused_acc = plan.fused_acc;
    launch->plane_acc_cells = plan.plane_acc_cells;
    launch->any_group = plan.any_group ? 1 : 0;
    launch->max_scans = plan.max_scans;
    launch->per_unit = plan.per_unit;
  });
}

}  // extern "C"
