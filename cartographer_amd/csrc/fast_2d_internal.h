// What the translation units of the fast 2D matcher share on the host:
//   fast_2d_stack.hip    precomputation stack (Fast2DMatcher)
//   fast_2d_coarse.hip   scan preparation + lowest-resolution scoring (the front end)
//   fast_2d.hip          branch and bound: scratch layout, depth 1, the fall-back ladder
//   fast_2d_seed.hip       ... what runs before either strategy: seeds + dive, filter
//   fast_2d_queue.hip      ... the work-queue strategy
//   fast_2d_levels.hip     ... the level-synchronous strategy (its SubtreeKernel: fast_2d_seed.hip)
//                        (what these four hand each other: fast_2d_search.h)
//   fast_2d_match.hip    MatchBatch, tie resolution, C ABI
//   fast_2d_pairs.hip    lists of (node, submap) pairs: grouping into MatchBatch calls, C ABI
// Every unit owns its kernels and exposes the host functions declared here; no kernel is launched
// from another file than the one that defines it.
#ifndef CMX_FAST_2D_INTERNAL_H_
#define CMX_FAST_2D_INTERNAL_H_

#include <vector>

#include "scan_matching_2d.h"

namespace cmx {

// Cells by which the lowest-resolution level is dilated, either way, for the group bounds of the
// fused front end (DilateLevelKernel builds the image, PrepScoreFusedKernel sums over it).
constexpr int kGroupDilation = 2;
constexpr int kFusedGroup = 3;           // rotations per workgroup under group bounds (see the kernel)
// Node lists (frontiers, leaves) are split into kSubLists sub-lists, each with
// its own counter, so that thousands of blocks appending at once do not
// serialise on one atomic word (one word sustains only ~90 atomics/us).
constexpr int kSubLists = 64;

// SearchParameters ctor (SM2/correlative_scan_matcher_2d.cc:27-55), host side.
struct HostSearch {
  int num_angular;
  double step;
  int num_scans;
  int nl;
};
// (MakeSearch, fast_2d_coarse.hip)

struct PreparedBatch {
  StageTrace* trace = nullptr;
  int num_problems = 0;
  int n = 0;
  int max_scans = 0;
  long long plane_acc_cells = 0;   // LDS accumulators the plane kernel needs (upper bound)
  std::vector<HostSearch> search;
  std::vector<cmx_pose2d> initial;
  Fast2DProblem* d_problems = nullptr;
  ProblemState* d_states = nullptr;
  std::vector<Fast2DProblem> h_problems;
  // Search scratch carved before the first kernel so that it can clear the counters.
  char* d_misc = nullptr;          // (ReserveSearchScratch; layout: fast_2d_search.h)
  int num_counter_words = 0;       // ints at the start of d_misc that the first kernel of a call clears
  bool write_all_discrete = false; // debug entry point: keep every discretised scan
  unsigned long long* d_timeline = nullptr;   // CMX_TIMELINE=1
  int timeline_blocks = 0;
  // The fused front end's launch, kept for the exact re-run of a problem whose leaves tie
  // (RescoreExact): under group bounds the lowest-resolution scores are bounds.
  bool any_group = false;
  size_t fused_lds = 0;
  int fused_acc = 0, fused_threads = 0;
  const float* d_xyz = nullptr;
};

struct BatchResult {
  std::vector<BestLeaf> best;
  std::vector<ProblemState> states;
  double device_ms = 0., dominant_ms = 0.;
  double expansion_ms = 0.;          // wave-per-node stages of the first pass
  int expansion_launches = 0;
  long long expansion_nodes = 0, expansion_lookups = 0;
  // Where the search left its leaf records (depth > 1): what the tie resolution reads.
  const Node2D* d_leaves = nullptr;  // [kSubLists][leaf_sub_capacity]
  int leaf_sub_capacity = 0;
  std::vector<int> leaf_counts;      // [kSubLists] records per sub-list (may exceed the capacity)
};

// ---- fast_2d_coarse.hip
// What the front end's planner reads of a matcher: of a Fast2DMatcher, or of a grid's geometry
// alone (the plan entry of cartographer_mi355x_debug.h: no device needed).
struct PlanMatcher {
  cmx_grid2d_limits limits;
  double linear_search_window, angular_search_window;
  int depth;
  bool planes, planes_group;       // the phase planes (of the level / of its dilation) exist
  int plane_i, plane_j, plane_stride;
};
PlanMatcher PlanMatcherOf(const Fast2DMatcher& m);
// (fast_2d_stack.hip: the planes a matcher of this grid and these options would build)
PlanMatcher PlanMatcherOf(const cmx_fast2d_options& options, const cmx_grid2d_limits& limits);

// The route of one problem through the front end ...
struct ProblemPlan {
  HostSearch search;
  long long ax = 0, ay = 0;        // lowest-resolution candidates per scan and axis (upper bound)
  long long acc = 0;               // padded LDS accumulators of the plane kernels
  bool use_planes = false, use_fused = false;
  int group = 1;                   // rotations per workgroup of the fused front end: 1 or kFusedGroup
};
// ... and the sizes of the launches of the call, which are maxima / "any" flags over its problems.
struct FrontEndPlan {
  std::vector<ProblemPlan> problems;
  bool any_fused = false, any_unfused = false, any_group = false;
  long long fused_acc = 0;         // accumulators of the fused launch (largest of its problems)
  long long plane_acc_cells = 0;   // accumulators of the plane launches
  int max_scans = 0;
  int per_unit = 1;                // rotations per unit of the fused launch's grid
  size_t fused_lds = 0;            // dynamic LDS of the fused launch, bytes (0: no fused problem)
};
// Every decision PrepareAndScoreCoarse takes before it launches; launches nothing itself.
// `full_flags` (or null: `full_submap` for all) as there; `write_all_discrete`: the introspection
// entry, which needs exact lowest-resolution sums (no group bounds).
FrontEndPlan PlanFrontEnd(const PlanMatcher* matchers, int num, const int32_t* full_flags,
                          bool full_submap, int n, float max_range_xy, bool write_all_discrete);

// Uploads problem descriptors, carves scratch and runs the preparation +
// lowest-resolution scoring kernels.  `d_xyz` is the device point cloud.
void PrepareAndScoreCoarse(Workspace& ws, const Fast2DMatcher* const* matchers, int num,
                           const cmx_pose2d* initial_or_null, bool full_submap,
                           const float* d_xyz, int n, float max_range_xy, float min_score,
                           PreparedBatch* out, const int32_t* full_flags = nullptr,
                           const float* min_scores = nullptr);
// The exact lowest-resolution scores of problem p of a batch scored under group bounds (no-op
// otherwise), in place.
void RescoreExact(Workspace& ws, const PreparedBatch& batch, int p);

// ---- fast_2d.hip (QueueSearchWanted: fast_2d_queue.hip)
// Whether a batch of `num` problems over n points goes to the work-queue search (it keeps the
// cells of surviving scans, which the front end has to know).
bool QueueSearchWanted(int n, int num);
// Before PrepareAndScoreCoarse: the search's scratch block, whose counters the front end clears.
void ReserveSearchScratch(Workspace& ws, int num, PreparedBatch* batch);
// Full search of a prepared batch; best leaves as the device selected them (ties unresolved).
void RunBranchAndBound(Workspace& ws, const PreparedBatch& batch, BatchResult* result);
// Nanoseconds this thread's current call has spent in the final synchronisation (host_trace).
extern thread_local long long g_host_wait_ns;

// ---- fast_2d_match.hip
// max ||p.xy|| over a host cloud, in f32 as SearchParameters computes it.
float MaxRangeXY(const float* xyz, int n);
// One cloud (`host_xyz`, uploaded here, or `cloud`, resident) of n points against `num` matchers
// of ONE depth, entry p windowed around initial[p] or a full-submap search (`full_flags`, or
// null: `full_submap` for all) against min_scores[p] (or null: `min_score` for all).
// `allow_fanout`: a batch of 32 and more full-submap searches may go out as independent searches
// over the host pool; false for a call that is itself an item of such a fan-out.
void MatchBatch(const cmx_fast2d* const* handles, int num, const cmx_pose2d* initial,
                bool full_submap, const float* host_xyz, const cmx_cloud* cloud, int n,
                float min_score, int32_t* found, float* scores, cmx_pose2d* poses,
                cmx_match_stats* stats, const int32_t* full_flags = nullptr,
                const float* min_scores = nullptr, bool allow_fanout = true);
// The sum of two calls' statistics, as the fan-out of a batch reports it.
void AddMatchStats(const cmx_match_stats& part, cmx_match_stats* total);

}  // namespace cmx

#endif  // CMX_FAST_2D_INTERNAL_H_
