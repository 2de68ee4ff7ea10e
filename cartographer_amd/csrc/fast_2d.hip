// FastCorrelativeScanMatcher2D on gfx950: the driver of the batched branch and bound behind the
// front end.
//
// Reference behaviour being replaced:
//   SM2/fast_correlative_scan_matcher_2d.cc:227-378  MatchWithSearchParameters, BranchAndBound
// (SM2 = cartographer/mapping/internal/2d/scan_matching).
//
// Search schedule (any sound schedule returns the reference's best score), the lowest-resolution
// candidates having been scored (fast_2d_coarse.hip):
//   2. "dive": greedy descents from the best few of them give a real leaf
//      score b0, a valid lower bound (fast_2d_seed.hip);
//   3. every lowest-resolution node whose upper bound reaches the bound is
//      searched, all workers sharing the problem's bound through one atomic word;
//   4. among the leaves with the best score, the one the reference's
//      depth-first search meets first is returned (SelectBestBody, fast_2d_search_device.h).
//
// Two strategies walk the tree: a work queue in ONE launch (fast_2d_queue.hip) and a chain of
// level-synchronous launches (fast_2d_levels.hip), which is also what a queue overflow falls back
// to.  RunBranchAndBound picks.
//
// This unit owns the scratch layout of a search (SearchMiscBytes, ReserveSearchScratch), the
// members of SearchRun (fast_2d_search.h), the depth-1 shortcut (SelectDepthOneKernel) and the
// fall-back ladder; it exports what fast_2d_internal.h declares of the search.
//
// The other units of the matcher: fast_2d_stack.hip (precomputation stack), fast_2d_coarse.hip
// (front end), fast_2d_match.hip (MatchBatch, tie resolution, C ABI); fast_2d_internal.h and
// fast_2d_device.h hold what they share.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <utility>

#include "fast_2d_search.h"

namespace cmx {
namespace {

// depth == 1: the lowest-resolution candidates are the leaves
// (BranchAndBound returns candidates[0], SM2/fast_...2d.cc:340-343).
__global__ void __launch_bounds__(1024)
SelectDepthOneKernel(const Fast2DProblem* __restrict__ problems,
                     const ProblemState* __restrict__ states, int n, BestLeaf* __restrict__ best,
                     ProblemState* __restrict__ states_out) {
  const int problem = blockIdx.x;
  const Fast2DProblem& P = problems[problem];
  __shared__ unsigned long long keys[16];
  __shared__ int s_total;
  if (threadIdx.x == 0) s_total = 0;
  __syncthreads();
  unsigned long long key = 0;
  int total = 0;
  for (int s = threadIdx.x; s < P.num_scans; s += blockDim.x) {
    total += P.coarse_dims[s].x * P.coarse_dims[s].y;
    const int2 b = P.scan_best[s];
    // larger sum first, then smaller scan index (generation order)
    const unsigned long long k = (static_cast<unsigned long long>(static_cast<unsigned>(b.x)) << 32) |
                                 static_cast<unsigned>(0x7fffffff - s);
    key = k > key ? k : key;
  }
  key = WaveMaxU64(key);
  total = WaveSum(total);
  if ((threadIdx.x & 63) == 0) {
    keys[threadIdx.x >> 6] = key;
    if (total) atomicAdd(&s_total, total);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ProblemState st = states[problem];
    st.coarse_total = s_total;
    states_out[problem] = st;
    for (int w = 1; w < 16; ++w) key = keys[w] > key ? keys[w] : key;
    BestLeaf b{};
    if (!states[problem].error && P.num_scans > 0) {
      const int s = 0x7fffffff - static_cast<int>(key & 0xffffffffu);
      const int2 sb = P.scan_best[s];
      const float score = ToScore(P, sb.x, n);
      if (score > P.min_score) {
        const int2 dims = P.coarse_dims[s];
        const int4 bd = P.bounds[s];
        b.found = 1; b.score = score; b.scan = s;
        b.dx = bd.x + sb.y / dims.y;
        b.dy = bd.z + sb.y % dims.y;
        b.ties = 1;
      }
    }
    best[problem] = b;
  }
}

// The scratch block of a search: the counters and the tail (SearchTail, fast_2d_search.h).
size_t SearchMiscBytes(int num) { return sizeof(Counters) + SearchTail::Bytes(num); }

// depth == 1: the lowest-resolution candidates are the leaves, no tree.
void RunDepthOne(SearchRun& run) {
  Workspace& ws = run.ws;
  SelectDepthOneKernel<<<run.num, 1024, 0, ws.stream>>>(
      run.batch.d_problems, run.batch.d_states, run.n, run.d_tail.best, run.d_tail.states);
  CMX_HIP(hipGetLastError());
  RecordEvent(ws.ev_end, ws.stream);
  run.FetchResults(false);
}

// (debug switch trace)
void TraceListSizes(const CountersSummary& h_counters) {
  fprintf(stderr, "[cmx trace] list sizes:");
  for (int st = 0; st < kMaxStages; ++st)
    if (h_counters.frontier_total[st])
      fprintf(stderr, " frontier[%d]=%d", st, h_counters.frontier_total[st]);
  long long leaves = 0;
  for (int k = 0; k < kSubLists; ++k) leaves += h_counters.leaves[k];
  fprintf(stderr, " leaves=%lld\n", leaves);
  const unsigned* q = h_counters.queue_stats;
  if (q[5])
    fprintf(stderr, "[cmx trace] work queue: %u chains (%u nodes from the list, %u popped), %u "
            "pushed, %u lost races, %u slot re-reads\n", q[5], q[4], q[0], q[3], q[1], q[2]);
}

}  // namespace

SearchRun::SearchRun(Workspace& ws, const PreparedBatch& batch, BatchResult* result)
    : ws(ws), batch(batch), result(result), num(batch.num_problems), n(batch.n),
      depth(batch.h_problems[0].depth) {
  // Nodes per frontier / leaf buffer.  The debug switch frontier_capacity shrinks the frontiers
  // (tests only) so that the overflow -> strict, chunked retry is exercised.
  const auto capacity = [](int v, int fallback) {
    return v >= kSubLists ? std::min(v, fallback) / kSubLists * kSubLists : fallback;
  };
  // 64 K nodes per problem (a weak match keeps ~30 k lowest-resolution nodes alive), at
  // least 2 M, at most 32 M (1 GB per buffer): HBM is not the scarce resource here, and
  // an overflow costs a whole second, chunked pass (64 submaps: 34 -> 20 ms per scan).
  const int frontier_default = static_cast<int>(
      std::min<long long>(1ll << 25, std::max<long long>(1ll << 21, 65536ll * num)));
  frontier_capacity = capacity(Debug().frontier_capacity, frontier_default);
  frontier_sub = frontier_capacity / kSubLists;
  const int leaf_capacity = capacity(0, 1 << 20);
  Node2D* d_leaves = ws.dev[12].ReserveAs<Node2D>(leaf_capacity);
  // Carved by ReserveSearchScratch before the first kernel of the call, which clears the
  // counters.
  d_counters = reinterpret_cast<Counters*>(batch.d_misc);
  d_tail = SearchTail(batch.d_misc + sizeof(Counters), num);
  leaf_list = NodeList{d_leaves, d_counters->leaves, leaf_capacity / kSubLists};
  // One D2H for the counters' summary + selection state + best leaves.
  h_tail = SearchTail(static_cast<char*>(ws.pinned[3].Reserve(SearchTail::Bytes(num))), num);
  // (depth > 1: the selecting workgroup stores the tail into h_tail itself)
  direct = Debug().no_direct_results == 0 && h_tail.bytes % sizeof(unsigned) == 0;
}

// The work queue reads and the level-synchronous chain ping-pongs: one buffer or two.
void SearchRun::ReserveFronts(int count) {
  d_front[0] = ws.dev[10].ReserveAs<Node2D>(frontier_capacity);
  if (count > 1) d_front[1] = ws.dev[11].ReserveAs<Node2D>(frontier_capacity);
}

void SearchRun::FetchResults(bool published) {
  if (!published)
    SmallCopyAsync(h_tail.base, d_tail.base, h_tail.bytes, /*to_device=*/false, ws.stream);
  const auto t0 = std::chrono::steady_clock::now();
  CMX_HIP(hipStreamSynchronize(ws.stream));
  g_host_wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(
                        std::chrono::steady_clock::now() - t0).count();
}

// Something was dropped (a full frontier / queue / leaf list).  Bounds found so far are real
// leaf scores and stay valid; the search is repeated in strict mode (prunes ties, records
// only improving leaves) over more, smaller chunks of scans.  The best leaf found so far is
// re-found by lowering the bound one ulp.
void SearchRun::PrepareStrictRetry() {
  CMX_REQUIRE(num_chunks < (1 << 12), "branch-and-bound overflow not resolvable");
  if (h_tail.summary->frontier_overflow) num_chunks *= 4;
  strict = 1;
  for (int p = 0; p < num; ++p) {
    const float floor_score = std::max(batch.h_problems[p].min_score, 0.f);
    unsigned floor_bits;
    std::memcpy(&floor_bits, &floor_score, sizeof(float));
    if (h_tail.states[p].best_bits > floor_bits) h_tail.states[p].best_bits -= 1;
  }
  CMX_HIP(hipMemcpyAsync(batch.d_states, h_tail.states, num * sizeof(ProblemState),
                         hipMemcpyHostToDevice, ws.stream));
  CMX_HIP(hipMemsetAsync(d_counters, 0, sizeof(Counters), ws.stream));
}

// Carved before the first kernel of a call so that it can clear the counters.
void ReserveSearchScratch(Workspace& ws, int num, PreparedBatch* batch) {
  batch->d_misc = static_cast<char*>(ws.dev[14].Reserve(SearchMiscBytes(num)));
  batch->num_counter_words = static_cast<int>(sizeof(Counters) / sizeof(int));
}

// (debug switch host_trace: where a caller's wall clock goes -- tools only)
thread_local long long g_host_wait_ns = 0;

// Full search of a prepared batch: the fall-back ladder.  Depth 1 has no tree; otherwise the dive,
// then the work queue if it can take the batch, then the level-synchronous chain if it cannot or
// after an overflow.
void RunBranchAndBound(Workspace& ws, const PreparedBatch& batch, BatchResult* result) {
  const int num = batch.num_problems;
  const int depth = batch.h_problems[0].depth;
  for (const Fast2DProblem& P : batch.h_problems)
    CMX_REQUIRE(P.depth == depth, "all matchers of a batch must share branch_and_bound_depth");
  SearchRun run(ws, batch, result);
  if (depth == 1) {
    RunDepthOne(run);
  } else {
    // (the launches of the search proper: one turn from the dive to the tree launch)
    std::unique_ptr<LaunchTurn> turn(new LaunchTurn);
    LaunchDive(run);
    bool searched = false;
    if (QueueSearchPossible(run)) {
      switch (RunQueueSearch(run, std::move(turn))) {
        case QueueOutcome::kDone:
          searched = true;
          break;
        case QueueOutcome::kLeafOverflow:
          run.PrepareStrictRetry();
          break;
        case QueueOutcome::kQueueOverflow:
          // A sub-queue filled up (it holds 1 K nodes: one wavefront's siblings -- landscapes where
          // nearly everything ties fill it).  The level-synchronous path has room for millions of
          // nodes and reproduces the reference's order among ANY number of tied leaves, which the
          // strict retry cannot: it runs first, from the bounds found so far (real leaf scores),
          // with the lists cleared.
          CMX_HIP(hipMemsetAsync(run.d_counters, 0, sizeof(Counters), ws.stream));
          break;
      }
    }
    turn.reset();      // (the level-synchronous launches issue as they come)
    if (!searched) RunLevelSynchronous(run);
  }

  result->best.assign(run.h_tail.best, run.h_tail.best + num);
  result->states.assign(run.h_tail.states, run.h_tail.states + num);
  if (depth > 1) {
    if (batch.trace && batch.trace->enabled()) TraceListSizes(*run.h_tail.summary);
    result->d_leaves = run.leaf_list.nodes;
    result->leaf_sub_capacity = run.leaf_list.sub_capacity;
    result->leaf_counts.assign(run.h_tail.summary->leaves, run.h_tail.summary->leaves + kSubLists);
  }
  result->device_ms = ElapsedMs(ws.ev_begin, ws.ev_end);
  result->dominant_ms = ElapsedMs(ws.ev_k0, ws.ev_k1);
  if (result->expansion_launches > 0) result->expansion_ms = ElapsedMs(ws.ev_x0, ws.ev_x1);
}

}  // namespace cmx
