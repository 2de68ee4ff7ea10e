// What the units of the fast 2D tree search hand each other on the host:
//   fast_2d.hip          the driver: scratch layout, depth 1, the fall-back ladder (RunBranchAndBound)
//   fast_2d_seed.hip     what runs before either strategy: seeds + dive, lowest-resolution filter
//                        (and the level-synchronous strategy's SubtreeKernel, DiveKernel's sibling)
//   fast_2d_levels.hip   the level-synchronous strategy
//   fast_2d_queue.hip    the work-queue strategy
// A search is one SearchRun, which the driver builds and the stage functions below take by
// reference; every unit launches its own kernels only.  What the rest of the matcher sees of the
// search is in fast_2d_internal.h.
//
// (SearchTail and SearchRun name types of the kernels' unnamed namespace, fast_2d_search_device.h:
// every unit has its own, identical copy of those, so the layouts agree.)
#ifndef CMX_FAST_2D_SEARCH_H_
#define CMX_FAST_2D_SEARCH_H_

#include <memory>

#include "fast_2d_internal.h"
#include "fast_2d_search_device.h"

namespace cmx {

// ---------------------------------------------------------------------------
// The scratch block of a search
// ---------------------------------------------------------------------------
// d_misc: Counters | CountersSummary | SelectState[num] | BestLeaf[num] | ProblemState[num].
// Everything behind the Counters -- the tail -- is what the host reads after a search: it travels
// back in one D2H, or the selecting workgroup stores it into the caller's pinned buffer itself.
// The one description of that layout, for the device block and for its pinned host copy.
struct SearchTail {
  static_assert(sizeof(Counters) % 16 == 0 && sizeof(CountersSummary) % 8 == 0, "alignment");
  static size_t Bytes(int num) {
    return sizeof(CountersSummary) +
           num * (sizeof(SelectState) + sizeof(BestLeaf) + sizeof(ProblemState));
  }
  SearchTail() = default;
  SearchTail(char* base, int num)
      : base(base), bytes(Bytes(num)),
        summary(reinterpret_cast<CountersSummary*>(base)),
        sel(reinterpret_cast<SelectState*>(summary + 1)),
        best(reinterpret_cast<BestLeaf*>(sel + num)),
        states(reinterpret_cast<ProblemState*>(best + num)) {}
  unsigned* words() const { return reinterpret_cast<unsigned*>(base); }
  int num_words() const { return static_cast<int>(bytes / sizeof(unsigned)); }
  char* base = nullptr;
  size_t bytes = 0;
  CountersSummary* summary = nullptr;
  SelectState* sel = nullptr;
  BestLeaf* best = nullptr;
  ProblemState* states = nullptr;
};

// ---------------------------------------------------------------------------
// One search of a prepared batch
// ---------------------------------------------------------------------------
// What the stages share and hand to each other: the lists and the scratch block of the call, and
// the state of the overflow fall-back (`strict`, `num_chunks`).  (Members: fast_2d.hip.)
struct SearchRun {
  SearchRun(Workspace& ws, const PreparedBatch& batch, BatchResult* result);
  // The frontier buffers, `count` (1 or 2) of them: reserved by the strategy that runs.
  void ReserveFronts(int count);
  // Stage k reads list k and appends to list k+1 (buffers ping-pong, counters
  // do not: they are all zeroed by the first kernel of the call).
  NodeList Front(int stage) const {
    return NodeList{d_front[stage & 1], d_counters->frontier[stage], frontier_sub};
  }
  void Mark(const char* name) const { if (batch.trace) batch.trace->Mark(name); }
  // Where the selecting workgroup stores the tail itself (null: the host fetches it).
  unsigned* PublishTo() const { return direct ? h_tail.words() : nullptr; }
  void FetchResults(bool published);
  void PrepareStrictRetry();

  Workspace& ws;
  const PreparedBatch& batch;
  BatchResult* result;
  const int num, n, depth;
  int frontier_capacity, frontier_sub;    // nodes per frontier buffer / per sub-list of one
  Node2D* d_front[2] = {nullptr, nullptr};
  NodeList leaf_list;
  Counters* d_counters;
  SearchTail d_tail, h_tail;
  bool direct;                            // the last kernel stores the tail into h_tail itself
  int strict = 0;                         // 1: prune ties, record only improving leaves
  int num_chunks = 1;                     // the scans go through the level-synchronous path in chunks
};

// ---- fast_2d_seed.hip
// Whether a wavefront can walk chains of this batch's nodes (fast_2d_chain_device.h).
bool ChainWalkPossible(const SearchRun& run);
// Seeds and their greedy descents: real leaf scores, the first bound of every problem.  A
// wavefront per dive wherever ChainWalkPossible, a workgroup per dive otherwise.
void LaunchDive(SearchRun& run);
// The lowest-resolution nodes of chunk `chunk` of `num_chunks` that reach the bound, into
// run.Front(0).
void LaunchFilter(SearchRun& run, int chunk, int num_chunks, int strict, int affinity);
// A depth-first stage of the level-synchronous strategy: the subtrees below the nodes of
// run.Front(stage), on `blocks` workgroups; nodes that reach `stop_level` (> 0) go to
// run.Front(stage + 1), leaves to run.leaf_list.
void LaunchSubtree(SearchRun& run, int stage, int stop_level, int strict, int blocks);

// ---- fast_2d_queue.hip
// Whether the work queue can take this batch.
bool QueueSearchPossible(const SearchRun& run);
enum class QueueOutcome { kDone, kLeafOverflow, kQueueOverflow };
// Filter + ONE launch for the whole tree and the selection; the results are in run.h_tail
// whatever the outcome.  Takes over the caller's turn at the launch path (held since the dive)
// and gives it up behind the tree launch, before it waits for the results.
QueueOutcome RunQueueSearch(SearchRun& run, std::unique_ptr<LaunchTurn> turn);

// ---- fast_2d_levels.hip
// Filter, wave stages, subtree stages, selection: over run.num_chunks chunks of scans, and once
// more in strict mode (run.PrepareStrictRetry) for as long as a list overflows.
void RunLevelSynchronous(SearchRun& run);

}  // namespace cmx

#endif  // CMX_FAST_2D_SEARCH_H_
