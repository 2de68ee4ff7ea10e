// FastCorrelativeScanMatcher2D on gfx950: the work-queue strategy of the tree search.
//
// Owns the queue (TreeQueue and its slot / granule / push / pop / steal helpers) and
// TreeQueueKernel<kChain>, which walks the whole tree and selects in its last workgroup.  Exports
// QueueSearchWanted (fast_2d_internal.h) and the stage functions QueueSearchPossible and
// RunQueueSearch (fast_2d_search.h).
//
// ONE launch behind the dive and the lowest-resolution filter (fast_2d_seed.hip) instead of the
// wave / subtree / select chain of launches of the level-synchronous strategy
// (fast_2d_levels.hip), which is what an overflow of the queue falls back to.
//
// A worker is a WAVEFRONT.  It takes a node from the queue and walks a CHAIN from it: expand
// (one quad gather per point, the node's scan held in registers: 16 cells per lane), continue
// with the best child, hand the other children that can still matter to the queue; a chain ends
// at a leaf (which raises the problem's bound) or when no child reaches the bound.  Every chain is
// a greedy dive, so the bound tightens as fast as the reference's depth-first search tightens it
// (SM2/fast_...2d.cc:335-378), while thousands of chains run at once.  The level-synchronous
// kernels expand a whole level against the bound the dive has left: 93 000 node expansions on a
// hard scan where the reference's own order needs 40 000.
//
// The queue: kQueues sub-queues (a control word takes ~90 atomics per microsecond).  A slot is
// eight 8-byte granules {tag = the call's epoch, word of the node}, each written by ONE
// agent-scope store and polled with agent-scope loads: the data is its own flag, no fence
// (MI355X guide, inter-workgroup hand-off R2).  push: one atomic add on `reserved`, then the
// granules.  pop: look at every sub-queue (one wave-wide load), CAS `head` of one that has
// something -- never a ticket for a node that does not exist yet, so a worker NEVER waits for
// work: a wavefront that finds every sub-queue empty is done for good.  That is safe because
// whoever publishes a node looks again when its own chain has ended, and it is what makes eight
// such launches share the chip: no wavefront spins on another one's progress (only, briefly,
// on the granules of a slot that has been reserved and is being written).  The last workgroup to
// run out of work selects the best leaves and publishes the results (SelectBestBody).
// Slots are never reused within a call; a sub-queue that fills up sets frontier_overflow and
// the driver (fast_2d.hip) repeats the search on the level-synchronous path.
#include <algorithm>
#include <type_traits>
#include <utility>

#include "fast_2d_chain_device.h"
#include "fast_2d_search.h"

namespace cmx {
namespace {

struct TreeQueue {
  unsigned long long* slots;     // [kQueues][capacity][8] granules
  int capacity;                  // nodes per sub-queue
  unsigned epoch;                // tag of this call (never 0; the buffer only holds older tags)
};

__device__ __forceinline__ unsigned long long* QueueSlot(const TreeQueue& Q, int q, int slot) {
  return Q.slots + (static_cast<size_t>(q) * Q.capacity + slot) * 8;
}

__device__ __forceinline__ void StoreGranule(unsigned long long* g, unsigned epoch, unsigned value) {
  __hip_atomic_store(g, (static_cast<unsigned long long>(epoch) << 32) | value, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// One lane writes one node (the calling lanes hold different nodes).
__device__ __forceinline__ void StoreNodeGranules(const TreeQueue& Q, int q, int slot,
                                                  const Node2D& nd) {
  unsigned long long* g = QueueSlot(Q, q, slot);
  StoreGranule(g + 0, Q.epoch, static_cast<unsigned>(nd.problem));
  StoreGranule(g + 1, Q.epoch, static_cast<unsigned>(nd.scan));
  StoreGranule(g + 2, Q.epoch, static_cast<unsigned>(nd.dx));
  StoreGranule(g + 3, Q.epoch, static_cast<unsigned>(nd.dy));
  StoreGranule(g + 4, Q.epoch, __float_as_uint(nd.score));
  StoreGranule(g + 5, Q.epoch, static_cast<unsigned>(nd.coarse_index));
  StoreGranule(g + 6, Q.epoch, nd.path);
  StoreGranule(g + 7, Q.epoch, __float_as_uint(nd.coarse_score));
}

// Wave-wide push of the lanes with `keep` to sub-queue q: one reservation, slots in lane order.
// A full sub-queue raises the overflow flag (the reservation stands: poppers never look beyond
// `capacity`; slots below it are still filled, so every reserved slot below it IS published).
__device__ __forceinline__ void QueuePush(const TreeQueue& Q, Counters* __restrict__ counters,
                                          int q, bool keep, const Node2D& nd) {
  const int lane = threadIdx.x & 63;
  const unsigned long long mask = __ballot(keep);
  if (mask == 0) return;
  const int m = __popcll(mask);
  int first = 0;
  if (lane == 0)
    first = __hip_atomic_fetch_add(&counters->queue[q].reserved, m, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
  first = __builtin_amdgcn_readfirstlane(first);
  // (agent-scope stores: the selecting workgroup of this launch reads the flag)
  if (first + m > Q.capacity && lane == 0)
    __hip_atomic_store(&counters->frontier_overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (keep) {
    const int slot = first + __popcll(mask & ((1ull << lane) - 1));
    if (slot < Q.capacity) StoreNodeGranules(Q, q, slot, nd);
  }
}

// Lanes 0..7 sweep the granules of a slot that has been taken -- it is reserved, i.e. written or
// being written -- until every tag is this call's; the node comes back wave-uniform.
__device__ __forceinline__ void ReadSlot(const TreeQueue& Q, int q, int slot, Node2D* out,
                                         unsigned* slot_rereads) {
  const int lane = threadIdx.x & 63;
  const unsigned long long* g = QueueSlot(Q, q, slot);
  unsigned word = 0;
  for (;;) {
    bool ok = true;
    if (lane < 8) {
      const unsigned long long x = LoadAgent(&g[lane]);
      word = static_cast<unsigned>(x);
      ok = static_cast<unsigned>(x >> 32) == Q.epoch;
    }
    if (__all(ok)) break;
    ++*slot_rereads;
    __builtin_amdgcn_s_sleep(2);
  }
  out->problem = static_cast<int>(__builtin_amdgcn_readlane(word, 0));
  out->scan = static_cast<int>(__builtin_amdgcn_readlane(word, 1));
  out->dx = static_cast<int>(__builtin_amdgcn_readlane(word, 2));
  out->dy = static_cast<int>(__builtin_amdgcn_readlane(word, 3));
  out->score = __uint_as_float(__builtin_amdgcn_readlane(word, 4));
  out->coarse_index = static_cast<int>(__builtin_amdgcn_readlane(word, 5));
  out->path = __builtin_amdgcn_readlane(word, 6);
  out->coarse_score = __uint_as_float(__builtin_amdgcn_readlane(word, 7));
}

__device__ __forceinline__ bool TakeSlot(Counters* __restrict__ counters, int q, int slot) {
  int got = 0;
  if ((threadIdx.x & 63) == 0) {
    int expected = slot;
    got = __hip_atomic_compare_exchange_strong(&counters->queue[q].head, &expected, slot + 1,
                                               __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT) ? 1 : 0;
  }
  return __builtin_amdgcn_readfirstlane(got) != 0;
}

// The wavefront's HOME sub-queue (the only one it pushes to).  false: it is empty -- and, no
// push of this wavefront being outstanding, it stays empty: the wavefront may leave.
__device__ __forceinline__ bool PopHome(const TreeQueue& Q, Counters* __restrict__ counters,
                                        int home, Node2D* out, unsigned* lost_races,
                                        unsigned* slot_rereads) {
  for (;;) {
    const unsigned long long hr =
        LoadAgent(reinterpret_cast<const unsigned long long*>(&counters->queue[home].head));
    const int head = static_cast<int>(hr & 0xffffffffu);
    const int reserved = min(static_cast<int>(hr >> 32), Q.capacity);
    if (reserved <= head) return false;
    if (TakeSlot(counters, home, head)) {
      ReadSlot(Q, home, head, out, slot_rereads);
      return true;
    }
    ++*lost_races;          // a thief was faster: look again (the sub-queue only loses nodes that way)
  }
}

// Somebody else's node: up to `windows` windows of 64 sub-queues from a start that differs per
// wavefront and attempt, one of the busy sub-queues of a window (not the first: every thief
// would race for the same word).  A thief that loses `max_lost` races, or finds its windows
// empty, gives up: supply is short then, and whoever published a node takes it in the end.
__device__ __forceinline__ bool Steal(const TreeQueue& Q, Counters* __restrict__ counters,
                                      int home, int queues, unsigned salt, int windows,
                                      int max_lost, Node2D* out, unsigned* lost_races,
                                      unsigned* slot_rereads) {
  const int lane = threadIdx.x & 63;
  int lost = 0;
  for (int w = 0; w < windows; ++w) {
    const int base = static_cast<int>((static_cast<unsigned>(home) * 2654435761u + salt * 40503u + w * 64u) %
                                      static_cast<unsigned>(queues));
    const int mine = (base + lane) % queues;
    const unsigned long long hr =
        LoadAgent(reinterpret_cast<const unsigned long long*>(&counters->queue[mine].head));
    const int head = static_cast<int>(hr & 0xffffffffu);
    const int reserved = min(static_cast<int>(hr >> 32), Q.capacity);
    const unsigned long long avail = __ballot(reserved > head);
    if (avail == 0) continue;
    int skip = static_cast<int>((salt + home) % static_cast<unsigned>(__popcll(avail)));
    unsigned long long rest = avail;
    while (skip-- > 0) rest &= rest - 1;
    const int l = __ffsll(static_cast<long long>(rest)) - 1;
    const int q = (base + l) % queues;
    const int slot = __builtin_amdgcn_readlane(head, l);
    if (TakeSlot(counters, q, slot)) {
      ReadSlot(Q, q, slot, out, slot_rereads);
      return true;
    }
    ++*lost_races;
    if (++lost >= max_lost) return false;
    --w;                    // the same window again (another sub-queue of it: salt)
    ++salt;
  }
  return false;
}

// One leaf record, stored so that the selecting workgroup of the SAME launch reads it.
__device__ __forceinline__ void RecordLeafAgent(const Node2D& leaf, const NodeList& leaves,
                                                int sub, Counters* __restrict__ counters) {
  const int slot = ListReserve(leaves, sub, 1);
  if (slot >= leaves.sub_capacity) {
    __hip_atomic_store(&counters->leaf_overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  unsigned long long v[4];
  __builtin_memcpy(v, &leaf, sizeof(Node2D));
  unsigned long long* at = reinterpret_cast<unsigned long long*>(
      &leaves.nodes[static_cast<size_t>(sub) * leaves.sub_capacity + slot]);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    __hip_atomic_store(&at[k], v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// kChain (debug switch fast2d_chain): 1 = the bound (`best_bits`) loaded and waited for wherever it
// is used (the parity partner); 0 = two of those waits taken out.  The bound only rises, so a value
// that is a trip older prunes a little less and decides nothing; the queue protocol, the order of
// the list and every other load are the same either way.
//   * The best node of a list round is picked before the bound is looked at (the choice never
//     depended on it), and ONE load of the bound then decides about the round and about the node
//     (kChain = 1: a load for the round, a second one for the node).
//   * A chain step loads the bound WITH the first gathers of its level, not behind the child
//     scores: one trip to memory less per step.
// What else was measured and left out: DESIGN 5.2.
template <int kChain>
__global__ void __launch_bounds__(256)
TreeQueueKernel(const Fast2DProblem* __restrict__ problems, ProblemState* __restrict__ states, int n,
                NodeList in, TreeQueue Q, NodeList leaves, Counters* __restrict__ counters,
                SelectState* __restrict__ sel, BestLeaf* __restrict__ best_out, int num_problems,
                ProblemState* __restrict__ states_out, CountersSummary* __restrict__ summary,
                const unsigned* __restrict__ tail_dev, unsigned* __restrict__ tail_host,
                int tail_words, int counters_trace, int max_lost) {
  static_assert(sizeof(Node2D) == 32, "a node is eight words: eight granules, four leaf stores");
  static_assert(kChain == 0 || kChain == 1, "0: the lean step and pop, 1: every trip waited for");
  constexpr bool kLean = kChain == 0;
  const int lane = threadIdx.x & 63;
  const int wave_id = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int num_waves = gridDim.x * 4;
  const int queues = min(num_waves, kQueues);          // sub-queues in use
  const int home = wave_id % queues;
  unsigned steals = 0;
  unsigned long long scored = 0, expanded = 0;
  unsigned gathers = 0;
  unsigned q_pops = 0, q_lost = 0, q_rereads = 0, q_pushed = 0, q_listed = 0, q_chains = 0;
  int stat_problem = -1;
  const auto flush_stats = [&]() {
    if (lane == 0 && stat_problem >= 0 && expanded) {
      ProblemState& st = states[stat_problem];
      atomicAdd(&st.scored_shard[wave_id & (kStatShards - 1)], scored);
      atomicAdd(&st.expanded_shard[wave_id & (kStatShards - 1)], expanded);
    }
    scored = expanded = 0;
  };
  // Phase 1: this wavefront's share of the filter's list (written by the launch before: plain
  // loads), node i of the interleaved sub-lists for i = wave, wave + W, ...  Phase 2: the queue.
  // A static share is safe here because nobody ever waits for anybody: a workgroup that is not
  // resident yet simply walks its share when it gets there.
  // BEST FIRST within the share: 64 nodes of it at a time, one per lane (one wave-wide load), the
  // highest score among them taken next -- and the round dropped as soon as that score is below
  // the bound.  Every wavefront starts with the best node it owns, so the first thousand chains
  // are dives from the best thousand nodes of the list and the bound is close to its final value
  // when they end; the rest of the list then dies at a compare.  (In list order -- the filter's,
  // i.e. by rotation -- a hard scan expanded 23 000 nodes where 2 400 suffice with the final
  // bound known from the start: profiles/r06_queue_development.txt.)
  const int in_slots = ListMaxCount(in) * kSubLists;
  int round = 0;
  Node2D mine{};               // this lane's node of the current round
  unsigned mine_bits = 0;      // its score's bits; 0: none (taken, or no such node)
  bool round_loaded = false, share_done = false;
  bool pushed_any = false;
  Node2D nd;
  unsigned listed_top = 0;     // kLean: the score bits of the node taken from the list round
  for (;;) {
    bool have = false;
    while (!have && !share_done) {
      if (!round_loaded) {
        // (wave-uniform: the first lane's index is the smallest of the round)
        if (wave_id + static_cast<long long>(round) * 64 * num_waves >= in_slots) { share_done = true; break; }
        const long long i = wave_id + (static_cast<long long>(round) * 64 + lane) * num_waves;
        ++round;
        mine_bits = 0;
        if (i < in_slots) {
          const int in_sub = static_cast<int>(i & (kSubLists - 1)), j = static_cast<int>(i / kSubLists);
          if (j < min(in.counts[in_sub * kCountStride], in.sub_capacity)) {
            mine = in.nodes[static_cast<size_t>(in_sub) * in.sub_capacity + j];
            mine_bits = max(__float_as_uint(fmaxf(mine.score, 0.f)), 1u);
          }
        }
        round_loaded = true;
      }
      const unsigned top = static_cast<unsigned>(WaveMax(static_cast<int>(mine_bits)));
      // (the bound of problem 0 only prunes rounds of a single search; batches check per node)
      // kLean: which node is next does not depend on the bound, so it is taken first and the round
      // is tested below, against the bound loaded for the node
      float bound_now = 0.f;
      if constexpr (kLean) listed_top = top;
      else bound_now = __uint_as_float(LoadAgent(&states[0].best_bits));
      if (top == 0 || (!kLean && num_problems == 1 && __uint_as_float(top) < bound_now)) {
        round_loaded = false;      // nothing left in this round that can matter
        continue;
      }
      const int l = __ffsll(static_cast<long long>(__ballot(mine_bits == top))) - 1;
      nd.problem = __builtin_amdgcn_readlane(mine.problem, l);
      nd.scan = __builtin_amdgcn_readlane(mine.scan, l);
      nd.dx = __builtin_amdgcn_readlane(mine.dx, l);
      nd.dy = __builtin_amdgcn_readlane(mine.dy, l);
      nd.score = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(mine.score), l));
      nd.coarse_index = __builtin_amdgcn_readlane(mine.coarse_index, l);
      nd.path = __builtin_amdgcn_readlane(mine.path, l);
      nd.coarse_score =
          __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(mine.coarse_score), l));
      if (lane == l) mine_bits = 0;
      have = true;
      if constexpr (!kLean) ++q_listed;
    }
    if (!have) {
      // its own sub-queue first (whoever publishes nodes is who guarantees that they are taken:
      // by a thief, or in the end by itself), then somebody else's; nothing there, or the races
      // lost: this wavefront is done -- its own sub-queue is empty and stays so
      if (!(pushed_any && PopHome(Q, counters, home, &nd, &q_lost, &q_rereads)) &&
          !Steal(Q, counters, home, queues, ++steals, 2, max_lost, &nd, &q_lost, &q_rereads))
        break;
      ++q_pops;
    }
    const int problem = __builtin_amdgcn_readfirstlane(NodeProblem(nd));
    const Fast2DProblem& P = problems[problem];
    ProblemState& st = states[problem];
    float best = __uint_as_float(LoadAgent(&st.best_bits));
    if constexpr (kLean) {
      if (have) {
        // from the list: the round's best node.  Below the bound (a single search's), nothing
        // left in the round can matter
        if (num_problems == 1 && __uint_as_float(listed_top) < best) {
          round_loaded = false;
          continue;
        }
        ++q_listed;
      }
    }
    if (nd.score < best) continue;                       // the bound has risen since the push
    if (problem != stat_problem) { flush_stats(); stat_problem = problem; }
    ++q_chains;
    // the node's scan: 16 cells per lane, kept for the whole chain
    uint32_t cell[kChainCells];
    LoadChainCells<false>(P, n, nd.scan, cell);
    const int4 bd = P.bounds[nd.scan];
    const float min_score = P.min_score;
    for (;;) {                                           // the chain
      const int child_level = __builtin_amdgcn_readfirstlane(NodeLevel(nd) - 1);
      const int ndx = __builtin_amdgcn_readfirstlane(nd.dx), ndy = __builtin_amdgcn_readfirstlane(nd.dy);
      const ChainLevel L = MakeChainLevel(P, child_level, ndx, ndy);
      const int half = L.half;
      const bool vx = ndx + half <= bd.y, vy = ndy + half <= bd.w;
      const int parent_ub = SumUpperBound(P, nd.score, n);
      // (the level-(l+1) cell is the maximum of all four level-l cells whatever the bounds say, so
      // the early-exit bound below holds with the children beyond the search bounds summed)
      uint32_t even = 0, odd = 0;
      int seen_max = 0;
      bool dead = false;
      // The first 256 points, then -- unless no child can reach the bound any more -- ALL the
      // others in flight at once: two trips to memory per expansion at most (a check after every
      // 256 points was four).
      const auto gather = [&](auto first_tag, auto count_tag) {
        ChainGather<decltype(first_tag)::value, decltype(count_tag)::value, true>(L, cell, &even,
                                                                                  &odd, &seen_max);
      };
      unsigned step_bits = 0;
      if constexpr (kLean) step_bits = LoadAgent(&st.best_bits);
      gather(std::integral_constant<int, 0>{}, std::integral_constant<int, 4>{});
      gathers += 4;
      if constexpr (kLean) best = fmaxf(best, __uint_as_float(step_bits));
      if (n > 4 * kWave) {
        // what the best child of this lane's points still lacks to the parent (see
        // ExpandWaveKernel): no child can reach the bound -> the rest of the gathers is skipped
        const int most = static_cast<int>(max(max(even & 0xffffu, even >> 16),
                                              max(odd & 0xffffu, odd >> 16)));
        if (ToScore(P, parent_ub - WaveSum(seen_max - most), n) < best) {
          dead = true;
        } else {
          if (n > 8 * kWave) {
            gather(std::integral_constant<int, 4>{}, std::integral_constant<int, 12>{});
            gathers += 12;
          } else {
            gather(std::integral_constant<int, 4>{}, std::integral_constant<int, 4>{});
            gathers += 4;
          }
        }
      }
      ++expanded;
      scored += (1 + (vx ? 1 : 0)) * (1 + (vy ? 1 : 0));
      if (dead) break;
      const int total[4] = {WaveSum(static_cast<int>(even & 0xffffu)), WaveSum(static_cast<int>(odd & 0xffffu)),
                            WaveSum(static_cast<int>(even >> 16)), WaveSum(static_cast<int>(odd >> 16))};
      // lane k < 4 is child k = 2 * x-step + y-step (generation order: x outer, y inner)
      float sc[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool valid = ((k >> 1) == 0 || vx) && ((k & 1) == 0 || vy);
        sc[k] = valid ? ToScore(P, total[k], n) : -1.f;
      }
      const int k = lane & 3;
      const float mine = k == 0 ? sc[0] : (k == 1 ? sc[1] : (k == 2 ? sc[2] : sc[3]));
      int rank = 0;
#pragma unroll
      for (int o = 0; o < 4; ++o)
        if (o != k && sc[o] >= 0.f && (sc[o] > mine || (sc[o] == mine && o < k))) ++rank;
      if constexpr (!kLean) best = fmaxf(best, __uint_as_float(LoadAgent(&st.best_bits)));
      const bool keep = lane < 4 && mine >= 0.f && mine >= best;
      // the best valid child (rank 0; child 0 is always valid)
      const int kbest = __ffsll(static_cast<long long>(__ballot(lane < 4 && mine >= 0.f && rank == 0))) - 1;
      Node2D child;
      child.problem = problem | (child_level << 24);
      child.scan = nd.scan;
      child.dx = nd.dx + (k >> 1) * half;
      child.dy = nd.dy + (k & 1) * half;
      child.score = mine;
      child.coarse_index = nd.coarse_index;
      child.path = nd.path | (static_cast<unsigned>(rank) << (2 * child_level));
      child.coarse_score = nd.coarse_score;
      const bool best_kept = (__ballot(keep) >> kbest) & 1ull;
      if (child_level == 0) {
        // leaves: only the first-best child can be returned by the reference (:340-343 after the
        // stable sort of :331-332)
        if (best_kept && lane == kbest && child.score > min_score) {
          RecordLeafAgent(child, leaves, wave_id & (kSubLists - 1), counters);
          atomicMax(&st.best_bits, __float_as_uint(child.score));
        }
        break;
      }
      if (!best_kept) break;                              // the best child is below the bound: all are
      // the other children that can still matter go to the queue ...
      const bool others = keep && lane != kbest;
      if (__ballot(others)) {
        QueuePush(Q, counters, home, others, child);
        pushed_any = true;
        q_pushed += __popcll(__ballot(others));
      }
      // ... and the chain goes on with the best one
      nd.problem = child.problem;
      nd.dx = __builtin_amdgcn_readlane(child.dx, kbest);
      nd.dy = __builtin_amdgcn_readlane(child.dy, kbest);
      nd.score = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(child.score), kbest));
      nd.path = __builtin_amdgcn_readlane(child.path, kbest);
    }
  }
  // ---- out of work.  The work counters of the four wavefronts go out as one set of atomics per
  // workgroup (one per WAVEFRONT on a word per problem took 20 us of a 2048-wavefront launch: a
  // word takes ~90 atomics per microsecond), then the last workgroup to get here selects and
  // publishes. ---------------------------------------------------------------------------------
  __shared__ unsigned long long s_scored[4], s_expanded[4];
  __shared__ unsigned s_gathers[4];
  __shared__ unsigned s_queue_stats[8];
  __shared__ int s_problem[4];
  if (threadIdx.x < 8) s_queue_stats[threadIdx.x] = 0;
  __syncthreads();
  if (lane == 0 && counters_trace) {
    atomicAdd(&s_queue_stats[0], q_pops);
    atomicAdd(&s_queue_stats[1], q_lost);
    atomicAdd(&s_queue_stats[2], q_rereads);
    atomicAdd(&s_queue_stats[3], q_pushed);
    atomicAdd(&s_queue_stats[4], q_listed);
    atomicAdd(&s_queue_stats[5], q_chains);
  }
  __shared__ int s_last;
  if (lane == 0) {
    const int w = threadIdx.x >> 6;
    s_scored[w] = scored;
    s_expanded[w] = expanded;
    s_gathers[w] = gathers;
    s_problem[w] = expanded ? stat_problem : -1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wavefront's stores have landed
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned g = 0;
    for (int w = 0; w < 4; ++w) {
      g += s_gathers[w];
      if (s_problem[w] < 0) continue;
      unsigned long long sc = s_scored[w], ex = s_expanded[w];
      for (int v = w + 1; v < 4; ++v)
        if (s_problem[v] == s_problem[w]) { sc += s_scored[v]; ex += s_expanded[v]; s_problem[v] = -1; }
      ProblemState& st = states[s_problem[w]];
      atomicAdd(&st.scored_shard[blockIdx.x & (kStatShards - 1)], sc);
      atomicAdd(&st.expanded_shard[blockIdx.x & (kStatShards - 1)], ex);
    }
    if (g) atomicAdd(&counters->gathers_shard[(blockIdx.x & 15) * kCountStride], g);
    if (counters_trace)
      for (int k = 0; k < 6; ++k)
        if (s_queue_stats[k])
          atomicAdd(&counters->queue_stats[(blockIdx.x & 15) * kCountStride + k], s_queue_stats[k]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = __hip_atomic_fetch_add(&counters->blocks_done, 1, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT) == static_cast<int>(gridDim.x) - 1;
  }
  __syncthreads();
  if (!s_last) return;
  SelectBestBody<true>(leaves, states, sel, best_out, num_problems, states_out, counters, summary);
  if (tail_host == nullptr) return;
  __threadfence();
  __syncthreads();
  for (int i = threadIdx.x; i < tail_words; i += blockDim.x)
    tail_host[i] = __hip_atomic_load(&tail_dev[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// The work-queue tree search (TreeQueueKernel) holds a scan in registers, 16 cells per lane.
// Debug switch fast2d_queue: 2 = the chain of level-synchronous launches (fast_2d_levels.hip: the
// parity partner, and the path a queue overflow falls back to).
// Batches of four or more problems stay on the level-synchronous launches: wide frontiers of many
// problems keep the chip busy there, and they measure faster (16 submaps: 1.4 against 2.7 ms).
bool QueueSearchWanted(int n, int num) {
  return Debug().fast2d_queue != 2 && n <= kChainCells * kWave && (num < 4 || Debug().fast2d_queue == 1);
}

// Whether the work queue can take this batch: its wavefronts walk chains, of stored cells.
bool QueueSearchPossible(const SearchRun& run) {
  bool queue_ok = QueueSearchWanted(run.n, run.num) && ChainWalkPossible(run);
  for (const Fast2DProblem& P : run.batch.h_problems)
    queue_ok = queue_ok && (P.recompute_scans == 0 || P.store_scans != 0);
  return queue_ok;
}

// Filter + ONE launch for the whole tree and the selection.  Takes over the caller's turn at the
// launch path (held since the dive) and gives it up behind the tree launch, before it waits for
// the results.
QueueOutcome RunQueueSearch(SearchRun& run, std::unique_ptr<LaunchTurn> turn) {
  Workspace& ws = run.ws;
  const PreparedBatch& batch = run.batch;
  BatchResult* result = run.result;
  const int num = run.num, n = run.n;
  // 16 K nodes per sub-queue (1 M nodes, 64 MB) for up to 16 problems, 64 K per problem
  // beyond; slots are not reused within a call.
  const long long wanted = std::max<long long>(1ll << 20, 65536ll * num);
  int sub_capacity = static_cast<int>(std::min<long long>(wanted, 1ll << 23) / kQueues);
  if (Debug().fast2d_queue_capacity > 0) sub_capacity = Debug().fast2d_queue_capacity;
  TreeQueue queue;
  queue.capacity = sub_capacity;
  queue.slots = static_cast<unsigned long long*>(ws.tagged[0].Acquire(
      static_cast<size_t>(kQueues) * sub_capacity * 8 * sizeof(unsigned long long), ws.stream,
      &queue.epoch));
  run.ReserveFronts(1);
  LaunchFilter(run, 0, 1, /*strict=*/0, /*affinity=*/0);
  // (events only under the debug switch `timing`: RecordEvent is a no-op otherwise)
  RecordEvent(ws.ev_x0, ws.stream);
  // One workgroup per CU: 1024 wavefronts.  More of them shorten a single hard search (512
  // workgroups: 240 against 290 us on the hardest of the bench's eight scans) and cost the
  // eight-thread line more than that (17 200 against 19 300 matches/s): wavefronts that find
  // nothing to steal are pure overhead for the searches that share the chip.
  const int blocks = Debug().fast2d_queue_blocks > 0
                         ? Debug().fast2d_queue_blocks
                         : std::min(2048, 256 * std::max(1, (num + 3) / 4));
  // (debug switch fast2d_chain: 1 = the bound waited for wherever it is used, the parity partner)
  const auto tree_kernel = Debug().fast2d_chain == 1 ? TreeQueueKernel<1> : TreeQueueKernel<0>;
  tree_kernel<<<blocks, 256, 0, ws.stream>>>(
      batch.d_problems, batch.d_states, n, run.Front(0), queue, run.leaf_list, run.d_counters,
      run.d_tail.sel, run.d_tail.best, num, run.d_tail.states, run.d_tail.summary,
      run.d_tail.words(), run.PublishTo(), run.h_tail.num_words(),
      batch.trace && batch.trace->enabled() ? 1 : 0,
      Debug().fast2d_queue_lost > 0 ? Debug().fast2d_queue_lost : 3);
  run.Mark("queue");
  CMX_HIP(hipGetLastError());
  RecordEvent(ws.ev_x1, ws.stream);
  result->expansion_launches = 1;
  RecordEvent(ws.ev_end, ws.stream);
  turn.reset();
  run.FetchResults(run.direct);
  const CountersSummary& h_counters = *run.h_tail.summary;
  result->expansion_lookups = 64ll * h_counters.wave_gathers;
  for (int p = 0; p < num; ++p)
    for (int k = 0; k < kStatShards; ++k)
      result->expansion_nodes += run.h_tail.states[p].expanded_shard[k];
  if (h_counters.leaf_overflow) return QueueOutcome::kLeafOverflow;
  if (h_counters.frontier_overflow) return QueueOutcome::kQueueOverflow;
  return QueueOutcome::kDone;
}

}  // namespace cmx
