// What every kernel of the fast 2D tree search shares, whichever unit defines it (fast_2d_seed.hip,
// fast_2d_levels.hip, fast_2d_queue.hip, fast_2d.hip): the counters of a call and their summary,
// node lists, nodes and their children, leaf records, and the best-leaf selection that ends a
// search (SelectBestBody: a kernel of its own on the level-synchronous path, the last workgroup of
// the tree launch on the work-queue path).
//
// Device code and plain structs only.  The types stay in the unnamed namespace the kernels live
// in: the kernels' symbols spell their parameter types, and bench.py and the profiling tools name
// kernels by these symbols.  Every unit that includes this header therefore has its own,
// identical copy of them.
#ifndef CMX_FAST_2D_SEARCH_DEVICE_H_
#define CMX_FAST_2D_SEARCH_DEVICE_H_

#include "fast_2d_device.h"
#include "fast_2d_internal.h"

namespace cmx {
namespace {

constexpr int kSeedsPerProblem = 64;

constexpr int kMaxStages = kMaxDepth + 2;   // one frontier counter array per search stage

// Sub-list counters sit one per 128-byte line: returning atomics on words of the same line
// queue behind each other in L2 (64 adjacent counters = 2 lines took every list reservation of
// a batch through two queues).
constexpr int kCountStride = 32;
// The work queue of TreeQueueKernel (fast_2d_queue.hip): kQueues sub-queues, control words one
// 128-byte line per sub-queue (a word takes ~90 atomics per microsecond, and atomics on one line
// queue behind each other).
constexpr int kQueues = 2048;
struct alignas(8) QueueCtl {
  int head;           // nodes taken (CAS)
  int reserved;       // slots reserved by producers (every one of them gets published)
  int pad[30];        // (a pop reads the pair with ONE 8-byte load: both only grow, so halves of
};                    // different ages are harmless -- the CAS on `head` decides)
struct Counters {           // device, zeroed per call
  int frontier[kMaxStages][kSubLists * kCountStride];
  int leaves[kSubLists * kCountStride];
  int frontier_overflow;
  int leaf_overflow;
  unsigned wave_gathers;      // 64-lane quad gathers issued by the wave-per-node expansion (statistics)
  int blocks_done;            // TreeQueueKernel: workgroups that have run out of work
  int pad[28];
  unsigned gathers_shard[16 * kCountStride];   // TreeQueueKernel's share of wave_gathers, by workgroup
  unsigned queue_stats[16 * kCountStride];     // [shard][8] trace counters of the queue (CountersSummary)
  QueueCtl queue[kQueues];
};

// What the host needs of the counters, written next to the results by the last kernel of a
// search (the padded Counters are 120 KB: not something to copy back per match).
struct CountersSummary {
  int leaves[kSubLists];
  int frontier_total[kMaxStages];
  int frontier_overflow;
  int leaf_overflow;
  unsigned wave_gathers;
  int pad;
  unsigned queue_stats[8];    // trace: pops, lost races, slot re-reads, pushed nodes, list nodes, chains, -, -
};

struct NodeList {
  Node2D* nodes;      // [kSubLists][sub_capacity]
  int* counts;        // [kSubLists] at stride kCountStride
  int sub_capacity;
};

// Reserves `m` consecutive slots of sub-list `sub`; returns the first slot.
__device__ __forceinline__ int ListReserve(const NodeList& list, int sub, int m) {
  return atomicAdd(&list.counts[sub * kCountStride], m);
}
__device__ __forceinline__ bool ListStore(const NodeList& list, int sub, int slot,
                                          const Node2D& nd) {
  if (slot >= list.sub_capacity) return false;
  list.nodes[static_cast<size_t>(sub) * list.sub_capacity + slot] = nd;
  return true;
}
// Largest sub-list length (wave-uniform); every lane must call it.
__device__ __forceinline__ int ListMaxCount(const NodeList& list) {
  const int lane = threadIdx.x & 63;
  return WaveMax(min(list.counts[lane * kCountStride], list.sub_capacity));
}

__device__ __forceinline__ int NodeProblem(const Node2D& nd) { return nd.problem & 0xffffff; }
__device__ __forceinline__ int NodeLevel(const Node2D& nd) { return nd.problem >> 24; }

__device__ __forceinline__ Node2D CoarseNode(const Fast2DProblem& P, int problem, int s,
                                             int local) {
  const int2 dims = P.coarse_dims[s];
  const int4 bd = P.bounds[s];
  const int step = 1 << (P.depth - 1);
  const int ix = local / dims.y, iy = local - ix * dims.y;
  const int c = s * P.coarse_stride + local;
  Node2D nd;
  nd.problem = problem | ((P.depth - 1) << 24);
  nd.scan = s;
  nd.dx = bd.x + ix * step;
  nd.dy = bd.z + iy * step;
  nd.score = P.coarse_score[c];
  nd.coarse_index = c;
  nd.path = 0;
  nd.coarse_score = nd.score;
  return nd;
}

// The scores of the <=4 children of a node (SM2/fast_...2d.cc:351-368).  child_score[k] < 0 marks
// a child outside the search bounds; rank[k] is the position of child k in the reference's stable
// descending sort of the children.  (`partial`: the per-wavefront sums of ScoreChildren,
// fast_2d_block_device.h.)
struct ChildScratch {
  int partial[4][4];
  float child_score[4];
  int rank[4];
  int nvalid;
};

__device__ __forceinline__ Node2D MakeChild(const Node2D& nd, int k, int child_level,
                                            const ChildScratch& sh) {
  Node2D child = nd;
  child.problem = NodeProblem(nd) | (child_level << 24);
  child.dx = nd.dx + (k >> 1) * (1 << child_level);
  child.dy = nd.dy + (k & 1) * (1 << child_level);
  child.score = sh.child_score[k];
  child.path = nd.path | (static_cast<unsigned>(sh.rank[k]) << (2 * child_level));
  return child;
}

__device__ __forceinline__ void RecordLeaf(const Node2D& leaf, const NodeList& leaves,
                                           Counters* __restrict__ counters) {
  const int sub = blockIdx.x & (kSubLists - 1);
  if (!ListStore(leaves, sub, ListReserve(leaves, sub, 1), leaf)) counters->leaf_overflow = 1;
}

// Best-leaf selection in the reference's depth-first visiting order among
// equal scores: higher-scoring lowest-resolution ancestor first (the sorted
// order of :331-332; equal ancestors fall back to generation order), then the
// sibling ranks down the tree.  One block; the leaf list is short.
struct SelectState {         // per problem, device
  unsigned best_coarse_bits;
  int ties;
  unsigned long long key;    // (coarse_index << 32) | path, minimised
};

// A word another workgroup of the SAME launch may have written (atomics, agent-scope stores):
// read past this CU's L1 (global_load ... sc1).
template <typename T>
__device__ __forceinline__ T LoadAgent(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// kSameLaunch: the leaves, counters and problem states were written by other workgroups of the
// launch this runs in (TreeQueueKernel's last workgroup), not by an earlier launch: every word of
// them is read with agent-scope loads (the producers stored / updated them with agent-scope
// stores and atomics and drained their stores before they arrived on `blocks_done`).
template <bool kSameLaunch>
__device__ __forceinline__ void
SelectBestBody(NodeList leaves, const ProblemState* __restrict__ states,
               SelectState* __restrict__ sel, BestLeaf* __restrict__ best, int num_problems,
               ProblemState* __restrict__ states_out, const Counters* __restrict__ counters,
               CountersSummary* __restrict__ summary) {
  if constexpr (kSameLaunch) {
    static_assert(sizeof(ProblemState) % sizeof(unsigned) == 0, "copied by words");
    constexpr int kWords = sizeof(ProblemState) / sizeof(unsigned);
    const unsigned* from = reinterpret_cast<const unsigned*>(states);
    unsigned* to = reinterpret_cast<unsigned*>(states_out);
    for (int i = threadIdx.x; i < num_problems * kWords; i += blockDim.x) to[i] = LoadAgent(&from[i]);
  } else {
    for (int p = threadIdx.x; p < num_problems; p += blockDim.x) states_out[p] = states[p];
  }
  const auto word = [](const auto* p) {
    if constexpr (kSameLaunch) return LoadAgent(p);
    else return *p;
  };
  if (threadIdx.x < kSubLists) summary->leaves[threadIdx.x] = word(&counters->leaves[threadIdx.x * kCountStride]);
  if (threadIdx.x >= 64 && threadIdx.x < 64 + kMaxStages) {
    const int st = threadIdx.x - 64;
    int total = 0;
    for (int k = 0; k < kSubLists; ++k) total += word(&counters->frontier[st][k * kCountStride]);
    summary->frontier_total[st] = total;
  }
  if (threadIdx.x == 128) {
    summary->frontier_overflow = word(&counters->frontier_overflow);
    summary->leaf_overflow = word(&counters->leaf_overflow);
    unsigned gathers = word(&counters->wave_gathers);
    for (int k = 0; k < 16; ++k) gathers += word(&counters->gathers_shard[k * kCountStride]);
    summary->wave_gathers = gathers;
  }
  if (threadIdx.x >= 192 && threadIdx.x < 200) {
    unsigned total = 0;
    for (int k = 0; k < 16; ++k) total += word(&counters->queue_stats[k * kCountStride + (threadIdx.x - 192)]);
    summary->queue_stats[threadIdx.x - 192] = total;
  }
  __syncthreads();      // (states_out is complete: the selection below reads it, not `states`)
  states = states_out;
  int max_count;
  {
    const int lane = threadIdx.x & 63;
    max_count = WaveMax(min(word(&leaves.counts[lane * kCountStride]), leaves.sub_capacity));
  }
  const int total = max_count * kSubLists;
  auto leaf_at = [&](int i, Node2D* nd) {
    const int sub = i & (kSubLists - 1), j = i / kSubLists;
    if (j >= min(word(&leaves.counts[sub * kCountStride]), leaves.sub_capacity)) return false;
    const Node2D* at = &leaves.nodes[static_cast<size_t>(sub) * leaves.sub_capacity + j];
    if constexpr (kSameLaunch) {
      const unsigned long long* w = reinterpret_cast<const unsigned long long*>(at);
      unsigned long long v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = LoadAgent(&w[k]);
      __builtin_memcpy(nd, v, sizeof(Node2D));
    } else {
      *nd = *at;
    }
    return true;
  };
  // Common case (a handful of leaves, a few problems): every thread keeps its leaf in
  // registers and the four selection rounds run on LDS atomics -- one trip to memory
  // instead of five passes of global atomics and fences.
  constexpr int kFastProblems = 64;
  if (total <= static_cast<int>(blockDim.x) && num_problems <= kFastProblems) {
    __shared__ unsigned s_best_bits[kFastProblems], s_coarse[kFastProblems];
    __shared__ unsigned long long s_key[kFastProblems];
    __shared__ int s_ties[kFastProblems], s_scan[kFastProblems], s_dx[kFastProblems],
        s_dy[kFastProblems];
    if (static_cast<int>(threadIdx.x) < num_problems) {
      const int p = threadIdx.x;
      s_best_bits[p] = states[p].best_bits;
      s_coarse[p] = 0;
      s_key[p] = ~0ull;
      s_ties[p] = 0;
      s_scan[p] = -1; s_dx[p] = 0; s_dy[p] = 0;
    }
    Node2D nd;
    const bool have = leaf_at(threadIdx.x, &nd);
    const int p = have ? NodeProblem(nd) : 0;
    __syncthreads();
    const bool tied = have && __float_as_uint(nd.score) == s_best_bits[p];
    if (tied) {
      atomicMax(&s_coarse[p], __float_as_uint(nd.coarse_score));
      atomicAdd(&s_ties[p], 1);
    }
    __syncthreads();
    const unsigned long long key =
        (static_cast<unsigned long long>(static_cast<unsigned>(nd.coarse_index)) << 32) | nd.path;
    const bool top = tied && __float_as_uint(nd.coarse_score) == s_coarse[p];
    if (top) atomicMin(&s_key[p], key);
    __syncthreads();
    if (top && key == s_key[p]) {     // duplicates (dive + search) carry identical content
      s_scan[p] = nd.scan; s_dx[p] = nd.dx; s_dy[p] = nd.dy;
      BestLeaf b;
      b.score = nd.score; b.scan = nd.scan; b.dx = nd.dx; b.dy = nd.dy;
      b.found = 1; b.ties = 1; b.pad0 = b.pad1 = 0;
      best[p] = b;
    }
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < num_problems) s_ties[threadIdx.x] = 0;
    __syncthreads();
    // ties = 1 + tied records that are a DIFFERENT leaf than the chosen one.
    if (tied && (nd.scan != s_scan[p] || nd.dx != s_dx[p] || nd.dy != s_dy[p]))
      atomicAdd(&s_ties[p], 1);
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < num_problems) {
      const int q = threadIdx.x;
      sel[q].best_coarse_bits = s_coarse[q];
      sel[q].key = s_key[q];
      sel[q].ties = s_ties[q];
      if (s_scan[q] < 0) {
        BestLeaf b{};
        best[q] = b;
      } else {
        best[q].ties = 1 + s_ties[q];
      }
    }
    return;
  }
  for (int p = threadIdx.x; p < num_problems; p += blockDim.x) {
    sel[p].best_coarse_bits = 0;
    sel[p].ties = 0;
    sel[p].key = ~0ull;
    BestLeaf b{};
    best[p] = b;
  }
  __threadfence();
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    Node2D nd;
    if (!leaf_at(i, &nd)) continue;
    const int p = NodeProblem(nd);
    if (__float_as_uint(nd.score) == states[p].best_bits) {
      atomicMax(&sel[p].best_coarse_bits, __float_as_uint(nd.coarse_score));
      atomicAdd(&sel[p].ties, 1);
    }
  }
  __threadfence();
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    Node2D nd;
    if (!leaf_at(i, &nd)) continue;
    const int p = NodeProblem(nd);
    if (__float_as_uint(nd.score) == states[p].best_bits &&
        __float_as_uint(nd.coarse_score) ==
            __hip_atomic_load(&sel[p].best_coarse_bits, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT)) {
      const unsigned long long key =
          (static_cast<unsigned long long>(static_cast<unsigned>(nd.coarse_index)) << 32) | nd.path;
      atomicMin(&sel[p].key, key);
    }
  }
  __threadfence();
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    Node2D nd;
    if (!leaf_at(i, &nd)) continue;
    const int p = NodeProblem(nd);
    const unsigned long long key =
        (static_cast<unsigned long long>(static_cast<unsigned>(nd.coarse_index)) << 32) | nd.path;
    if (__float_as_uint(nd.score) == states[p].best_bits &&
        __float_as_uint(nd.coarse_score) ==
            __hip_atomic_load(&sel[p].best_coarse_bits, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) &&
        key == __hip_atomic_load(&sel[p].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
      BestLeaf b;
      b.score = nd.score; b.scan = nd.scan; b.dx = nd.dx; b.dy = nd.dy;
      b.found = 1;
      b.ties = 1;
      b.pad0 = b.pad1 = 0;
      best[p] = b;   // duplicates (dive + search) carry identical content
    }
  }
  __threadfence();
  __syncthreads();
  // ties = 1 + number of tied records that are a DIFFERENT leaf (the dive and
  // the search record the best leaf twice; that is not a tie).
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    Node2D nd;
    if (!leaf_at(i, &nd)) continue;
    const int p = NodeProblem(nd);
    if (__float_as_uint(nd.score) != states[p].best_bits) continue;
    const int scan = __hip_atomic_load(&best[p].scan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int dx = __hip_atomic_load(&best[p].dx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int dy = __hip_atomic_load(&best[p].dy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nd.scan != scan || nd.dx != dx || nd.dy != dy) atomicAdd(&best[p].ties, 1);
  }
}

}  // namespace
}  // namespace cmx

#endif  // CMX_FAST_2D_SEARCH_DEVICE_H_
