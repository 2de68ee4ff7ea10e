// FastCorrelativeScanMatcher2D on gfx950: the batched branch and bound behind the front end.
//
// Reference behaviour being replaced:
//   SM2/fast_correlative_scan_matcher_2d.cc:227-378  MatchWithSearchParameters, BranchAndBound
// (SM2 = cartographer/mapping/internal/2d/scan_matching).
//
// Search schedule (any sound schedule returns the reference's best score), the lowest-resolution
// candidates having been scored (fast_2d_coarse.hip):
//   2. "dive": greedy descents from the best few of them give a real leaf
//      score b0, a valid lower bound;
//   3. every lowest-resolution node whose upper bound reaches the bound is
//      searched depth-first by one workgroup, all workgroups sharing the
//      problem's bound through one atomic word;
//   4. among the leaves with the best score, the one the reference's
//      depth-first search meets first is returned (see SelectBestKernel).
//
// Two strategies walk the tree: a work queue in ONE launch (TreeQueueKernel, RunQueueSearch) and a
// chain of level-synchronous launches (RunLevelSynchronous), which is also what a queue overflow
// falls back to.  RunBranchAndBound picks.
//
// The other units of the matcher: fast_2d_stack.hip (precomputation stack), fast_2d_coarse.hip
// (front end), fast_2d_match.hip (MatchBatch, tie resolution, C ABI); fast_2d_internal.h and
// fast_2d_device.h hold what they share.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <type_traits>
#include <utility>

#include "fast_2d_device.h"
#include "fast_2d_internal.h"

namespace cmx {
namespace {

constexpr int kSeedsPerProblem = 64;

// ---------------------------------------------------------------------------
// Branch and bound
// ---------------------------------------------------------------------------
constexpr int kMaxStages = kMaxDepth + 2;   // one frontier counter array per search stage

// Sub-list counters sit one per 128-byte line: returning atomics on words of the same line
// queue behind each other in L2 (64 adjacent counters = 2 lines took every list reservation of
// a batch through two queues).
constexpr int kCountStride = 32;
// The work queue of TreeQueueKernel (below): kQueues sub-queues, control words one 128-byte line
// per sub-queue (a word takes ~90 atomics per microsecond, and atomics on one line queue behind
// each other).
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

// Seeds of the dive: the best candidate of each of the ~64 best scans (histogram
// threshold on the per-scan maxima).  Every dive block repeats the selection for its own
// problem -- 18 KB of per-scan maxima, L2-resident after the first block -- and takes
// seed number `want` in scan order: no separate launch (a kernel that does this alone
// costs ~5 us plus its boundary), no cross-block hand-off.  When want == 0 the block also
// totals the problem's lowest-resolution candidates (the layout needs no prefix sum).
struct SeedScratch {
  int hist[1024];
  int wave_total[4];
  int threshold_bin;
  int found_scan[4];
  int total;
};

// Seeds want0 .. want0 + wants - 1 (wants <= 4) into sh->found_scan[], -1 where there is no such
// seed.  The numbering depends on the size of the workgroup: every dive kernel calls this with
// 256 threads, so that they all start from the same seeds.
__device__ __forceinline__ void PickSeeds(const Fast2DProblem& P, int n, int want0, int wants,
                                          SeedScratch* sh) {
  const int tid = threadIdx.x, lane = tid & 63, T = blockDim.x;
  for (int i = tid; i < 1024; i += T) sh->hist[i] = 0;
  if (tid < 4) sh->found_scan[tid] = -1;
  if (tid == 0) sh->total = 0;
  __syncthreads();
  const int S = P.num_scans;
  const long long range = 255ll * n + 1;
  const auto* scan_best = AsGlobal(P.scan_best);
  const auto* coarse_dims = AsGlobal(P.coarse_dims);
  // Thread t owns scans t, t + T, ...: coalesced, independent loads (a contiguous chunk per
  // thread was a chain of L2 round trips); the first kOwn maxima stay in registers for the
  // second pass.
  // Under group bounds the rotations of a unit share their sums: only the one whose cells were
  // summed (the middle one) stands for its unit, or the seeds would be a third as many units.
  const bool grouped = P.group > 1;
  const auto best_of = [&](int s) -> int {
    if (grouped) {
      const int first = s - s % kFusedGroup;
      if (s != first + (S - first >= kFusedGroup ? 1 : 0)) return -1;
    }
    return scan_best[s].x;
  };
  constexpr int kOwn = 16;
  int own[kOwn];
#pragma unroll
  for (int k = 0; k < kOwn; ++k) {
    const int s = tid + k * T;
    own[k] = s < S ? best_of(s) : -1;
  }
  int total = 0;
#pragma unroll
  for (int k = 0; k < kOwn; ++k)
    if (own[k] >= 0) atomicAdd(&sh->hist[static_cast<int>(own[k] * 1024ll / range)], 1);
  for (int s = tid + kOwn * T; s < S; s += T) {
    const int b = best_of(s);
    if (b >= 0) atomicAdd(&sh->hist[static_cast<int>(b * 1024ll / range)], 1);
  }
  if (want0 == 0) {
    for (int s = tid; s < S; s += T) total += coarse_dims[s].x * coarse_dims[s].y;
    total = WaveSum(total);
    if (lane == 0 && total) atomicAdd(&sh->total, total);
  }
  __syncthreads();
  if (tid < 64) {
    // Highest bin b >= 1 with (number of scans in bins >= b) >= kSeedsPerProblem, else 0.
    // Lane l owns bins 1023 - 16 l down to 1008 - 16 l.
    int mine = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) mine += sh->hist[1023 - 16 * lane - k];
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    const unsigned long long reached = __ballot(incl >= kSeedsPerProblem);
    int tb = 0;
    if (reached) {
      const int first = __ffsll(static_cast<long long>(reached)) - 1;
      if (lane == first) {
        int acc = incl - mine;
        for (int k = 0; k < 16; ++k) {
          const int b = 1023 - 16 * lane - k;
          acc += sh->hist[b];
          if (acc >= kSeedsPerProblem) { tb = b; break; }   // b == 0 only in lane 63: tb = 0
        }
        sh->threshold_bin = tb;
      }
    } else if (lane == 0) {
      sh->threshold_bin = 0;
    }
  }
  __syncthreads();
  const int tb = sh->threshold_bin;
  const auto qualifies = [&](int best) {
    return best >= 0 && static_cast<int>(best * 1024ll / range) >= tb &&
           ToScore(P, best, n) > P.min_score;
  };
  // Seeds are numbered thread-major: thread t's qualifying scans (in its own order) follow
  // those of threads < t.
  int count = 0;
#pragma unroll
  for (int k = 0; k < kOwn; ++k) count += qualifies(own[k]) ? 1 : 0;
  for (int s = tid + kOwn * T; s < S; s += T) count += qualifies(best_of(s)) ? 1 : 0;
  int incl = count;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) sh->wave_total[tid >> 6] = incl;
  __syncthreads();
  int before = incl - count;
  for (int w = 0; w < (tid >> 6); ++w) before += sh->wave_total[w];
  const int want_end = want0 + wants;
  if (want0 < before + count && want_end > before) {
    int k = before;
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      if (qualifies(own[j])) {
        if (k >= want0 && k < want_end) sh->found_scan[k - want0] = tid + j * T;
        ++k;
      }
    }
    for (int s = tid + kOwn * T; s < S && k < want_end; s += T) {
      if (!qualifies(best_of(s))) continue;
      if (k >= want0) sh->found_scan[k - want0] = s;
      ++k;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ bool PickSeed(const Fast2DProblem& P, int n, int want,
                                         SeedScratch* sh, int* scan_out) {
  PickSeeds(P, n, want, 1, sh);
  *scan_out = sh->found_scan[0];
  return sh->found_scan[0] >= 0;
}

// Problem- and scan-invariant data a block keeps on chip while it works on
// nodes of one rotated scan: level descriptors and score constants (so that a
// node expansion starts without dependent global loads), the discretised
// points (LDS when they fit) and the search bounds of the scan.
constexpr int kPointCache = 4096;   // points kept in LDS (16 KB)

struct BlockContext {
  LevelDesc level[kMaxDepth];
  uint32_t cache[kPointCache];
  const uint32_t* global_pts;
  float min_s, score_scale, min_score;
  int n, cached;
  int max_x, max_y;    // linear_bounds[scan].max_x / max_y
};

__device__ __forceinline__ void LoadContext(const Fast2DProblem& P, int n, int scan,
                                            BlockContext* ctx, bool stored = false) {
  const uint32_t* pts = P.discrete + static_cast<size_t>(scan) * n;
  const bool cached = n <= kPointCache;
  if (P.recompute_scans && !stored) {   // (implies n <= kFusedMaxPoints = kPointCache)
    const float2 rot = P.scan_rot[scan];
    for (int i = threadIdx.x; i < n; i += blockDim.x) ctx->cache[i] = ScanCell(P, rot, i);
  } else if (cached) {
    const auto* gp = AsGlobal(pts);
    for (int i = threadIdx.x; i < n; i += blockDim.x) ctx->cache[i] = gp[i];
  }
  if (threadIdx.x < kMaxDepth && static_cast<int>(threadIdx.x) < P.depth)
    ctx->level[threadIdx.x] = P.level[threadIdx.x];
  if (threadIdx.x == 64) {
    const int4 bd = P.bounds[scan];
    ctx->max_x = bd.y;
    ctx->max_y = bd.w;
    ctx->global_pts = pts;
    ctx->cached = cached;
    ctx->n = n;
    ctx->min_s = P.min_s;
    ctx->score_scale = P.score_scale;
    ctx->min_score = P.min_score;
  }
  __syncthreads();
}

__device__ __forceinline__ float ToScoreCtx(const BlockContext& ctx, int sum) {
  return ctx.min_s + (static_cast<float>(sum) / static_cast<float>(ctx.n)) * ctx.score_scale;
}

// Scores the <=4 children of a node (SM2/fast_...2d.cc:351-368) with the whole
// 256-thread block: every wave takes a quarter of the points and gathers all
// four children per point.  child_score[k] < 0 marks a child outside the
// search bounds; rank[k] is the position of child k in the reference's stable
// descending sort of the children.
struct ChildScratch {
  int partial[4][4];
  float child_score[4];
  int rank[4];
  int nvalid;
};

__device__ __forceinline__ void ScoreChildren(const BlockContext& ctx, int dx, int dy,
                                              int child_level, ChildScratch* sh) {
  const int n = ctx.n;
  const LevelDesc L = ctx.level[child_level];
  const int half = 1 << child_level;
  const int off = half - 1;
  const bool vx = dx + half <= ctx.max_x, vy = dy + half <= ctx.max_y;  // `break`s at :356,361
  const bool cached = ctx.cached;
  const auto* gpts = AsGlobal(ctx.global_pts);
  const auto* quads = AsGlobal(L.quads);
  // Children beyond the search bounds (`break`s at :356,361) are masked out of the quad.
  const uint32_t child_mask = (vx ? 0xffffffffu : 0x0000ffffu) & (vy ? 0xffffffffu : 0x00ff00ffu);
  // Packed accumulators: (s00 | s10 << 16) and (s01 | s11 << 16); a lane adds at most
  // 255 per point, so 256 points fit before the halves are widened.
  int s00 = 0, s01 = 0, s10 = 0, s11 = 0;   // s[x-step][y-step]
  // The gathers of the unrolled loop are meant to be in flight together.  Until the end of
  // round 3 they were not: `cached ? ctx.cache[i] : gpts[i]` inside the body gave every unrolled
  // iteration a branch and a basic block of its own, closed with s_waitcnt vmcnt(0) lgkmcnt(0) --
  // which also waited for the previous iteration's gather -- and the plain
  // `quads[inside ? offset : 0]` became a load under an exec mask.  Now: one loop per source of
  // the cells (compile-time), quads by buffer loads (out-of-range offsets read 0; a level of more
  // than 2 GB of quads keeps plain loads).
  // (the level comes out of LDS: the compiler does not take it for wavefront-uniform and would
  // wrap every buffer load in a waterfall loop -- readfirstlane says it is)
  const unsigned long long quads_address = reinterpret_cast<unsigned long long>(L.quads);
  // (readfirstlane returns an int: through `unsigned`, or a low word with its top bit set
  // sign-extends over the high word -- the first version of this faulted on exactly that)
  const unsigned long long quads_uniform =
      static_cast<unsigned long long>(static_cast<unsigned>(
          __builtin_amdgcn_readfirstlane(static_cast<unsigned>(quads_address)))) |
      (static_cast<unsigned long long>(static_cast<unsigned>(
           __builtin_amdgcn_readfirstlane(static_cast<unsigned>(quads_address >> 32)))) << 32);
  const unsigned long long quad_bytes =
      static_cast<unsigned long long>((__builtin_amdgcn_readfirstlane(L.qy) + 3) >> 2) *
      static_cast<unsigned>(__builtin_amdgcn_readfirstlane(L.qtx)) * 128ull;
  const bool quads_by_buffer = quad_bytes < (1ull << 31);
  const __amdgpu_buffer_rsrc_t quad_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<uint32_t*>(quads_uniform), 0,
      quads_by_buffer ? static_cast<int>(quad_bytes) : 0, 0x00020000);
  const auto walk = [&](auto cached_tag, auto buffer_tag) {
    constexpr bool kCached = decltype(cached_tag)::value;
    constexpr bool kBuffer = decltype(buffer_tag)::value;
    for (int base = threadIdx.x; base < n; base += 256 * 256) {
      uint32_t even = 0, odd = 0;
      const int stop = min(n, base + 256 * 256);
#pragma unroll 4
      for (int i = base; i < stop; i += 256) {
        uint32_t p;
        if constexpr (kCached) p = ctx.cache[i];
        else p = gpts[i];
        const int X = static_cast<short>(p & 0xffffu) + dx + off + half;
        const int Y = static_cast<short>(p >> 16) + dy + off + half;
        const bool inside = static_cast<unsigned>(X) < static_cast<unsigned>(L.qx) &&
                            static_cast<unsigned>(Y) < static_cast<unsigned>(L.qy);
        uint32_t v;
        if constexpr (kBuffer) {
          v = __builtin_amdgcn_raw_buffer_load_b32(
                  quad_rsrc, inside ? QuadOffset(X, Y, L.qtx) * 4u : 0xfffffff0u, 0, 0) &
              child_mask;
        } else {
          const uint32_t q = quads[inside ? QuadOffset(X, Y, L.qtx) : 0u];
          v = inside ? (q & child_mask) : 0u;
        }
        even += v & 0x00ff00ffu;          // byte 0 (x0,y0) and byte 2 (x1,y0)
        odd += (v >> 8) & 0x00ff00ffu;    // byte 1 (x0,y1) and byte 3 (x1,y1)
      }
      s00 += even & 0xffffu; s10 += even >> 16;
      s01 += odd & 0xffffu;  s11 += odd >> 16;
    }
  };
  if (quads_by_buffer) {
    if (cached) walk(std::true_type{}, std::true_type{});
    else walk(std::false_type{}, std::true_type{});
  } else {
    if (cached) walk(std::true_type{}, std::false_type{});
    else walk(std::false_type{}, std::false_type{});
  }
  s00 = WaveSum(s00); s01 = WaveSum(s01); s10 = WaveSum(s10); s11 = WaveSum(s11);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh->partial[wave][0] = s00; sh->partial[wave][1] = s01;
    sh->partial[wave][2] = s10; sh->partial[wave][3] = s11;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    // Lanes 0..3 finish child k = 2*x-step + y-step (generation order: x outer,
    // y inner) and rank them through wave shuffles.
    const int k = threadIdx.x & 3;
    const bool valid = ((k >> 1) == 0 || vx) && ((k & 1) == 0 || vy);
    const int total = sh->partial[0][k] + sh->partial[1][k] + sh->partial[2][k] + sh->partial[3][k];
    const float mine = valid ? ToScoreCtx(ctx, total) : -1.f;
    int rank = 0, nvalid = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float other = __shfl(mine, j, 64);
      if (other >= 0.f) ++nvalid;
      if (j != k && other >= 0.f && (other > mine || (other == mine && j < k))) ++rank;
    }
    if (threadIdx.x < 4) {
      sh->child_score[k] = mine;
      sh->rank[k] = rank;
      if (k == 0) sh->nvalid = nvalid;
    }
  }
  __syncthreads();
}

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

// One greedy descent per seed: always continue with the best child.  The leaf
// reached is a real candidate, so its score is a valid bound.
__global__ void __launch_bounds__(256, 4)
DiveKernel(const Fast2DProblem* __restrict__ problems, ProblemState* __restrict__ states, int n,
           NodeList leaves, Counters* __restrict__ counters) {
  const int problem = blockIdx.y;
  const Fast2DProblem& P = problems[problem];
  ProblemState& st = states[problem];
  if (st.error) return;
  __shared__ BlockContext ctx;
  __shared__ ChildScratch sh;
  __shared__ Node2D cur;
  __shared__ SeedScratch seed_scratch;
  // Under group bounds a seed is a unit of three rotations (PickSeed) whose bound says nothing
  // about which of them holds the good leaf: a dive per rotation (blocks 3 k, 3 k + 1, 3 k + 2).
  const int per_seed = P.group > 1 ? kFusedGroup : 1;
  if (static_cast<int>(blockIdx.x) >= kSeedsPerProblem * per_seed) return;
  int seed_scan;
  const bool have_seed = PickSeed(P, n, blockIdx.x / per_seed, &seed_scratch, &seed_scan);
  if (blockIdx.x == 0 && threadIdx.x == 0) st.coarse_total = seed_scratch.total;
  if (!have_seed) return;
  if (per_seed > 1) {
    seed_scan = seed_scan - seed_scan % kFusedGroup + static_cast<int>(blockIdx.x) % per_seed;
    if (seed_scan >= P.num_scans) return;
  }
  const Node2D seed = CoarseNode(P, problem, seed_scan, P.scan_best[seed_scan].y);
  if (threadIdx.x == 0) cur = seed;
  LoadContext(P, n, seed.scan, &ctx);
  const int depth = NodeLevel(seed) + 1;
  unsigned long long scored = 0;
  for (int child_level = depth - 2; child_level >= 0; --child_level) {
    const Node2D nd = cur;
    ScoreChildren(ctx, nd.dx, nd.dy, child_level, &sh);
    scored += sh.nvalid;
    if (threadIdx.x == 0) {
      for (int k = 0; k < 4; ++k)
        if (sh.child_score[k] >= 0.f && sh.rank[k] == 0) cur = MakeChild(nd, k, child_level, sh);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const Node2D leaf = cur;
    if (leaf.score > ctx.min_score) {
      RecordLeaf(leaf, leaves, counters);
      atomicMax(&st.best_bits, __float_as_uint(leaf.score));
    }
    atomicAdd(&st.scored_shard[blockIdx.x & (kStatShards - 1)], scored);
    atomicAdd(&st.expanded_shard[blockIdx.x & (kStatShards - 1)],
              static_cast<unsigned long long>(depth - 1));
  }
}

// Lowest-resolution nodes that can still matter (reference: :346-350): one
// block per scan; whole scans are skipped through their best candidate.
// strict = 0 keeps nodes equal to the bound so that every leaf tied for the
// best score is found.
__global__ void __launch_bounds__(256)
FilterCoarseKernel(const Fast2DProblem* __restrict__ problems,
                   const ProblemState* __restrict__ states, int n, int chunk, int num_chunks,
                   int strict, int affinity, NodeList out, Counters* __restrict__ counters) {
  // One WAVEFRONT per rotated scan (grid: ceil(scans / 4) x problems): a scan's filter is a
  // chain of dependent loads (problem, best candidate, dimensions, scores, list slot) over
  // ~190 candidates; a block per scan kept 8 of those chains in flight per CU, and 36 k blocks
  // of a 16-submap batch took 320 us to dispatch and drain.
  const int problem = blockIdx.y;
  const Fast2DProblem& P = problems[problem];
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (s >= P.num_scans || states[problem].error) return;
  if (s % num_chunks != chunk) return;
  const float best = __uint_as_float(states[problem].best_bits);
  const float top = ToScore(P, P.scan_best[s].x, n);
  if (strict ? !(top > best) : (top < best)) return;
  const int2 dims = P.coarse_dims[s];
  const int count = dims.x * dims.y;
  const int base = s * P.coarse_stride;
  // The first 256 scores are fetched together (the passes below would otherwise be a chain of
  // load -> ballot -> list reservation round trips).
  const auto* scores = AsGlobal(P.coarse_score) + base;
  float ahead[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) ahead[k] = k * kWave + lane < count ? scores[k * kWave + lane] : 0.f;
  for (int c0 = 0; c0 < count; c0 += kWave) {
    // One reservation per wave; consecutive waves use consecutive sub-lists, so that one
    // rotation's survivors do not all queue in the same one.
    // With `affinity` a problem's nodes only go to the sub-lists the workgroups of ONE XCD
    // read (sub % 8 == problem % 8, see ExpandWaveKernel): the level data of that problem
    // then lives in one L2 instead of eight.
    const int sub = affinity ? (problem & 7) + 8 * ((s + (c0 >> 6)) & 7)
                             : (s + blockIdx.y + (c0 >> 6)) & (kSubLists - 1);
    const int c = c0 + lane;
    bool keep = false;
    if (c < count) {
      float score;
      switch (c0 >> 6) {
        case 0: score = ahead[0]; break;
        case 1: score = ahead[1]; break;
        case 2: score = ahead[2]; break;
        case 3: score = ahead[3]; break;
        default: score = scores[c];
      }
      keep = strict ? (score > best) : (score >= best);
    }
    // One reservation per wave: slots go to the kept lanes in lane order.
    const unsigned long long mask = __ballot(keep);
    if (mask == 0) continue;
    int first = 0;
    if (lane == 0) first = ListReserve(out, sub, __popcll(mask));
    first = __builtin_amdgcn_readfirstlane(first);
    if (keep) {
      const int slot = first + __popcll(mask & ((1ull << lane) - 1));
      if (!ListStore(out, sub, slot, CoarseNode(P, problem, s, c))) counters->frontier_overflow = 1;
    }
  }
}

// Level-synchronous expansion near the top of the tree, one WAVE per node
// (four independent nodes per block, no LDS, no barriers).  The top levels
// hold thousands of nodes most of which die after one expansion, so what
// matters there is how many nodes are in flight, not the latency of one.
// Children that can still matter go to `out`; child_level is always >= 1 here.
constexpr int kWaveStatProblems = 1024;   // problems whose work counters a block keeps in LDS

__global__ void __launch_bounds__(256)
ExpandWaveKernel(const Fast2DProblem* __restrict__ problems, ProblemState* __restrict__ states,
                 int n, NodeList in, int strict, int affinity, NodeList out,
                 Counters* __restrict__ counters) {
  // Work counters (candidates scored / nodes expanded per problem) are collected in LDS and
  // flushed once per block: one global atomic pair PER NODE -- half a million nodes of 16
  // problems hammering 32 cache lines -- was 64 % of this kernel on a 16-submap batch
  // (3.36 -> 1.21 ms, profiles/r02_c3_wave_atomics.txt).
  __shared__ unsigned stat_scored[kWaveStatProblems], stat_expanded[kWaveStatProblems];
  __shared__ unsigned stat_gathers;
  if (threadIdx.x == 0) stat_gathers = 0;
  for (int i = threadIdx.x; i < kWaveStatProblems; i += blockDim.x) {
    stat_scored[i] = 0;
    stat_expanded[i] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int max_count = ListMaxCount(in);
  // Workgroups go to the XCDs round-robin (blockIdx.x % 8).  With `affinity` the waves of XCD
  // x read and write only the sub-lists with sub % 8 == x (grid: a multiple of 16 blocks), so
  // that a node's children are expanded on the XCD whose L2 already holds that problem.
  int first = blockIdx.x * 4 + wave;
  if (affinity) {
    const int slot = (blockIdx.x >> 3) * 4 + wave;            // wave index within the XCD
    first = (slot >> 3) * kSubLists + (blockIdx.x & 7) + 8 * (slot & 7);
  }
  const int out_sub = first & (kSubLists - 1);
  for (int i = first; i < max_count * kSubLists; i += gridDim.x * 4) {
    const int in_sub = i & (kSubLists - 1), j = i / kSubLists;
    if (j >= in.counts[in_sub * kCountStride]) continue;   // wave-uniform
    const Node2D nd = in.nodes[static_cast<size_t>(in_sub) * in.sub_capacity + j];
    const int problem = NodeProblem(nd);
    const Fast2DProblem& P = problems[problem];
    ProblemState& st = states[problem];
    const float best = __uint_as_float(st.best_bits);
    if (strict ? !(nd.score > best) : (nd.score < best)) continue;
    const int child_level = NodeLevel(nd) - 1;
    const LevelDesc L = P.level[child_level];
    const int4 bd = P.bounds[nd.scan];
    const int half = 1 << child_level, off = half - 1;
    const bool vx = nd.dx + half <= bd.y, vy = nd.dy + half <= bd.w;
    const auto* pts = AsGlobal(P.discrete) + static_cast<size_t>(nd.scan) * n;
    const bool recompute = P.recompute_scans != 0 && P.store_scans == 0;
    const float2 rot = recompute ? P.scan_rot[nd.scan] : make_float2(1.f, 0.f);
    // Early exit.  A level-(l+1) cell is the maximum of the four level-l cells its
    // children read (the 2h window is tiled by four h windows), so for every point
    // max(children) <= parent value and
    //   child_k total <= partial_k + (parent total - sum of max(children) so far).
    // Most frontier nodes pass their own bound only marginally: after a few dozen
    // points no child can reach the bound any more and the rest of the gathers
    // (the expensive part: 64 distinct cache lines each) is skipped.  The outcome
    // is the same as scoring all points: no child would have been kept.
    const int parent_ub = SumUpperBound(P, nd.score, n);
    // (the tiled quad array: ceil(qy / 4) rows of qtx tiles of 32 dwords; a buffer resource
    // addresses up to 2 GB of it -- a level of more than 23 000 x 23 000 cells keeps plain loads)
    const unsigned long long quad_bytes =
        static_cast<unsigned long long>((L.qy + 3) >> 2) * static_cast<unsigned>(L.qtx) * 128ull;
    const bool quads_by_buffer = quad_bytes < (1ull << 31);
    const __amdgpu_buffer_rsrc_t quad_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint32_t*>(L.quads), 0, quads_by_buffer ? static_cast<int>(quad_bytes) : 0,
        0x00020000);
    const auto* quads = AsGlobal(L.quads);
    const uint32_t child_mask =
        (vx ? 0xffffffffu : 0x0000ffffu) & (vy ? 0xffffffffu : 0x00ff00ffu);
    int s00 = 0, s01 = 0, s10 = 0, s11 = 0, seen_max = 0;
    int groups = 0;
    bool dead = false;
    // 64-point iterations gathered between two bound checks (1, 2 and 4 measure the same on a
    // 16-submap batch; 16, i.e. everything in flight at once, was no faster for single
    // searches: 37 vs 33 us).
    constexpr int kIters = 4;
    constexpr int kGroup = kIters * kWave;
    // (The loop is instantiated twice, for stored and for re-derived scan cells.  With the choice
    // made per point -- `recompute ? ScanCell(...) : pts[...]` inside the unrolled body, as it
    // stood until the end of round 3 -- every one of the four "gathers in flight" began with a
    // branch and a basic block of its own, and the compiler closed each with s_waitcnt vmcnt(0):
    // ONE gather in flight per wavefront, sixteen dependent round trips per node.)
    const auto walk = [&](auto recompute_tag, auto buffer_tag) {
      constexpr bool kRecompute = decltype(recompute_tag)::value;
      constexpr bool kBuffer = decltype(buffer_tag)::value;
      for (int q0 = 0; q0 < n; q0 += kGroup) {
        uint32_t cell[kIters];
#pragma unroll
        for (int u = 0; u < kIters; ++u) {      // the four cells first: independent loads
          const int q = q0 + u * kWave + lane;
          const int at = q < n ? q : 0;
          if constexpr (kRecompute) cell[u] = ScanCell(P, rot, at);
          else cell[u] = pts[at];
        }
        uint32_t v[kIters];
#pragma unroll
        for (int u = 0; u < kIters; ++u) {
          const int q = q0 + u * kWave + lane;
          const bool live = q < n;
          const uint32_t p = cell[u];
          const int X = static_cast<short>(p & 0xffffu) + nd.dx + off + half;
          const int Y = static_cast<short>(p >> 16) + nd.dy + off + half;
          const bool inside = live && static_cast<unsigned>(X) < static_cast<unsigned>(L.qx) &&
                              static_cast<unsigned>(Y) < static_cast<unsigned>(L.qy);
          // one gather, four children.  A buffer load: the compiler turned the plain
          // `quads[inside ? offset : 0]` into a load under an exec mask with its own s_waitcnt --
          // the four gathers went out one after the other.  Out-of-range offsets read 0.
          if constexpr (kBuffer) {
            const uint32_t quad = __builtin_amdgcn_raw_buffer_load_b32(
                quad_rsrc, inside ? QuadOffset(X, Y, L.qtx) * 4u : 0xfffffff0u, 0, 0);
            v[u] = quad & child_mask;
          } else {
            const uint32_t quad = quads[inside ? QuadOffset(X, Y, L.qtx) : 0u];
            v[u] = inside ? (quad & child_mask) : 0u;
          }
        }
#pragma unroll
        for (int u = 0; u < kIters; ++u) {
          const int a00 = v[u] & 0xff, a01 = (v[u] >> 8) & 0xff;
          const int a10 = (v[u] >> 16) & 0xff, a11 = v[u] >> 24;
          s00 += a00; s01 += a01; s10 += a10; s11 += a11;
          seen_max += max(max(a00, a01), max(a10, a11));
        }
        ++groups;
        if (q0 + kGroup < n) {
          // max_k sum_lanes(s_k) <= sum_lanes(max_k s_k): ONE wavefront reduction (of what the
          // best child of each lane's points still lacks to the parent) instead of five -- a
          // slightly looser bound, the same results (the check only skips work that cannot
          // matter), 8 of 54 vector instructions per gather less.
          const int lacking = seen_max - max(max(s00, s01), max(s10, s11));
          // kept children satisfy score >= best (> best in strict mode)
          if (ToScore(P, parent_ub - WaveSum(lacking), n) < best) { dead = true; break; }
        }
      }
    };
    if (quads_by_buffer) {
      if (recompute) walk(std::true_type{}, std::true_type{});
      else walk(std::false_type{}, std::true_type{});
    } else {
      if (recompute) walk(std::true_type{}, std::false_type{});
      else walk(std::false_type{}, std::false_type{});
    }
    const auto count_node = [&](int nvalid) {     // lane 0
      atomicAdd(&stat_gathers, static_cast<unsigned>(min(groups * kIters, (n + kWave - 1) / kWave)));
      if (problem < kWaveStatProblems) {
        atomicAdd(&stat_scored[problem], static_cast<unsigned>(nvalid));
        atomicAdd(&stat_expanded[problem], 1u);
      } else {
        atomicAdd(&st.scored_shard[out_sub & (kStatShards - 1)],
                  static_cast<unsigned long long>(nvalid));
        atomicAdd(&st.expanded_shard[out_sub & (kStatShards - 1)], 1ull);
      }
    };
    if (dead) {   // every child provably below the bound: counted, not kept
      if (lane == 0) count_node((1 + (vx ? 1 : 0)) * (1 + (vy ? 1 : 0)));
      continue;
    }
    const int total[4] = {WaveSum(s00), WaveSum(s01), WaveSum(s10), WaveSum(s11)};
    ChildScratch cs;   // wave-uniform, in registers
    int nvalid = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool valid = ((k >> 1) == 0 || vx) && ((k & 1) == 0 || vy);
      cs.child_score[k] = valid ? ToScore(P, total[k], n) : -1.f;
      nvalid += valid;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int rank = 0;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        if (o != k && cs.child_score[o] >= 0.f &&
            (cs.child_score[o] > cs.child_score[k] ||
             (cs.child_score[o] == cs.child_score[k] && o < k)))
          ++rank;
      }
      cs.rank[k] = rank;
    }
    if (lane == 0) {
      count_node(nvalid);
      int keep_mask = 0, m = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float sc = cs.child_score[k];
        if (sc < 0.f) continue;
        if (strict ? !(sc > best) : (sc < best)) continue;
        keep_mask |= 1 << k;
        ++m;
      }
      if (m) {
        int slot = ListReserve(out, out_sub, m);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(keep_mask >> k & 1)) continue;
          if (!ListStore(out, out_sub, slot, MakeChild(nd, k, child_level, cs)))
            counters->frontier_overflow = 1;
          ++slot;
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && stat_gathers) atomicAdd(&counters->wave_gathers, stat_gathers);
  for (int i = threadIdx.x; i < kWaveStatProblems; i += blockDim.x) {
    if (stat_expanded[i] == 0) continue;
    ProblemState& st = states[i];
    atomicAdd(&st.scored_shard[blockIdx.x & (kStatShards - 1)],
              static_cast<unsigned long long>(stat_scored[i]));
    atomicAdd(&st.expanded_shard[blockIdx.x & (kStatShards - 1)],
              static_cast<unsigned long long>(stat_expanded[i]));
  }
}

// Depth-first search of the subtree below each frontier node by one block,
// pruned with the problem's shared bound (reference: :335-378).  Nodes
// reaching `stop_level` (> 0) are handed to `out` instead of being searched
// (used once near the top to create enough independent roots); stop_level = 0
// searches down to the leaves, where only the first-best child can be
// returned by the reference (:340-343 after the stable sort of :331-332).
// strict = 0 keeps nodes / leaves EQUAL to the bound, so every leaf tied for
// the best score is recorded and the reference's visiting order can be
// reproduced.  The bound is re-read from global memory once per root and every
// 8 expansions; in between the block uses its own copy, raised by its own
// leaves (a stale bound only costs extra work).
__global__ void __launch_bounds__(256, 4)
SubtreeKernel(const Fast2DProblem* __restrict__ problems, ProblemState* __restrict__ states, int n,
              NodeList in, int stop_level, int strict, NodeList out, NodeList leaves,
              Counters* __restrict__ counters) {
  __shared__ BlockContext ctx;
  __shared__ ChildScratch cs;
  __shared__ Node2D stack[kMaxDepth * 3 + 4];
  __shared__ Node2D cur;
  __shared__ int sp, have;
  __shared__ float s_best;
  const int max_count = ListMaxCount(in);
  const int out_sub = blockIdx.x & (kSubLists - 1);
  for (int i = blockIdx.x; i < max_count * kSubLists; i += gridDim.x) {
    const int in_sub = i & (kSubLists - 1), j = i / kSubLists;
    if (j >= in.counts[in_sub * kCountStride]) continue;   // block-uniform
    const Node2D root = in.nodes[static_cast<size_t>(in_sub) * in.sub_capacity + j];
    const int problem = NodeProblem(root);
    const Fast2DProblem& P = problems[problem];
    ProblemState& st = states[problem];
    if (threadIdx.x == 0) {
      stack[0] = root;
      sp = 1;
      s_best = __uint_as_float(__hip_atomic_load(&st.best_bits, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT));
    }
    LoadContext(P, n, root.scan, &ctx, P.store_scans != 0);   // ends with __syncthreads()
    unsigned long long scored = 0, expanded = 0;
    for (;;) {
      if (threadIdx.x == 0) {
        have = sp > 0;
        if (have) cur = stack[--sp];
        if (have && (expanded & 7) == 7)
          s_best = fmaxf(s_best, __uint_as_float(__hip_atomic_load(
                                     &st.best_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
      }
      __syncthreads();
      if (!have) break;
      const Node2D nd = cur;
      const float best = s_best;
      const bool skip = strict ? !(nd.score > best) : (nd.score < best);
      if (!skip) {
        const int child_level = NodeLevel(nd) - 1;
        ScoreChildren(ctx, nd.dx, nd.dy, child_level, &cs);
        scored += cs.nvalid;
        ++expanded;
        if (threadIdx.x == 0) {
          if (child_level == 0) {
            for (int k = 0; k < 4; ++k) {
              if (cs.child_score[k] >= 0.f && cs.rank[k] == 0) {
                const Node2D leaf = MakeChild(nd, k, 0, cs);
                const bool keep = strict ? (leaf.score > best) : (leaf.score >= best);
                if (leaf.score > ctx.min_score && keep) {
                  RecordLeaf(leaf, leaves, counters);
                  atomicMax(&st.best_bits, __float_as_uint(leaf.score));
                  s_best = fmaxf(s_best, leaf.score);
                }
              }
            }
          } else if (child_level == stop_level) {
            // Hand the surviving children to the next stage: one slot
            // reservation per expansion.
            int keep_mask = 0, m = 0;
            for (int k = 0; k < 4; ++k) {
              const float sc = cs.child_score[k];
              if (sc < 0.f) continue;
              if (strict ? !(sc > best) : (sc < best)) continue;
              keep_mask |= 1 << k;
              ++m;
            }
            if (m) {
              int slot = ListReserve(out, out_sub, m);
              for (int k = 0; k < 4; ++k) {
                if (!(keep_mask >> k & 1)) continue;
                if (!ListStore(out, out_sub, slot, MakeChild(nd, k, child_level, cs)))
                  counters->frontier_overflow = 1;
                ++slot;
              }
            }
          } else {
            // Push worst first so the best child is searched next.
            for (int r = 3; r >= 0; --r) {
              for (int k = 0; k < 4; ++k) {
                if (cs.child_score[k] < 0.f || cs.rank[k] != r) continue;
                const float sc = cs.child_score[k];
                if (strict ? !(sc > best) : (sc < best)) continue;
                stack[sp++] = MakeChild(nd, k, child_level, cs);
              }
            }
          }
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0 && expanded) {
      atomicAdd(&st.scored_shard[blockIdx.x & (kStatShards - 1)], scored);
      atomicAdd(&st.expanded_shard[blockIdx.x & (kStatShards - 1)], expanded);
    }
    __syncthreads();
  }
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

// The one block that selects also PUBLISHES: everything the host reads after a search (the
// counters' summary, selection states, best leaves, problem states: `tail_words` dwords behind
// the counters) goes from device memory straight into the caller's pinned buffer (mapped into
// the device's address space) -- no copy kernel behind this one in a chain of launches that is
// latency from end to end.  tail_host == nullptr: the host fetches the tail itself.
__global__ void __launch_bounds__(1024)
SelectBestKernel(NodeList leaves, const ProblemState* __restrict__ states,
                 SelectState* __restrict__ sel, BestLeaf* __restrict__ best, int num_problems,
                 ProblemState* __restrict__ states_out, const Counters* __restrict__ counters,
                 CountersSummary* __restrict__ summary, const unsigned* __restrict__ tail_dev,
                 unsigned* __restrict__ tail_host, int tail_words) {
  SelectBestBody<false>(leaves, states, sel, best, num_problems, states_out, counters, summary);
  if (tail_host == nullptr) return;
  __threadfence();
  __syncthreads();
  for (int i = threadIdx.x; i < tail_words; i += blockDim.x)
    tail_host[i] = __hip_atomic_load(&tail_dev[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// Branch and bound through a work queue (round 6): ONE launch behind the dive and the
// lowest-resolution filter instead of the wave / subtree / select chain of launches.
//
// A worker is a WAVEFRONT.  It takes a node from the queue and walks a CHAIN from it: expand
// (one quad gather per point, the node's scan held in registers: 16 cells per lane), continue
// with the best child, hand the other children that can still matter to the queue; a chain ends
// at a leaf (which raises the problem's bound) or when no child reaches the bound.  Every chain is
// a greedy dive, so the bound tightens as fast as the reference's depth-first search tightens it
// (SM2/fast_...2d.cc:335-378), while thousands of chains run at once.  The level-synchronous
// kernels this replaces expanded a whole level against the bound the dive had left: 93 000 node
// expansions on a hard scan where the reference's own order needs 40 000.
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
// the host repeats the search on the strict, chunked path below.
// ---------------------------------------------------------------------------
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

constexpr int kChainCells = 16;     // cells per lane held in registers: clouds of up to 1024 points
constexpr uint32_t kNoCell = 0x80008000u;   // (x, y) = (-32768, -32768): outside every level

// ---- what a wavefront that walks a chain of nodes of ONE scan does per scan and per expansion
// (TreeQueueKernel's chains and DiveWaveKernel's dives) ------------------------------------------
// The scan's cells, point j * 64 + lane in cell[j]: stored (`discrete`) or re-derived (ScanCell).
template <bool kRecompute>
__device__ __forceinline__ void LoadChainCells(const Fast2DProblem& P, int n, int scan,
                                               uint32_t (&cell)[kChainCells]) {
  const int lane = threadIdx.x & 63;
  const auto* pts = AsGlobal(P.discrete) + static_cast<size_t>(scan) * n;
  if constexpr (kRecompute) {
    // ScanCell is some hundred instructions with its exact fall-back: ONE copy of it in a loop
    // that is not unrolled, its result put into its register by selects on the (uniform) index.
    const float2 rot = P.scan_rot[scan];
#pragma unroll
    for (int u = 0; u < kChainCells; ++u) cell[u] = kNoCell;
#pragma unroll 1
    for (int j = 0; j * kWave < n; ++j) {
      const int i = j * kWave + lane;
      const uint32_t c = i < n ? ScanCell(P, rot, i) : kNoCell;
#pragma unroll
      for (int u = 0; u < kChainCells; ++u) cell[u] = u == j ? c : cell[u];
    }
  } else {
#pragma unroll
    for (int j = 0; j < kChainCells; ++j) {
      const int i = j * kWave + lane;
      cell[j] = kNoCell;
      if (j * kWave < n) cell[j] = i < n ? pts[i] : kNoCell;
    }
  }
}

// The level the children of a node at (dx, dy) are scored on.  Everything about a node is
// wavefront-uniform, and the compiler is TOLD so: a buffer resource it cannot prove uniform gets
// every one of the sixteen gathers wrapped in a readfirstlane loop of thirty instructions.
struct ChainLevel {
  int qx, qy, qtx;
  int half;                    // 1 << child_level
  int ax, ay;                  // what a cell's coordinates are moved by: d + 2 half - 1
  __amdgpu_buffer_rsrc_t quad_rsrc;
};

__device__ __forceinline__ ChainLevel MakeChainLevel(const Fast2DProblem& P, int child_level,
                                                     int dx, int dy) {
  const LevelDesc& Lm = P.level[child_level];
  ChainLevel L;
  L.half = 1 << child_level;
  L.ax = dx + 2 * L.half - 1;
  L.ay = dy + 2 * L.half - 1;
  L.qx = __builtin_amdgcn_readfirstlane(Lm.qx);
  L.qy = __builtin_amdgcn_readfirstlane(Lm.qy);
  L.qtx = __builtin_amdgcn_readfirstlane(Lm.qtx);
  const unsigned long long quads_address = reinterpret_cast<unsigned long long>(Lm.quads);
  const unsigned long long quads_uniform =
      static_cast<unsigned long long>(static_cast<unsigned>(
          __builtin_amdgcn_readfirstlane(static_cast<unsigned>(quads_address)))) |
      (static_cast<unsigned long long>(static_cast<unsigned>(
           __builtin_amdgcn_readfirstlane(static_cast<unsigned>(quads_address >> 32)))) << 32);
  const unsigned long long quad_bytes =
      static_cast<unsigned long long>((L.qy + 3) >> 2) * static_cast<unsigned>(L.qtx) * 128ull;
  // (levels beyond the 2 GB a buffer resource addresses do not come here: see ChainWalkPossible)
  L.quad_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<uint32_t*>(quads_uniform), 0, static_cast<int>(quad_bytes), 0x00020000);
  return L;
}

// Quad gathers of cells [kFirst, kFirst + kCount) of the lane, all in flight at once, added to
// packed 16-bit sums: even = (child 00 | child 10 << 16), odd = (child 01 | child 11 << 16); a
// lane adds at most 16 x 255.  Children beyond the search bounds (`break`s at :356,361) are
// summed like the others and dropped when the scores are formed.  seen_max: the sum of the
// largest child of every point (the early-exit bound of the queue's chains; kWantMax = false, a
// dive, which never gives up: not formed, seen_max untouched).
template <int kFirst, int kCount, bool kWantMax>
__device__ __forceinline__ void ChainGather(const ChainLevel& L, const uint32_t (&cell)[kChainCells],
                                            uint32_t* even, uint32_t* odd, int* seen_max) {
  typedef unsigned short Halves __attribute__((ext_vector_type(2)));
  uint32_t v[kCount];
#pragma unroll
  for (int u = 0; u < kCount; ++u) {
    const uint32_t p = cell[kFirst + u];
    const unsigned X = static_cast<unsigned>(static_cast<short>(p & 0xffffu) + L.ax);
    const unsigned Y = static_cast<unsigned>(static_cast<short>(p >> 16) + L.ay);
    const bool inside = X < static_cast<unsigned>(L.qx) && Y < static_cast<unsigned>(L.qy);
    // QuadOffset(X, Y, qtx) * 4, branch-free, the tile index by a 24-bit multiply-add
    // (inside: Y >> 2 and qtx are far below 2^24)
    const unsigned tile = __umul24(Y >> 2, static_cast<unsigned>(L.qtx)) + (X >> 3);
    const unsigned byte = (tile << 7) | ((Y & 3u) << 5) | ((X & 7u) << 2);
    v[u] = __builtin_amdgcn_raw_buffer_load_b32(L.quad_rsrc, inside ? byte : 0xfffffff0u, 0, 0);
  }
#pragma unroll
  for (int u = 0; u < kCount; ++u) {
    const uint32_t e = v[u] & 0x00ff00ffu, o = (v[u] >> 8) & 0x00ff00ffu;
    *even += e;
    *odd += o;
    if constexpr (kWantMax) {
      Halves eh, oh;
      __builtin_memcpy(&eh, &e, 4);
      __builtin_memcpy(&oh, &o, 4);
      const Halves m = __builtin_elementwise_max(eh, oh);
      *seen_max += static_cast<int>(max(m.x, m.y));
    }
  }
}

// The dive of DiveKernel, one per WAVEFRONT: the chain a worker of TreeQueueKernel walks, with
// nothing pushed and no bound to give up at.  The scan's cells sit in registers, every gather of a
// level is in flight at once, the children are summed and ranked by wavefront reductions: no LDS
// and no barrier behind the seed selection.  A workgroup selects once (256 threads, so the seeds
// are DiveKernel's) and dives into what it selected: the three rotations of ONE seed unit under
// group bounds (the fourth wavefront leaves), four seeds otherwise.  Leaves, bound and work
// counters as DiveKernel leaves them.
__global__ void __launch_bounds__(256)
DiveWaveKernel(const Fast2DProblem* __restrict__ problems, ProblemState* __restrict__ states, int n,
               NodeList leaves, Counters* __restrict__ counters) {
  const int problem = blockIdx.y;
  const Fast2DProblem& P = problems[problem];
  ProblemState& st = states[problem];
  if (st.error) return;
  __shared__ SeedScratch seed_scratch;
  const bool grouped = P.group > 1;
  const int seeds = grouped ? 1 : 4;
  const int want0 = static_cast<int>(blockIdx.x) * seeds;
  if (want0 >= kSeedsPerProblem) return;
  PickSeeds(P, n, want0, seeds, &seed_scratch);
  if (blockIdx.x == 0 && threadIdx.x == 0) st.coarse_total = seed_scratch.total;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (grouped && wave >= kFusedGroup) return;
  int seed_scan = __builtin_amdgcn_readfirstlane(seed_scratch.found_scan[grouped ? 0 : wave]);
  if (seed_scan < 0) return;
  if (grouped) {
    seed_scan = seed_scan - seed_scan % kFusedGroup + wave;
    if (seed_scan >= P.num_scans) return;
  }
  const Node2D seed = CoarseNode(P, problem, seed_scan, P.scan_best[seed_scan].y);
  uint32_t cell[kChainCells];
  // The front end has written this rotation's cells if it writes all of them, or (store_scans) if
  // the rotation's OWN best candidate reaches the threshold -- the test it applies itself, on the
  // sum it left in scan_best.  An outer rotation of a seed unit may miss it (its window need not
  // hold the candidate its unit qualified by): its cells are re-derived, sixteen ScanCells a lane.
  const bool stored =
      !P.recompute_scans ||
      (P.store_scans && !(ToScore(P, P.scan_best[seed_scan].x, n) < fmaxf(P.min_score, 0.f)));
  if (__builtin_amdgcn_readfirstlane(stored ? 1 : 0)) LoadChainCells<false>(P, n, seed_scan, cell);
  else LoadChainCells<true>(P, n, seed_scan, cell);
  const int4 bd = P.bounds[seed_scan];
  const int depth = P.depth;
  int dx = __builtin_amdgcn_readfirstlane(seed.dx), dy = __builtin_amdgcn_readfirstlane(seed.dy);
  float score = seed.score;
  unsigned long long scored = 0;
  for (int child_level = depth - 2; child_level >= 0; --child_level) {
    const ChainLevel L = MakeChainLevel(P, child_level, dx, dy);
    const bool vx = dx + L.half <= bd.y, vy = dy + L.half <= bd.w;
    uint32_t even = 0, odd = 0;
    if (n > 8 * kWave) ChainGather<0, 16, false>(L, cell, &even, &odd, nullptr);
    else if (n > 4 * kWave) ChainGather<0, 8, false>(L, cell, &even, &odd, nullptr);
    else ChainGather<0, 4, false>(L, cell, &even, &odd, nullptr);
    const int total[4] = {WaveSum(static_cast<int>(even & 0xffffu)), WaveSum(static_cast<int>(odd & 0xffffu)),
                          WaveSum(static_cast<int>(even >> 16)), WaveSum(static_cast<int>(odd >> 16))};
    // child k = 2 * x-step + y-step (generation order: x outer, y inner); the dive goes on with
    // the one the reference's stable descending sort puts first: the best, ties to the lower index
    int kbest = 0, nvalid = 0;
    float best_score = -1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool valid = ((k >> 1) == 0 || vx) && ((k & 1) == 0 || vy);
      const float sc = valid ? ToScore(P, total[k], n) : -1.f;
      nvalid += valid ? 1 : 0;
      if (sc >= 0.f && (k == 0 || sc > best_score)) { kbest = k; best_score = sc; }
    }
    kbest = __builtin_amdgcn_readfirstlane(kbest);
    dx += (kbest >> 1) * L.half;
    dy += (kbest & 1) * L.half;
    score = best_score;
    scored += nvalid;
  }
  if (lane == 0) {
    if (score > P.min_score) {
      Node2D leaf = seed;          // (rank 0 at every level: the path stays 0)
      leaf.problem = problem;      // level 0
      leaf.dx = dx;
      leaf.dy = dy;
      leaf.score = score;
      RecordLeaf(leaf, leaves, counters);
      atomicMax(&st.best_bits, __float_as_uint(score));
    }
    const int shard = (blockIdx.x * 4 + wave) & (kStatShards - 1);
    atomicAdd(&st.scored_shard[shard], scored);
    atomicAdd(&st.expanded_shard[shard], static_cast<unsigned long long>(depth - 1));
  }
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

// ---------------------------------------------------------------------------
// Host: the scratch block of a search
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
size_t SearchMiscBytes(int num) { return sizeof(Counters) + SearchTail::Bytes(num); }

// ---------------------------------------------------------------------------
// Host: one search of a prepared batch
// ---------------------------------------------------------------------------
// What the strategies below share and hand to each other: the lists and the scratch block of the
// call, and the state of the overflow fall-back (`strict`, `num_chunks`).
struct SearchRun {
  SearchRun(Workspace& ws, const PreparedBatch& batch, BatchResult* result);
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
  // (the two frontier buffers: reserved by the strategy that runs)
  Node2D* d_front[2] = {nullptr, nullptr};
  NodeList leaf_list;
  Counters* d_counters;
  SearchTail d_tail, h_tail;
  bool direct;                            // the last kernel stores the tail into h_tail itself
  int strict = 0;                         // 1: prune ties, record only improving leaves
  int num_chunks = 1;                     // the scans go through the level-synchronous path in chunks
};

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

// depth == 1: the lowest-resolution candidates are the leaves, no tree.
void RunDepthOne(SearchRun& run) {
  Workspace& ws = run.ws;
  SelectDepthOneKernel<<<run.num, 1024, 0, ws.stream>>>(
      run.batch.d_problems, run.batch.d_states, run.n, run.d_tail.best, run.d_tail.states);
  CMX_HIP(hipGetLastError());
  RecordEvent(ws.ev_end, ws.stream);
  run.FetchResults(false);
}

// Whether a wavefront can walk chains of this batch's nodes (LoadChainCells, ChainGather): it
// holds a scan in registers and gathers quads through buffer resources (2 GB per level).
bool ChainWalkPossible(const SearchRun& run) {
  bool chain_ok = run.n <= kChainCells * kWave;
  for (const Fast2DProblem& P : run.batch.h_problems)
    for (int l = 0; l + 1 < run.depth; ++l)
      chain_ok = chain_ok && static_cast<unsigned long long>((P.level[l].qy + 3) >> 2) *
                                     static_cast<unsigned>(P.level[l].qtx) * 128ull < (1ull << 31);
  return chain_ok;
}

// Whether the work queue can take this batch: its wavefronts walk chains, of stored cells.
bool QueueSearchPossible(const SearchRun& run) {
  bool queue_ok = QueueSearchWanted(run.n, run.num) && ChainWalkPossible(run);
  for (const Fast2DProblem& P : run.batch.h_problems)
    queue_ok = queue_ok && (P.recompute_scans == 0 || P.store_scans != 0);
  return queue_ok;
}

// ---- the work queue: filter + ONE launch for the whole tree and the selection ---------
// Takes over the caller's turn at the launch path (held since the dive) and gives it up behind
// the tree launch, before it waits for the results.
enum class QueueOutcome { kDone, kLeafOverflow, kQueueOverflow };

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
  run.d_front[0] = ws.dev[10].ReserveAs<Node2D>(run.frontier_capacity);
  FilterCoarseKernel<<<dim3(DivUp(batch.max_scans, 4), num), 256, 0, ws.stream>>>(
      batch.d_problems, batch.d_states, n, 0, 1, /*strict=*/0, /*affinity=*/0, run.Front(0),
      run.d_counters);
  run.Mark("filter");
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

// ---- the level-synchronous chain: filter, wave stages, subtree stages, selection ---------
// Top of the tree per scan, then the subtrees of the survivors down to the leaves on many
// blocks; over `run.num_chunks` chunks of scans, and once more in strict mode for as long as a
// list overflows.
void RunLevelSynchronous(SearchRun& run) {
  Workspace& ws = run.ws;
  const PreparedBatch& batch = run.batch;
  BatchResult* result = run.result;
  const int num = run.num, n = run.n;
  const CountersSummary& h_counters = *run.h_tail.summary;
  // Stage shape (tunable for experiments through the environment).
  const int kLevelsPerStage = std::max(0, Debug().fast2d_levels_per_stage);
  const int kWaveLevels = Debug().fast2d_wave_levels > 0 ? Debug().fast2d_wave_levels - 1 : -1;
  // Single searches are latency-bound: one wave stage, then one depth-first
  // kernel down to the leaves.  Batches are throughput-bound: two wave stages,
  // then depth-first stages of two levels.
  const int levels_per_stage = kLevelsPerStage > 0 ? kLevelsPerStage : (num < 4 ? kMaxDepth : 2);
  const int wave_levels = kWaveLevels >= 0 ? kWaveLevels : (num < 4 ? 1 : 2);
  // Frontier sizes are only known on the device; grids are sized for the
  // typical case (a few thousand nodes at the top, tens below) and every
  // kernel grid-strides, so larger frontiers (big batches) still fill the chip.
  // Batches: one problem's nodes stay on one XCD (debug switch fast2d_xcd_affinity overrides).
  const int affinity_override = Debug().fast2d_xcd_affinity;
  const int affinity = affinity_override ? affinity_override - 1 : (num >= 16 ? 1 : 0);
  const int wide_blocks = std::min(4096, 1024 * std::max(1, (num + 3) / 4));
  const int narrow_blocks = std::min(4096, 512 * std::max(1, (num + 3) / 4));
  run.d_front[0] = ws.dev[10].ReserveAs<Node2D>(run.frontier_capacity);
  run.d_front[1] = ws.dev[11].ReserveAs<Node2D>(run.frontier_capacity);
  for (;;) {
    const int strict = run.strict;
    for (int chunk = 0; chunk < run.num_chunks; ++chunk) {
      if (chunk > 0 || strict)
        CMX_HIP(hipMemsetAsync(run.d_counters->frontier, 0, sizeof(run.d_counters->frontier),
                               ws.stream));
      FilterCoarseKernel<<<dim3(DivUp(batch.max_scans, 4), num), 256, 0, ws.stream>>>(
          batch.d_problems, batch.d_states, n, chunk, run.num_chunks, strict, affinity,
          run.Front(0), run.d_counters);
      run.Mark("filter");
      int stage = 0;
      int top = run.depth - 1;
      // Wave-per-node level-synchronous expansion of the (wide, shallow-lived)
      // top levels.  (Timed for the statistics in the first pass of a batch: there the
      // expansion is the dominant kernel; a single search's chain of launches is not given
      // two more event packets to wait behind.)
      const bool timed = !strict && chunk == 0 && num >= 4;
      if (timed) RecordEvent(ws.ev_x0, ws.stream);
      for (int used = 0; used < wave_levels && top - 1 >= 1; ++used, --top, ++stage) {
        ExpandWaveKernel<<<used == 0 ? wide_blocks : narrow_blocks, 256, 0, ws.stream>>>(
            batch.d_problems, batch.d_states, n, run.Front(stage), strict, affinity,
            run.Front(stage + 1), run.d_counters);
        run.Mark("wave");
      }
      if (timed) {
        RecordEvent(ws.ev_x1, ws.stream);
        result->expansion_launches = stage;
      }
      // Block-per-node depth-first stages of kLevelsPerStage levels: the bushy
      // part of the tree near the optimum spreads over many blocks instead of
      // being walked serially by one.
      for (; top > 0; top -= levels_per_stage, ++stage) {
        const int stop = std::max(0, top - levels_per_stage);
        SubtreeKernel<<<narrow_blocks, 256, 0, ws.stream>>>(
            batch.d_problems, batch.d_states, n, run.Front(stage), stop, strict,
            run.Front(stage + 1), run.leaf_list, run.d_counters);
        run.Mark("subtree");
      }
    }
    SelectBestKernel<<<1, 1024, 0, ws.stream>>>(
        run.leaf_list, batch.d_states, run.d_tail.sel, run.d_tail.best, num, run.d_tail.states,
        run.d_counters, run.d_tail.summary, run.d_tail.words(), run.PublishTo(),
        run.h_tail.num_words());
    run.Mark("select");
    CMX_HIP(hipGetLastError());
    RecordEvent(ws.ev_end, ws.stream);
    run.FetchResults(run.direct);
    if (!strict) {
      for (int st = 0; st < result->expansion_launches; ++st)
        result->expansion_nodes += h_counters.frontier_total[st];
      result->expansion_lookups = 64ll * h_counters.wave_gathers;
    }
    if (!h_counters.frontier_overflow && !h_counters.leaf_overflow) break;
    run.PrepareStrictRetry();
  }
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

// The work-queue tree search (TreeQueueKernel) holds a scan in registers, 16 cells per lane.
// Debug switch fast2d_queue: 2 = the chain of level-synchronous launches of rounds 2 - 5 (the
// parity partner, and the path a queue overflow falls back to).
// Batches of four or more problems stay on the level-synchronous launches: wide frontiers of many
// problems keep the chip busy there, and they measure faster (16 submaps: 1.4 against 2.7 ms).
bool QueueSearchWanted(int n, int num) {
  return Debug().fast2d_queue != 2 && n <= kChainCells * kWave && (num < 4 || Debug().fast2d_queue == 1);
}

// Carved before the first kernel of a call so that it can clear the counters.
void ReserveSearchScratch(Workspace& ws, int num, PreparedBatch* batch) {
  batch->d_misc = static_cast<char*>(ws.dev[14].Reserve(SearchMiscBytes(num)));
  batch->num_counter_words = static_cast<int>(sizeof(Counters) / sizeof(int));
}

// (debug switch host_trace: where a caller's wall clock goes -- tools only)
thread_local long long g_host_wait_ns = 0;

// Full search of a prepared batch: picks the strategy and performs the fall-backs.
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
    // A wavefront per dive wherever a wavefront can hold the scan; a workgroup per dive for larger
    // clouds and as the parity partner (debug switch fast2d_dive).
    if (Debug().fast2d_dive != 1 && ChainWalkPossible(run)) {
      DiveWaveKernel<<<dim3(batch.any_group ? kSeedsPerProblem : kSeedsPerProblem / 4, num), 256, 0,
                       ws.stream>>>(batch.d_problems, batch.d_states, run.n, run.leaf_list,
                                    run.d_counters);
    } else {
      DiveKernel<<<dim3(kSeedsPerProblem * (batch.any_group ? kFusedGroup : 1), num), 256, 0, ws.stream>>>(
          batch.d_problems, batch.d_states, run.n, run.leaf_list, run.d_counters);
    }
    run.Mark("seed+dive");
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
