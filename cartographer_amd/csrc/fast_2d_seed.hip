// FastCorrelativeScanMatcher2D on gfx950: what runs before either strategy of the tree search.
//
// Owns the seed selection (PickSeeds), the dive kernels (DiveKernel: a workgroup per dive;
// DiveWaveKernel: a wavefront per dive) and the lowest-resolution filter (FilterCoarseKernel).
// Exports the stage functions LaunchDive and LaunchFilter (and LaunchSubtree, below), and
// ChainWalkPossible, the test both the dive and the work queue apply before a wavefront walks a
// chain (fast_2d_search.h).
//
// The dive gives every problem a real leaf score, a valid lower bound, before the tree is
// searched; the filter hands the lowest-resolution nodes that reach that bound to the strategy
// that runs: the work queue (fast_2d_queue.hip) or the level-synchronous chain
// (fast_2d_levels.hip).
//
// One guest: SubtreeKernel, the depth-first stage of the level-synchronous strategy, with its
// stage function LaunchSubtree.  It is the other user of the workgroup-per-node code
// (fast_2d_block_device.h), and the compiler's code for DiveKernel depends on which users of the
// helpers it inlines are compiled with it: DiveKernel comes out instruction for instruction as
// tuned and measured only in one unit with BOTH DiveWaveKernel (PickSeeds) and SubtreeKernel
// (LoadContext, ScoreChildren); tools/kernel_isa_diff.py shows it.  So the three stay together.
#include "fast_2d_block_device.h"
#include "fast_2d_chain_device.h"
#include "fast_2d_search.h"

namespace cmx {
namespace {

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

// (A stage of the level-synchronous strategy, fast_2d_levels.hip, which launches it through
// LaunchSubtree.  It is defined here, next to DiveKernel: see the head of this file.)
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

}  // namespace

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

// A wavefront per dive wherever a wavefront can hold the scan; a workgroup per dive for larger
// clouds and as the parity partner (debug switch fast2d_dive).
void LaunchDive(SearchRun& run) {
  Workspace& ws = run.ws;
  const PreparedBatch& batch = run.batch;
  const int num = run.num;
  if (Debug().fast2d_dive != 1 && ChainWalkPossible(run)) {
    DiveWaveKernel<<<dim3(batch.any_group ? kSeedsPerProblem : kSeedsPerProblem / 4, num), 256, 0,
                     ws.stream>>>(batch.d_problems, batch.d_states, run.n, run.leaf_list,
                                  run.d_counters);
  } else {
    DiveKernel<<<dim3(kSeedsPerProblem * (batch.any_group ? kFusedGroup : 1), num), 256, 0, ws.stream>>>(
        batch.d_problems, batch.d_states, run.n, run.leaf_list, run.d_counters);
  }
  run.Mark("seed+dive");
}

void LaunchFilter(SearchRun& run, int chunk, int num_chunks, int strict, int affinity) {
  const PreparedBatch& batch = run.batch;
  FilterCoarseKernel<<<dim3(DivUp(batch.max_scans, 4), run.num), 256, 0, run.ws.stream>>>(
      batch.d_problems, batch.d_states, run.n, chunk, num_chunks, strict, affinity, run.Front(0),
      run.d_counters);
  run.Mark("filter");
}

void LaunchSubtree(SearchRun& run, int stage, int stop_level, int strict, int blocks) {
  const PreparedBatch& batch = run.batch;
  SubtreeKernel<<<blocks, 256, 0, run.ws.stream>>>(
      batch.d_problems, batch.d_states, run.n, run.Front(stage), stop_level, strict,
      run.Front(stage + 1), run.leaf_list, run.d_counters);
  run.Mark("subtree");
}

}  // namespace cmx
