// FastCorrelativeScanMatcher2D on gfx950: the level-synchronous strategy of the tree search.
//
// Owns ExpandWaveKernel (a wavefront per node, the wide top levels) and SelectBestKernel (the
// selection as a launch of its own).  Exports the stage function RunLevelSynchronous
// (fast_2d_search.h).
//
// A chain of launches behind the dive: filter (LaunchFilter), wave stages, subtree stages
// (LaunchSubtree: SubtreeKernel, a workgroup per node, depth first below the wave stages, is
// compiled next to DiveKernel in fast_2d_seed.hip, whose head says why), selection.  It is what
// batches of four and more problems run, what a queue overflow falls back
// to (it has room for millions of nodes), the parity partner of the work queue
// (fast_2d_queue.hip), and -- in strict mode, over chunks of scans -- the retry after a list
// overflow.
#include <algorithm>
#include <type_traits>

#include "fast_2d_search.h"

namespace cmx {
namespace {

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
    // made per point -- `recompute ? ScanCell(...) : pts[...]` inside the unrolled body -- every
    // one of the four "gathers in flight" begins with a branch and a basic block of its own, and
    // the compiler closes each with s_waitcnt vmcnt(0): ONE gather in flight per wavefront,
    // sixteen dependent round trips per node.)
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

// The one block that selects (SelectBestBody, fast_2d_search_device.h) also PUBLISHES: everything
// the host reads after a search (the counters' summary, selection states, best leaves, problem
// states: `tail_words` dwords behind the counters) goes from device memory straight into the
// caller's pinned buffer (mapped into the device's address space) -- no copy kernel behind this
// one in a chain of launches that is latency from end to end.  tail_host == nullptr: the host
// fetches the tail itself.
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

}  // namespace

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
  run.ReserveFronts(2);
  for (;;) {
    const int strict = run.strict;
    for (int chunk = 0; chunk < run.num_chunks; ++chunk) {
      if (chunk > 0 || strict)
        CMX_HIP(hipMemsetAsync(run.d_counters->frontier, 0, sizeof(run.d_counters->frontier),
                               ws.stream));
      LaunchFilter(run, chunk, run.num_chunks, strict, affinity);
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
        LaunchSubtree(run, stage, stop, strict, narrow_blocks);
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

}  // namespace cmx
