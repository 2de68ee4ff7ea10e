// The fast 2D tree search with a WORKGROUP per node: what a 256-thread block keeps on chip while it
// works on nodes of one rotated scan, and how it scores a node's children.  Used by DiveKernel
// and SubtreeKernel only (both in fast_2d_seed.hip); the wavefront-per-chain counterpart is
// fast_2d_chain_device.h.
//
// Device code and plain structs only, in the unnamed namespace of the kernels (see
// fast_2d_search_device.h).
#ifndef CMX_FAST_2D_BLOCK_DEVICE_H_
#define CMX_FAST_2D_BLOCK_DEVICE_H_

#include <type_traits>

#include "fast_2d_search_device.h"

namespace cmx {
namespace {

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
  // The gathers of the unrolled loop are meant to be in flight together.  They are not with
  // `cached ? ctx.cache[i] : gpts[i]` inside the body: that gives every unrolled iteration a
  // branch and a basic block of its own, closed with s_waitcnt vmcnt(0) lgkmcnt(0) -- which also
  // waits for the previous iteration's gather -- and the plain `quads[inside ? offset : 0]`
  // becomes a load under an exec mask.  Hence: one loop per source of the cells (compile-time),
  // quads by buffer loads (out-of-range offsets read 0; a level of more than 2 GB of quads keeps
  // plain loads).
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

}  // namespace
}  // namespace cmx

#endif  // CMX_FAST_2D_BLOCK_DEVICE_H_
