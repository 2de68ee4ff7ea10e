// The fast 2D tree search with a WAVEFRONT per chain: what a wavefront that walks a chain of nodes
// of ONE scan does per scan and per expansion -- the scan's cells in registers, every gather of a
// level in flight at once, no LDS and no barrier.  Used by DiveWaveKernel's dives
// (fast_2d_seed.hip) and TreeQueueKernel's chains (fast_2d_queue.hip) only; the
// workgroup-per-node counterpart is fast_2d_block_device.h.  Which batches a wavefront can walk:
// ChainWalkPossible (fast_2d_seed.hip).
//
// Device code and plain structs only, in the unnamed namespace of the kernels (see
// fast_2d_search_device.h).
#ifndef CMX_FAST_2D_CHAIN_DEVICE_H_
#define CMX_FAST_2D_CHAIN_DEVICE_H_

#include "fast_2d_search_device.h"

namespace cmx {
namespace {

constexpr int kChainCells = 16;     // cells per lane held in registers: clouds of up to 1024 points
constexpr uint32_t kNoCell = 0x80008000u;   // (x, y) = (-32768, -32768): outside every level

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

}  // namespace
}  // namespace cmx

#endif  // CMX_FAST_2D_CHAIN_DEVICE_H_
