// The per-cell arithmetic of the fast 3D matcher's precomputation stack and the host rule of its
// geometry, shared by the kernels that build ONE matcher (fast_3d_stack.hip) and by their twins
// that build the matchers of many submaps in one chain of launches (fast_3d_stack_batch.hip): a
// single kernel and its twin call the same function, so a batch-built matcher is the single
// create's bit for bit.
#ifndef CMX_FAST_3D_STACK_DEVICE_H_
#define CMX_FAST_3D_STACK_DEVICE_H_

#include <algorithm>

#include "fast_3d_internal.h"

namespace cmx {
namespace {

// ---------------------------------------------------------------------------
// Precomputation stack (gather form of PrecomputeGrid's scatter-max)
// ---------------------------------------------------------------------------
// Cell (tx, ty, tz) of the level above `prev`:
// out(t) = max over octants o and (for half resolution) sub-cells e of
// prev(sub*t + e + shift*o)   <=>   t = (c - shift*o) >> (half ? 1 : 0).
__device__ __forceinline__ unsigned PrecomputedCell3D(const Brick& prev, int tx, int ty, int tz,
                                                      int shift, int half) {
  unsigned best = 0;
  const int sub = half ? 2 : 1;
  for (int oz = 0; oz < 2; ++oz)
    for (int oy = 0; oy < 2; ++oy)
      for (int ox = 0; ox < 2; ++ox)
        for (int ez = 0; ez < sub; ++ez)
          for (int ey = 0; ey < sub; ++ey)
            for (int ex = 0; ex < sub; ++ex)
              best = max(best, BrickValueU8(prev, sub * tx + ex + shift * ox,
                                            sub * ty + ey + shift * oy,
                                            sub * tz + ez + shift * oz));
  return best;
}

// Word (X, Y, Z) of level L's oct array (OctDesc): byte k = L(x + (k & 1) s, y + (k >> 1 & 1) s,
// z + (k >> 2) s) with (x, y, z) = (X, Y, Z) - s relative to the brick, cells outside it 0.
__device__ __forceinline__ uint2 OctWord3D(const Brick& L, int s, int X, int Y, int Z) {
  const uint8_t* __restrict__ cells = static_cast<const uint8_t*>(L.cells);
  unsigned lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int x = X - s + ((k & 1) ? s : 0), y = Y - s + ((k & 2) ? s : 0),
              z = Z - s + ((k & 4) ? s : 0);
    unsigned v = 0;
    if (static_cast<unsigned>(x) < static_cast<unsigned>(L.nx) &&
        static_cast<unsigned>(y) < static_cast<unsigned>(L.ny) &&
        static_cast<unsigned>(z) < static_cast<unsigned>(L.nz))
      v = cells[(static_cast<size_t>(z) * L.ny + y) * L.nx + x];
    if (k < 4) lo |= v << (8 * k); else hi |= v << (8 * (k - 4));
  }
  return make_uint2(lo, hi);
}

// ---------------------------------------------------------------------------
// Level 0 and the raw grids from resident HybridGrids
// ---------------------------------------------------------------------------
// The raw value a matcher's copy holds for cell (x, y, z) of the tight box: the source brick's,
// or 0 outside it (an empty grid's one-cell box), as in the voxel path.
__device__ __forceinline__ unsigned CropValue3D(const Brick& src, int x, int y, int z) {
  return src.cells ? BrickValueU16(src, x, y, z) : 0u;
}

// Tight bounds of the non-zero cells of a resident brick (dims in steps of 16 voxels, grid_3d.hip
// EnsureBrick: 8 consecutive cells of the x-fastest array are one 16-byte load within one row):
// groups first, first + stride, ... of 8 cells widen lo / hi.
__device__ __forceinline__ void WidenNonZeroBounds3D(const Brick& b, long long first,
                                                     long long stride, int lo[3], int hi[3]) {
  const long long groups = static_cast<long long>(b.nx) * b.ny * b.nz / 8;
  const uint4* __restrict__ cells = static_cast<const uint4*>(b.cells);
  for (long long g = first; g < groups; g += stride) {
    const uint4 v = cells[g];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    int first_cell = 8, last_cell = -1;      // non-zero cells k of the group (cell 2j = low half)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if ((w[k >> 1] >> (16 * (k & 1))) & 0xffffu) {
        first_cell = min(first_cell, k);
        last_cell = k;
      }
    }
    if (last_cell < 0) continue;
    const long long cell = 8 * g;
    const long long row = cell / b.nx;
    const int x = static_cast<int>(cell - row * b.nx) + b.lo_x;
    const int y = static_cast<int>(row % b.ny) + b.lo_y;
    const int z = static_cast<int>(row / b.ny) + b.lo_z;
    lo[0] = min(lo[0], x + first_cell); hi[0] = max(hi[0], x + last_cell);
    lo[1] = min(lo[1], y); hi[1] = max(hi[1], y);
    lo[2] = min(lo[2], z); hi[2] = max(hi[2], z);
  }
}

// Wave min / max of what the lanes found, one atomic per wave and bound into box[0..2] = min
// x, y, z, box[3..5] = max; untouched (min > max) for a grid without non-zero cells.
__device__ __forceinline__ void MergeBoundsIntoBox3D(const int lo[3], const int hi[3],
                                                     int* __restrict__ box) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int wlo = WaveMin(lo[k]), whi = WaveMax(hi[k]);
    if ((threadIdx.x & 63) == 0 && wlo <= whi) {
      atomicMin(&box[k], wlo);
      atomicMax(&box[3 + k], whi);
    }
  }
}

constexpr int kEmptyBoxLo = 0x7fffffff, kEmptyBoxHi = -0x7fffffff - 1;

}  // namespace

// ---------------------------------------------------------------------------
// Geometry (host): PrecomputationGridStack3D (:57-77) as pure integer work
// ---------------------------------------------------------------------------
// CHECKs of PrecomputationGridStack3D (:60-61).
inline void CheckFast3DOptions(const cmx_fast3d_options& options) {
  CMX_REQUIRE(options.branch_and_bound_depth >= 1 && options.branch_and_bound_depth <= kMaxDepth,
              "branch_and_bound_depth %d outside [1,%d]", options.branch_and_bound_depth,
              kMaxDepth);
  CMX_REQUIRE(options.full_resolution_depth >= 1, "full_resolution_depth must be >= 1");
}

// Level `depth` (>= 1) over level depth - 1 (`prev`), without cells, with the shift and the
// half-resolution flag its kernel takes; `bytes` = its cells.
inline Brick LevelAbove3D(const Brick& prev, int depth, int full_resolution_depth, int* shift,
                          int* half, size_t* bytes) {
  *half = depth >= full_resolution_depth ? 1 : 0;
  const int last_width = 1 << (depth - 1), next_width = 1 << depth;
  const int per_voxel = 1 << std::max(0, depth - full_resolution_depth);
  *shift = (next_width - last_width + (per_voxel - 1)) / per_voxel;
  Brick b{};
  int lo[3] = {prev.lo_x - *shift, prev.lo_y - *shift, prev.lo_z - *shift};
  int hi[3] = {prev.lo_x + prev.nx - 1, prev.lo_y + prev.ny - 1, prev.lo_z + prev.nz - 1};
  if (*half) {
    for (int k = 0; k < 3; ++k) { lo[k] >>= 1; hi[k] >>= 1; }
  }
  b.lo_x = lo[0]; b.lo_y = lo[1]; b.lo_z = lo[2];
  b.nx = hi[0] - lo[0] + 1; b.ny = hi[1] - lo[1] + 1; b.nz = hi[2] - lo[2] + 1;
  *bytes = static_cast<size_t>(b.nx) * b.ny * b.nz;
  CMX_REQUIRE(*bytes < (size_t(1) << 31), "precomputation level too large");
  return b;
}

// The oct array of level i (a child level: i + 1 < depth), without cells.  False: the level keeps
// byte loads (an array of 2^32 bytes and more: 32-bit offsets elsewhere).
inline bool OctOfLevel3D(const Brick& L, int i, int full_resolution_depth, OctDesc* oct,
                         size_t* bytes) {
  OctDesc O{nullptr, 0, 0, 0, 0};
  O.s = 1 << std::min(i, full_resolution_depth - 1);
  O.qx = L.nx + O.s; O.qy = L.ny + O.s; O.qz = L.nz + O.s;
  const size_t count = static_cast<size_t>(O.qx) * O.qy * O.qz;
  if (count * sizeof(uint2) >= (size_t(1) << 32)) return false;
  *oct = O;
  *bytes = count * sizeof(uint2);
  return true;
}

}  // namespace cmx

#endif  // CMX_FAST_3D_STACK_DEVICE_H_
