// What the two translation units of the resident hybrid grid share: grid_3d.hip (the grid, the
// single insertion, the intensity grid) and grid_3d_batch.hip (cmx_grid3d_insert_batch).
#ifndef CMX_GRID_3D_INTERNAL_H_
#define CMX_GRID_3D_INTERNAL_H_

#include <algorithm>
#include <map>

#include "cmx_common.h"
#include "cmx_device.h"
#include "cmx_odds_table.h"

struct cmx_grid3d {
  int device = 0;
  float resolution = 0.f;
  int grid_size = 128;                       // DynamicGrid starts at 2 x 64 voxels per axis
  int lo[3] = {0, 0, 0}, dims[3] = {0, 0, 0};   // brick bounds; empty while dims[0] == 0
  uint16_t* cells = nullptr;                 // device, dims[0] * dims[1] * dims[2]
  std::map<uint32_t, uint16_t*> tables;      // odds tables by float bits, device
};

namespace cmx {

// The odds table of `probability` on the grid's device, uploaded when the grid first asks for it
// and freed with the grid (grid_3d.hip).
const uint16_t* DeviceTable(cmx_grid3d* g, float probability);

// ---- device ------------------------------------------------------------------------------------
struct BrickView {
  uint16_t* cells;
  int lo_x, lo_y, lo_z, nx, ny, nz;
};

// HybridGridBase::GetCellIndex (hybrid_grid.h:428-433): f32 divide, lround.
__device__ __forceinline__ int3 CellOf(const float* __restrict__ p, float resolution) {
  return make_int3(LRoundF32(p[0] / resolution), LRoundF32(p[1] / resolution),
                   LRoundF32(p[2] / resolution));
}

// The sample `position` of ray origin -> hit (range_data_inserter_3d.cc:37-52):
// origin_cell + delta * position / num_samples, integer arithmetic truncating towards zero.
__device__ __forceinline__ int3 MissCell(int3 origin, int3 delta, int position, int num_samples) {
  return make_int3(origin.x + delta.x * position / num_samples,
                   origin.y + delta.y * position / num_samples,
                   origin.z + delta.z * position / num_samples);
}

// HybridGrid::ApplyLookupTable (hybrid_grid.h:471-481) for one voxel.
__device__ __forceinline__ void Apply(const BrickView& b, int3 c,
                                      const uint16_t* __restrict__ table, int* error) {
  const int x = c.x - b.lo_x, y = c.y - b.lo_y, z = c.z - b.lo_z;
  if (static_cast<unsigned>(x) >= static_cast<unsigned>(b.nx) ||
      static_cast<unsigned>(y) >= static_cast<unsigned>(b.ny) ||
      static_cast<unsigned>(z) >= static_cast<unsigned>(b.nz)) {
    *error = 1;                                          // the extent pass sized the brick
    return;
  }
  uint16_t* cell = b.cells + (static_cast<size_t>(z) * b.ny + y) * b.nx + x;
  const uint16_t old = *cell;
  if (old >= kUpdateMarker) return;
  *cell = table[old];
}

// ---- brick growth: plan (host only), stage (device work on a stream), commit -----------------
struct BrickBounds {
  int lo[3] = {0, 0, 0}, dims[3] = {0, 0, 0};            // empty while dims[0] == 0
};

inline int FloorTo(int v, int m) { return v >= 0 ? v / m * m : -((-v + m - 1) / m * m); }

// The bounds a brick of bounds `cur` needs to cover the voxels [lo, hi] (inclusive) as well;
// false: the bounds it has.  It grows in steps of 16 voxels so that a slowly widening scene does
// not re-allocate per scan.
inline bool PlanBrick(const BrickBounds& cur, const int lo[3], const int hi[3], BrickBounds* out) {
  const bool empty = cur.dims[0] == 0;
  bool change = empty;
  for (int k = 0; k < 3; ++k) {
    const int cur_lo = cur.lo[k], cur_hi = cur.lo[k] + cur.dims[k] - 1;
    const int nlo = empty ? FloorTo(lo[k], 16) : std::min(cur_lo, FloorTo(lo[k], 16));
    const int nhi = empty ? FloorTo(hi[k], 16) + 15 : std::max(cur_hi, FloorTo(hi[k], 16) + 15);
    change |= nlo != cur_lo || nhi != cur_hi;
    out->lo[k] = nlo;
    out->dims[k] = nhi - nlo + 1;
  }
  return change;
}

inline long long BrickCells(const BrickBounds& b) {      // (each dimension < 2^21)
  return static_cast<long long>(b.dims[0]) * b.dims[1] * b.dims[2];
}
constexpr long long kMaxBrickCells = 1ll << 30;

// DynamicGrid::mutable_value grows until every written index fits (hybrid_grid.h:282-287).
inline int PlanGridSize(int grid_size, const int lo[3], const int hi[3]) {
  const auto fits = [&](int v) { return v >= -(grid_size / 2) && v < grid_size / 2; };
  for (int k = 0; k < 3; ++k)
    while (!(fits(lo[k]) && fits(hi[k]))) grid_size *= 2;
  return grid_size;
}

// A zeroed brick of bounds `to` with the grid's cells copied into their place, queued on
// `stream`: the grid itself is not touched, and its old brick must stay until the stream has got
// there.  The caller owns the result until CommitBrick (hipFree it otherwise).
uint16_t* StageGrownBrick(const cmx_grid3d* g, const BrickBounds& to, hipStream_t stream);
// The grid takes `grown` (staged and complete) and releases the brick it had.
void CommitBrick(cmx_grid3d* g, uint16_t* grown, const BrickBounds& to);

}  // namespace cmx

#endif  // CMX_GRID_3D_INTERNAL_H_
