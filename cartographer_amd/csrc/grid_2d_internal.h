// What the two translation units of the resident probability grid share: grid_2d.hip (the grid,
// the single insertion, the matcher entries) and grid_2d_batch.hip (cmx_grid2d_insert_batch).
#ifndef CMX_GRID_2D_INTERNAL_H_
#define CMX_GRID_2D_INTERNAL_H_

#include <map>

#include "cmx_device.h"
#include "ray_mask_2d.h"
#include "scan_matching_2d.h"

struct cmx_grid2d {
  int device = 0;
  double resolution = 0., max_x = 0., max_y = 0.;
  int nx = 0, ny = 0;
  uint16_t* cells = nullptr;                             // device, nx * ny
  std::map<uint32_t, uint16_t*> tables;                  // odds tables by float bits, device
  unsigned long long version = 1;                        // bumped whenever the cells change
  mutable cmx::Rt2DImageCache rt_image;                  // the real-time matcher's staged image
};

namespace cmx {

struct GridView {
  uint16_t* cells;
  int nx, ny;
  double fine_resolution, max_x, max_y;                  // superscaled limits (:58-62)
};

// MapLimits::GetCellIndex on the superscaled limits (mapping/2d/map_limits.h:69-76).
__device__ __forceinline__ int2 FineIndex(const GridView& g, float px, float py) {
  return make_int2(LRoundF64((g.max_y - static_cast<double>(py)) / g.fine_resolution - 0.5),
                   LRoundF64((g.max_x - static_cast<double>(px)) / g.fine_resolution - 0.5));
}

// ComputeLookupTableToApplyCorrespondenceCostOdds (probability_values.cc:91-105); grid_2d.hip.
void Grid2DOddsTable(float probability, uint16_t* out /*[32768]*/);

}  // namespace cmx

#endif  // CMX_GRID_2D_INTERNAL_H_
