// Grid2D::GrowLimits composed over every doubling of a batched insertion call, for all grids of
// the call that grow in one launch: cmx_grid2d_insert_batch (one plane of cells) and
// cmx_tsdf2d_insert_batch (the tsd and weight planes, and the owner plane back at its idle value).
#ifndef CMX_GRID_GROW_BATCH_H_
#define CMX_GRID_GROW_BATCH_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cmx_batch.h"

namespace cmx {

// The old grid lands at its final offset in the new storage, everything around it is unknown (0).
template <int kPlanes>
struct GrowDesc {
  const uint16_t* old_cells[kPlanes];
  uint16_t* grown[kPlanes];
  int32_t* fill;              // nx * ny words set to `fill_value`; null: none
  int32_t fill_value;
  int old_nx, old_ny, nx, ny, start_x, start_y;
};

// blockIdx.y = grid.
template <int kPlanes>
__global__ void __launch_bounds__(256) BatchGrowKernel(const GrowDesc<kPlanes>* __restrict__ descs) {
  const GrowDesc<kPlanes>& G = descs[blockIdx.y];
  const size_t count = static_cast<size_t>(G.nx) * G.ny;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < count;
       i += static_cast<size_t>(gridDim.x) * 256) {
    const int x = static_cast<int>(i % G.nx) - G.start_x;
    const int y = static_cast<int>(i / G.nx) - G.start_y;
    const bool old = static_cast<unsigned>(x) < static_cast<unsigned>(G.old_nx) &&
                     static_cast<unsigned>(y) < static_cast<unsigned>(G.old_ny);
#pragma unroll
    for (int p = 0; p < kPlanes; ++p)
      G.grown[p][i] = old ? G.old_cells[p][static_cast<size_t>(y) * G.old_nx + x] : uint16_t{0};
    if (G.fill) G.fill[i] = G.fill_value;
  }
}

// `num` descriptors on the device; `largest_cells`: the most cells any of the grown grids has.
template <int kPlanes>
void LaunchBatchGrow(const GrowDesc<kPlanes>* d_descs, size_t num, size_t largest_cells,
                     hipStream_t stream) {
  const unsigned columns =
      static_cast<unsigned>(std::min<long long>(BlocksOf(largest_cells, 256), 4096));
  for (size_t first = 0; first < num; first += 65535) {
    const unsigned rows = static_cast<unsigned>(std::min<size_t>(num - first, 65535));
    BatchGrowKernel<kPlanes><<<dim3(columns, rows), 256, 0, stream>>>(d_descs + first);
  }
}

}  // namespace cmx
#endif  // CMX_GRID_GROW_BATCH_H_
