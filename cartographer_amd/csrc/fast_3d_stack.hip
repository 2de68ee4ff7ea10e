// The precomputation stack of the fast 3D matcher (Fast3DMatcher), from voxel lists or from two
// resident HybridGrids, and its introspection entries (reference map: fast_3d.hip).
#include <algorithm>

#include "fast_3d_stack_device.h"

namespace cmx {
namespace {

// The per-cell arithmetic of these kernels is fast_3d_stack_device.h's, shared with their twins
// in fast_3d_stack_batch.hip.
__global__ void PrecomputeLevel3DKernel(Brick prev, Brick out, int shift, int half) {
  const long long total = static_cast<long long>(out.nx) * out.ny * out.nz;
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int ix = static_cast<int>(i % out.nx);
  const int iy = static_cast<int>((i / out.nx) % out.ny);
  const int iz = static_cast<int>(i / (static_cast<long long>(out.nx) * out.ny));
  static_cast<uint8_t*>(const_cast<void*>(out.cells))[i] = static_cast<uint8_t>(
      PrecomputedCell3D(prev, ix + out.lo_x, iy + out.lo_y, iz + out.lo_z, shift, half));
}

__global__ void BuildOct3DKernel(Brick L, int s, uint2* __restrict__ out, int qx, int qy, int qz) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<size_t>(qx) * qy * qz) return;
  const int X = static_cast<int>(i % qx), Y = static_cast<int>((i / qx) % qy),
            Z = static_cast<int>(i / (static_cast<size_t>(qx) * qy));
  out[i] = OctWord3D(L, s, X, Y, Z);
}

// ---------------------------------------------------------------------------
// Level 0 and the raw grids from two resident HybridGrids (cmx_fast3d_create_from_grids)
// ---------------------------------------------------------------------------
// The bricks of the high- (blockIdx.y == 0) and low-resolution grid (1) as cmx_grid3d keeps them:
// dims in steps of 16 voxels (grid_3d.hip EnsureBrick), so 8 consecutive cells of the x-fastest
// array are one 16-byte load within one row.
struct GridPair3D {
  Brick grid[2];
};

// Tight bounds of the non-zero cells: box[6 g + 0..2] = min x, y, z, box[6 g + 3..5] = max of grid
// g; untouched (min > max) for a grid without any.  Grid-stride over groups of 8 cells, wave
// min / max, one atomic per wave and bound (as Grid3DExtentKernel).
__global__ void __launch_bounds__(256)
Grid3DNonZeroBoundsKernel(GridPair3D pair, int* __restrict__ box) {
  const Brick b = pair.grid[blockIdx.y];
  int lo[3] = {kEmptyBoxLo, kEmptyBoxLo, kEmptyBoxLo}, hi[3] = {kEmptyBoxHi, kEmptyBoxHi,
                                                                kEmptyBoxHi};
  WidenNonZeroBounds3D(b, static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x,
                       static_cast<long long>(gridDim.x) * blockDim.x, lo, hi);
  MergeBoundsIntoBox3D(lo, hi, box + 6 * blockIdx.y);
}

// One thread per cell of the tight boxes (x fastest): grid 0 writes the raw uint16 copy `high` and
// ConvertToPrecomputationGrid's level 0, grid 1 the raw copy `low`.  Cells of the box outside the
// source brick (an empty grid's one-cell box) read 0, as in the voxel path.
__global__ void __launch_bounds__(256)
Grid3DCropKernel(GridPair3D source, Brick high, Brick level0, Brick low) {
  const bool is_high = blockIdx.y == 0;
  const Brick out = is_high ? high : low;
  const long long count = static_cast<long long>(out.nx) * out.ny * out.nz;
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const long long row = i / out.nx;
  const int x = static_cast<int>(i - row * out.nx) + out.lo_x;
  const int y = static_cast<int>(row % out.ny) + out.lo_y;
  const int z = static_cast<int>(row / out.ny) + out.lo_z;
  const unsigned v = CropValue3D(source.grid[blockIdx.y], x, y, z);
  static_cast<uint16_t*>(const_cast<void*>(out.cells))[i] = static_cast<uint16_t>(v);
  if (is_high)
    static_cast<uint8_t*>(const_cast<void*>(level0.cells))[i] = PrecomputationValueDev(v);
}

// PrecomputationGridStack3D (:57-77) over level 0 (m->levels[0]) and the octs of every level
// that can be a child level: the part both constructors share.
void BuildStackAndOcts(Workspace& ws, Fast3DMatcher* matcher) {
  Fast3DMatcher& m = *matcher;
  for (int depth = 1; depth != m.options.branch_and_bound_depth; ++depth) {
    const Brick prev = m.levels.back()->desc;
    std::unique_ptr<DeviceBrick> level(new DeviceBrick);
    int shift, half;
    Brick b = LevelAbove3D(prev, depth, m.options.full_resolution_depth, &shift, &half,
                           &level->bytes);
    CMX_HIP(hipMalloc(&level->mem, level->bytes + 16));   // (+16: aligned 8-byte reads of the last cells)
    b.cells = level->mem;
    level->desc = b;
    PrecomputeLevel3DKernel<<<DivUp(level->bytes, 256), 256, 0, ws.stream>>>(prev, b, shift, half);
    CMX_HIP(hipGetLastError());
    m.levels.push_back(std::move(level));
  }
  // Octs of every level that can be a child level (debug switch fast3d_no_oct: none, tests).
  {
    const bool build_octs = Debug().fast3d_no_oct == 0;
    const int depth = m.options.branch_and_bound_depth;
    m.oct_desc.assign(depth, OctDesc{nullptr, 0, 0, 0, 0});
    for (int i = 0; build_octs && i + 1 < depth; ++i) {
      const Brick L = m.levels[i]->desc;
      OctDesc O;
      std::unique_ptr<DeviceBrick> mem(new DeviceBrick);
      if (!OctOfLevel3D(L, i, m.options.full_resolution_depth, &O, &mem->bytes)) continue;
      CMX_HIP(hipMalloc(&mem->mem, mem->bytes));
      O.cells = static_cast<const uint2*>(mem->mem);
      BuildOct3DKernel<<<DivUp(mem->bytes / sizeof(uint2), 256), 256, 0, ws.stream>>>(
          L, O.s, static_cast<uint2*>(mem->mem), O.qx, O.qy, O.qz);
      CMX_HIP(hipGetLastError());
      m.oct_desc[i] = O;
      m.octs.push_back(std::move(mem));
    }
  }
}

}  // namespace

void CheckVoxelSource3D(float resolution, const cmx_voxel* voxels, int64_t num_voxels,
                        float low_resolution, const cmx_voxel* low_resolution_voxels,
                        int64_t num_low_resolution_voxels, const float* histogram,
                        int32_t histogram_size) {
  CMX_REQUIRE(resolution > 0.f && low_resolution > 0.f, "resolutions must be > 0");
  CMX_REQUIRE(num_voxels == 0 || voxels, "voxels is null");
  CMX_REQUIRE(num_low_resolution_voxels == 0 || low_resolution_voxels, "low voxels null");
  CMX_REQUIRE(histogram_size >= 0 && (histogram_size == 0 || histogram), "bad histogram");
}

void ResidentSource3D(const cmx_grid3d* high_resolution_grid, const cmx_grid3d* low_resolution_grid,
                      const float* histogram, int32_t histogram_size, Brick grid[2],
                      float resolution[2], int32_t* grid_size, int* device) {
  CMX_REQUIRE(high_resolution_grid && low_resolution_grid, "null argument");
  CMX_REQUIRE(histogram_size >= 0 && (histogram_size == 0 || histogram), "bad histogram");
  int on[2];
  const cmx_grid3d* grids[2] = {high_resolution_grid, low_resolution_grid};
  for (int g = 0; g < 2; ++g) {
    if (!Grid3DBrick(grids[g], &grid[g], &resolution[g], &on[g])) grid[g] = Brick{};
    CMX_REQUIRE(grid[g].nx % 8 == 0, "internal error: resident brick not in 8-cell rows");
  }
  CMX_REQUIRE(on[0] == on[1], "the grids live on different devices (%d, %d)", on[0], on[1]);
  *device = on[0];
  const cmx_status status = cmx_grid3d_info(high_resolution_grid, nullptr, grid_size, nullptr);
  CMX_REQUIRE(status == CMX_OK, "cmx_grid3d_info failed");
}

// For sharded.hip: the device a 3D matcher's grids live on.
int Fast3DDevice(const cmx_fast3d* matcher) { return matcher->impl.device; }
// For ceres_3d.hip: the raw grids a 3D matcher keeps in HBM.
void Fast3DGrids(const cmx_fast3d* matcher, Brick* high, float* resolution, Brick* low,
                 float* low_resolution) {
  *high = matcher->impl.high.desc;
  *resolution = matcher->impl.resolution;
  *low = matcher->impl.low.desc;
  *low_resolution = matcher->impl.low_resolution;
}

}  // namespace cmx

extern "C" {

cmx_status cmx_fast3d_create(const cmx_fast3d_options* options, float resolution,
                             int32_t grid_size, const cmx_voxel* voxels, int64_t num_voxels,
                             float low_resolution, const cmx_voxel* low_resolution_voxels,
                             int64_t num_low_resolution_voxels,
                             const float* rotational_scan_matcher_histogram,
                             int32_t histogram_size, int32_t device, cmx_fast3d** out) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(options && out, "null argument");
    *out = nullptr;
    CheckFast3DOptions(*options);
    CheckVoxelSource3D(resolution, voxels, num_voxels, low_resolution, low_resolution_voxels,
                       num_low_resolution_voxels, rotational_scan_matcher_histogram,
                       histogram_size);
    CMX_REQUIRE(grid_size >= GridSizeOf(voxels, num_voxels),
                "grid_size %d is smaller than the voxels' extent", grid_size);
    std::unique_ptr<cmx_fast3d> h(new cmx_fast3d);
    Fast3DMatcher& m = h->impl;
    m.options = *options;
    m.device = device;
    m.resolution = resolution;
    m.low_resolution = low_resolution;
    m.width_in_voxels = grid_size;
    m.histogram.assign(rotational_scan_matcher_histogram,
                       rotational_scan_matcher_histogram + histogram_size);
    WorkspaceLease ws(device);
    m.levels.emplace_back(new DeviceBrick);
    BuildBrickFromVoxels(*ws, voxels, num_voxels, 1, m.levels[0].get());
    CMX_REQUIRE(m.levels[0]->bytes < (size_t(1) << 31), "grid too large");   // 32-bit cell offsets
    BuildBrickFromVoxels(*ws, low_resolution_voxels, num_low_resolution_voxels, 2, &m.low);
    // The raw high-resolution values (level 0 of the stack is their 8-bit quantisation) stay
    // resident for the refinement that follows a match (cmx_fast3d_refine_batch).
    BuildBrickFromVoxels(*ws, voxels, num_voxels, 2, &m.high);
    BuildStackAndOcts(*ws, &m);
    CMX_HIP(hipStreamSynchronize(ws->stream));
    *out = h.release();
  });
}

// The same matcher from two resident HybridGrids.  The bricks never come to the host: one launch
// finds the tight bounds of both grids' non-zero cells (what the voxel path's lists span), one
// crops them into the matcher's own level 0 and raw copies, then the shared stack build.
cmx_status cmx_fast3d_create_from_grids(const cmx_fast3d_options* options,
                                        const cmx_grid3d* high_resolution_grid,
                                        const cmx_grid3d* low_resolution_grid,
                                        const float* rotational_scan_matcher_histogram,
                                        int32_t histogram_size, cmx_fast3d** out) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(options && high_resolution_grid && low_resolution_grid && out, "null argument");
    *out = nullptr;
    CheckFast3DOptions(*options);
    GridPair3D source{};
    float resolution[2];
    int32_t grid_size = 0;
    int on_device = 0;
    ResidentSource3D(high_resolution_grid, low_resolution_grid, rotational_scan_matcher_histogram,
                     histogram_size, source.grid, resolution, &grid_size, &on_device);
    std::unique_ptr<cmx_fast3d> h(new cmx_fast3d);
    Fast3DMatcher& m = h->impl;
    m.options = *options;
    m.device = on_device;
    m.resolution = resolution[0];
    m.low_resolution = resolution[1];
    m.width_in_voxels = grid_size;
    m.histogram.assign(rotational_scan_matcher_histogram,
                       rotational_scan_matcher_histogram + histogram_size);
    WorkspaceLease ws(m.device);
    // (a) Tight bounds; the 12 ints are the only host synchronisation before the allocations.
    int* d_box = ws->dev[1].ReserveAs<int>(12);
    int* h_box = ws->pinned[1].ReserveAs<int>(12);
    for (int g = 0; g < 2; ++g)
      for (int k = 0; k < 3; ++k) {
        h_box[6 * g + k] = kEmptyBoxLo;
        h_box[6 * g + 3 + k] = kEmptyBoxHi;
      }
    const long long groups = std::max(
        static_cast<long long>(source.grid[0].nx) * source.grid[0].ny * source.grid[0].nz,
        static_cast<long long>(source.grid[1].nx) * source.grid[1].ny * source.grid[1].nz) / 8;
    if (groups > 0) {
      CMX_HIP(hipMemcpyAsync(d_box, h_box, 12 * sizeof(int), hipMemcpyHostToDevice, ws->stream));
      const int blocks = static_cast<int>(std::min<long long>(DivUp(groups, 256), 1024));
      Grid3DNonZeroBoundsKernel<<<dim3(blocks, 2), 256, 0, ws->stream>>>(source, d_box);
      CMX_HIP(hipGetLastError());
      CMX_HIP(hipMemcpyAsync(h_box, d_box, 12 * sizeof(int), hipMemcpyDeviceToHost, ws->stream));
      CMX_HIP(hipStreamSynchronize(ws->stream));
    }
    // BuildBrickFromVoxels' boxes: a grid without non-zero cells is the empty voxel list's
    // single cell at the origin.
    int lo[2][3], hi[2][3];
    for (int g = 0; g < 2; ++g)
      for (int k = 0; k < 3; ++k) {
        const bool empty = h_box[6 * g] > h_box[6 * g + 3];
        lo[g][k] = empty ? 0 : h_box[6 * g + k];
        hi[g][k] = empty ? 0 : h_box[6 * g + 3 + k];
      }
    m.levels.emplace_back(new DeviceBrick);
    AllocateDenseBrick(lo[0], hi[0], 1, m.levels[0].get());
    CMX_REQUIRE(m.levels[0]->bytes < (size_t(1) << 31), "grid too large");   // 32-bit cell offsets
    AllocateDenseBrick(lo[0], hi[0], 2, &m.high);
    AllocateDenseBrick(lo[1], hi[1], 2, &m.low);
    // (b) One crop pass over both boxes.
    const long long cells = std::max(m.levels[0]->bytes, m.low.bytes / 2);
    Grid3DCropKernel<<<dim3(DivUp(cells, 256), 2), 256, 0, ws->stream>>>(
        source, m.high.desc, m.levels[0]->desc, m.low.desc);
    CMX_HIP(hipGetLastError());
    // (c) The precomputation stack and the octs, as cmx_fast3d_create builds them.
    BuildStackAndOcts(*ws, &m);
    CMX_HIP(hipStreamSynchronize(ws->stream));
    *out = h.release();
  });
}

void cmx_fast3d_destroy(cmx_fast3d* matcher) {
  if (!matcher) return;
  (void)hipSetDevice(matcher->impl.device);
  delete matcher;
}

// Introspection for the parity tests: dimensions / contents of one
// precomputation level (dense brick, x fastest).
cmx_status cmx_fast3d_level_info(const cmx_fast3d* matcher, int32_t depth, int32_t* lo_xyz,
                                 int32_t* dims_xyz) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(matcher && lo_xyz && dims_xyz, "null argument");
    CMX_REQUIRE(depth >= 0 && depth < static_cast<int>(matcher->impl.levels.size()), "bad depth");
    const Brick& b = matcher->impl.levels[depth]->desc;
    lo_xyz[0] = b.lo_x; lo_xyz[1] = b.lo_y; lo_xyz[2] = b.lo_z;
    dims_xyz[0] = b.nx; dims_xyz[1] = b.ny; dims_xyz[2] = b.nz;
  });
}

cmx_status cmx_fast3d_level_cells(const cmx_fast3d* matcher, int32_t depth, uint8_t* out) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(matcher && out, "null argument");
    CMX_REQUIRE(depth >= 0 && depth < static_cast<int>(matcher->impl.levels.size()), "bad depth");
    UseDevice(matcher->impl.device);
    // (desc.cells: a batch-built matcher's bricks lie in its slab and own no memory)
    const DeviceBrick& b = *matcher->impl.levels[depth];
    CMX_HIP(hipMemcpy(out, b.desc.cells, b.bytes, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
