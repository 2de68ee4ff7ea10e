// The precomputation stack of the fast 3D matcher (Fast3DMatcher), from voxel lists or from two
// resident HybridGrids, and its introspection entries (reference map: fast_3d.hip).
#include <algorithm>

#include "fast_3d_internal.h"

namespace cmx {
namespace {

// ---------------------------------------------------------------------------
// Precomputation stack (gather form of PrecomputeGrid's scatter-max)
// ---------------------------------------------------------------------------
__global__ void PrecomputeLevel3DKernel(Brick prev, Brick out, int shift, int half) {
  const long long total = static_cast<long long>(out.nx) * out.ny * out.nz;
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int ix = static_cast<int>(i % out.nx);
  const int iy = static_cast<int>((i / out.nx) % out.ny);
  const int iz = static_cast<int>(i / (static_cast<long long>(out.nx) * out.ny));
  const int tx = ix + out.lo_x, ty = iy + out.lo_y, tz = iz + out.lo_z;
  unsigned best = 0;
  const int sub = half ? 2 : 1;
  // out(t) = max over octants o and (for half resolution) sub-cells e of
  // prev(sub*t + e + shift*o)   <=>   t = (c - shift*o) >> (half ? 1 : 0).
  for (int oz = 0; oz < 2; ++oz)
    for (int oy = 0; oy < 2; ++oy)
      for (int ox = 0; ox < 2; ++ox)
        for (int ez = 0; ez < sub; ++ez)
          for (int ey = 0; ey < sub; ++ey)
            for (int ex = 0; ex < sub; ++ex)
              best = max(best, BrickValueU8(prev, sub * tx + ex + shift * ox,
                                            sub * ty + ey + shift * oy,
                                            sub * tz + ez + shift * oz));
  static_cast<uint8_t*>(const_cast<void*>(out.cells))[i] = static_cast<uint8_t>(best);
}

__global__ void BuildOct3DKernel(Brick L, int s, uint2* __restrict__ out, int qx, int qy, int qz) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<size_t>(qx) * qy * qz) return;
  const int X = static_cast<int>(i % qx), Y = static_cast<int>((i / qx) % qy),
            Z = static_cast<int>(i / (static_cast<size_t>(qx) * qy));
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
  out[i] = make_uint2(lo, hi);
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
  const long long groups = static_cast<long long>(b.nx) * b.ny * b.nz / 8;
  const uint4* __restrict__ cells = static_cast<const uint4*>(b.cells);
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-0x7fffffff - 1, -0x7fffffff - 1,
                                                             -0x7fffffff - 1};
  for (long long g = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; g < groups;
       g += static_cast<long long>(gridDim.x) * blockDim.x) {
    const uint4 v = cells[g];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    int first = 8, last = -1;                // non-zero cells k of the group (cell 2j = low half)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if ((w[k >> 1] >> (16 * (k & 1))) & 0xffffu) {
        first = min(first, k);
        last = k;
      }
    }
    if (last < 0) continue;
    const long long cell = 8 * g;
    const long long row = cell / b.nx;
    const int x = static_cast<int>(cell - row * b.nx) + b.lo_x;
    const int y = static_cast<int>(row % b.ny) + b.lo_y;
    const int z = static_cast<int>(row / b.ny) + b.lo_z;
    lo[0] = min(lo[0], x + first); hi[0] = max(hi[0], x + last);
    lo[1] = min(lo[1], y); hi[1] = max(hi[1], y);
    lo[2] = min(lo[2], z); hi[2] = max(hi[2], z);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int wlo = WaveMin(lo[k]), whi = WaveMax(hi[k]);
    if ((threadIdx.x & 63) == 0 && wlo <= whi) {
      atomicMin(&box[6 * blockIdx.y + k], wlo);
      atomicMax(&box[6 * blockIdx.y + 3 + k], whi);
    }
  }
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
  const Brick src = source.grid[blockIdx.y];
  const unsigned v = src.cells ? BrickValueU16(src, x, y, z) : 0u;
  static_cast<uint16_t*>(const_cast<void*>(out.cells))[i] = static_cast<uint16_t>(v);
  if (is_high)
    static_cast<uint8_t*>(const_cast<void*>(level0.cells))[i] = PrecomputationValueDev(v);
}

// CHECKs of PrecomputationGridStack3D (:60-61).
void CheckFast3DOptions(const cmx_fast3d_options& options) {
  CMX_REQUIRE(options.branch_and_bound_depth >= 1 && options.branch_and_bound_depth <= kMaxDepth,
              "branch_and_bound_depth %d outside [1,%d]", options.branch_and_bound_depth,
              kMaxDepth);
  CMX_REQUIRE(options.full_resolution_depth >= 1, "full_resolution_depth must be >= 1");
}

// PrecomputationGridStack3D (:57-77) over level 0 (m->levels[0]) and the octs of every level
// that can be a child level: the part both constructors share.
void BuildStackAndOcts(Workspace& ws, Fast3DMatcher* matcher) {
  Fast3DMatcher& m = *matcher;
  int last_width = 1;
  for (int depth = 1; depth != m.options.branch_and_bound_depth; ++depth) {
    const bool half = depth >= m.options.full_resolution_depth;
    const int next_width = 1 << depth;
    const int per_voxel = 1 << std::max(0, depth - m.options.full_resolution_depth);
    const int shift = (next_width - last_width + (per_voxel - 1)) / per_voxel;
    const Brick prev = m.levels.back()->desc;
    Brick b{};
    int lo[3] = {prev.lo_x - shift, prev.lo_y - shift, prev.lo_z - shift};
    int hi[3] = {prev.lo_x + prev.nx - 1, prev.lo_y + prev.ny - 1, prev.lo_z + prev.nz - 1};
    if (half) {
      for (int k = 0; k < 3; ++k) { lo[k] >>= 1; hi[k] >>= 1; }
    }
    b.lo_x = lo[0]; b.lo_y = lo[1]; b.lo_z = lo[2];
    b.nx = hi[0] - lo[0] + 1; b.ny = hi[1] - lo[1] + 1; b.nz = hi[2] - lo[2] + 1;
    std::unique_ptr<DeviceBrick> level(new DeviceBrick);
    level->bytes = static_cast<size_t>(b.nx) * b.ny * b.nz;
    CMX_REQUIRE(level->bytes < (size_t(1) << 31), "precomputation level too large");
    CMX_HIP(hipMalloc(&level->mem, level->bytes + 16));   // (+16: aligned 8-byte reads of the last cells)
    b.cells = level->mem;
    level->desc = b;
    PrecomputeLevel3DKernel<<<DivUp(level->bytes, 256), 256, 0, ws.stream>>>(prev, b, shift,
                                                                            half ? 1 : 0);
    CMX_HIP(hipGetLastError());
    m.levels.push_back(std::move(level));
    last_width = next_width;
  }
  // Octs of every level that can be a child level (debug switch fast3d_no_oct: none, tests).
  {
    const bool build_octs = Debug().fast3d_no_oct == 0;
    const int depth = m.options.branch_and_bound_depth;
    m.oct_desc.assign(depth, OctDesc{nullptr, 0, 0, 0, 0});
    for (int i = 0; build_octs && i + 1 < depth; ++i) {
      const Brick L = m.levels[i]->desc;
      OctDesc O;
      O.s = 1 << std::min(i, m.options.full_resolution_depth - 1);
      O.qx = L.nx + O.s; O.qy = L.ny + O.s; O.qz = L.nz + O.s;
      const size_t count = static_cast<size_t>(O.qx) * O.qy * O.qz;
      if (count * sizeof(uint2) >= (size_t(1) << 32)) continue;     // 32-bit offsets elsewhere
      std::unique_ptr<DeviceBrick> mem(new DeviceBrick);
      mem->bytes = count * sizeof(uint2);
      CMX_HIP(hipMalloc(&mem->mem, mem->bytes));
      O.cells = static_cast<const uint2*>(mem->mem);
      BuildOct3DKernel<<<DivUp(count, 256), 256, 0, ws.stream>>>(
          L, O.s, static_cast<uint2*>(mem->mem), O.qx, O.qy, O.qz);
      CMX_HIP(hipGetLastError());
      m.oct_desc[i] = O;
      m.octs.push_back(std::move(mem));
    }
  }
}

}  // namespace

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
    CMX_REQUIRE(resolution > 0.f && low_resolution > 0.f, "resolutions must be > 0");
    CMX_REQUIRE(num_voxels == 0 || voxels, "voxels is null");
    CMX_REQUIRE(num_low_resolution_voxels == 0 || low_resolution_voxels, "low voxels null");
    CMX_REQUIRE(histogram_size >= 0 && (histogram_size == 0 || rotational_scan_matcher_histogram),
                "bad histogram");
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
    CMX_REQUIRE(histogram_size >= 0 && (histogram_size == 0 || rotational_scan_matcher_histogram),
                "bad histogram");
    GridPair3D source{};
    float resolution[2];
    int device[2];
    const cmx_grid3d* grids[2] = {high_resolution_grid, low_resolution_grid};
    for (int g = 0; g < 2; ++g) {
      if (!Grid3DBrick(grids[g], &source.grid[g], &resolution[g], &device[g])) source.grid[g] = Brick{};
      CMX_REQUIRE(source.grid[g].nx % 8 == 0, "internal error: resident brick not in 8-cell rows");
    }
    CMX_REQUIRE(device[0] == device[1], "the grids live on different devices (%d, %d)", device[0],
                device[1]);
    int32_t grid_size = 0;
    {
      const cmx_status status = cmx_grid3d_info(high_resolution_grid, nullptr, &grid_size, nullptr);
      CMX_REQUIRE(status == CMX_OK, "cmx_grid3d_info failed");
    }
    std::unique_ptr<cmx_fast3d> h(new cmx_fast3d);
    Fast3DMatcher& m = h->impl;
    m.options = *options;
    m.device = device[0];
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
        h_box[6 * g + k] = 0x7fffffff;
        h_box[6 * g + 3 + k] = -0x7fffffff - 1;
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
    const DeviceBrick& b = *matcher->impl.levels[depth];
    CMX_HIP(hipMemcpy(out, b.mem, b.bytes, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
