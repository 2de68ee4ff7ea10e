// FastCorrelativeScanMatcher2D on gfx950: the precomputation-grid stack (levels, quad layouts,
// phase planes) and the matcher object that owns it.
//
// Reference behaviour being replaced:
//   SM2/fast_correlative_scan_matcher_2d.cc:91-186   PrecomputationGrid2D / Stack
// (SM2 = cartographer/mapping/internal/2d/scan_matching).
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "cmx_batch.h"
#include "fast_2d_internal.h"

struct cmx_grid2d;   // grid_2d.hip
struct cmx_tsdf2d;   // tsdf_2d.hip
namespace cmx {
const uint16_t* Grid2DDeviceCells(const cmx_grid2d* grid, cmx_grid2d_limits* limits, int* device);
void Tsdf2DDevicePlanes(const cmx_tsdf2d* grid, cmx_grid2d_limits* limits, const uint16_t** tsd,
                        const uint16_t** weight, float* max_weight, int* device);
}

namespace cmx {
namespace {

constexpr int kMaxPlaneCells = 256;    // plane_i * plane_j
constexpr int kMaxPlaneWidth = 128;    // w; plane index fits 14 bits

// ---------------------------------------------------------------------------
// Precomputation stack
// ---------------------------------------------------------------------------

// Level 0: ComputeCellValue(1 - |cost|)  (SM2/fast_...2d.cc:107-108,163-169)
// with the per-grid cost table of mapping/value_conversion_tables.cc:29-51
// evaluated arithmetically (same f32 expression the table is built from).
__device__ __forceinline__ uint8_t Level0Value(uint16_t cell, float min_cc, float max_cc) {
  const unsigned v = cell & 0x7fffu;
  float cost;
  if (v == 0) {
    cost = max_cc;
  } else {
    const float scale = (max_cc - min_cc) / 32766.f;
    cost = static_cast<float>(v) * scale + (min_cc - scale);
  }
  const float probability = 1.f - fabsf(cost);
  const float min_s = 1.f - max_cc, max_s = 1.f - min_cc;
  int value = LRoundF32((probability - min_s) * (255.f / (max_s - min_s)));
  value = min(max(value, 0), 255);
  return static_cast<uint8_t>(value);
}

__global__ void BuildLevel0Kernel(const uint16_t* __restrict__ cells, int count, float min_cc,
                                  float max_cc, uint8_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  out[i] = Level0Value(cells[i], min_cc, max_cc);
}

// The same from a grid plane resident in HBM: one pass reads the plane and writes the matcher's
// own copy of the cells (the grid may be inserted into or destroyed once the matcher exists) and
// level 0.
__global__ void CopyCellsBuildLevel0Kernel(const uint16_t* __restrict__ cells, int count,
                                           float min_cc, float max_cc,
                                           uint16_t* __restrict__ copy,
                                           uint8_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint16_t cell = cells[i];
  copy[i] = cell;
  out[i] = Level0Value(cell, min_cc, max_cc);
}

// Level w from level w/2: a w x w window is the union of four (w/2) x (w/2)
// windows.  The u8 quantisation is monotone, so max-then-quantise (reference)
// equals quantise-then-max (here).  Windows entirely outside the grid read 0,
// which never wins because at least one of the four overlaps the grid.
__device__ __forceinline__ uint8_t FourWindowMax(const uint8_t* __restrict__ prev, int pwx, int pwy,
                                                 int half, int X, int Y) {
  // (x0, y0) = (X - (w-1), Y - (w-1)); in the previous level's storage the
  // window at x0 sits at x0 + half - 1 = X - half.
  const int px0 = X - half, py0 = Y - half;
  int best = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int py = py0 + j * half;
    if (static_cast<unsigned>(py) >= static_cast<unsigned>(pwy)) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int px = px0 + i * half;
      if (static_cast<unsigned>(px) >= static_cast<unsigned>(pwx)) continue;
      best = max(best, static_cast<int>(prev[px + py * pwx]));
    }
  }
  return static_cast<uint8_t>(best);
}

__global__ void BuildLevelKernel(const uint8_t* __restrict__ prev, int pwx, int pwy, int half,
                                 uint8_t* __restrict__ out, int wx, int wy) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  const int Y = blockIdx.y;
  if (X >= wx) return;
  out[X + Y * wx] = FourWindowMax(prev, pwx, pwy, half, X, Y);
}

// planes[(py*w + px) * stride + J*PI + I] = level(I*w + px, J*w + py) (0 outside).  The plane
// layout: the cell (x, y) byte c of plane `plane` holds (w*w planes + 1 zero plane); false: none
// (the zero plane, the padding behind PI * PJ).
__device__ __forceinline__ bool PlaneCell(int w, int PI, int PJ, int plane, int c, int* x, int* y) {
  if (plane >= w * w || c >= PI * PJ) return false;
  const int px = plane % w, py = plane / w;
  const int I = c % PI, J = c / PI;
  *x = I * w + px;
  *y = J * w + py;
  return true;
}

__device__ __forceinline__ uint8_t PlaneValue(const uint8_t* __restrict__ level, int wx, int wy,
                                              int w, int PI, int PJ, int plane, int c) {
  int x, y, v = 0;
  if (PlaneCell(w, PI, PJ, plane, c, &x, &y) && x < wx && y < wy) v = level[x + y * wx];
  return static_cast<uint8_t>(v);
}

__global__ void BuildPlanesKernel(const uint8_t* __restrict__ level, int wx, int wy, int w, int PI,
                                  int PJ, int stride, uint8_t* __restrict__ planes) {
  const int plane = blockIdx.x;             // w*w planes + 1 zero plane
  for (int c = threadIdx.x; c < stride; c += blockDim.x)
    planes[static_cast<size_t>(plane) * stride + c] = PlaneValue(level, wx, wy, w, PI, PJ, plane, c);
}

// out(X, Y) = max of level(X - 2 + a, Y - 2 + b), a, b in [0, 4] (cells outside the level read 0), for
// X in [0, wx + 4), Y in [0, wy + 4): the level dilated by two cells either way, stored two cells
// up so that the border's dilation has a place (the group bounds of the fused front end).
__device__ __forceinline__ uint8_t DilatedValue(const uint8_t* __restrict__ level, int wx, int wy,
                                                int X, int Y) {
  int best = 0;
  for (int b = -kGroupDilation; b <= kGroupDilation; ++b) {
    const int y = Y - kGroupDilation + b;
    if (static_cast<unsigned>(y) >= static_cast<unsigned>(wy)) continue;
    for (int a = -kGroupDilation; a <= kGroupDilation; ++a) {
      const int x = X - kGroupDilation + a;
      if (static_cast<unsigned>(x) >= static_cast<unsigned>(wx)) continue;
      best = max(best, static_cast<int>(level[x + y * wx]));
    }
  }
  return static_cast<uint8_t>(best);
}

__global__ void DilateLevelKernel(const uint8_t* __restrict__ level, int wx, int wy,
                                  uint8_t* __restrict__ out) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  const int Y = blockIdx.y;
  const int ox = wx + 2 * kGroupDilation;
  if (X >= ox) return;
  out[X + Y * ox] = DilatedValue(level, wx, wy, X, Y);
}

// quads(x + w, y + w) = level(x, y) | level(x, y+w) << 8 | level(x+w, y) << 16 |
// level(x+w, y+w) << 24 for x in [-w, wx), y in [-w, wy); cells outside the level read 0.
// Tiled storage: QuadOffset (scan_matching_2d.h).
__device__ __forceinline__ uint32_t QuadValue(const uint8_t* __restrict__ level, int wx, int wy,
                                              int w, int X, int Y) {
  const int x = X - w, y = Y - w;
  auto at = [&](int cx, int cy) -> uint32_t {
    return (static_cast<unsigned>(cx) < static_cast<unsigned>(wx) &&
            static_cast<unsigned>(cy) < static_cast<unsigned>(wy))
               ? level[cx + cy * wx] : 0u;
  };
  return at(x, y) | (at(x, y + w) << 8) | (at(x + w, y) << 16) | (at(x + w, y + w) << 24);
}

__global__ void BuildQuadsKernel(const uint8_t* __restrict__ level, int wx, int wy, int w,
                                 uint32_t* __restrict__ quads, int qx, int qy, int qtx) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  const int Y = blockIdx.y;
  if (X >= qx) return;
  quads[QuadOffset(X, Y, qtx)] = QuadValue(level, wx, wy, w, X, Y);
}

// ---------------------------------------------------------------------------
// Batch build: the same stack for a table of submaps per launch
// ---------------------------------------------------------------------------
// Every kernel above, once more over a device table of problems.  A launch's workgroups are dealt
// to (problem, tile of 2048 consecutive cells) through a prefix table of block counts, not through
// a grid dimension over the problems with surplus blocks leaving early: the submaps of a call may
// be as unlike as 1 x 1 and 16384 x 16384 cells, and a grid sized for the largest of them times the
// number of problems would be almost all surplus.  With the table a launch has exactly the
// blocks its cells need, and a block finds its problem by a binary search over at most a chain's
// worth of entries, on values that are uniform over the block.  Indices inside a problem are int
// (16384 + 2^11 squared fits); across problems only pointers and block numbers are used.
constexpr int kStackThreads = 256;
// Cells per workgroup: eight per thread, so that finding the block's problem (a dozen dependent
// loads) is paid once per 2048 cells, not once per 256.
constexpr int kStackTile = 8 * kStackThreads;

struct StackLevel {
  uint8_t* cells;
  uint32_t* quads;          // (or null: the top level)
  int wx, wy;
  int qx, qy, qtx;
};

struct StackProblem {
  const uint16_t* source;   // the grid: in the chain's staging block, or the resident plane
  uint16_t* copy;           // the matcher's own copy of it
  StackLevel level[kMaxDepth];
  uint8_t* planes;          // (or null)
  uint8_t* planes_group;    // (or null)
  int count;                // nx * ny
  int w;                    // width of the top level: 2^(depth - 1)
  int plane_i, plane_j, plane_stride;
  float min_cc, max_cc;
};

// first[e] = first block of entry e of a launch, first[num] = its blocks: EntryOfBlock (cmx_batch.h).
__global__ void BatchLevel0Kernel(const StackProblem* __restrict__ problems,
                                  const int* __restrict__ first, int num) {
  const int p = EntryOfBlock(first, num, blockIdx.x);
  const StackProblem& P = problems[p];
  const int base = (blockIdx.x - first[p]) * kStackTile;
  const int end = min(base + kStackTile, P.count);
  for (int i = base + threadIdx.x; i < end; i += kStackThreads) {
    const uint16_t cell = P.source[i];
    P.copy[i] = cell;
    P.level[0].cells[i] = Level0Value(cell, P.min_cc, P.max_cc);
  }
}

__global__ void BatchLevelKernel(const StackProblem* __restrict__ problems,
                                 const int* __restrict__ first, int num, int l) {
  const int p = EntryOfBlock(first, num, blockIdx.x);
  const StackLevel& prev = problems[p].level[l - 1];
  const StackLevel& cur = problems[p].level[l];
  const int base = (blockIdx.x - first[p]) * kStackTile;
  const int end = min(base + kStackTile, cur.wx * cur.wy);
  for (int i = base + threadIdx.x; i < end; i += kStackThreads)
    cur.cells[i] =
        FourWindowMax(prev.cells, prev.wx, prev.wy, 1 << (l - 1), i % cur.wx, i / cur.wx);
}

// Dwords of a level's quad storage: whole tiles of 8 x 4.
__host__ __device__ inline int QuadSlots(int qy, int qtx) { return qtx * ((qy + 3) / 4) * 32; }

// Entry e = problem e / child_levels, level e % child_levels: the quad layouts of every level
// that can be a child level, of every problem, in one launch (they read finished levels only).
// A thread takes the element whose place in the tiled storage is its index -- 32 lanes fill one
// tile, a 128-byte line, where 64 cells of a row would touch eight lines a quarter each; the
// slots of a border tile outside the array stay unwritten, as the row-wise kernel leaves them.
__global__ void BatchQuadsKernel(const StackProblem* __restrict__ problems,
                                 const int* __restrict__ first, int num_entries,
                                 int child_levels) {
  const int e = EntryOfBlock(first, num_entries, blockIdx.x);
  const int l = e % child_levels;
  const StackLevel& L = problems[e / child_levels].level[l];
  const int base = (blockIdx.x - first[e]) * kStackTile;
  const int end = min(base + kStackTile, QuadSlots(L.qy, L.qtx));
  for (int i = base + threadIdx.x; i < end; i += kStackThreads) {
    const int tile = i >> 5;
    const int X = (tile % L.qtx) * 8 + (i & 7), Y = (tile / L.qtx) * 4 + ((i >> 3) & 3);
    if (X >= L.qx || Y >= L.qy) continue;
    // (QuadOffset(X, Y, qtx) == i: the layout stays written down in one place)
    L.quads[QuadOffset(X, Y, L.qtx)] = QuadValue(L.cells, L.wx, L.wy, 1 << l, X, Y);
  }
}

// The phase planes of the top level and, where the problem has them, those of its dilation,
// read straight from the level (25 cells per byte of at most w*w + 1 planes of 64 bytes: no
// dilated image, so no scratch that grows with the number of problems).
__global__ void BatchPlanesKernel(const StackProblem* __restrict__ problems,
                                  const int* __restrict__ first, int num, int top) {
  const int p = EntryOfBlock(first, num, blockIdx.x);
  const StackProblem& P = problems[p];
  const StackLevel& L = P.level[top];
  const int base = (blockIdx.x - first[p]) * kStackTile;
  const int end = min(base + kStackTile, (P.w * P.w + 1) * P.plane_stride);
  for (int i = base + threadIdx.x; i < end; i += kStackThreads) {
    const int plane = i / P.plane_stride, c = i % P.plane_stride;
    P.planes[i] = PlaneValue(L.cells, L.wx, L.wy, P.w, P.plane_i, P.plane_j, plane, c);
    if (P.planes_group == nullptr) continue;
    int x, y, v = 0;
    if (PlaneCell(P.w, P.plane_i, P.plane_j, plane, c, &x, &y) &&
        x < L.wx + 2 * kGroupDilation && y < L.wy + 2 * kGroupDilation)
      v = DilatedValue(L.cells, L.wx, L.wy, x, y);
    P.planes_group[i] = static_cast<uint8_t>(v);
  }
}

// What one chain of launches takes: host cells staged (pinned and device scratch of the call's
// workspace), blocks over all its launches (far inside a grid's 2^31 - 1), table entries.
constexpr size_t kChainStagingBytes = size_t(32) << 20;
constexpr long long kChainBlocks = 1ll << 30;
constexpr int kChainMatchers = 8192;

}  // namespace

// The phase planes of the lowest-resolution level a matcher of this grid builds: PI x PJ lattice
// cells per plane where the level is narrow enough for them, and the planes of the level dilated
// by two cells (group bounds of the fused front end) where the dilated image still fits that
// lattice.  Host arithmetic only: the constructor below and the front end's planner share it.
PlanMatcher PlanMatcherOf(const cmx_fast2d_options& options, const cmx_grid2d_limits& limits) {
  PlanMatcher pm{};
  pm.limits = limits;
  pm.linear_search_window = options.linear_search_window;
  pm.angular_search_window = options.angular_search_window;
  pm.depth = options.branch_and_bound_depth;
  const int depth = pm.depth;
  const int w = 1 << (depth - 1);
  const int wx = limits.num_x_cells + w - 1, wy = limits.num_y_cells + w - 1;   // the top level
  const int PI = (wx + w - 1) / w, PJ = (wy + w - 1) / w;
  if (w <= kMaxPlaneWidth && PI * PJ <= kMaxPlaneCells) {
    pm.planes = true;
    pm.plane_i = PI;
    pm.plane_j = PJ;
    pm.plane_stride = (PI * PJ + 63) & ~63;
    const int dwx = wx + 2 * kGroupDilation, dwy = wy + 2 * kGroupDilation;
    pm.planes_group = pm.plane_stride == 64 && depth > 1 && dwx <= PI * w && dwy <= PJ * w;
  }
  return pm;
}

PlanMatcher PlanMatcherOf(const Fast2DMatcher& m) {
  PlanMatcher pm = PlanMatcherOf(m.options(), m.limits());
  // (what the matcher holds is what counts: an allocation that failed would have thrown)
  pm.planes = m.planes() != nullptr;
  pm.planes_group = m.planes_group() != nullptr;
  pm.plane_i = m.plane_i();
  pm.plane_j = m.plane_j();
  pm.plane_stride = m.plane_stride();
  return pm;
}

// ---------------------------------------------------------------------------
// Fast2DMatcher (host)
// ---------------------------------------------------------------------------
void Fast2DMatcher::CheckArguments(const cmx_fast2d_options& options,
                                   const cmx_grid2d_limits& limits, const uint16_t* cells) {
  // CHECKs of the reference: SM2/fast_...2d.cc:100-102,174; map_limits.h:45-47;
  // grid_2d.cc:73.
  CMX_REQUIRE(cells != nullptr, "cells is null");
  CMX_REQUIRE(options.branch_and_bound_depth >= 1 && options.branch_and_bound_depth <= kMaxDepth,
              "branch_and_bound_depth %d outside [1,%d]", options.branch_and_bound_depth,
              kMaxDepth);
  CMX_REQUIRE(limits.resolution > 0., "resolution must be > 0");
  CMX_REQUIRE(limits.num_x_cells >= 1 && limits.num_y_cells >= 1, "empty cell limits");
  CMX_REQUIRE(limits.num_x_cells <= 16384 && limits.num_y_cells <= 16384,
              "grid larger than 16384 cells per side is unsupported");
  CMX_REQUIRE(limits.min_correspondence_cost < limits.max_correspondence_cost,
              "min_correspondence_cost must be < max_correspondence_cost");
  // The search orders scores by their f32 bit patterns and marks "no candidate" with a negative
  // value: both need every score, 1 - max_correspondence_cost at the least, to be >= 0.
  CMX_REQUIRE(limits.max_correspondence_cost <= 1.f,
              "max_correspondence_cost %g > 1 is unsupported: scores down to %g would be "
              "negative, which the search cannot represent",
              static_cast<double>(limits.max_correspondence_cost),
              1. - static_cast<double>(limits.max_correspondence_cost));
}

Fast2DMatcher::Fast2DMatcher(const cmx_fast2d_options& options, const cmx_grid2d_limits& limits,
                             const uint16_t* cells, int device, bool cells_on_device)
    : options_(options), limits_(limits), device_(device) {
  CheckArguments(options, limits, cells);
  WorkspaceLease ws(device);
  const int nx = limits.num_x_cells, ny = limits.num_y_cells;
  const int depth = options.branch_and_bound_depth;
  size_t total = 0;
  level_offsets_.resize(depth);
  levels_.resize(depth);
  for (int i = 0; i < depth; ++i) {
    const int w = 1 << i;
    level_offsets_[i] = total;
    levels_[i].wx = nx + w - 1;
    levels_[i].wy = ny + w - 1;
    total += Align256(static_cast<size_t>(levels_[i].wx) * levels_[i].wy);
  }
  CMX_HIP(hipMalloc(&stack_mem_, total));
  for (int i = 0; i < depth; ++i)
    levels_[i].cells = static_cast<uint8_t*>(stack_mem_) + level_offsets_[i];
  min_s_ = 1.f - limits.max_correspondence_cost;
  const float max_s = 1.f - limits.min_correspondence_cost;
  score_scale_ = (max_s - min_s_) / 255.f;

  const size_t count = static_cast<size_t>(nx) * ny;
  CMX_HIP(hipMalloc(reinterpret_cast<void**>(&grid_cells_), count * sizeof(uint16_t)));
  if (cells_on_device) {
    CopyCellsBuildLevel0Kernel<<<DivUp(count, 256), 256, 0, ws->stream>>>(
        cells, static_cast<int>(count), limits.min_correspondence_cost,
        limits.max_correspondence_cost, grid_cells_, const_cast<uint8_t*>(levels_[0].cells));
  } else {
    CMX_HIP(hipMemcpyAsync(grid_cells_, cells, count * sizeof(uint16_t), hipMemcpyHostToDevice,
                           ws->stream));
    BuildLevel0Kernel<<<DivUp(count, 256), 256, 0, ws->stream>>>(
        grid_cells_, static_cast<int>(count), limits.min_correspondence_cost,
        limits.max_correspondence_cost, const_cast<uint8_t*>(levels_[0].cells));
  }
  for (int i = 1; i < depth; ++i) {
    const LevelDesc& prev = levels_[i - 1];
    const LevelDesc& cur = levels_[i];
    BuildLevelKernel<<<dim3(DivUp(cur.wx, 256), cur.wy), 256, 0, ws->stream>>>(
        prev.cells, prev.wx, prev.wy, 1 << (i - 1), const_cast<uint8_t*>(cur.cells), cur.wx,
        cur.wy);
  }
  // Quad layouts of every level that can be a child level (0 .. depth-2).
  {
    size_t quad_total = 0;
    std::vector<size_t> quad_off(depth, 0);
    for (int i = 0; i + 1 < depth; ++i) {
      const int w = 1 << i;
      levels_[i].qx = levels_[i].wx + w;
      levels_[i].qy = levels_[i].wy + w;
      levels_[i].qtx = (levels_[i].qx + 7) / 8;
      quad_off[i] = quad_total;
      // whole tiles of 32 dwords (128 bytes)
      quad_total += static_cast<size_t>(levels_[i].qtx) * ((levels_[i].qy + 3) / 4) * 128;
    }
    levels_[depth - 1].quads = nullptr;
    levels_[depth - 1].qx = levels_[depth - 1].qy = levels_[depth - 1].qtx = 0;
    if (quad_total) {
      CMX_HIP(hipMalloc(&quads_mem_, quad_total));
      for (int i = 0; i + 1 < depth; ++i) {
        LevelDesc& L = levels_[i];
        uint32_t* q = reinterpret_cast<uint32_t*>(static_cast<char*>(quads_mem_) + quad_off[i]);
        L.quads = q;
        BuildQuadsKernel<<<dim3(DivUp(L.qx, 256), L.qy), 256, 0, ws->stream>>>(
            L.cells, L.wx, L.wy, 1 << i, q, L.qx, L.qy, L.qtx);
      }
    }
  }
  // Phase planes of the lowest-resolution level.
  {
    const int w = 1 << (depth - 1);
    const LevelDesc& top = levels_[depth - 1];
    const PlanMatcher layout = PlanMatcherOf(options, limits);
    if (layout.planes) {
      const int PI = layout.plane_i, PJ = layout.plane_j;
      plane_i_ = PI;
      plane_j_ = PJ;
      plane_stride_ = layout.plane_stride;
      const size_t bytes = static_cast<size_t>(w * w + 1) * plane_stride_;
      CMX_HIP(hipMalloc(reinterpret_cast<void**>(&planes_), bytes));
      BuildPlanesKernel<<<w * w + 1, 64, 0, ws->stream>>>(top.cells, top.wx, top.wy, w, PI, PJ,
                                                          plane_stride_, planes_);
      // The same planes of the level dilated by two cells (group bounds of the fused front end),
      // where the dilated image still fits the planes' PI x PJ lattice cells.
      const int dwx = top.wx + 2 * kGroupDilation, dwy = top.wy + 2 * kGroupDilation;
      if (layout.planes_group) {
        uint8_t* dilated = ws->dev[0].ReserveAs<uint8_t>(static_cast<size_t>(dwx) * dwy);
        DilateLevelKernel<<<dim3(DivUp(dwx, 256), dwy), 256, 0, ws->stream>>>(top.cells, top.wx,
                                                                             top.wy, dilated);
        CMX_HIP(hipMalloc(reinterpret_cast<void**>(&planes_group_), bytes));
        BuildPlanesKernel<<<w * w + 1, 64, 0, ws->stream>>>(dilated, dwx, dwy, w, PI, PJ,
                                                            plane_stride_, planes_group_);
      }
    }
  }
  CMX_HIP(hipGetLastError());
  CMX_HIP(hipStreamSynchronize(ws->stream));
}

// ---- batch build (host)
// The geometry the constructor above computes, with every region laid out in one allocation:
// [levels | quad layouts | planes | group planes | cells], each from a 256-byte boundary.
Fast2DMatcher::Fast2DMatcher(BatchTag, const cmx_fast2d_options& options,
                             const cmx_grid2d_limits& limits, int device)
    : options_(options), limits_(limits), device_(device) {
  const int nx = limits.num_x_cells, ny = limits.num_y_cells;
  const int depth = options.branch_and_bound_depth;
  size_t total = 0;
  level_offsets_.resize(depth);
  levels_.resize(depth);
  for (int i = 0; i < depth; ++i) {
    const int w = 1 << i;
    level_offsets_[i] = total;
    levels_[i].wx = nx + w - 1;
    levels_[i].wy = ny + w - 1;
    total += Align256(static_cast<size_t>(levels_[i].wx) * levels_[i].wy);
  }
  min_s_ = 1.f - limits.max_correspondence_cost;
  const float max_s = 1.f - limits.min_correspondence_cost;
  score_scale_ = (max_s - min_s_) / 255.f;
  const size_t quads_at = total;
  std::vector<size_t> quad_off(depth, 0);
  for (int i = 0; i + 1 < depth; ++i) {
    const int w = 1 << i;
    levels_[i].qx = levels_[i].wx + w;
    levels_[i].qy = levels_[i].wy + w;
    levels_[i].qtx = (levels_[i].qx + 7) / 8;
    quad_off[i] = total;
    // whole tiles of 32 dwords (128 bytes)
    total += static_cast<size_t>(levels_[i].qtx) * ((levels_[i].qy + 3) / 4) * 128;
  }
  levels_[depth - 1].quads = nullptr;
  levels_[depth - 1].qx = levels_[depth - 1].qy = levels_[depth - 1].qtx = 0;
  const bool any_quads = total != quads_at;
  total = Align256(total);
  const PlanMatcher layout = PlanMatcherOf(options, limits);
  size_t planes_at = 0, planes_group_at = 0;
  if (layout.planes) {
    const int w = 1 << (depth - 1);
    plane_i_ = layout.plane_i;
    plane_j_ = layout.plane_j;
    plane_stride_ = layout.plane_stride;
    const size_t bytes = Align256(static_cast<size_t>(w * w + 1) * plane_stride_);
    planes_at = total;
    total += bytes;
    if (layout.planes_group) {
      planes_group_at = total;
      total += bytes;
    }
  }
  const size_t cells_at = total;
  total += static_cast<size_t>(nx) * ny * sizeof(uint16_t);
  CMX_HIP(hipMalloc(&slab_, total));
  char* base = static_cast<char*>(slab_);
  stack_mem_ = base;
  for (int i = 0; i < depth; ++i) {
    levels_[i].cells = reinterpret_cast<uint8_t*>(base + level_offsets_[i]);
    if (i + 1 < depth) levels_[i].quads = reinterpret_cast<uint32_t*>(base + quad_off[i]);
  }
  if (any_quads) quads_mem_ = base + quads_at;
  if (layout.planes) planes_ = reinterpret_cast<uint8_t*>(base + planes_at);
  if (layout.planes_group) planes_group_ = reinterpret_cast<uint8_t*>(base + planes_group_at);
  grid_cells_ = reinterpret_cast<uint16_t*>(base + cells_at);
}

namespace {

// Blocks over all launches of a chain that one matcher adds (the bound of kChainBlocks).
long long ChainBlocksOf(const Fast2DMatcher& m) {
  long long blocks = BlocksOf(static_cast<long long>(m.limits().num_x_cells) *
                              m.limits().num_y_cells, kStackTile);
  for (int i = 0; i < m.depth(); ++i) {
    const LevelDesc& L = m.level(i);
    if (i > 0) blocks += BlocksOf(static_cast<long long>(L.wx) * L.wy, kStackTile);
    blocks += BlocksOf(QuadSlots(L.qy, L.qtx), kStackTile);
  }
  if (m.planes())
    blocks += BlocksOf((static_cast<long long>(1) << (2 * (m.depth() - 1))) * m.plane_stride() +
                       m.plane_stride(), kStackTile);
  return blocks;
}

}  // namespace

std::vector<std::unique_ptr<Fast2DMatcher>> Fast2DMatcher::BuildBatch(
    const cmx_fast2d_options& options, const Fast2DSource* sources, int num, int device) {
  using Clock = std::chrono::steady_clock;
  const bool host_trace = Debug().host_trace != 0;
  auto since = [](Clock::time_point t) {
    return std::chrono::duration<double, std::micro>(Clock::now() - t).count();
  };
  WorkspaceLease ws(device);
  const int depth = options.branch_and_bound_depth;
  const int child_levels = depth - 1;
  Clock::time_point lap = Clock::now();
  // Every allocation first: one that fails leaves nothing built and nothing in flight (the
  // vector frees what exists).
  std::vector<std::unique_ptr<Fast2DMatcher>> matchers(num);
  for (int k = 0; k < num; ++k)
    matchers[k].reset(new Fast2DMatcher(BatchTag{}, options, sources[k].limits, device));
  const double alloc_us = since(lap);

  const int most = Debug().fast2d_create_chain > 0 ? Debug().fast2d_create_chain : kChainMatchers;
  // The chains; total[0]: bytes of host cells staged, every grid from a 256-byte boundary.
  const std::vector<LaunchSet> chains = CutSets(
      std::vector<int>(num, 0), most, {kChainStagingBytes, kChainBlocks, 0},
      [&](int k, long long* add) {
        add[0] = sources[k].cells_on_device ? 0 : Align256(
            static_cast<size_t>(sources[k].limits.num_x_cells) * sources[k].limits.num_y_cells *
            sizeof(uint16_t));
        add[1] = ChainBlocksOf(*matchers[k]);
      },
      [](int, int, const long long*) {});

  double stage_us = 0., issue_us = 0., wait_us = 0.;
  int launches = 0;
  for (const LaunchSet& chain : chains) {
    lap = Clock::now();
    const int n = chain.end - chain.begin;
    // The upload block: problems, the prefix tables of the launches, the host grids.
    //   tables: level 0 | levels 1 .. depth-1 | quads (n * child_levels entries) | planes
    const size_t table_ints = static_cast<size_t>(depth) * (n + 1) +
                              (static_cast<size_t>(n) * child_levels + 1) + (n + 1);
    BlockLayout block;
    const auto problems_in = block.Add<StackProblem>(n);
    const auto tables_in = block.Add<int>(table_ints);
    const auto cells_in = block.Add<char>(chain.total[0]);
    char* h_block = static_cast<char*>(ws->pinned[0].Reserve(block.bytes));
    char* d_block = static_cast<char*>(ws->dev[0].Reserve(block.bytes));
    StackProblem* h_problems = problems_in(h_block);
    const StackProblem* d_problems = problems_in(d_block);
    int* first_level = tables_in(h_block);                         // [depth][n + 1]
    int* first_quads = first_level + static_cast<size_t>(depth) * (n + 1);
    int* first_planes = first_quads + static_cast<size_t>(n) * child_levels + 1;
    std::vector<size_t> staged_at(n, 0);
    long long planes_blocks = 0, quads_blocks = 0;
    std::vector<long long> level_blocks(depth, 0);
    size_t cursor = cells_in.at;
    for (int j = 0; j < n; ++j) {
      const Fast2DMatcher& m = *matchers[chain.begin + j];
      const Fast2DSource& src = sources[chain.begin + j];
      StackProblem P{};
      P.count = m.limits_.num_x_cells * m.limits_.num_y_cells;
      if (src.cells_on_device) {
        P.source = src.cells;
      } else {
        staged_at[j] = cursor;
        P.source = reinterpret_cast<const uint16_t*>(d_block + cursor);
        cursor += Align256(static_cast<size_t>(P.count) * sizeof(uint16_t));
      }
      P.copy = m.grid_cells_;
      for (int i = 0; i < depth; ++i) {
        const LevelDesc& L = m.levels_[i];
        P.level[i] = StackLevel{const_cast<uint8_t*>(L.cells), const_cast<uint32_t*>(L.quads),
                                L.wx, L.wy, L.qx, L.qy, L.qtx};
        first_level[static_cast<size_t>(i) * (n + 1) + j] = static_cast<int>(level_blocks[i]);
        level_blocks[i] += BlocksOf(static_cast<long long>(L.wx) * L.wy, kStackTile);
        if (i < child_levels) {
          first_quads[static_cast<size_t>(j) * child_levels + i] = static_cast<int>(quads_blocks);
          quads_blocks += BlocksOf(QuadSlots(L.qy, L.qtx), kStackTile);
        }
      }
      P.planes = m.planes_;
      P.planes_group = m.planes_group_;
      P.w = 1 << (depth - 1);
      P.plane_i = m.plane_i_;
      P.plane_j = m.plane_j_;
      P.plane_stride = m.plane_stride_;
      P.min_cc = m.limits_.min_correspondence_cost;
      P.max_cc = m.limits_.max_correspondence_cost;
      first_planes[j] = static_cast<int>(planes_blocks);
      if (m.planes_)
        planes_blocks +=
            BlocksOf(static_cast<long long>(P.w * P.w + 1) * P.plane_stride, kStackTile);
      h_problems[j] = P;
    }
    for (int i = 0; i < depth; ++i)
      first_level[static_cast<size_t>(i) * (n + 1) + n] = static_cast<int>(level_blocks[i]);
    first_quads[static_cast<size_t>(n) * child_levels] = static_cast<int>(quads_blocks);
    first_planes[n] = static_cast<int>(planes_blocks);
    // Host grids into the one staging block (the pool's threads: a copy is memory bound).
    ParallelFor(n, 2, [&](int j) {
      const Fast2DSource& src = sources[chain.begin + j];
      if (src.cells_on_device) return;
      memcpy(h_block + staged_at[j], src.cells,
             static_cast<size_t>(src.limits.num_x_cells) * src.limits.num_y_cells *
                 sizeof(uint16_t));
    });
    stage_us += since(lap);
    lap = Clock::now();

    hipStream_t stream = ws->stream;
    SmallCopyAsync(d_block, h_block, block.bytes, /*to_device=*/true, stream);
    ++launches;
    const int* d_first_level = tables_in(d_block);
    const int* d_first_quads = d_first_level + static_cast<size_t>(depth) * (n + 1);
    const int* d_first_planes = d_first_quads + static_cast<size_t>(n) * child_levels + 1;
    BatchLevel0Kernel<<<static_cast<unsigned>(level_blocks[0]), kStackThreads, 0, stream>>>(
        d_problems, d_first_level, n);
    ++launches;
    for (int i = 1; i < depth; ++i) {
      BatchLevelKernel<<<static_cast<unsigned>(level_blocks[i]), kStackThreads, 0, stream>>>(
          d_problems, d_first_level + static_cast<size_t>(i) * (n + 1), n, i);
      ++launches;
    }
    if (quads_blocks > 0) {
      BatchQuadsKernel<<<static_cast<unsigned>(quads_blocks), kStackThreads, 0, stream>>>(
          d_problems, d_first_quads, n * child_levels, child_levels);
      ++launches;
    }
    if (planes_blocks > 0) {
      BatchPlanesKernel<<<static_cast<unsigned>(planes_blocks), kStackThreads, 0, stream>>>(
          d_problems, d_first_planes, n, depth - 1);
      ++launches;
    }
    CMX_HIP(hipGetLastError());
    issue_us += since(lap);
    lap = Clock::now();
    // (the next chain reuses the staging block)
    CMX_HIP(hipStreamSynchronize(stream));
    wait_us += since(lap);
  }
  if (host_trace)
    fprintf(stderr,
            "[cmx host] fast2d_create_batch matchers=%d chains=%d launches=%d alloc=%.0f "
            "stage=%.0f issue=%.0f wait=%.0f\n",
            num, static_cast<int>(chains.size()), launches, alloc_us, stage_us, issue_us, wait_us);
  return matchers;
}

Fast2DMatcher::~Fast2DMatcher() {
  (void)hipSetDevice(device_);
  if (slab_) {                 // (BuildBatch: every region lies in it)
    (void)hipFree(slab_);
    return;
  }
  if (stack_mem_) (void)hipFree(stack_mem_);
  if (quads_mem_) (void)hipFree(quads_mem_);
  if (planes_) (void)hipFree(planes_);
  if (planes_group_) (void)hipFree(planes_group_);
  if (grid_cells_) (void)hipFree(grid_cells_);
}

// The matcher of a grid plane that lies in HBM on `device` (grid_2d.hip, tsdf_2d.hip): built
// where the plane lies; the matcher keeps a copy of its own.
cmx_fast2d* CreateFast2DFromDeviceCells(const cmx_fast2d_options& options,
                                        const cmx_grid2d_limits& limits,
                                        const uint16_t* device_cells, int device) {
  std::unique_ptr<cmx_fast2d> h(new cmx_fast2d);
  h->impl.reset(new Fast2DMatcher(options, limits, device_cells, device, /*cells_on_device=*/true));
  return h.release();
}

}  // namespace cmx

using cmx::Guard;

extern "C" {

cmx_status cmx_fast2d_create(const cmx_fast2d_options* options, const cmx_grid2d_limits* limits,
                             const uint16_t* cells, int32_t device, cmx_fast2d** out) {
  return Guard([&] {
    CMX_REQUIRE(options && limits && out, "null argument");
    *out = nullptr;
    std::unique_ptr<cmx_fast2d> h(new cmx_fast2d);
    h->impl.reset(new cmx::Fast2DMatcher(*options, *limits, cells, device));
    *out = h.release();
  });
}

cmx_status cmx_fast2d_create_batch(const cmx_fast2d_options* options,
                                   const cmx_fast2d_source* sources, int32_t num_sources,
                                   int32_t device, cmx_fast2d** out) {
  return Guard([&] {
    for (int k = 0; out && k < num_sources; ++k) out[k] = nullptr;
    CMX_REQUIRE(options && sources && out, "null argument");
    CMX_REQUIRE(num_sources >= 1, "num_sources %d < 1", num_sources);
    // Every check of the single creates, for every source, before the device is touched.
    std::vector<cmx::Fast2DSource> list(num_sources);
    for (int k = 0; k < num_sources; ++k) {
      const cmx_fast2d_source& s = sources[k];
      const int kinds = ((s.limits || s.cells) ? 1 : 0) + (s.grid ? 1 : 0) + (s.tsdf ? 1 : 0);
      CMX_REQUIRE(kinds == 1, "source %d: %s", k,
                  kinds == 0 ? "no kind set (limits and cells, grid or tsdf)"
                             : "more than one kind set (limits and cells, grid or tsdf)");
      cmx::Fast2DSource& item = list[k];
      int resident_on = device;
      if (s.grid) {
        item.cells = cmx::Grid2DDeviceCells(s.grid, &item.limits, &resident_on);
        item.cells_on_device = true;
      } else if (s.tsdf) {
        const uint16_t* weight;
        float max_weight;
        cmx::Tsdf2DDevicePlanes(s.tsdf, &item.limits, &item.cells, &weight, &max_weight,
                                &resident_on);
        item.cells_on_device = true;
      } else {
        CMX_REQUIRE(s.limits != nullptr, "source %d: null argument", k);
        item.limits = *s.limits;
        item.cells = s.cells;
        item.cells_on_device = false;
      }
      CMX_REQUIRE(resident_on == device, "source %d: resident on device %d, the call builds on %d",
                  k, resident_on, device);
      try {
        cmx::Fast2DMatcher::CheckArguments(*options, item.limits, item.cells);
      } catch (const cmx::HipError&) {
        const std::string what = cmx::LastError();
        CMX_REQUIRE(false, "source %d: %s", k, what.c_str());
      }
    }
    std::vector<std::unique_ptr<cmx::Fast2DMatcher>> built =
        cmx::Fast2DMatcher::BuildBatch(*options, list.data(), num_sources, device);
    std::vector<std::unique_ptr<cmx_fast2d>> handles(num_sources);
    for (int k = 0; k < num_sources; ++k) {
      handles[k].reset(new cmx_fast2d);
      handles[k]->impl = std::move(built[k]);
    }
    for (int k = 0; k < num_sources; ++k) out[k] = handles[k].release();
  });
}

void cmx_fast2d_destroy(cmx_fast2d* matcher) { delete matcher; }

cmx_status cmx_fast2d_level_dims(const cmx_fast2d* matcher, int32_t level, int32_t* wide_x,
                                 int32_t* wide_y) {
  return Guard([&] {
    CMX_REQUIRE(matcher && matcher->impl && wide_x && wide_y, "null argument");
    CMX_REQUIRE(level >= 0 && level < matcher->impl->depth(), "level out of range");
    *wide_x = matcher->impl->level(level).wx;
    *wide_y = matcher->impl->level(level).wy;
  });
}

cmx_status cmx_fast2d_level_cells(const cmx_fast2d* matcher, int32_t level, uint8_t* out) {
  return Guard([&] {
    CMX_REQUIRE(matcher && matcher->impl && out, "null argument");
    CMX_REQUIRE(level >= 0 && level < matcher->impl->depth(), "level out of range");
    cmx::UseDevice(matcher->impl->device());
    const cmx::LevelDesc& L = matcher->impl->level(level);
    CMX_HIP(hipMemcpy(out, L.cells, static_cast<size_t>(L.wx) * L.wy, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
