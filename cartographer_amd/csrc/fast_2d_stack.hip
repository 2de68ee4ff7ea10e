// FastCorrelativeScanMatcher2D on gfx950: the precomputation-grid stack (levels, quad layouts,
// phase planes) and the matcher object that owns it.
//
// Reference behaviour being replaced:
//   SM2/fast_correlative_scan_matcher_2d.cc:91-186   PrecomputationGrid2D / Stack
// (SM2 = cartographer/mapping/internal/2d/scan_matching).
#include <memory>
#include <vector>

#include "fast_2d_internal.h"

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
__global__ void BuildLevelKernel(const uint8_t* __restrict__ prev, int pwx, int pwy, int half,
                                 uint8_t* __restrict__ out, int wx, int wy) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  const int Y = blockIdx.y;
  if (X >= wx) return;
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
  out[X + Y * wx] = static_cast<uint8_t>(best);
}

// planes[(py*w + px) * stride + J*PI + I] = level(I*w + px, J*w + py) (0 outside).
__global__ void BuildPlanesKernel(const uint8_t* __restrict__ level, int wx, int wy, int w, int PI,
                                  int PJ, int stride, uint8_t* __restrict__ planes) {
  const int plane = blockIdx.x;             // w*w planes + 1 zero plane
  const int px = plane % w, py = plane / w;
  for (int c = threadIdx.x; c < stride; c += blockDim.x) {
    int v = 0;
    if (plane < w * w && c < PI * PJ) {
      const int I = c % PI, J = c / PI;
      const int x = I * w + px, y = J * w + py;
      if (x < wx && y < wy) v = level[x + y * wx];
    }
    planes[static_cast<size_t>(plane) * stride + c] = static_cast<uint8_t>(v);
  }
}

// out(X, Y) = max of level(X - 2 + a, Y - 2 + b), a, b in [0, 4] (cells outside the level read 0), for
// X in [0, wx + 4), Y in [0, wy + 4): the level dilated by two cells either way, stored two cells
// up so that the border's dilation has a place (the group bounds of the fused front end).
__global__ void DilateLevelKernel(const uint8_t* __restrict__ level, int wx, int wy,
                                  uint8_t* __restrict__ out) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  const int Y = blockIdx.y;
  const int ox = wx + 2 * kGroupDilation;
  if (X >= ox) return;
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
  out[X + Y * ox] = static_cast<uint8_t>(best);
}

// quads(x + w, y + w) = level(x, y) | level(x, y+w) << 8 | level(x+w, y) << 16 |
// level(x+w, y+w) << 24 for x in [-w, wx), y in [-w, wy); cells outside the level read 0.
// Tiled storage: QuadOffset (scan_matching_2d.h).
__global__ void BuildQuadsKernel(const uint8_t* __restrict__ level, int wx, int wy, int w,
                                 uint32_t* __restrict__ quads, int qx, int qy, int qtx) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  const int Y = blockIdx.y;
  if (X >= qx) return;
  const int x = X - w, y = Y - w;
  auto at = [&](int cx, int cy) -> uint32_t {
    return (static_cast<unsigned>(cx) < static_cast<unsigned>(wx) &&
            static_cast<unsigned>(cy) < static_cast<unsigned>(wy))
               ? level[cx + cy * wx] : 0u;
  };
  quads[QuadOffset(X, Y, qtx)] =
      at(x, y) | (at(x, y + w) << 8) | (at(x + w, y) << 16) | (at(x + w, y + w) << 24);
}

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
Fast2DMatcher::Fast2DMatcher(const cmx_fast2d_options& options, const cmx_grid2d_limits& limits,
                             const uint16_t* cells, int device, bool cells_on_device)
    : options_(options), limits_(limits), device_(device) {
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
    total += (static_cast<size_t>(levels_[i].wx) * levels_[i].wy + 255) & ~size_t(255);
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

Fast2DMatcher::~Fast2DMatcher() {
  (void)hipSetDevice(device_);
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
