// cmx_grid2d_insert_batch: ProbabilityGridRangeDataInserter2D::Insert + FinishUpdate for many
// (grid, scan) pairs in one call -- the two insertions of ActiveSubmaps2D::InsertRangeData
// (mapping/2d/submap_2d.cc:161-174), or those of many robots after one
// cmx_rt2d_match_grid_batch -- bit for bit the single calls of grid_2d.hip in list order.
//
// Rounds.  Round r holds the r-th insertion of every grid, so that no grid appears twice in a
// round; a round is three launches over all its insertions (hits, rays, marker clearing) and the
// rounds follow each other on the stream.  "First writer wins" inside a phase is what makes the
// single kernels exact (grid_2d.hip); insertions into different grids touch different cells and
// insertions into one grid are separated by launches, so batching adds no race.
//
// Growth.  GrowAsNeeded depends on the points only, which the host has: the plan replays the
// single call's GrowLimits loops insertion by insertion with the evolving limits, and every grid
// is grown ONCE, before the first round, to the size its last insertion needs (one launch for all
// grids that grow, no synchronisation).  Cell indices are NOT computed from the final limits:
// (max - p) / fine_resolution - 0.5 with another `max` may round differently at a sub-pixel
// boundary.  An insertion's descriptor carries the limits the grid has at that insertion -- they
// serve FineIndex and the Contains check behind the error flag exactly as in the single kernels --
// and a `cells` pointer to the view's cell (0, 0) inside the final storage with the final row
// stride: the view of an earlier insertion is a window of the final grid, whole cells apart.
//
// Blocks.  A workgroup never spans two insertions: every descriptor holds the first block it has
// in each of its set's three launches, and a block finds its insertion by bisection over them.
// Hits: 256 points per block; rays: 4 per block, one wavefront each (ForEachRayPixel); marker
// clearing sweeps the cell box of the insertion's own points padded by a cell -- every cell a
// hit or a ray marks lies inside the box of the origin's and the end points' cells, which the plan
// has from the growth step -- and so never more than the whole grid, which the single call sweeps.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/cartographer_mi355x_debug.h"
#include "cmx_batch.h"
#include "grid_2d_internal.h"
#include "grid_grow_batch.h"

namespace cmx {
namespace {

constexpr uint16_t kUpdateMarker = 1u << 15;
constexpr int kHitPoints = 256;            // points per block of the hit launch
constexpr int kRaysPerBlock = 4;           // one wavefront per ray
constexpr int kClearCells = 1024;          // cells per block of the clearing launch
constexpr int kChainInsertions = 4096;     // insertions per set of launches (grid2d_insert_chain)
constexpr long long kSetBlocks = 1ll << 24;  // blocks of any one launch of a set

// ---- plan (host only) ------------------------------------------------------------------
struct PlanLimits {
  double resolution, max_x, max_y;
  int nx, ny;
};

struct PlanInput {
  int grid;
  const float* origin;
  const float* returns;
  int num_returns;
  const float* misses;
  int num_misses;
};

struct PlannedInsertion {
  PlanLimits at{};            // the grid's limits at this insertion, after its own growth
  int start_x = 0, start_y = 0;  // where cell (0, 0) of the grid before the call lies in `at`
  int box_x = 0, box_y = 0, box_w = 0, box_h = 0;  // cells the insertion can mark, in `at`
};

struct PlannedGrid {
  PlanLimits limits{};        // in: before the call; out: after it
  int start_x = 0, start_y = 0;  // where cell (0, 0) of the grid before the call lies at the end
  int doublings = 0, insertions = 0;
};

// Contains / GrowLimits of grid_2d.hip on plain limits: the same expressions in the same order.
bool PlanContains(const PlanLimits& g, float px, float py) {
  const long ix = std::lround((g.max_y - py) / g.resolution - 0.5);
  const long iy = std::lround((g.max_x - px) / g.resolution - 0.5);
  return ix >= 0 && ix < g.nx && iy >= 0 && iy < g.ny;
}

void PlanGrow(PlannedGrid* grid, float px, float py, int index) {
  PlanLimits* g = &grid->limits;
  while (!PlanContains(*g, px, py)) {
    CMX_REQUIRE(static_cast<long long>(g->nx) * g->ny < (1ll << 28),
                "insertion %d: grid grows beyond 2^30 cells", index);
    const int x_offset = g->nx / 2, y_offset = g->ny / 2;
    g->max_x += g->resolution * y_offset;
    g->max_y += g->resolution * x_offset;
    g->nx *= 2;
    g->ny *= 2;
    grid->start_x += x_offset;
    grid->start_y += y_offset;
    ++grid->doublings;
  }
}

// The cell FineIndex(...) / kSubpixelScale of the kernels gives a coordinate.
long PlanCell(double max, float p, double resolution) {
  return std::lround((max - static_cast<double>(p)) / (resolution / kSubpixelScale) - 0.5) /
         kSubpixelScale;
}

// Limits and boxes of a call.  `grids` in: the limits before the call.
void PlanInsertions(std::vector<PlannedGrid>* grids, const PlanInput* in, int num,
                    std::vector<PlannedInsertion>* out) {
  out->assign(num, PlannedInsertion{});
  // GrowAsNeeded (:35-50): bounding box of origin, returns and misses.
  struct Box { float lo_x, hi_x, lo_y, hi_y; };
  std::vector<Box> boxes(num);
  ParallelFor(num, 16, [&](int k) {
    const PlanInput& I = in[k];
    Box b{I.origin[0], I.origin[0], I.origin[1], I.origin[1]};
    const auto extend = [&](const float* p) {
      b.lo_x = std::min(b.lo_x, p[0]); b.hi_x = std::max(b.hi_x, p[0]);
      b.lo_y = std::min(b.lo_y, p[1]); b.hi_y = std::max(b.hi_y, p[1]);
    };
    for (int i = 0; i != I.num_returns; ++i) extend(I.returns + 3 * static_cast<size_t>(i));
    for (int i = 0; i != I.num_misses; ++i) extend(I.misses + 3 * static_cast<size_t>(i));
    boxes[k] = b;
  });
  constexpr float kPadding = 1e-6f;
  for (int k = 0; k < num; ++k) {
    PlannedGrid& G = (*grids)[in[k].grid];
    const Box& b = boxes[k];
    PlanGrow(&G, b.lo_x - kPadding * 1.f, b.lo_y - kPadding * 1.f, k);
    PlanGrow(&G, b.hi_x + kPadding * 1.f, b.hi_y + kPadding * 1.f, k);
    PlannedInsertion& P = (*out)[k];
    ++G.insertions;
    P.at = G.limits;
    P.start_x = G.start_x;
    P.start_y = G.start_y;
    // The cell index falls as the coordinate rises; x cells come from y coordinates (FineIndex).
    const auto clip = [](long v, int n) { return static_cast<int>(std::min<long>(std::max<long>(v, 0), n - 1)); };
    const int x0 = clip(PlanCell(G.limits.max_y, b.hi_y, G.limits.resolution) - 1, G.limits.nx);
    const int x1 = clip(PlanCell(G.limits.max_y, b.lo_y, G.limits.resolution) + 1, G.limits.nx);
    const int y0 = clip(PlanCell(G.limits.max_x, b.hi_x, G.limits.resolution) - 1, G.limits.ny);
    const int y1 = clip(PlanCell(G.limits.max_x, b.lo_x, G.limits.resolution) + 1, G.limits.ny);
    P.box_x = x0;
    P.box_y = y0;
    P.box_w = std::max(x1 - x0 + 1, 0);
    P.box_h = std::max(y1 - y0 + 1, 0);
  }
}

// ---- device ----------------------------------------------------------------------------
struct Grid2DInsertionDesc {
  GridView view;              // limits at this insertion; cells: its cell (0, 0) in the final storage
  int stride;                 // row stride of the final storage
  float origin_x, origin_y;
  const float* returns;       // staged points
  const float* misses;
  int2* ends;                 // num_points superscaled cells
  int num_returns, num_points;
  int first_hit, first_ray, first_clear;   // first block in each launch of the set
  int box_x, box_y, box_w, box_h;
};

// Apply of grid_2d.hip on a view that is a window of a larger storage.
__device__ __forceinline__ void ApplyAt(const Grid2DInsertionDesc& D, int cx, int cy,
                                        const uint16_t* __restrict__ table, int* error) {
  if (static_cast<unsigned>(cx) >= static_cast<unsigned>(D.view.nx) ||
      static_cast<unsigned>(cy) >= static_cast<unsigned>(D.view.ny)) {
    *error = 1;                                          // DCHECK(limits().Contains(cell_index))
    return;
  }
  uint16_t* cell = D.view.cells + static_cast<size_t>(D.stride) * cy + cx;
  const uint16_t old = *cell;
  if (old >= kUpdateMarker) return;
  *cell = table[old];
}

__global__ void __launch_bounds__(kHitPoints)
BatchHitKernel(const Grid2DInsertionDesc* __restrict__ descs, int num,
               const uint16_t* __restrict__ hit_table, int* __restrict__ error) {
  const auto& D = descs[DescOfBlock<&Grid2DInsertionDesc::first_hit>(descs, num, blockIdx.x)];
  const int i = (blockIdx.x - D.first_hit) * kHitPoints + threadIdx.x;
  if (i >= D.num_points) return;
  const float* p = i < D.num_returns ? D.returns + 3 * static_cast<size_t>(i)
                                     : D.misses + 3 * static_cast<size_t>(i - D.num_returns);
  const int2 fine = FineIndex(D.view, p[0], p[1]);
  D.ends[i] = fine;
  if (i < D.num_returns) ApplyAt(D, fine.x / kSubpixelScale, fine.y / kSubpixelScale, hit_table, error);
}

__global__ void __launch_bounds__(64 * kRaysPerBlock)
BatchMissKernel(const Grid2DInsertionDesc* __restrict__ descs, int num,
                const uint16_t* __restrict__ miss_table, int* __restrict__ error) {
  const auto& D = descs[DescOfBlock<&Grid2DInsertionDesc::first_ray>(descs, num, blockIdx.x)];
  const int lane = threadIdx.x & 63;
  const int ray = (blockIdx.x - D.first_ray) * kRaysPerBlock + (threadIdx.x >> 6);
  if (ray >= D.num_points) return;
  ForEachRayPixel(FineIndex(D.view, D.origin_x, D.origin_y), D.ends[ray], lane,
                  [&](int x, int y) { ApplyAt(D, x, y, miss_table, error); });
}

// Grid2D::FinishUpdate over the insertion's box.
__global__ void __launch_bounds__(256)
BatchFinishKernel(const Grid2DInsertionDesc* __restrict__ descs, int num) {
  const auto& D = descs[DescOfBlock<&Grid2DInsertionDesc::first_clear>(descs, num, blockIdx.x)];
  const int count = D.box_w * D.box_h;
  const int base = (blockIdx.x - D.first_clear) * kClearCells;
  const int end = min(base + kClearCells, count);
  for (int i = base + threadIdx.x; i < end; i += 256) {
    uint16_t* cell = D.view.cells + static_cast<size_t>(D.stride) * (D.box_y + i / D.box_w) +
                     D.box_x + i % D.box_w;
    const uint16_t value = *cell;
    if (value >= kUpdateMarker) *cell = value - kUpdateMarker;
  }
}

// ---- host ------------------------------------------------------------------------------
// The odds table of a probability on a device, uploaded when it is first asked for and kept for
// the life of the process (64 KB each; a call has two).
const uint16_t* CachedOddsTable(int device, float probability) {
  static std::mutex mu;
  static auto* tables = new std::map<std::pair<int, uint32_t>, uint16_t*>;
  uint32_t bits;
  std::memcpy(&bits, &probability, sizeof(bits));
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_pair(device, bits);
  auto it = tables->find(key);
  if (it != tables->end()) return it->second;
  std::vector<uint16_t> host(32768);
  Grid2DOddsTable(probability, host.data());
  uint16_t* table = nullptr;
  CMX_HIP(hipMalloc(reinterpret_cast<void**>(&table), 32768 * sizeof(uint16_t)));
  const hipError_t err =
      hipMemcpy(table, host.data(), 32768 * sizeof(uint16_t), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    (void)hipFree(table);
    CMX_HIP(err);
  }
  (*tables)[key] = table;
  return table;
}

// The storage grids grow into: freed again unless the call gets as far as handing it to them.
struct GrownCells {
  std::vector<uint16_t*> cells;   // by grid of the call; null: does not grow
  ~GrownCells() {
    for (uint16_t* p : cells)
      if (p) (void)hipFree(p);
  }
};

void InsertBatch(const cmx_grid2d_insertion* insertions, int num, float hit_probability,
                 float miss_probability, bool insert_free_space) {
  // Every argument check before the device is touched.
  CMX_REQUIRE(insertions != nullptr, "null insertions");
  CMX_REQUIRE(num >= 1, "num_insertions %d < 1", num);
  CMX_REQUIRE(hit_probability > 0.f && hit_probability < 1.f && miss_probability > 0.f &&
                  miss_probability < 1.f,
              "probability must be in (0, 1)");
  TargetRounds<cmx_grid2d*> order;
  const std::vector<cmx_grid2d*>& grids = order.targets;
  StagedArrays scans(3);
  std::vector<PlanInput> inputs(num);
  size_t total_points = 0;
  for (int k = 0; k < num; ++k) {           // (no grid is looked into before all are known to be there)
    const cmx_grid2d_insertion& I = insertions[k];
    CMX_REQUIRE(I.grid && I.origin_xy, "insertion %d: null argument", k);
    CMX_REQUIRE(I.num_returns >= 0 && I.num_misses >= 0 && (I.num_returns == 0 || I.returns_xyz) &&
                    (I.num_misses == 0 || I.misses_xyz),
                "insertion %d: bad range data", k);
    CMX_REQUIRE(static_cast<long long>(I.num_returns) + I.num_misses <= 0x7fffffffll,
                "insertion %d: more than 2^31 - 1 points", k);
  }
  for (int k = 0; k < num; ++k) {
    const cmx_grid2d_insertion& I = insertions[k];
    CMX_REQUIRE(I.grid->device == insertions[0].grid->device,
                "insertion %d: all grids of a batch must live on one device", k);
    const auto mismatch = [](int item, int there, int here) {
      CMX_REQUIRE(false,
                  "insertion %d: points given by the pointer of an earlier scan of the call, "
                  "%d of them there and %d here",
                  item, there, here);
    };
    scans.Add(k, I.returns_xyz, I.num_returns, mismatch);
    scans.Add(k, I.misses_xyz, I.num_misses, mismatch);
    total_points += static_cast<size_t>(I.num_returns) + I.num_misses;
    order.Add(I.grid);
    inputs[k] = PlanInput{order.target_of[k], I.origin_xy, I.returns_xyz, I.num_returns,
                          I.misses_xyz, I.num_misses};
  }
  const int num_grids = static_cast<int>(grids.size());
  std::vector<PlannedGrid> planned_grids(num_grids);
  for (int g = 0; g < num_grids; ++g)
    planned_grids[g].limits = PlanLimits{grids[g]->resolution, grids[g]->max_x, grids[g]->max_y,
                                         grids[g]->nx, grids[g]->ny};
  std::vector<PlannedInsertion> plan;
  PlanInsertions(&planned_grids, inputs.data(), num, &plan);

  const int device = grids[0]->device;
  WorkspaceLease ws(device);
  hipStream_t stream = ws->stream;
  const uint16_t* hit_table = CachedOddsTable(device, hit_probability);
  const uint16_t* miss_table = CachedOddsTable(device, miss_probability);

  // Every allocation first: one that fails leaves every grid as it was.
  GrownCells grown;
  grown.cells.assign(num_grids, nullptr);
  std::vector<int> growing;
  for (int g = 0; g < num_grids; ++g) {
    if (planned_grids[g].doublings == 0) continue;
    const PlanLimits& L = planned_grids[g].limits;
    CMX_HIP(hipMalloc(reinterpret_cast<void**>(&grown.cells[g]),
                      static_cast<size_t>(L.nx) * L.ny * sizeof(uint16_t)));
    growing.push_back(g);
  }

  // One upload block: descriptors (set after set) | grow descriptors | points.
  BlockLayout block;
  const auto descs_in = block.Add<Grid2DInsertionDesc>(num);
  const auto grow_in = block.Add<GrowDesc<1>>(growing.size());
  const auto points_in = block.Add<float>(scans.floats());
  char* h_block = static_cast<char*>(ws->pinned[0].Reserve(block.bytes));
  char* d_block = static_cast<char*>(ws->dev[0].Reserve(block.bytes));
  int2* d_ends = ws->dev[1].ReserveAs<int2>(std::max<size_t>(total_points, 1));
  // (the kernels raise the flag in pinned memory themselves: nothing to copy back)
  int* h_error = ws->pinned[1].ReserveAs<int>(4);
  *h_error = 0;
  const float* d_points = points_in(d_block);

  size_t largest_growing = 0;
  for (size_t j = 0; j < growing.size(); ++j) {
    const int g = growing[j];
    const PlannedGrid& G = planned_grids[g];
    grow_in(h_block)[j] = GrowDesc<1>{{grids[g]->cells}, {grown.cells[g]}, nullptr, 0,
                                      grids[g]->nx, grids[g]->ny, G.limits.nx, G.limits.ny,
                                      G.start_x, G.start_y};
    largest_growing = std::max(largest_growing, static_cast<size_t>(G.limits.nx) * G.limits.ny);
  }

  std::vector<size_t> ends_at(num);
  {
    size_t cursor = 0;
    for (int k = 0; k < num; ++k) {
      ends_at[k] = cursor;
      cursor += static_cast<size_t>(inputs[k].num_returns) + inputs[k].num_misses;
    }
  }
  // The sets of launches (hits, rays, marker clearing), a descriptor where its set wants it.
  const int most = Debug().grid2d_insert_chain > 0 ? Debug().grid2d_insert_chain : kChainInsertions;
  const std::vector<LaunchSet> sets = CutSets(
      order.round_of, most, {kSetBlocks, kSetBlocks, kSetBlocks},
      [&](int k, long long* blocks) {
        const long long points = static_cast<long long>(inputs[k].num_returns) + inputs[k].num_misses;
        blocks[0] = BlocksOf(points, kHitPoints);
        blocks[1] = insert_free_space ? BlocksOf(points, kRaysPerBlock) : 0;
        blocks[2] = points ? BlocksOf(static_cast<long long>(plan[k].box_w) * plan[k].box_h,
                                      kClearCells) : 0;
      },
      [&](int k, int slot, const long long* first) {
        const PlanInput& I = inputs[k];
        const PlannedInsertion& P = plan[k];
        const PlannedGrid& G = planned_grids[I.grid];
        uint16_t* storage = grown.cells[I.grid] ? grown.cells[I.grid] : grids[I.grid]->cells;
        // Whole cells between this view and the final storage.
        const int off_x = G.start_x - P.start_x, off_y = G.start_y - P.start_y;
        Grid2DInsertionDesc D{};
        D.view = GridView{storage + static_cast<size_t>(G.limits.nx) * off_y + off_x, P.at.nx,
                          P.at.ny, P.at.resolution / kSubpixelScale, P.at.max_x, P.at.max_y};
        D.stride = G.limits.nx;
        D.origin_x = I.origin[0];
        D.origin_y = I.origin[1];
        D.returns = I.num_returns ? d_points + scans.OffsetOf(I.returns) : nullptr;
        D.misses = I.num_misses ? d_points + scans.OffsetOf(I.misses) : nullptr;
        D.ends = d_ends + ends_at[k];
        D.num_returns = I.num_returns;
        D.num_points = I.num_returns + I.num_misses;
        D.first_hit = static_cast<int>(first[0]);
        D.first_ray = static_cast<int>(first[1]);
        D.first_clear = static_cast<int>(first[2]);
        D.box_x = P.box_x;
        D.box_y = P.box_y;
        D.box_w = P.box_w;
        D.box_h = P.box_h;
        descs_in(h_block)[slot] = D;
      });
  // Every distinct scan once (the pool's threads: a copy is memory bound).
  scans.CopyTo(points_in(h_block), [](int n, const std::function<void(int)>& copy) {
    ParallelFor(n, 8, copy);
  });

  // From here on cells may change: whatever happens, the cached images of the grids are stale.
  struct Touched {
    const std::vector<cmx_grid2d*>& grids;
    hipStream_t stream;
    bool committed = false;
    ~Touched() {
      if (committed) return;
      (void)hipStreamSynchronize(stream);      // nothing in flight when the grown storage goes
      for (cmx_grid2d* g : grids) ++g->version;
    }
  } touched{grids, stream};

  SmallCopyAsync(d_block, h_block, block.bytes, /*to_device=*/true, stream);
  if (!growing.empty())
    LaunchBatchGrow(grow_in(d_block), growing.size(), largest_growing, stream);
  for (const LaunchSet& set : sets) {
    const int n = set.end - set.begin;
    const Grid2DInsertionDesc* descs = descs_in(d_block) + set.begin;
    if (set.total[0] > 0)
      BatchHitKernel<<<static_cast<unsigned>(set.total[0]), kHitPoints, 0, stream>>>(
          descs, n, hit_table, h_error);
    if (set.total[1] > 0)
      BatchMissKernel<<<static_cast<unsigned>(set.total[1]), 64 * kRaysPerBlock, 0, stream>>>(
          descs, n, miss_table, h_error);
    if (set.total[2] > 0)
      BatchFinishKernel<<<static_cast<unsigned>(set.total[2]), 256, 0, stream>>>(descs, n);
  }
  CMX_HIP(hipGetLastError());
  CMX_HIP(hipStreamSynchronize(stream));

  // The grids take their new storage and limits; the version moves as the single calls move it
  // (once per doubling, once per insertion).
  touched.committed = true;
  for (int g = 0; g < num_grids; ++g) {
    cmx_grid2d* grid = grids[g];
    const PlannedGrid& G = planned_grids[g];
    if (grown.cells[g]) {
      (void)hipFree(grid->cells);
      grid->cells = grown.cells[g];
      grown.cells[g] = nullptr;
    }
    grid->max_x = G.limits.max_x;
    grid->max_y = G.limits.max_y;
    grid->nx = G.limits.nx;
    grid->ny = G.limits.ny;
    grid->version += static_cast<unsigned long long>(G.doublings) + G.insertions;
  }
  CMX_REQUIRE(!*h_error, "internal error: range data left the grid after GrowLimits");
}

}  // namespace
}  // namespace cmx

extern "C" cmx_status cmx_grid2d_insert_batch(const cmx_grid2d_insertion* insertions,
                                              int32_t num_insertions, float hit_probability,
                                              float miss_probability, int32_t insert_free_space) {
  return cmx::Guard([&] {
    cmx::InsertBatch(insertions, num_insertions, hit_probability, miss_probability,
                     insert_free_space != 0);
  });
}

extern "C" cmx_status cmx_debug_grid2d_insert_plan(const cmx_grid2d_limits* limits,
                                                   int32_t num_grids,
                                                   const cmx_debug_grid2d_insertion* insertions,
                                                   int32_t num_insertions, int32_t* rounds,
                                                   cmx_grid2d_limits* final_limits) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(limits && insertions && rounds && final_limits, "null argument");
    CMX_REQUIRE(num_grids >= 1 && num_insertions >= 1, "nothing to plan");
    std::vector<PlannedGrid> grids(num_grids);
    for (int g = 0; g < num_grids; ++g) {
      CMX_REQUIRE(limits[g].resolution > 0. && limits[g].num_x_cells >= 1 &&
                      limits[g].num_y_cells >= 1,
                  "grid %d: bad map limits", g);
      grids[g].limits = PlanLimits{limits[g].resolution, limits[g].max_x, limits[g].max_y,
                                   limits[g].num_x_cells, limits[g].num_y_cells};
    }
    std::vector<PlanInput> inputs(num_insertions);
    for (int k = 0; k < num_insertions; ++k) {
      const cmx_debug_grid2d_insertion& I = insertions[k];
      CMX_REQUIRE(I.grid >= 0 && I.grid < num_grids && I.origin_xy, "insertion %d: bad grid or origin", k);
      CMX_REQUIRE(I.num_returns >= 0 && I.num_misses >= 0 &&
                      (I.num_returns == 0 || I.returns_xyz) && (I.num_misses == 0 || I.misses_xyz),
                  "insertion %d: bad range data", k);
      inputs[k] = PlanInput{I.grid, I.origin_xy, I.returns_xyz, I.num_returns, I.misses_xyz,
                            I.num_misses};
    }
    std::vector<PlannedInsertion> plan;
    PlanInsertions(&grids, inputs.data(), num_insertions, &plan);
    TargetRounds<int> order;
    for (int k = 0; k < num_insertions; ++k) order.Add(inputs[k].grid);
    std::copy(order.round_of.begin(), order.round_of.end(), rounds);
    for (int g = 0; g < num_grids; ++g) {
      final_limits[g] = limits[g];
      final_limits[g].max_x = grids[g].limits.max_x;
      final_limits[g].max_y = grids[g].limits.max_y;
      final_limits[g].num_x_cells = grids[g].limits.nx;
      final_limits[g].num_y_cells = grids[g].limits.ny;
    }
  });
}
