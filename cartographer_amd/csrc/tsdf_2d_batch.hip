// cmx_tsdf2d_insert_batch: TSDFRangeDataInserter2D::Insert for many (grid, scan) pairs in one
// call -- the two insertions of ActiveSubmaps2D::InsertRangeData on grid_type = "TSDF"
// (mapping/2d/submap_2d.cc:161-174), or those of many robots after one
// cmx_rt2d_match_tsdf_grid_batch -- bit for bit the single calls of tsdf_2d.hip in list order.
//
// Rounds.  Round r holds the r-th insertion of every grid, so that no grid appears twice in a
// round; a round is two launches over all its insertions (owner, apply: tsdf_2d.hip) and the
// rounds follow each other on the stream.  "The lowest hit index with a non-zero weight takes the
// cell", settled by atomicMin on the grid's owner plane and applied by the owner alone, is what
// makes the single kernels exact; hit indices are those of the insertion's own table.  Insertions
// into different grids touch different planes and insertions into one grid are separated by
// launches, so batching adds no race.  The apply launch puts every owner entry it meets back to
// kNoOwner, so a round finds the plane as the single call does.
//
// Host.  The O(N) libm work of an insertion (the sort, the normals, the weights) depends on the
// scan alone and is done once per distinct scan, the scans in parallel on the host pool; the ray
// ends depend on the grid's limits and are computed per insertion, in parallel, straight into the
// pinned upload block (tsdf_2d_host.h).  Every check is made there, before the device is touched.
//
// Growth.  GrowAsNeeded depends on the points only: the plan replays the single call's GrowLimits
// loops insertion by insertion with the evolving limits, and every grid is grown ONCE, before the
// first round, to the size its last insertion needs (one launch for all grids that grow: both
// planes, and the owner plane at kNoOwner).  Ray ends and cell centres are NOT computed from the
// final limits: (max - p) / fine_resolution - 0.5 and max_x - resolution * (cy + 0.5) with another
// `max` may round differently.  An insertion's descriptor carries the limits the grid has at that
// insertion -- they serve CellUpdate and the Inside check behind the error flag exactly as in the
// single kernels -- and plane pointers to its cell (0, 0) inside the final storage with the final
// row stride: the view of an earlier insertion is a window of the final grid, whole cells apart.
//
// Blocks.  A workgroup never spans two insertions: it holds 4 rays of one, a wavefront each
// (ForEachRayPixel).  Every descriptor holds the first block it has in the two launches of its
// set, and a block finds its insertion by bisection over them; the descriptor is the same for the
// whole block and is read once, into scalar registers.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/cartographer_mi355x_debug.h"
#include "cmx_batch.h"
#include "grid_grow_batch.h"
#include "tsdf_2d_internal.h"

namespace cmx {
namespace {

constexpr int kRaysPerBlock = 4;           // one wavefront per ray
constexpr int kChainInsertions = 4096;     // insertions per set of launches (tsdf2d_insert_chain)
constexpr long long kSetBlocks = 1ll << 24;  // blocks of a launch of a set

// ---- device ----------------------------------------------------------------------------
struct Tsdf2DInsertionDesc {
  TsdfParams P;               // limits at this insertion; planes: its cell (0, 0) in the final storage
  const TsdfRay* rays;
  int num_rays;
  int stride;                 // row stride of the final storage
  int first_block;            // in either launch of the set
};

// TsdfOwnerKernel of tsdf_2d.hip on a view that is a window of a larger storage.
__global__ void __launch_bounds__(64 * kRaysPerBlock)
TsdfBatchOwnerKernel(const Tsdf2DInsertionDesc* __restrict__ descs, int num) {
  const Tsdf2DInsertionDesc D =
      descs[DescOfBlock<&Tsdf2DInsertionDesc::first_block>(descs, num, blockIdx.x)];
  const TsdfParams& P = D.P;
  const int lane = threadIdx.x & 63;
  const int r = (blockIdx.x - D.first_block) * kRaysPerBlock + (threadIdx.x >> 6);
  if (r >= D.num_rays) return;
  const TsdfRay ray = D.rays[r];
  if (!P.distance_kernel && ray.weight_factor == 0.f) return;   // no cell of this ray updates
  ForEachRayPixel(ray.begin, ray.end, lane, [&](int x, int y) {
    if (!Inside(P, x, y)) return;
    const size_t flat = static_cast<size_t>(D.stride) * y + x;
    if (P.tsd[flat] >= kUpdateMarker) return;            // CellIsUpdated before this Insert
    if (CellUpdate(P, ray, x, y).y == 0.f) return;       // UpdateCell returns unmarked (:230)
    atomicMin(&P.owner[flat], r);
  });
}

// TsdfApplyKernel of tsdf_2d.hip likewise.
__global__ void __launch_bounds__(64 * kRaysPerBlock)
TsdfBatchApplyKernel(const Tsdf2DInsertionDesc* __restrict__ descs, int num) {
  const Tsdf2DInsertionDesc D =
      descs[DescOfBlock<&Tsdf2DInsertionDesc::first_block>(descs, num, blockIdx.x)];
  const TsdfParams& P = D.P;
  const int lane = threadIdx.x & 63;
  const int r = (blockIdx.x - D.first_block) * kRaysPerBlock + (threadIdx.x >> 6);
  if (r >= D.num_rays) return;
  const TsdfRay ray = D.rays[r];
  if (!P.distance_kernel && ray.weight_factor == 0.f) return;
  ForEachRayPixel(ray.begin, ray.end, lane, [&](int x, int y) {
    if (!Inside(P, x, y)) return;
    const size_t flat = static_cast<size_t>(D.stride) * y + x;
    if (P.owner[flat] != r || atomicCAS(&P.owner[flat], r, kNoOwner) != r) return;
    const float2 u = CellUpdate(P, ray, x, y);
    const float old_tsd = ValueToBounded(P.tsd[flat], -P.max_tsd, P.max_tsd);
    const float old_weight = ValueToBounded(P.weight[flat], 0.f, P.max_weight);
    float updated_weight = old_weight + u.y;
    const float updated_sdf = (old_tsd * old_weight + u.x * u.y) / updated_weight;
    updated_weight = P.maximum_weight < updated_weight ? P.maximum_weight : updated_weight;
    P.tsd[flat] = TsdToValue(P, updated_sdf);
    P.weight[flat] = WeightToValue(P, updated_weight);
  });
}

// ---- host ------------------------------------------------------------------------------
[[noreturn]] void ThrowPlanError(const tsdf2d::PlanError& e) {
  switch (e.kind) {
    case tsdf2d::PlanError::kCountMismatch:
      CMX_REQUIRE(false,
                  "insertion %d: returns given by the pointer of an earlier scan of the call, "
                  "%ld of them there and %ld here",
                  e.insertion, e.a, e.b);
    case tsdf2d::PlanError::kTooManyCells:
      CMX_REQUIRE(false, "insertion %d: grid grows beyond 2^30 cells", e.insertion);
    default:
      CMX_REQUIRE(false,
                  "insertion %d: range data leaves the grid limits after GrowAsNeeded "
                  "(hit %ld; z != 0?)",
                  e.insertion, e.a);
  }
  throw HipError{CMX_INVALID_ARGUMENT};
}

// Distinct scans and ray tables on the host pool (ParallelFor: at most 16 threads).  A scan costs
// a hundred microseconds or more, so two are worth a wake-up of the pool; a ray table costs
// about ten, so the two tables of an ActiveSubmaps2D pair are built where they are.
const auto kScansOnPool = [](int n, const std::function<void(int)>& fn) { ParallelFor(n, 2, fn); };
const auto kTablesOnPool = [](int n, const std::function<void(int)>& fn) {
  ParallelFor(n, 16, fn);
};

// The storage grids grow into: freed again unless the call gets as far as handing it to them.
struct GrownPlanes {
  struct Planes { uint16_t* tsd = nullptr; uint16_t* weight = nullptr; int32_t* owner = nullptr; };
  std::vector<Planes> planes;     // by grid of the call; null: does not grow
  ~GrownPlanes() {
    for (const Planes& p : planes) {
      if (p.tsd) (void)hipFree(p.tsd);
      if (p.weight) (void)hipFree(p.weight);
      if (p.owner) (void)hipFree(p.owner);
    }
  }
};

void InsertBatch(const cmx_tsdf2d_insertion* insertions, int num,
                 const cmx_tsdf_inserter_options_2d* options) {
  // Every argument check before the device is touched.
  CMX_REQUIRE(insertions != nullptr, "null insertions");
  CMX_REQUIRE(num >= 1, "num_insertions %d < 1", num);
  for (int k = 0; k < num; ++k) {           // (no grid is looked into before all are known to be there)
    const cmx_tsdf2d_insertion& I = insertions[k];
    CMX_REQUIRE(I.grid && I.origin_xyz, "insertion %d: null argument", k);
    CMX_REQUIRE(I.num_returns >= 0 && (I.num_returns == 0 || I.returns_xyz),
                "insertion %d: bad range data", k);
  }
  RequireInserterOptions(options);
  TargetRounds<cmx_tsdf2d*> order;
  const std::vector<cmx_tsdf2d*>& grids = order.targets;
  std::vector<tsdf2d::InsertionInput> inputs(num);
  for (int k = 0; k < num; ++k) {
    const cmx_tsdf2d_insertion& I = insertions[k];
    CMX_REQUIRE(I.grid->device == insertions[0].grid->device,
                "insertion %d: all grids of a batch must live on one device", k);
    order.Add(I.grid);
    inputs[k] = tsdf2d::InsertionInput{order.target_of[k], I.origin_xyz, I.returns_xyz,
                                       I.num_returns};
  }
  const int num_grids = static_cast<int>(grids.size());
  tsdf2d::CallPlan plan;
  plan.grids.resize(num_grids);
  for (int g = 0; g < num_grids; ++g)
    plan.grids[g].limits = tsdf2d::Limits{grids[g]->resolution, grids[g]->max_x, grids[g]->max_y,
                                          grids[g]->nx, grids[g]->ny};
  if (const tsdf2d::PlanError e = tsdf2d::PlanCall(&plan, inputs.data(), num, *options, kScansOnPool))
    ThrowPlanError(e);
  std::vector<int> growing;
  size_t largest_growing = 0;
  for (int g = 0; g < num_grids; ++g) {
    if (plan.grids[g].doublings == 0) continue;
    growing.push_back(g);
    largest_growing = std::max(largest_growing, static_cast<size_t>(plan.grids[g].limits.nx) *
                                                    plan.grids[g].limits.ny);
  }

  const int device = grids[0]->device;
  WorkspaceLease ws(device);
  hipStream_t stream = ws->stream;

  // One upload block: descriptors (set after set) | grow descriptors | ray tables.  The ray
  // tables hold the last check: a ray end outside the limits its insertion has.
  BlockLayout block;
  const auto descs_in = block.Add<Tsdf2DInsertionDesc>(num);
  const auto grow_in = block.Add<GrowDesc<2>>(growing.size());
  const auto rays_in = block.Add<TsdfRay>(plan.total_rays);
  char* h_block = static_cast<char*>(ws->pinned[0].Reserve(block.bytes));
  if (const tsdf2d::PlanError e = tsdf2d::BuildRayTables(plan, rays_in(h_block), kTablesOnPool))
    ThrowPlanError(e);
  char* d_block = static_cast<char*>(ws->dev[0].Reserve(block.bytes));
  // (the kernels raise the flag in pinned memory themselves: nothing to copy back)
  int* h_error = ws->pinned[1].ReserveAs<int>(4);
  *h_error = 0;

  // Every allocation first: one that fails leaves every grid as it was.
  GrownPlanes grown;
  grown.planes.resize(num_grids);
  for (const int g : growing) {
    const size_t count = static_cast<size_t>(plan.grids[g].limits.nx) * plan.grids[g].limits.ny;
    GrownPlanes::Planes& p = grown.planes[g];
    CMX_HIP(hipMalloc(reinterpret_cast<void**>(&p.tsd), count * sizeof(uint16_t)));
    CMX_HIP(hipMalloc(reinterpret_cast<void**>(&p.weight), count * sizeof(uint16_t)));
    CMX_HIP(hipMalloc(reinterpret_cast<void**>(&p.owner), count * sizeof(int32_t)));
  }
  for (size_t j = 0; j < growing.size(); ++j) {
    const int g = growing[j];
    const tsdf2d::PlannedGrid& G = plan.grids[g];
    const GrownPlanes::Planes& p = grown.planes[g];
    grow_in(h_block)[j] = GrowDesc<2>{{grids[g]->tsd, grids[g]->weight}, {p.tsd, p.weight},
                                      p.owner, kNoOwner, grids[g]->nx, grids[g]->ny,
                                      G.limits.nx, G.limits.ny, G.start_x, G.start_y};
  }

  // The sets of launches (owner, apply), a descriptor where its set wants it.
  const int most =
      Debug().tsdf2d_insert_chain > 0 ? Debug().tsdf2d_insert_chain : kChainInsertions;
  const TsdfRay* d_rays = rays_in(d_block);
  const std::vector<LaunchSet> sets = CutSets(
      order.round_of, most, {kSetBlocks, kSetBlocks, kSetBlocks},
      [&](int k, long long* blocks) {
        blocks[0] = BlocksOf(plan.insertions[k].num_rays, kRaysPerBlock);
      },
      [&](int k, int slot, const long long* first) {
        const tsdf2d::PlannedInsertion& I = plan.insertions[k];
        const int g = inputs[k].grid;
        const tsdf2d::PlannedGrid& G = plan.grids[g];
        const GrownPlanes::Planes& p = grown.planes[g];
        // Whole cells between this view and the final storage.
        const size_t window = static_cast<size_t>(G.limits.nx) * (G.start_y - I.start_y) +
                              (G.start_x - I.start_x);
        Tsdf2DInsertionDesc D{};
        D.P = MakeParams(*grids[g]);
        D.P.tsd = (p.tsd ? p.tsd : grids[g]->tsd) + window;
        D.P.weight = (p.weight ? p.weight : grids[g]->weight) + window;
        D.P.owner = (p.owner ? p.owner : grids[g]->owner) + window;
        D.P.nx = I.at.nx;
        D.P.ny = I.at.ny;
        D.P.max_x = I.at.max_x;
        D.P.max_y = I.at.max_y;
        SetInsertion(&D.P, inputs[k].origin, *options);
        D.P.error = h_error;
        D.rays = d_rays + I.first_ray;
        D.num_rays = I.num_rays;
        D.stride = G.limits.nx;
        D.first_block = static_cast<int>(first[0]);
        descs_in(h_block)[slot] = D;
      });

  // From here on planes may change: whatever happens, the cached images of the grids are stale.
  struct Touched {
    const std::vector<cmx_tsdf2d*>& grids;
    hipStream_t stream;
    bool committed = false;
    ~Touched() {
      if (committed) return;
      (void)hipStreamSynchronize(stream);      // nothing in flight when the grown storage goes
      for (cmx_tsdf2d* g : grids) ++g->version;
    }
  } touched{grids, stream};

  SmallCopyAsync(d_block, h_block, block.bytes, /*to_device=*/true, stream);
  if (!growing.empty())
    LaunchBatchGrow(grow_in(d_block), growing.size(), largest_growing, stream);
  for (const LaunchSet& set : sets) {
    if (set.total[0] == 0) continue;
    const int n = set.end - set.begin;
    const Tsdf2DInsertionDesc* descs = descs_in(d_block) + set.begin;
    const unsigned blocks = static_cast<unsigned>(set.total[0]);
    TsdfBatchOwnerKernel<<<blocks, 64 * kRaysPerBlock, 0, stream>>>(descs, n);
    TsdfBatchApplyKernel<<<blocks, 64 * kRaysPerBlock, 0, stream>>>(descs, n);
  }
  CMX_HIP(hipGetLastError());
  CMX_HIP(hipStreamSynchronize(stream));

  // The grids take their new storage and limits; the version moves as the single calls move it
  // (once per doubling, once per insertion).
  touched.committed = true;
  for (int g = 0; g < num_grids; ++g) {
    cmx_tsdf2d* grid = grids[g];
    const tsdf2d::PlannedGrid& G = plan.grids[g];
    GrownPlanes::Planes& p = grown.planes[g];
    if (p.tsd) {
      (void)hipFree(grid->tsd);
      (void)hipFree(grid->weight);
      (void)hipFree(grid->owner);
      grid->tsd = p.tsd;
      grid->weight = p.weight;
      grid->owner = p.owner;
      p = GrownPlanes::Planes{};
    }
    grid->max_x = G.limits.max_x;
    grid->max_y = G.limits.max_y;
    grid->nx = G.limits.nx;
    grid->ny = G.limits.ny;
    grid->version += static_cast<unsigned long long>(G.doublings) + G.insertions;
  }
  CMX_REQUIRE(!*h_error, "internal error: a ray left the grid after GrowAsNeeded");
}

}  // namespace
}  // namespace cmx

extern "C" cmx_status cmx_tsdf2d_insert_batch(const cmx_tsdf2d_insertion* insertions,
                                              int32_t num_insertions,
                                              const cmx_tsdf_inserter_options_2d* options) {
  return cmx::Guard([&] { cmx::InsertBatch(insertions, num_insertions, options); });
}

extern "C" cmx_status cmx_debug_tsdf2d_insert_plan(
    const cmx_grid2d_limits* limits, int32_t num_grids,
    const cmx_debug_tsdf2d_insertion* insertions, int32_t num_insertions,
    const cmx_tsdf_inserter_options_2d* options, int32_t* rounds, cmx_grid2d_limits* limits_at,
    int32_t* num_rays, int32_t* num_scans) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(limits && insertions && rounds && limits_at && num_rays && num_scans,
                "null argument");
    CMX_REQUIRE(num_grids >= 1 && num_insertions >= 1, "nothing to plan");
    RequireInserterOptions(options);
    tsdf2d::CallPlan plan;
    plan.grids.resize(num_grids);
    for (int g = 0; g < num_grids; ++g) {
      CMX_REQUIRE(limits[g].resolution > 0. && limits[g].num_x_cells >= 1 &&
                      limits[g].num_y_cells >= 1,
                  "grid %d: bad map limits", g);
      plan.grids[g].limits = tsdf2d::Limits{limits[g].resolution, limits[g].max_x, limits[g].max_y,
                                            limits[g].num_x_cells, limits[g].num_y_cells};
    }
    std::vector<tsdf2d::InsertionInput> inputs(num_insertions);
    TargetRounds<int> order;
    for (int k = 0; k < num_insertions; ++k) {
      const cmx_debug_tsdf2d_insertion& I = insertions[k];
      CMX_REQUIRE(I.grid >= 0 && I.grid < num_grids && I.origin_xyz,
                  "insertion %d: bad grid or origin", k);
      CMX_REQUIRE(I.num_returns >= 0 && (I.num_returns == 0 || I.returns_xyz),
                  "insertion %d: bad range data", k);
      inputs[k] = tsdf2d::InsertionInput{I.grid, I.origin_xyz, I.returns_xyz, I.num_returns};
      order.Add(I.grid);
    }
    if (const tsdf2d::PlanError e =
            tsdf2d::PlanCall(&plan, inputs.data(), num_insertions, *options, kScansOnPool))
      ThrowPlanError(e);
    if (const tsdf2d::PlanError e = tsdf2d::BuildRayTables(plan, nullptr, kTablesOnPool))
      ThrowPlanError(e);
    for (int k = 0; k < num_insertions; ++k) {
      const tsdf2d::Limits& at = plan.insertions[k].at;
      rounds[k] = order.round_of[k];
      limits_at[k] = limits[inputs[k].grid];
      limits_at[k].max_x = at.max_x;
      limits_at[k].max_y = at.max_y;
      limits_at[k].num_x_cells = at.nx;
      limits_at[k].num_y_cells = at.ny;
      num_rays[k] = plan.insertions[k].num_rays;
    }
    *num_scans = static_cast<int32_t>(plan.scans.size());
  });
}
