// cmx_grid3d_insert_batch: RangeDataInserter3D::Insert for many (grid, cloud) pairs in one call --
// the four insertions of ActiveSubmaps3D::InsertData (two submaps, a high- and a low-resolution
// grid each; mapping/3d/submap_3d.cc:271-287,310-329), or those of many robots after one
// cmx_fast3d_match_pairs -- bit for bit the single calls of grid_3d.hip in list order.
//
// Rounds.  Round r holds the r-th insertion of every grid, so that no grid appears twice in a
// round; a round is three launches over all its insertions (hits, miss samples, marker clearing)
// and the rounds follow each other on the stream.  "First writer wins" inside a phase is what
// makes the single kernels exact (grid_3d.hip); insertions into different grids touch different
// bricks and insertions into one grid are separated by launches, so batching adds no race.
//
// Growth.  Which voxels an insertion touches is known on the device only (f32 divide and lround
// per point), so pass 0 is one extent launch over every insertion of the call and one read-back.
// The plan then replays the single call's growth insertion by insertion: grid_size doubles until
// the box fits and the brick becomes the union of the 16-aligned boxes.  Both are monotone and a
// voxel's value does not depend on either, so every grid is grown ONCE, before the first round,
// to what its last insertion needs: a cell's address changes, never its content.
//
// Blocks.  A workgroup never spans two insertions: every descriptor holds the first block it has
// in the extent launch and in each of its set's three launches, and a block finds its insertion by
// bisection over them -- the same for all its threads, so the search runs on the scalar unit.
//
// Marker clearing.  The single call sweeps the whole brick, millions of cells for a few thousand
// touched ones.  A resident grid holds no marker between calls (cmx_grid3d_create starts empty,
// every insertion clears its own), so the only marked cells are those the insertion's own hits and
// miss samples visited: the clearing launch walks the same (return) and (return, k) indices again
// and stores `cell & 0x7fff` where bit 15 is set.  Threads that meet on a voxel store one value.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/cartographer_mi355x_debug.h"
#include "cmx_batch.h"
#include "grid_3d_internal.h"

namespace cmx {
namespace {

constexpr int kBlock = 256;                  // threads per block of every launch
constexpr int kChainInsertions = 4096;       // insertions per set of launches (grid3d_insert_chain)
constexpr long long kSetBlocks = 1ll << 24;  // blocks of any one launch of a set
constexpr int kIntMax = 0x7fffffff, kIntMin = -0x7fffffff - 1;

// ---- plan (host only) ------------------------------------------------------------------
struct PlanInput {
  int grid;
  int box[6];                 // touched voxels: min x, y, z, max x, y, z; min > max: none
};

struct PlannedGrid {
  BrickBounds brick;          // in: before the call; out: after it
  int grid_size = 128;
  bool grows = false;
};

// What InsertRangeData's growth steps (grid_3d.hip) make of every grid when the insertions run in
// list order.  `grids` in: the state before the call.
void PlanInsertions(std::vector<PlannedGrid>* grids, const PlanInput* in, int num) {
  for (int k = 0; k < num; ++k) {
    PlannedGrid& G = (*grids)[in[k].grid];
    const int* lo = in[k].box;
    const int* hi = in[k].box + 3;
    if (lo[0] > hi[0]) continue;                         // no returns: nothing is written
    for (int a = 0; a < 3; ++a)
      CMX_REQUIRE(lo[a] > -(1 << 20) && hi[a] < (1 << 20) && lo[a] <= hi[a],
                  "insertion %d: voxel index out of range", k);
    G.grid_size = PlanGridSize(G.grid_size, lo, hi);
    BrickBounds to;
    if (!PlanBrick(G.brick, lo, hi, &to)) continue;
    CMX_REQUIRE(BrickCells(to) < kMaxBrickCells,
                "insertion %d: dense voxel brick of %d x %d x %d is too large", k, to.dims[0],
                to.dims[1], to.dims[2]);
    G.brick = to;
    G.grows = true;
  }
}

// ---- device ----------------------------------------------------------------------------
struct Grid3DInsertionDesc {
  BrickView view;             // the grid's brick after the call's growth (set once it is planned)
  const float* returns;       // staged points
  float origin[3];
  float resolution;
  int num_returns;
  int first_extent;           // first block in the extent launch of the call
  int first_hit, first_miss, first_clear;   // first block in each launch of its set
};

// Grid3DExtentKernel of grid_3d.hip, segmented: out[8 * d] = {min x, y, z, max x, y, z, error,
// pad} of descriptor d; error 2: a ray of 2^15 voxels or more.
__global__ void __launch_bounds__(kBlock)
BatchExtentKernel(const Grid3DInsertionDesc* __restrict__ descs, int num, int num_free_space_voxels,
                  int* __restrict__ out) {
  const int d = DescOfBlock<&Grid3DInsertionDesc::first_extent>(descs, num, blockIdx.x);
  const Grid3DInsertionDesc& D = descs[d];
  int* box = out + 8 * static_cast<size_t>(d);
  const long long i = static_cast<long long>(blockIdx.x - D.first_extent) * kBlock + threadIdx.x;
  int lo[3] = {kIntMax, kIntMax, kIntMax}, hi[3] = {kIntMin, kIntMin, kIntMin};
  if (i < D.num_returns) {
    const int3 o = CellOf(D.origin, D.resolution);
    const int3 h = CellOf(D.returns + 3 * static_cast<size_t>(i), D.resolution);
    const auto extend = [&](int3 c) {
      lo[0] = min(lo[0], c.x); lo[1] = min(lo[1], c.y); lo[2] = min(lo[2], c.z);
      hi[0] = max(hi[0], c.x); hi[1] = max(hi[1], c.y); hi[2] = max(hi[2], c.z);
    };
    extend(h);
    const int3 delta = make_int3(h.x - o.x, h.y - o.y, h.z - o.z);
    const int num_samples = max(abs(delta.x), max(abs(delta.y), abs(delta.z)));
    if (num_samples >= (1 << 15)) {
      box[6] = 2;
    } else {
      // Samples are monotone along the ray, so the first and the last touched sample bound
      // every one in between, component by component.
      const int first = max(0, num_samples - num_free_space_voxels);
      if (first < num_samples) {
        extend(MissCell(o, delta, first, num_samples));
        extend(MissCell(o, delta, num_samples - 1, num_samples));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int wlo = WaveMin(lo[k]), whi = WaveMax(hi[k]);
    if ((threadIdx.x & 63) == 0 && wlo <= whi) {
      atomicMin(&box[k], wlo);
      atomicMax(&box[3 + k], whi);
    }
  }
}

// `errors`: one flag per descriptor of the set ("a voxel fell outside the brick").
__global__ void __launch_bounds__(kBlock)
BatchHitKernel(const Grid3DInsertionDesc* __restrict__ descs, int num,
               const uint16_t* __restrict__ hit_table, int* __restrict__ errors) {
  const int d = DescOfBlock<&Grid3DInsertionDesc::first_hit>(descs, num, blockIdx.x);
  const Grid3DInsertionDesc& D = descs[d];
  const long long i = static_cast<long long>(blockIdx.x - D.first_hit) * kBlock + threadIdx.x;
  if (i >= D.num_returns) return;
  Apply(D.view, CellOf(D.returns + 3 * static_cast<size_t>(i), D.resolution), hit_table,
        errors + d);
}

// One thread per (return, k): sample position num_samples - num_free_space_voxels + k.
__global__ void __launch_bounds__(kBlock)
BatchMissKernel(const Grid3DInsertionDesc* __restrict__ descs, int num, int num_free_space_voxels,
                const uint16_t* __restrict__ miss_table, int* __restrict__ errors) {
  const int d = DescOfBlock<&Grid3DInsertionDesc::first_miss>(descs, num, blockIdx.x);
  const Grid3DInsertionDesc& D = descs[d];
  const long long t = static_cast<long long>(blockIdx.x - D.first_miss) * kBlock + threadIdx.x;
  if (t >= static_cast<long long>(D.num_returns) * num_free_space_voxels) return;
  const int i = static_cast<int>(t / num_free_space_voxels);
  const int k = static_cast<int>(t - static_cast<long long>(i) * num_free_space_voxels);
  const int3 o = CellOf(D.origin, D.resolution);
  const int3 h = CellOf(D.returns + 3 * static_cast<size_t>(i), D.resolution);
  const int3 delta = make_int3(h.x - o.x, h.y - o.y, h.z - o.z);
  const int num_samples = max(abs(delta.x), max(abs(delta.y), abs(delta.z)));
  const int position = num_samples - num_free_space_voxels + k;
  if (position < 0 || position >= num_samples) return;
  Apply(D.view, MissCell(o, delta, position, num_samples), miss_table, errors + d);
}

// HybridGrid::FinishUpdate (hybrid_grid.h:463-469) for the voxels the insertion visited: one
// thread per (return, k), k = num_free_space_voxels being the hit itself.
__global__ void __launch_bounds__(kBlock)
BatchClearKernel(const Grid3DInsertionDesc* __restrict__ descs, int num, int num_free_space_voxels) {
  const auto& D = descs[DescOfBlock<&Grid3DInsertionDesc::first_clear>(descs, num, blockIdx.x)];
  const long long per_return = static_cast<long long>(num_free_space_voxels) + 1;
  const long long t = static_cast<long long>(blockIdx.x - D.first_clear) * kBlock + threadIdx.x;
  if (t >= D.num_returns * per_return) return;
  const int i = static_cast<int>(t / per_return);
  const int k = static_cast<int>(t - i * per_return);
  int3 c = CellOf(D.returns + 3 * static_cast<size_t>(i), D.resolution);
  if (k < num_free_space_voxels) {
    const int3 o = CellOf(D.origin, D.resolution);
    const int3 delta = make_int3(c.x - o.x, c.y - o.y, c.z - o.z);
    const int num_samples = max(abs(delta.x), max(abs(delta.y), abs(delta.z)));
    const int position = num_samples - num_free_space_voxels + k;
    if (position < 0 || position >= num_samples) return;
    c = MissCell(o, delta, position, num_samples);
  }
  const BrickView& b = D.view;
  const int x = c.x - b.lo_x, y = c.y - b.lo_y, z = c.z - b.lo_z;
  if (static_cast<unsigned>(x) >= static_cast<unsigned>(b.nx) ||
      static_cast<unsigned>(y) >= static_cast<unsigned>(b.ny) ||
      static_cast<unsigned>(z) >= static_cast<unsigned>(b.nz))
    return;                                              // (flagged by the launch that met it)
  uint16_t* cell = b.cells + (static_cast<size_t>(z) * b.ny + y) * b.nx + x;
  const uint16_t value = *cell;
  if (value >= kUpdateMarker) *cell = value & (kUpdateMarker - 1);
}

// ---- host ------------------------------------------------------------------------------
// The bricks grids grow into: released again unless the call gets as far as handing them over.
struct StagedBricks {
  hipStream_t stream;
  std::vector<uint16_t*> cells;   // by grid of the call; null: does not grow
  ~StagedBricks() {
    bool any = false;
    for (uint16_t* p : cells) any |= p != nullptr;
    if (!any) return;
    (void)hipStreamSynchronize(stream);        // nothing in flight when they go
    for (uint16_t* p : cells)
      if (p) (void)hipFree(p);
  }
};

void InsertBatch(const cmx_grid3d_insertion* insertions, int num, float hit_probability,
                 float miss_probability, int num_free_space_voxels) {
  // Every argument check before the device is touched.
  CMX_REQUIRE(insertions != nullptr, "null insertions");
  CMX_REQUIRE(num >= 1, "num_insertions %d < 1", num);
  CMX_REQUIRE(num_free_space_voxels >= 0, "num_free_space_voxels must not be negative");
  CMX_REQUIRE(hit_probability > 0.f && hit_probability < 1.f && miss_probability > 0.f &&
                  miss_probability < 1.f,
              "probability must be in (0, 1)");
  const long long per_return = static_cast<long long>(num_free_space_voxels) + 1;
  for (int k = 0; k < num; ++k) {           // (no grid is looked into before all are known to be there)
    const cmx_grid3d_insertion& I = insertions[k];
    CMX_REQUIRE(I.grid && I.origin_xyz, "insertion %d: null argument", k);
    CMX_REQUIRE(I.num_returns >= 0 && (I.num_returns == 0 || I.returns_xyz),
                "insertion %d: bad range data", k);
    CMX_REQUIRE(I.reserved == 0, "insertion %d: reserved must be 0", k);
    CMX_REQUIRE(static_cast<long long>(I.num_returns) * num_free_space_voxels < (1ll << 38),
                "insertion %d: too many free-space samples", k);
  }
  TargetRounds<cmx_grid3d*> order;
  const std::vector<cmx_grid3d*>& grids = order.targets;
  const std::vector<int>& grid_of = order.target_of;
  StagedArrays clouds(3);
  for (int k = 0; k < num; ++k) {
    const cmx_grid3d_insertion& I = insertions[k];
    CMX_REQUIRE(I.grid->device == insertions[0].grid->device,
                "insertion %d: all grids of a batch must live on one device", k);
    clouds.Add(k, I.returns_xyz, I.num_returns, [](int item, int there, int here) {
      CMX_REQUIRE(false,
                  "insertion %d: returns given by the pointer of an earlier cloud of the call, "
                  "%d of them there and %d here",
                  item, there, here);
    });
    order.Add(I.grid);
  }
  const int num_grids = static_cast<int>(grids.size());

  // The sets of launches (hits, miss samples, marker clearing).  An insertion's descriptor stands
  // where its set wants it; `slot_of` finds it from the list.
  const int most = Debug().grid3d_insert_chain > 0 ? Debug().grid3d_insert_chain : kChainInsertions;
  std::vector<Grid3DInsertionDesc> descs(num);
  std::vector<int> slot_of(num);
  long long extent_blocks = 0;
  const std::vector<LaunchSet> sets = CutSets(
      order.round_of, most, {kSetBlocks, kSetBlocks, kSetBlocks},
      [&](int k, long long* blocks) {
        const long long n = insertions[k].num_returns;
        blocks[0] = BlocksOf(n, kBlock);
        blocks[1] = BlocksOf(n * num_free_space_voxels, kBlock);
        blocks[2] = BlocksOf(n * per_return, kBlock);
      },
      [&](int k, int slot, const long long* first) {
        Grid3DInsertionDesc D{};
        for (int a = 0; a < 3; ++a) D.origin[a] = insertions[k].origin_xyz[a];
        D.resolution = grids[grid_of[k]]->resolution;
        D.num_returns = insertions[k].num_returns;
        D.first_extent = static_cast<int>(extent_blocks);
        D.first_hit = static_cast<int>(first[0]);
        D.first_miss = static_cast<int>(first[1]);
        D.first_clear = static_cast<int>(first[2]);
        slot_of[k] = slot;
        descs[slot] = D;
        extent_blocks += BlocksOf(D.num_returns, kBlock);
        CMX_REQUIRE(extent_blocks <= kIntMax, "insertion %d: too many returns in one call", k);
      });

  const int device = grids[0]->device;
  WorkspaceLease ws(device);
  hipStream_t stream = ws->stream;
  const uint16_t* hit_table = DeviceTable(grids[0], hit_probability);
  const uint16_t* miss_table = DeviceTable(grids[0], miss_probability);
  if (extent_blocks == 0) return;                        // nothing is written, FinishUpdate no-op

  // One upload block: descriptors | extent boxes (preset) | points.
  BlockLayout block;
  const auto descs_in = block.Add<Grid3DInsertionDesc>(num);
  const auto boxes_in = block.Add<int>(8 * static_cast<size_t>(num));
  const auto points_in = block.Add<float>(clouds.floats());
  char* h_block = static_cast<char*>(ws->pinned[0].Reserve(block.bytes));
  char* d_block = static_cast<char*>(ws->dev[0].Reserve(block.bytes));
  Grid3DInsertionDesc* h_descs = descs_in(h_block);
  const Grid3DInsertionDesc* d_descs = descs_in(d_block);
  int* d_boxes = boxes_in(d_block);
  const float* d_points = points_in(d_block);
  // Read back: the boxes; raised by the kernels in pinned memory themselves: the error flags.
  int* h_boxes = ws->pinned[1].ReserveAs<int>(9 * static_cast<size_t>(num));
  int* h_errors = h_boxes + 8 * static_cast<size_t>(num);
  std::memset(h_errors, 0, sizeof(int) * num);
  for (int k = 0; k < num; ++k)
    if (insertions[k].num_returns > 0)
      descs[slot_of[k]].returns = d_points + clouds.OffsetOf(insertions[k].returns_xyz);
  std::memcpy(h_descs, descs.data(), sizeof(Grid3DInsertionDesc) * num);
  for (int s = 0; s < num; ++s) {
    const int preset[8] = {kIntMax, kIntMax, kIntMax, kIntMin, kIntMin, kIntMin, 0, 0};
    std::memcpy(boxes_in(h_block) + 8 * static_cast<size_t>(s), preset, sizeof(preset));
  }
  // Every distinct cloud once (the pool's threads: a copy is memory bound).
  clouds.CopyTo(points_in(h_block), [](int n, const std::function<void(int)>& copy) {
    ParallelFor(n, 8, copy);
  });

  // Pass 0: the box of every insertion, one launch and one read-back.
  SmallCopyAsync(d_block, h_block, block.bytes, /*to_device=*/true, stream);
  BatchExtentKernel<<<static_cast<unsigned>(extent_blocks), kBlock, 0, stream>>>(
      d_descs, num, num_free_space_voxels, d_boxes);
  CMX_HIP(hipGetLastError());
  SmallCopyAsync(h_boxes, d_boxes, 8 * sizeof(int) * num, /*to_device=*/false, stream);
  CMX_HIP(hipStreamSynchronize(stream));

  // The plan, in list order; an error names the first insertion a run of single calls would have
  // stopped at, and nothing has been written yet.
  int planned = num;
  for (int k = num - 1; k >= 0; --k)
    if (h_boxes[8 * static_cast<size_t>(slot_of[k]) + 6] != 0) planned = k;
  std::vector<PlanInput> inputs(num);
  for (int k = 0; k < num; ++k) {
    inputs[k].grid = grid_of[k];
    std::memcpy(inputs[k].box, h_boxes + 8 * static_cast<size_t>(slot_of[k]), 6 * sizeof(int));
  }
  std::vector<PlannedGrid> planned_grids(num_grids);
  for (int g = 0; g < num_grids; ++g) {
    for (int a = 0; a < 3; ++a) {
      planned_grids[g].brick.lo[a] = grids[g]->lo[a];
      planned_grids[g].brick.dims[a] = grids[g]->dims[a];
    }
    planned_grids[g].grid_size = grids[g]->grid_size;
  }
  PlanInsertions(&planned_grids, inputs.data(), planned);
  CMX_REQUIRE(planned == num, "insertion %d: a ray spans 2^15 voxels or more", planned);

  // Every new brick before any old one is released: an allocation that fails leaves every grid
  // as it was.
  StagedBricks staged{stream, std::vector<uint16_t*>(num_grids, nullptr)};
  for (int g = 0; g < num_grids; ++g)
    if (planned_grids[g].grows)
      staged.cells[g] = StageGrownBrick(grids[g], planned_grids[g].brick, stream);

  for (int k = 0; k < num; ++k) {
    const int g = grid_of[k];
    const BrickBounds& B = planned_grids[g].brick;
    h_descs[slot_of[k]].view =
        BrickView{staged.cells[g] ? staged.cells[g] : grids[g]->cells, B.lo[0], B.lo[1], B.lo[2],
                  B.dims[0], B.dims[1], B.dims[2]};
  }
  SmallCopyAsync(d_block, h_block, sizeof(Grid3DInsertionDesc) * num, /*to_device=*/true, stream);
  for (const LaunchSet& set : sets) {
    const int n = set.end - set.begin;
    const Grid3DInsertionDesc* set_descs = d_descs + set.begin;
    if (set.total[0] > 0)
      BatchHitKernel<<<static_cast<unsigned>(set.total[0]), kBlock, 0, stream>>>(
          set_descs, n, hit_table, h_errors + set.begin);
    if (set.total[1] > 0)
      BatchMissKernel<<<static_cast<unsigned>(set.total[1]), kBlock, 0, stream>>>(
          set_descs, n, num_free_space_voxels, miss_table, h_errors + set.begin);
    if (set.total[2] > 0)
      BatchClearKernel<<<static_cast<unsigned>(set.total[2]), kBlock, 0, stream>>>(
          set_descs, n, num_free_space_voxels);
  }
  CMX_HIP(hipGetLastError());
  CMX_HIP(hipStreamSynchronize(stream));

  for (int g = 0; g < num_grids; ++g) {
    grids[g]->grid_size = planned_grids[g].grid_size;
    if (!staged.cells[g]) continue;
    uint16_t* grown = staged.cells[g];
    staged.cells[g] = nullptr;
    CommitBrick(grids[g], grown, planned_grids[g].brick);
  }
  for (int k = 0; k < num; ++k)
    CMX_REQUIRE(!h_errors[slot_of[k]],
                "insertion %d: internal error: a voxel fell outside the brick", k);
}

}  // namespace
}  // namespace cmx

extern "C" cmx_status cmx_grid3d_insert_batch(const cmx_grid3d_insertion* insertions,
                                              int32_t num_insertions, float hit_probability,
                                              float miss_probability,
                                              int32_t num_free_space_voxels) {
  return cmx::Guard([&] {
    cmx::InsertBatch(insertions, num_insertions, hit_probability, miss_probability,
                     num_free_space_voxels);
  });
}

extern "C" cmx_status cmx_debug_grid3d_insert_plan(const cmx_debug_grid3d_state* grids,
                                                   int32_t num_grids,
                                                   const cmx_debug_grid3d_insertion* insertions,
                                                   int32_t num_insertions, int32_t* rounds,
                                                   cmx_debug_grid3d_state* final_states) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(grids && insertions && rounds && final_states, "null argument");
    CMX_REQUIRE(num_grids >= 1 && num_insertions >= 1, "nothing to plan");
    std::vector<PlannedGrid> planned(num_grids);
    for (int g = 0; g < num_grids; ++g) {
      const cmx_debug_grid3d_state& S = grids[g];
      const bool empty = S.dims[0] == 0 && S.dims[1] == 0 && S.dims[2] == 0;
      CMX_REQUIRE(empty || (S.dims[0] >= 1 && S.dims[1] >= 1 && S.dims[2] >= 1),
                  "grid %d: bad brick", g);
      CMX_REQUIRE(S.grid_size >= 128 && (S.grid_size & (S.grid_size - 1)) == 0,
                  "grid %d: bad grid_size", g);
      for (int a = 0; a < 3; ++a) {
        planned[g].brick.lo[a] = empty ? 0 : S.lo[a];
        planned[g].brick.dims[a] = S.dims[a];
      }
      planned[g].grid_size = S.grid_size;
    }
    std::vector<PlanInput> inputs(num_insertions);
    for (int k = 0; k < num_insertions; ++k) {
      CMX_REQUIRE(insertions[k].grid >= 0 && insertions[k].grid < num_grids,
                  "insertion %d: bad grid", k);
      inputs[k].grid = insertions[k].grid;
      std::memcpy(inputs[k].box, insertions[k].box, sizeof(inputs[k].box));
    }
    TargetRounds<int> order;
    for (int k = 0; k < num_insertions; ++k) order.Add(inputs[k].grid);
    std::copy(order.round_of.begin(), order.round_of.end(), rounds);
    PlanInsertions(&planned, inputs.data(), num_insertions);
    for (int g = 0; g < num_grids; ++g) {
      final_states[g] = cmx_debug_grid3d_state{};
      for (int a = 0; a < 3; ++a) {
        final_states[g].lo[a] = planned[g].brick.lo[a];
        final_states[g].dims[a] = planned[g].brick.dims[a];
      }
      final_states[g].grid_size = planned[g].grid_size;
    }
  });
}
