// The fast 3D matchers of many submaps in one call (cmx_fast3d_create_batch): what
// ConstraintBuilder3D::DispatchScanMatcherConstruction (constraint_builder_3d.cc:170-198) does once
// per submap of a loaded map, as ONE chain of launches whose length does not depend on the number
// of submaps.  Every kernel here is the twin of a single-matcher kernel (fast_3d_stack.hip,
// dense_brick_3d.hip) and calls the same per-cell function (fast_3d_stack_device.h, ScatterVoxel), so a
// matcher of a batch is the single create's bit for bit.  Workgroups are dealt to (submap, tile of
// cells) through prefix tables of block counts; every matcher lives in one allocation of its own.
#include <algorithm>
#include <chrono>

#include "cmx_batch.h"
#include "fast_3d_stack_device.h"

namespace cmx {
namespace {

constexpr int kBatchThreads = 256;
// Per workgroup: cells of a level or a crop box (four consecutive per thread: a wavefront writes
// 256 consecutive level bytes), oct words (two per thread: 1 KiB per wavefront), voxels, zeroed
// bytes, and the most workgroups that scan one resident brick.  One pass per thread for the cell
// and oct tiles: a lone C5-sized submap still gives every CU a dozen workgroups per launch (with
// four passes its chain took 600 us where the single create's launches take 300).
constexpr int kCellTile = 4 * kBatchThreads;
constexpr int kOctTile = 2 * kBatchThreads;
constexpr int kVoxelTile = 4 * kBatchThreads;
constexpr int kZeroTile = 16 * 1024;
constexpr int kBoundsGroupsPerBlock = 4 * kBatchThreads;
constexpr int kBoundsBlocks = 256;

// One matcher of a chain.
struct StackProblem3D {
  Brick level[kMaxDepth];
  OctDesc oct[kMaxDepth];          // cells == nullptr: not built
  int shift[kMaxDepth], half[kMaxDepth];
  Brick high, low;                 // the matcher's raw copies
  Brick source[2];                 // resident: the grids' bricks (cells == nullptr: empty)
  const cmx_voxel* voxels[2];      // voxel lists: in the chain's staging block
  long long num_voxels[2];
  char* zero;                      // voxel lists: level 0 and the raw copies, to be zeroed
  unsigned long long zero_bytes;   // (a multiple of 16)
};

// first[e] = first block of entry e of the launch, first[num] = blocks of the launch: the entry
// that owns this workgroup (entries without blocks own none), searched by one thread.
__device__ __forceinline__ int EntryOfWorkgroup(const int* __restrict__ first, int num) {
  __shared__ int entry;
  if (threadIdx.x == 0) entry = EntryOfBlock(first, num, blockIdx.x);
  __syncthreads();
  return entry;
}

// Cell i of a dense brick (x fastest).
__device__ __forceinline__ void CellOf(const Brick& b, long long i, int* x, int* y, int* z) {
  const long long row = i / b.nx;
  *x = static_cast<int>(i - row * b.nx);
  *y = static_cast<int>(row % b.ny);
  *z = static_cast<int>(row / b.ny);
}
__device__ __forceinline__ void NextCell(const Brick& b, int* x, int* y, int* z) {
  if (++*x == b.nx) {
    *x = 0;
    if (++*y == b.ny) { *y = 0; ++*z; }
  }
}

// Entry e = brick e of `bricks` (2 r: the high-, 2 r + 1: the low-resolution grid of resident
// source r), box + 6 e its bounds: Grid3DNonZeroBoundsKernel for all of them.
__global__ void __launch_bounds__(kBatchThreads)
BatchBounds3DKernel(const Brick* __restrict__ bricks, const int* __restrict__ first, int num,
                    int* __restrict__ box) {
  const int e = EntryOfWorkgroup(first, num);
  const Brick b = bricks[e];
  const long long local = blockIdx.x - first[e], blocks = first[e + 1] - first[e];
  int lo[3] = {kEmptyBoxLo, kEmptyBoxLo, kEmptyBoxLo}, hi[3] = {kEmptyBoxHi, kEmptyBoxHi,
                                                                kEmptyBoxHi};
  WidenNonZeroBounds3D(b, local * kBatchThreads + threadIdx.x, blocks * kBatchThreads, lo, hi);
  MergeBoundsIntoBox3D(lo, hi, box + 6 * e);
}

// Entry e = grid e % 2 of problem members[e / 2]: Grid3DCropKernel for all resident sources.
__global__ void __launch_bounds__(kBatchThreads)
BatchCrop3DKernel(const StackProblem3D* __restrict__ problems, const int* __restrict__ members,
                  const int* __restrict__ first, int num) {
  const int e = EntryOfWorkgroup(first, num);
  const StackProblem3D& P = problems[members[e >> 1]];
  const bool is_high = (e & 1) == 0;
  const Brick out = is_high ? P.high : P.low;
  const Brick src = P.source[e & 1];
  const long long count = static_cast<long long>(out.nx) * out.ny * out.nz;
  const long long base = static_cast<long long>(blockIdx.x - first[e]) * kCellTile;
  const long long end = min(base + kCellTile, count);
  uint16_t* raw = static_cast<uint16_t*>(const_cast<void*>(out.cells));
  uint8_t* level0 = static_cast<uint8_t*>(const_cast<void*>(P.level[0].cells));
  for (long long i = base + 4 * threadIdx.x; i < end; i += 4 * kBatchThreads) {
    int x, y, z;
    CellOf(out, i, &x, &y, &z);
    unsigned v[4] = {0, 0, 0, 0};
    const int cells = static_cast<int>(min(4ll, count - i));
    for (int k = 0; k < cells; ++k) {
      v[k] = CropValue3D(src, x + out.lo_x, y + out.lo_y, z + out.lo_z);
      NextCell(out, &x, &y, &z);
    }
    if (cells == 4) {               // (regions start at 256-byte boundaries, i % 4 == 0)
      *reinterpret_cast<uint2*>(raw + i) = make_uint2(v[0] | v[1] << 16, v[2] | v[3] << 16);
      if (is_high)
        *reinterpret_cast<unsigned*>(level0 + i) =
            PrecomputationValueDev(v[0]) | PrecomputationValueDev(v[1]) << 8 |
            PrecomputationValueDev(v[2]) << 16 | PrecomputationValueDev(v[3]) << 24;
    } else {
      for (int k = 0; k < cells; ++k) {
        raw[i + k] = static_cast<uint16_t>(v[k]);
        if (is_high) level0[i + k] = PrecomputationValueDev(v[k]);
      }
    }
  }
}

// Entry e = problem members[e]: zeroes level 0 and the raw copies of a voxel-list source.
__global__ void __launch_bounds__(kBatchThreads)
BatchZero3DKernel(const StackProblem3D* __restrict__ problems, const int* __restrict__ members,
                  const int* __restrict__ first, int num) {
  const int e = EntryOfWorkgroup(first, num);
  const StackProblem3D& P = problems[members[e]];
  const unsigned long long base = static_cast<unsigned long long>(blockIdx.x - first[e]) * kZeroTile;
  const unsigned long long end = min(base + kZeroTile, P.zero_bytes);
  for (unsigned long long i = base + 16ull * threadIdx.x; i < end; i += 16ull * kBatchThreads)
    *reinterpret_cast<uint4*>(P.zero + i) = make_uint4(0, 0, 0, 0);
}

// Entry e = list e % 2 of problem members[e / 2]: ScatterVoxelsKernel for the three bricks of all
// voxel-list sources (the high-resolution list fills level 0 and the raw copy).
__global__ void __launch_bounds__(kBatchThreads)
BatchScatter3DKernel(const StackProblem3D* __restrict__ problems, const int* __restrict__ members,
                     const int* __restrict__ first, int num) {
  const int e = EntryOfWorkgroup(first, num);
  const StackProblem3D& P = problems[members[e >> 1]];
  const int list = e & 1;
  const cmx_voxel* __restrict__ voxels = P.voxels[list];
  const long long base = static_cast<long long>(blockIdx.x - first[e]) * kVoxelTile;
  const long long end = min(base + kVoxelTile, P.num_voxels[list]);
  for (long long i = base + threadIdx.x; i < end; i += kBatchThreads) {
    const cmx_voxel v = voxels[i];
    if (list == 0) {
      ScatterVoxel(v, P.level[0], 1);
      ScatterVoxel(v, P.high, 2);
    } else {
      ScatterVoxel(v, P.low, 2);
    }
  }
}

// Entry p = problem p: PrecomputeLevel3DKernel for level d of all of them (each reads its own
// level d - 1 only: stream order is enough).
__global__ void __launch_bounds__(kBatchThreads)
BatchLevel3DKernel(const StackProblem3D* __restrict__ problems, const int* __restrict__ first,
                   int num, int d) {
  const int p = EntryOfWorkgroup(first, num);
  const StackProblem3D& P = problems[p];
  const Brick prev = P.level[d - 1], out = P.level[d];
  const int shift = P.shift[d], half = P.half[d];
  const long long count = static_cast<long long>(out.nx) * out.ny * out.nz;
  const long long base = static_cast<long long>(blockIdx.x - first[p]) * kCellTile;
  const long long end = min(base + kCellTile, count);
  uint8_t* cells = static_cast<uint8_t*>(const_cast<void*>(out.cells));
  for (long long i = base + 4 * threadIdx.x; i < end; i += 4 * kBatchThreads) {
    int x, y, z;
    CellOf(out, i, &x, &y, &z);
    unsigned v[4] = {0, 0, 0, 0};
    const int todo = static_cast<int>(min(4ll, count - i));
    for (int k = 0; k < todo; ++k) {
      v[k] = PrecomputedCell3D(prev, x + out.lo_x, y + out.lo_y, z + out.lo_z, shift, half);
      NextCell(out, &x, &y, &z);
    }
    if (todo == 4) {
      *reinterpret_cast<unsigned*>(cells + i) = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
    } else {
      for (int k = 0; k < todo; ++k) cells[i + k] = static_cast<uint8_t>(v[k]);
    }
  }
}

// Entry e = level e % child_levels of problem e / child_levels: BuildOct3DKernel for every level
// that can be a child level, of every problem, in one launch (they read finished levels only).
__global__ void __launch_bounds__(kBatchThreads)
BatchOct3DKernel(const StackProblem3D* __restrict__ problems, const int* __restrict__ first,
                 int num_entries, int child_levels) {
  const int e = EntryOfWorkgroup(first, num_entries);
  const StackProblem3D& P = problems[e / child_levels];
  const int l = e % child_levels;
  const Brick L = P.level[l];
  const OctDesc O = P.oct[l];
  Brick words{};                   // the array's index space
  words.nx = O.qx; words.ny = O.qy; words.nz = O.qz;
  const long long count = static_cast<long long>(O.qx) * O.qy * O.qz;
  const long long base = static_cast<long long>(blockIdx.x - first[e]) * kOctTile;
  const long long end = min(base + kOctTile, count);
  uint2* out = const_cast<uint2*>(O.cells);
  for (long long i = base + 2 * threadIdx.x; i < end; i += 2 * kBatchThreads) {
    int X, Y, Z;
    CellOf(words, i, &X, &Y, &Z);
    const uint2 a = OctWord3D(L, O.s, X, Y, Z);
    if (i + 1 < count) {
      NextCell(words, &X, &Y, &Z);
      const uint2 b = OctWord3D(L, O.s, X, Y, Z);
      *reinterpret_cast<uint4*>(out + i) = make_uint4(a.x, a.y, b.x, b.y);
    } else {
      out[i] = a;
    }
  }
}

// What one chain of launches takes: voxel lists staged (pinned and device scratch of the call's
// workspace), blocks over all its launches (far inside a grid's 2^31 - 1), table entries.
constexpr size_t kChainStagingBytes = size_t(32) << 20;
constexpr long long kChainBlocks = 1ll << 30;
constexpr int kChainMatchers = 8192;

long long CellsOf(const Brick& b) { return static_cast<long long>(b.nx) * b.ny * b.nz; }

// The geometry of one matcher -- pure integer work from the two boxes, the rule of
// BuildStackAndOcts -- and where its regions lie in its allocation:
//   level 0 | raw high | raw low | levels 1 .. depth-1 | octs
// each from a 256-byte boundary; the byte and uint16 bricks carry the 16 spare bytes the aligned
// 8-byte reads of their last cells rely on.
struct Plan3D {
  Brick level[kMaxDepth];          // (cells unset)
  int shift[kMaxDepth], half[kMaxDepth];
  size_t level_bytes[kMaxDepth], level_at[kMaxDepth];
  OctDesc oct[kMaxDepth];
  bool has_oct[kMaxDepth];
  size_t oct_bytes[kMaxDepth], oct_at[kMaxDepth];
  Brick high, low;
  size_t high_bytes, low_bytes, high_at, low_at;
  size_t zero_bytes;               // level 0 and the raw copies: what a voxel-list source zeroes
  size_t total;
  long long blocks;                // over all launches of a chain
};

// Throws the single creates' argument errors ("grid too large", "precomputation level too
// large", the dense-brick and index limits); allocates nothing.
Plan3D PlanOf(const cmx_fast3d_options& options, const int lo[2][3], const int hi[2][3],
              bool build_octs) {
  Plan3D plan{};
  const int depth = options.branch_and_bound_depth;
  plan.level[0] = DenseBrickGeometry(lo[0], hi[0], 1, &plan.level_bytes[0]);
  CMX_REQUIRE(plan.level_bytes[0] < (size_t(1) << 31), "grid too large");   // 32-bit cell offsets
  plan.low = DenseBrickGeometry(lo[1], hi[1], 2, &plan.low_bytes);
  plan.high = DenseBrickGeometry(lo[0], hi[0], 2, &plan.high_bytes);
  for (int d = 1; d < depth; ++d)
    plan.level[d] = LevelAbove3D(plan.level[d - 1], d, options.full_resolution_depth,
                                 &plan.shift[d], &plan.half[d], &plan.level_bytes[d]);
  for (int i = 0; build_octs && i + 1 < depth; ++i)
    plan.has_oct[i] = OctOfLevel3D(plan.level[i], i, options.full_resolution_depth, &plan.oct[i],
                                   &plan.oct_bytes[i]);
  BlockLayout slab;
  auto region = [&slab](size_t bytes) { return slab.Add<char>(bytes).at; };
  plan.level_at[0] = region(plan.level_bytes[0] + 16);
  plan.high_at = region(plan.high_bytes + 16);
  plan.low_at = region(plan.low_bytes + 16);
  plan.zero_bytes = slab.bytes;
  for (int d = 1; d < depth; ++d) plan.level_at[d] = region(plan.level_bytes[d] + 16);
  for (int i = 0; i + 1 < depth; ++i)
    if (plan.has_oct[i]) plan.oct_at[i] = region(plan.oct_bytes[i]);
  plan.total = slab.bytes;
  plan.blocks = BlocksOf(CellsOf(plan.high), kCellTile) + BlocksOf(CellsOf(plan.low), kCellTile) +
                BlocksOf(static_cast<long long>(plan.zero_bytes), kZeroTile);
  for (int d = 1; d < depth; ++d) plan.blocks += BlocksOf(CellsOf(plan.level[d]), kCellTile);
  for (int i = 0; i + 1 < depth; ++i)
    if (plan.has_oct[i])
      plan.blocks += BlocksOf(static_cast<long long>(plan.oct_bytes[i] / sizeof(uint2)), kOctTile);
  return plan;
}

Plan3D PlanOfSource(const cmx_fast3d_options& options, const int lo[2][3], const int hi[2][3],
                    bool build_octs, int index) {
  try {
    return PlanOf(options, lo, hi, build_octs);
  } catch (const HipError&) {
    const std::string what = LastError();
    CMX_REQUIRE(false, "source %d: %s", index, what.c_str());
  }
  return Plan3D{};
}

// The matcher of `plan` with its one allocation; nothing is built yet.
std::unique_ptr<cmx_fast3d> AllocateMatcher(const cmx_fast3d_options& options,
                                            const Fast3DSource& source, const Plan3D& plan,
                                            int device) {
  std::unique_ptr<cmx_fast3d> h(new cmx_fast3d);
  Fast3DMatcher& m = h->impl;
  m.options = options;
  m.device = device;
  m.resolution = source.resolution;
  m.low_resolution = source.low_resolution;
  m.width_in_voxels = source.width_in_voxels;
  m.histogram.assign(source.histogram, source.histogram + source.histogram_size);
  m.slab.bytes = plan.total;
  CMX_HIP(hipMalloc(&m.slab.mem, plan.total));
  char* base = static_cast<char*>(m.slab.mem);
  auto place = [base](DeviceBrick* brick, Brick desc, size_t at, size_t bytes) {
    desc.cells = base + at;
    brick->desc = desc;
    brick->bytes = bytes;
  };
  const int depth = options.branch_and_bound_depth;
  for (int d = 0; d < depth; ++d) {
    m.levels.emplace_back(new DeviceBrick);
    place(m.levels[d].get(), plan.level[d], plan.level_at[d], plan.level_bytes[d]);
  }
  place(&m.high, plan.high, plan.high_at, plan.high_bytes);
  place(&m.low, plan.low, plan.low_at, plan.low_bytes);
  m.oct_desc.assign(depth, OctDesc{nullptr, 0, 0, 0, 0});
  for (int i = 0; i + 1 < depth; ++i) {
    if (!plan.has_oct[i]) continue;
    m.oct_desc[i] = plan.oct[i];
    m.oct_desc[i].cells = reinterpret_cast<const uint2*>(base + plan.oct_at[i]);
    m.octs.emplace_back(new DeviceBrick);
    m.octs.back()->desc.cells = m.oct_desc[i].cells;
    m.octs.back()->bytes = plan.oct_bytes[i];
  }
  return h;
}

// Stage 1: the tight boxes of all resident sources, in one launch, one read-back and one
// synchronisation.  box[k] (12 ints) is written for resident sources k only.
void ResidentBoxes(Workspace& ws, const Fast3DSource* sources, const std::vector<int>& resident,
                   std::vector<int>* box, int* launches) {
  const int R = static_cast<int>(resident.size());
  const int entries = 2 * R;
  // The block: bricks | first[entries + 1] | boxes, one pinned mirror.
  BlockLayout block;
  const auto bricks_in = block.Add<Brick>(entries);
  const auto first_in = block.Add<int>(entries + 1);
  const auto box_in = block.Add<int>(6 * entries);
  char* h_block = static_cast<char*>(ws.pinned[1].Reserve(block.bytes));
  char* d_block = static_cast<char*>(ws.dev[1].Reserve(block.bytes));
  Brick* h_bricks = bricks_in(h_block);
  int* h_first = first_in(h_block);
  int* h_box = box_in(h_block);
  long long blocks = 0;
  for (int e = 0; e < entries; ++e) {
    const Brick& b = sources[resident[e >> 1]].grid[e & 1];
    h_bricks[e] = b;
    h_first[e] = static_cast<int>(blocks);
    const long long groups = b.cells ? CellsOf(b) / 8 : 0;
    blocks += std::min<long long>(BlocksOf(groups, kBoundsGroupsPerBlock), kBoundsBlocks);
    for (int k = 0; k < 3; ++k) {
      h_box[6 * e + k] = kEmptyBoxLo;
      h_box[6 * e + 3 + k] = kEmptyBoxHi;
    }
  }
  h_first[entries] = static_cast<int>(blocks);
  if (blocks > 0) {
    SmallCopyAsync(d_block, h_block, block.bytes, /*to_device=*/true, ws.stream);
    BatchBounds3DKernel<<<static_cast<unsigned>(blocks), kBatchThreads, 0, ws.stream>>>(
        bricks_in(d_block), first_in(d_block), entries, box_in(d_block));
    CMX_HIP(hipGetLastError());
    SmallCopyAsync(h_box, box_in(d_block), sizeof(int) * 6 * entries, /*to_device=*/false,
                   ws.stream);
    CMX_HIP(hipStreamSynchronize(ws.stream));
    *launches += 3;
  }
  for (int r = 0; r < R; ++r)
    std::copy(h_box + 12 * r, h_box + 12 * r + 12, box->begin() + 12 * resident[r]);
}

size_t StagedBytesOf(const Fast3DSource& s) {
  if (s.resident) return 0;
  return Align256(static_cast<size_t>(s.num_voxels[0]) * sizeof(cmx_voxel)) +
         Align256(static_cast<size_t>(s.num_voxels[1]) * sizeof(cmx_voxel));
}

}  // namespace

std::vector<std::unique_ptr<cmx_fast3d>> BuildFast3DBatch(const cmx_fast3d_options& options,
                                                          const Fast3DSource* sources, int num,
                                                          int device) {
  using Clock = std::chrono::steady_clock;
  const bool host_trace = Debug().host_trace != 0;
  auto since = [](Clock::time_point t) {
    return std::chrono::duration<double, std::micro>(Clock::now() - t).count();
  };
  const int depth = options.branch_and_bound_depth;
  const int child_levels = depth - 1;
  const bool build_octs = Debug().fast3d_no_oct == 0;
  Clock::time_point lap = Clock::now();

  // The geometry of the voxel-list sources needs no device: their limits are argument errors
  // before it is touched.
  std::vector<Plan3D> plans(num);
  std::vector<int> resident;
  for (int k = 0; k < num; ++k) {
    if (sources[k].resident) {
      resident.push_back(k);
    } else {
      plans[k] = PlanOfSource(options, sources[k].lo, sources[k].hi, build_octs, k);
    }
  }
  WorkspaceLease ws(device);
  hipStream_t stream = ws->stream;
  int launches = 0;
  if (!resident.empty()) {
    std::vector<int> box(static_cast<size_t>(num) * 12);
    ResidentBoxes(*ws, sources, resident, &box, &launches);
    for (int k : resident) {
      // BuildBrickFromVoxels' boxes: a grid without non-zero cells is the empty voxel list's
      // single cell at the origin.
      int lo[2][3], hi[2][3];
      for (int g = 0; g < 2; ++g) {
        const int* b = &box[static_cast<size_t>(k) * 12 + 6 * g];
        const bool empty = b[0] > b[3];
        for (int c = 0; c < 3; ++c) {
          lo[g][c] = empty ? 0 : b[c];
          hi[g][c] = empty ? 0 : b[3 + c];
        }
      }
      plans[k] = PlanOfSource(options, lo, hi, build_octs, k);
    }
  }
  const double bounds_us = since(lap);
  lap = Clock::now();

  // Every allocation first: one that fails leaves nothing built and nothing in flight (the
  // vector frees what exists).
  std::vector<std::unique_ptr<cmx_fast3d>> matchers(num);
  for (int k = 0; k < num; ++k) matchers[k] = AllocateMatcher(options, sources[k], plans[k], device);
  const double alloc_us = since(lap);

  const int most = Debug().fast3d_create_chain > 0 ? Debug().fast3d_create_chain : kChainMatchers;
  // The chains; total[0]: bytes of voxel lists staged, every list from a 256-byte boundary.
  const std::vector<LaunchSet> chains = CutSets(
      std::vector<int>(num, 0), most, {kChainStagingBytes, kChainBlocks, 0},
      [&](int k, long long* add) {
        add[0] = StagedBytesOf(sources[k]);
        add[1] = plans[k].blocks;
      },
      [](int, int, const long long*) {});

  double stage_us = 0., issue_us = 0., wait_us = 0.;
  for (const LaunchSet& chain : chains) {
    lap = Clock::now();
    const int n = chain.end - chain.begin;
    std::vector<int> crop_members, voxel_members;
    for (int j = 0; j < n; ++j)
      (sources[chain.begin + j].resident ? crop_members : voxel_members).push_back(j);
    const int R = static_cast<int>(crop_members.size()), V = static_cast<int>(voxel_members.size());
    // The upload block: problems | members of the crop, of the zero and scatter launches | the
    // prefix tables of the launches | the voxel lists.
    //   tables: crop (2 R + 1) | zero (V + 1) | scatter (2 V + 1) | levels 1 .. depth-1 (n + 1
    //   each) | octs (n * child_levels + 1)
    const size_t oct_entries = static_cast<size_t>(n) * child_levels;
    const size_t table_ints = static_cast<size_t>(R + V) + (2 * R + 1) + (V + 1) + (2 * V + 1) +
                              static_cast<size_t>(child_levels) * (n + 1) + (oct_entries + 1);
    BlockLayout block;
    const auto problems_in = block.Add<StackProblem3D>(n);
    const auto tables_in = block.Add<int>(table_ints);
    const auto lists_in = block.Add<char>(chain.total[0]);
      char* h_block = static_cast<char*>(ws->pinned[0].Reserve(block.bytes));
    char* d_block = static_cast<char*>(ws->dev[0].Reserve(block.bytes));
    StackProblem3D* h_problems = problems_in(h_block);
    int* crop_of = tables_in(h_block);
    int* voxel_of = crop_of + R;
    int* first_crop = voxel_of + V;
    int* first_zero = first_crop + 2 * R + 1;
    int* first_scatter = first_zero + V + 1;
    int* first_level = first_scatter + 2 * V + 1;            // [child_levels][n + 1]: level d at d - 1
    int* first_oct = first_level + static_cast<size_t>(child_levels) * (n + 1);
    auto on_device = [&](const int* host) {
      return reinterpret_cast<const int*>(d_block + (reinterpret_cast<const char*>(host) - h_block));
    };
    std::copy(crop_members.begin(), crop_members.end(), crop_of);
    std::copy(voxel_members.begin(), voxel_members.end(), voxel_of);

    std::vector<size_t> staged_at(static_cast<size_t>(n) * 2, 0);
    size_t cursor = lists_in.at;
    long long crop_blocks = 0, zero_blocks = 0, scatter_blocks = 0, oct_blocks = 0;
    std::vector<long long> level_blocks(depth, 0);
    int r = 0, v = 0;
    for (int j = 0; j < n; ++j) {
      const Fast3DSource& src = sources[chain.begin + j];
      const Fast3DMatcher& m = matchers[chain.begin + j]->impl;
      const Plan3D& plan = plans[chain.begin + j];
      StackProblem3D P{};
      for (int d = 0; d < depth; ++d) {
        P.level[d] = m.levels[d]->desc;
        P.oct[d] = m.oct_desc[d];
        P.shift[d] = plan.shift[d];
        P.half[d] = plan.half[d];
      }
      P.high = m.high.desc;
      P.low = m.low.desc;
      if (src.resident) {
        P.source[0] = src.grid[0];
        P.source[1] = src.grid[1];
        first_crop[2 * r] = static_cast<int>(crop_blocks);
        crop_blocks += BlocksOf(CellsOf(P.high), kCellTile);
        first_crop[2 * r + 1] = static_cast<int>(crop_blocks);
        crop_blocks += BlocksOf(CellsOf(P.low), kCellTile);
        ++r;
      } else {
        for (int list = 0; list < 2; ++list) {
          staged_at[2 * j + list] = cursor;
          P.voxels[list] = reinterpret_cast<const cmx_voxel*>(d_block + cursor);
          P.num_voxels[list] = src.num_voxels[list];
          cursor += Align256(static_cast<size_t>(src.num_voxels[list]) * sizeof(cmx_voxel));
          first_scatter[2 * v + list] = static_cast<int>(scatter_blocks);
          scatter_blocks += BlocksOf(src.num_voxels[list], kVoxelTile);
        }
        P.zero = static_cast<char*>(m.slab.mem);
        P.zero_bytes = plan.zero_bytes;
        first_zero[v] = static_cast<int>(zero_blocks);
        zero_blocks += BlocksOf(static_cast<long long>(plan.zero_bytes), kZeroTile);
        ++v;
      }
      for (int d = 1; d < depth; ++d) {
        first_level[static_cast<size_t>(d - 1) * (n + 1) + j] = static_cast<int>(level_blocks[d]);
        level_blocks[d] += BlocksOf(CellsOf(P.level[d]), kCellTile);
      }
      for (int i = 0; i < child_levels; ++i) {
        first_oct[static_cast<size_t>(j) * child_levels + i] = static_cast<int>(oct_blocks);
        if (P.oct[i].cells)
          oct_blocks += BlocksOf(static_cast<long long>(P.oct[i].qx) * P.oct[i].qy * P.oct[i].qz,
                                 kOctTile);
      }
      h_problems[j] = P;
    }
    first_crop[2 * R] = static_cast<int>(crop_blocks);
    first_zero[V] = static_cast<int>(zero_blocks);
    first_scatter[2 * V] = static_cast<int>(scatter_blocks);
    for (int d = 1; d < depth; ++d)
      first_level[static_cast<size_t>(d - 1) * (n + 1) + n] = static_cast<int>(level_blocks[d]);
    first_oct[oct_entries] = static_cast<int>(oct_blocks);
    // The voxel lists into the one staging block (the pool's threads: a copy is memory bound).
    ParallelFor(2 * n, 2, [&](int item) {
      const Fast3DSource& src = sources[chain.begin + item / 2];
      if (src.resident || src.num_voxels[item & 1] == 0) return;
      memcpy(h_block + staged_at[item], src.voxels[item & 1],
             static_cast<size_t>(src.num_voxels[item & 1]) * sizeof(cmx_voxel));
    });
    stage_us += since(lap);
    lap = Clock::now();

    const StackProblem3D* d_problems = problems_in(d_block);
    SmallCopyAsync(d_block, h_block, block.bytes, /*to_device=*/true, stream);
    ++launches;
    if (crop_blocks > 0) {
      BatchCrop3DKernel<<<static_cast<unsigned>(crop_blocks), kBatchThreads, 0, stream>>>(
          d_problems, on_device(crop_of), on_device(first_crop), 2 * R);
      ++launches;
    }
    if (zero_blocks > 0) {
      BatchZero3DKernel<<<static_cast<unsigned>(zero_blocks), kBatchThreads, 0, stream>>>(
          d_problems, on_device(voxel_of), on_device(first_zero), V);
      ++launches;
    }
    if (scatter_blocks > 0) {
      BatchScatter3DKernel<<<static_cast<unsigned>(scatter_blocks), kBatchThreads, 0, stream>>>(
          d_problems, on_device(voxel_of), on_device(first_scatter), 2 * V);
      ++launches;
    }
    for (int d = 1; d < depth; ++d) {
      BatchLevel3DKernel<<<static_cast<unsigned>(level_blocks[d]), kBatchThreads, 0, stream>>>(
          d_problems, on_device(first_level + static_cast<size_t>(d - 1) * (n + 1)), n, d);
      ++launches;
    }
    if (oct_blocks > 0) {
      BatchOct3DKernel<<<static_cast<unsigned>(oct_blocks), kBatchThreads, 0, stream>>>(
          d_problems, on_device(first_oct), static_cast<int>(oct_entries), child_levels);
      ++launches;
    }
    CMX_HIP(hipGetLastError());
    issue_us += since(lap);
    lap = Clock::now();
    // (the lists are borrowed host memory, and the next chain reuses the staging block)
    CMX_HIP(hipStreamSynchronize(stream));
    wait_us += since(lap);
  }
  if (host_trace)
    fprintf(stderr,
            "[cmx host] fast3d_create_batch matchers=%d chains=%d launches=%d bounds=%.0f "
            "alloc=%.0f stage=%.0f issue=%.0f wait=%.0f\n",
            num, static_cast<int>(chains.size()), launches, bounds_us, alloc_us, stage_us,
            issue_us, wait_us);
  return matchers;
}

}  // namespace cmx

extern "C" {

cmx_status cmx_fast3d_create_batch(const cmx_fast3d_options* options,
                                   const cmx_fast3d_source* sources, int32_t num_sources,
                                   int32_t device, cmx_fast3d** out) {
  using namespace cmx;
  return Guard([&] {
    for (int k = 0; out && k < num_sources; ++k) out[k] = nullptr;
    CMX_REQUIRE(options && sources && out, "null argument");
    CMX_REQUIRE(num_sources >= 1, "num_sources %d < 1", num_sources);
    // Every check of the single creates, for every source, before the device is touched.
    std::vector<Fast3DSource> list(num_sources);
    auto checked = [](int k, const std::function<void()>& check) {
      try {
        check();
      } catch (const HipError&) {
        const std::string what = LastError();
        CMX_REQUIRE(false, "source %d: %s", k, what.c_str());
      }
    };
    checked(0, [&] { CheckFast3DOptions(*options); });
    for (int k = 0; k < num_sources; ++k) {
      const cmx_fast3d_source& s = sources[k];
      Fast3DSource& item = list[k];
      const bool grids = s.high_resolution_grid || s.low_resolution_grid;
      const bool lists = s.voxels || s.low_resolution_voxels;
      CMX_REQUIRE(!(grids && lists),
                  "source %d: more than one kind set (voxel lists and resident grids)", k);
      item.histogram = s.rotational_scan_matcher_histogram;
      item.histogram_size = s.histogram_size;
      if (grids) {
        item.resident = true;
        float resolution[2];
        int32_t grid_size = 0;
        int resident_on = device;
        checked(k, [&] {
          ResidentSource3D(s.high_resolution_grid, s.low_resolution_grid, item.histogram,
                           item.histogram_size, item.grid, resolution, &grid_size, &resident_on);
        });
        CMX_REQUIRE(resident_on == device,
                    "source %d: resident on device %d, the call builds on %d", k, resident_on,
                    device);
        item.resolution = resolution[0];
        item.low_resolution = resolution[1];
        item.width_in_voxels = grid_size;
      } else {
        // (no pointer at all is the voxel kind: the single create's empty case with both counts
        // 0; a source nobody filled in fails on its resolutions)
        checked(k, [&] {
          CMX_REQUIRE(s.num_voxels >= 0 && s.num_low_resolution_voxels >= 0, "negative count");
          CheckVoxelSource3D(s.resolution, s.voxels, s.num_voxels, s.low_resolution,
                             s.low_resolution_voxels, s.num_low_resolution_voxels,
                             item.histogram, item.histogram_size);
        });
        item.resolution = s.resolution;
        item.low_resolution = s.low_resolution;
        item.width_in_voxels = s.grid_size;
        item.voxels[0] = s.voxels;
        item.num_voxels[0] = s.num_voxels;
        item.voxels[1] = s.low_resolution_voxels;
        item.num_voxels[1] = s.num_low_resolution_voxels;
      }
    }
    // The passes over the lists (extent for the grid_size check, boxes) by the host pool.
    std::vector<int> needed(num_sources, 0);
    ParallelFor(num_sources, 2, [&](int k) {
      Fast3DSource& item = list[k];
      if (item.resident) return;
      for (int g = 0; g < 2; ++g)
        VoxelBoxOrOrigin(item.voxels[g], item.num_voxels[g], item.lo[g], item.hi[g]);
      needed[k] = GridSizeOf(item.voxels[0], item.num_voxels[0]);
    });
    for (int k = 0; k < num_sources; ++k)
      CMX_REQUIRE(list[k].resident || list[k].width_in_voxels >= needed[k],
                  "source %d: grid_size %d is smaller than the voxels' extent", k,
                  list[k].width_in_voxels);
    std::vector<std::unique_ptr<cmx_fast3d>> built =
        BuildFast3DBatch(*options, list.data(), num_sources, device);
    for (int k = 0; k < num_sources; ++k) out[k] = built[k].release();
  });
}

}  // extern "C"
