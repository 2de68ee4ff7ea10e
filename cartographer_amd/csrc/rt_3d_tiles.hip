// Real-time 3D matcher: the LDS-tiled bulk passes.
//
// The gathers of the bulk passes of rt_3d_bounds.hip go to memory one byte per lane: a wave's 64
// lookups of one point touch ~30 cache lines, and the L1's tag rate (~1 line per cycle and CU) is what bounds
// them (1.3e12 lookups/s, profiles/r03_gather_ceiling.txt).  But all lanes of a workgroup read
// the SAME point at the same time, displaced only by their translations (a window of a dozen
// cells) -- so for a spatially compact CHUNK of points everything a workgroup reads lies in a
// box of a few ten cells per axis.  The cloud is therefore sorted into bins of kTileBin^3 cells
// (counting sort on the device, integer sums do not care about the order) and cut into chunks
// of at most kTileChunk points; per chunk a workgroup
//   1. rotates the chunk by its rotation(s) into LDS (as before) and takes the bounding box of
//      the rotated points in cell coordinates (wave reductions + LDS atomics),
//   2. widens the box by the span of the translation table, copies that box of the brick into
//      LDS with aligned dword loads (row-major brick, pitch a multiple of 4),
//   3. runs the same lookup loop against the tile: ds_read_u8 instead of buffer_load_ubyte.
// A box that does not fit the tile capacity (a chunk of far points under a wide rotation
// block) takes the memory gathers for that chunk -- same arithmetic, same sums.  The integer
// sums are accumulated over chunk slices (blockIdx.y) with atomics; bounds come from
// Rt3DSumBoundsKernel / Rt3DBoundsKernel.  Every sum is identical to what Rt3DBulkKernel
// computes (debug switch rt3d_no_tiles runs that kernel; tests compare the two).
#include <algorithm>
#include <type_traits>

#include "rt_3d_internal.h"

namespace cmx {
namespace {

constexpr int kTileChunkGroups = 512;      // points per chunk, group pass (fewer, fuller work units)
constexpr int kTileChunkCandidates = 256;  // ... candidate pass (its f32 stage is 12 B per point and rotation)
constexpr int kTileBin = 24;

// Bin of a point: its cell at the central candidate (rotation index R/2, translation T/2).
struct Rt3DBinParams {
  float4 rotation, translation;
  float inv_resolution, off_x, off_y, off_z;
  float t0x, t0y, t0z, lo_x, hi_x, lo_y, hi_y, lo_z, hi_z;     // ClampStage
  int bins_x, bins_y, bins_z;
  int n;
};

__device__ __forceinline__ int Rt3DBinOf(const Rt3DBinParams& P, const float* __restrict__ xyz,
                                         int i) {
  const Quat q{P.rotation.w, P.rotation.x, P.rotation.y, P.rotation.z};
  const F3 rp = Rotate(q, F3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
  const float x = ClampStage(rp.x, P.t0x, P.lo_x, P.hi_x) + P.translation.x;
  const float y = ClampStage(rp.y, P.t0y, P.lo_y, P.hi_y) + P.translation.y;
  const float z = ClampStage(rp.z, P.t0z, P.lo_z, P.hi_z) + P.translation.z;
  // (NaN coordinates never get here: the bulk path requires finite points)
  const int cx = static_cast<int>(rintf(fmaf(x, P.inv_resolution, P.off_x)));
  const int cy = static_cast<int>(rintf(fmaf(y, P.inv_resolution, P.off_y)));
  const int cz = static_cast<int>(rintf(fmaf(z, P.inv_resolution, P.off_z)));
  const int bx = min(max(cx / kTileBin, 0), P.bins_x - 1);
  const int by = min(max(cy / kTileBin, 0), P.bins_y - 1);
  const int bz = min(max(cz / kTileBin, 0), P.bins_z - 1);
  return (bz * P.bins_y + by) * P.bins_x + bx;
}

// counters[bin] += (lanes of this wave with that bin); returns the lane's own slot.  Scan order
// puts neighbouring points into the same bin, so a wave needs one or two atomics.
__device__ __forceinline__ int WaveAggregatedAdd(int* __restrict__ counters, int bin, bool active) {
  const int lane = threadIdx.x & 63;
  int slot = 0;
  for (;;) {
    const unsigned long long todo = __ballot(active);
    if (todo == 0ull) break;
    const int leader = __ffsll(static_cast<long long>(todo)) - 1;
    const int leader_bin = __shfl(bin, leader, 64);
    const bool mine = active && bin == leader_bin;
    const unsigned long long group = __ballot(mine);
    int base = 0;
    if (lane == leader) base = atomicAdd(&counters[leader_bin], __popcll(group));
    base = __shfl(base, leader, 64);
    if (mine) {
      slot = base + __popcll(group & ((1ull << lane) - 1ull));
      active = false;
    }
  }
  return slot;
}

__global__ void Rt3DBinCountKernel(Rt3DBinParams P, const float* __restrict__ xyz,
                                   int* __restrict__ bin_count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < P.n;
  const int bin = active ? Rt3DBinOf(P, xyz, i) : 0;
  (void)WaveAggregatedAdd(bin_count, bin, active);
}

// Point segments of the staged candidate pass ("Staged candidate pass", rt_3d_bounds.hip): the
// cloud is cut into three parts -- about a quarter, a quarter and a half of the points -- that BOTH chunk
// lists respect, so that the group pass can report a group's sum over each part and the
// candidate pass can stop after the first or the second.  The unit is a group-pass piece (at
// most kTileChunkGroups points of one bin; the candidate pass's pieces are its halves): a
// piece belongs to the segment its midpoint falls into on the axis of bin-sorted point
// indices, which is cut into windows of `window` points -- first quarter of a window: segment
// 0, second quarter: 1, rest: 2.  Any assignment is correct; this one keeps the parts close to
// their nominal sizes whatever the bins hold and interleaves them through the volume.
__device__ __forceinline__ int Rt3DSegmentOf(int first_point, int length, int window, int end0,
                                             int end1) {
  const int at = (first_point + (length >> 1)) & (window - 1);       // window: a power of two
  return at < end0 ? 0 : at < end1 ? 1 : 2;          // (end0, end1: window / 4, window / 2)
}

// One workgroup: exclusive scan of the bin counts -> first point of every bin (written over the
// counts: the scatter kernel's cursors) and the two chunk lists (pieces of at most
// kTileChunkGroups / kTileChunkCandidates points of one bin), each ordered by segment:
// num_chunks[0 / 1] = pieces of the group / candidate list, [2], [3] = where segments 1 and 2
// of the group list begin, [4], [5] = the same for the candidate list.
__global__ void __launch_bounds__(1024)
Rt3DBinScanKernel(int* __restrict__ bin_count, int num_bins, int2* __restrict__ chunks_groups,
                  int2* __restrict__ chunks_candidates, int* __restrict__ num_chunks,
                  int window, int end0, int end1) {
  static_assert(kTileChunkGroups == 2 * kTileChunkCandidates, "candidate pieces are halves");
  __shared__ int part_points[1024], part_a[3][1024], part_b[3][1024];
  __shared__ int seg_base_a[3], seg_base_b[3];
  const int tid = threadIdx.x;
  const int per = (num_bins + 1023) / 1024;
  const int begin = min(tid * per, num_bins), end = min(begin + per, num_bins);
  // pass 1: points per thread (the segment of a piece depends on its first point)
  int points = 0;
  for (int b = begin; b < end; ++b) points += bin_count[b];
  part_points[tid] = points;
  __syncthreads();
  if (tid == 0) {
    int p = 0;
    for (int k = 0; k < 1024; ++k) {
      const int pp = part_points[k];
      part_points[k] = p;
      p += pp;
    }
  }
  __syncthreads();
  // pass 2: pieces per segment
  int na[3] = {0, 0, 0}, nb[3] = {0, 0, 0};
  {
    int p = part_points[tid];
    for (int b = begin; b < end; ++b) {
      const int count = bin_count[b];
      for (int first = 0; first < count; first += kTileChunkGroups) {
        const int len = min(kTileChunkGroups, count - first);
        const int seg = Rt3DSegmentOf(p + first, len, window, end0, end1);
        const int halves = (len + kTileChunkCandidates - 1) / kTileChunkCandidates;
        if (seg == 0) { na[0] += 1; nb[0] += halves; }
        else if (seg == 1) { na[1] += 1; nb[1] += halves; }
        else { na[2] += 1; nb[2] += halves; }
      }
      p += count;
    }
  }
#pragma unroll
  for (int g = 0; g < 3; ++g) { part_a[g][tid] = na[g]; part_b[g][tid] = nb[g]; }
  __syncthreads();
  if (tid < 6) {                           // six independent serial scans
    int* part = tid < 3 ? part_a[tid] : part_b[tid - 3];
    int run = 0;
    for (int k = 0; k < 1024; ++k) {
      const int v = part[k];
      part[k] = run;
      run += v;
    }
    (tid < 3 ? seg_base_a : seg_base_b)[tid % 3] = run;       // totals, turned into bases below
  }
  __syncthreads();
  if (tid == 0) {
    const int a0 = seg_base_a[0], a1 = seg_base_a[1], a2 = seg_base_a[2];
    const int b0 = seg_base_b[0], b1 = seg_base_b[1], b2 = seg_base_b[2];
    seg_base_a[0] = 0; seg_base_a[1] = a0; seg_base_a[2] = a0 + a1;
    seg_base_b[0] = 0; seg_base_b[1] = b0; seg_base_b[2] = b0 + b1;
    num_chunks[0] = a0 + a1 + a2;
    num_chunks[1] = b0 + b1 + b2;
    num_chunks[2] = a0; num_chunks[3] = a0 + a1;
    num_chunks[4] = b0; num_chunks[5] = b0 + b1;
  }
  __syncthreads();
  // pass 3: the lists
  int ca[3], cb[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    ca[g] = seg_base_a[g] + part_a[g][tid];
    cb[g] = seg_base_b[g] + part_b[g][tid];
  }
  int p = part_points[tid];
  for (int b = begin; b < end; ++b) {
    const int count = bin_count[b];
    bin_count[b] = p;
    for (int first = 0; first < count; first += kTileChunkGroups) {
      const int len = min(kTileChunkGroups, count - first);
      const int seg = Rt3DSegmentOf(p + first, len, window, end0, end1);
      // (static selects: no dynamically indexed private array)
      int at_a = seg == 0 ? ca[0] : seg == 1 ? ca[1] : ca[2];
      int at_b = seg == 0 ? cb[0] : seg == 1 ? cb[1] : cb[2];
      chunks_groups[at_a++] = make_int2(p + first, len);
      for (int half = 0; half < len; half += kTileChunkCandidates)
        chunks_candidates[at_b++] =
            make_int2(p + first + half, min(kTileChunkCandidates, len - half));
      if (seg == 0) { ca[0] = at_a; cb[0] = at_b; }
      else if (seg == 1) { ca[1] = at_a; cb[1] = at_b; }
      else { ca[2] = at_a; cb[2] = at_b; }
    }
    p += count;
  }
}

__global__ void Rt3DBinScatterKernel(Rt3DBinParams P, const float* __restrict__ xyz,
                                     int* __restrict__ cursor, float* __restrict__ sorted) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < P.n;
  const int bin = active ? Rt3DBinOf(P, xyz, i) : 0;
  const int slot = WaveAggregatedAdd(cursor, bin, active);
  if (active) {
    sorted[3 * slot] = xyz[3 * i];
    sorted[3 * slot + 1] = xyz[3 * i + 1];
    sorted[3 * slot + 2] = xyz[3 * i + 2];
  }
}

// Bounding boxes of the rotated chunks, once per match: box[(block, chunk)] = min x, y, z, max
// x, y, z over the chunk's points rotated by every rotation of rotation block `block`
// (`rotations_per_block` consecutive rotations), clamped like the staged points, in cells
// (coordinate * inv_resolution; no offset, no translation).  grid (rotation blocks, chunk
// slices), 256 threads: ONE WAVE per chunk (no workgroup barrier, no LDS: a block per chunk
// with an LDS reduction cost 0.5 ms per match).
__global__ void __launch_bounds__(256)
Rt3DChunkBoxKernel(Rt3DBulkParams P, const float* __restrict__ sorted_xyz,
                   const int2* __restrict__ chunks, const int* __restrict__ num_chunks,
                   int rotations_per_block, float* __restrict__ boxes) {
  const int block = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rotation_a = block * rotations_per_block;
  const int num_rot = min(rotations_per_block, P.num_rotations - rotation_a);
  const int total = *num_chunks;
  for (int chunk = blockIdx.y * 4 + wave; chunk < total; chunk += gridDim.y * 4) {
    const int2 span = chunks[chunk];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = lane; k < span.y; k += 64) {
      const int i = span.x + k;
      const F3 p{sorted_xyz[3 * i], sorted_xyz[3 * i + 1], sorted_xyz[3 * i + 2]};
      for (int w = 0; w < num_rot; ++w) {
        const float4 q4 = P.rotation[rotation_a + w];
        const F3 rp = Rotate(Quat{q4.w, q4.x, q4.y, q4.z}, p);
        const float c[3] = {ClampStage(rp.x, P.t0x, P.lo_x, P.hi_x) * P.inv_resolution,
                            ClampStage(rp.y, P.t0y, P.lo_y, P.hi_y) * P.inv_resolution,
                            ClampStage(rp.z, P.t0z, P.lo_z, P.hi_z) * P.inv_resolution};
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], c[a]); mx[a] = fmaxf(mx[a], c[a]); }
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        mn[a] = fminf(mn[a], __shfl_xor(mn[a], off, 64));
        mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off, 64));
      }
    }
    if (lane < 6) {
      const float v = lane == 0 ? mn[0] : lane == 1 ? mn[1] : lane == 2 ? mn[2]
                      : lane == 3 ? mx[0] : lane == 4 ? mx[1] : mx[2];
      boxes[(static_cast<size_t>(block) * total + chunk) * 6 + lane] = v;
    }
  }
}

typedef unsigned uint4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void LdsRead128Asm(uint4v* out, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1" : "=v"(*out) : "v"(addr));
}
__device__ __forceinline__ void LdsReadU8Asm(unsigned* out, unsigned addr) {
  asm volatile("ds_read_u8 %0, %1" : "=v"(*out) : "v"(addr));
}

// Dynamic LDS of Rt3DTileKernel<kGroups, kLists>, in this order:
//   tile (tile_capacity bytes) | staged points, kStageStride v2f per rotation | (group pass) the
//   points again as packed fixed-point words, kPackedWords per rotation | box (six ints).
// The kernel lays its pointers out from these constants and every launch sizes its LDS by Bytes():
// the box lies behind everything else, so a size that falls short of the layout is a fault.
template <bool kGroups, bool kLists>
struct Rt3DTileLds {
  static constexpr int kChunk = kLists ? kTileChunkCandidates : kTileChunkGroups;
  static constexpr int kStageStride = 3 * kChunk / 2 + 2;   // v2f per staged rotation (+16 B: bank shift)
  static constexpr int kPackedWords = kGroups ? kChunk : 0;
  static constexpr int kBoxBytes = 32;
  static constexpr size_t Bytes(int rotations, int tile_capacity) {
    return (sizeof(v2f) * kStageStride + sizeof(uint32_t) * kPackedWords) * rotations +
           tile_capacity + kBoxBytes;
  }
};
// ... at the shipped parameters: 2 and 8 rotations, tiles of 44 and 48 KiB.
constexpr bool TileLdsIs(int rot, int cap) {
  return Rt3DTileLds<true, false>::Bytes(rot, cap) ==
             static_cast<size_t>((8 * (3 * 512 / 2 + 2) + 4 * 512) * rot + cap + 32) &&
         Rt3DTileLds<true, true>::Bytes(rot, cap) ==
             static_cast<size_t>((8 * (3 * 256 / 2 + 2) + 4 * 256) * rot + cap + 32) &&
         Rt3DTileLds<false, true>::Bytes(rot, cap) ==
             static_cast<size_t>(8 * (3 * 256 / 2 + 2) * rot + cap + 32);
}
static_assert(TileLdsIs(2, 44 * 1024) && TileLdsIs(8, 44 * 1024) && TileLdsIs(2, 48 * 1024) &&
                  TileLdsIs(8, 48 * 1024),
              "dynamic LDS of the three tile kernels");

// kGroups: grid (ceil(R / rotations_per_block), chunk slices), blockDim = the (rotation, group)
// lanes of a block rounded up to whole waves.  Candidate pass: grid (work descriptors, chunk
// slices), blockDim = block_items.  Dynamic LDS: Rt3DTileLds.
// kGroups: the arithmetic of the group pass (centre lookups in a dilated brick: fixed-point
// words, no ambiguity bookkeeping, sums by segment).  kLists: lanes are entries of work lists over
// P.list_rotations rotations (Rt3DCompactKernel) instead of all (rotation, translation) pairs of
// TP.rotations_per_block rotations.  <true, false>: the dense group pass (and the rotation-block
// pass above it); <true, true>: the group pass over the (rotation, group) pairs a rotation-block
// bound could not exclude; <false, true>: the candidate passes.
template <bool kGroups, bool kLists>
__global__ void __launch_bounds__(1024)
Rt3DTileKernel(Rt3DBulkParams P, Rt3DTileParams TP) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tile_smem[];
  static_assert(kGroups || kLists, "candidates always come from work lists");
  using Lds = Rt3DTileLds<kGroups, kLists>;
  constexpr int kChunk = Lds::kChunk, kStageStride = Lds::kStageStride;
  const int tid = threadIdx.x;
  const int rotations = kLists ? P.list_rotations : TP.rotations_per_block;
  // Dynamic LDS: tile | staged points | (group pass) the points again as packed fixed-point
  // words, see step 2b.  The tile comes first: its LDS address is then a compile-time constant
  // that folds into the gathers' offset field.
  uint8_t* const tile = tile_smem;
  if (static_cast<unsigned>(reinterpret_cast<uintptr_t>(tile)) != 0u) __builtin_trap();
  v2f* const stage = reinterpret_cast<v2f*>(tile_smem + TP.tile_capacity);
  uint32_t* const packed = reinterpret_cast<uint32_t*>(stage + kStageStride * rotations);
  // min x, y, z, max x, y, z of the rotated chunk (cells).  (No static __shared__ in this kernel:
  // the tile then starts at LDS address 0 and the gathers need no base.)
  int* const box = reinterpret_cast<int*>(packed + Lds::kPackedWords * rotations);

  int r, t, rotation_a, num_rot;
  bool valid;
  if (!kLists) {
    rotation_a = blockIdx.x * rotations;
    num_rot = min(rotations, P.num_rotations - rotation_a);
    const int item = tid;
    valid = item < num_rot * P.num_translations;
    const int which = valid ? item / P.num_translations : 0;
    r = rotation_a + which;
    t = valid ? item - which * P.num_translations : 0;
  } else {
    const int2 work = P.blocks[blockIdx.x];
    const int list = work.x;
    rotation_a = list * P.list_rotations;
    num_rot = min(P.list_rotations, P.num_rotations - rotation_a);
    const int count = P.counts[list];
    const int slot = work.y * TP.block_items + tid;
    valid = slot < count;
    if (work.y * TP.block_items >= count) return;
    const int entry = P.items[static_cast<size_t>(list) * P.list_rotations * P.num_translations +
                              (valid ? slot : count - 1)];
    const int w = entry / P.num_translations;
    t = entry - w * P.num_translations;
    r = rotation_a + w;
  }
  const v2f* const my_stage = stage + (r - rotation_a) * kStageStride;
  const float4 tr = P.translation[t];
  const v2f trx = {tr.x, tr.x}, try_ = {tr.y, tr.y}, trz = {tr.z, tr.z};
  const v2f inv = {P.inv_resolution, P.inv_resolution};
  const v2f ofx = {P.off_x, P.off_x}, ofy = {P.off_y, P.off_y}, ofz = {P.off_z, P.off_z};
  const float guard = P.guard;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(P.cells), 0, P.cell_count, 0x00020000);
  unsigned acc = 0, ambiguous = 0;
  const int num_chunks = *TP.num_chunks;
  // the chunks of this pass: all of them, or the segments seg_first .. seg_last of the list
  int chunk_begin = 0, chunk_end = num_chunks, split0 = num_chunks, split1 = num_chunks;
  if (TP.seg_bounds != nullptr) {
    split0 = TP.seg_bounds[0];
    split1 = TP.seg_bounds[1];
    chunk_begin = TP.seg_first <= 0 ? 0 : TP.seg_first == 1 ? split0 : split1;
    chunk_end = TP.seg_last >= 2 ? num_chunks : TP.seg_last == 1 ? split1 : split0;
  }
  unsigned acc_seen = 0, acc_seg0 = 0, acc_seg1 = 0;     // group pass: the total by segment
  // Fixed-point group pass.  The centre of a group needs no exact cell: its lookup in the
  // 3 x 3 x 3-dilated brick covers the members as long as the cell it reads is the cell of a
  // point within 1 - 0.87 = 0.13 cells (per axis) of the true centre.  So cell coordinates are
  // kept in 1/16 cells: 10 bits per axis, three axes in one word, tile-relative.  The point
  // word (built once per chunk and rotation) carries + 0.5 for the rounding, the lane word
  // (built once) the translation above the table's minimum; ONE integer add then yields all
  // three cell indices -- against 3 + 3 packed f32 operations and six roundings.  Error: both
  // words are rounded to 1/32 cell: 1/16 in total (+ 1e-5 of f32 arithmetic) < 0.13.
  constexpr int kFrac = 4;
  unsigned lane_word = 0;
  if (kGroups) {
    const float s = static_cast<float>(1 << kFrac);
    const unsigned tx = static_cast<unsigned>(rintf((tr.x * P.inv_resolution - TP.tr_lo[0]) * s));
    const unsigned ty = static_cast<unsigned>(rintf((tr.y * P.inv_resolution - TP.tr_lo[1]) * s));
    const unsigned tz = static_cast<unsigned>(rintf((tr.z * P.inv_resolution - TP.tr_lo[2]) * s));
    lane_word = tx | (ty << 10) | (tz << 20);
  }

  for (int chunk = chunk_begin + blockIdx.y; chunk < chunk_end; chunk += gridDim.y) {
    const int2 span = TP.chunks[chunk];
    const int len = span.y;
    if (kGroups) {
      // what the previous chunk added belongs to that chunk's segment (chunks ascend; lanes that
      // skip the lookups add nothing)
      const int previous = chunk - static_cast<int>(gridDim.y);
      const unsigned added = acc - acc_seen;
      acc_seen = acc;
      if (previous < split0) acc_seg0 += added;
      else if (previous < split1) acc_seg1 += added;
    }
    __syncthreads();                                     // the previous chunk is done with
    const bool have_box = TP.boxes != nullptr;
    if (have_box) {
      // The box comes from the pre-pass: no reduction, no barrier, and the points are rotated
      // ONCE, straight into the form the lookups read (step 2c).
      if (tid < 6) {
        const int block_index = kLists ? rotation_a / rotations : static_cast<int>(blockIdx.x);
        const float v = TP.boxes[(static_cast<size_t>(block_index) * num_chunks + chunk) * 6 + tid];
        const float offs[3] = {P.off_x, P.off_y, P.off_z};
        box[tid] = tid < 3 ? static_cast<int>(floorf(v + TP.tr_lo[tid] + offs[tid])) - 1
                           : static_cast<int>(ceilf(v + TP.tr_hi[tid - 3] + offs[tid - 3])) + 1;
      }
    } else {
    if (tid < 3) box[tid] = 0x7fffffff;
    else if (tid < 6) box[tid] = -0x7fffffff;
    __syncthreads();
    // 1. rotate the chunk by every rotation of the block; bounding box in cell coordinates
    {
      float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
      const int len_even = (len + 1) & ~1;               // (an odd chunk's pair partner is defined)
      for (int s = tid; s < num_rot * kChunk; s += blockDim.x) {
        const int w = s / kChunk, k = s % kChunk;      // (a power of two: shifts)
        if (k >= len_even) continue;
        const int i = span.x + min(k, len - 1);
        const float4 q4 = P.rotation[rotation_a + w];
        const F3 rp = Rotate(Quat{q4.w, q4.x, q4.y, q4.z},
                             F3{TP.sorted_xyz[3 * i], TP.sorted_xyz[3 * i + 1],
                                TP.sorted_xyz[3 * i + 2]});
        const float x = ClampStage(rp.x, P.t0x, P.lo_x, P.hi_x);
        const float y = ClampStage(rp.y, P.t0y, P.lo_y, P.hi_y);
        const float z = ClampStage(rp.z, P.t0z, P.lo_z, P.hi_z);
        float* dst = reinterpret_cast<float*>(stage + w * kStageStride) + 6 * (k >> 1) + (k & 1);
        dst[0] = x; dst[2] = y; dst[4] = z;
        const float c[3] = {x * P.inv_resolution, y * P.inv_resolution, z * P.inv_resolution};
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], c[a]); mx[a] = fmaxf(mx[a], c[a]); }
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          mn[a] = fminf(mn[a], __shfl_xor(mn[a], off, 64));
          mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off, 64));
        }
      }
      if ((tid & 63) == 0 && mn[0] <= mx[0]) {
        const float offs[3] = {P.off_x, P.off_y, P.off_z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          // one cell of slack either side: the lookups round (c + tr) * inv + off, not this sum
          atomicMin(&box[a], static_cast<int>(floorf(mn[a] + TP.tr_lo[a] + offs[a])) - 1);
          atomicMax(&box[3 + a], static_cast<int>(ceilf(mx[a] + TP.tr_hi[a] + offs[a])) + 1);
        }
      }
    }
    }
    __syncthreads();
    // 2. the box, clipped to the brick (ClampStage keeps every lookup inside it), x aligned to 4
    const int lo_x = max(box[0], 0) & ~3, lo_y = max(box[1], 0), lo_z = max(box[2], 0);
    const int hi_x = min(box[3], TP.pitch_x - 1), hi_y = min(box[4], TP.pitch_y - 1),
              hi_z = min(box[5], TP.pitch_z - 1);
    const int dx = (hi_x - lo_x + 4) & ~3, dy = hi_y - lo_y + 1, dz = hi_z - lo_z + 1;
    // (a wave's DMA instruction writes 256 bytes: the last one may run past the box's end)
    const bool in_lds = dx > 0 && dx <= 256 && dy > 0 && dz > 0 &&
                        static_cast<long long>(dx) * dy * dz + 256 <= TP.tile_capacity;
    if (in_lds) {
      // The box enters LDS by LDS-DMA (global_load_lds_dword: lane l of a wave writes base + 4 l,
      // no registers, all loads of a wave in flight at once; ordered by vmcnt(0) + the barrier
      // below): dword e = row * (dx / 4) + xq of the tile, row = z * dy + y; the two divisions
      // through 2^32 reciprocals (exact: e, row < 2^16).  The rotation pass (2c) runs meanwhile.
      const unsigned qx = dx >> 2, total = qx * dy * dz;
      const unsigned rq = static_cast<unsigned>((1ull << 32) / qx) + 1u;
      const unsigned ry = static_cast<unsigned>((1ull << 32) / static_cast<unsigned>(dy)) + 1u;
      const unsigned row_q = TP.pitch_x >> 2, slice_q = TP.pitch_y * row_q;
      const uint32_t* base = reinterpret_cast<const uint32_t*>(P.cells) +
                             (static_cast<size_t>(lo_z) * TP.pitch_y + lo_y) * row_q + (lo_x >> 2);
      const unsigned wave_first = __builtin_amdgcn_readfirstlane(tid & ~63);
      auto* dst = (__attribute__((address_space(3))) unsigned char*)tile;
      for (unsigned first = wave_first; first < total; first += blockDim.x) {
        const unsigned e = min(first + (tid & 63), total - 1);       // (the tail re-reads the last dword)
        const unsigned row = qx == 1 ? e : __umulhi(e, rq);
        const unsigned xq = e - row * qx;
        const unsigned z = dy == 1 ? row : __umulhi(row, ry);
        const unsigned y = row - z * dy;
        const auto* src = (const __attribute__((address_space(1))) unsigned char*)(
            base + (z * slice_q + y * row_q + xq));
        __builtin_amdgcn_global_load_lds(src, dst + 4 * first, 4, 0, 0);
      }
    }
    // 2b. group pass: the staged points as fixed-point words relative to the tile
    const bool fixed = kGroups && TP.fixed_point && in_lds && dx <= 63 && dy <= 63 && dz <= 63;
    if (fixed && !have_box) {
      const float s = static_cast<float>(1 << kFrac);
      const float bx = P.off_x + TP.tr_lo[0] - static_cast<float>(lo_x) + 0.5f;
      const float by = P.off_y + TP.tr_lo[1] - static_cast<float>(lo_y) + 0.5f;
      const float bz = P.off_z + TP.tr_lo[2] - static_cast<float>(lo_z) + 0.5f;
      const int len_even = (len + 1) & ~1;
      for (int e = tid; e < num_rot * kChunk; e += blockDim.x) {
        const int w = e / kChunk, k = e % kChunk;
        if (k >= len_even) continue;
        const float* src = reinterpret_cast<const float*>(stage + w * kStageStride) +
                           6 * (k >> 1) + (k & 1);
        const unsigned px = static_cast<unsigned>(rintf(fmaf(src[0], P.inv_resolution, bx) * s));
        const unsigned py = static_cast<unsigned>(rintf(fmaf(src[2], P.inv_resolution, by) * s));
        const unsigned pz = static_cast<unsigned>(rintf(fmaf(src[4], P.inv_resolution, bz) * s));
        packed[w * kChunk + k] = px | (py << 10) | (pz << 20);
      }
    }
    // 2c. with the box from the pre-pass: ONE rotation pass, into fixed-point words or f32 triples
    if (have_box) {
      const float s = static_cast<float>(1 << kFrac);
      const float bx = P.off_x + TP.tr_lo[0] - static_cast<float>(lo_x) + 0.5f;
      const float by = P.off_y + TP.tr_lo[1] - static_cast<float>(lo_y) + 0.5f;
      const float bz = P.off_z + TP.tr_lo[2] - static_cast<float>(lo_z) + 0.5f;
      const int len_even = (len + 1) & ~1;
      for (int e = tid; e < num_rot * kChunk; e += blockDim.x) {
        const int w = e / kChunk, k = e % kChunk;
        if (k >= len_even) continue;
        const int i = span.x + min(k, len - 1);
        const float4 q4 = P.rotation[rotation_a + w];
        const F3 rp = Rotate(Quat{q4.w, q4.x, q4.y, q4.z},
                             F3{TP.sorted_xyz[3 * i], TP.sorted_xyz[3 * i + 1],
                                TP.sorted_xyz[3 * i + 2]});
        const float x = ClampStage(rp.x, P.t0x, P.lo_x, P.hi_x);
        const float y = ClampStage(rp.y, P.t0y, P.lo_y, P.hi_y);
        const float z = ClampStage(rp.z, P.t0z, P.lo_z, P.hi_z);
        if (fixed) {
          const unsigned px = static_cast<unsigned>(rintf(fmaf(x, P.inv_resolution, bx) * s));
          const unsigned py = static_cast<unsigned>(rintf(fmaf(y, P.inv_resolution, by) * s));
          const unsigned pz = static_cast<unsigned>(rintf(fmaf(z, P.inv_resolution, bz) * s));
          packed[w * kChunk + k] = px | (py << 10) | (pz << 20);
        } else {
          float* dst = reinterpret_cast<float*>(stage + w * kStageStride) + 6 * (k >> 1) + (k & 1);
          dst[0] = x; dst[2] = y; dst[4] = z;
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's LDS-DMA has landed
    __syncthreads();
    if (TP.stats != nullptr && tid == 0) {
      atomicAdd(&TP.stats[in_lds ? 0 : 1], 1ull);
      atomicAdd(&TP.stats[2], static_cast<unsigned long long>(dx) * dy * dz);
      atomicAdd(&TP.stats[3], static_cast<unsigned long long>(len));
    }
    if (!valid) continue;
    // 3. the lookups.  Cell indices are computed exactly as in Rt3DBulkKernel (the candidate
    //    pass's ambiguity argument rests on that expression); only the address differs.
    const v2f lx = {static_cast<float>(lo_x), static_cast<float>(lo_x)};
    const v2f ly = {static_cast<float>(lo_y), static_cast<float>(lo_y)};
    const v2f lz = {static_cast<float>(lo_z), static_cast<float>(lo_z)};
    const v2f dxf = {static_cast<float>(dx), static_cast<float>(dx)};
    const v2f dyf = {static_cast<float>(dy), static_cast<float>(dy)};
    const v2f px2 = {static_cast<float>(TP.pitch_x), static_cast<float>(TP.pitch_x)};
    const v2f py2 = {static_cast<float>(TP.pitch_y), static_cast<float>(TP.pitch_y)};
    // One pair of points (already in registers) -> two lookups.  kLds is a compile-time
    // property of the loop it runs in: the two address paths never share a loop body.
    const auto pair = [&](auto lds_tag, const v2f* pr, unsigned* v0, unsigned* v1, float* g) {
      constexpr bool kLds = decltype(lds_tag)::value;
      const v2f cx = pr[0] + trx, cy = pr[1] + try_, cz = pr[2] + trz;
      const v2f qx = __builtin_elementwise_fma(cx, inv, ofx);
      const v2f qy = __builtin_elementwise_fma(cy, inv, ofy);
      const v2f qz = __builtin_elementwise_fma(cz, inv, ofz);
      const v2f nx = {rintf(qx.x), rintf(qx.y)};
      const v2f ny = {rintf(qy.x), rintf(qy.y)};
      const v2f nz = {rintf(qz.x), rintf(qz.y)};
      if (!kGroups) {
        const v2f ex = qx - nx, ey = qy - ny, ez = qz - nz;
        float m = fmaxf(fmaxf(*g, fabsf(ex.x)), fabsf(ex.y));
        m = fmaxf(fmaxf(m, fabsf(ey.x)), fabsf(ey.y));
        *g = fmaxf(fmaxf(m, fabsf(ez.x)), fabsf(ez.y));
      }
      if (kLds) {
        const v2f o = __builtin_elementwise_fma(
            __builtin_elementwise_fma(nz - lz, dyf, ny - ly), dxf, nx - lx);
        *v0 = tile[static_cast<unsigned>(o.x)];
        *v1 = tile[static_cast<unsigned>(o.y)];
      } else {
        const v2f o = __builtin_elementwise_fma(__builtin_elementwise_fma(nz, py2, ny), px2, nx);
        *v0 = __builtin_amdgcn_raw_buffer_load_b8(rsrc, static_cast<unsigned>(o.x), 0, 0);
        *v1 = __builtin_amdgcn_raw_buffer_load_b8(rsrc, static_cast<unsigned>(o.y), 0, 0);
      }
    };
    const int len4 = len & ~3;
    // LDS returns in issue order: a wait for point data also waits for every gather issued
    // before that read.  So the points of iteration j + 1 are requested BEFORE the gathers of
    // iteration j are issued, and the gathers of iteration j are consumed in iteration j + 1:
    // every wait is for something issued a whole iteration earlier.
    const auto run = [&](auto lds_tag) {
      unsigned p0 = 0, p1 = 0, p2 = 0, p3 = 0;          // the previous four lookups, in flight
      v2f cur[6], nxt[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) cur[k] = my_stage[k];
#pragma unroll 2
      for (int j = 0; j < len4; j += 4) {
        const v2f* ahead = my_stage + 3 * (min(j + 4, kChunk - 4) >> 1);
#pragma unroll
        for (int k = 0; k < 6; ++k) nxt[k] = ahead[k];
        unsigned v[4];
        float g = 0.f;
        pair(lds_tag, cur, &v[0], &v[1], &g);
        pair(lds_tag, cur + 3, &v[2], &v[3], &g);
        if (!kGroups) ambiguous += g > guard ? 1u : 0u;
        acc += (p0 + p1) + (p2 + p3);
        p0 = v[0]; p1 = v[1]; p2 = v[2]; p3 = v[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) cur[k] = nxt[k];
      }
      acc += (p0 + p1) + (p2 + p3);
      // the last 1..3 points: pairs whose second element may lie beyond the chunk (an odd
      // chunk staged its last point twice; the duplicate can only flag an ambiguity its twin
      // flags as well)
      for (int j = len4; j < len; j += 2) {
        unsigned v0, v1;
        float g = 0.f;
        pair(lds_tag, my_stage + 3 * (j >> 1), &v0, &v1, &g);
        acc += v0 + (j + 1 < len ? v1 : 0u);
        if (!kGroups) ambiguous += g > guard ? 1u : 0u;
      }
    };
    if (fixed) {
      const uint32_t* __restrict__ words = packed + (r - rotation_a) * kChunk;
      const unsigned udx = dx, udy = dy;
      const auto cell = [&](unsigned point_word) -> unsigned {
        const unsigned sum = point_word + lane_word;
        const unsigned x = (sum >> kFrac) & 63u, y = (sum >> (10 + kFrac)) & 63u,
                       z = sum >> (20 + kFrac);
        unsigned row, at;
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(row) : "v"(z), "s"(udy), "v"(y));
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(at) : "v"(row), "s"(udx), "v"(x));
        // (the tile starts at LDS address 0, checked at kernel entry: `at` IS the address)
        typedef __attribute__((address_space(3))) const uint8_t LdsByte;
        return *reinterpret_cast<LdsByte*>(static_cast<uintptr_t>(at));
      };
      // Hand-scheduled (as the window loop of rt_2d.hip): the compiler's version of this loop kept
      // four register copies per four lookups (its unroll-by-two failed) and loaded the next
      // point words right before their use -- an LDS round trip exposed in every iteration of
      // the pass the match spends half its time in.  Eight lookups per iteration in two halves
      // A and B.  LDS operations are issued in the order  A x 4, W0', B x 4, Wb'  (W': the point
      // words of the NEXT iteration) and return in issue order, so every wait names exactly how
      // many later operations may still be pending: A's gathers and the word loads land under
      // B's address arithmetic, B's gathers under the next iteration's A addresses.  Every
      // asynchronous result is waited for before the loop's back edge -- what crosses it (the A
      // addresses, the B words) are ordinary values the compiler may copy as it likes -- and the
      // waits carry the registers they release as in/out operands, which pins the consuming
      // arithmetic behind them.
      const auto address = [&](unsigned point_word) -> unsigned {
        const unsigned sum = point_word + lane_word;
        const unsigned x = (sum >> kFrac) & 63u, y = (sum >> (10 + kFrac)) & 63u,
                       z = sum >> (20 + kFrac);
        unsigned row, at;
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(row) : "v"(z), "s"(udy), "v"(y));
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(at) : "v"(row), "s"(udx), "v"(x));
        return at;
      };
      const int len8 = len & ~7;
      if (len8 > 0) {
        const unsigned wbase = static_cast<unsigned>(reinterpret_cast<uintptr_t>(
            (const __attribute__((address_space(3))) uint32_t*)words));
        uint4v Wa, Wb;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // nothing of the compiler's pending
        LdsRead128Asm(&Wa, wbase);
        LdsRead128Asm(&Wb, wbase + 16);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(Wa), "+v"(Wb));
        unsigned a0 = address(Wa.x), a1 = address(Wa.y), a2 = address(Wa.z), a3 = address(Wa.w);
        for (int j = 0; j < len8; j += 8) {
          const unsigned next = wbase + 4u * static_cast<unsigned>(min(j + 8, kChunk - 8));
          unsigned A0, A1, A2, A3, B0, B1, B2, B3;
          uint4v W0;
          LdsReadU8Asm(&A0, a0); LdsReadU8Asm(&A1, a1); LdsReadU8Asm(&A2, a2); LdsReadU8Asm(&A3, a3);
          LdsRead128Asm(&W0, next);
          const unsigned b0 = address(Wb.x), b1 = address(Wb.y), b2 = address(Wb.z),
                         b3 = address(Wb.w);
          LdsReadU8Asm(&B0, b0); LdsReadU8Asm(&B1, b1); LdsReadU8Asm(&B2, b2); LdsReadU8Asm(&B3, b3);
          // (Wb's words have been turned into addresses: the next ones go straight into it)
          asm volatile("ds_read_b128 %0, %1 offset:16" : "=v"(Wb) : "v"(next));
          asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(A0), "+v"(A1), "+v"(A2), "+v"(A3));   // after A: W0', B x 4, Wb'
          acc += (A0 + A1) + (A2 + A3);
          asm volatile("s_waitcnt lgkmcnt(5)" : "+v"(W0));                                  // after W0': B x 4, Wb'
          a0 = address(W0.x); a1 = address(W0.y); a2 = address(W0.z); a3 = address(W0.w);
          // (the A addresses of the next iteration are operands too: their arithmetic is what
          // B's gathers land under, it must not sink below this wait)
          asm volatile("s_waitcnt lgkmcnt(0)"
                       : "+v"(B0), "+v"(B1), "+v"(B2), "+v"(B3), "+v"(Wb), "+v"(a0), "+v"(a1),
                         "+v"(a2), "+v"(a3));
          acc += (B0 + B1) + (B2 + B3);
        }
      }
      for (int j = len8; j < len; ++j) acc += cell(words[j]);
    } else if (in_lds) {
      run(std::true_type{});
    } else {
      run(std::false_type{});
    }
  }
  if (valid && (acc | ambiguous)) {
    const size_t c = static_cast<size_t>(r) * P.num_translations + t;
    atomicAdd(&P.sums[c].x, acc);
    if (ambiguous) atomicAdd(&P.sums[c].y, ambiguous);
    if (kGroups && TP.seg_sums != nullptr) {
      // the last chunk of this lane's loop: chunk_begin + blockIdx.y + k gridDim.y < chunk_end
      const int steps = (chunk_end - chunk_begin - static_cast<int>(blockIdx.y) +
                         static_cast<int>(gridDim.y) - 1) / static_cast<int>(gridDim.y);
      const int last = chunk_begin + static_cast<int>(blockIdx.y) +
                       (steps - 1) * static_cast<int>(gridDim.y);
      const unsigned added = acc - acc_seen;
      if (last < split0) acc_seg0 += added;
      else if (last < split1) acc_seg1 += added;
      if (acc_seg0) atomicAdd(&TP.seg_sums[c].x, acc_seg0);
      if (acc_seg1) atomicAdd(&TP.seg_sums[c].y, acc_seg1);
    }
  }
}

// Span of a translation table in cells (what widens a chunk's box into its tile).
void SpanOf(const std::vector<float4>& table, float inv_resolution, Rt3DTileParams* tp) {
  for (int a = 0; a < 3; ++a) { tp->tr_lo[a] = INFINITY; tp->tr_hi[a] = -INFINITY; }
  for (const float4& v : table) {
    const float c[3] = {v.x * inv_resolution, v.y * inv_resolution, v.z * inv_resolution};
    for (int a = 0; a < 3; ++a) {
      tp->tr_lo[a] = std::min(tp->tr_lo[a], c[a]);
      tp->tr_hi[a] = std::max(tp->tr_hi[a], c[a]);
    }
  }
}

// ---- the tile parameters of the passes, next to GroupParams, PairParams and CandidateParams ----

// Group pass: the group table's span, several rotations per workgroup; staged: the sums over
// point segments 0 and 1 next to the totals.
Rt3DTileParams GroupTiles(const Rt3DBoundsSearch& run) {
  Rt3DTileParams t = run.tiles;
  SpanOf(run.S->group, run.base.inv_resolution, &t);
  t.rotations_per_block = run.mode.rot_per_block;
  t.tile_capacity = run.mode.group_tile_capacity;
  t.fixed_point = run.mode.group_fixed_point;
  if (run.mode.staged) {
    t.seg_bounds = run.d_segment_counts + kGroupSegments;
    t.seg_first = 0; t.seg_last = 2;
    t.seg_sums = run.d_group_sums + run.RG;
  }
  return t;
}

// Sparse pair pass: the group pass on the candidate pass's chunk list (256 points) and boxes.
Rt3DTileParams PairTiles(const Rt3DBoundsSearch& run) {
  Rt3DTileParams t = GroupTiles(run);
  t.chunks = run.tiles.chunks + run.max_chunks;
  t.num_chunks = run.d_segment_counts + kCandidateChunks;
  t.block_items = kPairItems;
  t.boxes = run.d_list_boxes;
  if (run.mode.staged) t.seg_bounds = run.d_segment_counts + kCandidateSegments;
  return t;
}

// Candidate passes: the translation table's span, the candidate chunk list and its boxes.
Rt3DTileParams CandidateTiles(const Rt3DBoundsSearch& run) {
  Rt3DTileParams t = run.tiles;
  SpanOf(run.S->trans, run.base.inv_resolution, &t);
  t.chunks = run.tiles.chunks + run.max_chunks;                 // the candidate pass's own list
  t.num_chunks = run.d_segment_counts + kCandidateChunks;
  t.rotations_per_block = 1;
  t.boxes = run.d_list_boxes;                                   // (computed before the group pass)
  t.tile_capacity = run.mode.cand_tile_capacity;
  t.block_items = run.mode.block_items;
  return t;
}

// Chunk slices (blockIdx.y) of a tiled launch of `blocks` workgroups over `chunks` chunks at
// most: about eight workgroups per CU.
int SlicesOf(const Rt3DBoundsSearch& run, int chunks, int blocks) {
  return std::max(1, std::min(chunks, DivUp(8 * run.cus, blocks)));
}

// Launch shape of a tiled pass over whole rotations (the dense group pass, the rotation blocks).
struct Rt3DGroupLaunch {
  int threads, blocks, slices;
  size_t lds;
};
Rt3DGroupLaunch GroupLaunch(const Rt3DBoundsSearch& run, long long rotations) {
  const int rot_per_block = run.mode.rot_per_block;
  Rt3DGroupLaunch l;
  l.threads = std::min(1024, DivUp(rot_per_block * run.S->G, 64) * 64);
  l.lds = Rt3DTileLds<true, false>::Bytes(rot_per_block, run.mode.group_tile_capacity);
  l.blocks = DivUp(rotations, rot_per_block);
  l.slices = SlicesOf(run, run.max_chunks, l.blocks);
  return l;
}

}  // namespace

// (bins of kTileBin^3 cells)
void SortCloudIntoBins(Rt3DBoundsSearch* run) {
  Workspace& ws = *run->ws;
  const Rt3DSearchSpace& S = *run->S;
  const Rt3DBulkGeometry& g = run->geo;
  const Rt3DBulkParams& B = run->base;
  const int n = S.n;
  Rt3DBinParams BP{};
  BP.rotation = S.rot[S.R / 2];
  BP.translation = S.trans[S.T / 2];
  BP.inv_resolution = B.inv_resolution;
  BP.off_x = B.off_x; BP.off_y = B.off_y; BP.off_z = B.off_z;
  BP.t0x = B.t0x; BP.t0y = B.t0y; BP.t0z = B.t0z;
  BP.lo_x = B.lo_x; BP.hi_x = B.hi_x; BP.lo_y = B.lo_y; BP.hi_y = B.hi_y;
  BP.lo_z = B.lo_z; BP.hi_z = B.hi_z;
  BP.bins_x = DivUp(g.bx, kTileBin); BP.bins_y = DivUp(g.by, kTileBin);
  BP.bins_z = DivUp(g.bz, kTileBin);
  BP.n = n;
  const int num_bins = BP.bins_x * BP.bins_y * BP.bins_z;
  run->max_chunks = n / kTileChunkCandidates + num_bins + 1;      // (either list)
  const int max_chunks = run->max_chunks;
  float* d_sorted = ws.dev[kSlotSorted].ReserveAs<float>(3 * static_cast<size_t>(n));
  // [bin counts | Rt3DSegmentCount | group chunk list | candidate chunk list]
  int* d_bin_count = static_cast<int*>(ws.dev[kSlotBins].Reserve(
      sizeof(int) * (num_bins + kNumSegmentCounts) +
      2 * sizeof(int2) * static_cast<size_t>(max_chunks)));
  int* d_chunk_count = d_bin_count + num_bins;
  int2* d_chunks = reinterpret_cast<int2*>(d_chunk_count + kNumSegmentCounts);
  int2* d_chunks_candidates = d_chunks + max_chunks;
  CMX_HIP(hipMemsetAsync(d_bin_count, 0, sizeof(int) * (num_bins + kNumSegmentCounts), ws.stream));
  Rt3DBinCountKernel<<<DivUp(n, 256), 256, 0, ws.stream>>>(BP, run->D->d_xyz, d_bin_count);
  // (segment windows: sixteen or more periods over a large cloud, never shorter than four
  // group-pass pieces)
  const int segment_window = n >= 32768 ? 4096 : 2048;
  Rt3DBinScanKernel<<<1, 1024, 0, ws.stream>>>(
      d_bin_count, num_bins, d_chunks, d_chunks_candidates, d_chunk_count, segment_window,
      segment_window / 16 * run->mode.sixteenths0, segment_window / 16 * run->mode.sixteenths1);
  run->d_segment_counts = d_chunk_count;
  Rt3DBinScatterKernel<<<DivUp(n, 256), 256, 0, ws.stream>>>(BP, run->D->d_xyz, d_bin_count,
                                                              d_sorted);
  CMX_HIP(hipGetLastError());
  Rt3DTileParams& TG = run->tiles;
  if (run->mode.report) {
    TG.stats = reinterpret_cast<unsigned long long*>(ws.dev[kSlotReport].Reserve(64));
    CMX_HIP(hipMemsetAsync(TG.stats, 0, 64, ws.stream));
  }
  TG.sorted_xyz = d_sorted;
  TG.chunks = d_chunks;
  TG.num_chunks = d_chunk_count + kGroupChunks;
  TG.pitch_x = static_cast<int>(g.bx); TG.pitch_y = static_cast<int>(g.by);
  TG.pitch_z = static_cast<int>(g.bz);
  run->trace->Mark("bins");
}

// (the candidate chunk list under list_rotations rotations: the sparse pair pass and the
// candidate passes share the boxes)
void BoxListChunks(Rt3DBoundsSearch* run) {
  if (!run->mode.use_boxes) return;
  Workspace& ws = *run->ws;
  run->d_list_boxes = ws.dev[kSlotListBoxes].ReserveAs<float>(
      static_cast<size_t>(run->num_lists) * run->max_chunks * 6);
  Rt3DChunkBoxKernel<<<dim3(run->num_lists, 8), 256, 0, ws.stream>>>(
      GroupParams(*run), run->tiles.sorted_xyz, run->tiles.chunks + run->max_chunks,
      run->d_segment_counts + kCandidateChunks, run->mode.list_rotations, run->d_list_boxes);
}

// Chunk boxes of the group chunk list under the rotations of each workgroup, then the tile kernel.
void TileGroups(Rt3DBoundsSearch* run, bool rotation_blocks) {
  Workspace& ws = *run->ws;
  const Rt3DBulkParams P = rotation_blocks ? BlockParams(*run) : GroupParams(*run);
  Rt3DTileParams T = GroupTiles(*run);
  if (rotation_blocks) {                       // (one segment: every chunk)
    T.seg_bounds = nullptr; T.seg_sums = nullptr; T.seg_first = 0; T.seg_last = 2;
  }
  const Rt3DGroupLaunch l = GroupLaunch(*run, P.num_rotations);
  OptInLds(reinterpret_cast<const void*>(Rt3DTileKernel<true, false>), ws.device, l.lds);
  if (run->mode.use_boxes) {
    float* d_boxes = ws.dev[kSlotGroupBoxes].ReserveAs<float>(
        static_cast<size_t>(l.blocks) * run->max_chunks * 6);
    Rt3DChunkBoxKernel<<<dim3(l.blocks, 8), 256, 0, ws.stream>>>(
        P, run->tiles.sorted_xyz, run->tiles.chunks, run->tiles.num_chunks,
        run->mode.rot_per_block, d_boxes);
    T.boxes = d_boxes;
  }
  Rt3DTileKernel<true, false><<<dim3(l.blocks, l.slices), l.threads, l.lds, ws.stream>>>(P, T);
}

void TilePairs(Rt3DBoundsSearch* run, int blocks, int list_chunks) {
  const size_t lds =
      Rt3DTileLds<true, true>::Bytes(run->mode.list_rotations, run->mode.group_tile_capacity);
  OptInLds(reinterpret_cast<const void*>(Rt3DTileKernel<true, true>), run->ws->device, lds);
  Rt3DTileKernel<true, true>
      <<<dim3(blocks, SlicesOf(*run, list_chunks, blocks)), kPairItems, lds, run->stream()>>>(
          PairParams(*run), PairTiles(*run));
}

void TileCandidates(Rt3DBoundsSearch* run, int blocks, int seg_first, int seg_last, int chunks) {
  Rt3DTileParams T = CandidateTiles(*run);
  if (seg_first > 0 || seg_last < 2) {
    T.seg_bounds = run->d_segment_counts + kCandidateSegments;
    T.seg_first = seg_first; T.seg_last = seg_last;
  }
  const size_t lds =
      Rt3DTileLds<false, true>::Bytes(run->mode.list_rotations, run->mode.cand_tile_capacity);
  OptInLds(reinterpret_cast<const void*>(Rt3DTileKernel<false, true>), run->ws->device, lds);
  Rt3DTileKernel<false, true>
      <<<dim3(blocks, SlicesOf(*run, chunks, blocks)), run->mode.block_items, lds,
         run->stream()>>>(CandidateParams(*run), T);
}

void ReportGroupTiles(Rt3DBoundsSearch* run) {
  Workspace& ws = *run->ws;
  const Rt3DGroupLaunch l = GroupLaunch(*run, run->S->R);
  unsigned long long* d_stats = run->tiles.stats;
  unsigned long long h[4];
  int chunks_made = 0;
  CMX_HIP(hipMemcpyAsync(h, d_stats, sizeof(h), hipMemcpyDeviceToHost, ws.stream));
  CMX_HIP(hipMemcpyAsync(&chunks_made, run->tiles.num_chunks, sizeof(int), hipMemcpyDeviceToHost,
                         ws.stream));
  CMX_HIP(hipMemsetAsync(d_stats, 0, 64, ws.stream));
  CMX_HIP(hipStreamSynchronize(ws.stream));
  const double units = static_cast<double>(h[0] + h[1]);
  fprintf(stderr,
          "[cmx] rt3d tiles (groups): %d chunks, %d rotations x %d lanes per block, %d "
          "slices; %.0f (block, chunk) units: %.1f %% in LDS, mean tile %.1f KB, mean "
          "chunk %.1f points\n",
          chunks_made, run->mode.rot_per_block, l.threads, l.slices, units,
          100. * h[0] / std::max(units, 1.), h[2] / std::max(units, 1.) / 1024.,
          h[3] / std::max(units, 1.));
}

}  // namespace cmx
