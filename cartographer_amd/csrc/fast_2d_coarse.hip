// FastCorrelativeScanMatcher2D on gfx950: the front end of a search -- scan preparation and the
// scores of every lowest-resolution candidate.
//
// Reference behaviour being replaced:
//   SM2/correlative_scan_matcher_2d.cc:27-55,73-127  SearchParameters / ShrinkToFit /
//                                                    GenerateRotatedScans / DiscretizeScans
//   SM2/fast_correlative_scan_matcher_2d.cc:264-333  lowest-resolution candidates, ScoreCandidates
// (SM2 = cartographer/mapping/internal/2d/scan_matching).
//
// Lowest-resolution scoring ("phase planes").  Lowest-resolution candidates
// of one rotated scan sit on a lattice of pitch w = 2^(depth-1) cells, so for
// a given point p all of them read level cells with the same residue
// (phase) modulo w.  The level is therefore stored a second time as w*w small
// planes, plane(py,px)[J][I] = cell(I*w+px, J*w+py): ONE 64-byte plane holds
// everything a point contributes to all ~13x13 candidates of its scan.  Points
// are bucketed by the lattice block they fall in; within a bucket the lane ->
// candidate map is fixed, so a wave adds planes into registers (one coalesced
// 64 B load + one add per point for ALL candidates) and flushes once per
// bucket.  Out-of-grid lookups (60 % of the reference's reads here) cost
// nothing.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "fast_2d_device.h"
#include "fast_2d_internal.h"

namespace cmx {
namespace {

constexpr int kMaxBuckets = 4096;      // LDS histogram size of the point bucketing
constexpr int kMaxCoarsePerScan = 4096;  // lowest-resolution candidates per scan (plane kernel)
constexpr int kMaxAccCells = 12288;      // padded LDS accumulators of the plane kernel (48 KB)

// ---------------------------------------------------------------------------
// Scan preparation: rotate, translate, discretise, ShrinkToFit, bucket
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
PrepScansKernel(const Fast2DProblem* __restrict__ problems, const float* __restrict__ xyz, int n,
                ProblemState* __restrict__ states, int* __restrict__ counters_words,
                int num_counter_words) {
  // First kernel of a call: it also clears the list counters of the search (saves a
  // memset and its launch gap).
  // (every workgroup clears a slice: the counters with the work queue's control words are 376 KB)
  if (counters_words)
    for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
         i < num_counter_words; i += gridDim.x * gridDim.y * blockDim.x)
      counters_words[i] = 0;
  const Fast2DProblem& P = problems[blockIdx.y];
  const int s = blockIdx.x;
  if (s >= P.num_scans || P.use_fused) return;
  const Quat q0{P.init_qw, 0.f, 0.f, P.init_qz};
  const float2 r = P.scan_rot[s];
  const Quat qs{r.x, 0.f, 0.f, r.y};
  uint32_t* out = P.discrete + static_cast<size_t>(s) * n;
  int lo_x = 0, lo_y = 0, hi_x = 0, hi_y = 0, bad = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const F3 p{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    F3 a = Rotate(q0, p);                   // rotated_point_cloud (+ zero translation)
    a.x += 0.f; a.y += 0.f; a.z += 0.f;
    F3 b = Rotate(qs, a);                   // GenerateRotatedScans
    b.x += 0.f; b.y += 0.f;
    const float x = (1.f * b.x + 0.f * b.y) + P.tx;   // Affine2f(translation) * v
    const float y = (0.f * b.x + 1.f * b.y) + P.ty;
    // MapLimits::GetCellIndex (mapping/2d/map_limits.h:69-76).
    const int ix = CellIndexF64(P.max_y - static_cast<double>(y), P.res, P.inv_res);
    const int iy = CellIndexF64(P.max_x - static_cast<double>(x), P.res, P.inv_res);
    if (ix < -32768 || ix > 32767 || iy < -32768 || iy > 32767) bad = 1;
    out[i] = (static_cast<uint32_t>(ix) & 0xffffu) | (static_cast<uint32_t>(iy) << 16);
    lo_x = min(lo_x, -ix);
    lo_y = min(lo_y, -iy);
    hi_x = max(hi_x, P.nx - 1 - ix);
    hi_y = max(hi_y, P.ny - 1 - iy);
  }
  __shared__ int red[4][5];
  __shared__ int4 s_bounds;
  __shared__ int2 s_dims;
  lo_x = WaveMin(lo_x); lo_y = WaveMin(lo_y);
  hi_x = WaveMax(hi_x); hi_y = WaveMax(hi_y);
  bad = WaveMax(bad);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave][0] = lo_x; red[wave][1] = lo_y; red[wave][2] = hi_x; red[wave][3] = hi_y;
    red[wave][4] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      lo_x = min(lo_x, red[w][0]); lo_y = min(lo_y, red[w][1]);
      hi_x = max(hi_x, red[w][2]); hi_y = max(hi_y, red[w][3]);
      bad = max(bad, red[w][4]);
    }
    // SearchParameters::ShrinkToFit (SM2/correlative_scan_matcher_2d.cc:73-91).
    int4 bd;
    bd.x = max(-P.nl, lo_x);
    bd.y = min(P.nl, hi_x);
    bd.z = max(-P.nl, lo_y);
    bd.w = min(P.nl, hi_y);
    P.bounds[s] = bd;
    // GenerateLowestResolutionCandidates counts (SM2/fast_...2d.cc:279-292).
    const int step = 1 << (P.depth - 1);
    const int2 dims = make_int2((bd.y - bd.x + step) / step, (bd.w - bd.z + step) / step);
    P.coarse_dims[s] = dims;
    s_bounds = bd;
    s_dims = dims;
    if (bad) atomicMax(&states[blockIdx.y].error, 1);
    const int count = dims.x * dims.y;
    if (count > P.coarse_stride || (P.use_planes && count > kMaxCoarsePerScan))
      atomicMax(&states[blockIdx.y].error, 2);
  }
  if (!P.use_planes) return;

  // ---- bucket the points by the lattice block they fall in ---------------
  __shared__ int hist[kMaxBuckets];
  __shared__ int partial[256];
  __syncthreads();
  const int4 bd = s_bounds;
  const int2 dims = s_dims;
  const int shift = P.depth - 1, w = 1 << shift;
  const int BW = dims.x + P.plane_i - 1, BH = dims.y + P.plane_j - 1;
  const int NB = BW * BH;   // <= kMaxBuckets (checked on the host with upper bounds)
  for (int b = threadIdx.x; b < NB; b += blockDim.x) hist[b] = 0;
  __syncthreads();
  auto classify = [&](uint32_t packed, int* bucket, int* plane, uint32_t* block = nullptr) {
    const int U = static_cast<short>(packed & 0xffffu) + bd.x + w - 1;
    const int V = static_cast<short>(packed >> 16) + bd.z + w - 1;
    const int bx = (U >> shift) + dims.x - 1, by = (V >> shift) + dims.y - 1;
    *plane = (V & (w - 1)) * w + (U & (w - 1));
    *bucket = (bx >= 0 && bx < BW && by >= 0 && by < BH) ? by * BW + bx : -1;
    if (block) *block = static_cast<uint32_t>(bx) | (static_cast<uint32_t>(by) << 8);
  };
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    int bucket, plane;
    classify(out[i], &bucket, &plane);
    if (bucket >= 0) atomicAdd(&hist[bucket], 1);
  }
  __syncthreads();
  // exclusive scan of hist[0..NB)
  const int chunk = (NB + 255) / 256;
  const int b0 = min(static_cast<int>(threadIdx.x) * chunk, NB), b1 = min(b0 + chunk, NB);
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += hist[b];
  partial[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x < 64) {   // exclusive scan of the 256 partials by one wave, 4 per lane
    const int l = threadIdx.x;
    const int a0 = partial[4 * l], a1 = partial[4 * l + 1], a2 = partial[4 * l + 2],
              a3 = partial[4 * l + 3];
    const int mine = a0 + a1 + a2 + a3;
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (l >= off) incl += o;
    }
    const int base = incl - mine;
    partial[4 * l] = base;
    partial[4 * l + 1] = base + a0;
    partial[4 * l + 2] = base + a0 + a1;
    partial[4 * l + 3] = base + a0 + a1 + a2;
    if (l == 63) P.sorted_count[s] = incl;
  }
  __syncthreads();
  int run = partial[threadIdx.x];
  for (int b = b0; b < b1; ++b) { const int v = hist[b]; hist[b] = run; run += v; }
  __syncthreads();
  // Records carry what the plane scorer would otherwise compute per point: the byte
  // offset of the point's plane and the constant bx * pitch + by its lattice block
  // subtracts in the accumulator index (pitch = dims.y + 2 * plane_j - 2).
  uint2* sorted = P.sorted + static_cast<size_t>(s) * n;
  const int pitch = dims.y + 2 * P.plane_j - 2;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    int bucket, plane;
    uint32_t block;
    classify(out[i], &bucket, &plane, &block);
    if (bucket >= 0) {
      const int pos = atomicAdd(&hist[bucket], 1);
      sorted[pos] = make_uint2(static_cast<uint32_t>(plane) * P.plane_stride,
                               (block & 0xffu) * pitch + (block >> 8));
    }
  }
}

// ---------------------------------------------------------------------------
// Scoring
// ---------------------------------------------------------------------------
// Integer sum of one candidate over all points, one wave per candidate
// (SM2/fast_...2d.cc:320-329 with GetValue of .h:56-71).  Generic fallback of
// the lowest resolution when the phase-plane layout does not apply.
__device__ __forceinline__ int ScoreCandidateWave(const LevelDesc& L, int level,
                                                  const uint32_t* __restrict__ scan, int n, int dx,
                                                  int dy, int lane) {
  const int off = (1 << level) - 1;   // -offset_
  const int ax = dx + off, ay = dy + off;
  const auto* cells = AsGlobal(L.cells);
  const auto* gscan = AsGlobal(scan);
  int sum = 0;
#pragma unroll 4
  for (int i = lane; i < n; i += kWave) {
    const uint32_t p = gscan[i];
    const int x = static_cast<short>(p & 0xffffu) + ax;
    const int y = static_cast<short>(p >> 16) + ay;
    const bool ok = static_cast<unsigned>(x) < static_cast<unsigned>(L.wx) &&
                    static_cast<unsigned>(y) < static_cast<unsigned>(L.wy);
    const unsigned v = cells[ok ? x + y * L.wx : 0];   // unconditional load, masked value
    sum += ok ? v : 0u;
  }
  return WaveSum(sum);
}

// Block-wide (sum, local index) maximum, smallest index on ties; result valid
// in thread 0.
__device__ __forceinline__ int2 BlockBest(int sum, int index, int2* scratch /*[4]*/) {
  // sum >= -1 (idle threads pass -1); bias by one so the key is unsigned.
  unsigned long long key =
      (static_cast<unsigned long long>(static_cast<unsigned>(sum + 1)) << 32) |
      static_cast<unsigned>(0x7fffffff - index);
  key = WaveMaxU64(key);
  if ((threadIdx.x & 63) == 0)
    scratch[threadIdx.x >> 6] = make_int2(static_cast<int>(key >> 32) - 1,
                                          0x7fffffff - static_cast<int>(key & 0xffffffffu));
  __syncthreads();
  int2 best = scratch[0];
  if (threadIdx.x == 0) {
    for (int w = 1; w < static_cast<int>(blockDim.x >> 6); ++w) {
      const int2 o = scratch[w];
      if (o.x > best.x || (o.x == best.x && o.y < best.y)) best = o;
    }
  }
  return best;
}

__global__ void __launch_bounds__(256)
ScoreCoarseGenericKernel(const Fast2DProblem* __restrict__ problems, int n,
                         const ProblemState* __restrict__ states) {
  const Fast2DProblem& P = problems[blockIdx.y];
  const int s = blockIdx.x;
  if (s >= P.num_scans || states[blockIdx.y].error || P.use_planes) return;
  const int level = P.depth - 1;
  const int step = 1 << level;
  const int2 dims = P.coarse_dims[s];
  const int4 bd = P.bounds[s];
  const int base = s * P.coarse_stride;
  const uint32_t* scan = P.discrete + static_cast<size_t>(s) * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int count = dims.x * dims.y;
  int best_sum = -1, best_index = 0x7ffffff;  // idle threads (sum -1) never win
  for (int c = wave; c < count; c += 4) {
    const int ix = c / dims.y, iy = c - ix * dims.y;   // x outer, y inner (:295-307)
    const int sum = ScoreCandidateWave(P.level[level], level, scan, n, bd.x + ix * step,
                                       bd.z + iy * step, lane);
    if (lane == 0) {
      P.coarse_sum[base + c] = sum;
      P.coarse_score[base + c] = ToScore(P, sum, n);
    }
    if (sum > best_sum) { best_sum = sum; best_index = c; }
  }
  __shared__ int2 scratch[4];
  const int2 best = BlockBest(best_sum, best_index, scratch);
  if (threadIdx.x == 0) P.scan_best[s] = best;
}

// Phase-plane scoring of all lowest-resolution candidates of one scan.
template <int CHUNKS>
__global__ void __launch_bounds__(256)
ScoreCoarsePlanesKernel(const Fast2DProblem* __restrict__ problems, int n,
                        const ProblemState* __restrict__ states) {
  const Fast2DProblem& P = problems[blockIdx.y];
  const int s = blockIdx.x;
  if (s >= P.num_scans || states[blockIdx.y].error || !P.use_planes || P.use_fused) return;
  if ((P.plane_stride >> 6) != CHUNKS) return;
  // Candidate accumulators, padded by the plane extent on every side: a lane's cell
  // (I, J) in lattice block (bx, by) belongs to candidate
  //   (ix, iy) = (I - bx + dims.x - 1, J - by + dims.y - 1),
  // which may lie outside [0, dims); with the padding its accumulator index
  //   (ix + PI - 1) * pitch + (iy + PJ - 1) = lane_const - (bx * pitch + by)
  // is always inside the array, so a flush is one subtract and one LDS add per lane,
  // no bounds logic (out-of-range candidates collect in padding nobody reads).
  extern __shared__ int cand_acc[];
  __shared__ int2 scratch[4];
  const int2 dims = P.coarse_dims[s];
  const int count = dims.x * dims.y;
  const int PI = P.plane_i, PJ = P.plane_j, PIJ = PI * PJ;
  const int pitch = dims.y + 2 * PJ - 2;
  const int acc_cells = (dims.x + 2 * PI - 2) * pitch;
  for (int i = threadIdx.x; i < acc_cells; i += blockDim.x) cand_acc[i] = 0;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int M = P.sorted_count[s];
  // (x = plane byte offset, y = block constant) as one 64-bit word per record
  const auto* rec = AsGlobal(reinterpret_cast<const unsigned long long*>(P.sorted)) +
                    static_cast<size_t>(s) * n;
  const int waves = blockDim.x >> 6;     // 2..4, chosen by the host (see the launch)
  const int begin = static_cast<int>(static_cast<long long>(M) * wave / waves);
  const int end = static_cast<int>(static_cast<long long>(M) * (wave + 1) / waves);
  const int stride = P.plane_stride;
  const unsigned zero_plane = 1u << (2 * (P.depth - 1));   // index w*w: the all-zero plane

  int acc[CHUNKS], lane_const[CHUNKS];
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    acc[c] = 0;
    // Lanes past the plane read its zero padding: let them add 0 to the last cell.
    const int cell = min(c * 64 + lane, PIJ - 1);
    lane_const[c] = (cell % PI + dims.x + PI - 2) * pitch + (cell / PI + dims.y + PJ - 2);
  }
  int cur = -1;
  auto flush = [&](int block_const) {
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      atomicAdd(&cand_acc[lane_const[c] - block_const], acc[c]);
      acc[c] = 0;
    }
  };

  // Records are wave-uniform: 64 of them arrive with one coalesced 8-byte load per lane
  // (the next 64 prefetched meanwhile) and are broadcast with v_readlane (immediate lane
  // index: the batch loops are fully unrolled).  A plane read is a buffer load: lane
  // offset in a VGPR, the record's plane offset in an SGPR, no address arithmetic at all.
  // kBatch plane loads are in flight before the first one is consumed.  Lanes past `end`
  // hold the sentinel (all-zero plane, block -1): adding zeros changes nothing.
  constexpr int kBatch = CHUNKS == 1 ? 32 : (CHUNKS == 2 ? 16 : 8);
  const int kSentinelBlock = -1;
  const unsigned long long sentinel =
      (static_cast<unsigned long long>(static_cast<uint32_t>(kSentinelBlock)) << 32) |
      static_cast<uint32_t>(zero_plane * stride);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(P.planes), 0, static_cast<int>((zero_plane + 1) * stride), 0x00020000);
  unsigned long long mine = sentinel;
  if (begin + lane < end) mine = rec[begin + lane];
  for (int base_i = begin; base_i < end; base_i += 64) {
    unsigned long long next = sentinel;
#pragma unroll
    for (int j0 = 0; j0 < 64; j0 += kBatch) {
      if (base_i + j0 >= end) break;          // wave-uniform
      int block[kBatch];
      int v[kBatch][CHUNKS];
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        const int plane_offset =
            __builtin_amdgcn_readlane(static_cast<int>(mine & 0xffffffffu), j0 + k);
        block[k] = __builtin_amdgcn_readlane(static_cast<int>(mine >> 32), j0 + k);
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c)
          v[k][c] = __builtin_amdgcn_raw_buffer_load_b8(rsrc, lane + c * 64, plane_offset, 0);
      }
      if (j0 == 0) {   // prefetch the next 64 records behind this batch's plane loads
        const int nidx = base_i + 64 + lane;
        next = rec[min(nidx, end - 1)];
        if (nidx >= end) next = sentinel;
      }
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        if (block[k] != cur) {
          if (cur >= 0) flush(cur);
          cur = block[k];     // the sentinel block (-1) only ever follows real ones
        }
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) acc[c] += v[k][c];
      }
    }
    mine = next;
  }
  if (cur >= 0) flush(cur);
  __syncthreads();

  const int base = s * P.coarse_stride;
  auto* coarse_sum = AsGlobal(P.coarse_sum) + base;
  auto* coarse_score = AsGlobal(P.coarse_score) + base;
  int best_sum = -1, best_index = 0x7ffffff;  // idle threads (sum -1) never win
  for (int i = threadIdx.x; i < count; i += blockDim.x) {
    const int ix = i / dims.y, iy = i - ix * dims.y;
    const int sum = cand_acc[(ix + PI - 1) * pitch + (iy + PJ - 1)];
    coarse_sum[i] = sum;
    coarse_score[i] = ToScore(P, sum, n);
    if (sum > best_sum) { best_sum = sum; best_index = i; }
  }
  const int2 best = BlockBest(best_sum, best_index, scratch);
  if (threadIdx.x == 0) P.scan_best[s] = best;
}

// The same scoring for 64-byte planes (plane_i * plane_j <= 64, the usual case) with DWORD
// gathers.  A wave-wide `buffer_load_ubyte` costs the texture-address path ~12 cycles
// however few cache lines it touches (2.3 M of them were the 45 us of the byte variant:
// SQ/TA counters in profiles/HISTORY.md); here a lane fetches four plane cells at once, sixteen lanes
// cover a plane, and one instruction serves FOUR records (lane group g = lane / 16 takes
// records 4t + g).  Groups sit in different lattice blocks, so the block bookkeeping is
// per lane: packed 16-bit partial sums (cells 0|2 and 1|3), flushed to the LDS
// accumulators when the lane's block changes or after 256 records.
__global__ void __launch_bounds__(256)
ScoreCoarsePlanesDwordKernel(const Fast2DProblem* __restrict__ problems, int n,
                             const ProblemState* __restrict__ states) {
  const Fast2DProblem& P = problems[blockIdx.y];
  const int s = blockIdx.x;
  if (s >= P.num_scans || states[blockIdx.y].error || !P.use_planes || P.use_fused) return;
  if (P.plane_stride != 64) return;
  extern __shared__ int cand_acc[];
  __shared__ int2 scratch[4];
  const int2 dims = P.coarse_dims[s];
  const int count = dims.x * dims.y;
  const int PI = P.plane_i, PJ = P.plane_j, PIJ = PI * PJ;
  const int pitch = dims.y + 2 * PJ - 2;
  const int acc_cells = (dims.x + 2 * PI - 2) * pitch;
  for (int i = threadIdx.x; i < acc_cells; i += blockDim.x) cand_acc[i] = 0;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int group = lane >> 4, sub = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int M = P.sorted_count[s];
  const auto* rec = AsGlobal(reinterpret_cast<const unsigned long long*>(P.sorted)) +
                    static_cast<size_t>(s) * n;
  const int waves = blockDim.x >> 6;
  const int begin = static_cast<int>(static_cast<long long>(M) * wave / waves);
  const int end = static_cast<int>(static_cast<long long>(M) * (wave + 1) / waves);
  const unsigned zero_plane = 1u << (2 * (P.depth - 1));   // index w*w: the all-zero plane

  int lane_const[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // Cells past the plane are zero padding: they add 0 to the last cell.
    const int cell = min(4 * sub + j, PIJ - 1);
    lane_const[j] = (cell % PI + dims.x + PI - 2) * pitch + (cell / PI + dims.y + PJ - 2);
  }
  int cur = -1, pending = 0;
  uint32_t even = 0, odd = 0;               // cells 0 | 2 << 16 and 1 | 3 << 16
  const auto flush = [&]() {
    const int a0 = even & 0xffffu, a2 = even >> 16, a1 = odd & 0xffffu, a3 = odd >> 16;
    if (a0) atomicAdd(&cand_acc[lane_const[0] - cur], a0);
    if (a1) atomicAdd(&cand_acc[lane_const[1] - cur], a1);
    if (a2) atomicAdd(&cand_acc[lane_const[2] - cur], a2);
    if (a3) atomicAdd(&cand_acc[lane_const[3] - cur], a3);
    even = odd = 0;
    pending = 0;
  };

  constexpr int kSteps = 8;                 // gathers (of four records each) in flight
  const unsigned long long sentinel = (0xffffffffull << 32) | (zero_plane * 64u);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(P.planes), 0, static_cast<int>((zero_plane + 1) * 64), 0x00020000);
  unsigned long long mine = sentinel;
  if (begin + lane < end) mine = rec[begin + lane];
  for (int base_i = begin; base_i < end; base_i += 64) {
    unsigned long long next = sentinel;
#pragma unroll
    for (int t0 = 0; t0 < 16; t0 += kSteps) {
      if (base_i + 4 * t0 >= end) break;      // wave-uniform
      int block[kSteps];
      uint32_t q[kSteps];
#pragma unroll
      for (int k = 0; k < kSteps; ++k) {
        const int src = 4 * (t0 + k) + group;                 // this lane group's record
        const int plane_offset = __shfl(static_cast<int>(mine & 0xffffffffu), src, 64);
        block[k] = __shfl(static_cast<int>(mine >> 32), src, 64);
        q[k] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, plane_offset + 4 * sub, 0, 0);
      }
      if (t0 == 0) {   // prefetch the next 64 records behind the first gathers
        const int nidx = base_i + 64 + lane;
        next = rec[min(nidx, end - 1)];
        if (nidx >= end) next = sentinel;
      }
#pragma unroll
      for (int k = 0; k < kSteps; ++k) {
        if (block[k] != cur) {                // per lane group
          if (cur >= 0) flush();
          cur = block[k];                     // -1 (sentinel) only ever follows real blocks
        }
        even += q[k] & 0x00ff00ffu;
        odd += (q[k] >> 8) & 0x00ff00ffu;
        if (++pending == 256) flush();        // 16-bit partial sums: 256 x 255 fits
      }
    }
    mine = next;
  }
  if (cur >= 0) flush();
  __syncthreads();

  const int base = s * P.coarse_stride;
  auto* coarse_sum = AsGlobal(P.coarse_sum) + base;
  auto* coarse_score = AsGlobal(P.coarse_score) + base;
  int best_sum = -1, best_index = 0x7ffffff;  // idle threads (sum -1) never win
  for (int i = threadIdx.x; i < count; i += blockDim.x) {
    const int ix = i / dims.y, iy = i - ix * dims.y;
    const int sum = cand_acc[(ix + PI - 1) * pitch + (iy + PJ - 1)];
    coarse_sum[i] = sum;
    coarse_score[i] = ToScore(P, sum, n);
    if (sum > best_sum) { best_sum = sum; best_index = i; }
  }
  const int2 best = BlockBest(best_sum, best_index, scratch);
  if (threadIdx.x == 0) P.scan_best[s] = best;
}

// ---------------------------------------------------------------------------
// Fused front end (the usual case: 64-byte phase planes, the scan fits in LDS)
// ---------------------------------------------------------------------------
// One block per rotated scan does everything the reference does for that scan before
// branch and bound -- GenerateRotatedScans + DiscretizeScans + ShrinkToFit
// (SM2/correlative_scan_matcher_2d.cc:73-127), GenerateLowestResolutionCandidates and
// their ScoreCandidates (SM2/fast_correlative_scan_matcher_2d.cc:264-333) -- with the
// discretised scan staged in LDS only.  As separate launches the same work wrote 27 MB per
// match (discrete scans + 64-bit bucketed records) and the scorer fetched 20 MB of it back;
// here only the candidates' scores (1.7 MB) leave the chip -- the tree search re-derives the
// cells of the scans it descends into (ScanCell) -- and the per-scan candidate layout needs
// no prefix sum: scan s owns [s * coarse_stride, (s + 1) * coarse_stride).
//
// Unlike the separate launches this kernel does NOT sort the points by lattice block.  The
// sort (histogram, scan, scatter: seven barriers) was a third of a block's latency, and it
// buys little: a range scan is spatially coherent -- consecutive returns fall into the same
// 2^(depth-1)-cell lattice block for dozens of points -- so scoring in point order flushes
// the register accumulators only when a lane group's block really changes.  (An unordered
// cloud stays correct: it flushes more often.)  Every lane classifies its own point of a
// 64-point chunk (plane, lattice block); lane group g = lane / 16 takes points 4 t + g, so
// one buffer_load_dword still serves four points, sixteen of them in flight per wave.
// (Wider gathers do not help: the plane reads run at ~8 B/clk per CU whatever the
// instruction width -- buffer_load_dwordx4, sixteen points per instruction, was slower --
// because every point touches its own 64-byte half of a 128-byte L2 line.)
// The integer sums are order-free: results are bit-identical to the sorted variant
// (ScoreCoarsePlanesDwordKernel, kept for CMX_FUSED=0 and for problems this kernel does not
// take).
// Dynamic LDS: pts[group][n_pad] u32 | misc[kFusedMisc] | cand_acc[acc_cap] | point words[waves][64].
constexpr int kFusedMaxPoints = 4096;    // = kPointCache of the tree search
constexpr int kFusedMisc = 128;          // ints of bookkeeping between the cells and the accumulators
constexpr long long kFusedLdsLimit = 64 * 1024;   // dynamic LDS of a launch that does not opt in to more

// Points kFirst .. kFirst + 7 of a lane group (LDS words at a stride of 16 bytes from `base`): the
// low halves into lo[0..7], the high halves into hi[0..7], zero-extended; returns when they landed.
template <int kFirst>
__device__ __forceinline__ void ReadHalves8(unsigned base, uint32_t* lo, uint32_t* hi) {
  constexpr int o = 16 * kFirst;
  asm volatile(
      "ds_read_u16 %0, %16 offset:%17\n\tds_read_u16 %8, %16 offset:%18\n\t"
      "ds_read_u16 %1, %16 offset:%19\n\tds_read_u16 %9, %16 offset:%20\n\t"
      "ds_read_u16 %2, %16 offset:%21\n\tds_read_u16 %10, %16 offset:%22\n\t"
      "ds_read_u16 %3, %16 offset:%23\n\tds_read_u16 %11, %16 offset:%24\n\t"
      "ds_read_u16 %4, %16 offset:%25\n\tds_read_u16 %12, %16 offset:%26\n\t"
      "ds_read_u16 %5, %16 offset:%27\n\tds_read_u16 %13, %16 offset:%28\n\t"
      "ds_read_u16 %6, %16 offset:%29\n\tds_read_u16 %14, %16 offset:%30\n\t"
      "ds_read_u16 %7, %16 offset:%31\n\tds_read_u16 %15, %16 offset:%32\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(lo[0]), "=&v"(lo[1]), "=&v"(lo[2]), "=&v"(lo[3]), "=&v"(lo[4]), "=&v"(lo[5]),
        "=&v"(lo[6]), "=&v"(lo[7]), "=&v"(hi[0]), "=&v"(hi[1]), "=&v"(hi[2]), "=&v"(hi[3]),
        "=&v"(hi[4]), "=&v"(hi[5]), "=&v"(hi[6]), "=&v"(hi[7])
      : "v"(base), "n"(o), "n"(o + 2), "n"(o + 16), "n"(o + 18), "n"(o + 32), "n"(o + 34),
        "n"(o + 48), "n"(o + 50), "n"(o + 64), "n"(o + 66), "n"(o + 80), "n"(o + 82),
        "n"(o + 96), "n"(o + 98), "n"(o + 112), "n"(o + 114)
      : "memory");
}

// The sums of a unit of PrepScoreFusedKernel (below, where the terms are explained): the cells of ONE
// rotation of the unit summed over the phase planes -- the dilated level's under group bounds, the
// level's own otherwise -- and the sums handed to the rotations they stand for.  Everything it needs
// comes out of the block's bookkeeping words in LDS, so that nothing but those is live across the
// gather loop (which fills the 64 VGPRs of eight wavefronts per SIMD on its own: no scratch).
template <bool kTimeline>
__device__ __forceinline__ void FusedPass(const Fast2DProblem& P, ProblemState* state, int n,
                                          int acc_cap, int s0, int timeline_block) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fused_smem[];
  const auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
  const int n_pad = (n + 63) & ~63;
  const int G = P.group > 1 ? kFusedGroup : 1;
  auto* pts_all = reinterpret_cast<uint32_t*>(fused_smem);        // [G][n_pad]
  int* misc = reinterpret_cast<int*>(pts_all + G * n_pad);
  int* cand_acc = misc + kFusedMisc;
  const int T = blockDim.x;
  const int waves = T >> 6;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const auto stamp = [&](int k) {
    if constexpr (kTimeline) Stamp(P.timeline, timeline_block, k);
  };
  const int gcount = uni(misc[1]), gm = uni(misc[2]);
  const bool far = uni(misc[7]) != 0;       // the premise of the group bound failed for this unit
  const int2 dims_all = make_int2(uni(misc[4]), uni(misc[5]));
  const int PI = P.plane_i, PJ = P.plane_j, PIJ = PI * PJ;
  const int shift = P.depth - 1, w = 1 << shift;
  const unsigned zero_plane = 1u << (2 * (P.depth - 1));
  const int group = lane >> 4, sub = lane & 15;
  const int begin = static_cast<int>(static_cast<long long>(n) * wave / waves);
  const int end = static_cast<int>(static_cast<long long>(n) * (wave + 1) / waves);
  constexpr int kSteps = 16;                // all gathers of a 64-point chunk in flight
  uint32_t* const wave_words = reinterpret_cast<uint32_t*>(cand_acc + acc_cap) + 64 * wave;
  const unsigned group_base = static_cast<unsigned>(reinterpret_cast<uintptr_t>(
      (__attribute__((address_space(3))) uint32_t*)(wave_words + group)));
  int2* const scratch = reinterpret_cast<int2*>(misc + 8);      // [4]
  const bool verify = (P.group_verify & 1) != 0;
    const bool group_pass = G > 1;
    const int gp = group_pass ? gm : 0;                  // whose cells are summed
    const uint32_t* const pts = pts_all + gp * n_pad;
    const int* const mine = misc + 16 + 8 * gp;
    const int4 bd = make_int4(uni(mine[0]), uni(mine[1]), uni(mine[2]), uni(mine[3]));
    const int2 dims = group_pass ? dims_all : make_int2(uni(mine[4]), uni(mine[5]));
    const int lift = group_pass ? kGroupDilation : 0;    // (the dilated level is stored two cells up)
    const int pitch = dims.y + 2 * PJ - 2;
    const int BW = dims.x + PI - 1, BH = dims.y + PJ - 1;

  // ---- score in point order (cf. ScoreCoarsePlanesDwordKernel) ------------------------
  int lane_const[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int cell = min(4 * sub + j, PIJ - 1);
    lane_const[j] = (cell % PI + dims.x + PI - 2) * pitch + (cell / PI + dims.y + PJ - 2);
    // (opaque from here on: the flush behind the loop otherwise re-derives the constant from its
    // terms, which then stay live across the loop -- two of them in scratch memory, the gather
    // loop filling the 64 registers).  This steers the register allocator, it does not bind it:
    // after any edit to this function or a compiler change, run tools/kernel_isa_diff.py again
    // and look for private = 0 and vgpr <= 64 on both instantiations of PrepScoreFusedKernel
    // (profiles/fast2d_wave_dive_isa.txt is the last such reading, not a check).
    asm volatile("" : "+v"(lane_const[j]));
  }
  // Four 32-bit running sums, one per plane cell of the lane's dword (round 4's per-chunk stamps:
  // a step of this loop is ~15 issued instructions on a SIMD shared by 4.5 wavefronts -- 1.9 of a
  // chunk's 2.1 us, the gathers themselves land in 0.16 -- so the packed 16-bit pairs, whose
  // overflow guard cost a counter, a compare and a branch per step, are gone: byte k of the dword
  // is added with one (SDWA) instruction each).
  uint32_t cur = 0;                         // lattice block + 1 of the running sums; 0: none yet
  uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  const auto flush = [&]() {
    const int at = static_cast<int>(cur) - 1;
    if (a0) atomicAdd(&cand_acc[lane_const[0] - at], static_cast<int>(a0));
    if (a1) atomicAdd(&cand_acc[lane_const[1] - at], static_cast<int>(a1));
    if (a2) atomicAdd(&cand_acc[lane_const[2] - at], static_cast<int>(a2));
    if (a3) atomicAdd(&cand_acc[lane_const[3] - at], static_cast<int>(a3));
    a0 = a1 = a2 = a3 = 0;
  };
  // (the selected pointer made uniform by hand: the compiler turns the selection into ONE vector
  // load from a selected address, and a resource out of vector registers costs a waterfall loop
  // around every gather)
  const unsigned long long planes_bits =
      reinterpret_cast<unsigned long long>(group_pass ? P.planes_group : P.planes);
  // (readfirstlane returns an int: through `unsigned`, or the low half sign-extends over the high one)
  const unsigned planes_lo = static_cast<unsigned>(
      __builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<unsigned>(planes_bits))));
  const unsigned planes_hi = static_cast<unsigned>(
      __builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<unsigned>(planes_bits >> 32))));
  const uint8_t* const planes_uniform = reinterpret_cast<const uint8_t*>(
      (static_cast<unsigned long long>(planes_hi) << 32) | planes_lo);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(planes_uniform), 0, static_cast<int>((zero_plane + 1) * 64), 0x00020000);
  for (int base_i = begin; base_i < end; base_i += 64) {
    // (instrumented instantiation only -- wavefront 0's first chunk step by step: [8] chunk
    // begins, [9] its sixteen gathers issued, [10] all of them landed, [11] consumed; [12..15]:
    // the next four chunks begin.  profiles/HISTORY.md 5.1: which part of a chunk takes its 2.25 us)
    const int chunk_index = (base_i - begin) >> 6;
    if constexpr (kTimeline) {
      if (chunk_index == 0) stamp(8);
      else if (chunk_index <= 4) stamp(11 + chunk_index);
    }
    // This lane's point of the chunk: byte offset of its phase plane and the constant
    // bx * pitch + by of its lattice block (-1: no candidate of this scan can reach it).
    // ONE word per point: plane index (low half; the zero plane for a point no candidate
    // reaches) and lattice block + 1 (high half; BW, BH <= 255 and the host keeps the pitch so
    // that it fits).  The wavefront parks its 64 words in LDS and a lane group reads point
    // 4 k + group of the chunk at the IMMEDIATE offset 16 k from its own base, as two 16-bit
    // halves: the plane index needs one shift-or to become the gather's offset and the block goes
    // straight into the compare.  (Before: two ds_bpermute and an address add per step; as ONE
    // packed word a shift, a mask and a decrement more -- on the unit the loop is bound by.)
    uint32_t my_word = zero_plane;
    if (base_i + lane < end) {
      const uint32_t packed = pts[base_i + lane];
      const int U = static_cast<short>(packed & 0xffffu) + bd.x + w - 1 + lift;
      const int V = static_cast<short>(packed >> 16) + bd.z + w - 1 + lift;
      const int bx = (U >> shift) + dims.x - 1, by = (V >> shift) + dims.y - 1;
      if (bx >= 0 && bx < BW && by >= 0 && by < BH)
        my_word = static_cast<uint32_t>((V & (w - 1)) * w + (U & (w - 1))) |
                  (static_cast<uint32_t>(bx * pitch + by + 1) << 16);
    }
    wave_words[lane] = my_word;
    __builtin_amdgcn_wave_barrier();
    uint32_t block[kSteps];                            // lattice block + 1; 0: a skipped point
    uint32_t plane[kSteps];
    uint32_t q[kSteps];
    // (inline assembly: written as 16-bit loads in C++, the compiler merges the two halves of a
    // word into one ds_read_b32 and takes them apart again with a mask and a shift per step)
    ReadHalves8<0>(group_base, plane, block);
    ReadHalves8<8>(group_base, plane + 8, block + 8);
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
      q[k] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (plane[k] << 6) | (4 * sub), 0, 0);
    __builtin_amdgcn_wave_barrier();                   // (the next chunk overwrites the words)
    if constexpr (kTimeline) {
      if (chunk_index == 0) {
        stamp(9);
        __builtin_amdgcn_s_waitcnt(0x0f70);      // vmcnt(0): the gathers' latency on its own
        stamp(10);
      }
    }
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
      if (block[k] != cur) {                // per lane group; 0 = skipped point (adds zeros)
        // (cur == 0: nothing has been added but bytes of the zero plane, every sum is 0 and
        // flush() issues no addition -- no second test per step)
        flush();
        cur = block[k];
      }
      a0 += q[k] & 0xffu;
      a1 += (q[k] >> 8) & 0xffu;
      a2 += (q[k] >> 16) & 0xffu;
      a3 += q[k] >> 24;
    }
    if constexpr (kTimeline) {
      if (chunk_index == 0) stamp(11);
    }
  }
  if (cur != 0) flush();
  stamp(4);      // wave 0 done gathering
  __syncthreads();
  stamp(5);      // all waves done

    // ---- the sums of this pass to the rotations they stand for ------------------------------
    // (a unit whose premise failed -- a point's cell, or a bound, further than one from the middle
    // rotation's: not seen so far, the angular step excludes it up to rounding -- keeps the middle
    // rotation's bound, which holds whatever the others do, and gives every candidate of the other
    // rotations the largest sum there is: nothing of them is excluded up here)
    for (int t = 0; t < gcount; ++t) {
      const int s = s0 + t;
      const int2 tdims = make_int2(misc[16 + 8 * t + 4], misc[16 + 8 * t + 5]);
      const int count = tdims.x * tdims.y;
      const int base = s * P.coarse_stride;
      auto* coarse_sum = AsGlobal(P.coarse_sum) + base;
      auto* coarse_score = AsGlobal(P.coarse_score) + base;
      const bool unbounded = far && t != gm;
      int best_sum = -1, best_index = 0x7ffffff;
      for (int i = threadIdx.x; i < count; i += T) {
        const int ix = i / tdims.y, iy = i - ix * tdims.y;
        const int csum = unbounded ? 255 * n : cand_acc[(ix + PI - 1) * pitch + (iy + PJ - 1)];
        if (group_pass) {
          // fast2d_group_verify: the exact sums of an earlier launch (group = 1) are in place
          if (verify && coarse_sum[i] > csum) atomicMax(&state->error, 3);
        } else if (P.write_all_discrete || verify) {
          coarse_sum[i] = csum;     // introspection only
        }
        coarse_score[i] = ToScore(P, csum, n);
        if (csum > best_sum) { best_sum = csum; best_index = i; }
      }
      const int2 best = BlockBest(best_sum, best_index, scratch);
      if (threadIdx.x == 0) P.scan_best[s] = best;
      stamp(6);      // scores written
      // The discretised scan stays on chip: the tree search re-derives the cells of the few scans
      // it descends into (ScanCell).  Only the introspection entry point asks for the array.
      // Batches (store_scans): a scan whose best candidate reaches the initial bound may enter the
      // tree search, where several nodes per scan are expanded by independent wavefronts; its
      // cells are written for them (a superset of what the coarse filter keeps: the bound only
      // rises).  Re-deriving the cells per node made that expansion VALU-bound.
      bool keep_cells = P.write_all_discrete != 0;
      if (!keep_cells && P.store_scans) {
        int top_sum = scratch[0].x;
        for (int k = 1; k < T >> 6; ++k) top_sum = max(top_sum, scratch[k].x);
        keep_cells = !(ToScore(P, top_sum, n) < fmaxf(P.min_score, 0.f));
      }
      if (keep_cells) {
        auto* out = AsGlobal(P.discrete) + static_cast<size_t>(s) * n;
        const uint32_t* const cells = pts_all + t * n_pad;
        for (int i = threadIdx.x; i < n; i += T) out[i] = cells[i];
      }
      __syncthreads();                       // (the next rotation's BlockBest reuses the scratch)
    }
}

template <bool kTimeline>    // (true: the debug switch `timeline`; the shipped instantiation has no stamps)
__global__ void __launch_bounds__(256, 8)   // (eight wavefronts per SIMD: at most 64 VGPRs)
PrepScoreFusedKernel(const Fast2DProblem* __restrict__ problems, const float* __restrict__ xyz,
                     int n, ProblemState* __restrict__ states, int acc_cap,
                     int* __restrict__ counters_words, int num_counter_words) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fused_smem[];
  // First kernel of a fully fused batch: it also clears the list counters of the search.
  // (every workgroup clears a slice: the counters with the work queue's control words are 376 KB)
  if (counters_words)
    for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
         i < num_counter_words; i += gridDim.x * gridDim.y * blockDim.x)
      counters_words[i] = 0;
  const Fast2DProblem& P = problems[blockIdx.y];
  // GROUP BOUNDS (round 6).  Neighbouring rotations move a point by at most one cell (the angular
  // step is chosen so, SM2/correlative_scan_matcher_2d.cc:31-44), and their search bounds -- the
  // minimum over the points -- by at most one with it.  So for the G = 3 rotations g of a unit and
  // the middle one m, the cell a lowest-resolution candidate (kx, ky) of rotation g reads for point
  // p lies within two cells (per axis) of the cell candidate (kx, ky) of rotation m reads for p,
  // and ONE sum of m's cells over the level DILATED by two cells bounds the score of (kx, ky) of
  // all three from above.  Everything behind the front end (dive, filter, tree search) takes a
  // lowest-resolution score as the upper bound of the subtree below it and nothing else, so the
  // bound takes the score's place: a third of the gathers.  What needs the exact scores -- the
  // replay of the reference's std::sort when leaves tie (ResolveTies), depth 1, the introspection
  // entry point -- runs this kernel (again) with group = 1.  The premise is CHECKED per unit (every
  // point's cells, every bound): in a unit that fails it the outer rotations get the largest sum
  // there is, i.e. no bound (FusedPass).  fast2d_group_verify: every bound against the exact sums
  // of a launch with group = 1, on the device.
  const int G = P.group > 1 ? kFusedGroup : 1;
  // Units u, u + 256, u + 512, ... tend to share a CU (u % 8 picks the XCD, round-robin
  // within it): give them ADJACENT rotations.  Neighbouring rotations move a point by less
  // than a cell, so co-resident blocks gather the same or the neighbouring phase plane at
  // about the same time and meet in the CU's L1 instead of each going to L2.  (Any bijection
  // is correct; only speed depends on the dispatch order.)
  const int slots = (gridDim.x + 255) >> 8;
  const int unit = (blockIdx.x & 255) * slots + (blockIdx.x >> 8);
  const int s0 = unit * G;
  if (!P.use_fused || s0 >= P.num_scans) return;
  const int gcount = min(G, P.num_scans - s0);
  const int gm = gcount == 3 ? 1 : 0;       // the rotation of the unit whose cells are summed
  const int n_pad = (n + 63) & ~63;
  auto* pts_all = reinterpret_cast<uint32_t*>(fused_smem);        // [G][n_pad]
  int* misc = reinterpret_cast<int*>(pts_all + G * n_pad);
  int* cand_acc = misc + kFusedMisc;
  // misc: [0, 8) the pass (bounds, dims, ok, grouped) | [8, 16) BlockBest | [16 + 8 g, ...) bounds
  // and dims of rotation g | [40 + 20 g + 5 wave, ...) partials | [100 + wave] cell deltas
  const int T = blockDim.x;              // 128, 192 or 256
  const int waves = T >> 6;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const auto stamp = [&](int k) {
    if constexpr (kTimeline) Stamp(P.timeline, blockIdx.y * gridDim.x + blockIdx.x, k);
  };
  stamp(0);

  // ---- rotate, translate, discretise (PrepScansKernel's arithmetic) ----------
  const bool identity_q0 = P.init_qw == 1.f && P.init_qz == 0.f;
  // The cell of a point from an f32 ESTIMATE of the value the reference rounds,
  //     t = (max - translation) / res - 0.5 - (rotated coordinate) / res,
  // in two FMAs per coordinate (the real-time matcher's discretisation, rt_2d_tiles.hip, where
  // the error bound is derived: the estimate differs from GetCellIndex over RotateZ's f32 chain
  // by less than 2^-24 [((k_z + 4) (|ax| + |ay|) + |translation|) / res + 3 |K|], k_z =
  // max(2 + 4 z^2, 1 + 6 |z|) for this scan's rotation (w, z)); when it lies further than
  // 1.25 x that from every half-integer its rounding IS the reference's cell.  Otherwise -- three
  // points in a thousand at 60 m (20 M random points over the full circle: 0 wrong cells among
  // the decided ones) -- the exact expressions below run for that lane.  ~30 instead of ~110
  // vector instructions per point (a third of this kernel's instructions) -- and no measurable
  // change of its duration (same-box A/B: 132.4 -> 130.4 - 132.5 us per search): the kernel is
  // not bound by instruction issue but by the plane gathers below.
  const double inv_res_d = P.inv_res;
  const double Kyd = (P.max_y - static_cast<double>(P.ty)) * inv_res_d - 0.5;
  const double Kxd = (P.max_x - static_cast<double>(P.tx)) * inv_res_d - 0.5;
  const float Ky = static_cast<float>(Kyd), Kx = static_cast<float>(Kxd);
  const float bound_fixed = static_cast<float>(
      1.25 * 0x1p-24 * (inv_res_d * fmax(fabs(static_cast<double>(P.tx)), fabs(static_cast<double>(P.ty))) +
                        3.0 * fmax(fabs(Kxd), fabs(Kyd)) + 1.0));
  for (int g = 0; g < gcount; ++g) {
    const float2 r = P.scan_rot[s0 + g];
    const double zd = r.y;
    const float Ci = static_cast<float>((1.0 - 2.0 * zd * zd) * inv_res_d);
    const float Si = static_cast<float>(2.0 * static_cast<double>(r.x) * zd * inv_res_d);
    const float bound_per_m = static_cast<float>(
        1.25 * 0x1p-24 * inv_res_d * (4.0 + fmax(2.0 + 4.0 * zd * zd, 1.0 + 6.0 * fabs(zd))));
    uint32_t* const pts = pts_all + g * n_pad;
    int lo_x = 0, lo_y = 0, hi_x = 0, hi_y = 0, bad = 0;
    for (int i0 = threadIdx.x; i0 < n; i0 += 4 * T) {
      // Four points' loads in flight before the first is used.
      F3 p[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = min(i0 + k * T, n - 1);
        p[k] = F3{xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]};
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * T;
        if (i >= n) break;
        // Two yaw rotations (initial estimate, then this scan's perturbation), then the
        // translation: Rotate / `+ 0.f` / `1.f * x + 0.f * y` of PrepScansKernel without the
        // terms that are exactly zero (RotateZ, cmx_device.h).  A full-submap search starts
        // from yaw 0: its first rotation is the identity.
        float ax = p[k].x, ay = p[k].y;
        if (!identity_q0) RotateZ(P.init_qw, P.init_qz, p[k].x, p[k].y, &ax, &ay);
        const float tY = fmaf(-Ci, ay, fmaf(-Si, ax, Ky));    // cell x index from the map's y
        const float tX = fmaf(-Ci, ax, fmaf(Si, ay, Kx));
        const float nY = rintf(tY), nX = rintf(tX);
        const float margin = fminf(0.5f - fabsf(tY - nY), 0.5f - fabsf(tX - nX));
        const float bound = fmaf(fabsf(ax) + fabsf(ay), bound_per_m, bound_fixed);
        int ix, iy;
        if (margin > bound && fabsf(tY) < 1e6f && fabsf(tX) < 1e6f) {     // (NaN: not greater)
          ix = static_cast<int>(nY);
          iy = static_cast<int>(nX);
        } else {
          float bx, by;
          RotateZ(r.x, r.y, ax, ay, &bx, &by);
          const float x = bx + P.tx;
          const float y = by + P.ty;
          // lround((max - v) / res - 0.5), exact (cmx_device.h)
          ix = CellIndexFast(P.max_y, y, P.res, P.inv_res);
          iy = CellIndexFast(P.max_x, x, P.res, P.inv_res);
        }
        if (ix < -32768 || ix > 32767 || iy < -32768 || iy > 32767) bad = 1;
        pts[i] = (static_cast<uint32_t>(ix) & 0xffffu) | (static_cast<uint32_t>(iy) << 16);
        lo_x = min(lo_x, -ix);
        lo_y = min(lo_y, -iy);
        hi_x = max(hi_x, P.nx - 1 - ix);
        hi_y = max(hi_y, P.ny - 1 - iy);
      }
    }
    lo_x = WaveMinDpp(lo_x); lo_y = WaveMinDpp(lo_y);
    hi_x = WaveMaxDpp(hi_x); hi_y = WaveMaxDpp(hi_y);
    bad = WaveMaxDpp(bad);
    if (lane == 0) {
      int* red = misc + 40 + 20 * g + wave * 5;      // [G][4][5]
      red[0] = lo_x; red[1] = lo_y; red[2] = hi_x; red[3] = hi_y; red[4] = bad;
    }
  }
  for (int i = threadIdx.x; i < acc_cap; i += T) cand_acc[i] = 0;
  stamp(1);      // points discretised
  __syncthreads();
  if (gcount > 1) {            // (uniform)
    // the premise of the group bound: no point's cell further than one from the middle rotation's
    int far = 0;
    const uint32_t* const mid = pts_all + gm * n_pad;
    for (int g = 0; g < gcount; ++g) {
      if (g == gm) continue;
      const uint32_t* const other = pts_all + g * n_pad;
      for (int i = threadIdx.x; i < n; i += T) {
        const uint32_t a = mid[i], b = other[i];
        const int dx = static_cast<short>(a & 0xffffu) - static_cast<short>(b & 0xffffu);
        const int dy = static_cast<short>(a >> 16) - static_cast<short>(b >> 16);
        far |= (dx < -1 || dx > 1 || dy < -1 || dy > 1) ? 1 : 0;
      }
    }
    far = WaveMaxDpp(far);
    if (lane == 0) misc[100 + wave] = far;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int step = 1 << (P.depth - 1);
    int bad = 0, far = 0;
    int2 dims_all = make_int2(0, 0);
    for (int g = 0; g < gcount; ++g) {
      const int* red = misc + 40 + 20 * g;
      int lo_x = red[0], lo_y = red[1], hi_x = red[2], hi_y = red[3];
      bad = max(bad, red[4]);
      for (int w = 1; w < waves; ++w) {
        red += 5;
        lo_x = min(lo_x, red[0]); lo_y = min(lo_y, red[1]);
        hi_x = max(hi_x, red[2]); hi_y = max(hi_y, red[3]);
        bad = max(bad, red[4]);
      }
      int4 bd;   // ShrinkToFit
      bd.x = max(-P.nl, lo_x);
      bd.y = min(P.nl, hi_x);
      bd.z = max(-P.nl, lo_y);
      bd.w = min(P.nl, hi_y);
      P.bounds[s0 + g] = bd;
      const int2 dims = make_int2((bd.y - bd.x + step) / step, (bd.w - bd.z + step) / step);
      P.coarse_dims[s0 + g] = dims;
      int* mine = misc + 16 + 8 * g;
      mine[0] = bd.x; mine[1] = bd.y; mine[2] = bd.z; mine[3] = bd.w;
      mine[4] = dims.x; mine[5] = dims.y;
      dims_all.x = max(dims_all.x, dims.x);
      dims_all.y = max(dims_all.y, dims.y);
    }
    if (gcount > 1) {
      far = (P.group_verify & 2) ? 1 : 0;       // (tests: every unit as if its premise had failed)
      for (int w = 0; w < waves; ++w) far |= misc[100 + w];
      for (int g = 0; g < gcount; ++g)
        far |= (abs(misc[16 + 8 * g] - misc[16 + 8 * gm]) > 1 ||
                abs(misc[16 + 8 * g + 2] - misc[16 + 8 * gm + 2]) > 1) ? 1 : 0;
    }
    if (bad) atomicMax(&states[blockIdx.y].error, 1);
    // (checked on the largest candidate grid of the unit: the accumulators of a group pass hold it)
    const int count = dims_all.x * dims_all.y;
    const int BW = dims_all.x + P.plane_i - 1, BH = dims_all.y + P.plane_j - 1;
    // (block + 1 = bx * pitch + by + 1 travels in 16 bits, see the scoring loop)
    const int ok = count <= P.coarse_stride && count <= kMaxCoarsePerScan && BW <= 255 &&
                   BH <= 255 && (BW - 1) * (dims_all.y + 2 * P.plane_j - 2) + BH <= 65535 &&
                   (dims_all.x + 2 * P.plane_i - 2) * (dims_all.y + 2 * P.plane_j - 2) <= acc_cap;
    misc[1] = gcount; misc[2] = gm;
    misc[4] = dims_all.x; misc[5] = dims_all.y;
    misc[6] = ok;
    misc[7] = far;
    if (far) atomicAdd(&states[blockIdx.y].done_top, 1);      // (statistics: units without a group bound)
    if (!ok) {
      atomicMax(&states[blockIdx.y].error, 2);
      for (int g = 0; g < gcount; ++g) P.scan_best[s0 + g] = make_int2(0, 0);
    }
  }
  __syncthreads();
  if (!misc[6]) return;
  stamp(2);      // bounds known
  FusedPass<kTimeline>(P, &states[blockIdx.y], n, acc_cap, s0, blockIdx.y * gridDim.x + blockIdx.x);
  stamp(7);
}

// ---------------------------------------------------------------------------
// Host
// ---------------------------------------------------------------------------
// SearchParameters ctor (SM2/correlative_scan_matcher_2d.cc:27-55), host side.
HostSearch MakeSearch(double linear_window, double angular_window, float max_range_xy,
                      double resolution) {
  float max_scan_range = 3.f * resolution;
  max_scan_range = std::max(max_range_xy, max_scan_range);
  const double kSafetyMargin = 1. - 1e-3;
  const float range_sq = max_scan_range * (max_scan_range * 1.f);
  const double res_sq = resolution * (resolution * 1.);
  HostSearch h;
  h.step = kSafetyMargin * std::acos(1. - res_sq / (2. * range_sq));
  h.num_angular = std::ceil(angular_window / h.step);
  h.num_scans = 2 * h.num_angular + 1;
  h.nl = std::ceil(linear_window / resolution);
  return h;
}

// The debug switch fast2d_unfused routes every problem through the separate prep / score
// launches (the fallback of problems the fused kernel does not take); parity tests run both.
bool FusedEnabled() { return Debug().fast2d_unfused == 0; }

// Blocks of PrepScoreFusedKernel the whole chip holds at once (occupancy query, cached).
long long FusedResidentBlocks(int device, int threads, size_t lds_bytes) {
  struct Key { int device, threads; size_t lds; long long blocks; };
  static std::mutex mu;
  static std::vector<Key>* cache = new std::vector<Key>;
  const size_t lds = (lds_bytes + 1023) & ~size_t(1023);
  {
    std::lock_guard<std::mutex> lock(mu);
    for (const Key& k : *cache)
      if (k.device == device && k.threads == threads && k.lds == lds) return k.blocks;
  }
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, PrepScoreFusedKernel<false>, threads, lds) !=
          hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  // (one fewer per CU than the API says: it over-reports by one for some SGPR counts,
  // MI355X_MICROARCH.md "Residency and cooperative launch")
  const long long blocks = static_cast<long long>(std::max(per_cu - 1, 0)) * cus;
  std::lock_guard<std::mutex> lock(mu);
  if (cache->size() < 256) cache->push_back(Key{device, threads, lds, blocks});
  return blocks;
}

}  // namespace

void FillRotationTable(double step, int num_angular, float2* out) {
  // delta_theta accumulates in f64, each angle is narrowed to f32 for AngleAxisf.
  const int num_scans = 2 * num_angular + 1;
  double delta_theta = -num_angular * step;
  for (int s = 0; s < num_scans; ++s, delta_theta += step) {
    const float ha = 0.5f * static_cast<float>(delta_theta);
    out[s] = make_float2(std::cos(ha), std::sin(ha) * 1.f);
  }
}

std::shared_ptr<const std::vector<float2>> HostRotationTable(double step, int num_angular) {
  struct Entry {
    double step;
    int num_angular;
    std::shared_ptr<const std::vector<float2>> table;
  };
  static std::mutex mu;
  static std::vector<Entry>* cache = new std::vector<Entry>;   // most recent last
  {
    std::lock_guard<std::mutex> lock(mu);
    for (size_t i = cache->size(); i-- > 0;) {
      if ((*cache)[i].step == step && (*cache)[i].num_angular == num_angular)
        return (*cache)[i].table;
    }
  }
  const int num_scans = 2 * num_angular + 1;
  auto table = std::make_shared<std::vector<float2>>(num_scans);
  FillRotationTable(step, num_angular, table->data());
  std::lock_guard<std::mutex> lock(mu);
  if (cache->size() >= 64) cache->erase(cache->begin());      // bound the cache
  cache->push_back(Entry{step, num_angular, table});
  return table;
}

// Every decision of the front end, per problem and per launch (fast_2d_internal.h).
FrontEndPlan PlanFrontEnd(const PlanMatcher* matchers, int num, const int32_t* full_flags,
                          bool full_submap, int n, float max_range_xy, bool write_all_discrete) {
  const auto is_full = [&](int p) { return full_flags ? full_flags[p] != 0 : full_submap; };
  FrontEndPlan plan;
  plan.problems.resize(num);
  const bool fused_enabled = FusedEnabled();
  const long long n_pad = (n + 63) & ~63;
  // Dynamic LDS of PrepScoreFusedKernel: pts | misc | candidate sums | 64 point words per
  // wavefront (at most four).  The kernel does not opt in to more than kFusedLdsLimit.
  const auto fused_lds = [&](int group, long long acc) {
    return 4 * n_pad * group + 4 * (kFusedMisc + acc) + 4 * 256;
  };
  for (int p = 0; p < num; ++p) {
    const PlanMatcher& m = matchers[p];
    const cmx_grid2d_limits& lim = m.limits;
    ProblemPlan& Q = plan.problems[p];
    HostSearch h;
    if (is_full(p)) {
      // SM2/fast_...2d.cc:213-222.
      h = MakeSearch(1e6 * lim.resolution, M_PI, max_range_xy, lim.resolution);
    } else {
      h = MakeSearch(m.linear_search_window, m.angular_search_window, max_range_xy, lim.resolution);
    }
    CMX_REQUIRE(h.num_scans >= 1 && h.num_scans < (1 << 20), "unsupported number of scans %d",
                h.num_scans);
    Q.search = h;
    plan.max_scans = std::max(plan.max_scans, h.num_scans);
    // Upper bound of lowest-resolution candidates per scan: the shrunk window
    // never exceeds nx-1 plus the cell spread of the scan, nor 2*nl.
    const int step = 1 << (m.depth - 1);
    const double spread_cells = 2.0 * (std::max(max_range_xy, 0.f) / lim.resolution + 2.0);
    auto per_axis = [&](int cells) {
      const double width = std::min(2.0 * h.nl, cells - 1 + spread_cells);
      return static_cast<long long>(width / step) + 2;
    };
    const long long ax = per_axis(lim.num_x_cells), ay = per_axis(lim.num_y_cells);
    CMX_REQUIRE(ax * ay * h.num_scans < (1ll << 30),
                "search too large: %lld lowest-resolution candidates", ax * ay * h.num_scans);
    Q.ax = ax;
    Q.ay = ay;
    Q.use_planes = m.planes && ax * ay <= kMaxCoarsePerScan &&
                   (ax + m.plane_i - 1) * (ay + m.plane_j - 1) <= kMaxBuckets &&
                   ax + m.plane_i - 1 <= 255 && ay + m.plane_j - 1 <= 255 &&   // 8-bit bx, by
                   (ax + 2 * m.plane_i - 2) * (ay + 2 * m.plane_j - 2) <= kMaxAccCells &&
                   m.depth > 1;
    const long long acc = (ax + 2 * m.plane_i - 2) * (ay + 2 * m.plane_j - 2);
    Q.acc = acc;
    if (Q.use_planes) plan.plane_acc_cells = std::max(plan.plane_acc_cells, acc);
    // Fused front end: 64-byte planes, the scan + the accumulators within the 64 KB of
    // dynamic LDS a launch gets without opting in to more.
    // (... and the lattice block of a point + 1 within 16 bits: the fused kernel's point words)
    Q.use_fused = fused_enabled && Q.use_planes && m.plane_stride == 64 &&
                  n <= kFusedMaxPoints && fused_lds(1, acc) <= kFusedLdsLimit &&
                  (ax + m.plane_i - 2) * (ay + 2 * m.plane_j - 2) + (ay + m.plane_j - 1) <= 65535;
    if (Q.use_fused) {
      plan.any_fused = true;
      plan.fused_acc = std::max(plan.fused_acc, acc);
    } else {
      plan.any_unfused = true;
    }
    // Group bounds: three rotations per workgroup, one sum over the dilated level (the kernel's
    // long comment).  Not for the callers that need every exact lowest-resolution score
    // (introspection, depth 1), not where two cells of dilation are a large part of the
    // lowest-resolution window (below 16 cells the bounds stop excluding anything).
    // fast2d_group: 1 never, 2 whenever the planes exist.
    const int sw = Debug().fast2d_group;
    const bool wanted = sw == 1 ? false : sw == 2 ? true : m.depth >= 5;
    Q.group = (wanted && Q.use_fused && m.planes_group && m.depth > 1 && !write_all_discrete &&
               h.num_scans >= kFusedGroup && fused_lds(kFusedGroup, acc) <= kFusedLdsLimit)
                  ? kFusedGroup : 1;
    if (Q.group > 1) plan.any_group = true;
  }
  if (plan.any_fused) {
    // The launch is ONE for all fused problems of the call: three scans of points as soon as any
    // problem is grouped, the accumulators of the largest problem -- which need not be a grouped
    // one.  Either fitted on its own; where the two together do not, nobody is grouped (every
    // rotation summed on the level itself: same results, the sums are exact instead of bounds).
    if (plan.any_group && fused_lds(kFusedGroup, plan.fused_acc) > kFusedLdsLimit) {
      for (ProblemPlan& Q : plan.problems) Q.group = 1;
      plan.any_group = false;
    }
    // (units of a launch: rotations, or groups of three; a batch that mixes both is sized for
    // single rotations -- surplus workgroups of a grouped problem return at once)
    bool all_group = true;
    for (const ProblemPlan& Q : plan.problems) all_group = all_group && (!Q.use_fused || Q.group > 1);
    plan.per_unit = all_group ? kFusedGroup : 1;
    plan.fused_lds = static_cast<size_t>(fused_lds(plan.any_group ? kFusedGroup : 1, plan.fused_acc));
    CMX_REQUIRE(plan.fused_lds <= static_cast<size_t>(kFusedLdsLimit),
                "internal error: the fused front end planned %zu bytes of LDS", plan.fused_lds);
  }
  return plan;
}

// Uploads problem descriptors, carves scratch and runs the preparation +
// lowest-resolution scoring kernels.  `d_xyz` is the device point cloud.
void PrepareAndScoreCoarse(Workspace& ws, const Fast2DMatcher* const* matchers, int num,
                           const cmx_pose2d* initial_or_null, bool full_submap,
                           const float* d_xyz, int n, float max_range_xy, float min_score,
                           PreparedBatch* out, const int32_t* full_flags,
                           const float* min_scores) {
  // Mixed batches (the ConstraintBuilder front): per-problem full-submap flag and
  // acceptance threshold override the uniform ones.
  const auto is_full = [&](int p) { return full_flags ? full_flags[p] != 0 : full_submap; };
  const auto min_of = [&](int p) { return min_scores ? min_scores[p] : min_score; };
  out->num_problems = num;
  out->n = n;
  out->search.resize(num);
  out->initial.resize(num);
  out->h_problems.resize(num);

  std::vector<PlanMatcher> views(num);
  for (int p = 0; p < num; ++p) views[p] = PlanMatcherOf(*matchers[p]);
  const FrontEndPlan plan = PlanFrontEnd(views.data(), num, full_flags, full_submap, n, max_range_xy,
                                         out->write_all_discrete);
  out->plane_acc_cells = std::max(out->plane_acc_cells, plan.plane_acc_cells);
  out->any_group = plan.any_group;
  const long long fused_acc = plan.fused_acc;
  const bool any_fused = plan.any_fused, any_unfused = plan.any_unfused;

  // Per-problem search parameters and scratch sizes.
  size_t discrete_total = 0, scans_total = 0, coarse_total = 0;
  // Rotation tables (host libm values, cached process-wide) of the distinct
  // (step, num_angular) pairs of this batch; they travel in the problem upload.
  struct Rotation { double step; int num_angular; std::shared_ptr<const std::vector<float2>> table; size_t offset; };
  std::vector<Rotation> rotations;
  std::vector<int> rotation_of(num);
  size_t rotation_floats = 0;
  for (int p = 0; p < num; ++p) {
    const Fast2DMatcher& m = *matchers[p];
    const cmx_grid2d_limits& lim = m.limits();
    const ProblemPlan& Q = plan.problems[p];
    const HostSearch& h = Q.search;
    cmx_pose2d init;
    if (is_full(p)) {
      // SM2/fast_...2d.cc:213-222.
      init.x = lim.max_x - 0.5 * lim.resolution * lim.num_y_cells;
      init.y = lim.max_y - 0.5 * lim.resolution * lim.num_x_cells;
      init.theta = 0.;
    } else {
      init = initial_or_null[p];
    }
    out->search[p] = h;
    out->initial[p] = init;
    int r = -1;
    for (size_t k = 0; k < rotations.size(); ++k)
      if (rotations[k].step == h.step && rotations[k].num_angular == h.num_angular) r = static_cast<int>(k);
    if (r < 0) {
      r = static_cast<int>(rotations.size());
      rotations.push_back(Rotation{h.step, h.num_angular, HostRotationTable(h.step, h.num_angular),
                                   rotation_floats});
      rotation_floats += 2 * static_cast<size_t>(h.num_scans);
    }
    rotation_of[p] = r;
    discrete_total += static_cast<size_t>(h.num_scans) * n;
    scans_total += h.num_scans + 1;
    const long long cap = Q.ax * Q.ay * h.num_scans;
    Fast2DProblem& P = out->h_problems[p];
    P.coarse_capacity = static_cast<int>(cap);
    P.coarse_stride = static_cast<int>(Q.ax * Q.ay);
    P.use_planes = Q.use_planes;
    P.use_fused = Q.use_fused;
    P.write_all_discrete = out->write_all_discrete ? 1 : 0;
    P.group = Q.group;
    P.group_verify = Debug().fast2d_group_verify;
    P.timeline = nullptr;
    coarse_total += cap;
  }

  // Scratch carving.  The bucketed records exist in HBM only for unfused problems.
  uint32_t* d_discrete =
      ws.dev[2].ReserveAs<uint32_t>(discrete_total + (any_unfused ? 2 * discrete_total + 2 : 0));
  uint2* d_sorted = reinterpret_cast<uint2*>(d_discrete + discrete_total + (discrete_total & 1));
  int4* d_bounds = ws.dev[3].ReserveAs<int4>(scans_total);
  int2* d_dims = ws.dev[4].ReserveAs<int2>(2 * scans_total);
  int2* d_scan_best = d_dims + scans_total;
  int* d_sorted_count = ws.dev[5].ReserveAs<int>(scans_total);
  float* d_cscore = ws.dev[6].ReserveAs<float>(coarse_total);
  int* d_csum = ws.dev[7].ReserveAs<int>(coarse_total);
  const size_t problems_bytes = (num * sizeof(Fast2DProblem) + 255) & ~size_t(255);
  const size_t states_bytes = (num * sizeof(ProblemState) + 255) & ~size_t(255);
  const size_t upload_bytes = problems_bytes + states_bytes + rotation_floats * sizeof(float);
  char* d_upload = static_cast<char*>(ws.dev[8].Reserve(upload_bytes));
  out->d_problems = reinterpret_cast<Fast2DProblem*>(d_upload);
  out->d_states = reinterpret_cast<ProblemState*>(d_upload + problems_bytes);
  const float* d_rotations = reinterpret_cast<const float*>(d_upload + problems_bytes + states_bytes);
  char* h_upload = static_cast<char*>(ws.pinned[1].Reserve(upload_bytes));
  Fast2DProblem* h_prob = reinterpret_cast<Fast2DProblem*>(h_upload);
  ProblemState* h_state = reinterpret_cast<ProblemState*>(h_upload + problems_bytes);
  float* h_rotations = reinterpret_cast<float*>(h_upload + problems_bytes + states_bytes);
  for (const Rotation& r : rotations)
    std::memcpy(h_rotations + r.offset, r.table->data(), r.table->size() * sizeof(float2));

  if (TimelineEnabled() && any_fused) {
    int max_scans = 0;
    for (const HostSearch& h : out->search) max_scans = std::max(max_scans, h.num_scans);
    out->timeline_blocks = (max_scans + 255) / 256 * 256 * num;
    const size_t bytes = static_cast<size_t>(out->timeline_blocks) * kTimelineStamps * 8;
    out->d_timeline = static_cast<unsigned long long*>(ws.dev[15].Reserve(bytes));
    CMX_HIP(hipMemsetAsync(out->d_timeline, 0, bytes, ws.stream));
  }
  // Batches and the work-queue search keep the cells of surviving scans (debug switch
  // fast2d_store_scans overrides).
  const int store_override = Debug().fast2d_store_scans;
  const int store_scans =
      store_override ? store_override - 1 : ((num >= 4 || QueueSearchWanted(n, num)) ? 1 : 0);
  size_t disc_off = 0, scan_off = 0, coarse_off = 0;
  for (int p = 0; p < num; ++p) {
    const Fast2DMatcher& m = *matchers[p];
    const cmx_grid2d_limits& lim = m.limits();
    const HostSearch& h = out->search[p];
    Fast2DProblem& P = out->h_problems[p];
    P.timeline = out->d_timeline;
    P.xyz = d_xyz;
    P.recompute_scans = (P.use_fused && !P.write_all_discrete) ? 1 : 0;
    P.store_scans = store_scans;
    for (int i = 0; i < m.depth(); ++i) P.level[i] = m.level(i);
    P.depth = m.depth();
    P.nx = lim.num_x_cells; P.ny = lim.num_y_cells;
    P.nl = h.nl;
    P.res = lim.resolution; P.max_x = lim.max_x; P.max_y = lim.max_y;
    P.tx = static_cast<float>(out->initial[p].x);
    P.ty = static_cast<float>(out->initial[p].y);
    {  // Quaternion(AngleAxisf(initial_rotation.cast<float>().angle(), Z))
      const float ha = 0.5f * static_cast<float>(out->initial[p].theta);
      P.init_qw = std::cos(ha);
      P.init_qz = std::sin(ha) * 1.f;
    }
    P.num_scans = h.num_scans;
    P.inv_res = 1.0 / P.res;
    P.scan_rot = reinterpret_cast<const float2*>(d_rotations + rotations[rotation_of[p]].offset);
    P.min_s = m.min_s();
    P.score_scale = m.score_scale();
    P.min_score = min_of(p);
    P.planes = m.planes();
    P.planes_group = m.planes_group();
    P.plane_i = m.plane_i();
    P.plane_j = m.plane_j();
    P.plane_stride = m.plane_stride();
    P.discrete = d_discrete + disc_off;
    P.sorted = d_sorted + disc_off;
    P.bounds = d_bounds + scan_off;
    P.coarse_dims = d_dims + scan_off;
    P.scan_best = d_scan_best + scan_off;
    P.sorted_count = d_sorted_count + scan_off;
    P.coarse_score = d_cscore + coarse_off;
    P.coarse_sum = d_csum + coarse_off;
    h_prob[p] = P;
    std::memset(&h_state[p], 0, sizeof(ProblemState));
    const float bound = std::max(min_of(p), 0.f);
    std::memcpy(&h_state[p].best_bits, &bound, sizeof(float));
    disc_off += static_cast<size_t>(h.num_scans) * n;
    scan_off += h.num_scans + 1;
    coarse_off += P.coarse_capacity;
    out->max_scans = std::max(out->max_scans, h.num_scans);
  }
  // (from here to the end of this function: the call's turn at the runtime's launch path)
  LaunchTurn turn;
  // One H2D for the problem descriptors, their initial states and the rotation tables.
  SmallCopyAsync(d_upload, h_upload, upload_bytes, /*to_device=*/true, ws.stream);

  const dim3 per_scan(out->max_scans, num);
  auto mark = [&](const char* name) { if (out->trace) out->trace->Mark(name); };
  mark("upload");
  // Whichever kernel runs first clears the search's list counters.
  int* clear_words = reinterpret_cast<int*>(out->d_misc);
  const int clear_count = out->d_misc ? out->num_counter_words : 0;
  RecordEvent(ws.ev_k0, ws.stream);
  if (any_fused) {
    // Threads per block: with 192 (three waves) ten blocks fit a CU, i.e. a single search's
    // ~2300 rotations are all resident at once and the launch takes one block's latency;
    // batches run several rounds anyway and use full 256-thread blocks.
    // (units and LDS of the launch: PlanFrontEnd)
    const int per_unit = plan.per_unit;
    const int units = (out->max_scans + per_unit - 1) / per_unit;
    const long long blocks = static_cast<long long>(units) * num;
    const size_t lds = plan.fused_lds;
    out->fused_lds = lds;
    out->fused_acc = static_cast<int>(fused_acc);
    out->d_xyz = d_xyz;
    int threads = 256;
    for (int t : {256, 192, 128}) {
      if (blocks <= FusedResidentBlocks(ws.device, t, lds)) { threads = t; break; }
    }
    if (Debug().fast2d_fused_threads > 0) threads = Debug().fast2d_fused_threads;   // experiments
    if (out->trace && out->trace->enabled())
      fprintf(stderr, "[cmx trace] fused front end: %lld blocks x %d threads, %zu B LDS\n", blocks,
              threads, lds);
    // (grid.x rounded up to a multiple of 256 for the rotation -> block map of the kernel)
    const dim3 fused_grid((units + 255) / 256 * 256, num);
    out->fused_threads = threads;
    if (out->any_group && (Debug().fast2d_group_verify & 1)) {
      // Verification of the group bounds: first every rotation on the level itself (the same
      // descriptors with group = 1; the exact sums stay in coarse_sum), then the launch proper,
      // which compares every bound with them (error 3).
      std::vector<Fast2DProblem> exact(out->h_problems);
      for (Fast2DProblem& P : exact) { P.group = 1; P.store_scans = 0; }
      Fast2DProblem* d_exact = ws.dev[16].ReserveAs<Fast2DProblem>(num);
      CMX_HIP(hipMemcpyAsync(d_exact, exact.data(), num * sizeof(Fast2DProblem), hipMemcpyHostToDevice,
                             ws.stream));
      CMX_HIP(hipStreamSynchronize(ws.stream));        // (`exact` is a local)
      const dim3 exact_grid((out->max_scans + 255) / 256 * 256, num);
      PrepScoreFusedKernel<false><<<exact_grid, threads, lds, ws.stream>>>(
          d_exact, d_xyz, n, out->d_states, static_cast<int>(fused_acc), clear_words, clear_count);
      clear_words = nullptr;
    }
    (out->d_timeline ? PrepScoreFusedKernel<true> : PrepScoreFusedKernel<false>)
        <<<fused_grid, threads, lds, ws.stream>>>(out->d_problems, d_xyz, n, out->d_states,
                                                  static_cast<int>(fused_acc), clear_words,
                                                  clear_count);
    clear_words = nullptr;
    mark("fused");
  }
  if (any_unfused) {
    PrepScansKernel<<<per_scan, 256, 0, ws.stream>>>(out->d_problems, d_xyz, n, out->d_states,
                                                     clear_words, clear_count);
    mark("prep");
    bool any_generic = false;
    int chunk_mask = 0;
    for (const Fast2DProblem& P : out->h_problems) {
      if (P.use_fused) continue;
      if (P.use_planes) chunk_mask |= 1 << (P.plane_stride >> 6);
      else any_generic = true;
    }
    const size_t acc_bytes = static_cast<size_t>(out->plane_acc_cells) * sizeof(int);
    const int plane_threads = 256;
    if (chunk_mask & (1 << 1))
      ScoreCoarsePlanesDwordKernel<<<per_scan, plane_threads, acc_bytes, ws.stream>>>(
          out->d_problems, n, out->d_states);
    if (chunk_mask & (1 << 2))
      ScoreCoarsePlanesKernel<2><<<per_scan, plane_threads, acc_bytes, ws.stream>>>(
          out->d_problems, n, out->d_states);
    if (chunk_mask & (1 << 3))
      ScoreCoarsePlanesKernel<3><<<per_scan, plane_threads, acc_bytes, ws.stream>>>(
          out->d_problems, n, out->d_states);
    if (chunk_mask & (1 << 4))
      ScoreCoarsePlanesKernel<4><<<per_scan, plane_threads, acc_bytes, ws.stream>>>(
          out->d_problems, n, out->d_states);
    if (any_generic)
      ScoreCoarseGenericKernel<<<per_scan, 256, 0, ws.stream>>>(out->d_problems, n, out->d_states);
    mark("coarse");
  }
  RecordEvent(ws.ev_k1, ws.stream);
  CMX_HIP(hipGetLastError());
}

// Under group bounds the lowest-resolution scores of a problem are upper bounds shared by three
// rotations.  The replay of the reference's order needs the scores themselves: the fused front
// end once more for THIS problem, every rotation summed on the level itself (group = 1; same
// buffers, the search is over).  Rare: leaves that tie for the best score.
void RescoreExact(Workspace& ws, const PreparedBatch& batch, int p) {
  Fast2DProblem P = batch.h_problems[p];
  if (P.group <= 1) return;
  P.group = 1;
  P.group_verify = 0;
  P.store_scans = 0;
  P.timeline = nullptr;
  CMX_HIP(hipMemcpyAsync(batch.d_problems + p, &P, sizeof(P), hipMemcpyHostToDevice, ws.stream));
  CMX_HIP(hipStreamSynchronize(ws.stream));          // (`P` is a local)
  const dim3 grid((P.num_scans + 255) / 256 * 256, 1);
  PrepScoreFusedKernel<false><<<grid, batch.fused_threads, batch.fused_lds, ws.stream>>>(
      batch.d_problems + p, batch.d_xyz, batch.n, batch.d_states + p, batch.fused_acc, nullptr, 0);
  CMX_HIP(hipGetLastError());
  CMX_HIP(hipStreamSynchronize(ws.stream));
}

}  // namespace cmx
