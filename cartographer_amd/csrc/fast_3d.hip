// FastCorrelativeScanMatcher3D on gfx950.
//
// Reference behaviour being replaced (SM3 = cartographer/mapping/internal/3d/scan_matching):
//   SM3/precomputation_grid_3d.cc:49-81              ConvertToPrecomputationGrid / PrecomputeGrid
//   SM3/fast_correlative_scan_matcher_3d.cc:57-77    PrecomputationGridStack3D
//   SM3/fast_correlative_scan_matcher_3d.cc:127-198  Match / MatchFullSubmap / MatchWithSearchParameters
//   SM3/fast_correlative_scan_matcher_3d.cc:200-295  DiscretizeScan / GenerateDiscreteScans
//   SM3/fast_correlative_scan_matcher_3d.cc:297-440  candidates, ScoreCandidates, BranchAndBound
//   SM3/rotational_scan_matcher.cc:121-189           histogram yaw pre-filter (host: A x bins work)
//   SM3/low_resolution_matcher.cc:23-35              leaf verification
//
// Host / device split.  Everything that involves libm (acos, sin, cos, atan2)
// or Eigen-ordered quaternion algebra on a handful of values runs on the host
// with the reference's operation order; the device does the N-point work:
// discretising every surviving yaw, scoring every lowest-resolution candidate,
// and the branch and bound (one wave per node, eight children scored per
// point), including the low-resolution verification of leaves.
//
// This unit is the branch and bound.  The precomputation stack is fast_3d_stack.hip, the front end
// of a chain of launches (staging, discretisation, lowest-resolution scoring) fast_3d_coarse.hip,
// the host side of a search (yaw pre-filter, batching, tie resolution, C ABI) fast_3d_match.hip;
// fast_3d_internal.h says what they share.
#include <algorithm>
#include <cstring>

#include "../../include/cartographer_mi355x_debug.h"
#include "fast_3d_internal.h"

namespace cmx {
namespace {

typedef int I4 __attribute__((ext_vector_type(4)));   // (an int4 the compiler can load from address space 1)

__device__ __forceinline__ Node3D CoarseNode3D(const Fast3DProblem& P, int c) {
  const int per_scan = P.ncx * P.ncy * P.ncz;
  const int step = 1 << (P.depth - 1);
  const int s = c / per_scan;
  int r = c - s * per_scan;
  const int iz = r / (P.ncy * P.ncx);
  r -= iz * P.ncy * P.ncx;
  const int iy = r / P.ncx, ix = r - iy * P.ncx;
  Node3D nd;
  nd.level = P.depth - 1;
  nd.scan = s;
  nd.ox = -P.wxy + ix * step; nd.oy = -P.wxy + iy * step; nd.oz = -P.wz + iz * step;
  nd.score = P.coarse_score[c];
  nd.coarse_score = nd.score;
  nd.coarse_index = c;
  nd.path = 0;
  nd.low_resolution_score = 0.f;
  nd.problem = P.index;
  nd.family = 1;
  nd.pad = 0;
  return nd;
}

__device__ __forceinline__ bool Push3(const List3& list, int sub, int slot, const Node3D& nd) {
  if (slot >= list.sub_capacity) return false;
  list.nodes[static_cast<size_t>(sub) * list.sub_capacity + slot] = nd;
  return true;
}
__device__ __forceinline__ int ListMax3(const List3& list) {
  return WaveMax(min(list.counts[(threadIdx.x & 63) * kCountStride3], list.sub_capacity));
}

// Seeds of the dive: the ~64 best lowest-resolution candidates (histogram
// threshold on the scores).
__global__ void __launch_bounds__(1024)
SeedSelect3DKernel(const Fast3DProblem* __restrict__ problems) {
  const Fast3DProblem& P = problems[blockIdx.x];
  const List3 seeds{P.seeds, P.seed_count, kSeeds3};
  __shared__ int hist[1024];
  __shared__ int threshold_bin;
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int total = P.ncx * P.ncy * P.ncz * P.num_scans;
  auto bin_of = [](float score) {   // scores lie in [0.1, 0.9]
    return min(1023, max(0, static_cast<int>((score - 0.1f) * (1023.f / 0.8f))));
  };
  for (int c = threadIdx.x; c < total; c += blockDim.x) atomicAdd(&hist[bin_of(P.coarse_score[c])], 1);
  __syncthreads();
  // threshold_bin = the largest b >= 1 with sum_{j >= b} hist[j] >= kSeeds3, else 0 -- found
  // by one wave (16 bins per lane, suffix sums across lanes) instead of a 1023-step serial
  // walk by one thread (51 us when there are fewer than kSeeds3 candidates).
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) mine += hist[16 * l + k];
    int suffix = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_down(suffix, off, 64);
      if (l + off < 64) suffix += o;
    }
    const unsigned long long reach = __ballot(suffix >= kSeeds3);
    if (reach == 0) {
      if (l == 0) threshold_bin = 0;
    } else {
      const int owner = 63 - __clzll(reach);          // highest lane whose suffix reaches it
      const int above = suffix - mine;                 // bins of the lanes above
      if (l == owner) {
        int acc = above, b = 16 * l + 15;
        for (; b > 16 * l; --b) {
          acc += hist[b];
          if (acc >= kSeeds3) break;
        }
        threshold_bin = b;     // b == 16 l: reached with the lane's lowest bin (0 only for l == 0)
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < total; c += blockDim.x) {
    const float sc = P.coarse_score[c];
    if (bin_of(sc) >= threshold_bin && sc > P.min_score) {
      const int slot = atomicAdd(&seeds.counts[0], 1);
      if (slot < kSeeds3) Push3(seeds, 0, slot, CoarseNode3D(P, c));
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) seeds.counts[0] = min(seeds.counts[0], kSeeds3);   // only kSeeds3 stored
}

// Lowest-resolution nodes that can still matter (reference: :405-408).
// grid (blocks, problems)
__global__ void __launch_bounds__(256)
Filter3DKernel(const Fast3DProblem* __restrict__ problems, int strict, int chunk, int num_chunks,
               int affinity, List3 out, Counters3* __restrict__ counters) {
  const Fast3DProblem& P = problems[blockIdx.y];
  const int total = P.ncx * P.ncy * P.ncz * P.num_scans;
  const float best = __uint_as_float(*P.best_bits);
  // With `affinity` the nodes of a problem stay in the sub-lists the workgroups of ONE XCD
  // read (sub % 8 == problem % 8, see Expand3DKernel): lines of its grids that neighbouring
  // nodes share are then found in that XCD's L2 instead of being fetched by eight.
  const int sub = affinity ? (blockIdx.y & 7) | ((blockIdx.x & 7) << 3)
                           : blockIdx.x & (kSubLists3 - 1);
  // One reservation per wavefront: the survivors among 64 consecutive candidates (neighbours
  // in x, then y, z) take consecutive slots, so that nodes which read the same cache lines sit
  // next to each other in the list and are expanded at about the same time.
  const int lane = threadIdx.x & 63;
  for (int c0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63); c0 < total;
       c0 += gridDim.x * blockDim.x) {
    const int c = c0 + lane;
    bool keep = false;
    if (c < total && c % num_chunks == chunk) {
      const float sc = P.coarse_score[c];
      keep = strict ? (sc > best) : (sc >= best);
    }
    const unsigned long long mask = __ballot(keep);
    if (mask == 0) continue;
    int first = 0;
    if (lane == 0) first = atomicAdd(&out.counts[sub * kCountStride3], __popcll(mask));
    first = __builtin_amdgcn_readfirstlane(first);
    if (keep && !Push3(out, sub, first + __popcll(mask & ((1ull << lane) - 1)), CoarseNode3D(P, c)))
      counters->overflow = 1;
  }
}

// CreateLowResolutionMatcher's lambda (SM3/low_resolution_matcher.cc:23-35) for the pose
// of one leaf, by a whole block: the per-point probabilities are computed in parallel
// into LDS, then summed sequentially in point order (as the reference does) by every
// thread from LDS broadcasts.
constexpr int kLowChunk = 2048;

__device__ __forceinline__ float LowResolutionScore(const Fast3DProblem& P, const Quat& q, float tx,
                                                    float ty, float tz, float* prob /*[kLowChunk]*/) {
  float acc = 0.f;
  for (int base = 0; base < P.n_low; base += kLowChunk) {
    const int cnt = min(kLowChunk, P.n_low - base);
    __syncthreads();                                   // previous chunk consumed
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
      const float* xyz = P.low_xyz + 3 * static_cast<size_t>(base + i);
      const F3 r = Rotate(q, F3{xyz[0], xyz[1], xyz[2]});
      const F3 t{r.x + tx, r.y + ty, r.z + tz};
      const int3 c = CellIndex3(t, P.low_resolution);
      prob[i] = ValueToProbabilityDev(BrickValueU16(P.low, c.x, c.y, c.z));
    }
    __syncthreads();
#pragma unroll 8
    for (int i = 0; i < cnt; ++i) acc += prob[i];
  }
  return acc / static_cast<float>(P.n_low);
}

// Debug switch fast3d_byte_loads (tools / tests): every child cell with its own byte load.
__device__ int g_fast3d_byte_loads = 0;

// Which loads sum the children of a node whose two x positions lie `dx` cells apart at the child
// level (oct words O): ChildSums3D and FamilySums3D ask here, nowhere else.  `family`: the node
// leads a family of 2 .. 8; the family loop takes it only with at most 256 points per lane
// (`stride` lanes share `n` points), else its members go one by one.
enum SumsPath3D {
  kSumsOctBuffer = CMX_FAST3D_SUMS_OCT_BUFFER,  // oct words through a buffer resource, packed 16-bit accumulators
  kSumsOctPlain = CMX_FAST3D_SUMS_OCT_PLAIN,  // oct words through plain loads (an oct array of 2 GB or more)
  kSumsWindows = CMX_FAST3D_SUMS_WINDOWS,  // no oct words, dx <= 4: four 8-byte windows per point
  kSumsBytes = CMX_FAST3D_SUMS_BYTES,  // one byte load per child cell
  kSumsFamily = CMX_FAST3D_SUMS_FAMILY,  // FamilyLoop3D
};
__device__ __forceinline__ int SumsPath3DOf(const OctDesc& O, int dx, bool family, int n,
                                            int stride) {
  if (O.cells != nullptr && O.s == dx && !g_fast3d_byte_loads) {
    const bool buffer = OctBytes(O) != 0;
    if (family && buffer && n <= 256 * stride) return kSumsFamily;   // (packed sums: FamilyLoop3D)
    return buffer ? kSumsOctBuffer : kSumsOctPlain;
  }
  return dx <= 4 && !g_fast3d_byte_loads ? kSumsWindows : kSumsBytes;
}

// Integer sums of the <= 8 children of `nd` over the points first, first + stride, ...
// (ScoreCandidates at the child level, :332-355): the eight child cells of a point are addressed
// from per-axis clamped offsets (two positions per axis), loads of several points in flight.
// Returns the path that summed them.
__device__ __forceinline__ int ChildSums3D(const Fast3DProblem& P, const Node3D& nd, int first,
                                           int stride, int sum[8]) {
  {
    const int child_depth = nd.level - 1;
    const int half = 1 << child_depth;
    const int e = max(0, child_depth - P.full_resolution_depth + 1);
    const Brick L = P.level[child_depth];
    const uint8_t* __restrict__ cells8 = static_cast<const uint8_t*>(L.cells);
    const int4* __restrict__ cells = P.cells + static_cast<size_t>(nd.scan) * P.n;
    // Shifted offsets of the 2 positions per axis, relative to the brick origin.
    const int fx[2] = {(nd.ox >> e) - L.lo_x, ((nd.ox + half) >> e) - L.lo_x};
    const int fy[2] = {(nd.oy >> e) - L.lo_y, ((nd.oy + half) >> e) - L.lo_y};
    const int fz[2] = {(nd.oz >> e) - L.lo_z, ((nd.oz + half) >> e) - L.lo_z};
    const int row = L.nx, slab = L.nx * L.ny;
    // The two x positions of a point lie dx = fx[1] - fx[0] cells apart in one row (1, 2 or 4
    // for the usual full_resolution_depth <= 3).  Up to dx == 4 ONE aligned 8-byte load serves
    // both: half the gather instructions of the search, which are what bounds it.
    const int dx = fx[1] - fx[0];
    const OctDesc O = P.oct[child_depth];
    const int path = SumsPath3DOf(O, dx, false, P.n, stride);
    if (path == kSumsOctBuffer || path == kSumsOctPlain) {
      // One 8-byte gather per point: the eight child cells (see OctDesc).  Bytes are summed
      // as packed 16-bit pairs, widened every 256 points.
      const int ox = fx[0] + O.s, oy = fy[0] + O.s, oz = fz[0] + O.s;
      // (round 4: through a buffer resource when the array is addressable by one -- the plain
      // `O.cells[inside ? index : 0]` was a flat load under an exec mask with a wait of its
      // own, so the four gathers of the unrolled loop went out one after the other)
      const unsigned long long oct_bytes = OctBytes(O);
      const __amdgpu_buffer_rsrc_t oct = UniformBuffer(O.cells, oct_bytes);
      const auto* gcells = AsGlobal(reinterpret_cast<const I4*>(cells));
      const int n = P.n, wxy = P.wxy, wz = P.wz;
      typedef unsigned U2 __attribute__((ext_vector_type(2)));
      for (int q0 = first; q0 < n; q0 += 256 * stride) {
        unsigned e0 = 0, o0 = 0, e1 = 0, o1 = 0;
        const int stop = min(n, q0 + 256 * stride);
        if (path == kSumsOctBuffer) {
          constexpr int kPoints = 4;             // cells first, then their four gathers
          for (int q = q0; q < stop; q += kPoints * stride) {
            I4 cv[kPoints];
#pragma unroll
            for (int u = 0; u < kPoints; ++u) cv[u] = gcells[min(q + u * stride, n - 1)];
            U2 w[kPoints];
#pragma unroll
            for (int u = 0; u < kPoints; ++u) {
              const int3 d = DepthIndexAny(cv[u].x, cv[u].y, cv[u].z, e, -wxy, -wxy, -wz);
              const int X = d.x + ox, Y = d.y + oy, Z = d.z + oz;
              const bool inside = q + u * stride < stop &&
                                  static_cast<unsigned>(X) < static_cast<unsigned>(O.qx) &&
                                  static_cast<unsigned>(Y) < static_cast<unsigned>(O.qy) &&
                                  static_cast<unsigned>(Z) < static_cast<unsigned>(O.qz);
              const unsigned offset = static_cast<unsigned>((Z * O.qy + Y) * O.qx + X) * 8u;
              w[u] = __builtin_bit_cast(U2, __builtin_amdgcn_raw_buffer_load_b64(
                                                oct, inside ? offset : kOutOfBuffer, 0, 0));
            }
#pragma unroll
            for (int u = 0; u < kPoints; ++u) {
              e0 += w[u].x & 0x00ff00ffu; o0 += (w[u].x >> 8) & 0x00ff00ffu;
              e1 += w[u].y & 0x00ff00ffu; o1 += (w[u].y >> 8) & 0x00ff00ffu;
            }
          }
        } else {
#pragma unroll 4
          for (int q = q0; q < stop; q += stride) {
            const int3 d = DepthIndex(cells[q], e, -P.wxy, -P.wxy, -P.wz);
            const int X = d.x + ox, Y = d.y + oy, Z = d.z + oz;
            const bool inside = static_cast<unsigned>(X) < static_cast<unsigned>(O.qx) &&
                                static_cast<unsigned>(Y) < static_cast<unsigned>(O.qy) &&
                                static_cast<unsigned>(Z) < static_cast<unsigned>(O.qz);
            // unconditional load from a valid offset, masked afterwards
            const uint2 w = O.cells[inside ? (static_cast<size_t>(Z) * O.qy + Y) * O.qx + X : 0];
            const unsigned lo = inside ? w.x : 0u, hi = inside ? w.y : 0u;
            e0 += lo & 0x00ff00ffu; o0 += (lo >> 8) & 0x00ff00ffu;
            e1 += hi & 0x00ff00ffu; o1 += (hi >> 8) & 0x00ff00ffu;
          }
        }
        sum[0] += e0 & 0xffffu; sum[2] += e0 >> 16;      // bytes 0, 2 of the low word
        sum[1] += o0 & 0xffffu; sum[3] += o0 >> 16;      // bytes 1, 3
        sum[4] += e1 & 0xffffu; sum[6] += e1 >> 16;
        sum[5] += o1 & 0xffffu; sum[7] += o1 >> 16;
      }
    } else if (path == kSumsWindows) {
#pragma unroll 2
      for (int q = first; q < P.n; q += stride) {
        const int3 d = DepthIndex(cells[q], e, -P.wxy, -P.wxy, -P.wz);
        const int ix0 = d.x + fx[0], ix1 = ix0 + dx;
        const bool okx0 = static_cast<unsigned>(ix0) < static_cast<unsigned>(L.nx);
        const bool okx1 = static_cast<unsigned>(ix1) < static_cast<unsigned>(L.nx);
        const int base = min(max(ix0, 0), L.nx - 1);   // first byte wanted (when any is)
        int ay[2], az[2];
        bool oky[2], okz[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int iy = d.y + fy[b], iz = d.z + fz[b];
          oky[b] = static_cast<unsigned>(iy) < static_cast<unsigned>(L.ny);
          okz[b] = static_cast<unsigned>(iz) < static_cast<unsigned>(L.nz);
          ay[b] = oky[b] ? iy * row : 0;
          az[b] = okz[b] ? iz * slab : 0;
        }
        uint2 w[4];
        unsigned j0[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {     // unconditional loads from in-range addresses
          const unsigned a = static_cast<unsigned>(az[(k >> 1) & 1] + ay[k & 1] + base);
          j0[k] = a & 3u;
          w[k] = *reinterpret_cast<const uint2*>(cells8 + (a & ~3u));
        }
        const unsigned j1 = static_cast<unsigned>(ix1 - base);   // 0 .. 4 when okx1
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned b0 = j0[k], b1 = j0[k] + j1;             // byte indices, < 8
          const unsigned v0 = ((b0 & 4u) ? w[k].y : w[k].x) >> (8u * (b0 & 3u)) & 0xffu;
          const unsigned v1 = ((b1 & 4u) ? w[k].y : w[k].x) >> (8u * (b1 & 3u)) & 0xffu;
          const bool okyz = oky[k & 1] && okz[(k >> 1) & 1];
          sum[2 * k] += (okx0 && okyz) ? v0 : 0u;
          sum[2 * k + 1] += (okx1 && okyz) ? v1 : 0u;
        }
      }
    } else {
#pragma unroll 2
    for (int q = first; q < P.n; q += stride) {
      const int3 d = DepthIndex(cells[q], e, -P.wxy, -P.wxy, -P.wz);
      // Per axis and position: in-range flag and (clamped) address term.
      int ax[2], ay[2], az[2];
      bool okx[2], oky[2], okz[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int ix = d.x + fx[b], iy = d.y + fy[b], iz = d.z + fz[b];
        okx[b] = static_cast<unsigned>(ix) < static_cast<unsigned>(L.nx);
        oky[b] = static_cast<unsigned>(iy) < static_cast<unsigned>(L.ny);
        okz[b] = static_cast<unsigned>(iz) < static_cast<unsigned>(L.nz);
        ax[b] = okx[b] ? ix : 0;
        ay[b] = oky[b] ? iy * row : 0;
        az[b] = okz[b] ? iz * slab : 0;
      }
      unsigned v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)    // unconditional loads from in-range addresses
        v[k] = cells8[az[(k >> 2) & 1] + ay[(k >> 1) & 1] + ax[k & 1]];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        sum[k] += (okx[k & 1] && oky[(k >> 1) & 1] && okz[(k >> 2) & 1]) ? v[k] : 0u;
    }
    }
    return path;
  }
}

// One 256-thread block per node: scores the <=8 children (z outer, y, x inner with the
// `break`s of :416-431), ranks them as the reference's stable descending sort does, then
//   child depth > 0, full: children that can still matter go to `out`;
//   child depth > 0, dive: only the best child continues;
//   child depth == 0: leaves are verified in rank order with the low-resolution
//     matcher; the first one that passes is recorded (:389-402).
// A search expands a few thousand nodes in total, so what matters is the latency of
// one expansion: four waves share the points, the eight child cells of a point are
// addressed from per-axis clamped offsets (two positions per axis), and the loads of
// several points are in flight together.
struct ExpandShared {
  int partial[4][8];
  int fam_partial[4][8][8];    // [wave][member][child]
  int fam_total[8][8];
  Node3D fam[8];
  float score[8];
  float low_prob[kLowChunk];
  Node3D next;       // dive: the child the descent continues with
  int has_next;
  // Work counters of this block (flushed once by FlushWork3D: a global atomic pair per node
  // was most of the 2D wave stage's time, profiles/r02_c3_wave_atomics.txt).
  unsigned scored, expanded;
};

__device__ __forceinline__ void InitWork3D(ExpandShared* sh) {
  if (threadIdx.x == 0) { sh->scored = 0; sh->expanded = 0; }
  __syncthreads();
}
__device__ __forceinline__ void FlushWork3D(ExpandShared* sh, Counters3* __restrict__ counters) {
  __syncthreads();
  if (threadIdx.x == 0 && sh->expanded) {
    atomicAdd(&counters->scored[blockIdx.x & 15], static_cast<unsigned long long>(sh->scored));
    atomicAdd(&counters->expanded[blockIdx.x & 15], static_cast<unsigned long long>(sh->expanded));
  }
}

// Expansion of one node by the whole block (see above).  dive = 0: children that can still
// matter are appended to `out`; dive = 1: the best child is left in sh->next.
// The part of an expansion after the child sums: scores, ranks, then the children that can
// still matter (or, at the leaves, the low-resolution verification).  `totals` = the eight
// integer child sums of `nd` (any memory every thread can read).
__device__ __forceinline__ void FinishExpand3D(const Fast3DProblem& P, const Node3D& nd,
                                               const int* totals, float best, int dive, int strict,
                                               const List3& out, const List3& leaves,
                                               Counters3* __restrict__ counters, int sub_id,
                                               ExpandShared* sh) {
  if (threadIdx.x == 0) sh->has_next = 0;
  {
    const int child_depth = nd.level - 1;
    const int half = 1 << child_depth;
    const bool vx = nd.ox + half <= P.wxy, vy = nd.oy + half <= P.wxy, vz = nd.oz + half <= P.wz;
    __syncthreads();
    if (threadIdx.x < 8) {
      const int k = threadIdx.x;
      const bool valid = (!(k & 1) || vx) && (!(k & 2) || vy) && (!(k & 4) || vz);
      sh->score[k] = valid ? ToProbability(totals[k], P.n) : -1.f;
    }
    __syncthreads();
    float score[8];
    int nvalid = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      score[k] = sh->score[k];
      nvalid += score[k] >= 0.f;
    }
    int rank[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int r = 0;
#pragma unroll
      for (int o = 0; o < 8; ++o)
        if (o != k && score[o] >= 0.f && (score[o] > score[k] || (score[o] == score[k] && o < k)))
          ++r;
      rank[k] = r;
    }
    if (threadIdx.x == 0) {
      sh->scored += static_cast<unsigned>(nvalid);
      sh->expanded += 1u;
    }
    auto make_child = [&](int k) {
      Node3D child = nd;
      child.family = 0;
      child.level = child_depth;
      child.ox = nd.ox + ((k & 1) ? half : 0);
      child.oy = nd.oy + ((k & 2) ? half : 0);
      child.oz = nd.oz + ((k & 4) ? half : 0);
      child.score = score[k];
      child.path = nd.path | (static_cast<unsigned long long>(rank[k]) << (3 * child_depth));
      return child;
    };
    if (child_depth == 0) {
      // Leaves in descending order; the first that passes the low-resolution
      // matcher is the result of this sibling group.  (Everything below is
      // block-uniform, so the barriers inside LowResolutionScore are safe.)
      for (int r = 0; r < nvalid; ++r) {
        int k = 0;
#pragma unroll
        for (int o = 0; o < 8; ++o)
          if (score[o] >= 0.f && rank[o] == r) k = o;
        const float sc = score[k];
        __syncthreads();
        if (threadIdx.x == 0)
          sh->score[0] = __uint_as_float(__hip_atomic_load(P.best_bits, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT));
        __syncthreads();
        const float now = sh->score[0];
        if (!(sc > P.min_score) || (strict ? !(sc > now) : (sc < now))) break;
        const Node3D leaf = make_child(k);
        const float4 q4 = P.scan_q[nd.scan];
        const float low = LowResolutionScore(
            P, Quat{q4.w, q4.x, q4.y, q4.z},
            (P.pose_tx + 0.f) + P.resolution * static_cast<float>(leaf.ox),
            (P.pose_ty + 0.f) + P.resolution * static_cast<float>(leaf.oy),
            (P.pose_tz + 0.f) + P.resolution * static_cast<float>(leaf.oz), sh->low_prob);
        if (static_cast<double>(low) >= P.min_low_resolution_score) {
          if (threadIdx.x == 0) {
            Node3D rec = leaf;
            rec.low_resolution_score = low;
            if (!Push3(leaves, sub_id, atomicAdd(&leaves.counts[sub_id * kCountStride3], 1), rec))
              counters->overflow = 1;
            atomicMax(P.best_bits, __float_as_uint(sc));
          }
          break;
        }
      }
    } else if (threadIdx.x == 0) {
      int keep_mask = 0, m = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (score[k] < 0.f) continue;
        if (dive) {
          if (rank[k] != 0) continue;
        } else if (strict ? !(score[k] > best) : (score[k] < best)) {
          continue;
        }
        keep_mask |= 1 << k;
        ++m;
      }
      if (dive) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (keep_mask >> k & 1) { sh->next = make_child(k); sh->has_next = 1; }
      } else if (m) {
        int slot = atomicAdd(&out.counts[sub_id * kCountStride3], m);
        bool leader = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (!(keep_mask >> k & 1)) continue;
          Node3D child = make_child(k);
          child.family = leader ? m : 0;       // the kept children of one parent: a family
          leader = false;
          if (!Push3(out, sub_id, slot, child)) counters->overflow = 1;
          ++slot;
        }
      }
    }
    __syncthreads();   // scratch reused by the next node; sh->next / has_next visible
  }
}

// The eight child sums of `nd` by the whole block (256 threads), left in sh->fam_total[0] by
// threads 0 .. 7 (a barrier makes them everybody's).  Returns the path that summed them.
__device__ __forceinline__ int NodeSums3D(const Fast3DProblem& P, const Node3D& nd,
                                          ExpandShared* sh) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  int sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int path = ChildSums3D(P, nd, threadIdx.x, 256, sum);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int total = WaveSum(sum[k]);
    if (lane == 0) sh->partial[wave][k] = total;
  }
  __syncthreads();
  if (threadIdx.x < 8)
    sh->fam_total[0][threadIdx.x] = sh->partial[0][threadIdx.x] + sh->partial[1][threadIdx.x] +
                                    sh->partial[2][threadIdx.x] + sh->partial[3][threadIdx.x];
  return path;
}

// Expansion of one node by the whole block (see above).  dive = 0: children that can still
// matter are appended to `out`; dive = 1: the best child is left in sh->next.
__device__ __forceinline__ void ExpandNode3D(const Fast3DProblem& P, const Node3D& nd, float best,
                                             int dive, int strict, const List3& out,
                                             const List3& leaves,
                                             Counters3* __restrict__ counters, int sub_id,
                                             ExpandShared* sh) {
  NodeSums3D(P, nd, sh);
  FinishExpand3D(P, nd, sh->fam_total[0], best, dive, strict, out, leaves, counters, sub_id, sh);
}

// The child sums of a FAMILY (round 3): the kept children of one parent are expanded by one
// block.  What bounded the per-node expansion (profiles/r02e_c5_pmc_*): 4.9 GB of 128-byte lines
// per launch for 1.35 GB of oct words -- every (node, point) lookup fetched a line of its own,
// and every node re-read the scan's 16-byte cell records.  Members of a family read oct words
// `half` cells apart: the two x positions share a line, the cell record and its depth index
// are computed once per point for all members, and up to eight gathers per point are in
// flight together.  Returns false (nothing summed) when the level has no oct grid.
// The family loop for a compile-time family size F (round 4).  Until the end of round 3 the
// member loop `if (m >= fam || !(live >> m & 1)) continue;` gave every member a basic block of
// its own -- flat_load_dwordx2 with 64-bit address arithmetic, closed by s_waitcnt vmcnt(0)
// lgkmcnt(0): ONE gather in flight per wavefront where the comment above promises eight.  Now
// the loop body is branch-free: oct words come through a buffer resource (32-bit offsets; dead
// members and cells outside the grid use an out-of-range offset, which reads 0 and fetches
// nothing), so the F gathers of a point -- 2 F with the unroll -- go out back to back.
template <int F>
__device__ __forceinline__ void FamilyLoop3D(__amdgpu_buffer_rsrc_t oct, const OctDesc& O,
                                             const I4 CMX_GLOBAL* __restrict__ cells, int n,
                                             int e, int wxy, int wz, const int (&mx)[8],
                                             const int (&my)[8], const int (&mz)[8],
                                             unsigned live, int first, int stride,
                                             ExpandShared* sh) {
  typedef unsigned U2 __attribute__((ext_vector_type(2)));
  constexpr int kPoints = 2;          // points per iteration: 2 F gathers in flight
  // (n <= 256 * stride, FamilySums3D checks it: a lane adds at most 255 per point, so the
  // packed 16-bit halves cannot overflow and are widened once, after the loop)
  unsigned acc[F][4];
#pragma unroll
  for (int m = 0; m < F; ++m) acc[m][0] = acc[m][1] = acc[m][2] = acc[m][3] = 0;
  for (int q = first; q < n; q += kPoints * stride) {
    I4 cv[kPoints];
#pragma unroll
    for (int u = 0; u < kPoints; ++u) cv[u] = cells[min(q + u * stride, n - 1)];
    U2 w[kPoints][F];
#pragma unroll
    for (int u = 0; u < kPoints; ++u) {
      const bool in_cloud = q + u * stride < n;
      const int3 d = DepthIndexAny(cv[u].x, cv[u].y, cv[u].z, e, -wxy, -wxy, -wz);
#pragma unroll
      for (int m = 0; m < F; ++m) {
        const int X = d.x + mx[m], Y = d.y + my[m], Z = d.z + mz[m];
        const bool inside = in_cloud && (live >> m & 1) &&
                            static_cast<unsigned>(X) < static_cast<unsigned>(O.qx) &&
                            static_cast<unsigned>(Y) < static_cast<unsigned>(O.qy) &&
                            static_cast<unsigned>(Z) < static_cast<unsigned>(O.qz);
        const unsigned offset = static_cast<unsigned>((Z * O.qy + Y) * O.qx + X) * 8u;
        w[u][m] = __builtin_bit_cast(U2, __builtin_amdgcn_raw_buffer_load_b64(
                                             oct, inside ? offset : kOutOfBuffer, 0, 0));
      }
    }
#pragma unroll
    for (int u = 0; u < kPoints; ++u) {
#pragma unroll
      for (int m = 0; m < F; ++m) {
        acc[m][0] += w[u][m].x & 0x00ff00ffu; acc[m][1] += (w[u][m].x >> 8) & 0x00ff00ffu;
        acc[m][2] += w[u][m].y & 0x00ff00ffu; acc[m][3] += (w[u][m].y >> 8) & 0x00ff00ffu;
      }
    }
  }
  // Wave totals of the live members' eight child sums, left in sh->fam_partial[wave][m][k]
  // (the caller adds the four waves after a barrier).
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < F; ++m) {
    if (!(live >> m & 1)) continue;                   // block-uniform
    const int s8[8] = {static_cast<int>(acc[m][0] & 0xffffu), static_cast<int>(acc[m][1] & 0xffffu),
                       static_cast<int>(acc[m][0] >> 16),     static_cast<int>(acc[m][1] >> 16),
                       static_cast<int>(acc[m][2] & 0xffffu), static_cast<int>(acc[m][3] & 0xffffu),
                       static_cast<int>(acc[m][2] >> 16),     static_cast<int>(acc[m][3] >> 16)};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int total = WaveSum(s8[k]);
      if (lane == 0) sh->fam_partial[wave][m][k] = total;
    }
  }
}

__device__ __forceinline__ bool FamilySums3D(const Fast3DProblem& P, const Node3D* fam_nodes,
                                             int fam, unsigned live, int first, int stride,
                                             ExpandShared* sh) {
  const int child_depth = fam_nodes[0].level - 1;
  const int half = 1 << child_depth;
  const int e = max(0, child_depth - P.full_resolution_depth + 1);
  const Brick L = P.level[child_depth];
  const OctDesc O = P.oct[child_depth];
  // (no oct words, plain loads only, or more than 256 points per lane: the members one by one)
  const int dx = ((fam_nodes[0].ox + half) >> e) - (fam_nodes[0].ox >> e);
  if (SumsPath3DOf(O, dx, true, P.n, stride) != kSumsFamily) return false;
  const __amdgpu_buffer_rsrc_t oct = UniformBuffer(O.cells, OctBytes(O));
  const auto* cells = AsGlobal(
      reinterpret_cast<const I4*>(P.cells + static_cast<size_t>(fam_nodes[0].scan) * P.n));
  int mx[8], my[8], mz[8];                          // block-uniform (the family lies in LDS)
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const Node3D& nd = fam_nodes[min(m, fam - 1)];
    mx[m] = __builtin_amdgcn_readfirstlane((nd.ox >> e) - L.lo_x + O.s);
    my[m] = __builtin_amdgcn_readfirstlane((nd.oy >> e) - L.lo_y + O.s);
    mz[m] = __builtin_amdgcn_readfirstlane((nd.oz >> e) - L.lo_z + O.s);
  }
  const int n = P.n, wxy = P.wxy, wz = P.wz;
  switch (fam) {                                    // block-uniform
    case 2: FamilyLoop3D<2>(oct, O, cells, n, e, wxy, wz, mx, my, mz, live, first, stride, sh); break;
    case 3: FamilyLoop3D<3>(oct, O, cells, n, e, wxy, wz, mx, my, mz, live, first, stride, sh); break;
    case 4: FamilyLoop3D<4>(oct, O, cells, n, e, wxy, wz, mx, my, mz, live, first, stride, sh); break;
    case 5: FamilyLoop3D<5>(oct, O, cells, n, e, wxy, wz, mx, my, mz, live, first, stride, sh); break;
    case 6: FamilyLoop3D<6>(oct, O, cells, n, e, wxy, wz, mx, my, mz, live, first, stride, sh); break;
    case 7: FamilyLoop3D<7>(oct, O, cells, n, e, wxy, wz, mx, my, mz, live, first, stride, sh); break;
    default: FamilyLoop3D<8>(oct, O, cells, n, e, wxy, wz, mx, my, mz, live, first, stride, sh); break;
  }
  return true;
}

// After FamilySums3D returned true: the members' child sums, the four waves added, in
// sh->fam_total[member][child] for every thread (rows of dead members hold no sums: nobody
// reads them).
__device__ __forceinline__ void FamilyTotals3D(ExpandShared* sh) {
  __syncthreads();
  if (threadIdx.x < 64) {
    const int m = threadIdx.x >> 3, k = threadIdx.x & 7;
    sh->fam_total[m][k] = sh->fam_partial[0][m][k] + sh->fam_partial[1][m][k] +
                          sh->fam_partial[2][m][k] + sh->fam_partial[3][m][k];
  }
  __syncthreads();
}

// (One wavefront per node for the levels above the leaves -- four times as many nodes in
// flight, 43 points per lane -- was measured and changed nothing: 5.26 vs 5.34 ms for 32 pairs;
// a single pair got slower, 0.45 vs 0.41 ms.  Removed.)
__global__ void __launch_bounds__(256)
Expand3DKernel(const Fast3DProblem* __restrict__ problems, List3 in, int strict, int affinity,
               int use_families, List3 out, List3 leaves, Counters3* __restrict__ counters) {
  __shared__ ExpandShared sh;
  InitWork3D(&sh);
  const int max_count = ListMax3(in);
  for (int i = blockIdx.x; i < max_count * kSubLists3; i += gridDim.x) {
    const int in_sub = i & (kSubLists3 - 1), j = i / kSubLists3;
    if (j >= min(in.counts[in_sub * kCountStride3], in.sub_capacity)) continue;   // block-uniform
    // Children go to a sub-list derived from the node's slot, not from the block: the
    // survivors of a search cluster in a few subtrees, and appending them to their
    // parent's sub-list would leave the next level with one long list that a handful
    // of blocks walk serially (measured: 0.9 us per node, chip idle).
    // (Workgroup b runs on XCD b % 8 and reads the sub-lists with sub % 8 == b % 8: the grid
    // is a multiple of 64 blocks.  With `affinity` the children stay on their parent's XCD.)
    // (Sending the children of 32 consecutive nodes to one sub-list, to keep neighbours
    // together in the next level, measured worse: 7.7 vs 7.2 ms for 32 pairs -- the lists of an
    // XCD then differ in length.)
    const Node3D* slot0 = in.nodes + static_cast<size_t>(in_sub) * in.sub_capacity + j;
    const int family = slot0->family;
    if (family == 0) continue;            // a later member: its leader's block takes it (uniform)
    const int fam = min(family, min(in.counts[in_sub * kCountStride3], in.sub_capacity) - j);
    const Fast3DProblem& P = problems[slot0->problem];
    // The bound moves while this kernel runs: ONE thread reads it and the block shares that
    // value.  (Every thread reading it for itself let some threads skip a node that the
    // others expanded -- barriers of different nodes then met, children were summed from a
    // mixture of two nodes, and about one search in fifty returned a leaf that does not
    // exist.  Present since round 1; found with tools/stress_fast3d.py.)
    __syncthreads();
    if (threadIdx.x == 0)
      sh.score[0] = __uint_as_float(
          __hip_atomic_load(P.best_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (threadIdx.x < fam) sh.fam[threadIdx.x] = slot0[threadIdx.x];
    __syncthreads();
    const float best = sh.score[0];
    unsigned live = 0;
    for (int m = 0; m < fam; ++m)
      if (!(strict ? !(sh.fam[m].score > best) : (sh.fam[m].score < best))) live |= 1u << m;
    if (live == 0) continue;                                              // block-uniform
    bool summed = false;
    if (fam > 1 && use_families) {
      summed = FamilySums3D(P, sh.fam, fam, live, threadIdx.x, 256, &sh);
      if (summed) FamilyTotals3D(&sh);
    }
    for (int m = 0; m < fam; ++m) {
      if (!(live >> m & 1)) continue;
      // (each member's children go to a sub-list of their own, as single nodes' did)
      const int sub_m = affinity ? (in_sub & 7) | ((((in_sub >> 3) * 5 + j + m) & 7) << 3)
                                 : (in_sub * 17 + j + m) & (kSubLists3 - 1);
      const Node3D nd = sh.fam[m];
      if (summed)
        FinishExpand3D(P, nd, sh.fam_total[m], best, 0, strict, out, leaves, counters, sub_m, &sh);
      else
        ExpandNode3D(P, nd, best, 0, strict, out, leaves, counters, sub_m, &sh);
    }
  }
  FlushWork3D(&sh, counters);
}

// Greedy descents (always the best child) from the seeds, one block per seed, all levels in
// one launch: the verified leaf scores bound the search that follows.
// grid (kSeeds3, problems)
__global__ void __launch_bounds__(256)
Dive3DKernel(const Fast3DProblem* __restrict__ problems, List3 leaves,
             Counters3* __restrict__ counters) {
  __shared__ ExpandShared sh;
  const Fast3DProblem& P = problems[blockIdx.y];
  const List3 seeds{P.seeds, P.seed_count, kSeeds3};
  if (static_cast<int>(blockIdx.x) >= min(seeds.counts[0], seeds.sub_capacity)) return;
  InitWork3D(&sh);
  Node3D nd = seeds.nodes[blockIdx.x];
  const int sub_id = (blockIdx.x + 7 * blockIdx.y) & (kSubLists3 - 1);
  while (nd.level >= 1) {
    ExpandNode3D(P, nd, 0.f, 1, 0, seeds, leaves, counters, sub_id, &sh);
    if (!sh.has_next) break;
    nd = sh.next;
    __syncthreads();   // everyone has read sh.next before the next expansion resets it
  }
  FlushWork3D(&sh, counters);
}

// cmx_debug_fast3d_child_sums: the child sums of `nodes` by the device functions of the search.
// as_family = 0: workgroup i sums node i as ExpandNode3D does (NodeSums3D).  as_family = 1: one
// workgroup takes the nodes as a family, as Expand3DKernel does -- FamilySums3D and
// FamilyTotals3D, or, where the family loop refuses, the live members one by one.  sums
// [num_nodes][8] and path [num_nodes] (SumsPath3D); the rows of dead members are not written.
__global__ void __launch_bounds__(256)
DebugChildSums3DKernel(const Fast3DProblem* __restrict__ problem, const Node3D* __restrict__ nodes,
                       int num_nodes, int as_family, unsigned live, int* __restrict__ sums,
                       int* __restrict__ path) {
  __shared__ ExpandShared sh;
  const Fast3DProblem& P = *problem;
  if (!as_family) {
    const int i = blockIdx.x;
    const Node3D nd = nodes[i];
    const int took = NodeSums3D(P, nd, &sh);     // (threads 0 .. 7 hold the totals they wrote)
    if (threadIdx.x < 8) sums[8 * i + threadIdx.x] = sh.fam_total[0][threadIdx.x];
    if (threadIdx.x == 0) path[i] = took;
    return;
  }
  if (threadIdx.x < num_nodes) sh.fam[threadIdx.x] = nodes[threadIdx.x];
  __syncthreads();
  const bool summed = FamilySums3D(P, sh.fam, num_nodes, live, threadIdx.x, 256, &sh);
  if (summed) FamilyTotals3D(&sh);
  for (int m = 0; m < num_nodes; ++m) {
    if (!(live >> m & 1)) continue;                                         // block-uniform
    int took = kSumsFamily;
    if (!summed) {
      const Node3D nd = sh.fam[m];
      took = NodeSums3D(P, nd, &sh);
    }
    if (threadIdx.x < 8) sums[8 * m + threadIdx.x] = sh.fam_total[summed ? m : 0][threadIdx.x];
    if (threadIdx.x == 0) path[m] = took;
    __syncthreads();   // (the scratch of NodeSums3D is reused by the next member)
  }
}

// Among the recorded leaves with the best score, the one the reference's
// depth-first search meets first (see fast_2d_search_device.h SelectBestBody).
// grid (problems): block p looks at the leaves of problem p only.
// Block p also PUBLISHES problem p's record -- and block 0 the counters and the problems' states,
// complete since the kernels before this one -- into the caller's pinned mirror of `misc` (mapped
// into the device's address space): no copy kernel behind the last launch of the chain.
// misc_host == nullptr: the host fetches `misc` itself.
__global__ void __launch_bounds__(1024)
SelectBest3DKernel(List3 leaves, const Fast3DProblem* __restrict__ problems,
                   Best3* __restrict__ results, const unsigned* __restrict__ misc_dev,
                   unsigned* __restrict__ misc_host, int counters_words, int state_word0,
                   int state_words, int best_word0) {
  __shared__ unsigned best_coarse;
  __shared__ unsigned long long best_key[2];
  __shared__ int ties;
  const int problem = blockIdx.x;
  Best3* out = results + problem;
  const int total = ListMax3(leaves) * kSubLists3;
  const unsigned best_bits = *problems[problem].best_bits;
  if (threadIdx.x == 0) {
    best_coarse = 0; ties = 0; best_key[0] = ~0ull; best_key[1] = ~0ull;
    Best3 b{};
    *out = b;
  }
  __syncthreads();
  auto leaf_at = [&](int i, Node3D* nd) {
    const int sub = i & (kSubLists3 - 1), j = i / kSubLists3;
    if (j >= min(leaves.counts[sub * kCountStride3], leaves.sub_capacity)) return false;
    *nd = leaves.nodes[static_cast<size_t>(sub) * leaves.sub_capacity + j];
    return nd->problem == problem;
  };
  Node3D nd;
  for (int i = threadIdx.x; i < total; i += blockDim.x)
    if (leaf_at(i, &nd) && __float_as_uint(nd.score) == best_bits) {
      atomicMax(&best_coarse, __float_as_uint(nd.coarse_score));
      atomicAdd(&ties, 1);
    }
  __syncthreads();
  // key = (coarse_index, path), minimised lexicographically in two steps
  for (int i = threadIdx.x; i < total; i += blockDim.x)
    if (leaf_at(i, &nd) && __float_as_uint(nd.score) == best_bits &&
        __float_as_uint(nd.coarse_score) == best_coarse)
      atomicMin(&best_key[0], static_cast<unsigned long long>(static_cast<unsigned>(nd.coarse_index)));
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += blockDim.x)
    if (leaf_at(i, &nd) && __float_as_uint(nd.score) == best_bits &&
        __float_as_uint(nd.coarse_score) == best_coarse &&
        static_cast<unsigned long long>(static_cast<unsigned>(nd.coarse_index)) == best_key[0])
      atomicMin(&best_key[1], nd.path);
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += blockDim.x)
    if (leaf_at(i, &nd) && __float_as_uint(nd.score) == best_bits &&
        __float_as_uint(nd.coarse_score) == best_coarse &&
        static_cast<unsigned long long>(static_cast<unsigned>(nd.coarse_index)) == best_key[0] &&
        nd.path == best_key[1]) {
      Best3 b;
      b.score = nd.score; b.scan = nd.scan; b.ox = nd.ox; b.oy = nd.oy; b.oz = nd.oz;
      b.low_resolution_score = nd.low_resolution_score;
      b.found = 1; b.ties = 1;
      *out = b;
    }
  __threadfence();
  __syncthreads();
  // ties = 1 + tied records that are a different leaf (dive + search duplicate the best).
  for (int i = threadIdx.x; i < total; i += blockDim.x)
    if (leaf_at(i, &nd) && __float_as_uint(nd.score) == best_bits) {
      const int scan = __hip_atomic_load(&out->scan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int ox = __hip_atomic_load(&out->ox, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int oy = __hip_atomic_load(&out->oy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int oz = __hip_atomic_load(&out->oz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (nd.scan != scan || nd.ox != ox || nd.oy != oy || nd.oz != oz) atomicAdd(&out->ties, 1);
    }
  if (misc_host == nullptr) return;
  __threadfence();
  __syncthreads();
  const auto publish = [&](int word0, int words) {
    for (int i = threadIdx.x; i < words; i += blockDim.x)
      misc_host[word0 + i] =
          __hip_atomic_load(&misc_dev[word0 + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  constexpr int kBestWords = static_cast<int>(sizeof(Best3) / sizeof(unsigned));
  publish(best_word0 + problem * kBestWords, kBestWords);
  if (problem == 0) {
    publish(0, counters_words);
    publish(state_word0, state_words);
  }
}

// depth == 1: lowest-resolution candidates are the leaves; they are verified
// in descending score order (BranchAndBound at candidate_depth 0, :382-402).
// Rare configuration; handled by treating every candidate as a leaf group of
// one through the generic expansion of a virtual parent is not possible, so a
// dedicated wave-per-candidate pass records every passing candidate.
__global__ void __launch_bounds__(256)
VerifyCoarseLeaves3DKernel(const Fast3DProblem* __restrict__ problems, List3 leaves,
                           Counters3* __restrict__ counters) {
  const Fast3DProblem& P = problems[blockIdx.y];
  __shared__ float low_prob[kLowChunk];
  const int total = P.ncx * P.ncy * P.ncz * P.num_scans;
  const int sub_id = blockIdx.x & (kSubLists3 - 1);
  for (int c = blockIdx.x; c < total; c += gridDim.x) {     // one block per candidate
    const Node3D nd = CoarseNode3D(P, c);
    if (!(nd.score > P.min_score)) continue;                // block-uniform
    const float4 q4 = P.scan_q[nd.scan];
    const float low = LowResolutionScore(
        P, Quat{q4.w, q4.x, q4.y, q4.z},
        (P.pose_tx + 0.f) + P.resolution * static_cast<float>(nd.ox),
        (P.pose_ty + 0.f) + P.resolution * static_cast<float>(nd.oy),
        (P.pose_tz + 0.f) + P.resolution * static_cast<float>(nd.oz), low_prob);
    if (static_cast<double>(low) >= P.min_low_resolution_score && threadIdx.x == 0) {
      Node3D rec = nd;
      rec.level = 0;
      rec.low_resolution_score = low;
      if (!Push3(leaves, sub_id, atomicAdd(&leaves.counts[sub_id * kCountStride3], 1), rec)) counters->overflow = 1;
      atomicMax(P.best_bits, __float_as_uint(nd.score));
    }
  }
}


}  // namespace

namespace {
// The debug switch fast3d_byte_loads as the kernels of this unit read it.
void UploadByteLoadsSwitch3D() {
  const int byte_loads = Debug().fast3d_byte_loads ? 1 : 0;
  static int uploaded = -1;              // (tools only: not meant to be toggled concurrently)
  if (uploaded != byte_loads) {
    CMX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_fast3d_byte_loads), &byte_loads, sizeof(int)));
    uploaded = byte_loads;
  }
}
}  // namespace

void ReserveSearchScratch3D(Workspace& ws, Chain3D* chain) {
  UploadByteLoadsSwitch3D();
  // The debug switch frontier_capacity shrinks the frontier buffers (tests only): overflow ->
  // strict retry.
  const int cap_req = Debug().frontier_capacity;
  chain->frontier_capacity =
      cap_req >= kSubLists3 ? std::min(cap_req, 1 << 21) / kSubLists3 * kSubLists3 : 1 << 21;
  chain->leaf_capacity = 1 << 18;
  chain->d_front[0] = ws.dev[5].ReserveAs<Node3D>(chain->frontier_capacity);
  chain->d_front[1] = ws.dev[6].ReserveAs<Node3D>(chain->frontier_capacity);
  chain->d_leaves = ws.dev[7].ReserveAs<Node3D>(chain->leaf_capacity);
  chain->d_seeds = ws.dev[8].ReserveAs<Node3D>(static_cast<size_t>(kSeeds3) * chain->num);
}

namespace {

List3 Frontier3(const Chain3D& c, int stage) {
  return List3{c.d_front[stage & 1], c.d_counters()->frontier[stage],
               c.frontier_capacity / kSubLists3};
}
List3 Leaves3(const Chain3D& c) {
  return List3{c.d_leaves, c.d_counters()->leaves, c.leaf_capacity / kSubLists3};
}

// One pass over the chain's lowest-resolution candidates, from the seeds to the selection of
// every problem's best leaf (not synchronised).  strict = 0: the first pass, with the dives, whose
// expansion launches are the timed ones (`st`); strict = 1: a retry that prunes ties.
void LaunchSearch3D(Workspace& ws, const Chain3D& c, int strict, int num_chunks, StageTrace* trace,
                    cmx_match_stats* st) {
  const int num = c.num;
  Fast3DProblem* d_problems = c.d_problems();
  Counters3* d_counters = c.d_counters();
  const List3 leaf_list = Leaves3(c);
  const int blocks = 2048;
  // Batches: one problem's nodes stay on one XCD (debug switch fast3d_affinity overrides).
  const int affinity_override = Debug().fast3d_affinity;
  const int affinity = affinity_override ? affinity_override - 1 : (num >= 16 ? 1 : 0);
  // fast3d_no_families: every node of a family expanded on its own (A/B runs, parity tests)
  const int families = Debug().fast3d_no_families ? 0 : 1;
  if (c.max_depth == 1) {
    VerifyCoarseLeaves3DKernel<<<dim3(blocks, num), 256, 0, ws.stream>>>(d_problems, leaf_list,
                                                                         d_counters);
  } else {
    if (!strict) {
      // dive: greedy descents from the best lowest-resolution candidates give
      // a verified leaf score to bound the search with.
      SeedSelect3DKernel<<<num, 1024, 0, ws.stream>>>(d_problems);
      DebugSync3D(ws, "seed");
      trace->Mark("seed");
      Dive3DKernel<<<dim3(kSeeds3, num), 256, 0, ws.stream>>>(d_problems, leaf_list, d_counters);
      DebugSync3D(ws, "dive");
      trace->Mark("dive");
    }
    // The lowest-resolution candidates are searched in `num_chunks` interleaved subsets
    // (1 unless an earlier pass overflowed); later chunks profit from the bound the
    // earlier ones raised.
    for (int chunk = 0; chunk < num_chunks; ++chunk) {
      CMX_HIP(hipMemsetAsync(d_counters->frontier, 0, sizeof(d_counters->frontier), ws.stream));
      Filter3DKernel<<<dim3(256, num), 256, 0, ws.stream>>>(
          d_problems, strict, chunk, num_chunks, affinity, Frontier3(c, 0), d_counters);
      DebugSync3D(ws, "filter");
      trace->Mark("filter");
      int stage = 0;
      const bool timed = !strict && chunk == 0;      // statistics: the first pass
      if (timed) RecordEvent(ws.ev_x0, ws.stream);
      for (int child = c.max_depth - 2; child >= 0; --child, ++stage) {
        Expand3DKernel<<<blocks, 256, 0, ws.stream>>>(d_problems, Frontier3(c, stage), strict,
                                                      affinity, families, Frontier3(c, stage + 1),
                                                      leaf_list, d_counters);
        DebugSync3D(ws, "expand level");
        trace->Mark("expand");
      }
      if (timed) {
        RecordEvent(ws.ev_x1, ws.stream);
        st->expansion_launches = stage;
      }
    }
  }
  const bool direct = Debug().no_direct_results == 0;
  SelectBest3DKernel<<<num, 1024, 0, ws.stream>>>(
      leaf_list, d_problems, c.d_best(), reinterpret_cast<const unsigned*>(c.d_misc()),
      direct ? reinterpret_cast<unsigned*>(c.h_misc()) : nullptr,
      static_cast<int>(sizeof(Counters3) / sizeof(unsigned)),
      static_cast<int>(c.off_state / sizeof(unsigned)), 2 * num,
      static_cast<int>(c.off_best / sizeof(unsigned)));
  trace->Mark("select");
  CMX_HIP(hipGetLastError());
  RecordEvent(ws.ev_end, ws.stream);
  if (!direct) SmallCopyAsync(c.h_misc(), c.d_misc(), c.misc_bytes, false, ws.stream);
}

// A single search dropped nodes: its lists emptied (the work counters kept), its bound lowered by
// one ulp so that the best leaf is found again -- but not below the floor of `min_score` -- and
// its seeds forgotten, for a strict pass.
void RestartBound3D(Workspace& ws, const Chain3D& c, float min_score) {
  const float floor_score = std::max(min_score, 0.f);
  unsigned floor_bits;
  std::memcpy(&floor_bits, &floor_score, sizeof(float));
  Counters3* h_counters = c.h_counters();
  unsigned* h_state = c.h_state();
  Counters3 reset{};
  std::memcpy(reset.scored, h_counters->scored, sizeof(reset.scored));
  std::memcpy(reset.expanded, h_counters->expanded, sizeof(reset.expanded));
  *h_counters = reset;
  h_state[0] = h_state[0] > floor_bits ? h_state[0] - 1 : floor_bits;
  h_state[1] = 0;
  CMX_HIP(hipMemcpyAsync(c.d_misc(), c.h_misc(), c.off_best, hipMemcpyHostToDevice, ws.stream));
}

}  // namespace

void RunBranchAndBound3D(Workspace& ws, const Chain3D& c, float first_min_score,
                         StageTrace* trace, HostLaps3D* laps, Searched3D* searched) {
  cmx_match_stats st{};
  st.num_scans = static_cast<int32_t>(c.scans_total);
  const Counters3* h_counters = c.h_counters();
  int strict = 0, num_chunks = 1;
  for (;;) {
    LaunchSearch3D(ws, c, strict, num_chunks, trace, &st);
    CMX_HIP(hipStreamSynchronize(ws.stream));
    trace->Report();
    laps->Lap("device");
    if (!strict) {
      // (the nodes the expansion kernel took off its lists and found at or above the bound)
      for (int k = 0; k < 16; ++k) st.expansion_nodes += static_cast<int64_t>(h_counters->expanded[k]);
      // (per wave-wide gather: 64; searches of unlike clouds share the counters -- not reported)
      st.expansion_lookups =
          c.same_n ? st.expansion_nodes * (static_cast<int64_t>(c.max_n + 63) / 64 * 64) : 0;
    }
    if (!h_counters->overflow || c.num > 1) break;
    // Something was dropped.  Retry pruning ties (strict) with the bound lowered by one
    // ulp so the best leaf is found again, over four times as many, smaller chunks.
    CMX_REQUIRE(num_chunks < (1 << 12), "branch-and-bound frontier overflow (search too wide)");
    if (strict) num_chunks *= 4;
    strict = 1;
    RestartBound3D(ws, c, first_min_score);
  }
  st.coarse_candidates = static_cast<int64_t>(c.coarse_total);
  st.candidates_scored = static_cast<int64_t>(c.coarse_total);
  for (int k = 0; k < 16; ++k) {
    st.candidates_scored += h_counters->scored[k];
    st.nodes_expanded += h_counters->expanded[k];
  }
  st.device_ms = ElapsedMs(ws.ev_begin, ws.ev_end);
  st.dominant_kernel_ms = ElapsedMs(ws.ev_k0, ws.ev_k1);
  if (st.expansion_launches > 0) st.expansion_ms = ElapsedMs(ws.ev_x0, ws.ev_x1);
  searched->best = c.h_best();
  searched->overflow = h_counters->overflow != 0;
  searched->stats = st;
  searched->d_leaves = c.d_leaves;
  searched->leaf_sub_capacity = c.leaf_capacity / kSubLists3;
  searched->leaf_counts = h_counters->leaves;
}

namespace {

// cmx_debug_fast3d_child_sums after its argument checks: a problem of one scan whose cells are
// given, the nodes, and the caller's `sums` and `path` go up in one block; DebugChildSums3DKernel
// overwrites the rows it computes and the block's tail comes back (rows it left alone unchanged).
void DebugChildSums3D(const Fast3DMatcher& m, const int32_t* cells_xyz, int n, int wxy, int wz,
                      const cmx_debug_fast3d_node* nodes, int num_nodes, int as_family,
                      unsigned live_mask, int32_t* sums, int32_t* path) {
  const size_t off_nodes = sizeof(Fast3DProblem);
  const size_t off_cells = (off_nodes + sizeof(Node3D) * num_nodes + 15) / 16 * 16;
  const size_t off_sums = off_cells + sizeof(int4) * n;
  const size_t off_path = off_sums + sizeof(int) * 8 * num_nodes;
  const size_t bytes = off_path + sizeof(int) * num_nodes;
  static_assert(sizeof(Fast3DProblem) % 16 == 0, "alignment");
  WorkspaceLease ws(m.device);
  UploadByteLoadsSwitch3D();
  char* d = static_cast<char*>(ws->dev[0].Reserve(bytes));
  char* h = static_cast<char*>(ws->pinned[0].Reserve(bytes));
  const int depth = m.options.branch_and_bound_depth;
  Fast3DProblem P{};
  for (int l = 0; l < depth; ++l) P.level[l] = m.levels[l]->desc;
  for (size_t l = 0; l < m.oct_desc.size(); ++l) P.oct[l] = m.oct_desc[l];
  P.depth = depth;
  P.full_resolution_depth = m.options.full_resolution_depth;
  P.resolution = m.resolution;
  P.wxy = wxy; P.wz = wz;
  P.num_scans = 1; P.n = n;
  P.cells = reinterpret_cast<const int4*>(d + off_cells);
  std::memcpy(h, &P, sizeof(P));
  Node3D* h_nodes = reinterpret_cast<Node3D*>(h + off_nodes);
  for (int i = 0; i < num_nodes; ++i) {
    Node3D nd{};
    nd.level = nodes[i].level;
    nd.ox = nodes[i].ox; nd.oy = nodes[i].oy; nd.oz = nodes[i].oz;
    nd.family = as_family ? (i == 0 ? num_nodes : 0) : 1;
    h_nodes[i] = nd;
  }
  int4* h_cells = reinterpret_cast<int4*>(h + off_cells);
  for (int i = 0; i < n; ++i)
    h_cells[i] = make_int4(cells_xyz[3 * i], cells_xyz[3 * i + 1], cells_xyz[3 * i + 2], 0);
  std::memcpy(h + off_sums, sums, sizeof(int) * 8 * num_nodes);
  std::memcpy(h + off_path, path, sizeof(int) * num_nodes);
  CMX_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ws->stream));
  DebugChildSums3DKernel<<<as_family ? 1 : num_nodes, 256, 0, ws->stream>>>(
      reinterpret_cast<const Fast3DProblem*>(d), reinterpret_cast<const Node3D*>(d + off_nodes),
      num_nodes, as_family, live_mask, reinterpret_cast<int*>(d + off_sums),
      reinterpret_cast<int*>(d + off_path));
  CMX_HIP(hipGetLastError());
  CMX_HIP(hipMemcpyAsync(h + off_sums, d + off_sums, bytes - off_sums, hipMemcpyDeviceToHost,
                         ws->stream));
  CMX_HIP(hipStreamSynchronize(ws->stream));
  std::memcpy(sums, h + off_sums, sizeof(int) * 8 * num_nodes);
  std::memcpy(path, h + off_path, sizeof(int) * num_nodes);
}

}  // namespace
}  // namespace cmx

extern "C" {

cmx_status cmx_debug_fast3d_child_sums(const cmx_fast3d* matcher, const int32_t* cells_xyz,
                                       int32_t num_points, int32_t wxy, int32_t wz,
                                       const cmx_debug_fast3d_node* nodes, int32_t num_nodes,
                                       int32_t as_family, uint32_t live_mask, int32_t* sums,
                                       int32_t* path) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(matcher && cells_xyz && nodes && sums && path, "null argument");
    CMX_REQUIRE(num_points >= 1 && num_points <= (1 << 24), "num_points %d outside [1, 2^24]",
                num_points);
    CMX_REQUIRE(wxy >= 0 && wz >= 0 && wxy < (1 << 20) && wz < (1 << 20), "bad search window");
    CMX_REQUIRE(as_family == 0 || as_family == 1, "as_family must be 0 or 1");
    if (as_family)
      CMX_REQUIRE(num_nodes >= 2 && num_nodes <= 8, "a family has 2 .. 8 nodes, not %d", num_nodes);
    else
      CMX_REQUIRE(num_nodes >= 1 && num_nodes <= 65535, "num_nodes %d outside [1, 65535]",
                  num_nodes);
    const int depth = matcher->impl.options.branch_and_bound_depth;
    for (int i = 0; i < num_nodes; ++i) {
      CMX_REQUIRE(nodes[i].level >= 1 && nodes[i].level <= depth - 1,
                  "node %d: level %d outside [1, %d]", i, nodes[i].level, depth - 1);
      CMX_REQUIRE(!as_family || nodes[i].level == nodes[0].level,
                  "node %d: the nodes of a family share a level", i);
      // (candidate offsets lie within the window; anything an index of a 2^21 grid can meet)
      CMX_REQUIRE(std::abs(nodes[i].ox) <= (1 << 22) && std::abs(nodes[i].oy) <= (1 << 22) &&
                      std::abs(nodes[i].oz) <= (1 << 22),
                  "node %d: offset beyond 2^22 cells", i);
    }
    DebugChildSums3D(matcher->impl, cells_xyz, num_points, wxy, wz, nodes, num_nodes, as_family,
                     live_mask, sums, path);
  });
}

}  // extern "C"
