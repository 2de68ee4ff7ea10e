// The voxel filters of one small cloud by ONE workgroup, out of LDS: the device code that the
// single calls' SmallFilterKernel (filters.hip) and FilterBatchKernel (filters_batch.hip: a
// workgroup per job of cmx_filter_batch) have in common.  Up to kSmallCloud points the steps of
// the multi-launch path (filters.hip) run in one workgroup: bitonic sort of (key, index), segment
// heads, ranks, the prefix sum of the draws, the draws, the reservoir's last writer, the prefix
// sum of the kept flags -- and the adaptive filter's whole search (voxel_filter.cc:38-75), the
// lengths decided by the workgroup itself.  Same arithmetic, same point sets (tests: both paths
// against the oracle and each other).
#ifndef CMX_FILTERS_SMALL_DEVICE_H_
#define CMX_FILTERS_SMALL_DEVICE_H_

#include "cmx_device.h"
#include "filters_batch_plan.h"

namespace cmx {

constexpr unsigned kMinstdA = 16807u, kMinstdM = 2147483647u;      // std::minstd_rand0
constexpr unsigned long long kUrngRange = 2147483645ull;           // max() - min()

__device__ __forceinline__ unsigned MulMod(unsigned a, unsigned b) {
  return static_cast<unsigned>((static_cast<unsigned long long>(a) * b) % kMinstdM);
}
// t-th output (t >= 1) of a default-seeded (state 1) minstd_rand0.
__device__ __forceinline__ unsigned MinstdOutput(unsigned long long t) {
  unsigned result = 1u, base = kMinstdA;
  while (t) {
    if (t & 1ull) result = MulMod(result, base);
    base = MulMod(base, base);
    t >>= 1;
  }
  return result;
}

struct SmallFilterLds {       // carved from dynamic LDS; N = the cloud's size rounded up to a power of two
  unsigned long long* key;    // [N]
  unsigned* idx;              // [N]
  int *seg, *rank, *voxel, *pos, *selected;   // [N] each
  int* used;                  // = seg: the segment starts are dead when the flags are written
  int* wave_totals;           // [kSmallThreads / 64]
};
// (its size: SmallFilterLdsBytes, filters_batch_plan.h)
__device__ __forceinline__ SmallFilterLds CarveSmall(unsigned char* base, int N) {
  SmallFilterLds L;
  L.key = reinterpret_cast<unsigned long long*>(base); base += static_cast<size_t>(N) * 8;
  L.idx = reinterpret_cast<unsigned*>(base); base += static_cast<size_t>(N) * 4;
  int** ints[] = {&L.seg, &L.rank, &L.voxel, &L.pos, &L.selected};
  for (int** p : ints) { *p = reinterpret_cast<int*>(base); base += static_cast<size_t>(N) * 4; }
  L.used = L.seg;
  L.wave_totals = reinterpret_cast<int*>(base);
  return L;
}

// In place: data[i] <- sum of data[0 .. i - 1] (i < n <= 4 x blockDim); returns the total.
// Thread t owns elements 4 t .. 4 t + 3.
__device__ __forceinline__ int BlockExclusiveScan4(int* data, int n, int* wave_totals) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int v[4], sum = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = 4 * t + k;
    v[k] = i < n ? data[i] : 0;
    sum += v[k];
  }
  int incl = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) wave_totals[wave] = incl;
  __syncthreads();
  int before = incl - sum;
  int total = 0;
  for (int w = 0; w < static_cast<int>(blockDim.x >> 6); ++w) {
    const int wt = wave_totals[w];
    if (w < wave) before += wt;
    total += wt;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = 4 * t + k;
    if (i < n) data[i] = before;
    before += v[k];
  }
  __syncthreads();
  return total;
}

// In place inclusive MAX scan (segment starts from head-or-zero flags), same ownership.
__device__ __forceinline__ void BlockInclusiveMaxScan4(int* data, int n, int* wave_totals) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int v[4], top = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = 4 * t + k;
    v[k] = i < n ? data[i] : 0;
    top = max(top, v[k]);
    v[k] = top;                          // running maximum inside the thread
  }
  int incl = top;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl = max(incl, o);
  }
  if (lane == 63) wave_totals[wave] = incl;
  __syncthreads();
  int before = __shfl_up(incl, 1, 64);
  if (lane == 0) before = 0;
  for (int w = 0; w < wave; ++w) before = max(before, wave_totals[w]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = 4 * t + k;
    if (i < n) data[i] = max(v[k], before);
  }
  __syncthreads();
}

// RandomizedVoxelFilterIndices (voxel_filter.cc:88-131) of the n <= N points xyz[src[i]] (src:
// LDS or null = identity): L.used[i] = 1 for the kept ones, L.pos[i] = their exclusive prefix
// sum; returns the number kept.  Every thread of the workgroup calls it.
static __device__ int SmallVoxelFilter(const float* __restrict__ xyz, const int* src, int n, int N,
                                       float resolution, const SmallFilterLds& L,
                                       int* rejected_flag) {
  const int t = threadIdx.x, T = blockDim.x;
  // 1. keys, padded with the largest key (sorted behind every point)
  for (int i = t; i < N; i += T) {
    unsigned long long key = ~0ull;
    if (i < n) {
      const int at = src ? src[i] : i;
      const unsigned long long x = static_cast<unsigned long long>(
          static_cast<long long>(LRoundF32(xyz[3 * at] / resolution)));
      const unsigned long long y = static_cast<unsigned long long>(
          static_cast<long long>(LRoundF32(xyz[3 * at + 1] / resolution)));
      const unsigned long long z = static_cast<unsigned long long>(
          static_cast<long long>(LRoundF32(xyz[3 * at + 2] / resolution)));
      key = (x << 42) + (y << 21) + z;
    }
    L.key[i] = key;
    L.idx[i] = static_cast<unsigned>(i);
  }
  if (t == 0) *rejected_flag = 0;
  __syncthreads();
  // 2. bitonic sort by (key, index): indices are distinct, so this is the stable sort by key
  for (int k = 2; k <= N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < N; i += T) {
        const int partner = i ^ j;
        if (partner > i) {
          const unsigned long long ka = L.key[i], kb = L.key[partner];
          const unsigned ia = L.idx[i], ib = L.idx[partner];
          const bool greater = ka > kb || (ka == kb && ia > ib);
          const bool ascending = (i & k) == 0;
          if (greater == ascending) {
            L.key[i] = kb; L.key[partner] = ka;
            L.idx[i] = ib; L.idx[partner] = ia;
          }
        }
      }
      __syncthreads();
    }
  }
  // 3. segment starts (sorted position p: its own position if it opens a voxel, else 0; max-scan)
  for (int p = t; p < n; p += T) L.seg[p] = (p > 0 && L.key[p] != L.key[p - 1]) ? p : 0;
  __syncthreads();
  BlockInclusiveMaxScan4(L.seg, n, L.wave_totals);
  // 4. back to point order: k (1-based position in the voxel), the voxel (= segment start), the
  //    draw flag; the voxel's reservoir cleared
  for (int p = t; p < n; p += T) {
    const int i = static_cast<int>(L.idx[p]);
    const int k = p - L.seg[p] + 1;
    L.rank[i] = k;
    L.voxel[i] = L.seg[p];
    L.pos[i] = k >= 2 ? 1 : 0;
    if (k == 1) L.selected[p] = -1;
  }
  __syncthreads();
  // 5. stream position of every draw, the draws, the reservoir's last writer
  BlockExclusiveScan4(L.pos, n, L.wave_totals);
  for (int i = t; i < n; i += T) {
    const int k = L.rank[i];
    bool replace = true;
    if (k >= 2) {
      const unsigned long long ret = MinstdOutput(static_cast<unsigned long long>(L.pos[i]) + 1) - 1;
      const unsigned long long scaling = kUrngRange / static_cast<unsigned long long>(k);
      if (ret >= static_cast<unsigned long long>(k) * scaling) {
        *rejected_flag = 1;
        replace = false;
      } else {
        replace = ret / scaling == static_cast<unsigned long long>(k - 1);
      }
    }
    if (replace) atomicMax(&L.selected[L.voxel[i]], i);
  }
  __syncthreads();
  if (*rejected_flag) {
    // a draw was rejected (probability < k / 2^31 each) and shifts every later stream position:
    // one lane replays the generator in point order (SequentialDrawKernel)
    if (t == 0) {
      unsigned state = 1u;
      for (int i = 0; i < n; ++i) {
        const int k = L.rank[i];
        if (k >= 2) {
          const unsigned long long scaling = kUrngRange / static_cast<unsigned long long>(k);
          const unsigned long long past = static_cast<unsigned long long>(k) * scaling;
          unsigned long long ret;
          do {
            state = MulMod(state, kMinstdA);
            ret = state - 1u;
          } while (ret >= past);
          if (ret / scaling == static_cast<unsigned long long>(k - 1)) L.selected[L.voxel[i]] = i;
        } else {
          L.selected[L.voxel[i]] = i;
        }
      }
    }
    __syncthreads();
  }
  // 6. points_used and their prefix sum
  for (int i = t; i < n; i += T) {
    const int u = L.selected[L.voxel[i]] == i ? 1 : 0;
    L.used[i] = u;
    L.pos[i] = u;
  }
  __syncthreads();
  return BlockExclusiveScan4(L.pos, n, L.wave_totals);
}

// Where a workgroup leaves its result.  `count`, `indices`, `points`: pinned host memory, the
// number kept, their indices in the input (ascending) and their coordinates; `device_count`,
// `device_points`: the same in device memory, for a job of a later launch that filters this
// result.  All but `count` may be null.
struct SmallFilterResult {
  int* count;
  int* indices;
  float* points;
  int* device_count;
  float* device_points;
};

// The whole filter of the n0 <= N points `xyz`, by every thread of a workgroup of kSmallThreads
// with SmallFilterLaunchLds(N) bytes of dynamic LDS at `smem`.  mode 0: VoxelFilter(resolution =
// length);  mode 1: AdaptiveVoxelFilter(max_length = length, min_num_points, max_range).
__device__ __forceinline__ void SmallFilterWorkgroup(unsigned char* smem,
                                                     const float* __restrict__ xyz, int n0, int N,
                                                     int mode, float length, float min_num_points,
                                                     float max_range, const SmallFilterResult& out) {
  const SmallFilterLds L = CarveSmall(smem, N);
  // behind the filter's arrays: the active list (adaptive: the points in range), the best
  // result so far as flags
  int* src = L.wave_totals + 64;
  unsigned char* best_used = reinterpret_cast<unsigned char*>(src + N);
  __shared__ int rejected;
  const int t = threadIdx.x, T = blockDim.x;
  int n = n0;
  const int* active = nullptr;
  if (mode == 1) {
    // FilterByMaxRange (voxel_filter.cc:30-36)
    for (int i = t; i < n0; i += T) {
      const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
      const int u = sqrtf((x * x + y * y) + z * z) <= max_range ? 1 : 0;   // position.norm()
      L.used[i] = u;
      L.pos[i] = u;
    }
    __syncthreads();
    n = BlockExclusiveScan4(L.pos, n0, L.wave_totals);
    for (int i = t; i < n0; i += T)
      if (L.used[i]) src[L.pos[i]] = i;
    __syncthreads();
    active = src;
  }
  bool have_flags = false;             // false: every active point is kept
  if (mode == 0) {
    SmallVoxelFilter(xyz, active, n, N, length, L, &rejected);
    for (int i = t; i < n; i += T) best_used[i] = static_cast<unsigned char>(L.used[i]);
    have_flags = true;
    __syncthreads();
  } else if (!(static_cast<float>(n) <= min_num_points)) {
    // AdaptivelyVoxelFiltered (voxel_filter.cc:38-75): the same sequence of VoxelFilter calls;
    // every thread walks the same control flow (counts come back uniform).
    const auto evaluate = [&](float len, bool accept_always, int* count) {
      const int m = SmallVoxelFilter(xyz, active, n, N, len, L, &rejected);
      *count = m;
      const bool accept = accept_always || static_cast<float>(m) >= min_num_points;
      if (accept) {
        for (int i = t; i < n; i += T) best_used[i] = static_cast<unsigned char>(L.used[i]);
        __syncthreads();
      }
      return accept;
    };
    int m = 0;
    bool done = false;
    evaluate(length, true, &m);                      // result = VoxelFilter(cloud, max_length)
    have_flags = true;
    if (static_cast<float>(m) >= min_num_points) done = true;
    for (float high_length = length; !done && high_length > 1e-2f * length; high_length /= 2.f) {
      float low_length = high_length / 2.f;
      evaluate(low_length, true, &m);                // result = VoxelFilter(cloud, low_length)
      if (static_cast<float>(m) >= min_num_points) {
        while ((high_length - low_length) / low_length > 1e-1f) {
          const float mid_length = (low_length + high_length) / 2.f;
          if (evaluate(mid_length, false, &m)) {
            low_length = mid_length;
          } else {
            high_length = mid_length;
          }
        }
        done = true;
      }
    }
  }
  // ---- the result: indices into the input, ascending, and the points -------------------------
  for (int i = t; i < n; i += T) {
    const int u = have_flags ? best_used[i] : 1;
    L.used[i] = u;
    L.pos[i] = u;
  }
  __syncthreads();
  const int total = BlockExclusiveScan4(L.pos, n, L.wave_totals);
  for (int i = t; i < n; i += T) {
    if (!L.used[i]) continue;
    const int at = active ? active[i] : i;
    const int o = L.pos[i];
    if (out.indices) out.indices[o] = at;
    if (out.points || out.device_points) {
      const float x = xyz[3 * at], y = xyz[3 * at + 1], z = xyz[3 * at + 2];
      if (out.points) {
        out.points[3 * o] = x;
        out.points[3 * o + 1] = y;
        out.points[3 * o + 2] = z;
      }
      if (out.device_points) {
        out.device_points[3 * o] = x;
        out.device_points[3 * o + 1] = y;
        out.device_points[3 * o + 2] = z;
      }
    }
  }
  if (t == 0) {
    *out.count = total;
    if (out.device_count) *out.device_count = total;
  }
}

}  // namespace cmx

#endif  // CMX_FILTERS_SMALL_DEVICE_H_
