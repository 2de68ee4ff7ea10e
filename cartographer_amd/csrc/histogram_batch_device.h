// RotationalScanMatcher::ComputeHistogram of one small cloud by ONE workgroup, out of LDS: the
// device code of cmx_compute_histogram_batch (histogram_batch.hip: a workgroup per job).  Up to
// kSmallCloud points the steps of the single call (filters.hip: three radix sorts, a scan,
// SliceKeyKernel, SliceAngleKernel, SliceWalkKernel, HistogramChainKernel) run in one workgroup
// with their expressions unchanged:
//   1. slice keys; bitonic sort of (key, input index); the runs of equal key are the slices, in
//      input order inside;
//   2. the first centroid of every slice, a sequential f32 sum in that order, one lane per
//      (slice, coordinate) chain;
//   3. the angle of every point around it; bitonic sort of (slice, angle key, position in the
//      slice order) -- the third component is the radix sort's stability;
//   4. the second centroid over the kept points in angle order; the `last_point_position` walk,
//      a short slice by one lane, a long one by a wavefront 64 points per step; every point's
//      vote (bucket, value);
//   5. bitonic sort of (bucket, position) -- 32-bit keys --, which groups the votes stably by
//      bucket; one lane per bucket adds its segment up in order, into a zero.
// No atomics, no partial histograms: f32 addition does not associate (HistogramChainKernel).
//
// LDS, for N = the points rounded up to a power of two (HistogramLdsBytes: 36 N + 320):
//   key   [N] u64   sort keys (step 5: 32-bit ones); between the sorts of steps 3 and 5 the
//                   second centroids
//   a.x a.y [N] f32 coordinates by input index; first centroids by slice; coordinates in angle
//                   order; the votes' values in bucket order
//   b.x b.y [N] f32 coordinates in slice order; the walk's `last` of every point; the votes
//   slice [N] int   slice of every position (the same in slice and in angle order)
//   begin [N] int   first position of every slice
//   kept  [N] int   end of the kept points of every slice
#ifndef CMX_HISTOGRAM_BATCH_DEVICE_H_
#define CMX_HISTOGRAM_BATCH_DEVICE_H_

#include "cmx_atan2f.h"
#include "cmx_device.h"
#include "filters_small_device.h"
#include "histogram_batch_plan.h"
#include "histogram_common.h"

// (a probe that includes this header may define the hook to time the steps; nothing in the library)
#ifndef CMX_HISTOGRAM_STAMP
#define CMX_HISTOGRAM_STAMP(k)
#endif

namespace cmx {

constexpr int kWindowSlice = 256;      // kept points of a slice from which a wavefront walks it

struct HistogramLds {
  unsigned long long* key;
  float *ax, *ay, *bx, *by;
  int *slice, *begin, *kept;
  int* wave_totals;            // [64]
};
__device__ __forceinline__ HistogramLds CarveHistogram(unsigned char* base, int N) {
  HistogramLds L;
  L.key = reinterpret_cast<unsigned long long*>(base); base += static_cast<size_t>(N) * 8;
  float** rows[] = {&L.ax, &L.ay, &L.bx, &L.by};
  for (float** p : rows) { *p = reinterpret_cast<float*>(base); base += static_cast<size_t>(N) * 4; }
  int** ints[] = {&L.slice, &L.begin, &L.kept};
  for (int** p : ints) { *p = reinterpret_cast<int*>(base); base += static_cast<size_t>(N) * 4; }
  L.wave_totals = reinterpret_cast<int*>(base);
  return L;
}

// Ascending bitonic sort of the N (a power of two, 64 .. 4 x blockDim) keys at `key` in LDS
// (Key: 64 or 32 bits, unsigned), by every thread of the workgroup; begins and ends with a
// barrier.  (The keys of the points are distinct -- their low bits are a position -- so the order
// is the stable one; only the padding repeats.)  Thread t keeps elements 4 t .. 4 t + 3 in
// registers, so a wavefront owns 256 neighbours: the compare-exchange steps at distance 1 and 2
// stay inside the thread, those at 4 .. 128 are lane exchanges without a barrier, and only the
// distances from 256 on -- 10 of the 78 steps of N = 4096 -- go through LDS: every thread stores
// its four, one barrier, every thread reads its partner's four.  Those steps alternate between
// `key` and `spare` (N keys too), so that a store never meets the reads of the step before.
// With all 16 wavefronts at work a step is bound by its vector instructions (four wavefronts
// share a SIMD), so a step is kept short: from distance 4 on a thread's four elements are on the
// same side of their pairs and of their block, one predicate for the four.
template <class Key>
__device__ __forceinline__ void BitonicSortLds(Key* key, Key* spare, int N) {
  const int base = 4 * static_cast<int>(threadIdx.x);
  const bool active = base < N;
  const bool wave_active = 4 * static_cast<int>(threadIdx.x & ~63u) < N;
  __syncthreads();
  Key v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = active ? key[base + e] : static_cast<Key>(~static_cast<Key>(0));
  // a pair of the thread's own: the lower one keeps the smaller key in an ascending block
  const auto inside = [&](int low, int high, bool ascending) {
    const Key a = v[low], b = v[high];
    if ((a > b) == ascending) { v[low] = b; v[high] = a; }
  };
  bool to_spare = true;
  for (int k = 2; k <= N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      // (a wavefront without elements only meets the barriers: four wavefronts share a SIMD)
      if (j < 256 && !wave_active) continue;
      if (j >= 4) {
        // the thread's elements keep the smaller keys if they are the lower ones of an ascending
        // block or the upper ones of a descending block
        const bool keep_min = ((base & j) == 0) == ((base & k) == 0);
        Key other[4];
        if (j >= 256) {
          Key* const buffer = to_spare ? spare : key;
          to_spare = !to_spare;
          if (active) {
#pragma unroll
            for (int e = 0; e < 4; ++e) buffer[base + e] = v[e];
          }
          __syncthreads();
#pragma unroll
          for (int e = 0; e < 4; ++e) other[e] = active ? buffer[(base ^ j) + e] : v[e];
        } else {
          // (every lane of the wavefront takes part: one without elements carries padding
          //  nobody asks for)
#pragma unroll
          for (int e = 0; e < 4; ++e) other[e] = __shfl_xor(v[e], j >> 2, 64);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if ((other[e] < v[e]) == keep_min) v[e] = other[e];
      } else if (j == 2) {
        const bool ascending = (base & k) == 0;            // (k >= 4)
        inside(0, 2, ascending);
        inside(1, 3, ascending);
      } else {
        inside(0, 1, (base & k) == 0);
        inside(2, 3, ((base + 2) & k) == 0);
      }
    }
  }
  __syncthreads();       // (the last step through LDS may have been read from `key`)
  if (active) {
#pragma unroll
    for (int e = 0; e < 4; ++e) key[base + e] = v[e];
  }
  __syncthreads();
}

// acc + row[b] + row[b + 1] + ... + row[e - 1], one addition after the other, by one lane: the
// whole blocks of 64 (64-float aligned: `row` is a carved array) through ChainSumLds, the ends
// one by one.
__device__ __forceinline__ float ChainRangeLds(const float* row, int b, int e, float acc) {
  int k = b;
  const int aligned = min((b + 63) & ~63, e);
  for (; k < aligned; ++k) acc += row[k];
  const int whole = (e - k) & ~63;
  if (whole > 0) {
    acc = ChainSumLds(row + k, whole, acc);
    k += whole;
  }
  for (; k < e; ++k) acc += row[k];
  return acc;
}

// The whole histogram of the n <= N points `xyz`, by every thread of a workgroup of
// kSmallThreads with HistogramLdsBytes(N) bytes of dynamic LDS at `smem`; `histogram`:
// histogram_size floats (pinned host or device memory).  The coordinates are finite.
__device__ __forceinline__ void HistogramWorkgroup(unsigned char* smem,
                                                   const float* __restrict__ xyz, int n, int N,
                                                   int histogram_size, float min_distance_sq,
                                                   float max_distance_sq,
                                                   float* __restrict__ histogram) {
  const HistogramLds L = CarveHistogram(smem, N);
  const int t = threadIdx.x, T = blockDim.x;
  const int wave = t >> 6, lane = t & 63, waves = T >> 6;

  CMX_HISTOGRAM_STAMP(0);
  // ---- 1. slices --------------------------------------------------------------------------
  for (int i = t; i < N; i += T) {
    unsigned long long key = ~0ull;              // padding sorts behind every point
    if (i < n) {
      L.ax[i] = xyz[3 * i];
      L.ay[i] = xyz[3 * i + 1];
      // std::map<int, ...> order: ascending RoundToInt(z / kSliceHeight); biased to unsigned.
      const unsigned z_key = static_cast<unsigned>(LRoundF32(xyz[3 * i + 2] / kSliceHeight)) ^ 0x80000000u;
      key = (static_cast<unsigned long long>(z_key) << 32) | static_cast<unsigned>(i);
    }
    L.key[i] = key;
  }
  CMX_HISTOGRAM_STAMP(1);
  BitonicSortLds(L.key, reinterpret_cast<unsigned long long*>(L.bx), N);   // (b: not yet written)
  CMX_HISTOGRAM_STAMP(2);
  const auto opens_slice = [&](int p) {
    return p == 0 || static_cast<unsigned>(L.key[p] >> 32) != static_cast<unsigned>(L.key[p - 1] >> 32);
  };
  for (int p = t; p < n; p += T) {
    const int i = static_cast<int>(L.key[p] & 0xffffffffull);
    L.bx[p] = L.ax[i];
    L.by[p] = L.ay[i];
    L.slice[p] = opens_slice(p) ? 1 : 0;
  }
  __syncthreads();
  const int slices = BlockExclusiveScan4(L.slice, n, L.wave_totals);   // heads before p
  for (int p = t; p < n; p += T) {
    const bool head = opens_slice(p);
    const int s = L.slice[p] + (head ? 1 : 0) - 1;
    L.slice[p] = s;
    if (head) L.begin[s] = p;
  }
  __syncthreads();
  CMX_HISTOGRAM_STAMP(3);
  const auto slice_end = [&](int s) { return s + 1 < slices ? L.begin[s + 1] : n; };

  // ---- 2. ComputeCentroid (:47-53) of every slice: chain c = (slice, coordinate), dealt to
  //         the wavefronts first so that the long ones do not share one -------------------------
  float* const c1x = L.ax;       // (the coordinates by input index are dead)
  float* const c1y = L.ay;
  for (int c = lane * waves + wave; c < 2 * slices; c += T) {
    const int s = c >> 1, b = L.begin[s], e = slice_end(s);
    const float sum = ChainRangeLds((c & 1) ? L.by : L.bx, b, e, 0.f);
    ((c & 1) ? c1y : c1x)[s] = sum / static_cast<float>(e - b);
  }
  __syncthreads();

  CMX_HISTOGRAM_STAMP(4);
  // ---- 3. angles around the first centroid (SliceAngleKernel); sorted by (slice, angle,
  //         position in slice order = ascending input index inside a slice) ---------------------
  for (int p = t; p < N; p += T) {
    unsigned long long key = ~0ull;
    if (p < n) {
      const int s = L.slice[p];
      const float dx = L.bx[p] - c1x[s], dy = L.by[p] - c1y[s];
      unsigned angle_key = 0xffffffffu;           // dropped: behind the kept points of the slice
      if (!(sqrtf(dx * dx + dy * dy) < kMinDistance)) {
        const unsigned bits = FloatToBits(Atan2fGlibc(dy, dx));
        angle_key = bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
        if (angle_key == 0xffffffffu) angle_key -= 1;     // keep the "dropped" key unique
      }
      key = (static_cast<unsigned long long>(s) << 44) |
            (static_cast<unsigned long long>(angle_key) << 12) | static_cast<unsigned>(p);
    }
    L.key[p] = key;
  }
  for (int s = t; s < slices; s += T) L.kept[s] = slice_end(s);
  CMX_HISTOGRAM_STAMP(5);
  BitonicSortLds(L.key, reinterpret_cast<unsigned long long*>(L.ax), N);   // (a: the centroids are dead)
  CMX_HISTOGRAM_STAMP(6);
  const auto dropped = [&](int p) {
    return (static_cast<unsigned>(L.key[p] >> 12) & 0xffffffffu) == 0xffffffffu;
  };
  for (int p = t; p < n; p += T) {
    const int from = static_cast<int>(L.key[p] & 0xfffull);
    L.ax[p] = L.bx[from];
    L.ay[p] = L.by[from];
    // the first dropped point of its slice ends the kept ones
    if (dropped(p) && (p == L.begin[L.slice[p]] || !dropped(p - 1))) L.kept[L.slice[p]] = p;
  }
  __syncthreads();

  CMX_HISTOGRAM_STAMP(7);
  // ---- 4. per slice in angle order: AddPointCloudSliceToHistogram's walk (:55-83) ----------
  float* const c2x = reinterpret_cast<float*>(L.key);     // (the keys are dead until step 5)
  float* const c2y = c2x + N;
  for (int c = lane * waves + wave; c < 2 * slices; c += T) {
    const int s = c >> 1, b = L.begin[s], e = L.kept[s];
    if (e <= b) continue;
    const float sum = ChainRangeLds((c & 1) ? L.ay : L.ax, b, e, 0.f);
    ((c & 1) ? c2y : c2x)[s] = sum / static_cast<float>(e - b);
  }
  __syncthreads();
  CMX_HISTOGRAM_STAMP(8);
  const float kNaN = __uint_as_float(0x7fc00000u);
  float* const last_x = L.bx;      // (the coordinates in slice order are dead)
  float* const last_y = L.by;
  for (int p = t; p < n; p += T)
    if (p >= L.kept[L.slice[p]]) last_x[p] = kNaN;       // dropped: no vote
  // A slice of fewer than kWindowSlice kept points is walked by ONE LANE, point after point, 64
  // slices to a wavefront (the low wavefronts first: a wavefront costs its instructions whether
  // one lane or 64 are at work): a cloud of many short slices, where `last` moves at almost every
  // point, is bound by the instructions of the walk, not by their latency.
  for (int s = t; s < slices; s += T) {
    const int begin = L.begin[s], kept_end = L.kept[s];
    if (kept_end <= begin || kept_end - begin >= kWindowSlice) continue;
    const float cx = c2x[s], cy = c2y[s];
    float lx = L.ax[begin], ly = L.ay[begin];
    for (int k = begin; k < kept_end; ++k) {
      const float px = L.ax[k], py = L.ay[k];
      const float ex = px - cx, ey = py - cy;
      const bool near = sqrtf(ex * ex + ey * ey) < kMinDistance;
      const float dx = px - lx, dy = py - ly;
      const float d2 = dx * dx + dy * dy;
      const bool skip = d2 < min_distance_sq || near;
      const bool moves = !skip && d2 > max_distance_sq;
      last_x[k] = moves ? kNaN : lx;           // (the point that becomes `last` -- no vote)
      last_y[k] = ly;
      if (moves) { lx = px; ly = py; }
    }
  }
  // A longer slice (16 of them at most) by a wavefront, SliceWalkKernel's window: 64 points in
  // registers while `last` moves inside it.
  for (int s = wave; s < slices; s += waves) {
    const int begin = L.begin[s], kept_end = L.kept[s];
    if (kept_end - begin < kWindowSlice) continue;
    const float cx = c2x[s], cy = c2y[s];
    float lx = L.ax[begin], ly = L.ay[begin];
    for (int c = begin; c < kept_end; c += 64) {
      const int k = c + lane;
      const bool valid = k < kept_end;
      const float px = valid ? L.ax[k] : 0.f, py = valid ? L.ay[k] : 0.f;
      const float ex = px - cx, ey = py - cy;
      const bool near = valid && sqrtf(ex * ex + ey * ey) < kMinDistance;
      float my_lx = 0.f, my_ly = 0.f;
      for (int start = 0;;) {
        const float dx = px - lx, dy = py - ly;
        const float d2 = dx * dx + dy * dy;
        const bool skip = d2 < min_distance_sq || near;
        const unsigned long long moves =
            __ballot(valid && lane >= start && !skip && d2 > max_distance_sq);
        const int j = moves ? __builtin_ctzll(moves) : 64;
        if (lane >= start && lane <= j) {      // (lane j: the point that becomes `last` -- no vote)
          my_lx = lane == j ? kNaN : lx;
          my_ly = ly;
        }
        if (j == 64) break;
        lx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(px), j));
        ly = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(py), j));
        start = j + 1;
      }
      if (valid) { last_x[k] = my_lx; last_y[k] = my_ly; }
    }
  }
  __syncthreads();
  CMX_HISTOGRAM_STAMP(9);
  // every point's vote at its position in the global (slice, angle) order
  const float kPi = static_cast<float>(M_PI);
  for (int k = t; k < n; k += T) {
    unsigned bucket = kNoVote;
    float v = 0.f;
    const float lx = last_x[k];
    if (!(lx != lx)) {
      const int s = L.slice[k];
      const float px = L.ax[k], py = L.ay[k];
      const float dx = px - lx, dy = py - last_y[k];
      const float ex = px - c2x[s], ey = py - c2y[s];
      const float distance = sqrtf(dx * dx + dy * dy);
      const float direction_norm = sqrtf(ex * ex + ey * ey);
      // (distance > kMaxDistance cannot occur here: that point moved `last`)
      if (!(distance < kMinDistance || direction_norm < kMinDistance)) {
        float angle = Atan2fGlibc(dy, dx);
        const float ndx = dx / distance, ndy = dy / distance;
        const float nex = ex / direction_norm, ney = ey / direction_norm;
        v = fmaxf(0.f, 1.f - fabsf(ndx * nex + ndy * ney));
        while (angle > kPi) angle -= kPi;
        while (angle < 0.f) angle += kPi;
        const float zero_to_one = angle / kPi;
        bucket = static_cast<unsigned>(min(
            max(LRoundF32(histogram_size * zero_to_one - 0.5f), 0), histogram_size - 1));
      }
    }
    L.bx[k] = v;                                  // (over this thread's own `last`)
    L.by[k] = __uint_as_float(bucket);
  }
  __syncthreads();

  // ---- 5. the votes grouped stably by bucket, a bucket's added one by one ---------------------
  // (bucket <= kNoVote and position < 4096: 28 bits, a 32-bit key -- a third of the sort's
  //  instructions)
  unsigned* const vote_key = reinterpret_cast<unsigned*>(L.key);
  for (int k = t; k < N; k += T)
    vote_key[k] = k < n ? (__float_as_uint(L.by[k]) << 12) | static_cast<unsigned>(k) : ~0u;
  CMX_HISTOGRAM_STAMP(10);
  BitonicSortLds(vote_key, reinterpret_cast<unsigned*>(L.ax), N);   // (a: the coordinates are dead)
  CMX_HISTOGRAM_STAMP(11);
  float* const votes = L.ax;
  float* const vote_of = L.bx;
  for (int q = t; q < n; q += T) votes[q] = vote_of[vote_key[q] & 0xfffu];
  __syncthreads();
  CMX_HISTOGRAM_STAMP(12);
  const auto lower_bound = [&](unsigned bucket) {
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((vote_key[mid] >> 12) < bucket) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  for (int b = lane * waves + wave; b < histogram_size; b += T) {
    const int first = lower_bound(static_cast<unsigned>(b));
    const int last = lower_bound(static_cast<unsigned>(b) + 1);
    histogram[b] = ChainRangeLds(votes, first, last, 0.f);
  }
  CMX_HISTOGRAM_STAMP(13);
}

}  // namespace cmx

#endif  // CMX_HISTOGRAM_BATCH_DEVICE_H_
