// Batched RealTimeCorrelativeScanMatcher2D::Match on device-resident TSDF2Ds
// (cmx_rt2d_match_tsdf_grid_batch, cmx_rt2d_match_tsdf_grid_batch_resident).
//
// Reference: SM2/real_time_correlative_scan_matcher_2d.cc:38-59 (ComputeCandidateScore on a
// TSDF2D), :117-176 (Match, ScoreCandidates), mapping/internal/2d/tsdf_2d.cc:88-98
// (GetTSDAndWeight), mapping/value_conversion_tables.cc:29-52.
//
// A candidate's score is chain(sum a_p) / chain(sum b_p): a_p = ((T - |tsd_p|) / T) w_p and
// b_p = w_p in f32, summed in point order; cells outside the grid and unknown cells give
// (a, b) = (0, 0) or (0, w).  Behind the two value tables sits an integer model: with v_t, v_w
// the cell values masked of bit 15,
//     D = 16383 - |v_t - 16384|  (0 for v_t = 0),   B = v_w - 1  (0 for v_w = 0),   A = D B,
//     a_p = W / (16383 * 32766) * A_p,   b_p = W / 32766 * B_p   up to the tables' rounding,
// so the real-valued score is  R = sum A / (16383 sum B)  (0 when sum B = 0).
//
// Stage A (Tsdf2DImageKernel): two byte images per grid version, qa = ceil(A / kQA) and
//   qb = ceil(B / kQB), with a zero halo; a zero cell stays zero, a non-zero cell is non-zero.
// Stage B (TsdfBulkKernel): a workgroup = (match, group of rotations) copies both images of a tile
//   into LDS, discretises its rotations' points with the bit-exact cell routine, and every thread
//   = (rotation, y offset) sums the row of x offsets of both images with packed 16-bit adds over
//   aligned dword reads.  From the two integer sums, the quantisation width, the slack of the f32
//   chains and the roundings it writes an interval [lo, hi] that holds the candidate's weighted
//   reference score, and the match keeps the best lower end.
// Stage C: candidates with hi >= best lo (strictly: only hi < best lo drops one, so the winner and
//   every tie stay) are compacted (TsdfSelectKernel) and evaluated by the reference's own two
//   sequential f32 chains out of the uint16 planes (TsdfExactKernel: TsdfTerm, unchanged); those
//   within 1e-5 of the best exact weighted score go to the host (TsdfCollectKernel), which applies
//   the libm weight and the first-maximum rule exactly as the per-candidate path does.  The exact
//   evaluation walks the planes point by point whichever arithmetic it runs, so the f32 chains ride
//   on the loads an exact integer re-sum would need and no separate integer stage is run.
// A match whose finalist list overflows (flat landscapes: thousands of exact ties) is repeated
// alone on the per-candidate kernels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "rt_2d_device.h"
#include "scan_matching_2d.h"

namespace cmx {

Tsdf2DImageCache::~Tsdf2DImageCache() {
  if (images) (void)hipFree(images);
}

namespace {

constexpr int kQA = 2113536;          // 16383 * 32766 / kQA < 254
constexpr int kQB = 129;              // 32766 / kQB = 254
constexpr int kTsdfMaxNl = 7;         // side <= 15: four dwords of x offsets per row
constexpr int kTsdfThreads = 256;
constexpr int kTsdfMaxRotations = 32; // rotations per workgroup
constexpr int kTsdfMaxCoreW = 1024;   // columns of a tile's core
constexpr int kTsdfLdsBytes = 150 * 1024;
// Words of a match's 128-word result slot beyond the finalist head (2 + 2 * kFinalistHead = 124).
constexpr int kCtlBestLo = 124, kCtlSurvivors = 125, kCtlError = 126;

// Slack of an interval for what separates the reference's f32 score from R: two chains of n
// non-negative terms ((n - 1) 2^-24 relative each in first order), the division, the weight
// table (three roundings per term) and the normalised tsd (absolute 5 * 2^-24 per term: the
// cancellation in T - |tsd|).  The score is at most 1, so relative and absolute agree; twice the
// first-order sum plus 1e-4.
__host__ __device__ inline float TsdfSlack(int n) { return 1e-4f + 2.4e-7f * static_cast<float>(n); }

struct TsdfBatchParams {
  const uint16_t* tsd;
  const uint16_t* weight;
  uint8_t* images;           // numerator image [irows][ipitch], then the weight image
  int nx, ny, ipitch, irows;
  int build;                 // 1: this call builds `images`
  Rt2DFrame frame;
  int nl, side, num_scans, num_angular, n;
  int rot_per_group, groups;
  int c_begin, c_end, r_begin, r_end;   // image columns / rows a point's cell can take
  int core_w, core_h, tiles_x, tiles_y, tile_w, tile_h;
  double step, wt, wr;
  float max_tsd, max_weight, slack;
  const float2* scan_rot;
  const float* xyz;
  float* lo;                 // [num_candidates] interval of the weighted score
  float* hi;
  int num_candidates;
  unsigned* misc;            // [0] best exact weighted bits, [1] finalists, pairs; kCtl* words
  unsigned* overflow;
  unsigned* survivors;       // [num_candidates] candidate indices the intervals leave
  float* surv_score;         // [num_candidates], by survivor slot
  float* surv_weighted;
};

// exp(-(hypot * wt + |theta| * wr)^2) of candidate (s, dx, dy) as the device evaluates it; the
// host repeats it with libm for the finalists.
__device__ __forceinline__ double TsdfDeviceWeight(const TsdfBatchParams& P, int s, int dx, int dy) {
  const double cx = -dy * P.frame.res, cy = -dx * P.frame.res;
  const double theta = (s - P.num_angular) * P.step;
  const double t = hypot(cx, cy) * P.wt + fabs(theta) * P.wr;
  return exp(-(t * t));
}

// grid (blocks, 1, matches); matches that do not build return at once.
__global__ void __launch_bounds__(256) Tsdf2DImageKernel(const TsdfBatchParams* __restrict__ params) {
  const TsdfBatchParams& P = params[blockIdx.z];
  if (!P.build) return;
  const int total = P.ipitch * P.irows;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int row = e / P.ipitch, col = e - row * P.ipitch;
  const int x = col - kTsdfImageHalo, y = row - kTsdfImageHalo;
  unsigned qa = 0, qb = 0;
  if (static_cast<unsigned>(x) < static_cast<unsigned>(P.nx) &&
      static_cast<unsigned>(y) < static_cast<unsigned>(P.ny)) {
    const int flat = P.nx * y + x;
    const int vt = P.tsd[flat] & 32767, vw = P.weight[flat] & 32767;
    const int b = vw ? vw - 1 : 0;
    const int d = vt ? 16383 - abs(vt - 16384) : 0;
    const unsigned a = static_cast<unsigned>(d) * static_cast<unsigned>(b);   // < 2^29
    qa = (a + (kQA - 1)) / kQA;
    qb = (static_cast<unsigned>(b) + (kQB - 1)) / kQB;
  }
  P.images[e] = static_cast<uint8_t>(qa);
  P.images[total + e] = static_cast<uint8_t>(qb);
}

// The interval of a candidate's weighted reference score from its two quantised sums.
__device__ __forceinline__ void TsdfInterval(unsigned sa, unsigned sb, int n, double e, float slack,
                                             float* lo, float* hi) {
  if (sb == 0) {           // every weight is zero: the reference returns 0 (:55)
    *lo = 0.f;
    *hi = 0.f;
    return;
  }
  const double un = static_cast<double>(n);
  const double a_hi = static_cast<double>(kQA) * sa;
  const double a_lo = a_hi - (kQA - 1) * fmin(un, static_cast<double>(sa));
  const double b_hi = static_cast<double>(kQB) * sb;
  const double b_lo = b_hi - (kQB - 1) * fmin(un, static_cast<double>(sb));   // >= sb > 0
  const double r_lo = a_lo / (16383.0 * b_hi);
  const double r_hi = fmin(1.0, a_hi / (16383.0 * b_lo));   // a_p <= b_p: the ratio never exceeds 1
  const double s_lo = fmax(0.0, r_lo - slack), s_hi = fmin(1.0, r_hi + slack);
  *lo = static_cast<float>(s_lo * e * (1.0 - 1e-6));
  *hi = static_cast<float>(s_hi * e * (1.0 + 1e-6));
}

// grid (rotation groups, matches), kTsdfThreads threads; dynamic LDS: [rot_per_group][64] packed
// cells of the current 64 points, then the tile's two byte images ([tile_h][tile_w] each).
// ND = dwords of x offsets per row (side <= 4 ND).
template <int ND>
__global__ void __launch_bounds__(kTsdfThreads)
TsdfBulkKernel(const TsdfBatchParams* __restrict__ params) {
  extern __shared__ uint32_t tsdf_lds[];
  const TsdfBatchParams& P = params[blockIdx.y];
  const int group = blockIdx.x;
  if (group >= P.groups) return;
  const int t = threadIdx.x;
  const int side = P.side, nl = P.nl, G = P.rot_per_group, n = P.n;
  const int r = t / side, dyi = t - r * side;
  const int s = group * G + r;
  const bool active = r < G && s < P.num_scans;
  uint32_t* cellbuf = tsdf_lds;
  uint32_t* img = tsdf_lds + G * 64;
  const int wd = P.tile_w >> 2;                    // dwords per tile row
  const int plane_dwords = wd * P.tile_h;
  const Rt2DFrame F = P.frame;
  const float* __restrict__ xyz = P.xyz;
  const int total = P.ipitch * P.irows;

  uint32_t acc_a[4 * ND], acc_b[4 * ND];
#pragma unroll
  for (int k = 0; k < 4 * ND; ++k) acc_a[k] = acc_b[k] = 0;

  for (int ty = 0; ty < P.tiles_y; ++ty) {
    for (int tx = 0; tx < P.tiles_x; ++tx) {
      const int c0 = P.c_begin + tx * P.core_w, c1 = min(c0 + P.core_w, P.c_end);
      const int r0 = P.r_begin + ty * P.core_h, r1 = min(r0 + P.core_h, P.r_end);
      const int ox = (c0 - nl) & ~3, oy = r0 - nl;
      __syncthreads();                             // the previous tile has been read
      for (int j = t >> 6; j < 2 * P.tile_h; j += kTsdfThreads / 64) {
        const int plane = j >= P.tile_h ? 1 : 0;
        const int row = oy + (j - plane * P.tile_h);
        for (int i = t & 63; i < wd; i += 64) {
          const int col = ox + 4 * i;
          uint32_t v = 0;
          if (row >= 0 && row < P.irows && col >= 0 && col + 4 <= P.ipitch)
            v = *reinterpret_cast<const uint32_t*>(P.images + static_cast<size_t>(plane) * total +
                                                   static_cast<size_t>(row) * P.ipitch + col);
          img[j * wd + i] = v;
        }
      }
      for (int base = 0; base < n; base += 64) {
        __syncthreads();                           // image loaded / previous chunk summed
        for (int e = t; e < G * 64; e += kTsdfThreads) {
          const int rr = e >> 6, i = e & 63;
          const int ss = group * G + rr, pt = base + i;
          uint32_t packed = 0xffffffffu;
          if (ss < P.num_scans && pt < n) {
            const float2 rot = P.scan_rot[ss];
            int ix, iy;
            Rt2DCellOf(F, rot.x, rot.y, xyz[3 * pt], xyz[3 * pt + 1], &ix, &iy);
            packed = static_cast<uint32_t>(ix + kTsdfImageHalo) |
                     (static_cast<uint32_t>(iy + kTsdfImageHalo) << 16);
          }
          cellbuf[e] = packed;
        }
        __syncthreads();
        if (active) {
          uint32_t pe_a[ND], po_a[ND], pe_b[ND], po_b[ND];
#pragma unroll
          for (int k = 0; k < ND; ++k) pe_a[k] = po_a[k] = pe_b[k] = po_b[k] = 0;
          const int count = min(64, n - base);
          for (int i = 0; i < count; ++i) {
            const uint32_t packed = cellbuf[r * 64 + i];
            const int col = static_cast<int>(packed & 0xffffu), row = static_cast<int>(packed >> 16);
            if (static_cast<unsigned>(col - c0) < static_cast<unsigned>(c1 - c0) &&
                static_cast<unsigned>(row - r0) < static_cast<unsigned>(r1 - r0)) {
              const int start = col - nl - ox;                       // >= 0
              const int word = (row + dyi - nl - oy) * wd + (start >> 2);
              const int sh = (start & 3) * 8;
              const uint32_t* pa = img + word;
              const uint32_t* pb = pa + plane_dwords;
              uint32_t wa[ND + 1], wb[ND + 1];
#pragma unroll
              for (int k = 0; k <= ND; ++k) { wa[k] = pa[k]; wb[k] = pb[k]; }
#pragma unroll
              for (int k = 0; k < ND; ++k) {
                // bytes start .. start + 3 of the row: neighbouring x offsets, realigned
                const uint32_t va = static_cast<uint32_t>(
                    ((static_cast<uint64_t>(wa[k + 1]) << 32) | wa[k]) >> sh);
                const uint32_t vb = static_cast<uint32_t>(
                    ((static_cast<uint64_t>(wb[k + 1]) << 32) | wb[k]) >> sh);
                pe_a[k] += va & 0x00ff00ffu; po_a[k] += (va >> 8) & 0x00ff00ffu;
                pe_b[k] += vb & 0x00ff00ffu; po_b[k] += (vb >> 8) & 0x00ff00ffu;
              }
            }
          }
          // 64 points of at most 254 each never carry out of a 16-bit field
#pragma unroll
          for (int k = 0; k < ND; ++k) {
            acc_a[4 * k + 0] += pe_a[k] & 0xffffu; acc_a[4 * k + 2] += pe_a[k] >> 16;
            acc_a[4 * k + 1] += po_a[k] & 0xffffu; acc_a[4 * k + 3] += po_a[k] >> 16;
            acc_b[4 * k + 0] += pe_b[k] & 0xffffu; acc_b[4 * k + 2] += pe_b[k] >> 16;
            acc_b[4 * k + 1] += po_b[k] & 0xffffu; acc_b[4 * k + 3] += po_b[k] >> 16;
          }
        }
      }
    }
  }

  float best_lo = 0.f;
  if (active) {
#pragma unroll
    for (int dxi = 0; dxi < 4 * ND; ++dxi) {
      if (dxi < side) {
        const int c = (s * side + dxi) * side + dyi;               // x outer, y inner (:99-113)
        const double e = TsdfDeviceWeight(P, s, dxi - nl, dyi - nl);
        float lo, hi;
        TsdfInterval(acc_a[dxi], acc_b[dxi], n, e, P.slack, &lo, &hi);
        P.lo[c] = lo;
        P.hi[c] = hi;
        best_lo = fmaxf(best_lo, lo);
      }
    }
  }
  unsigned bits = __float_as_uint(best_lo);        // intervals are >= 0
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bits = max(bits, __shfl_xor(bits, off, 64));
  if ((t & 63) == 0 && bits) atomicMax(&P.misc[kCtlBestLo], bits);
}

// grid (ceil(candidates / 256), matches): the candidates the intervals cannot exclude.
__global__ void __launch_bounds__(256) TsdfSelectKernel(const TsdfBatchParams* __restrict__ params) {
  const TsdfBatchParams& P = params[blockIdx.y];
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= P.num_candidates) return;
  const float best_lo = __uint_as_float(P.misc[kCtlBestLo]);
  if (P.hi[c] >= best_lo) {                        // dropped only on hi < best lo
    const unsigned slot = atomicAdd(&P.misc[kCtlSurvivors], 1u);
    P.survivors[slot] = static_cast<unsigned>(c);   // (one slot per candidate: never full)
  }
}

// The reference's score of one candidate: two sequential f32 chains in point order.
__device__ __forceinline__ float TsdfExactScore(const TsdfBatchParams& P, int s, int dx, int dy) {
  const Rt2DFrame F = P.frame;
  const float2 rot = P.scan_rot[s];
  const float* __restrict__ xyz = P.xyz;
  const float min_tsd = -P.max_tsd;
  float sum = 0.f, weight_sum = 0.f;
  for (int i = 0; i < P.n; ++i) {
    int ix, iy;
    Rt2DCellOf(F, rot.x, rot.y, xyz[3 * i], xyz[3 * i + 1], &ix, &iy);
    const int x = ix + dx, y = iy + dy;
    float tsd = min_tsd, weight = 0.f;               // getMinTSD / getMinWeight outside
    if (static_cast<unsigned>(x) < static_cast<unsigned>(P.nx) &&
        static_cast<unsigned>(y) < static_cast<unsigned>(P.ny)) {
      const int flat = P.nx * y + x;
      tsd = BoundedValue(P.tsd[flat], min_tsd, min_tsd, P.max_tsd);
      weight = BoundedValue(P.weight[flat], 0.f, 0.f, P.max_weight);
    }
    const float2 term = TsdfTerm(tsd, weight, P.max_tsd);
    sum += term.x;
    weight_sum += term.y;
  }
  return weight_sum == 0.f ? 0.f : sum / weight_sum;
}

// grid (blocks of 64, matches).  kVerify: every candidate of the search space is evaluated and
// checked against its interval (debug switch rt2d_tsdf_verify); else the survivors.
template <bool kVerify>
__global__ void __launch_bounds__(64) TsdfExactKernel(const TsdfBatchParams* __restrict__ params) {
  const TsdfBatchParams& P = params[blockIdx.y];
  const int k = blockIdx.x * 64 + threadIdx.x;
  const int count = kVerify ? P.num_candidates
                            : static_cast<int>(min(P.misc[kCtlSurvivors],
                                                   static_cast<unsigned>(P.num_candidates)));
  if (k >= count) return;
  const int c = kVerify ? k : static_cast<int>(P.survivors[k]);
  const int side = P.side;
  const int s = c / (side * side);
  const int rem = c - s * side * side;
  const int dxi = rem / side, dyi = rem - dxi * side;
  const float score = TsdfExactScore(P, s, dxi - P.nl, dyi - P.nl);
  const double e = TsdfDeviceWeight(P, s, dxi - P.nl, dyi - P.nl);
  const float w = static_cast<float>(static_cast<double>(score) * e);
  if constexpr (kVerify) {
    if (!(w >= P.lo[c] && w <= P.hi[c])) atomicOr(&P.misc[kCtlError], 1u);
  } else {
    P.surv_score[k] = score;
    P.surv_weighted[k] = w;
    atomicMax(&P.misc[0], __float_as_uint(w));      // scores are >= 0
  }
}

// Survivors within 1e-5 of the best exact weighted score: (index, score bits) pairs, the layout
// the per-candidate path hands to the host (rt_2d.hip, Rt2DCollectKernel).
__global__ void __launch_bounds__(256) TsdfCollectKernel(const TsdfBatchParams* __restrict__ params) {
  const TsdfBatchParams& P = params[blockIdx.y];
  const int k = blockIdx.x * 256 + threadIdx.x;
  const unsigned count = min(P.misc[kCtlSurvivors], static_cast<unsigned>(P.num_candidates));
  if (static_cast<unsigned>(k) >= count) return;
  const float threshold = __uint_as_float(P.misc[0]) * (1.f - 1e-5f);
  if (P.surv_weighted[k] >= threshold) {
    const unsigned slot = atomicAdd(&P.misc[1], 1u);
    if (slot < static_cast<unsigned>(kFinalistCap)) {
      unsigned* pair = slot < static_cast<unsigned>(kFinalistHead)
                           ? P.misc + 2 + 2 * slot
                           : P.overflow + 2 * (slot - kFinalistHead);
      pair[0] = P.survivors[k];
      pair[1] = __float_as_uint(P.surv_score[k]);
    }
  }
}

size_t Align16(size_t v) { return (v + 15) & ~static_cast<size_t>(15); }

// A match's use of its grid's image cache; released (and, after a successful build, published)
// when the call ends.
struct ImageUse {
  Tsdf2DImageCache* cache = nullptr;
  bool reader = false, builder = false;
  unsigned long long version = 0;
  int nx = 0, ny = 0;
};
struct ImageUses {
  std::vector<ImageUse> uses;
  bool built = false;               // the call's stream has been waited for
  ~ImageUses() {
    for (const ImageUse& u : uses) {
      if (!u.cache) continue;
      std::lock_guard<std::mutex> lock(u.cache->mutex);
      if (u.reader) --u.cache->readers;
      if (u.builder) {
        u.cache->building = false;
        if (built) {
          u.cache->valid = true;
          u.cache->version = u.version;
          u.cache->nx = u.nx;
          u.cache->ny = u.ny;
        }
      }
    }
  }
};

void LaunchBulk(int nd, dim3 grid, size_t lds, int device, hipStream_t stream,
                const TsdfBatchParams* d_params) {
  const auto launch = [&](auto kernel) {
    if (lds > 64 * 1024) OptInLds(reinterpret_cast<const void*>(kernel), device, kTsdfLdsBytes);
    kernel<<<grid, kTsdfThreads, lds, stream>>>(d_params);
  };
  switch (nd) {
    case 1: launch(TsdfBulkKernel<1>); break;
    case 2: launch(TsdfBulkKernel<2>); break;
    case 3: launch(TsdfBulkKernel<3>); break;
    default: launch(TsdfBulkKernel<4>); break;
  }
}

}  // namespace

void Rt2DTsdfMatchBatch(const cmx_rt_options* options, const Rt2DItem* items, int num,
                        int32_t device, cmx_match_stats* stats) {
  Rt2DCheckItems(options, items, num);
  CMX_REQUIRE(items[0].tsdf(), "not a TSDF batch");
  CMX_REQUIRE(num <= 65535, "too many matches in one batch");
  UseDevice(device);
  std::vector<Rt2DSearch> search(num);
  ParallelFor(num, Debug().rt2d_host_par > 0 ? Debug().rt2d_host_par : 4096,
              [&](int m) { Rt2DComputeSearch(options, items[m], &search[m]); });
  // Routing, from the measurement in profiles/tsdf_batch_timing.json (128 and 1024 distinct
  // triples, 200 x 200 grids, 13 x 13 x 29 windows, one box; recorded with every second point of
  // the scans, ~480 points -- the ~1000-point legs are unmeasured): the bulk path took 0.73 /
  // 4.16 ms per call, the per-candidate kernels on the same batch 0.46 / 3.32 ms -- it wins at
  // neither size, nor at the margin (3.8 against 3.2 us per further match).  The entries
  // therefore run the per-candidate batch kernels at every size; the bulk path runs under the
  // debug switch rt2d_tsdf_batch_bulk (tests, tools) until it is measured faster.
  bool eligible = Debug().rt2d_tsdf_batch_bulk && !Debug().rt2d_tsdf_batch_legacy;
  for (int m = 0; m < num; ++m) {
    const Rt2DSearch& sr = search[m];
    CMX_REQUIRE(sr.num_scans >= 1 && sr.num_scans < (1 << 16) && sr.nl >= 0 && sr.nl < (1 << 12),
                "unsupported search window");
    const long long side = 2ll * sr.nl + 1;
    CMX_REQUIRE(side * side * sr.num_scans < (1ll << 30), "search window too large");
    const Rt2DItem& it = items[m];
    // The bulk pass takes resident planes, windows of up to kTsdfMaxNl cells and grids whose
    // image coordinates fit 16 bits; anything else runs on the per-candidate kernels.
    eligible = eligible && it.device_cells && it.device_weight_cells && it.tsdf_image_cache &&
               sr.nl <= kTsdfMaxNl && it.limits->num_x_cells <= 32000 &&
               it.limits->num_y_cells <= 32000;
  }
  if (!eligible) {
    Rt2DLegacyBatch(options, items, search.data(), num, device, stats);
    return;
  }

  struct Plan {
    int ipitch, irows, side, num_candidates;
    size_t off_xyz, off_rot;              // in the staging buffer
    size_t off_cand, off_images;          // device scratch
    bool scratch_images;
  };
  std::vector<Plan> plan(num);
  std::vector<TsdfBatchParams> host_params(num);
  ImageUses image_uses;
  image_uses.uses.resize(num);
  std::map<Tsdf2DImageCache*, int> first_use;
  size_t in_bytes = Align16(sizeof(TsdfBatchParams) * num);
  size_t cand_total = 0, image_bytes = 0, lds_bytes = 0;
  unsigned max_groups = 0, max_image_blocks = 0, max_cand_blocks = 0;
  int max_side = 1;
  bool any_build = false;
  for (int m = 0; m < num; ++m) {
    const Rt2DItem& it = items[m];
    const Rt2DSearch& sr = search[m];
    Plan& pl = plan[m];
    TsdfBatchParams& P = host_params[m];
    P = TsdfBatchParams{};
    const int nx = it.limits->num_x_cells, ny = it.limits->num_y_cells, nl = sr.nl;
    pl.side = 2 * nl + 1;
    pl.num_candidates = pl.side * pl.side * sr.num_scans;
    pl.ipitch = (nx + 40 + 3) & ~3;
    pl.irows = ny + 2 * kTsdfImageHalo;
    max_side = std::max(max_side, pl.side);
    P.tsd = it.device_cells;
    P.weight = it.device_weight_cells;
    P.nx = nx; P.ny = ny; P.ipitch = pl.ipitch; P.irows = pl.irows;
    P.frame.res = it.limits->resolution;
    P.frame.inv_res = 1.0 / P.frame.res;
    P.frame.max_x = it.limits->max_x;
    P.frame.max_y = it.limits->max_y;
    P.frame.tx = static_cast<float>(it.initial->x);
    P.frame.ty = static_cast<float>(it.initial->y);
    P.frame.q0w = sr.q0w; P.frame.q0z = sr.q0z;
    P.frame.nx = nx; P.frame.ny = ny; P.frame.nl = nl;
    P.nl = nl; P.side = pl.side; P.num_scans = sr.num_scans; P.num_angular = sr.na; P.n = it.n;
    P.rot_per_group = std::max(1, std::min(kTsdfMaxRotations, kTsdfThreads / pl.side));
    P.groups = DivUp(sr.num_scans, P.rot_per_group);
    // A point's cell is clamped to [-(nl + 1), nx + nl] (Rt2DCellOf): image columns / rows
    P.c_begin = kTsdfImageHalo - (nl + 1); P.c_end = nx + nl + kTsdfImageHalo + 1;
    P.r_begin = kTsdfImageHalo - (nl + 1); P.r_end = ny + nl + kTsdfImageHalo + 1;
    const int full_w = P.c_end - P.c_begin, full_h = P.r_end - P.r_begin;
    const int image_budget = kTsdfLdsBytes - P.rot_per_group * 64 * 4;
    P.core_w = std::min(full_w, kTsdfMaxCoreW);
    P.tile_w = ((P.core_w + 2) & ~3) + 20;          // realigned start, window, one dword of over-read
    P.core_h = std::min(full_h, image_budget / (2 * P.tile_w) - 2 * nl);
    P.tile_h = P.core_h + 2 * nl;
    P.tiles_x = DivUp(full_w, P.core_w);
    P.tiles_y = DivUp(full_h, P.core_h);
    lds_bytes = std::max<size_t>(lds_bytes, static_cast<size_t>(P.rot_per_group) * 64 * 4 +
                                                2 * static_cast<size_t>(P.tile_w) * P.tile_h);
    P.step = sr.step;
    P.wt = options->translation_delta_cost_weight;
    P.wr = options->rotation_delta_cost_weight;
    P.max_tsd = it.max_tsd; P.max_weight = it.max_weight;
    P.slack = TsdfSlack(it.n);
    P.num_candidates = pl.num_candidates;

    // The grid's images: the cache's when they are current, built into the cache when it is
    // stale and idle, else built into scratch of this call.
    const size_t bytes = 2 * static_cast<size_t>(pl.ipitch) * pl.irows;
    pl.scratch_images = false;
    Tsdf2DImageCache* cache = it.tsdf_image_cache;
    const auto seen = first_use.find(cache);
    if (seen != first_use.end()) {                  // the same grid again: its first item's images
      P.images = host_params[seen->second].images;
      P.build = 0;
      pl.scratch_images = plan[seen->second].scratch_images;
      pl.off_images = plan[seen->second].off_images;
    } else {
      first_use[cache] = m;
      ImageUse& use = image_uses.uses[m];
      std::lock_guard<std::mutex> lock(cache->mutex);
      if (cache->valid && cache->version == it.grid_version && cache->nx == nx && cache->ny == ny) {
        ++cache->readers;
        use.cache = cache; use.reader = true;
        P.images = cache->images;
      } else if (!cache->building && cache->readers == 0) {
        if (cache->capacity < bytes) {
          if (cache->images) CMX_HIP(hipFree(cache->images));
          cache->images = nullptr; cache->capacity = 0; cache->valid = false;
          CMX_HIP(hipMalloc(reinterpret_cast<void**>(&cache->images), bytes));
          cache->capacity = bytes;
        }
        cache->valid = false;
        cache->building = true;
        use.cache = cache; use.builder = true;
        use.version = it.grid_version; use.nx = nx; use.ny = ny;
        P.images = cache->images;
        P.build = 1;
      } else {
        pl.scratch_images = true;
        pl.off_images = image_bytes;
        image_bytes = (image_bytes + bytes + 255) & ~static_cast<size_t>(255);
        P.build = 1;
      }
      if (P.build) {
        any_build = true;
        max_image_blocks = std::max<unsigned>(max_image_blocks, DivUp(pl.ipitch * pl.irows, 256));
      }
    }

    pl.off_xyz = in_bytes;
    pl.off_rot = pl.off_xyz + (it.device_xyz ? 0 : Align16(3 * sizeof(float) * it.n));
    in_bytes = pl.off_rot + Align16(sizeof(float2) * sr.num_scans);
    pl.off_cand = cand_total;
    cand_total += static_cast<size_t>(pl.num_candidates);
    max_groups = std::max<unsigned>(max_groups, P.groups);
    max_cand_blocks = std::max<unsigned>(max_cand_blocks, DivUp(pl.num_candidates, 256));
  }
  const size_t off_misc = in_bytes;
  in_bytes += Align16(sizeof(unsigned) * 128 * static_cast<size_t>(num));

  WorkspaceLease ws(device);
  char* h_in = ws->pinned[0].ReserveAs<char>(in_bytes);
  char* d_in = ws->dev[0].ReserveAs<char>(in_bytes);
  float* d_lo = ws->dev[1].ReserveAs<float>(cand_total);
  float* d_hi = ws->dev[2].ReserveAs<float>(cand_total);
  unsigned* d_survivors = ws->dev[3].ReserveAs<unsigned>(cand_total);
  float* d_surv_score = ws->dev[4].ReserveAs<float>(cand_total);
  float* d_surv_weighted = ws->dev[5].ReserveAs<float>(cand_total);
  unsigned* d_overflow = ws->dev[6].ReserveAs<unsigned>(static_cast<size_t>(num) * 2 *
                                                        (kFinalistCap - kFinalistHead));
  uint8_t* d_images = image_bytes ? ws->dev[7].ReserveAs<uint8_t>(image_bytes) : nullptr;
  unsigned* h_misc = ws->pinned[1].ReserveAs<unsigned>(static_cast<size_t>(num) * 128);
  unsigned* d_misc = reinterpret_cast<unsigned*>(d_in + off_misc);
  static_assert(2 + 2 * kFinalistHead <= kCtlBestLo, "the control words follow the finalist head");
  std::memset(h_in + off_misc, 0, sizeof(unsigned) * 128 * static_cast<size_t>(num));

  ParallelFor(num, 8, [&](int m) {
    const Rt2DItem& it = items[m];
    const Plan& pl = plan[m];
    const Rt2DSearch& sr = search[m];
    TsdfBatchParams& P = host_params[m];
    if (!it.device_xyz) std::memcpy(h_in + pl.off_xyz, it.xyz, 3 * sizeof(float) * it.n);
    FillRotationTable(sr.step, sr.na, reinterpret_cast<float2*>(h_in + pl.off_rot));
    if (pl.scratch_images) P.images = d_images + pl.off_images;
    P.scan_rot = reinterpret_cast<const float2*>(d_in + pl.off_rot);
    P.xyz = it.device_xyz ? it.device_xyz : reinterpret_cast<const float*>(d_in + pl.off_xyz);
    P.lo = d_lo + pl.off_cand;
    P.hi = d_hi + pl.off_cand;
    P.misc = d_misc + static_cast<size_t>(m) * 128;
    P.overflow = d_overflow + static_cast<size_t>(m) * 2 * (kFinalistCap - kFinalistHead);
    P.survivors = d_survivors + pl.off_cand;
    P.surv_score = d_surv_score + pl.off_cand;
    P.surv_weighted = d_surv_weighted + pl.off_cand;
  });
  std::memcpy(h_in, host_params.data(), sizeof(TsdfBatchParams) * num);
  SmallCopyAsync(d_in, h_in, in_bytes, /*to_device=*/true, ws->stream);
  const TsdfBatchParams* d_params = reinterpret_cast<const TsdfBatchParams*>(d_in);

  const bool verify = Debug().rt2d_tsdf_verify != 0;
  RecordEvent(ws->ev_begin, ws->stream);
  if (any_build)
    Tsdf2DImageKernel<<<dim3(max_image_blocks, 1, num), 256, 0, ws->stream>>>(d_params);
  RecordEvent(ws->ev_k0, ws->stream);
  LaunchBulk((max_side + 3) / 4, dim3(max_groups, num), lds_bytes, device, ws->stream, d_params);
  RecordEvent(ws->ev_k1, ws->stream);
  TsdfSelectKernel<<<dim3(max_cand_blocks, num), 256, 0, ws->stream>>>(d_params);
  TsdfExactKernel<false><<<dim3(max_cand_blocks * 4, num), 64, 0, ws->stream>>>(d_params);
  TsdfCollectKernel<<<dim3(max_cand_blocks, num), 256, 0, ws->stream>>>(d_params);
  if (verify)
    TsdfExactKernel<true><<<dim3(max_cand_blocks * 4, num), 64, 0, ws->stream>>>(d_params);
  CMX_HIP(hipGetLastError());
  RecordEvent(ws->ev_end, ws->stream);
  SmallCopyAsync(h_misc, d_misc, sizeof(unsigned) * 128 * num, /*to_device=*/false, ws->stream);
  CMX_HIP(hipStreamSynchronize(ws->stream));
  image_uses.built = true;

  cmx_match_stats total{};
  std::vector<std::pair<int, float>> finalists;
  std::vector<unsigned> extra;
  std::vector<int> redo;
  for (int m = 0; m < num; ++m) {
    const Plan& pl = plan[m];
    const unsigned* head = h_misc + static_cast<size_t>(m) * 128;
    CMX_REQUIRE(!(verify && head[kCtlError]),
                "internal error: a TSDF candidate's exact score lies outside its interval "
                "(rt2d_tsdf_verify)");
    const long long survivors = head[kCtlSurvivors], count = head[1];
    if (count > kFinalistCap) {                      // flat landscape: repeated below
      redo.push_back(m);
      continue;
    }
    CMX_REQUIRE(count >= 1, "internal error: no candidate collected");
    finalists.resize(count);
    const long long in_head = std::min<long long>(count, kFinalistHead);
    if (count > kFinalistHead) {
      extra.resize(2 * (count - kFinalistHead));
      CMX_HIP(hipMemcpyAsync(extra.data(),
                             d_overflow + static_cast<size_t>(m) * 2 * (kFinalistCap - kFinalistHead),
                             sizeof(unsigned) * extra.size(), hipMemcpyDeviceToHost, ws->stream));
      CMX_HIP(hipStreamSynchronize(ws->stream));
    }
    for (long long i = 0; i < count; ++i) {
      const unsigned* pair = i < in_head ? head + 2 + 2 * i : extra.data() + 2 * (i - in_head);
      float v;
      std::memcpy(&v, &pair[1], sizeof(float));
      finalists[i] = {static_cast<int>(pair[0]), v};
    }
    std::sort(finalists.begin(), finalists.end());
    Rt2DFinishOnHost(options, items[m], search[m], finalists.data(), finalists.size());
    total.candidates_scored += pl.num_candidates;
    total.coarse_candidates += pl.num_candidates;
    total.num_scans += search[m].num_scans;
    total.refined_candidates += survivors;
    total.finalists += count;
  }
  total.device_ms = ElapsedMs(ws->ev_begin, ws->ev_end);
  total.dominant_kernel_ms = ElapsedMs(ws->ev_k0, ws->ev_k1);
  if (!redo.empty()) {
    std::vector<Rt2DItem> again_items;
    std::vector<Rt2DSearch> again_search;
    for (int m : redo) {
      again_items.push_back(items[m]);
      again_search.push_back(search[m]);
    }
    cmx_match_stats again{};
    Rt2DLegacyBatch(options, again_items.data(), again_search.data(),
                    static_cast<int>(redo.size()), device, &again);
    total.candidates_scored += again.candidates_scored;
    total.coarse_candidates += again.coarse_candidates;
    total.num_scans += again.num_scans;
    total.refined_candidates += again.refined_candidates;
    total.finalists += again.finalists;
  }
  if (stats) *stats = total;
}

}  // namespace cmx
