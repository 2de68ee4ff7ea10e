// Device-visible types of the real-time 3D matcher that kernels of more than one translation
// unit take, the device helpers those kernels share, the constants host and device both read,
// and the layouts of the misc blocks the kernels receive pointers into.
//
// The types stay in the unnamed namespace the kernels live in, as in fast_3d_device.h: the
// kernels' symbols spell their parameter types, and bench.py and the profiling tools name kernels
// by these symbols.  Every unit that includes this header therefore has its own, identical copy.
#ifndef CMX_RT_3D_DEVICE_H_
#define CMX_RT_3D_DEVICE_H_

#include <cstddef>

#include "scan_matching_3d.h"

namespace cmx {
namespace {

// Dense f32 probability brick with a one-cell border of kMinProbability: a voxel
// index clamped to the border reads what HybridGrid::GetProbability returns for any
// cell outside the stored box (value 0 -> kMinProbability, hybrid_grid.h:521-523).
struct PaddedBrick {
  const float* cells;   // [(nz+2)][(ny+2)][(nx+2)]
  int lo_x, lo_y, lo_z; // index of padded cell (1,1,1)
  int nx, ny, nz;
};

struct Rt3DParams {
  PaddedBrick grid;
  float resolution, inv_resolution;
  int num_translations, num_rotations, side_t, side_r;
  const float4* rotation;     // [R] candidate rotation (x,y,z,w) = normalized(init.q * q_r)
  const float4* translation;  // [T] candidate translation (xyz) = init.q * t_c + init.t; w = |t_c|
  const float* rotation_angle;  // [R] GetAngle(transform)
  double wt, wr;
};

// lround(c / resolution) (HybridGrid::GetCellIndex, hybrid_grid.h:428-433) without the
// IEEE division in the common case.  q0 = c * RN(1/res) differs from the correctly
// rounded quotient qe by less than |q0| * 2^-21; when q0 is further than |q0| * 2^-20
// from every half-integer, qe lies strictly inside (n - 0.5, n + 0.5) with n = rint(q0),
// so lround(qe) == n.  Otherwise (about |q0| * 2^-19 of the inputs, NaN/inf included)
// `ok` is cleared and the caller recomputes with the reference's exact expression.
__device__ __forceinline__ int FastCellIndex(float c, float inv_resolution, bool* ok) {
  const float q0 = c * inv_resolution;
  const float n = rintf(q0);
  const float margin = 0.5f - fabsf(q0 - n);          // exact
  *ok = *ok && (margin > fabsf(q0) * 0x1p-20f);
  return static_cast<int>(n);
}

// The bounds search (rt_3d_bounds.hip has the derivation): launch shapes of the gather kernels.
constexpr int kBulk3DThreads = 256;
constexpr int kCand3DThreads = 128;         // candidate pass: work lists are short (a block's idle
                                            // wavefronts only hold wave slots)
constexpr int kBulk3DChunk = 256;          // points staged per round (one per thread)
constexpr int kAmbiguousQuad = 4 * 255;    // what one flagged group of four lookups can move Q by

typedef float v2f __attribute__((ext_vector_type(2)));

struct Rt3DBulkParams {
  const uint8_t* cells;          // [(nz+2p)][(ny+2p)][(nx+2p)] q = u >> 7 (or its dilation)
  unsigned cell_count;
  float pitch_x, pitch_y;        // nx + 2p, ny + 2p as floats (index arithmetic stays < 2^24)
  int tiles_y, pitch_z;          // candidate brick: columns of 8 x 4 cells, see TiledOffset
  float off_x, off_y, off_z;     // pad - lo
  float inv_resolution;
  float guard;                   // a lookup is unambiguous when max |q - rint(q)| <= guard
  float t0x, t0y, t0z;           // init.t: rp + init.t is what gets clamped
  float lo_x, hi_x, lo_y, hi_y, lo_z, hi_z;   // clamp range in metres
  int num_translations;          // entries of `translation` (T, or the number of groups)
  int num_rotations, n;
  const float4* rotation;        // as Rt3DParams
  const float4* translation;     // xyz + distance entering the weight (group: its smallest)
  const float* rotation_angle;
  // Group pass: every translation of rotation blockIdx.y.  Candidate pass: block blockIdx.x
  // takes work descriptor (r, chunk) = blocks[blockIdx.x]: items[r][256 chunk ..] of the
  // counts[r] listed translations.
  const int* counts;
  const int* items;              // [R][num_translations]
  const int2* blocks;
  double wt, wr;
  double min_probability;        // the f32 constants of the value table, widened
  double scale_over_n;           // 128 kScale / N
  double slack_hi;               // 127 kScale + 2e-7 (quantisation + rounding of the table)
  double delta;                  // relative slack of the f32 chain + exp
  float* upper;                  // [R][num_translations] weighted upper bound
  int block_items;               // candidate pass: items per work descriptor (= blockDim.x)
  int list_rotations;            // candidate pass: consecutive rotations sharing one work list;
                                 // an entry is w * num_translations + t (w: rotation in the list)
  uint2* sums;                   // candidate pass: [R][T] (Q, A) accumulated over point slices
  int slice_points;              // points per blockIdx.z (a multiple of the chunk)
  unsigned* max_lower_bits;      // atomicMax of the weighted lower bounds (candidate pass)
  unsigned* max_upper_bits;      // atomicMax of the weighted upper bounds (group pass)
};

__device__ __forceinline__ float ClampStage(float rp, float t0, float lo, float hi) {
  const float b = rp + t0;
  if (b < lo) return lo - t0;
  if (b > hi) return hi - t0;
  return rp;
}

// The candidate pass reads few, scattered translations per rotation: its brick is stored as
// columns of 8 (x) by 4 (y) cells running along z, so that a 128-byte line holds an 8 x 4 x 4
// block of cells -- the eight members of a group of translations (3 x 3 x 3 cells at most)
// touch one or two lines instead of up to nine rows.
//   offset = ((x >> 3) * tiles_y + (y >> 2)) * pitch_z * 32 + z * 32 + (y & 3) * 8 + (x & 7)
// (pitch_z is a multiple of 4, so lines never straddle columns.)
__host__ __device__ __forceinline__ unsigned TiledOffset(unsigned x, unsigned y, unsigned z,
                                                         unsigned tiles_y, unsigned pitch_z) {
  const unsigned column = (x >> 3) * tiles_y + (y >> 2);
  return ((column * pitch_z + z) << 5) | ((y & 3u) << 3) | (x & 7u);
}

// Weighted bounds of the f32 score from the integer sum `acc` and `ambiguous` flagged groups
// of four lookups; rounded outwards: a float strictly below / above the f64 bound.
__device__ __forceinline__ void Bounds3D(const Rt3DBulkParams& P, unsigned acc,
                                         unsigned ambiguous, float distance, int r, float* lower,
                                         float* upper) {
  const double spread = static_cast<double>(ambiguous) * kAmbiguousQuad;
  const double q_lo = fmax(static_cast<double>(acc) - spread, 0.);
  const double q_hi = static_cast<double>(acc) + spread;
  const double mean_lo = P.min_probability + P.scale_over_n * q_lo - 2e-7;
  const double mean_hi = P.min_probability + P.scale_over_n * q_hi + P.slack_hi;
  const double penalty = static_cast<double>(distance) * P.wt +
                         static_cast<double>(P.rotation_angle[r]) * P.wr;
  const double w = exp(-(penalty * penalty));
  *lower = static_cast<float>(mean_lo * w * (1. - P.delta)) * (1.f - 0x1p-22f);
  *upper = static_cast<float>(mean_hi * w * (1. + P.delta)) * (1.f + 0x1p-22f);
}

// The LDS-tiled passes (rt_3d_tiles.hip): what a tile kernel takes next to Rt3DBulkParams.
constexpr int kTileMaxRotations = 8;       // most rotations a workgroup stages

struct Rt3DTileParams {
  const float* sorted_xyz;       // bin-sorted cloud
  const int2* chunks;            // (first point, length)
  const int* num_chunks;
  int pitch_x, pitch_y, pitch_z; // brick dims (pitch_x a multiple of 4)
  float tr_lo[3], tr_hi[3];      // span of translation * inv_resolution over the table
  int rotations_per_block;       // group pass: rotations of a workgroup
  int tile_capacity;             // bytes of dynamic LDS behind the staged points
  int block_items;               // candidate pass: items per work descriptor (= blockDim.x)
  int fixed_point;               // group pass: packed fixed-point cell arithmetic (see kernel)
  const float* boxes;            // Rt3DChunkBoxKernel: [rotation block][chunk][6], or null (boxes
                                 // are then reduced inside the tile kernel)
  // Point segments (Rt3DBinScanKernel): seg_bounds[0], [1] = first chunk of segments 1 and 2 of
  // this pass's list, or null (one segment: every chunk).  The pass takes the chunks of segments
  // seg_first .. seg_last.  Group pass: seg_sums[(r, group)] = (sum over segment 0, sum over
  // segment 1) next to the total in P.sums, or null.
  const int* seg_bounds;
  int seg_first, seg_last;
  uint2* seg_sums;
  unsigned long long* stats;     // debug switch rt3d_report (its atomics cost ~0.5 ms per pass: not for timing): [0] chunks in LDS, [1] on the gather path,
                                 // [2] tile bytes, [3] points (per workgroup and chunk); or null
};

// The misc blocks: one struct each for the device block and its pinned copy.  The kernels
// receive pointers to single fields, so the layouts are pinned down below.
constexpr int kFinalistCap = 4096;
struct Rt3DExhaustiveMisc {               // Rt3DScoreKernel, Rt3DCollectKernel
  unsigned max_bits;                      // atomicMax of the weighted scores
  int count;                              // candidates collected (may exceed the capacity)
  int reserved[2];
  long long finalists[kFinalistCap];      // candidate index t * R + r
};
constexpr size_t kExhaustiveHeadBytes = offsetof(Rt3DExhaustiveMisc, finalists);   // zeroed per call
static_assert(offsetof(Rt3DExhaustiveMisc, count) == 4 && kExhaustiveHeadBytes == 16 &&
                  sizeof(Rt3DExhaustiveMisc) == 16 + sizeof(long long) * kFinalistCap,
              "layout of the exhaustive search's misc block");

constexpr int kBulkFinalistCap = 4096;
struct Rt3DBulkHead {                     // head of the bounds search's misc block
  unsigned max_lower;                     // bits of the best weighted lower bound (candidates)
  int count;                              // finalists collected (may exceed the capacity)
  unsigned max_upper;                     // bits of the best weighted upper bound (groups)
  int total;                              // candidates that went through the candidate passes
  int finalists[kBulkFinalistCap];        // r * T + t
  float exact[kBulkFinalistCap];          // their exact unweighted scores
};
constexpr size_t kBulkHeadZeroed = offsetof(Rt3DBulkHead, finalists);              // zeroed per call
static_assert(offsetof(Rt3DBulkHead, count) == 4 && offsetof(Rt3DBulkHead, max_upper) == 8 &&
                  offsetof(Rt3DBulkHead, total) == 12 && kBulkHeadZeroed == 16 &&
                  offsetof(Rt3DBulkHead, exact) == 16 + sizeof(int) * kBulkFinalistCap &&
                  sizeof(Rt3DBulkHead) == 16 + (sizeof(int) + sizeof(float)) * kBulkFinalistCap,
              "layout of the bounds search's misc head");

struct Rt3DCounters {                     // behind the work blocks (two int2 slots)
  int num_blocks;                         // work blocks of the list being compacted
  int violations;                         // rt3d_verify: bounds that do not hold
  int stage_total;                        // items of the staged re-compactions (kept apart from
                                          // Rt3DBulkHead::total, which counts every item once)
  int pair_total;                         // (rotation, group) pairs the pair rounds computed
};
static_assert(sizeof(Rt3DCounters) == 2 * sizeof(int2) && offsetof(Rt3DCounters, violations) == 4 &&
                  offsetof(Rt3DCounters, stage_total) == 8 && offsetof(Rt3DCounters, pair_total) == 12,
              "layout of the bounds search's counters");

// Chunk counts Rt3DBinScanKernel leaves behind the bins (eight ints).
enum Rt3DSegmentCount {
  kGroupChunks = 0, kCandidateChunks = 1,   // chunks of either list
  kGroupSegments = 2,                       // [2..3]: first chunk of segments 1 and 2, group list
  kCandidateSegments = 4,                   // [4..5]: ... candidate list
  kNumSegmentCounts = 8,
};
struct Rt3DReadBack {                     // pinned: what the host sizes its launches by
  int num_blocks;
  int segments[kNumSegmentCounts];
  int pair_total;
};
// One pinned reservation: the two searches of a call read back into regions of their own.
struct Rt3DPinnedReadBack {
  Rt3DExhaustiveMisc exhaustive;
  Rt3DReadBack bounds;
};

}  // namespace
}  // namespace cmx

#endif  // CMX_RT_3D_DEVICE_H_
