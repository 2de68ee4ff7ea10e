// Device-visible types of the fast 3D matcher that more than one translation unit uses, and the
// few device helpers kernels of more than one unit call (the front end, fast_3d_coarse.hip, writes
// the cells and scores the branch and bound, fast_3d.hip, reads).
//
// The types stay in the unnamed namespace the kernels live in: the kernels' symbols spell their
// parameter types, and bench.py and the profiling tools name kernels by these symbols.  Every
// unit that includes this header therefore has its own, identical copy of them.
#ifndef CMX_FAST_3D_DEVICE_H_
#define CMX_FAST_3D_DEVICE_H_

#include "scan_matching_3d.h"

namespace cmx {
namespace {

constexpr int kSubLists3 = 64;
// (Padding the sub-list counters to a cache line each, which took the 2D coarse filter from 323
// to 30 us, measured nothing here -- a node's list reservation is once per block -- and cost
// 40 us per single search in the larger counter copies.)
constexpr int kCountStride3 = 1;
constexpr int kSeeds3 = 64;

struct Node3D {
  int level;               // depth of this node (0 = leaf)
  int scan;
  int ox, oy, oz;          // Candidate3D::offset
  float score;
  float coarse_score;      // score of the lowest-resolution ancestor
  int coarse_index;        // its generation index
  unsigned long long path; // sibling ranks along the descent, 3 bits per level
  float low_resolution_score;
  int problem;             // index into the batch's Fast3DProblem array
  int family;              // > 0: this node and the next family - 1 slots of its sub-list are the
                           // children one parent kept (same problem, scan and level, offsets
                           // half a parent step apart); 0: a later member of such a run
  int pad;
};

struct Counters3 {
  int frontier[kMaxDepth + 2][kSubLists3 * kCountStride3];
  int dive[2][kSubLists3];
  int leaves[kSubLists3 * kCountStride3];
  int overflow;
  int pad0;
  int pad1;
  int pad;
  unsigned long long scored[16];
  unsigned long long expanded[16];
};

struct List3 {
  Node3D* nodes;
  int* counts;
  int sub_capacity;
};

// The eight cells the children of a node read for one point, in ONE 8-byte word (what quads
// are to the 2D search): oct(X, Y, Z) byte k = level(x + (k & 1) s, y + (k >> 1 & 1) s,
// z + (k >> 2) s) with (x, y, z) = (X, Y, Z) - s relative to the level's brick, cells outside
// the brick 0; s = the level's child stride 2^min(level, full_resolution_depth - 1).  One
// gather per point and node instead of four (eight in round 1); 8x the bytes of the level
// itself, i.e. ~90 MB per 150^3 submap instead of 12 -- HBM is not the scarce resource.
struct OctDesc {
  const uint2* cells;      // [(nz + s)][(ny + s)][(nx + s)]; null: not built
  int qx, qy, qz, s;
};

// Bytes of a level's oct array (the buffer resource's range); 0 = not addressable by one
// (>= 2 GB: a level of more than ~640^3 cells keeps plain loads).
__device__ __forceinline__ unsigned long long OctBytes(const OctDesc& O) {
  const unsigned long long bytes =
      static_cast<unsigned long long>(O.qx) * O.qy * static_cast<unsigned long long>(O.qz) * 8ull;
  return bytes < kMaxBufferBytes ? bytes : 0ull;
}

struct Fast3DProblem {
  Brick level[kMaxDepth];
  OctDesc oct[kMaxDepth];
  int depth, full_resolution_depth;
  Brick low;
  float low_resolution, resolution;
  int wxy, wz;
  int num_scans, n, n_low;
  const int4* cells;        // [num_scans][n] full-resolution cell indices
  const float* low_xyz;     // low-resolution cloud
  const float4* scan_q;     // [num_scans] rotation of GetPoseFromCandidate (x,y,z,w)
  float pose_tx, pose_ty, pose_tz;
  float min_score;
  double min_low_resolution_score;
  int ncx, ncy, ncz;        // lowest-resolution candidates per scan and axis
  float* coarse_score;      // [num_scans * ncx*ncy*ncz]
  // Per-problem search state (a batch of searches shares the frontier and leaf lists; nodes
  // carry their problem's index).
  unsigned* best_bits;      // float bits of the best verified leaf (>= min_score floor)
  Node3D* seeds;            // [kSeeds3] dive seeds
  int* seed_count;
  int index;                // this problem's index in the batch
};

// One rotated scan of a batch whose pairs bring their own nodes: where its node's cloud lies and
// where its cells go (its problem's `cells` + scan * n).
struct Scan3D {
  const float* xyz;
  int4* cells;
  int n, pad;
};

// What SelectBest3DKernel leaves per problem.
struct Best3 {
  float score;
  int scan, ox, oy, oz;
  float low_resolution_score;
  int found, ties;
};

__device__ __forceinline__ float ToProbability(int sum, int n) {
  // PrecomputationGrid3D::ToProbability(sum / float(N))  (:347-350)
  const float kMinP = 0.1f;
  const float kMaxP = 1.f - kMinP;
  return kMinP + (static_cast<float>(sum) / static_cast<float>(n)) * ((kMaxP - kMinP) / 255.f);
}

// Cell index of point `c` at `depth` (DiscretizeScan's low-resolution
// indices, :223-241) — e = max(0, depth - full_resolution_depth + 1).
__device__ __forceinline__ int3 DepthIndex(const int4& c, int e, int sx, int sy, int sz) {
  if (e == 0) return make_int3(c.x, c.y, c.z);
  return make_int3(((c.x + sx) >> e) - (sx >> e), ((c.y + sy) >> e) - (sy >> e),
                   ((c.z + sz) >> e) - (sz >> e));
}

// The same without the branch on e (for e == 0 the shifts are no-ops and the expression is c):
// a branch inside an unrolled gather loop is a basic-block boundary the loads cannot cross.
__device__ __forceinline__ int3 DepthIndexAny(int cx, int cy, int cz, int e, int sx, int sy,
                                              int sz) {
  return make_int3(((cx + sx) >> e) - (sx >> e), ((cy + sy) >> e) - (sy >> e),
                   ((cz + sz) >> e) - (sz >> e));
}

}  // namespace
}  // namespace cmx

#endif  // CMX_FAST_3D_DEVICE_H_
