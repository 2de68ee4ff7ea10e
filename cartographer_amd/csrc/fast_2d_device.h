// Device helpers of the fast 2D matcher that kernels of more than one translation unit use: the
// score conversions (the front end, fast_2d_coarse.hip, writes scores the tree search --
// fast_2d_seed.hip, fast_2d_levels.hip, fast_2d_queue.hip, fast_2d.hip -- prunes with) and the
// re-derivation of a scan's cells from the point cloud (bit-identical to what the front end
// scored).  What only the tree search's kernels share: fast_2d_search_device.h.
#ifndef CMX_FAST_2D_DEVICE_H_
#define CMX_FAST_2D_DEVICE_H_

#include "scan_matching_2d.h"

namespace cmx {

__device__ __forceinline__ float ToScore(const Fast2DProblem& P, int sum, int n) {
  // ToScore(sum / float(N))  (SM2/fast_...2d.cc:330-331, .h:74-76)
  return P.min_s + (static_cast<float>(sum) / static_cast<float>(n)) * P.score_scale;
}

// An integer >= the sum a node's score was computed from (inverse of ToScore,
// rounded generously upwards; only used to prune).
__device__ __forceinline__ int SumUpperBound(const Fast2DProblem& P, float score, int n) {
  const float s = (score - P.min_s) / P.score_scale * static_cast<float>(n);
  const float ub = ceilf(s * (1.f + 1e-5f)) + 2.f;
  return static_cast<int>(fminf(fmaxf(ub, 0.f), 255.f * static_cast<float>(n)));
}

// Cell of point i of rotated scan `rot` = P.scan_rot[scan], packed (x | y << 16): the fused
// front end's arithmetic (RotateZ twice, translation, CellIndexFast), so bit-identical to what
// it scored -- and to PrepScansKernel's `discrete` array.
__device__ __forceinline__ uint32_t ScanCell(const Fast2DProblem& P, float2 rot, int i) {
  const float* __restrict__ xyz = P.xyz;
  const float px = xyz[3 * i], py = xyz[3 * i + 1];
  float ax = px, ay = py;
  if (!(P.init_qw == 1.f && P.init_qz == 0.f)) RotateZ(P.init_qw, P.init_qz, px, py, &ax, &ay);
  float bx, by;
  RotateZ(rot.x, rot.y, ax, ay, &bx, &by);
  const float x = bx + P.tx;
  const float y = by + P.ty;
  const int ix = CellIndexFast(P.max_y, y, P.res, P.inv_res);
  const int iy = CellIndexFast(P.max_x, x, P.res, P.inv_res);
  return (static_cast<uint32_t>(ix) & 0xffffu) | (static_cast<uint32_t>(iy) << 16);
}

}  // namespace cmx

#endif  // CMX_FAST_2D_DEVICE_H_
