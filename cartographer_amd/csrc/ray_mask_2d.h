// RayToPixelMask (mapping/internal/2d/ray_to_pixel_mask.cc:34-156) for one wavefront, shared by
// the range-data inserters of the probability grid (grid_2d.hip) and of the TSDF (tsdf_2d.hip).
#ifndef CMX_RAY_MASK_2D_H_
#define CMX_RAY_MASK_2D_H_

#include <hip/hip_runtime.h>

namespace cmx {

constexpr int kSubpixelScale = 1000;                     // ..._inserter_2d.cc:33 / :27

__device__ __forceinline__ long long FloorDiv(long long a, long long b) {
  return a >= 0 ? a / b : -((-a + b - 1) / b);
}
__device__ __forceinline__ long long CeilDiv(long long a, long long b) { return -FloorDiv(-a, b); }

// Calls visit(x, y) for every pixel of the ray from superscaled cell `begin` to `end`, column by
// column over the 64 lanes: the ray enters pixel column `col` at height y_in and leaves it at
// y_out (exact integers in half-sub-pixel units scaled by dx); the column contributes the pixels
// between them, a corner touched exactly adding none.  Every pixel is visited once.
template <typename Visit>
__device__ __forceinline__ void ForEachRayPixel(int2 begin, int2 end, int lane, Visit&& visit) {
  if (begin.x > end.x) { const int2 t = begin; begin = end; end = t; }
  const int scale = kSubpixelScale;
  const int col0 = begin.x / scale, col1 = end.x / scale;
  if (col0 == col1) {                                    // stays inside one pixel column
    const int lo = min(begin.y, end.y) / scale, hi = max(begin.y, end.y) / scale;
    for (int y = lo + lane; y <= hi; y += 64) visit(col0, y);
    return;
  }
  const long long dx = static_cast<long long>(end.x) - begin.x;
  const long long dy = static_cast<long long>(end.y) - begin.y;
  const long long x2_begin = 2ll * begin.x + 1, x2_end = 2ll * end.x + 1;
  const long long y2_begin = 2ll * begin.y + 1;
  const long long pixel = 2ll * scale * dx;
  for (int col = col0 + lane; col <= col1; col += 64) {
    const long long left = max(2ll * scale * col, x2_begin);
    const long long right = min(2ll * scale * (col + 1), x2_end);
    const long long y_in = y2_begin * dx + (left - x2_begin) * dy;
    const long long y_out = y2_begin * dx + (right - x2_begin) * dy;
    long long first, last;
    if (dy > 0) {
      first = FloorDiv(y_in, pixel);
      last = CeilDiv(y_out, pixel) - 1;
    } else {
      last = CeilDiv(y_in, pixel) - 1;
      first = FloorDiv(y_out, pixel);
    }
    for (long long y = first; y <= last; ++y) visit(col, static_cast<int>(y));
  }
}

}  // namespace cmx

#endif  // CMX_RAY_MASK_2D_H_
