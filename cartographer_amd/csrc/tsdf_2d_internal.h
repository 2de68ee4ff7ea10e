// What the two translation units of the resident TSDF2D share: tsdf_2d.hip (the grid, the single
// insertion, crop, the matcher entries) and tsdf_2d_batch.hip (cmx_tsdf2d_insert_batch).  The
// host preparation both insertions go through is tsdf_2d_host.h (plain C++17).
#ifndef CMX_TSDF_2D_INTERNAL_H_
#define CMX_TSDF_2D_INTERNAL_H_

#include <cmath>

#include "ray_mask_2d.h"
#include "scan_matching_2d.h"
#include "tsdf_2d_host.h"

struct cmx_tsdf2d {
  int device = 0;
  double resolution = 0., max_x = 0., max_y = 0.;
  int nx = 0, ny = 0;
  float max_tsd = 0.f, max_weight = 0.f;                 // the grid's TSDValueConverter
  uint16_t* tsd = nullptr;                               // device, nx * ny
  uint16_t* weight = nullptr;                            // device, nx * ny
  int32_t* owner = nullptr;                              // device, nx * ny; kNoOwner between calls
  unsigned long long version = 1;                        // bumped whenever the planes change
  mutable cmx::Tsdf2DImageCache rt_image;                // byte images of the batched matcher
};

namespace cmx {
// (Internal linkage in either unit: the kernels of the single insertion keep their symbols.)
namespace {

static_assert(tsdf2d::kSubpixels == kSubpixelScale, "host and device superscale alike");

constexpr uint16_t kUpdateMarker = 1u << 15;
constexpr int kNoOwner = 0x7f7f7f7f;                     // hipMemset(0x7f): above any hit index

// ---- device ----------------------------------------------------------------------
struct TsdfParams {
  uint16_t* tsd;
  uint16_t* weight;
  int* owner;
  int nx, ny;
  double resolution, max_x, max_y;
  float origin_x, origin_y;
  float truncation;                // the inserter's truncation_distance (f32, :133-134)
  float maximum_weight;            // the inserter's maximum_weight (f32, :237)
  int project, distance_kernel;
  double kernel_scale, kernel_sigma2;  // 1.0 / (kSqrtTwoPi * sigma), double(sigma * sigma)
  float max_tsd, tsd_resolution;   // the grid's TSDValueConverter
  float max_weight, weight_resolution;
  int* error;
};

__device__ __forceinline__ float ClampF(float v, float lo, float hi) {   // common::Clamp
  if (v > hi) return hi;
  if (v < lo) return lo;
  return v;
}

// ValueConversionTables::GetConversionTable(unknown = lower, lower, upper) for one value; the
// update marker is masked.
__device__ __forceinline__ float ValueToBounded(unsigned raw, float lower, float upper) {
  const unsigned v = raw & 32767u;
  if (v == 0) return lower;
  const float scale = (upper - lower) / 32766.f;
  return static_cast<float>(v) * scale + (lower - scale);
}

// TSDValueConverter::TSDToValue / WeightToValue (tsd_value_converter.h:39-57).
__device__ __forceinline__ uint16_t TsdToValue(const TsdfParams& P, float tsd) {
  return static_cast<uint16_t>(
      LRoundF32((ClampF(tsd, -P.max_tsd, P.max_tsd) - -P.max_tsd) * P.tsd_resolution) + 1);
}
__device__ __forceinline__ uint16_t WeightToValue(const TsdfParams& P, float weight) {
  return static_cast<uint16_t>(
      LRoundF32((ClampF(weight, 0.f, P.max_weight) - 0.f) * P.weight_resolution) + 1);
}

// InsertHit's per-cell update (:206-222): the clamped tsd and the update weight of `cell` for
// `ray`.  GetCellCenter (map_limits.h:79-82) takes (x, y) = (max_x - r (iy + .5), max_y - r (ix + .5)).
__device__ __forceinline__ float2 CellUpdate(const TsdfParams& P, const TsdfRay& ray, int cx,
                                             int cy) {
  const float center_x = static_cast<float>(P.max_x - P.resolution * (cy + 0.5));
  const float center_y = static_cast<float>(P.max_y - P.resolution * (cx + 0.5));
  const float dx = center_x - P.origin_x, dy = center_y - P.origin_y;
  const float distance_cell_to_origin = sqrtf(dx * dx + dy * dy);
  float update_tsd = ray.range - distance_cell_to_origin;
  if (P.project) {
    update_tsd = (center_x - ray.hit_x) * ray.cos_normal + (center_y - ray.hit_y) * ray.sin_normal;
  }
  update_tsd = ClampF(update_tsd, -P.truncation, P.truncation);
  float update_weight = ray.weight_factor;
  if (P.distance_kernel) {
    // GaussianKernel (:49-51): float of 1.0 / (kSqrtTwoPi * sigma) * exp(-0.5 x x / (sigma sigma))
    const double e = -0.5 * static_cast<double>(update_tsd) * static_cast<double>(update_tsd) /
                     P.kernel_sigma2;
    update_weight *= static_cast<float>(P.kernel_scale * exp(e));
  }
  return make_float2(update_tsd, update_weight);
}

__device__ __forceinline__ bool Inside(const TsdfParams& P, int cx, int cy) {
  if (static_cast<unsigned>(cx) < static_cast<unsigned>(P.nx) &&
      static_cast<unsigned>(cy) < static_cast<unsigned>(P.ny))
    return true;
  *P.error = 1;                                          // the host checked the ray ends
  return false;
}

// ---- host ------------------------------------------------------------------------
// The part of the parameters that is the grid's ...
inline TsdfParams MakeParams(const cmx_tsdf2d& g) {
  TsdfParams P{};
  P.tsd = g.tsd;
  P.weight = g.weight;
  P.owner = g.owner;
  P.nx = g.nx;
  P.ny = g.ny;
  P.resolution = g.resolution;
  P.max_x = g.max_x;
  P.max_y = g.max_y;
  P.max_tsd = g.max_tsd;
  P.tsd_resolution = 32766.f / (g.max_tsd - -g.max_tsd);
  P.max_weight = g.max_weight;
  P.weight_resolution = 32766.f / (g.max_weight - 0.f);
  return P;
}

// ... and the part that is the insertion's: the origin and the inserter's options.
inline void SetInsertion(TsdfParams* P, const float* origin_xyz,
                         const cmx_tsdf_inserter_options_2d& o) {
  const double distance_bandwidth = o.update_weight_distance_cell_to_hit_kernel_bandwidth;
  P->origin_x = origin_xyz[0];
  P->origin_y = origin_xyz[1];
  P->truncation = static_cast<float>(o.truncation_distance);
  P->maximum_weight = static_cast<float>(o.maximum_weight);
  P->project = o.project_sdf_distance_to_scan_normal != 0;
  P->distance_kernel = distance_bandwidth != 0.f;
  if (P->distance_kernel) {
    const float sigma = static_cast<float>(distance_bandwidth);
    const float kSqrtTwoPi = std::sqrt(2.0 * M_PI);
    P->kernel_scale = 1.0 / (kSqrtTwoPi * sigma);
    P->kernel_sigma2 = sigma * sigma;
  }
}

// The checks of the inserter's options (:64-74).
inline void RequireInserterOptions(const cmx_tsdf_inserter_options_2d* options) {
  CMX_REQUIRE(options != nullptr, "null options");
  CMX_REQUIRE(options->num_normal_samples > 0, "num_normal_samples must be > 0");
  CMX_REQUIRE(options->sample_radius > 0., "sample_radius must be > 0");
}

}  // namespace
}  // namespace cmx

#endif  // CMX_TSDF_2D_INTERNAL_H_
