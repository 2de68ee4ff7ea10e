// Device-resident TSDF2D with range-data insertion on gfx950: what grid_2d.hip does for the
// ProbabilityGrid, for the submaps of grid_type = "TSDF" (mapping/2d/submap_2d.cc:58-60,
// :183-186).  Insertion, real-time matching and the loop-closure stack then read the two planes
// where they are.
//
// Reference: mapping/internal/2d/tsdf_range_data_inserter_2d.cc:33-240 (GrowAsNeeded,
// RangeDataSorter, Insert, InsertHit, UpdateCell), normal_estimation_2d.cc:23-110,
// tsdf_2d.cc:49-135 (CellIsUpdated, SetCell, GetTSDAndWeight, GrowLimits, ComputeCroppedGrid),
// mapping/2d/grid_2d.cc:99-164, tsd_value_converter.{h,cc}, value_conversion_tables.cc:29-52.
//
// Parallel form.  The reference walks the hits in order and updates a cell at most once per
// Insert (the update marker, CellIsUpdated at :205); a zero update weight returns before the
// marker is set (UpdateCell, :230), so a later ray may still take the cell.  The value written
// depends on which ray takes it, so "first writer wins" is not order-independent as it is for
// the probability grid.  Equivalent rule: each cell takes the update of the LOWEST hit index
// whose ray mask contains it and whose update weight is non-zero, applied to the cell's
// pre-insert value.  Two kernels, one wavefront per ray (lanes over pixel columns):
//   TsdfOwnerKernel   every covered cell with a non-zero weight: atomicMin(owner, hit index)
//   TsdfApplyKernel   the owner recomputes its update, UpdateCell + SetCell, and resets the
//                     owner entry (an atomicCAS, so a cell met twice is applied once)
// No update marker is written, so FinishUpdate has nothing to clear; TSDToValue >= 1 keeps
// "known = non-zero" for cropping.  A created plane that already carries the marker on a cell
// is never updated there (SetCell returns early) and keeps the bit.
//
// Host and device split.  The O(N) per-hit work runs on the host with the libm the reference
// uses, so that it is bit-exact without restating any transcendental: GrowAsNeeded, the sort,
// EstimateNormals, the angle kernel, the range weight (std::pow), cos / sin of the normal and
// the superscaled ray ends.  Per cell, on the device: GetCellCenter, the distance to the origin
// (f32 norm, terms left to right), the projection on the normal, the clamp, GaussianKernel of
// the distance (a float of a double exp), the weighted average and the value converters.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "ray_mask_2d.h"
#include "scan_matching_2d.h"

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
namespace {

constexpr uint16_t kUpdateMarker = 1u << 15;
constexpr int kNoOwner = 0x7f7f7f7f;                     // hipMemset(0x7f): above any hit index

// ---- device ----------------------------------------------------------------------
// One hit of the sorted range data, prepared on the host.
struct TsdfRay {
  int2 begin, end;                 // superscaled ray ends (SuperscaleRay, :53-67)
  float hit_x, hit_y, range;
  float weight_factor;             // weight_factor_range * weight_factor_angle_ray_normal
  float cos_normal, sin_normal;    // projection on the scan normal
};

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

// Pass 1: the lowest hit index with a non-zero update weight claims each cell.
__global__ void __launch_bounds__(256)
TsdfOwnerKernel(TsdfParams P, const TsdfRay* __restrict__ rays, int num_rays) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= num_rays) return;
  const TsdfRay ray = rays[r];
  if (!P.distance_kernel && ray.weight_factor == 0.f) return;   // no cell of this ray updates
  ForEachRayPixel(ray.begin, ray.end, lane, [&](int x, int y) {
    if (!Inside(P, x, y)) return;
    const size_t flat = static_cast<size_t>(P.nx) * y + x;
    if (P.tsd[flat] >= kUpdateMarker) return;            // CellIsUpdated before this Insert
    if (CellUpdate(P, ray, x, y).y == 0.f) return;       // UpdateCell returns unmarked (:230)
    atomicMin(&P.owner[flat], r);
  });
}

// Pass 2: UpdateCell + SetCell (:227-239, tsdf_2d.cc:49-61) by the owner, on the pre-insert
// value (no other ray writes an owned cell), then the owner entry is reset.
__global__ void __launch_bounds__(256)
TsdfApplyKernel(TsdfParams P, const TsdfRay* __restrict__ rays, int num_rays) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= num_rays) return;
  const TsdfRay ray = rays[r];
  if (!P.distance_kernel && ray.weight_factor == 0.f) return;
  ForEachRayPixel(ray.begin, ray.end, lane, [&](int x, int y) {
    if (!Inside(P, x, y)) return;
    const size_t flat = static_cast<size_t>(P.nx) * y + x;
    if (P.owner[flat] != r || atomicCAS(&P.owner[flat], r, kNoOwner) != r) return;
    const float2 u = CellUpdate(P, ray, x, y);
    const float old_tsd = ValueToBounded(P.tsd[flat], -P.max_tsd, P.max_tsd);
    const float old_weight = ValueToBounded(P.weight[flat], 0.f, P.max_weight);
    float updated_weight = old_weight + u.y;
    const float updated_sdf = (old_tsd * old_weight + u.x * u.y) / updated_weight;
    updated_weight = P.maximum_weight < updated_weight ? P.maximum_weight : updated_weight;
    P.tsd[flat] = TsdToValue(P, updated_sdf);
    P.weight[flat] = WeightToValue(P, updated_weight);
  });
}

// TSDF2D::ComputeCroppedGrid (tsdf_2d.cc:118-135): every known cell of the box is written into
// the new grid as SetCell(GetTSD, GetWeight): both values round-trip through float.
__global__ void TsdfCropKernel(TsdfParams P, int off_x, int off_y, uint16_t* __restrict__ tsd,
                               uint16_t* __restrict__ weight, int cnx) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= cnx) return;
  const size_t src = static_cast<size_t>(y + off_y) * P.nx + x + off_x;
  const size_t dst = static_cast<size_t>(y) * cnx + x;
  const uint16_t v = P.tsd[src];
  if (v == 0) {                                          // !IsKnown: stays unknown
    tsd[dst] = 0;
    weight[dst] = 0;
    return;
  }
  tsd[dst] = TsdToValue(P, ValueToBounded(v, -P.max_tsd, P.max_tsd));
  weight[dst] = WeightToValue(P, ValueToBounded(P.weight[src], 0.f, P.max_weight));
}

// ---- host ------------------------------------------------------------------------
struct P3 { float x, y, z; };
struct V2 { float x, y; };

// The stand-in Eigen's fixed-size norms: terms left to right; normalized() = v / sqrt(z) if
// z = squaredNorm > 0, else v (Eigen 3.3 Dot.h).
float Norm2(float x, float y) { return std::sqrt(x * x + y * y); }
float Norm3(const P3& v) { return std::sqrt((v.x * v.x + v.y * v.y) + v.z * v.z); }
V2 Normalized2(float x, float y) {
  const float z = x * x + y * y;
  if (z > 0.f) {
    const float n = std::sqrt(z);
    return {x / n, y / n};
  }
  return {x, y};
}
P3 Normalized3(const P3& v) {
  const float z = (v.x * v.x + v.y * v.y) + v.z * v.z;
  if (z > 0.f) {
    const float n = std::sqrt(z);
    return {v.x / n, v.y / n, v.z / n};
  }
  return v;
}
P3 Sub3(const P3& a, const P3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }

// GaussianKernel (:49-51) on the host.
float GaussianKernel(float x, float sigma) {
  const float kSqrtTwoPi = std::sqrt(2.0 * M_PI);
  return 1.0 / (kSqrtTwoPi * sigma) * std::exp(-0.5 * x * x / (sigma * sigma));
}

// common::NormalizeAngleDifference<float>.
float NormalizeAngleDifference(float difference) {
  const float kPi = float(M_PI);
  while (difference > kPi) difference -= 2. * kPi;
  while (difference < -kPi) difference += 2. * kPi;
  return difference;
}

// EstimateNormal / EstimateNormals (normal_estimation_2d.cc:31-110).
float EstimateNormal(const std::vector<P3>& returns, size_t estimation_point_index,
                     size_t sample_window_begin, size_t sample_window_end, const P3& origin) {
  const P3& estimation_point = returns[estimation_point_index];
  if (sample_window_end - sample_window_begin < 2) {
    const P3 d = Sub3(origin, estimation_point);
    return std::atan2(d.y, d.x);
  }
  P3 mean_normal{0.f, 0.f, 0.f};
  const P3 estimation_point_to_observation = Sub3(origin, estimation_point);
  for (size_t k = sample_window_begin; k < sample_window_end; ++k) {
    if (k == estimation_point_index) continue;
    const P3 tangent = Sub3(estimation_point, returns[k]);
    P3 sample_normal{-tangent.y, tangent.x, 0.f};
    constexpr float kMinNormalLength = 1e-6f;
    if (Norm3(sample_normal) < kMinNormalLength) continue;
    const P3& o = estimation_point_to_observation;
    if ((sample_normal.x * o.x + sample_normal.y * o.y) + sample_normal.z * o.z < 0) {
      sample_normal = {-sample_normal.x, -sample_normal.y, -sample_normal.z};
    }
    sample_normal = Normalized3(sample_normal);
    mean_normal.x += sample_normal.x;
    mean_normal.y += sample_normal.y;
    mean_normal.z += sample_normal.z;
  }
  return std::atan2(mean_normal.y, mean_normal.x);
}

std::vector<float> EstimateNormals(const std::vector<P3>& returns, const P3& origin,
                                   int num_normal_samples, double sample_radius_d) {
  std::vector<float> normals;
  normals.reserve(returns.size());
  const size_t max_num_samples = num_normal_samples;
  const float sample_radius = sample_radius_d;
  for (size_t current = 0; current < returns.size(); ++current) {
    const P3& hit = returns[current];
    size_t begin = current;
    for (; begin > 0 && current - begin < max_num_samples / 2 &&
           Norm3(Sub3(hit, returns[begin - 1])) < sample_radius;
         --begin) {
    }
    size_t end = current;
    for (; end < returns.size() && end - current < ceil(max_num_samples / 2.0) + 1 &&
           Norm3(Sub3(hit, returns[end])) < sample_radius;
         ++end) {
    }
    normals.push_back(EstimateNormal(returns, current, begin, end, origin));
  }
  return normals;
}

// MapLimits::GetCellIndex (map_limits.h:69-76).
void CellIndex(double resolution, double max_x, double max_y, float px, float py, int* ix,
               int* iy) {
  *ix = static_cast<int>(std::lround((max_y - py) / resolution - 0.5));
  *iy = static_cast<int>(std::lround((max_x - px) / resolution - 0.5));
}

bool Contains(const cmx_tsdf2d& g, float px, float py) {
  int ix, iy;
  CellIndex(g.resolution, g.max_x, g.max_y, px, py, &ix, &iy);
  return ix >= 0 && ix < g.nx && iy >= 0 && iy < g.ny;
}

void ResetOwner(cmx_tsdf2d* g, hipStream_t stream) {
  CMX_HIP(hipMemsetAsync(g->owner, 0x7f, static_cast<size_t>(g->nx) * g->ny * sizeof(int32_t),
                         stream));
}

// TSDF2D::GrowLimits (tsdf_2d.cc:100-105 -> grid_2d.cc:130-164): both planes, unknown 0 in each.
void GrowLimits(cmx_tsdf2d* g, Workspace& ws, float px, float py) {
  while (!Contains(*g, px, py)) {
    CMX_REQUIRE(static_cast<long long>(g->nx) * g->ny < (1ll << 28), "grid grows beyond 2^30 cells");
    const int x_offset = g->nx / 2, y_offset = g->ny / 2;
    const size_t new_count = 4 * static_cast<size_t>(g->nx) * g->ny;
    uint16_t* grown[2] = {nullptr, nullptr};
    int32_t* owner = nullptr;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&grown[0]), new_count * sizeof(uint16_t));
    if (err == hipSuccess)
      err = hipMalloc(reinterpret_cast<void**>(&grown[1]), new_count * sizeof(uint16_t));
    if (err == hipSuccess)
      err = hipMalloc(reinterpret_cast<void**>(&owner), new_count * sizeof(int32_t));
    if (err != hipSuccess) {
      (void)hipFree(grown[0]);
      (void)hipFree(grown[1]);
      (void)hipFree(owner);
      CMX_HIP(err);
    }
    uint16_t* const old[2] = {g->tsd, g->weight};
    for (int k = 0; k < 2; ++k) {
      CMX_HIP(hipMemsetAsync(grown[k], 0, new_count * sizeof(uint16_t), ws.stream));
      LaunchGridGrow(old[k], g->nx, g->ny, grown[k], x_offset, y_offset, ws.stream);
    }
    CMX_HIP(hipStreamSynchronize(ws.stream));
    CMX_HIP(hipFree(g->tsd));
    CMX_HIP(hipFree(g->weight));
    CMX_HIP(hipFree(g->owner));
    g->tsd = grown[0];
    g->weight = grown[1];
    g->owner = owner;
    ++g->version;
    g->max_x += g->resolution * y_offset;
    g->max_y += g->resolution * x_offset;
    g->nx *= 2;
    g->ny *= 2;
    ResetOwner(g, ws.stream);
  }
}

TsdfParams MakeParams(const cmx_tsdf2d& g) {
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

}  // namespace

// For ceres_2d.hip: the planes and ranges of a resident grid.
void Tsdf2DDevicePlanes(const cmx_tsdf2d* grid, cmx_grid2d_limits* limits, const uint16_t** tsd,
                        const uint16_t** weight, float* max_weight, int* device) {
  limits->resolution = grid->resolution;
  limits->max_x = grid->max_x;
  limits->max_y = grid->max_y;
  limits->num_x_cells = grid->nx;
  limits->num_y_cells = grid->ny;
  // Grid2D(limits, -truncation_distance, truncation_distance) (tsdf_2d.cc:25-26)
  limits->min_correspondence_cost = -grid->max_tsd;
  limits->max_correspondence_cost = grid->max_tsd;
  *tsd = grid->tsd;
  *weight = grid->weight;
  *max_weight = grid->max_weight;
  *device = grid->device;
}

}  // namespace cmx

using cmx::Guard;

extern "C" cmx_status cmx_tsdf2d_create(const cmx_grid2d_limits* limits, float truncation_distance,
                                        float max_weight, const uint16_t* tsd_cells,
                                        const uint16_t* weight_cells, int32_t device,
                                        cmx_tsdf2d** out) {
  return Guard([&] {
    CMX_REQUIRE(limits && out, "null argument");
    CMX_REQUIRE(limits->resolution > 0. && limits->num_x_cells >= 1 && limits->num_y_cells >= 1,
                "bad map limits");
    CMX_REQUIRE(truncation_distance > 0.f && max_weight > 0.f, "bad TSDF ranges");
    CMX_REQUIRE((tsd_cells == nullptr) == (weight_cells == nullptr),
                "give both planes or neither");
    cmx::UseDevice(device);
    std::unique_ptr<cmx_tsdf2d, void (*)(cmx_tsdf2d*)> g(new cmx_tsdf2d, cmx_tsdf2d_destroy);
    g->device = device;
    g->resolution = limits->resolution;
    g->max_x = limits->max_x;
    g->max_y = limits->max_y;
    g->nx = limits->num_x_cells;
    g->ny = limits->num_y_cells;
    g->max_tsd = truncation_distance;
    g->max_weight = max_weight;
    const size_t count = static_cast<size_t>(g->nx) * g->ny;
    CMX_HIP(hipMalloc(reinterpret_cast<void**>(&g->tsd), count * sizeof(uint16_t)));
    CMX_HIP(hipMalloc(reinterpret_cast<void**>(&g->weight), count * sizeof(uint16_t)));
    CMX_HIP(hipMalloc(reinterpret_cast<void**>(&g->owner), count * sizeof(int32_t)));
    if (tsd_cells) {
      CMX_HIP(hipMemcpy(g->tsd, tsd_cells, count * sizeof(uint16_t), hipMemcpyHostToDevice));
      CMX_HIP(hipMemcpy(g->weight, weight_cells, count * sizeof(uint16_t), hipMemcpyHostToDevice));
    } else {
      CMX_HIP(hipMemset(g->tsd, 0, count * sizeof(uint16_t)));      // getUnknownTSDValue
      CMX_HIP(hipMemset(g->weight, 0, count * sizeof(uint16_t)));   // getUnknownWeightValue
    }
    CMX_HIP(hipMemset(g->owner, 0x7f, count * sizeof(int32_t)));     // kNoOwner
    *out = g.release();
  });
}

extern "C" void cmx_tsdf2d_destroy(cmx_tsdf2d* grid) {
  if (!grid) return;
  (void)hipSetDevice(grid->device);
  if (grid->tsd) (void)hipFree(grid->tsd);
  if (grid->weight) (void)hipFree(grid->weight);
  if (grid->owner) (void)hipFree(grid->owner);
  delete grid;
}

extern "C" cmx_status cmx_tsdf2d_get_limits(const cmx_tsdf2d* grid, cmx_grid2d_limits* limits) {
  return Guard([&] {
    CMX_REQUIRE(grid && limits, "null argument");
    limits->resolution = grid->resolution;
    limits->max_x = grid->max_x;
    limits->max_y = grid->max_y;
    limits->num_x_cells = grid->nx;
    limits->num_y_cells = grid->ny;
    // Grid2D(limits, -truncation_distance, truncation_distance) (tsdf_2d.cc:25-26)
    limits->min_correspondence_cost = -grid->max_tsd;
    limits->max_correspondence_cost = grid->max_tsd;
  });
}

extern "C" cmx_status cmx_tsdf2d_download(const cmx_tsdf2d* grid, uint16_t* tsd_cells,
                                          uint16_t* weight_cells) {
  return Guard([&] {
    CMX_REQUIRE(grid && (tsd_cells || weight_cells), "null argument");
    cmx::UseDevice(grid->device);
    const size_t bytes = static_cast<size_t>(grid->nx) * grid->ny * sizeof(uint16_t);
    if (tsd_cells) CMX_HIP(hipMemcpy(tsd_cells, grid->tsd, bytes, hipMemcpyDeviceToHost));
    if (weight_cells) CMX_HIP(hipMemcpy(weight_cells, grid->weight, bytes, hipMemcpyDeviceToHost));
  });
}

extern "C" cmx_status cmx_tsdf2d_insert(cmx_tsdf2d* grid, const float* origin_xyz,
                                        const float* returns_xyz, int32_t num_returns,
                                        const cmx_tsdf_inserter_options_2d* options) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(grid && origin_xyz && options, "null argument");
    CMX_REQUIRE(num_returns >= 0 && (num_returns == 0 || returns_xyz), "bad range data");
    CMX_REQUIRE(options->num_normal_samples > 0, "num_normal_samples must be > 0");   // :64-74
    CMX_REQUIRE(options->sample_radius > 0., "sample_radius must be > 0");
    const cmx_tsdf_inserter_options_2d& o = *options;
    WorkspaceLease ws(grid->device);
    const float truncation_distance = static_cast<float>(o.truncation_distance);
    const P3 origin{origin_xyz[0], origin_xyz[1], origin_xyz[2]};
    std::vector<P3> returns(num_returns);
    if (num_returns) std::memcpy(returns.data(), returns_xyz, sizeof(P3) * num_returns);

    // GrowAsNeeded (:33-47): the box of origin.xy and hit + t * direction, direction in 3D.
    float lo_x = origin.x, hi_x = origin.x, lo_y = origin.y, hi_y = origin.y;
    for (const P3& hit : returns) {
      const P3 direction = Normalized3(Sub3(hit, origin));
      const float end_x = hit.x + truncation_distance * direction.x;
      const float end_y = hit.y + truncation_distance * direction.y;
      lo_x = std::min(lo_x, end_x); hi_x = std::max(hi_x, end_x);
      lo_y = std::min(lo_y, end_y); hi_y = std::max(hi_y, end_y);
    }
    constexpr float kPadding = 1e-6f;
    GrowLimits(grid, *ws, lo_x - kPadding * 1.f, lo_y - kPadding * 1.f);
    GrowLimits(grid, *ws, hi_x + kPadding * 1.f, hi_y + kPadding * 1.f);

    // Normals, on the returns sorted by RangeDataSorter (:69-88, :139-152).
    const double angle_bandwidth = o.update_weight_angle_scan_normal_to_ray_kernel_bandwidth;
    const double distance_bandwidth = o.update_weight_distance_cell_to_hit_kernel_bandwidth;
    const bool angle_kernel = angle_bandwidth != 0.f;
    std::vector<float> normals;
    if (o.project_sdf_distance_to_scan_normal || angle_kernel) {
      const V2 o2{origin.x, origin.y};
      std::sort(returns.begin(), returns.end(), [o2](const P3& lhs, const P3& rhs) {
        const V2 delta_lhs = Normalized2(lhs.x - o2.x, lhs.y - o2.y);
        const V2 delta_rhs = Normalized2(rhs.x - o2.x, rhs.y - o2.y);
        if ((delta_lhs.y < 0.f) != (delta_rhs.y < 0.f)) {
          return delta_lhs.y < 0.f;
        } else if (delta_lhs.y < 0.f) {
          return delta_lhs.x < delta_rhs.x;
        } else {
          return delta_lhs.x > delta_rhs.x;
        }
      });
      normals = EstimateNormals(returns, origin, o.num_normal_samples, o.sample_radius);
    }

    // InsertHit's per-hit part (:171-201); hits closer than the truncation distance add no ray.
    const double fine_resolution = grid->resolution / kSubpixelScale;
    std::vector<TsdfRay> rays;
    rays.reserve(returns.size());
    for (size_t i = 0; i < returns.size(); ++i) {
      const V2 hit{returns[i].x, returns[i].y};
      const float normal = normals.empty() ? std::numeric_limits<float>::quiet_NaN() : normals[i];
      const V2 ray{hit.x - origin.x, hit.y - origin.y};
      const float range = Norm2(ray.x, ray.y);
      if (range < truncation_distance) continue;
      const float truncation_ratio = truncation_distance / range;
      V2 begin{origin.x, origin.y};
      if (!o.update_free_space) {
        const float s = 1.0f - truncation_ratio;
        begin = {origin.x + s * ray.x, origin.y + s * ray.y};
      }
      const float e = 1.0f + truncation_ratio;
      const V2 end{origin.x + e * ray.x, origin.y + e * ray.y};
      TsdfRay r{};
      CellIndex(fine_resolution, grid->max_x, grid->max_y, begin.x, begin.y, &r.begin.x,
                &r.begin.y);
      CellIndex(fine_resolution, grid->max_x, grid->max_y, end.x, end.y, &r.end.x, &r.end.y);
      // Every pixel of the mask lies in the box of the two end pixels.
      for (const int2 c : {r.begin, r.end}) {
        CMX_REQUIRE(c.x >= 0 && c.y >= 0 && c.x / kSubpixelScale < grid->nx &&
                        c.y / kSubpixelScale < grid->ny,
                    "range data leaves the grid limits after GrowAsNeeded (hit %zu; z != 0?)", i);
      }
      float weight_factor_angle_ray_normal = 1.f;
      if (angle_kernel) {
        const float angle_ray_normal =
            NormalizeAngleDifference(normal - std::atan2(-ray.y, -ray.x));
        weight_factor_angle_ray_normal = GaussianKernel(angle_ray_normal, angle_bandwidth);
      }
      float weight_factor_range = 1.f;
      if (o.update_weight_range_exponent != 0) {               // ComputeRangeWeightFactor
        weight_factor_range = 0.f;
        if (std::abs(range) > 1e-6f)
          weight_factor_range = 1.f / (std::pow(range, o.update_weight_range_exponent));
      }
      r.hit_x = hit.x;
      r.hit_y = hit.y;
      r.range = range;
      r.weight_factor = weight_factor_range * weight_factor_angle_ray_normal;
      if (o.project_sdf_distance_to_scan_normal) {
        r.cos_normal = std::cos(normal);
        r.sin_normal = std::sin(normal);
      }
      rays.push_back(r);
    }

    ++grid->version;
    const int num_rays = static_cast<int>(rays.size());
    if (num_rays == 0) {
      CMX_HIP(hipStreamSynchronize(ws->stream));
      return;
    }
    TsdfParams P = MakeParams(*grid);
    P.origin_x = origin.x;
    P.origin_y = origin.y;
    P.truncation = truncation_distance;
    P.maximum_weight = static_cast<float>(o.maximum_weight);
    P.project = o.project_sdf_distance_to_scan_normal != 0;
    P.distance_kernel = distance_bandwidth != 0.f;
    if (P.distance_kernel) {
      const float sigma = static_cast<float>(distance_bandwidth);
      const float kSqrtTwoPi = std::sqrt(2.0 * M_PI);
      P.kernel_scale = 1.0 / (kSqrtTwoPi * sigma);
      P.kernel_sigma2 = sigma * sigma;
    }
    P.error = ws->dev[2].ReserveAs<int>(1);
    TsdfRay* h_rays = ws->pinned[0].ReserveAs<TsdfRay>(num_rays);
    std::memcpy(h_rays, rays.data(), sizeof(TsdfRay) * num_rays);
    TsdfRay* d_rays = ws->dev[0].ReserveAs<TsdfRay>(num_rays);
    CMX_HIP(hipMemsetAsync(P.error, 0, sizeof(int), ws->stream));
    CMX_HIP(hipMemcpyAsync(d_rays, h_rays, sizeof(TsdfRay) * num_rays, hipMemcpyHostToDevice,
                           ws->stream));
    TsdfOwnerKernel<<<DivUp(num_rays, 4), 256, 0, ws->stream>>>(P, d_rays, num_rays);
    TsdfApplyKernel<<<DivUp(num_rays, 4), 256, 0, ws->stream>>>(P, d_rays, num_rays);
    CMX_HIP(hipGetLastError());
    int* h_error = ws->pinned[1].ReserveAs<int>(1);
    CMX_HIP(hipMemcpyAsync(h_error, P.error, sizeof(int), hipMemcpyDeviceToHost, ws->stream));
    CMX_HIP(hipStreamSynchronize(ws->stream));
    CMX_REQUIRE(!*h_error, "internal error: a ray left the grid after GrowAsNeeded");
  });
}

extern "C" cmx_status cmx_tsdf2d_crop(cmx_tsdf2d* grid) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(grid != nullptr, "null argument");
    WorkspaceLease ws(grid->device);
    int* d_box = ws->dev[2].ReserveAs<int>(4);
    const int preset[4] = {0x7fffffff, 0x7fffffff, -1, -1};
    int* h_box = ws->pinned[0].ReserveAs<int>(4);
    std::memcpy(h_box, preset, sizeof(preset));
    CMX_HIP(hipMemcpyAsync(d_box, h_box, sizeof(preset), hipMemcpyHostToDevice, ws->stream));
    LaunchKnownBox(grid->tsd, grid->nx, grid->ny, d_box, ws->stream);
    CMX_HIP(hipMemcpyAsync(h_box, d_box, sizeof(preset), hipMemcpyDeviceToHost, ws->stream));
    CMX_HIP(hipStreamSynchronize(ws->stream));
    const bool empty = h_box[2] < 0;
    // ComputeCroppedLimits: no known cell -> offset 0, CellLimits(1, 1) (grid_2d.cc:106-110).
    const int off_x = empty ? 0 : h_box[0], off_y = empty ? 0 : h_box[1];
    const int cnx = empty ? 1 : h_box[2] - h_box[0] + 1, cny = empty ? 1 : h_box[3] - h_box[1] + 1;
    const size_t count = static_cast<size_t>(cnx) * cny;
    uint16_t* planes[2] = {nullptr, nullptr};
    int32_t* owner = nullptr;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&planes[0]), count * sizeof(uint16_t));
    if (err == hipSuccess)
      err = hipMalloc(reinterpret_cast<void**>(&planes[1]), count * sizeof(uint16_t));
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&owner), count * sizeof(int32_t));
    if (err == hipSuccess) err = hipMemsetAsync(owner, 0x7f, count * sizeof(int32_t), ws->stream);
    if (err == hipSuccess) {
      if (empty) {
        err = hipMemsetAsync(planes[0], 0, count * sizeof(uint16_t), ws->stream);
        if (err == hipSuccess) err = hipMemsetAsync(planes[1], 0, count * sizeof(uint16_t), ws->stream);
      } else {
        TsdfCropKernel<<<dim3(DivUp(cnx, 256), cny), 256, 0, ws->stream>>>(
            MakeParams(*grid), off_x, off_y, planes[0], planes[1], cnx);
        err = hipGetLastError();
      }
    }
    if (err == hipSuccess) err = hipStreamSynchronize(ws->stream);
    if (err != hipSuccess) {
      (void)hipFree(planes[0]);
      (void)hipFree(planes[1]);
      (void)hipFree(owner);
      CMX_HIP(err);
    }
    CMX_HIP(hipFree(grid->tsd));
    CMX_HIP(hipFree(grid->weight));
    CMX_HIP(hipFree(grid->owner));
    grid->tsd = planes[0];
    grid->weight = planes[1];
    grid->owner = owner;
    ++grid->version;
    // max = limits().max() - resolution * (offset.y, offset.x) (tsdf_2d.cc:123-124).
    grid->max_x = grid->max_x - grid->resolution * off_y;
    grid->max_y = grid->max_y - grid->resolution * off_x;
    grid->nx = cnx;
    grid->ny = cny;
  });
}

extern "C" cmx_status cmx_rt2d_match_tsdf_grid(const cmx_rt_options* options,
                                               const cmx_tsdf2d* grid,
                                               const cmx_pose2d* initial_pose_estimate,
                                               const float* point_cloud_xyz, int32_t num_points,
                                               double* score, cmx_pose2d* pose_estimate,
                                               cmx_match_stats* stats) {
  return Guard([&] {
    CMX_REQUIRE(options && grid, "null argument");
    cmx_grid2d_limits limits{grid->resolution, grid->max_x, grid->max_y, grid->nx, grid->ny,
                             0.f, 0.f};
    cmx::Rt2DItem item{};
    item.limits = &limits;
    item.device_cells = grid->tsd;
    item.device_weight_cells = grid->weight;
    item.max_tsd = grid->max_tsd;
    item.max_weight = grid->max_weight;
    item.initial = initial_pose_estimate;
    item.xyz = point_cloud_xyz;
    item.n = num_points;
    item.score = score;
    item.pose = pose_estimate;
    item.grid_version = grid->version;
    cmx::Rt2DMatchBatch(options, &item, 1, grid->device, stats);
  });
}

namespace {
// One item of a batch entry: grid m, pose m, its cloud (host pointer, or a cmx_cloud).
cmx::Rt2DItem TsdfBatchItem(const cmx_tsdf2d* g, const cmx_grid2d_limits* limits,
                            const cmx_pose2d* initial, double* score, cmx_pose2d* pose) {
  cmx::Rt2DItem item{};
  item.limits = limits;
  item.device_cells = g->tsd;
  item.device_weight_cells = g->weight;
  item.max_tsd = g->max_tsd;
  item.max_weight = g->max_weight;
  item.initial = initial;
  item.score = score;
  item.pose = pose;
  item.grid_version = g->version;
  item.tsdf_image_cache = &g->rt_image;
  return item;
}
}  // namespace

extern "C" cmx_status cmx_rt2d_match_tsdf_grid_batch(const cmx_rt_options* options,
                                                     const cmx_tsdf2d* const* grids,
                                                     int32_t num_matches,
                                                     const cmx_pose2d* initial_pose_estimates,
                                                     const float* const* point_clouds_xyz,
                                                     const int32_t* num_points, double* scores,
                                                     cmx_pose2d* pose_estimates,
                                                     cmx_match_stats* stats) {
  return Guard([&] {
    CMX_REQUIRE(options && grids && initial_pose_estimates && point_clouds_xyz && num_points &&
                    scores && pose_estimates && num_matches >= 1,
                "null argument");
    std::vector<cmx_grid2d_limits> limits(num_matches);
    std::vector<cmx::Rt2DItem> items(num_matches);
    for (int m = 0; m < num_matches; ++m) {
      const cmx_tsdf2d* g = grids[m];
      CMX_REQUIRE(g != nullptr, "null grid");
      CMX_REQUIRE(g->device == grids[0]->device, "all grids of a batch must live on one device");
      limits[m] = cmx_grid2d_limits{g->resolution, g->max_x, g->max_y, g->nx, g->ny, 0.f, 0.f};
      items[m] = TsdfBatchItem(g, &limits[m], &initial_pose_estimates[m], &scores[m],
                               &pose_estimates[m]);
      items[m].xyz = point_clouds_xyz[m];
      items[m].n = num_points[m];
    }
    cmx::Rt2DTsdfMatchBatch(options, items.data(), num_matches, grids[0]->device, stats);
  });
}

extern "C" cmx_status cmx_rt2d_match_tsdf_grid_batch_resident(
    const cmx_rt_options* options, const cmx_tsdf2d* const* grids, int32_t num_matches,
    const cmx_pose2d* initial_pose_estimates, const cmx_cloud* const* clouds, double* scores,
    cmx_pose2d* pose_estimates, cmx_match_stats* stats) {
  return Guard([&] {
    CMX_REQUIRE(options && grids && initial_pose_estimates && clouds && scores &&
                    pose_estimates && num_matches >= 1,
                "null argument");
    std::vector<cmx_grid2d_limits> limits(num_matches);
    std::vector<cmx::Rt2DItem> items(num_matches);
    for (int m = 0; m < num_matches; ++m) {
      const cmx_tsdf2d* g = grids[m];
      const cmx_cloud* c = clouds[m];
      CMX_REQUIRE(g != nullptr && c != nullptr, "null grid or cloud");
      CMX_REQUIRE(g->device == grids[0]->device && c->device == g->device,
                  "all grids and clouds of a batch must live on one device");
      limits[m] = cmx_grid2d_limits{g->resolution, g->max_x, g->max_y, g->nx, g->ny, 0.f, 0.f};
      items[m] = TsdfBatchItem(g, &limits[m], &initial_pose_estimates[m], &scores[m],
                               &pose_estimates[m]);
      items[m].xyz = c->host_xyz.data();      // the range scan of SearchParameters runs on the host
      items[m].device_xyz = c->xyz;
      if (!c->far_points.empty()) {
        items[m].far_points = c->far_points.data();
        items[m].num_far_points = static_cast<int>(c->far_points.size());
      }
      items[m].n = c->num_points;
    }
    cmx::Rt2DTsdfMatchBatch(options, items.data(), num_matches, grids[0]->device, stats);
  });
}

extern "C" cmx_status cmx_fast2d_create_from_tsdf(const cmx_fast2d_options* options,
                                                  const cmx_tsdf2d* grid, cmx_fast2d** out) {
  return Guard([&] {
    CMX_REQUIRE(options && grid && out, "null argument");
    // The stack is built from the tsd plane where it lies: the matcher takes its own copy
    // on the device (the grid may be inserted into or destroyed afterwards), nothing comes back
    // to the host.  Every call that changes the grid has synchronised before it returned.
    *out = nullptr;
    cmx_grid2d_limits limits;
    const cmx_status st = cmx_tsdf2d_get_limits(grid, &limits);
    if (st != CMX_OK) throw cmx::HipError{st};           // last error already set
    *out = cmx::CreateFast2DFromDeviceCells(*options, limits, grid->tsd, grid->device);
  });
}
