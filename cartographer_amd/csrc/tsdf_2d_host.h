// The host part of TSDFRangeDataInserter2D::Insert, shared by cmx_tsdf2d_insert (tsdf_2d.hip),
// cmx_tsdf2d_insert_batch and cmx_debug_tsdf2d_insert_plan (tsdf_2d_batch.hip): GrowAsNeeded on
// plain limits, RangeDataSorter, EstimateNormals, the per-hit part of InsertHit and the ray table
// the kernels read.  Plain C++17 without HIP types or CMX_REQUIRE, as cmx_batch.h: a failure is
// returned and the call site words it; loops that may run in parallel take the runner as an
// argument.  Pinned on the host by tests/test_abi_tsdf2d_insert_batch.py
// (tests/native/tsdf2d_prepare_check.cc, under the address and undefined-behaviour sanitizers).
//
// Reference: mapping/internal/2d/tsdf_range_data_inserter_2d.cc:33-201,
// normal_estimation_2d.cc:23-110, mapping/2d/map_limits.h:69-76, grid_2d.cc:130-164.
//
// What depends on the scan alone (the sort, the normals, every libm call, the box GrowAsNeeded
// takes) is prepared once per distinct scan: PreparedScan.  What depends on the grid's limits
// (the superscaled ray ends and the check that they lie inside) is done per insertion with the
// limits the grid has AT that insertion: BuildRays.
#ifndef CMX_TSDF_2D_HOST_H_
#define CMX_TSDF_2D_HOST_H_
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <map>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/cartographer_mi355x.h"

namespace cmx {
namespace {
// One hit of the sorted range data, as the kernels read it.  (Internal linkage, like the kernels
// that take it: their symbols are those they had before this file existed.)
#ifdef __HIPCC__
using TsdfCell = int2;
#else
struct alignas(8) TsdfCell { int x, y; };
#endif
struct TsdfRay {
  TsdfCell begin, end;             // superscaled ray ends (SuperscaleRay, :53-67)
  float hit_x, hit_y, range;
  float weight_factor;             // weight_factor_range * weight_factor_angle_ray_normal
  float cos_normal, sin_normal;    // projection on the scan normal
};
static_assert(sizeof(TsdfRay) == 40, "host and device agree on the ray table");
}  // namespace

namespace tsdf2d {

constexpr int kSubpixels = 1000;   // kSubpixelScale (..._inserter_2d.cc:27)

struct P3 { float x, y, z; };
struct V2 { float x, y; };

// The stand-in Eigen's fixed-size norms: terms left to right; normalized() = v / sqrt(z) if
// z = squaredNorm > 0, else v (Eigen 3.3 Dot.h).
inline float Norm2(float x, float y) { return std::sqrt(x * x + y * y); }
inline float Norm3(const P3& v) { return std::sqrt((v.x * v.x + v.y * v.y) + v.z * v.z); }
inline V2 Normalized2(float x, float y) {
  const float z = x * x + y * y;
  if (z > 0.f) {
    const float n = std::sqrt(z);
    return {x / n, y / n};
  }
  return {x, y};
}
inline P3 Normalized3(const P3& v) {
  const float z = (v.x * v.x + v.y * v.y) + v.z * v.z;
  if (z > 0.f) {
    const float n = std::sqrt(z);
    return {v.x / n, v.y / n, v.z / n};
  }
  return v;
}
inline P3 Sub3(const P3& a, const P3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }

// GaussianKernel (:49-51) on the host.
inline float GaussianKernel(float x, float sigma) {
  const float kSqrtTwoPi = std::sqrt(2.0 * M_PI);
  return 1.0 / (kSqrtTwoPi * sigma) * std::exp(-0.5 * x * x / (sigma * sigma));
}

// common::NormalizeAngleDifference<float>.
inline float NormalizeAngleDifference(float difference) {
  const float kPi = float(M_PI);
  while (difference > kPi) difference -= 2. * kPi;
  while (difference < -kPi) difference += 2. * kPi;
  return difference;
}

// EstimateNormal / EstimateNormals (normal_estimation_2d.cc:31-110).
inline float EstimateNormal(const std::vector<P3>& returns, size_t estimation_point_index,
                            size_t sample_window_begin, size_t sample_window_end,
                            const P3& origin) {
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

inline std::vector<float> EstimateNormals(const std::vector<P3>& returns, const P3& origin,
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

// ---- limits ------------------------------------------------------------------------------
struct Limits {
  double resolution, max_x, max_y;
  int nx, ny;
};

// MapLimits::GetCellIndex (map_limits.h:69-76).
inline void CellIndex(double resolution, double max_x, double max_y, float px, float py, int* ix,
                      int* iy) {
  *ix = static_cast<int>(std::lround((max_y - py) / resolution - 0.5));
  *iy = static_cast<int>(std::lround((max_x - px) / resolution - 0.5));
}

inline bool Contains(const Limits& g, float px, float py) {
  int ix, iy;
  CellIndex(g.resolution, g.max_x, g.max_y, px, py, &ix, &iy);
  return ix >= 0 && ix < g.nx && iy >= 0 && iy < g.ny;
}

// A grid of a call: its limits (in: before the call; while planning: at the insertion the plan
// has reached; out: after the call) and where cell (0, 0) of the grid before the call lies in them.
struct PlannedGrid {
  Limits limits{};
  int start_x = 0, start_y = 0;
  int doublings = 0, insertions = 0;
};

// TSDF2D::GrowLimits (tsdf_2d.cc:100-105 -> grid_2d.cc:130-164) on plain limits: the expressions
// of the device grid's GrowLimits in the same order.  false: the grid would pass 2^30 cells.
inline bool PlanGrow(PlannedGrid* grid, float px, float py) {
  Limits* g = &grid->limits;
  while (!Contains(*g, px, py)) {
    if (!(static_cast<long long>(g->nx) * g->ny < (1ll << 28))) return false;
    const int x_offset = g->nx / 2, y_offset = g->ny / 2;
    g->max_x += g->resolution * y_offset;
    g->max_y += g->resolution * x_offset;
    g->nx *= 2;
    g->ny *= 2;
    grid->start_x += x_offset;
    grid->start_y += y_offset;
    ++grid->doublings;
  }
  return true;
}

// ---- one scan ----------------------------------------------------------------------------
// A hit with f32 range >= truncation distance: InsertHit's per-hit part (:171-201) but for the
// cell indices of the ray ends.
struct RayProto {
  V2 begin, end;                   // map frame
  size_t hit;                      // index in the sorted range data
  float hit_x, hit_y, range, weight_factor, cos_normal, sin_normal;
};

struct PreparedScan {
  float lo_x = 0.f, hi_x = 0.f, lo_y = 0.f, hi_y = 0.f;   // GrowAsNeeded's box, without the padding
  std::vector<RayProto> rays;                              // in the order of the sorted hits
};

inline PreparedScan PrepareScan(const float* origin_xyz, const float* returns_xyz,
                                int num_returns, const cmx_tsdf_inserter_options_2d& o) {
  PreparedScan out;
  const float truncation_distance = static_cast<float>(o.truncation_distance);
  const P3 origin{origin_xyz[0], origin_xyz[1], origin_xyz[2]};
  std::vector<P3> returns(num_returns);
  if (num_returns) memcpy(returns.data(), returns_xyz, sizeof(P3) * num_returns);

  // GrowAsNeeded (:33-47): the box of origin.xy and hit + t * direction, direction in 3D.
  float lo_x = origin.x, hi_x = origin.x, lo_y = origin.y, hi_y = origin.y;
  for (const P3& hit : returns) {
    const P3 direction = Normalized3(Sub3(hit, origin));
    const float end_x = hit.x + truncation_distance * direction.x;
    const float end_y = hit.y + truncation_distance * direction.y;
    lo_x = std::min(lo_x, end_x); hi_x = std::max(hi_x, end_x);
    lo_y = std::min(lo_y, end_y); hi_y = std::max(hi_y, end_y);
  }
  out.lo_x = lo_x; out.hi_x = hi_x; out.lo_y = lo_y; out.hi_y = hi_y;

  // Normals, on the returns sorted by RangeDataSorter (:69-88, :139-152).
  const double angle_bandwidth = o.update_weight_angle_scan_normal_to_ray_kernel_bandwidth;
  const bool angle_kernel = angle_bandwidth != 0.f;
  std::vector<float> normals;
  if (o.project_sdf_distance_to_scan_normal || angle_kernel) {
    // RangeDataSorter normalises both deltas in every comparison; they depend on the point
    // alone, so each is computed once and travels with its point.  std::sort asks the same
    // questions of the same sequence and gets the same answers: the order is the reference's,
    // ties included.
    struct Keyed { V2 delta; P3 point; };
    std::vector<Keyed> keyed(returns.size());
    for (size_t i = 0; i < returns.size(); ++i)
      keyed[i] = Keyed{Normalized2(returns[i].x - origin.x, returns[i].y - origin.y), returns[i]};
    std::sort(keyed.begin(), keyed.end(), [](const Keyed& lhs, const Keyed& rhs) {
      const V2& delta_lhs = lhs.delta;
      const V2& delta_rhs = rhs.delta;
      if ((delta_lhs.y < 0.f) != (delta_rhs.y < 0.f)) {
        return delta_lhs.y < 0.f;
      } else if (delta_lhs.y < 0.f) {
        return delta_lhs.x < delta_rhs.x;
      } else {
        return delta_lhs.x > delta_rhs.x;
      }
    });
    for (size_t i = 0; i < returns.size(); ++i) returns[i] = keyed[i].point;
    normals = EstimateNormals(returns, origin, o.num_normal_samples, o.sample_radius);
  }

  // InsertHit's per-hit part (:171-201); hits closer than the truncation distance add no ray.
  out.rays.reserve(returns.size());
  for (size_t i = 0; i < returns.size(); ++i) {
    const V2 hit{returns[i].x, returns[i].y};
    const float normal = normals.empty() ? std::numeric_limits<float>::quiet_NaN() : normals[i];
    const V2 ray{hit.x - origin.x, hit.y - origin.y};
    const float range = Norm2(ray.x, ray.y);
    if (range < truncation_distance) continue;
    const float truncation_ratio = truncation_distance / range;
    RayProto r{};
    r.begin = {origin.x, origin.y};
    if (!o.update_free_space) {
      const float s = 1.0f - truncation_ratio;
      r.begin = {origin.x + s * ray.x, origin.y + s * ray.y};
    }
    const float e = 1.0f + truncation_ratio;
    r.end = {origin.x + e * ray.x, origin.y + e * ray.y};
    r.hit = i;
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
    out.rays.push_back(r);
  }
  return out;
}

// GrowAsNeeded's two GrowLimits calls for a scan.  false: the grid would pass 2^30 cells.
inline bool PlanGrowForScan(PlannedGrid* grid, const PreparedScan& scan) {
  constexpr float kPadding = 1e-6f;
  return PlanGrow(grid, scan.lo_x - kPadding * 1.f, scan.lo_y - kPadding * 1.f) &&
         PlanGrow(grid, scan.hi_x + kPadding * 1.f, scan.hi_y + kPadding * 1.f);
}

// The ray table of one insertion of `scan` into a grid with the limits `at`: scan.rays.size()
// entries to `out` (null: the check alone).  Every pixel of a ray's mask lies in the box of its
// two end pixels, which must be inside the limits: -1, or the sorted index of the first hit
// whose ray is not.
inline long BuildRays(const PreparedScan& scan, const Limits& at, TsdfRay* out) {
  const double fine_resolution = at.resolution / kSubpixels;
  for (size_t j = 0; j < scan.rays.size(); ++j) {
    const RayProto& p = scan.rays[j];
    TsdfRay r{};
    CellIndex(fine_resolution, at.max_x, at.max_y, p.begin.x, p.begin.y, &r.begin.x, &r.begin.y);
    CellIndex(fine_resolution, at.max_x, at.max_y, p.end.x, p.end.y, &r.end.x, &r.end.y);
    for (const TsdfCell& c : {r.begin, r.end}) {
      if (!(c.x >= 0 && c.y >= 0 && c.x / kSubpixels < at.nx && c.y / kSubpixels < at.ny))
        return static_cast<long>(p.hit);
    }
    if (!out) continue;
    r.hit_x = p.hit_x;
    r.hit_y = p.hit_y;
    r.range = p.range;
    r.weight_factor = p.weight_factor;
    r.cos_normal = p.cos_normal;
    r.sin_normal = p.sin_normal;
    out[j] = r;
  }
  return -1;
}

// ---- a call ------------------------------------------------------------------------------
struct InsertionInput {
  int grid;                        // index into the call's grids
  const float* origin;             // 3 floats
  const float* returns;
  int num_returns;
};

struct PlannedInsertion {
  Limits at{};                     // the grid's limits at this insertion, after its own growth
  int start_x = 0, start_y = 0;    // where cell (0, 0) of the grid before the call lies in `at`
  int scan = -1;                   // index into CallPlan::scans; -1: no returns
  size_t first_ray = 0;            // of its table in the call's ray table
  int num_rays = 0;
};

struct CallPlan {
  std::vector<PlannedGrid> grids;  // in: limits before the call; out: after it
  std::vector<PlannedInsertion> insertions;
  std::vector<PreparedScan> scans; // the distinct scans of the call
  size_t total_rays = 0;
};

struct PlanError {
  enum Kind { kNone, kCountMismatch, kTooManyCells, kLeavesLimits } kind = kNone;
  int insertion = -1;
  long a = 0, b = 0;               // kCountMismatch: returns there, here; kLeavesLimits: a = hit
  explicit operator bool() const { return kind != kNone; }
};

// Plans a call: every distinct scan -- the same returns pointer with bitwise equal origin
// values -- prepared once (run(n, fn) calls fn(0) .. fn(n - 1) in any order, on any threads),
// GrowAsNeeded replayed insertion by insertion in list order, the ray tables laid out one behind
// the other.  plan->grids in: the limits before the call.
template <class Run>
PlanError PlanCall(CallPlan* plan, const InsertionInput* in, int num,
                   const cmx_tsdf_inserter_options_2d& options, Run&& run) {
  using Key = std::tuple<const float*, uint32_t, uint32_t, uint32_t>;
  std::unordered_map<const float*, int> count_of;
  std::map<Key, int> scan_of;
  std::vector<int> first_user;     // by scan: the insertion that brought it
  plan->insertions.assign(num, PlannedInsertion{});
  for (int k = 0; k < num; ++k) {
    const InsertionInput& I = in[k];
    if (I.num_returns == 0) continue;
    const auto [seen, fresh] = count_of.emplace(I.returns, I.num_returns);
    if (!fresh && seen->second != I.num_returns)
      return PlanError{PlanError::kCountMismatch, k, seen->second, I.num_returns};
    uint32_t bits[3];
    memcpy(bits, I.origin, sizeof(bits));
    const auto found = scan_of.emplace(Key{I.returns, bits[0], bits[1], bits[2]},
                                       static_cast<int>(first_user.size()));
    if (found.second) first_user.push_back(k);
    plan->insertions[k].scan = found.first->second;
  }
  plan->scans.assign(first_user.size(), PreparedScan{});
  run(static_cast<int>(first_user.size()), [&](int s) {
    const InsertionInput& I = in[first_user[s]];
    plan->scans[s] = PrepareScan(I.origin, I.returns, I.num_returns, options);
  });
  plan->total_rays = 0;
  for (int k = 0; k < num; ++k) {
    PlannedInsertion& P = plan->insertions[k];
    PlannedGrid& G = plan->grids[in[k].grid];
    PreparedScan origin_only;      // no returns: the box is the origin
    origin_only.lo_x = origin_only.hi_x = in[k].origin[0];
    origin_only.lo_y = origin_only.hi_y = in[k].origin[1];
    const PreparedScan& scan = P.scan >= 0 ? plan->scans[P.scan] : origin_only;
    if (!PlanGrowForScan(&G, scan)) return PlanError{PlanError::kTooManyCells, k};
    ++G.insertions;
    P.at = G.limits;
    P.start_x = G.start_x;
    P.start_y = G.start_y;
    P.first_ray = plan->total_rays;
    P.num_rays = static_cast<int>(scan.rays.size());
    plan->total_rays += scan.rays.size();
  }
  return PlanError{};
}

// The ray tables of a planned call into `table` (plan.total_rays entries; null: the checks
// alone), insertion by insertion through run().  The error of the first insertion in list order
// that has one.
template <class Run>
PlanError BuildRayTables(const CallPlan& plan, TsdfRay* table, Run&& run) {
  const int num = static_cast<int>(plan.insertions.size());
  std::vector<long> bad(num, -1);
  run(num, [&](int k) {
    const PlannedInsertion& P = plan.insertions[k];
    if (P.scan >= 0)
      bad[k] = BuildRays(plan.scans[P.scan], P.at, table ? table + P.first_ray : nullptr);
  });
  for (int k = 0; k < num; ++k)
    if (bad[k] >= 0) return PlanError{PlanError::kLeavesLimits, k, bad[k]};
  return PlanError{};
}

}  // namespace tsdf2d
}  // namespace cmx
#endif  // CMX_TSDF_2D_HOST_H_
