// Test driver (never linked into the product): the reference's own TSDFMatchCostFunction2D and
// CeresScanMatcher2D::Match on a TSDF2D, as oracle/_ref/libref_ceres.so compiles them over the
// stand-in solver of oracle/ref_shims/ceres.  tests/golden/make_ceres2d_tsdf_golden.py builds it
// into a temporary directory:
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -Ioracle/ref_shims -I<reference>
//       tests/native/ceres2d_tsdf_ref.cc oracle/_ref/libref_ceres.so
// and writes tests/golden/ceres2d_tsdf_golden.npz from it.
#include <cmath>
#include <cstdint>
#include <memory>
#include <vector>

#include "cartographer/mapping/internal/2d/scan_matching/ceres_scan_matcher_2d.h"
#include "cartographer/mapping/internal/2d/scan_matching/tsdf_match_cost_function_2d.h"
#include "cartographer/mapping/internal/2d/tsdf_2d.h"
#include "cartographer/mapping/value_conversion_tables.h"

namespace {
namespace cm = cartographer::mapping;
namespace sm = cartographer::mapping::scan_matching;

cartographer::sensor::PointCloud MakeCloud(const float* xyz, int n) {
  std::vector<cartographer::sensor::RangefinderPoint> points;
  for (int i = 0; i != n; ++i)
    points.push_back({Eigen::Vector3f(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])});
  return cartographer::sensor::PointCloud(std::move(points));
}

// The planes enter the real TSDF2D through its proto constructor (grid_2d.cc:77-98,
// tsdf_2d.cc:35-47).
std::unique_ptr<cm::TSDF2D> MakeTsdf(const uint16_t* tsd, const uint16_t* weight, int nx, int ny,
                                     double resolution, double max_x, double max_y,
                                     float truncation_distance, float max_weight,
                                     cm::ValueConversionTables* tables) {
  cm::proto::Grid2D proto;
  *proto.mutable_limits() = cm::ToProto(
      cm::MapLimits(resolution, Eigen::Vector2d(max_x, max_y), cm::CellLimits(nx, ny)));
  const size_t count = static_cast<size_t>(nx) * ny;
  proto.mutable_cells()->assign(tsd, tsd + count);
  proto.set_min_correspondence_cost(-truncation_distance);
  proto.set_max_correspondence_cost(truncation_distance);
  proto.mutable_tsdf_2d()->set_truncation_distance(truncation_distance);
  proto.mutable_tsdf_2d()->set_max_weight(max_weight);
  proto.mutable_tsdf_2d()->mutable_weight_cells()->assign(weight, weight + count);
  return std::make_unique<cm::TSDF2D>(proto, tables);
}

}  // namespace

extern "C" {

// TSDFMatchCostFunction2D::Evaluate with Jacobians: returns the functor's result; residuals[n]
// and jacobian[3n] (row-major) are written only when it is true.
int drv_tsdf_residuals(const uint16_t* tsd, const uint16_t* weight, int nx, int ny, double res,
                       double max_x, double max_y, float truncation_distance, float max_weight,
                       double scaling, const double* pose, const float* xyz, int n,
                       double* residuals, double* jacobian) {
  cm::ValueConversionTables tables;
  const auto grid = MakeTsdf(tsd, weight, nx, ny, res, max_x, max_y, truncation_distance,
                             max_weight, &tables);
  const cartographer::sensor::PointCloud cloud = MakeCloud(xyz, n);
  std::unique_ptr<ceres::CostFunction> f(
      sm::CreateTSDFMatchCostFunction2D(scaling, cloud, *grid));
  std::vector<double> r(n), J(3 * static_cast<size_t>(n));
  const double* params[1] = {pose};
  double* jacobians[1] = {J.data()};
  const bool ok = f->Evaluate(params, r.data(), jacobians);
  if (ok) {
    for (int i = 0; i != n; ++i) residuals[i] = r[i];
    for (int i = 0; i != 3 * n; ++i) jacobian[i] = J[i];
  }
  return ok ? 1 : 0;
}

// CeresScanMatcher2D::Match on the TSDF.  options5 = occupied_space_weight, translation_weight,
// rotation_weight, use_nonmonotonic_steps, max_num_iterations.  summary5 = initial cost, final
// cost, successful steps, unsuccessful steps, termination (0 CONVERGENCE, 1 NO_CONVERGENCE,
// 2 FAILURE).  As oracle/ref_ceres_wrapper.cc, the successful steps leave out Ceres' iteration 0;
// a solve whose initial evaluation failed ran no iteration and keeps the Summary's own values.
void drv_tsdf_match(const uint16_t* tsd, const uint16_t* weight, int nx, int ny, double res,
                    double max_x, double max_y, float truncation_distance, float max_weight,
                    const double* options5, const double* target_xy, const double* init_xyt,
                    const float* xyz, int n, double* pose_xyt, double* summary5) {
  cm::ValueConversionTables tables;
  const auto grid = MakeTsdf(tsd, weight, nx, ny, res, max_x, max_y, truncation_distance,
                             max_weight, &tables);
  sm::proto::CeresScanMatcherOptions2D o;
  o.set_occupied_space_weight(options5[0]);
  o.set_translation_weight(options5[1]);
  o.set_rotation_weight(options5[2]);
  o.mutable_ceres_solver_options()->set_use_nonmonotonic_steps(options5[3] != 0.);
  o.mutable_ceres_solver_options()->set_max_num_iterations(static_cast<int>(options5[4]));
  o.mutable_ceres_solver_options()->set_num_threads(1);
  const sm::CeresScanMatcher2D matcher(o);
  const cartographer::sensor::PointCloud cloud = MakeCloud(xyz, n);
  cartographer::transform::Rigid2d pose;
  ceres::Solver::Summary summary;
  matcher.Match(Eigen::Vector2d(target_xy[0], target_xy[1]),
                cartographer::transform::Rigid2d({init_xyt[0], init_xyt[1]}, init_xyt[2]), cloud,
                *grid, &pose, &summary);
  pose_xyt[0] = pose.translation().x();
  pose_xyt[1] = pose.translation().y();
  pose_xyt[2] = pose.rotation().angle();
  const bool ran = !summary.iterations.empty();
  summary5[0] = summary.initial_cost;
  summary5[1] = summary.final_cost;
  summary5[2] = ran ? summary.num_successful_steps - 1 : summary.num_successful_steps;
  summary5[3] = summary.num_unsuccessful_steps;
  summary5[4] = summary.termination_type == ceres::CONVERGENCE      ? 0
                : summary.termination_type == ceres::NO_CONVERGENCE ? 1
                                                                    : 2;
}

}  // extern "C"
