// Loop closure over submaps that the 3D submap code itself built: simulated lidar sweeps are
// inserted at their true poses into ActiveSubmaps3D until several submaps are finished, and the
// reference's ConstraintBuilder3D (mapping/internal/constraints/constraint_builder_3d.cc, compiled
// UNMODIFIED) then searches every (node, finished submap) pair, local and global.
//
// The same file is linked four times (Makefile):
//   constraint_builder_3d_submaps_reference        the reference's submaps, inserter, fast and
//       Ceres matchers (over the stand-in solver of oracle/ref_shims/ceres)            (CPU)
//   constraint_builder_3d_submaps_mi355x           the reference's submaps and inserter, our
//       adapters (scan_matchers_3d_mi355x.cc) flattening the host grids                (MI355X)
//   constraint_builder_3d_submaps_resident_mi355x  resident/ submaps: both grids of every submap
//       are cmx_grid3d in HBM; the adapters build the fast matcher from them
//       (cmx_fast3d_create_from_grids) and refine on them; no host inserter is linked  (MI355X)
//   constraint_builder_3d_submaps_batched_resident_mi355x   the same submaps under batched/'s
//       ConstraintBuilder3D                                                            (MI355X)
// Each prints one line per constraint (constraint_builder_3d_main.cc's format) in a fixed order;
// tests/test_dropin_fast3d_resident.py compares them.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "cartographer/common/internal/testing/thread_pool_for_testing.h"
#include "cartographer/mapping/3d/submap_3d.h"
#include "cartographer/mapping/internal/3d/scan_matching/rotational_scan_matcher.h"
#include "cartographer/mapping/internal/constraints/constraint_builder_3d.h"

using namespace cartographer;
using mapping::constraints::ConstraintBuilder3D;

namespace {

struct Box {
  double lo[3], hi[3];
};

// The hall of local_trajectory_builder_3d_main.cc: 24 m x 16 m x 5 m with pillars, a gallery,
// crates, ledges and sills.
const Box kHall{{-6., -7., 0.}, {18., 9., 5.}};
std::vector<Box> Obstacles() {
  return {Box{{2., 2.5, 0.}, {3., 3.5, 5.}},      Box{{6.5, -3.5, 0.}, {7.5, -2., 5.}},
          Box{{-3., -4., 0.}, {-2.2, -3.2, 2.}},  Box{{10., 4., 0.}, {10.6, 7., 3.}},
          Box{{3.5, -6., 0.}, {5.5, -5.6, 1.5}},  Box{{-6., 6., 2.5}, {18., 9., 2.8}},
          Box{{12., -7., 0.}, {12.3, -1., 5.}},   Box{{14., 1., 0.}, {15.5, 2.5, 1.2}},
          Box{{-6., -7., 3.2}, {18., -6.6, 3.5}}, Box{{-6., -7., 1.4}, {18., -6.8, 1.6}},
          Box{{-6., -7., 2.2}, {-5.6, 9., 2.5}},  Box{{17.6, -7., 1.8}, {18., 9., 2.1}},
          Box{{17.7, -7., 3.6}, {18., 9., 3.8}},  Box{{-6., 8.7, 1.0}, {18., 9., 1.3}}};
}

// Where the ray origin + t * dir (t > 0) first meets a surface.
double Cast(const std::vector<Box>& obstacles, const double o[3], const double d[3]) {
  double best = 1e30;
  for (int a = 0; a != 3; ++a) {
    if (std::abs(d[a]) < 1e-12) continue;
    const double t = ((d[a] > 0. ? kHall.hi[a] : kHall.lo[a]) - o[a]) / d[a];
    if (t > 0. && t < best) best = t;
  }
  for (const Box& b : obstacles) {
    double t0 = 0., t1 = best;
    bool hit = true;
    for (int a = 0; a != 3 && hit; ++a) {
      if (std::abs(d[a]) < 1e-12) {
        hit = o[a] >= b.lo[a] && o[a] <= b.hi[a];
        continue;
      }
      double ta = (b.lo[a] - o[a]) / d[a], tb = (b.hi[a] - o[a]) / d[a];
      if (ta > tb) std::swap(ta, tb);
      t0 = std::max(t0, ta);
      t1 = std::min(t1, tb);
      hit = t0 <= t1;
    }
    if (hit && t0 > 1e-6 && t0 < best) best = t0;
  }
  return best;
}

struct Pose {
  double x, y, yaw;
};

// A slalom at 0.5 m/s, one sweep every 0.4 s; the lidar sits 2.5 m up.
constexpr double kHeight = 2.5;
Pose TruePose(int k) {
  const double s = 0.2 * k;
  return Pose{s, 1.2 * std::sin(0.35 * s), std::atan2(1.2 * 0.35 * std::cos(0.35 * s), 1.)};
}

struct Noise {   // a fixed stream in [-1, 1): the sweeps are the same in every build
  uint32_t state = 12345u;
  double Next() {
    state = state * 1664525u + 1013904223u;
    return (state >> 8) * (2. / 16777216.) - 1.;
  }
};

// One sweep in the sensor frame (level, yawed with the robot; no motion during the sweep).
sensor::PointCloud Sweep(const std::vector<Box>& obstacles, const Pose& at, int beams, int columns,
                         Noise* noise) {
  sensor::PointCloud cloud;
  const double cy = std::cos(at.yaw), sy = std::sin(at.yaw);
  const double origin[3] = {at.x, at.y, kHeight};
  for (int c = 0; c != columns; ++c) {
    for (int b = 0; b != beams; ++b) {
      const double bearing = -M_PI + 2. * M_PI * c / columns;
      const double elevation = (-15. + 30. * b / (beams - 1)) * M_PI / 180.;
      const double local[3] = {std::cos(elevation) * std::cos(bearing),
                               std::cos(elevation) * std::sin(bearing), std::sin(elevation)};
      const double dir[3] = {cy * local[0] - sy * local[1], sy * local[0] + cy * local[1], local[2]};
      const double range = Cast(obstacles, origin, dir) + 0.005 * noise->Next();
      cloud.push_back({Eigen::Vector3f(static_cast<float>(range * local[0]),
                                       static_cast<float>(range * local[1]),
                                       static_cast<float>(range * local[2]))});
    }
  }
  return cloud;
}

transform::Rigid3d LocalPose(const Pose& p) {
  return transform::Rigid3d(Eigen::Vector3d(p.x, p.y, kHeight),
                            Eigen::Quaterniond(Eigen::AngleAxisd(p.yaw, Eigen::Vector3d::UnitZ())));
}

// Every `stride`-th point, from `first` on: a deterministic reduction of the sweep.
sensor::PointCloud Every(const sensor::PointCloud& cloud, int first, int stride) {
  sensor::PointCloud out;
  for (size_t i = first; i < cloud.size(); i += stride) out.push_back(cloud[i]);
  return out;
}

mapping::proto::SubmapsOptions3D SubmapsOptions() {
  // trajectory_builder_3d.lua's submaps with 4 sweeps each, so that a short drive finishes several,
  // and hit / miss probabilities of 0.7 / 0.4: with lua's 0.55 / 0.49 a handful of sweeps leaves
  // every score below pose_graph.lua's min_score.
  mapping::proto::SubmapsOptions3D o;
  o.set_high_resolution(0.10);
  o.set_high_resolution_max_range(20.);
  o.set_low_resolution(0.45);
  o.set_num_range_data(4);
  auto* inserter = o.mutable_range_data_inserter_options();
  inserter->set_hit_probability(0.7);
  inserter->set_miss_probability(0.4);
  inserter->set_num_free_space_voxels(2);
  inserter->set_intensity_threshold(40.);
  return o;
}

// pose_graph.lua constraint_builder defaults (configuration_files/pose_graph.lua:17-63), every
// pair sampled.
mapping::constraints::proto::ConstraintBuilderOptions BuilderOptions() {
  mapping::constraints::proto::ConstraintBuilderOptions o;
  o.sampling_ratio_ = 1.;
  o.max_constraint_distance_ = 15.;
  o.min_score_ = 0.55;
  o.global_localization_min_score_ = 0.6;
  o.loop_closure_translation_weight_ = 1.1e4;
  o.loop_closure_rotation_weight_ = 1e5;
  o.log_matches_ = false;
  o.fast_3d_.set_branch_and_bound_depth(8);
  o.fast_3d_.set_full_resolution_depth(3);
  o.fast_3d_.set_min_rotational_score(0.77);
  o.fast_3d_.set_min_low_resolution_score(0.55);
  o.fast_3d_.set_linear_xy_search_window(5.);
  o.fast_3d_.set_linear_z_search_window(1.);
  o.fast_3d_.set_angular_search_window(15. * M_PI / 180.);
  o.ceres_3d_.add_occupied_space_weight(5.);
  o.ceres_3d_.add_occupied_space_weight(30.);
  o.ceres_3d_.set_translation_weight(10.);
  o.ceres_3d_.set_rotation_weight(1.);
  o.ceres_3d_.set_only_optimize_yaw(false);
  o.ceres_3d_.mutable_ceres_solver_options()->set_use_nonmonotonic_steps(false);
  o.ceres_3d_.mutable_ceres_solver_options()->set_max_num_iterations(10);
  o.ceres_3d_.mutable_ceres_solver_options()->set_num_threads(1);
  return o;
}

constexpr int kHistogramSize = 120;

}  // namespace

int main(int argc, char** argv) {
  const int num_sweeps = argc > 1 ? std::atoi(argv[1]) : 18;
  const int beams = argc > 2 ? std::atoi(argv[2]) : 16;
  const int columns = argc > 3 ? std::atoi(argv[3]) : 240;
  const std::vector<Box> obstacles = Obstacles();
  Noise noise;

  // Submaps: every sweep at its true pose into the active submaps (LocalTrajectoryBuilder3D's
  // InsertIntoSubmap without the matching); a submap is kept once its insertion is finished.
  mapping::ActiveSubmaps3D active(SubmapsOptions());
  std::vector<std::shared_ptr<const mapping::Submap3D>> finished;
  for (int k = 0; k != num_sweeps; ++k) {
    const Pose at = TruePose(k);
    const transform::Rigid3d local_pose = LocalPose(at);
    const sensor::PointCloud cloud = Sweep(obstacles, at, beams, columns, &noise);
    sensor::RangeData range_data{local_pose.translation().cast<float>(),
                                 sensor::TransformPointCloud(cloud, local_pose.cast<float>()), {}};
    // The histogram of the sweep in the gravity-aligned frame (level here: the sensor frame).
    const Eigen::VectorXf histogram =
        mapping::scan_matching::RotationalScanMatcher::ComputeHistogram(Every(cloud, 0, 4),
                                                                        kHistogramSize);
    const auto submaps = active.InsertData(range_data, local_pose.rotation(), histogram);
    if (submaps.front()->insertion_finished() &&
        (finished.empty() || finished.back() != submaps.front()))
      finished.push_back(submaps.front());
  }
  std::printf("finished submaps %zu\n", finished.size());
  if (finished.size() < 3) return 1;

  // Nodes: later sweeps from between the insertion poses, their global pose off the truth by
  // 0.25 m and 3 degrees (what an odometry drift leaves for loop closure to fix).
  std::vector<mapping::TrajectoryNode::Data> nodes;
  std::vector<transform::Rigid3d> node_poses;
  for (int k = 1; k < num_sweeps; k += 4) {
    Pose at = TruePose(k);
    at.x += 0.1;
    at.y -= 0.05;
    const sensor::PointCloud cloud = Sweep(obstacles, at, beams, columns, &noise);
    mapping::TrajectoryNode::Data data;
    data.gravity_alignment = Eigen::Quaterniond::Identity();
    data.high_resolution_point_cloud = Every(cloud, 1, 8);
    data.low_resolution_point_cloud = Every(cloud, 3, 24);
    data.rotational_scan_matcher_histogram =
        mapping::scan_matching::RotationalScanMatcher::ComputeHistogram(
            data.high_resolution_point_cloud, kHistogramSize);
    data.local_pose = LocalPose(at);
    nodes.push_back(data);
    node_poses.push_back(LocalPose(Pose{at.x + 0.2, at.y - 0.15, at.yaw + 3. * M_PI / 180.}));
  }

  common::testing::ThreadPoolForTesting thread_pool;
  ConstraintBuilder3D builder(BuilderOptions(), &thread_pool);
  for (size_t n = 0; n != nodes.size(); ++n) {
    for (size_t s = 0; s != finished.size(); ++s) {
      const mapping::SubmapId submap_id{0, static_cast<int>(s)};
      const mapping::NodeId node_id{0, static_cast<int>(n)};
      const transform::Rigid3d submap_pose = finished[s]->local_pose();
      builder.MaybeAddConstraint(submap_id, finished[s].get(), node_id, &nodes[n], node_poses[n],
                                 submap_pose);
      builder.MaybeAddGlobalConstraint(submap_id, finished[s].get(), node_id, &nodes[n],
                                       node_poses[n].rotation(), submap_pose.rotation());
    }
    builder.NotifyEndOfNode();
  }
  builder.WhenDone([&](const ConstraintBuilder3D::Result& result) {
    // (the builder's result order follows the thread pool, and a node's local and global
    // constraint to one submap share a tag: the lines are printed sorted)
    std::vector<std::string> lines;
    for (const auto& c : result) {
      const auto& t = c.pose.zbar_ij.translation();
      const auto& q = c.pose.zbar_ij.rotation();
      char line[256];
      std::snprintf(line, sizeof line,
                    "constraint submap %d node %d t %.9f %.9f %.9f q %.9f %.9f %.9f %.9f tag %d\n",
                    c.submap_id.submap_index, c.node_id.node_index, t.x(), t.y(), t.z(), q.w(),
                    q.x(), q.y(), q.z(), static_cast<int>(c.tag));
      lines.push_back(line);
    }
    std::sort(lines.begin(), lines.end());
    for (const std::string& line : lines) std::fputs(line.c_str(), stdout);
    std::printf("constraints %zu\n", result.size());
  });
  thread_pool.WaitUntilIdle();
  for (size_t s = 0; s != finished.size(); ++s)
    builder.DeleteScanMatcher(mapping::SubmapId{0, static_cast<int>(s)});
  return 0;
}
