// Submap2D / ActiveSubmaps2D with the probability grid RESIDENT IN HBM: the third build of the
// local-trajectory-builder test.  Same bookkeeping as shims_local/.../submap_2d.h (which restates
// mapping/2d/submap_2d.cc:70-76,140-155,159-183,221-236), but the grid is a cmx_grid2d:
// InsertRangeData is cmx_grid2d_insert_batch (the reference's ProbabilityGridRangeDataInserter2D +
// FinishUpdate on the device, bit for bit, for both active submaps in one call), Finish is
// cmx_grid2d_crop, and grid() hands the matchers a Grid2D that is also a
// dropin::DeviceGrid2DView, so that the adapters take the *_match_grid entry points: per scan
// only the point clouds cross PCIe.  With grid_type = "TSDF"
// the submap is a cmx_tsdf2d instead: cmx_tsdf2d_insert_batch (TSDFRangeDataInserter2D::Insert for
// both active submaps in one call, the scan sorted and its normals estimated once),
// cmx_tsdf2d_crop, and a TSDF2D view that is a dropin::DeviceTsdf2DView, so that the matchers take
// cmx_rt2d_match_tsdf_grid and cmx_ceres2d_match_tsdf_grid.
#ifndef DROPIN_RESIDENT_SUBMAP_2D_H_
#define DROPIN_RESIDENT_SUBMAP_2D_H_
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "Eigen/Core"
#include "absl/types/optional.h"
#include "cartographer/mapping/2d/grid_2d.h"
#include "cartographer/mapping/2d/map_limits.h"
#include "cartographer/mapping/internal/2d/tsdf_2d.h"
#include "cartographer/mapping/probability_values.h"
#include "cartographer/mapping/proto/submaps_options_2d.pb.h"
#include "cartographer/mapping/trajectory_node.h"
#include "cartographer/mapping/value_conversion_tables.h"
#include "cartographer/sensor/range_data.h"
#include "cartographer/transform/rigid_transform.h"
#include "device_grids.h"
namespace cartographer { namespace mapping {

inline void DropinCheckOk(cmx_status status, const char* what) {
  if (status == CMX_OK) return;
  std::fprintf(stderr, "Check failed: %s: %s (%s)\n", what, cmx_status_string(status),
               cmx_last_error());
  std::abort();
}

// What the matchers are handed: a Grid2D with the device grid's CURRENT limits and no cells of
// its own until SyncToHost() is asked for them (the test main's digest).
class DeviceGrid2D : public Grid2D, public dropin::DeviceGrid2DView {
 public:
  DeviceGrid2D(const cmx_grid2d* grid, const cmx_grid2d_limits& l, ValueConversionTables* tables)
      : Grid2D(MapLimits(l.resolution, Eigen::Vector2d(l.max_x, l.max_y),
                         CellLimits(l.num_x_cells, l.num_y_cells)),
               kMinCorrespondenceCost, kMaxCorrespondenceCost, tables),
        grid_(grid) {}
  const cmx_grid2d* device_grid() const override { return grid_; }
  GridType GetGridType() const override { return GridType::PROBABILITY_GRID; }
  std::unique_ptr<Grid2D> ComputeCroppedGrid() const override {
    std::fprintf(stderr, "DeviceGrid2D is cropped through its submap (cmx_grid2d_crop)\n");
    std::abort();
  }
  bool DrawToSubmapTexture(proto::SubmapQuery::Response::SubmapTexture*,
                           transform::Rigid3d) const override {
    return false;
  }
  void SyncToHost() {
    DropinCheckOk(cmx_grid2d_download(grid_, mutable_correspondence_cost_cells()->data()),
                  "cmx_grid2d_download");
  }
 private:
  const cmx_grid2d* grid_;
};

// The TSDF twin: a TSDF2D with the device grid's current limits and ranges; SyncToHost fills its
// tsd plane (the correspondence cost cells the digest reads).
class DeviceTsdf2D : public TSDF2D, public dropin::DeviceTsdf2DView {
 public:
  DeviceTsdf2D(const cmx_tsdf2d* grid, const cmx_grid2d_limits& l, float truncation_distance,
               float max_weight, ValueConversionTables* tables)
      : TSDF2D(MapLimits(l.resolution, Eigen::Vector2d(l.max_x, l.max_y),
                         CellLimits(l.num_x_cells, l.num_y_cells)),
               truncation_distance, max_weight, tables),
        grid_(grid) {}
  const cmx_tsdf2d* device_tsdf() const override { return grid_; }
  std::unique_ptr<Grid2D> ComputeCroppedGrid() const override {
    std::fprintf(stderr, "DeviceTsdf2D is cropped through its submap (cmx_tsdf2d_crop)\n");
    std::abort();
  }
  void SyncToHost() {
    DropinCheckOk(cmx_tsdf2d_download(grid_, mutable_correspondence_cost_cells()->data(), nullptr),
                  "cmx_tsdf2d_download");
  }
 private:
  const cmx_tsdf2d* grid_;
};

inline void DropinSyncGridToHost(const Grid2D& grid) {
  if (const auto* device = dynamic_cast<const DeviceGrid2D*>(&grid))
    const_cast<DeviceGrid2D*>(device)->SyncToHost();
  if (const auto* device = dynamic_cast<const DeviceTsdf2D*>(&grid))
    const_cast<DeviceTsdf2D*>(device)->SyncToHost();
}

class Submap2D {
 public:
  // tsdf_options == nullptr: a probability grid; otherwise a TSDF2D(limits, truncation_distance,
  // maximum_weight) as ActiveSubmaps2D::CreateGrid makes it (submap_2d.cc:205-218).
  Submap2D(const Eigen::Vector2f& origin, const MapLimits& limits, const int device,
           ValueConversionTables* conversion_tables,
           const proto::TSDFRangeDataInserterOptions2D* tsdf_options = nullptr)
      : local_pose_(transform::Rigid3d::Translation(
            Eigen::Vector3d(origin.x(), origin.y(), 0.))),
        conversion_tables_(conversion_tables) {
    const cmx_grid2d_limits l{limits.resolution(), limits.max().x(), limits.max().y(),
                              limits.cell_limits().num_x_cells, limits.cell_limits().num_y_cells,
                              kMinCorrespondenceCost, kMaxCorrespondenceCost};
    if (tsdf_options != nullptr) {
      truncation_distance_ = static_cast<float>(tsdf_options->truncation_distance());
      max_weight_ = static_cast<float>(tsdf_options->maximum_weight());
      DropinCheckOk(cmx_tsdf2d_create(&l, truncation_distance_, max_weight_, nullptr, nullptr,
                                      device, &device_tsdf_),
                    "cmx_tsdf2d_create");
    } else {
      DropinCheckOk(cmx_grid2d_create(&l, nullptr, device, &device_grid_), "cmx_grid2d_create");
    }
    RefreshView();
  }
  ~Submap2D() {
    if (device_grid_) cmx_grid2d_destroy(device_grid_);
    if (device_tsdf_) cmx_tsdf2d_destroy(device_tsdf_);
  }
  Submap2D(const Submap2D&) = delete;
  Submap2D& operator=(const Submap2D&) = delete;

  transform::Rigid3d local_pose() const { return local_pose_; }
  const Grid2D* grid() const {
    return device_tsdf_ ? static_cast<const Grid2D*>(tsdf_view_.get()) : view_.get();
  }
  int num_range_data() const { return num_range_data_; }
  bool insertion_finished() const { return insertion_finished_; }

  // The insertion itself is made by ActiveSubmaps2D::InsertRangeData, for both active submaps
  // in one cmx_grid2d_insert_batch (cmx_tsdf2d_insert_batch) call; these are
  // Submap2D::InsertRangeData's bookkeeping before and after it.
  cmx_grid2d* BeginInsertRangeData() {
    CHECK(!insertion_finished_);
    return device_grid_;
  }
  cmx_tsdf2d* BeginInsertTsdfRangeData() {
    CHECK(!insertion_finished_);
    return device_tsdf_;
  }
  void EndInsertRangeData() {
    RefreshView();
    ++num_range_data_;
  }
  static std::vector<float> Flatten(const sensor::PointCloud& cloud) {
    std::vector<float> xyz;
    xyz.reserve(3 * cloud.size());
    for (const sensor::RangefinderPoint& p : cloud) {
      xyz.push_back(p.position.x());
      xyz.push_back(p.position.y());
      xyz.push_back(p.position.z());
    }
    return xyz;
  }
  void Finish() {
    CHECK(!insertion_finished_);
    if (device_tsdf_) {
      DropinCheckOk(cmx_tsdf2d_crop(device_tsdf_), "cmx_tsdf2d_crop");
    } else {
      DropinCheckOk(cmx_grid2d_crop(device_grid_), "cmx_grid2d_crop");
    }
    RefreshView();
    insertion_finished_ = true;
  }

 private:
  // A new view only when the limits moved (the grid grew or was cropped): scans of a known area
  // leave the matchers' object alone.
  void RefreshView() {
    cmx_grid2d_limits l{};
    if (device_tsdf_) {
      DropinCheckOk(cmx_tsdf2d_get_limits(device_tsdf_, &l), "cmx_tsdf2d_get_limits");
      if (tsdf_view_ != nullptr && SameLimits(tsdf_view_->limits(), l)) return;
      tsdf_view_ = std::make_unique<DeviceTsdf2D>(device_tsdf_, l, truncation_distance_,
                                                  max_weight_, conversion_tables_);
      return;
    }
    DropinCheckOk(cmx_grid2d_get_limits(device_grid_, &l), "cmx_grid2d_get_limits");
    if (view_ != nullptr) {
      const MapLimits& have = view_->limits();
      if (have.cell_limits().num_x_cells == l.num_x_cells &&
          have.cell_limits().num_y_cells == l.num_y_cells && have.max().x() == l.max_x &&
          have.max().y() == l.max_y)
        return;
    }
    view_ = std::make_unique<DeviceGrid2D>(device_grid_, l, conversion_tables_);
  }
  static bool SameLimits(const MapLimits& have, const cmx_grid2d_limits& l) {
    return have.cell_limits().num_x_cells == l.num_x_cells &&
           have.cell_limits().num_y_cells == l.num_y_cells && have.max().x() == l.max_x &&
           have.max().y() == l.max_y;
  }
  const transform::Rigid3d local_pose_;
  ValueConversionTables* conversion_tables_;
  cmx_grid2d* device_grid_ = nullptr;
  cmx_tsdf2d* device_tsdf_ = nullptr;
  float truncation_distance_ = 0.f, max_weight_ = 0.f;
  std::unique_ptr<DeviceGrid2D> view_;
  std::unique_ptr<DeviceTsdf2D> tsdf_view_;
  int num_range_data_ = 0;
  bool insertion_finished_ = false;
};

class ActiveSubmaps2D {
 public:
  explicit ActiveSubmaps2D(const proto::SubmapsOptions2D& options) : options_(options) {
    const char* e = std::getenv("CMX_DEVICE");
    device_ = e ? std::atoi(e) : 0;
  }
  ActiveSubmaps2D(const ActiveSubmaps2D&) = delete;
  ActiveSubmaps2D& operator=(const ActiveSubmaps2D&) = delete;

  std::vector<std::shared_ptr<const Submap2D>> submaps() const {
    return std::vector<std::shared_ptr<const Submap2D>>(submaps_.begin(), submaps_.end());
  }
  std::vector<std::shared_ptr<const Submap2D>> InsertRangeData(
      const sensor::RangeData& range_data) {
    if (submaps_.empty() || submaps_.back()->num_range_data() == options_.num_range_data()) {
      AddSubmap(range_data.origin.head<2>());
    }
    if (tsdf()) {
      InsertIntoTsdfGrids(range_data);
    } else {
      InsertIntoProbabilityGrids(range_data);
    }
    if (submaps_.front()->num_range_data() == 2 * options_.num_range_data()) {
      submaps_.front()->Finish();
    }
    return submaps();
  }
 private:
  // The same range data into every active submap: one call, the points passed by the same
  // pointers, so that they cross PCIe once.
  void InsertIntoProbabilityGrids(const sensor::RangeData& range_data) {
    const proto::ProbabilityGridRangeDataInserterOptions2D& options =
        options_.probability_grid_range_data_inserter_options_2d();
    const float origin[2] = {range_data.origin.x(), range_data.origin.y()};
    const std::vector<float> returns = Submap2D::Flatten(range_data.returns);
    const std::vector<float> misses = Submap2D::Flatten(range_data.misses);
    std::vector<cmx_grid2d_insertion> insertions;
    for (auto& submap : submaps_) {
      insertions.push_back(cmx_grid2d_insertion{
          submap->BeginInsertRangeData(), origin, returns.data(),
          static_cast<int32_t>(range_data.returns.size()), misses.data(),
          static_cast<int32_t>(range_data.misses.size())});
    }
    DropinCheckOk(cmx_grid2d_insert_batch(insertions.data(),
                                          static_cast<int32_t>(insertions.size()),
                                          static_cast<float>(options.hit_probability()),
                                          static_cast<float>(options.miss_probability()),
                                          options.insert_free_space() ? 1 : 0),
                  "cmx_grid2d_insert_batch");
    for (auto& submap : submaps_) submap->EndInsertRangeData();
  }
  // TSDFRangeDataInserter2D::Insert (tsdf_range_data_inserter_2d.cc:131-240) likewise: the scan is
  // flattened once and passed by the same pointers, so that it is sorted and its normals are
  // estimated once for both submaps.
  void InsertIntoTsdfGrids(const sensor::RangeData& range_data) {
    const proto::TSDFRangeDataInserterOptions2D& o = options_.tsdf_range_data_inserter_options_2d();
    const float origin[3] = {range_data.origin.x(), range_data.origin.y(), range_data.origin.z()};
    const std::vector<float> returns = Submap2D::Flatten(range_data.returns);
    const cmx_tsdf_inserter_options_2d options{
        o.truncation_distance(), o.maximum_weight(), o.update_free_space() ? 1 : 0,
        o.normal_estimation_options().num_normal_samples(),
        o.normal_estimation_options().sample_radius(),
        o.project_sdf_distance_to_scan_normal() ? 1 : 0, o.update_weight_range_exponent(),
        o.update_weight_angle_scan_normal_to_ray_kernel_bandwidth(),
        o.update_weight_distance_cell_to_hit_kernel_bandwidth()};
    std::vector<cmx_tsdf2d_insertion> insertions;
    for (auto& submap : submaps_) {
      insertions.push_back(cmx_tsdf2d_insertion{
          submap->BeginInsertTsdfRangeData(), origin, returns.empty() ? nullptr : returns.data(),
          static_cast<int32_t>(range_data.returns.size())});
    }
    DropinCheckOk(cmx_tsdf2d_insert_batch(insertions.data(),
                                          static_cast<int32_t>(insertions.size()), &options),
                  "cmx_tsdf2d_insert_batch");
    for (auto& submap : submaps_) submap->EndInsertRangeData();
  }
  void AddSubmap(const Eigen::Vector2f& origin) {
    if (submaps_.size() >= 2) {
      CHECK(submaps_.front()->insertion_finished());
      submaps_.erase(submaps_.begin());
    }
    constexpr int kInitialSubmapSize = 100;
    const float resolution = options_.grid_options_2d().resolution();
    const double half = 0.5 * kInitialSubmapSize * resolution;
    submaps_.push_back(std::make_shared<Submap2D>(
        origin,
        MapLimits(resolution, Eigen::Vector2d(origin.x() + half, origin.y() + half),
                  CellLimits(kInitialSubmapSize, kInitialSubmapSize)),
        device_, &conversion_tables_,
        tsdf() ? &options_.tsdf_range_data_inserter_options_2d() : nullptr));
  }
  bool tsdf() const {
    return options_.grid_options_2d().grid_type() == proto::GridOptions2D_GridType_TSDF;
  }
  const proto::SubmapsOptions2D options_;
  int device_ = 0;
  std::vector<std::shared_ptr<Submap2D>> submaps_;
  ValueConversionTables conversion_tables_;
};
} }
#endif  // DROPIN_RESIDENT_SUBMAP_2D_H_
