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
// Host and device split.  The O(N) per-hit work runs on the host (tsdf_2d_host.h, shared with
// cmx_tsdf2d_insert_batch of tsdf_2d_batch.hip; the device pieces both share are in
// tsdf_2d_internal.h) with the libm the reference uses, so that it is bit-exact without restating any transcendental: GrowAsNeeded, the sort,
// EstimateNormals, the angle kernel, the range weight (std::pow), cos / sin of the normal and
// the superscaled ray ends.  Per cell, on the device: GetCellCenter, the distance to the origin
// (f32 norm, terms left to right), the projection on the normal, the clamp, GaussianKernel of
// the distance (a float of a double exp), the weighted average and the value converters.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "tsdf_2d_internal.h"

namespace cmx {
namespace {

// ---- device ----------------------------------------------------------------------
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
bool Contains(const cmx_tsdf2d& g, float px, float py) {
  return tsdf2d::Contains(tsdf2d::Limits{g.resolution, g.max_x, g.max_y, g.nx, g.ny}, px, py);
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
    RequireInserterOptions(options);
    const cmx_tsdf_inserter_options_2d& o = *options;
    WorkspaceLease ws(grid->device);

    // The sort, the normals and the per-hit part of InsertHit (tsdf_2d_host.h), then
    // GrowAsNeeded (:33-47) on the box they give.
    const tsdf2d::PreparedScan scan = tsdf2d::PrepareScan(origin_xyz, returns_xyz, num_returns, o);
    constexpr float kPadding = 1e-6f;
    GrowLimits(grid, *ws, scan.lo_x - kPadding * 1.f, scan.lo_y - kPadding * 1.f);
    GrowLimits(grid, *ws, scan.hi_x + kPadding * 1.f, scan.hi_y + kPadding * 1.f);

    // The ray table, straight into the upload buffer; hits closer than the truncation distance
    // add no ray.
    const int num_rays = static_cast<int>(scan.rays.size());
    TsdfRay* h_rays = ws->pinned[0].ReserveAs<TsdfRay>(std::max(num_rays, 1));
    const long outside = tsdf2d::BuildRays(
        scan, tsdf2d::Limits{grid->resolution, grid->max_x, grid->max_y, grid->nx, grid->ny},
        h_rays);
    CMX_REQUIRE(outside < 0,
                "range data leaves the grid limits after GrowAsNeeded (hit %ld; z != 0?)", outside);

    ++grid->version;
    if (num_rays == 0) {
      CMX_HIP(hipStreamSynchronize(ws->stream));
      return;
    }
    TsdfParams P = MakeParams(*grid);
    SetInsertion(&P, origin_xyz, o);
    P.error = ws->dev[2].ReserveAs<int>(1);
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
