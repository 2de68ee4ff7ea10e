/*
 * cartographer_mi355x.h — C ABI of the MI355X-native correlative scan matchers.
 *
 * Drop-in boundary for cartographer's scan-matching hot path.  Every entry
 * point replaces one method of the four reference classes (paths relative to
 * the reference tree, `SM2` = cartographer/mapping/internal/2d/scan_matching,
 * `SM3` = .../3d/scan_matching):
 *
 *   cmx_rt2d_match                 RealTimeCorrelativeScanMatcher2D::Match
 *                                  SM2/real_time_correlative_scan_matcher_2d.h:66-68, .cc:117-149
 *   cmx_rt2d_match_tsdf            the same method on a TSDF2D grid (.cc:38-59, :159-167)
 *   cmx_fast2d_create / _destroy   FastCorrelativeScanMatcher2D ctor / dtor
 *                                  SM2/fast_correlative_scan_matcher_2d.h:114-118, .cc:188-196
 *   cmx_fast2d_create_batch        the same ctor for many submaps in one call (the
 *                                  DispatchScanMatcherConstruction of a loaded map or of a first
 *                                  global constraint, constraints/constraint_builder_2d.cc:165-186)
 *   cmx_fast2d_match               FastCorrelativeScanMatcher2D::Match        .h:124-126, .cc:198-208
 *   cmx_fast2d_match_full_submap   FastCorrelativeScanMatcher2D::MatchFullSubmap .h:132-133, .cc:210-225
 *   cmx_fast2d_match_batch, cmx_fast2d_match_full_submap_batch
 *                                  the ConstraintBuilder2D fan-out of independent
 *                                  (node, submap) searches, constraints/constraint_builder_2d.cc:97-137
 *   cmx_ceres2d_match, cmx_ceres2d_match_grid, cmx_fast2d_refine_batch
 *                                  CeresScanMatcher2D::Match, SM2/ceres_scan_matcher_2d.cc:63-107
 *   cmx_ceres2d_match_tsdf, cmx_ceres2d_match_tsdf_grid, cmx_ceres2d_refine_batch_tsdf
 *                                  the same method on a TSDF2D (.cc:83-90, the GridType::TSDF case)
 *   cmx_ceres2d_match_grid_batch   the same method for many trajectories in one call, on resident
 *                                  probability grids and TSDF2Ds alike: the Ceres match of
 *                                  LocalTrajectoryBuilder2D::ScanMatch
 *                                  (mapping/internal/2d/local_trajectory_builder_2d.cc:64-107)
 *   cmx_ceres2d_tsdf_residuals     TSDFMatchCostFunction2D::Evaluate,
 *                                  SM2/tsdf_match_cost_function_2d.cc:40-66
 *   cmx_ceres3d_match, cmx_fast3d_refine_batch, cmx_fast3d_refine_pairs
 *                                  CeresScanMatcher3D::Match, SM3/ceres_scan_matcher_3d.cc:90-156
 *   cmx_rt3d_match                 RealTimeCorrelativeScanMatcher3D::Match
 *                                  SM3/real_time_correlative_scan_matcher_3d.h:47-50, .cc:34-53
 *   cmx_rt3d_match_grid_batch, cmx_ceres3d_match_grids_batch
 *                                  LocalTrajectoryBuilder3D::ScanMatch's two matchers
 *                                  (mapping/internal/3d/local_trajectory_builder_3d.cc:96-123) for
 *                                  many trajectories in one call each, on resident grids
 *   cmx_fast3d_*                   FastCorrelativeScanMatcher3D ctor / Match / MatchFullSubmap
 *                                  SM3/fast_correlative_scan_matcher_3d.h:75-101, .cc:112-170
 *   cmx_fast3d_create_batch        the same ctor for many submaps in one call (the
 *                                  DispatchScanMatcherConstruction of a loaded map or of a first
 *                                  global constraint, constraints/constraint_builder_3d.cc:170-198)
 *   cmx_grid2d_insert_batch        ProbabilityGridRangeDataInserter2D::Insert for many (grid, scan)
 *                                  pairs in one call: the two insertions of
 *                                  ActiveSubmaps2D::InsertRangeData (mapping/2d/submap_2d.cc:161-174),
 *                                  or those of many trajectories
 *   cmx_tsdf2d_insert_batch        TSDFRangeDataInserter2D::Insert for many (grid, scan) pairs in
 *                                  one call: the same two insertions on grid_type = "TSDF"
 *                                  (mapping/internal/2d/tsdf_range_data_inserter_2d.cc:131-240)
 *   cmx_grid3d_insert_batch        RangeDataInserter3D::Insert for many (grid, cloud) pairs in one
 *                                  call: the four insertions of ActiveSubmaps3D::InsertData
 *                                  (mapping/3d/submap_3d.cc:271-287,310-329), or those of many
 *                                  trajectories
 *   cmx_filter_batch               sensor::VoxelFilter / AdaptiveVoxelFilter for many clouds in one
 *                                  call, a filter's output handed to the next on the device: the
 *                                  filter chains of LocalTrajectoryBuilder2D / 3D::AddRangeData
 *                                  (sensor/internal/voxel_filter.cc), or those of many trajectories
 *   cmx_compute_histogram_batch    RotationalScanMatcher::ComputeHistogram for many clouds in one
 *                                  call: the histograms of the nodes that
 *                                  LocalTrajectoryBuilder3D::InsertIntoSubmap inserts
 *                                  (3d/local_trajectory_builder_3d.cc:399-404), for many trajectories
 *
 * Conventions
 *   - Plain C, POD only.  Host pointers are borrowed for the duration of the
 *     call; outputs are written to caller memory.  No exceptions cross the
 *     boundary: every function returns a cmx_status.
 *   - Reference CHECK failures (invalid options, null outputs) map to
 *     CMX_INVALID_ARGUMENT; "no match above min_score" is CMX_OK with
 *     *found == 0, exactly like the reference's `false` / `nullptr`.
 *   - There is NO CPU fallback: without a usable HIP device every compute
 *     entry point returns CMX_DEVICE_ERROR.
 *   - Matcher handles are immutable after creation and may be used from
 *     several host threads at once (the reference calls `Match*` concurrently
 *     from its thread pool, constraints/constraint_builder_2d.cc:97-111).
 */
#ifndef CARTOGRAPHER_MI355X_H_
#define CARTOGRAPHER_MI355X_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cmx_status {
  CMX_OK = 0,
  CMX_INVALID_ARGUMENT = 1,
  CMX_DEVICE_ERROR = 2,
  CMX_OUT_OF_MEMORY = 3,
  CMX_UNSUPPORTED = 4
} cmx_status;

/* transform::Rigid2d (transform/rigid_transform.h:34-87): translation + yaw. */
typedef struct cmx_pose2d { double x, y, theta; } cmx_pose2d;
/* transform::Rigid3d (rigid_transform.h:117-180): translation + quaternion (w,x,y,z). */
typedef struct cmx_pose3d { double t[3]; double q[4]; } cmx_pose3d;

/* mapping::MapLimits + the Grid2D cost range (mapping/2d/map_limits.h:40-96,
 * grid_2d.h:60-63).  `cells` passed next to it are Grid2D's
 * correspondence_cost_cells(): row-major nx*iy+ix, 0 = unknown. */
typedef struct cmx_grid2d_limits {
  double resolution;
  double max_x, max_y;
  int32_t num_x_cells, num_y_cells;
  float min_correspondence_cost, max_correspondence_cost;
} cmx_grid2d_limits;

/* proto::RealTimeCorrelativeScanMatcherOptions
 * (mapping/proto/scan_matching/real_time_correlative_scan_matcher_options.proto). */
typedef struct cmx_rt_options {
  double linear_search_window;
  double angular_search_window;
  double translation_delta_cost_weight;
  double rotation_delta_cost_weight;
} cmx_rt_options;

/* proto::FastCorrelativeScanMatcherOptions2D. */
typedef struct cmx_fast2d_options {
  double linear_search_window;
  double angular_search_window;
  int32_t branch_and_bound_depth;
} cmx_fast2d_options;

/* proto::FastCorrelativeScanMatcherOptions3D. */
typedef struct cmx_fast3d_options {
  int32_t branch_and_bound_depth;
  int32_t full_resolution_depth;
  double min_rotational_score;
  double min_low_resolution_score;
  double linear_xy_search_window;
  double linear_z_search_window;
  double angular_search_window;
} cmx_fast3d_options;

/* Work counters of one call (or summed over a batch). */
typedef struct cmx_match_stats {
  int64_t candidates_scored;  /* every scored candidate, all depths; real-time matchers: the SEARCH
                                 SPACE the call covered (what the reference scores) -- how much of it
                                 the device summed is coarse_candidates */
  int64_t coarse_candidates;  /* lowest-resolution (or exhaustive) candidates; real-time 2D with block
                                 bounds: the bounds evaluated + the candidates summed behind them.
                                 Fast 2D from branch_and_bound_depth 5 on: every lowest-resolution
                                 candidate is counted (here and in candidates_scored), three
                                 neighbouring rotations share ONE sum that bounds all three */
  int64_t nodes_expanded;     /* branch-and-bound nodes whose children were scored */
  int32_t num_scans;          /* rotated scans */
  int32_t expansion_launches; /* launches inside expansion_ms (0: none timed) */
  /* The three *_ms fields are recorded only after cmx_debug_set("timing", 1) (the event packets
     cost a latency-bound call ~15 % of its wall time); otherwise they are 0.  The switch is
     process-wide: set it while no call is in flight. */
  double device_ms;           /* HIP-event time of the call's device work */
  double dominant_kernel_ms;  /* HIP-event time of the lowest-resolution (or exhaustive) scoring kernel(s) */
  double expansion_ms;        /* HIP-event time of the level-synchronous branch-and-bound expansion
                                 launches (fast 2D: ExpandWaveKernel, fast 3D: Expand3DKernel) */
  int64_t expansion_nodes;    /* nodes those launches took from their frontiers */
  int64_t expansion_lookups;  /* grid lookups they issued (64 per wave-wide gather instruction) */
  int64_t refined_candidates; /* real-time matchers: candidates the integer bounds could not decide,
                                 re-summed with exact integers */
  int64_t finalists;          /* real-time matchers: candidates scored with the reference's own
                                 sequential f32 sum (the only ones whose score is returned) */
} cmx_match_stats;

/* One flattened HybridGrid voxel (mapping/3d/hybrid_grid.h:304-372 Iterator):
 * cell index and raw uint16 probability value (0 never appears). */
typedef struct cmx_voxel { int32_t x, y, z; uint16_t value; uint16_t pad; } cmx_voxel;

typedef struct cmx_fast2d cmx_fast2d;   /* opaque FastCorrelativeScanMatcher2D */
typedef struct cmx_fast3d cmx_fast3d;   /* opaque FastCorrelativeScanMatcher3D */

/* ---- library / device ------------------------------------------------- */
const char* cmx_version(void);
/* sizeof(cmx_match_stats) of the LIBRARY.  The struct has grown between versions (0.1: 88 bytes;
 * since 0.2: 104) and carries no size field: a caller built against another header passes a
 * buffer of the wrong size -- compare once at start-up ("ABI"). */
int32_t cmx_sizeof_match_stats(void);
const char* cmx_status_string(cmx_status s);
/* Last error text of the calling thread ("" if none). */
const char* cmx_last_error(void);
/* Number of HIP devices visible (0 when there is none). */
int32_t cmx_device_count(void);
/* Streams: by default every call runs on a library-owned stream of `device`.
 * A caller that owns a HIP stream (e.g. torch.cuda.current_stream()) can make
 * the calling thread's subsequent calls on `device` use it instead;
 * pass NULL to go back to the library stream. */
cmx_status cmx_set_stream(int32_t device, void* hip_stream);

/* ---- real-time 2D ------------------------------------------------------ */
/* Returns the best score (already weighted by the delta cost) in *score and
 * the pose in *pose_estimate; always succeeds for valid inputs
 * (reference: CHECK_GT(score, 0)). */
cmx_status cmx_rt2d_match(const cmx_rt_options* options, const cmx_grid2d_limits* limits,
                          const uint16_t* cells, const cmx_pose2d* initial_pose_estimate,
                          const float* point_cloud_xyz, int32_t num_points, int32_t device,
                          double* score, cmx_pose2d* pose_estimate, cmx_match_stats* stats);
/* TSDF2D branch of the same method (SM2/real_time_correlative_scan_matcher_2d.cc:38-59,
 * mapping/internal/2d/tsdf_2d.cc:88-98): `tsd_cells` are the grid's
 * correspondence_cost_cells, `weight_cells` its weight plane (both uint16,
 * 0 = unknown, bit 15 = update marker), `truncation_distance` / `max_weight`
 * the TSDValueConverter ranges.  A TSDF may score 0 everywhere; the first
 * candidate then wins, as std::max_element does in the reference. */
cmx_status cmx_rt2d_match_tsdf(const cmx_rt_options* options, const cmx_grid2d_limits* limits,
                               const uint16_t* tsd_cells, const uint16_t* weight_cells,
                               float truncation_distance, float max_weight,
                               const cmx_pose2d* initial_pose_estimate,
                               const float* point_cloud_xyz, int32_t num_points, int32_t device,
                               double* score, cmx_pose2d* pose_estimate, cmx_match_stats* stats);

/* RealTimeCorrelativeScanMatcher2D::ScoreCandidates, the method the reference keeps "visible for
 * testing" (SM2/real_time_correlative_scan_matcher_2d.h:70-76, .cc:147-175), so that its unit
 * tests run against the device: ANY candidate list over caller-made discrete scans.
 * cmx_candidate2d mirrors Candidate2D (SM2/correlative_scan_matcher_2d.h:69-98): the caller fills
 * everything but `score`.  discrete_scans_xy holds the (x, y) cell indices of all scans back to
 * back, scan s being points scan_begin[s] .. scan_begin[s + 1] - 1.  weight_cells == NULL: a
 * ProbabilityGrid; otherwise the TSDF2D planes as in cmx_rt2d_match_tsdf. */
typedef struct cmx_candidate2d {
  int32_t scan_index, x_index_offset, y_index_offset;
  float score;                 /* out: weighted by the delta costs */
  double x, y, orientation;
} cmx_candidate2d;
cmx_status cmx_rt2d_score_candidates(const cmx_rt_options* options,
                                     const cmx_grid2d_limits* limits, const uint16_t* cells,
                                     const uint16_t* weight_cells, float truncation_distance,
                                     float max_weight, const int32_t* discrete_scans_xy,
                                     const int32_t* scan_begin, int32_t num_scans,
                                     cmx_candidate2d* candidates, int32_t num_candidates,
                                     int32_t device);

/* ---- device-resident probability grid ------------------ */
/* The active submap's ProbabilityGrid kept in HBM: LocalTrajectoryBuilder2D's per-scan
 * pair Match() -> InsertRangeData() (mapping/internal/2d/local_trajectory_builder_2d.cc:
 * 78-80, :288-289) then moves only the scan across PCIe.
 *   cmx_grid2d_create     ProbabilityGrid(limits) (all unknown) or a copy of `cells`; the cost
 *                         bounds of `limits` are ignored, the grid always has the probability
 *                         range (so cmx_fast2d_create_from_grid never meets another one).
 *                         `cells` are those of a grid between two updates, values 0 .. 32767: a
 *                         cell with bit 15 (the update marker) set is refused with
 *                         CMX_INVALID_ARGUMENT, cmx_last_error naming the cell, before the device
 *                         is touched -- an insertion could not tell such a marker from its own
 *   cmx_grid2d_insert     ProbabilityGridRangeDataInserter2D::Insert + FinishUpdate
 *                         (mapping/2d/probability_grid_range_data_inserter_2d.cc:33-96,
 *                          mapping/internal/2d/ray_to_pixel_mask.cc:34-156); grows the
 *                         limits like GrowAsNeeded / Grid2D::GrowLimits. Points are in the
 *                         map frame (range data already transformed), xyz triples.
 *   cmx_grid2d_insert_batch  the same for many (grid, range data) pairs in one call (below)
 *   cmx_grid2d_crop       grid = grid->ComputeCroppedGrid(): what Submap2D::Finish does before the
 *                         loop-closure matcher is built (mapping/2d/submap_2d.cc:146-149,
 *                         mapping/2d/probability_grid.cc:90-106, grid_2d.cc:104-114)
 *   cmx_rt2d_match_grid   RealTimeCorrelativeScanMatcher2D::Match on that grid
 *   cmx_fast2d_create_from_grid  FastCorrelativeScanMatcher2D of the (finished) grid */
typedef struct cmx_grid2d cmx_grid2d;
cmx_status cmx_grid2d_create(const cmx_grid2d_limits* limits, const uint16_t* cells_or_null,
                             int32_t device, cmx_grid2d** out);
void cmx_grid2d_destroy(cmx_grid2d* grid);
cmx_status cmx_grid2d_get_limits(const cmx_grid2d* grid, cmx_grid2d_limits* limits);
cmx_status cmx_grid2d_download(const cmx_grid2d* grid, uint16_t* cells);
cmx_status cmx_grid2d_crop(cmx_grid2d* grid);
cmx_status cmx_grid2d_insert(cmx_grid2d* grid, const float* origin_xy, const float* returns_xyz,
                             int32_t num_returns, const float* misses_xyz, int32_t num_misses,
                             float hit_probability, float miss_probability,
                             int32_t insert_free_space);

/* One insertion of a cmx_grid2d_insert_batch call: the arguments of cmx_grid2d_insert that differ
 * from insertion to insertion. */
typedef struct cmx_grid2d_insertion {
  cmx_grid2d* grid;
  const float* origin_xy;      /* 2 floats */
  const float* returns_xyz;    /* num_returns xyz triples, map frame */
  int32_t num_returns;
  const float* misses_xyz;
  int32_t num_misses;
} cmx_grid2d_insertion;

/* cmx_grid2d_insert(insertions[i] ...) for i = 0 .. num_insertions - 1 in list order, bit for bit
 * (cells, limits and the staleness of the real-time matcher's cached image), in shared launches:
 * what ActiveSubmaps2D::InsertRangeData does to its two submaps, or a fleet to the active submaps of
 * every robot after one cmx_rt2d_match_grid_batch.
 *   - A grid may appear several times: its insertions apply in list order.  The r-th insertion of
 *     every grid forms round r; a round is three launches (hits, rays, marker clearing) over all
 *     its insertions, so the number of launches grows with the most insertions any one grid has,
 *     not with the number of grids.  One synchronisation per call.
 *   - Equal returns_xyz (or misses_xyz) pointers are the same scan and cross PCIe once per call;
 *     their counts must be equal too.
 *   - An insertion may have no returns, no misses, or neither (the grid still grows around the
 *     origin), as in the single call.  One set of probabilities holds for the whole call.
 *   - Every argument check of the single call is made for every insertion before the device is
 *     touched: CMX_INVALID_ARGUMENT names `insertion <index>` in cmx_last_error and no grid has
 *     changed.  num_insertions < 1, null `insertions`, a null grid or origin and grids on different
 *     devices are invalid.
 *   - Every grid is grown once, to the size its last insertion needs, before anything is inserted.
 *     When a device allocation fails there (CMX_OUT_OF_MEMORY), no grid has changed: neither its
 *     size nor its cells, and no insertion has been applied. */
cmx_status cmx_grid2d_insert_batch(const cmx_grid2d_insertion* insertions,
                                   int32_t num_insertions, float hit_probability,
                                   float miss_probability, int32_t insert_free_space);

cmx_status cmx_rt2d_match_grid(const cmx_rt_options* options, const cmx_grid2d* grid,
                               const cmx_pose2d* initial_pose_estimate,
                               const float* point_cloud_xyz, int32_t num_points, double* score,
                               cmx_pose2d* pose_estimate, cmx_match_stats* stats);

/* `num_matches` independent real-time matches (one per trajectory / robot: scan i against
 * grid i around pose i) in one set of kernel launches.  A single match occupies 81 of the
 * chip's 8192 wave slots and is bound by the latency of its sequential f32 sums; batching
 * is what fills the machine. */
cmx_status cmx_rt2d_match_grid_batch(const cmx_rt_options* options,
                                     const cmx_grid2d* const* grids, int32_t num_matches,
                                     const cmx_pose2d* initial_pose_estimates,
                                     const float* const* point_clouds_xyz,
                                     const int32_t* num_points, double* scores,
                                     cmx_pose2d* pose_estimates, cmx_match_stats* stats);

/* The same batch with the scans already in HBM (cmx_cloud_upload, declared below): per call
 * only the initial poses, the per-scan rotation tables (libm, host) and the results cross PCIe.
 * The grid's staged image (quantised cells + halo, what the kernel copies into LDS) is kept
 * with the cmx_grid2d and rebuilt only after the grid changed. */
typedef struct cmx_cloud cmx_cloud;
cmx_status cmx_rt2d_match_grid_batch_resident(const cmx_rt_options* options,
                                              const cmx_grid2d* const* grids,
                                              int32_t num_matches,
                                              const cmx_pose2d* initial_pose_estimates,
                                              const cmx_cloud* const* clouds, double* scores,
                                              cmx_pose2d* pose_estimates, cmx_match_stats* stats);

/* ---- device-resident TSDF2D ------------------------------------------------ */
/* The active submap of grid_type = "TSDF" (mapping/2d/submap_2d.cc:58-60, :183-186) kept in
 * HBM: the tsd plane (Grid2D's correspondence_cost_cells) and the weight plane, both uint16
 * row-major nx*iy+ix, 0 = unknown.
 *   cmx_tsdf2d_create     TSDF2D(limits, truncation_distance, max_weight) (all unknown) or a
 *                         copy of the two planes (mapping/internal/2d/tsdf_2d.cc:24-47).  The
 *                         two values are the grid's TSDValueConverter, separate from the
 *                         inserter's options.  A cell whose tsd value carries the update marker
 *                         (bit 15) is never updated and keeps the bit, as in the reference.
 *   cmx_tsdf2d_get_limits the MapLimits; the cost range is [-truncation, truncation]
 *   cmx_tsdf2d_insert     TSDFRangeDataInserter2D::Insert (mapping/internal/2d/
 *                         tsdf_range_data_inserter_2d.cc:131-240, normal_estimation_2d.cc:23-110);
 *                         grows the limits like GrowAsNeeded / Grid2D::GrowLimits.  Points are
 *                         in the map frame, xyz triples; `origin_xyz` is the sensor origin.
 *                         Range data whose rays leave the grown limits (z != 0 shortens the
 *                         box GrowAsNeeded builds from 3D directions) is CMX_INVALID_ARGUMENT.
 *   cmx_tsdf2d_insert_batch  the same for many (grid, range data) pairs in one call (below)
 *   cmx_tsdf2d_crop       grid = grid->ComputeCroppedGrid() (tsdf_2d.cc:118-135)
 *   cmx_rt2d_match_tsdf_grid  cmx_rt2d_match_tsdf with the planes read from HBM
 *   cmx_fast2d_create_from_tsdf  FastCorrelativeScanMatcher2D of the tsd plane over the cost
 *                         range [-truncation, truncation]; truncation > 1 is
 *                         CMX_INVALID_ARGUMENT (see cmx_fast2d_create) */
/* proto::TSDFRangeDataInserterOptions2D with its proto::NormalEstimationOptions2D
 * (num_normal_samples > 0 and sample_radius > 0, normal_estimation_2d.cc:64-74). */
typedef struct cmx_tsdf_inserter_options_2d {
  double truncation_distance;
  double maximum_weight;
  int32_t update_free_space;
  int32_t num_normal_samples;
  double sample_radius;
  int32_t project_sdf_distance_to_scan_normal;
  int32_t update_weight_range_exponent;
  double update_weight_angle_scan_normal_to_ray_kernel_bandwidth;
  double update_weight_distance_cell_to_hit_kernel_bandwidth;
} cmx_tsdf_inserter_options_2d;

typedef struct cmx_tsdf2d cmx_tsdf2d;
cmx_status cmx_tsdf2d_create(const cmx_grid2d_limits* limits, float truncation_distance,
                             float max_weight, const uint16_t* tsd_cells_or_null,
                             const uint16_t* weight_cells_or_null, int32_t device,
                             cmx_tsdf2d** out);
void cmx_tsdf2d_destroy(cmx_tsdf2d* grid);
cmx_status cmx_tsdf2d_get_limits(const cmx_tsdf2d* grid, cmx_grid2d_limits* limits);
cmx_status cmx_tsdf2d_download(const cmx_tsdf2d* grid, uint16_t* tsd_cells,
                               uint16_t* weight_cells);
cmx_status cmx_tsdf2d_insert(cmx_tsdf2d* grid, const float* origin_xyz, const float* returns_xyz,
                             int32_t num_returns, const cmx_tsdf_inserter_options_2d* options);
cmx_status cmx_tsdf2d_crop(cmx_tsdf2d* grid);

/* One insertion of a cmx_tsdf2d_insert_batch call: the arguments of cmx_tsdf2d_insert that differ
 * from insertion to insertion. */
typedef struct cmx_tsdf2d_insertion {
  cmx_tsdf2d* grid;
  const float* origin_xyz;     /* 3 floats */
  const float* returns_xyz;    /* num_returns xyz triples, map frame */
  int32_t num_returns;
} cmx_tsdf2d_insertion;

/* cmx_tsdf2d_insert(insertions[i] ..., options) for i = 0 .. num_insertions - 1 in list order, bit
 * for bit (both planes, the limits and the staleness of the cached matcher images), in shared
 * launches: what ActiveSubmaps2D::InsertRangeData does to its two submaps on grid_type = "TSDF",
 * or a fleet to the active submaps of every robot after one cmx_rt2d_match_tsdf_grid_batch.
 *   - A grid may appear several times: its insertions apply in list order.  The r-th insertion of
 *     every grid forms round r; a round is two launches (owner, apply) over all its insertions, so
 *     the number of launches grows with the most insertions any one grid has, not with the number
 *     of grids.  One upload and one synchronisation per call.
 *   - Insertions with equal returns_xyz pointers and equal origin values are the same scan: it is
 *     sorted and its normals are estimated once per call (distinct scans in parallel on the host).
 *     Equal pointers must come with equal counts.
 *   - An insertion may have no returns (the grid still grows around the origin), or only returns
 *     closer than the truncation distance (no rays; the hits are still sorted and feed the
 *     normals), as in the single call.  One set of options holds for the whole call.
 *   - All or nothing, which is stricter than the single call: every check of the single call is
 *     made for every insertion before the device is touched, against the limits its grid has at
 *     that insertion -- null pointers and counts, num_normal_samples and sample_radius, a grid
 *     beyond 2^30 cells, range data that leaves the limits after GrowAsNeeded.
 *     CMX_INVALID_ARGUMENT names `insertion <index>` in cmx_last_error and no grid has changed,
 *     neither its size nor its cells.  num_insertions < 1, null `insertions`, a null grid or origin
 *     and grids on different devices are invalid.
 *   - Every grid is grown once, to the size its last insertion needs, before anything is inserted.
 *     When a device allocation fails there (CMX_OUT_OF_MEMORY), no grid has changed: neither its
 *     size nor its cells, and no insertion has been applied. */
cmx_status cmx_tsdf2d_insert_batch(const cmx_tsdf2d_insertion* insertions,
                                   int32_t num_insertions,
                                   const cmx_tsdf_inserter_options_2d* options);

cmx_status cmx_rt2d_match_tsdf_grid(const cmx_rt_options* options, const cmx_tsdf2d* grid,
                                    const cmx_pose2d* initial_pose_estimate,
                                    const float* point_cloud_xyz, int32_t num_points,
                                    double* score, cmx_pose2d* pose_estimate,
                                    cmx_match_stats* stats);
/* `num_matches` independent real-time matches on resident TSDF2Ds in one set of kernel
 * launches: match i is exactly cmx_rt2d_match_tsdf_grid(options, grids[i],
 * &initial_pose_estimates[i], cloud i, ...), score and pose bit for bit.  All grids (and clouds)
 * of a call live on one device.  The entries run the one-thread-per-candidate batch kernels:
 * `stats` sums the matches, candidates_scored is the search space, coarse_candidates and
 * finalists equal it (every candidate is summed with the reference's own f32 sums and stands
 * for the host's first-maximum rule) and refined_candidates is 0.  Debug only (switch
 * rt2d_tsdf_batch_bulk): an integer bulk pass over two quantised byte images kept with the
 * cmx_tsdf2d; then coarse_candidates is what that pass summed, refined_candidates the
 * candidates evaluated with the f32 sums and finalists those weighted on the host. */
cmx_status cmx_rt2d_match_tsdf_grid_batch(const cmx_rt_options* options,
                                          const cmx_tsdf2d* const* grids, int32_t num_matches,
                                          const cmx_pose2d* initial_pose_estimates,
                                          const float* const* point_clouds_xyz,
                                          const int32_t* num_points, double* scores,
                                          cmx_pose2d* pose_estimates, cmx_match_stats* stats);
cmx_status cmx_rt2d_match_tsdf_grid_batch_resident(const cmx_rt_options* options,
                                                   const cmx_tsdf2d* const* grids,
                                                   int32_t num_matches,
                                                   const cmx_pose2d* initial_pose_estimates,
                                                   const cmx_cloud* const* clouds, double* scores,
                                                   cmx_pose2d* pose_estimates,
                                                   cmx_match_stats* stats);
cmx_status cmx_fast2d_create_from_tsdf(const cmx_fast2d_options* options, const cmx_tsdf2d* grid,
                                       cmx_fast2d** out);

/* ---- fast 2D (branch and bound) ---------------------------------------- */
/* Uploads the grid and builds the PrecomputationGridStack2D on `device`
 * (SM2/fast_correlative_scan_matcher_2d.cc:171-186).
 * This call and _from_tsdf above take any cost range with
 * min_correspondence_cost < max_correspondence_cost <= 1 (_from_grid always gets the probability
 * range of a cmx_grid2d).  A range with
 * max_correspondence_cost > 1 (a TSDF2D whose truncation distance exceeds 1 m) is
 * CMX_INVALID_ARGUMENT: scores go down to 1 - max_correspondence_cost, and the search cannot
 * represent negative scores.  Scores above 1 are fine (a TSDF's perfect hit is 1.00118 at
 * truncation distance 0.3), and so is a negative min_score. */
cmx_status cmx_fast2d_create(const cmx_fast2d_options* options, const cmx_grid2d_limits* limits,
                             const uint16_t* cells, int32_t device, cmx_fast2d** out);
cmx_status cmx_fast2d_create_from_grid(const cmx_fast2d_options* options, const cmx_grid2d* grid,
                                       cmx_fast2d** out);
/* One submap of a cmx_fast2d_create_batch call.  Exactly one source is set:
 * (limits, cells) = the arguments of cmx_fast2d_create (host memory), or grid
 * (cmx_fast2d_create_from_grid), or tsdf (cmx_fast2d_create_from_tsdf). */
typedef struct cmx_fast2d_source {
  const cmx_grid2d_limits* limits;
  const uint16_t* cells;
  const cmx_grid2d* grid;
  const cmx_tsdf2d* tsdf;
} cmx_fast2d_source;
/* The matchers of `num_sources` submaps on `device` -- a loaded map, or the first global
 * constraint of a node against every finished submap (constraints/constraint_builder_2d.cc:113-137,
 * :165-186) -- in ONE call: out[k] is, bit for bit, the matcher the single create of sources[k]
 * returns (sources may differ in kind, size, resolution, origin and cost range; `options` holds
 * for all, as a ConstraintBuilder2D has one set).  The number of launches does not grow with
 * num_sources: one chain of launches builds the whole list (a list too large for the scratch
 * memory, a launch grid or a 32-bit count: consecutive chains), one synchronisation per chain.
 * Every matcher owns its memory, is used like any other and is destroyed with
 * cmx_fast2d_destroy, in any order; the sources are free once the call returns.
 * All or nothing: every argument check of the single creates is made for every source before
 * the device is touched -- a failing one is CMX_INVALID_ARGUMENT and cmx_last_error names the
 * index of the source; so are num_sources < 1, a source with no kind or more than one kind set,
 * and a resident source on another device.  On any error (a device allocation that fails
 * half-way included) nothing is left allocated and every out[k] is NULL. */
cmx_status cmx_fast2d_create_batch(const cmx_fast2d_options* options,
                                   const cmx_fast2d_source* sources, int32_t num_sources,
                                   int32_t device, cmx_fast2d** out /* num_sources */);
void cmx_fast2d_destroy(cmx_fast2d* matcher);

cmx_status cmx_fast2d_match(const cmx_fast2d* matcher, const cmx_pose2d* initial_pose_estimate,
                            const float* point_cloud_xyz, int32_t num_points, float min_score,
                            int32_t* found, float* score, cmx_pose2d* pose_estimate,
                            cmx_match_stats* stats);
cmx_status cmx_fast2d_match_full_submap(const cmx_fast2d* matcher, const float* point_cloud_xyz,
                                        int32_t num_points, float min_score, int32_t* found,
                                        float* score, cmx_pose2d* pose_estimate,
                                        cmx_match_stats* stats);
/* One scan against `num_matchers` submaps (all on the same device), results
 * per submap; `stats` is the sum over the batch. */
cmx_status cmx_fast2d_match_full_submap_batch(const cmx_fast2d* const* matchers,
                                              int32_t num_matchers, const float* point_cloud_xyz,
                                              int32_t num_points, float min_score,
                                              int32_t* found, float* scores,
                                              cmx_pose2d* pose_estimates, cmx_match_stats* stats);

/* The general batch behind a ConstraintBuilder2D front
 * (constraints/constraint_builder_2d.cc:77-137, :194-236): one node's scan against many
 * submaps in ONE device batch, each entry either a windowed Match around its own
 * initial pose (match_full_submap[i] == 0: MaybeAddConstraint) or a MatchFullSubmap
 * (!= 0: MaybeAddGlobalConstraint), each with its own acceptance threshold
 * (min_score / global_localization_min_score). */
cmx_status cmx_fast2d_match_batch(const cmx_fast2d* const* matchers, int32_t num_matchers,
                                  const cmx_pose2d* initial_pose_estimates,
                                  const int32_t* match_full_submap, const float* min_scores,
                                  const float* point_cloud_xyz, int32_t num_points, int32_t* found,
                                  float* scores, cmx_pose2d* pose_estimates,
                                  cmx_match_stats* stats);

/* Device-resident variant for throughput measurement: the point cloud is
 * uploaded once, repeated matches touch no host buffer except the results. */
cmx_status cmx_cloud_upload(const float* point_cloud_xyz, int32_t num_points, int32_t device,
                            cmx_cloud** out);
void cmx_cloud_destroy(cmx_cloud* cloud);
cmx_status cmx_fast2d_match_full_submap_batch_resident(
    const cmx_fast2d* const* matchers, int32_t num_matchers, const cmx_cloud* cloud,
    float min_score, int32_t* found, float* scores, cmx_pose2d* pose_estimates,
    cmx_match_stats* stats);

/* ---- Ceres refinement, 2D -------------------------------- */
/* proto::CeresScanMatcherOptions2D + the three ceres_solver_options cartographer sets
 * (mapping/proto/scan_matching/ceres_scan_matcher_options_2d.proto,
 * common/internal/ceres_solver_options.cc:38-45; num_threads has no meaning here). */
typedef struct cmx_ceres2d_options {
  double occupied_space_weight;
  double translation_weight;
  double rotation_weight;
  int32_t use_nonmonotonic_steps;
  int32_t max_num_iterations;
} cmx_ceres2d_options;
/* The fields of ceres::Solver::Summary the callers and tests read. */
typedef struct cmx_ceres_summary {
  double initial_cost, final_cost;
  int32_t num_successful_steps, num_unsuccessful_steps;
  int32_t termination;   /* 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE */
  int32_t reserved;
} cmx_ceres_summary;
/* CeresScanMatcher2D::Match (SM2/ceres_scan_matcher_2d.h:51-56, .cc:63-107) on a probability
 * grid: bicubic occupied-space residuals + translation / rotation delta residuals, Ceres's
 * trust-region Levenberg-Marquardt with its default options.  `cells` as in cmx_rt2d_match. */
cmx_status cmx_ceres2d_match(const cmx_ceres2d_options* options, const cmx_grid2d_limits* limits,
                             const uint16_t* cells, const double* target_translation_xy,
                             const cmx_pose2d* initial_pose_estimate, const float* point_cloud_xyz,
                             int32_t num_points, int32_t device, cmx_pose2d* pose_estimate,
                             cmx_ceres_summary* summary);
/* The same on a grid resident in HBM: LocalTrajectoryBuilder2D::ScanMatch's
 * real-time match -> Ceres match pair (local_trajectory_builder_2d.cc:78-107) without the
 * grid crossing PCIe. */
cmx_status cmx_ceres2d_match_grid(const cmx_ceres2d_options* options, const cmx_grid2d* grid,
                                  const double* target_translation_xy,
                                  const cmx_pose2d* initial_pose_estimate,
                                  const float* point_cloud_xyz, int32_t num_points,
                                  cmx_pose2d* pose_estimate, cmx_ceres_summary* summary);
/* ConstraintBuilder2D::ComputeConstraint's refinement (constraints/constraint_builder_2d.cc:
 * 245-249) for the results of cmx_fast2d_match_batch, one launch for the whole batch, each
 * against the grid its matcher keeps in HBM: entry i refines pose_estimates_in[i] with target
 * translation pose_estimates_in[i].{x,y}; entries with found[i] == 0 (found may be NULL) are
 * passed through.  The matchers' grids are probability grids, refined with the occupied-space
 * cost; callers with TSDF submaps use cmx_ceres2d_refine_batch_tsdf. */
cmx_status cmx_fast2d_refine_batch(const cmx_ceres2d_options* options,
                                   const cmx_fast2d* const* matchers, int32_t num_matchers,
                                   const int32_t* found, const cmx_pose2d* pose_estimates_in,
                                   const float* point_cloud_xyz, int32_t num_points,
                                   cmx_pose2d* pose_estimates_out, cmx_ceres_summary* summaries);

/* ---- Ceres refinement on a TSDF2D ---------------------------------------------------------- */
/* CeresScanMatcher2D::Match with grid_type = "TSDF" (SM2/ceres_scan_matcher_2d.cc:83-90): the
 * point residuals are TSDFMatchCostFunction2D (SM2/tsdf_match_cost_function_2d.cc:40-66,
 * bilinear InterpolatedTSDF2D, SM2/interpolated_tsdf_2d.h:42-125), r_i = n s C_i w_i / sum_j w_j
 * with s = occupied_space_weight / sqrt(n); translation / rotation delta residuals and solver as
 * in cmx_ceres2d_match.  The planes and ranges are those of cmx_rt2d_match_tsdf.
 *   - When every interpolated weight is 0 the cost function fails.  A failed initial evaluation
 *     ends the solve with termination 2 (FAILURE): the pose is the initial estimate and the
 *     summary keeps ceres::Solver::Summary's initial values (costs -1, both step counts -1).
 *     A failed candidate evaluation costs DBL_MAX and is an unsuccessful step.
 *   - num_points == 0 is accepted (point_cloud_xyz may then be NULL): the reference's functor
 *     fails on an empty cloud, so the solve ends with FAILURE as above.
 *   cmx_ceres2d_match_tsdf        the planes are uploaded for the call
 *   cmx_ceres2d_match_tsdf_grid   the planes of a resident grid are read in place:
 *                                 LocalTrajectoryBuilder2D's pair after cmx_rt2d_match_tsdf_grid
 *   cmx_ceres2d_refine_batch_tsdf ConstraintBuilder2D's refinement against finished TSDF
 *                                 submaps, the contract of cmx_fast2d_refine_batch: target =
 *                                 pose_estimates_in[i].{x,y}, found[i] == 0 passes through
 *                                 (found may be NULL), one launch per device the grids live on
 *   cmx_ceres2d_tsdf_residuals    TSDFMatchCostFunction2D::Evaluate at `pose` (x, y, theta) with
 *                                 `residual_scaling_factor` = s: residuals[n] and the row-major
 *                                 n x 3 Jacobian, *valid = 0 where the functor returns false
 *                                 (then residuals / jacobian are not written; n == 0 gives 0),
 *                                 kept visible for testing like cmx_rt2d_score_candidates. */
cmx_status cmx_ceres2d_match_tsdf(const cmx_ceres2d_options* options,
                                  const cmx_grid2d_limits* limits, const uint16_t* tsd_cells,
                                  const uint16_t* weight_cells, float truncation_distance,
                                  float max_weight, const double* target_translation_xy,
                                  const cmx_pose2d* initial_pose_estimate,
                                  const float* point_cloud_xyz, int32_t num_points, int32_t device,
                                  cmx_pose2d* pose_estimate, cmx_ceres_summary* summary);
cmx_status cmx_ceres2d_match_tsdf_grid(const cmx_ceres2d_options* options, const cmx_tsdf2d* grid,
                                       const double* target_translation_xy,
                                       const cmx_pose2d* initial_pose_estimate,
                                       const float* point_cloud_xyz, int32_t num_points,
                                       cmx_pose2d* pose_estimate, cmx_ceres_summary* summary);
cmx_status cmx_ceres2d_refine_batch_tsdf(const cmx_ceres2d_options* options,
                                         const cmx_tsdf2d* const* grids, int32_t num_grids,
                                         const int32_t* found,
                                         const cmx_pose2d* pose_estimates_in,
                                         const float* point_cloud_xyz, int32_t num_points,
                                         cmx_pose2d* pose_estimates_out,
                                         cmx_ceres_summary* summaries);

/* ---- many trajectories' Ceres matches on resident grids ------------------------------------ */
/* CeresScanMatcher2D::Match for many robots in one call: with
 * use_online_correlative_scan_matching = false (trajectory_builder_2d.lua's default) the whole
 * scan match of LocalTrajectoryBuilder2D::ScanMatch (local_trajectory_builder_2d.cc:64-107), else
 * its second half.  Unlike the refine entries above, every job brings its own target translation
 * (the pose prediction's) and its own initial estimate.  num_jobs >= 1.
 *   - pose_estimates[i] and summaries[i] (summaries may be NULL) are bit for bit what the single
 *     call returns for the same arguments: cmx_ceres2d_match_grid for a job with `grid`,
 *     cmx_ceres2d_match_tsdf_grid for a job with `tsdf` -- the FAILURE of a TSDF job whose
 *     interpolated weights are all 0 included (the pose is the initial estimate, costs -1, both
 *     step counts -1), and max_num_iterations too.  `options` are one set for the whole call, as
 *     a LocalTrajectoryBuilder2D has one.
 *   - Probability grids and TSDFs may alternate freely in one list; a grid may appear in several
 *     jobs (the call only reads its grids).
 *   - A job's cloud is host memory (point_cloud_xyz, num_points) or a cloud uploaded with
 *     cmx_cloud_upload (cloud; num_points is then 0 or the cloud's own count); both kinds may be
 *     mixed.  Equal point_cloud_xyz pointers are one cloud, staged once, and must come with equal
 *     counts.  A TSDF job may have num_points == 0 with both cloud fields NULL: it ends with
 *     FAILURE as the single call does.  A probability-grid job needs at least one point.
 *   - One upload, ONE launch (Ceres2DJobKernel, one workgroup per job whatever its kind), one
 *     read-back and one synchronisation per call: the launches do not grow with num_jobs.  The
 *     call runs on the stream of cmx_set_stream when the calling thread has set one.
 *   - All grids and resident clouds of a call live on one device.
 *   - Every check is made before the device is touched: null options / jobs / pose_estimates,
 *     num_jobs < 1, the option checks of the single calls, and per job: neither or both of grid /
 *     tsdf, neither or both of point_cloud_xyz / cloud, a count outside 1 .. 2^24 (0 .. 2^24 for a
 *     TSDF job), reserved != 0, one pointer with two counts, a grid or cloud on another device
 *     than job 0's grid.  Each is CMX_INVALID_ARGUMENT, cmx_last_error names "job <index>", and no
 *     output is written (nor on any other error).
 *   - Without a HIP device, valid arguments give CMX_DEVICE_ERROR ("no CPU fallback"). */
typedef struct cmx_ceres2d_job {
  const cmx_grid2d* grid;          /* exactly one of grid / tsdf is set            */
  const cmx_tsdf2d* tsdf;
  const float* point_cloud_xyz;    /* exactly one of point_cloud_xyz / cloud is set */
  const cmx_cloud* cloud;          /* uploaded with cmx_cloud_upload                */
  int32_t num_points;              /* of point_cloud_xyz; with `cloud`: 0 or the cloud's own count */
  int32_t reserved;                /* 0 */
  double target_translation_xy[2];
  cmx_pose2d initial_pose_estimate;
} cmx_ceres2d_job;

cmx_status cmx_ceres2d_match_grid_batch(const cmx_ceres2d_options* options,
                                        const cmx_ceres2d_job* jobs, int32_t num_jobs,
                                        cmx_pose2d* pose_estimates,      /* num_jobs */
                                        cmx_ceres_summary* summaries);   /* num_jobs, may be NULL */

/* ---- many nodes against 2D submaps: lists of (node, submap) pairs ------------------------- */
/* The other half of PoseGraph2D::ComputeConstraintsForNode (pose_graph_2d.cc:383-393: when a
 * submap finishes, every old node is matched against it) and any other list of (node, submap)
 * pairs: as cmx_fast2d_match_batch, but pair p brings its own cloud.  num_pairs >= 1.
 *   - found[p], scores[p] and pose_estimates[p] are bit for bit what cmx_fast2d_match returns for
 *     (matchers[p], cloud p, initial_pose_estimates[p], min_scores[p]) -- where
 *     match_full_submap[p] != 0, what cmx_fast2d_match_full_submap returns.
 *     initial_pose_estimates may be NULL only if every pair is a full-submap search.
 *   - Entries of point_clouds_xyz / clouds may repeat: equal pointers are the same node, and a
 *     host cloud is uploaded once per distinct pointer, not once per pair.  The num_points of
 *     equal pointers must agree (else CMX_INVALID_ARGUMENT).  A null or empty cloud is
 *     CMX_INVALID_ARGUMENT, as in the single calls.
 *   - Matchers of different branch_and_bound_depth may appear in one list.
 *   - All matchers (and clouds) of a call live on one device; a mixed list is
 *     CMX_INVALID_ARGUMENT before anything is launched.
 *   - The pairs are grouped by (cloud, depth).  A group is one cmx_fast2d_match_batch: the pairs
 *     of a node share that node's launches.  Several groups run concurrently, each on a stream
 *     of its own; under a cmx_set_stream override of the calling thread they run one after the
 *     other on that stream.  Pairs of different clouds do not share launches.
 *   - The first error by pair index is the call's error.  *stats is the sum over the pairs.
 *   - Without a HIP device: CMX_DEVICE_ERROR ("no CPU fallback"), whatever the arguments.
 * The _resident entry takes clouds uploaded by cmx_cloud_upload and uploads nothing. */
cmx_status cmx_fast2d_match_pairs(const cmx_fast2d* const* matchers, int32_t num_pairs,
                                  const cmx_pose2d* initial_pose_estimates,
                                  const int32_t* match_full_submap, const float* min_scores,
                                  const float* const* point_clouds_xyz, const int32_t* num_points,
                                  int32_t* found, float* scores, cmx_pose2d* pose_estimates,
                                  cmx_match_stats* stats);
cmx_status cmx_fast2d_match_pairs_resident(const cmx_fast2d* const* matchers, int32_t num_pairs,
                                           const cmx_pose2d* initial_pose_estimates,
                                           const int32_t* match_full_submap,
                                           const float* min_scores,
                                           const cmx_cloud* const* clouds, int32_t* found,
                                           float* scores, cmx_pose2d* pose_estimates,
                                           cmx_match_stats* stats);
/* The refinement of those results (constraint_builder_2d.cc:245-249) in ONE launch, one result
 * copy and one synchronisation for the whole list: entry p is bit for bit what
 * cmx_fast2d_refine_batch (cmx_ceres2d_refine_batch_tsdf for the _tsdf entry) returns for that
 * pair alone, the pass-through of found[p] == 0 included (found may be NULL: every pair is
 * refined).  Clouds may repeat as above (a host cloud is staged once per distinct pointer), all
 * matchers / grids (and clouds) live on one device, num_pairs >= 1; a null or empty cloud is
 * CMX_INVALID_ARGUMENT, except that the TSDF entry accepts num_points[p] == 0 as
 * cmx_ceres2d_refine_batch_tsdf does (FAILURE, the pose untouched).  Without a HIP device:
 * CMX_DEVICE_ERROR ("no CPU fallback"), whatever the arguments. */
cmx_status cmx_fast2d_refine_pairs(const cmx_ceres2d_options* options,
                                   const cmx_fast2d* const* matchers, int32_t num_pairs,
                                   const int32_t* found, const cmx_pose2d* pose_estimates_in,
                                   const float* const* point_clouds_xyz,
                                   const int32_t* num_points, cmx_pose2d* pose_estimates_out,
                                   cmx_ceres_summary* summaries);
cmx_status cmx_fast2d_refine_pairs_resident(const cmx_ceres2d_options* options,
                                            const cmx_fast2d* const* matchers, int32_t num_pairs,
                                            const int32_t* found,
                                            const cmx_pose2d* pose_estimates_in,
                                            const cmx_cloud* const* clouds,
                                            cmx_pose2d* pose_estimates_out,
                                            cmx_ceres_summary* summaries);
cmx_status cmx_ceres2d_refine_pairs_tsdf(const cmx_ceres2d_options* options,
                                         const cmx_tsdf2d* const* grids, int32_t num_pairs,
                                         const int32_t* found,
                                         const cmx_pose2d* pose_estimates_in,
                                         const float* const* point_clouds_xyz,
                                         const int32_t* num_points,
                                         cmx_pose2d* pose_estimates_out,
                                         cmx_ceres_summary* summaries);

cmx_status cmx_ceres2d_tsdf_residuals(const cmx_grid2d_limits* limits, const uint16_t* tsd_cells,
                                      const uint16_t* weight_cells, float truncation_distance,
                                      float max_weight, double residual_scaling_factor,
                                      const double* pose, const float* point_cloud_xyz,
                                      int32_t num_points, int32_t device, double* residuals,
                                      double* jacobian, int32_t* valid);

/* ---- CeresScanMatcher3D ------------------------------------------- */
/* proto::CeresScanMatcherOptions3D (mapping/proto/scan_matching/ceres_scan_matcher_options_3d.proto)
 * + the ceres_solver_options cartographer sets; the per-pair IntensityCostFunctionOptions ride
 * with the pair they belong to (cmx_ceres3d_pair). */
typedef struct cmx_ceres3d_options {
  double occupied_space_weight[3];   /* one per (point cloud, hybrid grid) pair */
  double translation_weight;
  double rotation_weight;
  int32_t num_pairs;                 /* 1 .. 3: high-resolution, low-resolution, ... */
  int32_t only_optimize_yaw;
  int32_t use_nonmonotonic_steps;
  int32_t max_num_iterations;
} cmx_ceres3d_options;
/* One cell of an IntensityHybridGrid (mapping/3d/hybrid_grid.h:543-571): AverageIntensityData
 * {sum, count}; GetIntensity = sum / count, 0 where count == 0 or the cell is absent. */
typedef struct cmx_intensity_voxel {
  int32_t x, y, z;
  int32_t count;
  float sum;
} cmx_intensity_voxel;
/* CeresScanMatcher3D::PointCloudAndHybridGridsPointers (SM3/ceres_scan_matcher_3d.h:42-46); the
 * grid as the voxel list HybridGrid::Iterator yields. */
typedef struct cmx_ceres3d_pair {
  const float* point_cloud_xyz;
  int32_t num_points;
  float resolution;
  const cmx_voxel* voxels;
  int64_t num_voxels;
  /* IntensityCostFunction3D (SM3/intensity_cost_function_3d.h, ceres_scan_matcher_3d.cc:118-137):
   * `intensities` == NULL: the pair has no intensity_hybrid_grid (what ConstraintBuilder3D
   * passes).  Otherwise num_points intensities (PointCloud::intensities()), the intensity grid
   * (same resolution as the pair's hybrid grid) and its IntensityCostFunctionOptions; the block
   * carries ceres::HuberLoss(intensity_huber_scale). */
  const float* intensities;
  const cmx_intensity_voxel* intensity_voxels;
  int64_t num_intensity_voxels;
  double intensity_weight;
  double intensity_huber_scale;
  float intensity_threshold;
  int32_t reserved;
} cmx_ceres3d_pair;
/* CeresScanMatcher3D::Match (SM3/ceres_scan_matcher_3d.h:55-60, .cc:90-156): occupied-space
 * residuals through InterpolatedGrid (SM3/interpolated_grid.h), translation / rotation delta
 * residuals, quaternion (or yaw-only) local parameterization, Ceres's trust-region
 * Levenberg-Marquardt with its default options.  The rotation target is the initial rotation. */
cmx_status cmx_ceres3d_match(const cmx_ceres3d_options* options,
                             const double* target_translation_xyz,
                             const cmx_pose3d* initial_pose_estimate,
                             const cmx_ceres3d_pair* pairs, int32_t device,
                             cmx_pose3d* pose_estimate, cmx_ceres_summary* summary);

/* Introspection used by the parity tests (not needed by a caller). */
cmx_status cmx_fast2d_level_dims(const cmx_fast2d* matcher, int32_t level, int32_t* wide_x,
                                 int32_t* wide_y);
cmx_status cmx_fast2d_level_cells(const cmx_fast2d* matcher, int32_t level, uint8_t* out);
/* Prepared search of a (full-submap or windowed) match: rotated+discretised
 * scans [num_scans][n][2], shrunk linear bounds [num_scans][4]
 * (min_x,max_x,min_y,max_y) and the integer sums of every lowest-resolution
 * candidate in the reference's generation order (scan, x, y).  Any output may
 * be NULL; capacities are in elements. */
cmx_status cmx_fast2d_debug_prepare(const cmx_fast2d* matcher,
                                    const cmx_pose2d* initial_pose_estimate,
                                    const float* point_cloud_xyz, int32_t num_points,
                                    int32_t full_submap, int32_t* num_scans,
                                    double* angular_step, int32_t* discrete_xy,
                                    int64_t discrete_capacity, int32_t* bounds,
                                    int64_t bounds_capacity, int32_t* coarse_sums,
                                    int64_t sums_capacity, int64_t* num_coarse);

/* ---- real-time 3D ------------------------------------------------------ */
cmx_status cmx_rt3d_match(const cmx_rt_options* options, float grid_resolution,
                          const cmx_voxel* voxels, int64_t num_voxels,
                          const cmx_pose3d* initial_pose_estimate, const float* point_cloud_xyz,
                          int32_t num_points, int32_t device, float* score,
                          cmx_pose3d* pose_estimate, cmx_match_stats* stats);

/* ---- device-resident hybrid grid -------------------- */
/* The active 3D submap's HybridGrid kept in HBM as a dense uint16 brick:
 *   cmx_grid3d_create    HybridGrid(resolution) (mapping/3d/hybrid_grid.h:459-462)
 *   cmx_grid3d_insert    RangeDataInserter3D::Insert without intensities
 *                        (mapping/3d/range_data_inserter_3d.cc:27-52, :93-114): hits, then the last
 *                        `num_free_space_voxels` voxels of every ray as misses, FinishUpdate;
 *                        points in the map frame, xyz triples
 *   cmx_grid3d_insert_batch  the same for many (grid, cloud) pairs in one call (below)
 *   cmx_grid3d_info     resolution(), DynamicGrid::grid_size() (hybrid_grid.h:259,381-398) and
 *                        the number of known voxels
 *   cmx_grid3d_download  the voxels HybridGrid::Iterator yields (hybrid_grid.h:304-372), sorted
 *                        (z, y, x): the list cmx_rt3d_match / cmx_fast3d_create take */
typedef struct cmx_grid3d cmx_grid3d;
cmx_status cmx_grid3d_create(float resolution, int32_t device, cmx_grid3d** out);
void cmx_grid3d_destroy(cmx_grid3d* grid);
cmx_status cmx_grid3d_insert(cmx_grid3d* grid, const float* origin_xyz, const float* returns_xyz,
                             int32_t num_returns, float hit_probability, float miss_probability,
                             int32_t num_free_space_voxels);

/* One insertion of a cmx_grid3d_insert_batch call: the arguments of cmx_grid3d_insert that differ
 * from insertion to insertion. */
typedef struct cmx_grid3d_insertion {
  cmx_grid3d* grid;
  const float* origin_xyz;     /* 3 floats */
  const float* returns_xyz;    /* num_returns xyz triples, map frame */
  int32_t num_returns;
  int32_t reserved;            /* 0 */
} cmx_grid3d_insertion;

/* cmx_grid3d_insert(insertions[i] ...) for i = 0 .. num_insertions - 1 in list order, bit for bit
 * (every voxel value, grid_size and the brick bounds), in shared launches: what
 * ActiveSubmaps3D::InsertData does to the high- and low-resolution grids of its two submaps, or a
 * fleet to the active submaps of every robot after one cmx_fast3d_match_pairs.
 *   - Grids of different resolutions may share a call.  One set of probabilities and one
 *     num_free_space_voxels hold for the whole call.
 *   - A grid may appear several times: its insertions apply in list order.  The r-th insertion of
 *     every grid forms round r; a round is three launches (hits, miss samples, marker clearing)
 *     over all its insertions, so the number of launches grows with the most insertions any one
 *     grid has, not with the number of grids.
 *   - One extent launch for the whole call finds the touched voxels and the rays of 2^15 voxels or
 *     more of every insertion; the host reads it back once and plans the growth of all grids.  Two
 *     stream synchronisations per call: after that pass and at the end.
 *   - The clouds go up in one staged copy.  Equal returns_xyz pointers are the same cloud and cross
 *     PCIe once per call; their counts must be equal too.
 *   - An insertion with num_returns == 0 does nothing to its grid, as in the single call; it still
 *     takes its place in the count of rounds.
 *   - Every argument check of the single call is made for every insertion before the device is
 *     touched: CMX_INVALID_ARGUMENT names `insertion <index>` in cmx_last_error.  num_insertions
 *     < 1, null `insertions`, a null grid or origin, num_returns < 0, num_returns > 0 with null
 *     returns, reserved != 0, num_free_space_voxels < 0, probabilities outside (0, 1) and grids on
 *     different devices are invalid.
 *   - A ray of 2^15 voxels or more and a voxel index outside +-2^20 are found by the extent pass:
 *     CMX_INVALID_ARGUMENT names the first such insertion, and no grid has changed: not its brick,
 *     its grid_size or any cell.
 *   - Every grid is grown once, to what its last insertion needs, before anything is inserted, and
 *     all new bricks are allocated before any old one is released.  When an allocation fails there
 *     (CMX_OUT_OF_MEMORY), no grid has changed.
 * cmx_grid3d_insert_with_intensities has no batch form. */
cmx_status cmx_grid3d_insert_batch(const cmx_grid3d_insertion* insertions, int32_t num_insertions,
                                   float hit_probability, float miss_probability,
                                   int32_t num_free_space_voxels);

cmx_status cmx_grid3d_info(const cmx_grid3d* grid, float* resolution, int32_t* grid_size,
                           int64_t* num_voxels);
cmx_status cmx_grid3d_download(const cmx_grid3d* grid, cmx_voxel* voxels, int64_t capacity,
                               int64_t* num_voxels);

/* RealTimeCorrelativeScanMatcher3D::Match on the resident grid: LocalTrajectoryBuilder3D's per-scan
 * pair Match() -> InsertRangeData() (mapping/internal/3d/local_trajectory_builder_3d.cc:96-108,
 * :344-347) then moves only the scan across PCIe.  Same result as cmx_rt3d_match on
 * cmx_grid3d_download's voxel list. */
cmx_status cmx_rt3d_match_grid(const cmx_rt_options* options, const cmx_grid3d* grid,
                               const cmx_pose3d* initial_pose_estimate,
                               const float* point_cloud_xyz, int32_t num_points, float* score,
                               cmx_pose3d* pose_estimate, cmx_match_stats* stats);

/* `num_matches` independent cmx_rt3d_match_grid calls (one per trajectory / robot: scan i against
 * grid i around pose i) in one call; scores[i] and pose_estimates[i] are bit for bit what the
 * single call returns for entry i.  One set of options for the call; grids of different
 * resolutions may share it, a grid may appear in several matches, a grid nothing was inserted into
 * is valid.  Equal point_clouds_xyz pointers are one cloud, staged once (their num_points must
 * agree).  The grids are read where they lie and nothing derived from them is kept between calls.
 * Small searches (the 0.15 m / 1 degree window of trajectory_builder_3d.lua: 42 875 candidates, a
 * few hundred points) share two launches, one upload and one synchronisation; larger ones run as
 * the single call does, one after the other inside the call.  Every argument check, and the
 * limits of the search window (fewer than 512 linear and 64 angular steps, fewer than 2^31
 * candidates), are made for every match before the device is touched: CMX_INVALID_ARGUMENT names
 * "match <index>" in cmx_last_error and no output is written.  `stats` (may be NULL) is one struct
 * for the call: candidates_scored, coarse_candidates, num_scans and nodes_expanded summed over the
 * matches, device_ms the span of the shared launches plus the device time of the other matches. */
cmx_status cmx_rt3d_match_grid_batch(const cmx_rt_options* options,
                                     const cmx_grid3d* const* grids, int32_t num_matches,
                                     const cmx_pose3d* initial_pose_estimates,
                                     const float* const* point_clouds_xyz,
                                     const int32_t* num_points, float* scores,
                                     cmx_pose3d* pose_estimates, cmx_match_stats* stats);

/* CeresScanMatcher3D::Match as LocalTrajectoryBuilder3D::ScanMatch calls it
 * (mapping/internal/3d/local_trajectory_builder_3d.cc:96-123) against the ACTIVE submap: pair k is
 * (point_clouds_xyz[k], num_points[k]) with the resident HybridGrid grids[k] (its resolution is
 * the grid's); options->num_pairs pairs, all grids on one device.  Nothing but the clouds is
 * uploaded.  Pairs with an intensity term: cmx_ceres3d_match_grids_intensity below. */
cmx_status cmx_ceres3d_match_grids(const cmx_ceres3d_options* options,
                                   const double* target_translation_xyz,
                                   const cmx_pose3d* initial_pose_estimate,
                                   const cmx_grid3d* const* grids,
                                   const float* const* point_clouds_xyz,
                                   const int32_t* num_points, cmx_pose3d* pose_estimate,
                                   cmx_ceres_summary* summary);

/* `num_matches` independent cmx_ceres3d_match_grids calls (the refinement that follows
 * cmx_rt3d_match_grid_batch for a fleet) in one upload, one launch and one synchronisation; entry
 * i is bit for bit the single call on target_translations_xyz + 3 i, initial_pose_estimates[i] and
 * the options->num_pairs pairs grids / point_clouds_xyz / num_points [i * num_pairs ..].  The
 * target translation is an argument of its own: after a real-time match it differs from the
 * initial pose's (local_trajectory_builder_3d.cc:96-123).  Equal cloud pointers are one cloud,
 * staged once (their num_points must agree); all grids live on one device; a grid nothing was
 * inserted into is valid.  Checks are made before the device is touched and name "match <index>".
 * There is no batch form with intensity terms: cmx_ceres3d_match_grids_intensity stays a single
 * call.  `summaries` [num_matches] may be NULL. */
cmx_status cmx_ceres3d_match_grids_batch(const cmx_ceres3d_options* options, int32_t num_matches,
                                         const double* target_translations_xyz,
                                         const cmx_pose3d* initial_pose_estimates,
                                         const cmx_grid3d* const* grids,
                                         const float* const* point_clouds_xyz,
                                         const int32_t* num_points,
                                         cmx_pose3d* pose_estimates,
                                         cmx_ceres_summary* summaries);

/* ---- IntensityHybridGrid in HBM -------------------------------------------
 * mapping/3d/hybrid_grid.h:543-571: AverageIntensityData {sum, count} per voxel.
 *   cmx_grid3d_insert_with_intensities  RangeDataInserter3D::Insert with an intensity grid
 *                                       (mapping/3d/range_data_inserter_3d.cc:93-114): hits and
 *                                       misses into `grid` exactly as cmx_grid3d_insert, then
 *                                       InsertIntensitiesIntoGrid (:54-70) -- returns whose
 *                                       intensity exceeds `intensity_threshold` are skipped, the
 *                                       others add to their voxel's count and, IN POINT ORDER,
 *                                       to its f32 sum (bit-identical to the reference's loop).
 *                                       `intensities` = PointCloud::intensities() of the returns
 *                                       (num_returns floats); NULL inserts none (:57).
 *   cmx_intensity_grid3d_download       the voxels with count > 0, (z, y, x) order.
 *   cmx_ceres3d_match_grids_intensity   cmx_ceres3d_match_grids with IntensityCostFunction3D
 *                                       terms (SM3/ceres_scan_matcher_3d.cc:118-137) read from
 *                                       resident intensity grids: terms[k].grid == NULL: pair k
 *                                       has none.  Bit-identical to cmx_ceres3d_match on the same
 *                                       voxels. */
typedef struct cmx_intensity_grid3d cmx_intensity_grid3d;
cmx_status cmx_intensity_grid3d_create(float resolution, int32_t device,
                                       cmx_intensity_grid3d** out);
void cmx_intensity_grid3d_destroy(cmx_intensity_grid3d* grid);
cmx_status cmx_grid3d_insert_with_intensities(cmx_grid3d* grid,
                                              cmx_intensity_grid3d* intensity_grid,
                                              const float* origin_xyz, const float* returns_xyz,
                                              const float* intensities, int32_t num_returns,
                                              float hit_probability, float miss_probability,
                                              int32_t num_free_space_voxels,
                                              float intensity_threshold);
cmx_status cmx_intensity_grid3d_download(const cmx_intensity_grid3d* grid,
                                         cmx_intensity_voxel* voxels, int64_t capacity,
                                         int64_t* num_voxels);
typedef struct cmx_ceres3d_intensity_term {
  cmx_intensity_grid3d* grid;   /* NULL: no intensity term for this pair */
  const float* intensities;     /* num_points[k] intensities of the pair's cloud */
  double weight;                /* IntensityCostFunctionOptions::weight */
  double huber_scale;           /* ... ::huber_scale */
  float intensity_threshold;    /* ... ::intensity_threshold */
  int32_t reserved;
} cmx_ceres3d_intensity_term;
cmx_status cmx_ceres3d_match_grids_intensity(const cmx_ceres3d_options* options,
                                             const double* target_translation_xyz,
                                             const cmx_pose3d* initial_pose_estimate,
                                             const cmx_grid3d* const* grids,
                                             const float* const* point_clouds_xyz,
                                             const int32_t* num_points,
                                             const cmx_ceres3d_intensity_term* terms,
                                             cmx_pose3d* pose_estimate,
                                             cmx_ceres_summary* summary);

/* ---- fast 3D ------------------------------------------------------------ */
/* hybrid_grid.h:137 grid_size(): 8*8*2^bits cells per axis of the dynamic
 * grid the voxels came from (needed by MatchFullSubmap's window). */
cmx_status cmx_fast3d_create(const cmx_fast3d_options* options, float resolution,
                             int32_t grid_size, const cmx_voxel* voxels, int64_t num_voxels,
                             float low_resolution, const cmx_voxel* low_resolution_voxels,
                             int64_t num_low_resolution_voxels,
                             const float* rotational_scan_matcher_histogram,
                             int32_t histogram_size, int32_t device, cmx_fast3d** out);
/* The same matcher built from two resident HybridGrids (cmx_grid3d) without moving them across
 * PCIe: ConstraintBuilder3D's FastCorrelativeScanMatcher3D(high_resolution_hybrid_grid,
 * low_resolution_hybrid_grid, histogram, options) over submaps kept in HBM.  The device, both
 * resolutions and grid_size (cmx_grid3d_info) come from the grids, which must live on one device.
 * Bit-identical to cmx_fast3d_create on the lists cmx_grid3d_download returns for the two grids
 * (every precomputation level, its bounds, and the raw grids cmx_fast3d_refine_batch reads).  The
 * matcher keeps its own copies: the grids may be inserted into or destroyed afterwards. */
cmx_status cmx_fast3d_create_from_grids(const cmx_fast3d_options* options,
                                        const cmx_grid3d* high_resolution_grid,
                                        const cmx_grid3d* low_resolution_grid,
                                        const float* rotational_scan_matcher_histogram,
                                        int32_t histogram_size, cmx_fast3d** out);
/* One submap of a cmx_fast3d_create_batch call.  Exactly one kind is set: the voxel lists of
 * cmx_fast3d_create (host memory; resolution, grid_size, low_resolution with them), or the two
 * resident grids of cmx_fast3d_create_from_grids.  The histogram belongs to either kind. */
typedef struct cmx_fast3d_source {
  float resolution;  int32_t grid_size;
  const cmx_voxel* voxels;                 int64_t num_voxels;
  float low_resolution;
  const cmx_voxel* low_resolution_voxels;  int64_t num_low_resolution_voxels;
  const cmx_grid3d* high_resolution_grid;
  const cmx_grid3d* low_resolution_grid;
  const float* rotational_scan_matcher_histogram;  int32_t histogram_size;
} cmx_fast3d_source;
/* The matchers of `num_sources` submaps on `device` -- a loaded map, or the first global
 * constraint of a node against every finished submap (constraints/constraint_builder_3d.cc:118-142,
 * :170-198) -- in ONE call: out[k] is, bit for bit, the matcher the single create of sources[k]
 * returns (every precomputation level with its bounds, every oct array, both raw uint16 grids
 * cmx_fast3d_refine_* reads, the histogram, grid_size and both resolutions).  Sources may differ
 * in kind, extent and resolution; `options` holds for all, as a ConstraintBuilder3D has one set.
 * The number of launches and synchronisations does not grow with num_sources: one launch finds
 * the boxes of all resident sources (one synchronisation, none without a resident source), one
 * chain of launches builds the whole list (a list too large for the staging memory, a launch
 * grid or a 32-bit count: consecutive chains), one synchronisation per chain.
 * Every matcher owns its memory (one allocation each), is used like any other and is destroyed
 * with cmx_fast3d_destroy, in any order; the sources are free once the call returns.
 * All or nothing: every argument check of the two single creates is made for every source
 * before the device is touched -- a failing one is CMX_INVALID_ARGUMENT and cmx_last_error names
 * the index of the source; so are num_sources < 1, a source with both kinds set (a voxel pointer
 * together with a grid pointer) or none (a source without any pointer is the voxel kind: valid
 * with both counts 0 and its resolutions set, the single create's empty case), and a resident
 * source on another device than `device`.  The limits of a dense grid (index range, size of a
 * level) are argument errors that name the index too, found before anything is allocated.  On
 * any error (a device allocation that fails half-way included) nothing is left allocated and
 * every out[k] is NULL. */
cmx_status cmx_fast3d_create_batch(const cmx_fast3d_options* options,
                                   const cmx_fast3d_source* sources, int32_t num_sources,
                                   int32_t device, cmx_fast3d** out /* num_sources */);
void cmx_fast3d_destroy(cmx_fast3d* matcher);

/* TrajectoryNode::Data (mapping/trajectory_node.h:45-63), the fields the
 * matcher reads. */
typedef struct cmx_node_data3d {
  double gravity_alignment[4];                 /* quaternion w,x,y,z */
  const float* high_resolution_point_cloud;    /* xyz */
  int32_t num_high_resolution_points;
  const float* low_resolution_point_cloud;     /* xyz */
  int32_t num_low_resolution_points;
  const float* rotational_scan_matcher_histogram;
  int32_t histogram_size;
} cmx_node_data3d;

/* FastCorrelativeScanMatcher3D::Result. */
typedef struct cmx_result3d {
  float score;
  cmx_pose3d pose_estimate;
  float rotational_score;
  float low_resolution_score;
} cmx_result3d;

cmx_status cmx_fast3d_match(const cmx_fast3d* matcher, const cmx_pose3d* global_node_pose,
                            const cmx_pose3d* global_submap_pose, const cmx_node_data3d* data,
                            float min_score, int32_t* found, cmx_result3d* result,
                            cmx_match_stats* stats);
cmx_status cmx_fast3d_match_full_submap(const cmx_fast3d* matcher,
                                        const double* global_node_rotation_wxyz,
                                        const double* global_submap_rotation_wxyz,
                                        const cmx_node_data3d* data, float min_score,
                                        int32_t* found, cmx_result3d* result,
                                        cmx_match_stats* stats);

/* ConstraintBuilder3D's fan-out for one node (constraints/constraint_builder_3d.cc:79-147):
 * `data` against num_pairs matchers, pair p a windowed Match around node_poses[p] /
 * submap_poses[p] or, where match_full_submap[p] != 0, a MatchFullSubmap with their rotations,
 * against its own threshold min_scores[p].  All pairs whose matchers live on one device are ONE
 * chain of launches on that device (every kernel takes the array of problems; frontier and
 * leaf lists are shared, bounds and seeds are per problem); found[p] / results[p] as in the
 * single calls; *stats summed. */
cmx_status cmx_fast3d_match_batch(const cmx_fast3d* const* matchers, int32_t num_pairs,
                                  const cmx_pose3d* node_poses, const cmx_pose3d* submap_poses,
                                  const int32_t* match_full_submap, const float* min_scores,
                                  const cmx_node_data3d* data, int32_t* found,
                                  cmx_result3d* results, cmx_match_stats* stats);
/* The other half of PoseGraph3D::ComputeConstraintsForNode (mapping/internal/3d/
 * pose_graph_3d.cc:370-379: when a submap finishes, every old node is matched against it), and
 * any other list of (node, submap) pairs: as cmx_fast3d_match_batch, but pair p brings its own
 * data[p] -- clouds, histogram and gravity alignment.  found[p] / results[p] are bit for bit
 * what cmx_fast3d_match (cmx_fast3d_match_full_submap where match_full_submap[p] != 0) returns
 * for (matchers[p], data[p], node_poses[p], submap_poses[p], min_scores[p]).  Entries of `data`
 * may repeat: equal pointers mean the same node, whose clouds go to the device once per chain
 * of launches.  All matchers must live on one device; data[p]'s histogram size is checked
 * against matchers[p]'s; num_pairs >= 1.  A list whose lowest-resolution candidates or rotated
 * points (scans x points, summed) reach 2^31 runs as consecutive sub-batches that fit, one
 * after the other (so does cmx_fast3d_match_batch); a single pair that large is
 * CMX_INVALID_ARGUMENT.  The size of the scratch memory is no criterion of that split: a chain
 * of launches asks the device for 16 bytes per rotated point, and a list that the device cannot
 * hold fails with CMX_DEVICE_ERROR -- pass it in parts.  Without a HIP device the call is
 * CMX_DEVICE_ERROR whatever its arguments are (no matcher can exist then).  *stats summed; stats->expansion_lookups is 0 for a chain of launches
 * whose pairs differ in their number of high-resolution points (the expansion counters are
 * shared by its pairs). */
cmx_status cmx_fast3d_match_pairs(const cmx_fast3d* const* matchers, int32_t num_pairs,
                                  const cmx_pose3d* node_poses, const cmx_pose3d* submap_poses,
                                  const int32_t* match_full_submap, const float* min_scores,
                                  const cmx_node_data3d* const* data, /* one per pair */
                                  int32_t* found, cmx_result3d* results, cmx_match_stats* stats);
/* ConstraintBuilder3D::ComputeConstraint's refinement (constraints/constraint_builder_3d.cc:
 * 263-276) for the results of cmx_fast3d_match_batch: pair i runs CeresScanMatcher3D::Match
 * (target translation = pose_estimates_in[i].t, initial pose = pose_estimates_in[i]) with
 * {data's high-resolution cloud, matcher i's high-resolution grid} and {low-resolution cloud,
 * low-resolution grid}; both grids are the ones the matcher keeps in HBM since
 * cmx_fast3d_create.  One launch per device, one workgroup per pair.  options->num_pairs must
 * be 2.  Entries with found[i] == 0 (found may be NULL) are passed through. */
cmx_status cmx_fast3d_refine_batch(const cmx_ceres3d_options* options,
                                   const cmx_fast3d* const* matchers, int32_t num_pairs,
                                   const int32_t* found, const cmx_pose3d* pose_estimates_in,
                                   const cmx_node_data3d* data, cmx_pose3d* pose_estimates_out,
                                   cmx_ceres_summary* summaries);
/* The same for the results of cmx_fast3d_match_pairs (pose_graph_3d.cc:370-379): pair i is
 * refined with the clouds of data[i], bit for bit what cmx_fast3d_refine_batch returns for that
 * pair alone.  Equal pointers in `data` mean the same node, staged once; one launch per device,
 * one workgroup per pair; num_pairs >= 1 and no entry of `data` may be NULL.  Without a HIP
 * device the call is CMX_DEVICE_ERROR whatever its arguments are. */
cmx_status cmx_fast3d_refine_pairs(const cmx_ceres3d_options* options,
                                   const cmx_fast3d* const* matchers, int32_t num_pairs,
                                   const int32_t* found, const cmx_pose3d* pose_estimates_in,
                                   const cmx_node_data3d* const* data,
                                   cmx_pose3d* pose_estimates_out, cmx_ceres_summary* summaries);

/* ---- upstream point preparation ---------------------------------------- */
/* sensor::VoxelFilter(PointCloud, resolution) (sensor/internal/voxel_filter.cc:88-152): one
 * RANDOM point per voxel -- the reference's reservoir sample, reproduced exactly (the draws of
 * its default-seeded std::minstd_rand0 are located in the generator's stream by a prefix sum).
 * `filtered_xyz` needs room for num_points points; kept points stay in input order. */
cmx_status cmx_voxel_filter(const float* point_cloud_xyz, int32_t num_points, float resolution,
                            int32_t device, float* filtered_xyz, int32_t* num_filtered);
/* The same filter, returning WHICH points it kept (ascending indices into the input; room for
 * num_points of them): what the overloads of sensor::VoxelFilter over timed points and range
 * measurements (voxel_filter.cc:154-191) need to carry the points' payload along --
 * LocalTrajectoryBuilder3D filters TimedPointCloudOriginData::RangeMeasurement lists
 * (3d/local_trajectory_builder_3d.cc:158-159). */
cmx_status cmx_voxel_filter_indices(const float* point_cloud_xyz, int32_t num_points,
                                    float resolution, int32_t device, int32_t* kept_indices,
                                    int32_t* num_filtered);
/* sensor::AdaptiveVoxelFilter (voxel_filter.cc:30-75,193-198): range cut, then the search for
 * the voxel length that keeps at least min_num_points (proto::AdaptiveVoxelFilterOptions). */
cmx_status cmx_adaptive_voxel_filter(const float* point_cloud_xyz, int32_t num_points,
                                     float max_length, float min_num_points, float max_range,
                                     int32_t device, float* filtered_xyz, int32_t* num_filtered);
/* The same filter, returning WHICH points it kept (ascending indices into the input; room for
 * num_points of them), so that a caller can carry the points' payload along: sensor::PointCloud
 * keeps the intensities of the kept points (voxel_filter.cc:138-161,193-198), which
 * LocalTrajectoryBuilder3D needs when use_intensities is set
 * (3d/local_trajectory_builder_3d.cc:262,298). */
cmx_status cmx_adaptive_voxel_filter_indices(const float* point_cloud_xyz, int32_t num_points,
                                             float max_length, float min_num_points,
                                             float max_range, int32_t device,
                                             int32_t* kept_indices, int32_t* num_filtered);
/* Many filters in one call, and chains of them: the VoxelFilter and AdaptiveVoxelFilter that
 * LocalTrajectoryBuilder2D runs one on the other's output (2d/local_trajectory_builder_2d.cc),
 * the VoxelFilter and the two AdaptiveVoxelFilters of LocalTrajectoryBuilder3D
 * (3d/local_trajectory_builder_3d.cc), for one robot or for a fleet.  Job i returns, bit for
 * bit, what cmx_voxel_filter(_indices) / cmx_adaptive_voxel_filter(_indices) return for its
 * input.  A chained job (input_job >= 0) filters the points an earlier job kept, which never
 * leave the device in between; its indices refer to THAT cloud.  A job may have several chained
 * jobs, a chained job none (chains of two).  Output arrays need room for the num_points of the
 * host cloud the job goes back to; a job without output pointers is valid only if a job is
 * chained on it.  Equal point_cloud_xyz pointers are one cloud, with equal num_points, and are
 * uploaded once.  A job without points yields 0, and so do the jobs chained on it.
 * Host clouds of up to 4096 points and the jobs chained on them run one workgroup per job: all
 * host clouds in a first stage of launches, all chained jobs in a second, one synchronisation at
 * the end (calls that stage more than 32 MB go out in consecutive parts).  A host cloud above
 * 4096 points, and every job chained on it, runs inside the call as the single calls do, one
 * after the other with the host between the stages: same results, nothing gained.
 * Every argument check is made for every job before the device is touched; CMX_INVALID_ARGUMENT
 * names the job ("job <index>") in cmx_last_error.  num_jobs >= 1. */
enum { CMX_FILTER_VOXEL = 0, CMX_FILTER_ADAPTIVE = 1 };
typedef struct cmx_filter_job {
  const float* point_cloud_xyz; /* host cloud, xyz triples; NULL iff input_job >= 0 */
  int32_t num_points;           /* of the host cloud; 0 iff input_job >= 0 */
  int32_t input_job;            /* -1: the host cloud.  Else the index of an EARLIER job whose own
                                   input_job is -1: this job filters that job's output */
  int32_t mode;                 /* CMX_FILTER_VOXEL / CMX_FILTER_ADAPTIVE */
  float length;                 /* resolution (voxel) / max_length (adaptive); > 0 */
  float min_num_points;         /* adaptive only */
  float max_range;              /* adaptive only */
  int32_t* kept_indices;        /* may be NULL; indices into THIS job's input, ascending */
  float* filtered_xyz;          /* may be NULL */
} cmx_filter_job;
cmx_status cmx_filter_batch(const cmx_filter_job* jobs, int32_t num_jobs, int32_t device,
                            int32_t* num_filtered /* [num_jobs] */);
/* RotationalScanMatcher::ComputeHistogram (SM3/rotational_scan_matcher.cc:164-177): slices of
 * 0.2 m, points sorted by angle around the slice centroid, one weighted vote per point pair.
 * Same accumulation order as the reference; atan2f is the device's (<= 1 ulp from libm's). */
cmx_status cmx_compute_histogram(const float* point_cloud_xyz, int32_t num_points,
                                 int32_t histogram_size, int32_t device, float* histogram);
/* ComputeHistogram for many clouds in one call: the histogram of every node that
 * LocalTrajectoryBuilder3D::InsertIntoSubmap inserts (3d/local_trajectory_builder_3d.cc:399-404),
 * for a fleet.  Job i returns, bit for bit, what cmx_compute_histogram(point_cloud_xyz,
 * num_points, histogram_size, device, histogram) returns for it -- including the single call's
 * order for points of equal angle inside a slice: ascending input index (both of its radix sorts
 * are stable).  The cloud is what the caller would hand to ComputeHistogram: the rotation into
 * the gravity-aligned frame stays with the caller.  Equal point_cloud_xyz pointers are one
 * cloud, with equal num_points, and are uploaded once; two jobs may ask different histogram_size
 * of one cloud.  A job without points yields zeros.
 * Clouds of 1 .. 4096 finite points run one workgroup per job out of LDS: one upload, one launch
 * and one synchronisation for all of them (calls that stage more than 32 MB go out in
 * consecutive parts).  A cloud above 4096 points, or with a non-finite coordinate, runs inside
 * the call as the single call does: same result, nothing gained.
 * Every argument check is made for every job before the device is touched;
 * CMX_INVALID_ARGUMENT names the job ("job <index>") in cmx_last_error and no histogram has
 * been written.  num_jobs >= 1. */
typedef struct cmx_histogram_job {
  const float* point_cloud_xyz;  /* host cloud, xyz triples; may be NULL iff num_points == 0 */
  int32_t num_points;            /* 0 .. 2^24 */
  int32_t histogram_size;        /* 1 .. 8192 */
  float* histogram;              /* histogram_size floats, written by the call */
} cmx_histogram_job;
cmx_status cmx_compute_histogram_batch(const cmx_histogram_job* jobs, int32_t num_jobs,
                                       int32_t device);

/* ---- multi-GPU: one scan against submaps spread over the GPUs of a node ---------------- */
/* The (node, submap) searches of a ConstraintBuilder fan-out are independent
 * (constraints/constraint_builder_2d.cc:97-111, constraint_builder_3d.cc:79-142): submaps are
 * partitioned over the devices -- a matcher lives on the device it was created on
 * (cmx_comm_device_of gives the block partition) -- and every device searches its own block
 * concurrently, one host thread per device.  Results come back per pair, in the caller's order.
 * The node-wide best match (global localisation) is agreed on by ONE RCCL all-reduce(max) of a
 * packed 8-byte key over xGMI (score bits << 32 | 0xFFFFFFFF - index: equal scores resolve to
 * the lowest index whatever the partition).  RCCL is loaded by cmx_comm_init (dlopen). */
typedef struct cmx_comm cmx_comm;
/* devices == NULL: devices 0 .. num_devices-1. */
cmx_status cmx_comm_init(const int32_t* devices, int32_t num_devices, cmx_comm** out);
void cmx_comm_destroy(cmx_comm* comm);
int32_t cmx_comm_num_devices(const cmx_comm* comm);
/* 1 if the communicator's collective is RCCL's (several devices), 0 if it needs none (one
 * device: the key is its own). */
int32_t cmx_comm_uses_rccl(const cmx_comm* comm);
/* Device that owns item `index` of `num_items` under the contiguous block partition. */
int32_t cmx_comm_device_of(const cmx_comm* comm, int64_t index, int64_t num_items);
/* As cmx_fast2d_match_batch, the matchers spread over the communicator's devices.
 * best_index / best_score (may be NULL): the best found pair node-wide, -1 if none. */
cmx_status cmx_fast2d_match_sharded(cmx_comm* comm, const cmx_fast2d* const* matchers,
                                    int32_t num_matchers, const cmx_pose2d* initial_pose_estimates,
                                    const int32_t* match_full_submap, const float* min_scores,
                                    const float* point_cloud_xyz, int32_t num_points,
                                    int32_t* found, float* scores, cmx_pose2d* pose_estimates,
                                    int32_t* best_index, float* best_score,
                                    cmx_match_stats* stats);
/* As cmx_fast3d_match_batch (BASELINE config C5: one node against 256 submaps on 8 GPUs). */
cmx_status cmx_fast3d_match_sharded(cmx_comm* comm, const cmx_fast3d* const* matchers,
                                    int32_t num_pairs, const cmx_pose3d* node_poses,
                                    const cmx_pose3d* submap_poses,
                                    const int32_t* match_full_submap, const float* min_scores,
                                    const cmx_node_data3d* data, int32_t* found,
                                    cmx_result3d* results, int32_t* best_index, float* best_score,
                                    cmx_match_stats* stats);
/* The partition and the key, as plain host arithmetic (no device needed; rank processes that
 * shard with torch.distributed / MPI instead of cmx_comm use the same rules):
 * items [begin, end) of `rank`; key of the best found entry of a block (-1: none found). */
void cmx_shard_range(int64_t num_items, int32_t rank, int32_t world_size, int64_t* begin,
                     int64_t* end);
int64_t cmx_pack_best_key(const int32_t* found, const float* scores, int64_t num,
                          int64_t first_global_index);
void cmx_unpack_best_key(int64_t key, int32_t* found, float* score, int64_t* global_index);

/* Introspection used by the parity tests: one precomputation level as a dense
 * brick (x fastest) with the cell index of its first element. */
cmx_status cmx_fast3d_level_info(const cmx_fast3d* matcher, int32_t depth, int32_t* lo_xyz,
                                 int32_t* dims_xyz);
cmx_status cmx_fast3d_level_cells(const cmx_fast3d* matcher, int32_t depth, uint8_t* out);

#ifdef __cplusplus
}
#endif

#endif /* CARTOGRAPHER_MI355X_H_ */
