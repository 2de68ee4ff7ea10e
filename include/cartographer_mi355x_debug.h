/* Test and tool switches of libcartographer_mi355x -- NOT part of the drop-in boundary.
 *
 * The parity tests run every device path against its partner (the tile path of the real-time
 * 2D matcher against the one-thread-per-candidate kernels, verification modes of the 3D
 * matchers, ...) and the profiling tools override tuning choices.  Those selections go through
 * this call; the product reads no environment variable on a call path.  Names are the fields of
 * cmx::DebugOptions (cartographer_amd/csrc/cmx_common.h); everything is 0 by default.
 * Process-wide and not synchronised: set switches before the calls they should affect. */
#ifndef CARTOGRAPHER_MI355X_DEBUG_H_
#define CARTOGRAPHER_MI355X_DEBUG_H_

#include "cartographer_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* CMX_INVALID_ARGUMENT for an unknown name. */
cmx_status cmx_debug_set(const char* name, int32_t value);
/* Every switch back to 0. */
void cmx_debug_reset(void);

/* The plan of the fast 2D front end for one call of cmx_fast2d_match / _match_full_submap /
 * _match_batch: which of its routes every problem takes and how the launches of the call are
 * sized.  The launch path asks the same function; this entry launches nothing.  Tests use it
 * to show that a batch really mixes the routes it is meant to mix. */
typedef struct cmx_debug_fast2d_problem_plan {
  int32_t use_planes;     /* lowest resolution scored over phase planes (0: the generic kernel) */
  int32_t plane_stride;   /* bytes per phase plane: 64, 128, 192 or 256 (0: no planes) */
  int32_t use_fused;      /* preparation and scoring in the one fused launch */
  int32_t group;          /* rotations per workgroup of the fused launch: 1, or 3 (group bounds) */
  int32_t num_scans;
  int32_t reserved;
  int64_t acc;            /* padded LDS accumulators this problem asks of a plane kernel */
} cmx_debug_fast2d_problem_plan;

typedef struct cmx_debug_fast2d_launch_plan {
  int64_t fused_lds;        /* dynamic LDS of the fused launch, bytes (0: no fused problem) */
  int64_t fused_acc;        /* its accumulators: the largest `acc` of the fused problems */
  int64_t plane_acc_cells;  /* accumulators of the separate plane launches */
  int32_t any_group;
  int32_t max_scans;
  int32_t per_unit;         /* rotations per unit of the fused launch's grid: 3 if all are grouped */
  int32_t reserved;
} cmx_debug_fast2d_launch_plan;

/* `matchers` [num_matchers], or -- with `matchers` null -- the grids and options matchers would be
 * created from (`limits`, `options` [num_matchers]): the plan depends on their geometry only, so
 * that form needs no device.  `match_full_submap` [num_matchers] as in cmx_fast2d_match_batch
 * (null: all windowed); `max_range_xy`: the largest xy range of the cloud's `num_points` points.
 * The switches above apply as they do to a match.  `problems` [num_matchers] and `launch` out. */
cmx_status cmx_debug_fast2d_plan(const cmx_fast2d* const* matchers,
                                 const cmx_grid2d_limits* limits,
                                 const cmx_fast2d_options* options, int32_t num_matchers,
                                 const int32_t* match_full_submap, int32_t num_points,
                                 float max_range_xy, cmx_debug_fast2d_problem_plan* problems,
                                 cmx_debug_fast2d_launch_plan* launch);

/* The plan of one cmx_grid2d_insert_batch call from the limits of its grids and the points alone:
 * the round of every insertion (how many earlier insertions of the list go to the same grid) and
 * the limits every grid has after the call (GrowAsNeeded of every insertion replayed in list
 * order).  The launch path asks the same function; this entry launches nothing and needs no
 * device.  `limits` [num_grids] are the grids' limits before the call; an insertion names its grid
 * by index. */
typedef struct cmx_debug_grid2d_insertion {
  int32_t grid;                /* index into `limits` */
  int32_t num_returns;
  const float* origin_xy;      /* 2 floats */
  const float* returns_xyz;
  const float* misses_xyz;
  int32_t num_misses;
  int32_t reserved;
} cmx_debug_grid2d_insertion;

cmx_status cmx_debug_grid2d_insert_plan(const cmx_grid2d_limits* limits, int32_t num_grids,
                                        const cmx_debug_grid2d_insertion* insertions,
                                        int32_t num_insertions, int32_t* rounds,
                                        cmx_grid2d_limits* final_limits);

/* The plan of one cmx_tsdf2d_insert_batch call from the limits of its grids, the range data and
 * the options alone: for every insertion its round (how many earlier insertions of the list go to
 * the same grid), the limits its grid has AT that insertion (GrowAsNeeded of the insertions up to
 * and including it replayed in list order; the cost bounds are copied from `limits`) and its number
 * of rays (hits whose f32 range is at least the truncation distance); for the call the number of
 * distinct scans the host prepares (sort, normals, weights): insertions with the same returns_xyz
 * pointer and bitwise equal origin values share one.  The launch path asks the same functions;
 * this entry launches nothing and needs no device.  `limits` [num_grids] are the grids' limits
 * before the call; an insertion names its grid by index.  `rounds`, `limits_at`, `num_rays`
 * [num_insertions] and `num_scans` [1] out.  The errors are those of the call itself, naming the
 * insertion: a grid beyond 2^30 cells, range data that leaves the limits after GrowAsNeeded, one
 * pointer with two counts. */
typedef struct cmx_debug_tsdf2d_insertion {
  int32_t grid;                /* index into `limits` */
  int32_t num_returns;
  const float* origin_xyz;     /* 3 floats */
  const float* returns_xyz;
} cmx_debug_tsdf2d_insertion;

cmx_status cmx_debug_tsdf2d_insert_plan(const cmx_grid2d_limits* limits, int32_t num_grids,
                                        const cmx_debug_tsdf2d_insertion* insertions,
                                        int32_t num_insertions,
                                        const cmx_tsdf_inserter_options_2d* options,
                                        int32_t* rounds, cmx_grid2d_limits* limits_at,
                                        int32_t* num_rays, int32_t* num_scans);

/* The plan of one cmx_grid3d_insert_batch call from the state of its grids before the call and the
 * box of voxels every insertion touches (what the call's extent pass reads back): the round of
 * every insertion (how many earlier insertions of the list go to the same grid) and the brick
 * bounds and grid_size every grid has after the call (the growth steps of cmx_grid3d_insert
 * replayed in list order: the brick becomes the union of the 16-aligned boxes, grid_size doubles
 * until every index lies in [-grid_size / 2, grid_size / 2)).  The launch path asks the same
 * function; this entry launches nothing and needs no device.  An insertion names its grid by
 * index; a voxel index outside +-2^20 is CMX_INVALID_ARGUMENT naming the insertion. */
typedef struct cmx_debug_grid3d_state {
  int32_t lo[3];               /* lowest voxel of the brick */
  int32_t dims[3];             /* its extent in voxels; all 0: nothing inserted yet */
  int32_t grid_size;           /* DynamicGrid::grid_size(), 128 for a new grid */
  int32_t reserved;
} cmx_debug_grid3d_state;

typedef struct cmx_debug_grid3d_insertion {
  int32_t grid;                /* index into `grids` */
  int32_t reserved;
  int32_t box[6];              /* min x, y, z, max x, y, z; min x > max x: touches no voxel */
} cmx_debug_grid3d_insertion;

cmx_status cmx_debug_grid3d_insert_plan(const cmx_debug_grid3d_state* grids, int32_t num_grids,
                                        const cmx_debug_grid3d_insertion* insertions,
                                        int32_t num_insertions, int32_t* rounds,
                                        cmx_debug_grid3d_state* final_states);

/* The plan of one cmx_filter_batch call from its jobs alone (no cloud is read): which jobs take a
 * workgroup of which launch.  Host clouds are stage 0, chained jobs stage 1; a stage is at most two
 * launches, `launch` 0 for N <= 2048 (a compute unit holds two such workgroups) and 1 for N = 4096,
 * each with the dynamic LDS of its largest N.  N is the LDS carve: a host cloud's points rounded up
 * to a power of two, at least 64; a chained job takes its parent's.  A job without input (no
 * points, or chained on such a job) takes no workgroup: set and launch -1, N 0.  A host cloud above
 * 4096 points and the jobs chained on it run as the single calls do: `single` 1, set and launch
 * -1.  `set` counts the consecutive parts a call goes out in (switch filter_batch_set_kb: the
 * bound on a part's staged clouds and on its result slots, default 32 MB).  The launch path asks
 * the same function; this entry launches nothing and needs no device.  The errors are those of
 * the call itself, naming the job. */
typedef struct cmx_debug_filter_job_plan {
  int32_t set;
  int32_t stage;               /* 0: a host cloud, 1: chained */
  int32_t launch;              /* within its stage */
  int32_t N;
  int64_t lds_bytes;           /* the dynamic LDS its N asks for */
  int32_t cloud_slot;          /* a host cloud with points: which of the call's distinct clouds
                                  (equal pointers, equal slot); else -1 */
  int32_t single;
} cmx_debug_filter_job_plan;

typedef struct cmx_debug_filter_call_plan {
  int64_t staged_bytes;        /* the clouds uploaded for the workgroups of all sets */
  int32_t num_launches;
  int32_t num_sets;
} cmx_debug_filter_call_plan;

cmx_status cmx_debug_filter_batch_plan(const cmx_filter_job* jobs, int32_t num_jobs,
                                       cmx_debug_filter_job_plan* job_plans,
                                       cmx_debug_filter_call_plan* call_plan);

/* The plan of one cmx_compute_histogram_batch call: the route of every job -- CMX_HISTOGRAM_NONE
 * (no points: zeros), CMX_HISTOGRAM_BATCHED (1 .. 4096 finite points: one workgroup of the batch
 * kernel) or CMX_HISTOGRAM_SINGLE (more points, or a non-finite coordinate: the single path
 * inside the call; the clouds of up to 4096 points are read for it) -- and for a batched job its
 * set (the consecutive parts a call goes out in; switch histogram_batch_set_kb: the bound on a
 * part's staged clouds and on its result block, default 32 MB), its launch within the set, its
 * descriptor slot, N (the LDS carve: the points rounded up to a power of two, at least 64) and the
 * dynamic LDS its N asks for; else set, launch and slot -1, N and lds_bytes 0.  A set has one
 * launch per class of N that changes how many workgroups a compute unit holds, each with the
 * LDS of its largest N.  The launch path asks the same function; this entry launches nothing and
 * needs no device.  The errors are those of the call itself, naming the job. */
enum { CMX_HISTOGRAM_NONE = 0, CMX_HISTOGRAM_BATCHED = 1, CMX_HISTOGRAM_SINGLE = 2 };
typedef struct cmx_debug_histogram_job_plan {
  int32_t route;
  int32_t set;
  int32_t launch;              /* within its set */
  int32_t slot;                /* its descriptor in the table of its set */
  int32_t N;
  int32_t cloud_slot;          /* a job with points: which of the call's distinct clouds (equal
                                  pointers, equal slot); else -1 */
  int64_t lds_bytes;
} cmx_debug_histogram_job_plan;

typedef struct cmx_debug_histogram_call_plan {
  int64_t staged_bytes;        /* the clouds uploaded for the workgroups of all sets */
  int32_t num_launches;
  int32_t num_sets;
} cmx_debug_histogram_call_plan;

cmx_status cmx_debug_histogram_batch_plan(const cmx_histogram_job* jobs, int32_t num_jobs,
                                          cmx_debug_histogram_job_plan* job_plans,
                                          cmx_debug_histogram_call_plan* call_plan);

/* The plan of one cmx_rt3d_match_grid_batch call from the options and, per match, the resolution
 * of its grid, its number of points and the largest norm of a point (a NaN or infinity stands for
 * a cloud with a non-finite coordinate, planned with the window of the smallest range, three
 * cells): the search window in steps (L, A) with its T = (2L + 1)^3
 * translations and R = (2A + 1)^3 rotations, the route (0: the segmented exhaustive launches, 1:
 * the single path), and for the segmented route the set of launches, the first block and the
 * number of blocks the match has in either launch of its set (single path: set -1, no blocks).
 * The switch rt3d_batch_route applies as it does to the call.  The launch path asks the same
 * functions; this entry needs no grid and no device.  A window beyond the limits of the library
 * (L < 512, A < 64, fewer than 2^31 candidates) is CMX_INVALID_ARGUMENT naming the match, as in
 * the call itself. */
typedef struct cmx_debug_rt3d_match_plan {
  int32_t L, A;
  int64_t T, R;
  int32_t route;
  int32_t set;
  int32_t first_block;
  int32_t blocks;
} cmx_debug_rt3d_match_plan;

cmx_status cmx_debug_rt3d_batch_plan(const cmx_rt_options* options, int32_t num_matches,
                                     const float* resolutions, const int32_t* num_points,
                                     const float* max_point_norms,
                                     cmx_debug_rt3d_match_plan* plans);

/* The plan of one cmx_ceres2d_match_grid_batch call from, per job, the kind of its grid
 * (CMX_CERES2D_PROBABILITY_GRID or CMX_CERES2D_TSDF), the identity of its host cloud
 * (`point_clouds_xyz`: compared, never read; NULL for a resident cloud and for a TSDF job without
 * points), its number of points (a resident cloud's own count) and whether its cloud is resident
 * (`resident` may be NULL: none is): the staging layout of the call's one upload block -- the
 * problem array to a 256-byte boundary (`problem_bytes`), then one slot per distinct host cloud
 * in first-seen order, each to a 256-byte boundary -- with every job's kind, cloud slot and the
 * slot's byte offset (a resident or empty cloud: slot -1, offset 0), and for the call the bytes of
 * the block, the number of distinct host clouds and the number of launches, which does not depend
 * on the list.  The launch path asks the same function; this entry launches nothing and needs no
 * device.  The errors are those of the call itself that these inputs decide, naming the job: an
 * unknown kind, a job with a host cloud and a resident one, a job with points and neither, a
 * count outside 1 .. 2^24 (0 .. 2^24 for a TSDF job), one pointer with two counts. */
enum { CMX_CERES2D_PROBABILITY_GRID = 0, CMX_CERES2D_TSDF = 1 };
typedef struct cmx_debug_ceres2d_job_plan {
  int32_t kind;
  int32_t cloud_slot;
  int64_t cloud_offset;
} cmx_debug_ceres2d_job_plan;

typedef struct cmx_debug_ceres2d_call_plan {
  int64_t total_bytes;
  int64_t problem_bytes;
  int32_t num_clouds;
  int32_t num_launches;
} cmx_debug_ceres2d_call_plan;

cmx_status cmx_debug_ceres2d_batch_plan(const int32_t* kinds, const float* const* point_clouds_xyz,
                                        const int32_t* num_points, const int32_t* resident,
                                        int32_t num_jobs, cmx_debug_ceres2d_job_plan* job_plans,
                                        cmx_debug_ceres2d_call_plan* call_plan);

/* The eight integer child sums the fast 3D branch and bound computes for a node (ScoreCandidates
 * at the node's child level, before ToProbability), by the device functions the search itself
 * calls -- a small kernel around them, nothing restated.  `cells_xyz` [num_points][3]: the
 * full-resolution cell indices of ONE discretised scan (any int32; what lies outside a level
 * reads 0); `wxy`, `wz`: the search window in voxels, in [0, 2^20).  A node is a candidate offset
 * at `level` in [1, branch_and_bound_depth - 1]; child k of it has the offset + 2^(level - 1) *
 * (k & 1, k >> 1 & 1, k >> 2 & 1).  as_family = 0: every node on its own, 1 .. 65535 of them.
 * as_family = 1: the nodes are one family (2 .. 8 nodes of one level, the children one parent
 * kept) and bit m of `live_mask` says whether member m is summed; a family the family loop does
 * not take (no oct words, more than 65536 points) goes member by member, as in the search.
 * `sums` [num_nodes][8] and `path` [num_nodes] out; the rows of dead members are left as they
 * were.  `path`: the loads that produced the row -- CMX_FAST3D_SUMS_OCT_BUFFER (oct words through
 * a buffer resource: the shipped default), _OCT_PLAIN (an oct array of 2 GB or more), _WINDOWS
 * (no oct words, child cells at most 4 apart: four 8-byte windows per point), _BYTES (a byte load
 * per child cell: switch fast3d_byte_loads, or no oct words and child cells 8 or more apart) or
 * _FAMILY (the family loop).  The switches fast3d_byte_loads (at the call) and fast3d_no_oct (at
 * the matcher's creation) apply as they do to a search.  CMX_INVALID_ARGUMENT: a null pointer,
 * num_points outside [1, 2^24], a level outside its range, a family of mixed levels or of a size
 * outside 2 .. 8, an offset beyond 2^22 cells. */
enum {
  CMX_FAST3D_SUMS_OCT_BUFFER = 0,
  CMX_FAST3D_SUMS_OCT_PLAIN = 1,
  CMX_FAST3D_SUMS_WINDOWS = 2,
  CMX_FAST3D_SUMS_BYTES = 3,
  CMX_FAST3D_SUMS_FAMILY = 4
};
typedef struct cmx_debug_fast3d_node {
  int32_t level;
  int32_t ox, oy, oz;
} cmx_debug_fast3d_node;

cmx_status cmx_debug_fast3d_child_sums(const cmx_fast3d* matcher, const int32_t* cells_xyz,
                                       int32_t num_points, int32_t wxy, int32_t wz,
                                       const cmx_debug_fast3d_node* nodes, int32_t num_nodes,
                                       int32_t as_family, uint32_t live_mask, int32_t* sums,
                                       int32_t* path);

#ifdef __cplusplus
}
#endif

#endif  /* CARTOGRAPHER_MI355X_DEBUG_H_ */
