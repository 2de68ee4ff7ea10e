// What the translation units of the real-time 3D matcher share on the host:
//   rt_3d.hip         search space, mode, uploads, Rt3DMatch, final weighting, the C ABI
//   rt_3d_exact.hip   the reference's own arithmetic: f32 probability brick, exhaustive search,
//                     exact scores of the bounds search's finalists
//   rt_3d_bounds.hip  integer bounds: q bricks, the gather passes, selection, the stages of the
//                     bounds search
//   rt_3d_tiles.hip   the same integer sums on LDS tiles: bin sort, chunk boxes, tile kernel
//   rt_3d_batch.hip   cmx_rt3d_match_grid_batch: the exhaustive search of many small matches in
//                     one segmented launch, on the resident uint16 bricks (rt_3d_batch_plan.h)
// (dense_brick_3d.hip, declared in scan_matching_3d.h, has the dense-brick helpers every 3D
// matcher uses.)  Every unit owns its kernels and exposes the host functions declared here; no
// kernel is launched from another file than the one that defines it.  The functions that cross
// units take the host structs below, never a device-visible type: those live in every unit's own
// unnamed namespace (rt_3d_device.h).
#ifndef CMX_RT_3D_INTERNAL_H_
#define CMX_RT_3D_INTERNAL_H_

#include <optional>
#include <vector>

#include "rt_3d_batch_plan.h"
#include "rt_3d_device.h"

namespace cmx {

// Workspace buffers (Workspace::dev) of the family, one name per slot.
enum Rt3DSlot {
  kSlotCloud = 0,            // the cloud as uploaded
  kSlotRotations = 1,
  kSlotTranslations = 2,
  kSlotAngles = 3,
  kSlotUnweighted = 4,       // exhaustive search: unweighted scores; bounds search: work items
  kSlotWeighted = 5,         // exhaustive search: weighted scores; bounds search: candidate bounds
  kSlotMisc = 6,             // Rt3DExhaustiveMisc
  kSlotProbabilities = 7,    // the padded f32 brick
  kSlotQBrick = 8,           // q = value >> 7: row-major | tiled
  kSlotDilated = 9,
  kSlotScratch = 10,         // dilation scratch, then the (Q, A) sums of the candidate passes
  kSlotGroupUpper = 11,
  kSlotFlags = 12,           // [R][G] group expanded | [R][T] candidate flagged
  kSlotBulkMisc = 13,        // Rt3DBulkHead | counts per rotation | work blocks | Rt3DCounters
  kSlotGroups = 14,
  kSlotVoxels = 15,          // the voxel list as uploaded (UploadVoxels, dense_brick_3d.hip)
  kSlotSorted = 16,          // the cloud sorted into bins
  kSlotBins = 17,
  kSlotGroupSums = 18,
  kSlotCrosscheck = 19,      // rt3d_crosscheck: the gather kernels' results
  kSlotGroupBoxes = 20,
  kSlotListBoxes = 21,
  kSlotStageBounds = 22,     // rt3d_verify: what the staged round decided
  kSlotStageDropped = 23,
  kSlotBlockRotations = 24,
  kSlotBlockAngles = 25,
  kSlotDilatedTwice = 26,
  kSlotBlockBounds = 27,
  kSlotPairs = 28,           // [R][G] pair computed | [R][G] pair flagged
  kSlotReport = 29,          // rt3d_report: the tile kernels' counters
};
// ... and of Workspace::pinned.
enum Rt3DPinnedSlot { kPinnedReadBack = 1, kPinnedBulkHead = 2, kPinnedGroups = 3 };

// What is computed before the GPU is touched: GenerateExhaustiveSearchTransforms (:55-95) and
// the 2 x 2 x 2 blocks of its two lattices.
struct Rt3DSearchSpace {
  int n = 0;                         // points
  float resolution = 0.f;
  int L = 0, A = 0;                  // linear / angular window in steps
  float step = 0.f;                  // angular step
  int side_t = 0, side_r = 0;
  long long T = 0, R = 0, num_candidates = 0;
  h3::Rigid init;
  std::vector<float4> rot;           // [R] normalized(init.q * q_r), (x, y, z, w)
  std::vector<float4> trans;         // [T] init.q * t_c + init.t; w = |t_c|
  std::vector<float> angle;          // [R] GetAngle(transform)
  // Rotation blocks (see Rt3DSelectPairsKernel): the centre rotation and the smallest member
  // angle of each.
  int Ab = 0;
  long long Rb = 0;
  std::vector<float4> rot_b;
  std::vector<float> angle_b;
  // Translation groups: centre translation; w = the smallest member distance.
  int gpa = 0, G = 0;
  std::vector<float4> group;
};

// The HybridGrid of a call: the voxel list (host memory) or, when `resident` is set, the dense
// uint16 brick cmx_grid3d keeps in HBM (`voxels` unused then).
struct Rt3DGridSource {
  const cmx_voxel* voxels;
  int64_t num_voxels;
  const Brick* resident;
};

// The bricks of the bounds search: the grid's box widened by `pad` cells on every side.
struct Rt3DBulkGeometry {
  int reach = 0;                    // |init.q * t_c| in cells, rounded up
  int pad = 0;
  long long bx = 0, by = 0, bz = 0; // (rows a multiple of 4 cells: the tiled passes copy boxes
                                    // of the brick with aligned dwords)
  size_t cells = 0;
  int tiles_x = 0, tiles_y = 0, pitch_z = 0;   // the tiled brick, see TiledOffset
  size_t tiled_cells = 0;
};

// Which of the equivalent paths run, and their tuning: the debug switches (all zero in
// production; parity tests run every path) and the problem sizes, read in one place.
struct Rt3DMode {
  bool use_bulk;          // integer bounds before the exact scores (else: exhaustive search only)
  bool use_tiles;         // bulk passes on LDS tiles (else: memory gathers, Rt3DBulkKernel)
  bool crosscheck;        // tiled passes next to the gather kernels, every sum compared
  bool use_boxes;         // chunk boxes from a pre-pass kernel (else: reduced per chunk in the tile kernel)
  bool staged;            // second candidate round segment by segment (Rt3DStageFilterKernel)
  bool rotblocks;         // the rotation-block level above the group pass (Rt3DSelectPairsKernel)
  bool verify;            // every bound checked on the device against what it bounds
  bool report;            // pass-by-pass report on stderr
  bool expand_all;        // every group expanded in the first round
  int rot_per_block;      // rotations of a group-pass workgroup
  int list_rotations;     // rotations sharing one work list of the tiled list passes
  int block_items;        // items per work block of the candidate passes
  int group_tile_capacity, cand_tile_capacity;   // bytes of LDS tile
  int group_fixed_point;  // group centres in packed fixed point (0: f32)
  int sixteenths0, sixteenths1;                  // ends of point segments 0 and 1, per window
  float first_pair_factor, first_round_factor;   // thresholds of the first rounds
};

// What a call keeps on the device for both searches.
struct Rt3DDevice {
  PaddedBrick brick;                 // f32 probabilities, border of kMinProbability
  const cmx_voxel* d_vox = nullptr;  // the uploaded voxel list, or null (none, or a resident grid)
  float* d_xyz = nullptr;
  float4 *d_rot = nullptr, *d_trans = nullptr, *d_rot_b = nullptr;
  float *d_angle = nullptr, *d_angle_b = nullptr;
  float *d_unweighted = nullptr, *d_weighted = nullptr;   // [num_candidates] each
  Rt3DExhaustiveMisc* d_misc = nullptr;
  Rt3DPinnedReadBack* pinned = nullptr;
  Rt3DParams P;
};

// What either search hands to the final weighting, and what the bounds search counted.
struct Rt3DFinalists {
  std::vector<long long> index;      // reference candidate index t * R + r, ascending
  std::vector<float> acc;            // their exact unweighted scores
  int num_finalists = 0;             // bounds search: candidates re-scored exactly
  long long bounds_evaluated = 0;
  long long group_bounds = 0;        // bounds above the candidates: rotation blocks + (rotation, group) pairs
  bool second_pairs_pass = false;    // (its span: ev_x0 .. ev_x1)
};

// What crosses between the stages of the bounds search.
struct Rt3DBoundsSearch {
  Workspace* ws = nullptr;
  const Rt3DSearchSpace* S = nullptr;
  const Rt3DDevice* D = nullptr;
  Rt3DMode mode{};
  Rt3DBulkGeometry geo;
  int cus = 256;
  long long RG = 0;                  // (rotation, group) pairs
  int num_lists = 0;                 // work lists of the list passes
  int max_chunks = 0;                // capacity of either chunk list
  // bricks of q = value >> 7
  uint8_t* d_rows = nullptr;         // row-major (the input of the dilation, the tiled passes)
  uint8_t* d_tiled = nullptr;        // columns of 8 x 4 cells (the gather candidate pass)
  uint8_t* d_dilated = nullptr;      // 2 x 2 x 2 maximum: the group pass
  uint8_t* d_tmp = nullptr;          // dilation scratch first, then the candidates' (Q, A)
  // groups and candidates
  float4* d_group = nullptr;
  float* d_group_upper = nullptr;    // [R][G]
  uint2* d_group_sums = nullptr;     // tiled passes: [R][G] totals (| [R][G] per segment: staged)
  uint8_t* d_expanded = nullptr;     // [R][G]
  uint8_t* d_flags = nullptr;        // [R][T]
  float* d_upper = nullptr;          // [R][T], the exhaustive search's weighted scores reused
  int* d_items = nullptr;            // [R][T], ... unweighted scores reused
  Rt3DBulkHead* d_head = nullptr;
  int* d_counts = nullptr;           // [R] items per rotation
  int2* d_blocks = nullptr;          // work descriptors of a round
  Rt3DCounters* d_counters = nullptr;
  Rt3DBulkHead* h_head = nullptr;    // pinned
  Rt3DReadBack* h_read = nullptr;    // pinned
  // tiled passes
  int* d_segment_counts = nullptr;   // Rt3DSegmentCount
  float* d_list_boxes = nullptr;     // chunk boxes of the candidate chunk list, per work list
  // rotation blocks
  uint8_t* d_computed = nullptr;     // [R][G] pair computed | [R][G] pair flagged
  uint8_t* d_dilated_twice = nullptr;   // 5 x 5 x 5 maximum
  uint2* d_block_sums = nullptr;     // [Rb][G]
  float* d_block_upper = nullptr;    // [Rb][G]
  unsigned* d_block_max = nullptr;
  Rt3DBulkParams base{};             // what every pass shares
  Rt3DTileParams tiles{};            // ... every tiled pass: sorted cloud, group chunk list
  int round_blocks[2] = {0, 0};
  int stage_blocks[2] = {-1, -1};    // work blocks left after segments 0 and 1
  bool second_pairs_pass = false;
  std::optional<StageTrace> trace;

  hipStream_t stream() const { return ws->stream; }
};

// ---- the parameter sets of the passes: what differs from the base -----------------------------

// Group pass: every rotation, every block of translations, on the dilated brick.
inline Rt3DBulkParams GroupParams(const Rt3DBoundsSearch& run) {
  Rt3DBulkParams p = run.base;
  p.cells = run.d_dilated;
  p.translation = run.d_group; p.num_translations = run.S->G;
  p.upper = run.d_group_upper;
  p.sums = run.d_group_sums;
  return p;
}

// Rotation blocks: the group pass over the centre rotations of the blocks, on the twice-dilated
// brick, into bounds of their own.
inline Rt3DBulkParams BlockParams(const Rt3DBoundsSearch& run) {
  Rt3DBulkParams p = GroupParams(run);
  p.cells = run.d_dilated_twice;
  p.num_rotations = static_cast<int>(run.S->Rb);
  p.rotation = run.D->d_rot_b; p.rotation_angle = run.D->d_angle_b;
  p.upper = run.d_block_upper; p.sums = run.d_block_sums;
  p.max_upper_bits = run.d_block_max;
  return p;
}

// Sparse pair pass: the group pass over work lists of (rotation, group) pairs, on the
// candidate pass's chunk list (256 points).
constexpr int kPairItems = 512;
inline Rt3DBulkParams PairParams(const Rt3DBoundsSearch& run) {
  Rt3DBulkParams p = GroupParams(run);
  p.counts = run.d_counts; p.items = run.d_items; p.blocks = run.d_blocks;
  p.list_rotations = run.mode.list_rotations; p.block_items = kPairItems;
  return p;
}

// Candidate passes: work lists over the translation table; the tiled brick for the gathers, the
// row-major one for the tiles.
inline Rt3DBulkParams CandidateParams(const Rt3DBoundsSearch& run) {
  Rt3DBulkParams p = run.base;
  p.cells = run.d_tiled;
  p.cell_count = static_cast<unsigned>(run.geo.tiled_cells);
  p.tiles_y = run.geo.tiles_y; p.pitch_z = run.geo.pitch_z;
  p.translation = run.D->d_trans; p.num_translations = static_cast<int>(run.S->T);
  p.counts = run.d_counts; p.items = run.d_items; p.blocks = run.d_blocks;
  p.upper = run.d_upper;
  p.sums = reinterpret_cast<uint2*>(run.d_tmp);
  p.block_items = run.mode.block_items;
  p.list_rotations = run.mode.list_rotations;
  if (run.mode.use_tiles) {
    p.cells = run.d_rows;
    p.cell_count = static_cast<unsigned>(run.geo.cells);
  }
  return p;
}

// ---- rt_3d.hip (what the batched call of rt_3d_batch.hip shares with the single one)
// The search space of a window Rt3DWindowOf found supported, without the rotation blocks and
// translation groups of the bounds search.
Rt3DSearchSpace SearchSpaceOf(const Rt3DWindow& W, float resolution,
                              const cmx_pose3d& initial_pose_estimate, int n);
// Exact weighting and the strict '>' first-maximum rule over the finalists.
void PickBest(const Rt3DSearchSpace& S, double wt, double wr, const Rt3DFinalists& fin,
              float* score, cmx_pose3d* pose_estimate);
// The single match: cmx_rt3d_match (a voxel list) and cmx_rt3d_match_grid (`resident`).
void Rt3DMatch(const cmx_rt_options* options, float grid_resolution, const cmx_voxel* voxels,
               int64_t num_voxels, const Brick* resident, const cmx_pose3d* initial_pose_estimate,
               const float* point_cloud_xyz, int32_t num_points, int32_t device, float* score,
               cmx_pose3d* pose_estimate, cmx_match_stats* stats);

// ---- rt_3d_exact.hip
// Padded f32 probability brick over the box D->brick names (no cells yet), filled with
// kMinProbability and then with the voxels (uploaded here) or the resident brick's cells.
void BuildProbabilityBrick(Workspace& ws, const Rt3DGridSource& grid, Rt3DDevice* D);
// Every candidate on the one-thread-per-candidate kernel; finalists = the candidates within
// 1e-5 (relative) of the best weighted score, or all of them when the list overflows.
void RunExhaustiveSearch(Workspace& ws, const Rt3DSearchSpace& S, const Rt3DDevice& D,
                         Rt3DFinalists* out);
// Bounds search: the candidates whose upper bound reaches the best lower bound into the head's
// finalist list, and their exact scores next to them (enqueued).
void CollectAndScoreFinalists(Rt3DBoundsSearch* run);

// ---- rt_3d_tiles.hip
// The tiled passes compute the sums the gather kernels of rt_3d_bounds.hip compute; the chunk
// lists, the LDS layout, the slice counts and the LDS opt-ins stay behind these calls.
// The cloud sorted into bins at the central candidate, and the two chunk lists over the bins
// (run->max_chunks, d_segment_counts and tiles are set here).
void SortCloudIntoBins(Rt3DBoundsSearch* run);
// Chunk boxes of the list passes below (mode.use_boxes), once per match.
void BoxListChunks(Rt3DBoundsSearch* run);
// Dense group pass: the sums of every group under every rotation (GroupParams), or under the
// centre rotation of every rotation block (BlockParams).
void TileGroups(Rt3DBoundsSearch* run, bool rotation_blocks);
// Group pass over the `blocks` work blocks of (rotation, group) pairs just compacted
// (PairParams); `list_chunks`: the candidate chunk list's length as read back.
void TilePairs(Rt3DBoundsSearch* run, int blocks, int list_chunks);
// Candidate pass over `blocks` work blocks (CandidateParams) and the chunks of point segments
// seg_first .. seg_last, `chunks` of them at most (0 .. 2: every chunk of the list).
void TileCandidates(Rt3DBoundsSearch* run, int blocks, int seg_first, int seg_last, int chunks);
// rt3d_report: what the tile kernels of the group level counted.
void ReportGroupTiles(Rt3DBoundsSearch* run);

// ---- rt_3d_bounds.hip
// The bounds search; false when it did not narrow the search down (a flat score landscape: more
// finalists than the list holds) -- every candidate on the per-candidate kernel then.
bool RunBoundsSearch(Workspace& ws, const Rt3DSearchSpace& S, const Rt3DMode& mode,
                     const Rt3DBulkGeometry& geo, const Rt3DDevice& D, const Rt3DGridSource& grid,
                     Rt3DFinalists* out);

}  // namespace cmx

#endif  // CMX_RT_3D_INTERNAL_H_
