// What the translation units of the fast 3D matcher share on the host:
//   fast_3d_stack.hip    precomputation stack and octs (Fast3DMatcher), from voxels or resident grids
//   fast_3d_stack_batch.hip  the same for the matchers of many submaps, one chain of launches
//   fast_3d_coarse.hip   staging of a chain of launches, scan discretisation, lowest-resolution
//                        scoring (the front end)
//   fast_3d.hip          branch and bound
//   fast_3d_match.hip    yaw pre-filter, Match3DMany, tie resolution, C ABI of the searches
// Every unit owns its kernels and exposes the host functions declared here; no kernel is launched
// from another file than the one that defines it.
#ifndef CMX_FAST_3D_INTERNAL_H_
#define CMX_FAST_3D_INTERNAL_H_

#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "fast_3d_device.h"

namespace cmx {

struct Fast3DMatcher {
  cmx_fast3d_options options;
  int device;
  float resolution, low_resolution;
  int width_in_voxels;
  std::vector<std::unique_ptr<DeviceBrick>> levels;
  std::vector<std::unique_ptr<DeviceBrick>> octs;   // per child level (see OctDesc)
  std::vector<OctDesc> oct_desc;
  DeviceBrick low;
  DeviceBrick high;                                 // raw uint16 grid (Ceres refinement)
  std::vector<float> histogram;
  // A matcher of cmx_fast3d_create_batch keeps everything above in ONE allocation: its bricks
  // carry `desc` and `bytes`, own no memory (mem == nullptr) and point into the slab.
  DeviceBrick slab;
};

// One submap of a batch create, checked (CheckVoxelSource3D / ResidentSource3D): voxel lists in
// host memory with their boxes, or the bricks of two resident grids.
struct Fast3DSource {
  bool resident = false;
  float resolution = 0.f, low_resolution = 0.f;
  int width_in_voxels = 0;
  const cmx_voxel* voxels[2] = {nullptr, nullptr};   // high, low
  int64_t num_voxels[2] = {0, 0};
  int lo[2][3] = {}, hi[2][3] = {};                  // VoxelBoxOrOrigin of the lists
  Brick grid[2] = {};                                // resident (cells == nullptr: still empty)
  const float* histogram = nullptr;
  int histogram_size = 0;
};

// A node's constant data with what GenerateDiscreteScans (:246-295) needs of it on the host, made
// once per call and node (NodeOf3D); the searches of one node name the same object.
struct NodeHost3D {
  const cmx_node_data3d* data;
  float max_point;                   // norm of the farthest high-resolution point
  std::vector<float> scan_hist;
  h3::Q g_inv;
};

// One (node, submap) search of a batch: MatchWithSearchParameters' arguments (:172-198).
struct Search3D {
  const Fast3DMatcher* m;
  int wxy, wz;
  double angular_search_window;
  h3::Rigid node, submap;
  float min_score;
  const NodeHost3D* data;
};

// Host side of one search: the yaw pre-filter and the candidate lattice.
struct Prepared3D {
  std::vector<h3::Q> pose_q, scan_q;
  std::vector<float> rotational_score;
  h3::V3 pose_t;
  int S = 0;
  long long ncx = 0, ncz = 0, per_scan = 0, total = 0;
  // within the chain of launches the search runs in (LayOutChain3D)
  size_t scan_base = 0, coarse_base = 0, cells_base = 0;
};

// A distinct node of a chain: its clouds are staged once.
struct Cloud3D {
  const cmx_node_data3d* data;
  float inv_cell;                 // Morton cell of the sort: its first search's
  size_t hi_floats, low_floats;   // where its clouds lie in the upload (in floats)
};

// Everything laid out for ONE chain of launches over `num` prepared searches: every kernel takes
// the array of problems (blockIdx.y, or the index its nodes carry), frontier and leaf lists are
// shared.
struct Chain3D {
  int num = 0;
  // Counts and totals over the searches.
  size_t scans_total = 0, coarse_total = 0, cells_total = 0;
  long long max_total = 0;         // most lowest-resolution candidates of one search
  int max_depth = 0, max_n = 0;
  bool same_n = true;              // every search's high-resolution cloud has max_n points
  bool one_node = true;
  std::vector<Cloud3D> clouds;     // in the order their first search comes
  std::vector<int> cloud_of;       // [num]
  // Everything the call uploads lives in ONE device buffer with ONE pinned mirror, in the order
  //   high-resolution clouds | low-resolution clouds | per-scan poses | Scan3D records (several
  //   nodes only) | misc = [Counters3 | problems | per problem: best bits, seed count | Best3]
  // and goes up in one transfer (they were four copy kernels in a chain of launches that is
  // latency from end to end); the Best3 records are only ever written on the device.
  size_t up_q = 0, up_scans = 0, up_misc = 0;                  // bytes from the block's start
  size_t off_problems = 0, off_state = 0, off_best = 0, misc_bytes = 0;   // bytes from misc's
  char* d_up = nullptr;            // (clouds at Cloud3D::hi_floats, low_floats)
  char* h_up = nullptr;
  int4* d_cells = nullptr;         // [cells_total]
  float* d_coarse = nullptr;       // [coarse_total]
  // Search scratch (ReserveSearchScratch3D): node capacities are totals over the sub-lists.
  Node3D* d_front[2] = {nullptr, nullptr};
  Node3D* d_leaves = nullptr;
  Node3D* d_seeds = nullptr;       // [num][kSeeds3]
  int frontier_capacity = 0, leaf_capacity = 0;

  float* d_xyz() const { return reinterpret_cast<float*>(d_up); }
  // per scan: pose rotation | rotation of GetPoseFromCandidate | translation + resolution
  float4* d_pose_q() const { return reinterpret_cast<float4*>(d_up + up_q); }
  float4* d_scan_q() const { return d_pose_q() + scans_total; }
  float4* d_pose_t() const { return d_scan_q() + scans_total; }
  const Scan3D* d_scans() const { return reinterpret_cast<const Scan3D*>(d_up + up_scans); }
  char* d_misc() const { return d_up + up_misc; }
  char* h_misc() const { return h_up + up_misc; }
  Counters3* d_counters() const { return reinterpret_cast<Counters3*>(d_misc()); }
  Counters3* h_counters() const { return reinterpret_cast<Counters3*>(h_misc()); }
  Fast3DProblem* d_problems() const { return reinterpret_cast<Fast3DProblem*>(d_misc() + off_problems); }
  Fast3DProblem* h_problems() const { return reinterpret_cast<Fast3DProblem*>(h_misc() + off_problems); }
  unsigned* d_state() const { return reinterpret_cast<unsigned*>(d_misc() + off_state); }   // [num][2]
  unsigned* h_state() const { return reinterpret_cast<unsigned*>(h_misc() + off_state); }
  Best3* d_best() const { return reinterpret_cast<Best3*>(d_misc() + off_best); }
  const Best3* h_best() const { return reinterpret_cast<const Best3*>(h_misc() + off_best); }
};

// What the branch and bound leaves of a chain.  The pointers name the chain's buffers: they hold
// while its workspace does.
struct Searched3D {
  const Best3* best = nullptr;     // [num] as the device selected them (ties unresolved)
  bool overflow = false;           // the lists dropped nodes (a chain of several searches)
  cmx_match_stats stats{};
  // Where the search left its leaf records: what the tie resolution reads.
  const Node3D* d_leaves = nullptr;   // [kSubLists3][leaf_sub_capacity]
  int leaf_sub_capacity = 0;
  const int* leaf_counts = nullptr;   // [kSubLists3 * kCountStride3] records per sub-list (may
                                      // exceed the capacity)
};

// Debug switch host_trace: wall clock of the host phases of one chain (tools only).
struct HostLaps3D {
  bool enabled = Debug().host_trace != 0;
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  std::string report;
  void Lap(const char* name) {
    if (!enabled) return;
    const auto now = std::chrono::steady_clock::now();
    char buf[64];
    snprintf(buf, sizeof buf, " %s=%.0f", name,
             std::chrono::duration<double, std::micro>(now - last).count());
    report += buf;
    last = now;
  }
};

// Debug switch sync: waits for what the chain has launched so far, by name (localises a fault).
inline void DebugSync3D(Workspace& ws, const char* name) {
  if (Debug().sync == 0) return;
  fprintf(stderr, "[cmx sync] %s ...\n", name);
  CMX_HIP(hipStreamSynchronize(ws.stream));
}

// ---- fast_3d_stack.hip
// The argument checks of cmx_fast3d_create short of grid_size (which takes a pass over the list).
void CheckVoxelSource3D(float resolution, const cmx_voxel* voxels, int64_t num_voxels,
                        float low_resolution, const cmx_voxel* low_resolution_voxels,
                        int64_t num_low_resolution_voxels, const float* histogram,
                        int32_t histogram_size);
// The argument checks of cmx_fast3d_create_from_grids; bricks (zeroed for a grid that is still
// empty), resolutions and grid_size of the pair, the device both live on.
void ResidentSource3D(const cmx_grid3d* high_resolution_grid, const cmx_grid3d* low_resolution_grid,
                      const float* histogram, int32_t histogram_size, Brick grid[2],
                      float resolution[2], int32_t* grid_size, int* device);

// ---- fast_3d_stack_batch.hip
// The matchers of `num` checked sources on `device`, built by chains of launches whose length
// does not depend on `num`; all or nothing (an exception leaves nothing allocated).
std::vector<std::unique_ptr<cmx_fast3d>> BuildFast3DBatch(const cmx_fast3d_options& options,
                                                          const Fast3DSource* sources, int num,
                                                          int device);

// ---- fast_3d_coarse.hip
// Totals, bases (into `prep`) and the layout of the upload block; host only.  False: no search
// has a scan left, there is nothing to run.
bool LayOutChain3D(const Search3D* searches, Prepared3D* prep, int num, Chain3D* chain);
// The upload block, its pinned mirror, the cells and the lowest-resolution scores.
void ReserveChainBuffers3D(Workspace& ws, Chain3D* chain);
// After ReserveSearchScratch3D (the problems name their seeds): fills the pinned mirror -- poses,
// Scan3D records, problems, states, the clouds (high-resolution ones Morton-sorted) -- and sends
// it up in one transfer.
void StageAndUploadChain3D(Workspace& ws, const Search3D* searches, const Prepared3D* prep,
                           const Chain3D& chain);
// Discretises every scan and scores every lowest-resolution candidate of the chain.
void DiscretizeAndScoreCoarse3D(Workspace& ws, const Chain3D& chain, StageTrace* trace);

// ---- fast_3d.hip
// Before StageAndUploadChain3D: the frontier, leaf and seed buffers.
void ReserveSearchScratch3D(Workspace& ws, Chain3D* chain);
// Seeds, dives, filter, expansions and selection of a scored chain, synchronised.  A single
// search whose frontier overflows is retried here (strict, then in chunks), its bound restarted
// from `first_min_score`, the search's min_score; a chain of several reports `overflow`.
void RunBranchAndBound3D(Workspace& ws, const Chain3D& chain, float first_min_score,
                         StageTrace* trace, HostLaps3D* laps, Searched3D* searched);

}  // namespace cmx

struct cmx_fast3d {
  cmx::Fast3DMatcher impl;
};

#endif  // CMX_FAST_3D_INTERNAL_H_
