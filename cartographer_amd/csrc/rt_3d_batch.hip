// cmx_rt3d_match_grid_batch: RealTimeCorrelativeScanMatcher3D::Match for many (grid, scan) pairs
// in one call -- LocalTrajectoryBuilder3D::ScanMatch's first half (mapping/internal/3d/
// local_trajectory_builder_3d.cc:96-108) for a fleet -- bit for bit the single calls of rt_3d.hip.
//
// The window the reference's configuration asks for (0.15 m / 1 degree: 125 translations x 343
// rotations, a few hundred points) is far too small for the single call's machinery: a padded f32
// copy of the brick, six uploads, a bounds search in rounds with read-backs.  Such matches take
// the SEGMENTED route: one score launch over every candidate of every match and one collect
// launch, two launches, one upload, one read-back and one synchronisation per set of launches.
//   * A block is 64 translations of one rotation, Rt3DScoreKernel's wavefront, and finds its match
//     by bisection over the first blocks of the descriptors (DescOfBlock).  The arithmetic is that
//     kernel's, operation by operation: points in cloud order, rotated once per wavefront into LDS,
//     FastCellIndex with the CellIndex3 fallback, a sequential f32 sum, / float(n).
//   * The resident uint16 brick is read where it lies: an index outside it, or a stored 0, is the
//     kMinProbability (0.1f) the padded brick is filled with, any other value
//     ValueToProbabilityDev(value), what BrickProbabilitiesKernel stores.  A grid nothing was
//     inserted into is a brick of no cells and no memory.
//   * The finish is the single exhaustive search's: atomicMax of the device-weighted score per
//     match, the candidates within 1e-5 (relative) of it collected with their unweighted scores,
//     exp weighting and the strict-'>' first maximum on the host (PickBest).  A match's list holds
//     kBatchFinalistCap entries; a match whose list overflows (a flat landscape) runs again
//     through the single path.
// Matches with more work than kRt3DSegmentedMaxWork, or a non-finite coordinate, run through
// Rt3DMatch one after the other behind the segmented part (rt_3d_batch_plan.h has the plan).
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/cartographer_mi355x_debug.h"
#include "cmx_batch.h"
#include "grid_3d_internal.h"
#include "rt_3d_internal.h"

namespace cmx {
namespace {

constexpr int kBatchFinalistCap = 128;     // per match: 1 KB of read-back

struct Rt3DBatchHead {
  unsigned max_bits;                       // atomicMax of the weighted scores
  int count;                               // candidates collected (may exceed the capacity)
  int reserved[2];
};

struct Rt3DBatchDesc {
  const uint16_t* cells;                   // the resident brick (any mapped address when empty)
  unsigned cell_bytes;                     // 0: nothing inserted yet
  int lo_x, lo_y, lo_z, nx, ny, nz;
  float resolution, inv_resolution;
  int n, T, R;
  int tiles;                               // blocks per rotation: ceil(T / 64)
  int first_block;                         // in either launch of its set
  const float* xyz;                        // staged cloud
  const float4* rot;                       // [R], as Rt3DParams
  const float4* trans;                     // [T]
  const float* angle;                      // [R]
  float* unweighted;                       // [T * R], candidate t * R + r
  float* weighted;
  Rt3DBatchHead* head;
  int* finalists;                          // [kBatchFinalistCap] candidate index
  float* finalist_acc;                     // ... and its unweighted score
};

// Rt3DScoreKernel (rt_3d_exact.hip) for the block's match, on the uint16 brick.
__global__ void __launch_bounds__(kRt3DBatchLanes)
Rt3DBatchScoreKernel(const Rt3DBatchDesc* __restrict__ descs, int num, double wt, double wr) {
  __shared__ float4 rotated[64];
  const Rt3DBatchDesc& D =
      descs[DescOfBlock<&Rt3DBatchDesc::first_block>(descs, num, blockIdx.x)];
  const int local = blockIdx.x - D.first_block;
  const int r = local / D.tiles;
  const int lane = threadIdx.x;
  const int t = (local - r * D.tiles) * 64 + lane;
  const bool valid = t < D.T;
  const int n = D.n;
  const float* __restrict__ xyz = D.xyz;
  const float4 q4 = D.rot[r];
  const Quat q{q4.w, q4.x, q4.y, q4.z};
  const float4 tr = D.trans[valid ? t : 0];
  const float res = D.resolution, inv = D.inv_resolution;
  const unsigned lo_x = D.lo_x, lo_y = D.lo_y, lo_z = D.lo_z;
  const unsigned nx = D.nx, ny = D.ny, nz = D.nz;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(D.cells), 0, D.cell_bytes, 0x00020000);

  // (byte offset of the cell, or -1 outside the brick)
  const auto cell_offset = [&](const float4& rp) -> int {
    const float cx = rp.x + tr.x, cy = rp.y + tr.y, cz = rp.z + tr.z;   // rigid * point
    bool ok = true;
    int ix = FastCellIndex(cx, inv, &ok);
    int iy = FastCellIndex(cy, inv, &ok);
    int iz = FastCellIndex(cz, inv, &ok);
    if (!ok) {
      const int3 idx = CellIndex3(F3{cx, cy, cz}, res);
      ix = idx.x; iy = idx.y; iz = idx.z;
    }
    const unsigned ux = static_cast<unsigned>(ix) - lo_x, uy = static_cast<unsigned>(iy) - lo_y,
                   uz = static_cast<unsigned>(iz) - lo_z;
    const bool inside = ux < nx && uy < ny && uz < nz;
    return inside ? static_cast<int>(((uz * ny + uy) * nx + ux) * 2u) : -1;
  };
  // An unconditional load from offset 0 for the cells outside (none at all from a brick of no
  // cells: the range check of the descriptor drops it), masked afterwards.
  const auto probability = [&](int offset) -> float {
    const unsigned raw = __builtin_amdgcn_raw_buffer_load_b16(rsrc, max(offset, 0), 0, 0);
    const unsigned value = offset >= 0 ? raw : 0u;
    return value == 0u ? 0.1f : ValueToProbabilityDev(value);
  };

  float acc = 0.f;
  constexpr int kBatch = 8;
  for (int base = 0; base < n; base += 64) {
    const int cnt = min(64, n - base);
    __syncthreads();                       // previous chunk fully consumed
    if (lane < cnt) {
      const int i = base + lane;
      const F3 rp = Rotate(q, F3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
      rotated[lane] = make_float4(rp.x, rp.y, rp.z, 0.f);
    }
    __syncthreads();
    int j = 0;
    for (; j + kBatch <= cnt; j += kBatch) {
      float v[kBatch];
#pragma unroll
      for (int k = 0; k < kBatch; ++k) v[k] = probability(cell_offset(rotated[j + k]));
#pragma unroll
      for (int k = 0; k < kBatch; ++k) acc += v[k];
    }
    for (; j < cnt; ++j) acc += probability(cell_offset(rotated[j]));
  }

  float w = 0.f;
  if (valid) {
    acc /= static_cast<float>(n);
    // Candidate order of the reference: z, y, x, rz, ry, rx nesting.
    const size_t c = static_cast<size_t>(t) * D.R + r;
    D.unweighted[c] = acc;
    const double penalty = static_cast<double>(tr.w) * wt + static_cast<double>(D.angle[r]) * wr;
    w = static_cast<float>(static_cast<double>(acc) * exp(-(penalty * penalty)));
    D.weighted[c] = w;
  }
  unsigned bits = __float_as_uint(w);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bits = max(bits, __shfl_xor(bits, off, 64));
  if (threadIdx.x == 0) atomicMax(&D.head->max_bits, bits);
}

// Rt3DCollectKernel over the same blocks; a finalist's unweighted score goes next to its index.
__global__ void __launch_bounds__(kRt3DBatchLanes)
Rt3DBatchCollectKernel(const Rt3DBatchDesc* __restrict__ descs, int num) {
  const Rt3DBatchDesc& D =
      descs[DescOfBlock<&Rt3DBatchDesc::first_block>(descs, num, blockIdx.x)];
  const int local = blockIdx.x - D.first_block;
  const int r = local / D.tiles;
  const int t = (local - r * D.tiles) * 64 + threadIdx.x;
  if (t >= D.T) return;
  const size_t c = static_cast<size_t>(t) * D.R + r;
  const float threshold = __uint_as_float(D.head->max_bits) * (1.f - 1e-5f);
  if (D.weighted[c] >= threshold) {
    const int slot = atomicAdd(&D.head->count, 1);
    if (slot < kBatchFinalistCap) {
      D.finalists[slot] = static_cast<int>(c);
      D.finalist_acc[slot] = D.unweighted[c];
    }
  }
}

// ---- host ------------------------------------------------------------------------------
struct BatchMatch {                        // a match as the checks leave it
  Brick brick{};                           // (no cells: nothing inserted yet)
  bool empty = true;
  float resolution = 0.f;
};

bool AllFinite(const float* xyz, int n) {
  for (int i = 0; i < 3 * n; ++i)
    if (!std::isfinite(xyz[i])) return false;
  return true;
}

void AddStats(const cmx_match_stats& one, cmx_match_stats* sum) {
  sum->candidates_scored += one.candidates_scored;
  sum->coarse_candidates += one.coarse_candidates;
  sum->num_scans += one.num_scans;
  sum->nodes_expanded += one.nodes_expanded;
  sum->device_ms += one.device_ms;
}

void MatchBatch(const cmx_rt_options* options, const cmx_grid3d* const* grids, int num,
                const cmx_pose3d* initial_pose_estimates, const float* const* point_clouds_xyz,
                const int32_t* num_points, float* scores, cmx_pose3d* pose_estimates,
                cmx_match_stats* stats) {
  // Every argument check, and the host-only limits of the search space, before the device is
  // touched.
  CMX_REQUIRE(num >= 1, "num_matches %d < 1", num);
  CMX_REQUIRE(options && grids && initial_pose_estimates && point_clouds_xyz && num_points,
              "null argument");
  CMX_REQUIRE(scores != nullptr && pose_estimates != nullptr,
              "scores and pose_estimates must not be null");
  for (int k = 0; k < num; ++k) {          // (no grid is looked into before all are known to be there)
    CMX_REQUIRE(grids[k] != nullptr, "match %d: null grid", k);
    CMX_REQUIRE(point_clouds_xyz[k] != nullptr, "match %d: null point cloud", k);
    CMX_REQUIRE(num_points[k] >= 1 && num_points[k] <= (1 << 24), "match %d: bad point count", k);
  }
  StagedArrays clouds(3);
  std::vector<BatchMatch> matches(num);
  std::vector<Rt3DMatchInput> inputs(num);
  int device = 0;
  for (int k = 0; k < num; ++k) {
    BatchMatch& M = matches[k];
    int d = 0;
    M.empty = !Grid3DBrick(grids[k], &M.brick, &M.resolution, &d);
    CMX_REQUIRE(k == 0 || d == device, "match %d: all grids of a batch must live on one device", k);
    device = d;
    clouds.Add(k, point_clouds_xyz[k], num_points[k], [](int item, int there, int here) {
      CMX_REQUIRE(false,
                  "match %d: point cloud given by the pointer of an earlier cloud of the call, "
                  "%d points there and %d here",
                  item, there, here);
    });
    Rt3DMatchInput& I = inputs[k];
    I.window = Rt3DWindowOf(*options, M.resolution,
                            Rt3DScanRange(M.resolution, point_clouds_xyz[k], num_points[k]));
    CMX_REQUIRE(I.window.unsupported == nullptr, "match %d: %s", k, I.window.unsupported);
    I.num_points = num_points[k];
    I.finite = AllFinite(point_clouds_xyz[k], num_points[k]);
    I.brick_in_reach =
        M.empty || static_cast<long long>(M.brick.nx) * M.brick.ny * M.brick.nz < (1ll << 29);
  }
  const Rt3DBatchPlan plan = PlanRt3DBatch(inputs.data(), num, Debug().rt3d_batch_route);

  std::vector<float> out_scores(num);
  std::vector<cmx_pose3d> out_poses(num);
  cmx_match_stats total{};
  std::vector<int> singles = plan.singles;
  {
    WorkspaceLease ws(device);
    hipStream_t stream = ws->stream;
    const double wt = options->translation_delta_cost_weight;
    const double wr = options->rotation_delta_cost_weight;
    for (const LaunchSet& set : plan.sets) {
      const int n_set = set.end - set.begin;
      // The search spaces, and the clouds of this set, each distinct pointer once.
      std::vector<Rt3DSearchSpace> spaces(n_set);
      StagedArrays staged(3);
      long long sum_r = 0, sum_t = 0;
      for (int s = 0; s < n_set; ++s) {
        const int k = plan.match_of_slot[set.begin + s];
        spaces[s] = SearchSpaceOf(inputs[k].window, matches[k].resolution,
                                  initial_pose_estimates[k], num_points[k]);
        staged.Add(k, point_clouds_xyz[k], num_points[k], [](int, int, int) {});
        sum_r += spaces[s].R;
        sum_t += spaces[s].T;
      }
      // One block: descriptors | tables | clouds | zeroed heads (uploaded so far) | finalists
      // (heads and finalists come back in one copy).
      BlockLayout block;
      const auto descs_in = block.Add<Rt3DBatchDesc>(n_set);
      const auto rot_in = block.Add<float4>(sum_r);
      const auto trans_in = block.Add<float4>(sum_t);
      const auto angle_in = block.Add<float>(sum_r);
      const auto points_in = block.Add<float>(staged.floats());
      const auto heads_in = block.Add<Rt3DBatchHead>(n_set);
      const size_t upload_bytes = block.bytes;
      const auto finalists_in = block.Add<int>(static_cast<size_t>(kBatchFinalistCap) * n_set);
      const auto acc_in = block.Add<float>(static_cast<size_t>(kBatchFinalistCap) * n_set);
      char* h_block = static_cast<char*>(ws->pinned[0].Reserve(block.bytes));
      char* d_block = static_cast<char*>(ws->dev[0].Reserve(block.bytes));
      float* d_unweighted = ws->dev[1].ReserveAs<float>(set.total[1]);
      float* d_weighted = ws->dev[2].ReserveAs<float>(set.total[1]);
      staged.CopyTo(points_in(h_block), [](int n, const std::function<void(int)>& copy) {
        ParallelFor(n, 8, copy);
      });
      std::memset(heads_in(h_block), 0, sizeof(Rt3DBatchHead) * n_set);
      long long at_r = 0, at_t = 0, at_c = 0;
      for (int s = 0; s < n_set; ++s) {
        const int k = plan.match_of_slot[set.begin + s];
        const Rt3DSearchSpace& S = spaces[s];
        const BatchMatch& M = matches[k];
        std::memcpy(rot_in(h_block) + at_r, S.rot.data(), sizeof(float4) * S.R);
        std::memcpy(angle_in(h_block) + at_r, S.angle.data(), sizeof(float) * S.R);
        std::memcpy(trans_in(h_block) + at_t, S.trans.data(), sizeof(float4) * S.T);
        Rt3DBatchDesc D{};
        if (M.empty) {
          D.cells = reinterpret_cast<const uint16_t*>(d_block);
        } else {
          D.cells = static_cast<const uint16_t*>(M.brick.cells);
          D.cell_bytes = static_cast<unsigned>(2ll * M.brick.nx * M.brick.ny * M.brick.nz);
          D.lo_x = M.brick.lo_x; D.lo_y = M.brick.lo_y; D.lo_z = M.brick.lo_z;
          D.nx = M.brick.nx; D.ny = M.brick.ny; D.nz = M.brick.nz;
        }
        D.resolution = S.resolution;
        D.inv_resolution = 1.f / S.resolution;
        D.n = S.n;
        D.T = static_cast<int>(S.T);
        D.R = static_cast<int>(S.R);
        D.tiles = static_cast<int>(BlocksOf(S.T, kRt3DBatchLanes));
        D.first_block = plan.matches[k].first_block;
        D.xyz = points_in(d_block) + staged.OffsetOf(point_clouds_xyz[k]);
        D.rot = rot_in(d_block) + at_r;
        D.angle = angle_in(d_block) + at_r;
        D.trans = trans_in(d_block) + at_t;
        D.unweighted = d_unweighted + at_c;
        D.weighted = d_weighted + at_c;
        D.head = heads_in(d_block) + s;
        D.finalists = finalists_in(d_block) + static_cast<size_t>(kBatchFinalistCap) * s;
        D.finalist_acc = acc_in(d_block) + static_cast<size_t>(kBatchFinalistCap) * s;
        descs_in(h_block)[s] = D;
        at_r += S.R; at_t += S.T; at_c += S.num_candidates;
      }
      const Rt3DBatchDesc* d_descs = descs_in(d_block);
      const unsigned blocks = static_cast<unsigned>(set.total[0]);
      SmallCopyAsync(d_block, h_block, upload_bytes, /*to_device=*/true, stream);
      RecordEvent(ws->ev_begin, stream);
      Rt3DBatchScoreKernel<<<blocks, kRt3DBatchLanes, 0, stream>>>(d_descs, n_set, wt, wr);
      Rt3DBatchCollectKernel<<<blocks, kRt3DBatchLanes, 0, stream>>>(d_descs, n_set);
      CMX_HIP(hipGetLastError());
      RecordEvent(ws->ev_end, stream);
      SmallCopyAsync(h_block + heads_in.at, d_block + heads_in.at, block.bytes - heads_in.at,
                     /*to_device=*/false, stream);
      CMX_HIP(hipStreamSynchronize(stream));
      total.device_ms += ElapsedMs(ws->ev_begin, ws->ev_end);

      for (int s = 0; s < n_set; ++s) {
        const int k = plan.match_of_slot[set.begin + s];
        const Rt3DSearchSpace& S = spaces[s];
        const int count = heads_in(h_block)[s].count;
        if (count > kBatchFinalistCap) {     // a flat landscape: the single path sorts it out
          singles.push_back(k);
          continue;
        }
        const int* index = finalists_in(h_block) + static_cast<size_t>(kBatchFinalistCap) * s;
        const float* acc = acc_in(h_block) + static_cast<size_t>(kBatchFinalistCap) * s;
        std::vector<std::pair<long long, float>> found(count);
        for (int i = 0; i < count; ++i) found[i] = {index[i], acc[i]};
        std::sort(found.begin(), found.end());
        Rt3DFinalists fin;
        for (const auto& f : found) {
          fin.index.push_back(f.first);
          fin.acc.push_back(f.second);
        }
        PickBest(S, wt, wr, fin, &out_scores[k], &out_poses[k]);
        cmx_match_stats one{};
        one.candidates_scored = one.coarse_candidates = S.num_candidates;
        one.num_scans = static_cast<int>(S.R);
        AddStats(one, &total);
      }
    }
  }
  // The single path, one match after the other (the reruns behind the planned ones).
  for (int k : singles) {
    const BatchMatch& M = matches[k];
    cmx_match_stats one{};
    Rt3DMatch(options, M.resolution, nullptr, 0, M.empty ? nullptr : &M.brick,
              &initial_pose_estimates[k], point_clouds_xyz[k], num_points[k], device,
              &out_scores[k], &out_poses[k], &one);
    AddStats(one, &total);
  }
  std::copy(out_scores.begin(), out_scores.end(), scores);
  std::copy(out_poses.begin(), out_poses.end(), pose_estimates);
  if (stats) *stats = total;
}

}  // namespace
}  // namespace cmx

extern "C" cmx_status cmx_rt3d_match_grid_batch(const cmx_rt_options* options,
                                                const cmx_grid3d* const* grids,
                                                int32_t num_matches,
                                                const cmx_pose3d* initial_pose_estimates,
                                                const float* const* point_clouds_xyz,
                                                const int32_t* num_points, float* scores,
                                                cmx_pose3d* pose_estimates,
                                                cmx_match_stats* stats) {
  return cmx::Guard([&] {
    cmx::MatchBatch(options, grids, num_matches, initial_pose_estimates, point_clouds_xyz,
                    num_points, scores, pose_estimates, stats);
  });
}

extern "C" cmx_status cmx_debug_rt3d_batch_plan(const cmx_rt_options* options,
                                                int32_t num_matches, const float* resolutions,
                                                const int32_t* num_points,
                                                const float* max_point_norms,
                                                cmx_debug_rt3d_match_plan* plans) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(options && resolutions && num_points && max_point_norms && plans, "null argument");
    CMX_REQUIRE(num_matches >= 1, "num_matches %d < 1", num_matches);
    std::vector<Rt3DMatchInput> inputs(num_matches);
    for (int k = 0; k < num_matches; ++k) {
      CMX_REQUIRE(resolutions[k] > 0.f, "match %d: resolution must be > 0", k);
      CMX_REQUIRE(num_points[k] >= 1 && num_points[k] <= (1 << 24), "match %d: bad point count", k);
      Rt3DMatchInput& I = inputs[k];
      I.finite = std::isfinite(max_point_norms[k]);
      I.window = Rt3DWindowOf(*options, resolutions[k],
                              I.finite ? std::max(max_point_norms[k], 3.f * resolutions[k])
                                       : 3.f * resolutions[k]);
      CMX_REQUIRE(I.window.unsupported == nullptr, "match %d: %s", k, I.window.unsupported);
      I.num_points = num_points[k];
    }
    const Rt3DBatchPlan plan = PlanRt3DBatch(inputs.data(), num_matches, Debug().rt3d_batch_route);
    for (int k = 0; k < num_matches; ++k) {
      cmx_debug_rt3d_match_plan& P = plans[k];
      P = cmx_debug_rt3d_match_plan{};
      P.L = inputs[k].window.L;
      P.A = inputs[k].window.A;
      P.T = inputs[k].window.T;
      P.R = inputs[k].window.R;
      P.route = plan.matches[k].route;
      P.set = plan.matches[k].set;
      P.first_block = plan.matches[k].first_block;
      P.blocks = plan.matches[k].blocks;
    }
  });
}
