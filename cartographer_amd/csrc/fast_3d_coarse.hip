// The front end of a chain of fast-3D searches: the chain's layout and its one upload, scan
// discretisation and lowest-resolution scoring (reference map: fast_3d.hip).
#include <algorithm>
#include <cstring>

#include "fast_3d_internal.h"

namespace cmx {
namespace {

// ---------------------------------------------------------------------------
// Scan discretisation (DiscretizeScan, :200-244: transform + GetCellIndex)
// ---------------------------------------------------------------------------
// Point i of a cloud under one scan's pose: `t4` = the translation of the scan's problem, .w its
// grid resolution.
__device__ __forceinline__ int4 DiscretizePoint3D(const float* __restrict__ xyz, int i,
                                                  const float4& q4, const float4& t4) {
  const Quat q{q4.w, q4.x, q4.y, q4.z};
  const F3 p{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  const F3 r = Rotate(q, p);
  const F3 t{r.x + t4.x, r.y + t4.y, r.z + t4.z};
  const int3 c = CellIndex3(t, t4.w);
  return make_int4(c.x, c.y, c.z, 0);
}

// grid (ceil(n / 256), scans of the whole batch): every scan rotates the one cloud of the batch's
// node.
__global__ void __launch_bounds__(256)
Discretize3DKernel(const float* __restrict__ xyz, int n, const float4* __restrict__ pose_q,
                   const float4* __restrict__ pose_t, int4* __restrict__ cells) {
  const int s = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cells[static_cast<size_t>(s) * n + i] = DiscretizePoint3D(xyz, i, pose_q[s], pose_t[s]);
}

// The same for a batch of several nodes, in one launch: grid (scans of the whole batch, tiles of
// 256 points of the largest cloud, at most 65535 -- a block strides over what is left).  The scan
// is blockIdx.x, whose range does not bound the batch; its descriptor is uniform per block (scalar
// loads).
__global__ void __launch_bounds__(256)
Discretize3DNodesKernel(const Scan3D* __restrict__ scans, const float4* __restrict__ pose_q,
                        const float4* __restrict__ pose_t) {
  const unsigned s = blockIdx.x;
  const Scan3D scan = scans[s];
  const float4 q4 = pose_q[s];
  const float4 t4 = pose_t[s];
  for (long long i = static_cast<long long>(blockIdx.y) * blockDim.x + threadIdx.x; i < scan.n;
       i += static_cast<long long>(gridDim.y) * blockDim.x)
    scan.cells[i] = DiscretizePoint3D(scan.xyz, static_cast<int>(i), q4, t4);
}

// ---------------------------------------------------------------------------
// Scoring
// ---------------------------------------------------------------------------
// Integer sum of one candidate, one wave (ScoreCandidates, :332-355).
__device__ __forceinline__ int ScoreCandidate3D(const Fast3DProblem& P, int depth, int scan,
                                                int ox, int oy, int oz, int lane) {
  const int e = max(0, depth - P.full_resolution_depth + 1);
  const Brick& L = P.level[depth];
  const int4* __restrict__ cells = P.cells + static_cast<size_t>(scan) * P.n;
  const int fx = ox >> e, fy = oy >> e, fz = oz >> e;
  int sum = 0;
#pragma unroll 4
  for (int i = lane; i < P.n; i += kWave) {
    const int3 d = DepthIndex(cells[i], e, -P.wxy, -P.wxy, -P.wz);
    sum += BrickValueU8(L, d.x + fx, d.y + fy, d.z + fz);
  }
  return WaveSum(sum);
}

// grid (blocks, problems)
__global__ void __launch_bounds__(256)
ScoreCoarse3DKernel(const Fast3DProblem* __restrict__ problems) {
  const Fast3DProblem& P = problems[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int per_scan = P.ncx * P.ncy * P.ncz;
  const int total = per_scan * P.num_scans;
  const int step = 1 << (P.depth - 1);
  for (int c = blockIdx.x * 4 + wave; c < total; c += gridDim.x * 4) {
    const int s = c / per_scan;
    int r = c - s * per_scan;
    // z outer, y, x inner (:313-326)
    const int iz = r / (P.ncy * P.ncx);
    r -= iz * P.ncy * P.ncx;
    const int iy = r / P.ncx, ix = r - iy * P.ncx;
    const int sum = ScoreCandidate3D(P, P.depth - 1, s, -P.wxy + ix * step, -P.wxy + iy * step,
                                     -P.wz + iz * step, lane);
    if (lane == 0) P.coarse_score[c] = ToProbability(sum, P.n);
  }
}

// Few lowest-resolution candidates (deep stacks: one per yaw): a whole block per
// candidate, so that its sum is not a 43-iteration chain of one wavefront.
__global__ void __launch_bounds__(256)
ScoreCoarse3DBlockKernel(const Fast3DProblem* __restrict__ problems) {
  const Fast3DProblem& P = problems[blockIdx.y];
  __shared__ int partial[4];
  const int per_scan = P.ncx * P.ncy * P.ncz;
  const int total = per_scan * P.num_scans;
  const int step = 1 << (P.depth - 1);
  const int depth = P.depth - 1;
  const int e = max(0, depth - P.full_resolution_depth + 1);
  const Brick L = P.level[depth];
  for (int c = blockIdx.x; c < total; c += gridDim.x) {
    const int s = c / per_scan;
    int r = c - s * per_scan;
    const int iz = r / (P.ncy * P.ncx);
    r -= iz * P.ncy * P.ncx;
    const int iy = r / P.ncx, ix = r - iy * P.ncx;
    const int fx = (-P.wxy + ix * step) >> e, fy = (-P.wxy + iy * step) >> e,
              fz = (-P.wz + iz * step) >> e;
    const int4* __restrict__ cells = P.cells + static_cast<size_t>(s) * P.n;
    int sum = 0;
#pragma unroll 4
    for (int i = threadIdx.x; i < P.n; i += 256) {
      const int3 d = DepthIndex(cells[i], e, -P.wxy, -P.wxy, -P.wz);
      sum += BrickValueU8(L, d.x + fx, d.y + fy, d.z + fz);
    }
    sum = WaveSum(sum);
    if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
      P.coarse_score[c] = ToProbability(partial[0] + partial[1] + partial[2] + partial[3], P.n);
    __syncthreads();
  }
}

// The high-resolution cloud only ever feeds integer sums (ScoreCandidates), which do
// not depend on the order of the points.  It goes up sorted along a Morton curve: the
// 64 points a wavefront gathers together then fall into neighbouring voxels, i.e. into
// a handful of cache lines instead of 64 (the search is bound by that line traffic).
void SortAlongMortonCurve(const float* hi, int n, float inv_cell, float* out) {
  float lo3[3] = {hi[0], hi[1], hi[2]};
  for (int i = 1; i < n; ++i)
    for (int k = 0; k < 3; ++k) lo3[k] = std::min(lo3[k], hi[3 * i + k]);
  auto spread = [](uint32_t v) {   // 10 bits -> every third bit
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
  };
  std::vector<uint64_t> order(n);
  for (int i = 0; i < n; ++i) {
    uint32_t key = 0;
    for (int k = 0; k < 3; ++k) {
      const float cell = (hi[3 * i + k] - lo3[k]) * inv_cell;
      const uint32_t c = cell >= 1023.f ? 1023u : (cell > 0.f ? static_cast<uint32_t>(cell) : 0u);
      key |= spread(c) << k;
    }
    order[i] = (static_cast<uint64_t>(key) << 32) | static_cast<uint32_t>(i);
  }
  std::sort(order.begin(), order.end());
  for (int i = 0; i < n; ++i) {
    const uint32_t src = static_cast<uint32_t>(order[i]);
    out[3 * i] = hi[3 * src]; out[3 * i + 1] = hi[3 * src + 1]; out[3 * i + 2] = hi[3 * src + 2];
  }
}

}  // namespace

bool LayOutChain3D(const Search3D* searches, Prepared3D* prep, int num, Chain3D* chain) {
  Chain3D& c = *chain;
  c.num = num;
  c.cloud_of.resize(num);
  for (int p = 0; p < num; ++p) {
    const cmx_node_data3d* data = searches[p].data->data;
    // (a chain has at most 64 searches, or fast3d_batch of them: a linear lookup will do)
    size_t cloud = 0;
    while (cloud < c.clouds.size() && c.clouds[cloud].data != data) ++cloud;
    if (cloud == c.clouds.size())
      c.clouds.push_back(Cloud3D{data, 1.f / (2.f * searches[p].m->resolution), 0, 0});
    c.cloud_of[p] = static_cast<int>(cloud);
    Prepared3D& pr = prep[p];
    pr.scan_base = c.scans_total;
    pr.coarse_base = c.coarse_total;
    pr.cells_base = c.cells_total;
    c.scans_total += pr.S;
    c.coarse_total += static_cast<size_t>(pr.total);
    c.cells_total += static_cast<size_t>(pr.S) * data->num_high_resolution_points;
    c.max_total = std::max(c.max_total, pr.total);
    c.max_depth = std::max(c.max_depth, searches[p].m->options.branch_and_bound_depth);
    c.max_n = std::max(c.max_n, data->num_high_resolution_points);
    c.same_n &= data->num_high_resolution_points == c.clouds[0].data->num_high_resolution_points;
  }
  if (c.scans_total == 0) return false;
  CMX_REQUIRE(c.coarse_total < (size_t(1) << 31) && c.cells_total < (size_t(1) << 31),
              "batch too large");
  c.one_node = c.clouds.size() == 1;

  // The upload block (see Chain3D).
  const auto align256 = [](size_t bytes) { return (bytes + 255) & ~size_t(255); };
  size_t up_low = 0;
  for (Cloud3D& cloud : c.clouds) {
    cloud.hi_floats = up_low / sizeof(float);
    up_low += align256(3 * sizeof(float) * static_cast<size_t>(cloud.data->num_high_resolution_points));
  }
  c.up_q = up_low;
  for (Cloud3D& cloud : c.clouds) {
    cloud.low_floats = c.up_q / sizeof(float);
    c.up_q += align256(3 * sizeof(float) * static_cast<size_t>(cloud.data->num_low_resolution_points));
  }
  // (several nodes: one Scan3D per scan behind the poses, for Discretize3DNodesKernel)
  c.up_scans = c.up_q + align256(3 * sizeof(float4) * c.scans_total);
  c.up_misc = c.up_scans + (c.one_node ? 0 : align256(sizeof(Scan3D) * c.scans_total));
  c.off_problems = sizeof(Counters3);
  c.off_state = c.off_problems + sizeof(Fast3DProblem) * num;
  c.off_best = c.off_state + sizeof(unsigned) * 2 * num;
  c.misc_bytes = c.off_best + sizeof(Best3) * num;
  static_assert(sizeof(Counters3) % 8 == 0 && sizeof(Fast3DProblem) % 8 == 0, "alignment");
  static_assert(sizeof(Best3) % sizeof(unsigned) == 0, "Best3 is copied by dwords");
  return true;
}

void ReserveChainBuffers3D(Workspace& ws, Chain3D* chain) {
  Chain3D& c = *chain;
  c.d_up = static_cast<char*>(ws.dev[0].Reserve(c.up_misc + c.misc_bytes));
  c.h_up = static_cast<char*>(ws.pinned[0].Reserve(c.up_misc + c.misc_bytes));
  c.d_cells = ws.dev[3].ReserveAs<int4>(c.cells_total);
  c.d_coarse = ws.dev[4].ReserveAs<float>(c.coarse_total);
}

void StageAndUploadChain3D(Workspace& ws, const Search3D* searches, const Prepared3D* prep,
                           const Chain3D& c) {
  float4* h_q = reinterpret_cast<float4*>(c.h_up + c.up_q);
  Scan3D* h_scans = reinterpret_cast<Scan3D*>(c.h_up + c.up_scans);
  Fast3DProblem* h_problems = c.h_problems();
  unsigned* h_state = c.h_state();
  std::memset(c.h_misc(), 0, c.misc_bytes);
  for (int p = 0; p < c.num; ++p) {
    const Search3D& q = searches[p];
    const Fast3DMatcher& m = *q.m;
    const Prepared3D& pr = prep[p];
    const Cloud3D& cloud = c.clouds[c.cloud_of[p]];
    const int n = cloud.data->num_high_resolution_points;
    for (int s = 0; s < pr.S; ++s) {
      const size_t k = pr.scan_base + s;
      if (!c.one_node)
        h_scans[k] = Scan3D{c.d_xyz() + cloud.hi_floats,
                            c.d_cells + pr.cells_base + static_cast<size_t>(s) * n, n, 0};
      h_q[k] = make_float4(pr.pose_q[s].x, pr.pose_q[s].y, pr.pose_q[s].z, pr.pose_q[s].w);
      h_q[c.scans_total + k] =
          make_float4(pr.scan_q[s].x, pr.scan_q[s].y, pr.scan_q[s].z, pr.scan_q[s].w);
      h_q[2 * c.scans_total + k] = make_float4(pr.pose_t.x, pr.pose_t.y, pr.pose_t.z, m.resolution);
    }
    const float floor_score = std::max(q.min_score, 0.f);
    std::memcpy(&h_state[2 * p], &floor_score, sizeof(float));
    const int depth = m.options.branch_and_bound_depth;
    Fast3DProblem P{};
    for (int d = 0; d < depth; ++d) P.level[d] = m.levels[d]->desc;
    for (size_t d = 0; d < m.oct_desc.size(); ++d) P.oct[d] = m.oct_desc[d];
    P.depth = depth;
    P.full_resolution_depth = m.options.full_resolution_depth;
    P.low = m.low.desc;
    P.low_resolution = m.low_resolution;
    P.resolution = m.resolution;
    P.wxy = q.wxy; P.wz = q.wz;
    P.num_scans = pr.S; P.n = n; P.n_low = cloud.data->num_low_resolution_points;
    P.cells = c.d_cells + pr.cells_base;
    P.low_xyz = c.d_xyz() + cloud.low_floats;
    P.scan_q = c.d_scan_q() + pr.scan_base;
    P.pose_tx = pr.pose_t.x; P.pose_ty = pr.pose_t.y; P.pose_tz = pr.pose_t.z;
    P.min_score = q.min_score;
    P.min_low_resolution_score = m.options.min_low_resolution_score;
    P.ncx = static_cast<int>(pr.ncx); P.ncy = static_cast<int>(pr.ncx);
    P.ncz = static_cast<int>(pr.ncz);
    P.coarse_score = c.d_coarse + pr.coarse_base;
    P.best_bits = c.d_state() + 2 * p;
    P.seed_count = reinterpret_cast<int*>(c.d_state() + 2 * p + 1);
    P.seeds = c.d_seeds + static_cast<size_t>(kSeeds3) * p;
    P.index = p;
    h_problems[p] = P;
  }
  // The clouds into the pinned mirror (the high-resolution ones sorted, the low-resolution ones
  // as they are), then one upload: a copy kernel while it is small (cmx_common.h: SmallCopyAsync).
  float* h_xyz = reinterpret_cast<float*>(c.h_up);
  // (a sort is ~30 ns per point, serial host time that exceeds the device time of a batch of many
  // nodes: several clouds are sorted on the host pool)
  ParallelFor(static_cast<int>(c.clouds.size()), 3, [&](int k) {
    const Cloud3D& cloud = c.clouds[k];
    SortAlongMortonCurve(cloud.data->high_resolution_point_cloud,
                         cloud.data->num_high_resolution_points, cloud.inv_cell,
                         h_xyz + cloud.hi_floats);
    std::memcpy(h_xyz + cloud.low_floats, cloud.data->low_resolution_point_cloud,
                3 * sizeof(float) * cloud.data->num_low_resolution_points);
  });
  SmallCopyAsync(c.d_up, c.h_up, c.up_misc + c.off_best, true, ws.stream);
}

void DiscretizeAndScoreCoarse3D(Workspace& ws, const Chain3D& c, StageTrace* trace) {
  trace->Mark("begin");
  RecordEvent(ws.ev_begin, ws.stream);
  if (c.one_node)
    Discretize3DKernel<<<dim3(DivUp(c.max_n, 256), static_cast<unsigned>(c.scans_total)), 256, 0,
                         ws.stream>>>(c.d_xyz(), c.max_n, c.d_pose_q(), c.d_pose_t(), c.d_cells);
  else
    Discretize3DNodesKernel<<<dim3(static_cast<unsigned>(c.scans_total),
                                   std::min<unsigned>(DivUp(c.max_n, 256), 65535u)),
                              256, 0, ws.stream>>>(c.d_scans(), c.d_pose_q(), c.d_pose_t());
  DebugSync3D(ws, "discretize");
  trace->Mark("discretize");
  RecordEvent(ws.ev_k0, ws.stream);
  if (c.max_total <= 4096)
    ScoreCoarse3DBlockKernel<<<dim3(static_cast<unsigned>(c.max_total), c.num), 256, 0,
                               ws.stream>>>(c.d_problems());
  else
    ScoreCoarse3DKernel<<<dim3(std::min<long long>(8192, DivUp(c.max_total, 4)), c.num), 256, 0,
                          ws.stream>>>(c.d_problems());
  RecordEvent(ws.ev_k1, ws.stream);
  DebugSync3D(ws, "coarse");
  trace->Mark("coarse");
}

}  // namespace cmx
