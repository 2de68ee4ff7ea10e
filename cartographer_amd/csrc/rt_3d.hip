// RealTimeCorrelativeScanMatcher3D::Match on gfx950: the search space, the choice of paths,
// the uploads and the final weighting.  rt_3d_internal.h lists the units of the family.
//
// Reference: SM3/real_time_correlative_scan_matcher_3d.cc:34-53 (Match),
// :55-95 (GenerateExhaustiveSearchTransforms), :97-114 (ScoreCandidate).
//
// Parity notes
//   * Candidate = init.cast<float>() * Rigid3f(t, q) (renormalised product).
//     The (2A+1)^3 rotations and (2L+1)^3 translations are composed on the
//     host with the reference's f32/f64 operation order (sin/cos/atan2 from
//     libm); the device only performs IEEE +,-,*,/ on them.
//   * The reference transforms every point by every candidate and sums the N
//     probabilities sequentially in f32.  One thread per candidate does exactly
//     that, so the unweighted score is bit-identical; a wave holds 64
//     translations of one rotation, so the point load and the rotation are
//     wave-uniform and neighbouring lanes read neighbouring voxels.
//   * exp() weighting and the strict-'>' first-maximum rule are finished on the
//     host for the candidates within 1e-5 (relative) of the device maximum.
#include <algorithm>

#include "rt_3d_internal.h"

namespace cmx {
namespace {

// A tuning override (debug switches of the profiling tools): 0 = the default.
int Override(int value, int fallback) { return value > 0 ? value : fallback; }

// The 2 x 2 x 2 blocks (fewer members along the far faces) of a side^3 lattice whose index
// `half` is the origin: emit(k, centre in lattice steps * step, the smallest value_of(member)).
template <typename ValueOf, typename Emit>
void ForEachBlock2x2x2(int side, int half, float step, ValueOf value_of, Emit emit) {
  const int per_axis = (side + 1) / 2;
  long long k = 0;
  for (int bz = 0; bz < per_axis; ++bz)
    for (int by = 0; by < per_axis; ++by)
      for (int bx = 0; bx < per_axis; ++bx, ++k) {
        const int nx = std::min(2, side - 2 * bx), ny = std::min(2, side - 2 * by),
                  nz = std::min(2, side - 2 * bz);
        const h3::V3 centre{(2 * bx + 0.5f * (nx - 1) - half) * step,
                            (2 * by + 0.5f * (ny - 1) - half) * step,
                            (2 * bz + 0.5f * (nz - 1) - half) * step};
        float smallest = INFINITY;
        for (int c = 0; c < nz; ++c)
          for (int b = 0; b < ny; ++b)
            for (int a = 0; a < nx; ++a)
              smallest = std::min(
                  smallest, value_of(((2 * bz + c) * side + (2 * by + b)) * side + (2 * bx + a)));
        emit(k, centre, smallest);
      }
}

void FillCandidateTables(Rt3DSearchSpace* S) {
  const int A = S->A, L = S->L;
  const float step = S->step, resolution = S->resolution;
  const h3::Rigid& init = S->init;
  S->rot.resize(S->R); S->angle.resize(S->R); S->trans.resize(S->T);
  long long k = 0;
  for (int rz = -A; rz <= A; ++rz)
    for (int ry = -A; ry <= A; ++ry)
      for (int rx = -A; rx <= A; ++rx, ++k) {
        h3::Rigid tf;
        tf.q = h3::FromAngleAxisVector({rx * step, ry * step, rz * step});
        S->angle[k] = h3::GetAngle(tf);
        const h3::Q q = h3::Normalized(h3::Mul(init.q, tf.q));
        S->rot[k] = make_float4(q.x, q.y, q.z, q.w);
      }
  k = 0;
  for (int z = -L; z <= L; ++z)
    for (int y = -L; y <= L; ++y)
      for (int x = -L; x <= L; ++x, ++k) {
        const h3::V3 tc{x * resolution, y * resolution, z * resolution};
        const h3::V3 r = h3::Rotate(init.q, tc);
        S->trans[k] = make_float4(r.x + init.t.x, r.y + init.t.y, r.z + init.t.z, h3::Norm(tc));
      }
}

void FillBlockTables(Rt3DSearchSpace* S) {
  const h3::Rigid& init = S->init;
  S->Ab = (S->side_r + 1) / 2;
  S->Rb = 1ll * S->Ab * S->Ab * S->Ab;
  S->rot_b.resize(S->Rb); S->angle_b.resize(S->Rb);
  ForEachBlock2x2x2(
      S->side_r, S->A, S->step, [&](int r) { return S->angle[r]; },
      [&](long long k, const h3::V3& centre, float smallest) {
        const h3::Q q = h3::Normalized(h3::Mul(init.q, h3::FromAngleAxisVector(centre)));
        S->rot_b[k] = make_float4(q.x, q.y, q.z, q.w);
        S->angle_b[k] = smallest;
      });
  S->gpa = (S->side_t + 1) / 2;
  S->G = S->gpa * S->gpa * S->gpa;
  S->group.resize(S->G);
  ForEachBlock2x2x2(
      S->side_t, S->L, S->resolution, [&](int t) { return S->trans[t].w; },
      [&](long long g, const h3::V3& centre, float nearest) {
        const h3::V3 rc = h3::Rotate(init.q, centre);
        S->group[g] = make_float4(rc.x + init.t.x, rc.y + init.t.y, rc.z + init.t.z, nearest);
      });
}

}  // namespace

Rt3DSearchSpace SearchSpaceOf(const Rt3DWindow& W, float resolution,
                              const cmx_pose3d& initial_pose_estimate, int n) {
  Rt3DSearchSpace S;
  S.n = n;
  S.resolution = resolution;
  S.L = W.L; S.A = W.A; S.step = W.step;
  S.side_t = 2 * S.L + 1; S.side_r = 2 * S.A + 1;
  S.T = W.T; S.R = W.R; S.num_candidates = W.num_candidates;
  S.init = h3::FromPose(initial_pose_estimate);
  FillCandidateTables(&S);
  return S;
}

namespace {

Rt3DSearchSpace BuildSearchSpace(const cmx_rt_options& options, float resolution,
                                 const cmx_pose3d& initial_pose_estimate,
                                 const float* point_cloud_xyz, int n) {
  const Rt3DWindow W =
      Rt3DWindowOf(options, resolution, Rt3DScanRange(resolution, point_cloud_xyz, n));
  CMX_REQUIRE(W.unsupported == nullptr, "%s", W.unsupported);
  Rt3DSearchSpace S = SearchSpaceOf(W, resolution, initial_pose_estimate, n);
  FillBlockTables(&S);
  return S;
}

// The grid's box (no cells yet): the resident brick's own box (cells never written hold 0) or
// the voxels' bounding box.
PaddedBrick GridBox(const Rt3DGridSource& grid) {
  const Brick* resident = grid.resident;
  int lo[3], hi[3];
  if (resident != nullptr) {
    lo[0] = resident->lo_x; lo[1] = resident->lo_y; lo[2] = resident->lo_z;
    hi[0] = lo[0] + resident->nx - 1; hi[1] = lo[1] + resident->ny - 1;
    hi[2] = lo[2] + resident->nz - 1;
  } else {
    VoxelBoxOrOrigin(grid.voxels, grid.num_voxels, lo, hi);
  }
  const Brick box = BoxBrick(lo, hi);
  const size_t cells = static_cast<size_t>(box.nx + 2) * (box.ny + 2) * (box.nz + 2);
  CMX_REQUIRE(cells < (size_t(1) << 29), "dense grid of %d x %d x %d cells is too large", box.nx,
              box.ny, box.nz);
  return PaddedBrick{nullptr, box.lo_x, box.lo_y, box.lo_z, box.nx, box.ny, box.nz};
}

Rt3DBulkGeometry BulkGeometry(const PaddedBrick& brick, int L) {
  Rt3DBulkGeometry g;
  g.reach = static_cast<int>(std::ceil(L * 1.7320508075688772)) + 1;
  g.pad = 2 * g.reach + 2;
  g.bx = (brick.nx + 2ll * g.pad + 3) & ~3ll;
  g.by = brick.ny + 2ll * g.pad;
  g.bz = brick.nz + 2ll * g.pad;
  g.cells = static_cast<size_t>(g.bx * g.by * g.bz);
  g.tiles_x = DivUp(g.bx, 8); g.tiles_y = DivUp(g.by, 4);
  g.pitch_z = DivUp(g.bz, 4) * 4;
  g.tiled_cells = static_cast<size_t>(g.tiles_x) * g.tiles_y * g.pitch_z * 32;
  return g;
}

// The only reader of the debug switches on the match path.
// Limits of the bounds search: finite points (a NaN would read an unchecked cell), N small
// enough for the rounding bound of the f32 chain to mean something, index arithmetic exact in
// f32, weights that decrease with distance (a group is weighted by its nearest member).
Rt3DMode ModeOf(const Rt3DSearchSpace& S, const Rt3DBulkGeometry& geo,
                const cmx_rt_options& options, const float* point_cloud_xyz) {
  const DebugOptions& debug = Debug();
  Rt3DMode m{};
  m.use_bulk = debug.rt3d_legacy == 0 && S.n <= (1 << 21) && S.R <= 65535 &&
               geo.bx * geo.by * geo.bz < (1ll << 24) &&
               options.translation_delta_cost_weight >= 0. &&
               options.rotation_delta_cost_weight >= 0.;
  for (int i = 0; i < 3 * S.n && m.use_bulk; ++i) m.use_bulk = std::isfinite(point_cloud_xyz[i]);
  // Rotations of a group-pass workgroup: as many as fit 512 lanes, so that TWO workgroups
  // share a CU and one computes while the other stages its next chunk (C4, 216 groups: two
  // rotations = 448 lanes, group pass 5.51 -> 4.91 ms against four rotations in one 896-lane
  // workgroup per CU; debug switch rt3d_group_rotations overrides, experiments).
  m.rot_per_block = std::max(
      1, std::min({kTileMaxRotations, std::max(1, 512 / std::max(S.G, 1)),
                   Override(debug.rt3d_group_rotations, kTileMaxRotations)}));
  m.use_tiles = debug.rt3d_no_tiles == 0 && S.G <= 1024;
  m.crosscheck = m.use_tiles && debug.rt3d_crosscheck != 0;
  m.use_boxes = debug.rt3d_no_boxes == 0;
  // The cross-check compares complete sums and the expand-all mode has no second round.
  m.staged = m.use_tiles && !m.crosscheck && debug.rt3d_unstaged == 0 && debug.rt3d_expand_all == 0;
  // The rotation-block level needs a window of more than one rotation per axis, small enough
  // for the 1.03 of its bound, and the lists of the tiled passes.
  m.rotblocks = m.use_tiles && !m.crosscheck && debug.rt3d_no_rotblocks == 0 && S.A >= 1 &&
                (S.A + 1) * static_cast<double>(S.step) * 1.7320508 <= 0.2;
  m.verify = debug.rt3d_verify != 0;
  m.report = debug.rt3d_report != 0;
  // (with rt3d_verify: every group bound is then checked against every one of its members)
  m.expand_all = debug.rt3d_expand_all != 0;
  // (several rotations per work list, so that a tile serves some hundred lanes even when a
  // rotation keeps only a few dozen entries)
  m.list_rotations = m.use_tiles && !m.crosscheck
                         ? std::max(1, std::min(8, Override(debug.rt3d_cand_rotations, 8))) : 1;
  m.block_items = !m.use_tiles ? kCand3DThreads
                  : m.crosscheck ? 256 : Override(debug.rt3d_cand_threads, 512);
  m.group_tile_capacity = Override(debug.rt3d_group_tile_kb, 44) * 1024;
  m.cand_tile_capacity = Override(debug.rt3d_cand_tile_kb, 48) * 1024;
  // (the float path reproduces the gather kernel's sums)
  m.group_fixed_point = (debug.rt3d_group_float || m.crosscheck) ? 0 : 1;
  // rt3d_segments = a | b << 8: the first segment ends at a / 16, the second at b / 16 of a
  // window; default a quarter and a half.
  m.sixteenths0 = 4; m.sixteenths1 = 8;
  if (const int seg = debug.rt3d_segments; seg > 0) {
    m.sixteenths0 = std::max(1, std::min(15, seg & 0xff));
    m.sixteenths1 = std::max(m.sixteenths0, std::min(15, (seg >> 8) & 0xff));
  }
  // first rounds: the pairs of the blocks / the members of the groups next to the best bound
  const int permille = debug.rt3d_rotblock_permille;
  m.first_pair_factor =
      m.expand_all ? 0.f : permille > 0 ? std::min(permille, 1000) * 1e-3f : 0.97f;
  m.first_round_factor = m.expand_all ? 0.f : 0.97f;
  return m;
}

template <typename T>
T* Upload(Workspace& ws, int slot, const std::vector<T>& table) {
  T* d = ws.dev[slot].ReserveAs<T>(table.size());
  CMX_HIP(hipMemcpyAsync(d, table.data(), table.size() * sizeof(T), hipMemcpyHostToDevice,
                         ws.stream));
  return d;
}

// Cloud and candidate tables; returns when the copies are done.
void UploadTables(Workspace& ws, const Rt3DSearchSpace& S, const cmx_rt_options& options,
                  const float* point_cloud_xyz, Rt3DDevice* D) {
  D->d_xyz = ws.dev[kSlotCloud].ReserveAs<float>(3 * static_cast<size_t>(S.n));
  D->d_unweighted = ws.dev[kSlotUnweighted].ReserveAs<float>(S.num_candidates);
  D->d_weighted = ws.dev[kSlotWeighted].ReserveAs<float>(S.num_candidates);
  D->d_misc = static_cast<Rt3DExhaustiveMisc*>(ws.dev[kSlotMisc].Reserve(sizeof(Rt3DExhaustiveMisc)));
  D->pinned = static_cast<Rt3DPinnedReadBack*>(
      ws.pinned[kPinnedReadBack].Reserve(sizeof(Rt3DPinnedReadBack)));
  CMX_HIP(hipMemcpyAsync(D->d_xyz, point_cloud_xyz, 3 * sizeof(float) * S.n,
                         hipMemcpyHostToDevice, ws.stream));
  D->d_rot = Upload(ws, kSlotRotations, S.rot);
  D->d_trans = Upload(ws, kSlotTranslations, S.trans);
  D->d_angle = Upload(ws, kSlotAngles, S.angle);
  D->d_rot_b = Upload(ws, kSlotBlockRotations, S.rot_b);
  D->d_angle_b = Upload(ws, kSlotBlockAngles, S.angle_b);
  CMX_HIP(hipMemsetAsync(D->d_misc, 0, kExhaustiveHeadBytes, ws.stream));
  // pageable sources above: make sure the copies are done before they go away
  CMX_HIP(hipStreamSynchronize(ws.stream));

  Rt3DParams& P = D->P;
  P.grid = D->brick;
  P.resolution = S.resolution;
  P.inv_resolution = 1.f / S.resolution;
  P.num_translations = static_cast<int>(S.T);
  P.num_rotations = static_cast<int>(S.R);
  P.side_t = S.side_t; P.side_r = S.side_r;
  P.rotation = D->d_rot; P.translation = D->d_trans; P.rotation_angle = D->d_angle;
  P.wt = options.translation_delta_cost_weight;
  P.wr = options.rotation_delta_cost_weight;
}

}  // namespace

// Exact weighting and the strict '>' running maximum of :44-50.
void PickBest(const Rt3DSearchSpace& S, double wt, double wr, const Rt3DFinalists& fin,
              float* score, cmx_pose3d* pose_estimate) {
  CMX_REQUIRE(!fin.index.empty(), "internal error: no candidate collected");
  float best_score = -1.f;
  long long best = -1;
  for (size_t i = 0; i < fin.index.size(); ++i) {
    const long long c = fin.index[i];
    const long long t = c / S.R, r = c % S.R;
    float sc = fin.acc[i];
    const double penalty = static_cast<double>(S.trans[t].w) * wt +
                           static_cast<double>(S.angle[r]) * wr;
    sc *= std::exp(-(penalty * (penalty * 1.)));
    if (sc > best_score) { best_score = sc; best = c; }
  }
  const long long t = best / S.R, r = best % S.R;
  h3::Rigid candidate;
  candidate.t = {S.trans[t].x, S.trans[t].y, S.trans[t].z};
  candidate.q = {S.rot[r].w, S.rot[r].x, S.rot[r].y, S.rot[r].z};
  *pose_estimate = h3::ToPose(candidate);
  *score = best_score;
}

namespace {

// Bounds search: the search space is covered by bounds -- the group bounds plus the candidates
// scored one by one; `candidates_scored` stays the size of the search space (what the
// reference scores), `coarse_candidates` says how many bounds that took.
cmx_match_stats StatsOf(Workspace& ws, const Rt3DSearchSpace& S, const Rt3DFinalists& fin) {
  cmx_match_stats st{};
  st.candidates_scored = S.num_candidates;
  st.coarse_candidates = fin.bounds_evaluated ? fin.bounds_evaluated : S.num_candidates;
  st.num_scans = static_cast<int>(S.R);
  st.nodes_expanded = fin.num_finalists;
  st.device_ms = ElapsedMs(ws.ev_begin, ws.ev_end);
  st.dominant_kernel_ms = ElapsedMs(ws.ev_k0, ws.ev_k1);
  // the bounds above the candidates (rotation blocks, then the (rotation, group) pairs they
  // leave): how many, their lookups, and the time of ALL their passes
  st.expansion_nodes = fin.group_bounds;
  st.expansion_lookups = fin.group_bounds * S.n;
  st.expansion_ms = st.dominant_kernel_ms;
  if (fin.second_pairs_pass) st.expansion_ms += ElapsedMs(ws.ev_x0, ws.ev_x1);
  return st;
}

}  // namespace

// RealTimeCorrelativeScanMatcher3D::Match: the bounds search where its limits hold (ModeOf) and
// it narrows the search down, else the exhaustive search; the reference's weighting and
// first-maximum rule over what either leaves.
void Rt3DMatch(const cmx_rt_options* options, float grid_resolution, const cmx_voxel* voxels,
               int64_t num_voxels, const Brick* resident, const cmx_pose3d* initial_pose_estimate,
               const float* point_cloud_xyz, int32_t num_points, int32_t device, float* score,
               cmx_pose3d* pose_estimate, cmx_match_stats* stats) {
  CMX_REQUIRE(options && initial_pose_estimate && point_cloud_xyz, "null argument");
  CMX_REQUIRE(pose_estimate != nullptr && score != nullptr,
              "pose_estimate must not be null");                       // CHECK at :39
  CMX_REQUIRE(resident != nullptr || num_voxels == 0 || voxels != nullptr, "voxels is null");
  CMX_REQUIRE(num_points >= 1 && num_points <= (1 << 24), "bad point count");
  CMX_REQUIRE(grid_resolution > 0.f, "resolution must be > 0");
  const Rt3DSearchSpace S = BuildSearchSpace(*options, grid_resolution, *initial_pose_estimate,
                                             point_cloud_xyz, num_points);
  WorkspaceLease ws(device);
  const Rt3DGridSource grid{voxels, num_voxels, resident};
  const PaddedBrick box = GridBox(grid);
  const Rt3DBulkGeometry geo = BulkGeometry(box, S.L);
  const Rt3DMode mode = ModeOf(S, geo, *options, point_cloud_xyz);
  Rt3DDevice D;
  D.brick = box;
  BuildProbabilityBrick(*ws, grid, &D);
  UploadTables(*ws, S, *options, point_cloud_xyz, &D);

  Rt3DFinalists finalists;
  RecordEvent(ws->ev_begin, ws->stream);
  const bool done = mode.use_bulk && RunBoundsSearch(*ws, S, mode, geo, D, grid, &finalists);
  if (!done) RunExhaustiveSearch(*ws, S, D, &finalists);
  PickBest(S, D.P.wt, D.P.wr, finalists, score, pose_estimate);
  if (stats) *stats = StatsOf(*ws, S, finalists);
}

namespace {

cmx_status Rt3DMatchImpl(const cmx_rt_options* options, float grid_resolution,
                         const cmx_voxel* voxels, int64_t num_voxels, const Brick* resident,
                         const cmx_pose3d* initial_pose_estimate, const float* point_cloud_xyz,
                         int32_t num_points, int32_t device, float* score,
                         cmx_pose3d* pose_estimate, cmx_match_stats* stats) {
  return Guard([&] {
    Rt3DMatch(options, grid_resolution, voxels, num_voxels, resident, initial_pose_estimate,
              point_cloud_xyz, num_points, device, score, pose_estimate, stats);
  });
}
}  // namespace
}  // namespace cmx

extern "C" cmx_status cmx_rt3d_match(const cmx_rt_options* options, float grid_resolution,
                                     const cmx_voxel* voxels, int64_t num_voxels,
                                     const cmx_pose3d* initial_pose_estimate,
                                     const float* point_cloud_xyz, int32_t num_points,
                                     int32_t device, float* score, cmx_pose3d* pose_estimate,
                                     cmx_match_stats* stats) {
  return cmx::Rt3DMatchImpl(options, grid_resolution, voxels, num_voxels, nullptr,
                            initial_pose_estimate, point_cloud_xyz, num_points, device, score,
                            pose_estimate, stats);
}

// The same search on the ACTIVE submap's HybridGrid where cmx_grid3d keeps it in HBM
// (LocalTrajectoryBuilder3D's per-scan Match -> InsertRangeData pair, mapping/internal/3d/
// local_trajectory_builder_3d.cc:96-108): only the scan crosses PCIe.
extern "C" cmx_status cmx_rt3d_match_grid(const cmx_rt_options* options, const cmx_grid3d* grid,
                                          const cmx_pose3d* initial_pose_estimate,
                                          const float* point_cloud_xyz, int32_t num_points,
                                          float* score, cmx_pose3d* pose_estimate,
                                          cmx_match_stats* stats) {
  using namespace cmx;
  if (grid == nullptr) {
    return Guard([] { CMX_REQUIRE(false, "null argument"); });
  }
  Brick brick{};
  float resolution = 0.f;
  int device = 0;
  if (!Grid3DBrick(grid, &brick, &resolution, &device)) {
    // nothing inserted yet: an empty voxel list (every candidate scores kMinProbability)
    return Rt3DMatchImpl(options, resolution, nullptr, 0, nullptr, initial_pose_estimate,
                         point_cloud_xyz, num_points, device, score, pose_estimate, stats);
  }
  return Rt3DMatchImpl(options, resolution, nullptr, 0, &brick, initial_pose_estimate,
                       point_cloud_xyz, num_points, device, score, pose_estimate, stats);
}
