// Host side of the fast 3D searches: the yaw pre-filter and candidate lattice of every search,
// batches of searches in chains of launches, tie resolution, result poses, and the C ABI
// (reference map: fast_3d.hip).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <functional>
#include <unordered_map>

#include "fast_3d_internal.h"

namespace cmx {
namespace {

float Dot(const std::vector<float>& a, const std::vector<float>& b) {
  float s = 0.f;
  for (size_t i = 0; i != a.size(); ++i) s += a[i] * b[i];
  return s;
}

// RotationalScanMatcher::Match with its histogram rotation and normalised correlation
// (SM3/rotational_scan_matcher.cc:121-189), host side, as one object per yaw sweep of a search
// (tens of angles per pair, hundreds of pairs per node): no allocation per angle, no integer
// division per bucket, the submap's norm computed once.  Reductions are sequential f32 (Eigen's
// packet reduction order is unpinned).
struct YawSweep {
  const std::vector<float>& submap;
  const std::vector<float>& scan;
  float submap_norm;
  std::vector<float> rotated;
  YawSweep(const std::vector<float>& submap_histogram, const std::vector<float>& scan_histogram)
      : submap(submap_histogram), scan(scan_histogram),
        submap_norm(std::sqrt(Dot(submap_histogram, submap_histogram))),
        rotated(scan_histogram.size()) {}
  float Score(float angle) {
    const int size = static_cast<int>(scan.size());
    if (size != 0) {
      const float rotate_by_buckets =
          static_cast<float>(static_cast<double>(-angle * static_cast<float>(size)) / M_PI);
      int full_buckets = static_cast<int>(std::lround(rotate_by_buckets - 0.5f));
      const float fraction = rotate_by_buckets - full_buckets;
      while (full_buckets < 0) full_buckets += size;
      int i0 = full_buckets % size;
      for (int i = 0; i != size; ++i) {
        const int i1 = i0 + 1 == size ? 0 : i0 + 1;
        rotated[i] = fraction * scan[i1] + (1.f - fraction) * scan[i0];
        i0 = i1;
      }
    }
    const float scan_norm = std::sqrt(Dot(rotated, rotated));
    const float normalization = scan_norm * submap_norm;
    if (normalization < 1e-3f) return 1.f;
    return Dot(submap, rotated) / normalization;
  }
};

// Norm of the farthest high-resolution point (does not throw: runs on the host pool for batches).
float FarthestPoint3D(const cmx_node_data3d& data) {
  const float* hi = data.high_resolution_point_cloud;
  float max_point = 0.f;
  for (int i = 0; i < data.num_high_resolution_points; ++i)
    max_point = std::max(h3::Norm({hi[3 * i], hi[3 * i + 1], hi[3 * i + 2]}), max_point);
  return max_point;
}

// Everything of a node but `max_point` (FarthestPoint3D).
NodeHost3D NodeOf3D(const cmx_node_data3d& data) {
  CMX_REQUIRE(data.high_resolution_point_cloud && data.num_high_resolution_points >= 1,
              "empty high-resolution point cloud");
  CMX_REQUIRE(data.low_resolution_point_cloud && data.num_low_resolution_points >= 1,
              "empty low-resolution point cloud");
  CMX_REQUIRE(data.histogram_size >= 0 &&
                  (data.histogram_size == 0 || data.rotational_scan_matcher_histogram != nullptr),
              "null histogram");
  NodeHost3D node;
  node.data = &data;
  node.max_point = 0.f;
  if (data.histogram_size > 0)
    node.scan_hist.assign(data.rotational_scan_matcher_histogram,
                          data.rotational_scan_matcher_histogram + data.histogram_size);
  const double* g = data.gravity_alignment;   // w, x, y, z
  const double n2 = (g[1] * g[1] + g[3] * g[3]) + (g[2] * g[2] + g[0] * g[0]);
  node.g_inv = h3::Q{static_cast<float>(g[0] / n2), static_cast<float>(-g[1] / n2),
                     static_cast<float>(-g[2] / n2), static_cast<float>(-g[3] / n2)};
  return node;
}

void AddStats3D(const cmx_match_stats& st, cmx_match_stats* total) {
  total->candidates_scored += st.candidates_scored; total->coarse_candidates += st.coarse_candidates;
  total->nodes_expanded += st.nodes_expanded; total->num_scans += st.num_scans;
  total->device_ms += st.device_ms; total->dominant_kernel_ms += st.dominant_kernel_ms;
  total->expansion_ms += st.expansion_ms; total->expansion_nodes += st.expansion_nodes;
  total->expansion_lookups += st.expansion_lookups;
  total->expansion_launches += st.expansion_launches;
}

// Match (:127-146) / MatchFullSubmap (:148-170): MatchWithSearchParameters' arguments for `node`
// (max_point set) against `m`.  A full-submap search reads only the rotations of the poses.
Search3D MakeSearch3D(const Fast3DMatcher& m, const NodeHost3D* node, bool full_submap,
                      const cmx_pose3d& node_pose, const cmx_pose3d& submap_pose,
                      float min_score) {
  Search3D q;
  q.m = &m;
  q.min_score = min_score;
  q.data = node;
  q.node = h3::FromPose(node_pose);
  q.submap = h3::FromPose(submap_pose);
  if (full_submap) {
    // (MatchFullSubmap's window reaches as far as the node's farthest point)
    const int window = (m.width_in_voxels + 1) / 2 +
                       static_cast<int>(std::lround(node->max_point / m.resolution + 0.5f));
    q.wxy = q.wz = window;
    q.angular_search_window = M_PI;
    q.node.t = q.submap.t = h3::V3{0, 0, 0};
  } else {
    q.wxy = static_cast<int>(std::lround(m.options.linear_xy_search_window / m.resolution));
    q.wz = static_cast<int>(std::lround(m.options.linear_z_search_window / m.resolution));
    q.angular_search_window = m.options.angular_search_window;
  }
  return q;
}

// GenerateDiscreteScans (:246-295), host part of one search: the yaws that pass the histogram
// pre-filter, their poses, and the lattice of lowest-resolution candidates (:297-330).
void PrepareSearch3D(const Search3D& q, Prepared3D* prepared) {
  const Fast3DMatcher& m = *q.m;
  Prepared3D& pr = *prepared;
  const NodeHost3D& node = *q.data;
  const float max_scan_range = std::max(node.max_point, 3.f * m.resolution);
  const float kSafetyMargin = 1.f - 1e-2f;
  const float step =
      kSafetyMargin * std::acos(1.f - (m.resolution * (m.resolution * 1.f)) /
                                          (2.f * (max_scan_range * (max_scan_range * 1.f))));
  const int angular_window_size = static_cast<int>(std::lround(q.angular_search_window / step));
  CMX_REQUIRE(angular_window_size >= 0 && angular_window_size < (1 << 20), "bad angular window");
  const h3::Rigid node_to_submap = h3::Mul(h3::InverseRigid(q.submap), q.node);
  const float initial_angle = h3::GetYaw(h3::Mul(node_to_submap.q, node.g_inv));
  YawSweep sweep(m.histogram, node.scan_hist);
  for (int rz = -angular_window_size; rz <= angular_window_size; ++rz) {
    const float angle = rz * step;
    const float sc = sweep.Score(initial_angle + angle);
    if (sc < m.options.min_rotational_score) continue;
    pr.pose_q.push_back(h3::Mul(h3::Mul(h3::Inverse(q.submap.q),
                                        h3::FromAngleAxisVector({0.f, 0.f, angle})),
                                q.node.q));
    pr.rotational_score.push_back(sc);
  }
  pr.S = static_cast<int>(pr.pose_q.size());
  pr.pose_t = node_to_submap.t;
  // Lowest-resolution candidates (:297-330).
  const int depth = m.options.branch_and_bound_depth;
  const int step_cells = 1 << (depth - 1);
  pr.ncx = (2ll * q.wxy + step_cells) / step_cells;
  pr.ncz = (2ll * q.wz + step_cells) / step_cells;
  pr.per_scan = pr.ncx * pr.ncx * pr.ncz;
  pr.total = pr.per_scan * pr.S;
  CMX_REQUIRE(pr.total < (1ll << 30), "search too large: %lld lowest-resolution candidates",
              pr.total);
  // GetPoseFromCandidate (:369-375): Translation(res * offset) * pose renormalises
  // the rotation; Identity * q is exact, the normalisation is not.
  pr.scan_q.resize(pr.S);
  for (int s = 0; s < pr.S; ++s)
    pr.scan_q[s] = h3::Normalized(h3::Mul(h3::Q{1.f, 0.f, 0.f, 0.f}, pr.pose_q[s]));
}

// What the tie resolution of a chain fetches from the device, lazily and once: the recorded
// leaves, the lowest-resolution scores.
struct TieDownloads3D {
  bool have_leaves = false;
  std::vector<Node3D> leaves;
  std::vector<float> coarse;
};

// The recorded leaves of problem p whose score has the bits `score_bits`.
std::vector<Node3D> TiedLeaves3D(const Searched3D& searched, int p, unsigned score_bits,
                                 TieDownloads3D* downloads) {
  if (!downloads->have_leaves) {
    downloads->have_leaves = true;
    // one strided copy: the first max-count slots of every sub-list
    const auto count_of = [&](int sub) {
      return std::min(searched.leaf_counts[sub * kCountStride3], searched.leaf_sub_capacity);
    };
    int max_count = 0;
    for (int sub = 0; sub < kSubLists3; ++sub) max_count = std::max(max_count, count_of(sub));
    if (max_count > 0) {
      std::vector<Node3D> rows(static_cast<size_t>(max_count) * kSubLists3);
      CMX_HIP(hipMemcpy2D(rows.data(), max_count * sizeof(Node3D), searched.d_leaves,
                          searched.leaf_sub_capacity * sizeof(Node3D), max_count * sizeof(Node3D),
                          kSubLists3, hipMemcpyDeviceToHost));
      for (int sub = 0; sub < kSubLists3; ++sub)
        downloads->leaves.insert(downloads->leaves.end(),
                                 rows.begin() + static_cast<size_t>(sub) * max_count,
                                 rows.begin() + static_cast<size_t>(sub) * max_count + count_of(sub));
    }
  }
  std::vector<Node3D> tied;
  for (const Node3D& nd : downloads->leaves) {
    unsigned bits;
    std::memcpy(&bits, &nd.score, sizeof(float));
    if (nd.problem == p && bits == score_bits) tied.push_back(nd);
  }
  return tied;
}

// Exact tie resolution of problem p, whose selected `best` has ties (see fast_2d_match.hip
// ResolveTies): repeat the reference's std::sort of the lowest-resolution candidates (:352-353)
// and take the tied leaf its depth-first search meets first.  The dive and the search record the
// same leaf twice, so first check that distinct leaves tie.
void ResolveTies3D(const Chain3D& chain, const Searched3D& searched, const Prepared3D& pr, int p,
                   TieDownloads3D* downloads, Best3* best) {
  unsigned best_bits;
  std::memcpy(&best_bits, &best->score, sizeof(float));
  const std::vector<Node3D> tied = TiedLeaves3D(searched, p, best_bits, downloads);
  bool distinct = false;
  for (const Node3D& nd : tied)
    distinct |= !(nd.scan == tied[0].scan && nd.ox == tied[0].ox && nd.oy == tied[0].oy &&
                  nd.oz == tied[0].oz);
  if (!distinct) return;
  if (downloads->coarse.empty()) {
    downloads->coarse.resize(chain.coarse_total);
    CMX_HIP(hipMemcpy(downloads->coarse.data(), chain.d_coarse, chain.coarse_total * sizeof(float),
                      hipMemcpyDeviceToHost));
  }
  const float* scores = downloads->coarse.data() + pr.coarse_base;
  struct ScoreIndex {
    float score; int index;
    bool operator>(const ScoreIndex& o) const { return score > o.score; }
  };
  const long long total = pr.total;
  std::vector<ScoreIndex> sorted(total);
  for (long long c = 0; c < total; ++c) sorted[c] = {scores[c], static_cast<int>(c)};
  std::sort(sorted.begin(), sorted.end(), std::greater<ScoreIndex>());
  std::vector<int> position(total);
  for (long long i = 0; i < total; ++i) position[sorted[i].index] = static_cast<int>(i);
  bool have = false;
  int best_pos = 0;
  unsigned long long best_path = 0;
  for (const Node3D& nd : tied) {
    const int pos = position[nd.coarse_index];
    if (!have || pos < best_pos || (pos == best_pos && nd.path < best_path)) {
      have = true;
      best_pos = pos;
      best_path = nd.path;
      best->scan = nd.scan; best->ox = nd.ox; best->oy = nd.oy; best->oz = nd.oz;
      best->low_resolution_score = nd.low_resolution_score;
    }
  }
}

// The Result of a search (:389-402) from its best leaf, if it has one above min_score.
void WriteResult3D(const Search3D& q, const Prepared3D& pr, const Best3& best, int32_t* found,
                   cmx_result3d* result) {
  if (!(best.found && best.score > q.min_score)) return;
  const float resolution = q.m->resolution;
  *found = 1;
  result->score = best.score;
  h3::Rigid pose;
  // Translation(res * offset) * scan.pose
  pose.t = {(pr.pose_t.x + 0.f) + resolution * static_cast<float>(best.ox),
            (pr.pose_t.y + 0.f) + resolution * static_cast<float>(best.oy),
            (pr.pose_t.z + 0.f) + resolution * static_cast<float>(best.oz)};
  pose.q = pr.scan_q[best.scan];
  result->pose_estimate = h3::ToPose(pose);
  result->rotational_score = pr.rotational_score[best.scan];
  result->low_resolution_score = best.low_resolution_score;
}

// One chain of launches for `num` prepared searches.  True: the shared lists of a chain of
// several searches dropped nodes -- nothing was written but the statistics, every search has to
// run alone (SearchEachAlone3D; a single search owns its overflow retry, RunBranchAndBound3D).
bool RunChain3D(const Search3D* searches, Prepared3D* prep, int num, int32_t* found,
                cmx_result3d* results, cmx_match_stats* stats) {
  HostLaps3D laps;
  Chain3D chain;
  if (!LayOutChain3D(searches, prep, num, &chain)) {
    *stats = cmx_match_stats{};
    return false;
  }
  laps.Lap("prepare");
  WorkspaceLease ws(searches[0].m->device);   // (held until the ties have read the device buffers)
  ReserveChainBuffers3D(*ws, &chain);
  ReserveSearchScratch3D(*ws, &chain);
  StageAndUploadChain3D(*ws, searches, prep, chain);
  DebugSync3D(*ws, "uploads");
  laps.Lap("buffers+uploads");
  StageTrace trace(ws->stream);
  DiscretizeAndScoreCoarse3D(*ws, chain, &trace);
  Searched3D searched;
  RunBranchAndBound3D(*ws, chain, searches[0].min_score, &trace, &laps, &searched);
  *stats = searched.stats;
  if (num > 1 && searched.overflow) return true;
  TieDownloads3D downloads;
  for (int p = 0; p < num; ++p) {
    Best3 best = searched.best[p];
    if (best.found && best.ties > 1) ResolveTies3D(chain, searched, prep[p], p, &downloads, &best);
    WriteResult3D(searches[p], prep[p], best, &found[p], &results[p]);
  }
  laps.Lap("results");
  if (laps.enabled)
    fprintf(stderr, "[cmx host] RunSearches3D(%d):%s us\n", num, laps.report.c_str());
  return false;
}

// The shared lists of a chain dropped nodes: every search again in a chain of its own.
void SearchEachAlone3D(const Search3D* searches, Prepared3D* prep, int num, int32_t* found,
                       cmx_result3d* results, cmx_match_stats* stats) {
  for (int p = 0; p < num; ++p) {
    cmx_match_stats again{};
    RunChain3D(searches + p, prep + p, 1, found + p, results + p, &again);
    stats->candidates_scored += again.candidates_scored;
    stats->nodes_expanded += again.nodes_expanded;
    stats->device_ms += again.device_ms;
  }
}

// `num` searches, each of its own node's data (Search3D::data; equal pointers = one node, whose
// clouds go up once per chain of launches).  All searches must live on the same device.  The
// searches run in ONE chain of launches (RunChain3D) unless the index ranges say otherwise:
// then in consecutive sub-batches that fit, one after the other, statistics summed.
void Match3DMany(const Search3D* searches, int num, int32_t* found, cmx_result3d* results,
                 cmx_match_stats* stats) {
  CMX_REQUIRE(searches && num >= 1 && found && results, "null output");
  const int device = searches[0].m->device;
  int min_depth = kMaxDepth;
  for (int p = 0; p < num; ++p) {
    const Fast3DMatcher& m = *searches[p].m;
    CMX_REQUIRE(searches[p].data != nullptr, "null node data");
    const cmx_node_data3d& data = *searches[p].data->data;
    CMX_REQUIRE(m.device == device, "the searches of a batch must share a device");
    CMX_REQUIRE(data.histogram_size == static_cast<int>(m.histogram.size()),
                "histogram size %d does not match the submap's %d", data.histogram_size,
                static_cast<int>(m.histogram.size()));
    CMX_REQUIRE(searches[p].wxy >= 0 && searches[p].wz >= 0 && searches[p].wxy < (1 << 20) &&
                    searches[p].wz < (1 << 20),
                "bad search window");
    min_depth = std::min(min_depth, m.options.branch_and_bound_depth);
    found[p] = 0;
  }
  if (num > 1 && min_depth < 2) {     // depth-1 stacks take the leaf-verification path: one by one
    cmx_match_stats total{};
    for (int p = 0; p < num; ++p) {
      cmx_match_stats st{};
      Match3DMany(searches + p, 1, found + p, results + p, &st);
      AddStats3D(st, &total);
    }
    if (stats) *stats = total;
    return;
  }
  std::vector<Prepared3D> prep(num);
  for (int p = 0; p < num; ++p) PrepareSearch3D(searches[p], &prep[p]);

  // Sub-batches: consecutive searches while the lowest-resolution candidates and the discretised
  // cells (scans x points, summed) of a chain of launches stay below 2^31 -- its 32-bit index
  // ranges.  A search that exceeds them alone is an error there ("batch too large").  The debug
  // switch fast3d_chunk_cells lowers the cap on the cells (tests).
  const size_t kIndexRange = size_t(1) << 31;
  const size_t cell_cap = Debug().fast3d_chunk_cells > 0
                              ? std::min(static_cast<size_t>(Debug().fast3d_chunk_cells), kIndexRange)
                              : kIndexRange;
  cmx_match_stats total{};
  for (int first = 0; first < num;) {
    size_t coarse = 0, cells = 0;
    int end = first;
    for (; end < num; ++end) {
      const size_t pair_cells = static_cast<size_t>(prep[end].S) *
                                searches[end].data->data->num_high_resolution_points;
      if (end > first && (coarse + static_cast<size_t>(prep[end].total) >= kIndexRange ||
                          cells + pair_cells >= cell_cap))
        break;
      coarse += static_cast<size_t>(prep[end].total);
      cells += pair_cells;
    }
    cmx_match_stats st{};
    if (RunChain3D(searches + first, prep.data() + first, end - first, found + first,
                   results + first, &st))
      SearchEachAlone3D(searches + first, prep.data() + first, end - first, found + first,
                        results + first, &st);
    if (first == 0 && end == num) total = st;      // (one chain: its statistics as they are)
    else AddStats3D(st, &total);
    first = end;
  }
  if (stats) *stats = total;
}

// One search of `data` against `matcher`.
void Match3D(const cmx_fast3d* matcher, bool full_submap, const cmx_pose3d& node_pose,
             const cmx_pose3d& submap_pose, const cmx_node_data3d& data, float min_score,
             int32_t* found, cmx_result3d* result, cmx_match_stats* stats) {
  NodeHost3D node = NodeOf3D(data);
  node.max_point = FarthestPoint3D(data);
  const Search3D one =
      MakeSearch3D(matcher->impl, &node, full_submap, node_pose, submap_pose, min_score);
  Match3DMany(&one, 1, found, result, stats);
}

// Match / MatchFullSubmap arguments of every pair, then one chain of launches per device and
// `group` pairs (Match3DMany).  matchers[p] and datas[p] are not null.
void MatchPairs3D(const cmx_fast3d* const* matchers, int num_pairs, const cmx_pose3d* node_poses,
                  const cmx_pose3d* submap_poses, const int32_t* match_full_submap,
                  const float* min_scores, const cmx_node_data3d* const* datas, int32_t* found,
                  cmx_result3d* results, cmx_match_stats* stats) {
  // The distinct nodes of the call (equal pointers = one node), each prepared once.
  std::vector<NodeHost3D> nodes;
  nodes.reserve(num_pairs);                              // (searches keep pointers into it)
  std::unordered_map<const cmx_node_data3d*, const NodeHost3D*> node_of;
  for (int p = 0; p < num_pairs; ++p) {
    if (node_of.count(datas[p])) continue;
    nodes.push_back(NodeOf3D(*datas[p]));
    node_of[datas[p]] = &nodes.back();
  }
  ParallelFor(static_cast<int>(nodes.size()), 3,
              [&](int k) { nodes[k].max_point = FarthestPoint3D(*nodes[k].data); });
  std::vector<Search3D> searches(num_pairs);
  for (int p = 0; p < num_pairs; ++p)
    searches[p] = MakeSearch3D(matchers[p]->impl, node_of[datas[p]], match_full_submap[p] != 0,
                               node_poses[p], submap_poses[p], min_scores[p]);
  // The debug switch fast3d_batch caps the searches per chain (tools / tests; 1 = one by one).
  const int group = Debug().fast3d_batch > 0 ? Debug().fast3d_batch : 64;
  cmx_match_stats total{};
  std::vector<char> done(num_pairs, 0);
  for (int first = 0; first < num_pairs; ++first) {
    if (done[first]) continue;
    // the not yet searched pairs on this pair's device, `group` at a time
    std::vector<int> idx;
    for (int p = first; p < num_pairs && static_cast<int>(idx.size()) < group; ++p)
      if (!done[p] && searches[p].m->device == searches[first].m->device) idx.push_back(p);
    std::vector<Search3D> part(idx.size());
    std::vector<int32_t> part_found(idx.size(), 0);
    std::vector<cmx_result3d> part_results(idx.size());
    for (size_t k = 0; k < idx.size(); ++k) part[k] = searches[idx[k]];
    cmx_match_stats st{};
    Match3DMany(part.data(), static_cast<int>(part.size()), part_found.data(),
                part_results.data(), &st);
    for (size_t k = 0; k < idx.size(); ++k) {
      done[idx[k]] = 1;
      found[idx[k]] = part_found[k];
      if (part_found[k]) results[idx[k]] = part_results[k];
    }
    AddStats3D(st, &total);
  }
  if (stats) *stats = total;
}
}  // namespace
}  // namespace cmx

extern "C" {

cmx_status cmx_fast3d_match(const cmx_fast3d* matcher, const cmx_pose3d* global_node_pose,
                            const cmx_pose3d* global_submap_pose, const cmx_node_data3d* data,
                            float min_score, int32_t* found, cmx_result3d* result,
                            cmx_match_stats* stats) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(matcher && global_node_pose && global_submap_pose && data, "null argument");
    Match3D(matcher, false, *global_node_pose, *global_submap_pose, *data, min_score, found,
            result, stats);
  });
}

cmx_status cmx_fast3d_match_full_submap(const cmx_fast3d* matcher,
                                        const double* global_node_rotation_wxyz,
                                        const double* global_submap_rotation_wxyz,
                                        const cmx_node_data3d* data, float min_score,
                                        int32_t* found, cmx_result3d* result,
                                        cmx_match_stats* stats) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(matcher && global_node_rotation_wxyz && global_submap_rotation_wxyz && data,
                "null argument");
    CMX_REQUIRE(data->high_resolution_point_cloud && data->num_high_resolution_points >= 1,
                "empty high-resolution point cloud");
    cmx_pose3d node{}, submap{};
    std::copy(global_node_rotation_wxyz, global_node_rotation_wxyz + 4, node.q);
    std::copy(global_submap_rotation_wxyz, global_submap_rotation_wxyz + 4, submap.q);
    Match3D(matcher, true, node, submap, *data, min_score, found, result, stats);
  });
}

// The ConstraintBuilder3D fan-out (constraints/constraint_builder_3d.cc:79-147): one node's
// constant data against many submaps' matchers, windowed and full-submap pairs mixed.  The
// reference runs one thread-pool task per pair; here the pairs of a node are ONE chain of
// launches (Match3DMany: every kernel indexes the search with blockIdx.y or through its nodes,
// frontier and leaf lists are shared), so a level of all searches is one launch instead of
// one short launch per search.  `node_poses[p]` / `submap_poses[p]`: the global poses of pair
// p (only their rotations are read where match_full_submap[p] != 0).
cmx_status cmx_fast3d_match_batch(const cmx_fast3d* const* matchers, int32_t num_pairs,
                                  const cmx_pose3d* node_poses, const cmx_pose3d* submap_poses,
                                  const int32_t* match_full_submap, const float* min_scores,
                                  const cmx_node_data3d* data, int32_t* found,
                                  cmx_result3d* results, cmx_match_stats* stats) {
  using namespace cmx;
  return Guard([&] {
    CMX_REQUIRE(matchers && node_poses && submap_poses && match_full_submap && min_scores &&
                    data && found && results && num_pairs >= 1,
                "null argument");
    for (int p = 0; p < num_pairs; ++p) CMX_REQUIRE(matchers[p] != nullptr, "null matcher handle");
    const auto entry_time = std::chrono::steady_clock::now();
    // The case "all pairs share one data" of MatchPairs3D.
    const std::vector<const cmx_node_data3d*> datas(num_pairs, data);
    MatchPairs3D(matchers, num_pairs, node_poses, submap_poses, match_full_submap, min_scores,
                 datas.data(), found, results, stats);
    if (Debug().host_trace)
      fprintf(stderr, "[cmx host] cmx_fast3d_match_batch(%d): %.0f us\n", num_pairs,
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() -
                                                        entry_time).count());
  });
}

// The other half of PoseGraph3D::ComputeConstraintsForNode (pose_graph_3d.cc:370-379): a
// finished submap against every old node, or any list of (node, submap) pairs -- pair p with
// its own data[p].  One chain of launches as above; a node named by several pairs is staged once.
cmx_status cmx_fast3d_match_pairs(const cmx_fast3d* const* matchers, int32_t num_pairs,
                                  const cmx_pose3d* node_poses, const cmx_pose3d* submap_poses,
                                  const int32_t* match_full_submap, const float* min_scores,
                                  const cmx_node_data3d* const* data, int32_t* found,
                                  cmx_result3d* results, cmx_match_stats* stats) {
  using namespace cmx;
  return Guard([&] {
    // (a matcher handle cannot exist without a device: say so, whatever the arguments are)
    if (cmx_device_count() <= 0) UseDevice(0);
    CMX_REQUIRE(num_pairs >= 1, "num_pairs must be at least 1");
    CMX_REQUIRE(matchers && node_poses && submap_poses && match_full_submap && min_scores &&
                    data && found && results,
                "null argument");
    for (int p = 0; p < num_pairs; ++p) {
      CMX_REQUIRE(matchers[p] != nullptr, "null matcher handle");
      CMX_REQUIRE(data[p] != nullptr, "the node data of pair %d is null", p);
      CMX_REQUIRE(matchers[p]->impl.device == matchers[0]->impl.device,
                  "the matchers of a call must live on one device (pair %d)", p);
      CMX_REQUIRE(data[p]->histogram_size == static_cast<int>(matchers[p]->impl.histogram.size()),
                  "histogram size %d of pair %d does not match its submap's %d",
                  data[p]->histogram_size, p,
                  static_cast<int>(matchers[p]->impl.histogram.size()));
    }
    MatchPairs3D(matchers, num_pairs, node_poses, submap_poses, match_full_submap, min_scores,
                 data, found, results, stats);
  });
}

}  // extern "C"
