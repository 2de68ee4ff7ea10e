// The host's plan of a real-time 2D tile-matcher call (rt_2d_tiles.hip): every LDS byte of its
// kernels, the tile geometry of every match, the work items, the launch grid, and every offset of
// the scratch regions and of the upload block -- as plain C++17 without a HIP type, so that a
// stand-alone program checks it under the sanitizers (tests/native/rt2d_plan_check.cc).  The
// sizing constants and LDS-size functions the kernels share with the planner live here too: no
// kernel keeps a private copy of a size the planner computes.
//
// PlanRt2DTiles() runs the named stages below in order; StageRt2DTiles() lays out the upload block.
#ifndef CMX_RT_2D_PLAN_H_
#define CMX_RT_2D_PLAN_H_
#include <stddef.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>
#ifdef __HIPCC__
#define CMX_RT2D_HD __host__ __device__
#else
#define CMX_RT2D_HD
#endif

namespace cmx {

constexpr int kRt2DMaxPoints = 8192;        // points per scan the tile path takes
constexpr int kMaxRowsPerLane = 8;
#ifndef CMX_RT2D_TASK_ITERS
#define CMX_RT2D_TASK_ITERS 64
#endif
constexpr int kPairTaskIters = CMX_RT2D_TASK_ITERS;          // iterations (entries per stream) of one task
#ifndef CMX_RT2D_JOB_CHUNKS
#define CMX_RT2D_JOB_CHUNKS 8
#endif
constexpr int kJobChunks = CMX_RT2D_JOB_CHUNKS;                // chunks of 64 points of one rotation a wavefront discretises in one job
constexpr int kFusedMaxPoints = 2048;        // (clouds beyond: the prep kernel, more rotations per workgroup)
constexpr int kMaxTiles = 16;               // tiles of a match's bounding box (x 4 phases = 64 keys)
constexpr int kStage1Cap = 1024;            // candidates the exact integer pass takes per match

// ---- block bounds (rt_2d_bounds.h) ----------------------------------------------------------------
constexpr int kBoundMinMatches = 96;        // matches per call from which the bound kernel is the default
constexpr int kBoundMaxBlocks = 8;          // block columns in one ds_read_b64: side <= 16
constexpr int kBoundDiscBytes = 48;         // sizeof(BoundDisc): a rotation's discretisation constants
constexpr int kBoundListCap = 128;           // blocks phase C sums per match; more: the per-candidate kernels
// words of the block-sum region: the sums of the match's blocks, later the summed candidates
// (index, quantised sum) the fused finish looks at
CMX_RT2D_HD constexpr size_t BoundSumWords(int blocks) {
  return (static_cast<size_t>(blocks > 8 * (kBoundListCap + 1) ? blocks : 8 * (kBoundListCap + 1)) + 3) & ~size_t{3};
}
constexpr int kBoundTailGroup = 2;           // finalists per round of f32 chains (LDS rows)
CMX_RT2D_HD constexpr size_t BoundTailRegion(int n_pad, int num_scans) {
  const size_t fin = 4 * static_cast<size_t>(n_pad) + static_cast<size_t>(kBoundTailGroup) * 4 * (static_cast<size_t>(n_pad) + 4) +
                     4 * ((static_cast<size_t>(num_scans) + 3) & ~size_t{3}) + 12 * static_cast<size_t>(kStage1Cap);
  const size_t cloud = 8 * static_cast<size_t>(n_pad);
  return ((fin > cloud ? fin : cloud) + 15) & ~size_t{15};
}
CMX_RT2D_HD constexpr size_t BoundTailLds(int n_pad, int num_scans, int nb) {
  return BoundTailRegion(n_pad, num_scans) + 8 * ((static_cast<size_t>(num_scans) + 1) & ~size_t{1}) +
         4 * BoundSumWords(num_scans * nb * nb) + 20 * size_t{kBoundListCap};
}
constexpr int kList4Cap = 96;                // 4 x 4 blocks summed per match besides the best; more: the per-candidate kernels
                                             // (a wavefront per block: a match with hundreds of them holds its
                                             // whole launch up for longer than its repeat takes)
constexpr int kCand4Cap = 512;               // candidates handed to the finish; more (a landscape of ties): the same
CMX_RT2D_HD constexpr size_t Tail4Region(int lp, int lh, int n_pad, int num_scans) {
  const size_t fin = BoundTailRegion(n_pad, num_scans);
  const size_t own = static_cast<size_t>(lh) * lp + ((4 * static_cast<size_t>(lp) + 16 + 15) & ~size_t{15}) +
                     8 * static_cast<size_t>(n_pad);
  return ((fin > own ? fin : own) + 15) & ~size_t{15};
}
CMX_RT2D_HD constexpr size_t BoundTail4Lds(int lp, int lh, int n_pad, int num_scans, int nb4) {
  return Tail4Region(lp, lh, n_pad, num_scans) + kBoundDiscBytes * static_cast<size_t>(num_scans) +
         4 * ((static_cast<size_t>(num_scans) * nb4 * nb4 + 3) & ~size_t{3}) +
         4 * static_cast<size_t>(16 + kList4Cap + 2 * kCand4Cap) + 64;
}

inline size_t Align16(size_t v) { return (v + 15) & ~static_cast<size_t>(15); }

// Conflict-free LDS row pitch (bytes, a multiple of 16, >= min_bytes; 0: none exists): the H x B
// 8-byte blocks a half-wavefront reads in one LDS cycle fall into 2 H B distinct banks for every
// base address.  The bank pattern depends on the pitch modulo 256 only: the sixteen residues are
// tested once per (H, B).
inline int ConflictFreePitch(int H, int B, int min_bytes) {
  static std::mutex mu;
  static int valid[33][33];                  // bit k: pitch = 16 k (mod 256) is conflict-free; -1 unset
  static bool init = false;
  unsigned mask;
  {
    std::lock_guard<std::mutex> lock(mu);
    if (!init) {
      for (auto& row : valid) for (int& v : row) v = -1;
      init = true;
    }
    if (valid[H][B] < 0) {
      int m = 0;
      for (int k = 0; k < 16; ++k) {
        const int cand = 16 * k + 256;
        unsigned long long used = 0;
        bool ok = true;
        for (int r = 0; r < H && ok; ++r)
          for (int b = 0; b < B && ok; ++b)
            for (int w = 0; w < 2; ++w) {
              const int bank = ((r * cand + b * 8) / 4 + w) & 63;
              if (used >> bank & 1) ok = false;
              used |= 1ull << bank;
            }
        if (ok) m |= 1 << k;
      }
      valid[H][B] = m;
    }
    mask = static_cast<unsigned>(valid[H][B]);
  }
  if (mask == 0) return 0;
  for (int cand = (min_bytes + 15) & ~15;; cand += 16)
    if (mask >> ((cand >> 4) & 15) & 1) return cand;
}

struct TileGeometry {
  int B, H, hl, ht, gpitch, grows;
  int box_x0, box_y0, T, ntx, nty, lp, th_img, tile_image_bytes;
  int cap_s, gmin, gmax, target, rw, list_lds, task_cap;
  int groups;               // fused: the rotation groups (work items) of this match, chosen by the host
  size_t lds;               // of the tile kernel
  size_t image_bytes;       // of the grid image in HBM: quantised image + pooled planes
  size_t q_bytes;           // of the quantised image alone (the planes start behind it)
  int m2_pitch, m2_rows;    // pooled planes (0: window beyond 16 x 16, no planes)
  int b_lpb, b_lh;          // bound kernel: LDS copy of the planes
  size_t b_lds;             // bound kernel: dynamic LDS of this match
  size_t b_finish_room;     // of it: planes | zeros | cloud, which its fused finish lays out anew
  size_t b_tail_at;         // where the rest starts: behind those, and behind what the finish needs
  int m4_pitch, m4_rows;    // 4 x 4 pooled planes (round 6)
  size_t q8_bytes;          // the byte image behind them
  int b8_lp, b8_lh;         // tail kernel: LDS box of the byte image
  size_t t4_lds;
  int b4_lpb, b4_lh, b4_pstride;
  size_t b4_tail_at, b4_lds;
};

// ---- inputs ---------------------------------------------------------------------------------------
struct Rt2DPlanMatch {
  int n;                               // points of the cloud
  int num_x_cells, num_y_cells;        // the grid's limits
  double resolution, max_x, max_y;
  double x, y;                         // initial pose
  int nl, num_scans;                   // Rt2DSearch
  float max_range;
  bool device_xyz, device_cells;       // cloud / cells already in HBM: no room in the upload block
};
struct Rt2DPlanSwitches {              // the debug switches of the same names (cmx_common.h)
  int rt2d_lds_kb = 0, rt2d_tile = 0, rt2d_unfused = 0, rt2d_groups = 0, rt2d_target = 0;
  int rt2d_no_bounds = 0, rt2d_bounds = 0, rt2d_bounds_verify = 0, rt2d_bounds_fused = 0;
  int rt2d_bounds_level = 0;
};
struct Rt2DPlanCall {
  int cus = 256;                       // compute units of the device
  int share = 1;                       // calls sharing the device (the parts of a batch)
  int batch_matches = 0;               // matches of the whole batch (>= the call's)
  Rt2DPlanSwitches dbg;
};

// ---- outputs --------------------------------------------------------------------------------------
// Where a match's share of the launch's HBM scratch starts (lists in bytes, the rest in elements),
// and its rotation table among the call's.
struct Rt2DMatchAt { size_t lists, hdr, qsum, table; int ub; };
struct Rt2DPlan {
  std::vector<TileGeometry> geo;
  std::vector<Rt2DMatchAt> at;
  int rpl = 1, max_scans = 0, common_stride = -1, group = 8;
  size_t tile_lds = 0, prep_lds = 0, finish_lds = 0;
  size_t lists_total = 0, hdr_total = 0, qsum_total = 0, ub_total = 0, tables_total = 0;
  long long work_cap = 0, entries_total = 0;
  int tile_grid = 0, tile_threads = 512;
  bool fused = false;                   // one tile per match, prep fused into the tile kernel
  bool bounds = false;                  // block bounds first (rt_2d_bounds.h): fused shape only
  bool split = false;                   // ... with the tail of every match in a kernel of its own
  bool level4 = false;                  // ... and blocks of 4 x 4 translations first (always split)
  size_t tail_lds = 0;
  size_t bound4_lds = 0, tail4_lds = 0;
  int bound_nb = 0;                     // blocks per window axis (launch-wide: the largest)
  size_t bound_lds = 0;
};
// The upload block: params | per match: xyz, rotations, cells | counters | tickets | work | misc.
struct Rt2DStagingAt { size_t xyz, rot, cells; };
struct Rt2DStaging {
  std::vector<Rt2DStagingAt> match;
  size_t counters = 0;                  // [0] work items, [1] next item (zeroed)
  size_t tickets = 0;                   // block bounds: a ticket counter per match (zeroed)
  size_t work = 0;                      // fused: the work items, listed here
  size_t misc = 0;                      // the matches' result words, 128 each
  size_t bytes = 0;
};

// Matches with the same window (the usual batch) share ONE tile geometry, chosen for the largest
// box, cloud and rotation count among them.
struct Rt2DWindowClass { int nl, span_x, span_y, n_pad, scans, items; TileGeometry g; };
struct Rt2DReach { int span_x, span_y, window_class; };

// ---- window geometry per item; launch-wide rows per lane: the largest any item needs.
// (H = the most rows of B blocks a half-wavefront holds for which a conflict-free pitch of whole
// 16-byte DMA pieces exists: e.g. 8 rather than 10 rows of 3 blocks)
inline bool Rt2DBlockShapes(const Rt2DPlanMatch* in, int num, TileGeometry* geo, int* rows_per_lane) {
  int rpl = 1;
  for (int m = 0; m < num; ++m) {
    const int side = 2 * in[m].nl + 1;
    const int B = (side + 3 + 3) / 4;
    if (B > 32 || in[m].n > kRt2DMaxPoints || in[m].num_scans > 4096) return false;
    if (in[m].num_x_cells > 32000 || in[m].num_y_cells > 32000)
      return false;                                        // (cells travel as int16 pairs)
    int H = m > 0 && geo[m - 1].B == B ? geo[m - 1].H : 32 / B;
    while (H > 1 && ConflictFreePitch(H, B, 16) == 0) --H;
    geo[m].B = B;
    geo[m].H = H;
    rpl = std::max(rpl, (side + H - 1) / H);
  }
  if (rpl > kMaxRowsPerLane) return false;
  if (rpl == 5) rpl = 6;
  if (rpl == 7) rpl = 8;                         // (instantiated: 1, 2, 3, 4, 6, 8 rows per lane)
  *rows_per_lane = rpl;
  return true;
}

// ---- per item: the box of window starts the scan can reach.  Every rotated point lies within
// max_range of the initial translation (plus a cell for the f32 roundings of rotation and
// index, plus the half cell of lround); cells are clamped to [-(nl + 1), n + nl] as on the
// device.  Returns the entries (points x rotations) of the call.
inline long long Rt2DReachBoxes(const Rt2DPlanMatch* in, int num, TileGeometry* geo, Rt2DReach* reach,
                                std::vector<Rt2DWindowClass>* classes) {
  long long entries_total = 0;
  for (int m = 0; m < num; ++m) {
    const Rt2DPlanMatch& it = in[m];
    TileGeometry& g = geo[m];
    const int nx = it.num_x_cells, ny = it.num_y_cells, nl = it.nl;
    g.hl = (2 * nl + 1 + 7) & ~7;
    g.ht = 2 * nl + 1;
    const double res = it.resolution;
    const double range = (it.max_range * (1.0 + 1e-5)) / res + 2.0;
    const double cxc = (it.max_y - it.y) / res - 0.5;   // cell x from the map's y
    const double cyc = (it.max_x - it.x) / res - 0.5;
    const auto clampi = [](double v, int lo, int hi) {
      return static_cast<int>(std::min<double>(std::max<double>(v, lo), hi));
    };
    const int ix_lo = clampi(std::floor(cxc - range), -(nl + 1), nx + nl);
    const int ix_hi = clampi(std::ceil(cxc + range), -(nl + 1), nx + nl);
    const int iy_lo = clampi(std::floor(cyc - range), -(nl + 1), ny + nl);
    const int iy_hi = clampi(std::ceil(cyc + range), -(nl + 1), ny + nl);
    g.box_x0 = (ix_lo - nl + g.hl) & ~7;
    g.box_y0 = iy_lo - nl + g.ht;
    reach[m].span_x = ix_hi - nl + g.hl - g.box_x0 + 1;
    reach[m].span_y = iy_hi - nl + g.ht - g.box_y0 + 1;
    const int n_pad = (it.n + 63) / 64 * 64;
    int c = 0;
    while (c < static_cast<int>(classes->size()) && (*classes)[c].nl != nl) ++c;
    if (c == static_cast<int>(classes->size())) classes->push_back(Rt2DWindowClass{nl, 0, 0, 0, 0, 0, g});
    Rt2DWindowClass& k = (*classes)[c];
    k.span_x = std::max(k.span_x, reach[m].span_x); k.span_y = std::max(k.span_y, reach[m].span_y);
    k.n_pad = std::max(k.n_pad, n_pad); k.scans = std::max(k.scans, it.num_scans);
    ++k.items;
    reach[m].window_class = c;
    entries_total += static_cast<long long>(it.n) * it.num_scans;
  }
  return entries_total;
}

// ---- the tile chooser: does a class fit tiles of core T within `budget` bytes of LDS?  On true,
// *out holds the tile's shape.  (`k` is only read; out may be its own geometry.)
inline bool Rt2DTileFits(const Rt2DWindowClass* k, int rpl, int T, size_t budget, bool one_tile,
                         bool fuse, TileGeometry* out) {
  const int H = k->g.H, B = k->g.B;
  const int side = 2 * k->nl + 1;
  const int rows_extra = rpl * H;
  const int cap_tile = k->n_pad + 64;                // a rotation's entries of ONE tile, padded
  const int ntx = (k->span_x + T - 1) / T, nty = (k->span_y + T - 1) / T;
  if (ntx * nty > (one_tile ? 1 : kMaxTiles)) return false;
  const int lp = ConflictFreePitch(H, B, 2 * (T + 4 * B));
  if (lp == 0) return false;
  const int th_img = T + rows_extra;
  const int image = ((th_img + rows_extra) * lp + 1023) & ~1023;
  // rotations a workgroup's LDS holds: all of them (the planner gives a light tile ONE item)
  // or -- one tile per match -- as many as fit beside the image
  for (int gmin = std::max(1, (k->scans + 63) / 64); gmin <= k->scans; ++gmin) {
    const int rw = (k->scans + gmin - 1) / gmin;
    const bool fused_shape = one_tile && fuse;
    // (fused: rw = the rotations of one ROUND; a discretisation job's region of the list buffer
    // holds its chunks' entries plus the padding of four sub-lists, its tasks two more than its
    // chunks: Rt2DTileKernel)
    const int jpr = (k->n_pad / 64 + kJobChunks - 1) / kJobChunks;
    const int cap_rot = fused_shape ? k->n_pad + 64 * jpr : cap_tile;
    const int task_cap = fused_shape ? rw * jpr * (kJobChunks + 2) : rw * (k->n_pad / kPairTaskIters + 2);
    size_t fixed = static_cast<size_t>(image) + 4 * ((static_cast<size_t>(rw) * side * side + 3) & ~size_t{3}) +
                   16 * static_cast<size_t>(rw) + 4 * ((static_cast<size_t>(rw) + 1 + 3) & ~size_t{3}) +
                   16 * static_cast<size_t>(task_cap) + 64;
    if (fused_shape) {
      // (all rotations of the match, the cloud rotated by the initial yaw)
      fixed += 8 * ((static_cast<size_t>(k->scans) + 1) & ~size_t{1}) + 8 * static_cast<size_t>(k->n_pad);
    }
    if (fixed + 2 * static_cast<size_t>(cap_rot) > budget) {
      if (!one_tile) return false;
      continue;                                      // fewer rotations per workgroup
    }
    // list buffer: what is left, at most every rotation's entries at once
    const size_t want = static_cast<size_t>(rw) * cap_rot;
    const size_t room = (budget - fixed) / 2;
    if (one_tile && room < want) continue;           // (all of an item's lists in one round)
    out->list_lds = static_cast<int>(std::min(want, room) & ~size_t{7});
    out->T = T; out->ntx = ntx; out->nty = nty; out->lp = lp; out->th_img = th_img;
    out->tile_image_bytes = image; out->gmin = gmin; out->rw = rw; out->task_cap = task_cap;
    out->lds = fixed + 2 * static_cast<size_t>(out->list_lds);
    return true;
  }
  return false;
}

// The largest tile core from t_first down that leaves room for two workgroups per CU, then
// (`smaller_core`) the smallest core with the same number of tiles (less image to stage, more room
// for lists).
inline bool Rt2DSeveralTiles(Rt2DWindowClass* k, int rpl, int t_first, size_t budget, bool smaller_core) {
  TileGeometry& g = k->g;
  bool found = false;
  for (int T = t_first; T >= 16 && !found; T -= 8) found = Rt2DTileFits(k, rpl, T, budget, false, false, &g);
  if (found && smaller_core) {
    TileGeometry smaller = g;
    for (int T = g.T - 8; T >= 16; T -= 8) {
      if ((k->span_x + T - 1) / T != g.ntx || (k->span_y + T - 1) / T != g.nty) break;
      if (Rt2DTileFits(k, rpl, T, budget, false, false, &smaller)) g = smaller;
    }
  }
  return found;
}

// Two shapes.  (1) ONE tile per match, a workgroup of 1024 threads alone on its CU (up to
// 150 KB of LDS): whenever the whole box of a match fits -- the items of a match are then its
// rotation groups, all of one size, their sums plain stores.  C1's box (217 window starts per
// axis at 5 cm) is such a case: as four tiles one of them held most of the points, and the
// planner's smaller items each paid the ~4 us before their first window update.  (2) Several
// tiles, workgroups of 512 threads, two per CU (76 KB each): boxes beyond that (long-range
// scans, fine grids), sums by atomics.  False: a class fits neither.
inline bool Rt2DChooseShape(std::vector<Rt2DWindowClass>* classes, int rpl, const Rt2DPlanSwitches& dbg,
                            bool* single_tile_out, bool* want_fused_out) {
  const size_t kLdsTwoPerCu = (dbg.rt2d_lds_kb > 0 ? dbg.rt2d_lds_kb : 76) * size_t{1024};
  const size_t kLdsOnePerCu = 150 * size_t{1024};
  bool single_tile = dbg.rt2d_tile <= 0;
  bool want_fused = !dbg.rt2d_unfused;
  for (const Rt2DWindowClass& k : *classes) want_fused = want_fused && k.n_pad <= kFusedMaxPoints;
  for (Rt2DWindowClass& k : *classes) {
    bool found = false;
    if (single_tile) {
      const int T = (std::max(k.span_x, k.span_y) + 7) & ~7;
      found = Rt2DTileFits(&k, rpl, T, kLdsOnePerCu, true, want_fused, &k.g);
      if (!found) single_tile = false;
    }
    if (!found)
      found = Rt2DSeveralTiles(&k, rpl, dbg.rt2d_tile > 0 ? (dbg.rt2d_tile & ~7) : 128, kLdsTwoPerCu,
                               dbg.rt2d_tile <= 0);
    if (!found) return false;
  }
  // (classes of one launch share the shape: a class that needs several tiles puts all on shape 2:
  // a one-tile class beyond the two-per-CU budget is planned again with it)
  if (!single_tile)
    for (Rt2DWindowClass& k : *classes)
      if (k.g.ntx * k.g.nty == 1 && k.g.lds > kLdsTwoPerCu && !Rt2DSeveralTiles(&k, rpl, 128, kLdsTwoPerCu, false))
        return false;
  *single_tile_out = single_tile;
  *want_fused_out = want_fused;
  return true;
}

// ---- per match: its class's tile, its own tiles, rotation groups and work items.
inline void Rt2DMatchTiles(const Rt2DPlanMatch& it, const TileGeometry& cg, const Rt2DReach& reach,
                           int target, bool fused, const Rt2DPlanSwitches& dbg, TileGeometry* geo) {
  TileGeometry& g = *geo;
  const int n_pad = (it.n + 63) / 64 * 64;
  g.T = cg.T; g.lp = cg.lp; g.th_img = cg.th_img; g.tile_image_bytes = cg.tile_image_bytes;
  g.task_cap = cg.task_cap; g.list_lds = cg.list_lds; g.lds = cg.lds;
  g.ntx = (reach.span_x + g.T - 1) / g.T;
  g.nty = (reach.span_y + g.T - 1) / g.T;
  // (rotations per workgroup: the class's -- its LDS is sized for that -- in as few groups as
  // this match's own rotation count needs)
  g.rw = std::min(cg.rw, it.num_scans);
  g.gmin = (it.num_scans + g.rw - 1) / g.rw;
  g.gmax = dbg.rt2d_groups > 0 ? std::max(fused ? 1 : g.gmin, std::min(dbg.rt2d_groups, it.num_scans))
                               : std::max(g.gmin, std::min(it.num_scans, 32));
  g.target = target;
  g.groups = 0;
  if (fused) {                         // the planner's rule (Rt2DTilePrepKernel), on the host
    const long long entries = static_cast<long long>(it.n) * it.num_scans;
    // (any number of groups: an item takes its rotations in rounds of g.rw)
    long long G = std::max<long long>(1, (entries + target / 2) / target);
    G = std::min<long long>(G, std::min(g.gmax, it.num_scans));
    g.groups = static_cast<int>(std::max<long long>(G, 1));
  }
  g.cap_s = n_pad + 16 * 4 * g.ntx * g.nty;
}

// ---- per match: the grid image in HBM -- halo + grid, rows of whole 16-byte pieces, one zero row
// below (what lies right of or below it is zeros by definition: the tile DMA substitutes the zero
// corner) -- and behind it the pooled planes (rt_2d_bounds.h) and the byte image.  They are part
// of the image whenever the window allows them, whichever kernel this call runs: a cached image
// serves both.
inline void Rt2DImageSizes(const Rt2DPlanMatch& it, TileGeometry* geo) {
  TileGeometry& g = *geo;
  const int nx = it.num_x_cells, ny = it.num_y_cells;
  g.gpitch = 2 * ((g.hl + nx + 7) & ~7);
  g.grows = g.ht + ny + 1;
  g.q_bytes = Align16(static_cast<size_t>(g.gpitch) * g.grows);
  g.m2_pitch = g.m2_rows = 0;
  g.m4_pitch = g.m4_rows = 0;
  if (2 * it.nl + 1 <= 2 * kBoundMaxBlocks) {
    // (room behind the last column a window reads: the bound kernel copies 8-byte pieces)
    g.m2_pitch = (((nx + g.hl) >> 1) + 28 + 3) & ~3;
    g.m2_rows = ((ny + g.ht) >> 1) + kBoundMaxBlocks + 2;
    // (the sixteen phase planes of the 4 x 4 pooling: four block columns / rows and the 8-byte
    // pieces of the LDS copy behind the last window start)
    g.m4_pitch = (((nx + g.hl) >> 2) + 20 + 3) & ~3;
    g.m4_rows = ((ny + g.ht) >> 2) + 4 + 2;
  }
  g.q8_bytes = g.m4_rows ? Align16(static_cast<size_t>(g.gpitch >> 1) * g.grows) : 0;
  g.image_bytes = g.q_bytes + 4 * static_cast<size_t>(g.m2_pitch) * g.m2_rows +
                  16 * static_cast<size_t>(g.m4_pitch) * g.m4_rows + g.q8_bytes;
}

// ---- per match: the LDS of the bound kernels and of the 4 x 4 tail (`nb`: blocks per window
// axis, launch-wide -- the kernel is instantiated for the largest).  b_lds still lacks b_tail_at:
// Rt2DDecideBounds.
inline void Rt2DBoundShapes(const Rt2DPlanMatch& it, int nb, TileGeometry* geo) {
  TileGeometry& g = *geo;
  const int n_pad = (it.n + 63) / 64 * 64;
  // (rows are read as three aligned dwords and copied in 8-byte pieces; an odd number of
  // 8-byte pieces: the rows of a wall on different banks)
  g.b_lpb = ((g.T >> 1) + 12 + 4 + 7) & ~7;
  if ((g.b_lpb & 15) == 0) g.b_lpb += 8;
  g.b_lh = (g.T >> 1) + nb + 1;
  // planes | zeros | cloud: what the finish of the match is laid out in afterwards
  g.b_finish_room = 4 * static_cast<size_t>(g.b_lh) * g.b_lpb + ((static_cast<size_t>(nb) * g.b_lpb + 16 + 15) & ~size_t{15}) +
                    8 * static_cast<size_t>(n_pad);
  // | rotations | block sums (later: the summed candidates and their sums) | list | its sums
  g.b_lds = 8 * ((static_cast<size_t>(it.num_scans) + 1) & ~size_t{1}) +
            4 * BoundSumWords(it.num_scans * nb * nb) + 20 * size_t{kBoundListCap};   // (+ b_tail_at)
  // 4 x 4 blocks: sixteen planes of (T / 4 + nb4 + 1) rows; a row holds T / 4 window starts,
  // nb4 block columns, up to two columns in front (b4_c0 is a multiple of 4) and the seven
  // bytes a shifted pair of dwords reads behind -- in an ODD number of 8-byte pieces (rows on
  // different banks), the planes two banks apart (neighbouring cells lie in different planes)
  const int nb4 = (nb + 1) / 2;
  g.b4_lpb = ((g.T >> 2) + nb4 + 9 + 7) & ~7;
  if ((g.b4_lpb & 15) == 0) g.b4_lpb += 8;
  g.b4_lh = (g.T >> 2) + nb4 + 1;
  g.b4_pstride = g.b4_lh * g.b4_lpb;
  g.b4_pstride += (8 - g.b4_pstride % 128 + 128) % 128;
  g.b4_tail_at = 16 * static_cast<size_t>(g.b4_pstride) + ((static_cast<size_t>(nb4) * g.b4_lpb + 16 + 15) & ~size_t{15}) +
                 8 * static_cast<size_t>(n_pad);
  // the tail kernel's box of the byte image: every window start of the box plus the 4 nb4
  // cells of the blocks, eight bytes for the shifted dword pair; an odd number of 8-byte pieces
  g.b8_lp = (g.T + 4 * nb4 + 8 + 7) & ~7;
  if ((g.b8_lp & 15) == 0) g.b8_lp += 8;
  g.b8_lh = g.T + 4 * nb4;
  g.t4_lds = BoundTail4Lds(g.b8_lp, g.b8_lh, n_pad, it.num_scans, nb4);
  // | rotations | block sums | discretisation constants (the tail kernel has LDS of its own)
  g.b4_lds = g.b4_tail_at + 8 * ((static_cast<size_t>(it.num_scans) + 1) & ~size_t{1}) +
             4 * ((static_cast<size_t>(it.num_scans) * nb4 * nb4 + 3) & ~size_t{3}) +
             kBoundDiscBytes * static_cast<size_t>(it.num_scans);
}

// ---- a match joins the launch: where its lists, headers, sums and rotation table start, the
// launch-wide maxima, the work items it may need.  False: its cloud is beyond the finish kernel.
inline bool Rt2DJoinLaunch(const Rt2DPlanMatch& it, const TileGeometry& g, int m, int target,
                           Rt2DMatchAt* at, Rt2DPlan* plan) {
  Rt2DPlan& I = *plan;
  const int side = 2 * it.nl + 1, n_pad = (it.n + 63) / 64 * 64;
  *at = Rt2DMatchAt{I.lists_total, I.hdr_total, I.qsum_total, I.tables_total, 0};
  I.tile_lds = std::max(I.tile_lds, g.lds);
  I.prep_lds = std::max<size_t>(I.prep_lds, 6 * static_cast<size_t>(n_pad) + 512);
  I.lists_total += Align16(2 * static_cast<size_t>(it.num_scans) * g.cap_s);
  I.hdr_total += static_cast<size_t>(it.num_scans) * g.ntx * g.nty * 4;
  I.qsum_total += static_cast<size_t>(it.num_scans) * side * side;
  I.tables_total += static_cast<size_t>(it.num_scans);
  // (an upper bound of the planner's items: a tile's groups are capped by gmax and by its share
  // of the entries, and the shares of a match's tiles add up to all its entries)
  I.work_cap += I.fused ? g.groups
                        : std::min<long long>(static_cast<long long>(g.ntx) * g.nty * g.gmax,
                                              static_cast<long long>(it.n) * it.num_scans / target +
                                                  static_cast<long long>(g.ntx) * g.nty * (g.gmin + 1));
  I.max_scans = std::max(I.max_scans, it.num_scans);
  const int stride = g.H * g.lp;
  I.common_stride = m == 0 ? stride : (I.common_stride == stride ? stride : 0);
  // finish kernel: cells + `group` probability rows + lists within 96 KB
  const size_t fin_fixed = 4 * static_cast<size_t>(n_pad) + 4 * ((static_cast<size_t>(it.num_scans) + 3) & ~size_t{3}) +
                           12 * static_cast<size_t>(kStage1Cap) + 64 + 128;
  const size_t row = 4 * (static_cast<size_t>(n_pad) + 4);
  const size_t budget = 96 * 1024;
  if (fin_fixed + row > budget) return false;
  I.group = std::min<int>(I.group, static_cast<int>((budget - fin_fixed) / row));
  I.finish_lds = std::max(I.finish_lds, fin_fixed);
  return true;
}

// ---- block bounds first (rt_2d_bounds.h): every match ONE work item of the bound kernel, two
// workgroups of 512 threads per CU where their LDS allows.  Not for windows beyond 16 x 16
// cells (the block columns of a row are one 8-byte read) -- the exhaustive tile kernel keeps
// those, and stays the parity partner behind the debug switch.
// From kBoundMinMatches matches per call on: below, the tile kernel's finer work items (a match
// in four or more, none of which waits for a last one) give the shorter call -- measured on C1,
// bounds / tiles: 1 match 62 / 52 us, 16: 92 / 74, 128: 114 - 126 / 117 (on 400 x 400 grids
// 139 - 161 / 106), 256: 144 / 168, 1024: 330 - 357 / 449 - 503 (profiles/r05_c1_bounds.txt).
// Debug switches: rt2d_bounds = 1 always, rt2d_no_bounds never.
inline void Rt2DDecideBounds(const Rt2DPlanMatch* in, int num, const Rt2DPlanCall& call, int launch_nb,
                             Rt2DPlan* plan) {
  Rt2DPlan& I = *plan;
  const Rt2DPlanSwitches& dbg = call.dbg;
  TileGeometry* geo = I.geo.data();
  I.bounds = I.fused && !dbg.rt2d_no_bounds && (call.batch_matches >= kBoundMinMatches || dbg.rt2d_bounds);
  // (round 6) the tail of a match -- phases B, C and the finish: ~30 us of dependent round trips
  // during which a workgroup's 70 KB of LDS and its place on the CU did nothing -- in a kernel of
  // its own behind the bound kernel (Rt2DBoundTailKernel: 33 KB, every match of the part in flight
  // at once).  rt2d_bounds_fused = 1: one kernel as in round 5 (the parity partner; verify mode).
  I.split = I.bounds && !dbg.rt2d_bounds_verify && !dbg.rt2d_bounds_fused;
  // (round 6) blocks of 4 x 4 translations first, their survivors refined by the tail kernel:
  // rt2d_bounds_level = 2 keeps the 2 x 2 blocks as the first level (the parity partner)
  I.level4 = I.bounds && !dbg.rt2d_bounds_fused && dbg.rt2d_bounds_level != 2;
  for (int m = 0; m < num && I.bounds; ++m) {
    const int side = 2 * in[m].nl + 1;
    // (the fused bound kernel finishes a match itself, in the LDS of its planes and cloud -- a
    // small box leaves less than the finish needs: the rest of the layout moves back)
    geo[m].b_tail_at = I.split ? geo[m].b_finish_room : std::max(geo[m].b_finish_room, Align16(I.finish_lds));
    I.tail_lds = std::max(I.tail_lds, BoundTailLds((in[m].n + 63) / 64 * 64, in[m].num_scans, launch_nb));
    geo[m].b_lds += geo[m].b_tail_at;
    I.bounds = side <= 2 * kBoundMaxBlocks && geo[m].b_lds <= 150 * size_t{1024};
    I.bound_nb = std::max(I.bound_nb, (side + 1) / 2);
    I.bound_lds = std::max(I.bound_lds, geo[m].b_lds);
    I.bound4_lds = std::max(I.bound4_lds, geo[m].b4_lds);
    I.tail4_lds = std::max(I.tail4_lds, geo[m].t4_lds);
  }
  I.level4 = I.level4 && I.bounds && I.bound4_lds <= 150 * size_t{1024};
  if (I.level4) { I.split = true; I.bound_lds = I.bound4_lds; }
  if (!I.bounds) return;
  // rotation groups per match: about two items per CU over the whole call (an item stages the
  // match's planes and cloud: ~4 us), one per match in large batches
  const int per_cu = I.bound_lds <= 78 * size_t{1024} ? 2 : 1;
  const int slots = std::max(1, per_cu * call.cus / call.share);
  // (block sums of matches bounded by several workgroups; read only where groups > 1)
  const int nb_level = I.level4 ? (I.bound_nb + 1) / 2 : I.bound_nb;
  I.work_cap = 0;
  for (int m = 0; m < num; ++m) {
    const int G = dbg.rt2d_groups > 0 ? dbg.rt2d_groups : slots / num;
    geo[m].groups = std::max(1, std::min(G, in[m].num_scans));
    I.work_cap += geo[m].groups;
    I.at[m].ub = static_cast<int>(I.ub_total);
    I.ub_total += static_cast<size_t>(in[m].num_scans) * nb_level * nb_level;
  }
}

// ---- the launch grid: persistent workgroups, one per slot or work item.
inline void Rt2DLaunchGrid(const Rt2DPlanCall& call, int tile_slots, Rt2DPlan* plan) {
  Rt2DPlan& I = *plan;
  I.tile_grid = static_cast<int>(std::max<long long>(1, std::min<long long>(tile_slots, I.work_cap)));
  if (I.bounds) {
    const int per_cu = I.bound_lds <= 78 * size_t{1024} ? 2 : 1;
    // (the whole chip even when the call is one part of a batch: the workgroups are persistent and
    // two of them share a CU -- a part whose grid is its share of the CUs leaves a wavefront per
    // SIMD short of hiding the LDS latency of phase A whenever the parts do not overlap)
    I.tile_grid = static_cast<int>(std::max<long long>(1, std::min<long long>(per_cu * call.cus, I.work_cap)));
  }
}

// The plan of one call.  False: a match is not eligible for the tile path (huge window, cloud or
// grid); *plan is then unspecified.
inline bool PlanRt2DTiles(const Rt2DPlanMatch* in, int num, const Rt2DPlanCall& call, Rt2DPlan* plan) {
  Rt2DPlan& I = *plan;
  I = Rt2DPlan{};
  I.geo.assign(num, TileGeometry{});
  I.at.assign(num, Rt2DMatchAt{});
  TileGeometry* geo = I.geo.data();
  if (!Rt2DBlockShapes(in, num, geo, &I.rpl)) return false;
  std::vector<Rt2DReach> reach(num);
  std::vector<Rt2DWindowClass> classes;
  I.entries_total = Rt2DReachBoxes(in, num, geo, reach.data(), &classes);
  bool single_tile = false, want_fused = false;
  if (!Rt2DChooseShape(&classes, I.rpl, call.dbg, &single_tile, &want_fused)) return false;
  I.tile_threads = single_tile ? 1024 : 512;
  I.fused = single_tile && want_fused;
  // Entries per work item: the whole batch in about two items per resident workgroup (an item
  // costs ~4 us before its first window update: ticket, headers, lists, tasks, image), not less
  // than two thousand entries (sixteen tasks: one per wavefront).
  int launch_nb = 1;                     // block bounds: blocks per window axis, launch-wide
  for (int m = 0; m < num; ++m) launch_nb = std::max(launch_nb, in[m].nl + 1);
  const int tile_slots = std::max(1, (single_tile ? call.cus : 2 * call.cus) / call.share);
  const int target = call.dbg.rt2d_target > 0
                         ? call.dbg.rt2d_target
                         : static_cast<int>(std::min<long long>(16384, std::max<long long>(2048, I.entries_total / (2ll * tile_slots))));
  for (int m = 0; m < num; ++m) {
    Rt2DMatchTiles(in[m], classes[reach[m].window_class].g, reach[m], target, I.fused, call.dbg, &geo[m]);
    Rt2DImageSizes(in[m], &geo[m]);
    Rt2DBoundShapes(in[m], launch_nb, &geo[m]);
    if (!Rt2DJoinLaunch(in[m], geo[m], m, target, &I.at[m], &I)) return false;
  }
  {
    size_t max_row = 0;
    for (int m = 0; m < num; ++m) max_row = std::max<size_t>(max_row, 4 * (static_cast<size_t>((in[m].n + 63) / 64 * 64) + 4));
    I.finish_lds += static_cast<size_t>(I.group) * max_row;
  }
  Rt2DDecideBounds(in, num, call, launch_nb, &I);
  Rt2DLaunchGrid(call, tile_slots, &I);
  return true;
}

// The upload block of a planned call (`params_bytes`: of one match's parameter block).
inline void StageRt2DTiles(const Rt2DPlanMatch* in, int num, const Rt2DPlan& plan, size_t params_bytes,
                           Rt2DStaging* staging) {
  Rt2DStaging& S = *staging;
  S.match.resize(num);
  size_t in_bytes = Align16(params_bytes * num);
  for (int m = 0; m < num; ++m) {
    const Rt2DPlanMatch& it = in[m];
    S.match[m].xyz = in_bytes;
    S.match[m].rot = S.match[m].xyz + (it.device_xyz ? 0 : Align16(3 * sizeof(float) * it.n));
    S.match[m].cells = S.match[m].rot + Align16(2 * sizeof(float) * it.num_scans);
    in_bytes = S.match[m].cells + (it.device_cells ? 0 : Align16(2 * static_cast<size_t>(it.num_x_cells) * it.num_y_cells));
  }
  S.counters = in_bytes;
  in_bytes += 64;
  S.tickets = in_bytes;
  if (plan.bounds) in_bytes += Align16(sizeof(int) * static_cast<size_t>(num));
  S.work = in_bytes;
  if (plan.fused) in_bytes += Align16(3 * 16 * static_cast<size_t>(plan.work_cap));   // (three int4 per item)
  S.misc = in_bytes;
  in_bytes += Align16(sizeof(unsigned) * 128 * static_cast<size_t>(num));
  S.bytes = in_bytes;
}

}  // namespace cmx

#endif  // CMX_RT_2D_PLAN_H_
