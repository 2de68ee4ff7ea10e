// Host-side check of cartographer_amd/csrc/rt_2d_plan.h: the plan and the staging layout of a
// real-time 2D tile-matcher call.  Every output field of a fixed case list is compared with
// tests/golden/rt2d_plan_parent.json -- recorded from the statements of Rt2DTileCall::Plan() and
// Enqueue() as they stood before the header existed -- and every eligible case must keep what the
// record cannot be wrong about: LDS within the launches' budgets, conflict-free pitches, disjoint
// aligned staging regions.  Built with the address and undefined-behaviour sanitizers and run by
// tests/test_rt2d_plan.py: rt2d_plan_check <golden file>; exit status 0 and "failures 0" when all
// holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rt_2d_plan.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (++failures <= 20) {                             \
        printf("%s:%d: %s: ", __FILE__, __LINE__, #cond); \
        printf(__VA_ARGS__);                              \
        printf("\n");                                     \
      }                                                   \
    }                                                     \
  } while (0)

using cmx::Rt2DPlan;
using cmx::Rt2DPlanCall;
using cmx::Rt2DPlanMatch;
using cmx::Rt2DStaging;
using cmx::TileGeometry;

constexpr size_t kParamsBytes = 480;   // of a match's parameter block (any multiple of 4 serves)
constexpr int kFullRecord = 8;         // matches up to which a case records every per-match field

struct Case {
  std::string name;
  std::vector<Rt2DPlanMatch> in;
  Rt2DPlanCall call;
};

// A match of `n` points within `range` metres on an nx x ny grid whose centre is the origin.
Rt2DPlanMatch Match(int n, int nx, int ny, double res, int nl, int scans, double range, double x = 0,
                    double y = 0, bool resident = true) {
  Rt2DPlanMatch m{};
  m.n = n; m.num_x_cells = nx; m.num_y_cells = ny;
  m.resolution = res; m.max_x = 0.5 * ny * res; m.max_y = 0.5 * nx * res;
  m.x = x; m.y = y;
  m.nl = nl; m.num_scans = scans; m.max_range = static_cast<float>(range);
  m.device_xyz = m.device_cells = resident;
  return m;
}
Rt2DPlanMatch C1() { return Match(1000, 200, 200, 0.05, 6, 27, 4.9); }

std::vector<Case> Cases() {
  std::vector<Case> cases;
  const auto add = [&](const std::string& name, std::vector<Rt2DPlanMatch> in) -> Case& {
    cases.push_back(Case{name, std::move(in), Rt2DPlanCall{}});
    cases.back().call.batch_matches = static_cast<int>(cases.back().in.size());
    return cases.back();
  };
  // windows: side 1, 3, 5 (B = 2), 7, 9 (B = 3), 13 (C1), 15, 17 (B = 5), 23; rows per lane 5 and 7
  // (instantiated as 6 and 8); B > 32
  for (int nl : {0, 1, 2, 3, 4, 6, 7, 8, 11, 10, 13, 63}) {
    add("window_nl" + std::to_string(nl), {Match(500, 200, 200, 0.05, nl, 21, 4.0), Match(61, 200, 200, 0.05, nl, 9, 2.5)});
    add("window_bounds_nl" + std::to_string(nl), {Match(500, 200, 200, 0.05, nl, 21, 4.0)}).call.dbg.rt2d_bounds = 1;
  }
  // clouds: 1 .. 2048 fused, 2049 .. 8192 through the prep kernel, 8193 not at all
  for (int n : {1, 61, 64, 65, 1000, 2048, 2049, 8192, 8193})
    add("cloud_" + std::to_string(n), {Match(n, 200, 200, 0.05, 6, 27, 4.9), Match(n, 97, 83, 0.05, 6, 31, 1.9, 0.3, -0.2, false)});
  add("cloud_8192_bounds", {Match(8192, 200, 200, 0.05, 6, 27, 4.9)}).call.dbg.rt2d_bounds = 1;
  // grids: small, odd, C1's, too wide; poses near corners (the reach box clamps)
  add("grid_64", {Match(300, 64, 64, 0.05, 6, 27, 1.5), Match(300, 64, 64, 0.05, 6, 27, 4.9)});
  add("grid_97x83", {Match(300, 97, 83, 0.05, 6, 27, 1.9), Match(300, 83, 97, 0.10, 3, 15, 3.0, 0.4, 0.4, false)});
  add("grid_200", {C1(), C1(), C1()});
  add("grid_32001", {Match(300, 32001, 64, 0.05, 6, 27, 1.5)});
  add("grid_32001_y", {Match(300, 64, 32001, 0.05, 6, 27, 1.5)});
  add("grid_corners", {Match(1000, 200, 200, 0.05, 6, 27, 4.9, 4.9, 4.9), Match(1000, 200, 200, 0.05, 6, 27, 4.9, -4.95, 4.8),
                       Match(1000, 200, 200, 0.05, 6, 27, 4.9, -7.0, -7.0), Match(1000, 200, 200, 0.05, 6, 27, 4.9, 0.0, -4.99)});
  add("scans_4097", {Match(300, 200, 200, 0.05, 6, 4097, 4.9)});
  // two window classes in one batch, with and without the block bounds
  add("two_classes", {C1(), Match(1000, 200, 200, 0.05, 3, 27, 4.9), C1(), Match(640, 200, 200, 0.05, 3, 13, 3.0)});
  add("two_classes_bounds", {C1(), Match(1000, 200, 200, 0.05, 3, 27, 4.9)}).call.dbg.rt2d_bounds = 1;
  add("two_classes_wide_bounds", {C1(), Match(1000, 200, 200, 0.05, 8, 27, 4.9)}).call.dbg.rt2d_bounds = 1;
  // a long-range scan whose box needs several tiles
  add("long_range", {Match(1000, 600, 600, 0.05, 6, 19, 12.0), Match(1500, 600, 600, 0.05, 6, 21, 9.0, 3.0, -2.0, false)});
  add("long_range_fine", {Match(1000, 1000, 1000, 0.02, 6, 19, 5.0)});
  add("long_range_too_far", {Match(1000, 2000, 2000, 0.05, 6, 105, 40.0)});
  // the re-plan: a class that fits one tile with more than the two-per-CU budget next to a class
  // that needs several tiles
  // (the shapes of test_rt2d_replanned_window_class_next_to_a_several_tile_class: resident grids,
  // clouds from the host)
  {
    Case& c = add("replan", {Match(1000, 200, 200, 0.06, 5, 7, 4.9), Match(1000, 600, 600, 0.05, 6, 19, 12.0)});
    c.in[0].device_xyz = c.in[1].device_xyz = false;
  }
  add("replan_reversed", {Match(1000, 600, 600, 0.05, 6, 19, 12.0), Match(1000, 200, 200, 0.06, 5, 7, 4.9, 1.0, 1.0, false)});
  // batch sizes around kBoundMinMatches, shares of the device
  for (int num : {95, 96, 208})
    for (int share : {1, 2, 3}) {
      std::vector<Rt2DPlanMatch> in;
      for (int m = 0; m < num; ++m)
        in.push_back(Match(1000 - (m % 7), 200, 200, 0.05, 6, 27 - 2 * (m % 3), 4.9 - 0.01 * (m % 11), 0.02 * (m % 13), -0.03 * (m % 5), m % 4 != 0));
      add("batch_" + std::to_string(num) + "_share" + std::to_string(share), in).call.share = share;
    }
  {
    Case& c = add("part_of_batch", {C1(), C1(), C1(), C1()});   // a part of 4 of a batch of 1024
    c.call.batch_matches = 1024; c.call.share = 4;
  }
  // the debug switches
  add("switch_tile_64", {C1(), C1()}).call.dbg.rt2d_tile = 64;
  {
    Case& c = add("switch_tile_56_groups_target", {C1(), Match(3000, 200, 200, 0.05, 6, 27, 4.9)});
    c.call.dbg.rt2d_tile = 56; c.call.dbg.rt2d_groups = 1000; c.call.dbg.rt2d_target = 1;
  }
  add("switch_unfused", {C1(), C1()}).call.dbg.rt2d_unfused = 1;
  {
    Case& c = add("switch_no_bounds", {C1(), C1()});
    c.call.batch_matches = 512; c.call.dbg.rt2d_no_bounds = 1;
  }
  add("switch_bounds", {C1(), C1()}).call.dbg.rt2d_bounds = 1;
  {
    Case& c = add("switch_bounds_groups", {C1(), C1()});
    c.call.dbg.rt2d_bounds = 1; c.call.dbg.rt2d_groups = 5;
  }
  {
    Case& c = add("switch_bounds_fused", {C1(), Match(200, 64, 64, 0.05, 6, 27, 1.0)});
    c.call.dbg.rt2d_bounds = 1; c.call.dbg.rt2d_bounds_fused = 1;
  }
  {
    Case& c = add("switch_bounds_level_2", {C1(), C1()});
    c.call.dbg.rt2d_bounds = 1; c.call.dbg.rt2d_bounds_level = 2;
  }
  {
    Case& c = add("switch_bounds_verify", {C1(), C1()});
    c.call.dbg.rt2d_bounds = 1; c.call.dbg.rt2d_bounds_verify = 1;
  }
  {
    Case& c = add("switch_bounds_verify_level_2", {C1(), C1()});
    c.call.dbg.rt2d_bounds = 1; c.call.dbg.rt2d_bounds_verify = 1; c.call.dbg.rt2d_bounds_level = 2;
  }
  add("switch_lds_64", {C1(), Match(1000, 600, 600, 0.05, 6, 19, 9.0)}).call.dbg.rt2d_lds_kb = 64;
  return cases;
}

// ---- the record of a case: a sequence of keys and values, in the order of the golden file -------
#define RT2D_GEO_FIELDS(X)                                                                              \
  X(B) X(H) X(hl) X(ht) X(gpitch) X(grows) X(box_x0) X(box_y0) X(T) X(ntx) X(nty) X(lp) X(th_img)       \
  X(tile_image_bytes) X(cap_s) X(gmin) X(gmax) X(target) X(rw) X(list_lds) X(task_cap) X(groups) X(lds) \
  X(image_bytes) X(q_bytes) X(m2_pitch) X(m2_rows) X(b_lpb) X(b_lh) X(b_lds) X(b_finish_room)           \
  X(b_tail_at) X(m4_pitch) X(m4_rows) X(q8_bytes) X(b8_lp) X(b8_lh) X(t4_lds) X(b4_lpb) X(b4_lh)        \
  X(b4_pstride) X(b4_tail_at) X(b4_lds)
#define RT2D_LAUNCH_FIELDS(X)                                                                          \
  X(rpl) X(max_scans) X(common_stride) X(group) X(tile_lds) X(prep_lds) X(finish_lds) X(tail_lds)      \
  X(bound_lds) X(bound4_lds) X(tail4_lds) X(bound_nb) X(lists_total) X(hdr_total) X(qsum_total)        \
  X(ub_total) X(tables_total) X(work_cap) X(entries_total) X(tile_grid) X(tile_threads) X(fused)       \
  X(bounds) X(split) X(level4)

using Tokens = std::vector<std::string>;
void Key(Tokens* t, const char* key) { t->push_back(key); }
template <typename V>
void Value(Tokens* t, V v) { t->push_back(std::to_string(static_cast<long long>(v))); }

void MatchFields(const Rt2DPlan& plan, const Rt2DStaging& staging, int m, std::vector<long long>* out) {
  const TileGeometry& g = plan.geo[m];
#define X(f) out->push_back(static_cast<long long>(g.f));
  RT2D_GEO_FIELDS(X)
#undef X
  const cmx::Rt2DMatchAt& at = plan.at[m];
  for (size_t v : {at.lists, at.hdr, at.qsum, at.table, static_cast<size_t>(at.ub)}) out->push_back(static_cast<long long>(v));
  const cmx::Rt2DStagingAt& s = staging.match[m];
  for (size_t v : {s.xyz, s.rot, s.cells}) out->push_back(static_cast<long long>(v));
}

Tokens Record(const Case& c, bool eligible, const Rt2DPlan& plan, const Rt2DStaging& staging) {
  Tokens t;
  Key(&t, "name"); t.push_back(c.name);
  Key(&t, "eligible"); Value(&t, eligible);
  if (!eligible) return t;
  Key(&t, "launch");
#define X(f) Key(&t, #f); Value(&t, plan.f);
  RT2D_LAUNCH_FIELDS(X)
#undef X
  Key(&t, "staging");
  Key(&t, "counters"); Value(&t, staging.counters);
  Key(&t, "tickets"); Value(&t, staging.tickets);
  Key(&t, "work"); Value(&t, staging.work);
  Key(&t, "misc"); Value(&t, staging.misc);
  Key(&t, "bytes"); Value(&t, staging.bytes);
  const int num = static_cast<int>(c.in.size());
  std::vector<long long> fields;
  if (num <= kFullRecord) {
    Key(&t, "matches");     // per match: the geometry, then lists, hdr, qsum, table, ub, then xyz, rot, cells
    for (int m = 0; m < num; ++m) {
      fields.clear();
      MatchFields(plan, staging, m, &fields);
      for (long long v : fields) Value(&t, v);
    }
  } else {
    for (int m = 0; m < num; ++m) MatchFields(plan, staging, m, &fields);
    uint64_t h = 0xcbf29ce484222325ull;                    // FNV-1a over the values' eight bytes
    for (long long v : fields)
      for (int b = 0; b < 8; ++b) h = (h ^ ((static_cast<uint64_t>(v) >> (8 * b)) & 0xff)) * 0x100000001b3ull;
    char hex[32];
    snprintf(hex, sizeof(hex), "%016llx", static_cast<unsigned long long>(h));
    Key(&t, "matches_hash"); t.push_back(hex);
  }
  return t;
}

// The strings and numbers of a JSON text in order (its punctuation says nothing the order does not).
Tokens Tokenize(const std::string& text) {
  Tokens t;
  for (size_t i = 0; i < text.size();) {
    const char ch = text[i];
    if (ch == '"') {
      const size_t end = text.find('"', i + 1);
      if (end == std::string::npos) break;
      t.push_back(text.substr(i + 1, end - i - 1));
      i = end + 1;
    } else if (ch == '-' || (ch >= '0' && ch <= '9')) {
      size_t end = i + 1;
      while (end < text.size() && text[end] >= '0' && text[end] <= '9') ++end;
      t.push_back(text.substr(i, end - i));
      i = end;
    } else {
      ++i;
    }
  }
  return t;
}

// ---- what every eligible plan keeps ---------------------------------------------------------------
void CheckInvariants(const Case& c, const Rt2DPlan& plan, const Rt2DStaging& staging) {
  const char* name = c.name.c_str();
  const int num = static_cast<int>(c.in.size());
  const size_t kib = 1024;
  // the budgets the launches opt in to (static LDS taken off), and the planner's own
  CHECK(plan.tile_lds <= 160 * kib - 1024, "%s: tile kernel %zu", name, plan.tile_lds);
  const size_t two_per_cu = (c.call.dbg.rt2d_lds_kb > 0 ? c.call.dbg.rt2d_lds_kb : 76) * kib;
  CHECK(plan.tile_lds <= (plan.tile_threads == 1024 ? 150 * kib : two_per_cu), "%s: tile kernel %zu of %d threads", name,
        plan.tile_lds, plan.tile_threads);
  CHECK(plan.tile_threads == 1024 || plan.tile_threads == 512, "%s", name);
  if (!plan.fused) CHECK(plan.prep_lds <= 64 * kib, "%s: prep kernel %zu", name, plan.prep_lds);
  if (plan.bounds) CHECK(plan.bound_lds <= 160 * kib - 4096, "%s: bound kernel %zu", name, plan.bound_lds);
  if (plan.bounds && plan.split)
    CHECK((plan.level4 ? plan.tail4_lds : plan.tail_lds) <= 160 * kib - 4096, "%s: tail kernel %zu", name,
          plan.level4 ? plan.tail4_lds : plan.tail_lds);
  if (!plan.bounds || c.call.dbg.rt2d_bounds_verify)
    CHECK(plan.finish_lds <= 128 * kib, "%s: finish kernel %zu", name, plan.finish_lds);
  CHECK(plan.group >= 1, "%s: group %d", name, plan.group);
  CHECK(plan.work_cap >= 1 && plan.work_cap < (1ll << 24), "%s: work_cap %lld", name, plan.work_cap);
  CHECK(plan.tile_grid >= 1 && plan.tile_grid <= 2 * c.call.cus, "%s: grid %d", name, plan.tile_grid);
  CHECK(!plan.level4 || plan.split, "%s", name);
  CHECK(!plan.bounds || plan.fused, "%s", name);
  size_t lists = 0, hdr = 0, qsum = 0, table = 0;
  for (int m = 0; m < num; ++m) {
    const TileGeometry& g = plan.geo[m];
    CHECK(g.list_lds % 8 == 0 && g.list_lds > 0, "%s: match %d list_lds %d", name, m, g.list_lds);
    CHECK(g.lp % 16 == 0 && g.lp >= 2 * (g.T + 4 * g.B) && cmx::ConflictFreePitch(g.H, g.B, g.lp) == g.lp,
          "%s: match %d pitch %d for H %d, B %d", name, m, g.lp, g.H, g.B);
    CHECK(g.T % 8 == 0 && g.ntx >= 1 && g.nty >= 1 && g.ntx * g.nty <= cmx::kMaxTiles, "%s: match %d tiles", name, m);
    CHECK(!plan.fused || g.ntx * g.nty == 1, "%s: match %d fused with %d tiles", name, m, g.ntx * g.nty);
    CHECK(g.lds <= plan.tile_lds, "%s: match %d", name, m);
    CHECK(g.rw * g.gmin >= c.in[m].num_scans && g.rw <= 64, "%s: match %d rw %d gmin %d", name, m, g.rw, g.gmin);
    if (plan.bounds) CHECK(g.b_lds <= plan.bound_lds || plan.level4, "%s: match %d", name, m);
    if (plan.level4) CHECK(g.b4_lds <= plan.bound_lds && g.b4_pstride % 128 == 8, "%s: match %d", name, m);
    // the scratch regions of the matches follow one another
    const cmx::Rt2DMatchAt& at = plan.at[m];
    CHECK(at.lists == lists && at.hdr == hdr && at.qsum == qsum && at.table == table, "%s: match %d offsets", name, m);
    CHECK(at.lists % 16 == 0, "%s: match %d", name, m);
    lists += cmx::Align16(2 * static_cast<size_t>(c.in[m].num_scans) * g.cap_s);
    hdr += static_cast<size_t>(c.in[m].num_scans) * g.ntx * g.nty * 4;
    qsum += static_cast<size_t>(c.in[m].num_scans) * (2 * c.in[m].nl + 1) * (2 * c.in[m].nl + 1);
    table += c.in[m].num_scans;
  }
  CHECK(lists == plan.lists_total && hdr == plan.hdr_total && qsum == plan.qsum_total && table == plan.tables_total,
        "%s: totals", name);
  // the upload block: ascending, 16-byte aligned, disjoint
  size_t at = kParamsBytes * num;
  const auto region = [&](size_t begin, size_t bytes, const char* what) {
    CHECK(begin % 16 == 0 && begin >= at, "%s: %s at %zu, free from %zu", name, what, begin, at);
    at = begin + bytes;
  };
  for (int m = 0; m < num; ++m) {
    const Rt2DPlanMatch& in = c.in[m];
    region(staging.match[m].xyz, in.device_xyz ? 0 : 12 * static_cast<size_t>(in.n), "xyz");
    region(staging.match[m].rot, 8 * static_cast<size_t>(in.num_scans), "rot");
    region(staging.match[m].cells, in.device_cells ? 0 : 2 * static_cast<size_t>(in.num_x_cells) * in.num_y_cells, "cells");
  }
  region(staging.counters, 64, "counters");
  region(staging.tickets, plan.bounds ? 4 * static_cast<size_t>(num) : 0, "tickets");
  region(staging.work, plan.fused ? 48 * static_cast<size_t>(plan.work_cap) : 0, "work");
  region(staging.misc, 512 * static_cast<size_t>(num), "misc");
  region(staging.bytes, 0, "end");
}

bool Run(const Case& c, Rt2DPlan* plan, Rt2DStaging* staging) {
  const int num = static_cast<int>(c.in.size());
  if (!cmx::PlanRt2DTiles(c.in.data(), num, c.call, plan)) return false;
  cmx::StageRt2DTiles(c.in.data(), num, *plan, kParamsBytes, staging);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s tests/golden/rt2d_plan_parent.json\n", argv[0]);
    return 2;
  }
  std::string text;
  if (FILE* f = fopen(argv[1], "rb")) {
    char buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, got);
    fclose(f);
  }
  // the golden file's cases: each starts at its "name" key
  const Tokens golden = Tokenize(text);
  std::vector<Tokens> recorded;
  for (const std::string& tok : golden) {
    if (tok == "name") recorded.emplace_back();
    if (!recorded.empty()) recorded.back().push_back(tok);
  }
  const std::vector<Case> cases = Cases();
  CHECK(recorded.size() == cases.size(), "the golden file holds %zu cases, the list %zu", recorded.size(), cases.size());
  long long fields = 0;
  int eligible_cases = 0;
  for (size_t k = 0; k < cases.size() && k < recorded.size(); ++k) {
    const Case& c = cases[k];
    Rt2DPlan plan;
    Rt2DStaging staging;
    const bool eligible = Run(c, &plan, &staging);
    if (eligible) {
      ++eligible_cases;
      CheckInvariants(c, plan, staging);
    }
    const Tokens mine = Record(c, eligible, plan, staging);
    const Tokens& theirs = recorded[k];
    CHECK(mine.size() == theirs.size(), "%s: %zu values, recorded %zu", c.name.c_str(), mine.size(), theirs.size());
    std::string key;
    for (size_t i = 0; i < mine.size() && i < theirs.size(); ++i) {
      const bool is_value = !mine[i].empty() && (mine[i][0] == '-' || (mine[i][0] >= '0' && mine[i][0] <= '9'));
      if (!is_value) key = mine[i];
      else ++fields;
      CHECK(mine[i] == theirs[i], "%s: %s (value %zu): %s, recorded %s", c.name.c_str(), key.c_str(), i, mine[i].c_str(),
            theirs[i].c_str());
    }
  }
  printf("cases %zu (eligible %d), fields compared %lld, failures %d\n", cases.size(), eligible_cases, fields, failures);
  return failures == 0 ? 0 : 1;
}
