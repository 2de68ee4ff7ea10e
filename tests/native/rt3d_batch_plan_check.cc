// Host-side check of cartographer_amd/csrc/rt_3d_batch_plan.h: the windows, the routes and the
// launch sets of cmx_rt3d_match_grid_batch.  Built with the address and undefined-behaviour
// sanitizers and run by tests/test_rt3d_batch_plan.py; exit status 0 and "failures 0" when all
// holds.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "rt_3d_batch_plan.h"

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

using cmx::Rt3DBatchBounds;
using cmx::Rt3DBatchPlan;
using cmx::Rt3DMatchInput;

Rt3DMatchInput Input(int L, int A, int n, bool finite = true) {
  Rt3DMatchInput in;
  in.window.L = L;
  in.window.A = A;
  const long long st = 2 * L + 1, sr = 2 * A + 1;
  in.window.T = st * st * st;
  in.window.R = sr * sr * sr;
  in.window.num_candidates = in.window.T * in.window.R;
  in.num_points = n;
  in.finite = finite;
  return in;
}

// What every plan keeps, whatever the bounds: the segmented matches of a set own consecutive
// ranges of blocks in list order, strictly increasing first blocks, every block owned by the
// match a scan finds; a set passes a bound only when it is one match; the totals add up.
// Returns the blocks asked.
long long CheckPlan(const char* name, const std::vector<Rt3DMatchInput>& in, int route_switch,
                    const Rt3DBatchBounds& bounds) {
  const int num = static_cast<int>(in.size());
  const Rt3DBatchPlan plan = cmx::PlanRt3DBatch(in.data(), num, route_switch, bounds);
  CHECK(static_cast<int>(plan.matches.size()) == num, "%s", name);
  long long asked = 0;
  int segmented = 0;
  std::vector<int> singles;
  for (int k = 0; k < num; ++k) {
    const auto& P = plan.matches[k];
    const int route = cmx::Rt3DRouteOf(in[k], route_switch, bounds.max_work);
    CHECK(P.route == route, "%s: match %d route %d", name, k, P.route);
    if (route == cmx::kRt3DRouteSingle) {
      singles.push_back(k);
      CHECK(P.set == -1 && P.slot == -1 && P.blocks == 0, "%s: single match %d", name, k);
    } else {
      ++segmented;
      CHECK(P.set >= 0 && P.set < static_cast<int>(plan.sets.size()), "%s: match %d set %d", name,
            k, P.set);
      CHECK(P.blocks == in[k].window.R * ((in[k].window.T + 63) / 64) && P.blocks >= 1,
            "%s: match %d blocks %d", name, k, P.blocks);
    }
  }
  CHECK(plan.singles == singles, "%s: singles", name);
  CHECK(static_cast<int>(plan.match_of_slot.size()) == segmented, "%s: slots", name);
  int next_slot = 0, last_match = -1;
  for (size_t s = 0; s < plan.sets.size(); ++s) {
    const cmx::LaunchSet& set = plan.sets[s];
    CHECK(set.begin == next_slot && set.end > set.begin, "%s: set %zu [%d, %d)", name, s,
          set.begin, set.end);
    next_slot = set.end;
    long long blocks = 0, candidates = 0, staged = 0;
    std::vector<int> first;
    for (int slot = set.begin; slot < set.end; ++slot) {
      const int k = plan.match_of_slot[slot];
      const auto& P = plan.matches[k];
      CHECK(k > last_match, "%s: list order", name);
      last_match = k;
      CHECK(P.slot == slot && P.set == static_cast<int>(s), "%s: match %d slot", name, k);
      CHECK(P.first_block == blocks, "%s: match %d first block %d, %lld before it", name, k,
            P.first_block, blocks);
      CHECK(slot == set.begin || P.first_block > plan.matches[plan.match_of_slot[slot - 1]].first_block,
            "%s: first blocks not strictly increasing", name);
      first.push_back(P.first_block);
      blocks += P.blocks;
      candidates += in[k].window.num_candidates;
      staged += cmx::Rt3DBatchStagedBytes(in[k].window, in[k].num_points);
    }
    first.push_back(static_cast<int>(blocks));
    CHECK(blocks == set.total[0] && candidates == set.total[1] && staged == set.total[2],
          "%s: set %zu totals", name, s);
    const bool alone = set.end - set.begin == 1;
    CHECK(alone || (blocks <= bounds.blocks && candidates <= bounds.candidates &&
                    staged <= bounds.staged_bytes),
          "%s: set %zu passes a bound with %d matches", name, s, set.end - set.begin);
    // every block (of small sets), or the edges of every match's range, against a scan
    const int n_set = set.end - set.begin;
    const auto ask = [&](long long block, int owner) {
      const int found = cmx::EntryOfBlock(first.data(), n_set, static_cast<int>(block));
      CHECK(found == owner, "%s: set %zu block %lld: %d, scan %d", name, s, block, found, owner);
      ++asked;
    };
    for (int e = 0; e < n_set; ++e) {
      if (blocks <= 20000) {
        for (long long b = first[e]; b < first[e + 1]; ++b) ask(b, e);
      } else {
        ask(first[e], e);
        ask(first[e + 1] - 1, e);
      }
    }
  }
  CHECK(next_slot == segmented, "%s: %d slots in sets, %d segmented matches", name, next_slot,
        segmented);
  return asked;
}

int SetsOf(const std::vector<Rt3DMatchInput>& in, const Rt3DBatchBounds& bounds) {
  return static_cast<int>(
      cmx::PlanRt3DBatch(in.data(), static_cast<int>(in.size()), 1, bounds).sets.size());
}

}  // namespace

int main() {
  long long asked = 0;
  // Random lists: windows from a single candidate up, one-block matches among them, clouds of a
  // point up, a non-finite cloud now and then; default bounds and tight ones.
  std::mt19937 rng(12345);
  for (int round = 0; round < 300; ++round) {
    const int num = 1 + static_cast<int>(rng() % 24);
    std::vector<Rt3DMatchInput> in;
    for (int k = 0; k < num; ++k) {
      const int L = static_cast<int>(rng() % 4), A = static_cast<int>(rng() % 4);
      in.push_back(Input(rng() % 3 == 0 ? 0 : L, rng() % 3 == 0 ? 0 : A,
                         1 + static_cast<int>(rng() % 700), rng() % 11 != 0));
    }
    Rt3DBatchBounds bounds;
    if (round % 3 == 1) bounds.blocks = 1 + rng() % 2000;
    if (round % 3 == 2) bounds.candidates = 1 + rng() % 100000;
    if (round % 5 == 4) bounds.staged_bytes = 600 + rng() % 40000;
    if (round % 7 == 6) bounds.max_work = 1 + rng() % 5000000;
    asked += CheckPlan("random", in, round % 4 == 3 ? 1 : round % 9 == 8 ? 2 : 0, bounds);
  }
  // One-block matches only (a single candidate each): block b belongs to match b.
  {
    std::vector<Rt3DMatchInput> in(40, Input(0, 0, 5));
    asked += CheckPlan("one-block", in, 0, Rt3DBatchBounds());
    const Rt3DBatchPlan plan = cmx::PlanRt3DBatch(in.data(), 40, 0);
    for (int k = 0; k < 40; ++k)
      CHECK(plan.matches[k].first_block == k && plan.matches[k].blocks == 1, "one-block %d", k);
  }
  // A set is cut at each of the three bounds: three matches of the lua window (L 1, A 3: 343
  // blocks, 9 261 candidates, 512 + 6860 + 432 + 3600 staged bytes at 300 points).
  {
    const std::vector<Rt3DMatchInput> in(3, Input(1, 3, 300));
    const long long staged = cmx::Rt3DBatchStagedBytes(in[0].window, 300);
    CHECK(staged == 512 + 20 * 343 + 16 * 27 + 3600, "staged bytes %lld", staged);
    CHECK(SetsOf(in, Rt3DBatchBounds()) == 1, "default bounds");
    Rt3DBatchBounds b;
    b.blocks = 2 * 343;
    CHECK(SetsOf(in, b) == 2, "cut at the blocks");
    b.blocks = 2 * 343 - 1;
    CHECK(SetsOf(in, b) == 3, "cut at the blocks, one fewer");
    b = Rt3DBatchBounds();
    b.candidates = 2 * 9261;
    CHECK(SetsOf(in, b) == 2, "cut at the candidates");
    b.candidates = 2 * 9261 - 1;
    CHECK(SetsOf(in, b) == 3, "cut at the candidates, one fewer");
    b = Rt3DBatchBounds();
    b.staged_bytes = 2 * staged;
    CHECK(SetsOf(in, b) == 2, "cut at the staged bytes");
    b.staged_bytes = 2 * staged - 1;
    CHECK(SetsOf(in, b) == 3, "cut at the staged bytes, one fewer");
    for (long long* bound : {&b.blocks, &b.candidates, &b.staged_bytes}) {
      b = Rt3DBatchBounds();
      *bound = 1;                                        // every match exceeds it alone
      asked += CheckPlan("alone", in, 1, b);
      CHECK(SetsOf(in, b) == 3, "a match that exceeds a bound alone is a set of its own");
    }
  }
  // The largest supported window forced onto the segmented route: blocks below 2^31, a set of its
  // own behind a small match.
  {
    std::vector<Rt3DMatchInput> in = {Input(1, 1, 10), Input(200, 1, 10), Input(1, 1, 10)};
    CHECK(in[1].window.num_candidates < (1ll << 31), "window");
    asked += CheckPlan("large", in, 1, Rt3DBatchBounds());
    CHECK(SetsOf(in, Rt3DBatchBounds()) == 3, "large match alone");
  }
  // The window formulas at their limits.
  {
    cmx_rt_options o{0.15, 0.017453292519943295, 1e-1, 1e-1};
    cmx::Rt3DWindow W = cmx::Rt3DWindowOf(o, 0.1f, 15.f);
    CHECK(W.L == 1 && W.A == 3 && W.T == 27 && W.R == 343 && !W.unsupported, "lua %d %d", W.L, W.A);
    o.linear_search_window = 51.1;
    W = cmx::Rt3DWindowOf(o, 0.1f, 15.f);
    CHECK(W.L == 511 && W.unsupported != nullptr, "2^31 candidates: L %d", W.L);   // 1023^3 x 343
    o.linear_search_window = 51.2;
    CHECK(cmx::Rt3DWindowOf(o, 0.1f, 15.f).unsupported != nullptr, "L 512");
    const float points[6] = {3.f, 4.f, 0.f, 0.f, 0.f, 12.f};
    CHECK(cmx::Rt3DScanRange(0.1f, points, 2) == 12.f, "scan range");
    CHECK(cmx::Rt3DScanRange(5.f, points, 2) == 15.f, "scan range floor");
  }
  printf("blocks asked %lld\nfailures %d\n", asked, failures);
  return failures == 0 ? 0 : 1;
}
