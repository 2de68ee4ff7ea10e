// Host-side check of cartographer_amd/csrc/cmx_batch.h: the bisection a block finds its entry
// with, the cutting of a call's items into sets of launches, the staging of host arrays by
// pointer and the layout of an upload block.  Built with the address and undefined-behaviour
// sanitizers and run by tests/test_batch_plan.py; exit status 0 and "failures 0" when all holds.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "cmx_batch.h"

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

// Every table of 1 to 6 entries with 0 to 3 blocks each, every block of it, against a scan.
int CheckBisection() {
  struct Desc { int pad, first; };
  int tables = 0;
  for (int num = 1; num <= 6; ++num) {
    int codes = 1;
    for (int e = 0; e < num; ++e) codes *= 4;
    for (int code = 0; code < codes; ++code) {
      std::vector<int> first(num + 1, 0);
      std::vector<Desc> descs(num);
      for (int e = 0, c = code; e < num; ++e, c /= 4) {
        descs[e] = Desc{-1, first[e]};
        first[e + 1] = first[e] + c % 4;
      }
      if (first[num] == 0) continue;                   // no block, nothing to ask
      ++tables;
      for (int block = 0; block < first[num]; ++block) {
        int owner = 0;                                 // the entry with first <= block < next first
        while (!(first[owner] <= block && block < first[owner + 1])) ++owner;
        const int by_table = cmx::EntryOfBlock(first.data(), num, block);
        const int by_member = cmx::DescOfBlock<&Desc::first>(descs.data(), num, block);
        const int by_callable =
            cmx::OwnerOfBlock([&](int i) { return first[i]; }, num, block);
        CHECK(by_table == owner && by_member == owner && by_callable == owner,
              "num %d code %d block %d: %d %d %d, scan %d", num, code, block, by_table, by_member,
              by_callable, owner);
      }
    }
  }
  CHECK(tables == 5460 - 6, "%d tables", tables);      // 4 + .. + 4^6, less the six empty ones
  return tables;
}

// One list of items cut with `most` and `bound`; blocks[k][a] = blocks of item k in launch a.
void CheckCut(const char* name, const std::vector<int>& target,
              const std::vector<std::vector<long long>>& blocks, int most, long long bound) {
  const int num = static_cast<int>(target.size());
  cmx::TargetRounds<int> order;
  for (int t : target) order.Add(t);
  // Rounds and first-seen indices against their definition.
  std::vector<int> seen;
  for (int k = 0; k < num; ++k) {
    int earlier = 0, index = -1;
    for (int j = 0; j < k; ++j) earlier += target[j] == target[k];
    for (size_t s = 0; s < seen.size(); ++s)
      if (seen[s] == target[k]) index = static_cast<int>(s);
    if (index < 0) {
      index = static_cast<int>(seen.size());
      seen.push_back(target[k]);
    }
    CHECK(order.round_of[k] == earlier, "%s: item %d in round %d", name, k, order.round_of[k]);
    CHECK(order.target_of[k] == index, "%s: item %d target %d", name, k, order.target_of[k]);
  }
  CHECK(order.targets == seen, "%s: targets", name);

  std::vector<int> slot_of(num, -1), item_at(num, -1);
  std::vector<std::vector<long long>> first_of(num, std::vector<long long>(3, -1));
  int next_slot = 0;
  const std::vector<cmx::LaunchSet> sets = cmx::CutSets(
      order.round_of, most, {bound, bound, bound},
      [&](int k, long long* add) {
        for (int a = 0; a < 3; ++a) add[a] = blocks[k][a];
      },
      [&](int k, int slot, const long long* first) {
        CHECK(slot == next_slot, "%s: slot %d follows %d", name, slot, next_slot - 1);
        ++next_slot;
        CHECK(slot_of[k] == -1, "%s: item %d placed twice", name, k);
        slot_of[k] = slot;
        if (slot >= 0 && slot < num) item_at[slot] = k;
        for (int a = 0; a < 3; ++a) first_of[k][a] = first[a];
      });
  for (int k = 0; k < num; ++k) CHECK(slot_of[k] >= 0, "%s: item %d in no set", name, k);
  int expected_begin = 0;
  for (const cmx::LaunchSet& set : sets) {
    CHECK(set.begin == expected_begin && set.end > set.begin && set.end <= num,
          "%s: set [%d, %d)", name, set.begin, set.end);
    expected_begin = set.end;
    CHECK(set.end - set.begin <= most, "%s: set of %d items", name, set.end - set.begin);
    std::set<int> targets_of_set;
    long long sum[3] = {0, 0, 0};
    for (int slot = set.begin; slot < set.end && slot < num; ++slot) {
      const int k = item_at[slot];
      if (k < 0) continue;                             // (reported above)
      CHECK(targets_of_set.insert(target[k]).second, "%s: target %d twice in a set", name,
            target[k]);
      CHECK(order.round_of[k] == order.round_of[item_at[set.begin]], "%s: set spans rounds", name);
      for (int a = 0; a < 3; ++a) {
        CHECK(first_of[k][a] == sum[a], "%s: item %d launch %d first %lld, prefix %lld", name, k,
              a, first_of[k][a], sum[a]);
        sum[a] += blocks[k][a];
      }
    }
    for (int a = 0; a < 3; ++a) {
      CHECK(set.total[a] == sum[a], "%s: total %lld of %lld", name, set.total[a], sum[a]);
      CHECK(set.end - set.begin == 1 || sum[a] <= bound, "%s: launch %d of %lld blocks", name, a,
            sum[a]);
    }
  }
  CHECK(expected_begin == num, "%s: sets end at %d", name, expected_begin);
  // Rounds in order, list order inside a round.
  for (int slot = 1; slot < num; ++slot) {
    const int k = item_at[slot], before = item_at[slot - 1];
    if (k < 0 || before < 0) continue;
    CHECK(order.round_of[before] < order.round_of[k] ||
              (order.round_of[before] == order.round_of[k] && before < k),
          "%s: item %d stands before item %d", name, before, k);
  }
  // Nothing is cut that would have fitted: a set ends at its round's end, at `most` items, or
  // where the next item of the round would pass a bound.
  for (size_t s = 0; s + 1 < sets.size(); ++s) {
    const int k = item_at[sets[s + 1].begin];
    if (k < 0 || order.round_of[k] != order.round_of[item_at[sets[s].begin]]) continue;
    bool full = sets[s].end - sets[s].begin == most;
    for (int a = 0; a < 3; ++a) full |= sets[s].total[a] + blocks[k][a] > bound;
    CHECK(full, "%s: set %zu cut early", name, s);
  }
}

void CheckCuts() {
  // Target 7 three times, the others once: rounds of 4, 1 and 1 items.  Item 2 alone exceeds a
  // bound of 10 in its second launch; items 1 and 4 have launches without blocks.
  const std::vector<int> target = {7, 3, 7, 9, 5, 7};
  const std::vector<std::vector<long long>> blocks = {
      {4, 2, 1}, {0, 0, 3}, {3, 25, 2}, {6, 1, 0}, {1, 0, 0}, {5, 5, 5}};
  for (int most : {1, 2, 100})
    for (long long bound : {10ll, 7ll, 1ll << 24}) CheckCut("mixed", target, blocks, most, bound);
  // Two items fill two launches to the bound exactly; the third opens the next set.
  CheckCut("exact fit", {0, 1, 2}, {{6, 4, 0}, {4, 6, 0}, {1, 0, 0}}, 100, 10);
  CheckCut("two targets repeat", {1, 2, 2, 1, 2}, {{1, 1, 1}, {2, 0, 2}, {3, 3, 0}, {0, 4, 4}, {5, 5, 5}},
           2, 8);
  CheckCut("single", {1}, {{0, 0, 0}}, 1, 10);
  CheckCut("one round", {0, 1, 2, 3}, {{6, 0, 0}, {5, 0, 0}, {11, 0, 0}, {4, 0, 0}}, 100, 10);
  const std::vector<cmx::LaunchSet> none =
      cmx::CutSets({}, 4, {1, 1, 1}, [](int, long long*) {}, [](int, int, const long long*) {});
  CHECK(none.empty(), "%zu sets of no items", none.size());
}

void CheckStaging() {
  const float a[6] = {1, 2, 3, 4, 5, 6}, b[3] = {7, 8, 9}, c[9] = {10, 11, 12, 13, 14, 15, 16, 17, 18};
  struct { int item = -1, there = 0, here = 0, calls = 0; } bad;
  const auto mismatch = [&](int item, int there, int here) {
    bad.item = item; bad.there = there; bad.here = here; ++bad.calls;
  };
  cmx::StagedArrays arrays(3);
  arrays.Add(0, a, 2, mismatch);
  arrays.Add(1, nullptr, 0, mismatch);                 // ignored, as is a real pointer with count 0
  arrays.Add(2, c, 0, mismatch);
  arrays.Add(3, b, 1, mismatch);
  arrays.Add(4, a, 2, mismatch);                       // the same array again: one offset
  arrays.Add(5, c, 3, mismatch);
  CHECK(bad.calls == 0, "%d mismatches", bad.calls);
  CHECK(arrays.floats() == 18, "%zu floats", arrays.floats());
  CHECK(arrays.OffsetOf(a) == 0 && arrays.OffsetOf(b) == 6 && arrays.OffsetOf(c) == 9,
        "offsets %zu %zu %zu", arrays.OffsetOf(a), arrays.OffsetOf(b), arrays.OffsetOf(c));
  arrays.Add(6, b, 2, mismatch);
  CHECK(bad.calls == 1 && bad.item == 6 && bad.there == 1 && bad.here == 2,
        "mismatch %d: item %d, %d there, %d here", bad.calls, bad.item, bad.there, bad.here);
  CHECK(arrays.floats() == 18 && arrays.OffsetOf(b) == 6, "a mismatch changed the staging");
  std::vector<float> staging(arrays.floats(), -1.f);   // exactly as large: the sanitizer watches
  int copies = 0;
  arrays.CopyTo(staging.data(), [&](int n, const auto& copy) {
    copies = n;
    for (int s = n - 1; s >= 0; --s) copy(s);          // (any order)
  });
  CHECK(copies == 3, "%d copies", copies);
  for (int i = 0; i < 18; ++i) CHECK(staging[i] == i + 1.f, "staging[%d] = %g", i, staging[i]);
}

void CheckLayout() {
  struct Wide { char bytes[40]; };
  for (size_t n : {size_t(0), size_t(1), size_t(6), size_t(7), size_t(64), size_t(1000)}) {
    cmx::BlockLayout block;
    const auto wide = block.Add<Wide>(n);
    const size_t after_wide = block.bytes;
    const auto ints = block.Add<int>(n + 1);
    const size_t after_ints = block.bytes;
    const auto empty = block.Add<float>(0);
    const auto bytes = block.Add<char>(3 * n);
    CHECK(wide.at == 0 && wide.at + sizeof(Wide) * n <= ints.at, "n %zu: wide", n);
    CHECK(ints.at == after_wide && ints.at + sizeof(int) * (n + 1) <= empty.at, "n %zu: ints", n);
    CHECK(empty.at == after_ints && bytes.at == empty.at, "n %zu: an empty region", n);
    CHECK(bytes.at + 3 * n <= block.bytes && block.bytes < bytes.at + 3 * n + 256, "n %zu: total", n);
    for (size_t at : {wide.at, ints.at, empty.at, bytes.at, block.bytes})
      CHECK(at % 256 == 0, "n %zu: offset %zu", n, at);
    std::vector<char> host(block.bytes + 1), device(block.bytes + 1);
    CHECK(reinterpret_cast<char*>(ints(host.data())) == host.data() + ints.at &&
              reinterpret_cast<char*>(ints(device.data())) == device.data() + ints.at,
          "n %zu: typed pointers", n);
  }
  CHECK(cmx::Align256(0) == 0 && cmx::Align256(1) == 256 && cmx::Align256(256) == 256 &&
            cmx::Align256(257) == 512, "Align256");
  CHECK(cmx::BlocksOf(0, 256) == 0 && cmx::BlocksOf(1, 256) == 1 && cmx::BlocksOf(256, 256) == 1 &&
            cmx::BlocksOf(257, 256) == 2 && cmx::BlocksOf((1ll << 40) + 1, 4) == (1ll << 38) + 1,
        "BlocksOf");
}

}  // namespace

int main() {
  const int tables = CheckBisection();
  CheckCuts();
  CheckStaging();
  CheckLayout();
  printf("tables %d\nfailures %d\n", tables, failures);
  return failures ? 1 : 0;
}
