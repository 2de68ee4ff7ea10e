// What the batched calls share (cmx_{fast2d,fast3d}_create_batch,
// cmx_{grid2d,grid3d,tsdf2d}_insert_batch, cmx_filter_batch):
// a block finds the item of the call it works for, and the host lays out one upload block, stages
// every distinct host array once, sorts the items into rounds and cuts them into launches.
// Plain C++17 without HIP types or CMX_REQUIRE (a failure goes to a callback, the call site words
// the error), pinned on the host by tests/test_batch_plan.py (tests/native/batch_plan_check.cc).
#ifndef CMX_BATCH_H_
#define CMX_BATCH_H_
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>
#ifdef __HIPCC__
#define CMX_BATCH_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define CMX_BATCH_HD inline
#endif
namespace cmx {

// ---- device and host -------------------------------------------------------------------
// first_of(i) = first block of entry i of a launch, first_of(num) = blocks of the launch (never
// asked for): the entry that owns `block`.  An entry without blocks shares its first block with
// its successor and owns none.
template <class FirstOf>
CMX_BATCH_HD int OwnerOfBlock(FirstOf first_of, int num, int block) {
  int lo = 0, hi = num;       // first_of(lo) <= block < first_of(hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first_of(mid) <= block) lo = mid; else hi = mid;
  }
  return lo;
}

// ... over a prefix table of block counts,
CMX_BATCH_HD int EntryOfBlock(const int* __restrict__ first, int num, int block) {
  return OwnerOfBlock([first](int i) { return first[i]; }, num, block);
}

// ... and over the member `First` of a table of descriptors.
template <auto First, class Desc>
CMX_BATCH_HD int DescOfBlock(const Desc* __restrict__ descs, int num, int block) {
  return OwnerOfBlock([descs](int i) { return descs[i].*First; }, num, block);
}

// ---- host ------------------------------------------------------------------------------
inline size_t Align256(size_t bytes) { return (bytes + 255) & ~static_cast<size_t>(255); }
inline long long BlocksOf(long long items, long long tile) { return (items + tile - 1) / tile; }

// One upload block: typed regions, each from a 256-byte boundary, in the order they are added.
// A region gives its typed pointer in the pinned and in the device copy of the block alike.
template <class T>
struct BlockRegion {
  size_t at = 0;
  T* operator()(char* base) const { return reinterpret_cast<T*>(base + at); }
};
struct BlockLayout {
  size_t bytes = 0;           // of the regions so far: a multiple of 256
  template <class T>
  BlockRegion<T> Add(size_t count) {
    const BlockRegion<T> region{bytes};
    bytes = Align256(bytes + sizeof(T) * count);
    return region;
  }
};

// The host arrays of a call (`width` floats per element), each distinct pointer once, in
// first-seen order, densely one behind the other in a staging region.
class StagedArrays {
 public:
  explicit StagedArrays(int width) : width_(width) {}
  // An array without elements is ignored, whatever its pointer.  A pointer that came before
  // with another count: mismatch(item, count there, count here).
  template <class Mismatch>
  void Add(int item, const float* p, int count, Mismatch&& mismatch) {
    if (count == 0) return;
    const auto [found, fresh] = index_.emplace(p, arrays_.size());
    if (fresh) {
      arrays_.push_back(Array{p, count, floats_});
      floats_ += static_cast<size_t>(width_) * count;
    } else if (arrays_[found->second].count != count) {
      mismatch(item, arrays_[found->second].count, count);
    }
  }
  size_t floats() const { return floats_; }                       // of the staging region
  size_t OffsetOf(const float* p) const { return arrays_[index_.at(p)].at; }   // in floats
  // Every distinct array once; run(n, copy) calls copy(0) .. copy(n - 1), in any order.
  template <class Run>
  void CopyTo(float* staging, Run&& run) const {
    run(static_cast<int>(arrays_.size()), [&](int s) {
      const Array& a = arrays_[s];
      memcpy(staging + a.at, a.p, sizeof(float) * width_ * a.count);
    });
  }

 private:
  struct Array { const float* p; int count; size_t at; };
  int width_;
  size_t floats_ = 0;
  std::vector<Array> arrays_;
  std::unordered_map<const float*, size_t> index_;
};

// The targets of a call's items (grids) in first-seen order, and the round of every item: the
// r-th item of a target is in round r, so that no target occurs twice in a round.
template <class Target>
struct TargetRounds {
  std::vector<Target> targets;
  std::vector<int> target_of, round_of;   // by item
  void Add(Target target) {
    auto& [index, items] =
        seen_.emplace(target, std::make_pair(static_cast<int>(targets.size()), 0)).first->second;
    if (items == 0) targets.push_back(target);
    target_of.push_back(index);
    round_of.push_back(items++);
  }

 private:
  std::unordered_map<Target, std::pair<int, int>> seen_;   // target -> its index, items so far
};

// Items [begin, end) in slot order, launched together; what they add up to in each launch.
struct LaunchSet {
  int begin = 0, end = 0;
  long long total[3] = {0, 0, 0};
};

// Cuts items into sets: round by round, a round in list order, a set cut where it is full -- at
// `most` items, or where an amount (blocks of a launch, staged bytes) would pass its bound.  An
// item that exceeds a bound alone still goes out: as a set of its own.  amounts_of(item, add[3])
// says what the item adds; place(item, slot, first[3]) follows in slot order with what the set
// held before it: the item's first block in each launch.
template <class AmountsOf, class Place>
std::vector<LaunchSet> CutSets(const std::vector<int>& round_of, int most,
                               const long long (&bound)[3], AmountsOf&& amounts_of,
                               Place&& place) {
  int rounds = 0;
  for (int r : round_of) rounds = std::max(rounds, r + 1);
  std::vector<std::vector<int>> by_round(rounds);
  for (size_t k = 0; k < round_of.size(); ++k) by_round[round_of[k]].push_back(static_cast<int>(k));
  std::vector<LaunchSet> sets;
  int next = 0;
  for (const std::vector<int>& round : by_round) {
    for (size_t j = 0; j < round.size();) {
      LaunchSet set;
      set.begin = next;
      for (; j < round.size() && next - set.begin < most; ++j) {
        long long add[3] = {0, 0, 0};
        amounts_of(round[j], add);
        if (next > set.begin && (set.total[0] + add[0] > bound[0] ||
                                 set.total[1] + add[1] > bound[1] ||
                                 set.total[2] + add[2] > bound[2]))
          break;
        place(round[j], next++, set.total);
        for (int a = 0; a < 3; ++a) set.total[a] += add[a];
      }
      set.end = next;
      sets.push_back(set);
    }
  }
  return sets;
}

}  // namespace cmx
#endif  // CMX_BATCH_H_
