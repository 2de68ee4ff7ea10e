// histogram_batch_plan.h on the host, under the sanitizers (tests/test_histogram_batch_plan.py):
// random lists of histogram jobs through the checks and the plan of
// cmx_compute_histogram_batch.  Every batched job has one descriptor slot of one set, the
// launches of a set tile its table, a launch's N is the largest of its jobs and all of them are of
// its class, no set passes a bound unless one job does so alone, equal pointers share a cloud
// slot and a route, the LDS of the largest carve fits a compute unit, and a list broken in one
// place is refused with the index of that place.
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "histogram_batch_plan.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (++failures < 20) std::printf("line %d: %s\n", __LINE__, #cond);  \
    }                                                                      \
  } while (0)

struct Verdict { int job = -1; };

bool Check(const std::vector<cmx_histogram_job>& jobs, Verdict* v) {
  return cmx::CheckHistogramJobs(jobs.data(), static_cast<int>(jobs.size()),
                                 [v](int job, const char*) { v->job = job; });
}

}  // namespace

int main() {
  using namespace cmx;
  std::mt19937 rng(11);
  const auto draw = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  static float cloud_store[64];            // addresses only: `finite` is the test's own
  static float out;
  const int sizes[] = {0, 1, 63, 64, 65, 300, 1000, 2048, 2049, 4096, 4097, 5000, 1 << 24};
  const int bins[] = {1, 7, 120, 8192};

  // the carves and their classes
  EXPECT(HistogramLdsBytes(4096) <= 160 * 1024);
  EXPECT(HistogramLdsBytes(4096) <= 160 * 1024 - 256);      // the kernel's opt-in
  EXPECT(HistogramN(1) == 64 && HistogramN(64) == 64 && HistogramN(65) == 128);
  EXPECT(HistogramN(2049) == 4096 && HistogramN(4096) == 4096);
  for (int N = 64; N <= 4096; N <<= 1) {
    EXPECT(HistogramWorkgroupsPerUnit(N) >= 1);
    EXPECT(HistogramWorkgroupsPerUnit(N) <= kHistogramWorkgroupsByRegisters);
    EXPECT(HistogramWorkgroupsPerUnit(N) * static_cast<long long>(HistogramLdsBytes(N)) <= kLdsPerUnit);
    if (N > 64) {
      EXPECT(HistogramLaunchClass(N) >= HistogramLaunchClass(N / 2));
      EXPECT((HistogramLaunchClass(N) != HistogramLaunchClass(N / 2)) ==
             (HistogramWorkgroupsPerUnit(N) != HistogramWorkgroupsPerUnit(N / 2)));
    }
  }
  EXPECT(HistogramLaunchClass(64) == 0);
  const float finite_cloud[6] = {0.f, -1.f, 3e38f, 1e-45f, -0.f, 2.f};
  float broken_cloud[6] = {0.f, -1.f, 3e38f, 1e-45f, -0.f, 2.f};
  EXPECT(CloudIsFinite(finite_cloud, 2));
  for (float poison : {NAN, INFINITY, -INFINITY})
    for (int at = 0; at < 6; ++at) {
      broken_cloud[at] = poison;
      EXPECT(!CloudIsFinite(broken_cloud, 2));
      broken_cloud[at] = finite_cloud[at];
    }

  int calls = 0, sets_seen = 0, launches_seen = 0;
  for (; calls < 2000; ++calls) {
    const int num = draw(1, 40);
    std::vector<cmx_histogram_job> jobs(num);
    std::vector<int> size_of_cloud(64, -1);
    std::vector<char> poisoned(64, 0);
    for (int k = 0; k < num; ++k) {
      cmx_histogram_job& J = jobs[k];
      const int c = draw(0, 63);
      if (size_of_cloud[c] < 0) {
        size_of_cloud[c] = sizes[draw(0, 12)];
        poisoned[c] = draw(0, 7) == 0;
      }
      J.point_cloud_xyz = size_of_cloud[c] ? &cloud_store[c] : nullptr;
      J.num_points = size_of_cloud[c];
      J.histogram_size = bins[draw(0, 3)];
      J.histogram = &out;
    }
    Verdict verdict;
    EXPECT(Check(jobs, &verdict) && verdict.job == -1);

    // a list broken in one place
    {
      std::vector<cmx_histogram_job> broken = jobs;
      const int at = draw(0, num - 1);
      switch (draw(0, 5)) {
        case 0: broken[at].num_points = -1; break;
        case 1: broken[at].num_points = (1 << 24) + 1; break;
        case 2: broken[at].histogram_size = 0; break;
        case 3: broken[at].histogram_size = 8193; break;
        case 4: broken[at].histogram = nullptr; break;
        default: broken[at].point_cloud_xyz = nullptr; broken[at].num_points = 5; break;
      }
      Verdict v;
      EXPECT(!Check(broken, &v) && v.job == at);
    }

    const long long bound = draw(0, 3) == 0 ? 1024ll * draw(1, 200) : kHistogramSetBytes;
    int asked = 0;
    const auto cloud_of = [&](int k) { return static_cast<int>(jobs[k].point_cloud_xyz - cloud_store); };
    const HistogramBatchPlan plan = PlanHistogramBatch(jobs.data(), num, bound, [&](int k) {
      ++asked;
      EXPECT(jobs[k].num_points >= 1 && jobs[k].num_points <= kSmallCloud);
      return !poisoned[cloud_of(k)];
    });
    EXPECT(static_cast<int>(plan.jobs.size()) == num);
    sets_seen += static_cast<int>(plan.sets.size());
    launches_seen += plan.num_launches;

    // routes, carves, cloud slots
    std::map<const float*, int> slot_of;
    int small_clouds = 0, singles = 0;
    for (int k = 0; k < num; ++k) {
      const HistogramJobPlan& P = plan.jobs[k];
      const int n = jobs[k].num_points;
      if (n == 0) {
        EXPECT(P.route == kHistogramNone && P.cloud_slot == -1);
      } else {
        const bool single = n > kSmallCloud || poisoned[cloud_of(k)];
        EXPECT(P.route == (single ? kHistogramSingle : kHistogramBatched));
        singles += single;
        const auto [at, fresh] = slot_of.emplace(jobs[k].point_cloud_xyz, static_cast<int>(slot_of.size()));
        EXPECT(P.cloud_slot == at->second);
        if (fresh && n <= kSmallCloud) ++small_clouds;
      }
      if (P.route == kHistogramBatched) {
        EXPECT(P.N >= 64 && P.N >= n && (P.N == 64 || P.N / 2 < n) && (P.N & (P.N - 1)) == 0);
        EXPECT(P.lds_bytes == static_cast<long long>(HistogramLdsBytes(P.N)));
        EXPECT(P.set >= 0 && P.set < static_cast<int>(plan.sets.size()));
      } else {
        EXPECT(P.set == -1 && P.launch == -1 && P.slot == -1 && P.N == 0 && P.lds_bytes == 0);
      }
    }
    EXPECT(asked == small_clouds);                 // every distinct small cloud is scanned once
    EXPECT(static_cast<int>(plan.single_jobs.size()) == singles);

    // sets, launches, slots
    std::vector<int> seen(num, 0);
    int launches = 0, previous_first_job = -1;
    long long staged = 0;
    for (size_t s = 0; s < plan.sets.size(); ++s) {
      const HistogramSetPlan& set = plan.sets[s];
      EXPECT(!set.jobs.empty());
      int next = 0, previous_class = -1;
      for (size_t l = 0; l < set.launches.size(); ++l) {
        const HistogramLaunchPlan& L = set.launches[l];
        EXPECT(L.first == next && L.count > 0);               // contiguous: the launches tile the table
        EXPECT(L.cls > previous_class);
        previous_class = L.cls;
        int largest = 0;
        for (int slot = L.first; slot < L.first + L.count && slot < static_cast<int>(set.jobs.size()); ++slot) {
          const HistogramJobPlan& P = plan.jobs[set.jobs[slot]];
          EXPECT(P.set == static_cast<int>(s) && P.launch == static_cast<int>(l) && P.slot == slot);
          EXPECT(HistogramLaunchClass(P.N) == L.cls);
          largest = std::max(largest, P.N);
          ++seen[set.jobs[slot]];
        }
        EXPECT(L.N == largest && HistogramLaunchClass(L.N) == L.cls);
        next += L.count;
        ++launches;
      }
      EXPECT(next == static_cast<int>(set.jobs.size()));
      // the bounds: distinct clouds and the result block, unless the set is one job
      std::map<const float*, int> clouds;
      long long results = 0;
      int first_job = num;
      for (int k : set.jobs) {
        clouds.emplace(jobs[k].point_cloud_xyz, jobs[k].num_points);
        results += HistogramResultBytes(jobs[k]);
        first_job = std::min(first_job, k);
      }
      long long floats = 0;
      for (const auto& [p, n] : clouds) floats += 3ll * n;
      EXPECT(set.staged_floats == floats && set.result_bytes == results);
      if (set.jobs.size() > 1) EXPECT(4 * floats <= bound && results <= bound);
      EXPECT(first_job > previous_first_job);                  // sets follow the list
      previous_first_job = first_job;
      staged += 4 * floats;
    }
    EXPECT(launches == plan.num_launches && staged == plan.staged_bytes);
    for (int k = 0; k < num; ++k) EXPECT(seen[k] == (plan.jobs[k].route == kHistogramBatched ? 1 : 0));
  }

  // one pointer with two counts, in a fixed place
  {
    std::vector<cmx_histogram_job> jobs(3, cmx_histogram_job{&cloud_store[0], 10, 120, &out});
    jobs[2].num_points = 11;
    Verdict v;
    EXPECT(!Check(jobs, &v) && v.job == 2);
  }
  EXPECT(sets_seen > 2000 && launches_seen >= sets_seen);
  std::printf("calls %d sets %d launches %d failures %d\n", calls, sets_seen, launches_seen, failures);
  return failures == 0 ? 0 : 1;
}
