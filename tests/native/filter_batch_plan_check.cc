// filters_batch_plan.h on the host, under the sanitizers (tests/test_abi_filter_batch.py): random
// forests of filter jobs through the checks and the plan of cmx_filter_batch.  Every job that
// takes a workgroup has one descriptor slot of one set, the launches of a set tile its table stage
// after stage, a launch's N is the largest of its jobs and on its side of the occupancy line, a
// child sits in its root's set behind it with its root's N, and a list broken in one place is
// refused with the index of that place.
#include <cstdio>
#include <random>
#include <vector>

#include "filters_batch_plan.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (++failures < 20) std::printf("line %d: %s\n", __LINE__, #cond);  \
    }                                                                      \
  } while (0)

struct Verdict { int job = -1; };

bool Check(const std::vector<cmx_filter_job>& jobs, Verdict* v) {
  return cmx::CheckFilterJobs(jobs.data(), static_cast<int>(jobs.size()),
                              [v](int job, const char*) { v->job = job; });
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  const auto draw = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  static float cloud_store[64];            // addresses only: the plan reads no cloud
  static float out_xyz;
  static int32_t out_idx;
  const int sizes[] = {0, 1, 63, 64, 65, 300, 1000, 2048, 2049, 4096, 4097, 5000, 1 << 26};
  int calls = 0;
  for (; calls < 2000; ++calls) {
    const int num = draw(1, 40);
    std::vector<cmx_filter_job> jobs(num);
    std::vector<int> roots, size_of_cloud(64, -1);
    for (int k = 0; k < num; ++k) {
      cmx_filter_job& J = jobs[k];
      J = cmx_filter_job{};
      J.mode = draw(0, 1);
      J.length = 0.5f;
      J.input_job = -1;
      if (!roots.empty() && draw(0, 2) == 0) {
        J.input_job = roots[draw(0, static_cast<int>(roots.size()) - 1)];
      } else {
        const int c = draw(0, 63);
        if (size_of_cloud[c] < 0) size_of_cloud[c] = sizes[draw(0, 12)];
        J.point_cloud_xyz = size_of_cloud[c] ? &cloud_store[c] : nullptr;
        J.num_points = size_of_cloud[c];
        roots.push_back(k);
      }
      if (draw(0, 3) != 0) J.kept_indices = &out_idx;
      if (draw(0, 3) != 0) J.filtered_xyz = &out_xyz;
    }
    // (a job without outputs needs a child: give it an output instead)
    std::vector<char> has_child(num, 0);
    for (const cmx_filter_job& J : jobs)
      if (J.input_job >= 0) has_child[J.input_job] = 1;
    for (int k = 0; k < num; ++k)
      if (!jobs[k].kept_indices && !jobs[k].filtered_xyz && !has_child[k])
        jobs[k].kept_indices = &out_idx;
    Verdict ok;
    EXPECT(Check(jobs, &ok) && ok.job == -1);

    const long long bound = draw(0, 3) == 0 ? 1000 * draw(1, 200) : cmx::kFilterSetBytes;
    const cmx::FilterBatchPlan plan = cmx::PlanFilterBatch(jobs.data(), num, bound);
    int in_sets = 0, launches = 0;
    long long staged = 0;
    for (size_t s = 0; s < plan.sets.size(); ++s) {
      const cmx::FilterSetPlan& set = plan.sets[s];
      EXPECT(!set.jobs.empty());
      in_sets += static_cast<int>(set.jobs.size());
      staged += 4 * set.staged_floats;
      int next = 0;
      for (int stage = 0; stage < 2; ++stage) {
        for (int launch = 0; launch < 2; ++launch) {
          const cmx::FilterLaunchPlan& L = set.launch[stage][launch];
          EXPECT(L.first == next);
          int largest = 0;
          for (int slot = L.first; slot < L.first + L.count; ++slot) {
            const int k = set.jobs[slot];
            const cmx::FilterJobPlan& P = plan.jobs[k];
            EXPECT(P.set == static_cast<int>(s) && P.slot == slot && P.stage == stage &&
                   P.launch == launch && !P.single);
            EXPECT((P.N <= cmx::kTwoPerUnitN) == (launch == 0));
            EXPECT(P.lds_bytes == static_cast<long long>(cmx::SmallFilterLaunchLds(P.N)));
            EXPECT(P.lds_bytes <= 160 * 1024 - 256);
            largest = P.N > largest ? P.N : largest;
            const cmx::FilterJobPlan& R = plan.jobs[P.root];
            EXPECT(jobs[P.root].num_points >= 1 && jobs[P.root].num_points <= P.N &&
                   P.N < 2 * jobs[P.root].num_points + 64);
            if (stage == 1) EXPECT(R.set == P.set && R.slot < P.slot && R.N == P.N && P.root != k);
          }
          EXPECT(L.N == largest);
          next += L.count;
          launches += L.count > 0;
        }
      }
      EXPECT(next == static_cast<int>(set.jobs.size()));
    }
    EXPECT(launches == plan.num_launches && staged == plan.staged_bytes);
    int expected_in_sets = 0;
    for (int k = 0; k < num; ++k) {
      const cmx::FilterJobPlan& P = plan.jobs[k];
      const int n = jobs[P.root].num_points;
      EXPECT(P.single == (n > cmx::kSmallCloud));
      EXPECT((P.set >= 0) == (n >= 1 && n <= cmx::kSmallCloud));
      expected_in_sets += P.set >= 0;
      EXPECT((P.cloud_slot >= 0) == (jobs[k].input_job < 0 && n > 0));
      for (int j = 0; j < k; ++j)
        if (plan.jobs[j].cloud_slot >= 0 && P.cloud_slot >= 0)
          EXPECT((plan.jobs[j].cloud_slot == P.cloud_slot) ==
                 (jobs[j].point_cloud_xyz == jobs[k].point_cloud_xyz));
    }
    EXPECT(in_sets == expected_in_sets);

    // One rule broken in one place.
    const int at = draw(0, num - 1);
    std::vector<cmx_filter_job> broken = jobs;
    switch (draw(0, 4)) {
      case 0: broken[at].mode = 2; break;
      case 1: broken[at].length = 0.f; break;
      case 2: broken[at].num_points = -1; break;
      case 3: broken[at].input_job = at; break;
      default: broken[at].input_job = num; break;
    }
    Verdict v;
    EXPECT(!Check(broken, &v) && v.job == at);
  }
  std::printf("calls %d failures %d\n", calls, failures);
  return failures == 0 ? 0 : 1;
}
