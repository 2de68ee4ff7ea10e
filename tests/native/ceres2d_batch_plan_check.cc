// ceres_2d_batch_plan.h on the host, under the sanitizers (tests/test_ceres2d_batch_plan.py):
// random job lists through the checks and the plan of cmx_ceres2d_match_grid_batch.  Kinds come
// back in list order, equal host pointers share one slot, resident and empty clouds take none,
// the slots lie one behind the other from 256-byte boundaries behind the problem array without
// overlap, the total is the aligned problem array plus the distinct clouds, the launch count does
// not depend on the list, and a list broken in one place is refused with the index of that place.
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "ceres_2d_batch_plan.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (++failures < 20) std::printf("line %d: %s\n", __LINE__, #cond);  \
    }                                                                      \
  } while (0)

struct Verdict { int job = -1; };

bool Check(const std::vector<cmx::Ceres2DJobShape>& shapes, Verdict* v) {
  return cmx::CheckCeres2DJobShapes(shapes.data(), static_cast<int>(shapes.size()),
                                    [v](int job, const char*) { v->job = job; });
}

size_t Align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

}  // namespace

int main() {
  using namespace cmx;
  std::mt19937 rng(23);
  const auto draw = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  static float cloud_store[48];            // addresses only: the plan reads no cloud
  const int sizes[] = {1, 2, 21, 63, 64, 200, 255, 256, 257, 4096, 1 << 24};
  const size_t problem_sizes[] = {1, 152, 160, 256, 257};

  int calls = 0, slots_seen = 0, shared_seen = 0;
  for (; calls < 2000; ++calls) {
    const int num = calls < 3 ? (calls == 0 ? 1 : calls == 1 ? 7 : 300) : draw(1, 60);
    const size_t problem_size = problem_sizes[draw(0, 4)];
    std::vector<Ceres2DJobShape> shapes(num);
    std::vector<int> size_of_cloud(48, -1);
    for (int k = 0; k < num; ++k) {
      Ceres2DJobShape& S = shapes[k];
      S.kind = draw(0, 1);
      const int source = draw(0, 9);
      if (source == 0 && S.kind == kCeres2DTsdf) {          // a TSDF job without points
        S.num_points = 0;
        S.host_xyz = draw(0, 1) ? &cloud_store[0] : nullptr;   // (a pointer with 0 points is no cloud)
      } else if (source <= 2) {                             // resident
        S.resident = true;
        S.num_points = sizes[draw(0, 10)];
      } else {
        const int c = draw(0, 47);
        if (size_of_cloud[c] < 0) size_of_cloud[c] = sizes[draw(0, 10)];
        S.host_xyz = &cloud_store[c];
        S.num_points = size_of_cloud[c];
      }
    }
    Verdict verdict;
    EXPECT(Check(shapes, &verdict) && verdict.job == -1);

    // a list broken in one place
    {
      std::vector<Ceres2DJobShape> broken = shapes;
      const int at = draw(0, num - 1);
      Ceres2DJobShape& S = broken[at];
      switch (draw(0, 5)) {
        case 0: S.kind = 2; break;
        case 1: S.num_points = -1; break;
        case 2: S.num_points = (1 << 24) + 1; break;
        case 3: S.kind = kCeres2DProbabilityGrid; S.num_points = 0; break;
        case 4: S.resident = true; S.host_xyz = &cloud_store[1]; S.num_points = 5; break;
        default: S.resident = false; S.host_xyz = nullptr; S.num_points = 5; break;
      }
      Verdict v;
      EXPECT(!Check(broken, &v) && v.job == at);
    }

    const Ceres2DBatchPlan plan = PlanCeres2DBatch(shapes.data(), num, problem_size);
    EXPECT(static_cast<int>(plan.jobs.size()) == num);
    EXPECT(plan.num_launches == kCeres2DBatchLaunches && plan.num_launches <= 2);
    EXPECT(plan.problem_bytes == Align(problem_size * num));

    std::map<const float*, int> slot_of;
    size_t expected = plan.problem_bytes;
    for (int k = 0; k < num; ++k) {
      const Ceres2DJobShape& S = shapes[k];
      const Ceres2DJobPlan& P = plan.jobs[k];
      EXPECT(P.kind == S.kind);
      if (S.resident || S.num_points == 0) {
        EXPECT(P.cloud_slot == -1 && P.cloud_at == 0);
        continue;
      }
      const auto [at, fresh] = slot_of.emplace(S.host_xyz, static_cast<int>(slot_of.size()));
      EXPECT(P.cloud_slot == at->second);                  // first-seen order, shared by pointer
      if (!fresh) ++shared_seen;
      EXPECT(P.cloud_slot >= 0 && P.cloud_slot < static_cast<int>(plan.clouds.size()));
      if (P.cloud_slot < 0 || P.cloud_slot >= static_cast<int>(plan.clouds.size())) continue;
      const Ceres2DCloudSlot& C = plan.clouds[P.cloud_slot];
      EXPECT(C.host_xyz == S.host_xyz && C.num_points == S.num_points && C.at == P.cloud_at);
      if (fresh) {
        EXPECT(C.at == expected && C.at % 256 == 0);       // one behind the other, no overlap
        expected += Align(12 * static_cast<size_t>(S.num_points));
      }
    }
    EXPECT(plan.clouds.size() == slot_of.size());
    EXPECT(plan.total_bytes == expected);
    slots_seen += static_cast<int>(plan.clouds.size());
  }

  // one pointer with two counts, in a fixed place: the later job is named
  {
    std::vector<Ceres2DJobShape> shapes(4);
    for (Ceres2DJobShape& S : shapes) { S.host_xyz = &cloud_store[0]; S.num_points = 10; }
    shapes[1].kind = kCeres2DTsdf;
    shapes[2].num_points = 11;
    Verdict v;
    EXPECT(!Check(shapes, &v) && v.job == 2);
    // ... but not for a resident cloud, whose pointer field is not set, nor for an empty TSDF job
    shapes[2].num_points = 0;
    shapes[2].kind = kCeres2DTsdf;
    Verdict w;
    EXPECT(Check(shapes, &w) && w.job == -1);
  }
  EXPECT(slots_seen > 2000 && shared_seen > 2000);
  std::printf("calls %d slots %d shared %d failures %d\n", calls, slots_seen, shared_seen, failures);
  return failures == 0 ? 0 : 1;
}
