// The host preparation of cmx_tsdf2d_insert_batch (cartographer_amd/csrc/tsdf_2d_host.h: plan,
// shared sort and normals, ray tables) as a stand-alone program, built by
// tests/test_abi_tsdf2d_insert_batch.py under the address and undefined-behaviour sanitizers:
// four rings of 64 hits into two 16 x 16 grids at 5 cm, once serially and once over a pool of
// threads, the two ray tables compared byte for byte.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#include "tsdf_2d_host.h"

namespace {

using cmx::TsdfRay;
namespace t2 = cmx::tsdf2d;

int failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      ++failures;                                                     \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond);    \
    }                                                                 \
  } while (0)

std::vector<float> Ring(float radius) {
  std::vector<float> xyz;
  for (int i = 0; i < 64; ++i) {
    const double a = 2.0 * M_PI * (i + 0.25) / 64;
    xyz.push_back(static_cast<float>(radius * std::cos(a)));
    xyz.push_back(static_cast<float>(radius * std::sin(a)));
    xyz.push_back(0.f);
  }
  return xyz;
}

const auto kSerial = [](int n, const std::function<void(int)>& fn) {
  for (int i = 0; i < n; ++i) fn(i);
};

const auto kThreads = [](int n, const std::function<void(int)>& fn) {
  std::atomic<int> next{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < 4; ++t)
    pool.emplace_back([&] {
      for (int i = next++; i < n; i = next++) fn(i);
    });
  for (std::thread& t : pool) t.join();
};

struct Prepared {
  t2::CallPlan plan;
  std::vector<TsdfRay> table;
};

template <class Run>
Prepared Prepare(const std::vector<t2::InsertionInput>& inputs,
                 const cmx_tsdf_inserter_options_2d& options, Run&& run) {
  Prepared out;
  out.plan.grids.resize(2);
  for (t2::PlannedGrid& g : out.plan.grids) g.limits = t2::Limits{0.05, 0.4, 0.4, 16, 16};
  const t2::PlanError planned =
      t2::PlanCall(&out.plan, inputs.data(), static_cast<int>(inputs.size()), options, run);
  EXPECT(!planned);
  out.table.assign(out.plan.total_rays, TsdfRay{});
  const t2::PlanError built = t2::BuildRayTables(out.plan, out.table.data(), run);
  EXPECT(!built);
  return out;
}

}  // namespace

int main() {
  // configuration_files/trajectory_builder_2d.lua:100-112
  const cmx_tsdf_inserter_options_2d lua{0.3, 10.0, 0, 4, 0.5, 1, 0, 0.5, 0.5};
  const float origin[3] = {0.f, 0.f, 0.f};
  const float radii[4] = {1.0f, 1.1f, 2.5f, 1.2f};
  std::vector<std::vector<float>> rings;
  for (float r : radii) rings.push_back(Ring(r));
  std::vector<t2::InsertionInput> inputs;
  for (const std::vector<float>& ring : rings)
    for (int grid = 0; grid < 2; ++grid)
      inputs.push_back(t2::InsertionInput{grid, origin, ring.data(), 64});

  const Prepared serial = Prepare(inputs, lua, kSerial);
  const Prepared pooled = Prepare(inputs, lua, kThreads);

  EXPECT(serial.plan.scans.size() == 4);            // eight insertions, four distinct scans
  EXPECT(serial.plan.total_rays == 8 * 64);
  const int sizes[4] = {64, 64, 128, 128};          // +-0.8, +-1.6, +-3.2 m around the centre
  for (size_t k = 0; k < inputs.size(); ++k) {
    const t2::PlannedInsertion& a = serial.plan.insertions[k];
    const t2::PlannedInsertion& b = pooled.plan.insertions[k];
    EXPECT(a.at.nx == sizes[k / 2] && a.at.ny == sizes[k / 2]);
    EXPECT(a.num_rays == 64 && a.first_ray == 64 * k);
    EXPECT(a.at.nx == b.at.nx && a.at.max_x == b.at.max_x && a.at.max_y == b.at.max_y);
    EXPECT(a.start_x == b.start_x && a.start_y == b.start_y && a.scan == b.scan);
  }
  EXPECT(serial.table.size() == pooled.table.size());
  EXPECT(std::memcmp(serial.table.data(), pooled.table.data(),
                     sizeof(TsdfRay) * serial.table.size()) == 0);
  // The same scan at two limits: other ray ends, everything else equal.
  const TsdfRay& early = serial.table[0];           // ring 0 at 64 cells
  EXPECT(early.begin.x >= 0 && early.begin.x / t2::kSubpixels < 64);

  // One pointer with two counts, and a ray that leaves the limits (z != 0 shortens the box).
  std::vector<t2::InsertionInput> bad = inputs;
  bad[5].num_returns = 63;
  t2::CallPlan plan;
  plan.grids.resize(2);
  for (t2::PlannedGrid& g : plan.grids) g.limits = t2::Limits{0.05, 0.4, 0.4, 16, 16};
  const t2::PlanError mismatch = t2::PlanCall(&plan, bad.data(), 8, lua, kSerial);
  EXPECT(mismatch.kind == t2::PlanError::kCountMismatch && mismatch.insertion == 5);
  const float far[3] = {3.5f, 0.f, 30.f};
  cmx_tsdf_inserter_options_2d wide = lua;
  wide.truncation_distance = 0.5;
  std::vector<t2::InsertionInput> leaves = {inputs[0], t2::InsertionInput{1, origin, far, 1},
                                            inputs[2]};
  t2::CallPlan plan2;
  plan2.grids.resize(2);
  for (t2::PlannedGrid& g : plan2.grids) g.limits = t2::Limits{0.05, 1.0, 1.0, 16, 16};
  EXPECT(!t2::PlanCall(&plan2, leaves.data(), 3, wide, kThreads));
  const t2::PlanError outside = t2::BuildRayTables(plan2, nullptr, kThreads);
  EXPECT(outside.kind == t2::PlanError::kLeavesLimits && outside.insertion == 1);

  std::printf("rays %zu failures %d\n", serial.table.size(), failures);
  return failures ? 1 : 0;
}
