// csrc/ceres_trust_region.h on the host (tests/test_ceres_trust_region.py builds this with the
// address and undefined-behaviour sanitizers): the minimizer the two Ceres kernels share, run over
// oracle::CeresResiduals2D and compared with oracle::CeresScanMatcher2DMatch.  Both sides are then
// the same statements over the same sums, so pose, costs, step counts and termination must be
// EQUAL; every case also asserts that it reaches the branch it is named for.  Two cases with a
// failing evaluator follow the rules in the header's comments (the oracle has no such evaluator).
// Every case runs twice: with array bound 3, and with bound 6 and three unknowns, which is how
// the 3D kernel instantiates the loop and SolveSpd (K < kMaxLocal).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ceres_trust_region.h"
#include "oracle_ceres_2d.h"

namespace {

int failures = 0;
#define CHECK_THAT(cond, ...)                                  \
  do {                                                         \
    if (!(cond)) {                                             \
      ++failures;                                              \
      std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                \
      std::printf("\n");                                       \
    }                                                          \
  } while (0)

// ---- the scene: a 64 x 48 probability grid with three walls, blurred so that the cost has a
// basin around them, and 200 points on the walls seen from kTruth ---------------------------------
constexpr int kNx = 64, kNy = 48;
constexpr double kRes = 0.05;
constexpr double kTruth[3] = {1.3, 1.5, 0.3};
struct Segment { double x0, y0, x1, y1; };
const Segment kWalls[3] = {{0.4, 0.5, 0.4, 2.7}, {0.4, 2.7, 2.0, 2.7}, {2.0, 2.7, 2.0, 1.6}};

double DistanceToWalls(double x, double y) {
  double best = 1e9;
  for (const Segment& s : kWalls) {
    const double dx = s.x1 - s.x0, dy = s.y1 - s.y0;
    double t = ((x - s.x0) * dx + (y - s.y0) * dy) / (dx * dx + dy * dy);
    t = std::fmin(1., std::fmax(0., t));
    best = std::fmin(best, std::hypot(x - (s.x0 + t * dx), y - (s.y0 + t * dy)));
  }
  return best;
}

struct Scene {
  std::vector<uint16_t> cells;
  oracle::ProbabilityGridView grid;
  oracle::PointCloud cloud;
};

const Scene& TheScene() {
  static const Scene scene = [] {
    Scene s;
    s.cells.assign(kNx * kNy, 0);
    oracle::MapLimits limits;
    limits.resolution = kRes;
    limits.max_x = kNy * kRes;           // iy counts down from max_x, ix down from max_y
    limits.max_y = kNx * kRes;
    limits.num_x_cells = kNx;
    limits.num_y_cells = kNy;
    for (int iy = 0; iy < kNy; ++iy) {
      for (int ix = 0; ix < kNx; ++ix) {
        const double x = limits.max_x - kRes * (iy + 0.5), y = limits.max_y - kRes * (ix + 0.5);
        const double d = DistanceToWalls(x, y) / (3. * kRes);
        const double cost = 0.9 - 0.8 * std::exp(-0.5 * d * d);     // in [0.1, 0.9]
        // a border of unknown cells, so that stencils near the edge read value 0 as well
        if (ix == 0 || iy == 0 || ix == kNx - 1 || iy == kNy - 1) continue;
        s.cells[kNx * iy + ix] =
            static_cast<uint16_t>(1 + std::lround((cost - 0.1) / 0.8 * 32766.));
      }
    }
    s.grid.limits = limits;
    s.grid.cells = s.cells.data();
    const double c = std::cos(kTruth[2]), sn = std::sin(kTruth[2]);
    for (int i = 0; i < 200; ++i) {
      const Segment& w = kWalls[i % 3];
      const double t = (i / 3 + 0.5) / 67.;
      const double wx = w.x0 + t * (w.x1 - w.x0) - kTruth[0];
      const double wy = w.y0 + t * (w.y1 - w.y0) - kTruth[1];
      s.cloud.push_back({static_cast<float>(c * wx + sn * wy),
                         static_cast<float>(-sn * wx + c * wy), 0.f});
    }
    return s;
  }();
  return scene;
}

// ---- the problem handed to the shared minimizer ------------------------------------------------
struct Setup {
  oracle::CeresOptions2D options;
  double target[2];
  double init[3];
  const oracle::PointCloud* cloud;
};

template <int kBound>
struct HostProblem {
  static constexpr int kAmbient = 3, kMaxLocal = kBound;
  static constexpr bool kEvaluationCanFail = true;
  const Setup& setup;
  int fail_at = 0;                       // the evaluation (counted from 1) that reports failure
  int evaluations = 0;
  std::vector<double> plus_from;         // the x of every Plus, three numbers each
  std::vector<double> candidates;        // what every Plus returned
  std::vector<double> r, J;

  int LocalSize() const { return 3; }
  // Cost, J^T r and J^T J in the order of CeresScanMatcher2DMatch's `evaluate`.
  bool Evaluate(const double* x, cmx::TrEvaluation<kBound>* e) {
    if (++evaluations == fail_at) return false;
    oracle::CeresResiduals2D(setup.options, setup.target, setup.init[2], *setup.cloud,
                             TheScene().grid, x, &r, &J);
    e->cost = 0.;
    for (int a = 0; a < 3; ++a) {
      e->g[a] = 0.;
      for (int b = 0; b < 3; ++b) e->H[a][b] = 0.;
    }
    for (size_t i = 0; i < r.size(); ++i) {
      e->cost += r[i] * r[i];
      const double* row = J.data() + 3 * i;
      for (int a = 0; a < 3; ++a) {
        e->g[a] += row[a] * r[i];
        for (int b = 0; b < 3; ++b) e->H[a][b] += row[a] * row[b];
      }
    }
    e->cost *= 0.5;
    return true;
  }
  void Plus(const double* x, const double* delta, double* out) {
    for (int a = 0; a < 3; ++a) out[a] = x[a] + delta[a];
    plus_from.insert(plus_from.end(), x, x + 3);
    candidates.insert(candidates.end(), out, out + 3);
  }
  double GradientMaxNorm(const double*, const cmx::TrEvaluation<kBound>& e) const {
    return std::fmax(std::fabs(e.g[0]), std::fmax(std::fabs(e.g[1]), std::fabs(e.g[2])));
  }
  double StepNorm(const double*, const double*, const double* delta) const {
    return std::sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
  }
  double Cube(double t) const { return std::pow(t, 3); }     // as oracle_ceres_2d.cc
};

struct Outcome {
  bool ok = false;
  cmx::TrResult<3> result;
  std::vector<double> plus_from, candidates;
};

bool SameBits(const Outcome& a, const Outcome& b) {
  if (a.ok != b.ok || a.plus_from != b.plus_from || a.candidates != b.candidates) return false;
  if (!a.ok) return true;
  return std::memcmp(a.result.x, b.result.x, sizeof(a.result.x)) == 0 &&
         a.result.initial_cost == b.result.initial_cost &&
         a.result.final_cost == b.result.final_cost && a.result.successful == b.result.successful &&
         a.result.unsuccessful == b.result.unsuccessful &&
         a.result.termination == b.result.termination;
}

template <int kBound>
Outcome Run(const Setup& setup, int fail_at) {
  HostProblem<kBound> problem{setup};
  problem.fail_at = fail_at;
  Outcome out;
  // what a failed initial evaluation must leave alone
  for (double& v : out.result.x) v = -7.;
  out.result.initial_cost = out.result.final_cost = -7.;
  out.result.successful = out.result.unsuccessful = out.result.termination = -7;
  out.ok = cmx::MinimizeTrustRegion(problem, setup.init, setup.options.use_nonmonotonic_steps,
                                    setup.options.max_num_iterations, &out.result);
  out.plus_from = problem.plus_from;
  out.candidates = problem.candidates;
  return out;
}

// Bound 3 and, as the 3D kernel instantiates the loop, bound 6 with three unknowns.
Outcome RunBoth(const char* name, const Setup& setup, int fail_at = 0) {
  const Outcome three = Run<3>(setup, fail_at), six = Run<6>(setup, fail_at);
  CHECK_THAT(SameBits(three, six), "%s: bound 6 with K = 3 differs from bound 3", name);
  return three;
}

struct Case {
  const char* name;
  double offset[3];                      // initial pose - kTruth
  double weights[3];                     // occupied space, translation, rotation
  bool nonmonotonic;
  int iterations;
  int termination;                       // expected, -1: any
  int min_successful, min_unsuccessful;
  int exact_successful, exact_unsuccessful;   // -1: any
};

Setup MakeSetup(const Case& c, const oracle::PointCloud* cloud) {
  Setup s;
  s.options.occupied_space_weight = c.weights[0];
  s.options.translation_weight = c.weights[1];
  s.options.rotation_weight = c.weights[2];
  s.options.use_nonmonotonic_steps = c.nonmonotonic;
  s.options.max_num_iterations = c.iterations;
  for (int a = 0; a < 3; ++a) s.init[a] = kTruth[a] + c.offset[a];
  s.target[0] = s.init[0];
  s.target[1] = s.init[1];
  s.cloud = cloud;
  return s;
}

// The shared minimizer against the oracle's own loop: everything EQUAL.
void AgainstOracle(const Case& c, const oracle::PointCloud* cloud) {
  const Setup setup = MakeSetup(c, cloud);
  const Outcome got = RunBoth(c.name, setup);
  oracle::Pose2d pose;
  oracle::CeresSummary2D sum;
  oracle::CeresScanMatcher2DMatch(setup.options, setup.target,
                                  oracle::Pose2d{setup.init[0], setup.init[1], setup.init[2]},
                                  *cloud, TheScene().grid, &pose, &sum);
  std::printf("%-28s steps (%d, %d) termination %d cost %.17g -> %.17g\n", c.name,
              sum.num_successful_steps, sum.num_unsuccessful_steps, sum.termination,
              sum.initial_cost, sum.final_cost);
  CHECK_THAT(got.ok, "%s: the initial evaluation failed", c.name);
  const cmx::TrResult<3>& r = got.result;
  CHECK_THAT(r.x[0] == pose.x && r.x[1] == pose.y && r.x[2] == pose.theta,
             "%s: pose (%.17g, %.17g, %.17g), oracle (%.17g, %.17g, %.17g)", c.name, r.x[0],
             r.x[1], r.x[2], pose.x, pose.y, pose.theta);
  CHECK_THAT(r.initial_cost == sum.initial_cost && r.final_cost == sum.final_cost,
             "%s: costs %.17g -> %.17g, oracle %.17g -> %.17g", c.name, r.initial_cost,
             r.final_cost, sum.initial_cost, sum.final_cost);
  CHECK_THAT(r.successful == sum.num_successful_steps &&
                 r.unsuccessful == sum.num_unsuccessful_steps && r.termination == sum.termination,
             "%s: steps (%d, %d) termination %d, oracle (%d, %d) %d", c.name, r.successful,
             r.unsuccessful, r.termination, sum.num_successful_steps, sum.num_unsuccessful_steps,
             sum.termination);
  // the case reaches its branch
  CHECK_THAT(c.termination < 0 || sum.termination == c.termination, "%s: termination %d", c.name,
             sum.termination);
  CHECK_THAT(sum.num_successful_steps >= c.min_successful &&
                 sum.num_unsuccessful_steps >= c.min_unsuccessful,
             "%s: steps (%d, %d)", c.name, sum.num_successful_steps, sum.num_unsuccessful_steps);
  CHECK_THAT((c.exact_successful < 0 || sum.num_successful_steps == c.exact_successful) &&
                 (c.exact_unsuccessful < 0 || sum.num_unsuccessful_steps == c.exact_unsuccessful),
             "%s: steps (%d, %d)", c.name, sum.num_successful_steps, sum.num_unsuccessful_steps);
}

constexpr int kConvergence = cmx::kTrConvergence, kNoConvergence = cmx::kTrNoConvergence;
static_assert(kConvergence == oracle::kCeresConvergence &&
                  kNoConvergence == oracle::kCeresNoConvergence &&
                  cmx::kTrFailure == oracle::kCeresFailure,
              "the terminations of the header are those of the oracle");

const Case kCases[] = {
    // name, offset, weights, nonmonotonic, iterations, termination, min steps, exact steps
    {"converges_monotonic", {0.03, -0.02, 0.02}, {1., 10., 40.}, false, 50, kConvergence, 2, 0, -1, -1},
    {"converges_nonmonotonic", {0.03, -0.02, 0.02}, {1., 10., 40.}, true, 50, kConvergence, 2, 0, -1, -1},
    {"step_rejected_monotonic", {-0.28, 0.26, 0.11}, {5., 1., 1.}, false, 50, -1, 2, 1, -1, -1},
    {"step_rejected_nonmonotonic", {-0.28, 0.26, 0.11}, {5., 1., 1.}, true, 50, -1, 2, 1, -1, -1},
    {"step_cap_1", {-0.28, 0.26, 0.11}, {5., 1., 1.}, true, 1, kNoConvergence, 0, 0, -1, -1},
    {"step_cap_2", {-0.28, 0.26, 0.11}, {5., 1., 1.}, true, 2, kNoConvergence, 0, 0, -1, -1},
    {"step_cap_3", {-0.28, 0.26, 0.11}, {5., 1., 1.}, true, 3, kNoConvergence, 0, 0, -1, -1},
    // every stencil reads the padding constant: zero gradient at the target
    {"all_outside_zero_gradient", {20., -15., 0.3}, {20., 10., 1.}, false, 10, kConvergence, 0, 0, 0, 0},
};

}  // namespace

int main() {
  const oracle::PointCloud& cloud = TheScene().cloud;
  int cases = 0;
  for (const Case& c : kCases) {
    AgainstOracle(c, &cloud);
    ++cases;
  }
  {
    // The first candidate's evaluation fails: a step counted as unsuccessful and never accepted,
    // so the second candidate starts from the initial point again, with a smaller radius.
    const Setup setup = MakeSetup(kCases[0], &cloud);
    const Outcome plain = RunBoth("plain", setup), got = RunBoth("failed_first_candidate", setup, 2);
    ++cases;
    CHECK_THAT(got.ok && got.result.unsuccessful >= 1, "unsuccessful steps %d",
               got.result.unsuccessful);
    CHECK_THAT(plain.candidates.size() >= 6 && got.candidates.size() >= 6,
               "the case needs two steps");
    if (plain.candidates.size() >= 6 && got.candidates.size() >= 6) {
      for (int a = 0; a < 3; ++a) {
        CHECK_THAT(plain.plus_from[3 + a] == plain.candidates[a],
                   "the case needs a first step that is accepted when it does not fail");
        CHECK_THAT(got.candidates[a] == plain.candidates[a], "first candidate moved");
        CHECK_THAT(got.plus_from[3 + a] == setup.init[a], "the failed candidate was accepted");
        CHECK_THAT(got.result.x[a] != got.candidates[a], "the failed candidate was returned");
      }
      double first = 0., second = 0.;
      for (int a = 0; a < 3; ++a) {
        first += std::pow(got.candidates[a] - setup.init[a], 2);
        second += std::pow(got.candidates[3 + a] - setup.init[a], 2);
      }
      CHECK_THAT(second < first, "the step after the failure is not shorter: %g, %g", second, first);
    }
    CHECK_THAT(got.result.initial_cost == plain.result.initial_cost &&
                   got.result.final_cost < got.result.initial_cost && got.result.successful >= 1,
               "the solve did not go on after the failed candidate");
  }
  {
    // The evaluation at the initial point fails: false, nothing written.
    const Setup setup = MakeSetup(kCases[0], &cloud);
    const Outcome got = RunBoth("failed_initial_evaluation", setup, 1);
    ++cases;
    CHECK_THAT(!got.ok && got.candidates.empty(), "a failed initial evaluation went on");
    CHECK_THAT(got.result.x[0] == -7. && got.result.initial_cost == -7. &&
                   got.result.final_cost == -7. && got.result.successful == -7 &&
                   got.result.unsuccessful == -7 && got.result.termination == -7,
               "a failed initial evaluation wrote a result");
  }
  std::printf("cases %d failures %d\n", cases, failures);
  return failures == 0 ? 0 : 1;
}
