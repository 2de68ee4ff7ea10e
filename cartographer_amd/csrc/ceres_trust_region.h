// What the two Ceres refinement kernels share (ceres_2d.hip, ceres_3d.hip): the trust-region
// Levenberg-Marquardt loop, the Cholesky solve of its damped system, and the block-wide sum of
// the evaluations.  The loop is Ceres' (trust_region_minimizer.cc, levenberg_marquardt_strategy.cc,
// trust_region_step_evaluator.cc with Solver::Options defaults), restated statement for statement
// the way oracle/oracle_ceres_2d.cc and oracle_ceres_3d.cc restate it (they document every rule
// taken from Ceres and what pins it, and stay separate restatements: they are the yardstick).
// Plain C++17: the minimizer and the solve compile without a HIP header, so that the host runs
// them under the sanitizers (tests/test_ceres_trust_region.py,
// tests/native/ceres_trust_region_check.cc); only BlockSumF64 is device code.
#ifndef CMX_CERES_TRUST_REGION_H_
#define CMX_CERES_TRUST_REGION_H_
#include <float.h>
#include <math.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
// always_inline, as cmx_batch.h has it: the kernels are one function each, and the 3D kernel (all
// 512 registers, spills) is sensitive to when the loop is inlined into it.
#define CMX_TR_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define CMX_TR_HD inline
#endif
namespace cmx {

// Threads of a Ceres workgroup: four wavefronts (BlockSumF64 folds exactly four partials).
constexpr int kCeresThreads = 256;

// ceres::TerminationType as the entry points report it.
constexpr int kTrConvergence = 0, kTrNoConvergence = 1, kTrFailure = 2;

// What a pass over the residual blocks leaves for the minimizer: 1/2 |r|^2, J^T r and J^T J of the
// local (tangent-space) Jacobian; entries at or beyond the local size are never read.
template <int kMaxLocal>
struct TrEvaluation {
  double cost;
  double g[kMaxLocal];
  double H[kMaxLocal][kMaxLocal];
};

template <int kAmbient>
struct TrResult {
  double x[kAmbient];          // the parameters of the lowest cost seen
  double initial_cost, final_cost;
  int successful, unsuccessful, termination;
};

// Cholesky solve of the symmetric positive definite k x k system (k <= kMax); false if the
// matrix is not SPD or the solution is not finite.
template <int kMax>
CMX_TR_HD bool SolveSpd(int k, const double A[kMax][kMax], const double* b, double* x) {
  double L[kMax][kMax];
  for (int i = 0; i < kMax; ++i)
    for (int j = 0; j < kMax; ++j) L[i][j] = 0.;
  for (int i = 0; i < k; ++i) {
    for (int j = 0; j <= i; ++j) {
      double sum = A[i][j];
      for (int m = 0; m < j; ++m) sum -= L[i][m] * L[j][m];
      if (i == j) {
        if (!(sum > 0.)) return false;
        L[i][i] = sqrt(sum);
      } else {
        L[i][j] = sum / L[j][j];
      }
    }
  }
  double y[kMax];
  for (int i = 0; i < k; ++i) {
    double sum = b[i];
    for (int m = 0; m < i; ++m) sum -= L[i][m] * y[m];
    y[i] = sum / L[i][i];
  }
  for (int i = k - 1; i >= 0; --i) {
    double sum = y[i];
    for (int m = i + 1; m < k; ++m) sum -= L[m][i] * x[m];
    x[i] = sum / L[i][i];
  }
  for (int i = 0; i < k; ++i)
    if (!isfinite(x[i])) return false;
  return true;
}

// The minimizer.  `problem` supplies what differs between the callers:
//   kAmbient, kMaxLocal      sizes of the parameter vector and bound of the tangent space
//   kEvaluationCanFail       whether Evaluate may return false (else the branch folds away)
//   int LocalSize()          K <= kMaxLocal
//   bool Evaluate(x, TrEvaluation<kMaxLocal>*)
//   void Plus(x, delta, out)                   the local parameterization
//   double GradientMaxNorm(x, evaluation)      TrustRegionMinimizer::ComputeGradientMaxNorm
//   double StepNorm(x, candidate, delta)       |x - candidate| as the caller's oracle forms it
//   double Cube(t)                             t^3 of the radius update, in the caller's form
// False when the evaluation at `initial` fails (FAILURE; `result` is untouched, the caller words
// its own summary).  On the device every thread carries the (identical) state: no broadcast is
// needed, the workgroup only meets inside Evaluate.
template <class Problem>
CMX_TR_HD bool MinimizeTrustRegion(Problem& problem, const double* initial,
                                   bool use_nonmonotonic_steps, int max_num_iterations,
                                   TrResult<Problem::kAmbient>* result) {
  constexpr int kAmbient = Problem::kAmbient, kMaxLocal = Problem::kMaxLocal;
  const double kFunctionTolerance = 1e-6, kGradientTolerance = 1e-10, kParameterTolerance = 1e-8;
  const double kMinRelativeDecrease = 1e-3, kMinLmDiagonal = 1e-6, kMaxLmDiagonal = 1e32;
  const double kMaxRadius = 1e16, kMinRadius = 1e-32;
  const int kMaxConsecutiveInvalidSteps = 5;
  const int max_consecutive_nonmonotonic_steps = use_nonmonotonic_steps ? 5 : 0;
  const int K = problem.LocalSize();

  double x[kAmbient];
  for (int a = 0; a < kAmbient; ++a) x[a] = initial[a];
  TrEvaluation<kMaxLocal> at_x;
  if (!problem.Evaluate(x, &at_x) && Problem::kEvaluationCanFail) return false;
  const double initial_cost = at_x.cost;
  double scale[kMaxLocal];
  for (int a = 0; a < K; ++a) scale[a] = 1. / (1. + sqrt(at_x.H[a][a]));
  const auto norm = [](const double* v) {
    double s = 0.;
    for (int a = 0; a < kAmbient; ++a) s += v[a] * v[a];
    return sqrt(s);
  };
  double x_cost = at_x.cost, x_norm = norm(x);
  double radius = 1e4, decrease_factor = 2.;
  bool reuse_diagonal = false;
  double diagonal[kMaxLocal];
  for (int a = 0; a < kMaxLocal; ++a) diagonal[a] = 0.;
  double minimum_cost = x_cost, current_cost = x_cost, reference_cost = x_cost,
         candidate_cost_eval = x_cost;
  double accumulated_reference_model_cost_change = 0., accumulated_candidate_model_cost_change = 0.;
  int num_consecutive_nonmonotonic_steps = 0, num_consecutive_invalid_steps = 0;
  double best_x[kAmbient];
  for (int a = 0; a < kAmbient; ++a) best_x[a] = x[a];
  double best_cost = x_cost;
  int successful = 0, unsuccessful = 0;
  int termination = kTrNoConvergence;
  bool done = problem.GradientMaxNorm(x, at_x) <= kGradientTolerance;
  if (done) termination = kTrConvergence;
  bool last_step_successful = false;
  for (int iteration = 1; !done; ++iteration) {
    if (iteration - 1 >= max_num_iterations) { termination = kTrNoConvergence; break; }
    if (last_step_successful && problem.GradientMaxNorm(x, at_x) <= kGradientTolerance) {
      termination = kTrConvergence;
      break;
    }
    if (radius < kMinRadius) { termination = kTrConvergence; break; }
    last_step_successful = false;

    double Hs[kMaxLocal][kMaxLocal], gs[kMaxLocal];
    for (int a = 0; a < K; ++a) {
      gs[a] = at_x.g[a] * scale[a];
      for (int b = 0; b < K; ++b) Hs[a][b] = at_x.H[a][b] * scale[a] * scale[b];
    }
    if (!reuse_diagonal)
      for (int a = 0; a < K; ++a) diagonal[a] = fmin(fmax(Hs[a][a], kMinLmDiagonal), kMaxLmDiagonal);
    double A[kMaxLocal][kMaxLocal], step[kMaxLocal];
    for (int a = 0; a < K; ++a)
      for (int b = 0; b < K; ++b) A[a][b] = Hs[a][b] + (a == b ? diagonal[a] / radius : 0.);
    const bool solved = SolveSpd<kMaxLocal>(K, A, gs, step);
    for (int a = 0; a < K; ++a) step[a] = -step[a];
    // A dead store (every path to the next ComputeStep sets the flag again), kept so that the
    // loop reads statement for statement like LevenbergMarquardtStrategy::ComputeStep: DESIGN.md.
    reuse_diagonal = true;
    double model_cost_change = 0.;
    if (solved) {
      double sg = 0., sHs = 0.;
      for (int a = 0; a < K; ++a) {
        sg += step[a] * gs[a];
        for (int b = 0; b < K; ++b) sHs += step[a] * Hs[a][b] * step[b];
      }
      model_cost_change = -(sg + 0.5 * sHs);
    }
    if (!solved || !(model_cost_change > 0.)) {
      if (++num_consecutive_invalid_steps >= kMaxConsecutiveInvalidSteps) {
        termination = kTrFailure;
        break;
      }
      radius *= 0.5;
      reuse_diagonal = false;
      ++unsuccessful;
      continue;
    }
    num_consecutive_invalid_steps = 0;
    double delta[kMaxLocal], candidate[kAmbient];
    for (int a = 0; a < K; ++a) delta[a] = step[a] * scale[a];
    problem.Plus(x, delta, candidate);
    // Residuals and Jacobian are evaluated together at every candidate (the Jacobian of a
    // rejected candidate is wasted; a second pass over the points would cost more).
    TrEvaluation<kMaxLocal> at_candidate;
    double candidate_cost;
    if (!problem.Evaluate(candidate, &at_candidate) && Problem::kEvaluationCanFail) {
      candidate_cost = DBL_MAX;
    } else {
      candidate_cost = at_candidate.cost;
    }

    const double step_norm = problem.StepNorm(x, candidate, delta);
    if (step_norm <= kParameterTolerance * (x_norm + kParameterTolerance)) {
      termination = kTrConvergence;
      break;
    }
    const double cost_change = x_cost - candidate_cost;
    if (fabs(cost_change) <= kFunctionTolerance * x_cost) { termination = kTrConvergence; break; }
    const double relative_decrease_now = (current_cost - candidate_cost) / model_cost_change;
    const double historical_relative_decrease =
        (reference_cost - candidate_cost) /
        (accumulated_reference_model_cost_change + model_cost_change);
    // A failed candidate evaluation is never a successful step (StepQuality: lowest()).
    const double relative_decrease =
        Problem::kEvaluationCanFail && candidate_cost >= DBL_MAX
            ? -DBL_MAX
            : fmax(relative_decrease_now, historical_relative_decrease);
    if (relative_decrease > kMinRelativeDecrease) {
      for (int a = 0; a < kAmbient; ++a) x[a] = candidate[a];
      x_norm = norm(x);
      at_x = at_candidate;
      x_cost = candidate_cost;
      last_step_successful = true;
      ++successful;
      if (x_cost < best_cost) {
        best_cost = x_cost;
        for (int a = 0; a < kAmbient; ++a) best_x[a] = x[a];
      }
      radius = radius / fmax(1. / 3., 1. - problem.Cube(2. * relative_decrease - 1.));
      radius = fmin(kMaxRadius, radius);
      decrease_factor = 2.;
      reuse_diagonal = false;
      current_cost = candidate_cost;
      accumulated_candidate_model_cost_change += model_cost_change;
      accumulated_reference_model_cost_change += model_cost_change;
      if (candidate_cost < minimum_cost) {
        minimum_cost = candidate_cost;
        num_consecutive_nonmonotonic_steps = 0;
        candidate_cost_eval = candidate_cost;
        accumulated_candidate_model_cost_change = 0.;
      } else {
        ++num_consecutive_nonmonotonic_steps;
        if (candidate_cost > candidate_cost_eval) {
          candidate_cost_eval = candidate_cost;
          accumulated_candidate_model_cost_change = 0.;
        }
      }
      if (num_consecutive_nonmonotonic_steps == max_consecutive_nonmonotonic_steps) {
        reference_cost = candidate_cost_eval;
        accumulated_reference_model_cost_change = accumulated_candidate_model_cost_change;
      }
    } else {
      radius = radius / decrease_factor;
      decrease_factor *= 2.;
      reuse_diagonal = true;
      ++unsuccessful;
    }
  }
  for (int a = 0; a < kAmbient; ++a) result->x[a] = best_x[a];
  result->initial_cost = initial_cost;
  result->final_cost = best_cost;
  result->successful = successful;
  result->unsuccessful = unsuccessful;
  result->termination = termination;
  return true;
}

#ifdef __HIPCC__
__device__ __forceinline__ double WaveSumF64(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Sums of kCount thread-local numbers over a workgroup of kCeresThreads, valid in every thread:
// across the wavefront with shuffles, across the four wavefronts through `scratch` (LDS) in a
// FIXED order, so that results do not depend on scheduling.  All threads of the workgroup call
// it; `scratch` is free again on return.
template <int kCount>
__device__ __forceinline__ void BlockSumF64(const double* acc, double (*scratch)[kCount],
                                            double* total) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kCount; ++k) {
    const double t = WaveSumF64(acc[k]);
    if ((threadIdx.x & 63) == 0) scratch[wave][k] = t;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kCount; ++k)
    total[k] = ((scratch[0][k] + scratch[1][k]) + scratch[2][k]) + scratch[3][k];
  __syncthreads();
}
#endif  // __HIPCC__

}  // namespace cmx
#endif  // CMX_CERES_TRUST_REGION_H_
