// CeresScanMatcher2D::Match on gfx950: the refinement step that follows
// every correlative match in both callers
//   mapping/internal/2d/local_trajectory_builder_2d.cc:104-107 (after the real-time matcher)
//   mapping/internal/constraints/constraint_builder_2d.cc:245-249 (after the fast matcher)
// so that a constraint no longer leaves HBM between the correlative search and the refined
// pose.
//
// Reference: SM2/ceres_scan_matcher_2d.cc:63-107, SM2/occupied_space_cost_function_2d.cc:39-108
// (bicubic interpolation of the correspondence costs at the transformed points),
// SM2/translation_delta_cost_functor_2d.h:42-47, SM2/rotation_delta_cost_functor_2d.h:42-45.
// The least-squares solver is Ceres (third party, absent from the reference tree): what runs
// here is its published trust-region Levenberg-Marquardt loop with Solver::Options defaults,
// restated the same way as oracle/oracle_ceres_2d.cc (which documents every rule taken from
// Ceres and what pins it).  Three unknowns, so the damped system is a 3 x 3 solve; all the
// work is in the residual blocks.
//
// One workgroup per problem.  Per evaluation every thread takes a few points: the 16
// correspondence costs around the point (uint16 -> f32 table expression -> f64, gathered
// from the grid in HBM / L2), two Catmull-Rom passes, the residual and its three partials,
// accumulated as cost, J^T r and J^T J in f64 (ten numbers per thread), reduced across the
// wavefront with DPP-free shuffles and across the four wavefronts through LDS in a FIXED
// order -- results do not depend on scheduling.  The trust-region logic is the loop shared with
// the 3D kernel (ceres_trust_region.h), its state replicated in every thread.
// Residual + Jacobian are evaluated together at every candidate (the Jacobian of a rejected
// candidate is wasted; evaluating it separately would be a second pass over the points).
//
// On a TSDF2D (the GridType::TSDF case, ceres_scan_matcher_2d.cc:83-90) the point residuals are
// SM2/tsdf_match_cost_function_2d.cc:40-66 over SM2/interpolated_tsdf_2d.h:42-125:
// r_i = n s C_i w_i / S with S = sum_j w_j, so no residual is separable from the others.  One
// pass accumulates, per thread, u_i = n s C_i w_i with its gradient a_i and w_i with its gradient
// g_i: U = sum u^2, A = sum u a, B = sum a a^T, S and G = sum g (14 numbers), reduced in the same
// fixed order.  Then sum r^2 = U / S^2, J^T r = (A - (U / S) G) / S^2 and
// J^T J = (B - (A G^T + G A^T) / S + (U / S^2) G G^T) / S^2.  S == 0 makes the functor return
// false (.cc:61): the evaluation fails, which the trust-region loop treats as the stand-in solver
// does (oracle/ref_shims/ceres/ceres.h: a failed initial evaluation ends the solve with FAILURE,
// a failed candidate costs DBL_MAX and is rejected).
//
// Many trajectories' matches in one call (cmx_ceres2d_match_grid_batch, the Ceres match of
// LocalTrajectoryBuilder2D::ScanMatch for a fleet): Ceres2DJobKernel, one workgroup per job on a
// resident grid of either kind, the upload block laid out by ceres_2d_batch_plan.h.
#include <cfloat>
#include <climits>
#include <cmath>
#include <map>
#include <vector>

#include "../../include/cartographer_mi355x_debug.h"
#include "ceres_2d_batch_plan.h"
#include "ceres_trust_region.h"
#include "scan_matching_2d.h"

struct cmx_grid2d;   // grid_2d.hip
struct cmx_tsdf2d;   // tsdf_2d.hip
namespace cmx {
const uint16_t* Grid2DDeviceCells(const cmx_grid2d* grid, cmx_grid2d_limits* limits, int* device);
// The two planes of a resident TSDF2D; limits carry the cost range [-truncation, truncation].
void Tsdf2DDevicePlanes(const cmx_tsdf2d* grid, cmx_grid2d_limits* limits, const uint16_t** tsd,
                        const uint16_t** weight, float* max_weight, int* device);
}

namespace cmx {
namespace {

constexpr int kPadding = INT_MAX / 4;   // occupied_space_cost_function_2d.cc:78

struct Ceres2DProblem {
  const uint16_t* cells;       // device grid (a TSDF's tsd plane)
  const uint16_t* weights;     // device weight plane of a TSDF (null for a probability grid)
  int nx, ny;
  double res, max_x, max_y;
  float min_cc, max_cc;        // the grid's correspondence cost range (value table)
  float max_weight;            // TSDF: the TSDValueConverter's weight range [0, max_weight]
  const float* xyz;            // device cloud
  int n;
  double init[3];              // initial pose estimate (x, y, theta)
  double target_x, target_y;   // target translation; the target angle is init[2]
  double occupied_scaling;     // occupied_space_weight / sqrt(n)
  double translation_weight, rotation_weight;
  int use_nonmonotonic_steps, max_num_iterations;
  int skip;                    // 1: no search result to refine (found == 0): pass through
  double* out;                 // [8]: pose x, y, theta, initial cost, final cost, successful,
                               //      unsuccessful, termination
};

// Grid2D::GetCorrespondenceCost through the per-grid table of
// mapping/value_conversion_tables.cc:29-51, evaluated arithmetically (same f32 expression).
__device__ __forceinline__ double CellCost(const Ceres2DProblem& P, int ix, int iy) {
  const bool inside = static_cast<unsigned>(ix) < static_cast<unsigned>(P.nx) &&
                      static_cast<unsigned>(iy) < static_cast<unsigned>(P.ny);
  const unsigned v = AsGlobal(P.cells)[inside ? P.nx * iy + ix : 0] & 0x7fffu;
  float cost = P.max_cc;
  if (inside && v != 0) {
    const float scale = (P.max_cc - P.min_cc) / 32766.f;
    cost = static_cast<float>(v) * scale + (P.min_cc - scale);
  }
  return static_cast<double>(cost);
}
// GridArrayAdapter::GetValue: kMaxCorrespondenceCost outside (the constant, not the grid's).
__device__ __forceinline__ double AdapterValue(const Ceres2DProblem& P, int row, int column) {
  const int ix = column - kPadding, iy = row - kPadding;
  const bool inside = static_cast<unsigned>(ix) < static_cast<unsigned>(P.nx) &&
                      static_cast<unsigned>(iy) < static_cast<unsigned>(P.ny);
  const double inner = CellCost(P, ix, iy);
  return inside ? inner : static_cast<double>(1.f - 0.1f);
}

// ceres::CubicHermiteSpline<1>.
__device__ __forceinline__ void Spline(double p0, double p1, double p2, double p3, double x,
                                       double* f, double* dfdx) {
  const double a = 0.5 * (-p0 + 3.0 * p1 - 3.0 * p2 + p3);
  const double b = 0.5 * (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3);
  const double c = 0.5 * (-p0 + p2);
  const double d = p1;
  *f = d + x * (c + x * (b + x * a));
  *dfdx = c + x * (2.0 * b + 3.0 * a * x);
}

// ceres::Jet<double, 3> over the pose (x, y, theta), with the operations of the TSDF cost in
// oracle/ref_shims/ceres/jet.h's order.
struct Jet3 {
  double a, v[3];
};
__device__ __forceinline__ Jet3 JetConst(double a) { return {a, {0., 0., 0.}}; }
__device__ __forceinline__ Jet3 operator+(const Jet3& f, const Jet3& g) {
  return {f.a + g.a, {f.v[0] + g.v[0], f.v[1] + g.v[1], f.v[2] + g.v[2]}};
}
__device__ __forceinline__ Jet3 operator-(const Jet3& f, const Jet3& g) {
  return {f.a - g.a, {f.v[0] - g.v[0], f.v[1] - g.v[1], f.v[2] - g.v[2]}};
}
__device__ __forceinline__ Jet3 operator*(const Jet3& f, const Jet3& g) {
  return {f.a * g.a, {f.a * g.v[0] + f.v[0] * g.a, f.a * g.v[1] + f.v[1] * g.a,
                      f.a * g.v[2] + f.v[2] * g.a}};
}
// f / g for a constant g: (f.v - (f.a / g) * 0) / g, through the inverse as the Jet does.
__device__ __forceinline__ Jet3 DivConst(const Jet3& f, double g) {
  const double inv = 1.0 / g;
  return {f.a * inv, {f.v[0] * inv, f.v[1] * inv, f.v[2] * inv}};
}

// TSDF2D::GetWeight (tsdf_2d.cc:80-86): the TSDValueConverter's weight table over
// [0, max_weight], 0 for unknown and outside cells.
__device__ __forceinline__ float TsdfWeight(const Ceres2DProblem& P, int ix, int iy) {
  const bool inside = static_cast<unsigned>(ix) < static_cast<unsigned>(P.nx) &&
                      static_cast<unsigned>(iy) < static_cast<unsigned>(P.ny);
  const unsigned raw = AsGlobal(P.weights)[inside ? P.nx * iy + ix : 0];
  return inside ? BoundedValue(raw, 0.f, 0.f, P.max_weight) : 0.f;
}

// InterpolatedTSDF2D::InterpolateBilinear (interpolated_tsdf_2d.h:89-98).
__device__ __forceinline__ Jet3 Bilinear(const Jet3& x, const Jet3& y, float x1, float y1,
                                         float x2, float y2, float q11, float q12, float q21,
                                         float q22) {
  const Jet3 nx = DivConst(x - JetConst(static_cast<double>(x1)), static_cast<double>(x2 - x1));
  const Jet3 ny = DivConst(y - JetConst(static_cast<double>(y1)), static_cast<double>(y2 - y1));
  const Jet3 q1 = JetConst(static_cast<double>(q12 - q11)) * ny + JetConst(static_cast<double>(q11));
  const Jet3 q2 = JetConst(static_cast<double>(q22 - q21)) * ny + JetConst(static_cast<double>(q21));
  return (q2 - q1) * nx + q1;
}

// One point of TSDFMatchCostFunction2D::operator() (tsdf_match_cost_function_2d.cc:40-59) at the
// pose whose rotation is (c, s): u = T(n) * scaling * C * w before the division by S, and w.
__device__ __forceinline__ void TsdfPoint(const Ceres2DProblem& P, const double x[3], double c,
                                          double s, double ns, int i, Jet3* u, Jet3* w) {
  const double px = static_cast<double>(P.xyz[3 * i]), py = static_cast<double>(P.xyz[3 * i + 1]);
  const Jet3 wx = {c * px + -s * py + x[0] * 1., {1., 0., -s * px - c * py}};
  const Jet3 wy = {s * px + c * py + x[1] * 1., {0., 1., c * px - s * py}};
  // CenterOfLowerPixel (interpolated_tsdf_2d.h:104-117) on the scalar parts: the point rounded
  // to f32, MapLimits::GetCellIndex in double, GetCellCenter computed in double and stored as
  // f32, compared with the double coordinate, moved down by one resolution in double.
  const float fx = static_cast<float>(wx.a), fy = static_cast<float>(wy.a);
  const int cx_index = LRoundF64((P.max_y - static_cast<double>(fy)) / P.res - 0.5);
  const int cy_index = LRoundF64((P.max_x - static_cast<double>(fx)) / P.res - 0.5);
  float x1 = static_cast<float>(P.max_x - P.res * (cy_index + 0.5));
  float y1 = static_cast<float>(P.max_y - P.res * (cx_index + 0.5));
  if (static_cast<double>(x1) > wx.a) x1 = static_cast<float>(static_cast<double>(x1) - P.res);
  if (static_cast<double>(y1) > wy.a) y1 = static_cast<float>(static_cast<double>(y1) - P.res);
  const float x2 = x1 + static_cast<float>(P.res), y2 = y1 + static_cast<float>(P.res);
  // index1 = GetCellIndex(Vector2f(x1, y1)); neighbours (-1, 0), (0, -1), (-1, -1).
  const int ix = LRoundF64((P.max_y - static_cast<double>(y1)) / P.res - 0.5);
  const int iy = LRoundF64((P.max_x - static_cast<double>(x1)) / P.res - 0.5);
  const float w11 = TsdfWeight(P, ix, iy), w12 = TsdfWeight(P, ix - 1, iy);
  const float w21 = TsdfWeight(P, ix, iy - 1), w22 = TsdfWeight(P, ix - 1, iy - 1);
  *w = Bilinear(wx, wy, x1, y1, x2, y2, w11, w12, w21, w22);
  Jet3 cost = JetConst(static_cast<double>(P.max_cc));
  if (!(w11 == 0.f || w12 == 0.f || w21 == 0.f || w22 == 0.f)) {
    const float q11 = static_cast<float>(CellCost(P, ix, iy));
    const float q12 = static_cast<float>(CellCost(P, ix - 1, iy));
    const float q21 = static_cast<float>(CellCost(P, ix, iy - 1));
    const float q22 = static_cast<float>(CellCost(P, ix - 1, iy - 1));
    cost = Bilinear(wx, wy, x1, y1, x2, y2, q11, q12, q21, q22);
  }
  *u = (JetConst(ns) * cost) * *w;
}

// Per-thread sums of one evaluation.  Probability grid: cost (sum of squares), g = J^T r,
// H = J^T J (upper triangle).  TSDF: U, A (3), B (upper triangle, 6), S, G (3).
template <bool kTsdf>
struct Sums {
  static constexpr int kCount = kTsdf ? 14 : 10;
  double v[kCount];
};

// Residual blocks at `x`: leaves 1/2 |r|^2, J^T r and J^T J (valid in every thread).  False when
// the cost function fails (a TSDF with S == 0); the outputs are then undefined.
template <bool kTsdf>
__device__ bool Evaluate(const Ceres2DProblem& P, const double x[3],
                         double (*scratch)[Sums<kTsdf>::kCount], double* cost, double g[3],
                         double H[3][3]) {
  constexpr int kCount = Sums<kTsdf>::kCount;
  const double c = cos(x[2]), s = sin(x[2]);
  Sums<kTsdf> acc;
#pragma unroll
  for (int k = 0; k < kCount; ++k) acc.v[k] = 0.;
  if constexpr (kTsdf) {
    const double ns = static_cast<double>(P.n) * P.occupied_scaling;
    for (int i = threadIdx.x; i < P.n; i += kCeresThreads) {
      Jet3 u, w;
      TsdfPoint(P, x, c, s, ns, i, &u, &w);
      acc.v[0] += u.a * u.a;
      acc.v[1] += u.a * u.v[0]; acc.v[2] += u.a * u.v[1]; acc.v[3] += u.a * u.v[2];
      acc.v[4] += u.v[0] * u.v[0]; acc.v[5] += u.v[0] * u.v[1]; acc.v[6] += u.v[0] * u.v[2];
      acc.v[7] += u.v[1] * u.v[1]; acc.v[8] += u.v[1] * u.v[2]; acc.v[9] += u.v[2] * u.v[2];
      acc.v[10] += w.a;
      acc.v[11] += w.v[0]; acc.v[12] += w.v[1]; acc.v[13] += w.v[2];
    }
  } else {
    for (int i = threadIdx.x; i < P.n; i += kCeresThreads) {
      const double px = static_cast<double>(P.xyz[3 * i]), py = static_cast<double>(P.xyz[3 * i + 1]);
      const double wx = c * px + -s * py + x[0] * 1.;
      const double wy = s * px + c * py + x[1] * 1.;
      const double r = (P.max_x - wx) / P.res - 0.5 + static_cast<double>(kPadding);
      const double cc = (P.max_y - wy) / P.res - 0.5 + static_cast<double>(kPadding);
      const int row = static_cast<int>(floor(r)), col = static_cast<int>(floor(cc));
      double fr[4], dfr[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int rr = row - 1 + k;
        Spline(AdapterValue(P, rr, col - 1), AdapterValue(P, rr, col), AdapterValue(P, rr, col + 1),
               AdapterValue(P, rr, col + 2), cc - col, &fr[k], &dfr[k]);
      }
      double f, dfdr, dfdc, unused;
      Spline(fr[0], fr[1], fr[2], fr[3], r - row, &f, &dfdr);
      Spline(dfr[0], dfr[1], dfr[2], dfr[3], r - row, &dfdc, &unused);
      const double res_i = P.occupied_scaling * f;
      const double dwx_dt = -s * px - c * py, dwy_dt = c * px - s * py;
      const double j0 = P.occupied_scaling * (dfdr * (-1. / P.res));
      const double j1 = P.occupied_scaling * (dfdc * (-1. / P.res));
      const double j2 = P.occupied_scaling * (dfdr * (-dwx_dt / P.res) + dfdc * (-dwy_dt / P.res));
      acc.v[0] += res_i * res_i;
      acc.v[1] += j0 * res_i; acc.v[2] += j1 * res_i; acc.v[3] += j2 * res_i;
      acc.v[4] += j0 * j0; acc.v[5] += j0 * j1; acc.v[6] += j0 * j2;
      acc.v[7] += j1 * j1; acc.v[8] += j1 * j2; acc.v[9] += j2 * j2;
    }
  }
  double total[kCount];
  BlockSumF64<kCount>(acc.v, scratch, total);
  if constexpr (kTsdf) {
    const double S = total[10];
    if (S == 0.) return false;                      // tsdf_match_cost_function_2d.cc:61
    const double S2 = S * S, U_S = total[0] / S, U_S2 = total[0] / S2;
    const double A[3] = {total[1], total[2], total[3]};
    const double G[3] = {total[11], total[12], total[13]};
    total[0] = U_S2;
    for (int a = 0; a < 3; ++a) total[1 + a] = (A[a] - U_S * G[a]) / S2;
    int k = 4;
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b, ++k)
        total[k] = (total[k] - (A[a] * G[b] + G[a] * A[b]) / S + U_S2 * (G[a] * G[b])) / S2;
  }
  // TranslationDeltaCostFunctor2D / RotationDeltaCostFunctor2D.
  const double rt0 = P.translation_weight * (x[0] - P.target_x);
  const double rt1 = P.translation_weight * (x[1] - P.target_y);
  const double rr = P.rotation_weight * (x[2] - P.init[2]);
  total[0] += rt0 * rt0; total[0] += rt1 * rt1; total[0] += rr * rr;
  total[1] += P.translation_weight * rt0;
  total[2] += P.translation_weight * rt1;
  total[3] += P.rotation_weight * rr;
  total[4] += P.translation_weight * P.translation_weight;
  total[7] += P.translation_weight * P.translation_weight;
  total[9] += P.rotation_weight * P.rotation_weight;
  *cost = 0.5 * total[0];
  g[0] = total[1]; g[1] = total[2]; g[2] = total[3];
  H[0][0] = total[4]; H[0][1] = H[1][0] = total[5]; H[0][2] = H[2][0] = total[6];
  H[1][1] = total[7]; H[1][2] = H[2][1] = total[8]; H[2][2] = total[9];
  return true;
}

// What MinimizeTrustRegion asks of CeresScanMatcher2D's problem: three unknowns without a local
// parameterization.
template <bool kTsdf>
struct Pose2DProblem {
  static constexpr int kAmbient = 3, kMaxLocal = 3;
  // Only a TSDF's evaluation fails (S == 0); on a probability grid Evaluate returns true and the
  // compiler folds the branches away.
  static constexpr bool kEvaluationCanFail = true;
  const Ceres2DProblem& P;
  double (*scratch)[Sums<kTsdf>::kCount];

  __device__ __forceinline__ int LocalSize() const { return 3; }
  __device__ __forceinline__ bool Evaluate(const double* x, TrEvaluation<3>* e) {
    return cmx::Evaluate<kTsdf>(P, x, scratch, &e->cost, e->g, e->H);
  }
  __device__ __forceinline__ void Plus(const double* x, const double* delta, double* out) const {
    for (int a = 0; a < 3; ++a) out[a] = x[a] + delta[a];
  }
  __device__ __forceinline__ double GradientMaxNorm(const double*, const TrEvaluation<3>& e) const {
    return fmax(fabs(e.g[0]), fmax(fabs(e.g[1]), fabs(e.g[2])));
  }
  __device__ __forceinline__ double StepNorm(const double*, const double*, const double* delta) const {
    return sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
  }
  // The radius update's (2 rho - 1)^3 as a product (oracle_ceres_2d.cc takes std::pow; the two
  // agree up to rounding, and the parity tests pin this form).
  __device__ __forceinline__ double Cube(double t) const { return t * t * t; }
};

// One workgroup per problem: the prologue of the entry points (nothing to refine, a failed
// initial evaluation), then the shared trust-region loop.
template <bool kTsdf>
__global__ void __launch_bounds__(kCeresThreads)
Ceres2DKernel(const Ceres2DProblem* __restrict__ problems) {
  const Ceres2DProblem& P = problems[blockIdx.x];
  __shared__ double scratch[4][Sums<kTsdf>::kCount];
  if (P.skip) {
    if (threadIdx.x == 0) {
      P.out[0] = P.init[0]; P.out[1] = P.init[1]; P.out[2] = P.init[2];
      P.out[3] = 0.; P.out[4] = 0.; P.out[5] = 0.; P.out[6] = 0.; P.out[7] = 1.;
    }
    return;
  }
  Pose2DProblem<kTsdf> problem{P, scratch};
  TrResult<3> r;
  if (!MinimizeTrustRegion(problem, P.init, P.use_nonmonotonic_steps != 0, P.max_num_iterations,
                           &r)) {
    // The initial evaluation failed: FAILURE, the pose untouched, and the summary fields keep
    // ceres::Solver::Summary's initial values.
    if (threadIdx.x == 0) {
      P.out[0] = P.init[0]; P.out[1] = P.init[1]; P.out[2] = P.init[2];
      P.out[3] = -1.; P.out[4] = -1.; P.out[5] = -1.; P.out[6] = -1.; P.out[7] = 2.;
    }
    return;
  }
  if (threadIdx.x == 0) {
    P.out[0] = r.x[0]; P.out[1] = r.x[1]; P.out[2] = r.x[2];
    P.out[3] = r.initial_cost; P.out[4] = r.final_cost;
    P.out[5] = r.successful; P.out[6] = r.unsuccessful; P.out[7] = r.termination;
  }
}

// One job of Ceres2DJobKernel on a grid of one kind: Ceres2DKernel's solve and its eight output
// doubles (a job is never skipped).
template <bool kTsdf>
__device__ __forceinline__ void SolveJob(const Ceres2DProblem& P,
                                         double (*scratch)[Sums<kTsdf>::kCount]) {
  Pose2DProblem<kTsdf> problem{P, scratch};
  TrResult<3> r;
  if (!MinimizeTrustRegion(problem, P.init, P.use_nonmonotonic_steps != 0, P.max_num_iterations,
                           &r)) {
    // The initial evaluation failed: FAILURE, as in Ceres2DKernel.
    if (threadIdx.x == 0) {
      P.out[0] = P.init[0]; P.out[1] = P.init[1]; P.out[2] = P.init[2];
      P.out[3] = -1.; P.out[4] = -1.; P.out[5] = -1.; P.out[6] = -1.; P.out[7] = 2.;
    }
    return;
  }
  if (threadIdx.x == 0) {
    P.out[0] = r.x[0]; P.out[1] = r.x[1]; P.out[2] = r.x[2];
    P.out[3] = r.initial_cost; P.out[4] = r.final_cost;
    P.out[5] = r.successful; P.out[6] = r.unsuccessful; P.out[7] = r.termination;
  }
}

// cmx_ceres2d_match_grid_batch: one workgroup per job, probability grids and TSDFs in one launch.
// A problem with a weight plane is a TSDF's.  The branch is taken by the whole workgroup alike (it
// depends on blockIdx.x only), so the barriers of BlockSumF64 inside either solve are met by all of
// its threads; each side is the code of Ceres2DKernel<kTsdf> with the same thread count and the
// same order of sums, so a job's result is that of its single call.  One LDS block serves both:
// it is sized for the TSDF's 4 x 14 partial sums, a probability grid uses 4 x 10 of it.
__global__ void __launch_bounds__(kCeresThreads)
Ceres2DJobKernel(const Ceres2DProblem* __restrict__ problems) {
  const Ceres2DProblem& P = problems[blockIdx.x];
  __shared__ double scratch[4 * Sums<true>::kCount];
  static_assert(Sums<true>::kCount >= Sums<false>::kCount, "the block is sized for the TSDF sums");
  if (P.weights != nullptr) {
    SolveJob<true>(P, reinterpret_cast<double (*)[Sums<true>::kCount]>(scratch));
  } else {
    SolveJob<false>(P, reinterpret_cast<double (*)[Sums<false>::kCount]>(scratch));
  }
}

// Residuals and Jacobian of TSDFMatchCostFunction2D alone (cmx_ceres2d_tsdf_residuals): S and G
// first, then per point r = u / S and J = (a - r G) / S as the Jet division forms them.
__global__ void __launch_bounds__(kCeresThreads)
TsdfResidualsKernel(const Ceres2DProblem* __restrict__ problem) {
  const Ceres2DProblem& P = *problem;
  __shared__ double scratch[4][4];
  const double x[3] = {P.init[0], P.init[1], P.init[2]};
  const double c = cos(x[2]), s = sin(x[2]);
  const double ns = static_cast<double>(P.n) * P.occupied_scaling;
  double acc[4] = {0., 0., 0., 0.};
  for (int i = threadIdx.x; i < P.n; i += kCeresThreads) {
    Jet3 u, w;
    TsdfPoint(P, x, c, s, ns, i, &u, &w);
    acc[0] += w.a; acc[1] += w.v[0]; acc[2] += w.v[1]; acc[3] += w.v[2];
  }
  double total[4];
  BlockSumF64<4>(acc, scratch, total);
  // out: [0] valid, [1, 1 + n) residuals, [1 + n, 1 + 4n) Jacobian rows.
  if (threadIdx.x == 0) P.out[0] = total[0] == 0. ? 0. : 1.;
  if (total[0] == 0.) return;
  const double inv = 1.0 / total[0];
  for (int i = threadIdx.x; i < P.n; i += kCeresThreads) {
    Jet3 u, w;
    TsdfPoint(P, x, c, s, ns, i, &u, &w);
    const double r = u.a * inv;
    P.out[1 + i] = r;
    for (int k = 0; k < 3; ++k) P.out[1 + P.n + 3 * i + k] = (u.v[k] - r * total[1 + k]) * inv;
  }
}

struct RefineItem {
  const uint16_t* device_cells;     // grid already in HBM, or null with host_cells
  const uint16_t* host_cells;
  const uint16_t* device_weights;   // TSDF: weight plane in HBM, or null with host_weights
  const uint16_t* host_weights;
  int tsdf;                         // 1: TSDF2D (cells = tsd plane, limits' cost range = +-truncation)
  float max_weight;
  cmx_grid2d_limits limits;
  double target[2];
  cmx_pose2d initial;
  int skip;
  // The item's cloud: in HBM already (device_xyz), or staged with the call (host_xyz; items that
  // name the same host array share one staged copy).
  const float* host_xyz;
  const float* device_xyz;
  int n;
};

void CheckOptions(const cmx_ceres2d_options* o) {
  // CHECK_GT at ceres_scan_matcher_2d.cc:73,91,96; CreateCeresSolverOptionsProto's CHECK_GT.
  CMX_REQUIRE(o != nullptr, "null options");
  CMX_REQUIRE(o->occupied_space_weight > 0. && o->translation_weight > 0. &&
                  o->rotation_weight > 0.,
              "occupied_space / translation / rotation weights must be > 0");
  CMX_REQUIRE(o->max_num_iterations > 0, "max_num_iterations must be > 0");
}

// What the options and the item decide of a problem; where its grid, its cloud and its result
// lie is the caller's to add.
void FillProblem(const cmx_ceres2d_options* options, const RefineItem& it, Ceres2DProblem* problem) {
  Ceres2DProblem& P = *problem;
  P.max_weight = it.max_weight;
  P.nx = it.limits.num_x_cells; P.ny = it.limits.num_y_cells;
  P.res = it.limits.resolution; P.max_x = it.limits.max_x; P.max_y = it.limits.max_y;
  P.min_cc = it.limits.min_correspondence_cost; P.max_cc = it.limits.max_correspondence_cost;
  P.n = it.n;
  P.init[0] = it.initial.x; P.init[1] = it.initial.y; P.init[2] = it.initial.theta;
  P.target_x = it.target[0]; P.target_y = it.target[1];
  P.occupied_scaling = options->occupied_space_weight / std::sqrt(static_cast<double>(it.n));
  P.translation_weight = options->translation_weight;
  P.rotation_weight = options->rotation_weight;
  P.use_nonmonotonic_steps = options->use_nonmonotonic_steps ? 1 : 0;
  P.max_num_iterations = options->max_num_iterations;
  P.skip = it.skip;
}

// The eight doubles every problem leaves, as poses and summaries.
void UnpackResults(const double* h_out, int num, cmx_pose2d* poses, cmx_ceres_summary* summaries) {
  for (int p = 0; p < num; ++p) {
    const double* o = h_out + 8 * static_cast<size_t>(p);
    poses[p].x = o[0]; poses[p].y = o[1]; poses[p].theta = o[2];
    if (summaries) {
      summaries[p].initial_cost = o[3];
      summaries[p].final_cost = o[4];
      summaries[p].num_successful_steps = static_cast<int32_t>(o[5]);
      summaries[p].num_unsuccessful_steps = static_cast<int32_t>(o[6]);
      summaries[p].termination = static_cast<int32_t>(o[7]);
      summaries[p].reserved = 0;
    }
  }
}

// One launch, one result copy and one synchronisation for `num` problems, each with the cloud
// its item names: the one-cloud entry points are the case of all items naming the same array.
void RefineBatch(const cmx_ceres2d_options* options, const RefineItem* items, int num, int device,
                 cmx_pose2d* poses, cmx_ceres_summary* summaries) {
  CheckOptions(options);
  CMX_REQUIRE(items && num >= 1 && poses, "null argument");
  const bool tsdf = items[0].tsdf != 0;
  // Staging: problems | distinct host clouds | host grids.
  const auto align = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
  size_t bytes = align(sizeof(Ceres2DProblem) * num);
  struct Staged { size_t offset; int n; };
  std::map<const float*, Staged> staged;
  std::vector<size_t> off_xyz(num, bytes);
  for (int p = 0; p < num; ++p) {
    const RefineItem& it = items[p];
    // A TSDF takes an empty cloud: S == 0 then fails the initial evaluation, as in the reference.
    CMX_REQUIRE((it.host_xyz != nullptr || it.device_xyz != nullptr || (tsdf && it.n == 0)) &&
                    it.n >= (tsdf ? 0 : 1) && it.n <= (1 << 24),
                "bad point cloud");
    if (it.device_xyz || it.n == 0) continue;
    const auto seen = staged.emplace(it.host_xyz, Staged{bytes, it.n});
    CMX_REQUIRE(seen.first->second.n == it.n,
                "entry %d names a cloud of an earlier entry with another num_points (%d, there %d)",
                p, it.n, seen.first->second.n);
    off_xyz[p] = seen.first->second.offset;
    if (seen.second) bytes += align(12 * static_cast<size_t>(it.n));
  }
  WorkspaceLease ws(device);
  std::vector<size_t> off_cells(num, 0), off_weights(num, 0);
  for (int p = 0; p < num; ++p) {
    const cmx_grid2d_limits& lim = items[p].limits;
    CMX_REQUIRE(lim.resolution > 0. && lim.num_x_cells >= 1 && lim.num_y_cells >= 1,
                "bad map limits");
    CMX_REQUIRE(items[p].device_cells || items[p].host_cells, "null grid");
    CMX_REQUIRE((items[p].tsdf != 0) == tsdf, "mixed grid types in one batch");
    if (tsdf) {
      CMX_REQUIRE(lim.max_correspondence_cost > 0.f && items[p].max_weight > 0.f,
                  "bad TSDF ranges");
      CMX_REQUIRE(items[p].device_weights || items[p].host_weights, "null weight plane");
    }
    const size_t plane = align(2 * static_cast<size_t>(lim.num_x_cells) * lim.num_y_cells);
    if (!items[p].device_cells) {
      off_cells[p] = bytes;
      bytes += plane;
    }
    if (tsdf && !items[p].device_weights) {
      off_weights[p] = bytes;
      bytes += plane;
    }
  }
  char* h_in = ws->pinned[0].ReserveAs<char>(bytes);
  char* d_in = ws->dev[0].ReserveAs<char>(bytes);
  double* d_out = ws->dev[1].ReserveAs<double>(8 * static_cast<size_t>(num));
  double* h_out = ws->pinned[1].ReserveAs<double>(8 * static_cast<size_t>(num));
  for (const auto& cloud : staged)
    std::memcpy(h_in + cloud.second.offset, cloud.first, 12 * static_cast<size_t>(cloud.second.n));
  Ceres2DProblem* h_prob = reinterpret_cast<Ceres2DProblem*>(h_in);
  for (int p = 0; p < num; ++p) {
    const RefineItem& it = items[p];
    Ceres2DProblem P{};
    if (it.device_cells) {
      P.cells = it.device_cells;
    } else {
      std::memcpy(h_in + off_cells[p], it.host_cells,
                  2 * static_cast<size_t>(it.limits.num_x_cells) * it.limits.num_y_cells);
      P.cells = reinterpret_cast<const uint16_t*>(d_in + off_cells[p]);
    }
    if (tsdf && it.device_weights) {
      P.weights = it.device_weights;
    } else if (tsdf) {
      std::memcpy(h_in + off_weights[p], it.host_weights,
                  2 * static_cast<size_t>(it.limits.num_x_cells) * it.limits.num_y_cells);
      P.weights = reinterpret_cast<const uint16_t*>(d_in + off_weights[p]);
    }
    FillProblem(options, it, &P);
    P.xyz = it.device_xyz ? it.device_xyz : reinterpret_cast<const float*>(d_in + off_xyz[p]);
    P.out = d_out + 8 * static_cast<size_t>(p);
    h_prob[p] = P;
  }
  SmallCopyAsync(d_in, h_in, bytes, /*to_device=*/true, ws->stream);
  const Ceres2DProblem* d_prob = reinterpret_cast<const Ceres2DProblem*>(d_in);
  if (tsdf) {
    Ceres2DKernel<true><<<num, kCeresThreads, 0, ws->stream>>>(d_prob);
  } else {
    Ceres2DKernel<false><<<num, kCeresThreads, 0, ws->stream>>>(d_prob);
  }
  CMX_HIP(hipGetLastError());
  SmallCopyAsync(h_out, d_out, 64 * static_cast<size_t>(num), /*to_device=*/false, ws->stream);
  CMX_HIP(hipStreamSynchronize(ws->stream));
  UnpackResults(h_out, num, poses, summaries);
}

// A host TSDF2D's item: the planes are uploaded with the call.
RefineItem HostTsdfItem(const cmx_grid2d_limits* limits, const uint16_t* tsd_cells,
                        const uint16_t* weight_cells, float truncation_distance,
                        float max_weight) {
  CMX_REQUIRE(limits && tsd_cells && weight_cells, "null argument");
  CMX_REQUIRE(truncation_distance > 0.f && max_weight > 0.f, "bad TSDF ranges");
  CMX_REQUIRE(limits->resolution > 0. && limits->num_x_cells >= 1 && limits->num_y_cells >= 1,
              "bad map limits");
  RefineItem item{};
  item.host_cells = tsd_cells;
  item.host_weights = weight_cells;
  item.tsdf = 1;
  item.max_weight = max_weight;
  item.limits = *limits;
  // Grid2D(limits, -truncation_distance, truncation_distance) (tsdf_2d.cc:25-26)
  item.limits.min_correspondence_cost = -truncation_distance;
  item.limits.max_correspondence_cost = truncation_distance;
  return item;
}

// A resident TSDF2D's item: the planes are read where they lie.
RefineItem ResidentTsdfItem(const cmx_tsdf2d* grid, int* device) {
  CMX_REQUIRE(grid, "null grid");
  RefineItem item{};
  item.tsdf = 1;
  Tsdf2DDevicePlanes(grid, &item.limits, &item.device_cells, &item.device_weights,
                     &item.max_weight, device);
  return item;
}

void TsdfResiduals(const RefineItem& it, double scaling, const double pose[3],
                   const float* host_xyz, int n, int device, double* residuals,
                   double* jacobian, int32_t* valid) {
  CMX_REQUIRE(pose && valid && n >= 0 && n <= (1 << 24), "bad argument");
  CMX_REQUIRE(n == 0 || (host_xyz && residuals && jacobian), "null argument");
  const cmx_grid2d_limits& lim = it.limits;
  CMX_REQUIRE(lim.resolution > 0. && lim.num_x_cells >= 1 && lim.num_y_cells >= 1,
              "bad map limits");
  WorkspaceLease ws(device);
  const auto align = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
  const size_t plane = align(2 * static_cast<size_t>(lim.num_x_cells) * lim.num_y_cells);
  const size_t off_xyz = align(sizeof(Ceres2DProblem));
  const size_t off_cells = off_xyz + align(12 * static_cast<size_t>(n));
  const size_t bytes = off_cells + 2 * plane;
  const size_t out_count = 1 + 4 * static_cast<size_t>(n);
  char* h_in = ws->pinned[0].ReserveAs<char>(bytes);
  char* d_in = ws->dev[0].ReserveAs<char>(bytes);
  double* d_out = ws->dev[1].ReserveAs<double>(out_count);
  double* h_out = ws->pinned[1].ReserveAs<double>(out_count);
  if (n > 0) std::memcpy(h_in + off_xyz, host_xyz, 12 * static_cast<size_t>(n));
  const size_t cell_bytes = 2 * static_cast<size_t>(lim.num_x_cells) * lim.num_y_cells;
  std::memcpy(h_in + off_cells, it.host_cells, cell_bytes);
  std::memcpy(h_in + off_cells + plane, it.host_weights, cell_bytes);
  Ceres2DProblem P{};
  P.cells = reinterpret_cast<const uint16_t*>(d_in + off_cells);
  P.weights = reinterpret_cast<const uint16_t*>(d_in + off_cells + plane);
  P.nx = lim.num_x_cells; P.ny = lim.num_y_cells;
  P.res = lim.resolution; P.max_x = lim.max_x; P.max_y = lim.max_y;
  P.min_cc = lim.min_correspondence_cost; P.max_cc = lim.max_correspondence_cost;
  P.max_weight = it.max_weight;
  P.xyz = reinterpret_cast<const float*>(d_in + off_xyz);
  P.n = n;
  P.init[0] = pose[0]; P.init[1] = pose[1]; P.init[2] = pose[2];
  P.occupied_scaling = scaling;
  P.out = d_out;
  std::memcpy(h_in, &P, sizeof(P));
  SmallCopyAsync(d_in, h_in, bytes, /*to_device=*/true, ws->stream);
  TsdfResidualsKernel<<<1, kCeresThreads, 0, ws->stream>>>(
      reinterpret_cast<const Ceres2DProblem*>(d_in));
  CMX_HIP(hipGetLastError());
  SmallCopyAsync(h_out, d_out, 8 * out_count, /*to_device=*/false, ws->stream);
  CMX_HIP(hipStreamSynchronize(ws->stream));
  *valid = h_out[0] != 0. ? 1 : 0;
  if (*valid) {
    std::memcpy(residuals, h_out + 1, 8 * static_cast<size_t>(n));
    std::memcpy(jacobian, h_out + 1 + n, 24 * static_cast<size_t>(n));
  }
}

}  // namespace
}  // namespace cmx

using cmx::Guard;

extern "C" {

cmx_status cmx_ceres2d_match(const cmx_ceres2d_options* options, const cmx_grid2d_limits* limits,
                             const uint16_t* cells, const double* target_translation_xy,
                             const cmx_pose2d* initial_pose_estimate, const float* point_cloud_xyz,
                             int32_t num_points, int32_t device, cmx_pose2d* pose_estimate,
                             cmx_ceres_summary* summary) {
  return Guard([&] {
    CMX_REQUIRE(limits && cells && target_translation_xy && initial_pose_estimate && pose_estimate,
                "null argument");
    cmx::RefineItem item{};
    item.host_cells = cells;
    item.limits = *limits;
    item.target[0] = target_translation_xy[0];
    item.target[1] = target_translation_xy[1];
    item.initial = *initial_pose_estimate;
    item.host_xyz = point_cloud_xyz;
    item.n = num_points;
    cmx::RefineBatch(options, &item, 1, device, pose_estimate, summary);
  });
}

cmx_status cmx_ceres2d_match_grid(const cmx_ceres2d_options* options, const cmx_grid2d* grid,
                                  const double* target_translation_xy,
                                  const cmx_pose2d* initial_pose_estimate,
                                  const float* point_cloud_xyz, int32_t num_points,
                                  cmx_pose2d* pose_estimate, cmx_ceres_summary* summary) {
  return Guard([&] {
    CMX_REQUIRE(grid && target_translation_xy && initial_pose_estimate && pose_estimate,
                "null argument");
    cmx::RefineItem item{};
    int device = 0;
    item.device_cells = cmx::Grid2DDeviceCells(grid, &item.limits, &device);
    item.target[0] = target_translation_xy[0];
    item.target[1] = target_translation_xy[1];
    item.initial = *initial_pose_estimate;
    item.host_xyz = point_cloud_xyz;
    item.n = num_points;
    cmx::RefineBatch(options, &item, 1, device, pose_estimate, summary);
  });
}

cmx_status cmx_fast2d_refine_batch(const cmx_ceres2d_options* options,
                                   const cmx_fast2d* const* matchers, int32_t num_matchers,
                                   const int32_t* found, const cmx_pose2d* pose_estimates_in,
                                   const float* point_cloud_xyz, int32_t num_points,
                                   cmx_pose2d* pose_estimates_out, cmx_ceres_summary* summaries) {
  return Guard([&] {
    CMX_REQUIRE(matchers && num_matchers >= 1 && pose_estimates_in && pose_estimates_out,
                "null argument");
    // Entries are grouped by the device their grid lives on (a node's batch may span the GPUs of
    // a cmx_comm); every group is one launch.
    std::map<int, std::vector<int>> by_device;
    for (int p = 0; p < num_matchers; ++p) {
      CMX_REQUIRE(matchers[p] && matchers[p]->impl, "null matcher handle");
      by_device[matchers[p]->impl->device()].push_back(p);
    }
    for (const auto& group : by_device) {
      const std::vector<int>& idx = group.second;
      const int m = static_cast<int>(idx.size());
      std::vector<cmx::RefineItem> items(m);
      for (int k = 0; k < m; ++k) {
        const int p = idx[k];
        const cmx::Fast2DMatcher& matcher = *matchers[p]->impl;
        cmx::RefineItem& it = items[k];
        it.device_cells = matcher.grid_cells();
        it.limits = matcher.limits();
        // constraint_builder_2d.cc:245-249: Match(pose_estimate.translation(), pose_estimate, ...)
        it.initial = pose_estimates_in[p];
        it.target[0] = pose_estimates_in[p].x;
        it.target[1] = pose_estimates_in[p].y;
        it.skip = found && !found[p] ? 1 : 0;
        it.host_xyz = point_cloud_xyz;
        it.n = num_points;
      }
      std::vector<cmx_pose2d> poses(m);
      std::vector<cmx_ceres_summary> sums(m);
      cmx::RefineBatch(options, items.data(), m, group.first, poses.data(),
                       summaries ? sums.data() : nullptr);
      for (int k = 0; k < m; ++k) {
        pose_estimates_out[idx[k]] = poses[k];
        if (summaries) summaries[idx[k]] = sums[k];
      }
    }
  });
}

cmx_status cmx_ceres2d_match_tsdf(const cmx_ceres2d_options* options,
                                  const cmx_grid2d_limits* limits, const uint16_t* tsd_cells,
                                  const uint16_t* weight_cells, float truncation_distance,
                                  float max_weight, const double* target_translation_xy,
                                  const cmx_pose2d* initial_pose_estimate,
                                  const float* point_cloud_xyz, int32_t num_points, int32_t device,
                                  cmx_pose2d* pose_estimate, cmx_ceres_summary* summary) {
  return Guard([&] {
    CMX_REQUIRE(target_translation_xy && initial_pose_estimate && pose_estimate, "null argument");
    cmx::RefineItem item = cmx::HostTsdfItem(limits, tsd_cells, weight_cells, truncation_distance,
                                             max_weight);
    item.target[0] = target_translation_xy[0];
    item.target[1] = target_translation_xy[1];
    item.initial = *initial_pose_estimate;
    item.host_xyz = point_cloud_xyz;
    item.n = num_points;
    cmx::RefineBatch(options, &item, 1, device, pose_estimate, summary);
  });
}

cmx_status cmx_ceres2d_match_tsdf_grid(const cmx_ceres2d_options* options, const cmx_tsdf2d* grid,
                                       const double* target_translation_xy,
                                       const cmx_pose2d* initial_pose_estimate,
                                       const float* point_cloud_xyz, int32_t num_points,
                                       cmx_pose2d* pose_estimate, cmx_ceres_summary* summary) {
  return Guard([&] {
    CMX_REQUIRE(grid && target_translation_xy && initial_pose_estimate && pose_estimate,
                "null argument");
    int device = 0;
    cmx::RefineItem item = cmx::ResidentTsdfItem(grid, &device);
    item.target[0] = target_translation_xy[0];
    item.target[1] = target_translation_xy[1];
    item.initial = *initial_pose_estimate;
    item.host_xyz = point_cloud_xyz;
    item.n = num_points;
    cmx::RefineBatch(options, &item, 1, device, pose_estimate, summary);
  });
}

cmx_status cmx_ceres2d_refine_batch_tsdf(const cmx_ceres2d_options* options,
                                         const cmx_tsdf2d* const* grids, int32_t num_grids,
                                         const int32_t* found,
                                         const cmx_pose2d* pose_estimates_in,
                                         const float* point_cloud_xyz, int32_t num_points,
                                         cmx_pose2d* pose_estimates_out,
                                         cmx_ceres_summary* summaries) {
  return Guard([&] {
    CMX_REQUIRE(grids && num_grids >= 1 && pose_estimates_in && pose_estimates_out,
                "null argument");
    // As cmx_fast2d_refine_batch: one launch per device the grids live on.
    std::map<int, std::vector<int>> by_device;
    std::vector<cmx::RefineItem> all(num_grids);
    for (int p = 0; p < num_grids; ++p) {
      CMX_REQUIRE(grids[p], "null grid handle");
      int device = 0;
      all[p] = cmx::ResidentTsdfItem(grids[p], &device);
      by_device[device].push_back(p);
    }
    for (const auto& group : by_device) {
      const std::vector<int>& idx = group.second;
      const int m = static_cast<int>(idx.size());
      std::vector<cmx::RefineItem> items(m);
      for (int k = 0; k < m; ++k) {
        const int p = idx[k];
        cmx::RefineItem& it = items[k];
        it = all[p];
        // constraint_builder_2d.cc:245-249: Match(pose_estimate.translation(), pose_estimate, ...)
        it.initial = pose_estimates_in[p];
        it.target[0] = pose_estimates_in[p].x;
        it.target[1] = pose_estimates_in[p].y;
        it.skip = found && !found[p] ? 1 : 0;
        it.host_xyz = point_cloud_xyz;
        it.n = num_points;
      }
      std::vector<cmx_pose2d> poses(m);
      std::vector<cmx_ceres_summary> sums(m);
      cmx::RefineBatch(options, items.data(), m, group.first, poses.data(),
                       summaries ? sums.data() : nullptr);
      for (int k = 0; k < m; ++k) {
        pose_estimates_out[idx[k]] = poses[k];
        if (summaries) summaries[idx[k]] = sums[k];
      }
    }
  });
}

}  // extern "C"

namespace cmx {
namespace {

// The refinement of a list of (node, submap) pairs: `items` carry grid and cloud of every pair,
// all on `device`; one RefineBatch, hence one launch, for the whole list.
void RefinePairs(const cmx_ceres2d_options* options, std::vector<RefineItem>* items, int device,
                 const int32_t* found, const cmx_pose2d* pose_estimates_in,
                 cmx_pose2d* pose_estimates_out, cmx_ceres_summary* summaries) {
  CMX_REQUIRE(pose_estimates_in && pose_estimates_out, "null argument");
  const int num = static_cast<int>(items->size());
  for (int p = 0; p < num; ++p) {
    RefineItem& it = (*items)[p];
    // constraint_builder_2d.cc:245-249: Match(pose_estimate.translation(), pose_estimate, ...)
    it.initial = pose_estimates_in[p];
    it.target[0] = pose_estimates_in[p].x;
    it.target[1] = pose_estimates_in[p].y;
    it.skip = found && !found[p] ? 1 : 0;
  }
  RefineBatch(options, items->data(), num, device, pose_estimates_out, summaries);
}

// The matcher's own copy of its grid as the item of pair p; all matchers on one device.
std::vector<RefineItem> MatcherItems(const cmx_fast2d* const* matchers, int num_pairs,
                                     int* device) {
  CMX_REQUIRE(matchers != nullptr, "null argument");
  std::vector<RefineItem> items(num_pairs);
  for (int p = 0; p < num_pairs; ++p) {
    CMX_REQUIRE(matchers[p] && matchers[p]->impl, "null matcher handle (pair %d)", p);
    const Fast2DMatcher& matcher = *matchers[p]->impl;
    if (p == 0) *device = matcher.device();
    CMX_REQUIRE(matcher.device() == *device,
                "the matchers of a call must live on one device (pair %d)", p);
    items[p].device_cells = matcher.grid_cells();
    items[p].limits = matcher.limits();
  }
  return items;
}

}  // namespace
}  // namespace cmx

extern "C" {

cmx_status cmx_fast2d_refine_pairs(const cmx_ceres2d_options* options,
                                   const cmx_fast2d* const* matchers, int32_t num_pairs,
                                   const int32_t* found, const cmx_pose2d* pose_estimates_in,
                                   const float* const* point_clouds_xyz,
                                   const int32_t* num_points, cmx_pose2d* pose_estimates_out,
                                   cmx_ceres_summary* summaries) {
  return Guard([&] {
    // (a matcher handle cannot exist without a device: say so, whatever the arguments are)
    if (cmx_device_count() <= 0) cmx::UseDevice(0);
    CMX_REQUIRE(num_pairs >= 1, "num_pairs must be at least 1");
    CMX_REQUIRE(point_clouds_xyz && num_points, "null argument");
    int device = 0;
    std::vector<cmx::RefineItem> items = cmx::MatcherItems(matchers, num_pairs, &device);
    for (int p = 0; p < num_pairs; ++p) {
      CMX_REQUIRE(point_clouds_xyz[p] != nullptr, "the point cloud of pair %d is null", p);
      items[p].host_xyz = point_clouds_xyz[p];
      items[p].n = num_points[p];
    }
    cmx::RefinePairs(options, &items, device, found, pose_estimates_in, pose_estimates_out,
                     summaries);
  });
}

cmx_status cmx_fast2d_refine_pairs_resident(const cmx_ceres2d_options* options,
                                            const cmx_fast2d* const* matchers, int32_t num_pairs,
                                            const int32_t* found,
                                            const cmx_pose2d* pose_estimates_in,
                                            const cmx_cloud* const* clouds,
                                            cmx_pose2d* pose_estimates_out,
                                            cmx_ceres_summary* summaries) {
  return Guard([&] {
    if (cmx_device_count() <= 0) cmx::UseDevice(0);
    CMX_REQUIRE(num_pairs >= 1, "num_pairs must be at least 1");
    CMX_REQUIRE(clouds != nullptr, "null argument");
    int device = 0;
    std::vector<cmx::RefineItem> items = cmx::MatcherItems(matchers, num_pairs, &device);
    for (int p = 0; p < num_pairs; ++p) {
      CMX_REQUIRE(clouds[p] != nullptr, "the point cloud of pair %d is null", p);
      CMX_REQUIRE(clouds[p]->device == device,
                  "cloud and matcher are on different devices (pair %d)", p);
      items[p].device_xyz = clouds[p]->xyz;
      items[p].n = clouds[p]->num_points;
    }
    cmx::RefinePairs(options, &items, device, found, pose_estimates_in, pose_estimates_out,
                     summaries);
  });
}

cmx_status cmx_ceres2d_refine_pairs_tsdf(const cmx_ceres2d_options* options,
                                         const cmx_tsdf2d* const* grids, int32_t num_pairs,
                                         const int32_t* found,
                                         const cmx_pose2d* pose_estimates_in,
                                         const float* const* point_clouds_xyz,
                                         const int32_t* num_points,
                                         cmx_pose2d* pose_estimates_out,
                                         cmx_ceres_summary* summaries) {
  return Guard([&] {
    if (cmx_device_count() <= 0) cmx::UseDevice(0);
    CMX_REQUIRE(num_pairs >= 1, "num_pairs must be at least 1");
    CMX_REQUIRE(grids && point_clouds_xyz && num_points, "null argument");
    int device = 0;
    std::vector<cmx::RefineItem> items(num_pairs);
    for (int p = 0; p < num_pairs; ++p) {
      CMX_REQUIRE(grids[p] != nullptr, "null grid handle (pair %d)", p);
      int device_p = 0;
      items[p] = cmx::ResidentTsdfItem(grids[p], &device_p);
      if (p == 0) device = device_p;
      CMX_REQUIRE(device_p == device, "the grids of a call must live on one device (pair %d)", p);
      // (an empty cloud is accepted, as by cmx_ceres2d_refine_batch_tsdf: FAILURE, pose untouched)
      CMX_REQUIRE(point_clouds_xyz[p] != nullptr || num_points[p] == 0,
                  "the point cloud of pair %d is null", p);
      items[p].host_xyz = point_clouds_xyz[p];
      items[p].n = num_points[p];
    }
    cmx::RefinePairs(options, &items, device, found, pose_estimates_in, pose_estimates_out,
                     summaries);
  });
}

cmx_status cmx_ceres2d_tsdf_residuals(const cmx_grid2d_limits* limits, const uint16_t* tsd_cells,
                                      const uint16_t* weight_cells, float truncation_distance,
                                      float max_weight, double residual_scaling_factor,
                                      const double* pose, const float* point_cloud_xyz,
                                      int32_t num_points, int32_t device, double* residuals,
                                      double* jacobian, int32_t* valid) {
  return Guard([&] {
    const cmx::RefineItem item = cmx::HostTsdfItem(limits, tsd_cells, weight_cells,
                                                   truncation_distance, max_weight);
    cmx::TsdfResiduals(item, residual_scaling_factor, pose, point_cloud_xyz, num_points, device,
                       residuals, jacobian, valid);
  });
}

}  // extern "C"

// ---- many trajectories' matches on resident grids: cmx_ceres2d_match_grid_batch -------------
namespace cmx {
namespace {

void CheckJobShapes(const std::vector<Ceres2DJobShape>& shapes) {
  CheckCeres2DJobShapes(shapes.data(), static_cast<int>(shapes.size()),
                        [](int job, const char* what) { CMX_REQUIRE(false, "job %d: %s", job, what); });
}

// The jobs of a call as items on one device, after every check of the contract; nothing here
// touches the device.  (A handle's limits and TSDF ranges were checked when it was created.)
std::vector<RefineItem> JobItems(const cmx_ceres2d_job* jobs, int num,
                                 std::vector<Ceres2DJobShape>* shapes, int* device) {
  shapes->resize(num);
  for (int k = 0; k < num; ++k) {
    const cmx_ceres2d_job& J = jobs[k];
    CMX_REQUIRE(J.grid || J.tsdf, "job %d: neither grid nor tsdf is set", k);
    CMX_REQUIRE(!(J.grid && J.tsdf), "job %d: both grid and tsdf are set", k);
    CMX_REQUIRE(J.reserved == 0, "job %d: reserved must be 0", k);
    Ceres2DJobShape& S = (*shapes)[k];
    S.kind = J.tsdf ? kCeres2DTsdf : kCeres2DProbabilityGrid;
    S.host_xyz = J.point_cloud_xyz;
    S.resident = J.cloud != nullptr;
    S.num_points = J.num_points;
    if (J.cloud && !J.point_cloud_xyz) {
      CMX_REQUIRE(J.num_points == 0 || J.num_points == J.cloud->num_points,
                  "job %d: num_points (%d) is neither 0 nor the count of its cloud (%d)", k,
                  J.num_points, J.cloud->num_points);
      S.num_points = J.cloud->num_points;
    }
  }
  CheckJobShapes(*shapes);
  std::vector<RefineItem> items(num);
  for (int k = 0; k < num; ++k) {
    const cmx_ceres2d_job& J = jobs[k];
    RefineItem& it = items[k];
    int device_k = 0;
    if (J.tsdf) {
      it = ResidentTsdfItem(J.tsdf, &device_k);
    } else {
      it.device_cells = Grid2DDeviceCells(J.grid, &it.limits, &device_k);
    }
    if (k == 0) *device = device_k;
    CMX_REQUIRE(device_k == *device, "job %d: its grid is on device %d, the grid of job 0 on %d", k,
                device_k, *device);
    if (J.cloud) {
      CMX_REQUIRE(J.cloud->device == *device,
                  "job %d: its cloud is on device %d, the grid of job 0 on %d", k, J.cloud->device,
                  *device);
      it.device_xyz = J.cloud->xyz;
    } else {
      it.host_xyz = J.point_cloud_xyz;
    }
    it.n = (*shapes)[k].num_points;
    it.target[0] = J.target_translation_xy[0];
    it.target[1] = J.target_translation_xy[1];
    it.initial = J.initial_pose_estimate;
  }
  return items;
}

// One upload block laid out by the plan (problems | distinct host clouds), one launch of
// Ceres2DJobKernel, one result copy and one synchronisation.
void RunJobs(const cmx_ceres2d_options* options, const std::vector<RefineItem>& items,
             const Ceres2DBatchPlan& plan, int device, cmx_pose2d* poses,
             cmx_ceres_summary* summaries) {
  const int num = static_cast<int>(items.size());
  WorkspaceLease ws(device);
  char* h_in = ws->pinned[0].ReserveAs<char>(plan.total_bytes);
  char* d_in = ws->dev[0].ReserveAs<char>(plan.total_bytes);
  double* d_out = ws->dev[1].ReserveAs<double>(8 * static_cast<size_t>(num));
  double* h_out = ws->pinned[1].ReserveAs<double>(8 * static_cast<size_t>(num));
  for (const Ceres2DCloudSlot& cloud : plan.clouds)
    std::memcpy(h_in + cloud.at, cloud.host_xyz, 12 * static_cast<size_t>(cloud.num_points));
  Ceres2DProblem* h_prob = reinterpret_cast<Ceres2DProblem*>(h_in);
  for (int k = 0; k < num; ++k) {
    const RefineItem& it = items[k];
    Ceres2DProblem P{};
    P.cells = it.device_cells;
    P.weights = it.device_weights;       // null on a probability grid: the kernel's kind
    FillProblem(options, it, &P);
    // (a job without points reads no cloud: its pointer is the block's start, as in RefineBatch)
    P.xyz = it.device_xyz ? it.device_xyz
                          : reinterpret_cast<const float*>(d_in + (plan.jobs[k].cloud_slot >= 0
                                                                       ? plan.jobs[k].cloud_at
                                                                       : plan.problem_bytes));
    P.out = d_out + 8 * static_cast<size_t>(k);
    h_prob[k] = P;
  }
  SmallCopyAsync(d_in, h_in, plan.total_bytes, /*to_device=*/true, ws->stream);
  static_assert(kCeres2DBatchLaunches == 1, "the plan counts this launch");
  Ceres2DJobKernel<<<num, kCeresThreads, 0, ws->stream>>>(
      reinterpret_cast<const Ceres2DProblem*>(d_in));
  CMX_HIP(hipGetLastError());
  SmallCopyAsync(h_out, d_out, 64 * static_cast<size_t>(num), /*to_device=*/false, ws->stream);
  CMX_HIP(hipStreamSynchronize(ws->stream));
  UnpackResults(h_out, num, poses, summaries);
}

}  // namespace
}  // namespace cmx

extern "C" {

cmx_status cmx_ceres2d_match_grid_batch(const cmx_ceres2d_options* options,
                                        const cmx_ceres2d_job* jobs, int32_t num_jobs,
                                        cmx_pose2d* pose_estimates,
                                        cmx_ceres_summary* summaries) {
  return Guard([&] {
    CMX_REQUIRE(options && jobs && pose_estimates, "null argument");
    CMX_REQUIRE(num_jobs >= 1, "num_jobs must be at least 1");
    cmx::CheckOptions(options);
    std::vector<cmx::Ceres2DJobShape> shapes;
    int device = 0;
    const std::vector<cmx::RefineItem> items = cmx::JobItems(jobs, num_jobs, &shapes, &device);
    const cmx::Ceres2DBatchPlan plan =
        cmx::PlanCeres2DBatch(shapes.data(), num_jobs, sizeof(cmx::Ceres2DProblem));
    cmx::RunJobs(options, items, plan, device, pose_estimates, summaries);
  });
}

cmx_status cmx_debug_ceres2d_batch_plan(const int32_t* kinds, const float* const* point_clouds_xyz,
                                        const int32_t* num_points, const int32_t* resident,
                                        int32_t num_jobs, cmx_debug_ceres2d_job_plan* job_plans,
                                        cmx_debug_ceres2d_call_plan* call_plan) {
  return Guard([&] {
    CMX_REQUIRE(kinds && point_clouds_xyz && num_points && job_plans && call_plan, "null argument");
    CMX_REQUIRE(num_jobs >= 1, "num_jobs must be at least 1");
    std::vector<cmx::Ceres2DJobShape> shapes(num_jobs);
    for (int k = 0; k < num_jobs; ++k) {
      shapes[k].kind = kinds[k];
      shapes[k].host_xyz = point_clouds_xyz[k];
      shapes[k].resident = resident && resident[k] != 0;
      shapes[k].num_points = num_points[k];
    }
    cmx::CheckJobShapes(shapes);
    const cmx::Ceres2DBatchPlan plan =
        cmx::PlanCeres2DBatch(shapes.data(), num_jobs, sizeof(cmx::Ceres2DProblem));
    for (int k = 0; k < num_jobs; ++k)
      job_plans[k] = cmx_debug_ceres2d_job_plan{plan.jobs[k].kind, plan.jobs[k].cloud_slot,
                                                static_cast<int64_t>(plan.jobs[k].cloud_at)};
    *call_plan = cmx_debug_ceres2d_call_plan{static_cast<int64_t>(plan.total_bytes),
                                             static_cast<int64_t>(plan.problem_bytes),
                                             static_cast<int32_t>(plan.clouds.size()),
                                             plan.num_launches};
  });
}

}  // extern "C"
