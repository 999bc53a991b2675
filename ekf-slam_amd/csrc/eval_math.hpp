// Scoring a filter against the truth (ekf_eval, ekf_sim_eval; kernels in ekf_eval.hip): the records,
// the frame transform, the pose and landmark errors and their NEES. Host + device, plain values in
// and out, nothing of HIP needed, so the host compiler alone compiles it
// (tests/eval_math_host_main.cpp holds it against numpy). Compiled with -ffp-contract=off on both
// sides: every product and sum below rounds on its own, as numpy's does.
#pragma once
#include <math.h>

#include "geom.hpp"

#if defined(__HIPCC__)
#define EKF_EVAL_HD __host__ __device__
#else
#define EKF_EVAL_HD
#endif

namespace ekfslam {

constexpr unsigned kEvalPoseNotPd = 1u;  // EKF_EVAL_POSE_NOT_PD
constexpr unsigned kEvalLmNotPd = 2u;    // EKF_EVAL_LM_NOT_PD

// ekf_lm_marginal (ekf.h): one landmark slot's estimate and its symmetrised 2×2 block of Σ.
struct LmMarginal {
  double xy[2];
  double cov[3];  // xx, xy, yy
  int seen;
  int pad;
};
static_assert(sizeof(LmMarginal) == 48, "ekf_lm_marginal");

// ekf_eval_rec (ekf.h): one filter's score.
struct EvalRec {
  double pose_err[3];
  double pose_cov[6];  // tt tx ty xx xy yy
  double pose_nees, lm_sq_err, lm_nees, lm_max_err, lm_var_trace;
  int n_seen, n_eval, n_nees;
  unsigned flags;
};
static_assert(sizeof(EvalRec) == 128, "ekf_eval_rec");

// ½(a + b): the symmetric part of a pair of mirrored entries (fp32 and resident Σ is symmetric only
// up to rounding). Exact for a == b.
EKF_EVAL_HD inline double sym_part(double a, double b) { return 0.5 * (a + b); }

// slam.cpp:213's first-sighting test, negated: the slot holds a landmark.
EKF_EVAL_HD inline bool lm_seen(double x, double y) { return !(x == 0.0 && y == 0.0); }

EKF_EVAL_HD inline bool pivot_ok(double d) { return d > 0.0 && isfinite(d); }

// eᵀP⁻¹e for the symmetric 3×3 P = {tt tx ty xx xy yy} by a square-root-free Cholesky
// (P = L·D·Lᵀ, then Σ zᵢ²/dᵢ with L·z = e). A pivot ≤ 0 or not finite: NaN and *pd = false (a NaN
// or infinite entry of P reaches a pivot whichever entry it is).
EKF_EVAL_HD inline double nees3(const double* P, const double* e, bool* pd) {
  *pd = false;
  const double nan = NAN;
  const double d0 = P[0];
  if (!pivot_ok(d0)) return nan;
  const double l10 = P[1] / d0, l20 = P[2] / d0;
  const double d1 = P[3] - l10 * P[1];
  if (!pivot_ok(d1)) return nan;
  const double u21 = P[4] - l20 * P[1];  // = l21·d1
  const double l21 = u21 / d1;
  const double d2 = P[5] - l20 * P[2] - l21 * u21;
  if (!pivot_ok(d2)) return nan;
  *pd = true;
  const double z0 = e[0];
  const double z1 = e[1] - l10 * z0;
  const double z2 = e[2] - l20 * z0 - l21 * z1;
  return z0 * z0 / d0 + z1 * z1 / d1 + z2 * z2 / d2;
}

// The same for the symmetric 2×2 C = {xx xy yy}.
EKF_EVAL_HD inline double nees2(const double* C, double e0, double e1, bool* pd) {
  *pd = false;
  const double nan = NAN;
  const double d0 = C[0];
  if (!pivot_ok(d0)) return nan;
  const double l = C[1] / d0;
  const double d1 = C[2] - l * C[1];
  if (!pivot_ok(d1)) return nan;
  *pd = true;
  const double z1 = e1 - l * e0;
  return e0 * e0 / d0 + z1 * z1 / d1;
}

// The truth's frame → the map frame. `inv` = inverse(frame), frame = the map frame's pose in the
// truth's frame; nullptr: no transform at all.
EKF_EVAL_HD inline Pose2 truth_pose_in_map(const Pose2* inv, double theta, double x, double y) {
  if (!inv) return Pose2{theta, x, y};
  Pose2 p = compose(*inv, Pose2{theta, x, y});
  p.theta = normalize_angle(p.theta);
  return p;
}
EKF_EVAL_HD inline void truth_point_in_map(const Pose2* inv, double x, double y, double* ox,
                                           double* oy) {
  if (!inv) {
    *ox = x;
    *oy = y;
    return;
  }
  const Pose2 p = compose(*inv, Pose2{0.0, x, y});
  *ox = p.x;
  *oy = p.y;
}

// The pose part of a record: the error (heading wrapped into (−π, π]), the covariance block as
// given (already symmetrised) and its NEES.
EKF_EVAL_HD inline void score_pose(const double* est, const double* P6, const double* truth,
                                   const Pose2* inv, EvalRec* r) {
  const Pose2 t = truth_pose_in_map(inv, truth[0], truth[1], truth[2]);
  r->pose_err[0] = normalize_angle(est[0] - t.theta);
  r->pose_err[1] = est[1] - t.x;
  r->pose_err[2] = est[2] - t.y;
  for (int k = 0; k < 6; ++k) r->pose_cov[k] = P6[k];
  bool pd;
  r->pose_nees = nees3(P6, r->pose_err, &pd);
  if (!pd) r->flags |= kEvalPoseNotPd;
}

// The landmark part of a record, accumulated slot by slot and merged pairwise: sums add, the
// maximum and the flags combine. Neither is associative in floating point, so whoever accumulates
// fixes the order (ekf_eval.hip: a lane's slots ascending, then a binary tree over the lanes).
struct LmAcc {  // (`LmAcc a{}` is the empty sum; no initialisers, so that it can live in LDS)
  double sq, nees, max_err, tr;
  int n_seen, n_eval, n_nees;
  unsigned flags;
};

EKF_EVAL_HD inline void lm_merge(LmAcc* a, const LmAcc& b) {
  a->sq = a->sq + b.sq;
  a->nees = a->nees + b.nees;
  a->tr = a->tr + b.tr;
  a->max_err = b.max_err > a->max_err ? b.max_err : a->max_err;
  a->n_seen += b.n_seen;
  a->n_eval += b.n_eval;
  a->n_nees += b.n_nees;
  a->flags |= b.flags;
}

// Slot j: estimate (ex, ey), symmetrised block C = {xx xy yy}; truth = the slot's true (x, y) in the
// truth's frame, or nullptr when the caller has none (j ≥ n_map). Evaluated when seen and the
// truth is there and not NaN.
EKF_EVAL_HD inline void lm_score(LmAcc* a, double ex, double ey, const double* C,
                                 const double* truth, const Pose2* inv) {
  if (!lm_seen(ex, ey)) return;
  a->n_seen += 1;
  a->tr = a->tr + (C[0] + C[2]);
  if (!truth || isnan(truth[0]) || isnan(truth[1])) return;
  double tx, ty;
  truth_point_in_map(inv, truth[0], truth[1], &tx, &ty);
  const double dx = ex - tx, dy = ey - ty;
  const double sq = dx * dx + dy * dy;
  const double err = sqrt(sq);
  a->n_eval += 1;
  a->sq = a->sq + sq;
  a->max_err = err > a->max_err ? err : a->max_err;
  bool pd;
  const double q = nees2(C, dx, dy, &pd);
  if (pd) {
    a->nees = a->nees + q;
    a->n_nees += 1;
  } else {
    a->flags |= kEvalLmNotPd;
  }
}

EKF_EVAL_HD inline void lm_store(const LmAcc& a, EvalRec* r) {
  r->lm_sq_err = a.sq;
  r->lm_nees = a.nees;
  r->lm_max_err = a.max_err;
  r->lm_var_trace = a.tr;
  r->n_seen = a.n_seen;
  r->n_eval = a.n_eval;
  r->n_nees = a.n_nees;
  r->flags |= a.flags;
}

}  // namespace ekfslam
