// Matching a filter's landmark slots to a truth map in any order (ekf_eval_match, ekf_sim_eval_match;
// kernel k_eval_match in ekf_eval.hip): the nearest truth landmark of a slot, the gate, the claim of
// a truth landmark by its lowest slot and the match record's identities. Host + device, plain values
// in and out, nothing of HIP needed, so the host compiler alone compiles it
// (tests/match_math_host_main.cpp holds it against numpy). Compiled with -ffp-contract=off on both
// sides: every product and sum below rounds on its own, as numpy's does.
#pragma once
#include <limits.h>
#include <math.h>

#include "eval_math.hpp"

namespace ekfslam {

constexpr int kMatchMaxMap = 1024;  // EKF_MATCH_MAX_MAP

// ekf_match_rec (ekf.h): one filter's association quality.
struct MatchRec {
  int n_truth, n_matched, n_primary, n_dup, n_spurious, n_missed;
  double max_match_dist;
};
static_assert(sizeof(MatchRec) == 32, "ekf_match_rec");

// The best truth landmark so far of one slot: k = -1 until a squared distance below +∞ is met.
struct Nearest {
  int k;
  double d2;
};
EKF_EVAL_HD inline Nearest nearest_none() { return Nearest{-1, INFINITY}; }

// Truth k at (tx, ty), already in the map frame, against the slot's estimate (ex, ey): the same
// dx·dx + dy·dy lm_score sums. A strict <, so that of equal distances the lowest k stays; a NaN
// coordinate gives a NaN distance, which is below nothing: a NaN truth never wins.
EKF_EVAL_HD inline void nearest_step(Nearest* n, int k, double ex, double ey, double tx,
                                     double ty) {
  const double dx = ex - tx, dy = ey - ty;
  const double d2 = dx * dx + dy * dy;
  if (d2 < n->d2) {
    n->d2 = d2;
    n->k = k;
  }
}

// The scan over pts[n][2] in ascending k.
EKF_EVAL_HD inline Nearest nearest_truth(double ex, double ey, const double* pts, int n) {
  Nearest b = nearest_none();
  for (int k = 0; k < n; ++k) nearest_step(&b, k, ex, ey, pts[2 * k], pts[2 * k + 1]);
  return b;
}

// gate2 = max_dist·max_dist, rounded once (+∞ for max_dist = +∞: every slot with a nearest truth).
EKF_EVAL_HD inline bool match_gate(const Nearest& n, double gate2) {
  return n.k >= 0 && n.d2 <= gate2;
}

EKF_EVAL_HD inline bool truth_present(double x, double y) { return !(isnan(x) || isnan(y)); }

// A truth landmark belongs to the lowest slot matched to it (slots open in ascending order, so
// that one is the landmark's original and the others its duplicates): claim[k] starts at INT_MAX
// and takes the minimum of its slots, in whatever order they come.
EKF_EVAL_HD inline void claim_take(int* claim, int j) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(claim, j);
#else
  if (j < *claim) *claim = j;
#endif
}
constexpr int kClaimFree = INT_MAX;

// The counts of a record, accumulated slot by slot and merged pairwise like LmAcc: integers and a
// maximum, so any order gives the same record.
struct MatchAcc {
  double max_d2;
  int n_truth, n_matched, n_primary, pad;
};

EKF_EVAL_HD inline void match_merge(MatchAcc* a, const MatchAcc& b) {
  a->max_d2 = b.max_d2 > a->max_d2 ? b.max_d2 : a->max_d2;
  a->n_truth += b.n_truth;
  a->n_matched += b.n_matched;
  a->n_primary += b.n_primary;
}

// A matched slot j at squared distance d2 from its truth landmark, whose claim ended at `owner`.
EKF_EVAL_HD inline void match_count(MatchAcc* a, int j, double d2, int owner) {
  a->n_matched += 1;
  a->n_primary += owner == j ? 1 : 0;
  a->max_d2 = d2 > a->max_d2 ? d2 : a->max_d2;
}

// The record's identities (n_seen: the seen slots, LmAcc's). sqrt is monotone and correctly
// rounded, so the root of the largest squared distance is the largest distance.
EKF_EVAL_HD inline MatchRec match_store(const MatchAcc& a, int n_seen) {
  MatchRec r;
  r.n_truth = a.n_truth;
  r.n_matched = a.n_matched;
  r.n_primary = a.n_primary;
  r.n_dup = a.n_matched - a.n_primary;
  r.n_spurious = n_seen - a.n_matched;
  r.n_missed = a.n_truth - a.n_primary;
  r.max_match_dist = sqrt(a.max_d2);
  return r;
}

}  // namespace ekfslam
