// The host planner (ekf_plan.hpp): the reference's two callbacks (nuslam/src/slam.cpp:180-316,
// :318-530) as descriptors and launches. No HIP.
#include "ekf_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "ekf.h"

namespace ekfslam {

namespace {

// slam.cpp:208-210 (host, glibc, as the reference)
inline void measure(double rx, double ry, double* zr, double* zb) {
  *zr = std::sqrt(std::pow(rx, 2) + std::pow(ry, 2));
  *zb = std::atan2(ry, rx);
}

}  // namespace

void Planner::init(int F, int N, bool resident, bool staging) {
  F_ = F;
  N_ = N;
  resident_ = resident;
  staging_ = staging;
  odom_.assign(F, {0.0, 0.0, 0.0});
  parity_.assign(F, 0);
  pending_.assign(F, 0);
  prev_m_.assign(F, -1);
  staged_.assign(F, {});
  prev_ids_.assign(F, std::array<int, kMaxChunk>{});
  msgs_.resize(F);
  absent_.assign(F, 0);
}

int Planner::set_message(int m, const int* ids, const int* actions, const double* rel_xy) {
  auto& mk = msgs_[0];
  mk.clear();
  for (int i = 0; i < m; ++i) {
    if (ids && actions && actions[i] == EKF_MARKER_DELETE) continue;
    if (ids && (ids[i] < 0 || ids[i] >= N_)) return EKF_E_RANGE;
    Marker k;
    k.id = ids ? ids[i] : -1;
    measure(rel_xy[2 * i], rel_xy[2 * i + 1], &k.zr, &k.zb);
    mk.push_back(k);
  }
  return EKF_OK;
}

int Planner::load_batch(int assoc_mode, int m_max, const int* counts, const int* ids,
                        const int* actions, const double* rel_xy, const double* odom) {
  for (int f = 0; f < F_; ++f) {
    const int c = counts[f];
    if (c < 0 || c > m_max) return EKF_E_ARG;
    if (!assoc_mode)
      for (int i = 0; i < c; ++i) {
        const size_t e = static_cast<size_t>(f) * m_max + i;
        if (actions && actions[e] == EKF_MARKER_DELETE) continue;
        if (ids[e] < 0 || ids[e] >= N_) return EKF_E_RANGE;
      }
  }
  for (int f = 0; f < F_; ++f) {
    if (odom) odom_[f] = {odom[3 * f], odom[3 * f + 1], odom[3 * f + 2]};
    absent_[f] = counts[f] == 0;
    auto& mk = msgs_[f];
    mk.clear();
    for (int i = 0; i < counts[f]; ++i) {
      const size_t e = static_cast<size_t>(f) * m_max + i;
      if (!assoc_mode && actions && actions[e] == EKF_MARKER_DELETE) continue;
      Marker k;
      k.id = assoc_mode ? -1 : ids[e];
      measure(rel_xy[2 * e], rel_xy[2 * e + 1], &k.zr, &k.zb);
      mk.push_back(k);
    }
  }
  return EKF_OK;
}

int Planner::largest(int nf) const {
  int mm = 1;
  for (int k = 0; k < nf; ++k) mm = std::max(mm, size(k));
  return mm;
}

MsgDesc* Planner::fill(size_t at, int m, int flags, int f) {
  MsgDesc* d = &plan_d_[at];
  std::memset(d, 0, sizeof(MsgDesc));
  d->m = m;
  d->flags = flags;
  d->parity = parity_[f];
  for (int i = 0; i < 3; ++i) d->odom[i] = odom_[f][i];
  return d;
}

void Planner::known(int f0, int nf, bool predict, const char* absent) {
  // Joseph form on the pipeline: ≤ kMaxJoseph (= kMaxChunk) markers per chunk (the chain's row map
  // Z holds K's and V = ΣHᵀ − K·S's columns, 4 per marker; k_chain<T, true>)
  const bool jos = joseph_ && !resident_;
  const int cm = jos ? kMaxJoseph : kMaxChunk;
  int chunks = 1;
  for (int k = 0; k < nf; ++k) chunks = std::max(chunks, (size(k) + cm - 1) / cm);
  for (int chunk = 0; chunk < chunks; ++chunk) {
    const size_t off = plan_d_.size();
    plan_d_.resize(off + nf);
    const long li = static_cast<long>(plan_l_.size());
    plan_l_.push_back(Launch{kLaunchKnown, off, f0, nf, 4, false, false});
    int kw = 4;
    bool nolook = false;
    for (int k = 0; k < nf; ++k) {
      const int f = f0 + k;
      const auto& mk = msgs_[k];
      const int nchunks = std::max(1, (size(k) + cm - 1) / cm);
      if (chunk >= nchunks || (absent && absent[k])) {
        std::memset(&plan_d_[off + k], 0, sizeof(MsgDesc));
        continue;
      }
      const int b = chunk * cm;
      const int m = std::max(0, std::min(cm, size(k) - b));
      int flags = kActive | (jos ? kJoseph : 0);
      if (chunk == 0 && (predict || pending_[f])) flags |= kFirst;
      if (chunk == nchunks - 1 && predict) flags |= kLast;
      // rebuild from the chunk before (its Σ pass may run); the resident kernel carries Σ itself
      if (prev_m_[f] >= 0 && !resident_) flags |= kLook;
      nolook = nolook || !(flags & kLook);
      MsgDesc* d = fill(off + k, m, flags, f);
      d->prev_m = prev_m_[f];
      for (int i = 0; i < kMaxChunk; ++i) d->prev_ids[i] = prev_ids_[f][i];
      for (int i = 0; i < m; ++i) {
        d->ids[i] = mk[b + i].id;
        d->z[i][0] = mk[b + i].zr;
        d->z[i][1] = mk[b + i].zb;
      }
      // the k_stage behind the Σ pass two chunks back gathers this chain's rebuild operands
      // (the Σ_in' it reads is that pass's output)
      const Staged two_back = staged_[f][1];
      if ((flags & kLook) && staging_ && two_back.desc >= 0) {
        MsgDesc* sd = &plan_d_[two_back.desc];
        sd->flags |= kStageOut;
        sd->stg_m = m;
        sd->stg_pm = prev_m_[f];
        for (int i = 0; i < kMaxChunk; ++i) {
          sd->stg_ids[i] = d->ids[i];
          sd->stg_pids[i] = prev_ids_[f][i];
        }
        plan_l_[two_back.launch].stage = true;
        d->flags |= kStageIn;
      }
      staged_[f] = {Staged{static_cast<long>(off + k), li}, staged_[f][0]};
      prev_m_[f] = m;
      for (int i = 0; i < m; ++i) prev_ids_[f][i] = mk[b + i].id;
      parity_[f] ^= 1;
      kw = std::max(kw, pass_kw(jos, m));
      if (chunk == 0) pending_[f] = 0;
    }
    plan_l_[li].kw = kw;
    plan_l_[li].nolook = nolook;
  }
}

void Planner::unknown(int f0, int nf, bool predict, bool posterior, int i0, int i1,
                      const char* absent, int route) {
  // markers per chunk: whole chunks through k_assoc_msg on the HBM pipeline (either form:
  // k_assoc_msg<T, J>), or one marker per launch
  const int per = route != EKF_ASSOC_MARKER ? kMaxChunk : 1;
  const LaunchKind kind = route != EKF_ASSOC_MARKER ? kLaunchAssocChunk : kLaunchAssoc;
  int chunks = 1;
  for (int k = 0; k < nf; ++k)
    chunks = std::max(chunks, (std::min(size(k), i1) - i0 + per - 1) / per);
  for (int chunk = 0; chunk < chunks; ++chunk) {
    const size_t off = plan_d_.size();
    plan_d_.resize(off + nf);
    bool any = false;
    for (int k = 0; k < nf; ++k) {
      const int f = f0 + k;
      const auto& mk = msgs_[k];
      const int mf = std::min(size(k), i1);
      const int nch = std::max(1, (mf - i0 + per - 1) / per);
      if (chunk >= nch || (absent && absent[k]) || (mf <= i0 && i0 > 0)) {
        std::memset(&plan_d_[off + k], 0, sizeof(MsgDesc));
        continue;
      }
      const int b = i0 + chunk * per;
      const int m = std::max(0, std::min(per, mf - b));
      // (the marker route runs on the resident path too, which has no Joseph chunks)
      const int jos = joseph_ && !resident_ ? kJoseph : 0;
      int flags = kActive | kNoInit | jos;
      forget(f);  // association chunks run unpipelined
      if (b == 0 && (predict || pending_[f])) flags |= kFirst;
      if (chunk == nch - 1 && posterior) flags |= kLast;
      MsgDesc* d = fill(off + k, m, flags, f);
      d->assoc_slot = b % kMaxAssoc;
      for (int i = 0; i < m; ++i) {
        d->ids[i] = -1;
        d->z[i][0] = mk[b + i].zr;
        d->z[i][1] = mk[b + i].zb;
      }
      parity_[f] ^= 1;
      if (b == 0) pending_[f] = 0;
      any = true;
    }
    plan_l_.push_back(Launch{kind, off, f0, nf, 4, any, false});
  }
}

void Planner::posterior(int f) {
  forget(f);
  const size_t off = plan_d_.size();
  plan_d_.resize(off + 1);
  fill(off, 0, kActive, f);
  plan_l_.push_back(Launch{kLaunchPosterior, off, f, 1, 4, true, false});
}

void Planner::forget(int f) {
  prev_m_[f] = -1;
  staged_[f] = {};
}

void Planner::reset(int f) {
  parity_[f] = 0;
  pending_[f] = 0;
  forget(f);
}

void Planner::set_joseph(bool on) {
  for (int f = 0; f < F_; ++f) forget(f);
  joseph_ = on;
}

void Planner::export_state(PlanState* st) const {
  for (int f = 0; f < F_; ++f) {
    PlanState& ps = st[f];
    ps = PlanState{};
    ps.parity = parity_[f];
    ps.prev_m = prev_m_[f];
    ps.pending = pending_[f];
    for (int i = 0; i < kMaxChunk; ++i) ps.prev_ids[i] = prev_ids_[f][i];
    for (int i = 0; i < 3; ++i) ps.odom[i] = odom_[f][i];
  }
}

void Planner::adopt(const PlanState* st) {
  for (int f = 0; f < F_; ++f) {
    const PlanState& ps = st[f];
    parity_[f] = ps.parity;
    prev_m_[f] = ps.prev_m;
    pending_[f] = static_cast<char>(ps.pending);
    for (int i = 0; i < kMaxChunk; ++i) prev_ids_[f][i] = ps.prev_ids[i];
    odom_[f] = {ps.odom[0], ps.odom[1], ps.odom[2]};
    staged_[f] = {};
  }
}

void Planner::take(const int* parity_after, const double* odom_after) {
  for (int f = 0; f < F_; ++f) {
    parity_[f] = parity_after[f];
    odom_[f] = {odom_after[3 * f], odom_after[3 * f + 1], odom_after[3 * f + 2]};
    pending_[f] = 0;
    forget(f);
  }
}

void Planner::clear() {
  plan_d_.clear();
  plan_l_.clear();
  for (int f = 0; f < F_; ++f) staged_[f] = {};
  if (resident_) std::fill(prev_m_.begin(), prev_m_.end(), -1);
}

}  // namespace ekfslam
