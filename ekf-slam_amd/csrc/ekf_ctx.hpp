// The handle behind include/ekf.h: device memory, the two HIP streams and what orders them, the
// upload ring, profiling, and the host planner. The HIP resources are owning members
// (hip_owned.hpp), so deleting the handle releases them. Shared by the scheduler (ekf_sched.cpp)
// and the C ABI (ekf_api.cpp), which also declares here what it calls of the scheduler.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "ekf.h"
#include "ekf_device.hpp"
#include "ekf_launch.hpp"
#include "ekf_plan.hpp"
#include "eval_math.hpp"
#include "hip_owned.hpp"

namespace ekfslam {

constexpr int kRing = 16;  // pinned staging slots (host may run this many uploads ahead)

struct StageSlot {
  PinnedBuf<MsgDesc> p;
  Event ev{hipEventDisableTiming};  // the slot's last upload is done
  bool used = false;
};

struct ProfEvents {
  std::vector<Event> start, stop;
};

// What timed() brackets with events; the numerals are ekf_profile_read's `kind` (ABI).
enum ProfSlot : int {
  kProfSigma = 0,     // Σ pass
  kProfChain = 1,     // chain (reported per chunk)
  kProfAssoc = 2,     // association
  kProfFactors = 3,   // factors
  kProfResident = 4,  // resident filter kernel
  kProfEval = 5,      // k_eval (ekf_eval, ekf_sim_eval)
  kProfEvalMatch = 6, // k_eval_match (ekf_eval_match, ekf_sim_eval_match)
  kProfSlots = 7,
};

}  // namespace ekfslam

static_assert(EKF_RESIDENT_MAX_N == ekfslam::kResidentMaxN, "ekf.h and ekf_launch.hpp agree");
static_assert(sizeof(ekf_trace_rec) == sizeof(ekfslam::TraceRec) &&
                  offsetof(ekf_trace_rec, map_odom) == offsetof(ekfslam::TraceRec, map_odom) &&
                  offsetof(ekf_trace_rec, seq) == offsetof(ekfslam::TraceRec, seq),
              "ekf.h's trace record is the device's");
static_assert(sizeof(ekf_eval_rec) == sizeof(ekfslam::EvalRec) &&
                  offsetof(ekf_eval_rec, pose_cov) == offsetof(ekfslam::EvalRec, pose_cov) &&
                  offsetof(ekf_eval_rec, pose_nees) == offsetof(ekfslam::EvalRec, pose_nees) &&
                  offsetof(ekf_eval_rec, lm_var_trace) == offsetof(ekfslam::EvalRec, lm_var_trace) &&
                  offsetof(ekf_eval_rec, n_seen) == offsetof(ekfslam::EvalRec, n_seen) &&
                  offsetof(ekf_eval_rec, flags) == offsetof(ekfslam::EvalRec, flags),
              "ekf.h's eval record is the device's");
static_assert(sizeof(ekf_lm_marginal) == sizeof(ekfslam::LmMarginal) &&
                  offsetof(ekf_lm_marginal, cov) == offsetof(ekfslam::LmMarginal, cov) &&
                  offsetof(ekf_lm_marginal, seen) == offsetof(ekfslam::LmMarginal, seen),
              "ekf.h's landmark marginal is the device's");
static_assert(EKF_EVAL_POSE_NOT_PD == ekfslam::kEvalPoseNotPd &&
                  EKF_EVAL_LM_NOT_PD == ekfslam::kEvalLmNotPd, "ekf.h and eval_math.hpp agree");

struct ekf_ctx {
  ekf_config cfg{};
  int n = 0, ld = 0, ldk = 0, F = 0;
  size_t w = 8;
  // Members are destroyed in reverse order of declaration: the streams come first, so they outlive
  // every buffer and event used on them (ekf_destroy synchronises both before deleting the handle).
  ekfslam::Stream stream;  // chain + factors (+ association, posterior)
  ekfslam::Stream bulk;    // Σ passes: chunk t's pass overlaps chunk t+1's chain
  bool serial = false;           // EKF_SERIAL=1: every kernel on one stream (per-dispatch PMC)
  bool resident = false;         // n ≤ kResidentMaxN, fp64: Σ in registers (ekf_resident.hip)
  bool defer = false;            // ekf_defer: plan now, upload and launch later
  bool assoc_msg = true;         // unknown association by chunks (k_assoc_msg); EKF_ASSOC_MSG=0:
                                 // one association kernel + launch pair per marker
  bool chain_fast = true;        // k_chain's lean wave-0 program runs the common-case
                                 // corrections; EKF_CHAIN_FAST=0: the generic program from step 0
                                 // (rounds 12 and 16; bit-identical either way,
                                 // tests compare the two)
  bool main_dirty = false;       // work on the main stream since the bulk stream last joined it
  bool main_unordered = false;   // the main stream ran descriptor-reading work (k_posterior) that
                                 // nothing on the bulk stream is ordered after: a device planner
                                 // on the bulk stream must wait for it before rewriting ddesc
  bool epoch_owed = false;       // the last Σ pass published no device epoch (the flush's last
                                 // launch: the next flush joins the bulk stream on the host)
  ekfslam::AmArgs am{};          // k_assoc_msg scratch (allocated at the first association chunk),
  ekfslam::DeviceBuf<ekfslam::AmHist> am_hist;  // ... which these own
  ekfslam::DeviceBuf<ekfslam::AmCur> am_cur;
  ekfslam::DeviceBuf<unsigned long long> am_gran;
  int am_route = 0;              // unknown association: EKF_ASSOC_* (fixed at ekf_create)
  int am_route_j = 0;            // ... for the Joseph-form kernel (its larger LDS may fit fewer)
  int am_group = 1;              // filters per k_assoc_msg launch (co-resident, assoc_msg_group)
  int am_group_j = 1;            // ... Joseph form
  int bulk_cus_per_xcd = 0;      // CUs the bulk stream may use on each XCD
  int main_cus_per_xcd = 0;      // CUs the main stream may use on each XCD (0: every CU, no mask)
  // host-mapped: a device poll timed out (EKF_E_TIMEOUT)
  ekfslam::PinnedBuf<unsigned> fatal_h{hipHostMallocMapped | hipHostMallocCoherent};
  unsigned* fatal_d = nullptr;   // its device address (PassArgs::fatal)
  ekfslam::Event ev_chain{hipEventDisableTiming};  // main → bulk: the chunk's chain is done
  ekfslam::Event ev_join{hipEventDisableTiming};   // bulk → main: everything issued so far
  bool devsync = false;                   // streams synchronise through device epochs
  ekfslam::DeviceBuf<unsigned> sync;      // device epochs: Σ pass done, its ticket, chains done
  // bulk → main: Σ pass of launch s, by s & 1
  ekfslam::Event ev_sig[2] = {ekfslam::Event{hipEventDisableTiming},
                              ekfslam::Event{hipEventDisableTiming}};
  long long seq = 0;                      // launch pairs issued
  ekfslam::DeviceBuf<void> sig[2];        // (void: fp32 or fp64 by cfg.dtype, sized in bytes)
  ekfslam::DeviceBuf<double> x[2];
  ekfslam::DeviceBuf<void> kcat, mcat;
  ekfslam::DeviceBuf<ekfslam::FilterCtl> ctl;
  ekfslam::DeviceBuf<ekfslam::ChunkRec> rec;
  ekfslam::DeviceBuf<void> stage;  // StageRec<T>[2][F]: a kLook chain's rebuild operands (kStageIn)
  ekfslam::DeviceBuf<ekfslam::MsgDesc> ddesc;
  // pose trace (ekf_trace_enable; off: all null / 0, and every launch's PassArgs says so)
  ekfslam::DeviceBuf<ekfslam::TraceRec> trace;  // [F][trace_cap]
  ekfslam::DeviceBuf<long long> trace_n;        // [F] records appended
  int trace_cap = 0;  // (not the buffer's capacity / F alone: the kernels' argument)
  // ekf_get_marginals / ekf_eval: one device buffer for a call's inputs and outputs (grown, never
  // shrunk; freed with the handle)
  ekfslam::DeviceBuf<char> eval_buf;
  size_t sig_stride = 0, x_stride = 0, km_stride = 0;
  // ekf_replay_device: the planning state lives on the device while dev_plan (ping-pong by
  // dstate_cur); the planner adopts it (adopt_device_plan) before it is used again
  ekfslam::DeviceBuf<ekfslam::PlanState> dstate[2];
  ekfslam::PinnedBuf<ekfslam::PlanState> hstate;  // pinned: host → device and back
  int dstate_cur = 0;
  bool dev_plan = false;
  hipStream_t plan_stream = nullptr;  // the stream the last device planner ran on
  unsigned plan_total = 0;    // kSyncPlan: descriptors device planners have counted so far
  unsigned need_plan = 0;     // the next chain launch polls kSyncPlan for this (0: none)
  // lm_replay_into: the messages' odometry, staged in pinned memory (ev_odom: its last upload is
  // done, the staging may be rewritten) and uploaded on the planning stream
  ekfslam::DeviceBuf<double> odom_d;
  ekfslam::PinnedBuf<double> odom_h;  // (the same capacity, in doubles)
  ekfslam::Event ev_odom{hipEventDisableTiming};  // created at the first staging
  // the host mirror and the launch plan (ekf_set_joseph's form lives there too)
  ekfslam::Planner plan;
  std::vector<unsigned> held;    // status bits taken off the device word by the synchronous forms
                                 // (take_numeric); ekf_get_status reports and clears them too
  // pinned staging ring (the host may run kRing uploads ahead of the device), every slot the same
  // capacity
  ekfslam::StageSlot ring[ekfslam::kRing];
  int ring_next = 0;
  // profiling
  bool prof = false;
  ekfslam::ProfEvents pe[ekfslam::kProfSlots];
  std::vector<ekfslam::Event> pool;  // timing events ekf_profile_read has read, for timed()
  long long prof_launches[ekfslam::kProfSlots] = {};
  long long prof_chunks = 0;  // chunks the timed chain launches walked
  double prof_ms[ekfslam::kProfSlots] = {};
};

#define HIPCHK(expr)                       \
  do {                                     \
    if ((expr) != hipSuccess) return EKF_E_HIP; \
  } while (0)

namespace ekfslam {

// fn(float{}) or fn(double{}) by the handle's dtype
template <typename Fn>
auto by_dtype(const ekf_ctx* h, Fn fn) {
  return h->cfg.dtype == EKF_F32 ? fn(float{}) : fn(double{});
}

// Launch `fn(start, stop)` bracketed by two pooled timing events when profiling (ekf_profile_read
// returns them to the pool); fn(nullptr, nullptr) when not, or when the pool cannot be brought to
// two events: one event alone stays pooled.
template <typename Fn>
int timed(ekf_ctx* h, ProfSlot kind, Fn fn) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto& pool = h->pool;
  while (h->prof && pool.size() < 2) {
    pool.emplace_back();
    if (pool.back().create() == EKF_OK) continue;
    pool.pop_back();
    break;
  }
  if (h->prof && pool.size() >= 2) {
    for (auto* v : {&h->pe[kind].start, &h->pe[kind].stop}) {
      v->push_back(std::move(pool.back()));
      pool.pop_back();
    }
    e0 = h->pe[kind].start.back().get();
    e1 = h->pe[kind].stop.back().get();
  }
  return fn(e0, e1) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

// ---- ekf_sched.cpp ----
constexpr int kCuSplitMaxFilters = 32;  // more filters: no CU split (create_streams)
constexpr size_t kDescInit = 256;       // descriptors at creation (×F/64 for wide handles)
int create_streams(ekf_ctx* h);         // both streams, their CU masks, devsync
int am_route(ekf_ctx* h, bool joseph);  // which path unknown association takes (EKF_ASSOC_*)
// the route in effect: the Joseph form keeps the chunk route only where its kernel fits alike
inline int assoc_route(const ekf_ctx* h) {
  return h->plan.joseph() && h->am_route_j != h->am_route ? EKF_ASSOC_MARKER : h->am_route;
}
int reserve_upload(ekf_ctx* h, size_t need);
int init_diag(ekf_ctx* h, void* sig0, int nf);  // Σ₀ diagonal of nf filters from sig0 on
int flush(ekf_ctx* h);                // upload the plan and enqueue its launches
int submit(ekf_ctx* h);               // flush, unless deferred and the plan is still small
bool plan_is_large(const ekf_ctx* h); // ≥ kFlushDesc descriptors planned
int drain(ekf_ctx* h);                // both streams idle
int adopt_device_plan(ekf_ctx* h);    // a device replay's planning state into the planner
int settle(ekf_ctx* h);               // flush, drain, adopt: before any host access to device state
int take_fatal(ekf_ctx* h);
int take_numeric(ekf_ctx* h, int f, unsigned* fl_out);
int status_rc(ekf_ctx* h, int f, bool range);
// association with the decisions read back, for the message in the planner's slots [0, nf)
int assoc_sync(ekf_ctx* h, int f0, int nf, bool predict, bool posterior, int m_max, int* j_out,
               int* new_out);
int replay_device(ekf_ctx* h, int T, int m_max, const int* d_counts, const int* d_ids,
                  const int* d_actions, const double* d_rel_xy, const double* d_odom);
// the chunk routes only: pipeline handle, assoc_route(h) != EKF_ASSOC_MARKER
inline bool device_assoc_supported(const ekf_ctx* h) {
  return !h->resident && assoc_route(h) != EKF_ASSOC_MARKER;
}
// Unknown-association replay planned on the GPU (k_plan_assoc). host_odom (nullable): [T][F][3] on
// the host, uploaded into the handle's own buffer and used instead of d_odom. ready (nullable):
// the planning stream waits for it before the planner reads its inputs; planned (nullable):
// recorded behind the planner kernel, after which the descriptors hold copies of every input.
int replay_device_assoc(ekf_ctx* h, int T, int m_max, const int* d_counts, const double* d_xy,
                        int xy_stride, const double* d_odom, const double* host_odom,
                        hipEvent_t ready, hipEvent_t planned);

// Resident handles: T messages from device memory in one launch of k_resident_replay. assoc = 0:
// known ids (d_ids, nullable d_actions), 1: unknown association. host_odom / ready as above;
// consumed (nullable): recorded behind the kernel, which reads its inputs for the whole launch.
int replay_resident(ekf_ctx* h, int assoc, int T, int m_max, const int* d_counts, const int* d_ids,
                    const int* d_actions, const double* d_xy, int xy_stride, const double* d_odom,
                    const double* host_odom, hipEvent_t ready, hipEvent_t consumed);

}  // namespace ekfslam
