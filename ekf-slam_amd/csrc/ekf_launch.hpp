// Kernel launchers (each defined beside its kernel: ekf_chain.hip, ekf_factors.hip,
// ekf_sigma_pass.hip, ekf_assoc.hip, ekf_resident.hip, plan_kernels.hip, ekf_small.hip,
// ekf_copy.hip; called by
// the host scheduler in ekf_sched.cpp).
// Optional e0/e1: timing events carried by the dispatch itself (kernel execution time).
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstddef>

#include "ekf_device.hpp"

namespace ekfslam {

// Everything a launch needs to find filter f's buffers. Filters [f0, f0 + grid.y) take part;
// desc[k] describes filter f0 + k.
template <typename T>
struct PassArgs {
  T* sig[2];            // Σ ping-pong copies, filter 0
  size_t sig_stride;    // elements between filters
  double* x[2];         // state ping-pong copies, filter 0
  size_t x_stride;
  T* kcat;              // [KW][ldk] per filter (row k = one rank-1 factor over rows i)
  T* mcat;              // [KW][ldk] per filter (row k = one rank-1 factor over cols c)
  size_t km_stride;
  int ldk;
  FilterCtl* ctl;
  ChunkRec* rec;        // [2][rec_stride]: chunk records by Σ parity (chain → factors, next chain)
  size_t rec_stride;
  StageRec<T>* stage;   // [2][rec_stride]: rebuild operands staged for a kLook chain (kStageIn)
  unsigned* sync;       // device epochs (ekf_device.hpp kSync*)
  unsigned* fatal;      // host-mapped word: set when any poll of the handle timed out (flag_timeout)
  unsigned seq;         // this launch pair's sequence number; its epochs are seq + 1
  unsigned need_sigma;  // chain: wait until the Σ-pass epoch reaches this (0 = no wait)
  unsigned need_plan;   // chain: the launch's descriptors are planned once the kSyncPlan count
                        // reaches this (ekf_replay_device's planner on the bulk stream; 0 = no wait)
  unsigned pub_sigma;   // factors: publish this Σ-pass epoch first (the previous chunk's pass, 0 = none)
  int first_ready;      // chain: the launch's first chunk skips its Σ-epoch poll (the host joined
                        // the bulk stream before it, and the last pass published no epoch)
  int polls;            // 1: the streams hand off through device epochs (kernels poll them);
                        // 0: stream order / events order everything, no poll and no epoch kernel
  int gather;           // chain (dev A/B, EKF_SERIAL_GATHER=1): in stream order every chunk
                        // gathers its complete Σ_in instead of a kLook rebuild
  int chain_fast;       // chain: wave 0 runs common-case corrections in its lean program
                        // (the default; EKF_CHAIN_FAST=0: every step in the generic one)
  const MsgDesc* desc;
  int desc_stride;      // descriptors between consecutive chunks of a chain launch
  int n, ld, N, f0;
  double q, r, gate;
  int joseph;           // resident path: Joseph-form Σ update (ekf_set_joseph)
  // Pose trace (ekf_trace_enable; trace == nullptr: off, one wave-uniform test in every writer of
  // a posterior t_map_odom). A filter's posterior writers are totally ordered — what makes
  // FilterCtl::tmo correct — and its count is read and written under that order: plain loads and
  // stores, no atomics.
  TraceRec* trace;        // [F][trace_cap]
  long long* trace_n;     // [F]: records appended so far (those beyond trace_cap are only counted)
  int trace_cap;
};

// Appends filter f's posterior as record n of its trace and returns the filter's new count (the
// caller stores it: where, and how often, is the writer's own business). One lane, four 16-byte
// stores: one 64-byte line.
template <typename T>
__device__ __forceinline__ long long trace_append(const PassArgs<T>& A, int f, long long n,
                                                  double p0, double p1, double p2, double t0,
                                                  double t1, double t2) {
  if (n < A.trace_cap) {
    double2* r = reinterpret_cast<double2*>(A.trace + static_cast<size_t>(f) * A.trace_cap + n);
    r[0] = double2{p0, p1};
    r[1] = double2{p2, t0};
    r[2] = double2{t1, t2};
    reinterpret_cast<longlong2*>(r)[3] = longlong2{n, 0};
  }
  return n + 1;
}

// What every launcher below calls. With events, the launch carries them in its dispatch
// (hipExtLaunchKernelGGL): they time the kernel's own execution, not the queueing / dispatch
// latency around it.
template <typename K, typename... Args>
void launch(K kernel, dim3 grid, dim3 block, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
            Args... args) {
  if (e0 && e1)
    hipExtLaunchKernelGGL(kernel, grid, block, 0, s, e0, e1, 0, args...);
  else
    hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
}

// Chain kernel: the chunk's sequential corrections on the |U|×|U| block (predict folded in),
// one workgroup per filter → ChunkRec.
// nchunks consecutive chunks in one launch (descriptors a.desc[i·a.desc_stride + filter]).
template <typename T>
hipError_t launch_chain(const PassArgs<T>& a, int n_filters, int nchunks, hipStream_t s,
                        hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// Factor kernel: Kcat = R·Z, Mcat = Y·C on f64 MFMA and the new state. 16 rows / columns per wave.
template <typename T>
hipError_t launch_factors(const PassArgs<T>& a, int n_filters, hipStream_t s,
                      hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// Σ pass: Σ_out = Σ_in + Q − Kcatᵀ·Mcat on MFMA, one tile per wave (fp32: the tiles also write the
// chain's fp64 Σ[U,U] over its block, ChunkRec::Pend), on the grid of sigma_grid.hpp. stage: some
// filter's descriptor has kStageOut, so k_stage follows. publish: launch the Σ-pass epoch kernel
// behind it; otherwise the next chunk's factor kernel publishes it (PassArgs::pub_sigma).
template <typename T>
hipError_t launch_sigma_pass(const PassArgs<T>& a, int n_filters, bool publish, bool stage, hipStream_t s,
                      hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// Mahalanobis nearest-neighbour association for one marker per filter (one workgroup each).
template <typename T>
hipError_t launch_assoc(const PassArgs<T>& a, int n_filters, hipStream_t s,
                      hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// Unknown association, a whole chunk of ≤ kMaxChunk markers in one launch (ekf_assoc.hip): the
// scratch of the handle's k_assoc_msg (per filter: hist [kMaxChunk][Np], cur [kMaxChunk + 1][Np],
// granules [kMaxChunk + 1][G][4], Np = G·kAmSlots ≥ N).
struct AmArgs {
  AmHist* hist;
  AmCur* cur;
  unsigned long long* gran;
  size_t hist_stride, cur_stride, gran_stride;  // elements between filters
  int G;                                        // workgroups per filter
  int xcd;  // XCD-local placement: 8 blocks per workgroup, a filter's G on one XCD (k_assoc_msg)
  unsigned spin;  // bounded polls per exchange (EKF_FLAG_TIMEOUT beyond; EKF_AM_SPIN_LOG2)
  int drop;       // fault injection (EKF_AM_DROP=1, tests only): the last workgroup never
                  // publishes its first exchange, so every workgroup's poll times out
  double prior;   // the landmark prior variance (ekf_config::init_var): fp32 Σ patches the block of
                  // a landmark that is still at it when a marker corrects it
};
// Workgroups of k_assoc_msg one CU holds at once (its LDS bounds it), for the co-residency check:
// a filter's G workgroups spin on each other, so all of them must fit the bulk stream's CUs
// (per XCD in the XCD-local placement) at once, or the host routes the markers through the
// one-marker-per-launch path instead (ekf_sched.cpp am_route). joseph: the Joseph-form kernel (its
// history rows are 96 bytes, so its LDS is larger).
int assoc_msg_blocks_per_cu(bool f32, bool joseph);
// Scores, decides and corrects every marker of the chunk (slam.cpp:338-488) and writes the chunk's
// Kcat / Mcat, the new state, t_map_odom and the decisions; the Σ pass then runs as for a known-id
// chunk. One grid (G, n_filters) of 64-lane workgroups; a filter's G workgroups exchange each
// step's argmin through granules.
template <typename T>
hipError_t launch_assoc_msg(const PassArgs<T>& a, const AmArgs& b, int n_filters, hipStream_t s,
                            hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// Posterior t_map_odom for filters with no pending Σ pass.
template <typename T>
hipError_t launch_posterior(const PassArgs<T>& a, int n_filters, hipStream_t s);

// Resident path (ekf_resident.hip): n ≤ kResidentMaxN, fp64. One 256-thread workgroup per filter
// [flo, flo + nfil) keeps Σ and x in registers across every entry of the plan (PlanEntry,
// ekf_device.hpp).
constexpr int kResidentMaxN = 128;
hipError_t launch_resident(const PassArgs<double>& a, const PlanEntry* plan, int nplan, int flo,
                           int nfil, hipStream_t s, hipEvent_t e0 = nullptr,
                           hipEvent_t e1 = nullptr);

// Resident path, a replay whose inputs lie in device memory (k_resident_replay, ekf_replay_resident):
// one workgroup per filter walks the T messages itself, no descriptors. The layouts of the two
// device-planned replays below; PlanState (ekf_device.hpp) before and after.
struct ResidentReplayArgs {
  const int* counts;      // [T][F]; ≤ 0: no message, > M: clamped to M
  const int* ids;         // known ids: [T][F][M]
  const int* actions;     // known ids: [T][F][M] or null
  const double* xy;       // marker i of (t, f): xy[((t·F + f)·M + i)·stride + {0, 1}]
  const double* odom;     // [T][F][3]
  const PlanState* st_in; // [F]
  PlanState* st_out;      // [F]
  int T, F, M;            // M ≤ kMaxAssoc
  int stride;             // doubles between markers (2: packed pairs, 4: lm_marker)
  int assoc;              // 0: known ids, 1: unknown association
};
hipError_t launch_resident_replay(const PassArgs<double>& a, const ResidentReplayArgs& r,
                                  hipStream_t s, hipEvent_t e0 = nullptr,
                                  hipEvent_t e1 = nullptr);

// Known-association replay planned on the GPU (plan_kernels.hip, ekf_replay_device): PlanState
// (ekf_device.hpp) before and after a replay.
struct ReplayArgs {
  const int* counts;      // [T][F]
  const int* ids;         // [T][F][M]
  const int* actions;     // [T][F][M] or null
  const double* rel;      // [T][F][M][2]
  const double* odom;     // [T][F][3]
  const PlanState* st_in; // [F]
  PlanState* st_out;      // [F]
  MsgDesc* desc;          // [T][F]
  int T, F, M, N;
  int joseph;             // 1: Joseph form (every chunk flagged kJoseph)
  int stage;              // staged rebuild operands (kStageOut / kStageIn)
  unsigned* plan_count;   // non-null: every wave adds 1 here once its descriptor is stored (the
                          // chain polls it instead of waiting for the planner's kernel boundary)
};
hipError_t launch_plan_replay(const ReplayArgs& a, hipStream_t s);

// Unknown-association replay planned on the GPU (k_plan_assoc, ekf_replay_device_assoc): C =
// ⌈M / kMaxChunk⌉ chunk descriptors per message, desc[(t·C + c)·F + f].
struct AssocReplayArgs {
  const int* counts;      // [T][F]; ≤ 0: no message, > M: clamped to M
  const double* xy;       // marker i of (t, f): xy[((t·F + f)·M + i)·stride + {0, 1}]
  const double* odom;     // [T][F][3]
  const PlanState* st_in; // [F]
  PlanState* st_out;      // [F]
  MsgDesc* desc;          // [T][C][F]
  int T, F, M, C;
  int stride;             // doubles between markers (2: packed pairs, 4: lm_marker)
  int joseph;             // 1: Joseph form (every chunk flagged kJoseph)
};
hipError_t launch_plan_assoc(const AssocReplayArgs& a, hipStream_t s);

// Gather and score (ekf_eval.hip; ekf_get_marginals, ekf_eval, ekf_sim_eval): one workgroup per
// filter [f0, f0 + n_filters) reads the pose block and the N diagonal 2×2 blocks of the filter's
// "in" Σ copy and its state; output k belongs to filter f0 + k. Nothing of the handle is written.
struct LmMarginal;  // eval_math.hpp
struct EvalRec;
struct EvalArgs {
  const void* sig[2];     // Σ ping-pong copies, filter 0 (fp64 or fp32: the launcher's T)
  size_t sig_stride;      // elements between filters
  const double* x[2];
  size_t x_stride;
  const FilterCtl* ctl;
  const int* parity;      // [F]: the copy each filter's next chunk would read
  int N, ld, f0;
};
struct MarginalOut {      // each nullable
  double* pose;           // [n_filters][3]
  double* pose_cov;       // [n_filters][9] row-major
  LmMarginal* lm;         // [n_filters][N]
  unsigned* counter;      // [n_filters]
};
struct EvalTruth {
  const double* pose;     // filter f's (θ, x, y) at pose[f·pose_stride]
  size_t pose_stride;     // doubles between filters
  const double* lm;       // [F][n_map][2], NaN: no truth for the slot (nullptr with n_map = 0)
  int n_map;
  int has_frame;          // 0: the truth is in the map frame already, no transform at all
  double frame[3];        // (θ0, x0, y0): the map frame's pose in the truth's frame
};
template <typename T>
hipError_t launch_marginals(const EvalArgs& a, const MarginalOut& o, int n_filters, hipStream_t s);
template <typename T>
hipError_t launch_eval(const EvalArgs& a, const EvalTruth& t, EvalRec* out, int n_filters,
                       hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// (e0, e1: start / stop events carried by the dispatch when both are given, ekf_profile_read)
// ekf_eval_match: t.lm is the truth map in any order, 1 ≤ t.n_map ≤ 1024 (staged in LDS; anything
// else is refused with hipErrorInvalidValue); gate2 = max_dist². Every output is required.
struct MatchRec;  // match_math.hpp
struct MatchOut {
  EvalRec* rec;    // [n_filters]
  MatchRec* mrec;  // [n_filters]
  int* match;      // [n_filters][N]: the slot's truth landmark, −1 unseen or unmatched
};
template <typename T>
hipError_t launch_eval_match(const EvalArgs& a, const EvalTruth& t, double gate2, const MatchOut& o,
                             int n_filters, hipStream_t s, hipEvent_t e0 = nullptr,
                             hipEvent_t e1 = nullptr);

// ekf_copy_state (ekf_copy.hip): Σ, x, t_map_odom and the counter of source filters into nf
// destination filters dst_f0 + k, each side's current "in" copy, on 64 × 64 tiles of the
// destination Σ (columns up to ld_dst included: the padding is written as zero). The handles may be
// one and the same; nothing of the source is written.
constexpr int kCopyTile = 64;
struct CopyArgs {
  const void* src_sig[2];  // Σ ping-pong copies, filter 0 (fp64 or fp32: src_f32)
  size_t src_sig_stride;   // elements between filters
  const double* src_x[2];
  size_t src_x_stride;
  const FilterCtl* src_ctl;
  const int* src_par;      // [F_src]: the copy each source filter's next chunk would read
  int n_src, ld_src;
  void* dst_sig[2];
  size_t dst_sig_stride;
  double* dst_x[2];
  size_t dst_x_stride;
  FilterCtl* dst_ctl;
  const int* dst_par;      // [F_dst]
  int n_dst, ld_dst;       // n_dst >= n_src: rows and columns beyond n_src get the prior's Σ₀
  int src_f;               // >= 0: every destination filter receives this one; < 0: each receives
                           // the source filter of its own index (fpb = 1)
  int dst_f0, nf;
  int fpb;                 // destination filters per workgroup, which reads its source tile once
  int skip;                // this destination filter is the source itself and is left out (−1: none)
  double prior;            // the destination's init_var
};
// sym: the destination is an fp64 pipeline handle, whose Σ takes the element on or above the
// diagonal and its mirror below (not with dst_f32).
hipError_t launch_copy_state(const CopyArgs& a, bool src_f32, bool dst_f32, bool sym,
                             hipStream_t s);

// Σ₀ diagonal: Σ[i][i] = v for i ≥ 3 (the rest is zero-filled by the caller).
template <typename T>
hipError_t launch_init_diag(T* sig, size_t stride, int n, int ld, double v, int nf, hipStream_t s);

// Diagnostics: n_blocks workgroups each fill kPoisonLdsBytes of LDS with `pattern` (three fit a
// CU's 160 KiB, so a grid of ≥ 3·256 blocks covers every CU's LDS).
constexpr int kPoisonLdsBytes = 53 * 1024;
hipError_t launch_poison_lds(unsigned long long pattern, int n_blocks, hipStream_t s);

}  // namespace ekfslam
