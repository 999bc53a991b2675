// Runtime internals shared by the filter runtime (ekf_sched.cpp), the on-device simulator
// (sim_api.cpp): how a device-written plan of known-association messages runs on a handle; and the
// landmark front-end (lm_api.cpp): how its marker buffer becomes a device-planned association replay.
#pragma once
#include <hip/hip_runtime.h>

#include "ekf.h"
#include "ekf_device.hpp"
#include "ekf_launch.hpp"

namespace ekfslam {

struct HandleInfo {
  int F, N, n, dtype, device;
  bool resident;  // n ≤ kResidentMaxN fp64: one resident launch per plan
  bool joseph;    // ekf_set_joseph is on (the HBM pipeline then needs one marker per chunk)
  bool serial;    // EKF_SCHED_SERIAL: every kernel runs on `stream`
  hipStream_t stream;
  hipStream_t bulk;  // the factors / Σ-pass stream (the main stream when serial)
};

// Runs everything the host has planned so far (flush) and describes the handle.
int handle_info(ekf_t h, HandleInfo* out);
// The parity each filter's next chunk reads (the planner's mirror).
int handle_parity(ekf_t h, int* parity);
// T messages whose descriptors the device wrote into dd[t·F + f] on the handle's main stream (one
// known-association chunk per message, the first of each filter non-pipelined), and for the
// resident path the plan entries dplan[T]. Enqueues the filter kernels behind them; then the host
// mirror takes parity_after[F], odom_after[F][3] (t_odom_robot after the plan's last message, the
// predict input of the next host-planned call), no pending predict, and a non-pipelined next chunk.
int run_device_plan(ekf_t h, const MsgDesc* dd, const PlanEntry* dplan, int T,
                    const int* parity_after, const double* odom_after);
// The filter side of lm_replay_into (lm_api.cpp): ekf_replay_device_assoc on the front-end's
// lm_marker[T·F][m_max] array (xy_stride 4) and counts on `device`, with the messages' odometry
// odom[T][F][3] taken from the host into a buffer the handle owns. The planning stream waits for
// `ready` (the front-end's detect) before the planner reads the markers; `planned` is recorded
// behind the planner, after which the marker buffer is free again. EKF_E_ARG as the entry point's,
// and for a handle on another device.
int replay_markers(ekf_t h, int device, int T, int m_max, const int* d_counts,
                   const double* d_markers, const double* odom, hipEvent_t ready,
                   hipEvent_t planned);

// The same for a resident handle (lm_replay_resident): one launch of k_resident_replay reads the
// markers in place for the whole replay, so `consumed` is recorded behind that kernel. EKF_E_ARG
// as ekf_replay_resident's, and for a handle on another device.
int replay_markers_resident(ekf_t h, int device, int T, int m_max, const int* d_counts,
                            const double* d_markers, const double* odom, hipEvent_t ready,
                            hipEvent_t consumed);

// ekf_eval with the truth already on the handle's device (ekf_sim_eval): filter f's true pose at
// d_pose[f·pose_stride], its map d_lm[F][n_map][2] (nullable with n_map = 0), frame[3] nullable.
// Synchronises like ekf_get_*; out[F] on the host. EKF_E_ARG as ekf_eval's.
int eval_device(ekf_t h, const double* d_pose, size_t pose_stride, const double* d_lm, int n_map,
                const double* frame, ekf_eval_rec* out);
// ekf_eval_match likewise (ekf_sim_eval_match): d_lm[F][n_map][2] in any order. EKF_E_ARG as
// ekf_eval_match's.
int eval_match_device(ekf_t h, const double* d_pose, size_t pose_stride, const double* d_lm,
                      int n_map, const double* frame, double max_dist, ekf_eval_rec* out,
                      ekf_match_rec* match_out, int* match);

}  // namespace ekfslam
