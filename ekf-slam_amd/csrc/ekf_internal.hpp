// Runtime internals shared by the filter runtime (ekf_sched.cpp), the on-device simulator
// (sim_api.cpp): how a device-written plan of known-association messages runs on a handle; and the
// landmark front-end (lm_api.cpp): how its marker buffer becomes a device-planned association replay.
#pragma once
#include <hip/hip_runtime.h>

#include "ekf.h"
#include "ekf_device.hpp"
#include "ekf_launch.hpp"
#include "landmarks.h"

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

// The two above with the messages' odometry d_odom[T][F][3] already on the device instead of on
// the host (ekf_sim_run_lidar: the simulator's own buffer, read by the planner / the replay kernel
// in place, so `planned` / `consumed` frees it as it frees the markers). Nothing is uploaded.
int replay_markers_device(ekf_t h, int device, int T, int m_max, const int* d_counts,
                          const double* d_markers, const double* d_odom, hipEvent_t ready,
                          hipEvent_t planned);
int replay_markers_resident_device(ekf_t h, int device, int T, int m_max, const int* d_counts,
                                   const double* d_markers, const double* d_odom,
                                   hipEvent_t ready, hipEvent_t consumed);

// The front-end side of ekf_sim_run_lidar (lm_api.cpp). lm_lidar_check: EKF_E_ARG for what the
// handle cannot take — another device, n_scans outside [1, max_scans], n_beams outside
// [2, max_beams], max_markers outside [1, 64], an invalid scan configuration (lm_simulate's
// rules; scan0 is not looked at) — and touches nothing.
int lm_lidar_check(lm_t h, int device, int n_scans, int n_beams, int max_markers,
                   const lm_scan_config* cfg);
// What a run hands the front-end: the simulator's device buffers and its noise shard.
struct LidarRun {
  const double* d_truth;  // [T·F][3]
  const double* d_lm;     // [F][L][2]
  int T, F, L, n_beams, max_markers;
  unsigned long long seed;  // cfg.seed + f0
  long long msg0;
  double radius, threshold;
  const lm_scan_config* scan;
};
// What the replay behind it reads: the handle's counts and markers (lm_marker rows, stride 4) and
// the events of lm_replay_into (the detect's, and the one the filter records once it has planned).
struct LidarFeed {
  const int* d_counts;
  const double* d_markers;
  hipEvent_t ready, planned;
};
// On the handle's stream, behind `after` (the simulation): k_lidar_scan_swarm into the range
// buffer, then the detect, as lm_simulate + lm_detect_device leave them (scans resident, markers on
// the device). Arguments as checked by lm_lidar_check.
int lm_lidar_enqueue(lm_t h, const LidarRun& run, hipEvent_t after, LidarFeed* out);
// A replay has been enqueued on feed.planned: the handle's next detect waits for it.
void lm_lidar_planned(lm_t h);

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
