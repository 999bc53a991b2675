/* On-device Monte-Carlo inputs for a filter handle: nusim's wheel
 * integration with slip and its fake landmark sensor, for every filter of an ekf_t, feeding the
 * filter with no host round trip.
 *
 * Replaces, per filter f (seeded seed + f0 + f, counter-based splitmix64 draws):
 *   nusim timer_callback   nusim/src/nusim.cpp:222-230  wheel angle += commanded increment ×
 *                                                      (1 + U(−slip, slip)); true pose =
 *                                                      DiffDrive::FKin(true wheel angles)
 *                                                      (turtlelib/src/diff_drive.cpp:10-28)
 *   slam jointStateCallback nuslam/src/slam.cpp:599-634 t_odom_robot = FKin(encoder angles): the
 *                                                      encoders report the COMMANDED angles — a
 *                                                      deliberate change from nusim, whose encoders
 *                                                      publish the slipped wheel_pos_l/r
 *                                                      (nusim.cpp:272-273), so its odometry follows
 *                                                      the truth; here odometry drifts from the
 *                                                      truth and the filter has work to do
 *   nusim sensor_timer_callback nusim.cpp:317-346      marker = landmark in the true body frame
 *                                                      + N(0, σ²) on x and y; ADD within range,
 *                                                      DELETE beyond (mode ALL) or the m nearest
 *                                                      in range (NEAREST)
 * and the host's per-message planning of ekf_replay (known association): the device writes each
 * message's descriptor itself, so a swarm replay is a few launches per upload window.
 * The same arithmetic, draw for draw, is restated on the host by pyekf.synth (the test oracle of
 * this path); the filter then equals oracle/ runs fed the device's own markers.
 * The last stage of a Monte-Carlo run, scoring the estimate against this truth (pose and map error,
 * NEES), runs on the device too: ekf_sim_eval.
 * Unknown association, what the real robot runs (Slam::sensor_cb, slam.cpp:318-530: Mahalanobis
 * nearest-neighbour association, no ids), has the same two stages: ekf_sim_run_assoc simulates the
 * same markers and hands them to the filter with the ids ignored, and ekf_sim_eval_match matches the
 * slots the filter opened to the simulator's map on the device, scores them and reports the
 * association's quality (duplicate, spurious and missed landmarks).
 * ekf_sim_run_lidar runs the real sensor path instead of the fake sensor: nusim's laser on the truth
 * poses, the `landmarks` node's circle detection (landmarks.h), then the same association replay.
 *
 * Collisions with obstacles (nusim.cpp:232-254) are off by default and turned on by
 * ekf_sim_set_collisions: after each tick's FKin the true pose is tested against the map's cylinders
 * in id order and pushed out of the first one it is inside, while the wheels and the odometry go
 * on as commanded. */
#ifndef EKF_SIM_H
#define EKF_SIM_H

#include "ekf.h"
#include "landmarks.h" /* lm_t, lm_scan_config (ekf_sim_run_lidar) */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ekf_sim* ekf_sim_t;

#define EKF_SENSE_NEAREST 0 /* the m nearest landmarks within max_range, nearest first */
#define EKF_SENSE_SURVEY 1  /* within 2·max_range, not-yet-sighted first, never empty. The sighted
                             * set: a landmark is sighted once a SURVEY message of this simulator
                             * has reported it; NEAREST and ALL messages neither read nor write
                             * the set */
#define EKF_SENSE_ALL 2     /* every landmark in id order, DELETE beyond max_range */

typedef struct {
  unsigned long long seed; /* filter f of the handle draws from seed + f0 + f */
  int f0;                  /* global index of the handle's filter 0 (one handle per rank) */
  int ticks_per_msg;       /* joint-state ticks per sensor message (nusim: 200 Hz / 5 Hz = 40) */
  double slip;             /* slip_fraction (nusim.cpp:224-227) */
  double sensor_sigma;     /* σ of the marker x, y noise (nusim.cpp:339-340) */
  double max_range;        /* sensor range, m */
  int max_markers;         /* m ≤ 16 for NEAREST / SURVEY messages */
  int marker_stride;       /* M: noise draws of message t, marker i use index t·M + i (≥ m; ≥ L
                            * when any message senses ALL) */
  double wheel_radius, track_width;               /* diff_params.yaml: 0.033, 0.160 */
  double start_theta, start_x, start_y;           /* true start pose (odometry starts at 0) */
  int record;              /* keep markers and poses for ekf_sim_markers / ekf_sim_poses */
} ekf_sim_config;

void ekf_sim_config_default(ekf_sim_config* c);

/* landmarks[F][L][2]: filter f's map (true positions); L ≤ 1024, ≤ the handle's n_landmarks.
 * ticks_per_msg ≤ 64 (one lane per tick). The simulator keeps its own true and odometry
 * poses and message counter across runs. */
int ekf_sim_create(ekf_sim_t* out, ekf_t filter, const ekf_sim_config* cfg, int n_map,
                   const double* landmarks);
int ekf_sim_destroy(ekf_sim_t s);

/* T messages: wheel_cmd[T·ticks_per_msg][2] commanded wheel-angle increments per tick (rad, left,
 * right; every filter's), sense[T] EKF_SENSE_* per message (NULL: NEAREST). Simulates, senses and
 * plans on the device, then runs the filter over the T messages (asynchronous like ekf_replay; the
 * call waits only for the device planning). A filter with no marker in a message gets no message
 * (as ekf_replay with counts 0). Afterwards the handle's t_odom_robot is the run's last odometry
 * pose, as if ekf_set_odom had been called with it (the next host-planned call predicts from it).
 * With ekf_set_joseph on, the chunks are Joseph-form ones. */
int ekf_sim_run(ekf_sim_t s, int T, const double* wheel_cmd, const int* sense);

/* T messages with unknown association: simulated exactly as by ekf_sim_run with sense = NULL (every
 * message senses NEAREST, so every marker is ADD: sensor_cb has no DELETE test, which is why SURVEY
 * and ALL are not offered here), the same draws and the same bits, always in the parallel form
 * (EKF_SIM_PARALLEL does not apply). The marker arrays then go to the filter with the ids ignored:
 * a pipeline handle gets ekf_replay_device_assoc(h, T, marker_stride, counts, rel_xy, 2, odom), a
 * resident handle ekf_replay_resident(h, 1, T, marker_stride, counts, NULL, NULL, rel_xy, 2, odom).
 * Nothing crosses PCIe but the wheel commands; asynchronous (the host waits for nothing). The
 * handle afterwards, its t_odom_robot included, the pose trace, ekf_get_decisions (the last
 * message's), ekf_set_joseph, ekf_sim_markers and ekf_sim_poses hold as for those replays and for
 * ekf_sim_run, with which this call may alternate on one simulator: both advance the same tick and
 * message counters.
 * EKF_E_ARG, and nothing changes: a NULL simulator, T < 0, NULL wheel_cmd with T > 0,
 * marker_stride > 64 (the replays' m_max limit), a pipeline handle on the one-marker route
 * (ekf_get_assoc_route: EKF_ASSOC_MARKER). T == 0: EKF_OK. */
int ekf_sim_run_assoc(ekf_sim_t s, int T, const double* wheel_cmd);

/* T messages through the real sensor path (unknown_data_assoc.launch.py: laser, circle detection,
 * Mahalanobis association), none of it leaving the device. The wheels and the truth poses are
 * simulated exactly as by ekf_sim_run_assoc (the fake sensor's markers are still written, so the
 * record and ekf_sim_markers hold, and the call may alternate with ekf_sim_run and
 * ekf_sim_run_assoc on one simulator: all three advance the same tick and message counters). Then,
 * on the front-end handle `lm`: nusim's laser (lm_simulate, landmarks.h) scans every (message,
 * filter) from its true pose against the filter's own map, each landmark a cylinder of
 * obstacle_radius, into the handle's range buffer — scan t*F + f is message t of filter f — and
 * the handle detects on them (lm_detect_device: n_beams, threshold, max_markers); the detected
 * markers go to the filter as lm_replay_into / lm_replay_resident would feed them, with the
 * simulator's own odometry. The laser's noise is sharded as the simulator's: scan (t, f) draws
 * under scan.seed + f0 + f, beam b taking normal draw (msg0 + t)*n_beams + b of stream 6, msg0 the
 * simulator's message counter before the run — the bits of lm_simulate called per filter with that
 * seed and scan0 = msg0, so a run split into several calls, or a swarm split over ranks by f0,
 * gives the bits of the single call.
 * Afterwards `lm` holds the scans and the markers as after lm_simulate + lm_detect_device
 * (lm_fetch_ranges, lm_fetch_markers, lm_last_simulate_us); the filter handle is as after those
 * replays. Nothing crosses PCIe but the wheel commands; asynchronous (the host waits for nothing).
 * With collisions on (ekf_sim_set_collisions with the same obstacle_radius and a collision_radius
 * of at least the lidar's 0.032 m mount offset; cylinders that do not overlap) the truth poses
 * keep the lidar out of every cylinder; with them off the caller keeps the drive clear of the
 * cylinders, as a lidar inside one is outside the laser's documented domain (lidar_kernels.hip).
 * EKF_E_ARG, and nothing changes and no counter advances: a NULL simulator, lm or cfg; T < 0, NULL
 * wheel_cmd with T > 0; T*F > lm's max_scans; n_beams outside [2, lm's max_beams]; max_markers
 * outside [1, 64]; obstacle_radius negative or NaN; an invalid scan (lm_simulate's rules:
 * sigma < 0 or NaN, range_min > range_max); the two handles on different devices; a pipeline
 * filter handle on the one-marker route (ekf_get_assoc_route: EKF_ASSOC_MARKER). T == 0: EKF_OK. */
typedef struct {
  int n_beams;             /* 360 */
  int max_markers;         /* detections kept per scan, 1..64; 32 */
  double threshold;        /* cluster break, 0.2 */
  double obstacle_radius;  /* every landmark's cylinder radius, 0.038 */
  lm_scan_config scan;     /* seed, arena, range_min/max, sigma; scan0 is ignored (the simulator's
                              message counter takes its place) */
} ekf_sim_lidar_config;
void ekf_sim_lidar_config_default(ekf_sim_lidar_config*);
int ekf_sim_run_lidar(ekf_sim_t s, lm_t lm, int T, const double* wheel_cmd,
                      const ekf_sim_lidar_config* cfg);

/* Monte-Carlo from a common prior: every filter of dst continues src_filter's run under its own
 * seed (dst's seed + f0 + f), on the device.
 *   The filters: ekf_copy_state(dst's handle, -1, src's handle, src_filter) (ekf.h), the handle's
 *     t_odom_robot included.
 *   The simulator: src_filter's true and odometry poses (with the collision count 0), its sighted
 *     set and its map landmarks[src_filter][L][2] into every dst filter; dst's tick and message
 *     counters become src's, so the draw indices go on from where the source's run stands.
 * The two simulators must agree on L, ticks_per_msg, wheel_radius, track_width and the start pose
 * (the map frame of ekf_sim_eval: a forked swarm scores in the source's frame); slip, sensor_sigma,
 * max_range, max_markers, marker_stride, seed, f0 and the collision setting may differ.
 * dst == src forks one filter over its own swarm; src_filter itself is left untouched.
 * Synchronises. EKF_E_ARG, with nothing changed and no counter moved: a NULL simulator, src_filter
 * out of range, a configuration mismatch, anything ekf_copy_state rejects (a smaller destination N,
 * another device). */
int ekf_sim_fork(ekf_sim_t dst, ekf_sim_t src, int src_filter);

/* Collisions with the map's cylinders (nusim.cpp:232-254), for ekf_sim_run, ekf_sim_run_assoc and
 * ekf_sim_run_lidar alike. Once per tick, after FKin, with the true pose at (x, y, θ) the landmarks
 * are tested in id order, R = collision_radius + obstacle_radius:
 *   d = sqrt((x − lx)·(x − lx) + (y − ly)·(y − ly));  if d < R:  a = atan2(ly − y, lx − x),
 *   x ← x − (R − d)·cos a,  y ← y − (R − d)·sin a,  θ kept, and no further landmark is tested in
 *   this tick (only the lowest colliding id acts).
 * The next tick's arc composes onto the corrected pose; the odometry is untouched (the encoders
 * report the commanded angles), so it runs away from the truth while the robot is held. At d = 0
 * the push goes along −x (atan2(0, 0) = 0). nusim's TF broadcast inside that loop is not mirrored.
 * collision_radius > 0 turns collisions on from the next run; 0 turns them off (the default: the
 * simulator then launches the same kernels and gives the same bits as without this call, and so
 * does a run with collisions on in which nothing is hit). obstacle_radius >= 0 is every landmark's
 * cylinder radius. EKF_E_ARG, nothing changes: NULL simulator, a negative or NaN radius. */
int ekf_sim_set_collisions(ekf_sim_t s, double collision_radius, double obstacle_radius);

/* total[F]: colliding ticks per filter since ekf_sim_create. per_msg[T][F] (nullable; needs
 * cfg.record): colliding ticks in each message of the last run. Synchronises. EKF_E_ARG: a NULL
 * simulator or total, per_msg without cfg.record. */
int ekf_sim_collisions(ekf_sim_t s, long long* total, int* per_msg);

/* A development hook, not part of the simulation's interface: measurement
 * (tools/sim_collide_bench.py), as lm_last_simulate_us is for the laser. A simulator created with EKF_SIM_TIMING=1 in the
 * environment records HIP events around each run's simulator launches (the wheel walk and the
 * sensing, on the simulator's stream; not the filter's work); us gets the last run's time between
 * them, in µs. Waits for that run's simulation. EKF_E_ARG: a NULL simulator or us, a simulator
 * created without EKF_SIM_TIMING, no run yet. */
int ekf_sim_last_us(ekf_sim_t s, double* us);

/* With cfg.record: the last run's inputs as ekf_replay would take them — counts[T][F],
 * ids/actions[T][F][M], rel_xy[T][F][M][2] (M = marker_stride) — and odom[T][3] (t_odom_robot) and
 * truth[T][F][3] (θ, x, y). Synchronises. */
int ekf_sim_markers(ekf_sim_t s, int* counts, int* ids, int* actions, double* rel_xy);
int ekf_sim_poses(ekf_sim_t s, double* odom, double* truth);

/* Scores every filter of the handle against the simulator's own truth (ekf_eval, ekf.h): each
 * filter's true pose after the last simulated tick and its map landmarks[F][L][2], both where the
 * simulator keeps them on the device, with frame = (start_theta, start_x, start_y) — the filter
 * starts at 0 where the truth starts at the configured pose. The truth never visits the host; only
 * out[F] comes back. Needs no cfg.record. Synchronises; the filter is left alone as by ekf_eval.
 * EKF_E_ARG: a NULL simulator or out. */
int ekf_sim_eval(ekf_sim_t s, ekf_eval_rec* out);

/* ekf_eval_match (ekf.h) fed the same device-resident truth: each filter's true pose, its map
 * landmarks[F][L][2] as the truth in any order (n_map = L), frame = the start pose. out[F];
 * match_out[F] and match[F][N] (N = the handle's n_landmarks) are nullable. The truth never visits
 * the host. Synchronises; the filter is left alone. EKF_E_ARG: a NULL simulator or out, max_dist
 * negative or NaN. */
int ekf_sim_eval_match(ekf_sim_t s, double max_dist, ekf_eval_rec* out, ekf_match_rec* match_out,
                       int* match);

#ifdef __cplusplus
}
#endif
#endif
