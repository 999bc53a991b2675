/*
 * landmarks.h — C-ABI of the MI355X-native lidar landmark front-end (libekfslam.so).
 *
 * Drop-in for the producer of the association path's input in maxipalay/ekf-slam: the
 * `landmarks` node (nuslam/src/landmarks.cpp) and turtlelib's circle classification / fitting
 * (turtlelib/src/landmark_detection.cpp). Its MarkerArray output is what `slam`'s sensor_cb
 * consumes (ekf_sensor / slam_markers with SOURCE_ASSOC). SURVEY.md §8f row 1.
 * Its input can be made on the device too: lm_simulate is nusim's simulated laser
 * (nusim/src/nusim.cpp:559-710), and lm_detect_resident detects on its scans where they lie.
 *
 * Batched: one call takes S scans (independent robots / filters of a Monte-Carlo swarm, or
 * consecutive scans of one robot), one wavefront per scan on the GPU. Plain C types only; every
 * call returns an EKF_* status code (ekf.h) and never throws. One handle is not thread-safe;
 * calls synchronise the handle's stream before returning host results.
 */
#ifndef EKFSLAM_LANDMARKS_H
#define EKFSLAM_LANDMARKS_H
#include "ekf.h" /* status codes, ekf_t (lm_replay_into) */
#ifdef __cplusplus
extern "C" {
#endif

#define LM_MAX_BEAMS 2048       /* beams per scan (LDS-resident)                           */
#define LM_MAX_CIRCLES 1024     /* cylinders per simulated scene (LDS-resident)              */
#define LM_MAX_CLUSTER 39       /* clusters of 4..39 points are fitted (landmarks.cpp:122)  */
#define LM_NO_BREAK (-1)        /* per-scan count: the scan has no cluster break; the
                                   reference throws at clusters.at(0) (landmarks.cpp:94)    */

typedef struct lm_ctx* lm_t;

/* One detected obstacle: visualization_msgs::Marker fields the slam node reads
 * (landmarks.cpp:146-148): id = index among circle-classified clusters, (x, y) = circle centre
 * in the laser frame, r = fitted radius (the marker's scale is 2r). */
typedef struct {
  double x, y, r;
  int id;
  int pad;
} lm_marker;

/* Handle with device buffers for up to max_scans scans of max_beams beams (≤ LM_MAX_BEAMS). */
int lm_create(lm_t* out, int max_scans, int max_beams, int device);
int lm_destroy(lm_t h);

/* Landmarks::laserCallback (landmarks.cpp:109-156) for S scans of B beams each.
 *   ranges       [S][B] float (sensor_msgs/LaserScan::ranges)
 *   angle_min    [S], angle_inc [S]: the messages' angle_min / angle_increment
 *   threshold    cluster break distance (landmarks.cpp:195: 0.2)
 *   markers      [S][max_markers] out; counts [S] out: published markers of each scan (those
 *                beyond max_markers are counted, not written), or LM_NO_BREAK.
 * Beam i's point is r_i·(cos, sin)(normalize_angle(i·inc) + angle_min) − (0.032, 0)
 * (landmarks.cpp:66-70). Returns EKF_OK even when some scans report LM_NO_BREAK. */
int lm_detect(lm_t h, int n_scans, int n_beams, const float* ranges, const double* angle_min,
              const double* angle_inc, double threshold, lm_marker* markers, int max_markers,
              int* counts);

/* turtlelib::fitCircle (landmark_detection.cpp:50-135) on n_clusters point sets: cluster c is
 * xy[2·offsets[c] .. 2·offsets[c+1]) as (x, y) pairs; out[3c..3c+2] = (c_x, c_y, R).
 * Any cluster size ≥ 1 (the node only fits 4..39 points). */
int lm_fit_circles(lm_t h, int n_clusters, const int* offsets, const double* xy, double* out);

/* turtlelib::checkCircle (landmark_detection.cpp:5-48) on the same layout; out[c] = 0 / 1.
 * Clusters need ≥ 3 points (the reference's angle vector has size − 2 entries). */
int lm_check_circles(lm_t h, int n_clusters, const int* offsets, const double* xy, int* out);

/* Per-kernel device time of the last lm_detect / lm_detect_resident (HIP events around the
 * dispatch), microseconds. */
int lm_last_kernel_us(lm_t h, double* us);

/* nusim's simulated laser (publish_lidar_data, nusim/src/nusim.cpp:559-710) for S scans on the
 * device: beam b of a scan taken at body pose (θ, x, y) leaves the lidar, mounted 0.032 m behind
 * the body origin, along θ + b·2π/B; its range is the nearest hit among the scene's cylinders and
 * the four walls of an axis-aligned arena centred on the origin, clamped to
 * [range_min, range_max], plus sigma·N(0, 1), rounded to float. The normal draw of beam b of scan
 * s is draw (scan0 + s)·B + b of stream 6 under `seed` (pyekf.synth's counter-based RNG), so a
 * run split into several calls by scan0 gives the bits of one call; sigma = 0 draws nothing. */
typedef struct {
  unsigned long long seed; long long scan0;   /* draw index base, see above (>= 0) */
  double arena_w, arena_h;                    /* default 10, 5 */
  double range_min, range_max;                /* 0.11, 10.0 (nusim.cpp:570-571) */
  double sigma;                               /* 0: noiseless (>= 0) */
} lm_scan_config;
void lm_scan_config_default(lm_scan_config*);

/* poses[S][3]; circles[G][C][3]; scene[S] in [0,G) or NULL (all scans use scene 0).
 * Leaves the scans resident in the handle (angle_min 0, angle_increment float32(2π/B) widened
 * to double); ranges_out nullable: a host copy, which makes the call synchronous. Without it the
 * call returns once the inputs are uploaded (they may be freed), the kernel still in flight on
 * the handle's stream. n_circles = 0 (walls only) is valid, and then circles may be NULL.
 * EKF_E_ARG: n_scans outside [1, max_scans], n_beams outside [2, max_beams], n_circles outside
 * [0, LM_MAX_CIRCLES], n_scenes < 1, a scene index outside [0, n_scenes), a NULL poses / cfg (or
 * circles with n_circles > 0), or a configuration with range_min > range_max. */
int lm_simulate(lm_t h, int n_scans, int n_beams, const double* poses, int n_scenes,
                int n_circles, const double* circles, const int* scene,
                const lm_scan_config* cfg, float* ranges_out);
/* lm_detect on the resident scans of the last lm_simulate: no range upload. EKF_E_ARG when
 * nothing is resident (no lm_simulate yet, or an lm_detect since overwrote the range buffer). */
int lm_detect_resident(lm_t h, double threshold, lm_marker* markers, int max_markers, int* counts);
/* Device time of the last scan kernel, lm_simulate's or ekf_sim_run_lidar's (ekf_sim.h), from HIP
 * events around the dispatch, microseconds. */
int lm_last_simulate_us(lm_t h, double* us);
/* The resident scans (the last lm_simulate's or ekf_sim_run_lidar's) to the host: out
 * [n_scans][n_beams] float, synchronising; for tests and inspection. EKF_E_ARG when nothing is
 * resident. */
int lm_fetch_ranges(lm_t h, float* out);

/* ---- scans to posterior without a host hop ---- */

/* lm_detect without the copy back: markers [n_scans][max_markers] and counts [n_scans] stay in
 * the handle (1 <= max_markers). Asynchronous: the call returns once the caller's scans are
 * uploaded (they may be freed), the detection still in flight on the handle's stream.
 * ranges == NULL: detect on the resident scans of the last lm_simulate (as lm_detect_resident;
 * n_scans, n_beams and the angle arrays are then ignored). The results stay until the handle's
 * next detect of any form. */
int lm_detect_device(lm_t h, int n_scans, int n_beams, const float* ranges,
                     const double* angle_min, const double* angle_inc, double threshold,
                     int max_markers);
/* The last lm_detect_device's results to the host (synchronising; for tests and inspection):
 * counts [n_scans] (nullable when markers are asked for), markers [n_scans][max_markers]
 * (columns beyond the detect's own max_markers are left untouched). */
int lm_fetch_markers(lm_t h, lm_marker* markers, int max_markers, int* counts);
/* Feed them to a filter handle on the same device as T messages of unknown association
 * (ekf_replay_device_assoc, ekf.h: Slam::sensor_cb per message): scan s = t*F + f is message t of
 * filter f, so n_scans of the last lm_detect_device must equal T*F, and m_max = its max_markers
 * (<= 64). odom[T][F][3] on the host, t_odom_robot per message (copied before the call returns).
 * A scan that published nothing (count 0 or LM_NO_BREAK, landmarks.cpp:153) is no message; a
 * count above max_markers is clamped to it. The filter's planning stream waits on the device for
 * the detection, and the handle's next detect waits on the device until the filter has planned
 * from the marker buffer: asynchronous on both handles, nothing crosses PCIe but odom.
 * EKF_E_ARG: nothing detected yet, T*F != n_scans, max_markers > 64, handles on different
 * devices, or a filter handle ekf_replay_device_assoc refuses (a resident one: it has
 * lm_replay_resident). */
int lm_replay_into(lm_t h, ekf_t e, int T, const double* odom);
/* lm_replay_into for a resident filter handle: same contract otherwise. The messages run as
 * ekf_replay_resident with assoc = 1 (ekf.h), one kernel launch that reads the marker buffer in
 * place throughout, so the handle's next detect waits on the device until that kernel has ended.
 * EKF_E_ARG: what lm_replay_into lists, with "a pipeline filter handle" for its last item. */
int lm_replay_resident(lm_t h, ekf_t e, int T, const double* odom);

#ifdef __cplusplus
}
#endif
#endif
