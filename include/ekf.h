/*
 * ekf.h — C-ABI of the MI355X-native EKF-SLAM update path (libekfslam.so).
 *
 * Drop-in boundary for the EKF inside maxipalay/ekf-slam's `slam` node (nuslam/src/slam.cpp).
 * The reference has no predict()/update()/associate() functions: the filter is inline code inside
 * two ROS 2 subscription callbacks. Each entry point below names the reference lines it replaces.
 * Plain C types only (no HIP / torch types); every call returns a status code and never throws.
 *
 * Threading: one handle is not thread-safe (the reference runs every callback on one executor
 * thread, slam.cpp:683); distinct handles are independent. The handle owns its device memory and a
 * private HIP stream; host arrays are caller-owned and copied in. Calls are asynchronous on the
 * handle's stream unless stated otherwise; ekf_get_* and ekf_sync synchronise.
 */
#ifndef EKFSLAM_EKF_H
#define EKFSLAM_EKF_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define EKF_OK 0
#define EKF_E_ARG (-1)     /* bad argument / handle */
#define EKF_E_RANGE (-2)   /* landmark id >= N, or counter_obstacles overflow: the reference's
                              Armadillo bounds check throws (slam.cpp:213, :351) */
#define EKF_E_EMPTY (-3)   /* empty MarkerArray: the reference throws at msg.markers.at(0)
                              (slam.cpp:281, :498) */
#define EKF_E_NUMERIC (-4) /* singular or non-finite innovation covariance S (slam.cpp:252): that
                              marker's correction was skipped (a first sighting keeps its landmark
                              and counter). Returned by the synchronous forms only — ekf_sensor and
                              ekf_associate_correct with decision outputs — by every call that
                              skipped a marker itself (skips of earlier asynchronous calls are not
                              charged to it); EKF_E_RANGE takes precedence when both apply. Every
                              asynchronous form reports a skip through EKF_FLAG_NUMERIC alone;
                              ekf_get_status shows the flag after either kind of call. */
#define EKF_E_HIP (-5)     /* HIP runtime error */
#define EKF_E_NOMEM (-6)
#define EKF_E_TIMEOUT (-7) /* a device hand-off (cross-stream epoch or k_assoc_msg's exchange
                              between a filter's workgroups) was not seen within its bounded poll:
                              the flagged filters' state after that message is undefined. Reported
                              once by the next ekf_sync / ekf_sensor / ekf_associate_correct;
                              ekf_get_status names the filters (EKF_FLAG_TIMEOUT). No reference
                              counterpart (the reference has no device). */

/* status flag bits (ekf_get_status), accumulated on the device */
#define EKF_FLAG_RANGE 1u   /* a marker was skipped: id >= N / map full (slam.cpp:213, :351) */
#define EKF_FLAG_NUMERIC 2u /* a marker was skipped: S singular or non-finite (slam.cpp:252) */
#define EKF_FLAG_TIMEOUT 4u /* a device poll timed out: this filter's state is undefined
                               (EKF_E_TIMEOUT) */

#define EKF_F64 0
#define EKF_F32 1 /* Σ stored and contracted in fp32; state and all O(n) math stay fp64 */

#define EKF_MARKER_ADD 0
#define EKF_MARKER_DELETE 2 /* visualization_msgs::msg::Marker::DELETE (skipped, slam.cpp:205) */

#define EKF_MAX_CHUNK 16 /* markers folded into one Σ pass; longer messages are split */

typedef struct ekf_ctx* ekf_t;

/* Filter parameters. Defaults = the reference's hard-coded members (slam.cpp:665-671, :130). */
typedef struct {
  int n_landmarks; /* N, state dim n = 3 + 2N (slam.cpp:665: 50)                 */
  int n_filters;   /* independent filters in one handle (Monte-Carlo swarm); 1 = one slam node */
  int dtype;       /* EKF_F64 | EKF_F32                                              */
  double q_noise;  /* Q̄ = q·I₃ on the pose block (slam.cpp:135-136, :666: 1e-2)     */
  double r_noise;  /* R = r·I₂ (slam.cpp:139, :667: 1e-2)                          */
  double init_var; /* landmark prior variance (slam.cpp:130: 10e6 = 1e7)           */
  double mah_gate; /* Mahalanobis gate on the squared distance (slam.cpp:671: 2.0)  */
  int device;      /* HIP device ordinal                                            */
} ekf_config;

void ekf_config_default(ekf_config* cfg);
const char* ekf_strerror(int status);

/* Filter construction: Σ₀ = diag(0,0,0, init_var·I_2N), state = 0, Q̄, R (slam.cpp:127-139, :674). */
int ekf_create(ekf_t* out, const ekf_config* cfg);
int ekf_destroy(ekf_t h);
/* n = 3+2N, ld = Σ row stride in elements, n_filters */
int ekf_dims(ekf_t h, int* n, int* ld, int* n_filters);

/* Which device path the handle runs (fixed at ekf_create):
 *   EKF_PATH_PIPELINE  Σ in HBM; per chunk of ≤ EKF_MAX_CHUNK markers a chain, a factor kernel and
 *                      one low-rank Σ pass (any n, fp64 or fp32);
 *   EKF_PATH_RESIDENT  fp64 with n ≤ EKF_RESIDENT_MAX_N (the reference's N = 50 map): one launch
 *                      per upload, Σ held in a workgroup's registers across all its messages.
 * The environment variable EKF_RESIDENT=0 forces the pipeline (both give the same results up to
 * summation order). */
#define EKF_PATH_PIPELINE 0
#define EKF_PATH_RESIDENT 1
#define EKF_RESIDENT_MAX_N 128
int ekf_get_path(ekf_t h, int* path);

/* How unknown association (ekf_sensor, ekf_associate_correct, assoc replays) runs on the pipeline
 * (fixed at ekf_create; same decisions either way, slam.cpp:344-440):
 *   EKF_ASSOC_CHUNK_XCD  a chunk of <= EKF_MAX_CHUNK markers per launch, one workgroup per 64
 *                        landmark slots, a filter's workgroups on one XCD exchanging through its L2;
 *   EKF_ASSOC_CHUNK      the same kernel with the workgroups anywhere (agent-coherent exchange;
 *                        EKF_AM_XCD=0 forces it);
 *   EKF_ASSOC_MARKER     one marker per launch (resident path, EKF_ASSOC_MSG=0, or a map whose
 *                        ceil(N/64) workgroups the CUs cannot hold at once).
 * The Joseph form (ekf_set_joseph) takes the chunk routes too, with its own kernel instantiation;
 * the route reported is the one in effect for the current form. */
#define EKF_ASSOC_MARKER 0
#define EKF_ASSOC_CHUNK 1
#define EKF_ASSOC_CHUNK_XCD 2
int ekf_get_assoc_route(ekf_t h, int* route);

/* The handle's schedule (fixed at ekf_create), bit flags:
 *   EKF_SCHED_DEVSYNC  <= 32 filters: the chain and bulk streams get disjoint CU masks and hand off
 *                      through device epochs (EKF_DEVSYNC=0: HIP events between the two streams);
 *   EKF_SCHED_SERIAL   every kernel on one stream. The default for > 32 filters (their Σ passes
 *                      fill every CU, so two streams overlap nothing; the staged rebuild operands
 *                      are off there too, EKF_STAGE=1 restores them); EKF_SERIAL=1 forces it for
 *                      any handle, EKF_SERIAL=0 keeps two streams (HIP events) for > 32 filters.
 * Every schedule gives bit-identical results.
 *   EKF_SCHED_BUILDER  deprecated: a block-builder schedule of earlier releases, retired; the bit is
 *                      never set (the name stays so that code written against it still compiles). */
#define EKF_SCHED_DEVSYNC 1
#define EKF_SCHED_BUILDER 2
#define EKF_SCHED_SERIAL 4
int ekf_get_schedule(ekf_t h, int* flags);

/* ---- the callbacks (fast path) ---- */

/* t_odom_robot ← DiffDrive::FKin output (slam.cpp:633, jointStateCallback :599-634). */
int ekf_set_odom(ekf_t h, int filter, double theta, double x, double y);

/* Slam::fake_sensor_cb (slam.cpp:180-316) minus ROS publishing: predict with the current
 * t_odom_robot, one correction per non-DELETE marker (ids known), posterior t_map_odom.
 * ids are validated before anything changes (EKF_E_RANGE). rel_xy = body-frame (x, y) pairs. */
int ekf_fake_sensor(ekf_t h, int filter, int m, const int* ids, const int* actions,
                    const double* rel_xy);

/* Slam::sensor_cb (slam.cpp:318-530) minus ROS publishing: predict, then per marker the
 * Mahalanobis nearest-neighbour association (:344-440) and the correction (:443-488).
 * If assoc_out/is_new_out are non-NULL the call synchronises and returns the decisions, and
 * EKF_E_RANGE (a marker met a full map) or else EKF_E_NUMERIC (a marker's correction was skipped)
 * as the oracle's sensor_cb does; without outputs it is asynchronous and both are reported through
 * ekf_get_status only. */
int ekf_sensor(ekf_t h, int filter, int m, const double* rel_xy, int* assoc_out,
               int* is_new_out);

/* All filters of the handle at once, one message per filter (the swarm / replay path).
 * counts[F], ids/actions[F][m_max], rel_xy[F][m_max][2], odom[F][3] (t_odom_robot per filter,
 * NULL = keep). ids may be NULL with assoc=1 (unknown association). Asynchronous.
 * counts[f] == 0: filter f gets no message this step and nothing of it changes (as ekf_fake_sensor
 * rejects an empty array, EKF_E_EMPTY: the reference throws at msg.markers.at(0), slam.cpp:281);
 * a message whose markers are all DELETE is a predict + posterior (slam.cpp:205). */
int ekf_batch_sensor(ekf_t h, int assoc, int m_max, const int* counts, const int* ids,
                     const int* actions, const double* rel_xy, const double* odom);

/* Replay T messages through ekf_batch_sensor (arrays as there, with a leading [T] axis):
 * counts[T][F], ids/actions[T][F][m_max], rel_xy[T][F][m_max][2], odom[T][F][3].
 * out_pose[T][F][3] (nullable) receives each posterior pose and makes every message synchronous;
 * the pose trace below (ekf_trace_enable) records the same poses without that. */
int ekf_replay(ekf_t h, int assoc, int T, int m_max, const int* counts, const int* ids,
               const int* actions, const double* rel_xy, const double* odom, double* out_pose);

/* ekf_replay with known ids (assoc = 0) whose inputs already live in device memory of the
 * handle's GPU (same layouts; d_actions nullable): the descriptors are planned on the GPU (one
 * chunk per message, so m_max <= EKF_MAX_CHUNK, in either form; no resident handle: EKF_E_ARG)
 * and no input crosses PCIe. The measurement (range, bearing) of slam.cpp:208-210 is computed on
 * the GPU (correctly rounded sqrt; the bearing's atan2 may differ from glibc's in the last bit).
 * Inputs are not validated on the host: an id outside [0, N) is skipped by the correction and
 * sets EKF_FLAG_RANGE in the filter's status. Asynchronous; the inputs must stay valid until the
 * next synchronising call (ekf_sync, a state read). The handle's planning state comes back to the
 * host at the next host-planned call or state access.
 * A resident handle (EKF_PATH_RESIDENT) takes ekf_replay_resident with assoc = 0 instead. */
int ekf_replay_device(ekf_t h, int T, int m_max, const int* d_counts, const int* d_ids,
                      const int* d_actions, const double* d_rel_xy, const double* d_odom);

/* ekf_replay with unknown association (assoc = 1, Slam::sensor_cb, slam.cpp:318-530, per message)
 * whose inputs already live in device memory of the handle's GPU: the chunk descriptors are
 * planned on the GPU and no input crosses PCIe.
 *   d_counts  [T][F] int. A count <= 0 is no message: `landmarks` published nothing for that scan
 *             (an empty detection, landmarks.cpp:153, or LM_NO_BREAK = -1) and nothing of the
 *             filter changes. A count above m_max is clamped to m_max: lm_detect counts the
 *             markers beyond its capacity but does not write them.
 *   d_xy      marker i of message t of filter f is the two doubles at
 *             d_xy[((t*F + f)*m_max + i)*xy_stride + {0, 1}]: xy_stride = 2 is rel_xy[T][F][m_max][2],
 *             xy_stride = 4 an lm_marker[T*F][m_max] array read in place (landmarks.h).
 *   d_odom    [T][F][3], t_odom_robot per message.
 * 1 <= m_max <= 64, so that a message's decisions all stay readable (ekf_get_decisions).
 * Pipeline handles on a chunk route only (ekf_get_assoc_route: EKF_ASSOC_CHUNK or
 * EKF_ASSOC_CHUNK_XCD), either form, both dtypes. EKF_E_ARG, and nothing changes: a resident
 * handle, the one-marker route, T < 1, m_max outside [1, 64], xy_stride < 2, a NULL d_counts /
 * d_xy / d_odom. The measurement (range, bearing) of slam.cpp:346-347 is computed on the GPU:
 * the range with a correctly rounded sqrt, the bearing's atan2 in double-double arithmetic and
 * rounded once, so it can differ from glibc's only in the last bit and only where glibc's own is
 * not the correctly rounded value (about one argument in a thousand).
 * Every message costs ceil(m_max / 16) launch pairs whatever its count, so choose m_max no larger
 * than needed. Asynchronous; the inputs must stay valid until the next synchronising call
 * (ekf_sync, a state read). A full map and skipped markers are reported through ekf_get_status.
 * The handle's planning state comes back to the host at the next host-planned call or state
 * access.
 * A resident handle (EKF_PATH_RESIDENT) takes ekf_replay_resident with assoc = 1 instead. */
int ekf_replay_device_assoc(ekf_t h, int T, int m_max, const int* d_counts, const double* d_xy,
                            int xy_stride, const double* d_odom);

/* Resident handles only (EKF_PATH_RESIDENT; a pipeline handle: EKF_E_ARG, it has ekf_replay_device
 * and ekf_replay_device_assoc). T messages per filter whose inputs already live on the handle's
 * GPU, run by ONE kernel launch, no descriptors, nothing crosses PCIe. assoc = 0: known ids
 * (d_ids required, d_actions nullable); assoc = 1: unknown association (d_ids/d_actions ignored).
 * 1 <= m_max <= 64, T >= 1, xy_stride >= 2. Either form (ekf_set_joseph). Asynchronous.
 *   d_counts  [T][F] int. A count <= 0 is no message: nothing of the filter changes (it is not
 *             even loaded if the whole replay holds no message for it). A count above m_max is
 *             clamped to m_max. Known ids: a message whose first min(count, m_max) markers are
 *             all DELETE is a predict + posterior (slam.cpp:205).
 *   d_ids, d_actions  [T][F][m_max] int, known ids only. Not validated on the host: an id outside
 *             [0, N) is skipped by the correction and sets EKF_FLAG_RANGE in the filter's status.
 *             A first sighting initialises its landmark (slam.cpp:213-216).
 *   d_xy      marker i of message t of filter f is the two doubles at
 *             d_xy[((t*F + f)*m_max + i)*xy_stride + {0, 1}], as ekf_replay_device_assoc's:
 *             xy_stride = 2 is rel_xy[T][F][m_max][2], 4 an lm_marker array read in place.
 *   d_odom    [T][F][3], t_odom_robot per message.
 * The measurement (range, bearing) of slam.cpp:208-210 / :346-347 is computed on the GPU, for both
 * kinds alike: the range x*x + y*y rounded product by product and a correctly rounded sqrt, the
 * bearing's atan2 in double-double arithmetic rounded once, so it differs from a host-planned
 * replay's only in the last bit and only where glibc's atan2 is not the correctly rounded value
 * (about one argument in a thousand).
 * Unknown association: marker i's decision lands in slot i (ekf_get_decisions shows the last
 * message's); a marker that meets a full map is skipped with decision -1 and EKF_FLAG_RANGE.
 * Skipped markers (EKF_FLAG_RANGE, EKF_FLAG_NUMERIC) are reported through ekf_get_status only.
 * The pose trace gets one record per message with count > 0, as from any other entry point.
 * EKF_E_ARG, and nothing changes: a NULL handle / d_counts / d_xy / d_odom, assoc = 0 with a NULL
 * d_ids, T < 1, m_max outside [1, 64], xy_stride < 2, a pipeline handle.
 * What the host planned before (deferred calls included) is submitted first. The inputs must stay
 * valid until the next synchronising call (ekf_sync, a state read): the kernel reads them
 * throughout. The handle's planning state comes back to the host at the next host-planned call
 * or state access; a later call of any kind continues from the state the replay left. */
int ekf_replay_resident(ekf_t h, int assoc, int T, int m_max, const int* d_counts,
                        const int* d_ids, const int* d_actions, const double* d_xy,
                        int xy_stride, const double* d_odom);

/* The decisions (slam.cpp:344-440) of `filter`'s most recent unknown-association message, its
 * first m <= 64 markers: assoc_out[i] = landmark slot, or -1 when the marker met a full map;
 * is_new_out[i] = 1 when it opened that slot. Either output may be NULL. After ekf_sensor,
 * ekf_batch_sensor / ekf_replay with assoc = 1, ekf_replay_device_assoc, ekf_replay_resident with
 * assoc = 1, lm_replay_into or lm_replay_resident; markers beyond the message's own count hold an
 * earlier message's decisions. Synchronises. */
int ekf_get_decisions(ekf_t h, int filter, int m, int* assoc_out, int* is_new_out);

/* ---- the finer-grained surface (north_star: predict()/update()/associate()) ---- */

/* Predict (slam.cpp:184-198): deferred and folded into the next Σ pass. */
int ekf_predict(ekf_t h, int filter);
/* One known-association correction (slam.cpp:207-268), predict folded in if pending. */
int ekf_correct(ekf_t h, int filter, int landmark_id, double rel_x, double rel_y);
/* One association + correction (slam.cpp:345-488). Synchronous when j/is_new non-NULL: then
 * EKF_E_RANGE (map full, *j = -1) or else EKF_E_NUMERIC (this marker's correction was skipped). */
int ekf_associate_correct(ekf_t h, int filter, double rel_x, double rel_y, int* j, int* is_new);
/* Posterior (slam.cpp:273-291): t_map_odom = T(x, y, θ)·t_odom_robot⁻¹. */
int ekf_posterior(ekf_t h, int filter);

/* Joseph-form covariance update, opt-in (off by default, like the reference, which applies
 * Σ ← (I − KH)Σ at slam.cpp:264-265): Σ ← (I − KH)Σ(I − KH)ᵀ + KRKᵀ for every later correction.
 * Equal in exact arithmetic with the optimal gain; it differs only in rounding. Resident path: its
 * own kernel instantiation. HBM pipeline (fp32 and fp64): the same chunks of <= 16 markers, each
 * folded into one Σ pass of rank 2 + 4m (K_c·M_c and (Σ_cHᵀ − K_c·S_c)·K_cᵀ per correction), so one
 * Σ pass per message as in the simple form. A switch makes each filter's next chunk gather its rows
 * from Σ (the chunk before cannot be rebuilt across forms). */
int ekf_set_joseph(ekf_t h, int on);

/* Deferred submission. While on, the callbacks above only plan their work on the host; the plan
 * goes to the device in one upload (and, on the resident path, one kernel launch) when it reaches
 * 8192 descriptors, when a synchronising call below needs the state, or when deferral is turned
 * off (which submits what is planned). Off by default: each callback is submitted as it is made.
 * A replay driver with no per-message outputs (slam_replay) turns it on, and so does one that takes
 * them from the pose trace (slam_replay_trace). */
int ekf_defer(ekf_t h, int on);

/* Back to the constructor's state (slam.cpp:127-139) on the device for filter `filter`, or every
 * filter when filter < 0: Σ₀, state 0, t_map_odom identity, counter 0, status clear. Host-side
 * odometry set by ekf_set_odom is kept. Synchronises. */
int ekf_reset(ekf_t h, int filter);

/* Submits what the host has planned (deferred callbacks included) without waiting for it: after
 * it, a device-wide synchronisation (hipDeviceSynchronize) covers all of the handle's work. */
int ekf_flush(ekf_t h);

/* ---- state access (synchronising) ---- */
/* Waits for everything submitted; EKF_E_TIMEOUT if a device hand-off timed out since the last
 * report (see EKF_E_TIMEOUT). */
int ekf_sync(ekf_t h);
int ekf_get_pose(ekf_t h, int filter, double* theta_x_y);
int ekf_get_map_odom(ekf_t h, int filter, double* theta_x_y); /* t_map_odom */
/* state[n] (fp64), sigma[n*n] row-major fp64 (nullable), counter (nullable) */
int ekf_get_state(ekf_t h, int filter, double* state, double* sigma, unsigned* counter);
/* overwrite a filter (fixtures / resync after an association flip); t_map_odom nullable.
 * fp64 pipeline handles keep Σ exactly symmetric (the Σ pass computes the upper triangle and
 * mirrors it), so sigma's upper triangle is taken and mirrored below the diagonal; the reference's
 * own (I − KH)Σ (slam.cpp:264-265) is symmetric up to rounding. fp32 and resident handles store
 * sigma as given. */
int ekf_set_state(ekf_t h, int filter, const double* state, const double* sigma,
                  const double* t_map_odom, unsigned counter);
int ekf_get_status(ekf_t h, int filter, unsigned* flags); /* and clears them */

/* ---- fork and hand over filter state on the device ---- */
/* A filter's state from one handle into another without the host: what
 *   ekf_get_state(src, fs, x, S, &cnt); ekf_get_map_odom(src, fs, tmo);
 *   ekf_set_state(dst, fd, x', S', tmo, cnt); ekf_set_odom(dst, fd, src's t_odom_robot)
 * leaves, bit for bit, by one copy-and-convert kernel over Σ (no n × ld Σ crosses PCIe, 2.1 MB per
 * filter at N = 256, and any number of filters go in one call).
 *   dst_filter >= 0, src_filter >= 0   one filter onto one filter;
 *   dst_filter <  0, src_filter >= 0   a fork: every filter of dst receives src_filter's state;
 *   both < 0                           a swarm hand-over: filter f receives filter f (equal
 *                                      n_filters);
 *   dst_filter >= 0, src_filter <  0   EKF_E_ARG.
 * dst == src is allowed (a fork inside one swarm); a filter copied onto itself is skipped entirely.
 * Any pairing of resident fp64, pipeline fp64 and pipeline fp32 handles on one device, with
 * N_dst >= N_src. A larger destination is padded with the constructor's state (x', S'): state 0,
 * dst's init_var on the new diagonal entries, 0 everywhere else.
 * The rules of ekf_get_state / ekf_set_state hold: the source element is widened to double exactly;
 * an fp64 destination stores it, an fp32 destination its static_cast<float>; an fp64 pipeline
 * destination takes the element on or above the diagonal and mirrors it below (its Σ pass relies on
 * exact symmetry, and resident and fp32 sources are symmetric only up to rounding), every other
 * destination stores Σ as given; columns n..ld of every written row are written as zero. Both
 * handles are settled first (what is planned runs, both streams drain, a device replay's planning
 * state is adopted); the data is read from the source's and written to the destination's current
 * copy, and the destination forgets what ekf_set_state makes it forget.
 * Two things the host route cannot carry make the copy a clone, whose next message does what the
 * source's next message would: src's host-side t_odom_robot (after a device replay or a simulator
 * run, the run's last odometry pose) and src's pending predict (ekf_predict).
 * The destination's status flags, decisions, pose trace, ekf_chain_path_counts counters and Joseph
 * setting are left alone; the source is only read. Synchronises, like ekf_reset.
 * EKF_E_ARG, detected before anything is touched: a NULL handle, a filter index out of range, the
 * forbidden sign combination, unequal n_filters in the swarm form, N_dst < N_src, handles on
 * different devices. */
int ekf_copy_state(ekf_t dst, int dst_filter, ekf_t src, int src_filter);

/* ---- the pose trace: every message's posterior, recorded on the device ---- */
/* The per-message outputs of the reference node (the posterior pose and t_map_odom it publishes as
 * TF, green/odom and green/path after every MarkerArray, slam.cpp:273-291) without a
 * synchronisation per message: the kernels append them to a per-filter buffer in device memory,
 * read back whenever the caller likes.
 *   Off by default. A handle that never enables the trace behaves exactly as without it, bit for
 *     bit, with the same launches.
 *   One record per posterior: a filter gets a record wherever a kernel stores its t_map_odom, i.e.
 *     once per message, in whichever form it arrived (ekf_fake_sensor, ekf_sensor,
 *     ekf_batch_sensor, ekf_replay, ekf_replay_device, ekf_replay_device_assoc,
 *     ekf_replay_resident, lm_replay_into, lm_replay_resident, ekf_sim_run; deferred or not),
 *     and once per ekf_posterior. A message a filter sits out (count <= 0) appends nothing; a
 *     message whose markers are all DELETE (predict + posterior) appends one; a message split over
 *     several chunks appends one, from its last chunk.
 *   Beyond `capacity`, records are counted, not written (as lm_detect counts the markers beyond
 *     max_markers): ekf_trace_count returns how many were appended, ekf_trace_read copies
 *     [first, first + n) ∩ [0, min(appended, capacity)) and sets *got to how many that is.
 *   ekf_trace_enable, _count, _read and _clear synchronise like ekf_get_* (they submit what is
 *     planned and wait for both streams).
 *   ekf_trace_enable on a handle that already traces reallocates and clears; capacity 0 turns the
 *     trace off and frees it. ekf_reset(h, f) restarts filter f's trace at record 0 (every
 *     filter's for f < 0); ekf_set_state leaves it alone. With the trace on, the filter's state,
 *     Σ, decisions and status are bit-identical to the trace being off.
 *   EKF_E_ARG: a NULL handle or output, capacity < 0, filter out of range, ekf_trace_count / _read /
 *     _clear on a handle whose trace is off, first < 0, n < 0. EKF_E_NOMEM: the
 *     n_filters·capacity·64 bytes cannot be allocated; nothing changes then. */
typedef struct {      /* 64 bytes, one per posterior */
  double pose[3];     /* state(0..2) = (θ, x, y) after the message's corrections */
  double map_odom[3]; /* t_map_odom = T(x, y, θ)·t_odom_robot⁻¹ as stored for the filter */
  long long seq;      /* index of this record in the filter's trace (0, 1, …) */
  long long reserved; /* 0 */
} ekf_trace_rec;

int ekf_trace_enable(ekf_t h, int capacity); /* records kept per filter; 0 = off and freed */
int ekf_trace_count(ekf_t h, int filter, long long* appended);
int ekf_trace_read(ekf_t h, int filter, long long first, int n, ekf_trace_rec* out, int* got);
int ekf_trace_clear(ekf_t h, int filter); /* filter < 0: every filter */

/* ---- marginals and scoring: the parts of Σ a consumer needs, gathered on the device ---- */
/* ekf_get_state copies a filter's whole n × ld Σ (2.1 MB at N = 256). What a node draws (the
 * covariance ellipses that go with green/obstacles) and what a Monte-Carlo run is scored by need
 * the 3 × 3 pose block and the N diagonal 2 × 2 landmark blocks only: a kernel gathers those from
 * where they lie and, for a score, reduces them against the truth on the device.
 *   Every call here synchronises like ekf_get_* (it submits what is planned and waits for both
 *     streams), runs its kernel on the handle's stream and copies the result back.
 *   The filter is left alone: Σ, the state, the status flags, the decisions, the pose trace and the
 *     planning state are only read, so a replay continued after one of these calls gives the bits
 *     it gives after an ekf_get_pose in its place.
 *   Blocks are widened to fp64 and symmetrised, ½(Σ[i][j] + Σ[j][i]): fp32 and resident handles keep
 *     Σ symmetric only up to rounding.
 *   A landmark slot is `seen` unless both its coordinates are exactly 0, the reference's own
 *     first-sighting test (slam.cpp:213). */
typedef struct {
  double xy[2];  /* state(3 + 2j), state(4 + 2j) */
  double cov[3]; /* xx, xy, yy of the slot's 2 × 2 block */
  int seen;
  int pad;       /* 0 */
} ekf_lm_marginal; /* 48 bytes */

/* pose[3] = state(0..2); pose_cov[9] row-major (θ, x, y); lm[N]; counter = counter_obstacles. Every
 * output is nullable. filter < 0: every filter, and each array gets a leading [n_filters] axis.
 * EKF_E_ARG: a NULL handle, filter >= n_filters. */
int ekf_get_marginals(ekf_t h, int filter, double* pose, double* pose_cov, ekf_lm_marginal* lm,
                      unsigned* counter);

#define EKF_EVAL_POSE_NOT_PD 1u /* the pose block is not positive definite: pose_nees is NaN */
#define EKF_EVAL_LM_NOT_PD 2u   /* an evaluated landmark's block is not positive definite */

/* One filter's score against the truth.
 *   pose_err      (normalize_angle(θ̂ − θ), x̂ − x, ŷ − y)
 *   pose_cov      the symmetrised pose block: tt tx ty xx xy yy
 *   pose_nees     eᵀP⁻¹e by a 3 × 3 Cholesky (square-root free); a pivot <= 0 or not finite gives
 *                 NaN and EKF_EVAL_POSE_NOT_PD (a fresh filter's pose block is exactly 0)
 * A landmark slot j is evaluated when it is seen, j < n_map, and its truth is not NaN:
 *   n_seen, n_eval          seen slots; evaluated slots
 *   lm_sq_err, lm_max_err   Σ |p̂ − p|² and max |p̂ − p| over the evaluated slots
 *   lm_nees, n_nees         Σ of the 2 × 2 NEES over the evaluated slots whose block is positive
 *                           definite, and how many those are; any other evaluated slot sets
 *                           EKF_EVAL_LM_NOT_PD
 *   lm_var_trace            Σ of the blocks' traces over the seen slots
 * The sums are taken in one fixed order: the same state and truth give the same bytes. */
typedef struct {
  double pose_err[3];
  double pose_cov[6];
  double pose_nees, lm_sq_err, lm_nees, lm_max_err, lm_var_trace;
  int n_seen, n_eval, n_nees;
  unsigned flags; /* EKF_EVAL_* */
} ekf_eval_rec;   /* 128 bytes */

/* Scores every filter of the handle: truth_pose[F][3] (θ, x, y), truth_lm[F][n_map][2] (NULL with
 * n_map = 0: poses only), out[F]. A NaN coordinate in truth_lm marks "no truth for this slot"; a
 * caller whose association is unknown takes ekf_eval_match below, which finds the slot order itself.
 * frame[3] = (θ0, x0, y0) (nullable): the map frame's pose in the truth's frame. The truth is
 * brought into the map frame first, pose (normalize_angle(θ − θ0), R(θ0)ᵀ((x, y) − (x0, y0))) and
 * landmarks likewise; NULL: no transform at all.
 * EKF_E_ARG, and nothing is touched: a NULL handle, truth_pose or out; n_map outside [0, N];
 * truth_lm NULL with n_map > 0. */
int ekf_eval(ekf_t h, const double* truth_pose, const double* truth_lm, int n_map,
             const double* frame, ekf_eval_rec* out);

/* ---- scoring with unknown association: the truth in any order ---- */
/* After an unknown-association run, slot j holds whatever landmark the filter opened j-th, so there
 * is no slot order to permute the truth into. ekf_eval_match finds it on the device, in the launch
 * that scores, and reports the quality of the association itself. Per filter:
 *   truth_lm[F][n_map][2], 1 <= n_map <= EKF_MATCH_MAX_MAP whatever N is, in any order; a NaN
 *     coordinate means "no such landmark". The truth is brought into the map frame once, exactly as
 *     ekf_eval does it.
 *   k(j), for every seen slot j: the truth landmark with the smallest dx*dx + dy*dy (each product
 *     rounded on its own), ties to the lowest k (a strict < scan in ascending k). A NaN truth never
 *     wins, nor does one at an infinite distance.
 *   Slot j is matched iff that minimum is <= max_dist*max_dist. match[f][j] = k(j) then, and -1 for
 *     an unseen or unmatched slot.
 *   Truth k is claimed by the lowest-index slot matched to it: slots open in ascending order, so
 *     that slot is the landmark's original (its primary) and the others are its duplicates.
 *   out[f] is the record ekf_eval gives for the same truth_pose and frame with
 *     truth_perm[j] = truth_lm[match[j]] (NaN where match[j] < 0) and n_map = N, byte for byte: every
 *     matched slot is evaluated, duplicates included, the terms and the order of the sums are the
 *     same.
 * The record holds integers and a maximum: the same state and truth give the same bytes.
 * EKF_E_ARG, and nothing is touched: a NULL handle, truth_pose, truth_lm or out; n_map outside
 * [1, EKF_MATCH_MAX_MAP]; max_dist negative or NaN (+infinity is valid). match_out[F] and
 * match[F][N] are nullable. Synchronises and leaves the filter alone, exactly as ekf_eval does. */
#define EKF_MATCH_MAX_MAP 1024
typedef struct {
  int n_truth;      /* truth landmarks with both coordinates not NaN */
  int n_matched;    /* seen slots with a truth landmark within max_dist */
  int n_primary;    /* distinct truth landmarks matched (= matched slots that are the lowest-index
                       slot of their landmark) */
  int n_dup;        /* n_matched - n_primary */
  int n_spurious;   /* n_seen - n_matched */
  int n_missed;     /* n_truth - n_primary */
  double max_match_dist; /* largest slot-to-matched-truth distance, 0 if none */
} ekf_match_rec;    /* 32 bytes */

int ekf_eval_match(ekf_t h, const double* truth_pose, const double* truth_lm, int n_map,
                   const double* frame, double max_dist, ekf_eval_rec* out,
                   ekf_match_rec* match_out, int* match);

/* A swarm's records in a few numbers. Pure host code: no handle, no GPU. A ratio whose denominator
 * is zero is NaN. */
typedef struct {
  int n;               /* records */
  int n_pose_nees;     /* finite pose_nees among them */
  double anees_pose;   /* their mean (3 for a consistent filter) */
  double pose_in_95;   /* share of them <= 7.814727903251179, χ²₃ at 0.95 */
  double pos_rmse;     /* √mean(ex² + ey²) */
  double heading_rmse; /* √mean(eθ²) */
  double lm_rmse;      /* √(Σ lm_sq_err / Σ n_eval) */
  double anees_lm;     /* Σ lm_nees / Σ n_nees (2 for a consistent filter) */
} ekf_eval_sum;

/* EKF_E_ARG: recs or out NULL, nf < 1. */
int ekf_eval_summary(const ekf_eval_rec* recs, int nf, ekf_eval_sum* out);

/* ---- helpers ---- */
/* turtlelib::normalize_angle (geometry2d.cpp:5-14): maps into (-π, π], -π → π. */
double ekf_normalize_angle(double rad);

/* ---- measurement ---- */
/* Per-kernel device time (0 = Σ pass, 1 = chain, 2 = association, 3 = factors, 4 = resident filter
 * kernel, 5 = the scoring kernel of ekf_eval, 6 = that of ekf_eval_match) from HIP events
 * carried by each timed dispatch (hipExtLaunchKernelGGL start/stop events: the kernel's own
 * execution, on the stream it runs on). Off by default. */
int ekf_profile_enable(ekf_t h, int enable);
int ekf_profile_read(ekf_t h, int kernel, long long* launches, double* total_ms);
/* Bytes the Σ pass must move per launch for the current handle: fp32 2·n²·w·F (Σ_in read, Σ_out
 * written); fp64 (n(n+1)/2 + n²)·w·F (the symmetric pass reads Σ_in's upper triangle). */
double ekf_sigma_pass_bytes(ekf_t h, int filters_in_launch);
/* Corrections the chain kernel (pipeline handles, known ids and the one-marker association route)
 * has run for `filter` since its creation or last ekf_reset, by the program of its sequential
 * wave that ran them: `lean` holds the common case alone (a mapped landmark, a valid id, a
 * nonsingular S, angles near (-π, π]) and hands a chunk over at the first marker that is anything
 * else; `generic` holds every case. Their sum is the corrections the kernel was given, skipped
 * ones included. The lean program is on by default; EKF_CHAIN_FAST=0 (read at ekf_create) runs
 * every correction in the generic program. Bit-identical either way. Synchronises. EKF_E_ARG:
 * NULL arguments or a filter out of range. */
int ekf_chain_path_counts(ekf_t h, int filter, unsigned long long* lean,
                          unsigned long long* generic);

/* ---- diagnostics ---- */
/* Fill every CU's LDS on `device` with a NaN bit pattern (default stream, synchronising): LDS then
 * holds what an arbitrary earlier kernel could have left, so a kernel that reads LDS it never
 * wrote produces a non-finite result deterministically instead of rarely (used by tests/). */
int ekf_debug_poison_lds(int device);

#ifdef __cplusplus
}
#endif
#endif
