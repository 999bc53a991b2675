// Host runtime behind include/landmarks.h: device buffers, the handle's stream and the batched
// laserCallback (nuslam/src/landmarks.cpp:109-156) over lm_kernels.hip, and the simulated laser
// (nusim/src/nusim.cpp:559-710) over lidar_kernels.hip whose scans it can detect on in place.
// lm_detect_device leaves the markers on the device, and lm_replay_into hands them to a filter
// handle's device planner (k_plan_assoc) without a host hop; lm_replay_resident to a resident
// handle's replay kernel, which reads them in place.
#include <hip/hip_runtime.h>

#include <new>

#include "ekf.h"
#include "ekf_internal.hpp"
#include "landmarks.h"
#include "lm_launch.hpp"

struct lm_ctx {
  int max_scans = 0, max_beams = 0, device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float* d_ranges = nullptr;
  double* d_amin = nullptr;
  double* d_ainc = nullptr;
  int* d_counts = nullptr;
  lm_marker* d_markers = nullptr;
  int marker_cap = 0;  // markers per scan the device buffer holds
  lmk::DetectWork work{};
  // lm_fit_circles / lm_check_circles staging (grown on demand)
  int* d_offs = nullptr;
  double* d_xy = nullptr;
  double* d_out = nullptr;
  size_t cap_c = 0, cap_p = 0;
  bool timed = false;
  // lm_simulate: inputs on the device (the scenes grown on demand), the upload's event, the
  // kernel's timing events, and the scans resident in d_ranges
  double* d_poses = nullptr;
  int* d_scene = nullptr;
  double* d_circles = nullptr;
  size_t cap_circles = 0;  // doubles d_circles holds
  hipEvent_t e_up = nullptr, s0 = nullptr, s1 = nullptr;
  bool sim_timed = false;
  int res_scans = 0, res_beams = 0;  // 0: nothing resident
  // lm_detect_device / lm_replay_into: the detect whose results stay in d_markers / d_counts
  // (dev_scans scans of dev_cap markers; 0: none), the event behind it that a filter's planning
  // stream waits for, and the event behind that planner which frees the marker buffer again
  int dev_scans = 0, dev_cap = 0;
  hipEvent_t e_det = nullptr, e_planned = nullptr;
  bool planner_reads = false;  // e_planned is recorded and this stream has not waited for it yet
};

namespace {

int grow(void** p, size_t bytes) {
  if (*p) hipFree(*p);
  *p = nullptr;
  return hipMalloc(p, bytes) == hipSuccess ? EKF_OK : EKF_E_NOMEM;
}

// fitCircle / checkCircle inputs → device (offsets validated on the host)
int stage_clusters(lm_t h, int nc, const int* offs, const double* xy) {
  if (!h || nc <= 0 || !offs || !xy || offs[0] != 0) return EKF_E_ARG;
  for (int c = 0; c < nc; ++c)
    if (offs[c + 1] <= offs[c]) return EKF_E_ARG;
  const size_t np = static_cast<size_t>(offs[nc]);
  if (static_cast<size_t>(nc) > h->cap_c) {
    if (grow(reinterpret_cast<void**>(&h->d_offs), sizeof(int) * (nc + 1)) ||
        grow(reinterpret_cast<void**>(&h->d_out), sizeof(double) * 3 * nc))
      return EKF_E_NOMEM;
    h->cap_c = nc;
  }
  if (np > h->cap_p) {
    if (grow(reinterpret_cast<void**>(&h->d_xy), sizeof(double) * 2 * np)) return EKF_E_NOMEM;
    h->cap_p = np;
  }
  if (hipSetDevice(h->device) != hipSuccess ||
      hipMemcpyAsync(h->d_offs, offs, sizeof(int) * (nc + 1), hipMemcpyHostToDevice, h->stream) !=
          hipSuccess ||
      hipMemcpyAsync(h->d_xy, xy, sizeof(double) * 2 * np, hipMemcpyHostToDevice, h->stream) !=
          hipSuccess)
    return EKF_E_HIP;
  return EKF_OK;
}

// Landmarks::laserCallback over the S × B ranges (and angles) already in the handle's buffers,
// enqueued: markers [S][cap] and counts [S] stay on the device.
int enqueue_detect(lm_t h, int S, int B, double thr, int max_markers) {
  const int cap = max_markers > 0 ? max_markers : 1;
  h->dev_scans = 0;
  if (h->planner_reads) {  // a filter's planner (lm_replay_into) may still read markers and counts
    if (cap > h->marker_cap && hipEventSynchronize(h->e_planned) != hipSuccess) return EKF_E_HIP;
    if (hipStreamWaitEvent(h->stream, h->e_planned, 0) != hipSuccess) return EKF_E_HIP;
    h->planner_reads = false;
  }
  if (cap > h->marker_cap) {
    if (grow(reinterpret_cast<void**>(&h->d_markers),
             sizeof(lm_marker) * static_cast<size_t>(h->max_scans) * cap))
      return EKF_E_NOMEM;
    h->marker_cap = cap;
  }
  if (hipEventRecord(h->e0, h->stream) != hipSuccess) return EKF_E_HIP;
  if (lmk::launch_detect(h->d_ranges, S, B, h->d_amin, h->d_ainc, thr, h->d_markers, cap,
                         h->d_counts, h->work, h->stream) != hipSuccess)
    return EKF_E_HIP;
  if (hipEventRecord(h->e1, h->stream) != hipSuccess) return EKF_E_HIP;
  h->timed = true;
  return EKF_OK;
}

// ... and its results to the host (synchronising).
int run_detect(lm_t h, int S, int B, double thr, lm_marker* markers, int max_markers,
               int* counts) {
  if (int rc = enqueue_detect(h, S, B, thr, max_markers)) return rc;
  const int cap = max_markers > 0 ? max_markers : 1;
  if (hipMemcpyAsync(counts, h->d_counts, sizeof(int) * S, hipMemcpyDeviceToHost, h->stream) !=
      hipSuccess)
    return EKF_E_HIP;
  if (max_markers > 0 &&
      hipMemcpyAsync(markers, h->d_markers, sizeof(lm_marker) * static_cast<size_t>(S) * cap,
                     hipMemcpyDeviceToHost, h->stream) != hipSuccess)
    return EKF_E_HIP;
  return hipStreamSynchronize(h->stream) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

// A host caller's scans into the handle's buffers (enqueued).
int upload_scans(lm_t h, int S, int B, const float* ranges, const double* amin,
                 const double* ainc) {
  h->res_scans = h->res_beams = 0;  // the upload overwrites lm_simulate's scans
  const size_t nr = static_cast<size_t>(S) * B;
  if (hipMemcpyAsync(h->d_ranges, ranges, sizeof(float) * nr, hipMemcpyHostToDevice, h->stream) !=
          hipSuccess ||
      hipMemcpyAsync(h->d_amin, amin, sizeof(double) * S, hipMemcpyHostToDevice, h->stream) !=
          hipSuccess ||
      hipMemcpyAsync(h->d_ainc, ainc, sizeof(double) * S, hipMemcpyHostToDevice, h->stream) !=
          hipSuccess)
    return EKF_E_HIP;
  return EKF_OK;
}

}  // namespace

extern "C" {

int lm_create(lm_t* out, int max_scans, int max_beams, int device) {
  if (!out || max_scans <= 0 || max_beams < 2 || max_beams > LM_MAX_BEAMS) return EKF_E_ARG;
  *out = nullptr;
  lm_ctx* h = new (std::nothrow) lm_ctx;
  if (!h) return EKF_E_NOMEM;
  h->max_scans = max_scans;
  h->max_beams = max_beams;
  h->device = device;
  const size_t S = max_scans;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&h->stream) != hipSuccess ||
      hipEventCreate(&h->e0) != hipSuccess || hipEventCreate(&h->e1) != hipSuccess ||
      hipEventCreate(&h->e_up) != hipSuccess || hipEventCreate(&h->s0) != hipSuccess ||
      hipEventCreate(&h->s1) != hipSuccess ||
      hipEventCreateWithFlags(&h->e_det, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->e_planned, hipEventDisableTiming) != hipSuccess) {
    lm_destroy(h);
    return EKF_E_HIP;
  }
  if (hipMalloc(&h->d_ranges, sizeof(float) * S * max_beams) != hipSuccess ||
      hipMalloc(&h->d_amin, sizeof(double) * S) != hipSuccess ||
      hipMalloc(&h->d_ainc, sizeof(double) * S) != hipSuccess ||
      hipMalloc(&h->d_counts, sizeof(int) * S) != hipSuccess ||
      hipMalloc(&h->d_poses, sizeof(double) * 3 * S) != hipSuccess ||
      hipMalloc(&h->d_scene, sizeof(int) * S) != hipSuccess ||
      hipMalloc(&h->work.px, sizeof(double) * S * max_beams) != hipSuccess ||
      hipMalloc(&h->work.py, sizeof(double) * S * max_beams) != hipSuccess ||
      hipMalloc(&h->work.cand, sizeof(lmk::Cand) * lmk::candidate_capacity(max_scans, max_beams)) !=
          hipSuccess ||
      hipMalloc(&h->work.gcount, sizeof(int) * lmk::kRegions) != hipSuccess ||
      hipMalloc(&h->work.sbase, sizeof(int) * S) != hipSuccess ||
      hipMalloc(&h->work.sncand, sizeof(int) * S) != hipSuccess) {
    lm_destroy(h);
    return EKF_E_NOMEM;
  }
  *out = h;
  return EKF_OK;
}

int lm_destroy(lm_t h) {
  if (!h) return EKF_E_ARG;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->planner_reads) hipEventSynchronize(h->e_planned);  // a filter's planner reads d_markers
  for (void* p : {static_cast<void*>(h->d_ranges), static_cast<void*>(h->d_amin),
                  static_cast<void*>(h->d_ainc), static_cast<void*>(h->d_counts),
                  static_cast<void*>(h->d_markers), static_cast<void*>(h->d_offs),
                  static_cast<void*>(h->d_xy), static_cast<void*>(h->d_out),
                  static_cast<void*>(h->work.px), static_cast<void*>(h->work.py),
                  static_cast<void*>(h->work.cand), static_cast<void*>(h->work.gcount),
                  static_cast<void*>(h->work.sbase), static_cast<void*>(h->work.sncand),
                  static_cast<void*>(h->d_poses), static_cast<void*>(h->d_scene),
                  static_cast<void*>(h->d_circles)})
    if (p) hipFree(p);
  for (hipEvent_t e : {h->e0, h->e1, h->e_up, h->s0, h->s1, h->e_det, h->e_planned})
    if (e) hipEventDestroy(e);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return EKF_OK;
}

int lm_detect(lm_t h, int S, int B, const float* ranges, const double* amin, const double* ainc,
              double thr, lm_marker* markers, int max_markers, int* counts) {
  if (!h || S <= 0 || S > h->max_scans || B < 2 || B > h->max_beams || !ranges || !amin ||
      !ainc || !counts || max_markers < 0 || (max_markers > 0 && !markers))
    return EKF_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return EKF_E_HIP;
  if (int rc = upload_scans(h, S, B, ranges, amin, ainc)) return rc;
  return run_detect(h, S, B, thr, markers, max_markers, counts);
}

void lm_scan_config_default(lm_scan_config* c) {
  if (!c) return;
  c->seed = 20240317ull;
  c->scan0 = 0;
  c->arena_w = 10.0;
  c->arena_h = 5.0;
  c->range_min = 0.11;
  c->range_max = 10.0;
  c->sigma = 0.0;
}

int lm_simulate(lm_t h, int S, int B, const double* poses, int G, int C, const double* circles,
                const int* scene, const lm_scan_config* cfg, float* ranges_out) {
  if (!h || S <= 0 || S > h->max_scans || B < 2 || B > h->max_beams || !poses || G < 1 || C < 0 ||
      C > LM_MAX_CIRCLES || (C > 0 && !circles) || !cfg || !(cfg->sigma >= 0.0) ||
      !(cfg->range_min <= cfg->range_max) || cfg->scan0 < 0)
    return EKF_E_ARG;
  for (int s = 0; scene && s < S; ++s)
    if (scene[s] < 0 || scene[s] >= G) return EKF_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return EKF_E_HIP;
  h->res_scans = h->res_beams = 0;
  const size_t nc = static_cast<size_t>(G) * C * 3;
  if (nc > h->cap_circles) {
    h->cap_circles = 0;
    if (grow(reinterpret_cast<void**>(&h->d_circles), sizeof(double) * nc)) return EKF_E_NOMEM;
    h->cap_circles = nc;
  }
  if (hipMemcpyAsync(h->d_poses, poses, sizeof(double) * 3 * S, hipMemcpyHostToDevice,
                     h->stream) != hipSuccess ||
      (nc && hipMemcpyAsync(h->d_circles, circles, sizeof(double) * nc, hipMemcpyHostToDevice,
                            h->stream) != hipSuccess) ||
      (scene && hipMemcpyAsync(h->d_scene, scene, sizeof(int) * S, hipMemcpyHostToDevice,
                               h->stream) != hipSuccess) ||
      hipEventRecord(h->e_up, h->stream) != hipSuccess)
    return EKF_E_HIP;
  lmk::ScanArgs a{};
  a.poses = h->d_poses;
  a.circles = h->d_circles;
  a.scene = scene ? h->d_scene : nullptr;
  a.ranges = h->d_ranges;
  a.angle_min = h->d_amin;
  a.angle_inc = h->d_ainc;
  a.n_scans = S;
  a.n_beams = B;
  a.n_circles = C;
  a.seed = cfg->seed;
  a.scan0 = cfg->scan0;
  a.arena_w = cfg->arena_w;
  a.arena_h = cfg->arena_h;
  a.range_min = cfg->range_min;
  a.range_max = cfg->range_max;
  a.sigma = cfg->sigma;
  if (hipEventRecord(h->s0, h->stream) != hipSuccess ||
      lmk::launch_scan(a, h->stream) != hipSuccess ||
      hipEventRecord(h->s1, h->stream) != hipSuccess)
    return EKF_E_HIP;
  h->sim_timed = true;
  if (ranges_out) {
    if (hipMemcpyAsync(ranges_out, h->d_ranges, sizeof(float) * static_cast<size_t>(S) * B,
                       hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
      return EKF_E_HIP;
  } else if (hipEventSynchronize(h->e_up) != hipSuccess) {  // the caller's inputs are consumed
    return EKF_E_HIP;
  }
  h->res_scans = S;
  h->res_beams = B;
  return EKF_OK;
}

int lm_detect_resident(lm_t h, double thr, lm_marker* markers, int max_markers, int* counts) {
  if (!h || h->res_scans <= 0 || !counts || max_markers < 0 || (max_markers > 0 && !markers))
    return EKF_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return EKF_E_HIP;
  return run_detect(h, h->res_scans, h->res_beams, thr, markers, max_markers, counts);
}

int lm_detect_device(lm_t h, int S, int B, const float* ranges, const double* amin,
                     const double* ainc, double thr, int max_markers) {
  if (!h || max_markers < 1) return EKF_E_ARG;
  if (ranges) {
    if (S <= 0 || S > h->max_scans || B < 2 || B > h->max_beams || !amin || !ainc) return EKF_E_ARG;
  } else if (h->res_scans <= 0) {
    return EKF_E_ARG;
  }
  if (hipSetDevice(h->device) != hipSuccess) return EKF_E_HIP;
  if (ranges) {
    if (int rc = upload_scans(h, S, B, ranges, amin, ainc)) return rc;
    if (hipEventRecord(h->e_up, h->stream) != hipSuccess) return EKF_E_HIP;
  } else {
    S = h->res_scans;
    B = h->res_beams;
  }
  if (int rc = enqueue_detect(h, S, B, thr, max_markers)) return rc;
  if (hipEventRecord(h->e_det, h->stream) != hipSuccess) return EKF_E_HIP;
  // the caller's scans are consumed (they may be freed); the detect itself is still in flight
  if (ranges && hipEventSynchronize(h->e_up) != hipSuccess) return EKF_E_HIP;
  h->dev_scans = S;
  h->dev_cap = max_markers;
  return EKF_OK;
}

int lm_fetch_markers(lm_t h, lm_marker* markers, int max_markers, int* counts) {
  if (!h || h->dev_scans <= 0 || max_markers < 0 || (max_markers > 0 && !markers) ||
      (max_markers == 0 && !counts))
    return EKF_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return EKF_E_HIP;
  const int S = h->dev_scans, w = max_markers < h->dev_cap ? max_markers : h->dev_cap;
  if (counts && hipMemcpyAsync(counts, h->d_counts, sizeof(int) * S, hipMemcpyDeviceToHost,
                               h->stream) != hipSuccess)
    return EKF_E_HIP;
  if (w > 0 && hipMemcpy2DAsync(markers, sizeof(lm_marker) * max_markers, h->d_markers,
                                sizeof(lm_marker) * h->dev_cap, sizeof(lm_marker) * w, S,
                                hipMemcpyDeviceToHost, h->stream) != hipSuccess)
    return EKF_E_HIP;
  return hipStreamSynchronize(h->stream) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

static_assert(sizeof(lm_marker) == 4 * sizeof(double), "k_plan_assoc reads lm_marker at stride 4");

int lm_replay_into(lm_t h, ekf_t e, int T, const double* odom) {
  if (!h || !e || T < 1 || !odom || h->dev_scans <= 0) return EKF_E_ARG;
  int F = 0;
  if (ekf_dims(e, nullptr, nullptr, &F) != EKF_OK || F < 1 ||
      static_cast<long long>(T) * F != h->dev_scans || h->dev_cap > 64)
    return EKF_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return EKF_E_HIP;
  const int rc = ekfslam::replay_markers(e, h->device, T, h->dev_cap, h->d_counts,
                                         reinterpret_cast<const double*>(h->d_markers), odom,
                                         h->e_det, h->e_planned);
  // (an argument error comes back before anything is enqueued; past that the planner may be)
  if (rc != EKF_E_ARG) h->planner_reads = true;
  return rc;
}

int lm_replay_resident(lm_t h, ekf_t e, int T, const double* odom) {
  if (!h || !e || T < 1 || !odom || h->dev_scans <= 0) return EKF_E_ARG;
  int F = 0;
  if (ekf_dims(e, nullptr, nullptr, &F) != EKF_OK || F < 1 ||
      static_cast<long long>(T) * F != h->dev_scans || h->dev_cap > 64)
    return EKF_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return EKF_E_HIP;
  // the filter's kernel reads the markers in place throughout: e_planned sits behind it
  const int rc = ekfslam::replay_markers_resident(e, h->device, T, h->dev_cap, h->d_counts,
                                                  reinterpret_cast<const double*>(h->d_markers),
                                                  odom, h->e_det, h->e_planned);
  if (rc != EKF_E_ARG) h->planner_reads = true;
  return rc;
}

int lm_last_simulate_us(lm_t h, double* us) {
  if (!h || !us || !h->sim_timed) return EKF_E_ARG;
  float ms = 0.0f;
  if (hipEventSynchronize(h->s1) != hipSuccess ||  // lm_simulate may have left the kernel in flight
      hipEventElapsedTime(&ms, h->s0, h->s1) != hipSuccess)
    return EKF_E_HIP;
  *us = 1e3 * ms;
  return EKF_OK;
}

int lm_fit_circles(lm_t h, int nc, const int* offs, const double* xy, double* out) {
  if (!out) return EKF_E_ARG;
  if (int rc = stage_clusters(h, nc, offs, xy)) return rc;
  if (lmk::launch_fit(nc, h->d_offs, h->d_xy, h->d_out, h->stream) != hipSuccess ||
      hipMemcpyAsync(out, h->d_out, sizeof(double) * 3 * nc, hipMemcpyDeviceToHost, h->stream) !=
          hipSuccess)
    return EKF_E_HIP;
  return hipStreamSynchronize(h->stream) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

int lm_check_circles(lm_t h, int nc, const int* offs, const double* xy, int* out) {
  if (!out) return EKF_E_ARG;
  for (int c = 0; offs && c < nc; ++c)
    if (offs[c + 1] - offs[c] < 3) return EKF_E_ARG;  // the reference's angle vector needs n − 2 ≥ 1
  if (int rc = stage_clusters(h, nc, offs, xy)) return rc;
  int* dout = reinterpret_cast<int*>(h->d_out);  // 3·nc doubles ≥ nc ints
  if (lmk::launch_check(nc, h->d_offs, h->d_xy, dout, h->stream) != hipSuccess ||
      hipMemcpyAsync(out, dout, sizeof(int) * nc, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
    return EKF_E_HIP;
  return hipStreamSynchronize(h->stream) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

int lm_last_kernel_us(lm_t h, double* us) {
  if (!h || !us || !h->timed) return EKF_E_ARG;
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, h->e0, h->e1) != hipSuccess) return EKF_E_HIP;
  *us = 1e3 * ms;
  return EKF_OK;
}

}  // extern "C"
