// Host runtime behind include/landmarks.h: device buffers, the handle's stream and the batched
// laserCallback (nuslam/src/landmarks.cpp:109-156) over lm_kernels.hip, and the simulated laser
// (nusim/src/nusim.cpp:559-710) over lidar_kernels.hip whose scans it can detect on in place.
// lm_detect_device leaves the markers on the device, and lm_replay_into hands them to a filter
// handle's device planner (k_plan_assoc) without a host hop; lm_replay_resident to a resident
// handle's replay kernel, which reads them in place. The simulator (sim_api.cpp) drives the same
// chain from its own device buffers through lm_lidar_enqueue: laser, detect, markers left in place.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <new>

#include "ekf.h"
#include "ekf_internal.hpp"
#include "hip_owned.hpp"
#include "landmarks.h"
#include "lm_launch.hpp"

struct lm_ctx {
  int max_scans = 0, max_beams = 0, device = 0;
  // (members are destroyed in reverse order: the stream outlives what is used on it)
  ekfslam::Stream stream;
  ekfslam::Event e0, e1;
  ekfslam::DeviceBuf<float> d_ranges;
  ekfslam::DeviceBuf<double> d_amin, d_ainc;
  ekfslam::DeviceBuf<int> d_counts;
  ekfslam::DeviceBuf<lm_marker> d_markers;  // [max_scans][markers per scan], grown on demand
  lmk::DetectWork work{};                   // its pointers into these:
  ekfslam::DeviceBuf<double> w_px, w_py;
  ekfslam::DeviceBuf<lmk::Cand> w_cand;
  ekfslam::DeviceBuf<int> w_gcount, w_sbase, w_sncand;
  // lm_fit_circles / lm_check_circles staging (grown on demand)
  ekfslam::DeviceBuf<int> d_offs;
  ekfslam::DeviceBuf<double> d_xy, d_out;
  bool timed = false;
  // lm_simulate: inputs on the device (the scenes grown on demand), the upload's event, the
  // kernel's timing events, and the scans resident in d_ranges
  ekfslam::DeviceBuf<double> d_poses, d_circles;
  ekfslam::DeviceBuf<int> d_scene;
  ekfslam::Event e_up, s0, s1;
  bool sim_timed = false;
  int res_scans = 0, res_beams = 0;  // 0: nothing resident
  // lm_detect_device / lm_replay_into: the detect whose results stay in d_markers / d_counts
  // (dev_scans scans of dev_cap markers; 0: none), the event behind it that a filter's planning
  // stream waits for, and the event behind that planner which frees the marker buffer again
  int dev_scans = 0, dev_cap = 0;
  ekfslam::Event e_det{hipEventDisableTiming}, e_planned{hipEventDisableTiming};
  bool planner_reads = false;  // e_planned is recorded and this stream has not waited for it yet
};

namespace {

// fitCircle / checkCircle inputs → device (offsets validated on the host)
int stage_clusters(lm_t h, int nc, const int* offs, const double* xy) {
  if (!h || nc <= 0 || !offs || !xy || offs[0] != 0) return EKF_E_ARG;
  for (int c = 0; c < nc; ++c)
    if (offs[c + 1] <= offs[c]) return EKF_E_ARG;
  const size_t np = static_cast<size_t>(offs[nc]);
  const size_t c = static_cast<size_t>(nc);
  if (h->d_offs.reserve(c + 1) || h->d_out.reserve(3 * c) || h->d_xy.reserve(2 * np))
    return EKF_E_NOMEM;
  if (hipSetDevice(h->device) != hipSuccess ||
      hipMemcpyAsync(h->d_offs.get(), offs, sizeof(int) * (nc + 1), hipMemcpyHostToDevice,
                     h->stream.get()) != hipSuccess ||
      hipMemcpyAsync(h->d_xy.get(), xy, sizeof(double) * 2 * np, hipMemcpyHostToDevice,
                     h->stream.get()) != hipSuccess)
    return EKF_E_HIP;
  return EKF_OK;
}

// Landmarks::laserCallback over the S × B ranges (and angles) already in the handle's buffers,
// enqueued: markers [S][cap] and counts [S] stay on the device.
int enqueue_detect(lm_t h, int S, int B, double thr, int max_markers) {
  const int cap = max_markers > 0 ? max_markers : 1;
  h->dev_scans = 0;
  const size_t need = static_cast<size_t>(h->max_scans) * cap;
  if (h->planner_reads) {  // a filter's planner (lm_replay_into) may still read markers and counts
    if (need > h->d_markers.capacity() && hipEventSynchronize(h->e_planned.get()) != hipSuccess)
      return EKF_E_HIP;
    if (hipStreamWaitEvent(h->stream.get(), h->e_planned.get(), 0) != hipSuccess) return EKF_E_HIP;
    h->planner_reads = false;
  }
  if (int rc = h->d_markers.reserve(need)) return rc;
  if (hipEventRecord(h->e0.get(), h->stream.get()) != hipSuccess) return EKF_E_HIP;
  if (lmk::launch_detect(h->d_ranges.get(), S, B, h->d_amin.get(), h->d_ainc.get(), thr,
                         h->d_markers.get(), cap, h->d_counts.get(), h->work,
                         h->stream.get()) != hipSuccess)
    return EKF_E_HIP;
  if (hipEventRecord(h->e1.get(), h->stream.get()) != hipSuccess) return EKF_E_HIP;
  h->timed = true;
  return EKF_OK;
}

// ... and its results to the host (synchronising).
int run_detect(lm_t h, int S, int B, double thr, lm_marker* markers, int max_markers,
               int* counts) {
  if (int rc = enqueue_detect(h, S, B, thr, max_markers)) return rc;
  const int cap = max_markers > 0 ? max_markers : 1;
  if (hipMemcpyAsync(counts, h->d_counts.get(), sizeof(int) * S, hipMemcpyDeviceToHost,
                     h->stream.get()) != hipSuccess)
    return EKF_E_HIP;
  if (max_markers > 0 &&
      hipMemcpyAsync(markers, h->d_markers.get(), sizeof(lm_marker) * static_cast<size_t>(S) * cap,
                     hipMemcpyDeviceToHost, h->stream.get()) != hipSuccess)
    return EKF_E_HIP;
  return hipStreamSynchronize(h->stream.get()) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

// A host caller's scans into the handle's buffers (enqueued).
int upload_scans(lm_t h, int S, int B, const float* ranges, const double* amin,
                 const double* ainc) {
  h->res_scans = h->res_beams = 0;  // the upload overwrites lm_simulate's scans
  const size_t nr = static_cast<size_t>(S) * B;
  const hipStream_t st = h->stream.get();
  if (hipMemcpyAsync(h->d_ranges.get(), ranges, sizeof(float) * nr, hipMemcpyHostToDevice, st) !=
          hipSuccess ||
      hipMemcpyAsync(h->d_amin.get(), amin, sizeof(double) * S, hipMemcpyHostToDevice, st) !=
          hipSuccess ||
      hipMemcpyAsync(h->d_ainc.get(), ainc, sizeof(double) * S, hipMemcpyHostToDevice, st) !=
          hipSuccess)
    return EKF_E_HIP;
  return EKF_OK;
}

// lm_simulate's rules for a scan configuration (scan0 aside)
bool scan_config_ok(const lm_scan_config* cfg) {
  return cfg && cfg->sigma >= 0.0 && cfg->range_min <= cfg->range_max;
}

}  // namespace

// ---- ekf_sim_run_lidar's hook (ekf_internal.hpp) -------------------------------------------------
namespace ekfslam {

int lm_lidar_check(lm_t h, int device, int n_scans, int n_beams, int max_markers,
                   const lm_scan_config* cfg) {
  if (!h || device != h->device || n_scans < 1 || n_scans > h->max_scans || n_beams < 2 ||
      n_beams > h->max_beams || max_markers < 1 || max_markers > 64 || !scan_config_ok(cfg))
    return EKF_E_ARG;
  return EKF_OK;
}

int lm_lidar_enqueue(lm_t h, const LidarRun& run, hipEvent_t after, LidarFeed* out) {
  const int S = run.T * run.F;
  const hipStream_t st = h->stream.get();
  if (hipSetDevice(h->device) != hipSuccess) return EKF_E_HIP;
  h->res_scans = h->res_beams = 0;
  lmk::SwarmScanArgs a{};
  a.poses = run.d_truth;
  a.lm = run.d_lm;
  a.ranges = h->d_ranges.get();
  a.angle_min = h->d_amin.get();
  a.angle_inc = h->d_ainc.get();
  a.n_scans = S;
  a.n_beams = run.n_beams;
  a.n_filters = run.F;
  a.n_map = run.L;
  a.seed = run.seed;
  a.msg0 = run.msg0;
  a.radius = run.radius;
  a.arena_w = run.scan->arena_w;
  a.arena_h = run.scan->arena_h;
  a.range_min = run.scan->range_min;
  a.range_max = run.scan->range_max;
  a.sigma = run.scan->sigma;
  const char* from = std::getenv("EKF_LIDAR_CULL_FROM");  // (measurements only: same bits)
  a.cull_from = from ? std::atoi(from) : lmk::kCullFromMap;
  if (hipStreamWaitEvent(st, after, 0) != hipSuccess ||
      hipEventRecord(h->s0.get(), st) != hipSuccess ||
      lmk::launch_scan_swarm(a, st) != hipSuccess || hipEventRecord(h->s1.get(), st) != hipSuccess)
    return EKF_E_HIP;
  h->sim_timed = true;
  h->res_scans = S;
  h->res_beams = run.n_beams;
  if (int rc = enqueue_detect(h, S, run.n_beams, run.threshold, run.max_markers)) return rc;
  if (hipEventRecord(h->e_det.get(), st) != hipSuccess) return EKF_E_HIP;
  h->dev_scans = S;
  h->dev_cap = run.max_markers;
  *out = LidarFeed{h->d_counts.get(), reinterpret_cast<const double*>(h->d_markers.get()),
                   h->e_det.get(), h->e_planned.get()};
  return EKF_OK;
}

void lm_lidar_planned(lm_t h) { h->planner_reads = true; }

}  // namespace ekfslam

extern "C" {

int lm_create(lm_t* out, int max_scans, int max_beams, int device) {
  if (!out || max_scans <= 0 || max_beams < 2 || max_beams > LM_MAX_BEAMS) return EKF_E_ARG;
  *out = nullptr;
  lm_ctx* h = new (std::nothrow) lm_ctx;
  if (!h) return EKF_E_NOMEM;
  h->max_scans = max_scans;
  h->max_beams = max_beams;
  h->device = device;
  const size_t S = max_scans, SB = S * max_beams;
  if (hipSetDevice(device) != hipSuccess || h->stream.create() || h->e0.create() ||
      h->e1.create() || h->e_up.create() || h->s0.create() || h->s1.create() ||
      h->e_det.create() || h->e_planned.create()) {
    lm_destroy(h);
    return EKF_E_HIP;
  }
  if (h->d_ranges.reserve(SB) || h->d_amin.reserve(S) || h->d_ainc.reserve(S) ||
      h->d_counts.reserve(S) || h->d_poses.reserve(3 * S) || h->d_scene.reserve(S) ||
      h->w_px.reserve(SB) || h->w_py.reserve(SB) ||
      h->w_cand.reserve(lmk::candidate_capacity(max_scans, max_beams)) ||
      h->w_gcount.reserve(lmk::kRegions) || h->w_sbase.reserve(S) || h->w_sncand.reserve(S)) {
    lm_destroy(h);
    return EKF_E_NOMEM;
  }
  h->work = lmk::DetectWork{h->w_px.get(),     h->w_py.get(),    h->w_cand.get(),
                            h->w_gcount.get(), h->w_sbase.get(), h->w_sncand.get()};
  *out = h;
  return EKF_OK;
}

int lm_destroy(lm_t h) {
  if (!h) return EKF_E_ARG;
  hipSetDevice(h->device);
  if (h->stream.get()) hipStreamSynchronize(h->stream.get());
  // a filter's planner reads d_markers
  if (h->planner_reads) hipEventSynchronize(h->e_planned.get());
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
      C > LM_MAX_CIRCLES || (C > 0 && !circles) || !scan_config_ok(cfg) || cfg->scan0 < 0)
    return EKF_E_ARG;
  for (int s = 0; scene && s < S; ++s)
    if (scene[s] < 0 || scene[s] >= G) return EKF_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return EKF_E_HIP;
  h->res_scans = h->res_beams = 0;
  const size_t nc = static_cast<size_t>(G) * C * 3;
  if (int rc = h->d_circles.reserve(nc)) return rc;
  if (hipMemcpyAsync(h->d_poses.get(), poses, sizeof(double) * 3 * S, hipMemcpyHostToDevice,
                     h->stream.get()) != hipSuccess ||
      (nc && hipMemcpyAsync(h->d_circles.get(), circles, sizeof(double) * nc, hipMemcpyHostToDevice,
                            h->stream.get()) != hipSuccess) ||
      (scene && hipMemcpyAsync(h->d_scene.get(), scene, sizeof(int) * S, hipMemcpyHostToDevice,
                               h->stream.get()) != hipSuccess) ||
      hipEventRecord(h->e_up.get(), h->stream.get()) != hipSuccess)
    return EKF_E_HIP;
  lmk::ScanArgs a{};
  a.poses = h->d_poses.get();
  a.circles = h->d_circles.get();
  a.scene = scene ? h->d_scene.get() : nullptr;
  a.ranges = h->d_ranges.get();
  a.angle_min = h->d_amin.get();
  a.angle_inc = h->d_ainc.get();
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
  if (hipEventRecord(h->s0.get(), h->stream.get()) != hipSuccess ||
      lmk::launch_scan(a, h->stream.get()) != hipSuccess ||
      hipEventRecord(h->s1.get(), h->stream.get()) != hipSuccess)
    return EKF_E_HIP;
  h->sim_timed = true;
  if (ranges_out) {
    if (hipMemcpyAsync(ranges_out, h->d_ranges.get(), sizeof(float) * static_cast<size_t>(S) * B,
                       hipMemcpyDeviceToHost, h->stream.get()) != hipSuccess ||
        hipStreamSynchronize(h->stream.get()) != hipSuccess)
      return EKF_E_HIP;
  } else if (hipEventSynchronize(h->e_up.get()) != hipSuccess) {  // the caller's inputs: consumed
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
    if (hipEventRecord(h->e_up.get(), h->stream.get()) != hipSuccess) return EKF_E_HIP;
  } else {
    S = h->res_scans;
    B = h->res_beams;
  }
  if (int rc = enqueue_detect(h, S, B, thr, max_markers)) return rc;
  if (hipEventRecord(h->e_det.get(), h->stream.get()) != hipSuccess) return EKF_E_HIP;
  // the caller's scans are consumed (they may be freed); the detect itself is still in flight
  if (ranges && hipEventSynchronize(h->e_up.get()) != hipSuccess) return EKF_E_HIP;
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
  if (counts && hipMemcpyAsync(counts, h->d_counts.get(), sizeof(int) * S, hipMemcpyDeviceToHost,
                               h->stream.get()) != hipSuccess)
    return EKF_E_HIP;
  if (w > 0 && hipMemcpy2DAsync(markers, sizeof(lm_marker) * max_markers, h->d_markers.get(),
                                sizeof(lm_marker) * h->dev_cap, sizeof(lm_marker) * w, S,
                                hipMemcpyDeviceToHost, h->stream.get()) != hipSuccess)
    return EKF_E_HIP;
  return hipStreamSynchronize(h->stream.get()) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

static_assert(sizeof(lm_marker) == 4 * sizeof(double), "k_plan_assoc reads lm_marker at stride 4");

int lm_replay_into(lm_t h, ekf_t e, int T, const double* odom) {
  if (!h || !e || T < 1 || !odom || h->dev_scans <= 0) return EKF_E_ARG;
  int F = 0;
  if (ekf_dims(e, nullptr, nullptr, &F) != EKF_OK || F < 1 ||
      static_cast<long long>(T) * F != h->dev_scans || h->dev_cap > 64)
    return EKF_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return EKF_E_HIP;
  const int rc = ekfslam::replay_markers(e, h->device, T, h->dev_cap, h->d_counts.get(),
                                         reinterpret_cast<const double*>(h->d_markers.get()), odom,
                                         h->e_det.get(), h->e_planned.get());
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
  const double* markers = reinterpret_cast<const double*>(h->d_markers.get());
  const int rc = ekfslam::replay_markers_resident(e, h->device, T, h->dev_cap, h->d_counts.get(),
                                                  markers, odom, h->e_det.get(),
                                                  h->e_planned.get());
  if (rc != EKF_E_ARG) h->planner_reads = true;
  return rc;
}

int lm_fetch_ranges(lm_t h, float* out) {
  if (!h || !out || h->res_scans <= 0) return EKF_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return EKF_E_HIP;
  const size_t n = static_cast<size_t>(h->res_scans) * h->res_beams;
  if (hipMemcpyAsync(out, h->d_ranges.get(), sizeof(float) * n, hipMemcpyDeviceToHost,
                     h->stream.get()) != hipSuccess)
    return EKF_E_HIP;
  return hipStreamSynchronize(h->stream.get()) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

int lm_last_simulate_us(lm_t h, double* us) {
  if (!h || !us || !h->sim_timed) return EKF_E_ARG;
  float ms = 0.0f;
  // (lm_simulate and ekf_sim_run_lidar may have left the kernel in flight)
  if (hipEventSynchronize(h->s1.get()) != hipSuccess ||
      hipEventElapsedTime(&ms, h->s0.get(), h->s1.get()) != hipSuccess)
    return EKF_E_HIP;
  *us = 1e3 * ms;
  return EKF_OK;
}

int lm_fit_circles(lm_t h, int nc, const int* offs, const double* xy, double* out) {
  if (!out) return EKF_E_ARG;
  if (int rc = stage_clusters(h, nc, offs, xy)) return rc;
  const hipStream_t st = h->stream.get();
  if (lmk::launch_fit(nc, h->d_offs.get(), h->d_xy.get(), h->d_out.get(), st) != hipSuccess ||
      hipMemcpyAsync(out, h->d_out.get(), sizeof(double) * 3 * nc, hipMemcpyDeviceToHost, st) !=
          hipSuccess)
    return EKF_E_HIP;
  return hipStreamSynchronize(h->stream.get()) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

int lm_check_circles(lm_t h, int nc, const int* offs, const double* xy, int* out) {
  if (!out) return EKF_E_ARG;
  for (int c = 0; offs && c < nc; ++c)
    if (offs[c + 1] - offs[c] < 3) return EKF_E_ARG;  // the reference's angle vector: n − 2 ≥ 1
  if (int rc = stage_clusters(h, nc, offs, xy)) return rc;
  int* dout = reinterpret_cast<int*>(h->d_out.get());  // 3·nc doubles ≥ nc ints
  if (lmk::launch_check(nc, h->d_offs.get(), h->d_xy.get(), dout, h->stream.get()) != hipSuccess ||
      hipMemcpyAsync(out, dout, sizeof(int) * nc, hipMemcpyDeviceToHost, h->stream.get()) !=
          hipSuccess)
    return EKF_E_HIP;
  return hipStreamSynchronize(h->stream.get()) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

int lm_last_kernel_us(lm_t h, double* us) {
  if (!h || !us || !h->timed) return EKF_E_ARG;
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, h->e0.get(), h->e1.get()) != hipSuccess) return EKF_E_HIP;
  *us = 1e3 * ms;
  return EKF_OK;
}

}  // extern "C"
