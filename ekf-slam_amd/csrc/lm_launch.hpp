// Landmark front-end launchers (defined in lm_kernels.hip, called by lm_api.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "landmarks.h"

namespace lmk {

// One circle candidate (a cluster of 4..39 points) of the batch-wide list.
struct Cand {
  int scan, s0, n0, s1, n, pass;
  double cx, cy, r;
};

// Clusters with ≥ 4 points in a scan of B beams: each needs 4 points and a dropped break point.
inline int max_candidates(int B) { return B / 5 + 2; }
// The candidate list is split into regions (scan s → region s mod kRegions), one counter each.
constexpr int kRegions = 64;
inline size_t candidate_capacity(int S, int B) {
  return static_cast<size_t>(kRegions) * ((S + kRegions - 1) / kRegions) * max_candidates(B);
}

// Device workspace of lm_detect for up to S scans of B beams.
struct DetectWork {
  double* px;    // [S][B] beam points
  double* py;
  Cand* cand;    // [candidate_capacity(S, B)]: kRegions dense lists
  int* gcount;   // [kRegions] candidates in each region's list
  int* sbase;    // [S] first candidate of each scan
  int* sncand;   // [S] candidates of each scan (LM_NO_BREAK: no cluster break)
};

// Clusters, circle test, Hyper fit, marker compaction (k_clusters → k_candidates → k_markers).
hipError_t launch_detect(const float* ranges, int n_scans, int n_beams, const double* angle_min,
                         const double* angle_inc, double threshold, lm_marker* out,
                         int max_markers, int* counts, const DetectWork& w, hipStream_t st);
// One lane per point set: fitCircle / checkCircle on clusters given by offsets.
hipError_t launch_fit(int n_clusters, const int* offsets, const double* xy, double* out,
                      hipStream_t st);
hipError_t launch_check(int n_clusters, const int* offsets, const double* xy, int* out,
                        hipStream_t st);

// lm_simulate's kernel (lidar_kernels.hip): device pointers and the lm_scan_config by value.
struct ScanArgs {
  const double* poses;    // [S][3] body (θ, x, y)
  const double* circles;  // [G][C][3] (x, y, r); unread when n_circles = 0
  const int* scene;       // [S] in [0, G), nullptr: scene 0
  float* ranges;          // [S][B] out
  double* angle_min;      // [S] out: 0
  double* angle_inc;      // [S] out: float32(2π/B)
  int n_scans, n_beams, n_circles;  // n_circles ≤ LM_MAX_CIRCLES
  unsigned long long seed;
  long long scan0;
  double arena_w, arena_h, range_min, range_max, sigma;
};
hipError_t launch_scan(const ScanArgs& a, hipStream_t st);

// ekf_sim_run_lidar's kernel (k_lidar_scan_swarm): a simulator run scanned where it lies. Scan
// s = t·F + f is message t of filter f: its pose poses[s], its scene filter f's map with one
// radius, its noise seed + f with beam b on draw (msg0 + t)·B + b.
struct SwarmScanArgs {
  const double* poses;  // [T·F][3] body (θ, x, y): the simulator's truth buffer
  const double* lm;     // [F][L][2] cylinder centres: the simulator's maps
  float* ranges;        // [T·F][B] out
  double* angle_min;    // [T·F] out: 0
  double* angle_inc;    // [T·F] out: float32(2π/B)
  int n_scans, n_beams, n_filters, n_map;  // n_scans = T·F; 1 ≤ n_map ≤ LM_MAX_CIRCLES
  unsigned long long seed;                 // the simulator's seed + f0
  long long msg0;                          // the run's first message
  double radius, arena_w, arena_h, range_min, range_max, sigma;
  int cull_from;  // maps of fewer cylinders are staged whole (kCullFromMap)
};
// The smallest map the swarm kernel culls. Below it the cull's own cost (a second barrier, the
// ballot and the LDS atomic) is not earned back: DESIGN.md has the measurement it was read from.
// EKF_LIDAR_CULL_FROM overrides it for that measurement (tools/lidar_mc_bench.py); same bits.
constexpr int kCullFromMap = 32;
hipError_t launch_scan_swarm(const SwarmScanArgs& a, hipStream_t st);

}  // namespace lmk
