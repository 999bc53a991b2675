// nusim's simulated laser on the device (publish_lidar_data, nusim/src/nusim.cpp:559-710):
// k_lidar_scan ray-casts S scans of B beams against each scan's cylinders and the four walls of an
// axis-aligned arena centred on the origin, into the range buffer lm_detect's kernels read.
//
// The arithmetic is pyekf.synth.lidar_scans' (its counter-RNG twin lidar_scans_counter is the host
// restatement this is tested against), expression for expression, and the file is compiled with
// -ffp-contract=off so every product and sum rounds as numpy's does. With f = lidar − centre and
// unit direction d, bq = f·d, disc = bq² − (|f|² − r²); a hit is disc ≥ 0 with t = −bq − √disc > 0.
// That is the reference's own answer whenever the lidar is outside every cylinder and inside the
// arena:
//  * the reference projects the centre on the beam (u1 = (u·d) d, chord half-length m) and takes
//    min(|s + m|, |s − m|) with s = u·d = −bq and m = √disc: for s > m > 0 (the lidar outside the
//    cylinder, the cylinder ahead) that is s − m, the near root taken here;
//  * its m is NaN when the beam's line misses the cylinder (negative radicand), every comparison
//    with NaN is false, and the obstacle is passed over: a miss, disc < 0 here;
//  * its walls are infinite lines, hit where the beam's line crosses them in front of the lidar.
//    Inside a convex arena the nearest such crossing lies on the arena's boundary, so the nearest
//    line and the nearest wall segment are the same: min over den > 0 of (lim − org) / den.
// Two differences remain, both out of that domain's way: the reference only looks at walls when no
// cylinder was hit (inside the arena a cylinder hit is nearer than the wall behind it, so the
// minimum over both is the same), and it skips a cylinder whose centre is behind the lidar even if
// the lidar stands inside it.
//
// Noise (nusim.cpp:701-707): σ·N(0, 1) added after the clamp, beam b of scan s taking normal draw
// (scan0 + s)·B + b of stream 6 under the configuration's seed (synth._S_LIDAR); σ = 0 draws
// nothing. The sum is then rounded to float32, the LaserScan's type.
//
// Shape: grid S × ⌈B/256⌉, one thread per beam, so no result depends on the grid and k_lidar_scan
// has no atomics. A block stages its scan's scene in LDS as three arrays (f_x, f_y, |f|² − r²: the
// beam-independent half of the test, done once per block instead of once per beam); in the beam
// loop every lane reads the same entry, an LDS broadcast.
// k_lidar_scan_swarm (below) is the same laser on a simulator run's device buffers, its scene
// culled to what range_max can reach while it is staged; same beam body, same bits.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lm_launch.hpp"
#include "sim_rng.hpp"

namespace lmk {
namespace {

constexpr int kScanThreads = 256;
constexpr unsigned long long kLidarStream = 6;  // synth._S_LIDAR
constexpr double kLidarOffset = 0.032;          // nusim.cpp:577: the laser sits behind the body origin

// What the beam body needs beside the staged scene: the LaserScan geometry and the noise stream.
struct BeamCfg {
  int n_beams;
  double arena_w, arena_h, range_min, range_max, sigma;
  unsigned long long seed;  // the scan's noise seed
  unsigned long long scan;  // the scan's index in that seed's stream 6 (draw scan·B + b)
};

// The LaserScan header lm_detect's kernels read.
__device__ __forceinline__ void write_header(double* angle_min, double* angle_inc, int s,
                                             int n_beams) {
  angle_min[s] = 0.0;
  angle_inc[s] = static_cast<double>(static_cast<float>(2.0 * M_PI / n_beams));
}

// Beam b of a scan taken from lidar (lx, ly) at heading th0 against the n staged cylinders: the
// per-beam half of both kernels, expression for expression what k_lidar_scan has always run.
__device__ __forceinline__ float beam_range(const double* s_fx, const double* s_fy,
                                            const double* s_cc, int n, double th0, double lx,
                                            double ly, int b, const BeamCfg& K) {
  const double th = th0 + static_cast<double>(b) * (2.0 * M_PI / K.n_beams);
  const double dx = cos(th), dy = sin(th);
  double best = INFINITY;
  for (int c = 0; c < n; ++c) {
    const double bq = s_fx[c] * dx + s_fy[c] * dy;
    const double disc = bq * bq - s_cc[c];
    if (disc >= 0.0) {
      const double t = -bq - sqrt(disc);
      if (t > 0.0) best = fmin(best, t);
    }
  }
  const double hx = K.arena_w / 2.0, hy = K.arena_h / 2.0;
  if (dx > 1e-12) best = fmin(best, (hx - lx) / dx);
  if (-dx > 1e-12) best = fmin(best, (hx - -lx) / -dx);
  if (dy > 1e-12) best = fmin(best, (hy - ly) / dy);
  if (-dy > 1e-12) best = fmin(best, (hy - -ly) / -dy);
  best = fmin(fmax(best, K.range_min), K.range_max);
  if (K.sigma > 0.0) {
    const unsigned long long idx = K.scan * K.n_beams + b;
    best = best + K.sigma * ekfslam::normal(K.seed, kLidarStream, idx);
  }
  return static_cast<float>(best);
}

__global__ __launch_bounds__(kScanThreads) void k_lidar_scan(ScanArgs A) {
  extern __shared__ double s_scene[];  // 3·C doubles (≤ 24 KB at LM_MAX_CIRCLES)
  const int C = A.n_circles;
  double* const s_fx = s_scene;
  double* const s_fy = s_scene + C;
  double* const s_cc = s_scene + 2 * C;
  const int s = blockIdx.x;
  const int b = blockIdx.y * kScanThreads + threadIdx.x;
  const double th0 = A.poses[3 * s], px = A.poses[3 * s + 1], py = A.poses[3 * s + 2];
  const double lx = px - kLidarOffset * cos(th0);
  const double ly = py - kLidarOffset * sin(th0);
  const double* circ =
      A.circles + static_cast<size_t>(A.scene ? A.scene[s] : 0) * (3 * static_cast<size_t>(C));
  for (int c = threadIdx.x; c < C; c += kScanThreads) {
    const double cx = circ[3 * c], cy = circ[3 * c + 1], r = circ[3 * c + 2];
    const double fx = lx - cx, fy = ly - cy;
    s_fx[c] = fx;
    s_fy[c] = fy;
    s_cc[c] = fx * fx + fy * fy - r * r;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) write_header(A.angle_min, A.angle_inc, s, A.n_beams);
  __syncthreads();
  if (b >= A.n_beams) return;
  const BeamCfg K{A.n_beams, A.arena_w, A.arena_h, A.range_min, A.range_max, A.sigma, A.seed,
                  static_cast<unsigned long long>(A.scan0) + s};
  A.ranges[static_cast<size_t>(s) * A.n_beams + b] =
      beam_range(s_fx, s_fy, s_cc, C, th0, lx, ly, b, K);
}

// ---- the swarm's laser: device-resident inputs, the scene culled while it is staged ------------
// k_lidar_scan_swarm scans a simulator run where it lies (ekf_sim_run_lidar): scan s = t·F + f is
// message t of filter f, its pose poses[s] (the simulator's truth buffer), its scene filter f's map
// lm[f][L][2] with one radius r for every cylinder. Noise as the simulator shards it: seed + f
// (the caller has added f0), beam b taking draw (msg0 + t)·B + b of stream 6 — the bits of
// k_lidar_scan run per filter with that seed and scan0 = msg0.
//
// The cull. A swarm map spans ±0.5·√N m and the laser reaches range_max, so most cylinders can
// never be a beam's answer. While staging, a thread keeps its cylinder unless
//     |f|·(1 − 2⁻²⁰) − r > range_max,            |f| = sqrt(fx² + fy²) as computed,
// and the beam loop runs over the kept ones only. Kept slots are handed out by wave ballot and one
// LDS atomicAdd per wave and round, so the kept list's order changes from run to run; the beam's
// result is an fmin over the positive finite t of its hits, which no order changes.
// Why the output is k_lidar_scan's bit for bit, for every input: a dropped cylinder can only ever
// have contributed a computed t ≥ range_max, and fmin(fmax(min(X, t), range_min), range_max) =
// fmin(fmax(X, range_min), range_max) for every X once t ≥ range_max ≥ range_min (both sides are
// range_max when X ≥ t, and t is not looked at when X < t).
//  * range_max ≤ 0: a contributing t is > 0 ≥ range_max.
//  * range_max > 0: the test gives |f| > r ≥ 0. A hit has p = −bq > 0, and t = p − √(p² − c),
//    c = |f|² − r², falls as p grows; p ≤ |f||d|, so in exact arithmetic on the staged f and the
//    computed d, t ≥ |f||d| − √(r² + η|f|²) ≥ |f|(1 − |η|/2 − √|η|) − r with |d|² = 1 + η. cos and
//    sin are good to an ulp or two, |η| < 2⁻⁵⁰, √|η| < 3·10⁻⁸. Rounding: bq carries ≤ 3u|f|
//    (u = 2⁻⁵³), disc ≤ 8u|f|² absolute (bq², the three roundings of c, the difference), which
//    moves its root by at most √(8u)|f| < 3·10⁻⁸|f| (the grazing case; far less away from it), the
//    root and the last difference ≤ 2u|f| more. The computed t ≥ |f|(1 − 7·10⁻⁸) − r, and the
//    test's own |f| and product are off by ≤ 3u|f|. The margin 2⁻²⁰ ≈ 9.5·10⁻⁷ is 13 times that.
//  * NaN anywhere in the test (a NaN pose or map entry) compares false: kept.
// A kept cylinder is staged and tested exactly as k_lidar_scan does it (beam_range is shared).
// Maps of fewer than cull_from cylinders (kCullFromMap, lm_launch.hpp) are staged whole instead:
// there the cull's second barrier, ballot and atomic cost more than the beams it saves.
constexpr double kCullMargin = 0x1p-20;

__global__ __launch_bounds__(kScanThreads) void k_lidar_scan_swarm(SwarmScanArgs A) {
  extern __shared__ double s_scene[];  // 3·L doubles (≤ 24 KB at LM_MAX_CIRCLES)
  __shared__ int s_kept;
  const int L = A.n_map;
  double* const s_fx = s_scene;
  double* const s_fy = s_scene + L;
  double* const s_cc = s_scene + 2 * L;
  const int s = blockIdx.x, f = s % A.n_filters, t = s / A.n_filters;
  const int b = blockIdx.y * kScanThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const double th0 = A.poses[3 * s], px = A.poses[3 * s + 1], py = A.poses[3 * s + 2];
  const double lx = px - kLidarOffset * cos(th0);
  const double ly = py - kLidarOffset * sin(th0);
  const double* lm = A.lm + static_cast<size_t>(f) * (2 * static_cast<size_t>(L));
  const double r = A.radius;
  const bool cull = L >= A.cull_from;  // (the block's, like everything the barriers hang on)
  if (cull) {
    if (threadIdx.x == 0) s_kept = 0;
    __syncthreads();
    // (the trip count is the block's, so every lane of a wave reaches the ballot)
    for (int c0 = 0; c0 < L; c0 += kScanThreads) {
      const int c = c0 + threadIdx.x;
      double fx = 0.0, fy = 0.0;
      bool keep = false;
      if (c < L) {
        fx = lx - lm[2 * c];
        fy = ly - lm[2 * c + 1];
        keep = !(sqrt(fx * fx + fy * fy) * (1.0 - kCullMargin) - r > A.range_max);
      }
      const unsigned long long kept = __ballot(keep);
      if (kept == 0) continue;
      const int first = __ffsll(static_cast<long long>(kept)) - 1;
      int base = 0;
      if (lane == first) base = atomicAdd(&s_kept, __popcll(kept));
      base = __shfl(base, first);
      if (keep) {
        // (a slot per kept cylinder, so slot < L)
        const int slot = base + __popcll(kept & ((1ull << lane) - 1ull));
        s_fx[slot] = fx;
        s_fy[slot] = fy;
        s_cc[slot] = fx * fx + fy * fy - r * r;
      }
    }
  } else {  // a small map: every cylinder staged in place, as k_lidar_scan does
    for (int c = threadIdx.x; c < L; c += kScanThreads) {
      const double fx = lx - lm[2 * c], fy = ly - lm[2 * c + 1];
      s_fx[c] = fx;
      s_fy[c] = fy;
      s_cc[c] = fx * fx + fy * fy - r * r;
    }
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) write_header(A.angle_min, A.angle_inc, s, A.n_beams);
  __syncthreads();
  if (b >= A.n_beams) return;
  const int n = cull ? s_kept : L;
  const BeamCfg K{A.n_beams, A.arena_w, A.arena_h, A.range_min, A.range_max, A.sigma,
                  A.seed + static_cast<unsigned long long>(f),
                  static_cast<unsigned long long>(A.msg0) + t};
  A.ranges[static_cast<size_t>(s) * A.n_beams + b] =
      beam_range(s_fx, s_fy, s_cc, n, th0, lx, ly, b, K);
}

}  // namespace

hipError_t launch_scan(const ScanArgs& a, hipStream_t st) {
  const dim3 grid(a.n_scans, (a.n_beams + kScanThreads - 1) / kScanThreads);
  const size_t lds = sizeof(double) * 3 * static_cast<size_t>(a.n_circles);
  hipLaunchKernelGGL(k_lidar_scan, grid, dim3(kScanThreads), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_scan_swarm(const SwarmScanArgs& a, hipStream_t st) {
  const dim3 grid(a.n_scans, (a.n_beams + kScanThreads - 1) / kScanThreads);
  const size_t lds = sizeof(double) * 3 * static_cast<size_t>(a.n_map);
  hipLaunchKernelGGL(k_lidar_scan_swarm, grid, dim3(kScanThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace lmk
