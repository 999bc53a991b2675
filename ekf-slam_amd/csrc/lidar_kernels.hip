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
// Shape: grid S × ⌈B/256⌉, one thread per beam, so no result depends on the grid and there are no
// atomics. A block stages its scan's scene in LDS as three arrays (f_x, f_y, |f|² − r²: the
// beam-independent half of the test, done once per block instead of once per beam); in the beam
// loop every lane reads the same entry, an LDS broadcast.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lm_launch.hpp"
#include "sim_rng.hpp"

namespace lmk {
namespace {

constexpr int kScanThreads = 256;
constexpr unsigned long long kLidarStream = 6;  // synth._S_LIDAR
constexpr double kLidarOffset = 0.032;          // nusim.cpp:577: the laser sits behind the body origin

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
  if (blockIdx.y == 0 && threadIdx.x == 0) {  // the LaserScan header lm_detect's kernels read
    A.angle_min[s] = 0.0;
    A.angle_inc[s] = static_cast<double>(static_cast<float>(2.0 * M_PI / A.n_beams));
  }
  __syncthreads();
  if (b >= A.n_beams) return;

  const double th = th0 + static_cast<double>(b) * (2.0 * M_PI / A.n_beams);
  const double dx = cos(th), dy = sin(th);
  double best = INFINITY;
  for (int c = 0; c < C; ++c) {
    const double bq = s_fx[c] * dx + s_fy[c] * dy;
    const double disc = bq * bq - s_cc[c];
    if (disc >= 0.0) {
      const double t = -bq - sqrt(disc);
      if (t > 0.0) best = fmin(best, t);
    }
  }
  const double hx = A.arena_w / 2.0, hy = A.arena_h / 2.0;
  if (dx > 1e-12) best = fmin(best, (hx - lx) / dx);
  if (-dx > 1e-12) best = fmin(best, (hx - -lx) / -dx);
  if (dy > 1e-12) best = fmin(best, (hy - ly) / dy);
  if (-dy > 1e-12) best = fmin(best, (hy - -ly) / -dy);
  best = fmin(fmax(best, A.range_min), A.range_max);
  if (A.sigma > 0.0) {
    const unsigned long long idx =
        (static_cast<unsigned long long>(A.scan0) + s) * A.n_beams + b;
    best = best + A.sigma * ekfslam::normal(A.seed, kLidarStream, idx);
  }
  A.ranges[static_cast<size_t>(s) * A.n_beams + b] = static_cast<float>(best);
}

}  // namespace

hipError_t launch_scan(const ScanArgs& a, hipStream_t st) {
  const dim3 grid(a.n_scans, (a.n_beams + kScanThreads - 1) / kScanThreads);
  const size_t lds = sizeof(double) * 3 * static_cast<size_t>(a.n_circles);
  hipLaunchKernelGGL(k_lidar_scan, grid, dim3(kScanThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace lmk
