// pyekf.synth's counter-based RNG on the device, draw for draw (synth.rng_u64 / rng_uniform /
// rng_normal): every draw is a pure function of (seed, stream, index). Shared by the simulator
// kernels (sim_kernels.hip: streams 1 and 2) and the lidar scan kernel (lidar_kernels.hip: 6).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace ekfslam {

constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double uniform(unsigned long long seed, unsigned long long stream,
                                          unsigned long long idx) {
  const unsigned long long key = mix64(seed * kGolden + stream);
  return static_cast<double>(mix64(key + (idx + 1) * kGolden) >> 11) * 0x1p-53;
}
// N(0, 1) by Box–Muller from draws 2·idx, 2·idx + 1 (synth.rng_normal)
__device__ __forceinline__ double normal(unsigned long long seed, unsigned long long stream,
                                         unsigned long long idx) {
  const double u1 = 1.0 - uniform(seed, stream, 2 * idx);
  const double u2 = uniform(seed, stream, 2 * idx + 1);
  return sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
}

}  // namespace ekfslam
