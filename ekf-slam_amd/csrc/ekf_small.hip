// The filter's small kernels (gfx950 / CDNA4): the posterior t_map_odom of filters with no pending
// Σ pass, the Σ₀ diagonal, and the LDS poisoner of the tests.
#include <hip/hip_runtime.h>

#include "ekf_device.hpp"
#include "ekf_launch.hpp"
#include "geom.hpp"

namespace ekfslam {

template <typename T>
__global__ void k_posterior(PassArgs<T> A, int nf) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nf) return;
  const MsgDesc& d = A.desc[k];
  if (!(d.flags & kActive)) return;
  const int f = A.f0 + k;
  const double* x = A.x[d.parity] + f * A.x_stride;
  FilterCtl* ctl = A.ctl + f;
  const Pose2 tmo = compose(Pose2{x[0], x[1], x[2]}, inverse(Pose2{d.odom[0], d.odom[1], d.odom[2]}));
  ctl->tmo[0] = tmo.theta;
  ctl->tmo[1] = tmo.x;
  ctl->tmo[2] = tmo.y;
  if (A.trace)  // the pose trace's record (one thread per filter)
    A.trace_n[f] = trace_append(A, f, A.trace_n[f], x[0], x[1], x[2], tmo.theta, tmo.x, tmo.y);
}

template <typename T>
__global__ void k_init_diag(T* sig, size_t stride, int n, int ld, double v, int nf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x + 3;
  if (i >= n) return;
  for (int f = blockIdx.y; f < nf; f += gridDim.y)
    sig[f * stride + static_cast<size_t>(i) * ld + i] = static_cast<T>(v);
}
template <typename T>
hipError_t launch_posterior(const PassArgs<T>& a, int nf, hipStream_t s) {
  hipLaunchKernelGGL(k_posterior<T>, dim3((nf + 63) / 64), dim3(64), 0, s, a, nf);
  return hipGetLastError();
}
template hipError_t launch_posterior<double>(const PassArgs<double>&, int, hipStream_t);
template hipError_t launch_posterior<float>(const PassArgs<float>&, int, hipStream_t);

template <typename T>
hipError_t launch_init_diag(T* sig, size_t stride, int n, int ld, double v, int nf, hipStream_t s) {
  hipLaunchKernelGGL(k_init_diag<T>, dim3((n + 255) / 256, nf < 65535 ? nf : 65535), dim3(256), 0,
                     s, sig, stride, n, ld, v, nf);
  return hipGetLastError();
}
template hipError_t launch_init_diag<double>(double*, size_t, int, int, double, int, hipStream_t);
template hipError_t launch_init_diag<float>(float*, size_t, int, int, double, int, hipStream_t);

// Diagnostics (ekf_debug_poison_lds): overwrite a workgroup's whole LDS allocation with a NaN bit
// pattern. Launched over every CU several times, it leaves LDS the way an arbitrary previous kernel
// may, so a kernel that reads LDS it never wrote shows it deterministically (tests/).
__global__ __launch_bounds__(256) void k_poison_lds(unsigned long long pattern) {
  extern __shared__ unsigned long long lds_poison[];
  for (int e = threadIdx.x; e < kPoisonLdsBytes / 8; e += blockDim.x) lds_poison[e] = pattern;
  __syncthreads();
  // keep the stores: one lane publishes a word the compiler cannot prove dead
  if (threadIdx.x == 0 && lds_poison[blockIdx.x % (kPoisonLdsBytes / 8)] == 0x1ull)
    lds_poison[0] = 0;
}

hipError_t launch_poison_lds(unsigned long long pattern, int n_blocks, hipStream_t s) {
  hipLaunchKernelGGL(k_poison_lds, dim3(n_blocks), dim3(256), kPoisonLdsBytes, s, pattern);
  return hipGetLastError();
}

}  // namespace ekfslam
