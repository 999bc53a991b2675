// Gather and score (gfx950 / CDNA4): the marginals of a filter's Σ — the 3×3 pose block and the N
// diagonal 2×2 landmark blocks, 0.4 % of Σ's bytes at N = 256 — read where they lie, and a filter's
// score against the truth (eval_math.hpp) reduced on the device. One 256-thread workgroup per
// filter; a lane owns the landmark slots lane, lane + 256, …. Built with -ffp-contract=off.
//
// Column 3 + 2j is odd, so a slot's two entries of a row are 8-byte aligned in fp64 and 4-byte
// aligned in fp32: they are read as scalars. The reduction is a lane's slots in ascending order,
// then a binary tree over the 256 lanes in LDS (lane t takes lane t + s for s = 128, 64, …, 1):
// one order whatever the hardware does, no atomics, so the same state gives the same bits.
// Only the outputs are written: Σ, x, FilterCtl, the trace and the planning state are read at most.
#include <hip/hip_runtime.h>

#include "ekf_device.hpp"
#include "ekf_launch.hpp"
#include "eval_math.hpp"

namespace ekfslam {

namespace {

constexpr int kEvalThreads = 256;

// Filter f's "in" copies.
template <typename T>
struct FilterView {
  const T* sig;
  const double* x;
  int ld;
  __device__ double s(int i, int j) const {
    return static_cast<double>(sig[static_cast<size_t>(i) * ld + j]);
  }
};

template <typename T>
__device__ __forceinline__ FilterView<T> view_of(const EvalArgs& A, int f) {
  const int p = A.parity[f] & 1;
  return FilterView<T>{static_cast<const T*>(A.sig[p]) + f * A.sig_stride,
                       A.x[p] + f * A.x_stride, A.ld};
}

// slot j: its estimate and the symmetrised block {xx, xy, yy} at rows and columns 3 + 2j, 4 + 2j
template <typename T>
__device__ __forceinline__ void gather_slot(const FilterView<T>& v, int j, double* xy, double* C) {
  const int r = 3 + 2 * j;
  xy[0] = v.x[r];
  xy[1] = v.x[r + 1];
  C[0] = v.s(r, r);
  C[1] = sym_part(v.s(r, r + 1), v.s(r + 1, r));
  C[2] = v.s(r + 1, r + 1);
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(kEvalThreads) void k_marginals(EvalArgs A, MarginalOut O) {
  const int k = blockIdx.x, f = A.f0 + k, t = threadIdx.x;
  const FilterView<T> v = view_of<T>(A, f);
  if (t < 3 && O.pose) O.pose[3 * k + t] = v.x[t];
  if (t < 9 && O.pose_cov) O.pose_cov[9 * k + t] = sym_part(v.s(t / 3, t % 3), v.s(t % 3, t / 3));
  if (t == 0 && O.counter) O.counter[k] = A.ctl[f].counter;
  if (!O.lm) return;
  for (int j = t; j < A.N; j += kEvalThreads) {
    LmMarginal m;
    gather_slot(v, j, m.xy, m.cov);
    m.seen = lm_seen(m.xy[0], m.xy[1]) ? 1 : 0;
    m.pad = 0;
    O.lm[static_cast<size_t>(k) * A.N + j] = m;
  }
}

template <typename T>
__global__ __launch_bounds__(kEvalThreads) void k_eval(EvalArgs A, EvalTruth Tr, EvalRec* out) {
  __shared__ LmAcc sh[kEvalThreads];
  const int k = blockIdx.x, f = A.f0 + k, t = threadIdx.x;
  const FilterView<T> v = view_of<T>(A, f);
  Pose2 inv{};
  if (Tr.has_frame) inv = inverse(Pose2{Tr.frame[0], Tr.frame[1], Tr.frame[2]});
  const Pose2* invp = Tr.has_frame ? &inv : nullptr;
  const double* tlm = Tr.lm ? Tr.lm + static_cast<size_t>(f) * Tr.n_map * 2 : nullptr;
  LmAcc acc{};
  for (int j = t; j < A.N; j += kEvalThreads) {
    double xy[2], C[3];
    gather_slot(v, j, xy, C);
    lm_score(&acc, xy[0], xy[1], C, tlm && j < Tr.n_map ? tlm + 2 * j : nullptr, invp);
  }
  sh[t] = acc;
  __syncthreads();
  for (int s = kEvalThreads / 2; s > 0; s >>= 1) {
    if (t < s) lm_merge(&sh[t], sh[t + s]);
    __syncthreads();
  }
  if (t != 0) return;
  EvalRec r{};
  const double est[3] = {v.x[0], v.x[1], v.x[2]};
  const double P[6] = {v.s(0, 0),
                       sym_part(v.s(0, 1), v.s(1, 0)),
                       sym_part(v.s(0, 2), v.s(2, 0)),
                       v.s(1, 1),
                       sym_part(v.s(1, 2), v.s(2, 1)),
                       v.s(2, 2)};
  score_pose(est, P, Tr.pose + f * Tr.pose_stride, invp, &r);
  lm_store(sh[0], &r);
  out[k] = r;
}

template <typename T>
hipError_t launch_marginals(const EvalArgs& a, const MarginalOut& o, int nf, hipStream_t s) {
  hipLaunchKernelGGL(k_marginals<T>, dim3(nf), dim3(kEvalThreads), 0, s, a, o);
  return hipGetLastError();
}
template hipError_t launch_marginals<double>(const EvalArgs&, const MarginalOut&, int, hipStream_t);
template hipError_t launch_marginals<float>(const EvalArgs&, const MarginalOut&, int, hipStream_t);

template <typename T>
hipError_t launch_eval(const EvalArgs& a, const EvalTruth& t, EvalRec* out, int nf, hipStream_t s) {
  hipLaunchKernelGGL(k_eval<T>, dim3(nf), dim3(kEvalThreads), 0, s, a, t, out);
  return hipGetLastError();
}
template hipError_t launch_eval<double>(const EvalArgs&, const EvalTruth&, EvalRec*, int,
                                        hipStream_t);
template hipError_t launch_eval<float>(const EvalArgs&, const EvalTruth&, EvalRec*, int,
                                       hipStream_t);

}  // namespace ekfslam
