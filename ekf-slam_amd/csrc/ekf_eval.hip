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
// k_eval_match scores against a truth map in any order: it stages the truth in LDS, matches every
// seen slot to its nearest truth landmark (match_math.hpp) and reduces the same way; its claims are
// an integer minimum and its counts integers, so the order of the LDS atomics does not show.
#include <hip/hip_runtime.h>

#include "ekf_device.hpp"
#include "ekf_launch.hpp"
#include "eval_math.hpp"
#include "match_math.hpp"

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

// ---- k_eval_match: the truth in any order — match every seen slot to its nearest truth landmark,
// then score it against that one (match_math.hpp). All LDS is dynamic and carved in multiples of
// 16 bytes, so the 16-byte reads of the staged truth stay aligned:
//   pts[n_map]    the truth in the map frame, (x, y) interleaved: one 16-byte read per landmark,
//                 the same address in every lane (a broadcast, no bank conflicts)
//   sh, shm[256]  the two reduction trees
//   claim[n_map]  the lowest slot matched to each truth landmark

namespace {

constexpr int kMatchBlock = 4;  // slots a lane holds in registers per walk over the truth

struct MatchLds {
  double2* pts;
  LmAcc* sh;
  MatchAcc* shm;
  int* claim;
};
__device__ __forceinline__ MatchLds carve_match(char* base, int n_map) {
  MatchLds l;
  l.pts = reinterpret_cast<double2*>(base);
  l.sh = reinterpret_cast<LmAcc*>(base + static_cast<size_t>(n_map) * sizeof(double2));
  l.shm = reinterpret_cast<MatchAcc*>(l.sh + kEvalThreads);
  l.claim = reinterpret_cast<int*>(l.shm + kEvalThreads);
  return l;
}
static_assert(sizeof(LmAcc) * kEvalThreads % 16 == 0 && sizeof(MatchAcc) * kEvalThreads % 16 == 0,
              "16-byte carve");
size_t match_lds_bytes(int n_map) {
  return static_cast<size_t>(n_map) * (sizeof(double2) + sizeof(int)) +
         kEvalThreads * (sizeof(LmAcc) + sizeof(MatchAcc));
}

// Stage: filter f's truth into the map frame and into LDS, the claims free; counts the landmarks
// that are there. Every entry of pts and claim is written before the barrier that follows.
__device__ __forceinline__ int stage_truth(const MatchLds& l, const double* tlm, int n_map,
                                           const Pose2* invp, int t) {
  int n_truth = 0;
  for (int k = t; k < n_map; k += kEvalThreads) {
    const double x = tlm[2 * k], y = tlm[2 * k + 1];
    double2 p;
    truth_point_in_map(invp, x, y, &p.x, &p.y);
    n_truth += truth_present(x, y) ? 1 : 0;
    l.pts[k] = p;
    l.claim[k] = kClaimFree;
  }
  return n_truth;
}

// Scan and claim: the lane's slots in blocks of kMatchBlock, one walk over the truth per block.
// match[j] = the slot's truth landmark or −1; a matched slot bids for its landmark.
template <typename T>
__device__ __forceinline__ void scan_and_claim(const FilterView<T>& v, const MatchLds& l, int N,
                                               int n_map, double gate2, int* match, int t) {
  for (int j0 = t; j0 < N; j0 += kEvalThreads * kMatchBlock) {
    double ex[kMatchBlock], ey[kMatchBlock];
    Nearest best[kMatchBlock];
#pragma unroll
    for (int b = 0; b < kMatchBlock; ++b) {
      const int j = j0 + b * kEvalThreads;
      ex[b] = j < N ? v.x[3 + 2 * j] : 0.0;  // (a slot past N counts as unseen)
      ey[b] = j < N ? v.x[4 + 2 * j] : 0.0;
      best[b] = nearest_none();
    }
    for (int k = 0; k < n_map; ++k) {
      const double2 p = l.pts[k];
#pragma unroll
      for (int b = 0; b < kMatchBlock; ++b) nearest_step(&best[b], k, ex[b], ey[b], p.x, p.y);
    }
#pragma unroll
    for (int b = 0; b < kMatchBlock; ++b) {
      const int j = j0 + b * kEvalThreads;
      if (j >= N) continue;
      const bool hit = lm_seen(ex[b], ey[b]) && match_gate(best[b], gate2);
      match[j] = hit ? best[b].k : -1;
      if (hit) claim_take(&l.claim[best[b].k], j);
    }
  }
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(kEvalThreads) void k_eval_match(EvalArgs A, EvalTruth Tr, double gate2,
                                                             MatchOut O) {
  extern __shared__ __attribute__((aligned(16))) char match_lds[];
  const int k = blockIdx.x, f = A.f0 + k, t = threadIdx.x;
  const MatchLds l = carve_match(match_lds, Tr.n_map);
  const FilterView<T> v = view_of<T>(A, f);
  Pose2 inv{};
  if (Tr.has_frame) inv = inverse(Pose2{Tr.frame[0], Tr.frame[1], Tr.frame[2]});
  const Pose2* invp = Tr.has_frame ? &inv : nullptr;
  int* match = O.match + static_cast<size_t>(k) * A.N;
  MatchAcc macc{};
  macc.n_truth =
      stage_truth(l, Tr.lm + static_cast<size_t>(f) * Tr.n_map * 2, Tr.n_map, invp, t);
  __syncthreads();
  scan_and_claim(v, l, A.N, Tr.n_map, gate2, match, t);
  __syncthreads();
  // Score: k_eval's loop, with the slot's truth the staged point it matched (already in the map
  // frame) or none. (match[j] was written by this lane.)
  LmAcc acc{};
  for (int j = t; j < A.N; j += kEvalThreads) {
    double xy[2], C[3];
    gather_slot(v, j, xy, C);
    const int m = match[j];
    double pt[2] = {0.0, 0.0};
    if (m >= 0) {
      const double2 p = l.pts[m];
      pt[0] = p.x;
      pt[1] = p.y;
      const double dx = xy[0] - pt[0], dy = xy[1] - pt[1];
      match_count(&macc, j, dx * dx + dy * dy, l.claim[m]);
    }
    lm_score(&acc, xy[0], xy[1], C, m >= 0 ? pt : nullptr, nullptr);
  }
  l.sh[t] = acc;
  l.shm[t] = macc;
  __syncthreads();
  for (int s = kEvalThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      lm_merge(&l.sh[t], l.sh[t + s]);
      match_merge(&l.shm[t], l.shm[t + s]);
    }
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
  lm_store(l.sh[0], &r);
  O.rec[k] = r;
  O.mrec[k] = match_store(l.shm[0], r.n_seen);
}

template <typename T>
hipError_t launch_eval_match(const EvalArgs& a, const EvalTruth& t, double gate2, const MatchOut& o,
                             int nf, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  if (t.n_map < 1 || t.n_map > kMatchMaxMap) return hipErrorInvalidValue;
  const size_t lds = match_lds_bytes(t.n_map);
  if (e0 && e1)
    hipExtLaunchKernelGGL(k_eval_match<T>, dim3(nf), dim3(kEvalThreads), lds, s, e0, e1, 0, a, t,
                          gate2, o);
  else
    hipLaunchKernelGGL(k_eval_match<T>, dim3(nf), dim3(kEvalThreads), lds, s, a, t, gate2, o);
  return hipGetLastError();
}
template hipError_t launch_eval_match<double>(const EvalArgs&, const EvalTruth&, double,
                                              const MatchOut&, int, hipStream_t, hipEvent_t,
                                              hipEvent_t);
template hipError_t launch_eval_match<float>(const EvalArgs&, const EvalTruth&, double,
                                             const MatchOut&, int, hipStream_t, hipEvent_t,
                                             hipEvent_t);

template <typename T>
hipError_t launch_marginals(const EvalArgs& a, const MarginalOut& o, int nf, hipStream_t s) {
  hipLaunchKernelGGL(k_marginals<T>, dim3(nf), dim3(kEvalThreads), 0, s, a, o);
  return hipGetLastError();
}
template hipError_t launch_marginals<double>(const EvalArgs&, const MarginalOut&, int, hipStream_t);
template hipError_t launch_marginals<float>(const EvalArgs&, const MarginalOut&, int, hipStream_t);

template <typename T>
hipError_t launch_eval(const EvalArgs& a, const EvalTruth& t, EvalRec* out, int nf, hipStream_t s,
                       hipEvent_t e0, hipEvent_t e1) {
  if (e0 && e1)
    hipExtLaunchKernelGGL(k_eval<T>, dim3(nf), dim3(kEvalThreads), 0, s, e0, e1, 0, a, t, out);
  else
    hipLaunchKernelGGL(k_eval<T>, dim3(nf), dim3(kEvalThreads), 0, s, a, t, out);
  return hipGetLastError();
}
template hipError_t launch_eval<double>(const EvalArgs&, const EvalTruth&, EvalRec*, int,
                                        hipStream_t, hipEvent_t, hipEvent_t);
template hipError_t launch_eval<float>(const EvalArgs&, const EvalTruth&, EvalRec*, int,
                                       hipStream_t, hipEvent_t, hipEvent_t);

}  // namespace ekfslam
