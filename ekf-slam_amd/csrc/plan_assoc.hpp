// The scalar part of one unknown-association chunk descriptor, shared by the device planner
// (k_plan_assoc, plan_kernels.hip) and the CPU test that holds it against the host planner
// (tests/plan_assoc_host_main.cpp): what Planner::unknown (ekf_plan.cpp) leaves in a MsgDesc for
// chunk c of one message on a chunk route (kLaunchAssocChunk, predict = posterior = true), and the
// mirror Planner::export_state shows once the message has run. Plain values in, plain values out;
// nothing of HIP is needed, so the host compiler alone compiles it.
#pragma once
#include <math.h>

#include "atan2_dd.hpp"
#include "ekf_device.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EKF_PLAN_HD __host__ __device__
#else
#define EKF_PLAN_HD
#endif

namespace ekfslam {

struct AssocPlan {
  // ---- chunk c of the message (all zero when the chunk is not active) ----
  int active;      // 16·c < cnt: the chunk exists
  int m;           // its markers, min(16, cnt − 16c)
  int flags;       // kActive | kNoInit (| kJoseph) (| kFirst on c == 0) (| kLast on the last chunk)
  int parity;      // Σ / x copy it reads
  int assoc_slot;  // FilterCtl::assoc_j slot of its first marker
  // ---- marker i of the chunk (i < m, else id = 0 and z = 0 as Planner::fill leaves them) ----
  int id;          // −1: decided on the device
  double zr, zb;   // (range, bearing), slam.cpp:346-347
  // ---- the filter's mirror once this message's chunks have run ----
  int chunks;      // active chunks of this message
  int st_parity, st_prev_m, st_pending;
};

// cnt: the message's marker count (≤ 0: no message; > m_max: clamped to m_max, the markers beyond
// were never written). earlier: active chunks of the filter in the messages before this one, counted
// from the mirror (parity0, prev_m0, pending0) the replay started with. (x, y): marker 16·c + i.
EKF_PLAN_HD inline AssocPlan plan_assoc(int cnt, int m_max, int c, int i, double x, double y,
                                        int earlier, bool joseph, int parity0, int prev_m0,
                                        int pending0) {
#if defined(__clang__)
#pragma clang fp contract(off)  // x·x + y·y rounds product by product, as the host planner's does
#endif
  AssocPlan p{};
  const int n = cnt <= 0 ? 0 : (cnt < m_max ? cnt : m_max);
  p.chunks = (n + kMaxChunk - 1) / kMaxChunk;
  const int total = earlier + p.chunks;
  p.st_parity = parity0 ^ (total & 1);
  p.st_prev_m = total > 0 ? -1 : prev_m0;  // association chunks run unpipelined (Planner::forget)
  p.st_pending = total > 0 ? 0 : pending0;
  if (c < 0 || c >= p.chunks) return p;
  p.active = 1;
  p.m = n - kMaxChunk * c < kMaxChunk ? n - kMaxChunk * c : kMaxChunk;
  p.flags = kActive | kNoInit | (joseph ? kJoseph : 0) | (c == 0 ? kFirst : 0) |
            (c == p.chunks - 1 ? kLast : 0);
  p.parity = parity0 ^ ((earlier + c) & 1);
  p.assoc_slot = (kMaxChunk * c) % kMaxAssoc;
  if (i >= 0 && i < p.m) {
    p.id = -1;
    p.zr = sqrt(x * x + y * y);
#ifdef __HIP_DEVICE_COMPILE__
    p.zb = atan2_rounded(y, x);  // (ocml's atan2 is off glibc's last bit too often: atan2_dd.hpp)
#else
    p.zb = atan2(y, x);  // the host's libm, as the host planner's
#endif
  }
  return p;
}

}  // namespace ekfslam
