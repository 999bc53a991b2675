// Stand-alone driver for tests/test_plan_assoc_host.py: the descriptors the device planner of
// unknown-association replays (k_plan_assoc, ekf-slam_amd/csrc/plan_kernels.hip) assembles from
// plan_assoc (plan_assoc.hpp) against the host planner's (Planner::unknown, ekf_plan.cpp), byte for
// byte, and the mirror it leaves against Planner::export_state. No HIP, no GPU.
//
//   plan_assoc_host_main        prints one line per case and "ok", or the mismatches; exit 1 on any
//
// Per case (m_max, form): F = 3 filters, T = 70 messages, counts drawn from
// {−1, 0, 1, 15, 16, 17, 32, 33, 64, 70}, a starting mirror with parity 1, a pending predict and a
// pipelined chunk on record. The host side is ekf_replay's own sequence: load_batch on the clamped
// counts (≤ 0 → absent), then unknown(route EKF_ASSOC_CHUNK, predict = posterior = true), one call
// per message. Marker coordinates are multiples of 1/32 below 8, so x² + y² is exact however pow
// rounds; atan2 is the one libm on both sides.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ekf.h"
#include "ekf_plan.hpp"
#include "plan_assoc.hpp"

using namespace ekfslam;

namespace {

constexpr int kF = 3, kN = 40;
const int kCounts[10] = {-1, 0, 1, 15, 16, 17, 32, 33, 64, 70};

uint32_t g_rng = 12345u;
uint32_t draw() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}
double coord() {  // ±k/32, 1 ≤ k ≤ 255
  const int k = 1 + static_cast<int>(draw() % 255u);
  return (draw() & 1u ? -1.0 : 1.0) * k / 32.0;
}

int g_bad = 0;
void fail(const char* what, int m_max, int jos, int t, int c, int f, long byte) {
  if (++g_bad <= 20)
    std::printf("MISMATCH %s: m_max %d joseph %d t %d c %d f %d byte %ld\n", what, m_max, jos, t, c,
                f, byte);
}

long first_diff(const void* a, const void* b, size_t n) {
  const unsigned char* x = static_cast<const unsigned char*>(a);
  const unsigned char* y = static_cast<const unsigned char*>(b);
  for (size_t i = 0; i < n; ++i)
    if (x[i] != y[i]) return static_cast<long>(i);
  return -1;
}

// What one wave of k_plan_assoc stores for (t, c, f): every lane's plan_assoc, assembled.
MsgDesc device_desc(int cnt, int m_max, int c, const double* xy, const double* odom, int earlier,
                    bool joseph, const PlanState& s0) {
  MsgDesc d;
  std::memset(&d, 0, sizeof d);
  for (int lane = 0; lane < kMaxChunk; ++lane) {
    const int mi = kMaxChunk * c + lane;
    const bool has = mi < (cnt < m_max ? cnt : m_max);
    const AssocPlan p = plan_assoc(cnt, m_max, c, has ? lane : -1, has ? xy[2 * mi] : 0.0,
                                   has ? xy[2 * mi + 1] : 0.0, earlier, joseph, s0.parity,
                                   s0.prev_m, s0.pending);
    if (!p.active) continue;
    d.ids[lane] = p.id;
    d.z[lane][0] = p.zr;
    d.z[lane][1] = p.zb;
    if (lane < 3) d.odom[lane] = odom[lane];
    if (lane == 0) {
      d.m = p.m;
      d.flags = p.flags;
      d.parity = p.parity;
      d.assoc_slot = p.assoc_slot;
    }
  }
  return d;
}

// T messages; idle: every count ≤ 0 (the mirror is carried over).
void run_case(int m_max, bool joseph, int T, bool idle) {
  Planner P;
  P.init(kF, kN, false, true);
  P.set_joseph(joseph);
  PlanState st0[kF];
  for (int f = 0; f < kF; ++f) {
    PlanState& s = st0[f];
    s = PlanState{};
    s.parity = 1;
    s.prev_m = 3 + f;
    s.pending = 1;
    for (int i = 0; i < kMaxChunk; ++i) s.prev_ids[i] = (7 * i + f) % kN;
    s.odom[0] = 0.25 * f;
    s.odom[1] = 1.0 + f;
    s.odom[2] = -2.0 * f;
  }
  P.adopt(st0);
  const int C = (m_max + kMaxChunk - 1) / kMaxChunk;
  int earlier[kF] = {0, 0, 0};
  long compared = 0, active = 0, flags_or = 0;
  std::vector<double> last_odom(3 * kF, 0.0);
  std::vector<int> last_cnt(kF, 0);
  for (int t = 0; t < T; ++t) {
    std::vector<int> cnt(kF), clamped(kF);
    std::vector<double> rel(2 * static_cast<size_t>(kF) * m_max), odom(3 * kF);
    for (int f = 0; f < kF; ++f) {
      cnt[f] = idle ? -(static_cast<int>(draw() % 2u)) : kCounts[draw() % 10u];
      clamped[f] = cnt[f] <= 0 ? 0 : (cnt[f] < m_max ? cnt[f] : m_max);
      for (int i = 0; i < 2 * m_max; ++i) rel[2 * static_cast<size_t>(f) * m_max + i] = coord();
      odom[3 * f] = 0.01 * t + 0.1 * f;
      odom[3 * f + 1] = 0.5 * t - f;
      odom[3 * f + 2] = -0.25 * t + 2.0 * f;
    }
    // the host, as ekf_replay plans a message (load_and_plan, ekf_api.cpp)
    if (P.load_batch(1, m_max, clamped.data(), nullptr, nullptr, rel.data(), odom.data()) !=
        EKF_OK) {
      fail("load_batch", m_max, joseph, t, 0, 0, 0);
      return;
    }
    P.unknown(0, kF, true, true, 0, P.largest(kF), P.absent(), EKF_ASSOC_CHUNK);
    const std::vector<MsgDesc>& hd = P.desc();
    const int host_chunks = static_cast<int>(hd.size()) / kF;
    if (host_chunks > C && !idle) fail("host chunks", m_max, joseph, t, host_chunks, 0, 0);
    // the device, chunk by chunk of the fixed C per message
    for (int c = 0; c < C; ++c)
      for (int f = 0; f < kF; ++f) {
        const MsgDesc dd = device_desc(cnt[f], m_max, c, &rel[2 * static_cast<size_t>(f) * m_max],
                                       &odom[3 * f], earlier[f], joseph, st0[f]);
        MsgDesc zero;
        std::memset(&zero, 0, sizeof zero);
        // (a chunk launch the host never planned: every descriptor of it must be inactive)
        const MsgDesc& want = c < host_chunks ? hd[static_cast<size_t>(c) * kF + f] : zero;
        const long b = first_diff(&dd, &want, sizeof(MsgDesc));
        if (b >= 0) fail("desc", m_max, joseph, t, c, f, b);
        ++compared;
        if (dd.flags & kActive) ++active;
        flags_or |= dd.flags;
      }
    for (int f = 0; f < kF; ++f) {
      earlier[f] += plan_assoc(cnt[f], m_max, 0, -1, 0.0, 0.0, 0, joseph, 0, 0, 0).chunks;
      last_cnt[f] = cnt[f];
    }
    last_odom = odom;
    P.clear();  // (what a flush leaves)
  }
  // the mirror: what the wave of (T − 1, chunk 0) stores against export_state
  PlanState host[kF];
  P.export_state(host);
  for (int f = 0; f < kF; ++f) {
    const int before_last =
        earlier[f] - plan_assoc(last_cnt[f], m_max, 0, -1, 0.0, 0.0, 0, joseph, 0, 0, 0).chunks;
    const AssocPlan p = plan_assoc(last_cnt[f], m_max, 0, -1, 0.0, 0.0, before_last, joseph,
                                   st0[f].parity, st0[f].prev_m, st0[f].pending);
    PlanState so;
    std::memset(&so, 0, sizeof so);
    so.parity = p.st_parity;
    so.prev_m = p.st_prev_m;
    so.pending = p.st_pending;
    for (int i = 0; i < kMaxChunk; ++i) so.prev_ids[i] = st0[f].prev_ids[i];
    for (int i = 0; i < 3; ++i) so.odom[i] = last_odom[3 * f + i];
    const long b = first_diff(&so, &host[f], sizeof(PlanState));
    if (b >= 0) fail("mirror", m_max, joseph, T - 1, 0, f, b);
  }
  std::printf("case m_max %d joseph %d T %d idle %d: compared %ld active %ld flags %ld\n", m_max,
              joseph ? 1 : 0, T, idle ? 1 : 0, compared, active, flags_or);
}

// The bearing the device computes (atan2_rounded, atan2_dd.hpp: double-double, rounded once; on the
// host plan_assoc takes libm's atan2 as the host planner does) against libm's on 20 000 points of
// all four quadrants. A correctly rounded value and glibc's (< 0.55 ulp off the true one, so equal
// to it but for about one argument in a thousand) can differ by one ulp at most, and seldom: the
// two must be within 1 ulp everywhere and equal on 99.5 % of the points.
void check_bearings() {
  const int n = 20000;
  int equal = 0, far = 0;
  for (int i = 0; i < n; ++i) {
    const double x = coord() + (draw() % 4096u) / 1048576.0 * (i % 3 == 0 ? 1e-6 : 1.0);
    const double y = coord() * (i % 5 == 0 ? 1e-7 : 1.0) + (draw() % 4096u) / 2097152.0;
    const double a = atan2_rounded(y, x), b = std::atan2(y, x);
    if (a == b) ++equal;
    else if (a != std::nextafter(b, a)) ++far;
  }
  std::printf("bearings %d equal %d beyond-1ulp %d\n", n, equal, far);
  if (far || equal < n - n / 200) ++g_bad;
}

}  // namespace

int main() {
  check_bearings();
  const int sizes[3] = {16, 17, 64};
  for (int s = 0; s < 3; ++s)
    for (int jos = 0; jos < 2; ++jos) {
      run_case(sizes[s], jos != 0, 70, false);
      run_case(sizes[s], jos != 0, 3, true);
    }
  if (g_bad) {
    std::printf("%d mismatches\n", g_bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
