// Stand-alone driver of the host planner (ekf-slam_amd/csrc/ekf_plan.cpp) for
// tests/test_plan_host.py: replays a fixed script of planner calls and writes, per section, the
// MsgDesc bytes, the launch list, the two per-launch queries of the scheduler, the return codes of
// the message input and the final mirror. No HIP, no GPU.
//
//   plan_host_main <out file>
//
// The script talks to the planner through `Api` only. PLAN_API_HEADER (a file name) replaces the
// Api below by another one with the same members: that is how the fixtures under
// tests/golden/plan/ were recorded from the runtime before the planner was split out of it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#ifdef PLAN_API_HEADER
#include PLAN_API_HEADER
#else
#include "ekf.h"
#include "ekf_plan.hpp"

using namespace ekfslam;

struct Api {
  Planner p;
  void create(int F, int N, bool resident, bool staging) {
    p = Planner();
    p.init(F, N, resident, staging);
  }
  int set_message(int m, const int* ids, const int* actions, const double* rel) {
    return p.set_message(m, ids, actions, rel);
  }
  int load_batch(int assoc_mode, int m_max, const int* counts, const int* ids, const int* actions,
                 const double* rel, const double* odom) {
    return p.load_batch(assoc_mode, m_max, counts, ids, actions, rel, odom);
  }
  int largest(int nf) { return p.largest(nf); }
  void set_odom(int f, double th, double x, double y) { p.set_odom(f, th, x, y); }
  void known(int f0, int nf, bool predict, bool use_absent) {
    p.known(f0, nf, predict, use_absent ? p.absent() : nullptr);
  }
  void unknown(int f0, int nf, bool predict, bool posterior, int i0, int i1, bool use_absent,
               int route) {
    p.unknown(f0, nf, predict, posterior, i0, i1, use_absent ? p.absent() : nullptr, route);
  }
  void posterior(int f) { p.posterior(f); }
  void forget(int f) { p.forget(f); }
  void reset(int f) { p.reset(f); }
  void set_pending(int f, bool on) { p.set_pending(f, on); }
  void set_joseph(bool on) { p.set_joseph(on); }
  void export_state(PlanState* st) { p.export_state(st); }
  void adopt(const PlanState* st) { p.adopt(st); }
  void take(const int* parity_after, const double* odom_after) { p.take(parity_after, odom_after); }
  void clear() { p.clear(); }  // what a flush leaves

  size_t n_desc() { return p.desc().size(); }
  const MsgDesc* desc() { return p.desc().data(); }
  size_t n_launch() { return p.launches().size(); }
  // kind, off, f0, nf, kw, "some active filter has no kLook", "some active filter stages"
  void launch(size_t i, int32_t out[7]) {
    const Launch& L = p.launches()[i];
    const int32_t v[7] = {L.kind, static_cast<int32_t>(L.off), L.f0, L.nf, L.kw, L.nolook, L.stage};
    std::memcpy(out, v, sizeof v);
  }
  // parity, pending, prev_m, prev_ids[kMaxChunk]
  void mirror(int f, int32_t out[3 + kMaxChunk]) {
    out[0] = p.parity(f);
    out[1] = p.pending(f);
    out[2] = p.prev_m(f);
    for (int i = 0; i < kMaxChunk; ++i) out[3 + i] = p.prev_ids(f)[i];
  }
};
#endif

namespace {

constexpr int kN = 40;  // landmarks of every case
FILE* g_out = nullptr;
Api A;
int g_F = 0;
std::vector<int32_t> g_rc;

void put(const void* p, size_t n) {
  if (n && std::fwrite(p, 1, n, g_out) != n) std::exit(3);
}

// One section: name[48], {F, descriptors, launches, rcs}, MsgDesc bytes, launches [7], rcs,
// mirror [F][3 + kMaxChunk]. A section ends where a flush would: the plan is cleared.
void section(const std::string& name) {
  char nm[48] = {0};
  std::snprintf(nm, sizeof nm, "%s", name.c_str());
  put(nm, sizeof nm);
  const int32_t hdr[4] = {g_F, static_cast<int32_t>(A.n_desc()), static_cast<int32_t>(A.n_launch()),
                          static_cast<int32_t>(g_rc.size())};
  put(hdr, sizeof hdr);
  put(A.desc(), A.n_desc() * sizeof(MsgDesc));
  for (size_t i = 0; i < A.n_launch(); ++i) {
    int32_t l[7];
    A.launch(i, l);
    put(l, sizeof l);
  }
  put(g_rc.data(), g_rc.size() * sizeof(int32_t));
  for (int f = 0; f < g_F; ++f) {
    int32_t m[3 + kMaxChunk];
    A.mirror(f, m);
    put(m, sizeof m);
  }
  g_rc.clear();
  A.clear();
}

void create(int F, bool resident, bool staging) {
  g_F = F;
  A.create(F, kN, resident, staging);
}

// Marker i of a message: on an axis, so that range and bearing (sqrt, pow, atan2 of the host's
// libm) are exact on every machine; the range k tells the markers apart.
void rel_of(int i, int seed, double* r) {
  const double k = 1.0 + i + 0.25 * seed;
  const double ax[4][2] = {{k, 0.0}, {0.0, k}, {-k, 0.0}, {0.0, -k}};
  r[0] = ax[(i + seed) % 4][0];
  r[1] = ax[(i + seed) % 4][1];
}

struct Msg {
  std::vector<int> ids, actions;
  std::vector<double> rel;
};
// m markers, ids (3i + seed) mod N; del: every del-th marker is a DELETE (1: all of them)
Msg msg(int m, int seed, int del = 0) {
  Msg s;
  for (int i = 0; i < m; ++i) {
    s.ids.push_back((3 * i + seed) % kN);
    s.actions.push_back(del && i % del == 0 ? EKF_MARKER_DELETE : 0);
    double r[2];
    rel_of(i, seed, r);
    s.rel.push_back(r[0]);
    s.rel.push_back(r[1]);
  }
  return s;
}

void one_known(int f, int m, int seed, bool predict = true, int del = 0) {
  const Msg s = msg(m, seed, del);
  g_rc.push_back(A.set_message(m, s.ids.data(), s.actions.data(), s.rel.data()));
  A.known(f, 1, predict, false);
}
void one_unknown_msg(int m, int seed) {
  const Msg s = msg(m, seed);
  g_rc.push_back(A.set_message(m, nullptr, nullptr, s.rel.data()));
}

// One step of a batch: counts[f] markers for filter f (0: absent). Returns load_batch's status.
int batch(int assoc_mode, const std::vector<int>& counts, int seed, int del = 0, int bad_f = -1,
          int m_max_override = -1) {
  int m_max = 1;
  for (int c : counts) m_max = c > m_max ? c : m_max;
  if (m_max_override >= 0) m_max = m_max_override;
  const size_t F = counts.size();
  std::vector<int> ids(F * m_max, 0), actions(F * m_max, 0);
  std::vector<double> rel(2 * F * m_max, 0.0), odom(3 * F);
  for (size_t f = 0; f < F; ++f) {
    const Msg s = msg(counts[f] <= m_max ? counts[f] : m_max, seed + 5 * static_cast<int>(f), del);
    for (size_t i = 0; i < s.ids.size(); ++i) {
      ids[f * m_max + i] = s.ids[i];
      actions[f * m_max + i] = s.actions[i];
      rel[2 * (f * m_max + i)] = s.rel[2 * i];
      rel[2 * (f * m_max + i) + 1] = s.rel[2 * i + 1];
    }
    odom[3 * f] = 0.125 * seed;
    odom[3 * f + 1] = 1.5 + static_cast<double>(f);
    odom[3 * f + 2] = -0.5 * seed;
  }
  if (bad_f >= 0) ids[bad_f * m_max] = kN;  // out of range (filters before it are valid)
  const int rc = A.load_batch(assoc_mode, m_max, counts.data(), ids.data(), actions.data(),
                              rel.data(), odom.data());
  g_rc.push_back(rc);
  return rc;
}
void known_step(const std::vector<int>& counts, int seed, int del = 0) {
  if (batch(0, counts, seed, del) == EKF_OK) A.known(0, g_F, true, true);
}
void unknown_step(const std::vector<int>& counts, int seed, int route) {
  if (batch(1, counts, seed) == EKF_OK)
    A.unknown(0, g_F, true, true, 0, A.largest(g_F), true, route);
}

// ---- the cases ----

// message sizes at the chunk edges, five consecutive messages in one plan: kLook from the second
// chunk on, kStageOut set two chunks back with kStageIn following, then a plan after a flush
void known_sizes(const char* name, bool resident, bool staging, bool joseph) {
  create(1, resident, staging);
  if (joseph) A.set_joseph(true);
  one_known(0, 3, 1, true, 1);  // every marker a DELETE: m = 0
  const int sizes[4] = {1, 16, 17, 33};
  for (int i = 0; i < 4; ++i) one_known(0, sizes[i], 2 + i);
  section(std::string(name) + ".a");
  one_known(0, 5, 9);  // after a flush: kLook (events) but nothing staged for it
  one_known(0, 2, 10);
  one_known(0, 4, 11, true, 2);
  section(std::string(name) + ".b");
}

// three filters of unequal length, one absent at a time, DELETE markers, five steps
void known_batch(const char* name, bool resident, bool staging, bool joseph) {
  create(3, resident, staging);
  if (joseph) A.set_joseph(true);
  known_step({20, 5, 0}, 1);
  known_step({17, 0, 3}, 2, 3);
  known_step({1, 33, 16}, 3);
  known_step({0, 2, 2}, 4);
  known_step({6, 6, 6}, 5, 2);
  section(std::string(name) + ".a");
  known_step({3, 0, 18}, 6);
  section(std::string(name) + ".b");
}

// a Joseph switch between messages forgets the previous chunks (no kLook across it)
void joseph_switch() {
  create(2, false, true);
  known_step({17, 4}, 1);
  known_step({3, 16}, 2);
  section("joseph_switch.a");
  A.set_joseph(true);
  known_step({17, 4}, 3);
  known_step({16, 1}, 4);
  known_step({2, 2}, 5);
  section("joseph_switch.b");
  A.set_joseph(false);
  known_step({5, 5}, 6);
  section("joseph_switch.c");
}

// ekf_predict, ekf_correct, ekf_posterior: predict = false with and without a pending predict
void pending_and_posterior() {
  create(2, false, true);
  A.set_odom(1, 0.5, 1.25, -2.0);
  A.set_pending(1, true);
  one_known(1, 1, 3, false);  // kFirst from the pending predict, no kLast
  one_known(1, 1, 4, false);  // neither
  A.posterior(1);             // posterior alone
  A.set_pending(1, true);
  g_rc.push_back(A.set_message(0, nullptr, nullptr, nullptr));
  A.known(1, 1, true, false);  // ekf_posterior with a pending predict: a zero-marker pass
  one_known(0, 4, 5);
  A.set_pending(0, true);
  section("pending_and_posterior");
}

// forget / reset in the middle of a plan; rejected batches change nothing
void state_changes() {
  create(3, false, true);
  known_step({4, 4, 4}, 1);
  known_step({4, 4, 4}, 2);
  A.forget(1);
  A.reset(0);
  known_step({4, 4, 4}, 3);
  known_step({4, 4, 4}, 4);
  batch(0, {2, 2, 2}, 5, 0, 2);   // EKF_E_RANGE at the last filter
  batch(0, {2, 9, 2}, 6, 0, -1, 4);  // EKF_E_ARG: a count above m_max
  A.known(0, 3, true, true);      // plans step 4's messages again
  section("state_changes");
}

// unknown association of one filter, asynchronous (one window over the whole message) and in the
// synchronous form's windows of kMaxAssoc markers, each window its own plan
void unknown_sizes(const char* name, int route, bool resident, bool joseph) {
  const int sizes[7] = {0, 1, 16, 17, 64, 65, 130};
  create(2, resident, true);
  if (joseph) A.set_joseph(true);
  one_known(1, 3, 1);  // a pipelined chunk before: association forgets it
  for (int i = 0; i < 7; ++i) {
    one_unknown_msg(sizes[i], 1 + i);
    A.unknown(1, 1, true, true, 0, A.largest(1), false, route);
  }
  section(std::string(name) + ".async");
  A.set_pending(1, true);
  for (int i = 0; i < 7; ++i) {
    one_unknown_msg(sizes[i], 8 + i);
    const int mm = A.largest(1);
    for (int i0 = 0; i0 < mm; i0 += 64) {
      const int i1 = mm < i0 + 64 ? mm : i0 + 64;
      A.unknown(1, 1, i % 2 == 0, i1 == mm && i != 3, i0, i1, false, route);
      section(std::string(name) + ".sync" + std::to_string(sizes[i]) + "." + std::to_string(i0));
    }
  }
}

void unknown_batch(const char* name, int route, bool joseph) {
  create(3, false, true);
  if (joseph) A.set_joseph(true);
  known_step({2, 2, 2}, 1);
  unknown_step({33, 17, 0}, 2, route);
  unknown_step({0, 1, 16}, 3, route);
  unknown_step({65, 0, 64}, 4, route);
  known_step({2, 2, 2}, 5);
  section(name);
}

// the mirror to a device planner and back, then what a device-written plan leaves
void plan_state() {
  create(3, false, true);
  known_step({4, 16, 0}, 1);
  known_step({2, 0, 7}, 2);
  A.set_pending(2, true);
  PlanState st[3];
  A.export_state(st);
  section("plan_state.before");
  char nm[48] = "plan_state.export";
  put(nm, sizeof nm);
  const int32_t hdr[4] = {0, 0, 0, static_cast<int32_t>(sizeof st / (sizeof(int32_t)))};
  put(hdr, sizeof hdr);
  put(st, sizeof st);
  create(3, false, true);
  st[1].parity ^= 1;
  st[1].prev_m = 5;
  A.adopt(st);
  known_step({3, 3, 3}, 3);
  known_step({3, 3, 3}, 4);
  known_step({3, 3, 3}, 5);
  section("plan_state.adopted");
  const int parity_after[3] = {1, 0, 1};
  const double odom_after[9] = {0.25, 1.0, 2.0, -0.5, 3.0, 4.0, 0.75, 5.0, 6.0};
  A.set_pending(0, true);
  A.take(parity_after, odom_after);
  A.known(0, 3, true, false);  // step 5's messages, the new parity and odometry, no kLook
  section("plan_state.taken");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  g_out = std::fopen(argv[1], "wb");
  if (!g_out) return 2;
  known_sizes("known_sizes", false, true, false);
  known_sizes("known_sizes_nostage", false, false, false);
  known_sizes("known_sizes_resident", true, false, true);  // (no Joseph chunks, no kLook)
  known_sizes("known_sizes_joseph", false, true, true);
  known_batch("known_batch", false, true, false);
  known_batch("known_batch_nostage", false, false, false);
  known_batch("known_batch_resident", true, false, false);
  joseph_switch();
  pending_and_posterior();
  state_changes();
  unknown_sizes("unknown_marker", EKF_ASSOC_MARKER, false, false);
  unknown_sizes("unknown_marker_resident", EKF_ASSOC_MARKER, true, true);
  unknown_sizes("unknown_chunk", EKF_ASSOC_CHUNK, false, false);
  unknown_sizes("unknown_chunk_joseph", EKF_ASSOC_CHUNK_XCD, false, true);
  unknown_batch("unknown_batch_marker", EKF_ASSOC_MARKER, true);
  unknown_batch("unknown_batch_chunk", EKF_ASSOC_CHUNK, false);
  plan_state();
  return std::fclose(g_out) == 0 ? 0 : 3;
}
