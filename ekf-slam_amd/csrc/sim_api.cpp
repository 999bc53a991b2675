// Host side of include/ekf_sim.h: device buffers of the simulator, one run = one simulator launch
// (which also writes the filter's descriptors) + the filter's launches over the run's messages.
// The simulator runs on a stream of its own with double-buffered run buffers, so run r's
// simulation overlaps run r−1's filter work; the host waits only for the simulation (it needs
// each filter's final parity for the handle's host mirror).
// A run without SURVEY messages on the HBM pipeline takes the parallel form instead: the wheels per
// filter, then every (message, filter) sensed at once into marker arrays, which ekf_replay_device
// plans on the GPU — no host round trip at all (EKF_SIM_PARALLEL=0 keeps the sequential kernel).
// ekf_sim_run_assoc always simulates in the parallel form and hands the marker arrays, ids ignored,
// to the device-input association replay of the handle's path.
// ekf_sim_run_lidar simulates likewise, then has a landmark front-end handle scan the truth poses
// with the laser kernel and detect on the scans (lm_api.cpp's hook), and replays those markers.
// Collisions (ekf_sim_set_collisions) swap the wheel walk's kernel of either form for its collision
// variant and nothing else; the per-message counts go into a buffer pair of their own, allocated by
// the first run with collisions on, so a simulator that never turns them on allocates, launches and
// frees exactly what it did before.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ekf.h"
#include "ekf_device.hpp"
#include "ekf_internal.hpp"
#include "ekf_launch.hpp"
#include "ekf_sim.h"
#include "hip_owned.hpp"
#include "sim_launch.hpp"

using namespace ekfslam;

struct ekf_sim {
  ekf_t h = nullptr;
  ekf_sim_config cfg{};
  HandleInfo info{};
  int L = 0, m = 0;
  long long tick = 0, msg = 0;  // global tick / message index of the next run
  // (members are destroyed in reverse order: the simulator's stream outlives what is used on it)
  Stream sst;                             // the simulator's stream
  DeviceBuf<double> lm;
  DeviceBuf<unsigned> sighted;
  DeviceBuf<SimState> st;
  DeviceBuf<int> par;
  Event ev_sim{hipEventDisableTiming};    // simulation of the current run done
  // filter work of the run that used buffer b done
  Event ev_done[2] = {Event{hipEventDisableTiming}, Event{hipEventDisableTiming}};
  PinnedBuf<int> host_par_pinned;
  PinnedBuf<SimState> host_st_pinned;  // [F] poses after the last run (the handle's t_odom_robot)
  int buf = 0;                      // run buffer of the next run
  // markers and poses of a run by run buffer: the record (cfg.record) and the parallel form's
  // hand-over to ekf_replay_device
  struct Markers {
    DeviceBuf<int> ids;       // [T][F][M]
    DeviceBuf<int> act;       // [T][F][M]
    DeviceBuf<double> rel;    // [T][F][M][2]
    DeviceBuf<int> cnt;       // [T][F]
    DeviceBuf<double> truth;  // [T][F][3]
    DeviceBuf<double> odom;   // [T][3] (filter 0's)
    DeviceBuf<double> odomF;  // [T][F][3] (the planner's input)
  };
  // What reserve() sizes for a run, all or nothing. `run = Run{}` frees member by member in this
  // order, which is the order the buffers have always been freed in before a regrowth.
  struct Run {
    struct {
      DeviceBuf<double> cmd;
      DeviceBuf<int> sense;
      DeviceBuf<MsgDesc> desc;
    } in[2];  // by run buffer
    DeviceBuf<PlanEntry> plan;
    Markers mk[2];
  } run;
  // what `run` holds, recorded once all of it (the plan's upload included) is there
  size_t cap_ticks = 0, cap_msgs = 0;
  int mk_bufs = 0;                  // marker buffers allocated
  bool assoc = false;  // ekf_sim_run_assoc has been called: both marker buffers, always
  int last_T = 0, last_b = 0;
  std::vector<int> host_par;
  std::vector<double> host_odom;    // [F][3] t_odom_robot after the last run
  // collisions (ekf_sim_set_collisions): R = collision_radius + obstacle_radius, 0: off
  double hit_r = 0.0;
  DeviceBuf<int> hits[2];           // [T][F] colliding ticks per message, by marker buffer
  bool last_hits = false;           // the last run wrote hits[last_b]
  // maps of fewer landmarks are staged whole (kCollideCullFromMap; EKF_SIM_CULL_FROM at
  // ekf_sim_create overrides it for tools/sim_collide_bench.py and the tests: same bits)
  int cull_from = kCollideCullFromMap;
  // EKF_SIM_TIMING=1 at ekf_sim_create: timing events around each run's simulator launches
  // (ekf_sim_last_us; tools/sim_collide_bench.py). Unset, nothing is created or recorded.
  bool timing = false, timed = false;
  Event ev_t0, ev_t1;
};

namespace {

// The parallel form (no SURVEY message, HBM pipeline, M ≤ kMaxChunk; EKF_SIM_PARALLEL=0: never).
bool parallel_ok(const ekf_sim* s, int T, const int* sense) {
  const char* e = std::getenv("EKF_SIM_PARALLEL");
  if ((e && std::atoi(e) == 0) || s->info.resident || s->cfg.marker_stride > kMaxChunk) return false;
  for (int t = 0; sense && t < T; ++t)
    if (sense[t] == EKF_SENSE_SURVEY) return false;
  return true;
}

// run buffers for T messages (grown, never shrunk)
int reserve(ekf_sim* s, int T) {
  const size_t F = static_cast<size_t>(s->info.F), M = static_cast<size_t>(s->cfg.marker_stride);
  const size_t ticks = static_cast<size_t>(T) * s->cfg.ticks_per_msg;
  // markers: both buffers for the parallel form (one run's planner reads them while the next run's
  // simulation writes the other) and, at any stride and on either path, once ekf_sim_run_assoc has
  // been called (its replays read them); buffer 0 only for a record of the sequential form
  const bool par = !s->info.resident && s->cfg.marker_stride <= kMaxChunk;
  const int bufs = par || s->assoc ? 2 : s->cfg.record ? 1 : 0;
  if (static_cast<size_t>(T) <= s->cap_msgs && ticks <= s->cap_ticks && bufs <= s->mk_bufs)
    return EKF_OK;
  // (the bulk stream too: an association replay of ekf_sim_run_assoc may still read the buffers)
  if (hipStreamSynchronize(s->info.stream) != hipSuccess ||
      hipStreamSynchronize(s->info.bulk) != hipSuccess ||
      hipStreamSynchronize(s->sst.get()) != hipSuccess)
    return EKF_E_HIP;
  const size_t Tn = std::max<size_t>({static_cast<size_t>(T), s->cap_msgs, 1});
  const size_t tk = Tn * s->cfg.ticks_per_msg;
  ekf_sim::Run& r = s->run;
  // every buffer is freed before the first is allocated (bench.py's swarm workloads regrow inside
  // their timed region: the order of the frees and allocations is part of what they measure)
  r = ekf_sim::Run{};
  s->cap_ticks = s->cap_msgs = 0;
  s->mk_bufs = 0;
  bool ok = !r.plan.reserve(Tn);
  for (int b = 0; b < 2 && ok; ++b) {
    auto& in = r.in[b];
    ok = !(in.cmd.reserve(tk * 2) || in.sense.reserve(Tn) || in.desc.reserve(Tn * F));
  }
  for (int b = 0; b < bufs && ok; ++b) {
    auto& k = r.mk[b];
    ok = !(k.ids.reserve(Tn * F * M) || k.act.reserve(Tn * F * M) ||
           k.rel.reserve(Tn * F * M * 2) || k.cnt.reserve(Tn * F) || k.truth.reserve(Tn * F * 3) ||
           k.odom.reserve(Tn * 3) || k.odomF.reserve(Tn * F * 3));
  }
  int rc = ok ? EKF_OK : EKF_E_NOMEM;
  if (ok) {  // the resident plan: one entry per message, every filter (off = t·F)
    std::vector<PlanEntry> pe(Tn);
    for (size_t t = 0; t < Tn; ++t)
      pe[t] = PlanEntry{static_cast<int>(t * F), 0, static_cast<int>(F), 0};
    if (hipMemcpy(r.plan.get(), pe.data(), Tn * sizeof(PlanEntry), hipMemcpyHostToDevice) !=
        hipSuccess)
      rc = EKF_E_HIP;
  }
  if (rc) {  // all or nothing: no capacity is recorded for buffers whose plan never arrived
    r = ekf_sim::Run{};
    return rc;
  }
  s->cap_msgs = Tn;
  s->cap_ticks = tk;
  s->mk_bufs = bufs;
  return EKF_OK;
}

// The per-message collision counts of a run of T messages (with collisions on and a record kept
// only; grown, never shrunk). The kernels that wrote the old blocks are waited for before a
// regrowth frees them.
int reserve_hits(ekf_sim* s, int T) {
  if (!(s->hit_r > 0.0) || !s->cfg.record) return EKF_OK;
  const size_t n = static_cast<size_t>(T) * s->info.F;
  if (n <= s->hits[0].capacity() && n <= s->hits[1].capacity()) return EKF_OK;
  if (hipStreamSynchronize(s->sst.get()) != hipSuccess) return EKF_E_HIP;
  if (s->hits[0].reserve(n) || s->hits[1].reserve(n)) return reset_all(s->hits[0], s->hits[1]);
  return EKF_OK;
}

// the collision settings of a launch; `record`: the per-message counts are kept (buffer b)
bool set_collide(ekf_sim* s, SimArgs& a, bool record, int b) {
  const bool on = s->hit_r > 0.0;
  a.hit_r = s->hit_r;
  a.out_hits = on && record ? s->hits[b].get() : nullptr;
  a.cull_from = s->cull_from;
  s->last_hits = on && record;
  return on;
}

// the timing events around a run's simulator launches (EKF_SIM_TIMING)
bool stamp(ekf_sim* s, Event& e) {
  return !s->timing || hipEventRecord(e.get(), s->sst.get()) == hipSuccess;
}

// The simulation of the parallel form into run buffer b, on the simulator's stream; the handle's
// streams wait for it. Advances the tick and message counters.
int simulate_parallel(ekf_sim* s, int T, const double* wheel_cmd, const int* sense, int b) {
  const hipStream_t st = s->sst.get();
  const size_t ticks = static_cast<size_t>(T) * s->cfg.ticks_per_msg;
  auto& k = s->run.mk[b];
  // buffer b (commands, senses, markers) was last read by the run before the previous one
  if (hipStreamWaitEvent(st, s->ev_done[b].get(), 0) != hipSuccess ||
      hipMemcpyAsync(s->run.in[b].cmd.get(), wheel_cmd, ticks * 2 * sizeof(double),
                     hipMemcpyHostToDevice, st) != hipSuccess ||
      (sense && hipMemcpyAsync(s->run.in[b].sense.get(), sense, T * sizeof(int),
                               hipMemcpyHostToDevice, st) != hipSuccess))
    return EKF_E_HIP;
  SimArgs a{};
  a.cmd = s->run.in[b].cmd.get();
  a.sense = sense ? s->run.in[b].sense.get() : nullptr;
  a.lm = s->lm.get();
  a.st = s->st.get();
  a.out_ids = k.ids.get();
  a.out_act = k.act.get();
  a.out_rel = k.rel.get();
  a.out_cnt = k.cnt.get();
  a.out_truth = k.truth.get();
  a.out_odom = s->cfg.record ? k.odom.get() : nullptr;
  a.seed = s->cfg.seed;
  a.tick0 = s->tick;
  a.msg0 = s->msg;
  a.f0 = s->cfg.f0;
  a.F = s->info.F;
  a.L = s->L;
  a.T = T;
  a.tpm = s->cfg.ticks_per_msg;
  a.m = s->m;
  a.M = s->cfg.marker_stride;
  a.N = s->info.N;
  a.slip = s->cfg.slip;
  a.sigma = s->cfg.sensor_sigma;
  a.range = s->cfg.max_range;
  a.radius = s->cfg.wheel_radius;
  a.track = s->cfg.track_width;
  const bool collide = set_collide(s, a, s->cfg.record != 0, b);
  if (!stamp(s, s->ev_t0) ||
      launch_sim_parallel(a, collide, k.truth.get(), k.odomF.get(), st) != hipSuccess ||
      !stamp(s, s->ev_t1) ||
      hipEventRecord(s->ev_sim.get(), st) != hipSuccess ||
      hipStreamWaitEvent(s->info.stream, s->ev_sim.get(), 0) != hipSuccess ||
      hipStreamWaitEvent(s->info.bulk, s->ev_sim.get(), 0) != hipSuccess)
    return EKF_E_HIP;
  s->tick += static_cast<long long>(ticks);
  s->msg += T;
  s->last_T = T;
  s->last_b = b;
  s->timed = s->timing;
  return EKF_OK;
}

// The parallel form of ekf_sim_run (parallel_ok): simulation on the simulator's stream, then
// ekf_replay_device over its marker arrays behind it on the handle's streams. The planning state
// stays on the device (the handle adopts it at its next host access), so the host never waits.
int run_parallel(ekf_sim* s, int T, const double* wheel_cmd, const int* sense) {
  const int b = s->buf;
  s->buf ^= 1;
  if (int rc = simulate_parallel(s, T, wheel_cmd, sense, b)) return rc;
  const auto& k = s->run.mk[b];
  const int rc = ekf_replay_device(s->h, T, s->cfg.marker_stride, k.cnt.get(), k.ids.get(),
                                   k.act.get(), k.rel.get(), k.odomF.get());
  if (rc) return rc;
  // the chain launch on the main stream polls the planner (or follows it): done there ⇒ read
  return hipEventRecord(s->ev_done[b].get(), s->info.stream) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

// ekf_sim_run_assoc: the same simulation, handed over with the ids ignored. Which stream reads the
// buffers (ekf_sched.cpp): replay_device_assoc puts its planner k_plan_assoc, the only reader, and
// every association launch behind it on the main stream of a serial handle and on the bulk stream
// otherwise (`ps`); replay_resident launches k_resident_replay, which reads them throughout, on the
// main stream, the only one a resident handle uses. ev_done[b] is recorded on that stream behind
// the replay's last launch, so the run after next rewrites buffer b only once all of it has ended.
int run_assoc(ekf_sim* s, int T, const double* wheel_cmd) {
  const int b = s->buf;
  s->buf ^= 1;
  if (int rc = simulate_parallel(s, T, wheel_cmd, nullptr, b)) return rc;
  const auto& k = s->run.mk[b];
  const int M = s->cfg.marker_stride;
  const int rc = s->info.resident
                     ? ekf_replay_resident(s->h, 1, T, M, k.cnt.get(), nullptr, nullptr,
                                           k.rel.get(), 2, k.odomF.get())
                     : ekf_replay_device_assoc(s->h, T, M, k.cnt.get(), k.rel.get(), 2,
                                               k.odomF.get());
  if (rc) return rc;
  const hipStream_t rs = s->info.resident || s->info.serial ? s->info.stream : s->info.bulk;
  return hipEventRecord(s->ev_done[b].get(), rs) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

static_assert(kSimMaxMap <= LM_MAX_CIRCLES, "a simulator map is one LDS-resident laser scene");

// ekf_sim_run_lidar: the same simulation; then on the front-end's stream, behind ev_sim, the laser
// over the truth buffer and the maps and the detect over its scans; then the association replay of
// the handle's path over the front-end's markers and this run's odometry buffer, behind the
// detect's event. The replay's stream (as run_assoc's) reads the odometry; the laser's read of the
// truth buffer is ahead of it in that chain (scan → detect → e_det → replay), so ev_done[b] on the
// replay's stream covers both.
int run_lidar(ekf_sim* s, lm_t lm, int T, const double* wheel_cmd,
              const ekf_sim_lidar_config* cfg) {
  const int b = s->buf;
  s->buf ^= 1;
  const long long msg0 = s->msg;
  if (int rc = simulate_parallel(s, T, wheel_cmd, nullptr, b)) return rc;
  const auto& k = s->run.mk[b];
  LidarRun run{};
  run.d_truth = k.truth.get();
  run.d_lm = s->lm.get();
  run.T = T;
  run.F = s->info.F;
  run.L = s->L;
  run.n_beams = cfg->n_beams;
  run.max_markers = cfg->max_markers;
  run.seed = cfg->scan.seed + static_cast<unsigned long long>(s->cfg.f0);
  run.msg0 = msg0;
  run.radius = cfg->obstacle_radius;
  run.threshold = cfg->threshold;
  run.scan = &cfg->scan;
  LidarFeed feed{};
  if (int rc = lm_lidar_enqueue(lm, run, s->ev_sim.get(), &feed)) return rc;
  const int dev = s->info.device, M = cfg->max_markers;
  const int rc =
      s->info.resident
          ? replay_markers_resident_device(s->h, dev, T, M, feed.d_counts, feed.d_markers,
                                           k.odomF.get(), feed.ready, feed.planned)
          : replay_markers_device(s->h, dev, T, M, feed.d_counts, feed.d_markers, k.odomF.get(),
                                  feed.ready, feed.planned);
  // (an argument error comes back before anything is enqueued; past that the planner may be)
  if (rc != EKF_E_ARG) lm_lidar_planned(lm);
  if (rc) return rc;
  const hipStream_t rs = s->info.resident || s->info.serial ? s->info.stream : s->info.bulk;
  return hipEventRecord(s->ev_done[b].get(), rs) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

}  // namespace

extern "C" {

void ekf_sim_config_default(ekf_sim_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->seed = 20240317ull;
  c->ticks_per_msg = 40;
  c->slip = 0.02;
  c->sensor_sigma = 1e-3;
  c->max_range = 5.0;
  c->max_markers = 16;
  c->marker_stride = 16;
  c->wheel_radius = 0.033;
  c->track_width = 0.160;
  c->start_theta = -1.0;
}

int ekf_sim_create(ekf_sim_t* out, ekf_t filter, const ekf_sim_config* cfg, int n_map,
                   const double* landmarks) {
  if (!out || !filter || !cfg || n_map <= 0 || n_map > kSimMaxMap || !landmarks) return EKF_E_ARG;
  *out = nullptr;
  ekf_sim* s = new ekf_sim;
  s->h = filter;
  s->cfg = *cfg;
  if (int rc = handle_info(filter, &s->info)) {
    delete s;
    return rc;
  }
  s->L = n_map;
  s->m = std::min(cfg->max_markers, n_map);
  if (n_map > s->info.N || cfg->ticks_per_msg <= 0 || s->m <= 0 || s->m > kMaxChunk ||
      cfg->marker_stride < s->m || cfg->wheel_radius <= 0.0 || cfg->track_width <= 0.0 ||
      cfg->ticks_per_msg > 64) {
    delete s;
    return EKF_E_ARG;
  }
  const size_t F = static_cast<size_t>(s->info.F), words = (n_map + 31) / 32;
  hipSetDevice(s->info.device);
  auto fail = [&](int rc) {
    ekf_sim_destroy(s);
    return rc;
  };
  if (s->lm.reserve(F * n_map * 2) || s->sighted.reserve(F * words) || s->st.reserve(F) ||
      s->par.reserve(F) || s->host_par_pinned.reserve(F) || s->host_st_pinned.reserve(F))
    return fail(EKF_E_NOMEM);
  std::vector<SimState> st(F);
  for (auto& v : st) {
    std::memset(&v, 0, sizeof(v));
    v.truth[0] = cfg->start_theta;
    v.truth[1] = cfg->start_x;
    v.truth[2] = cfg->start_y;
  }
  if (s->sst.create(hipStreamNonBlocking) || s->ev_sim.create() || s->ev_done[0].create() ||
      s->ev_done[1].create() ||
      hipEventRecord(s->ev_done[0].get(), s->info.stream) != hipSuccess ||
      hipEventRecord(s->ev_done[1].get(), s->info.stream) != hipSuccess ||
      hipMemcpy(s->lm.get(), landmarks, F * n_map * 2 * sizeof(double), hipMemcpyHostToDevice) !=
          hipSuccess ||
      hipMemset(s->sighted.get(), 0, F * words * sizeof(unsigned)) != hipSuccess ||
      hipMemcpy(s->st.get(), st.data(), F * sizeof(SimState), hipMemcpyHostToDevice) != hipSuccess)
    return fail(EKF_E_HIP);
  if (const char* from = std::getenv("EKF_SIM_CULL_FROM")) {  // (digits only: anything else is
    char* end = nullptr;                                        // ignored, not read as 0)
    const long v = std::strtol(from, &end, 10);
    if (end != from && *end == '\0' && v >= 0) s->cull_from = static_cast<int>(std::min(v, 1L << 20));
  }
  const char* tm = std::getenv("EKF_SIM_TIMING");
  if (tm && std::atoi(tm) != 0) {
    if (s->ev_t0.create() || s->ev_t1.create()) return fail(EKF_E_HIP);
    s->timing = true;
  }
  s->host_par.assign(F, 0);
  s->host_odom.assign(3 * F, 0.0);
  *out = s;
  return EKF_OK;
}

int ekf_sim_destroy(ekf_sim_t s) {
  if (!s) return EKF_E_ARG;
  if (s->info.stream) hipStreamSynchronize(s->info.stream);
  if (s->sst.get()) hipStreamSynchronize(s->sst.get());
  delete s;
  return EKF_OK;
}

int ekf_sim_run(ekf_sim_t s, int T, const double* wheel_cmd, const int* sense) {
  if (!s || T < 0 || (T > 0 && !wheel_cmd)) return EKF_E_ARG;
  if (T == 0) return EKF_OK;
  if (sense)
    for (int t = 0; t < T; ++t) {
      if (sense[t] < EKF_SENSE_NEAREST || sense[t] > EKF_SENSE_ALL) return EKF_E_ARG;
      if (sense[t] == EKF_SENSE_ALL && (s->L > kMaxChunk || s->cfg.marker_stride < s->L))
        return EKF_E_ARG;
    }
  if (int rc = handle_info(s->h, &s->info)) return rc;  // host-planned work first, bulk joined
  // (Joseph form on the HBM pipeline: both forms write kJoseph chunks of ≤ kMaxJoseph = kMaxChunk
  // markers; the resident path carries the form in its own kernel)
  const bool par = parallel_ok(s, T, sense);
  hipSetDevice(s->info.device);
  if (int rc = reserve(s, T)) return rc;
  if (int rc = reserve_hits(s, T)) return rc;
  if (par) return run_parallel(s, T, wheel_cmd, sense);
  const int b = s->buf;
  s->buf ^= 1;
  const hipStream_t st = s->sst.get();
  const size_t F = static_cast<size_t>(s->info.F);
  const size_t ticks = static_cast<size_t>(T) * s->cfg.ticks_per_msg;
  // the handle's host mirror is authoritative (host-planned calls between runs flip parities)
  if (int rc = handle_parity(s->h, s->host_par.data())) return rc;
  std::memcpy(s->host_par_pinned.get(), s->host_par.data(), F * sizeof(int));
  if (hipMemcpyAsync(s->par.get(), s->host_par_pinned.get(), F * sizeof(int),
                     hipMemcpyHostToDevice, st) != hipSuccess)
    return EKF_E_HIP;
  // buffer b was last read by the filter work of the run before the previous one
  if (hipStreamWaitEvent(st, s->ev_done[b].get(), 0) != hipSuccess) return EKF_E_HIP;
  // (the record goes into marker buffer 0 whatever b is: a replay of the run before may read it)
  if (s->cfg.record && b != 0 && hipStreamWaitEvent(st, s->ev_done[0].get(), 0) != hipSuccess)
    return EKF_E_HIP;
  if (hipMemcpyAsync(s->run.in[b].cmd.get(), wheel_cmd, ticks * 2 * sizeof(double),
                     hipMemcpyHostToDevice, st) != hipSuccess ||
      (sense && hipMemcpyAsync(s->run.in[b].sense.get(), sense, T * sizeof(int),
                               hipMemcpyHostToDevice, st) != hipSuccess))
    return EKF_E_HIP;
  SimArgs a{};
  a.cmd = s->run.in[b].cmd.get();
  a.sense = sense ? s->run.in[b].sense.get() : nullptr;
  a.lm = s->lm.get();
  a.sighted = s->sighted.get();
  a.st = s->st.get();
  a.par = s->par.get();
  a.desc = s->run.in[b].desc.get();
  if (s->cfg.record) {
    const auto& k = s->run.mk[0];
    a.out_ids = k.ids.get();
    a.out_act = k.act.get();
    a.out_rel = k.rel.get();
    a.out_cnt = k.cnt.get();
    a.out_truth = k.truth.get();
    a.out_odom = k.odom.get();
  }
  a.seed = s->cfg.seed;
  a.tick0 = s->tick;
  a.msg0 = s->msg;
  a.f0 = s->cfg.f0;
  a.F = s->info.F;
  a.L = s->L;
  a.T = T;
  a.tpm = s->cfg.ticks_per_msg;
  a.m = s->m;
  a.M = s->cfg.marker_stride;
  a.N = s->info.N;
  a.slip = s->cfg.slip;
  a.sigma = s->cfg.sensor_sigma;
  a.range = s->cfg.max_range;
  a.radius = s->cfg.wheel_radius;
  a.track = s->cfg.track_width;
  a.joseph = s->info.joseph && !s->info.resident;
  // (the record, the counts included, is marker buffer 0's)
  if (!stamp(s, s->ev_t0) ||
      launch_sim(a, set_collide(s, a, s->cfg.record != 0, 0), st) != hipSuccess ||
      !stamp(s, s->ev_t1))
    return EKF_E_HIP;
  s->timed = s->timing;
  // each filter's final parity (its inactive messages do not flip it) and odometry: the host mirror
  if (hipMemcpyAsync(s->host_par_pinned.get(), s->par.get(), F * sizeof(int),
                     hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(s->host_st_pinned.get(), s->st.get(), F * sizeof(SimState),
                     hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipEventRecord(s->ev_sim.get(), st) != hipSuccess ||
      hipEventSynchronize(s->ev_sim.get()) != hipSuccess)
    return EKF_E_HIP;
  std::memcpy(s->host_par.data(), s->host_par_pinned.get(), F * sizeof(int));
  for (size_t f = 0; f < F; ++f)
    for (int k = 0; k < 3; ++k) s->host_odom[3 * f + k] = s->host_st_pinned.get()[f].odom[k];
  s->tick += static_cast<long long>(ticks);
  s->msg += T;
  s->last_T = T;
  s->last_b = 0;
  // the filter's kernels behind the simulation (their descriptors), then release buffer b
  if (hipStreamWaitEvent(s->info.stream, s->ev_sim.get(), 0) != hipSuccess) return EKF_E_HIP;
  const int rc = run_device_plan(s->h, s->run.in[b].desc.get(), s->run.plan.get(), T,
                                 s->host_par.data(), s->host_odom.data());
  if (rc) return rc;
  if (int r2 = handle_info(s->h, &s->info)) return r2;  // joins the bulk stream into main
  return hipEventRecord(s->ev_done[b].get(), s->info.stream) == hipSuccess ? EKF_OK : EKF_E_HIP;
}

int ekf_sim_run_assoc(ekf_sim_t s, int T, const double* wheel_cmd) {
  if (!s || T < 0 || (T > 0 && !wheel_cmd) || s->cfg.marker_stride > kMaxAssoc) return EKF_E_ARG;
  // what the replay underneath would refuse, before the simulator moves: a pipeline handle on the
  // one-marker route has no device-planned association replay
  int route = EKF_ASSOC_MARKER;
  if (int rc = ekf_get_assoc_route(s->h, &route)) return rc;
  if (!s->info.resident && route == EKF_ASSOC_MARKER) return EKF_E_ARG;
  if (T == 0) return EKF_OK;
  if (int rc = handle_info(s->h, &s->info)) return rc;  // host-planned work first, bulk joined
  hipSetDevice(s->info.device);
  s->assoc = true;
  if (int rc = reserve(s, T)) return rc;
  if (int rc = reserve_hits(s, T)) return rc;
  return run_assoc(s, T, wheel_cmd);
}

void ekf_sim_lidar_config_default(ekf_sim_lidar_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->n_beams = 360;
  c->max_markers = 32;
  c->threshold = 0.2;
  c->obstacle_radius = 0.038;
  lm_scan_config_default(&c->scan);
}

int ekf_sim_run_lidar(ekf_sim_t s, lm_t lm, int T, const double* wheel_cmd,
                      const ekf_sim_lidar_config* cfg) {
  if (!s || !lm || !cfg || T < 0 || (T > 0 && !wheel_cmd) || !(cfg->obstacle_radius >= 0.0))
    return EKF_E_ARG;
  // what the front-end or the replay underneath would refuse, before the simulator moves (T = 0
  // asks for no scan: the handle's limits are checked with one)
  const long long S = static_cast<long long>(T) * s->info.F;
  if (S > INT_MAX) return EKF_E_ARG;
  if (int rc = lm_lidar_check(lm, s->info.device, T > 0 ? static_cast<int>(S) : 1, cfg->n_beams,
                              cfg->max_markers, &cfg->scan))
    return rc;
  int route = EKF_ASSOC_MARKER;
  if (int rc = ekf_get_assoc_route(s->h, &route)) return rc;
  if (!s->info.resident && route == EKF_ASSOC_MARKER) return EKF_E_ARG;
  if (T == 0) return EKF_OK;
  if (int rc = handle_info(s->h, &s->info)) return rc;  // host-planned work first, bulk joined
  hipSetDevice(s->info.device);
  s->assoc = true;  // both marker buffers: the replay reads this run's odometry from its own
  if (int rc = reserve(s, T)) return rc;
  if (int rc = reserve_hits(s, T)) return rc;
  return run_lidar(s, lm, T, wheel_cmd, cfg);
}

// Every filter of dst continues src_filter's run: the filter by ekf_copy_state's fork form, the
// simulator's own per-filter state by device copies behind it, the counters on the host.
int ekf_sim_fork(ekf_sim_t dst, ekf_sim_t src, int src_filter) {
  if (!dst || !src || src_filter < 0 || src_filter >= src->info.F) return EKF_E_ARG;
  const ekf_sim_config &d = dst->cfg, &c = src->cfg;
  if (dst->L != src->L || d.ticks_per_msg != c.ticks_per_msg || d.wheel_radius != c.wheel_radius ||
      d.track_width != c.track_width || d.start_theta != c.start_theta ||
      d.start_x != c.start_x || d.start_y != c.start_y)
    return EKF_E_ARG;
  // (checks everything before it touches anything, and waits for both handles' work)
  if (int rc = ekf_copy_state(dst->h, -1, src->h, src_filter)) return rc;
  hipSetDevice(dst->info.device);
  // both simulators idle: nothing reads or writes the per-filter state copied below
  if (hipStreamSynchronize(src->sst.get()) != hipSuccess ||
      hipStreamSynchronize(dst->sst.get()) != hipSuccess)
    return EKF_E_HIP;
  const size_t F = static_cast<size_t>(dst->info.F), L = static_cast<size_t>(src->L);
  const size_t words = (L + 31) / 32, fs = static_cast<size_t>(src_filter);
  // the source filter's poses (hits = 0), sighted set and map, once for every destination filter
  std::vector<SimState> st(F);
  std::vector<unsigned> sighted(F * words);
  std::vector<double> lm(F * L * 2);
  if (hipMemcpy(st.data(), src->st.get() + fs, sizeof(SimState), hipMemcpyDeviceToHost) !=
          hipSuccess ||
      hipMemcpy(sighted.data(), src->sighted.get() + fs * words, words * sizeof(unsigned),
                hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(lm.data(), src->lm.get() + fs * L * 2, L * 2 * sizeof(double),
                hipMemcpyDeviceToHost) != hipSuccess)
    return EKF_E_HIP;
  st[0].hits = 0;
  for (size_t f = 1; f < F; ++f) {
    st[f] = st[0];
    std::copy_n(sighted.begin(), words, sighted.begin() + f * words);
    std::copy_n(lm.begin(), L * 2, lm.begin() + f * L * 2);
  }
  // filters [lo, hi) of dst; the source filter itself is left untouched
  const auto upload = [&](size_t lo, size_t hi) {
    const size_t k = hi - lo;
    return k == 0 ||
           (hipMemcpy(dst->st.get() + lo, st.data(), k * sizeof(SimState),
                      hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dst->sighted.get() + lo * words, sighted.data(),
                      k * words * sizeof(unsigned), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dst->lm.get() + lo * L * 2, lm.data(), k * L * 2 * sizeof(double),
                      hipMemcpyHostToDevice) == hipSuccess);
  };
  if (dst == src ? !(upload(0, fs) && upload(fs + 1, F)) : !upload(0, F)) return EKF_E_HIP;
  for (size_t f = 0; f < F; ++f)
    if (dst != src || f != fs)
      for (int k = 0; k < 3; ++k) dst->host_odom[3 * f + k] = st[0].odom[k];
  dst->tick = src->tick;
  dst->msg = src->msg;
  return EKF_OK;
}

int ekf_sim_set_collisions(ekf_sim_t s, double collision_radius, double obstacle_radius) {
  if (!s || !(collision_radius >= 0.0) || !(obstacle_radius >= 0.0)) return EKF_E_ARG;
  s->hit_r = collision_radius > 0.0 ? collision_radius + obstacle_radius : 0.0;
  return EKF_OK;
}

int ekf_sim_collisions(ekf_sim_t s, long long* total, int* per_msg) {
  if (!s || !total || (per_msg && !s->cfg.record)) return EKF_E_ARG;
  const size_t F = static_cast<size_t>(s->info.F), n = static_cast<size_t>(s->last_T) * F;
  hipSetDevice(s->info.device);
  if (hipStreamSynchronize(s->info.stream) != hipSuccess ||
      hipStreamSynchronize(s->sst.get()) != hipSuccess)
    return EKF_E_HIP;
  std::vector<SimState> st(F);
  if (hipMemcpy(st.data(), s->st.get(), F * sizeof(SimState), hipMemcpyDeviceToHost) != hipSuccess)
    return EKF_E_HIP;
  for (size_t f = 0; f < F; ++f) total[f] = st[f].hits;
  if (per_msg && n) {
    if (!s->last_hits)  // the last run had collisions off
      std::memset(per_msg, 0, n * sizeof(int));
    else if (hipMemcpy(per_msg, s->hits[s->last_b].get(), n * sizeof(int),
                       hipMemcpyDeviceToHost) != hipSuccess)
      return EKF_E_HIP;
  }
  return EKF_OK;
}

int ekf_sim_last_us(ekf_sim_t s, double* us) {
  if (!s || !us || !s->timed) return EKF_E_ARG;
  float ms = 0.0f;
  if (hipEventSynchronize(s->ev_t1.get()) != hipSuccess ||
      hipEventElapsedTime(&ms, s->ev_t0.get(), s->ev_t1.get()) != hipSuccess)
    return EKF_E_HIP;
  *us = 1e3 * static_cast<double>(ms);
  return EKF_OK;
}

int ekf_sim_markers(ekf_sim_t s, int* counts, int* ids, int* actions, double* rel_xy) {
  if (!s || !s->cfg.record) return EKF_E_ARG;
  const size_t n = static_cast<size_t>(s->last_T) * s->info.F, M = s->cfg.marker_stride;
  const auto& k = s->run.mk[s->last_b];
  if (hipStreamSynchronize(s->info.stream) != hipSuccess ||
      hipStreamSynchronize(s->sst.get()) != hipSuccess)
    return EKF_E_HIP;
  const auto d2h = [](void* dst, const void* src, size_t bytes) {  // (a null dst: not asked for)
    return !dst || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess;
  };
  if (!d2h(counts, k.cnt.get(), n * sizeof(int)) || !d2h(ids, k.ids.get(), n * M * sizeof(int)) ||
      !d2h(actions, k.act.get(), n * M * sizeof(int)) ||
      !d2h(rel_xy, k.rel.get(), n * M * 2 * sizeof(double)))
    return EKF_E_HIP;
  return EKF_OK;
}

int ekf_sim_poses(ekf_sim_t s, double* odom, double* truth) {
  if (!s || !s->cfg.record) return EKF_E_ARG;
  const size_t T = static_cast<size_t>(s->last_T);
  const auto& k = s->run.mk[s->last_b];
  if (hipStreamSynchronize(s->info.stream) != hipSuccess ||
      hipStreamSynchronize(s->sst.get()) != hipSuccess)
    return EKF_E_HIP;
  if ((odom && hipMemcpy(odom, k.odom.get(), T * 3 * sizeof(double), hipMemcpyDeviceToHost) !=
                   hipSuccess) ||
      (truth && hipMemcpy(truth, k.truth.get(), T * s->info.F * 3 * sizeof(double),
                          hipMemcpyDeviceToHost) != hipSuccess))
    return EKF_E_HIP;
  return EKF_OK;
}

int ekf_sim_eval(ekf_sim_t s, ekf_eval_rec* out) {
  if (!s || !out) return EKF_E_ARG;
  hipSetDevice(s->info.device);
  // SimState::truth is final once the simulator's stream is idle (the filter's own work is waited
  // for by the evaluation, like any state read)
  if (hipStreamSynchronize(s->sst.get()) != hipSuccess) return EKF_E_HIP;
  const double frame[3] = {s->cfg.start_theta, s->cfg.start_x, s->cfg.start_y};
  return eval_device(s->h, s->st.get()->truth, sizeof(SimState) / sizeof(double), s->lm.get(),
                     s->L, frame, out);
}

int ekf_sim_eval_match(ekf_sim_t s, double max_dist, ekf_eval_rec* out, ekf_match_rec* match_out,
                       int* match) {
  if (!s || !out || !(max_dist >= 0.0)) return EKF_E_ARG;
  hipSetDevice(s->info.device);
  if (hipStreamSynchronize(s->sst.get()) != hipSuccess) return EKF_E_HIP;  // (as ekf_sim_eval)
  const double frame[3] = {s->cfg.start_theta, s->cfg.start_x, s->cfg.start_y};
  return eval_match_device(s->h, s->st.get()->truth, sizeof(SimState) / sizeof(double),
                           s->lm.get(), s->L, frame, max_dist, out, match_out, match);
}

}  // extern "C"
