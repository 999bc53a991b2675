// The C ABI of include/ekf.h: argument checks, the message into the planner (ekf_plan.hpp), then
// the scheduler (ekf_sched.cpp). ekf_create / ekf_destroy own the handle's device resources.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>
#include <vector>

#include "ekf_ctx.hpp"
#include "ekf_internal.hpp"
#include "geom.hpp"
#include "match_math.hpp"

using namespace ekfslam;

namespace {

bool valid(ekf_ctx* h, int f) { return h && f >= 0 && f < h->F; }

// One message per filter (ekf_batch_sensor layout) into the planner and onto the plan.
int load_and_plan(ekf_ctx* h, int assoc_mode, int m_max, const int* counts, const int* ids,
                  const int* actions, const double* rel_xy, const double* odom) {
  Planner& p = h->plan;
  if (int rc = p.load_batch(assoc_mode, m_max, counts, ids, actions, rel_xy, odom)) return rc;
  if (assoc_mode)
    p.unknown(0, h->F, true, true, 0, p.largest(h->F), p.absent(), assoc_route(h));
  else
    p.known(0, h->F, true, p.absent());
  return EKF_OK;
}

// ---- gather and score (ekf_eval.hip): one device buffer per call (eval_buf), carved up ----

// A call's pieces of eval_buf in order, each starting on 16 bytes. Size first, then carve: a call
// runs its takes twice, over a null base to size the buffer (`off` ends as the bytes they need; the
// callers have settled, so nothing in flight reads a buffer that growth frees), then over it.
struct Carver {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t n) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (n * sizeof(T) + 15) / 16 * 16;
    return p;
  }
};

// The truth of ekf_eval / ekf_eval_match: from the host (h_pose [F][3], h_lm [F][n_map][2]) or,
// with h_pose NULL, on the device (d_pose / d_lm).
struct TruthSrc {
  const double *h_pose, *h_lm, *d_pose;
  size_t pose_stride;
  const double* d_lm;
  int n_map;
  const double* frame;
  double *up_pose = nullptr, *up_lm = nullptr;  // a host truth's place in eval_buf
  void carve(Carver& c, size_t F) {
    if (!h_pose) return;
    up_pose = c.take<double>(F * 3);
    if (n_map > 0) up_lm = c.take<double>(F * n_map * 2);
  }
};

// ... uploaded if it is the host's, and as the kernels take it.
int eval_truth(const TruthSrc& s, size_t F, EvalTruth* t) {
  if (s.h_pose) {
    HIPCHK(hipMemcpy(s.up_pose, s.h_pose, F * 3 * sizeof(double), hipMemcpyHostToDevice));
    if (s.n_map > 0)
      HIPCHK(hipMemcpy(s.up_lm, s.h_lm, F * s.n_map * 2 * sizeof(double), hipMemcpyHostToDevice));
  }
  *t = EvalTruth{};
  t->pose = s.h_pose ? s.up_pose : s.d_pose;
  t->pose_stride = s.h_pose ? 3 : s.pose_stride;
  t->lm = s.n_map <= 0 ? nullptr : s.h_pose ? s.up_lm : s.d_lm;
  t->n_map = s.n_map;
  t->has_frame = s.frame != nullptr;
  for (int k = 0; k < 3; ++k) t->frame[k] = s.frame ? s.frame[k] : 0.0;
  return EKF_OK;
}

// The planner's parity of every filter (valid after settle(): a device replay's planning state
// has been adopted) into d_par, and the launch arguments over it.
int eval_args(ekf_ctx* h, int* d_par, int f0, EvalArgs* a) {
  std::vector<int> par(h->F);
  for (int f = 0; f < h->F; ++f) par[f] = h->plan.parity(f);
  HIPCHK(hipMemcpy(d_par, par.data(), par.size() * sizeof(int), hipMemcpyHostToDevice));
  *a = EvalArgs{};
  for (int p = 0; p < 2; ++p) {
    a->sig[p] = h->sig[p].get();
    a->x[p] = h->x[p].get();
  }
  a->sig_stride = h->sig_stride;
  a->x_stride = h->x_stride;
  a->ctl = h->ctl.get();
  a->parity = d_par;
  a->N = h->cfg.n_landmarks;
  a->ld = h->ld;
  a->f0 = f0;
  return EKF_OK;
}

// ekf_eval and, `matched`, ekf_eval_match (the truth map in any order, slots matched within
// max_dist). Arguments checked by the callers.
int eval_run(ekf_ctx* h, TruthSrc src, bool matched, double max_dist, ekf_eval_rec* out,
             ekf_match_rec* match_out, int* match) {
  if (int rc = settle(h)) return rc;
  hipSetDevice(h->cfg.device);
  const size_t F = static_cast<size_t>(h->F), N = static_cast<size_t>(h->cfg.n_landmarks);
  int* par = nullptr;
  MatchOut o{};
  auto carve = [&](char* base) {
    Carver c{base};
    par = c.take<int>(F);
    o.rec = c.take<EvalRec>(F);
    if (matched) {
      o.mrec = c.take<MatchRec>(F);
      o.match = c.take<int>(F * N);
    }
    src.carve(c, F);
    return c.off;
  };
  if (int rc = h->eval_buf.reserve(carve(nullptr))) return rc;
  carve(h->eval_buf.get());
  EvalTruth t;
  if (int rc = eval_truth(src, F, &t)) return rc;
  EvalArgs a;
  if (int rc = eval_args(h, par, 0, &a)) return rc;
  const hipStream_t st = h->stream.get();
  const int rc = timed(h, matched ? kProfEvalMatch : kProfEval, [&](hipEvent_t e0, hipEvent_t e1) {
    return by_dtype(h, [&](auto tag) {
      using T = decltype(tag);
      return matched ? launch_eval_match<T>(a, t, max_dist * max_dist, o, h->F, st, e0, e1)
                     : launch_eval<T>(a, t, o.rec, h->F, st, e0, e1);
    });
  });
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpy(out, o.rec, F * sizeof(EvalRec), hipMemcpyDeviceToHost));
  if (match_out) HIPCHK(hipMemcpy(match_out, o.mrec, F * sizeof(MatchRec), hipMemcpyDeviceToHost));
  if (match) HIPCHK(hipMemcpy(match, o.match, F * N * sizeof(int), hipMemcpyDeviceToHost));
  return EKF_OK;
}

bool eval_args_ok(const ekf_ctx* h, const void* pose, const void* lm, int n_map, const void* out) {
  return h && pose && out && n_map >= 0 && n_map <= h->cfg.n_landmarks && (lm || n_map == 0);
}

// (max_dist: not negative and not NaN; +∞ is valid)
bool match_args_ok(const ekf_ctx* h, const void* pose, const void* lm, int n_map, double max_dist,
                   const void* out) {
  return h && pose && lm && out && n_map >= 1 && n_map <= kMatchMaxMap && max_dist >= 0.0;
}

}  // namespace

int ekfslam::eval_match_device(ekf_t h, const double* d_pose, size_t pose_stride,
                               const double* d_lm, int n_map, const double* frame, double max_dist,
                               ekf_eval_rec* out, ekf_match_rec* match_out, int* match) {
  if (!match_args_ok(h, d_pose, d_lm, n_map, max_dist, out)) return EKF_E_ARG;
  return eval_run(h, {nullptr, nullptr, d_pose, pose_stride, d_lm, n_map, frame}, true, max_dist,
                  out, match_out, match);
}

int ekfslam::eval_device(ekf_t h, const double* d_pose, size_t pose_stride, const double* d_lm,
                         int n_map, const double* frame, ekf_eval_rec* out) {
  if (!eval_args_ok(h, d_pose, d_lm, n_map, out)) return EKF_E_ARG;
  return eval_run(h, {nullptr, nullptr, d_pose, pose_stride, d_lm, n_map, frame}, false, 0.0, out,
                  nullptr, nullptr);
}

extern "C" {

void ekf_config_default(ekf_config* c) {
  if (!c) return;
  c->n_landmarks = 50;
  c->n_filters = 1;
  c->dtype = EKF_F64;
  c->q_noise = 1.0e-2;
  c->r_noise = 1.0e-2;
  c->init_var = 10e6;
  c->mah_gate = 2.0;
  c->device = 0;
}

const char* ekf_strerror(int s) {
  switch (s) {
    case EKF_OK: return "ok";
    case EKF_E_ARG: return "invalid argument";
    case EKF_E_RANGE: return "landmark index out of range / landmark capacity exhausted";
    case EKF_E_EMPTY: return "empty marker array";
    case EKF_E_NUMERIC: return "singular or non-finite innovation covariance";
    case EKF_E_HIP: return "HIP runtime error";
    case EKF_E_NOMEM: return "out of memory";
    case EKF_E_TIMEOUT:
      return "a device hand-off timed out: the state of the filters flagged EKF_FLAG_TIMEOUT is "
             "undefined (ekf_reset / ekf_set_state them)";
    default: return "unknown status";
  }
}

int ekf_create(ekf_t* out, const ekf_config* cfg_in) {
  if (!out) return EKF_E_ARG;
  *out = nullptr;
  ekf_config cfg;
  ekf_config_default(&cfg);
  if (cfg_in) cfg = *cfg_in;
  if (cfg.n_landmarks < 1 || cfg.n_filters < 1 || (cfg.dtype != EKF_F64 && cfg.dtype != EKF_F32))
    return EKF_E_ARG;
  ekf_ctx* h = new (std::nothrow) ekf_ctx;
  if (!h) return EKF_E_NOMEM;
  h->cfg = cfg;
  h->F = cfg.n_filters;
  h->n = 3 + 2 * cfg.n_landmarks;
  h->w = cfg.dtype == EKF_F32 ? 4 : 8;
  const int per_line = static_cast<int>(128 / h->w);
  h->ld = (h->n + per_line - 1) / per_line * per_line;
  h->ldk = (h->n + 63) / 64 * 64;
  h->sig_stride = static_cast<size_t>(h->n) * h->ld;
  h->x_stride = static_cast<size_t>((h->n + 15) / 16 * 16);
  h->km_stride = static_cast<size_t>(kMaxKW) * h->ldk;
  h->held.assign(h->F, 0);
  auto fail = [&](int rc) {
    ekf_destroy(h);  // (the members release what exists by then)
    return rc;
  };
  if (hipSetDevice(cfg.device) != hipSuccess) return fail(EKF_E_HIP);
  const char* serial_env = std::getenv("EKF_SERIAL");
  if (serial_env) h->serial = std::atoi(serial_env) != 0;
  if (const char* e = std::getenv("EKF_ASSOC_MSG")) h->assoc_msg = std::atoi(e) != 0;
  if (const char* e = std::getenv("EKF_CHAIN_FAST")) h->chain_fast = std::atoi(e) != 0;
  {  // EKF_RESIDENT=0: the HBM pipeline at every size (tests compare the two)
    const char* e = std::getenv("EKF_RESIDENT");
    h->resident = cfg.dtype == EKF_F64 && h->n <= kResidentMaxN && !(e && std::atoi(e) == 0);
  }
  if (create_streams(h) || h->ev_chain.create() || h->ev_join.create() || h->ev_sig[0].create() ||
      h->ev_sig[1].create())
    return fail(EKF_E_HIP);
  // Many filters (no CU split, so event hand-offs): the Σ pass's waves hold every CU a chain or a
  // factor kernel needs, so nothing overlaps it anyway; one stream turns the two
  // cross-stream hops per message into kernel boundaries: swarm 1.12 → 1.15e7 corrections/s, with
  // the staging off (below) 1.17e7 (profiles/r4/r4s_*). EKF_SERIAL=0 keeps the two streams.
  if (!serial_env && !h->devsync && h->F > kCuSplitMaxFilters) h->serial = true;
  h->am_route = am_route(h, false);
  h->am_route_j = am_route(h, true);
  if (int rc = h->fatal_h.reserve(64 / sizeof(unsigned))) return fail(rc);
  *h->fatal_h.get() = 0;
  if (hipHostGetDevicePointer(reinterpret_cast<void**>(&h->fatal_d), h->fatal_h.get(), 0) !=
      hipSuccess)
    return fail(EKF_E_HIP);
  const size_t F = static_cast<size_t>(h->F);
  const size_t sig_bytes = h->sig_stride * F * h->w, km_bytes = h->km_stride * F * h->w;
  for (int p = 0; p < 2; ++p)
    if (h->sig[p].reserve(sig_bytes) || h->x[p].reserve(h->x_stride * F)) return fail(EKF_E_NOMEM);
  if (h->kcat.reserve(km_bytes) || h->mcat.reserve(km_bytes) || h->ctl.reserve(F) ||
      h->rec.reserve(2 * F))
    return fail(EKF_E_NOMEM);
  // staged rebuild operands (EKF_STAGE=0: every kLook chain gathers its own, tests compare the two)
  // The same many-filter handles skip it by default (EKF_STAGE=1 keeps it): there every message's
  // k_stage runs on the serial critical path (≈ 18 µs for 512 filters), more than the chains'
  // own gathers cost (two rounds of ≈ 2 µs).
  const char* stage_env = std::getenv("EKF_STAGE");
  const size_t stage_bytes =
      2 * h->F * by_dtype(h, [](auto tag) { return sizeof(StageRec<decltype(tag)>); });
  const bool stage_on = stage_env ? std::atoi(stage_env) != 0
                                  : (h->devsync || h->F <= kCuSplitMaxFilters);
  if (stage_on) {
    if (int rc = h->stage.reserve(stage_bytes)) return fail(rc);
    if (hipMemset(h->stage.get(), 0, stage_bytes) != hipSuccess) return fail(EKF_E_HIP);
  }
  h->plan.init(h->F, cfg.n_landmarks, h->resident, stage_on);
  if (int rc = h->sync.reserve(kSyncChain + F)) return fail(rc);
  if (hipMemset(h->sync.get(), 0, sizeof(unsigned) * h->sync.capacity()) != hipSuccess)
    return fail(EKF_E_HIP);
  if (int rc = h->ddesc.reserve(std::max(kDescInit, F * 4))) return fail(rc);
  for (StageSlot& sl : h->ring)
    if (int rc = sl.ev.create()) return fail(rc);
  // every pinned slot up front
  if (int rc = reserve_upload(h, h->ddesc.capacity())) return fail(rc);
  // Σ₀ = diag(0,0,0, init_var·I_2N), state = 0 (slam.cpp:127-132, :674)
  for (int p = 0; p < 2; ++p) {
    if (hipMemsetAsync(h->sig[p].get(), 0, sig_bytes, h->stream.get()) != hipSuccess ||
        hipMemsetAsync(h->x[p].get(), 0, h->x_stride * F * sizeof(double), h->stream.get()) !=
            hipSuccess)
      return fail(EKF_E_HIP);
  }
  // chunk records start zeroed: no kernel ever sees a previous process's bytes, whatever the
  // stream interleaving
  if (hipMemsetAsync(h->rec.get(), 0, 2 * sizeof(ChunkRec) * F, h->stream.get()) != hipSuccess ||
      hipMemsetAsync(h->kcat.get(), 0, km_bytes, h->stream.get()) != hipSuccess ||
      hipMemsetAsync(h->mcat.get(), 0, km_bytes, h->stream.get()) != hipSuccess ||
      hipMemsetAsync(h->ctl.get(), 0, sizeof(FilterCtl) * F, h->stream.get()) != hipSuccess)
    return fail(EKF_E_HIP);
  if (init_diag(h, h->sig[0].get(), h->F) || hipStreamSynchronize(h->stream.get()) != hipSuccess)
    return fail(EKF_E_HIP);
  *out = h;
  return EKF_OK;
}

int ekf_destroy(ekf_t h) {
  if (!h) return EKF_E_ARG;
  hipSetDevice(h->cfg.device);
  if (h->bulk.get()) hipStreamSynchronize(h->bulk.get());
  if (h->stream.get()) hipStreamSynchronize(h->stream.get());
  delete h;
  return EKF_OK;
}

int ekf_dims(ekf_t h, int* n, int* ld, int* nf) {
  if (!h) return EKF_E_ARG;
  if (n) *n = h->n;
  if (ld) *ld = h->ld;
  if (nf) *nf = h->F;
  return EKF_OK;
}

int ekf_get_path(ekf_t h, int* path) {
  if (!h || !path) return EKF_E_ARG;
  *path = h->resident ? EKF_PATH_RESIDENT : EKF_PATH_PIPELINE;
  return EKF_OK;
}

int ekf_set_odom(ekf_t h, int f, double theta, double x, double y) {
  if (!valid(h, f)) return EKF_E_ARG;
  if (int rc = adopt_device_plan(h)) return rc;
  h->plan.set_odom(f, theta, x, y);
  return EKF_OK;
}

int ekf_fake_sensor(ekf_t h, int f, int m, const int* ids, const int* actions,
                    const double* rel_xy) {
  if (!valid(h, f) || m < 0 || (m > 0 && (!ids || !rel_xy))) return EKF_E_ARG;
  if (m == 0) return EKF_E_EMPTY;
  if (int rc = adopt_device_plan(h)) return rc;
  if (int rc = h->plan.set_message(m, ids, actions, rel_xy)) return rc;
  hipSetDevice(h->cfg.device);
  h->plan.known(f, 1, true);
  return submit(h);
}

int ekf_sensor(ekf_t h, int f, int m, const double* rel_xy, int* assoc_out, int* is_new_out) {
  if (!valid(h, f) || m < 0 || (m > 0 && !rel_xy)) return EKF_E_ARG;
  if (m == 0) return EKF_E_EMPTY;
  if (int rc = adopt_device_plan(h)) return rc;
  h->plan.set_message(m, nullptr, nullptr, rel_xy);
  hipSetDevice(h->cfg.device);
  if (!assoc_out && !is_new_out) {
    h->plan.unknown(f, 1, true, true, 0, m, nullptr, assoc_route(h));
    return submit(h);
  }
  if (int r0 = settle(h)) return r0;  // earlier (asynchronous) skips are not this call's
  if (int r0 = take_numeric(h, f, nullptr)) return r0;
  const int rc = assoc_sync(h, f, 1, true, true, m, assoc_out, is_new_out);
  if (rc) return rc;
  if (drain(h)) return EKF_E_HIP;
  if (int t = take_fatal(h)) return t;
  return status_rc(h, f, true);
}

int ekf_batch_sensor(ekf_t h, int assoc_mode, int m_max, const int* counts, const int* ids,
                     const int* actions, const double* rel_xy, const double* odom) {
  if (!h || m_max < 0 || !counts || (m_max > 0 && !rel_xy) || (!assoc_mode && m_max > 0 && !ids))
    return EKF_E_ARG;
  if (int r0 = adopt_device_plan(h)) return r0;
  if (int rc = load_and_plan(h, assoc_mode, m_max, counts, ids, actions, rel_xy, odom)) return rc;
  hipSetDevice(h->cfg.device);
  return submit(h);
}

int ekf_replay(ekf_t h, int assoc_mode, int T, int m_max, const int* counts, const int* ids,
               const int* actions, const double* rel_xy, const double* odom, double* out_pose) {
  if (!h || T < 0 || !counts || !odom || m_max < 0 || (m_max > 0 && !rel_xy) ||
      (!assoc_mode && m_max > 0 && !ids))
    return EKF_E_ARG;
  const size_t F = static_cast<size_t>(h->F);
  hipSetDevice(h->cfg.device);
  if (int rc = adopt_device_plan(h)) return rc;
  for (int t = 0; t < T; ++t) {
    const size_t o = static_cast<size_t>(t) * F * m_max;
    int rc = load_and_plan(h, assoc_mode, m_max, counts + t * F, ids ? ids + o : nullptr,
                           actions ? actions + o : nullptr, rel_xy + 2 * o, odom + 3 * F * t);
    if (rc) {
      flush(h);
      return rc;
    }
    // Many filters: upload and launch every ~kFlushDesc descriptors, so planning the next
    // messages on the host overlaps the GPU's work on these (one filter keeps the whole replay in
    // one upload and one persistent chain launch).
    if (!out_pose && plan_is_large(h)) {
      rc = flush(h);
      if (rc) return rc;
    }
    if (out_pose) {
      rc = flush(h);
      if (rc) return rc;
      if (drain(h)) return EKF_E_HIP;
      for (size_t f = 0; f < F; ++f)
        HIPCHK(hipMemcpy(out_pose + 3 * (F * t + f),
                         h->x[h->plan.parity(f)].get() + f * h->x_stride, 3 * sizeof(double),
                         hipMemcpyDeviceToHost));
    }
  }
  return submit(h);
}

int ekf_replay_device(ekf_t h, int T, int m_max, const int* d_counts, const int* d_ids,
                      const int* d_actions, const double* d_rel_xy, const double* d_odom) {
  if (!h || T < 0 || m_max < 0 || m_max > kMaxChunk || !d_counts || !d_odom ||
      (m_max > 0 && (!d_ids || !d_rel_xy)))
    return EKF_E_ARG;
  if (h->resident) return EKF_E_ARG;
  if (T == 0) return EKF_OK;
  return replay_device(h, T, m_max, d_counts, d_ids, d_actions, d_rel_xy, d_odom);
}

int ekf_replay_device_assoc(ekf_t h, int T, int m_max, const int* d_counts, const double* d_xy,
                            int xy_stride, const double* d_odom) {
  if (!h || T < 1 || m_max < 1 || m_max > kMaxAssoc || xy_stride < 2 || !d_counts || !d_xy ||
      !d_odom)
    return EKF_E_ARG;
  if (!device_assoc_supported(h)) return EKF_E_ARG;
  return replay_device_assoc(h, T, m_max, d_counts, d_xy, xy_stride, d_odom, nullptr, nullptr,
                             nullptr);
}

int ekf_replay_resident(ekf_t h, int assoc, int T, int m_max, const int* d_counts,
                        const int* d_ids, const int* d_actions, const double* d_xy, int xy_stride,
                        const double* d_odom) {
  if (!h || T < 1 || m_max < 1 || m_max > kMaxAssoc || xy_stride < 2 || !d_counts || !d_xy ||
      !d_odom || (!assoc && !d_ids))
    return EKF_E_ARG;
  if (!h->resident) return EKF_E_ARG;
  return replay_resident(h, assoc, T, m_max, d_counts, d_ids, d_actions, d_xy, xy_stride, d_odom,
                         nullptr, nullptr, nullptr);
}

int ekf_get_decisions(ekf_t h, int f, int m, int* assoc_out, int* is_new_out) {
  if (!valid(h, f) || m < 0 || m > kMaxAssoc) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  FilterCtl c;
  HIPCHK(hipMemcpy(&c, h->ctl.get() + f, sizeof(FilterCtl), hipMemcpyDeviceToHost));
  for (int i = 0; i < m; ++i) {
    if (assoc_out) assoc_out[i] = c.assoc_j[i];
    if (is_new_out) is_new_out[i] = c.assoc_new[i];
  }
  return EKF_OK;
}

int ekf_chain_path_counts(ekf_t h, int f, unsigned long long* lean, unsigned long long* generic) {
  if (!valid(h, f) || !lean || !generic) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  FilterCtl c;
  HIPCHK(hipMemcpy(&c, h->ctl.get() + f, sizeof(FilterCtl), hipMemcpyDeviceToHost));
  *lean = c.chain_steps[0];
  *generic = c.chain_steps[1];
  return EKF_OK;
}

int ekf_predict(ekf_t h, int f) {
  if (!valid(h, f)) return EKF_E_ARG;
  if (int rc = adopt_device_plan(h)) return rc;
  h->plan.set_pending(f, true);
  return EKF_OK;
}

int ekf_correct(ekf_t h, int f, int id, double rx, double ry) {
  if (!valid(h, f)) return EKF_E_ARG;
  if (id < 0 || id >= h->cfg.n_landmarks) return EKF_E_RANGE;
  if (int rc = adopt_device_plan(h)) return rc;
  const double rel[2] = {rx, ry};
  h->plan.set_message(1, &id, nullptr, rel);
  hipSetDevice(h->cfg.device);
  h->plan.known(f, 1, false);
  return submit(h);
}

int ekf_associate_correct(ekf_t h, int f, double rx, double ry, int* j, int* is_new) {
  if (!valid(h, f)) return EKF_E_ARG;
  if (int rc = adopt_device_plan(h)) return rc;
  const double rel[2] = {rx, ry};
  h->plan.set_message(1, nullptr, nullptr, rel);
  hipSetDevice(h->cfg.device);
  int jj = -1, nn = 0;
  if (int r0 = settle(h)) return r0;  // earlier (asynchronous) skips are not this call's
  if (int r0 = take_numeric(h, f, nullptr)) return r0;
  const int rc = assoc_sync(h, f, 1, false, false, 1, &jj, &nn);
  if (rc) return rc;
  if (int t = take_fatal(h)) return t;  // (assoc_sync drained)
  if (j) *j = jj;
  if (is_new) *is_new = nn;
  const int nrc = status_rc(h, f, false);
  if (jj < 0) return EKF_E_RANGE;
  return nrc;
}

int ekf_posterior(ekf_t h, int f) {
  if (!valid(h, f)) return EKF_E_ARG;
  if (int rc = adopt_device_plan(h)) return rc;
  hipSetDevice(h->cfg.device);
  if (h->plan.pending(f)) {  // fold the pending predict into a zero-marker pass, then the posterior
    h->plan.set_message(0, nullptr, nullptr, nullptr);
    h->plan.known(f, 1, true);
  } else {
    h->plan.posterior(f);
  }
  return submit(h);
}

int ekf_flush(ekf_t h) {
  if (!h) return EKF_E_ARG;
  return flush(h);
}

int ekf_sync(ekf_t h) {
  if (!h) return EKF_E_ARG;
  // (a device replay's planning state stays on the device: the next host access adopts it)
  if (int rc = flush(h)) return rc;
  if (drain(h)) return EKF_E_HIP;
  return take_fatal(h);
}

int ekf_get_schedule(ekf_t h, int* flags) {
  if (!h || !flags) return EKF_E_ARG;
  *flags = (h->devsync ? EKF_SCHED_DEVSYNC : 0) | (h->serial ? EKF_SCHED_SERIAL : 0);
  return EKF_OK;
}

int ekf_get_assoc_route(ekf_t h, int* route) {
  if (!h || !route) return EKF_E_ARG;
  *route = assoc_route(h);
  return EKF_OK;
}

int ekf_set_joseph(ekf_t h, int on) {
  if (!h) return EKF_E_ARG;
  if (int rc = flush(h)) return rc;  // what is planned runs with the form it was planned in
  if (h->plan.joseph() == (on != 0)) return EKF_OK;
  if (int rc = adopt_device_plan(h)) return rc;
  h->plan.set_joseph(on != 0);
  return EKF_OK;
}

int ekf_defer(ekf_t h, int on) {
  if (!h) return EKF_E_ARG;
  h->defer = on != 0;
  return on ? EKF_OK : flush(h);
}

// Σ₀ = diag(0,0,0, init_var·I_2N), state 0, t_map_odom identity, counter 0 (slam.cpp:127-139),
// on the device, for one filter or all (f < 0): a fresh run without reallocating.
int ekf_reset(ekf_t h, int f) {
  if (!h || f >= h->F) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  hipSetDevice(h->cfg.device);
  const int f0 = f < 0 ? 0 : f, nf = f < 0 ? h->F : 1;
  for (int k = f0; k < f0 + nf; ++k) {
    h->plan.reset(k);
    h->held[k] = 0;
  }
  const size_t sb = h->sig_stride * h->w;
  char* sig0 = static_cast<char*>(h->sig[0].get()) + f0 * sb;
  HIPCHK(hipMemsetAsync(sig0, 0, sb * nf, h->stream.get()));
  HIPCHK(hipMemsetAsync(h->x[0].get() + f0 * h->x_stride, 0, h->x_stride * nf * sizeof(double),
                        h->stream.get()));
  HIPCHK(hipMemsetAsync(h->ctl.get() + f0, 0, sizeof(FilterCtl) * nf, h->stream.get()));
  if (h->trace.get())  // the filters' pose traces restart at record 0
    HIPCHK(hipMemsetAsync(h->trace_n.get() + f0, 0, sizeof(long long) * nf, h->stream.get()));
  if (init_diag(h, sig0, nf)) return EKF_E_HIP;
  return drain(h);
}

// ---- the pose trace: records appended by the kernels that store a posterior t_map_odom ----

int ekf_trace_enable(ekf_t h, int capacity) {
  if (!h || capacity < 0) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;  // nothing in flight reads the buffers replaced below
  hipSetDevice(h->cfg.device);
  // the new buffers first, so that a failure changes nothing (ekf.h); the old ones go with the move
  DeviceBuf<TraceRec> recs;
  DeviceBuf<long long> counts;
  if (capacity > 0) {
    const size_t F = static_cast<size_t>(h->F);
    if (recs.reserve(F * capacity) || counts.reserve(F)) return EKF_E_NOMEM;
    HIPCHK(hipMemset(counts.get(), 0, F * sizeof(long long)));
  }
  h->trace = std::move(recs);
  h->trace_n = std::move(counts);
  h->trace_cap = capacity;
  return EKF_OK;
}

int ekf_trace_count(ekf_t h, int f, long long* appended) {
  if (!valid(h, f) || !appended || !h->trace.get()) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  HIPCHK(hipMemcpy(appended, h->trace_n.get() + f, sizeof(long long), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_trace_read(ekf_t h, int f, long long first, int n, ekf_trace_rec* out, int* got) {
  if (!valid(h, f) || !out || !got || !h->trace.get() || first < 0 || n < 0) return EKF_E_ARG;
  *got = 0;
  if (int rc = settle(h)) return rc;
  long long appended = 0;
  HIPCHK(hipMemcpy(&appended, h->trace_n.get() + f, sizeof(long long), hipMemcpyDeviceToHost));
  const long long kept = std::min<long long>(appended, h->trace_cap);
  if (first >= kept || n == 0) return EKF_OK;
  const long long k = std::min<long long>(n, kept - first);
  HIPCHK(hipMemcpy(out, h->trace.get() + static_cast<size_t>(f) * h->trace_cap + first,
                   static_cast<size_t>(k) * sizeof(TraceRec), hipMemcpyDeviceToHost));
  *got = static_cast<int>(k);
  return EKF_OK;
}

int ekf_trace_clear(ekf_t h, int f) {
  if (!h || f >= h->F || !h->trace.get()) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  hipSetDevice(h->cfg.device);
  const int f0 = f < 0 ? 0 : f, nf = f < 0 ? h->F : 1;
  HIPCHK(hipMemsetAsync(h->trace_n.get() + f0, 0, sizeof(long long) * nf, h->stream.get()));
  return drain(h);  // (the bulk stream's next launch is not ordered after the main stream's memset)
}

int ekf_get_pose(ekf_t h, int f, double* p) {
  if (!valid(h, f) || !p) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  HIPCHK(hipMemcpy(p, h->x[h->plan.parity(f)].get() + f * h->x_stride, 3 * sizeof(double),
                   hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_get_map_odom(ekf_t h, int f, double* p) {
  if (!valid(h, f) || !p) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  HIPCHK(hipMemcpy(p, h->ctl.get()[f].tmo, 3 * sizeof(double), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_get_state(ekf_t h, int f, double* state, double* sigma, unsigned* counter) {
  if (!valid(h, f)) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  const int p = h->plan.parity(f);
  if (state)
    HIPCHK(hipMemcpy(state, h->x[p].get() + f * h->x_stride, h->n * sizeof(double),
                     hipMemcpyDeviceToHost));
  if (sigma) {
    std::vector<char> buf(h->sig_stride * h->w);
    const char* src = static_cast<const char*>(h->sig[p].get()) + f * h->sig_stride * h->w;
    HIPCHK(hipMemcpy(buf.data(), src, buf.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < h->n; ++i)
      for (int j = 0; j < h->n; ++j) {
        const size_t e = static_cast<size_t>(i) * h->ld + j;
        sigma[static_cast<size_t>(i) * h->n + j] =
            h->w == 4 ? reinterpret_cast<const float*>(buf.data())[e]
                      : reinterpret_cast<const double*>(buf.data())[e];
      }
  }
  if (counter)
    HIPCHK(hipMemcpy(counter, &h->ctl.get()[f].counter, sizeof(unsigned), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_set_state(ekf_t h, int f, const double* state, const double* sigma, const double* tmo,
                  unsigned counter) {
  if (!valid(h, f)) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  h->plan.forget(f);
  const int p = h->plan.parity(f);
  if (state)
    HIPCHK(hipMemcpy(h->x[p].get() + f * h->x_stride, state, h->n * sizeof(double),
                     hipMemcpyHostToDevice));
  if (sigma) {
    std::vector<char> buf(h->sig_stride * h->w, 0);
    // fp64 pipeline: Σ is kept exactly symmetric (the symmetric Σ pass mirrors its upper triangle
    // and the factor kernel reads Σ_in[U, i] for Σ_in[i, U]), so the upper triangle is taken
    const bool sym = h->w == 8 && !h->resident;
    for (int i = 0; i < h->n; ++i)
      for (int j = 0; j < h->n; ++j) {
        const size_t e = static_cast<size_t>(i) * h->ld + j;
        const double v = sym && i > j ? sigma[static_cast<size_t>(j) * h->n + i]
                                      : sigma[static_cast<size_t>(i) * h->n + j];
        if (h->w == 4)
          reinterpret_cast<float*>(buf.data())[e] = static_cast<float>(v);
        else
          reinterpret_cast<double*>(buf.data())[e] = v;
      }
    char* dst = static_cast<char*>(h->sig[p].get()) + f * h->sig_stride * h->w;
    HIPCHK(hipMemcpy(dst, buf.data(), buf.size(), hipMemcpyHostToDevice));
  }
  if (tmo) HIPCHK(hipMemcpy(h->ctl.get()[f].tmo, tmo, 3 * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(&h->ctl.get()[f].counter, &counter, sizeof(unsigned), hipMemcpyHostToDevice));
  h->plan.set_pending(f, false);
  return EKF_OK;
}

// ekf_get_state + ekf_get_map_odom on `src`, ekf_set_state + ekf_set_odom on `dst`, without the
// host in between (k_copy_state, ekf_copy.hip): the same element rules as the two above, and the
// planner's t_odom_robot and pending predict carried as well.
int ekf_copy_state(ekf_t dst, int fd, ekf_t src, int fs) {
  if (!dst || !src || fd >= dst->F || fs >= src->F || (fd >= 0 && fs < 0)) return EKF_E_ARG;
  if (fd < 0 && fs < 0 && dst->F != src->F) return EKF_E_ARG;
  if (dst->cfg.n_landmarks < src->cfg.n_landmarks || dst->cfg.device != src->cfg.device)
    return EKF_E_ARG;
  if (int rc = settle(src)) return rc;
  if (dst != src)
    if (int rc = settle(dst)) return rc;
  // a filter onto itself is left out: nothing of it is read, written or forgotten
  const int skip = dst == src ? fs : -1;
  if (dst == src && (fs < 0 || fd == fs)) return EKF_OK;
  hipSetDevice(dst->cfg.device);
  const int f0 = fd < 0 ? 0 : fd, nf = fd < 0 ? dst->F : 1;
  int *spar = nullptr, *dpar = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    spar = c.take<int>(src->F);
    dpar = c.take<int>(dst->F);
    return c.off;
  };
  if (int rc = dst->eval_buf.reserve(carve(nullptr))) return rc;
  carve(dst->eval_buf.get());
  std::vector<int> par(std::max(src->F, dst->F));
  for (int f = 0; f < src->F; ++f) par[f] = src->plan.parity(f);
  HIPCHK(hipMemcpy(spar, par.data(), src->F * sizeof(int), hipMemcpyHostToDevice));
  for (int f = 0; f < dst->F; ++f) par[f] = dst->plan.parity(f);
  HIPCHK(hipMemcpy(dpar, par.data(), dst->F * sizeof(int), hipMemcpyHostToDevice));
  CopyArgs a{};
  for (int p = 0; p < 2; ++p) {
    a.src_sig[p] = src->sig[p].get();
    a.src_x[p] = src->x[p].get();
    a.dst_sig[p] = dst->sig[p].get();
    a.dst_x[p] = dst->x[p].get();
  }
  a.src_sig_stride = src->sig_stride;
  a.src_x_stride = src->x_stride;
  a.src_ctl = src->ctl.get();
  a.src_par = spar;
  a.n_src = src->n;
  a.ld_src = src->ld;
  a.dst_sig_stride = dst->sig_stride;
  a.dst_x_stride = dst->x_stride;
  a.dst_ctl = dst->ctl.get();
  a.dst_par = dpar;
  a.n_dst = dst->n;
  a.ld_dst = dst->ld;
  a.src_f = fs;
  a.skip = skip;
  a.prior = dst->cfg.init_var;
  // fp64 pipeline destinations keep Σ exactly symmetric (ekf_set_state's rule)
  const bool sym = dst->w == 8 && !dst->resident;
  // A fork splits its destination filters over enough workgroups to fill the device (a few per
  // CU), each reading its source tile once; the other forms have one workgroup per tile and filter.
  const int tiles = ((dst->ld + kCopyTile - 1) / kCopyTile) * ((dst->n + kCopyTile - 1) / kCopyTile);
  const int blocks = std::min(nf, (2048 + tiles - 1) / tiles);
  a.fpb = fs >= 0 ? (nf + blocks - 1) / blocks : 1;
  const int per_launch = 65535;  // (the grid's z limit, in workgroups of fpb filters)
  for (int k = 0; k < nf; k += per_launch * a.fpb) {
    a.dst_f0 = f0 + k;
    a.nf = std::min(nf - k, per_launch * a.fpb);
    HIPCHK(launch_copy_state(a, src->w == 4, dst->w == 4, sym, dst->stream.get()));
  }
  for (int k = f0; k < f0 + nf; ++k) {
    if (k == skip) continue;
    const int from = fs >= 0 ? fs : k;
    const std::array<double, 3> odom = src->plan.odom(from);
    dst->plan.forget(k);
    dst->plan.set_pending(k, src->plan.pending(from));
    dst->plan.set_odom(k, odom[0], odom[1], odom[2]);
  }
  return drain(dst);
}

int ekf_get_status(ekf_t h, int f, unsigned* flags) {
  if (!valid(h, f) || !flags) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  HIPCHK(hipMemcpy(flags, &h->ctl.get()[f].status, sizeof(unsigned), hipMemcpyDeviceToHost));
  const unsigned z = 0;
  HIPCHK(hipMemcpy(&h->ctl.get()[f].status, &z, sizeof(unsigned), hipMemcpyHostToDevice));
  *flags |= h->held[f];
  h->held[f] = 0;
  return EKF_OK;
}

// ---- marginals and scoring: read-only kernels over the filters' "in" copies (ekf_eval.hip) ----

int ekf_get_marginals(ekf_t h, int f, double* pose, double* pose_cov, ekf_lm_marginal* lm,
                      unsigned* counter) {
  if (!h || f >= h->F) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  hipSetDevice(h->cfg.device);
  const int f0 = f < 0 ? 0 : f;
  const size_t nf = f < 0 ? h->F : 1, N = h->cfg.n_landmarks;
  int* par = nullptr;
  MarginalOut o{};
  auto carve = [&](char* base) {
    Carver c{base};
    par = c.take<int>(h->F);
    o.pose = c.take<double>(nf * 3);
    o.pose_cov = c.take<double>(nf * 9);
    o.counter = c.take<unsigned>(nf);
    o.lm = lm ? c.take<LmMarginal>(nf * N) : nullptr;
    return c.off;
  };
  if (int rc = h->eval_buf.reserve(carve(nullptr))) return rc;
  carve(h->eval_buf.get());
  EvalArgs a;
  if (int rc = eval_args(h, par, f0, &a)) return rc;
  HIPCHK(by_dtype(h, [&](auto tag) {
    return launch_marginals<decltype(tag)>(a, o, static_cast<int>(nf), h->stream.get());
  }));
  HIPCHK(hipStreamSynchronize(h->stream.get()));
  if (pose) HIPCHK(hipMemcpy(pose, o.pose, nf * 3 * sizeof(double), hipMemcpyDeviceToHost));
  if (pose_cov)
    HIPCHK(hipMemcpy(pose_cov, o.pose_cov, nf * 9 * sizeof(double), hipMemcpyDeviceToHost));
  if (counter)
    HIPCHK(hipMemcpy(counter, o.counter, nf * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (lm) HIPCHK(hipMemcpy(lm, o.lm, nf * N * sizeof(LmMarginal), hipMemcpyDeviceToHost));
  return EKF_OK;
}

int ekf_eval(ekf_t h, const double* truth_pose, const double* truth_lm, int n_map,
             const double* frame, ekf_eval_rec* out) {
  if (!eval_args_ok(h, truth_pose, truth_lm, n_map, out)) return EKF_E_ARG;
  return eval_run(h, {truth_pose, truth_lm, nullptr, 0, nullptr, n_map, frame}, false, 0.0, out,
                  nullptr, nullptr);
}

int ekf_eval_match(ekf_t h, const double* truth_pose, const double* truth_lm, int n_map,
                   const double* frame, double max_dist, ekf_eval_rec* out,
                   ekf_match_rec* match_out, int* match) {
  if (!match_args_ok(h, truth_pose, truth_lm, n_map, max_dist, out)) return EKF_E_ARG;
  return eval_run(h, {truth_pose, truth_lm, nullptr, 0, nullptr, n_map, frame}, true, max_dist,
                  out, match_out, match);
}

int ekf_eval_summary(const ekf_eval_rec* recs, int nf, ekf_eval_sum* out) {
  if (!recs || !out || nf < 1) return EKF_E_ARG;
  const double chi2_3_95 = 7.814727903251179, nan = std::nan("");
  double nees = 0.0, pos_sq = 0.0, head_sq = 0.0, lm_sq = 0.0, lm_nees = 0.0;
  long long n_pose = 0, in_95 = 0, n_eval = 0, n_nees = 0;
  for (int i = 0; i < nf; ++i) {
    const ekf_eval_rec& r = recs[i];
    if (std::isfinite(r.pose_nees)) {
      n_pose += 1;
      nees += r.pose_nees;
      in_95 += r.pose_nees <= chi2_3_95;
    }
    head_sq += r.pose_err[0] * r.pose_err[0];
    pos_sq += r.pose_err[1] * r.pose_err[1] + r.pose_err[2] * r.pose_err[2];
    lm_sq += r.lm_sq_err;
    lm_nees += r.lm_nees;
    n_eval += r.n_eval;
    n_nees += r.n_nees;
  }
  out->n = nf;
  out->n_pose_nees = static_cast<int>(n_pose);
  out->anees_pose = n_pose ? nees / n_pose : nan;
  out->pose_in_95 = n_pose ? static_cast<double>(in_95) / n_pose : nan;
  out->pos_rmse = std::sqrt(pos_sq / nf);
  out->heading_rmse = std::sqrt(head_sq / nf);
  out->lm_rmse = n_eval ? std::sqrt(lm_sq / n_eval) : nan;
  out->anees_lm = n_nees ? lm_nees / n_nees : nan;
  return EKF_OK;
}

int ekf_profile_enable(ekf_t h, int enable) {
  if (!h) return EKF_E_ARG;
  h->prof = enable != 0;
  return EKF_OK;
}

int ekf_profile_read(ekf_t h, int kind, long long* launches, double* total_ms) {
  if (!h || kind < 0 || kind >= kProfSlots) return EKF_E_ARG;
  if (int rc = settle(h)) return rc;
  auto& pe = h->pe[kind];
  for (size_t i = 0; i < pe.start.size(); ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pe.start[i].get(), pe.stop[i].get()) == hipSuccess)
      h->prof_ms[kind] += ms;
    h->prof_launches[kind] += 1;
    h->pool.push_back(std::move(pe.start[i]));
    h->pool.push_back(std::move(pe.stop[i]));
  }
  pe.start.clear();
  pe.stop.clear();
  if (kind == kProfChain) {  // a chain launch walks several chunks: report per chunk
    h->prof_launches[kProfChain] = h->prof_chunks;
    h->prof_chunks = 0;
  }
  if (launches) *launches = h->prof_launches[kind];
  if (total_ms) *total_ms = h->prof_ms[kind];
  h->prof_launches[kind] = 0;
  h->prof_ms[kind] = 0.0;
  return EKF_OK;
}

double ekf_normalize_angle(double rad) { return normalize_angle(rad); }

int ekf_debug_poison_lds(int device) {
  if (hipSetDevice(device) != hipSuccess) return EKF_E_HIP;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
    return EKF_E_HIP;
  // a quiet NaN with a payload: NaN·0 = NaN, so any product with unwritten LDS poisons the result
  const unsigned long long nan = 0x7ff8dead0000beefull;
  if (launch_poison_lds(nan, 12 * (cus > 0 ? cus : 256), nullptr) != hipSuccess) return EKF_E_HIP;
  return hipDeviceSynchronize() == hipSuccess ? EKF_OK : EKF_E_HIP;
}

#ifdef EKF_DIAG_STAMPS
int ekfslam_diag_read_stamps(unsigned long long* out, int n);  // ekf_chain.hip
// dev only (libekfslam_diag.so): the chain kernel's s_memtime stamps of filter 0's last chunk
int ekf_diag_stamps(unsigned long long* out, int n) { return ekfslam_diag_read_stamps(out, n); }
int ekfslam_res_read_stamps(unsigned long long* out, int n);  // ekf_resident.hip
// dev only: the resident kernel's stamps (filter flo, thread 0): 6 per correction
int ekf_diag_res_stamps(unsigned long long* out, int n) { return ekfslam_res_read_stamps(out, n); }
extern "C" int ekfslam_diag_read_am_stamps(unsigned long long* out);  // ekf_assoc.hip
// dev only: k_assoc_msg's s_memrealtime stamps, [2 workgroups][kMaxChunk + 1][8]
int ekf_diag_am_stamps(unsigned long long* out) { return ekfslam_diag_read_am_stamps(out); }
#endif

double ekf_sigma_pass_bytes(ekf_t h, int nf) {
  if (!h) return 0.0;
  const double n = h->n;
  // fp64: the symmetric pass (k_sigma_pass, SigmaTile64) reads the upper triangle of Σ_in only
  const double elems = h->w == 8 ? n * (n + 1) / 2 + n * n : 2.0 * n * n;
  return elems * static_cast<double>(h->w) * nf;
}

}  // extern "C"
