// The scheduler of the runtime behind include/ekf.h: the handle's two HIP streams and their CU
// masks, the upload ring, and the launch sequence of a plan (ekf_plan.hpp) — host-planned (flush)
// or written on the device (ekf_replay_device, run_device_plan) — and the resident path's replay
// from device inputs, which needs no plan at all (ekf_replay_resident).
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "ekf_ctx.hpp"
#include "ekf_internal.hpp"

namespace ekfslam {

namespace {

template <typename T>
PassArgs<T> args(ekf_ctx* h, const MsgDesc* desc, int f0) {
  PassArgs<T> a{};
  a.sig[0] = static_cast<T*>(h->sig[0].get());
  a.sig[1] = static_cast<T*>(h->sig[1].get());
  a.sig_stride = h->sig_stride;
  a.x[0] = h->x[0].get();
  a.x[1] = h->x[1].get();
  a.x_stride = h->x_stride;
  a.kcat = static_cast<T*>(h->kcat.get());
  a.mcat = static_cast<T*>(h->mcat.get());
  a.km_stride = h->km_stride;
  a.ldk = h->ldk;
  a.ctl = h->ctl.get();
  a.rec = h->rec.get();
  a.rec_stride = static_cast<size_t>(h->F);
  a.stage = static_cast<StageRec<T>*>(h->stage.get());
  a.sync = h->sync.get();
  a.fatal = h->fatal_d;
  a.desc = desc;
  a.n = h->n;
  a.ld = h->ld;
  a.N = h->cfg.n_landmarks;
  a.f0 = f0;
  a.q = h->cfg.q_noise;
  a.r = h->cfg.r_noise;
  a.gate = h->cfg.mah_gate;
  a.joseph = h->plan.joseph() ? 1 : 0;
  a.chain_fast = h->chain_fast ? 1 : 0;
  a.trace = h->trace.get();
  a.trace_n = h->trace_n.get();
  a.trace_cap = h->trace_cap;
  return a;
}

// Main waits for everything issued to the bulk stream so far.
int join_bulk(ekf_ctx* h) {
  if (hipEventRecord(h->ev_join.get(), h->bulk.get()) != hipSuccess ||
      hipStreamWaitEvent(h->stream.get(), h->ev_join.get(), 0) != hipSuccess)
    return EKF_E_HIP;
  return EKF_OK;
}

// Bulk waits for everything issued to the main stream so far.
int fork_bulk(ekf_ctx* h) {
  HIPCHK(hipEventRecord(h->ev_chain.get(), h->stream.get()));
  HIPCHK(hipStreamWaitEvent(h->bulk.get(), h->ev_chain.get(), 0));
  return EKF_OK;
}

// ... and the main stream counts as clean: the bulk stream is ordered after all of it.
int fork_bulk_clean(ekf_ctx* h) {
  if (fork_bulk(h)) return EKF_E_HIP;
  h->main_dirty = false;
  h->main_unordered = false;
  return EKF_OK;
}

// The main stream runs the chains back to back; the bulk stream runs each chunk's factors and Σ
// pass. With disjoint CU masks (devsync) the two streams synchronise on the device only: a chain
// polls the Σ-pass epoch (it needs the pass two launches back: Σ_in and x of the chunk before the
// previous one, and this parity's ChunkRec free again), the factor kernel polls its filter's chain
// epoch. A hipStreamWaitEvent hop between the queues costs 6–12 µs, a device poll ≈ 1–2 µs.
// Without the CU split a spinning factor grid could hold every CU the chain needs, so events are
// used instead (the kernels' polls are then satisfied on arrival).
// `nchunks` consecutive chunks of filters [f0, f0+nf) (descriptors dptr[i·nf + k]): ONE chain
// launch that walks them all (rebuilding its block from the chunk before each time), then per chunk the factor
// kernel and the Σ pass on the bulk stream. More than one chunk only with devsync, where the bulk
// kernels of chunk i wait on the device for the chain's epoch of chunk i.
// L: the group's launches in the host plan (nullptr: descriptors written on the device).
// nolook: some active filter's first chunk gathers its own Σ_in (no kLook rebuild)
// publish_end: the group's last Σ pass publishes its device epoch (false only for a flush's last
// launch, whose successor the next flush orders on the host: one kernel less on the stream's tail)
// stage_hint (device-written descriptors): the group's first stage_hint chunks may stage rebuild
// operands (kStageOut), so only they are followed by the staging kernel
template <typename T>
int launch_group(ekf_ctx* h, const MsgDesc* dptr, const Launch* L, int f0, int nf, int nchunks,
                 bool pipelined, bool nolook, bool publish_end, int stage_hint) {
  PassArgs<T> a = args<T>(h, dptr, f0);
  a.desc_stride = nf;
  const unsigned s0 = static_cast<unsigned>(h->seq);
  a.seq = s0;
  const bool two = pipelined && !h->serial;
  hipStream_t ms = h->stream.get(), bs = two ? h->bulk.get() : h->stream.get();
  a.polls = two && h->devsync ? 1 : 0;
  a.need_plan = a.polls ? h->need_plan : 0u;
  h->need_plan = 0;
  a.first_ready = h->epoch_owed ? 1 : 0;  // (the host joined the bulk stream since that pass)
  {  // dev A/B: stream-ordered chains gather their (complete) Σ_in instead of rebuilding
    static const bool g = [] {
      const char* e = std::getenv("EKF_SERIAL_GATHER");
      return e && std::atoi(e) != 0;
    }();
    a.gather = g && ms == bs && !a.polls ? 1 : 0;
  }
  if (pipelined && !nolook) {
    // events: a rebuilding (kLook) chain needs the Σ pass two launches back
    if (!h->devsync) HIPCHK(hipStreamWaitEvent(ms, h->ev_sig[s0 & 1].get(), 0));
  } else if (!a.polls) {
    // a chain that gathers its own Σ_in needs the previous pass: everything on the bulk stream
    if (join_bulk(h)) return EKF_E_HIP;
  }
  int rc = timed(h, kProfChain, [&](hipEvent_t e0, hipEvent_t e1) {
    return launch_chain<T>(a, nf, nchunks, ms, e0, e1);
  });
  if (rc) return rc;
  if (h->prof) h->prof_chunks += nchunks;
  if (two && !h->devsync && fork_bulk(h)) return EKF_E_HIP;  // nchunks == 1 here
  for (int i = 0; i < nchunks; ++i) {
    PassArgs<T> ai = a;
    ai.desc = dptr + static_cast<size_t>(i) * nf;
    ai.seq = s0 + static_cast<unsigned>(i);
    // Inside a device-synchronised group the factor kernel of chunk i publishes the Σ-pass epoch
    // of chunk i−1 (the kernel boundary has made that pass's output visible): one launch less per
    // chunk on the bulk stream. The group's last pass gets its own epoch kernel.
    const bool in_group = h->devsync && nchunks > 1;
    ai.pub_sigma = in_group && i > 0 ? ai.seq : 0u;
    // factors gather the materialised Σ_in (the previous Σ pass, same stream) and the record
    rc = timed(h, kProfFactors, [&](hipEvent_t e0, hipEvent_t e1) {
      return launch_factors<T>(ai, nf, bs, e0, e1);
    });
    if (rc) return rc;
    // some filter stages the rebuild operands of its chunk after next (device-written descriptors:
    // the caller's hint — the group's first stage_hint chunks may, the last two of a device replay
    // have no chunk after next in it — the staging kernel reads every descriptor's own flags)
    const bool stage = L ? L[i].stage : i < stage_hint;
    const bool last = i + 1 == nchunks;
    rc = timed(h, kProfSigma, [&](hipEvent_t e0, hipEvent_t e1) {
      return launch_sigma_pass<T>(ai, nf, last ? publish_end : !in_group, stage, bs, e0, e1);
    });
    if (rc) return rc;
    if (!h->devsync) HIPCHK(hipEventRecord(h->ev_sig[(s0 + i) & 1].get(), bs));
  }
  h->seq += nchunks;
  h->epoch_owed = a.polls && !publish_end;
  return EKF_OK;
}

int group(ekf_ctx* h, const MsgDesc* dptr, const Launch* L, int f0, int nf, int nchunks,
          bool pipelined, bool nolook = true, bool publish_end = true, int stage_hint = 0) {
  return by_dtype(h, [&](auto tag) {
    return launch_group<decltype(tag)>(h, dptr, L, f0, nf, nchunks, pipelined, nolook, publish_end,
                                       stage_hint);
  });
}

// T chunks of all filters whose descriptors dd[t·F + f] a device planner wrote: one
// device-synchronised group, else one group per message.
// staged: the planner stages (kStageOut) for chunks two on inside these T: kStageOut needs next2
int issue_device_chunks(ekf_ctx* h, const MsgDesc* dd, int T, bool publish_end, bool staged) {
  int rc = EKF_OK;
  if (h->devsync && !h->serial) {
    rc = group(h, dd, nullptr, 0, h->F, T, true, true, publish_end, staged ? T - 2 : 0);
  } else {
    // Events: a chunk t ≥ 1 needs the Σ pass two back (kLook), or — no message of its filter
    // earlier in this replay — the passes before the replay, which the first chunk's join covers:
    // the wait on the pass two back suffices, and the chain of t runs beside the factor kernel and
    // Σ pass of t − 1 where the CUs allow (not a join of the whole bulk stream per message)
    for (int t = 0; t < T && !rc; ++t)
      rc = group(h, dd + static_cast<size_t>(t) * h->F, nullptr, 0, h->F, 1, true, t == 0, true,
                 staged && t + 2 < T ? 1 : 0);
  }
  h->main_dirty = true;
  return rc;
}

// devsync: k_assoc waits on the device for the last Σ pass (its epoch is h->seq) instead of the
// main stream joining the bulk stream first
int assoc(ekf_ctx* h, const MsgDesc* dptr, int f0, int nf, bool poll) {
  return by_dtype(h, [&](auto tag) -> int {
    using T = decltype(tag);
    PassArgs<T> a = args<T>(h, dptr, f0);
    a.polls = poll ? 1 : 0;
    a.need_sigma = poll ? static_cast<unsigned>(h->seq) : 0u;
    return timed(h, kProfAssoc, [&](hipEvent_t e0, hipEvent_t e1) {
      return launch_assoc<T>(a, nf, h->stream.get(), e0, e1);
    });
  });
}

// Which path unknown association takes (EKF_ASSOC_*). k_assoc_msg's G workgroups per filter spin
// on each other's granules, so all G must be resident at once on the CUs of the stream it runs on
// (the bulk stream; the main stream with EKF_SERIAL, whose CU mask may be narrower): G workgroups
// on one XCD (XCD-local placement) or ⌈G / 8⌉ on each (agent placement). A launch holds only as
// many filters as the CUs hold at once (assoc_msg_group: co-resident by construction). Beyond
// that the markers go one per launch (k_assoc + a launch pair).
int assoc_cus_per_xcd(const ekf_ctx* h) {
  return h->serial && h->main_cus_per_xcd > 0 ? h->main_cus_per_xcd : h->bulk_cus_per_xcd;
}

// k_assoc_msg's tables and granules for every filter (once; zeroed so no stale tag matches)
int ensure_am(ekf_ctx* h) {
  if (h->am.hist) return EKF_OK;  // (set below, once all three buffers and the memset succeeded)
  const int G = (h->cfg.n_landmarks + kAmSlots - 1) / kAmSlots;
  const size_t Np = static_cast<size_t>(G) * kAmSlots, F = static_cast<size_t>(h->F);
  AmArgs b{};
  b.G = G;
  b.hist_stride = kMaxChunk * Np;
  b.cur_stride = (kMaxChunk + 1) * Np;
  b.gran_stride = static_cast<size_t>(kMaxChunk + 1) * G * 4;
  b.xcd = h->am_route == EKF_ASSOC_CHUNK_XCD ? 1 : 0;
  b.prior = h->cfg.init_var;
  b.spin = 1u << 22;  // ≈ 0.1 s of polls per exchange
  if (const char* e = std::getenv("EKF_AM_SPIN_LOG2")) b.spin = 1u << std::min(std::atoi(e), 30);
  if (const char* e = std::getenv("EKF_AM_DROP")) b.drop = std::atoi(e) != 0 ? 1 : 0;
  if (h->am_hist.reserve(b.hist_stride * F) || h->am_cur.reserve(b.cur_stride * F) ||
      h->am_gran.reserve(b.gran_stride * F))
    return reset_all(h->am_hist, h->am_cur, h->am_gran);
  b.hist = h->am_hist.get();
  b.cur = h->am_cur.get();
  b.gran = h->am_gran.get();
  HIPCHK(hipMemset(b.gran, 0, sizeof(unsigned long long) * b.gran_stride * F));
  h->am = b;
  for (int jv = 0; jv < 2; ++jv) {
    const int slots_x =
        assoc_msg_blocks_per_cu(h->cfg.dtype == EKF_F32, jv != 0) * assoc_cus_per_xcd(h);
    (jv ? h->am_group_j : h->am_group) =
        b.xcd ? 8 * std::max(1, slots_x / G) : std::max(1, 8 * slots_x / G);
  }
  return EKF_OK;
}

// One association chunk per filter of [f0, f0+nf) (descriptors dptr), then its Σ pass, both on the
// bulk stream (the pass's CUs; the main stream's chains are not involved). The bulk stream joins
// the main stream first if the latter ran anything since (a chain wrote t_map_odom there).
int assoc_msg_group(ekf_ctx* h, const MsgDesc* dptr, int f0, int nf, bool publish_end) {
  if (int rc = ensure_am(h)) return rc;
  hipStream_t bs = h->serial ? h->stream.get() : h->bulk.get();
  if (!h->serial && h->main_dirty && fork_bulk_clean(h)) return EKF_E_HIP;
  const unsigned seq = static_cast<unsigned>(h->seq);
  // A filter's G workgroups spin on each other, so a launch holds only as many filters as the
  // stream's CUs hold at once (workgroups are not guaranteed to be dispatched in order): XCD-local
  // placement ⌊slots per XCD / G⌋ filters on each of the 8 XCDs (filter k of a launch on XCD
  // k mod 8), agent placement ⌊slots / G⌋ filters spread over all of them. Filters are
  // independent, so any grouping gives the same bits.
  const int group_nf = h->plan.joseph() ? h->am_group_j : h->am_group;
  const int rc = by_dtype(h, [&](auto tag) -> int {
    using T = decltype(tag);
    PassArgs<T> a = args<T>(h, dptr, f0);
    a.seq = seq;
    a.polls = h->devsync && !h->serial ? 1 : 0;
    for (int g0 = 0; g0 < nf; g0 += group_nf) {
      PassArgs<T> ag = args<T>(h, dptr + g0, f0 + g0);
      ag.seq = a.seq;
      ag.polls = a.polls;
      const int gn = std::min(group_nf, nf - g0);
      const int rc = timed(h, kProfAssoc, [&](hipEvent_t e0, hipEvent_t e1) {
        return launch_assoc_msg<T>(ag, h->am, gn, bs, e0, e1);
      });
      if (rc) return rc;
    }
    return timed(h, kProfSigma, [&](hipEvent_t e0, hipEvent_t e1) {
      return launch_sigma_pass<T>(a, nf, publish_end, false, bs, e0, e1);
    });
  });
  if (rc) return rc;
  if (!h->devsync) HIPCHK(hipEventRecord(h->ev_sig[seq & 1].get(), bs));
  h->seq += 1;
  h->epoch_owed = h->devsync && !h->serial && !publish_end;
  return EKF_OK;
}

int posterior_launch(ekf_ctx* h, const MsgDesc* dp, int f0, int nf) {
  const hipError_t e = by_dtype(h, [&](auto tag) {
    using T = decltype(tag);
    return launch_posterior<T>(args<T>(h, dp, f0), nf, h->stream.get());
  });
  return e == hipSuccess ? EKF_OK : EKF_E_HIP;
}

// Upload capacity for `need` descriptors. The device buffer grows geometrically (a re-allocation
// drains both streams). The pinned ring — host-planned uploads only, so ekf_replay_device never
// grows it — grows EVERY slot together, so an allocation happens the first time a plan this large
// is seen, never on a later same-sized call that lands on a ring slot not used before (a
// pinned allocation costs ≈ 120 µs, a device re-allocation a drain: round 3 measured both inside a
// 20-message bench region). Host plans are flushed every kFlushDesc descriptors (plus one
// message), which bounds the ring.
int reserve_device(ekf_ctx* h, size_t need) {
  if (need <= h->ddesc.capacity()) return EKF_OK;
  if (drain(h)) return EKF_E_HIP;  // the previous launch may still read the old buffer
  return h->ddesc.reserve(need, 2 * h->ddesc.capacity());
}

// The next pinned staging slot, once the device is done with its last upload.
int next_slot(ekf_ctx* h, StageSlot** out) {
  StageSlot& sl = h->ring[h->ring_next];
  h->ring_next = (h->ring_next + 1) % kRing;
  if (sl.used) HIPCHK(hipEventSynchronize(sl.ev.get()));
  *out = &sl;
  return EKF_OK;
}

// Resident path: the plan's descriptors and its entry list (packed behind them, in MsgDesc-sized
// slots) go up with one copy, then ONE kernel launch runs the whole plan, a workgroup per filter.
int flush_resident(ekf_ctx* h) {
  const std::vector<MsgDesc>& pd = h->plan.desc();
  const std::vector<Launch>& pl = h->plan.launches();
  const size_t nd = pd.size(), nl = pl.size();
  if (nl == 0) return EKF_OK;
  const size_t pslots = (nl * sizeof(PlanEntry) + sizeof(MsgDesc) - 1) / sizeof(MsgDesc);
  const size_t ns = nd + pslots;
  if (int rc = reserve_upload(h, ns)) return rc;
  StageSlot* slp = nullptr;
  if (int rc = next_slot(h, &slp)) return rc;
  StageSlot& sl = *slp;
  std::memcpy(sl.p.get(), pd.data(), nd * sizeof(MsgDesc));
  PlanEntry* pe = reinterpret_cast<PlanEntry*>(sl.p.get() + nd);
  int flo = INT_MAX, fhi = 0;
  for (size_t i = 0; i < nl; ++i) {
    const Launch& L = pl[i];
    pe[i] = PlanEntry{static_cast<int>(L.off), L.f0, L.nf, L.kind};
    flo = std::min(flo, L.f0);
    fhi = std::max(fhi, L.f0 + L.nf);
  }
  HIPCHK(hipMemcpyAsync(h->ddesc.get(), sl.p.get(), ns * sizeof(MsgDesc), hipMemcpyHostToDevice,
                        h->stream.get()));
  HIPCHK(hipEventRecord(sl.ev.get(), h->stream.get()));
  sl.used = true;
  const PassArgs<double> a = args<double>(h, h->ddesc.get(), 0);
  const PlanEntry* dplan = reinterpret_cast<const PlanEntry*>(h->ddesc.get() + nd);
  const int rc = timed(h, kProfResident, [&](hipEvent_t e0, hipEvent_t e1) {
    return launch_resident(a, dplan, static_cast<int>(nl), flo, fhi - flo, h->stream.get(), e0, e1);
  });
  h->plan.clear();
  return rc;
}

// The device replays' planning state: two device copies (ping-pong by dstate_cur) and the pinned
// host copy, allocated at the first device replay.
int ensure_plan_state(ekf_ctx* h) {
  const size_t F = static_cast<size_t>(h->F);
  if (h->hstate.capacity() >= F) return EKF_OK;  // (reserved last: all three are there)
  if (h->dstate[0].reserve(F) || h->dstate[1].reserve(F) || h->hstate.reserve(F))
    return reset_all(h->dstate[0], h->dstate[1], h->hstate);
  return EKF_OK;
}

// The host mirror goes down once, on the stream the device planner runs on; later device replays
// chain on the device.
int export_plan_state(ekf_ctx* h, hipStream_t ps) {
  if (h->dev_plan) return EKF_OK;
  h->plan.export_state(h->hstate.get());
  HIPCHK(hipMemcpyAsync(h->dstate[h->dstate_cur].get(), h->hstate.get(), h->F * sizeof(PlanState),
                        hipMemcpyHostToDevice, ps));
  h->dev_plan = true;
  return EKF_OK;
}

// A replay's odometry from the host (lm_replay_into, lm_replay_resident): `no` doubles into the
// handle's pinned staging, once the last upload has left it (stage_odom), then onto the device on
// the stream that reads it (upload_odom).
int stage_odom(ekf_ctx* h, const double* host_odom, size_t no) {
  if (int rc = h->ev_odom.create()) return rc;
  if (no > h->odom_h.capacity()) {  // (reserved last: both hold this much)
    if (drain(h)) return EKF_E_HIP;  // a kernel in flight may still read the old buffer
    const size_t floor = static_cast<size_t>(3 * 64) * h->F;
    reset_all(h->odom_d, h->odom_h);  // (both freed before either is allocated, as ever)
    if (h->odom_d.reserve(no, floor) || h->odom_h.reserve(no, floor))
      return reset_all(h->odom_d, h->odom_h);
  } else {
    HIPCHK(hipEventSynchronize(h->ev_odom.get()));  // the last upload has left the staging
  }
  std::memcpy(h->odom_h.get(), host_odom, no * sizeof(double));
  return EKF_OK;
}

int upload_odom(ekf_ctx* h, size_t no, hipStream_t ps) {
  HIPCHK(hipMemcpyAsync(h->odom_d.get(), h->odom_h.get(), no * sizeof(double),
                        hipMemcpyHostToDevice, ps));
  HIPCHK(hipEventRecord(h->ev_odom.get(), ps));
  return EKF_OK;
}

// Deferred submission (ekf_defer): callbacks append to the plan, which goes up with ONE upload and
// runs as one resident launch (or one pipelined run) once it is large or the caller synchronises.
constexpr size_t kFlushDesc = 8192;

}  // namespace

// The chain → factors kernels of a message are a latency-bound critical path; the Σ pass of the
// previous chunk runs beside them on the bulk stream and, sharing their CUs, slowed the chain by
// ~35 %. With few filters the two streams get disjoint CU masks: the main stream kCuSplit CUs per
// XCD, the bulk stream the rest (a CU mask must leave every XCD at least one CU; mask bit b lands on
// XCD b mod 8). EKF_CU_SPLIT=<CUs per XCD> overrides, 0 disables.
constexpr int kCuSplit = 4;

int create_streams(ekf_ctx* h) {
  int split = h->F <= kCuSplitMaxFilters ? kCuSplit : 0;
  if (const char* e = std::getenv("EKF_CU_SPLIT")) split = std::atoi(e);
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->cfg.device) !=
      hipSuccess)
    cus = 0;
  constexpr int kXcd = 8;
  h->bulk_cus_per_xcd = cus / kXcd;
  if (split > 0 && cus % kXcd == 0 && split * kXcd < cus) {
    h->bulk_cus_per_xcd = cus / kXcd - split;
    h->main_cus_per_xcd = split;
    const int words = (cus + 31) / 32;
    std::vector<uint32_t> mmain(words, 0), mbulk(words, 0);
    for (int b = 0; b < cus; ++b) (b < split * kXcd ? mmain : mbulk)[b / 32] |= 1u << (b % 32);
    hipStream_t sm = nullptr, sb = nullptr;
    const bool main_ok = hipExtStreamCreateWithCUMask(&sm, words, mmain.data()) == hipSuccess;
    if (main_ok) h->stream.adopt(sm);  // (without its twin, create() below replaces it)
    if (main_ok && hipExtStreamCreateWithCUMask(&sb, words, mbulk.data()) == hipSuccess) {
      h->bulk.adopt(sb);
      // device-epoch hand-offs by default; EKF_DEVSYNC=0 synchronises the streams with events
      // (same kernels, one chain launch per chunk: bit-identical to the single-stream order)
      // A persistent multi-chunk chain launch needs every filter's chain resident at once (a
      // chain's chunk i+2 waits for the Σ pass of chunk i over ALL filters, whose factor kernels
      // wait for every chain): with more filters than main-stream CUs it would spin into its
      // timeouts, so such a split synchronises with events.
      const char* e = std::getenv("EKF_DEVSYNC");
      h->devsync = !(e && std::atoi(e) == 0) && h->F <= split * kXcd;
      return EKF_OK;
    }
  }
  if (h->stream.create(hipStreamNonBlocking) || h->bulk.create(hipStreamNonBlocking))
    return EKF_E_HIP;
  return EKF_OK;
}

int am_route(ekf_ctx* h, bool joseph) {
  if (h->resident || !h->assoc_msg) return EKF_ASSOC_MARKER;
  const int G = (h->cfg.n_landmarks + kAmSlots - 1) / kAmSlots;
  const int per_xcd =
      assoc_msg_blocks_per_cu(h->cfg.dtype == EKF_F32, joseph) * assoc_cus_per_xcd(h);
  const char* e = std::getenv("EKF_AM_XCD");  // EKF_AM_XCD=0: the agent placement only
  if (G > 1 && G <= per_xcd && !(e && std::atoi(e) == 0)) return EKF_ASSOC_CHUNK_XCD;
  if ((G + 7) / 8 <= per_xcd) return EKF_ASSOC_CHUNK;
  return EKF_ASSOC_MARKER;
}

// Both streams idle (before host reads/writes of device state).
int drain(ekf_ctx* h) {
  HIPCHK(hipStreamSynchronize(h->bulk.get()));
  HIPCHK(hipStreamSynchronize(h->stream.get()));
  return EKF_OK;
}

int reserve_upload(ekf_ctx* h, size_t need) {
  if (int rc = reserve_device(h, need)) return rc;
  const size_t ring_cap = h->ring[kRing - 1].p.capacity();  // (reserved last: every slot's)
  if (need <= ring_cap) return EKF_OK;
  const size_t floor = std::min(2 * ring_cap, h->ddesc.capacity());
  for (StageSlot& sl : h->ring) {  // no upload in flight reads a slot that is freed below
    if (sl.used) HIPCHK(hipEventSynchronize(sl.ev.get()));
    sl.used = false;
  }
  for (StageSlot& sl : h->ring)
    if (sl.p.reserve(need, floor)) {
      for (StageSlot& o : h->ring) o.p.reset();  // all or nothing: the guard reads one slot
      return EKF_E_NOMEM;
    }
  return EKF_OK;
}

int init_diag(ekf_ctx* h, void* sig0, int nf) {
  const hipError_t e = by_dtype(h, [&](auto tag) {
    using T = decltype(tag);
    return launch_init_diag<T>(static_cast<T*>(sig0), h->sig_stride, h->n, h->ld, h->cfg.init_var,
                               nf, h->stream.get());
  });
  return e == hipSuccess ? EKF_OK : EKF_E_HIP;
}

// Upload the whole plan with one copy, then enqueue its launches in order.
int flush(ekf_ctx* h) {
  if (h->resident) return flush_resident(h);
  const std::vector<Launch>& pl = h->plan.launches();
  const size_t nd = h->plan.desc().size();
  if (nd == 0) return EKF_OK;
  if (int rc = reserve_upload(h, nd)) return rc;
  StageSlot* slp = nullptr;
  if (int rc = next_slot(h, &slp)) return rc;
  StageSlot& sl = *slp;
  std::memcpy(sl.p.get(), h->plan.desc().data(), nd * sizeof(MsgDesc));
  if (join_bulk(h)) return EKF_E_HIP;  // the bulk stream may still read descriptors
  HIPCHK(hipMemcpyAsync(h->ddesc.get(), sl.p.get(), nd * sizeof(MsgDesc), hipMemcpyHostToDevice,
                        h->stream.get()));
  // the bulk stream reads these descriptors too: one main → bulk hop per upload
  if (fork_bulk_clean(h)) return EKF_E_HIP;
  HIPCHK(hipEventRecord(sl.ev.get(), h->stream.get()));
  sl.used = true;
  int rc = EKF_OK;
  const size_t nl = pl.size();
  for (size_t li = 0; li < nl && !rc;) {
    const Launch& L = pl[li];
    const MsgDesc* dp = h->ddesc.get() + L.off;
    if (L.kind == kLaunchKnown) {  // a run of known-association chunks → one persistent chain launch
      size_t lj = li + 1;
      if (h->devsync && !h->serial)  // the bulk kernels must run beside the chain launch
        while (lj < nl && pl[lj].kind == kLaunchKnown && pl[lj].f0 == L.f0 && pl[lj].nf == L.nf &&
               pl[lj].off == pl[lj - 1].off + L.nf)
          ++lj;
      rc = group(h, dp, &L, L.f0, L.nf, static_cast<int>(lj - li), true, L.nolook, lj < nl);
      h->main_dirty = true;
      li = lj;
      continue;
    }
    if (L.kind == kLaunchAssocChunk) {
      // the pass's epoch is for another stream's consumer: the next association chunk runs on
      // the same (bulk) stream, behind the pass in stream order, so a run of them publishes once,
      // after its last pass (an epoch kernel per chunk cost ≈ 4.5 µs of each 106 µs chunk)
      rc = assoc_msg_group(h, dp, L.f0, L.nf,
                           li + 1 < nl && pl[li + 1].kind != kLaunchAssocChunk);
      ++li;
      continue;
    }
    if (L.kind == kLaunchAssoc) {
      // (an owed epoch: k_assoc cannot poll it; the flush's start joined the bulk stream anyway)
      const bool poll = h->devsync && !h->serial && !h->epoch_owed;
      if (!poll && join_bulk(h)) return EKF_E_HIP;
      rc = assoc(h, dp, L.f0, L.nf, poll);
      // the chunk's factors and Σ pass on the bulk stream (with split CU masks the main stream
      // has 4 CUs per XCD: a pass there took 33 µs against 9 at N = 1024 fp32); the next
      // association joins the bulk stream first
      if (!rc) rc = group(h, dp, &L, L.f0, L.nf, 1, true);
      h->main_dirty = true;
    }
    if (!rc && L.kind == kLaunchPosterior) {
      if (join_bulk(h)) return EKF_E_HIP;
      rc = posterior_launch(h, dp, L.f0, L.nf);
      h->main_dirty = true;
      h->main_unordered = true;  // (k_posterior reads its descriptor; no bulk work follows it)
    }
    ++li;
  }
  h->plan.clear();
  return rc;
}

bool plan_is_large(const ekf_ctx* h) { return h->plan.desc().size() >= kFlushDesc; }

int submit(ekf_ctx* h) {
  if (h->defer && !plan_is_large(h)) return EKF_OK;
  return flush(h);
}

// ekf_replay_device left the planning state on the device: bring it into the planner (behind
// everything enqueued so far) before the host plans or reads per-filter state again.
int adopt_device_plan(ekf_ctx* h) {
  if (!h->dev_plan) return EKF_OK;
  hipSetDevice(h->cfg.device);
  HIPCHK(hipMemcpyAsync(h->hstate.get(), h->dstate[h->dstate_cur].get(), h->F * sizeof(PlanState),
                        hipMemcpyDeviceToHost, h->plan_stream ? h->plan_stream : h->stream.get()));
  if (drain(h)) return EKF_E_HIP;
  h->plan.adopt(h->hstate.get());
  h->dev_plan = false;
  return EKF_OK;
}

// Before any host access to device state: run what is planned, then wait for it.
int settle(ekf_ctx* h) {
  if (int rc = flush(h)) return rc;
  if (drain(h)) return EKF_E_HIP;
  return adopt_device_plan(h);
}

// After a drain: did a device poll of this handle time out since the last report? Reported once
// (EKF_E_TIMEOUT); which filters it hit stays in their status (EKF_FLAG_TIMEOUT).
int take_fatal(ekf_ctx* h) {
  volatile unsigned* p = h->fatal_h.get();
  if (!p || *p == 0) return EKF_OK;
  *p = 0;
  return EKF_E_TIMEOUT;
}

// Association with the decisions read back (synchronous), kMaxAssoc markers per upload.
int assoc_sync(ekf_ctx* h, int f0, int nf, bool predict, bool posterior, int m_max, int* j_out,
               int* new_out) {
  const int mm = h->plan.largest(nf);
  for (int i0 = 0; i0 < mm; i0 += kMaxAssoc) {
    const int i1 = std::min(mm, i0 + kMaxAssoc);
    h->plan.unknown(f0, nf, predict, posterior && i1 == mm, i0, i1, nullptr, assoc_route(h));
    int rc = flush(h);
    if (rc) return rc;
    if (drain(h)) return EKF_E_HIP;
    for (int k = 0; k < nf; ++k) {
      FilterCtl c;
      HIPCHK(hipMemcpy(&c, h->ctl.get() + f0 + k, sizeof(FilterCtl), hipMemcpyDeviceToHost));
      const int mf = h->plan.size(k);
      for (int i = i0; i < std::min(i1, mf); ++i) {
        if (j_out) j_out[static_cast<size_t>(k) * m_max + i] = c.assoc_j[i % kMaxAssoc];
        if (new_out) new_out[static_cast<size_t>(k) * m_max + i] = c.assoc_new[i % kMaxAssoc];
      }
    }
  }
  return EKF_OK;
}

// The device's status word only accumulates (atomicOr), so a set EKF_FLAG_NUMERIC cannot show a
// second skip. The synchronous association forms therefore move that bit into a host-side word
// (reported and cleared by ekf_get_status like the device's): once before their own work, so that
// a skip of an earlier asynchronous call is not charged to them, and once after it, which tells
// whether this call skipped a marker (the oracle's -4). The device must be drained.
// *fl: the device word as read (nullable).
int take_numeric(ekf_ctx* h, int f, unsigned* fl_out) {
  unsigned fl = 0;
  HIPCHK(hipMemcpy(&fl, &h->ctl.get()[f].status, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (fl & EKF_FLAG_NUMERIC) {
    const unsigned rest = fl & ~EKF_FLAG_NUMERIC;
    HIPCHK(hipMemcpy(&h->ctl.get()[f].status, &rest, sizeof(unsigned), hipMemcpyHostToDevice));
    h->held[f] |= EKF_FLAG_NUMERIC;
  }
  if (fl_out) *fl_out = fl;
  return EKF_OK;
}

// After a synchronous form's drain: EKF_E_RANGE while the filter's status holds EKF_FLAG_RANGE
// (`range`: ekf_sensor), else EKF_E_NUMERIC if this call set EKF_FLAG_NUMERIC.
int status_rc(ekf_ctx* h, int f, bool range) {
  unsigned fl = 0;
  if (int rc = take_numeric(h, f, &fl)) return rc;
  if (range && (fl & EKF_FLAG_RANGE)) return EKF_E_RANGE;
  return (fl & EKF_FLAG_NUMERIC) ? EKF_E_NUMERIC : EKF_OK;
}

// Known-association replay whose inputs are already in device memory: the descriptors are planned
// on the GPU (plan_kernels.hip) into the upload buffer, then the same launch groups as a flush.
// The planning state (parity, previous chunk, odometry) stays on the device between such calls.
int replay_device(ekf_ctx* h, int T, int m_max, const int* d_counts, const int* d_ids,
                  const int* d_actions, const double* d_rel_xy, const double* d_odom) {
  // (Joseph form: one chunk per message too, kMaxJoseph = kMaxChunk, flagged kJoseph)
  hipSetDevice(h->cfg.device);
  if (int rc = flush(h)) return rc;  // what the host planned before runs first
  const size_t F = static_cast<size_t>(h->F);
  if (int rc = ensure_plan_state(h)) return rc;
  if (int rc = reserve_device(h, static_cast<size_t>(T) * F)) return rc;  // (no host staging)
  // device epochs: the planner runs on the bulk stream — ahead of the group's factor kernels and
  // Σ passes in stream order — and counts its descriptors, which the chain launch polls: the chain
  // starts beside the planner instead of behind a main → bulk event hop (≈ 6 µs of each replay)
  const bool beside = h->devsync && !h->serial;
  // the bulk stream may still read the last descriptors (an idle one reads nothing: no hop)
  if (hipStreamQuery(h->bulk.get()) != hipSuccess && join_bulk(h)) return EKF_E_HIP;
  // ... and the main stream: work there that the bulk stream is not ordered after (a k_posterior
  // of ekf_posterior reads its descriptor in ddesc) must end before a planner on the bulk stream
  // rewrites ddesc. (Chains are covered: the bulk stream's factor kernels follow every chain
  // through its epoch or an event, so a planner enqueued behind them runs after it.)
  if (beside && h->main_unordered) {
    if (fork_bulk(h)) return EKF_E_HIP;
    h->main_unordered = false;
  }
  hipStream_t ps = beside ? h->bulk.get() : h->stream.get();
  if (int rc = export_plan_state(h, ps)) return rc;
  ReplayArgs a{};
  a.counts = d_counts;
  a.ids = d_ids;
  a.actions = d_actions;
  a.rel = d_rel_xy;
  a.odom = d_odom;
  a.st_in = h->dstate[h->dstate_cur].get();
  a.st_out = h->dstate[h->dstate_cur ^ 1].get();
  a.desc = h->ddesc.get();
  a.T = T;
  a.joseph = h->plan.joseph() ? 1 : 0;
  a.F = h->F;
  a.M = m_max;
  a.N = h->cfg.n_landmarks;
  a.stage = h->stage.get() != nullptr;
  a.plan_count = beside ? h->sync.get() + kSyncPlan : nullptr;
  HIPCHK(launch_plan_replay(a, ps));
  h->dstate_cur ^= 1;
  h->plan_stream = ps;
  if (beside) {
    h->plan_total += static_cast<unsigned>(T) * static_cast<unsigned>(h->F);
    h->need_plan = h->plan_total;
  } else {
    // the bulk stream reads these descriptors too: one main → bulk hop (recorded before the
    // chain: behind a persistent chain launch the bulk kernels it waits for could never start)
    if (fork_bulk(h)) return EKF_E_HIP;
  }
  h->main_dirty = false;
  return issue_device_chunks(h, h->ddesc.get(), T, false, h->stage.get() != nullptr);
}

// Unknown-association replay whose inputs are already in device memory: k_plan_assoc writes the
// C = ⌈m_max / kMaxChunk⌉ chunk descriptors of every message into the upload buffer, then chunk by
// chunk the launches a host plan of kLaunchAssocChunk runs. The planner sits on the stream those
// launches run on, ahead of them in stream order, so nothing has to count its descriptors; which
// chunks are active only the device knows, and an inactive one costs its (empty) launch pair.
int replay_device_assoc(ekf_ctx* h, int T, int m_max, const int* d_counts, const double* d_xy,
                        int xy_stride, const double* d_odom, const double* host_odom,
                        hipEvent_t ready, hipEvent_t planned) {
  hipSetDevice(h->cfg.device);
  if (int rc = flush(h)) return rc;  // what the host planned before runs first
  const size_t F = static_cast<size_t>(h->F);
  const int C = (m_max + kMaxChunk - 1) / kMaxChunk;
  if (int rc = ensure_plan_state(h)) return rc;
  if (int rc = reserve_device(h, static_cast<size_t>(T) * C * F)) return rc;
  const size_t no = 3 * static_cast<size_t>(T) * F;
  if (host_odom)
    if (int rc = stage_odom(h, host_odom, no)) return rc;
  // The planner rewrites the upload buffer on the stream the association launches run on. Work on
  // that stream is ahead of it in stream order; work on the main stream that the bulk stream is
  // not ordered after yet (a chain, a k_posterior reading its descriptor) must end first: the hop a
  // host-planned association chunk takes (assoc_msg_group), taken before the planner instead.
  hipStream_t ps = h->serial ? h->stream.get() : h->bulk.get();
  if (!h->serial && (h->main_dirty || h->main_unordered) && fork_bulk_clean(h)) return EKF_E_HIP;
  if (ready) HIPCHK(hipStreamWaitEvent(ps, ready, 0));
  if (host_odom)
    if (int rc = upload_odom(h, no, ps)) return rc;
  if (int rc = export_plan_state(h, ps)) return rc;
  AssocReplayArgs a{};
  a.counts = d_counts;
  a.xy = d_xy;
  a.odom = host_odom ? h->odom_d.get() : d_odom;
  a.st_in = h->dstate[h->dstate_cur].get();
  a.st_out = h->dstate[h->dstate_cur ^ 1].get();
  a.desc = h->ddesc.get();
  a.T = T;
  a.F = h->F;
  a.M = m_max;
  a.C = C;
  a.stride = xy_stride;
  a.joseph = h->plan.joseph() ? 1 : 0;
  HIPCHK(launch_plan_assoc(a, ps));
  if (planned) HIPCHK(hipEventRecord(planned, ps));
  h->dstate_cur ^= 1;
  h->plan_stream = ps;
  // a run of association chunks publishes its Σ epoch once, behind its last pass; as the last
  // launch of a host plan, this run's last publishes none (the next flush joins the bulk stream)
  int rc = EKF_OK;
  for (size_t i = 0; i < static_cast<size_t>(T) * C && !rc; ++i)
    rc = assoc_msg_group(h, h->ddesc.get() + i * F, 0, h->F, false);
  return rc;
}

// Resident path: T messages whose inputs are in device memory, walked by ONE launch of
// k_resident_replay (ekf_resident.hip) on the main stream, the only stream a resident handle
// uses: no descriptors, no planner kernel. The planning state goes through the device copies as
// in the two replays above (the kernel leaves st_out), so adopt_device_plan works unchanged.
// host_odom / ready as replay_device_assoc's; consumed (nullable) is recorded behind the kernel,
// which reads its inputs for the whole launch.
int replay_resident(ekf_ctx* h, int assoc, int T, int m_max, const int* d_counts, const int* d_ids,
                    const int* d_actions, const double* d_xy, int xy_stride, const double* d_odom,
                    const double* host_odom, hipEvent_t ready, hipEvent_t consumed) {
  hipSetDevice(h->cfg.device);
  if (int rc = flush(h)) return rc;  // what the host planned before runs first
  if (int rc = ensure_plan_state(h)) return rc;
  const size_t no = 3 * static_cast<size_t>(T) * h->F;
  if (host_odom)
    if (int rc = stage_odom(h, host_odom, no)) return rc;
  hipStream_t ps = h->stream.get();
  if (ready) HIPCHK(hipStreamWaitEvent(ps, ready, 0));
  if (host_odom)
    if (int rc = upload_odom(h, no, ps)) return rc;
  if (int rc = export_plan_state(h, ps)) return rc;
  ResidentReplayArgs r{};
  r.counts = d_counts;
  r.ids = assoc ? nullptr : d_ids;
  r.actions = assoc ? nullptr : d_actions;
  r.xy = d_xy;
  r.odom = host_odom ? h->odom_d.get() : d_odom;
  r.st_in = h->dstate[h->dstate_cur].get();
  r.st_out = h->dstate[h->dstate_cur ^ 1].get();
  r.T = T;
  r.F = h->F;
  r.M = m_max;
  r.stride = xy_stride;
  r.assoc = assoc ? 1 : 0;
  const PassArgs<double> a = args<double>(h, nullptr, 0);
  const int rc = timed(h, kProfResident, [&](hipEvent_t e0, hipEvent_t e1) {
    return launch_resident_replay(a, r, ps, e0, e1);
  });
  // (a failed launch leaves dstate_cur where it is: the copy export_plan_state just wrote is the
  // one a later adopt_device_plan reads back, so the handle goes on from the state before the call)
  if (rc) return rc;
  if (consumed) HIPCHK(hipEventRecord(consumed, ps));
  h->dstate_cur ^= 1;
  h->plan_stream = ps;
  return EKF_OK;
}

int replay_markers(ekf_t h, int device, int T, int m_max, const int* d_counts,
                   const double* d_markers, const double* odom, hipEvent_t ready,
                   hipEvent_t planned) {
  if (!h || device != h->cfg.device || T < 1 || m_max < 1 || m_max > kMaxAssoc || !d_counts ||
      !d_markers || !odom || !device_assoc_supported(h))
    return EKF_E_ARG;
  return replay_device_assoc(h, T, m_max, d_counts, d_markers, 4, nullptr, odom, ready, planned);
}

int replay_markers_resident(ekf_t h, int device, int T, int m_max, const int* d_counts,
                            const double* d_markers, const double* odom, hipEvent_t ready,
                            hipEvent_t consumed) {
  if (!h || device != h->cfg.device || T < 1 || m_max < 1 || m_max > kMaxAssoc || !d_counts ||
      !d_markers || !odom || !h->resident)
    return EKF_E_ARG;
  return replay_resident(h, 1, T, m_max, d_counts, nullptr, nullptr, d_markers, 4, nullptr, odom,
                         ready, consumed);
}

int replay_markers_device(ekf_t h, int device, int T, int m_max, const int* d_counts,
                          const double* d_markers, const double* d_odom, hipEvent_t ready,
                          hipEvent_t planned) {
  if (!h || device != h->cfg.device || T < 1 || m_max < 1 || m_max > kMaxAssoc || !d_counts ||
      !d_markers || !d_odom || !device_assoc_supported(h))
    return EKF_E_ARG;
  return replay_device_assoc(h, T, m_max, d_counts, d_markers, 4, d_odom, nullptr, ready, planned);
}

int replay_markers_resident_device(ekf_t h, int device, int T, int m_max, const int* d_counts,
                                   const double* d_markers, const double* d_odom,
                                   hipEvent_t ready, hipEvent_t consumed) {
  if (!h || device != h->cfg.device || T < 1 || m_max < 1 || m_max > kMaxAssoc || !d_counts ||
      !d_markers || !d_odom || !h->resident)
    return EKF_E_ARG;
  return replay_resident(h, 1, T, m_max, d_counts, nullptr, nullptr, d_markers, 4, d_odom, nullptr,
                         ready, consumed);
}

int handle_info(ekf_t h, HandleInfo* out) {
  if (!h || !out) return EKF_E_ARG;
  if (int rc = flush(h)) return rc;
  hipSetDevice(h->cfg.device);
  if (join_bulk(h)) return EKF_E_HIP;  // work enqueued on the main stream next sees the bulk's done
  out->F = h->F;
  out->N = h->cfg.n_landmarks;
  out->n = h->n;
  out->dtype = h->cfg.dtype;
  out->device = h->cfg.device;
  out->resident = h->resident;
  out->joseph = h->plan.joseph();
  out->serial = h->serial;
  out->stream = h->stream.get();
  out->bulk = h->bulk.get() ? h->bulk.get() : h->stream.get();
  return EKF_OK;
}

int handle_parity(ekf_t h, int* parity) {
  if (!h || !parity) return EKF_E_ARG;
  if (int rc = adopt_device_plan(h)) return rc;
  for (int f = 0; f < h->F; ++f) parity[f] = h->plan.parity(f);
  return EKF_OK;
}

int run_device_plan(ekf_t h, const MsgDesc* dd, const PlanEntry* dplan, int T,
                    const int* parity_after, const double* odom_after) {
  if (!h || T < 0 || !dd || !parity_after || !odom_after) return EKF_E_ARG;
  hipSetDevice(h->cfg.device);
  if (int r0 = adopt_device_plan(h)) return r0;
  int rc = EKF_OK;
  if (T > 0) {
    if (h->resident) {
      const PassArgs<double> a = args<double>(h, dd, 0);
      rc = timed(h, kProfResident, [&](hipEvent_t e0, hipEvent_t e1) {
        return launch_resident(a, dplan, T, 0, h->F, h->stream.get(), e0, e1);
      });
    } else {
      // an owed Σ-pass epoch (the last flush's last pass published none): the chains take every
      // earlier pass as complete (PassArgs::first_ready), which holds once main has joined bulk
      if (h->epoch_owed && join_bulk(h)) return EKF_E_HIP;
      // the bulk stream reads these descriptors too (written on the main stream)
      if (fork_bulk(h)) return EKF_E_HIP;
      rc = issue_device_chunks(h, dd, T, true, false);
    }
  }
  h->plan.take(parity_after, odom_after);
  return rc;
}

}  // namespace ekfslam
