// On-device Monte-Carlo inputs (include/ekf_sim.h): one wavefront per filter walks a run's T
// messages in order — nusim's slipping wheels and DiffDrive::FKin truth (nusim/src/nusim.cpp:222-230,
// turtlelib/src/diff_drive.cpp:10-28) and the encoders' odometry (slam.cpp:599-634), the fake
// sensor (nusim.cpp:317-346) over the map on all 64 lanes, then the message's descriptor for the
// filter kernels (what ekf_plan.cpp's Planner::known writes on the host).
//
// FKin composes one arc per tick: config ← config · Δ_k. The ticks of a message are independent
// until that product, so lane j integrates tick j's arc and the wave composes the arcs with an
// inclusive scan (SE(2) composition is associative): log2(ticks) dependent compositions per
// message instead of one per tick. The host restatement (synth._simulate) composes tick by tick,
// so the two agree to rounding (≈1e-14 m per message), not bit for bit.
//
// Randomness is pyekf.synth's counter-based splitmix64, draw for draw: slip of wheel w at global
// tick k is uniform draw 2k + w of stream 1 under seed + f0 + f; the noise of marker i of message
// t is normal draw 2(t·M + i) (+1 for y) of stream 2. Compiled with -ffp-contract=off, so every
// product and sum rounds as numpy's does (synth.py is the host restatement this is tested against).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "ekf_device.hpp"
#include "ekf_math.hpp"
#include "geom.hpp"
#include "sim_launch.hpp"
#include "sim_rng.hpp"

namespace ekfslam {
namespace {

constexpr unsigned long long kSlipStream = 1, kNoiseStream = 2;  // synth._S_SLIP, _S_NOISE
constexpr int kSenseNearest = 0, kSenseSurvey = 1, kSenseAll = 2;
constexpr double kSurveyRange = 2.0;  // synth.SURVEY_RANGE
constexpr int kPerLane = kSimMaxMap / 64;

__device__ __forceinline__ double bcast(double v, int l) { return __shfl(v, l, 64); }

// the arc of one tick with wheel-angle increments (dl, dr) (DiffDrive::fkin's Δ)
__device__ __forceinline__ Pose2 arc(double dl, double dr, double radius, double track) {
  const Twist2 tw{radius / track * (-dl + dr), radius / 2.0 * (dl + dr), 0.0};
  return integrate_twist(tw);
}

// inclusive scan of compose over lanes 0..n−1 (lane j ends with Δ_0 · … · Δ_j)
__device__ __forceinline__ Pose2 scan_compose(Pose2 d, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const Pose2 e{__shfl_up(d.theta, o, 64), __shfl_up(d.x, o, 64), __shfl_up(d.y, o, 64)};
    if (lane >= o) d = compose(e, d);
  }
  return d;
}

struct SimShared {
  double bx[kSimMaxMap], by[kSimMaxMap];
  unsigned sighted[kSimMaxMap / 32];
  int sel[kMaxChunk];
  int ids[kMaxChunk], prev_ids[kMaxChunk];
};

// One message's wheels (nusim.cpp:222-230, slam.cpp:599-634): lane j < tpm is tick j, the wave
// composes the ticks' arcs by a scan into the message's products (true, odometry; wave-uniform),
// which the true pose and the odometry then advance by.
__device__ __forceinline__ void arc_products(const SimArgs& A, unsigned long long seed, int t,
                                             int lane, Pose2& pt, Pose2& po) {
  Pose2 dt{0.0, 0.0, 0.0}, dot{0.0, 0.0, 0.0};  // identity past the message's ticks
  if (lane < A.tpm) {
    const size_t k = static_cast<size_t>(t) * A.tpm + lane;
    const double cl = A.cmd[2 * k], cr = A.cmd[2 * k + 1];
    const unsigned long long g = static_cast<unsigned long long>(A.tick0) + k;
    const double sl = cl * (1.0 + A.slip * (2.0 * uniform(seed, kSlipStream, 2 * g) - 1.0));
    const double sr = cr * (1.0 + A.slip * (2.0 * uniform(seed, kSlipStream, 2 * g + 1) - 1.0));
    dt = arc(sl, sr, A.radius, A.track);
    dot = arc(cl, cr, A.radius, A.track);
  }
  dt = scan_compose(dt, lane);
  dot = scan_compose(dot, lane);
  const int last = A.tpm - 1;
  pt = Pose2{bcast(dt.theta, last), bcast(dt.x, last), bcast(dt.y, last)};
  po = Pose2{bcast(dot.theta, last), bcast(dot.x, last), bcast(dot.y, last)};
}
__device__ __forceinline__ void wheels(const SimArgs& A, unsigned long long seed, int t, int lane,
                                       Pose2& truth, Pose2& odo) {
  Pose2 pt, po;
  arc_products(A, seed, t, lane, pt, po);
  truth = compose(truth, pt);
  odo = compose(odo, po);
}

// ---- collisions (nusim.cpp:232-254; ekf_sim_set_collisions, include/ekf_sim.h) -----------------
// After each tick's FKin the true pose is tested against the map's cylinders in id order and pushed
// out of the first one it is inside, R = collision_radius + obstacle_radius; the wheel angles are
// not reset, so the next tick's arc composes onto the corrected pose. That makes the ticks of a
// message sequential from the first contact on, and only from there:
//  * optimistic: the arcs are scanned as without collisions, lane j forms the pose after tick j
//    as if nothing were hit, q_j = truth · (Δ_0 … Δ_j), and tests it against the message's
//    candidates. No hit in any lane: the truth advances to q_last, the expression (and the bits)
//    of `wheels`. Else the lowest hit lane j* is the first contact, and q_j* is right up to there;
//  * from the first contact: q_j* is pushed out of its lowest colliding id, then the remaining
//    ticks are walked one at a time (pose ← pose · Δ_j, the un-scanned arc of lane j), the wave
//    testing the pose with one lane per candidate, the lowest id taken with wave_argmin. Contact
//    usually lasts many ticks (the robot slides along the cylinder), so nothing is re-scanned. The
//    next message starts optimistic again.
// The arithmetic of a push is synth._simulate's, expression for expression (atan2 / cos / sin, not a
// unit vector: defined at d = 0, where the push goes along −x).
//
// The candidates (the cull), as k_lidar_scan_swarm's scene: per message, about the pose c at its
// start, with len_j an upper bound of tick j's chord (the arc's length |radius/2·(dl_j + dr_j)|; the
// computed chord where rounding makes it larger, which 1/ω in integrate_twist can at |ω| → 0),
//     ρ = (Σ_j len_j)·(1 + 2⁻²⁰),    landmark i is kept unless |c_i − c|·(1 − 2⁻²⁰) > ρ + R.
// One wave per filter, so the list's length is a wave-uniform register (no LDS atomic) and the
// list comes out in id order; the decision is a minimum over ids and does not rest on that.
// Why no decision changes, for every input: a pose p is pushed by landmark i only if the computed
// |p − c_i| < R. Between pushes the pose moves by the ticks' chords, so after tick j with no push
// since the list was built |p − c| ≤ Σ_{k ≤ j} len_k ≤ ρ, and a landmark that p can hit has
// |c_i − c| ≤ |p − c| + |p − c_i| < ρ + R: kept. The computed distances, sums and products are off
// by a few 2⁻⁵³ relative; the two margins of 2⁻²⁰ are 10⁹ times that. NaN anywhere in the test
// compares false: kept.
// A push moves the pose by up to R more than the chords account for (a start inside a cylinder,
// overlapping cylinders handing the robot from one to the next), so after every push at tick j the
// wave tests, uniformly, whether every pose of the message's remaining ticks stays in reach of
// the list:  |p − c| + Σ_{k > j} len_k ≤ ρ  (the suffix sums are a scan of non-negative terms).
// Where that fails the list is rebuilt about c = p with ρ = (Σ_{k > j} len_k)·(1 + 2⁻²⁰), for
// which the argument above starts again. So at every test the list holds every landmark the pose
// can hit, and the lowest colliding id of the list is the map's.
// Maps of fewer than cull_from landmarks (kCollideCullFromMap, sim_launch.hpp) are staged whole,
// once per run, and every test runs over all of them: no bound to keep.
constexpr double kHitMargin = 0x1p-20;

struct CollideShared {
  double cx[kSimMaxMap], cy[kSimMaxMap];  // the candidates' centres
  int id[kSimMaxMap];                     // and landmark ids
};

// The candidate list about (cx, cy): the landmarks within `reach` (ρ + R) by the test above, or
// the whole map (`cull` false). Returns its length (wave-uniform).
__device__ __forceinline__ int hit_candidates(const double* lm, int L, bool cull, double cx,
                                              double cy, double reach, CollideShared& cs, int lane) {
  __syncthreads();  // (one wave: the reads of the list it replaces are done)
  int n = 0;
  for (int c0 = 0; c0 < L; c0 += 64) {  // (the trip count is the wave's: every lane ballots)
    const int c = c0 + lane;
    double x = 0.0, y = 0.0;
    bool keep = false;
    if (c < L) {
      x = lm[2 * c];
      y = lm[2 * c + 1];
      const double dx = x - cx, dy = y - cy;
      keep = !cull || !(sqrt(dx * dx + dy * dy) * (1.0 - kHitMargin) > reach);
    }
    const unsigned long long kept = __ballot(keep);
    if (keep) {
      const int slot = n + __popcll(kept & ((1ull << lane) - 1ull));  // (≤ c < L)
      cs.cx[slot] = x;
      cs.cy[slot] = y;
      cs.id[slot] = c;
    }
    n += __popcll(kept);
  }
  __syncthreads();
  return n;
}

// the lowest id among the n candidates that (x, y) is inside, INT_MAX: none
// (d as nusim.cpp:239-240 and synth._simulate: sqrt of the sum of the rounded squares)
__device__ __forceinline__ int lowest_hit(const CollideShared& cs, int i0, int step, int n, double x,
                                          double y, double R) {
  int best = INT_MAX;
  for (int i = i0; i < n; i += step) {
    const double dx = x - cs.cx[i], dy = y - cs.cy[i];
    if (sqrt(dx * dx + dy * dy) < R) best = min(best, cs.id[i]);
  }
  return best;
}

// nusim.cpp:241-248: the pose out of landmark `id`, along the line of centres; θ kept
__device__ __forceinline__ void push_out(const double* lm, int id, double R, Pose2& p) {
  const double lx = lm[2 * id], ly = lm[2 * id + 1];
  const double dx = p.x - lx, dy = p.y - ly;
  const double d = sqrt(dx * dx + dy * dy);
  const double a = atan2(ly - p.y, lx - p.x);
  p.x = p.x - (R - d) * cos(a);
  p.y = p.y - (R - d) * sin(a);
}

// One message's wheels with collisions (`wheels` with the rule above; kOdo: the odometry too, else
// the caller has k_sim_arcs' products). `n_all`: the staged map's length where it is not culled.
// Returns the message's colliding ticks.
template <bool kOdo>
__device__ __forceinline__ int collide_wheels(const SimArgs& A, const double* lm,
                                              unsigned long long seed, int t, int lane, bool cull,
                                              int n_all, CollideShared& cs, Pose2& truth,
                                              Pose2& odo) {
  const double R = A.hit_r;
  const int last = A.tpm - 1;
  Pose2 a{0.0, 0.0, 0.0}, ao{0.0, 0.0, 0.0};  // identity past the message's ticks
  double rem = 0.0;
  if (lane < A.tpm) {  // (arc_products' expressions: the same bits)
    const size_t k = static_cast<size_t>(t) * A.tpm + lane;
    const double cl = A.cmd[2 * k], cr = A.cmd[2 * k + 1];
    const unsigned long long g = static_cast<unsigned long long>(A.tick0) + k;
    const double sl = cl * (1.0 + A.slip * (2.0 * uniform(seed, kSlipStream, 2 * g) - 1.0));
    const double sr = cr * (1.0 + A.slip * (2.0 * uniform(seed, kSlipStream, 2 * g + 1) - 1.0));
    a = arc(sl, sr, A.radius, A.track);
    if constexpr (kOdo) ao = arc(cl, cr, A.radius, A.track);
    rem = fmax(fabs(A.radius / 2.0 * (sl + sr)), sqrt(a.x * a.x + a.y * a.y));  // len_j
  }
  const Pose2 sc = scan_compose(a, lane);
  if constexpr (kOdo) {
    ao = scan_compose(ao, lane);
    odo = compose(odo, Pose2{bcast(ao.theta, last), bcast(ao.x, last), bcast(ao.y, last)});
  }
  int n = n_all;
  double ccx = truth.x, ccy = truth.y, rho = 0.0;  // the list's centre and ρ
  if (cull) {
    for (int o = 1; o < 64; o <<= 1) {  // lane j: len_j + … + len_last
      const double e = __shfl_down(rem, o, 64);
      if (lane + o < 64) rem += e;
    }
    rho = bcast(rem, 0) * (1.0 + kHitMargin);
    n = hit_candidates(lm, A.L, true, ccx, ccy, rho + R, cs, lane);
  }
  // optimistic: lane j is the pose after tick j with no contact so far
  const Pose2 q = compose(truth, sc);
  int id = lane < A.tpm ? lowest_hit(cs, 0, 1, n, q.x, q.y, R) : INT_MAX;
  const unsigned long long hit = __ballot(id != INT_MAX);
  if (hit == 0) {  // (lane last's q: compose(truth, the message's product), as `wheels`)
    truth = Pose2{bcast(q.theta, last), bcast(q.x, last), bcast(q.y, last)};
    return 0;
  }
  // from the first contact, tick j: wave-uniform from here
  int j = __ffsll(static_cast<long long>(hit)) - 1;
  Pose2 p{bcast(q.theta, j), bcast(q.x, j), bcast(q.y, j)};
  id = __shfl(id, j, 64);
  int hits = 0;
  for (;;) {
    push_out(lm, id, R, p);
    ++hits;
    if (j == last) break;
    if (cull) {
      const double left = bcast(rem, j + 1);
      const double dx = p.x - ccx, dy = p.y - ccy;
      if (!(sqrt(dx * dx + dy * dy) + left <= rho)) {  // the push broke the list's bound
        ccx = p.x;
        ccy = p.y;
        rho = left * (1.0 + kHitMargin);
        n = hit_candidates(lm, A.L, true, ccx, ccy, rho + R, cs, lane);
      }
    }
    id = INT_MAX;
    while (id == INT_MAX && j < last) {  // the ticks up to the next contact, one at a time
      ++j;
      p = compose(p, Pose2{bcast(a.theta, j), bcast(a.x, j), bcast(a.y, j)});
      if (n == 0) continue;
      id = lowest_hit(cs, lane, 64, n, p.x, p.y, R);
      double key = id == INT_MAX ? INFINITY : 0.0;
      wave_argmin(key, id);  // (key, then the lower id)
    }
    if (id == INT_MAX) break;
  }
  truth = p;
  return hits;
}

// The fake sensor of one message at the true pose (th, px, py) (nusim.cpp:317-346): every
// landmark of the map `lm` in the true body frame R(θ)ᵀ(p − x) into sh.bx / sh.by (kMap), the
// selected landmarks into sh.sel (nearest first, or id order for ALL). Returns their count k.
// Without the map (k_sim_sense: no SURVEY message) `marker` recomputes a selected landmark's body
// frame position by the same expressions (the same bits), and the wave needs 64 B of LDS, not 16 KB.
template <bool kMap = true, typename Sh>
__device__ __forceinline__ int sense(const SimArgs& A, const double* lm, int mode, double th,
                                     double px, double py, Sh& sh, int lane) {
  const int L = A.L;
  const double c = cos(th), s = sin(th);
  const double rng = mode == kSenseSurvey ? kSurveyRange * A.range : A.range;
  double key[kPerLane];
  double dmin = INFINITY;
  bool any = false;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int l = lane + 64 * j;
    key[j] = INFINITY;
    if (l < L) {
      const double dx = lm[2 * l] - px, dy = lm[2 * l + 1] - py;
      const double bx = c * dx + s * dy, by = -s * dx + c * dy;
      const double d = hypot(bx, by);
      if constexpr (kMap) {
        sh.bx[l] = bx;
        sh.by[l] = by;
      }
      dmin = fmin(dmin, d);
      double kk = d <= rng ? d : INFINITY;
      any = any || kk != INFINITY;
      if constexpr (kMap) {  // (SURVEY: a run with the map)
        if (mode == kSenseSurvey && kk != INFINITY && ((sh.sighted[l >> 5] >> (l & 31)) & 1u))
          kk = kk + 1e6;
      }
      key[j] = kk;
      if (mode == kSenseAll) key[j] = d;  // (the ADD / DELETE test below)
    }
  }
  if constexpr (kMap) __syncthreads();  // every lane's sh.bx / sh.by before the survey fallback
  int k = 0;
  if (mode == kSenseAll) {
    k = L;  // every landmark, in id order (L ≤ kMaxChunk, checked on the host)
    if (lane < L) sh.sel[lane] = lane;
  } else {
    if (kMap && mode == kSenseSurvey && !__any(any)) {  // never empty: the nearest, out of range
      for (int o = 32; o > 0; o >>= 1) dmin = fmin(dmin, __shfl_xor(dmin, o, 64));
      if constexpr (kMap) {
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
          const int l = lane + 64 * j;
          if (l < L) key[j] = hypot(sh.bx[l], sh.by[l]) == dmin ? dmin : INFINITY;
        }
      }
    }
    // the m smallest keys, ties to the lower index (synth: a stable argsort)
    unsigned taken = 0;
    for (; k < A.m; ++k) {
      double best = INFINITY;
      int bi = INT_MAX;
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) {
        const int l = lane + 64 * j;
        if (!((taken >> j) & 1u) && (key[j] < best || (key[j] == best && l < bi)) && l < L) {
          best = key[j];
          bi = l;
        }
      }
      // (smaller key, ties to the lower index: a strict total order, so the DPP tree of
      // ekf_math.hpp gives the pair the shuffle butterfly gave)
      wave_argmin(best, bi);
      if (best == INFINITY) break;  // wave-uniform
      if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
      if (lane == 0) sh.sel[k] = bi;
    }
  }
  __syncthreads();
  return k;
}

// Marker `lane` < k of message `msg`: its landmark, the noisy body-frame position (draws
// 2·(msg·M + lane) and + 1 of stream 2) and ADD / DELETE (beyond range, mode ALL).
// (kMap false: the body frame position from the map `lm` at the true pose (th, px, py), as sense)
template <bool kMap = true, typename Sh>
__device__ __forceinline__ void marker(const SimArgs& A, unsigned long long seed, long long msg,
                                       int mode, int k, const Sh& sh, int lane, int* id,
                                       int* act, double* rx, double* ry, const double* lm = nullptr,
                                       double th = 0.0, double px = 0.0, double py = 0.0) {
  *id = -1;
  *act = 0;
  *rx = *ry = 0.0;
  if (lane < k) {
    *id = sh.sel[lane];
    double bx, by;
    if constexpr (kMap) {
      bx = sh.bx[*id];
      by = sh.by[*id];
    } else {
      const double c = cos(th), s = sin(th);
      const double dx = lm[2 * *id] - px, dy = lm[2 * *id + 1] - py;
      bx = c * dx + s * dy;
      by = -s * dx + c * dy;
    }
    const unsigned long long idx = (static_cast<unsigned long long>(msg) * A.M + lane) * 2;
    *rx = bx + A.sigma * normal(seed, kNoiseStream, idx);
    *ry = by + A.sigma * normal(seed, kNoiseStream, idx + 1);
    *act = mode == kSenseAll && !(hypot(bx, by) <= A.range) ? 2 : 0;  // DELETE
  }
}

// the message's markers as ekf_replay takes them (row `rowo` = t·F + f of the record arrays)
__device__ __forceinline__ void record_markers(const SimArgs& A, size_t rowo, int k, int id,
                                               int act, double rx, double ry, int lane) {
  const int M = A.M;
  for (int i = lane; i < M; i += 64) {
    const size_t o = rowo * M + i;
    A.out_ids[o] = i < k ? __shfl(id, i, 64) : -1;
    A.out_act[o] = i < k ? __shfl(act, i, 64) : 0;
    A.out_rel[2 * o] = i < k ? __shfl(rx, i, 64) : 0.0;
    A.out_rel[2 * o + 1] = i < k ? __shfl(ry, i, 64) : 0.0;
  }
  if (lane == 0) A.out_cnt[rowo] = k;
}

}  // namespace

namespace {
// k_sim's body; kCollide: the wheels of every message under the collision rule (k_sim_collide)
template <bool kCollide>
__device__ __forceinline__ void sim_run(const SimArgs& A, SimShared& sh, CollideShared* cs) {
  const int f = blockIdx.x, lane = threadIdx.x;
  const int L = A.L;
  const unsigned long long seed = A.seed + static_cast<unsigned long long>(A.f0 + f);
  SimState& S = A.st[f];
  const double* lm = A.lm + static_cast<size_t>(f) * L * 2;
  const int words = (L + 31) / 32;
  for (int w = lane; w < words; w += 64) sh.sighted[w] = A.sighted[static_cast<size_t>(f) * words + w];
  __syncthreads();  // (one wave: order the lanes' LDS writes before any lane reads another's word)
  // the true pose (slipping wheels) and the odometry (commanded encoder angles), wave-uniform
  Pose2 truth{S.truth[0], S.truth[1], S.truth[2]};
  Pose2 odo{S.odom[0], S.odom[1], S.odom[2]};
  int par = A.par[f];
  int prev_m = -1;       // the previous active chunk of this run (−1: the run's first gathers Σ_in)
  [[maybe_unused]] long long hits = 0;
  [[maybe_unused]] bool cull = false;
  [[maybe_unused]] int n_all = 0;
  if constexpr (kCollide) {
    cull = L >= A.cull_from;
    if (!cull) n_all = hit_candidates(lm, L, false, 0.0, 0.0, 0.0, *cs, lane);
  }
  for (int t = 0; t < A.T; ++t) {
    const long long msg = A.msg0 + t;
    if constexpr (kCollide) {
      const int h = collide_wheels<true>(A, lm, seed, t, lane, cull, n_all, *cs, truth, odo);
      if (A.out_hits && lane == 0) A.out_hits[static_cast<size_t>(t) * A.F + f] = h;
      hits += h;
    } else {
      wheels(A, seed, t, lane, truth, odo);
    }
    const double th = truth.theta, px = truth.x, py = truth.y;
    const double oth = odo.theta, ox = odo.x, oy = odo.y;
    if (A.out_truth && lane < 3)
      A.out_truth[(static_cast<size_t>(t) * A.F + f) * 3 + lane] = lane == 0 ? th : (lane == 1 ? px : py);
    if (A.out_odom && f == 0 && lane < 3)
      A.out_odom[static_cast<size_t>(t) * 3 + lane] = lane == 0 ? oth : (lane == 1 ? ox : oy);
    const int mode = A.sense ? A.sense[t] : kSenseNearest;
    const int k = sense(A, lm, mode, th, px, py, sh, lane);
    // ---- markers: noise, record, descriptor ----
    const size_t rowo = static_cast<size_t>(t) * A.F + f;
    int id, act;
    double rx, ry;
    marker(A, seed, msg, mode, k, sh, lane, &id, &act, &rx, &ry);
    if (lane < k && mode == kSenseSurvey) atomicOr(&sh.sighted[id >> 5], 1u << (id & 31));
    if (A.out_ids) record_markers(A, rowo, k, id, act, rx, ry, lane);
    // the filter's chunk: the non-DELETE markers in order (slam.cpp:205), z as slam.cpp:208-210
    const bool add = lane < k && act != 2;
    const unsigned long long bal = __ballot(add);
    const int m = __popcll(bal);
    const int pos = __popcll(bal & ((1ull << lane) - 1ull));
    MsgDesc* d = A.desc + rowo;
    double* dz = reinterpret_cast<double*>(d);
    for (int e = lane; e < static_cast<int>(sizeof(MsgDesc) / 8); e += 64) dz[e] = 0.0;
    __syncthreads();
    if (k == 0) continue;  // no marker: the filter gets no message (ekf_replay's counts 0)
    if (add) {
      d->ids[pos] = id;
      sh.ids[pos] = id;
      d->z[pos][0] = sqrt(rx * rx + ry * ry);  // std::pow(x, 2) is x·x rounded
      d->z[pos][1] = atan2(ry, rx);
    }
    if (lane == 0) {
      d->m = m;
      d->flags = kActive | kFirst | kLast | (prev_m >= 0 ? kLook : 0) | (A.joseph ? kJoseph : 0);
      d->parity = par;
      d->odom[0] = oth;
      d->odom[1] = ox;
      d->odom[2] = oy;
      d->prev_m = prev_m;
    }
    if (lane < kMaxChunk) d->prev_ids[lane] = prev_m >= 0 ? sh.prev_ids[lane] : 0;
    __syncthreads();
    if (lane < kMaxChunk) sh.prev_ids[lane] = lane < m ? sh.ids[lane] : 0;
    __syncthreads();
    prev_m = m;
    par ^= 1;
  }
  // state for the next run
  if (lane == 0) {
    S.truth[0] = truth.theta;
    S.truth[1] = truth.x;
    S.truth[2] = truth.y;
    S.odom[0] = odo.theta;
    S.odom[1] = odo.x;
    S.odom[2] = odo.y;
    A.par[f] = par;
    if constexpr (kCollide) S.hits += hits;
  }
  for (int w = lane; w < words; w += 64) A.sighted[static_cast<size_t>(f) * words + w] = sh.sighted[w];
}
}  // namespace

__global__ __launch_bounds__(64) void k_sim(SimArgs A) {
  __shared__ SimShared sh;
  sim_run<false>(A, sh, nullptr);
}

__global__ __launch_bounds__(64) void k_sim_collide(SimArgs A) {
  __shared__ SimShared sh;
  __shared__ CollideShared cs;
  sim_run<true>(A, sh, &cs);
}

// ---- runs without SURVEY messages: every message sensed in parallel ----------------------------
// The sighted set: a landmark is sighted once a SURVEY message of this simulator has reported it;
// NEAREST and ALL messages neither read nor write the set (k_sim above; synth._sense on the host).
// Only that set carries sensing state from one message to the next; without a SURVEY message a
// message's markers depend on its true pose alone. Pass 1 (k_sim_arcs, one wave per message and
// filter: each message's tick scan; then k_sim_pose, one wave per filter: the products composed in
// message order — the only sequential part) writes every message's true pose and odometry; pass 2 (k_sim_sense, one wave per message and filter, T·F in
// flight instead of F) senses and records the markers as ekf_replay takes them, and the device
// planner of ekf_replay_device (plan_kernels.hip) writes the descriptors from those. Same
// functions, draws and order as k_sim, so the same bits.
// Pass 1a: each message's tick products (one wave per (message, filter), in parallel) into
// truth_all / odom_all; pass 1b (k_sim_pose) composes them in message order over them.
__global__ __launch_bounds__(64) void k_sim_arcs(SimArgs A, double* truth_all, double* odom_all) {
  const int t = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
  const unsigned long long seed = A.seed + static_cast<unsigned long long>(A.f0 + f);
  Pose2 pt, po;
  arc_products(A, seed, t, lane, pt, po);
  const size_t o = (static_cast<size_t>(t) * A.F + f) * 3;
  if (lane < 3) {
    truth_all[o + lane] = lane == 0 ? pt.theta : (lane == 1 ? pt.x : pt.y);
    odom_all[o + lane] = lane == 0 ? po.theta : (lane == 1 ? po.x : po.y);
  }
}

__global__ __launch_bounds__(64) void k_sim_pose(SimArgs A, double* truth_all, double* odom_all) {
  const int f = blockIdx.x, lane = threadIdx.x;
  SimState& S = A.st[f];
  Pose2 truth{S.truth[0], S.truth[1], S.truth[2]};
  Pose2 odo{S.odom[0], S.odom[1], S.odom[2]};
  for (int t = 0; t < A.T; ++t) {
    const size_t o = (static_cast<size_t>(t) * A.F + f) * 3;
    // the message's products (k_sim_arcs), then the poses after it over them (same slot, same wave)
    truth = compose(truth, Pose2{truth_all[o], truth_all[o + 1], truth_all[o + 2]});
    odo = compose(odo, Pose2{odom_all[o], odom_all[o + 1], odom_all[o + 2]});
    if (lane < 3) {
      const double tv = lane == 0 ? truth.theta : (lane == 1 ? truth.x : truth.y);
      const double ov = lane == 0 ? odo.theta : (lane == 1 ? odo.x : odo.y);
      truth_all[o + lane] = tv;
      odom_all[o + lane] = ov;
      if (A.out_truth) A.out_truth[o + lane] = tv;
      if (A.out_odom && f == 0) A.out_odom[static_cast<size_t>(t) * 3 + lane] = ov;
    }
  }
  if (lane == 0) {
    S.truth[0] = truth.theta;
    S.truth[1] = truth.x;
    S.truth[2] = truth.y;
    S.odom[0] = odo.theta;
    S.odom[1] = odo.x;
    S.odom[2] = odo.y;
  }
}

// k_sim_pose with collisions on (ekf_sim_set_collisions): a message's product cannot be composed
// blindly any more, so the wave walks each message as k_sim_collide does (collide_wheels, which
// recomputes the message's tick arcs from the counter-based draws: the same bits) for the truth;
// the odometry, which no collision touches, still composes k_sim_arcs' products.
__global__ __launch_bounds__(64) void k_sim_pose_collide(SimArgs A, double* truth_all,
                                                         double* odom_all) {
  __shared__ CollideShared cs;
  const int f = blockIdx.x, lane = threadIdx.x;
  const unsigned long long seed = A.seed + static_cast<unsigned long long>(A.f0 + f);
  const double* lm = A.lm + static_cast<size_t>(f) * A.L * 2;
  SimState& S = A.st[f];
  Pose2 truth{S.truth[0], S.truth[1], S.truth[2]};
  Pose2 odo{S.odom[0], S.odom[1], S.odom[2]};
  long long hits = 0;
  const bool cull = A.L >= A.cull_from;
  const int n_all = cull ? 0 : hit_candidates(lm, A.L, false, 0.0, 0.0, 0.0, cs, lane);
  for (int t = 0; t < A.T; ++t) {
    const size_t row = static_cast<size_t>(t) * A.F + f, o = row * 3;
    const int h = collide_wheels<false>(A, lm, seed, t, lane, cull, n_all, cs, truth, odo);
    hits += h;
    odo = compose(odo, Pose2{odom_all[o], odom_all[o + 1], odom_all[o + 2]});
    if (A.out_hits && lane == 0) A.out_hits[row] = h;
    if (lane < 3) {
      const double tv = lane == 0 ? truth.theta : (lane == 1 ? truth.x : truth.y);
      const double ov = lane == 0 ? odo.theta : (lane == 1 ? odo.x : odo.y);
      truth_all[o + lane] = tv;
      odom_all[o + lane] = ov;
      if (A.out_truth) A.out_truth[o + lane] = tv;
      if (A.out_odom && f == 0) A.out_odom[static_cast<size_t>(t) * 3 + lane] = ov;
    }
  }
  if (lane == 0) {
    S.truth[0] = truth.theta;
    S.truth[1] = truth.x;
    S.truth[2] = truth.y;
    S.odom[0] = odo.theta;
    S.odom[1] = odo.x;
    S.odom[2] = odo.y;
    S.hits += hits;
  }
}

struct SenseShared {
  int sel[kMaxChunk];
};
__global__ __launch_bounds__(64) void k_sim_sense(SimArgs A, const double* truth_all) {
  __shared__ SenseShared sh;
  const int t = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
  const unsigned long long seed = A.seed + static_cast<unsigned long long>(A.f0 + f);
  const size_t rowo = static_cast<size_t>(t) * A.F + f;
  const double th = truth_all[rowo * 3], px = truth_all[rowo * 3 + 1], py = truth_all[rowo * 3 + 2];
  const int mode = A.sense ? A.sense[t] : kSenseNearest;  // (never SURVEY here)
  const double* lm = A.lm + static_cast<size_t>(f) * A.L * 2;
  const int k = sense<false>(A, lm, mode, th, px, py, sh, lane);
  int id, act;
  double rx, ry;
  marker<false>(A, seed, A.msg0 + t, mode, k, sh, lane, &id, &act, &rx, &ry, lm, th, px, py);
  record_markers(A, rowo, k, id, act, rx, ry, lane);
}

hipError_t launch_sim(const SimArgs& a, bool collide, hipStream_t s) {
  if (collide)
    hipLaunchKernelGGL(k_sim_collide, dim3(a.F), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL(k_sim, dim3(a.F), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sim_parallel(const SimArgs& a, bool collide, double* truth_all, double* odom_all,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_sim_arcs, dim3(a.T, a.F), dim3(64), 0, s, a, truth_all, odom_all);
  if (collide)
    hipLaunchKernelGGL(k_sim_pose_collide, dim3(a.F), dim3(64), 0, s, a, truth_all, odom_all);
  else
    hipLaunchKernelGGL(k_sim_pose, dim3(a.F), dim3(64), 0, s, a, truth_all, odom_all);
  hipLaunchKernelGGL(k_sim_sense, dim3(a.T, a.F), dim3(64), 0, s, a,
                     static_cast<const double*>(truth_all));
  return hipGetLastError();
}

}  // namespace ekfslam
