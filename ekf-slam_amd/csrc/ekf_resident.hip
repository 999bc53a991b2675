// Register-resident filter kernel (gfx950) for small maps: n = 3 + 2N ≤ kResidentMaxN, fp64.
//
// The low-rank pipeline of ekf_chain.hip (chain → factors → Σ pass per chunk, an association
// kernel per marker) is built for covariances that live in HBM. At the reference's own map size
// (N = 50 slots, n = 103: basic_world and the rosbag drive, BASELINE configs[0] and [4]) the whole
// Σ is 83 KB, and that pipeline is launch- and hand-off-bound (≈ 94 µs per associated marker).
// Here one 256-thread workgroup (4 waves) owns one filter for an entire upload (every message of a
// replay): Σ stays in VGPRs (wave w holds rows w, w+4, …; lane ℓ holds columns ℓ, ℓ+64), x with it,
// and each correction is
//   gather   the owners of rows / columns {θ, x, y, jx, jy} write them to LDS (10·n doubles);
//   barrier  (one per correction: the gather buffers are double-buffered);
//   update   every thread forms ẑ, H, S = HΣHᵀ + R, S⁻¹, ν from the gathered values (the same
//            operands in every thread, so the same bits) and applies Σ ← Σ − K·(HΣ) and x += Kν
//            to the elements it owns: 2 FMAs per element, no LDS traffic for Σ itself.
// The Mahalanobis association of a marker (slam.cpp:344-440) is one wavefront: lane k scores
// landmark k from the gathered pose rows / columns, the 2×2 landmark blocks and x, then a DPP
// wave argmin (wave_argmin, ekf_math.hpp; first index wins, like arma::index_min).
//
// Numerics follow the chain kernel's helpers (range_bearing, inv2, rank2_sub, normalize_angle_near)
// and k_assoc's distance expression, so decisions match the HBM pipeline's; Σ differs from it by
// summation order only (Σ_ij − K_i0·M_0j − K_i1·M_1j as two FMAs; tests/test_gpu_resident.py:
// both paths against the oracle).
//
// In the source, in execution order. k_resident is the plan walk; a thread's share of the filter
// is one ResState, and every phase is a __forceinline__ function on it (one register allocation):
//   stage_plan_block      16 plan entries' descriptors → LDS
//   load_filter           first entry naming the filter: Σ, x, t_map_odom, counter, trace count
//   posterior_now / _from the deferred posterior t_map_odom (with the next gather of the pose)
//                         and its record in the pose trace (PassArgs::trace)
//   predict               gather_rows (pose) → barrier → Σ = AΣAᵀ + Q̄, the new pose
//   known ids, per marker: gather_rows → barrier → correct
//   unknown, per marker   associate_correct: gather_rows (pose), gather_assoc_blocks → barrier →
//                         score_and_decide (wave 0) → barrier → init_new_landmark → gather_rows
//                         (landmark) → barrier → correct
//   correct               innovation_gain (ẑ, H, M = HΣ, S, S⁻¹, ν, K) → apply_simple /
//                         apply_joseph → x += Kν
//   store_filter          decisions, Σ, x, t_map_odom, counter, status, trace count
// k_resident_replay (below k_resident) is the same walk over messages whose inputs lie in device
// memory (ekf_replay_resident): stage_replay_block turns 8 messages' counts, markers and odometry
// into (range, bearing) lists in LDS, and the phases above run on them with no descriptors.
// Shared algebra: times_H (five-term products with H), gain (K = q·S⁻¹), landmark_from (a first
// sighting's position); range_innovation and sub_rounded (ekf_math.hpp) pin the two roundings of
// z₀ − ẑ₀.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <climits>
#include <type_traits>

#include "atan2_dd.hpp"
#include "ekf.h"
#include "ekf_device.hpp"
#include "ekf_launch.hpp"
#include "ekf_math.hpp"
#include "geom.hpp"

namespace ekfslam {

// Diagnostic build only (libekfslam_diag.so, tools/resident_stamps.py): s_memtime of thread 0 of
// the first workgroup at RS_STAMP points, 8 slots per correction for the first 64 corrections.
#ifdef EKF_DIAG_STAMPS
__device__ unsigned long long g_res_stamps[512];
#define RS_STAMP(k, i)                                                        \
  do {                                                                        \
    if (blockIdx.x == 0 && threadIdx.x == 0 && (k) < 64)                      \
      g_res_stamps[8 * (k) + (i)] = __builtin_amdgcn_s_memtime();             \
  } while (0)
}  // namespace ekfslam
extern "C" int ekfslam_res_read_stamps(unsigned long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(ekfslam::g_res_stamps),
                             sizeof(unsigned long long) * (n < 512 ? n : 512)) == hipSuccess ? 0 : -5;
}
namespace ekfslam {
#else
#define RS_STAMP(k, i) \
  do {                 \
  } while (0)
#endif

namespace {

typedef unsigned u2 __attribute__((ext_vector_type(2)));
// a voffset past the descriptor's num_records: the access is dropped (loads return 0); the range
// check is on voffset, so rows past n (the SGPR offset) must use it too
constexpr int kOOB = 0x7ffffff0;

// The prefix of a MsgDesc the kernel reads (m … z), staged in LDS a block of plan entries at a time.
struct alignas(16) ResMsg {
  int m, flags, parity, assoc_slot;
  double odom[3];
  int prev_m, pad1;
  int ids[kMaxChunk];
  double z[kMaxChunk][2];
};
static_assert(offsetof(ResMsg, odom) == offsetof(MsgDesc, odom) &&
                  offsetof(ResMsg, ids) == offsetof(MsgDesc, ids) &&
                  offsetof(ResMsg, z) == offsetof(MsgDesc, z) && sizeof(ResMsg) % 16 == 0,
              "ResMsg is MsgDesc's prefix");
constexpr int kMsgQ = sizeof(ResMsg) / 16;  // 16-byte pieces per staged descriptor
constexpr int kBlk = 16;                    // plan entries staged per block

template <int W, int RS, int CS>
struct ResShared {
  ResMsg msg[kBlk];
  int kind[kBlk];  // the entry's kind, −1: it does not name this filter
  double grow[2][5][64 * CS];  // Σ[idx_a][c]  (idx = {0, 1, 2, j, j+1})
  double gcol[2][5][W * RS];   // Σ[r][idx_a]
  double gx[2][8];             // x[idx_a]
  double blk[(W * RS) / 2][4];  // association: Σ[jk..jk+1][jk..jk+1] of landmark k
  double xall[W * RS];          // association: x
  int dec[2];                   // association decision: slot j, is_new
  int decj[kMaxAssoc], decn[kMaxAssoc];  // decisions by slot, stored to FilterCtl at the end
  double junk[64];                        // sink of the branch-free block gather
  double kw[W][RS][4];          // per wave: K[row(s)] (and Joseph: (Σ·Hᵀ)[row(s)]), wave-private
};

// One thread's share of the filter and of the plan walk's state.
template <int W, int RS, int CS>
struct ResState {
  double sg[RS][CS];  // Σ[row(s)][col(t)]; indexed by compile-time constants only (registers)
  // x and per-row scalars live lane-distributed: lane s < RS holds row w + W·s (its own row rl)
  int lane, w, rl;
  bool rown;
  double xl = 0.0;
  double tmo[3];
  // posterior deferred to the next gather of the pose (the next message's predict gathers it
  // anyway; nothing moves the pose in between): one barrier per message instead of two
  bool post = false;
  double podom[3] = {0.0, 0.0, 0.0};
  unsigned counter = 0, status = 0;
  long long trace_n = 0;  // pose trace: the filter's record count (workgroup-uniform)
  unsigned long long dslots = 0;  // association slots decided in this launch (sh.decj/decn)
  int par = -1;                   // current parity (−1: not loaded yet)
  bool dirty = false;             // Σ / x changed (a chunk entry ran)
  int b = 0;                      // gather buffer
  // wq: the wave index re-materialised per correction (an opaque copy), so the compiler recomputes
  // the per-row conditions in a few scalar ops instead of hoisting them out of the plan loop into
  // (spilled) SGPRs
  int wq;
  int ncorr = 0;  // corrections so far (diagnostic stamps)

  __device__ __forceinline__ int row(int s) const { return wq + W * s; }
  __device__ __forceinline__ int col(int t) const { return lane + 64 * t; }
  // x[r] ← v on the owner of row r
  __device__ __forceinline__ void set_x(int r, double v) {
    if (rown && rl == r) xl = v;
  }
};

__device__ __forceinline__ int pos5(int r, int j) {
  return r < 3 ? r : (r == j ? 3 : (r == j + 1 ? 4 : -1));
}

// (o0, o1) = Σ_a (H0[a], H1[a])·v(a), a over {θ, x, y, jx, jy}, in that order: a column of H·Σ
// from gathered rows, a row of Σ·Hᵀ from gathered columns
template <typename V>
__device__ __forceinline__ void times_H(const double* H0, const double* H1, const V& v, double& o0,
                                        double& o1) {
  o0 = 0.0;
  o1 = 0.0;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const double va = v(a);
    o0 += H0[a] * va;
    o1 += H1[a] * va;
  }
}

// K = q·S⁻¹ for one row q of Σ·Hᵀ
__device__ __forceinline__ void gain(double q0, double q1, const double* Si, double& K0,
                                     double& K1) {
  K0 = q0 * Si[0] + q1 * Si[2];
  K1 = q0 * Si[1] + q1 * Si[3];
}

// A first sighting's landmark position from the pose and the measurement (slam.cpp:213-216,
// :351-356)
__device__ __forceinline__ void landmark_from(double th, double px, double py, double z0, double z1,
                                              double& lx, double& ly) {
  double sn, cs;
  sincos(z1 + th, &sn, &cs);
  lx = px + z0 * cs;
  ly = py + z0 * sn;
}

// Stage the block's descriptors: every thread fetches 16-byte pieces (plan entry → descriptor,
// one dependent pair of loads per thread, all in flight together), one barrier. Returns the
// number of entries staged.
template <int W, int RS, int CS>
__device__ __forceinline__ int stage_plan_block(ResShared<W, RS, CS>& sh, const MsgDesc* desc,
                                                const PlanEntry* plan, int nplan, int l0, int f) {
  const int nb = min(kBlk, nplan - l0);
  __syncthreads();  // the previous block's entries are consumed
  for (int t = threadIdx.x; t < nb * kMsgQ; t += W * 64) {
    const int e = t / kMsgQ, q = t - e * kMsgQ;
    const PlanEntry L = plan[l0 + e];
    const bool mine = f >= L.f0 && f < L.f0 + L.nf;
    if (q == 0) sh.kind[e] = mine ? L.kind : -1;
    if (mine)
      reinterpret_cast<uint4*>(&sh.msg[e])[q] =
          reinterpret_cast<const uint4*>(desc + L.off + (f - L.f0))[q];
  }
  __syncthreads();
  return nb;
}

// Σ and x of parity par into registers, t_map_odom and the counter from the filter's control block
template <int W, int RS, int CS>
__device__ __forceinline__ void load_filter(ResState<W, RS, CS>& st, const PassArgs<double>& A,
                                            const FilterCtl* ctl, int f, int par) {
  const int n = A.n, ld = A.ld;
  st.par = par;
  const double* S = A.sig[par] + f * A.sig_stride;
  const double* X = A.x[par] + f * A.x_stride;
  // buffer loads: row offset in the SGPR operand, column in the VGPR one; out-of-range
  // rows / columns read 0 (the descriptor covers exactly n rows)
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(S), 0, n * ld * 8, 0x00020000);
#pragma unroll
  for (int s = 0; s < RS; ++s) {
    const int r = st.row(s);
#pragma unroll
    for (int t = 0; t < CS; ++t) {
      const int c = st.col(t);
      const double v = __builtin_bit_cast(
          double, __builtin_amdgcn_raw_buffer_load_b64(rs, r < n && c < n ? c * 8 : kOOB, r * ld * 8, 0));
      st.sg[s][t] = (r < n && c < n) ? v : 0.0;
    }
  }
  st.xl = (st.rown && st.rl < n) ? X[st.rl] : 0.0;
  st.tmo[0] = ctl->tmo[0];
  st.tmo[1] = ctl->tmo[1];
  st.tmo[2] = ctl->tmo[2];
  st.counter = ctl->counter;
  if (A.trace) st.trace_n = A.trace_n[f];
}

// Rows / columns idx_a with a ≥ amin (j < 0: pose only) and their x into gather buffer bb
template <int W, int RS, int CS>
__device__ __forceinline__ void gather_rows(ResState<W, RS, CS>& st, ResShared<W, RS, CS>& sh,
                                            int n, int bb, int j, int amin) {
  asm volatile("" : "+s"(st.wq));
  // rows: θ, x, y are slot 0 of waves 0-2; jx, jy sit in slot r / W of wave r % W, picked by
  // one jump-table switch each (a few scalar ops and one indirect branch: the scalar unit is
  // shared by the CU's waves, a test per slot costs more; a run-time index into sg would send
  // the array to scratch)
  if (amin == 0 && st.wq < 3) {
#pragma unroll
    for (int t = 0; t < CS; ++t) sh.grow[bb][st.wq][st.col(t)] = st.sg[0][t];
  }
  // The switch picks among values, not among loads through st: this function is optimised on
  // its own before it is inlined, and there the cases' loads st.sg[q][t] merge into one load of
  // a selected address, which keeps that column of Σ in scratch. The copy vanishes once inlined.
  double v[RS][CS];
#pragma unroll
  for (int s = 0; s < RS; ++s)
#pragma unroll
    for (int t = 0; t < CS; ++t) v[s][t] = st.sg[s][t];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int r = j + e;
    if (j >= 0 && r < n && r % W == st.wq) {
      double* dst = &sh.grow[bb][3 + e][0];
      switch (r / W) {
#define RES_SLOT(q)                                                                \
  case q:                                                                          \
    if constexpr (q < RS) {                                                        \
      _Pragma("unroll") for (int t = 0; t < CS; ++t) dst[st.col(t)] = v[q][t];     \
    }                                                                              \
    break;
#define RES_SLOT8(q) RES_SLOT(q) RES_SLOT(q + 1) RES_SLOT(q + 2) RES_SLOT(q + 3) \
    RES_SLOT(q + 4) RES_SLOT(q + 5) RES_SLOT(q + 6) RES_SLOT(q + 7)
        RES_SLOT8(0) RES_SLOT8(8) RES_SLOT8(16) RES_SLOT8(24)
#undef RES_SLOT8
#undef RES_SLOT
        default:
          break;
      }
    }
  }
  {
    const int a = pos5(st.rl, j);
    if (st.rown && a >= amin && st.rl < n) sh.gx[bb][a] = st.xl;
  }
#pragma unroll
  for (int t = 0; t < CS; ++t) {
    const int c = st.col(t), a = pos5(c, j);
    if (a >= amin && c < n) {
#pragma unroll
      for (int s = 0; s < RS; ++s) sh.gcol[bb][a][st.row(s)] = st.sg[s][t];
    }
  }
}

// posterior t_map_odom = T(x, y, θ)·t_odom_robot⁻¹ (slam.cpp:273-291) from a gathered pose, and
// the pose trace's record of it (every thread holds the pose and the count: thread 0 stores)
template <int W, int RS, int CS>
__device__ __forceinline__ void posterior_from(ResState<W, RS, CS>& st, const PassArgs<double>& A,
                                               int f, double p0, double p1, double p2) {
  const Pose2 t = compose_sc(Pose2{p0, p1, p2},
                             inverse_sc(Pose2{st.podom[0], st.podom[1], st.podom[2]}));
  st.tmo[0] = t.theta;
  st.tmo[1] = t.x;
  st.tmo[2] = t.y;
  st.post = false;
  if (A.trace) {
    if (threadIdx.x == 0) trace_append(A, f, st.trace_n, p0, p1, p2, t.theta, t.x, t.y);
    st.trace_n += 1;
  }
}
template <int W, int RS, int CS>
__device__ __forceinline__ void posterior_now(ResState<W, RS, CS>& st, ResShared<W, RS, CS>& sh,
                                              const PassArgs<double>& A, int f) {
  st.b ^= 1;
  if (st.rown && st.rl < 3) sh.gx[st.b][st.rl] = st.xl;
  __syncthreads();
  posterior_from(st, A, f, sh.gx[st.b][0], sh.gx[st.b][1], sh.gx[st.b][2]);
}

// predict, slam.cpp:184-198: Σ = AΣAᵀ + Q̄, A = I + α·e0ᵀ; the last message's deferred posterior
// rides on its pose gather
template <int W, int RS, int CS>
__device__ __forceinline__ void predict(ResState<W, RS, CS>& st, ResShared<W, RS, CS>& sh,
                                        const PassArgs<double>& A, int f, const double* odom) {
  const int n = A.n;
  const double q = A.q;
  st.b ^= 1;
  const int b = st.b;
  gather_rows(st, sh, n, b, -8, 0);
  __syncthreads();
  const double prev[3] = {sh.gx[b][0], sh.gx[b][1], sh.gx[b][2]};
  if (st.post) posterior_from(st, A, f, prev[0], prev[1], prev[2]);
  const Pose2 cur = compose_sc(Pose2{st.tmo[0], st.tmo[1], st.tmo[2]},
                               Pose2{odom[0], odom[1], odom[2]});
  const double a1 = -(cur.y - prev[2]), a2 = cur.x - prev[1];
  const double s00 = sh.grow[b][0][0];
#pragma unroll
  for (int s = 0; s < RS; ++s) {
    const int r = st.row(s);
    const double aa = alpha_of(r, a1, a2);
    const double cr0 = sh.gcol[b][0][r];  // Σ[r][0], broadcast
#pragma unroll
    for (int t = 0; t < CS; ++t) {
      const int c = st.col(t);
      const double ab = alpha_of(c, a1, a2);
      double v = st.sg[s][t] + aa * sh.grow[b][0][c];
      v = v + (cr0 + aa * s00) * ab;
      if (r == c && r < 3) v += q;
      st.sg[s][t] = v;
    }
  }
  st.set_x(0, normalize_angle(cur.theta));
  st.set_x(1, cur.x);
  st.set_x(2, cur.y);
}

// What a correction's update needs from its geometry: H, S, S⁻¹, ν, this lane's columns of
// M = H·Σ and its row's gain
template <int CS>
struct Corr {
  double H0[5], H1[5], Sm[4], Si[4], nv0, nv1, K0, K1;
  double mc0[CS], mc1[CS];  // (H·Σ)[:, c] of this lane's columns
};

// ẑ, H, M, S, S⁻¹, ν and K of a correction against column j from gather buffer b; the wave's
// rows' K (and Σ·Hᵀ) are left in its kw slots. false: S is singular (the marker is skipped).
template <int W, int RS, int CS>
__device__ __forceinline__ bool innovation_gain(ResState<W, RS, CS>& st, ResShared<W, RS, CS>& sh,
                                                double r_noise, int j, double z0, double z1,
                                                bool noinit, Corr<CS>& c) {
  const int b = st.b;
  const double pose[3] = {sh.gx[b][0], sh.gx[b][1], sh.gx[b][2]};
  double lx = sh.gx[b][3], ly = sh.gx[b][4];
  if (!noinit && lx == 0.0 && ly == 0.0) {  // first sighting, slam.cpp:213-216
    landmark_from(pose[0], pose[1], pose[2], z0, z1, lx, ly);
    st.set_x(j, lx);
    st.set_x(j + 1, ly);
  }
  double zhat[2], braw;
  bool bok;
  range_bearing(pose, lx, ly, zhat, c.H0, c.H1, &braw, &bok);
  if (!bok) zhat[1] = normalize_angle(braw);
  RS_STAMP(st.ncorr, 2);
#pragma unroll
  for (int t = 0; t < CS; ++t)
    times_H(c.H0, c.H1, [&](int a) { return sh.grow[b][a][st.col(t)]; }, c.mc0[t], c.mc1[t]);
  // S = (H·Σ)[:, idx]·Hᵀ + R (slam.cpp:252, left to right like arma); (H·Σ)[:, idx] from the
  // lanes that own those columns
  c.Sm[0] = c.Sm[1] = c.Sm[2] = c.Sm[3] = 0.0;
#pragma unroll
  for (int bb = 0; bb < 5; ++bb) {
    const int cc = bb < 3 ? bb : j + bb - 3;
    double v0 = c.mc0[0], v1 = c.mc1[0];
#pragma unroll
    for (int t = 1; t < CS; ++t)
      if ((cc >> 6) == t) {
        v0 = c.mc0[t];
        v1 = c.mc1[t];
      }
    const double h0 = readlane_f64(v0, cc & 63), h1 = readlane_f64(v1, cc & 63);
    c.Sm[0] += h0 * c.H0[bb];
    c.Sm[1] += h0 * c.H1[bb];
    c.Sm[2] += h1 * c.H0[bb];
    c.Sm[3] += h1 * c.H1[bb];
  }
  c.Sm[0] += r_noise;
  c.Sm[3] += r_noise;
  if (!inv2(c.Sm, c.Si)) return false;  // arma::inv throws in the reference
  c.nv0 = range_innovation(pose, lx, ly, z0);
  bool nok;
  const double nn = normalize_angle_near(z1 - zhat[1], &nok);
  c.nv1 = nok ? nn : normalize_angle(z1 - zhat[1]);
  RS_STAMP(st.ncorr, 3);
  // K[rl] = (Σ·Hᵀ)[rl]·S⁻¹ on the lane that holds row rl, then every lane takes its rows' K
  double ka, kb;
  times_H(c.H0, c.H1, [&](int a) { return sh.gcol[b][a][st.rl]; }, ka, kb);
  gain(ka, kb, c.Si, c.K0, c.K1);
  // the wave's rows' K through its own LDS slots (one wave: LDS ops complete in issue order)
  if (st.rown) {
    sh.kw[st.w][st.lane][0] = c.K0;
    sh.kw[st.w][st.lane][1] = c.K1;
    sh.kw[st.w][st.lane][2] = ka;
    sh.kw[st.w][st.lane][3] = kb;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return true;
}

// Σ ← Σ − K·(HΣ), slam.cpp:264-265
template <int W, int RS, int CS>
__device__ __forceinline__ void apply_simple(ResState<W, RS, CS>& st, ResShared<W, RS, CS>& sh,
                                             const Corr<CS>& c) {
#pragma unroll
  for (int s = 0; s < RS; ++s) {
    const double k0 = sh.kw[st.w][s][0], k1 = sh.kw[st.w][s][1];  // broadcast reads
#pragma unroll
    for (int t = 0; t < CS; ++t)
      st.sg[s][t] = fma(-k1, c.mc1[t], fma(-k0, c.mc0[t], st.sg[s][t]));
  }
}

// Joseph form (opt-in): Σ ← (I−KH)Σ(I−KH)ᵀ + KRKᵀ = Σ − K·(HΣ) − (ΣHᵀ)·Kᵀ + K·S·Kᵀ. Per
// column c: K[c] from (ΣHᵀ)[c] (the gathered columns at row c) and u = S·K[c]ᵀ; then each
// element takes Σ_rc − K_r·(M_c − u_c) − (ΣHᵀ)_r·K_cᵀ, four FMAs
template <int W, int RS, int CS>
__device__ __forceinline__ void apply_joseph(ResState<W, RS, CS>& st, ResShared<W, RS, CS>& sh,
                                             Corr<CS>& c) {
  const int b = st.b;
  double kc0[CS], kc1[CS];
#pragma unroll
  for (int t = 0; t < CS; ++t) {
    const int cc = min(st.col(t), W * RS - 1);  // columns ≥ n: never stored
    double pa, pb;
    times_H(c.H0, c.H1, [&](int a) { return sh.gcol[b][a][cc]; }, pa, pb);
    gain(pa, pb, c.Si, kc0[t], kc1[t]);
    c.mc0[t] -= c.Sm[0] * kc0[t] + c.Sm[1] * kc1[t];
    c.mc1[t] -= c.Sm[2] * kc0[t] + c.Sm[3] * kc1[t];
  }
#pragma unroll
  for (int s = 0; s < RS; ++s) {
    const double k0 = sh.kw[st.w][s][0], k1 = sh.kw[st.w][s][1];
    const double p0 = sh.kw[st.w][s][2], p1 = sh.kw[st.w][s][3];
#pragma unroll
    for (int t = 0; t < CS; ++t)
      st.sg[s][t] = fma(-p1, kc1[t], fma(-p0, kc0[t],
                        fma(-k1, c.mc1[t], fma(-k0, c.mc0[t], st.sg[s][t]))));
  }
}

// One correction against landmark column j = 3 + 2·id (slam.cpp:219-267 / :443-488). The
// gather of idx into buffer b is done and the barrier passed.
template <int W, int RS, int CS, bool JOSEPH>
__device__ __forceinline__ void correct(ResState<W, RS, CS>& st, ResShared<W, RS, CS>& sh,
                                        double r_noise, int j, double z0, double z1, bool noinit) {
  RS_STAMP(st.ncorr, 1);
  asm volatile("" : "+s"(st.wq));
  Corr<CS> c;
  if (!innovation_gain(st, sh, r_noise, j, z0, z1, noinit, c)) {  // skip the marker, flag it
    st.status |= EKF_FLAG_NUMERIC_D;
    return;
  }
  // x's increment first (it reads nothing the Σ update writes): K and ν are then dead across the
  // update, which is where the Joseph kernels run out of registers
  double xt = st.xl + (c.K0 * c.nv0 + c.K1 * c.nv1);  // slam.cpp:261
  if constexpr (JOSEPH)
    apply_joseph(st, sh, c);
  else
    apply_simple(st, sh, c);
  if (st.rl == 0) {                                    // slam.cpp:267
    bool tok;
    const double tn = normalize_angle_near(xt, &tok);
    xt = tok ? tn : normalize_angle(xt);
  }
  st.xl = xt;
  RS_STAMP(st.ncorr, 4);
  ++st.ncorr;
}

// Landmark 2×2 blocks of the seen landmarks (rows < 3 + 2·counter) and x for the scoring wave:
// every (slot, column) element stores — to its block entry when it is one, else to this lane's
// junk slot. The row index is taken as a vector value (tid >> 6 unmerged), so the index math
// runs on each SIMD's VALU, not on the CU's one scalar unit.
template <int W, int RS, int CS>
__device__ __forceinline__ void gather_assoc_blocks(ResState<W, RS, CS>& st,
                                                    ResShared<W, RS, CS>& sh, int n) {
  const int wv = static_cast<int>(threadIdx.x) >> 6;
  const int rmax = 3 + 2 * static_cast<int>(st.counter);
#pragma unroll
  for (int s = 0; s < RS; ++s) {
    if (st.row(s) >= rmax) break;  // rows grow with s
    const int r = wv + W * s;
    const int k = (r - 3) >> 1, e = (r - 3) & 1;
#pragma unroll
    for (int t = 0; t < CS; ++t) {
      const int dc = st.col(t) - (3 + 2 * k);
      const bool in = r >= 3 && (dc == 0 || dc == 1);
      *(in ? &sh.blk[k < 0 ? 0 : k][2 * e + dc] : &sh.junk[st.lane]) = st.sg[s][t];
    }
  }
  if (st.rown && st.rl >= 3 && st.rl < n) sh.xall[st.rl] = st.xl;
}

// Wave 0: lane k scores landmark k (k + 64, …) against the marker, the wave takes the argmin and
// lane 0 decides between it and a new landmark at slot counter (slam.cpp:361-422)
template <int W, int RS, int CS>
__device__ __forceinline__ void score_and_decide(const ResState<W, RS, CS>& st,
                                                 ResShared<W, RS, CS>& sh, double r_noise,
                                                 double gate, double z0, double z1, int slot) {
  const int b = st.b;
  const double pose[3] = {sh.gx[b][0], sh.gx[b][1], sh.gx[b][2]};
  double bestd = INFINITY;
  int bestk = INT_MAX;
  for (unsigned k = st.lane; k < st.counter; k += 64) {
    const int j = 3 + 2 * static_cast<int>(k);
    // Σ over {θ, x, y, j, j+1}, read where it is used
    auto P = [&](int a, int c) __attribute__((always_inline)) -> double {
      if (a < 3) return sh.grow[b][a][c < 3 ? c : j + c - 3];
      if (c < 3) return sh.gcol[b][c][j + a - 3];
      return sh.blk[k][2 * (a - 3) + (c - 3)];
    };
    // assoc_dist's expression (ekf_math.hpp) with Σ read through P; kept apart from it because
    // this kernel has always rounded ẑ_range before the subtraction, where k_assoc and
    // k_assoc_msg contract the two: one shared form cannot keep all three bit for bit
    double zhat[2], H0[5], H1[5], braw;
    bool bok;
    range_bearing(pose, sh.xall[j], sh.xall[j + 1], zhat, H0, H1, &braw, &bok);
    if (!bok) zhat[1] = normalize_angle(braw);
    double psi[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int bb = 0; bb < 5; ++bb) {
      double hp0, hp1;  // (H·P)[:, bb]
      times_H(H0, H1, [&](int a) { return P(a, bb); }, hp0, hp1);
      psi[0] += hp0 * H0[bb];
      psi[1] += hp0 * H1[bb];
      psi[2] += hp1 * H0[bb];
      psi[3] += hp1 * H1[bb];
    }
    psi[0] += r_noise;
    psi[3] += r_noise;
    const double nu0 = sub_rounded(z0, zhat[0]);
    const double nu1 = normalize_angle(z1 - zhat[1]);
    double dist = NAN;
    const double det = psi[0] * psi[3] - psi[1] * psi[2];
    if (fabs(det) > 0.0) {  // (z_diffᵀ·ψ⁻¹)·z_diff, slam.cpp:401
      const double t0 = nu0 * psi[3] - nu1 * psi[2];
      const double t1 = nu1 * psi[0] - nu0 * psi[1];
      dist = (t0 * nu0 + t1 * nu1) / det;
    }
    if (dist < bestd) {  // strict: first index kept, NaN never selected
      bestd = dist;
      bestk = static_cast<int>(k);
    }
  }
  wave_argmin(bestd, bestk);  // (DPP, ekf_math.hpp; every lane holds the result)
  if (st.lane == 0) {
    // the new slot (d = gate, slam.cpp:406-408) wins only over a larger minimum
    const bool nw = !(bestd <= gate);
    const int jsel = nw ? static_cast<int>(st.counter) : bestk;
    sh.dec[0] = jsel;
    sh.dec[1] = nw;
    sh.decj[slot] = jsel;
    sh.decn[slot] = nw;
  }
}

// A new landmark at column j from the pose in gather buffer b (slam.cpp:351-356, kept: :421)
template <int W, int RS, int CS>
__device__ __forceinline__ void init_new_landmark(ResState<W, RS, CS>& st,
                                                  ResShared<W, RS, CS>& sh, int j, double z0,
                                                  double z1) {
  double lx, ly;
  landmark_from(sh.gx[st.b][0], sh.gx[st.b][1], sh.gx[st.b][2], z0, z1, lx, ly);
  st.set_x(j, lx);
  st.set_x(j + 1, ly);
  ++st.counter;
}

// Association + correction of one marker, slam.cpp:344-488
template <int W, int RS, int CS, bool JOSEPH>
__device__ __forceinline__ void associate_correct(ResState<W, RS, CS>& st,
                                                  ResShared<W, RS, CS>& sh,
                                                  const PassArgs<double>& A, double z0, double z1,
                                                  int slot) {
  st.dslots |= 1ull << slot;
  if (st.counter >= static_cast<unsigned>(A.N)) {  // the reference indexes out of range
    st.status |= EKF_FLAG_RANGE_D;
    if (threadIdx.x == 0) {
      sh.decj[slot] = -1;
      sh.decn[slot] = 0;
    }
    return;
  }
  RS_STAMP(st.ncorr, 0);
  st.b ^= 1;
  gather_rows(st, sh, A.n, st.b, -8, 0);  // pose rows / columns and pose x
  gather_assoc_blocks(st, sh, A.n);
  __syncthreads();
  RS_STAMP(st.ncorr, 6);
  if (st.w == 0) score_and_decide(st, sh, A.r, A.gate, z0, z1, slot);
  __syncthreads();
  const int j = 3 + 2 * sh.dec[0];
  if (sh.dec[1]) init_new_landmark(st, sh, j, z0, z1);
  RS_STAMP(st.ncorr, 7);
  gather_rows(st, sh, A.n, st.b, j, 3);  // the pose rows / columns are in b already
  RS_STAMP(st.ncorr, 5);
  __syncthreads();
  correct<W, RS, CS, JOSEPH>(st, sh, A.r, j, z0, z1, true);
}

// The decisions, Σ and x (when a chunk entry changed them, to parity par), t_map_odom, the
// counter and the status flags
template <int W, int RS, int CS>
__device__ __forceinline__ void store_filter(ResState<W, RS, CS>& st, ResShared<W, RS, CS>& sh,
                                             const PassArgs<double>& A, FilterCtl* ctl, int f) {
  const int n = A.n, ld = A.ld, tid = threadIdx.x;
  __syncthreads();  // the decisions in LDS
  if (tid < kMaxAssoc && (st.dslots >> tid & 1)) {
    ctl->assoc_j[tid] = sh.decj[tid];
    ctl->assoc_new[tid] = sh.decn[tid];
  }
  if (st.dirty) {
    double* S = A.sig[st.par] + f * A.sig_stride;
    double* X = A.x[st.par] + f * A.x_stride;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(S, 0, n * ld * 8, 0x00020000);
#pragma unroll
    for (int s = 0; s < RS; ++s) {
      const int r = st.row(s);
      if (r >= n) continue;
#pragma unroll
      for (int t = 0; t < CS; ++t) {
        const int c = st.col(t);  // columns ≥ n go out of the descriptor's range (dropped)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, st.sg[s][t]), rs,
                                              c < n ? c * 8 : kOOB, r * ld * 8, 0);
      }
    }
    if (st.rown && st.rl < n) X[st.rl] = st.xl;
  }
  if (tid == 0) {
    ctl->tmo[0] = st.tmo[0];
    ctl->tmo[1] = st.tmo[1];
    ctl->tmo[2] = st.tmo[2];
    ctl->counter = st.counter;
    if (A.trace) A.trace_n[f] = st.trace_n;
    if (st.status) atomicOr(&ctl->status, st.status);
  }
}

}  // namespace

// One workgroup per filter flo + blockIdx.x; walks the whole plan (PlanEntry list, in order) and
// applies the entries that name its filter. Σ / x are loaded on the first active entry from the
// entry's parity and written back once, to the parity the host's plan ends on.
template <int W, int RS, int CS, bool JOSEPH>
__global__ __launch_bounds__(W * 64) void k_resident(PassArgs<double> A, const PlanEntry* plan,
                                                     int nplan, int flo) {
  static_assert(RS <= 32, "jump-table gather covers 32 slots; x is lane-distributed");
  __shared__ ResShared<W, RS, CS> sh;
  const int f = flo + blockIdx.x;
  FilterCtl* ctl = A.ctl + f;
  ResState<W, RS, CS> st;
  st.lane = threadIdx.x & 63;
  st.w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: row offsets in SGPRs
  st.wq = st.w;
  st.rown = st.lane < RS;
  st.rl = st.w + W * (st.rown ? st.lane : RS - 1);

  for (int l0 = 0; l0 < nplan; l0 += kBlk) {
    const int nb = stage_plan_block(sh, A.desc, plan, nplan, l0, f);
    for (int e = 0; e < nb; ++e) {
      const int kind = sh.kind[e];
      if (kind < 0) continue;
      const ResMsg& d = sh.msg[e];
      const int flags = d.flags;
      if (!(flags & kActive)) continue;
      if (st.par < 0) load_filter(st, A, ctl, f, d.parity);  // first entry naming this filter
      if (st.post && kind != kLaunchPosterior && !(flags & kFirst))
        posterior_now(st, sh, A, f);  // corrections follow
      if (kind != kLaunchPosterior) {
        if (flags & kFirst) predict(st, sh, A, f, d.odom);
        if (kind == kLaunchKnown) {  // known association, slam.cpp:201-271
          for (int c = 0; c < d.m; ++c) {
            const int id = d.ids[c];
            if (id < 0 || id >= A.N) continue;  // validated on the host; never reached
            RS_STAMP(st.ncorr, 0);
            st.b ^= 1;
            gather_rows(st, sh, A.n, st.b, 3 + 2 * id, 0);
            RS_STAMP(st.ncorr, 5);
            __syncthreads();
            correct<W, RS, CS, JOSEPH>(st, sh, A.r, 3 + 2 * id, d.z[c][0], d.z[c][1],
                                       (flags & kNoInit) != 0);
          }
        } else if (d.m > 0) {
          associate_correct<W, RS, CS, JOSEPH>(st, sh, A, d.z[0][0], d.z[0][1], d.assoc_slot);
        }
        st.par ^= 1;
        st.dirty = true;
      }
      if ((flags & kLast) || kind == kLaunchPosterior) {  // posterior, slam.cpp:273-291 (deferred)
        // a posterior still owed here (only an ekf_posterior entry leaves one) would be overwritten
        // by this one: the same t_map_odom, but the pose trace owes it a record of its own
        if (st.post && A.trace) posterior_now(st, sh, A, f);
        st.post = true;
        st.podom[0] = d.odom[0];
        st.podom[1] = d.odom[1];
        st.podom[2] = d.odom[2];
      }
    }
  }
  if (st.par < 0) return;  // the plan does not name this filter
  if (st.post) posterior_now(st, sh, A, f);
  store_filter(st, sh, A, ctl, f);
}

hipError_t launch_resident(const PassArgs<double>& a, const PlanEntry* plan, int nplan, int flo,
                           int nfil, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  if (a.n > kResidentMaxN || nfil <= 0) return hipErrorInvalidValue;
  const dim3 grid(nfil);
  auto go = [&](auto kernel, int waves) {
    const dim3 block(64 * waves);
    if (e0 && e1)
      hipExtLaunchKernelGGL(kernel, grid, block, 0, s, e0, e1, 0, a, plan, nplan, flo);
    else
      hipLaunchKernelGGL(kernel, grid, block, 0, s, a, plan, nplan, flo);
  };
  // 4 waves (one per SIMD): the per-correction scalar work (geometry, S, gather control) runs
  // once per wave on the CU's one scalar unit, so fewer, wider waves finish a step sooner
  // Joseph form is its own instantiation: the default update keeps its register budget
  if (a.n <= 64)
    a.joseph ? go(k_resident<4, 16, 1, true>, 4) : go(k_resident<4, 16, 1, false>, 4);
  else if (a.n <= 4 * 26)  // N = 50 (n = 103): no idle row slots
    a.joseph ? go(k_resident<4, 26, 2, true>, 4) : go(k_resident<4, 26, 2, false>, 4);
  else
    a.joseph ? go(k_resident<4, 32, 2, true>, 4) : go(k_resident<4, 32, 2, false>, 4);
  return hipGetLastError();
}

// ---- device-input replays (ekf_replay_resident): the same phases, fed from device memory ----

namespace {

constexpr int kRBlk = 8;  // messages staged per block: two per wave

// A block of one filter's messages as the walk reads them.
struct ReplayShared {
  int m[kRBlk];  // corrections of the message (known ids: its non-DELETE markers); −1: no message
  double odom[kRBlk][3];
  int ids[kRBlk][kMaxAssoc];
  double z[kRBlk][kMaxAssoc][2];  // (range, bearing), slam.cpp:208-210 / :346-347
};

// x·x + y·y rounds product by product, as the host planner's std::pow(x, 2) + std::pow(y, 2)
__device__ __forceinline__ double marker_range(double x, double y) {
#pragma clang fp contract(off)
  return sqrt(x * x + y * y);
}

// The replay's arguments, read where they lie in the kernel's argument segment each time a block
// is staged (and once more for the state hand-over) instead of being held in SGPRs for the whole
// walk: the walk has none to spare, and an SGPR it spills costs the Joseph instantiations a VGPR.
// ReplayKernArgs mirrors k_resident_replay's parameter list (A, R): the argument segment lays
// parameters out like members, each at its own alignment, so R lies at offsetof(…, R) as long as
// the kernel takes exactly these two, in this order (the asserts hold the alignments to that).
struct ReplayKernArgs {
  PassArgs<double> A;
  ResidentReplayArgs R;
};
static_assert(alignof(ResidentReplayArgs) <= 8 && alignof(PassArgs<double>) <= 8 &&
                  sizeof(PassArgs<double>) % alignof(ResidentReplayArgs) == 0 &&
                  offsetof(ReplayKernArgs, R) == sizeof(PassArgs<double>),
              "R follows A in the kernel-argument segment without padding");
typedef const ResidentReplayArgs __attribute__((address_space(4))) * ReplayArgsPtr;
__device__ __forceinline__ ReplayArgsPtr replay_args() {
  typedef const char __attribute__((address_space(4))) * Bytes;
  return reinterpret_cast<ReplayArgsPtr>(
      (Bytes)__builtin_amdgcn_kernarg_segment_ptr() +
      offsetof(ReplayKernArgs, R));
}

// (field by field: the struct's copy constructor takes a generic reference)
__device__ __forceinline__ ResidentReplayArgs fetch_replay_args(ReplayArgsPtr p) {
  asm volatile("" : "+s"(p));  // opaque: the loads stay here, nothing is hoisted out of the walk
  ResidentReplayArgs r;
  r.counts = p->counts;
  r.ids = p->ids;
  r.actions = p->actions;
  r.xy = p->xy;
  r.odom = p->odom;
  r.st_in = p->st_in;
  r.st_out = p->st_out;
  r.T = p->T;
  r.F = p->F;
  r.M = p->M;
  r.stride = p->stride;
  r.assoc = p->assoc;
  return r;
}

// Stage messages [t0, t0 + kRBlk) ∩ [0, T) of filter f: wave w takes messages w and w + W, lane i
// marker i of each (m_max ≤ 64), so every load of the block is in flight at once and every
// (range, bearing) is formed in parallel, behind one barrier pair. Known ids: the non-DELETE
// markers of the first min(count, m_max) are compacted in order by ballot (slam.cpp:205's skip).
// Returns the number of messages staged.
template <int W, bool ASSOC>
__device__ __forceinline__ int stage_replay_block(ReplayShared& rs, ReplayArgsPtr Rp, int t0,
                                                  int f) {
  const ResidentReplayArgs R = fetch_replay_args(Rp);
  const int nb = min(kRBlk, R.T - t0);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  __syncthreads();  // the previous block's messages are consumed
  constexpr int kPer = kRBlk / W;
  int cnt[kPer], id[kPer];
  double x[kPer], y[kPer], od[kPer];
  bool del[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {  // the loads of both messages first
    const int e = w + W * k;
    cnt[k] = 0;
    id[k] = -1;
    del[k] = false;
    x[k] = y[k] = od[k] = 0.0;
    if (e < nb) {
      const size_t tf = static_cast<size_t>(t0 + e) * R.F + f;
      cnt[k] = min(R.counts[tf], R.M);
      if (lane < 3) od[k] = R.odom[tf * 3 + lane];
      if (lane < cnt[k]) {
        const size_t o = tf * R.M + lane;
        x[k] = R.xy[o * R.stride];
        y[k] = R.xy[o * R.stride + 1];
        if constexpr (!ASSOC) {
          id[k] = R.ids[o];
          del[k] = R.actions && R.actions[o] == EKF_MARKER_DELETE;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int e = w + W * k;
    if (e >= nb) continue;
    const bool add = lane < cnt[k] && !del[k];
    const unsigned long long bal = __ballot(add);
    const int pos = static_cast<int>(__popcll(bal & ((1ull << lane) - 1ull)));
    if (add) {
      rs.ids[e][pos] = id[k];
      rs.z[e][pos][0] = marker_range(x[k], y[k]);
      rs.z[e][pos][1] = atan2_rounded(y[k], x[k]);
    }
    if (lane == 0) rs.m[e] = cnt[k] > 0 ? static_cast<int>(__popcll(bal)) : -1;
    if (lane < 3) rs.odom[e][lane] = od[k];
    // one message's bearings at a time: interleaved, the two double-double atan2 take more
    // registers than the Joseph instantiations have left beside Σ
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  return nb;
}

}  // namespace

// One workgroup per filter blockIdx.x walks the replay's T messages in order: per message with
// count > 0 the predict, its corrections (known ids: first sightings initialise, an id outside
// [0, N) is skipped and flagged; unknown: associate_correct, slot = the marker's index) and the
// posterior, deferred to the next gather of the pose as in k_resident. Σ and x are loaded at the
// filter's first message from the copy st_in[f].parity names and stored back once, to that same
// copy: every element is in a register of the thread that stores it, nothing else reads the
// filter during the launch, so the parity does not move. A filter with no message is neither
// loaded nor stored. Every workgroup leaves its filter's PlanState for the host planner.
// The parameter list must stay (A, R), nothing before or between them: R is left unnamed and read
// through replay_args() at its offset in the argument segment (ReplayKernArgs above).
template <int W, int RS, int CS, bool JOSEPH, bool ASSOC>
__global__ __launch_bounds__(W * 64) void k_resident_replay(PassArgs<double> A,
                                                            ResidentReplayArgs) {
  static_assert(RS <= 32 && kRBlk % W == 0, "as k_resident; whole messages per wave");
  ReplayArgsPtr Rp = replay_args();
  const int T = Rp->T;
  __shared__ ResShared<W, RS, CS> sh;
  __shared__ ReplayShared rs;
  const int f = blockIdx.x;
  FilterCtl* ctl = A.ctl + f;
  ResState<W, RS, CS> st;
  st.lane = threadIdx.x & 63;
  st.w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  st.wq = st.w;
  st.rown = st.lane < RS;
  st.rl = st.w + W * (st.rown ? st.lane : RS - 1);

  for (int t0 = 0; t0 < T; t0 += kRBlk) {
    const int nb = stage_replay_block<W, ASSOC>(rs, Rp, t0, f);
    for (int e = 0; e < nb; ++e) {
      const int m = __builtin_amdgcn_readfirstlane(rs.m[e]);
      if (m < 0) continue;  // the filter sits this step out
      if (st.par < 0) load_filter(st, A, ctl, f, Rp->st_in[f].parity);
      predict(st, sh, A, f, rs.odom[e]);
      for (int c = 0; c < m; ++c) {
        const double z0 = rs.z[e][c][0], z1 = rs.z[e][c][1];
        if constexpr (ASSOC) {
          associate_correct<W, RS, CS, JOSEPH>(st, sh, A, z0, z1, c);
        } else {
          const int id = __builtin_amdgcn_readfirstlane(rs.ids[e][c]);
          if (id < 0 || id >= A.N) {  // the inputs are not validated on the host
            st.status |= EKF_FLAG_RANGE_D;
            continue;
          }
          st.b ^= 1;
          gather_rows(st, sh, A.n, st.b, 3 + 2 * id, 0);
          __syncthreads();
          correct<W, RS, CS, JOSEPH>(st, sh, A.r, 3 + 2 * id, z0, z1, false);
        }
      }
      st.dirty = true;
      st.post = true;  // posterior, slam.cpp:273-291 (deferred)
      st.podom[0] = rs.odom[e][0];
      st.podom[1] = rs.odom[e][1];
      st.podom[2] = rs.odom[e][2];
    }
  }
  // the planning state after the replay (the host adopts it lazily): the parity stays, nothing
  // is pipelined, t_odom_robot of the last message, active or not
  if (threadIdx.x < 64) {
    const ResidentReplayArgs R = fetch_replay_args(Rp);
    const PlanState& s0 = R.st_in[f];
    PlanState& so = R.st_out[f];
    const int lane = threadIdx.x;
    if (lane == 0) {
      so.parity = s0.parity;
      so.prev_m = -1;
      so.pending = st.par >= 0 ? 0 : s0.pending;
      so.pad = 0;
      so.pad2 = 0.0;
    }
    if (lane < kMaxChunk) so.prev_ids[lane] = s0.prev_ids[lane];
    if (lane < 3) so.odom[lane] = R.odom[(static_cast<size_t>(R.T - 1) * R.F + f) * 3 + lane];
  }
  if (st.par < 0) return;  // no message for this filter
  if (st.post) posterior_now(st, sh, A, f);
  store_filter(st, sh, A, ctl, f);
}

hipError_t launch_resident_replay(const PassArgs<double>& a, const ResidentReplayArgs& r,
                                  hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  if (a.n > kResidentMaxN || r.F <= 0 || r.T <= 0 || r.M < 1 || r.M > kMaxAssoc || r.stride < 2)
    return hipErrorInvalidValue;
  auto go = [&](auto kernel) { launch(kernel, dim3(r.F), dim3(256), s, e0, e1, a, r); };
  // the shapes of launch_resident; form and association are instantiations of their own, so each
  // keeps its register budget
  auto shape = [&](auto J, auto U) {
    constexpr bool j = decltype(J)::value, u = decltype(U)::value;
    if (a.n <= 64)
      go(k_resident_replay<4, 16, 1, j, u>);
    else if (a.n <= 4 * 26)
      go(k_resident_replay<4, 26, 2, j, u>);
    else
      go(k_resident_replay<4, 32, 2, j, u>);
  };
  using T = std::true_type;
  using N = std::false_type;
  if (a.joseph)
    r.assoc ? shape(T{}, T{}) : shape(T{}, N{});
  else
    r.assoc ? shape(N{}, T{}) : shape(N{}, N{});
  return hipGetLastError();
}

}  // namespace ekfslam
