// Unknown association (Slam::sensor_cb, nuslam/src/slam.cpp:318-530) for a whole chunk of markers
// in ONE launch, followed by a single Σ pass — instead of an association kernel, a chain, a factor
// kernel and a Σ pass per marker.
//
// Why it works. A chunk's corrections are Σ_{c+1} = Σ_c − K_c·M_c (slam.cpp:264-265, rank 2 each)
// on the predicted Σ_p (slam.cpp:321-335). Marker c's association (slam.cpp:358-440) reads, for every
// known landmark k, only the 5 × 5 block of Σ_c over {θ, x, y, kx, ky} and x_c at those indices. Those
// 16 entries per landmark evolve by the same rank-2 terms, so each landmark can carry its own block:
//   Σ_{c+1}[k, k] = Σ_c[k, k] − K_c[k]·M_c[:, k],  Σ_{c+1}[k, p] = Σ_c[k, p] − K_c[k]·M_c[:, p], …
// with K_c[k] = Σ_c[k, pA]·Hᵀ·S⁻¹ and M_c[:, k] = H·Σ_c[pA, k] over pA = {θ, x, y, jx, jy}. The only
// entries of Σ_c outside the blocks that a step needs are the crosses with its landmark j:
//   Σ_c[k, j] = Σ_p[k, j] − Σ_{c'<c} K_{c'}[k]·M_{c'}[:, j],   Σ_c[j, k] likewise,
// i.e. Σ_in (no predict term between landmarks) and the factor histories of k and of j. So:
//   * one lane per landmark slot, 64 slots per workgroup (wave 0; waves 1-2 only sum the history
//     terms, history_helper), G = ⌈N / 64⌉ workgroups per
//     filter; a lane keeps its slot's block and state in registers and its K / M history in LDS;
//   * per marker: every lane scores its landmark (k_assoc's expression, ekf_math.hpp assoc_dist),
//     a wave argmin (first index on ties, arma::index_min), then the G workgroups exchange their
//     (d, k) as tagged 8-byte granules (cdna_hip_programming.md Guideline 16, R2) and every one
//     takes the same decision: commit a new landmark (slam.cpp:421-422) or the argmin;
//   * the chosen landmark's block, state and history are read from write-through tables (every
//     lane publishes its slot's K, M and next block each step, drained before the granule), its
//     crosses with each lane's landmark are gathered from Σ_in; every workgroup then forms the same
//     S, S⁻¹, ν, K[pose], M[pose] and each lane its own K[k], M[k] — the chunk's Kcat / Mcat rows
//     for the Σ pass — and applies the step to its block and state.
// The Σ pass (k_sigma_pass, ekf_sigma_pass.hip) then applies Σ_out = Σ_in + Q̄ − Kcatᵀ·Mcat once.
// fp32 Σ: a chunk that commits a new landmark also writes the final Σ[U, U] in fp64 (ChunkRec::Pend,
// the first sighting's 1e7 − (1e7 − δ), slam.cpp:130) for the Σ pass's fp32 tiles, after a last
// exchange.
//
// In exact arithmetic this equals the reference's sequential dense algebra; the decisions are the
// reference's (tests/test_gpu_scale.py: every decision equal to the oracle's, new and known
// landmarks, a marker 3e-4 from the gate).
//
// In the source, in execution order. k_assoc_msg is the setup (filter_view: the filter's pointers
// and table descriptors; same_xcd), the predict (predict_pose_block, slot_block), the marker loop,
// the epilogue and the fp32 patch; every phase is a __forceinline__ function, and the loop body
// keeps both workgroup barriers and the diagnostic stamps:
//   score_slot (block5, assoc_dist) → wave_argmin → filter_argmin (exchange, uniform read-back) →
//   decide → fetch_landmark (G > 1: the tables; G == 1: readlane_slot) → barrier A → pose_step →
//   barrier B → slot_step, pose_update → write_step_factors → put_cur;
//   waves 1-2 run history_helper between the same barriers.
// Then write_predict_factors (and the new state), finish_filter and write_pend_patch. Shared
// algebra: times_H (a row times H), gain_row (K = q·S⁻¹, V), km_vk_sub (− K·M − V·Kᵀ), put_factor /
// put_predict_column (Kcat / Mcat rows of one state column), wave_lds_publish. A slot's live
// state is a Slot (AmCur's order; slot_pack / slot_unpack to its 18 doubles).
//
// The file's end holds the other unknown-association kernel, k_assoc: one marker per launch, each
// followed by a single-marker chunk (chain, factors, Σ pass) — the route the host takes when
// k_assoc_msg's workgroups cannot all be resident (ekf_sched.cpp am_route) or with EKF_ASSOC_MSG=0.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ekf_device.hpp"
#include "ekf_launch.hpp"
#include "ekf_math.hpp"
#include "geom.hpp"

namespace ekfslam {

#include "ekf_sync.hpp"

// Diagnostic build only (tools/assoc_stamps.py): s_memrealtime (100 MHz) of workgroup 0 / the last
// workgroup, lane 0, per step and phase, of the last launch.
#ifdef EKF_DIAG_STAMPS
__device__ unsigned long long g_am_stamps[2][kMaxChunk + 1][8];
#define AM_STAMP(c, i)                                                                    \
  do {                                                                                    \
    if (blockIdx.y == 0 && threadIdx.x == 0 && (g == 0 || g == G - 1))                    \
      g_am_stamps[g == 0 ? 0 : 1][c][i] = __builtin_amdgcn_s_memrealtime();               \
  } while (0)
#else
#define AM_STAMP(c, i) \
  do {                 \
  } while (0)
#endif

namespace {


// Three waves per workgroup: wave 0 does everything below; waves 1 and 2 (history_helper) only sum
// each step's history terms of the lanes' crosses with the step's landmark (Σ_c[k, j], Σ_c[j, k]),
// the even steps' on wave 1 and the odd steps' on wave 2 — the two fma chains wave 0 interleaved
// alone before, so the same bits — while wave 0 forms the step's pose-level quantities, which do
// not need them.
constexpr int kAmThreads = 3 * kAmSlots;

// A landmark slot's live state: its 16 entries of Σ over {θ, x, y, kx, ky} (kk = Σ[k][k],
// kp = Σ[k][pose], pk = Σ[pose][k]) and its state, in AmCur's order. As 18 doubles (slot_pack /
// slot_unpack) it is an AmCur row's payload, sh.jc and a row of sh.pb.
struct Slot {
  double kk[4], kp[6], pk[6], x[2];
};
constexpr int kSlotW = 18, kSlotKp = 4, kSlotPk = 10, kSlotX = 16;  // (kk at 0)
__device__ __forceinline__ void slot_pack(const Slot& s, double (&v)[kSlotW]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) v[t] = s.kk[t];
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    v[kSlotKp + t] = s.kp[t];
    v[kSlotPk + t] = s.pk[t];
  }
  v[kSlotX] = s.x[0];
  v[kSlotX + 1] = s.x[1];
}
__device__ __forceinline__ void slot_unpack(const double* v, Slot& s) {
#pragma unroll
  for (int t = 0; t < 4; ++t) s.kk[t] = v[t];
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    s.kp[t] = v[kSlotKp + t];
    s.pk[t] = v[kSlotPk + t];
  }
  s.x[0] = v[kSlotX];
  s.x[1] = v[kSlotX + 1];
}
// Lane l's slot (l wave-uniform: v_readlane) as 18 doubles at dst, stored by lane 0
__device__ __forceinline__ void readlane_slot(const Slot& s, int l, int lane, double* dst) {
  double v[kSlotW];
  slot_pack(s, v);
#pragma unroll
  for (int t = 0; t < kSlotW; ++t) v[t] = readlane_f64(v[t], l);
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < kSlotW; ++t) dst[t] = v[t];
  }
}
// The 5 × 5 block of Σ over {θ, x, y, kx, ky} from the pose block and a slot
__device__ __forceinline__ void block5(const double (&Pp)[3][3], const Slot& s, double (&P)[5][5]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) P[a][b] = Pp[a][b];
    P[a][3] = s.pk[2 * a];
    P[a][4] = s.pk[2 * a + 1];
    P[3][a] = s.kp[a];
    P[4][a] = s.kp[3 + a];
  }
  P[3][3] = s.kk[0];
  P[3][4] = s.kk[1];
  P[4][3] = s.kk[2];
  P[4][4] = s.kk[3];
}

// J: the Joseph form (ekf_set_joseph; every descriptor kJoseph). Each step then also subtracts
// V_c·K_cᵀ, V_c = Σ_c·Hᵀ − K_c·S_c (slam.cpp:264-265's update as (I − KH)Σ(I − KH)ᵀ + K·R·Kᵀ
// expanded, as k_chain's Joseph form), after the K_c·M_c term: the history carries V too.
template <bool J>
struct AmSharedT {
  static constexpr int HW = J ? 12 : 8;  // history doubles per (step, slot): K, M (, V)
  alignas(16) double hkm[kMaxChunk][kAmSlots][HW];  // wave 0's K_c[k] (0..3), M_c[:, k] (4..7)
                                       // (and V_c[k], 8..11), by lane: a lane's step in 64 (96)
                                       // contiguous bytes (ds_read_b128 × 4 (6))
  double es[2][8][kAmSlots];          // waves 1 / 2: the even / odd steps' history sums, by lane
  double jh[kMaxChunk][HW];           // the step's landmark: K (0..3), M (4..7) (, V) of every step
  double jc[18];                      // its block and state (AmCur, x included)
  double pb[kMaxChunk][18];           // fp32 patch: every marker's landmark's final block
  double pp[9];                       // fp32 patch: the final pose block
  int jl[kMaxChunk];                  // the chunk's landmark per marker (−1: skipped)
};

// The predicted pose block (slam.cpp:321-335): At·Σ·Atᵀ over {θ, x, y} (At has α only in rows
// 1, 2; α = 0 without kFirst, predicted_pose) plus Q on the diagonal of a message's first chunk.
template <typename T>
__device__ __forceinline__ void predict_pose_block(const T* S, int ld, double a1, double a2,
                                                   bool first, double q, double (&Pp)[3][3]) {
  double raw[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) raw[a][b] = static_cast<double>(S[a * ld + b]);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double aa = alpha_of(a, a1, a2), ab = alpha_of(b, a1, a2);
      double v = raw[a][b] + aa * raw[0][b];
      v = v + (raw[a][0] + aa * raw[0][0]) * ab;
      if (first && a == b) v += q;
      Pp[a][b] = v;
    }
}  // (raw: re-read for the factor rows at the end, not kept live through the steps)

// The lane's predicted block of slot entries: Σ_p[k][b] = Σ[k][b] + Σ[k][0]·α_b,
// Σ_p[a][k] = Σ[a][k] + α_a·Σ[0][k] (At has α only in rows 1, 2). Both kernels' gather.
template <typename T>
__device__ __forceinline__ void slot_block(const T* S, int ld, int ix, double a1, double a2,
                                           Slot& s) {
  const T* q0 = S + static_cast<size_t>(ix) * ld;
  const T* q1 = q0 + ld;
  double rk[2][3], rp[3][2];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    rk[0][b] = static_cast<double>(q0[b]);
    rk[1][b] = static_cast<double>(q1[b]);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    rp[a][0] = static_cast<double>(S[a * ld + ix]);
    rp[a][1] = static_cast<double>(S[a * ld + ix + 1]);
  }
  s.kk[0] = static_cast<double>(q0[ix]);
  s.kk[1] = static_cast<double>(q0[ix + 1]);
  s.kk[2] = static_cast<double>(q1[ix]);
  s.kk[3] = static_cast<double>(q1[ix + 1]);
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int b = 0; b < 3; ++b) s.kp[3 * e + b] = rk[e][b] + rk[e][0] * alpha_of(b, a1, a2);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int e = 0; e < 2; ++e) s.pk[2 * a + e] = rp[a][e] + alpha_of(a, a1, a2) * rp[0][e];
}

__device__ __forceinline__ unsigned long long ld_sc1_u64(const unsigned long long* p) {
  return __hip_atomic_load((const gu64*)(p), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// Coherence of what a filter's G workgroups exchange within a launch (granules, tables). Loads are
// sc1 in both modes: they miss the CU's L1 and read the XCD's L2 coherently. Stores:
//  - agent mode (any placement): sc1, written through past the XCD's L2 to memory, where a reader
//    on another XCD finds them;
//  - XCD-local mode (all G workgroups on one XCD, established by `same_xcd` at the launch's start):
//    plain, so they stop in the L2 the workgroups share (the CU's L1 is write-through).
// Measured (tools/xcd_probe.hip, one-way hand-off between two CUs): same XCD, plain store + sc1
// load 224 ns, sc1 store + sc1 load 414 ns; across XCDs sc1 + sc1 564 ns (plain stores are never
// seen there); sc0 loads hit a stale L1 line forever. Every value a local-mode launch reads was
// written in that launch by a CU of the same XCD, so a stale L2 line from an earlier launch is
// never read (the granules carry the launch's tag).
// Loads go through a buffer descriptor of the filter's table (wave-uniform) with the entry's byte
// offset per lane.
constexpr int kAuxSc1 = 16;
__device__ __forceinline__ unsigned long long ld_x64(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(unsigned long long,
                            __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, kAuxSc1));
}
__device__ __forceinline__ double ld_xf64(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __longlong_as_double(static_cast<long long>(ld_x64(r, off)));
}
__device__ __forceinline__ void st_x64(unsigned long long* p, unsigned long long v, bool loc) {
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  if (loc)  // a plain store (no cache-policy bits), as the probe's
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), buf_rsrc(p, 8), 0, 0, 0);
  else
    __hip_atomic_store((gu64*)(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 16-byte table store: write-through past L2 (agent mode) or into the shared L2 (XCD-local)
template <bool LOC>
__device__ __forceinline__ void st_x2(__amdgpu_buffer_rsrc_t r, int off, double a, double b) {
  if (LOC) {
    typedef int i4 __attribute__((ext_vector_type(4)));
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i4, make_double2(a, b)), r, off, 0, 0);
  } else {
    st_wt2(r, off, a, b);
  }
}

// This lane's rows of the write-through tables. The buffer descriptor is built from the
// workgroup's block of 64 rows (wave-uniform, so it stays in SGPRs); the lane's row is the voffset.
// (A per-lane descriptor made hipcc wrap every store in a 64-iteration waterfall loop: ≈ 30 µs per
// step.)
template <bool LOC>
__device__ __forceinline__ void put_cur_m(AmCur* blk, int lane, const Slot& s) {
  const auto r = buf_rsrc(blk, kAmSlots * sizeof(AmCur));
  const int o = lane * static_cast<int>(sizeof(AmCur));
  double v[kSlotW];
  slot_pack(s, v);
#pragma unroll
  for (int t = 0; t < kSlotW; t += 2) st_x2<LOC>(r, o + 8 * t, v[t], v[t + 1]);
}
template <bool LOC>
__device__ __forceinline__ void put_hist_m(AmHist* blk, int lane, const double* h, int hw) {
  const auto r = buf_rsrc(blk, kAmSlots * sizeof(AmHist));
  const int o = lane * static_cast<int>(sizeof(AmHist));
  for (int t = 0; t < hw; t += 2) st_x2<LOC>(r, o + 8 * t, h[t], h[t + 1]);  // (hw: 8 or 12)
}

__device__ __forceinline__ void put_cur(AmCur* blk, int lane, const Slot& s, bool loc) {
  if (loc) put_cur_m<true>(blk, lane, s);
  else put_cur_m<false>(blk, lane, s);
}
// h: K (4), M (4) and, hw = 12, V (4) — the lane's LDS history row layout
__device__ __forceinline__ void put_hist(AmHist* blk, int lane, const double* h, int hw, bool loc) {
  if (loc) put_hist_m<true>(blk, lane, h, hw);
  else put_hist_m<false>(blk, lane, h, hw);
}

// The G workgroups of a filter publish their (d, k) for exchange `c` and wait for everyone's:
// three 8-byte {tag, value} granules per workgroup (d's two halves, k), stored by lane 0 after the
// wave's write-through table stores have drained; lanes < G poll one workgroup's each. Returns the
// filter-wide argmin (the same in every workgroup), or a partial argmin and *timeout after `spin`
// polls — the filter's state is then undefined (EKF_FLAG_TIMEOUT, reported by the host as
// EKF_E_TIMEOUT). `drop`: fault injection, this workgroup does not publish (tests only).
__device__ __forceinline__ void exchange(unsigned long long* gran, int G, int g, int c,
                                         unsigned tag, double& d, int& k, bool* timeout, bool loc,
                                         unsigned spin, bool drop = false) {
  drain_stores();  // R1: this wave's table stores of the step are complete before its granule
  const int lane = threadIdx.x;
  unsigned long long* mine = gran + (static_cast<size_t>(c) * G + g) * 4;
  const unsigned long long hi = static_cast<unsigned long long>(tag) << 32;
  const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(d));
  if (lane == 0 && !drop) {
    st_x64(mine + 0, hi | (bits & 0xffffffffull), loc);
    st_x64(mine + 1, hi | (bits >> 32), loc);
    st_x64(mine + 2, hi | static_cast<unsigned>(k), loc);
  }
  const auto gr = buf_rsrc(gran, static_cast<unsigned>((kMaxChunk + 1) * G * 4 * 8));
  double od = INFINITY;
  int ok = INT_MAX;
  for (int base = 0; base < G; base += 64) {
    const int w = base + lane;
    const unsigned src = static_cast<unsigned>(((c * G + (w < G ? w : 0)) * 4) * 8);
    for (unsigned spins = 0;; ++spins) {
      bool got = true;
      unsigned long long v0 = 0, v1 = 0, v2 = 0;
      if (w < G) {
        v0 = ld_x64(gr, src + 0);
        v1 = ld_x64(gr, src + 8);
        v2 = ld_x64(gr, src + 16);
        got = (v0 >> 32) == tag && (v1 >> 32) == tag && (v2 >> 32) == tag;
      }
      if (__all(got)) {
        if (w < G) {
          const double dv = __longlong_as_double(
              static_cast<long long>(((v1 & 0xffffffffull) << 32) | (v0 & 0xffffffffull)));
          const int kv = static_cast<int>(static_cast<unsigned>(v2));
          if (dv < od || (dv == od && kv < ok)) {
            od = dv;
            ok = kv;
          }
        }
        break;
      }
      if (spins >= spin) {
        *timeout = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  // loads of the published tables come after the poll (sc1: they bypass this CU's L1)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  wave_argmin(od, ok);
  d = od;
  k = ok;
}

// Roll call of a launch in XCD-local placement: every workgroup of the filter publishes its XCD
// (HW_REG_XCC_ID) in word 3 of its step-0 granule, agent-coherent; workgroup 0 reads all G and
// publishes the launch's transport in word 3 of its step-1 granule (unused by the exchanges), and
// every other workgroup takes that one decision. XCD-local only if all G sit on one XCD; so every
// workgroup runs the same transport, also when a poll times out (workgroup 0 then publishes the
// agent transport; a workgroup that never sees the decision takes it too, and the timeout is
// flagged: EKF_FLAG_TIMEOUT, the filter's state is undefined).
__device__ bool same_xcd(unsigned long long* gran, int G, int g, unsigned tag, bool* timeout,
                         unsigned spin) {
  const unsigned xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (15 << 11)) & 0xffffu;
  const int lane = threadIdx.x;
  const unsigned long long hi = static_cast<unsigned long long>(tag) << 32;
  unsigned long long* decision = gran + static_cast<size_t>(G) * 4 + 3;  // (c = 1, g = 0) word 3
  if (lane == 0) st_x64(gran + static_cast<size_t>(g) * 4 + 3, hi | xcc, false);
  if (g != 0) {
    for (unsigned spins = 0;; ++spins) {
      const unsigned long long v = ld_sc1_u64(decision);
      if ((v >> 32) == tag) return (v & 1ull) != 0;  // (the same address in every lane: uniform)
      if (spins >= spin) {
        *timeout = true;
        return false;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  bool same = true;
  for (int base = 0; base < G; base += 64) {
    const int w = base + lane;
    const unsigned long long* src = gran + static_cast<size_t>(w < G ? w : 0) * 4 + 3;
    for (unsigned spins = 0;; ++spins) {
      bool got = true;
      unsigned long long v = 0;
      if (w < G) {
        v = ld_sc1_u64(src);
        got = (v >> 32) == tag;
      }
      if (__all(got)) {
        if (w < G) same = same && static_cast<unsigned>(v & 0xffffu) == xcc;
        break;
      }
      if (spins >= spin) {
        *timeout = true;
        same = false;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  const bool all = __all(same) != 0;
  if (lane == 0) st_x64(decision, hi | (all ? 1ull : 0ull), false);
  return all;
}

// One history term of a lane's crosses with the step's landmark j: acc[0..3] += K_cc[k]·M_cc[:, j],
// acc[4..7] += K_cc[j]·M_cc[:, k] (slam.cpp:264-265's rank-2 terms at (k, j) and (j, k)). The
// operands (this lane's history, 4 × ds_read_b128, and j's, broadcast) are loaded apart from the
// fmas so that several terms' reads can be in flight together.
template <bool J>
struct HistOps {
  static constexpr int kV = AmSharedT<J>::HW / 2;
  double2 o[kV], jv[kV];
};
template <bool J>
__device__ __forceinline__ void hist_load(const AmSharedT<J>& sh, int cc, int lane, HistOps<J>& p) {
  const double2* hl = reinterpret_cast<const double2*>(sh.hkm[cc][lane]);
  const double2* jl = reinterpret_cast<const double2*>(sh.jh[cc]);
#pragma unroll
  for (int i = 0; i < HistOps<J>::kV; ++i) {
    p.o[i] = hl[i];
    p.jv[i] = jl[i];
  }
}
template <bool J>
__device__ __forceinline__ void hist_fma(const HistOps<J>& p, double (&acc)[8]) {
  const double ok0 = p.o[0].x, ok1 = p.o[0].y, ok2 = p.o[1].x, ok3 = p.o[1].y;
  const double om0 = p.o[2].x, om1 = p.o[2].y, om2 = p.o[3].x, om3 = p.o[3].y;
  const double jk[4] = {p.jv[0].x, p.jv[0].y, p.jv[1].x, p.jv[1].y};
  const double jm[4] = {p.jv[2].x, p.jv[2].y, p.jv[3].x, p.jv[3].y};
  acc[0] = fma(ok1, jm[2], fma(ok0, jm[0], acc[0]));
  acc[1] = fma(ok1, jm[3], fma(ok0, jm[1], acc[1]));
  acc[2] = fma(ok3, jm[2], fma(ok2, jm[0], acc[2]));
  acc[3] = fma(ok3, jm[3], fma(ok2, jm[1], acc[3]));
  acc[4] = fma(jk[1], om2, fma(jk[0], om0, acc[4]));
  acc[5] = fma(jk[1], om3, fma(jk[0], om1, acc[5]));
  acc[6] = fma(jk[3], om2, fma(jk[2], om0, acc[6]));
  acc[7] = fma(jk[3], om3, fma(jk[2], om1, acc[7]));
  if constexpr (J) {  // + V_cc[k]·K_cc[j]ᵀ at (k, j) and V_cc[j]·K_cc[k]ᵀ at (j, k)
    const double ov0 = p.o[4].x, ov1 = p.o[4].y, ov2 = p.o[5].x, ov3 = p.o[5].y;
    const double jv0 = p.jv[4].x, jv1 = p.jv[4].y, jv2 = p.jv[5].x, jv3 = p.jv[5].y;
    acc[0] = fma(ov1, jk[1], fma(ov0, jk[0], acc[0]));
    acc[1] = fma(ov1, jk[3], fma(ov0, jk[2], acc[1]));
    acc[2] = fma(ov3, jk[1], fma(ov2, jk[0], acc[2]));
    acc[3] = fma(ov3, jk[3], fma(ov2, jk[2], acc[3]));
    acc[4] = fma(jv1, ok1, fma(jv0, ok0, acc[4]));
    acc[5] = fma(jv1, ok3, fma(jv0, ok2, acc[5]));
    acc[6] = fma(jv3, ok1, fma(jv2, ok0, acc[6]));
    acc[7] = fma(jv3, ok3, fma(jv2, ok2, acc[7]));
  }
}

// Waves 1 (par 0) and 2 (par 1): per step, after wave 0 has published j (sh.jl) and j's history
// (sh.jh) — barrier A — this lane's sums over the steps cc < c with cc ≡ par (mod 2) of
// K_cc[k]·M_cc[:, j] and K_cc[j]·M_cc[:, k] into sh.es[par], read by wave 0 after barrier B. Every
// wave passes both barriers at every step, whatever the step decides.
template <bool J>
__device__ __forceinline__ void history_helper(AmSharedT<J>& sh, int m, int k, int lane, int par) {
  for (int c = 0; c < m; ++c) {
    lds_barrier();  // A
    const int j = sh.jl[c];
    double e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (j >= 0) {  // (uniform; the lane k = j ignores its sums)
      int cc = par;
      for (; cc + 6 < c; cc += 8) {  // four terms' reads in flight, then their fmas in order
        HistOps<J> p0, p1, p2, p3;
        hist_load(sh, cc, lane, p0);
        hist_load(sh, cc + 2, lane, p1);
        hist_load(sh, cc + 4, lane, p2);
        hist_load(sh, cc + 6, lane, p3);
        hist_fma(p0, e);
        hist_fma(p1, e);
        hist_fma(p2, e);
        hist_fma(p3, e);
      }
      for (; cc < c; cc += 2) {
        HistOps<J> p0;
        hist_load(sh, cc, lane, p0);
        hist_fma(p0, e);
      }
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) sh.es[par][t][lane] = e[t];
    lds_barrier();  // B
  }
}

// ---- k_assoc_msg's phases (wave 0), in execution order. None holds a workgroup barrier. ----

// The filter's buffers and table descriptors, and this lane's place in it
template <typename T>
struct AmFilter {
  const T* S;         // Σ_in
  const double* xin;
  double* xout;
  T *kc, *mc;         // Kcat, Mcat
  FilterCtl* ctl;
  AmHist* hist;
  AmCur* cur;
  unsigned long long* gran;
  __amdgpu_buffer_rsrc_t cur_r, hist_r;  // (wave-uniform, for the sc1 loads of j's rows)
  int ld, ldk, G, g, Np, lane, k, ix;    // k: the lane's slot; ix: its state index
  bool valid, loc;                       // k < N; the XCD-local transport (same_xcd)
};
template <typename T>
__device__ __forceinline__ AmFilter<T> filter_view(const PassArgs<T>& A, const AmArgs& B,
                                                   const MsgDesc& d, int f, int g, int lane) {
  AmFilter<T> F;
  F.ld = A.ld, F.ldk = A.ldk, F.G = B.G, F.g = g, F.Np = B.G * kAmSlots, F.lane = lane;
  F.k = g * kAmSlots + lane;
  F.valid = F.k < A.N;
  F.ix = 3 + 2 * (F.valid ? F.k : A.N - 1);  // (clamped for the loads)
  F.loc = false;
  F.S = A.sig[d.parity] + f * A.sig_stride;
  F.xin = A.x[d.parity] + f * A.x_stride;
  F.xout = A.x[d.parity ^ 1] + f * A.x_stride;
  F.kc = A.kcat + f * A.km_stride;
  F.mc = A.mcat + f * A.km_stride;
  F.ctl = A.ctl + f;
  F.hist = B.hist + f * B.hist_stride;
  F.cur = B.cur + f * B.cur_stride;
  F.gran = B.gran + f * B.gran_stride;
  F.cur_r = buf_rsrc(F.cur, static_cast<unsigned>(B.cur_stride * sizeof(AmCur)));
  F.hist_r = buf_rsrc(F.hist, static_cast<unsigned>(B.hist_stride * sizeof(AmHist)));
  return F;
}

// The chunk's running state: the landmark counter, status flags, whether the fp32 block needs its
// patch, and whether an exchange timed out
struct AmChunk {
  unsigned s, status;
  bool any_new, timeout;
};

// H's shape (range_bearing): H0 = [0, h1, h2, −h1, −h2], H1 = [−1, g1, g2, −g1, −g2] (exact
// negations), so a row (v0, …, v4) times Hᵀ is two fmas on d1 = v1 − v3, d2 = v2 − v4, as in the
// chain's step; a column times H likewise.
struct HRows {
  double h1, h2, g1, g2;
};
__device__ __forceinline__ void times_H(const HRows& H, double v0, double d1, double d2,
                                        double& o0, double& o1) {
  o0 = fma(H.h2, d2, H.h1 * d1);
  o1 = fma(H.g2, d2, fma(H.g1, d1, -v0));
}
// K = q·S⁻¹ for a row q of Σ·Hᵀ and, Joseph, V = q − K·S (k_chain's V expression). Of a sum of
// two products one is rounded and the other fused onto it; written as `a * b + c * d` the compiler
// picks which by where the operands were defined, so moving the text flips it. The fmas below are
// what the unsplit kernel's binary did: the second product rounded, except in V at the slot (SLOT).
template <bool J, bool SLOT>
__device__ __forceinline__ void gain_row(double q0, double q1, const double (&Si)[4],
                                         const double (&S)[4], double (&K)[2], double (&V)[2]) {
  K[0] = fma(q0, Si[0], q1 * Si[2]);
  K[1] = fma(q0, Si[1], q1 * Si[3]);
  if (J) {
    V[0] = q0 - (SLOT ? fma(K[1], S[2], K[0] * S[0]) : fma(K[0], S[0], K[1] * S[2]));
    V[1] = q1 - (SLOT ? fma(K[1], S[3], K[0] * S[1]) : fma(K[0], S[1], K[1] * S[3]));
  }
}
// Σ[a][b] − K[a]·M[:, b] and, Joseph, then − V[a]·K[b]ᵀ (slam.cpp:482-488 at one entry)
template <bool J>
__device__ __forceinline__ double km_vk_sub(double v, const double (&Ka)[2], double m0, double m1,
                                            const double (&Va)[2], const double (&Kb)[2]) {
  v = rank2_sub(v, Ka[0], Ka[1], m0, m1);
  if (J) v = rank2_sub(v, Va[0], Va[1], Kb[0], Kb[1]);
  return v;
}

// What every lane of every workgroup shares in a step: the decision and the pose-level quantities
struct AmStep {
  int j;            // the step's landmark (−1: the marker is skipped)
  bool isnew, ok;   // committed by this marker; S was invertible (the step is applied)
  double nx, ny;    // a new landmark's state (slam.cpp:351-354)
  HRows H;
  double Si[4], Sv[4], nu0, nu1;           // S⁻¹, S (Joseph), ν
  double Kp[3][2], Mp[2][3], Vp[3][2];     // K, M and (Joseph) V = Σ·Hᵀ − K·S at the pose
};
// A lane's factors of the step: K[k], M[:, k] and (Joseph) V[k] (AmHist's order)
struct LaneKM {
  double K[2][2], M[2][2], V[2][2];
};

// Wave-local LDS hand-off between lanes of wave 0 (no other wave reads what it orders)
__device__ __forceinline__ void wave_lds_publish() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// Marker c's distance to this lane's landmark (slam.cpp:361-416)
__device__ __forceinline__ double score_slot(const double (&Pp)[3][3], const Slot& sl,
                                             const double* pose, double z0, double z1,
                                             double r_noise) {
  double P[5][5];
  block5(Pp, sl, P);
  const double dist = assoc_dist(P, pose, sl.x[0], sl.x[1], z0, z1, r_noise);
  return dist < INFINITY ? dist : INFINITY;  // NaN never wins (strict <, k_assoc)
}

// The workgroup's argmin (after wave_argmin) becomes the filter's: the exchange between the G
// workgroups, then the pair read back wave-uniform (every lane holds the same argmin).
template <typename T>
__device__ __forceinline__ void filter_argmin(const AmFilter<T>& F, int c, unsigned tag, bool full,
                                              unsigned spin, bool drop, double& key, int& kbest,
                                              bool* timeout) {
  if (F.G > 1 && !full)
    exchange(F.gran, F.G, F.g, c, tag, key, kbest, timeout, F.loc, spin, drop);
  key = readfirstlane_f64(key);
  kbest = __builtin_amdgcn_readfirstlane(kbest);
}

// The decision (slam.cpp:418-440): the new slot (index s, d = gate) wins only over a strictly
// larger existing minimum; a full map is the reference's out-of-range state index. Published to
// waves 1-2 (sh.jl) and, by workgroup 0, to the host (FilterCtl::assoc_j / assoc_new).
template <typename T, bool J>
__device__ __forceinline__ void decide(AmSharedT<J>& sh, const AmFilter<T>& F, const MsgDesc& d,
                                       int c, bool full, double key, int kbest, double gate,
                                       AmChunk& ch, AmStep& st) {
  st.isnew = false;
  if (full) {
    st.j = -1;
    ch.status |= EKF_FLAG_RANGE_D;
  } else if (!(key <= gate)) {
    st.j = static_cast<int>(ch.s);
    st.isnew = true;
    ++ch.s;
    ch.any_new = true;
  } else {
    st.j = kbest;
  }
  if (F.lane == 0) {
    sh.jl[c] = st.j;
    if (F.g == 0) {
      const int slot = (d.assoc_slot + c) & (kMaxAssoc - 1);
      F.ctl->assoc_j[slot] = st.j;
      F.ctl->assoc_new[slot] = st.isnew ? 1 : 0;
    }
  }
}

// j's block, state and history into sh.jc / sh.jh, and this lane's Σ_in crosses with j. G > 1: one
// round of sc1 loads of the write-through tables, one entry per lane; G == 1: j's lane holds its
// block (v_readlane) and its history is in LDS. A new landmark's state (the pose before this
// marker's correction) goes to st.nx / st.ny and into its own lane's slot.
template <typename T, bool J>
__device__ __forceinline__ void fetch_landmark(AmSharedT<J>& sh, const AmFilter<T>& F, int c,
                                               const double* pose, double z0, double z1, AmStep& st,
                                               Slot& sl, double (&rkj)[4], double (&rjk)[4]) {
  constexpr int HW = AmSharedT<J>::HW;
  const int j = st.j, jx = 3 + 2 * j, lane = F.lane, ix = F.ix, ld = F.ld, G = F.G;
  if (st.isnew) {  // (uniform)
    st.nx = pose[1] + z0 * cos(z1 + pose[0]);
    st.ny = pose[2] + z0 * sin(z1 + pose[0]);
    if (F.k == j) {
      sl.x[0] = st.nx;
      sl.x[1] = st.ny;
    }
  }
  constexpr int kJL = (kSlotW + HW * (kMaxChunk - 1) + 63) / 64;  // 3 (Joseph: 4)
  double vc = 0.0, v[kJL];  // this lane's entry of j's block (lanes 0..17), of its history
  const unsigned jco = static_cast<unsigned>((c * F.Np + j) * sizeof(AmCur));
  // (the block's load apart from the history's: from the two branches of one if / else the
  // compiler sinks the loads into one with a per-lane choice of descriptor, a waterfall loop; into
  // one variable from two ifs, the second load waits for the first)
  if (G > 1 && lane < kSlotW) vc = ld_xf64(F.cur_r, jco + 8 * lane);
#pragma unroll
  for (int i = 0; i < kJL; ++i) {
    const int e = lane + 64 * i;  // from 18 on: HW per earlier step
    v[i] = 0.0;
    if (G > 1 && e >= kSlotW && e < kSlotW + HW * c) {
      const int cc = (e - kSlotW) / HW, t = (e - kSlotW) % HW;  // AmHist: k[4], m[4] (, v[4])
      v[i] = ld_xf64(F.hist_r, static_cast<unsigned>((cc * F.Np + j) * sizeof(AmHist) + 8 * t));
    }
  }
  // Σ_in crosses of this lane's slot with j (no predict term between landmarks)
  const T* q0 = F.S + static_cast<size_t>(ix) * ld;
  const T* p0 = F.S + static_cast<size_t>(jx) * ld;
  rkj[0] = static_cast<double>(q0[jx]);
  rkj[1] = static_cast<double>(q0[jx + 1]);
  rkj[2] = static_cast<double>(q0[ld + jx]);
  rkj[3] = static_cast<double>(q0[ld + jx + 1]);
  rjk[0] = static_cast<double>(p0[ix]);
  rjk[1] = static_cast<double>(p0[ix + 1]);
  rjk[2] = static_cast<double>(p0[ld + ix]);
  rjk[3] = static_cast<double>(p0[ld + ix + 1]);
  if (G > 1) {
#pragma unroll
    for (int i = 0; i < kJL; ++i) {
      const int e = lane + 64 * i;
      if (e < kSlotW) sh.jc[e] = vc;
      else if (e < kSlotW + HW * c) sh.jh[(e - kSlotW) / HW][(e - kSlotW) % HW] = v[i];
    }
  } else {
    readlane_slot(sl, j, lane, sh.jc);
    for (int e = lane; e < HW * c; e += 64) {
      const int cc = e / HW, t = e % HW;
      sh.jh[cc][t] = sh.hkm[cc][j][t];
    }
  }
}

// What every lane shares in the step (slam.cpp:443-488), from j's block in sh.jc: ẑ, H, S, S⁻¹, ν
// and K / M (/ V) at the pose. st.ok stays false when S is singular: Armadillo's inv throws and
// the marker is skipped.
template <typename T, bool J>
__device__ __forceinline__ void pose_step(const AmSharedT<J>& sh, const double (&Pp)[3][3],
                                          const double* pose, double z0, double z1, double r_noise,
                                          double prior, AmChunk& ch, AmStep& st) {
  Slot sj;
  slot_unpack(sh.jc, sj);
  if (st.isnew) {
    sj.x[0] = st.nx;
    sj.x[1] = st.ny;
  }
  // fp32 Σ: a mapped landmark still at its prior variance (committed by a marker whose
  // correction was skipped, so never corrected) cancels 1e7 − (1e7 − δ) like a first sighting:
  // the chunk's block is patched for it too (uniform: every workgroup reads the same block)
  if (sizeof(T) == 4 && (sj.kk[0] >= 0.5 * prior || sj.kk[3] >= 0.5 * prior)) ch.any_new = true;
  double zhat[2], braw, H0[5], H1[5];
  bool bok;
  range_bearing(pose, sj.x[0], sj.x[1], zhat, H0, H1, &braw, &bok);
  if (!bok) zhat[1] = normalize_angle(braw);
  st.H = HRows{H0[1], H0[2], H1[1], H1[2]};
  double P5[5][5];
  block5(Pp, sj, P5);
  double Gt[5][2];  // (Σ·Hᵀ)[pA]
#pragma unroll
  for (int a = 0; a < 5; ++a)
    times_H(st.H, P5[a][0], P5[a][1] - P5[a][3], P5[a][2] - P5[a][4], Gt[a][0], Gt[a][1]);
  double Sm[4];  // S = H·(Σ·Hᵀ)[pA] + R (slam.cpp:476)
  times_H(st.H, Gt[0][0], Gt[1][0] - Gt[3][0], Gt[2][0] - Gt[4][0], Sm[0], Sm[2]);
  times_H(st.H, Gt[0][1], Gt[1][1] - Gt[3][1], Gt[2][1] - Gt[4][1], Sm[1], Sm[3]);
  Sm[0] = Sm[0] + r_noise;
  Sm[3] = Sm[3] + r_noise;
  st.ok = inv2(Sm, st.Si);
  if (!st.ok) {
    ch.status |= EKF_FLAG_NUMERIC_D;
    return;
  }
  st.nu0 = z0 - zhat[0];
  st.nu1 = normalize_angle(z1 - zhat[1]);
#pragma unroll
  for (int a = 0; a < 3; ++a)
    gain_row<J, false>(Gt[a][0], Gt[a][1], st.Si, Sm, st.Kp[a], st.Vp[a]);
  if (J)
#pragma unroll
    for (int t = 0; t < 4; ++t) st.Sv[t] = Sm[t];
#pragma unroll
  for (int b = 0; b < 3; ++b)  // (H·Σ)[:, pose b]
    times_H(st.H, P5[0][b], P5[1][b] - P5[3][b], P5[2][b] - P5[4][b], st.Mp[0][b], st.Mp[1][b]);
}

// This lane's slot at step c: its crosses with j, Σ_c[k, j] = Σ_p[k, j] − Σ_cc K_cc[k]·M_cc[:, j]
// and Σ_c[j, k] likewise (the sums from waves 1-2, sh.es), then K[k], M[:, k] (, V[k]) from them
// and Σ ← Σ − K·M (Joseph: − V·Kᵀ) on the lane's block, x += K·ν (slam.cpp:482-488).
template <typename T, bool J>
__device__ __forceinline__ void slot_step(const AmSharedT<J>& sh, const AmFilter<T>& F,
                                          const AmStep& st, double (&rkj)[4], double (&rjk)[4],
                                          Slot& sl, LaneKM& km) {
  const int lane = F.lane;
  if (F.k == st.j) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      rkj[t] = sl.kk[t];
      rjk[t] = sl.kk[t];
    }
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      rkj[t] = rkj[t] - (sh.es[0][t][lane] + sh.es[1][t][lane]);
      rjk[t] = rjk[t] - (sh.es[0][4 + t][lane] + sh.es[1][4 + t][lane]);
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {  // (Σ·Hᵀ)[k_a] over pA
    double q0, q1;
    times_H(st.H, sl.kp[3 * a], sl.kp[3 * a + 1] - rkj[2 * a], sl.kp[3 * a + 2] - rkj[2 * a + 1],
            q0, q1);
    gain_row<J, true>(q0, q1, st.Si, st.Sv, km.K[a], km.V[a]);
  }
#pragma unroll
  for (int b = 0; b < 2; ++b)  // (H·Σ)[:, k_b]
    times_H(st.H, sl.pk[b], sl.pk[2 + b] - rjk[b], sl.pk[4 + b] - rjk[2 + b], km.M[0][b],
            km.M[1][b]);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
      sl.kk[2 * a + b] =
          km_vk_sub<J>(sl.kk[2 * a + b], km.K[a], km.M[0][b], km.M[1][b], km.V[a], km.K[b]);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      sl.kp[3 * a + b] =
          km_vk_sub<J>(sl.kp[3 * a + b], km.K[a], st.Mp[0][b], st.Mp[1][b], km.V[a], st.Kp[b]);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
      sl.pk[2 * a + b] =
          km_vk_sub<J>(sl.pk[2 * a + b], st.Kp[a], km.M[0][b], km.M[1][b], st.Vp[a], km.K[b]);
  sl.x[0] = sl.x[0] + (km.K[0][0] * st.nu0 + km.K[0][1] * st.nu1);
  sl.x[1] = sl.x[1] + (km.K[1][0] * st.nu0 + km.K[1][1] * st.nu1);
}

// The step on the pose block and the pose (every lane, the same values)
template <bool J>
__device__ __forceinline__ void pose_update(const AmStep& st, double (&Pp)[3][3],
                                            double (&pose)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
      Pp[a][b] = km_vk_sub<J>(Pp[a][b], st.Kp[a], st.Mp[0][b], st.Mp[1][b], st.Vp[a], st.Kp[b]);
    pose[a] = pose[a] + (st.Kp[a][0] * st.nu0 + st.Kp[a][1] * st.nu1);
  }
  pose[0] = normalize_angle(pose[0]);  // slam.cpp:488
}

// Column i < 3's of three values (by value: a select between members keeps the struct in memory)
__device__ __forceinline__ double pick3(int i, double a, double b, double c) {
  return i == 0 ? a : (i == 1 ? b : c);
}
// Step c's factor e at the NC state columns from col: Kcat / Mcat row 2 + 2c + e holds K / M;
// Joseph: row 2 + 2m + 2c + e holds V / K, the V·Kᵀ term's factors. (A row's stores to one array
// stay together: Kcat and Mcat may alias for the compiler, so it pairs only adjacent ones.)
template <typename T, bool J, int NC>
__device__ __forceinline__ void put_factor(const AmFilter<T>& F, int c, int m, int e, int col,
                                           const double (&kv)[NC], const double (&mv)[NC],
                                           const double (&vv)[NC]) {
  T* kr = F.kc + (2 + 2 * c + e) * F.ldk + col;
  T* mr = F.mc + (2 + 2 * c + e) * F.ldk + col;
#pragma unroll
  for (int i = 0; i < NC; ++i) kr[i] = static_cast<T>(kv[i]);
#pragma unroll
  for (int i = 0; i < NC; ++i) mr[i] = static_cast<T>(mv[i]);
  if (J) {
#pragma unroll
    for (int i = 0; i < NC; ++i) kr[2 * m * F.ldk + i] = static_cast<T>(vv[i]);
#pragma unroll
    for (int i = 0; i < NC; ++i) mr[2 * m * F.ldk + i] = static_cast<T>(kv[i]);
  }
}
// The step's factors: the lane's history row (LDS and, for later steps' landmarks in other
// workgroups, the write-through table) and the Kcat / Mcat rows at the slot's two columns and, by
// workgroup 0, the pose's three. A skipped step writes zeros.
template <typename T, bool J>
__device__ __forceinline__ void write_step_factors(AmSharedT<J>& sh, const AmFilter<T>& F, int c,
                                                   int m, const LaneKM& km, const AmStep& st) {
  constexpr int HW = AmSharedT<J>::HW;
  const int lane = F.lane;
  const double hrow[12] = {km.K[0][0], km.K[0][1], km.K[1][0], km.K[1][1], km.M[0][0], km.M[0][1],
                           km.M[1][0], km.M[1][1], km.V[0][0], km.V[0][1], km.V[1][0], km.V[1][1]};
  double2* hl = reinterpret_cast<double2*>(sh.hkm[c][lane]);
#pragma unroll
  for (int t = 0; t < HW / 2; ++t) hl[t] = make_double2(hrow[2 * t], hrow[2 * t + 1]);
  if (F.valid) {
#pragma unroll
    for (int e = 0; e < 2; ++e)
      put_factor<T, J, 2>(F, c, m, e, F.ix, {km.K[0][e], km.K[1][e]}, {km.M[e][0], km.M[e][1]},
                          {km.V[0][e], km.V[1][e]});
    if (F.G > 1 && c + 1 < m)
      put_hist(F.hist + static_cast<size_t>(c) * F.Np + F.g * kAmSlots, lane, hrow, HW, F.loc);
  }
  if (F.g == 0 && lane < 3) {
#pragma unroll
    for (int e = 0; e < 2; ++e)
      put_factor<T, J, 1>(F, c, m, e, lane, {pick3(lane, st.Kp[0][e], st.Kp[1][e], st.Kp[2][e])},
                          {pick3(lane, st.Mp[e][0], st.Mp[e][1], st.Mp[e][2])},
                          {pick3(lane, st.Vp[0][e], st.Vp[1][e], st.Vp[2][e])});
  }
}

// Kcat / Mcat rows 0, 1 (the predict's two rank-1 terms) and the zero rows rank..kw at one column
template <typename T>
__device__ __forceinline__ void put_predict_column(const AmFilter<T>& F, int col, double k0,
                                                   double k1, double m0, double m1, int rank,
                                                   int kw) {
  F.kc[0 * F.ldk + col] = static_cast<T>(k0);
  F.kc[1 * F.ldk + col] = static_cast<T>(k1);
  F.mc[0 * F.ldk + col] = static_cast<T>(m0);
  F.mc[1 * F.ldk + col] = static_cast<T>(m1);
  for (int rr = rank; rr < kw; ++rr) {
    F.kc[rr * F.ldk + col] = static_cast<T>(0.0);
    F.mc[rr * F.ldk + col] = static_cast<T>(0.0);
  }
}
// The chunk's remaining factor rows: the predict's two rank-1 terms (slam.cpp:198, as k_factors
// writes them: K rows −α_i and −(Σ[i][0] + α_i·Σ[0][0]), M rows Σ[0][j] and α_j; α = 0 at landmark
// columns), zero rows up to the pass's rank kw — and the new state.
template <typename T, bool J>
__device__ __forceinline__ void write_predict_factors(const AmFilter<T>& F, int m, bool first,
                                                      double a1, double a2, const Slot& sl,
                                                      const double* pose) {
  const T* S = F.S;
  const int ix = F.ix, ld = F.ld, lane = F.lane;
  const int rank = 2 + (J ? 4 : 2) * m, kw = pass_kw(J, m);
  if (F.valid) {
    // Σ_in[ix + e][0] and Σ_in[0][ix + e] (raw, as slot_block read them)
    const double c0[2] = {static_cast<double>(S[static_cast<size_t>(ix) * ld]),
                          static_cast<double>(S[static_cast<size_t>(ix + 1) * ld])};
    const double r0[2] = {static_cast<double>(S[ix]), static_cast<double>(S[ix + 1])};
#pragma unroll
    for (int e = 0; e < 2; ++e)
      put_predict_column(F, ix + e, 0.0, first ? -c0[e] : 0.0, first ? r0[e] : 0.0, 0.0, rank, kw);
    F.xout[ix] = sl.x[0];
    F.xout[ix + 1] = sl.x[1];
  }
  if (F.g == 0 && lane < 3) {
    const double al = alpha_of(lane, a1, a2);
    const double rc0 = static_cast<double>(S[lane * ld]), r0c = static_cast<double>(S[lane]);
    const double s00 = static_cast<double>(S[0]);
    put_predict_column(F, lane, first ? -al : 0.0, first ? -(rc0 + al * s00) : 0.0,
                       first ? r0c : 0.0, first ? al : 0.0, rank, kw);
    F.xout[lane] = pose[lane];
  }
}

// The filter's counter, its posterior t_map_odom after a message's last chunk, and the flags.
// (flags: the descriptor's, read at the kernel's start; read again here, behind the factor rows'
// stores, the load would wait for all of them.)
template <typename T>
__device__ __forceinline__ void finish_filter(const AmFilter<T>& F, const MsgDesc& d, int flags,
                                              const double* pose, const AmChunk& ch,
                                              const PassArgs<T>& A, int f) {
  unsigned* const fatal = A.fatal;
  if (F.g == 0 && F.lane == 0) {
    F.ctl->counter = ch.s;
    if (flags & kLast) {  // posterior t_map_odom = T(x, y, θ)·t_odom_robot⁻¹ (slam.cpp:490-494)
      const Pose2 tmo = compose(Pose2{pose[0], pose[1], pose[2]},
                                inverse(Pose2{d.odom[0], d.odom[1], d.odom[2]}));
      F.ctl->tmo[0] = tmo.theta;
      F.ctl->tmo[1] = tmo.x;
      F.ctl->tmo[2] = tmo.y;
      // the pose trace's record: of a filter's ⌈N/64⌉ workgroups this one alone appends (the
      // count's earlier writers ended before this kernel read t_map_odom, at its start)
      if (A.trace)
        A.trace_n[f] = trace_append(A, f, A.trace_n[f], pose[0], pose[1], pose[2], tmo.theta,
                                    tmo.x, tmo.y);
    }
  }
  if (F.lane == 0 && F.g == 0 && ch.status) atomicOr(&F.ctl->status, ch.status);
  if (F.lane == 0 && ch.timeout) flag_timeout(&F.ctl->status, fatal);
}

// fp32 Σ: the final Σ[U, U] in fp64 over the pass's block when a landmark was committed
// (the Σ pass's fp32 tiles take it; its first sighting cancels 1e7 − (1e7 − δ) in fp32); otherwise
// the record's flag is cleared. G > 1: the final blocks (cur[m]) and every history row are
// published, then, after a last exchange, workgroup 0 alone builds the block.
template <typename T, bool J>
__device__ __forceinline__ void write_pend_patch(AmSharedT<J>& sh, const AmFilter<T>& F,
                                                 ChunkRec* rec, int m, unsigned tag, unsigned spin,
                                                 unsigned* fatal, bool any_new, const Slot& sl,
                                                 const double (&Pp)[3][3]) {
  constexpr int HW = AmSharedT<J>::HW;
  const int G = F.G, g = F.g, lane = F.lane, Np = F.Np;
  if (!any_new) {
    if (g == 0 && lane == 0) rec->flags = 0;
    return;
  }
  if (G > 1) {
    if (F.valid) {
      put_hist(F.hist + static_cast<size_t>(m - 1) * Np + g * kAmSlots, lane, sh.hkm[m - 1][lane],
               HW, F.loc);
      put_cur(F.cur + static_cast<size_t>(m) * Np + g * kAmSlots, lane, sl, F.loc);
    }
    double dd = 0.0;
    int kd = 0;
    bool late = false;
    exchange(F.gran, G, g, m, tag, dd, kd, &late, F.loc, spin);
    if (late && lane == 0) flag_timeout(&F.ctl->status, fatal);
    if (g != 0) return;
  }
  // workgroup 0: U = {θ, x, y, jx, jy per marker} (a skipped marker maps onto θ: never a first
  // position, never patched); every marker's landmark's final block (pb) and, with G > 1, its
  // factor history staged into the no longer needed own-history LDS (ph[c][cc][8])
  wave_lds_publish();
  const int nu = 3 + 2 * m;
  double* ph = &sh.hkm[0][0][0];  // G > 1: [m][m][HW] ≤ 3 072 doubles (the region holds 64·HW·16)
  if (G > 1) {
    for (int e = lane; e < m * kSlotW; e += 64) {
      const int c = e / kSlotW, t = e - c * kSlotW;
      sh.pb[c][t] = ld_xf64(
          F.cur_r, static_cast<unsigned>((m * Np + max(sh.jl[c], 0)) * sizeof(AmCur) + 8 * t));
    }
    for (int e = lane; e < m * m * HW; e += 64) {
      const int c = e / (HW * m), cc = (e / HW) % m, t = e % HW;
      const double v = ld_xf64(
          F.hist_r, static_cast<unsigned>((cc * Np + max(sh.jl[c], 0)) * sizeof(AmHist) + 8 * t));
      __builtin_amdgcn_wave_barrier();  // every lane's loads issued before any lane overwrites
      ph[e] = v;
    }
  } else {
    for (int c = 0; c < m; ++c)
      readlane_slot(sl, __builtin_amdgcn_readfirstlane(max(sh.jl[c], 0)), lane, sh.pb[c]);
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) sh.pp[3 * a + b] = Pp[a][b];
  }
  wave_lds_publish();
  // the history of marker position c's landmark at step cc: K (t < 4), M (t < 8), V (t < 12)
  auto hv = [&](int c, int cc, int t) -> double {
    if (G > 1) return ph[(c * m + cc) * HW + t];
    const int j = max(sh.jl[c], 0);
    return sh.hkm[cc][j][t];
  };
  for (int e = lane; e < nu * nu; e += 64) {
    const int a = e / nu, b = e - a * nu;
    const int ca = a < 3 ? -1 : (a - 3) >> 1, ea = (a - 3) & 1;
    const int cb = b < 3 ? -1 : (b - 3) >> 1, eb = (b - 3) & 1;
    const bool sa = ca >= 0 && sh.jl[ca] < 0, sb = cb >= 0 && sh.jl[cb] < 0;
    double v;
    if (sa || sb) {
      v = 0.0;  // a skipped marker's position (its column maps onto θ and is never patched)
    } else if (ca < 0 && cb < 0) {
      v = sh.pp[3 * a + b];
    } else if (ca < 0) {  // Σ[pose a][landmark]
      v = sh.pb[cb][kSlotPk + 2 * a + eb];
    } else if (cb < 0) {  // Σ[landmark][pose b]
      v = sh.pb[ca][kSlotKp + 3 * ea + b];
    } else if (sh.jl[ca] == sh.jl[cb]) {
      v = sh.pb[ca][2 * ea + eb];  // (Slot::kk)
    } else {  // two landmarks: Σ_in minus the chunk's rank-2 terms, as the lanes' crosses
      const int ja = 3 + 2 * sh.jl[ca] + ea, jb = 3 + 2 * sh.jl[cb] + eb;
      v = static_cast<double>(F.S[static_cast<size_t>(ja) * F.ld + jb]);
      for (int cc = 0; cc < m; ++cc) {
        v = rank2_sub(v, hv(ca, cc, 2 * ea), hv(ca, cc, 2 * ea + 1), hv(cb, cc, 4 + eb),
                      hv(cb, cc, 4 + 2 + eb));
        if (J)  // − V_cc[a]·K_cc[b]ᵀ
          v = rank2_sub(v, hv(ca, cc, 8 + 2 * ea), hv(ca, cc, 8 + 2 * ea + 1), hv(cb, cc, 2 * eb),
                        hv(cb, cc, 2 * eb + 1));
      }
    }
    rec->Pend[a][b] = v;
  }
  for (int a = lane; a < kMaxU + 1; a += 64) {
    int u = 0;
    if (a < 3) {
      u = a;
    } else if (a < nu) {
      const int jj = sh.jl[(a - 3) >> 1];
      u = jj < 0 ? 0 : 3 + 2 * jj + ((a - 3) & 1);
    }
    rec->u[a] = u;
  }
  if (lane == 0) {
    rec->nu = nu;
    rec->m = m;
    rec->flags = kPendValid;
  }
}

}  // namespace

template <typename T, bool J>
__global__ __launch_bounds__(kAmThreads) void k_assoc_msg(PassArgs<T> A, AmArgs B) {
  __shared__ AmSharedT<J> sh;
  const int G = B.G, fy = blockIdx.y;
  // XCD-local placement (B.xcd): the grid has 8 blocks per workgroup; filter fy's workgroups are
  // the blocks x ≡ fy (mod 8), which round-robin dispatch puts on one XCD (checked: same_xcd)
  int g = blockIdx.x;
  if (B.xcd) {
    if ((g & 7) != (fy & 7)) return;
    g >>= 3;
  }
  const MsgDesc& d = A.desc[fy];
  const int flags = d.flags;
  if (!(flags & kActive)) return;  // (every workgroup of the filter)
  const int lane = threadIdx.x & (kAmSlots - 1), m = d.m;
  if (threadIdx.x >= kAmSlots) {  // waves 1, 2: the history sums only (uniform per wave)
    history_helper(sh, m, g * kAmSlots + lane, lane, (threadIdx.x >> 6) - 1);
    return;
  }
  // ---- setup: the filter's buffers, this launch's tags and transport ----
  AmFilter<T> F = filter_view(A, B, d, A.f0 + fy, g, lane);
  const double r_noise = A.r, gate = A.gate;
  const unsigned tagbase = (A.seq & 0x07ffffffu) << 5;
  AmChunk ch = {0u, 0u, false, false};
  F.loc = B.xcd && G > 1 && same_xcd(F.gran, G, g, tagbase | 31u, &ch.timeout, B.spin);

  // ---- predict (slam.cpp:321-335): the pose, At's two entries, the pose block (every lane), the
  // lane's slot: its predicted block and state ----
  double pose[3], a1, a2, Pp[3][3];
  predicted_pose(F.ctl->tmo, d, F.xin, pose, &a1, &a2);
  const bool first = (flags & kFirst) != 0;
  predict_pose_block(F.S, F.ld, a1, a2, first, A.q, Pp);
  Slot sl;
  slot_block(F.S, F.ld, F.ix, a1, a2, sl);
  sl.x[0] = F.xin[F.ix];
  sl.x[1] = F.xin[F.ix + 1];
  ch.s = F.ctl->counter;
  // the state at the chunk's start, for the first step's exchange
  if (F.valid && G > 1) put_cur(F.cur + g * kAmSlots, lane, sl, F.loc);

  AM_STAMP(kMaxChunk, 0);
  for (int c = 0; c < m; ++c) {
    AM_STAMP(c, 0);
    const double z0 = d.z[c][0], z1 = d.z[c][1];
    // a full map: the reference's temporary landmark (slam.cpp:351-356) indexes the state out of
    // range and throws before any association; the marker is skipped (uniform: no exchange)
    const bool full = ch.s >= static_cast<unsigned>(A.N);
    double key = INFINITY;
    if (!full && F.valid && F.k < static_cast<int>(ch.s))
      key = score_slot(Pp, sl, pose, z0, z1, r_noise);
    int kbest = F.valid ? F.k : INT_MAX;
    wave_argmin(key, kbest);
    AM_STAMP(c, 1);
    filter_argmin(F, c, tagbase | static_cast<unsigned>(c + 1), full, B.spin,
                  B.drop && c == 0 && g == G - 1, key, kbest, &ch.timeout);
    AM_STAMP(c, 2);
    AmStep st = {};
    decide(sh, F, d, c, full, key, kbest, gate, ch, st);
    double rkj[4] = {0.0, 0.0, 0.0, 0.0}, rjk[4] = {0.0, 0.0, 0.0, 0.0};
    if (st.j >= 0) fetch_landmark(sh, F, c, pose, z0, z1, st, sl, rkj, rjk);
    // wave 0 forms what every lane shares while waves 1-2 (history_helper) sum this step's history
    // terms of every lane's crosses with j, between barriers A and B (all three waves pass both at
    // every step)
    lds_barrier();  // A: sh.jl[c], sh.jc and j's history sh.jh published to waves 1-2
    AM_STAMP(c, 3);
    if (st.j >= 0) pose_step<T, J>(sh, Pp, pose, z0, z1, r_noise, B.prior, ch, st);
    lds_barrier();  // B: waves 1 / 2's sums in sh.es
    AM_STAMP(c, 5);
    LaneKM km = {};
    if (st.ok) {
      slot_step(sh, F, st, rkj, rjk, sl, km);
      pose_update<J>(st, Pp, pose);
    }
    AM_STAMP(c, 4);
    write_step_factors(sh, F, c, m, km, st);
    if (F.valid && G > 1 && c + 1 < m)  // the slot's block and state as step c + 1 starts
      put_cur(F.cur + static_cast<size_t>(c + 1) * F.Np + g * kAmSlots, lane, sl, F.loc);
  }

  AM_STAMP(kMaxChunk, 1);
  write_predict_factors<T, J>(F, m, first, a1, a2, sl, pose);
  finish_filter(F, d, flags, pose, ch, A, A.f0 + fy);
  if (sizeof(T) == 4)
    write_pend_patch(sh, F, A.rec + static_cast<size_t>(d.parity) * A.rec_stride + (A.f0 + fy), m,
                     tagbase | static_cast<unsigned>(m + 1), B.spin, A.fatal, ch.any_new, sl, Pp);
}

#ifdef EKF_DIAG_STAMPS
}  // namespace ekfslam
extern "C" int ekfslam_diag_read_am_stamps(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(ekfslam::g_am_stamps), sizeof(ekfslam::g_am_stamps)) ==
                 hipSuccess ? 0 : -5;
}
namespace ekfslam {
#endif

template <typename T>
hipError_t launch_assoc_msg(const PassArgs<T>& a, const AmArgs& b, int nf, hipStream_t s,
                            hipEvent_t e0, hipEvent_t e1) {
  const dim3 grid(b.xcd ? 8 * b.G : b.G, nf);
  launch(a.joseph ? k_assoc_msg<T, true> : k_assoc_msg<T, false>, grid, dim3(kAmThreads), s, e0, e1,
         a, b);
  return hipGetLastError();
}

int assoc_msg_blocks_per_cu(bool f32, bool joseph) {
  int nb = 0;
  auto occ = [&](auto kern) { return hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, kAmThreads, 0); };
  const hipError_t e = f32 ? (joseph ? occ(k_assoc_msg<float, true>) : occ(k_assoc_msg<float, false>))
                           : (joseph ? occ(k_assoc_msg<double, true>) : occ(k_assoc_msg<double, false>));
  return e == hipSuccess ? nb : 0;
}

template hipError_t launch_assoc_msg<double>(const PassArgs<double>&, const AmArgs&, int,
                                             hipStream_t, hipEvent_t, hipEvent_t);
template hipError_t launch_assoc_msg<float>(const PassArgs<float>&, const AmArgs&, int, hipStream_t,
                                            hipEvent_t, hipEvent_t);

// ---- association of one marker per launch (k_assoc) -------------------------------------------
// slam.cpp:344-440 for the marker in desc.z[0]: d_k = νᵀψ_k⁻¹ν over the known landmarks k < counter
// (predict folded in when pending), the new slot's d forced to the gate (:406-408), first-index
// argmin (arma::index_min), then commit (new landmark written into x_in, counter++) or roll back.
constexpr int kAssocThreads = 1024;  // one known landmark per lane up to counter 1024: the gathers
                                     // of every landmark in flight in one round
template <typename T>
__global__ __launch_bounds__(kAssocThreads) void k_assoc(PassArgs<T> A) {
  __shared__ double s_pose[3], s_a[2], s_P33[3][3];
  __shared__ double s_bd[kAssocThreads / 64];
  __shared__ int s_bk[kAssocThreads / 64];
  __shared__ int s_abort;
  const MsgDesc& d = A.desc[blockIdx.y];
  if (!(d.flags & kActive) || d.m == 0) return;
  const int f = A.f0 + blockIdx.y;
  const int tid = threadIdx.x;
  const int ld = A.ld;
  const T* S = A.sig[d.parity] + f * A.sig_stride;
  double* x = A.x[d.parity] + f * A.x_stride;
  FilterCtl* ctl = A.ctl + f;
  // device epochs: Σ_in and x are the last Σ pass's (bulk stream), its epoch A.need_sigma
  if (A.polls && A.need_sigma) {
    if (tid == 0 && !epoch_wait_acquire(A.sync + kSyncSigma, A.need_sigma))
      flag_timeout(&ctl->status, A.fatal);
    __syncthreads();
  }
  const unsigned s = ctl->counter;
  const int slot = d.assoc_slot;
  if (tid == 0) {
    double a1, a2;
    predicted_pose(ctl->tmo, d, x, s_pose, &a1, &a2);
    s_a[0] = a1;
    s_a[1] = a2;
    predict_pose_block(S, ld, a1, a2, (d.flags & kFirst) != 0, A.q, s_P33);
    s_abort = 0;
    if (s >= static_cast<unsigned>(A.N)) {  // the reference indexes state(3+2·counter) out of range
      s_abort = 1;
      atomicOr(&ctl->status, EKF_FLAG_RANGE_D);
      ctl->assoc_j[slot] = -1;
      ctl->assoc_new[slot] = 0;
    }
  }
  __syncthreads();
  if (s_abort) return;
  const double z0 = d.z[0][0], z1 = d.z[0][1];
  const double a1 = s_a[0], a2 = s_a[1];  // (0 without kFirst: predicted_pose)
  double bestd = INFINITY;
  int bestk = INT_MAX;
  for (unsigned k = tid; k < s; k += blockDim.x) {
    const int j = 3 + 2 * static_cast<int>(k);
    Slot sl;
    slot_block(S, ld, j, a1, a2, sl);
    double P[5][5];
    block5(s_P33, sl, P);
    const double dist = assoc_dist(P, s_pose, x[j], x[j + 1], z0, z1, A.r);
    if (dist < bestd) {  // strict: first index kept, NaN never selected
      bestd = dist;
      bestk = static_cast<int>(k);
    }
  }
  wave_argmin(bestd, bestk);  // 64 lanes, ties → lower index (DPP, ekf_math.hpp)
  const int wv = tid >> 6;
  if ((tid & 63) == 0) {
    s_bd[wv] = bestd;
    s_bk[wv] = bestk;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < static_cast<int>(blockDim.x >> 6); ++w)
      if (s_bd[w] < bestd || (s_bd[w] == bestd && s_bk[w] < bestk)) {
        bestd = s_bd[w];
        bestk = s_bk[w];
      }
    // the new slot (index s, d = gate) wins only over a strictly larger existing minimum
    if (!(bestd <= A.gate)) {
      const int js = 3 + 2 * static_cast<int>(s);
      x[js] = s_pose[1] + z0 * cos(z1 + s_pose[0]);      // slam.cpp:351-354
      x[js + 1] = s_pose[2] + z0 * sin(z1 + s_pose[0]);
      ctl->counter = s + 1;
      ctl->assoc_j[slot] = static_cast<int>(s);
      ctl->assoc_new[slot] = 1;
    } else {
      ctl->assoc_j[slot] = bestk;
      ctl->assoc_new[slot] = 0;
    }
  }
}

template <typename T>
hipError_t launch_assoc(const PassArgs<T>& a, int nf, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  launch(k_assoc<T>, dim3(1, nf), dim3(kAssocThreads), s, e0, e1, a);
  return hipGetLastError();
}
template hipError_t launch_assoc<double>(const PassArgs<double>&, int, hipStream_t, hipEvent_t,
                                         hipEvent_t);
template hipError_t launch_assoc<float>(const PassArgs<float>&, int, hipStream_t, hipEvent_t,
                                        hipEvent_t);

}  // namespace ekfslam
