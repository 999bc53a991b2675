// k_chain (gfx950 / CDNA4): the sequential part of the EKF-SLAM predict → correct* → posterior path
// of maxipalay/ekf-slam nuslam/src/slam.cpp.
//
// A chunk (one message, up to kMaxChunk markers) runs as three kernels:
//
//   k_chain       (this file) One workgroup per filter. The m corrections of a chunk only couple
//                 through the rows/columns the chunk touches, U = {θ, x, y} ∪ {jx, jy per marker}
//                 (|U| ≤ 3+2m). The chain replays them on the |U|×|U| block in LDS (predict folded
//                 in) — the only sequential part — and hands the factor kernel the row / column
//                 maps Z (|U|×2m) and Y (2m×|U|) plus x[U] through a write-through record (ChunkRec).
//   k_factors     (ekf_factors.hip) Kcat = Σ_pred[:, U]·Z and Mcat = Y·Σ_pred[U, :] for every row /
//                 column on f64 MFMA (v_mfma_f64_16x16x4f64), plus the new state x.
//   k_sigma_pass  (ekf_sigma_pass.hip) Σ_out = Σ_in + Q̄ − Σ_k Kcat[k]ᵀ ⊗ Mcat[k], a rank-(2+2m)
//                 update of the dense covariance: the predict's two rank-1 terms (A Σ Aᵀ,
//                 slam.cpp:198) and one rank-2 term per correction ((I − KH)Σ, slam.cpp:264-265). It
//                 streams Σ once per chunk through MFMA (v_mfma_f32_32x32x2f32 for fp32 Σ,
//                 v_mfma_f64_16x16x4f64 for fp64), so the HBM cost of a correction is 2·n²·w / m
//                 instead of 2·n²·w.
//
// Equal to the reference's sequential dense algebra in exact arithmetic; the summation order
// differs (tolerances in tests/). Unknown association adds k_assoc (ekf_assoc.hip) before each
// single-marker chunk.
//
// k_chain is the chunk loop; a chunk's phases, in execution order (every one __forceinline__ into
// the kernel's one register allocation, except wave 0's two programs):
//   issue_early_loads         kLook, staged: the image and the previous record → ChainLoads
//   build_index_sets          A0: U and U'
//   rebuild_block             A1, kLook: land_rebuild_operands (staged image, or its own gather and
//                             store_raw_image), predict_prev (wave 3: map_U_into_prev),
//                             rebuild_km_simple / _joseph (K', M'; simple form, wave 3: x_in[U]),
//                             rebuild_p_simple / _joseph (Joseph form, wave 3: x_in[U]),
//                             pick_predicted_pose
//   gather_block              A1 otherwise: Σ_in[U, U], x[U] and the predicted pose from HBM
//   fold_predict              A3: this chunk's predict on the block
//   chain_wave0 (_lean) .. 3  A2: the corrections; Z (wave 1), Y (wave 2), the rest of the block,
//                             the posterior t_map_odom and the next predicted pose (wave 3)
//   write_pend_patch          fp32: the final Σ[U, U] in fp64 for the Σ pass's tiles
//   write_record              ChunkRec, write-through
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ekf_device.hpp"
#include "ekf_launch.hpp"
#include "ekf_math.hpp"
#include "geom.hpp"

namespace ekfslam {

#include "ekf_diag.hpp"  // (EKF_STAMP*, EKF_DUMP_BLOCK; empty in the product library)
#ifdef EKF_DIAG_STAMPS
__device__ unsigned long long g_stamps[4 * 512];
__device__ double g_blocks[64][kMaxU][kMaxU + 1];
__device__ double g_blockx[64][kMaxU];
}  // namespace ekfslam
extern "C" int ekfslam_diag_read_stamps(unsigned long long* out, int n) {
  using ekfslam::g_stamps;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * (n < 2048 ? n : 2048)) == hipSuccess ? 0 : -5;
}
extern "C" int ekfslam_diag_read_blocks(double* blocks, double* xs) {
  using namespace ekfslam;
  if (hipMemcpyFromSymbol(blocks, HIP_SYMBOL(g_blocks), sizeof(g_blocks)) != hipSuccess) return -5;
  return hipMemcpyFromSymbol(xs, HIP_SYMBOL(g_blockx), sizeof(g_blockx)) == hipSuccess ? 0 : -5;
}
namespace ekfslam {
#endif

#include "ekf_sync.hpp"  // (hand-off protocol, lds_barrier and buffer-descriptor helpers)

// J: the Joseph-form instantiation (round 6: a whole message of ≤ 16 markers per chunk): its row
// maps Z hold Zv beside Z (4m ≤ 64 columns) and V, S, C', D' are kept per step; the simple form's
// instantiation keeps the round-5 layout (ZC = 32 columns, one unused slot for the Joseph arrays).
template <bool J>
struct ChainSharedT {
  static constexpr int ZC = J ? kZJ : kZC;     // Z columns (the chain's and the rebuilt pv.Z / pv.K)
  static constexpr int JM = J ? kMaxJoseph : 1;  // Joseph steps kept
  int u[kMaxU];
  int skip[kMaxChunk];
  double alphaU[kMaxU];
  double row0raw[kMaxU];  // Σ_in[0][u_b]
  double col0raw[kMaxU];  // Σ_in[u_a][0]
  double xU[1][kMaxU];    // x[U], owned by wave 0 during the corrections
  // im.D = Σ[U,U], the chain's block (rows all, columns live). kLook: im.R = Σ_pred'[U][U'] and
  // im.C = Σ_pred'[U'][U] (U' = the previous chunk's index set; k over U' padded to 36 with zeros,
  // so MFMA operand reads need no predicate). One struct with StageRec's payload: a staged image
  // lands here piece by piece.
  RebuildImage<double> im;
  double Cz[kMaxChunk][4];  // wave 1, step c: C_k = M_k[:, pA_c]·Hᵀ·S⁻¹ (2×2) for k < c
  double Dy[kMaxChunk][4];  // wave 2, step c: D_k = H·K_k[pA_c] (2×2) for k < c
  double KU[kMaxChunk][kMaxU][2];
  double MU[kMaxChunk][kMaxU][2];
  double Z[kMaxU][ZC + 1];       // K_c[i] = r_0(i)[U] · Z[:, 2c..2c+1] (Joseph: Zv in 32 + 2c..)
  double Y[kZC][kMaxU + 1];      // M_c[:, j] = Y[2c..2c+1, :] · c_0(j)[U]
  double Zx[kMaxU];              // Σ_c Z_c ν_c: x_i += r_0(i)[U] · Zx
  double nu[kMaxChunk][2];
  double Hs[kMaxChunk][2][5];    // H_c over pA (published for waves 1–2)
  double Sis[kMaxChunk][4];      // S_c⁻¹
  // Joseph chunks (m ≤ kMaxJoseph): V_c = (Σ_c·Hᵀ − K_c·S_c)[U] and S_c per step (wave 0), wave 1's
  // C'_k = K_k[pA_c]ᵀ·Hᵀ and wave 2's D'_k = H·V_k[pA_c]
  double VU[JM][kMaxU][2];
  double Ss[JM][4];
  double Cv[JM][4];
  double Dv[JM][4];
  // kLook: the previous chunk's record and the blocks rebuilt from it
  struct {
    int u[kMaxU];
    int pos[kMaxU];  // where this chunk's u_a sits in U' (map_U_into_prev)
    int nu, m, first, joseph;
    double a1, a2, s00;
    double xU[kMaxU], Zx[kMaxU];
    // k (over U') padded to kMaxU + 1 = 36 with zeros, so MFMA operand reads need no predicate
    double Z[kMaxU + 1][ZC + 1];
    double Y[kZC][kMaxU + 1];
    double K[kMaxU][ZC + 1];      // R·Z'  = the previous K_c at U (Joseph: and V_c at U)
    double M[kZC][kMaxU + 1];     // Y'·C  = the previous M_c at U
    double r0U[kMaxU], c0U[kMaxU], r0P[kMaxU], c0P[kMaxU];
    double xg[kMaxU];             // x_in'[u] for this chunk's U (rows the previous chunk missed)
  } pv;
  double junk[4][64];             // per-wave sink of masked-off LDS stores (no divergent branch)
  double junk2[64][2];
  double pose[3];
  double xpose[3];  // x_in pose (posterior of the previous chunk)
  double npose[3], na1, na2;  // the next chunk's predicted pose and At entries (wave 3, ahead)
  int npose_ci;               // the chunk index they belong to (−1: none)
  double tmo[3];    // t_map_odom
  long long trace_n;  // pose trace: the filter's record count, carried over the launch's chunks
                      // (−1: not loaded yet; wave 3's lane 0 alone reads and writes it)
  double a1, a2, s00;
  int nu_cnt;
  unsigned status;
  int pub;    // steps whose K, M, H, S⁻¹ wave 0 has published
  int pdone;  // steps wave 3 has applied outside the cross
  int any_init;  // a correction of this chunk initialised its landmark (slam.cpp:213-216)
  int zdone;     // Joseph: steps whose Z_c, Zv_c wave 1 has stored (wave 2 reads them)
  // steps wave 0 has run in its lean and in its generic program during this launch (wave 0's
  // lane 0 alone; added to FilterCtl::chain_steps once, at the launch's end)
  unsigned n_lean, n_generic;
};

// Intra-workgroup hand-off through LDS (waves on different SIMDs; no s_barrier).
// The LDS executes one wave's accesses in issue order, so a flag stored after the data is seen
// after it by any wave: no s_waitcnt before the flag (a release would drain every LDS op of the
// wave first), only a compiler fence that keeps the data stores ahead of it.
__device__ __forceinline__ void lds_publish(int* flag, int v) {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_wait_ge(const int* flag, int v) {
  while (__builtin_amdgcn_readfirstlane(
             __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) < v)
    __builtin_amdgcn_s_sleep(1);
}

// Wave 0's corrections (see k_chain, A2): functions of their own, so that their register
// allocation is not the one of the kernel's four wave programs together (the shared allocation
// spilled SGPRs, and their reloads sat in this loop). LDS through address-space-3 references.
//
// Two programs: the generic one, chain_wave0 (wave0_steps), holds every case; the lean one,
// chain_wave0_lean (wave0_lean_steps), holds the common case alone — a landmark already in the
// map, a valid id, a finite nonsingular S, angles within normalize_angle_near's range — and neither
// the first sighting's cos / sin, nor the generic normalize_angle, the re-done scalars, the skip's
// zeroing or the status word. It never computes a rare case: it detects one and returns the index
// of the first step it did not run, and the generic program resumes there (k_chain). The lean
// program's step spells the generic step's expressions in the generic step's order (every sum of
// products an explicit fma), so a step has the same bits whichever ran it
// (tests/test_gpu_chain_fastpath.py, tests/test_gpu_lean_straight.py); what differs is the control
// flow around them: the lean step is straight-line code.
template <bool J>
using LdsChain = __attribute__((address_space(3))) ChainSharedT<J>;
typedef __attribute__((address_space(3))) const MsgDesc LdsDesc;
typedef __attribute__((address_space(3))) double ldsd;
__device__ __forceinline__ void lds_publish3(__attribute__((address_space(3))) int* flag, int v) {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_wait_ge3(const __attribute__((address_space(3))) int* flag,
                                             int v) {
  while (__builtin_amdgcn_readfirstlane(
             __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) < v)
    __builtin_amdgcn_s_sleep(1);
}

// J: a Joseph chunk (m ≤ kMaxJoseph). Every step then also subtracts V_c·K_cᵀ, V_c = Σ_c·Hᵀ − K_c·S_c
// (slam.cpp:264-265's update as (I − KH)Σ(I − KH)ᵀ + K·R·Kᵀ expanded), always after the K_c·M_c term
// — the order wave 3 uses, so an entry both waves compute has the same bits.
//
// c0: the step to start at. What step c0 > 0 would hold in registers had the function run from
// step 0 is all in LDS: wave 0 stores its cross (the next step's pk / pm) and x[U] every step,
// and wave 3 stores the rest of the block with the same operands in the same order, so the block
// after step c0 − 1 is whole once pdone ≥ c0.
template <bool J>
__device__ __forceinline__ void wave0_steps(LdsChain<J>& sh, LdsDesc& d, int c0, int m, int nu,
                                            double r_noise, unsigned seq) {
  constexpr int JM = ChainSharedT<J>::JM;
  const int lane = threadIdx.x & 63;
  (void)seq;  // (diagnostic stamps)
  // Lane ℓ carries row ℓ of the step's block columns (pk = Σ[ℓ, pA]) and column ℓ of its block
  // rows (pm = Σ[pA, ℓ]) in registers from one step to the next: the cross update of step c
  // produces exactly step c+1's pk (and pm for the later columns). S needs no block read:
  // (Σ·Hᵀ)[ℓ] is the first half of K anyway, and S = H·(Σ·Hᵀ)[pA] takes five lanes' values by
  // v_readlane. The pose / landmark x of a step come by v_readlane from the lane that updated
  // them. Lanes ≥ |U| carry a clamped row and never store.
  const int lr = lane < kMaxU ? lane : kMaxU - 1;
  const int ul = sh.u[lr];
  if (c0 > 0) {  // wave 3's step c0 − 1 outside the cross (the nx columns / rows below)
    lds_wait_ge3(&sh.pdone, c0);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
  }
  double pk[5], pm[5];
  double xl = sh.xU[0][lr];
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const int col = a < 3 ? a : 3 + 2 * c0 + a - 3;  // pA of step c0 = {0, 1, 2, pj, pj + 1}
    pk[a] = sh.im.D[lr][col];
    pm[a] = sh.im.D[col][lr];
  }
  // Look-ahead operands of the next marker's cross (see the step): rn = Σ[ℓ, nx..nx+1] and
  // qn = Σ[nx..nx+1, ℓ] one step old, and the previous step's K (kp) and M (mp) of this lane.
  // (A start at c0 > 0 reads them with step c0 − 1 applied and keeps step 0's kp = mp = 0.)
  double rn[2], qn[2], kp0 = 0.0, kp1 = 0.0, mp0 = 0.0, mp1 = 0.0, vp0 = 0.0, vp1 = 0.0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = min(5 + 2 * c0 + j, kMaxU - 1);
    rn[j] = sh.im.D[lr][col];
    qn[j] = sh.im.D[col][lr];
  }
  // A step's geometry (first sighting, ẑ, H) needs only x after the step before. It is computed
  // right after that step's state update, ahead of the step's cross update, so the two
  // independent chains (f64 ALU vs LDS round trips) interleave in one basic block.
  double lx = 0.0, ly = 0.0, H0[5], H1[5], zhat[2], braw = 0.0;
  bool init = false, bok = true;
  // the marker's measurement and skip flag, read one step ahead (the descriptor and the skip list
  // are constant during the chunk): their LDS round trip stays off the step's dependent chain
  const bool noinit = (d.flags & kNoInit) != 0;
  double zn0 = 0.0, zn1 = 0.0;
  int skn = 0;
  if (c0 < m) {
    zn0 = d.z[c0][0];
    zn1 = d.z[c0][1];
    skn = sh.skip[c0];
  }
  auto geometry = [&](int c) {
    const int pj = 3 + 2 * c;
    const double pose[3] = {readlane_f64(xl, 0), readlane_f64(xl, 1), readlane_f64(xl, 2)};
    lx = readlane_f64(xl, pj);
    ly = readlane_f64(xl, pj + 1);
    init = false;
    // slam.cpp:213-216 (zn, skn: marker c); a wave-uniform test, so a scalar branch
    if (__builtin_amdgcn_readfirstlane(!skn && !noinit && lx == 0.0 && ly == 0.0)) {
      init = true;
      sh.any_init = 1;
      lx = pose[1] + zn0 * cos(zn1 + pose[0]);
      ly = pose[2] + zn0 * sin(zn1 + pose[0]);
    }
    range_bearing(pose, lx, ly, zhat, H0, H1, &braw, &bok);
  };
  if (c0 < m) geometry(c0);
  for (int c = c0; c < m; ++c) {
    const int pj = 3 + 2 * c, nx = pj + 2;
    const bool more = c + 1 < m;
    EKF_STAMP(64 + 8 * c);
    const double z0 = zn0, z1 = zn1;
    bool sk = skn != 0;
    if (more) {  // marker c + 1's, for geometry(c + 1) and the next step
      zn0 = d.z[c + 1][0];
      zn1 = d.z[c + 1][1];
      skn = sh.skip[c + 1];
    }
    double Si[4], nv0, nv1, Sm_keep[4];
    EKF_STAMP(65 + 8 * c);
    // (Σ·Hᵀ)[ℓ] and (H·Σ)[:, ℓ]. H's shape (range_bearing): H0 = [0, h1, h2, −h1, −h2],
    // H1 = [−1, g1, g2, −g1, −g2] — a row times H is two FMAs on (v1 − v3, v2 − v4) (exact negations)
    const double dk1 = pk[1] - pk[3], dk2 = pk[2] - pk[4];
    const double dm1 = pm[1] - pm[3], dm2 = pm[2] - pm[4];
    double ka = fma(H0[2], dk2, H0[1] * dk1), kb = fma(H1[2], dk2, fma(H1[1], dk1, -pk[0]));
    double mm0 = fma(H0[2], dm2, H0[1] * dm1), mm1 = fma(H1[2], dm2, fma(H1[1], dm1, -pm[0]));
    {
      double Sm[4];  // S = H·(Σ·Hᵀ)[pA] + R (slam.cpp:252), the same shape
      {
        double ta[5], tb[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) {
          const int l = a < 3 ? a : pj + a - 3;
          ta[a] = readlane_f64(ka, l);
          tb[a] = readlane_f64(kb, l);
        }
        const double ta1 = ta[1] - ta[3], ta2 = ta[2] - ta[4], tb1 = tb[1] - tb[3], tb2 = tb[2] - tb[4];
        Sm[0] = fma(H0[2], ta2, H0[1] * ta1) + r_noise;
        Sm[1] = fma(H0[2], tb2, H0[1] * tb1);
        Sm[2] = fma(H1[2], ta2, fma(H1[1], ta1, -ta[0]));
        Sm[3] = fma(H1[2], tb2, fma(H1[1], tb1, -tb[0])) + r_noise;
      }
      for (int k = 0; k < 4; ++k) Sm_keep[k] = Sm[k];
      // The common case without a branch (so the step's scalar chain is one basic block): a
      // finite, nonsingular S and a bearing / innovation within normalize_angle_near's range.
      // Anything else — a skipped marker, a singular S (arma's inv throws), an angle beyond it —
      // redoes these scalars on the generic path below, in the reference's order; the common
      // case's values are that path's bit for bit.
      const double det = inv2_calc(Sm, Si);
      nv0 = z0 - zhat[0];
      bool nok;
      nv1 = normalize_angle_near(z1 - zhat[1], &nok);
      const bool good = !sk && bok && nok && inv2_ok(det, Si);
      if (!__builtin_amdgcn_readfirstlane(good)) {  // (uniform: every lane has the same scalars)
        if (!bok) zhat[1] = normalize_angle(braw);  // |θ| > π: the generic fmod path
        if (!sk && inv2(Sm, Si)) {
          nv0 = z0 - zhat[0];
          bool nok2;
          const double nn = normalize_angle_near(z1 - zhat[1], &nok2);
          nv1 = nok2 ? nn : normalize_angle(z1 - zhat[1]);
        } else {
          if (!sk) sh.status |= EKF_FLAG_NUMERIC_D;  // same value from every lane
          sk = true;
#pragma unroll
          for (int a = 0; a < 5; ++a) H0[a] = H1[a] = 0.0;
          Si[0] = Si[1] = Si[2] = Si[3] = 0.0;
          nv0 = nv1 = 0.0;
          ka = kb = mm0 = mm1 = 0.0;
          // ... and S itself (non-finite here): the Joseph form's V = Σ·Hᵀ − K·S below must come
          // out 0 like K, not 0·NaN
          for (int k = 0; k < 4; ++k) Sm_keep[k] = 0.0;
        }
      }
    }
    // The next marker's cross operands (Bx = {0, 1, 2, nx, nx+1}) after step c−1. Pose columns /
    // rows: pk / pm (pA ⊃ pose). The nx columns / rows were read one step back (rn / qn, after
    // step c−2) and get step c−1's rank-2 term here from registers: K_{c−1} of this lane (kp)
    // and of the nx rows (v_readlane), M_{c−1} of this column (mp) and of the nx columns
    // (v_readlane) — the writers' expression, operands and order (wave 3's, or this wave's cross
    // update), so the same bits. Step 0 has kp = mp = 0: rank2_sub(v, 0, 0, 0, 0) = v.
    double xr[5], xq[5];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      xr[k] = pk[k];
      xq[k] = pm[k];
    }
    // wave 3's progress, read here (≈ 1 000 cycles into the step, when it has normally finished
    // step c − 1) and tested below: the flag's LDS round trip off the chain's path
    const int pd_early = __hip_atomic_load(&sh.pdone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    {  // K_{c−1} and M_{c−1} of the nx rows / columns: broadcast LDS reads of what step c−1
       // stored (the stored values are the registers' values; two reads instead of 8 readlanes)
      const int l0 = more ? nx : 0, cp = c > 0 ? c - 1 : 0;
      const double mqx = sh.MU[cp][l0][0], mqy = sh.MU[cp][l0][1];
      const double mq2x = sh.MU[cp][l0 + 1][0], mq2y = sh.MU[cp][l0 + 1][1];
      const double kqx = sh.KU[cp][l0][0], kqy = sh.KU[cp][l0][1];
      const double kq2x = sh.KU[cp][l0 + 1][0], kq2y = sh.KU[cp][l0 + 1][1];
      // step 0: kp = mp = 0 and the (stale, finite) reads multiply zeros: rank2_sub returns v
      xr[3] = rank2_sub(rn[0], kp0, kp1, mqx, mqy);
      xr[4] = rank2_sub(rn[1], kp0, kp1, mq2x, mq2y);
      xq[3] = rank2_sub(qn[0], kqx, kqy, mp0, mp1);
      xq[4] = rank2_sub(qn[1], kq2x, kq2y, mp0, mp1);
      if (J) {  // − V_{c−1}·K_{c−1}ᵀ (step 0: vp = kp = 0)
        const int cj = min(cp, JM - 1);
        const double vqx = sh.VU[cj][l0][0], vqy = sh.VU[cj][l0][1];
        const double vq2x = sh.VU[cj][l0 + 1][0], vq2y = sh.VU[cj][l0 + 1][1];
        xr[3] = rank2_sub(xr[3], vp0, vp1, kqx, kqy);
        xr[4] = rank2_sub(xr[4], vp0, vp1, kq2x, kq2y);
        xq[3] = rank2_sub(xq[3], vqx, vqy, kp0, kp1);
        xq[4] = rank2_sub(xq[4], vq2x, vq2y, kp0, kp1);
      }
    }
    EKF_STAMP(66 + 8 * c);
    // the cross after next (nx + 2): read once wave 3 has applied step c−1 outside this step's
    // cross, before this step's cross update writes its Bx rows (wave 3 writes these entries for
    // step c only after the publish below, whose release waits for the reads)
    if (c + 2 < m) {
      // the LDS serves this wave's accesses in order, and wave 3 stored its entries before the
      // flag: once a flag value ≥ c has been read, later reads see the entries (a compiler fence
      // keeps them after the test)
      if (__builtin_amdgcn_readfirstlane(pd_early) < c) lds_wait_ge3(&sh.pdone, c);
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        rn[j] = sh.im.D[lr][nx + 2 + j];
        qn[j] = sh.im.D[nx + 2 + j][lr];
      }
    }
    const int jx = __builtin_amdgcn_readlane(ul, pj);  // sh.u[pj] (ul = sh.u[lane], pj < kMaxU)
    (void)jx;  // (a first sighting's rows: the generic program's)
    EKF_STAMP(67 + 8 * c);
    // K = Σ·Hᵀ·S⁻¹ = ka·Si[0] + kb·Si[2], ka·Si[1] + kb·Si[3]. Which product the compiler fuses
    // into the sum differed between the two programs (the lean one took ka's, 1e-12 in x after a
    // drive): these sums of products and the two below are spelled out, the way the single
    // program of before was compiled.
    const double K0 = fma(kb, Si[2], ka * Si[0]);
    const double K1 = fma(kb, Si[3], ka * Si[1]);
    // Joseph: V = Σ·Hᵀ − K·S of this lane's row (zero in exact arithmetic; the form's rounding)
    const double V0 = J ? ka - fma(K0, Sm_keep[0], K1 * Sm_keep[2]) : 0.0;
    const double V1 = J ? kb - fma(K0, Sm_keep[1], K1 * Sm_keep[3]) : 0.0;
    {
      double xt = xl;
      xt = (init && ul == jx) ? lx : ((init && ul == jx + 1) ? ly : xt);
      xt = xt + fma(K0, nv0, K1 * nv1);             // slam.cpp:261
      bool tok;                                     // slam.cpp:267 on lane 0, branch-free
      const double tn = normalize_angle_near(xt, &tok);
      const double xraw = xt;
      xt = lane == 0 ? tn : xt;
      // lane 0's θ beyond normalize_angle_near's range: the generic path (a scalar branch)
      if (__builtin_amdgcn_ballot_w64(!tok) & 1ull) {
        if (lane == 0) xt = normalize_angle(xraw);
      }
      xl = xt;
      *(lane < nu ? &sh.xU[0][lane] : &sh.junk[0][lane]) = xt;
    }
    {
      const bool in = lane < nu, st = lane < kMaxU;
      ldsd* kd = st ? &sh.KU[c][lane][0] : &sh.junk2[lane][0];
      ldsd* md = st ? &sh.MU[c][lane][0] : &sh.junk2[lane][0];
      kd[0] = in ? K0 : 0.0;
      kd[1] = in ? K1 : 0.0;
      md[0] = in ? mm0 : 0.0;
      md[1] = in ? mm1 : 0.0;
      if (J) {  // V and S of the step, for waves 1–3 and the fp32 block patch
        const int cj = min(c, JM - 1);
        ldsd* vd = st ? &sh.VU[cj][lane][0] : &sh.junk2[lane][0];
        vd[0] = in ? V0 : 0.0;
        vd[1] = in ? V1 : 0.0;
        if (lane == 0)
          for (int k = 0; k < 4; ++k) sh.Ss[cj][k] = sk ? 0.0 : Sm_keep[k];
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < 5; ++a) {
        sh.Hs[c][0][a] = H0[a];
        sh.Hs[c][1][a] = H1[a];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) sh.Sis[c][k] = Si[k];
      sh.nu[c][0] = nv0;
      sh.nu[c][1] = nv1;
    }
    lds_publish3(&sh.pub, c + 1);
    EKF_STAMP(68 + 8 * c);
    if (more) {
      // K and M of the five Bx rows / columns: broadcast LDS reads of what this step stored
      // above (issued before geometry(c + 1), so its latency hides; ds_read_b128 each)
      double kx0[5], kx1[5], mx0[5], mx1[5], vx0[5], vx1[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int l = k < 3 ? k : nx + k - 3;
        const double kkx = sh.KU[c][l][0], kky = sh.KU[c][l][1];
        const double mkx = sh.MU[c][l][0], mky = sh.MU[c][l][1];
        kx0[k] = kkx;
        kx1[k] = kky;
        mx0[k] = mkx;
        mx1[k] = mky;
        if (J) {
          const int cj = min(c, JM - 1);
          vx0[k] = sh.VU[cj][l][0];
          vx1[k] = sh.VU[cj][l][1];
        }
      }
      geometry(c + 1);
      // wave 3's step c−1 writes outside this step's cross must land before this cross update
      // overwrites the nx columns / rows (waited for above already when c + 2 < m)
      if (c + 2 >= m && __builtin_amdgcn_readfirstlane(pd_early) < c) lds_wait_ge3(&sh.pdone, c);
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      // all rows × Bx columns: next step's pk
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int col = k < 3 ? k : nx + k - 3;
        pk[k] = rank2_sub(xr[k], K0, K1, mx0[k], mx1[k]);
        if (J) pk[k] = rank2_sub(pk[k], V0, V1, kx0[k], kx1[k]);
        *(lane < nu ? &sh.im.D[lane][col] : &sh.junk[0][lane]) = pk[k];
      }
      // Bx rows × every other column (the block is kept whole so that the chunk's final Σ[U,U]
      // can seed the next chunk): next step's pm there
      const bool later = lane >= 3 && lane < nu && lane != nx && lane != nx + 1;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int row = k < 3 ? k : nx + k - 3;
        double v = rank2_sub(xq[k], kx0[k], kx1[k], mm0, mm1);
        if (J) v = rank2_sub(v, vx0[k], vx1[k], K0, K1);
        pm[k] = v;
        *(later ? &sh.im.D[row][lane] : &sh.junk[0][lane]) = v;
      }
      // (the Bx × Bx entries: lane `row` stored the same value as its pk, same operands)
      kp0 = K0;
      kp1 = K1;
      mp0 = mm0;
      mp1 = mm1;
      vp0 = V0;
      vp1 = V1;
    }
    EKF_STAMP(70 + 8 * c);
  }
}

// The lean program: wave0_steps' step from c0 = 0 for common-case markers, as straight-line code.
// → the first step it did not run (m: the whole chunk); nothing of that step is stored or
// published, and every step before it is complete (its cross update included), so the generic
// program resumes there from LDS.
//
// A step is two basic blocks, so that the scheduler can fill the f64 chains' latency (atan2, the
// reciprocals) with the independent work beside them (the M row, ν, the cross update's FMAs and
// stores, the publication):
//   1. the step's scalars up to the new x — H·Σ products, S, S⁻¹, ν, the look-ahead operands, K;
//   2. every store and the publication, geometry(c + 1) and the cross update.
// Between them, the step's one test: a wave-uniform word that collects every rare case (marker c
// skipped or sighted for the first time, found by geometry(c) a step earlier; a bearing, ν or θ
// beyond normalize_angle_near's range; S singular or not finite) and whether wave 3 is behind
// (pdone < c, the one place a spin can be needed; out of line). What it takes to get there:
//   - the last step is peeled (More = false: no look-ahead, no cross update), so the loop's steps
//     have a next marker without a test, and its look-ahead columns nx + 2 are read with a clamped
//     index where the generic step tests c + 2 < m (unused when there is no marker c + 2);
//   - lane 0's H, S⁻¹, ν (and S) go through a selected address like every other store here;
//   - a rare marker's scalars are computed (on whatever its x holds) and discarded.
template <bool J>
__device__ __forceinline__ int wave0_lean_steps(LdsChain<J>& sh, LdsDesc& d, int m, int nu,
                                                double r_noise, unsigned seq) {
  constexpr int JM = ChainSharedT<J>::JM;
  const int lane = threadIdx.x & 63;
  (void)seq;  // (diagnostic stamps)
  const int lr = lane < kMaxU ? lane : kMaxU - 1;
  // Entry: every LDS read is issued before the first is needed; geometry(0) waits for x alone and
  // the block reads land beside it. (An empty or an association chunk is the generic program's:
  // the descriptor's flags are the first read back.)
  const int flags = d.flags;
  double xl = sh.xU[0][lr];
  double zn0 = d.z[0][0], zn1 = d.z[0][1];
  int skn = sh.skip[0];
  double pk[5], pm[5], rn[2], qn[2];
#pragma unroll
  for (int a = 0; a < 5; ++a) {  // pA of step 0 = {0, 1, 2, 3, 4}
    pk[a] = sh.im.D[lr][a];
    pm[a] = sh.im.D[a][lr];
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    rn[j] = sh.im.D[lr][5 + j];
    qn[j] = sh.im.D[5 + j][lr];
  }
  if (m < 1 || (flags & kNoInit) != 0) return 0;
  double kp0 = 0.0, kp1 = 0.0, mp0 = 0.0, mp1 = 0.0, vp0 = 0.0, vp1 = 0.0;
  double H0[5], H1[5], zhat[2];
  bool bok = true;
  // marker c's ẑ and H from x after step c − 1 (zn, skn: marker c) → whether the marker is not the
  // lean program's: skipped, or a first sighting (slam.cpp:213-216). Wave-uniform.
  auto geometry = [&](int c) -> bool {
    const int pj = 3 + 2 * c;
    const double pose[3] = {readlane_f64(xl, 0), readlane_f64(xl, 1), readlane_f64(xl, 2)};
    const double lx = readlane_f64(xl, pj), ly = readlane_f64(xl, pj + 1);
    double braw;
    range_bearing(pose, lx, ly, zhat, H0, H1, &braw, &bok);
    return skn != 0 || (lx == 0.0 && ly == 0.0);
  };
  bool rare_next = geometry(0);
  // step c; → true: not run (a rare case)
  auto step = [&](int c, auto more_t) -> bool {
    constexpr bool More = decltype(more_t)::value;  // a marker c + 1 follows
    const int pj = 3 + 2 * c, nx = pj + 2;
    EKF_STAMP(64 + 8 * c);
    const double z0 = zn0, z1 = zn1;
    bool rare = rare_next;
    if constexpr (More) {  // marker c + 1's, for geometry(c + 1) and the next step
      zn0 = d.z[c + 1][0];
      zn1 = d.z[c + 1][1];
      skn = sh.skip[c + 1];
    }
    double Si[4], Sm[4];
    EKF_STAMP(65 + 8 * c);
    const double dk1 = pk[1] - pk[3], dk2 = pk[2] - pk[4];
    const double dm1 = pm[1] - pm[3], dm2 = pm[2] - pm[4];
    const double ka = fma(H0[2], dk2, H0[1] * dk1), kb = fma(H1[2], dk2, fma(H1[1], dk1, -pk[0]));
    const double mm0 = fma(H0[2], dm2, H0[1] * dm1), mm1 = fma(H1[2], dm2, fma(H1[1], dm1, -pm[0]));
    {
      double ta[5], tb[5];
#pragma unroll
      for (int a = 0; a < 5; ++a) {
        const int l = a < 3 ? a : pj + a - 3;
        ta[a] = readlane_f64(ka, l);
        tb[a] = readlane_f64(kb, l);
      }
      const double ta1 = ta[1] - ta[3], ta2 = ta[2] - ta[4], tb1 = tb[1] - tb[3], tb2 = tb[2] - tb[4];
      Sm[0] = fma(H0[2], ta2, H0[1] * ta1) + r_noise;
      Sm[1] = fma(H0[2], tb2, H0[1] * tb1);
      Sm[2] = fma(H1[2], ta2, fma(H1[1], ta1, -ta[0]));
      Sm[3] = fma(H1[2], tb2, fma(H1[1], tb1, -tb[0])) + r_noise;
    }
    const double det = inv2_calc(Sm, Si);
    const double nv0 = z0 - zhat[0];
    bool nok;
    const double nv1 = normalize_angle_near(z1 - zhat[1], &nok);
    rare |= !(bok & nok & inv2_ok(det, Si));  // (&: no short-circuit branch)
    // the next marker's cross operands after step c − 1 (wave0_steps)
    double xr[5], xq[5];
    int pd_early = 0;
    if constexpr (More) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        xr[k] = pk[k];
        xq[k] = pm[k];
      }
      pd_early = __hip_atomic_load(&sh.pdone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const int cp = c > 0 ? c - 1 : 0;
      const double mqx = sh.MU[cp][nx][0], mqy = sh.MU[cp][nx][1];
      const double mq2x = sh.MU[cp][nx + 1][0], mq2y = sh.MU[cp][nx + 1][1];
      const double kqx = sh.KU[cp][nx][0], kqy = sh.KU[cp][nx][1];
      const double kq2x = sh.KU[cp][nx + 1][0], kq2y = sh.KU[cp][nx + 1][1];
      xr[3] = rank2_sub(rn[0], kp0, kp1, mqx, mqy);
      xr[4] = rank2_sub(rn[1], kp0, kp1, mq2x, mq2y);
      xq[3] = rank2_sub(qn[0], kqx, kqy, mp0, mp1);
      xq[4] = rank2_sub(qn[1], kq2x, kq2y, mp0, mp1);
      if (J) {
        const int cj = min(cp, JM - 1);
        const double vqx = sh.VU[cj][nx][0], vqy = sh.VU[cj][nx][1];
        const double vq2x = sh.VU[cj][nx + 1][0], vq2y = sh.VU[cj][nx + 1][1];
        xr[3] = rank2_sub(xr[3], vp0, vp1, kqx, kqy);
        xr[4] = rank2_sub(xr[4], vp0, vp1, kq2x, kq2y);
        xq[3] = rank2_sub(xq[3], vqx, vqy, kp0, kp1);
        xq[4] = rank2_sub(xq[4], vq2x, vq2y, kp0, kp1);
      }
    }
    EKF_STAMP(66 + 8 * c);
    const double K0 = fma(kb, Si[2], ka * Si[0]);
    const double K1 = fma(kb, Si[3], ka * Si[1]);
    const double V0 = J ? ka - fma(K0, Sm[0], K1 * Sm[2]) : 0.0;
    const double V1 = J ? kb - fma(K0, Sm[1], K1 * Sm[3]) : 0.0;
    double xt = xl + fma(K0, nv0, K1 * nv1);      // slam.cpp:261
    bool tok;                                     // slam.cpp:267 on lane 0, branch-free
    const double tn = normalize_angle_near(xt, &tok);
    xt = lane == 0 ? tn : xt;
    // The step's one test, before its first store. (Lane 0's word: the other lanes' differ in tok
    // alone, which is about θ.)
    const int out = static_cast<int>(__builtin_amdgcn_ballot_w64(rare | !tok) & 1ull);
    const int behind = More ? __builtin_amdgcn_readfirstlane(pd_early) < c : 0;
    if (__builtin_expect((out | behind) != 0, 0)) {
      if (out) return true;
      // wave 3's step c − 1 outside this step's cross must land before the reads of the cross
      // after next and before this step's cross update overwrites the nx columns / rows
      lds_wait_ge3(&sh.pdone, c);
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    EKF_STAMP(67 + 8 * c);
    if constexpr (More) {  // the cross after next (nx + 2), before this step's cross update
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = min(nx + 2 + j, kMaxU - 1);
        rn[j] = sh.im.D[lr][col];
        qn[j] = sh.im.D[col][lr];
      }
    }
    xl = xt;
    ldsd* const sink = &sh.junk[0][lane];
    // lane 0's records (up to 10 doubles from one selected base): the other lanes' go to the sink
    // rows taken as one array, each lane's from its own 16 bytes on (lane 63 ends at entry 135 of
    // 256; the tails lap over the neighbours' and the other waves' sinks, which nobody reads)
    ldsd* const sink0 = &sh.junk[0][0] + 2 * lane;
    *(lane < nu ? &sh.xU[0][lane] : sink) = xt;
    {
      const bool in = lane < nu, st = lane < kMaxU;
      ldsd* kd = st ? &sh.KU[c][lane][0] : &sh.junk2[lane][0];
      ldsd* md = st ? &sh.MU[c][lane][0] : &sh.junk2[lane][0];
      kd[0] = in ? K0 : 0.0;
      kd[1] = in ? K1 : 0.0;
      md[0] = in ? mm0 : 0.0;
      md[1] = in ? mm1 : 0.0;
      if (J) {
        const int cj = min(c, JM - 1);
        ldsd* vd = st ? &sh.VU[cj][lane][0] : &sh.junk2[lane][0];
        vd[0] = in ? V0 : 0.0;
        vd[1] = in ? V1 : 0.0;
        ldsd* sd = lane == 0 ? &sh.Ss[cj][0] : sink0;
#pragma unroll
        for (int k = 0; k < 4; ++k) sd[k] = Sm[k];
      }
    }
    ldsd* hd = lane == 0 ? &sh.Hs[c][0][0] : sink0;
    ldsd* id = lane == 0 ? &sh.Sis[c][0] : sink0;
    ldsd* nd = lane == 0 ? &sh.nu[c][0] : sink0;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      hd[a] = H0[a];
      hd[5 + a] = H1[a];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) id[k] = Si[k];
    nd[0] = nv0;
    nd[1] = nv1;
    lds_publish3(&sh.pub, c + 1);
    EKF_STAMP(68 + 8 * c);
    if constexpr (More) {
      // K and M of the five Bx rows / columns: broadcast LDS reads of what this step stored
      double kx0[5], kx1[5], mx0[5], mx1[5], vx0[5], vx1[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int l = k < 3 ? k : nx + k - 3;
        kx0[k] = sh.KU[c][l][0];
        kx1[k] = sh.KU[c][l][1];
        mx0[k] = sh.MU[c][l][0];
        mx1[k] = sh.MU[c][l][1];
        if (J) {
          const int cj = min(c, JM - 1);
          vx0[k] = sh.VU[cj][l][0];
          vx1[k] = sh.VU[cj][l][1];
        }
      }
      rare_next = geometry(c + 1);
      // all rows × Bx columns: next step's pk
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int col = k < 3 ? k : nx + k - 3;
        pk[k] = rank2_sub(xr[k], K0, K1, mx0[k], mx1[k]);
        if (J) pk[k] = rank2_sub(pk[k], V0, V1, kx0[k], kx1[k]);
        *(lane < nu ? &sh.im.D[lane][col] : sink) = pk[k];
      }
      // Bx rows × every other column: next step's pm there
      const bool later = lane >= 3 && lane < nu && lane != nx && lane != nx + 1;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int row = k < 3 ? k : nx + k - 3;
        double v = rank2_sub(xq[k], kx0[k], kx1[k], mm0, mm1);
        if (J) v = rank2_sub(v, vx0[k], vx1[k], K0, K1);
        pm[k] = v;
        *(later ? &sh.im.D[row][lane] : sink) = v;
      }
      kp0 = K0;
      kp1 = K1;
      mp0 = mm0;
      mp1 = mm1;
      vp0 = V0;
      vp1 = V1;
    }
    EKF_STAMP(70 + 8 * c);
    return false;
  };
  for (int c = 0; c + 1 < m; ++c)
    if (step(c, std::true_type{})) return c;
  return step(m - 1, std::false_type{}) ? m - 1 : m;
}

template <bool J>
__device__ __noinline__ void chain_wave0(LdsChain<J>* shp, LdsDesc* dp, int c0, int m, int nu,
                                         double r_noise, unsigned seq) {
  wave0_steps<J>(*shp, *dp, c0, m, nu, r_noise, seq);
}
template <bool J>
__device__ __noinline__ int chain_wave0_lean(LdsChain<J>* shp, LdsDesc* dp, int m, int nu,
                                             double r_noise, unsigned seq) {
  // (arguments arrive in vector registers: said to be wave-uniform here, the step loop's control
  // flow and addresses are scalar)
  return wave0_lean_steps<J>(*shp, *dp, __builtin_amdgcn_readfirstlane(m),
                             __builtin_amdgcn_readfirstlane(nu), readfirstlane_f64(r_noise), seq);
}

// The previous chunk's predict on the rebuild operands: v + α_i·Σ[0][j] +
// (Σ[i][0] + α_i·Σ00)·α_j + Q̄, for D = Σ_in'[U, U] → im.D, R = Σ_in'[U, U'] → im.R and
// C = Σ_in'[U', U] → im.C (R / C columns k ≥ |U'| up to 36 zero: MFMA k padding). The raw blocks
// are in LDS first — a staged image (k_stage) copied in, or a gathering chain's own loads
// (thread tid's entries e = tid + i·256 of the 36 × 36 block) — then predict_prev applies the
// predict from the raw row 0 / column 0 (pv.r0U, c0U, r0P, c0P; pv.first, a1, a2).
constexpr int kChainThreads = 256;
constexpr int kRebW = kMaxU + 1;                                      // 36: entry e = a·36 + b
constexpr int kRebPer = (kRebW * kRebW + kChainThreads - 1) / kChainThreads;  // 6
// The predict (slam.cpp:198) changes an entry of a block over U × U' only in rows / columns 1 and 2
// (α_i = 0 unless u_i ∈ {1, 2}, and u_i = i for the pose positions of U and U') and on the pose
// diagonal (Q̄): 4·36 − 3 entries of the 36 × 36 block. Special entry s → (a, b): s < 72 rows 1, 2
// (b = 0..35); s < 140 columns 1, 2 (a = 0, 3..35); s = 140 the (0, 0) entry.
constexpr int kSpec = 141;
__device__ __forceinline__ void special_entry(int s, int& a, int& b) {
  if (s < 72) {
    a = 1 + (s >= 36);
    b = s - (s >= 36 ? 36 : 0);
  } else if (s < 140) {
    const int r = s - 72, h = r >= 34;
    b = 1 + h;
    const int a2 = r - (h ? 34 : 0);
    a = a2 == 0 ? 0 : a2 + 2;
  } else {
    a = 0;
    b = 0;
  }
}

// A gathering chain's raw blocks, stored at the image's positions with the image's zeros (what
// k_stage stores for a staged chain): thread tid's entries e = tid + 256·i = (a, b) of the
// 36-wide blocks, C transposed.
template <typename T, typename Shared>
__device__ __forceinline__ void store_raw_image(Shared& sh, const T (&vd)[kRebPer],
                                                const T (&vr)[kRebPer], const T (&vc)[kRebPer],
                                                int tid, int nu, int np) {
#pragma unroll
  for (int i = 0; i < kRebPer; ++i) {
    const int e = tid + i * kChainThreads;
    const int a = e / kRebW, b = e % kRebW;
    if (a < kMaxU) {
      sh.im.D[a][b] = a < nu && b < nu ? static_cast<double>(vd[i]) : 0.0;
      sh.im.R[a][b] = a < nu && b < np ? static_cast<double>(vr[i]) : 0.0;
    }
    if (e < kRebW * kRebW) sh.im.C[b][a] = a < nu && b < np ? static_cast<double>(vc[i]) : 0.0;
  }
}

// The previous chunk's predict over the raw image in LDS (staged or gathered: the one body both
// paths run), one special entry (a, b) per thread applied to D, R and C. An entry depends only on
// its own raw value and the raw row 0 / column 0 (pv.r0U, c0U, r0P, c0P), so one wait covers
// every operand read and no barrier separates reads from writes.
template <typename Shared>
__device__ __forceinline__ void predict_prev(Shared& sh, int tid, int nu, int np, double q) {
  if (sh.pv.first == 0) return;  // (uniform)
  int a, b;
  special_entry(min(tid, kSpec - 1), a, b);
  const bool sp = tid < kSpec;
  const int ac = min(a, kMaxU - 1), bc = min(b, kMaxU - 1);
  const double s00 = sh.pv.r0U[0], qa1 = sh.pv.a1, qa2 = sh.pv.a2;
  const double rd = sh.im.D[ac][b], rr = sh.im.R[ac][b], rc = sh.im.C[b][ac];
  const double r0u_b = sh.pv.r0U[bc], c0u_a = sh.pv.c0U[ac], r0p_b = sh.pv.r0P[bc];
  const double r0u_a = sh.pv.r0U[ac], c0p_b = sh.pv.c0P[bc];
  const double ai = alpha_of(a, qa1, qa2), aj = alpha_of(b, qa1, qa2);
  const bool qd = a == b && a < 3;
  double v = rd + ai * r0u_b;  // D = Σ_in'[U, U]
  v = v + (c0u_a + ai * s00) * aj;
  double v2 = rr + ai * r0p_b;  // R = Σ_in'[U, U'] (b = k over U')
  v2 = v2 + (c0u_a + ai * s00) * aj;
  double w2 = rc + aj * r0u_a;  // C = Σ_in'[U', U]
  w2 = w2 + (c0p_b + aj * s00) * ai;
  const bool okd = sp && a < nu && b < nu, okr = sp && a < nu && b < np;
  *(okd ? &sh.im.D[ac][b] : &sh.junk[0][tid & 63]) = qd ? v + q : v;
  *(okr ? &sh.im.R[ac][b] : &sh.junk[1][tid & 63]) = qd ? v2 + q : v2;
  *(okr ? &sh.im.C[b][ac] : &sh.junk[2][tid & 63]) = qd ? w2 + q : w2;
}

// A thread's coordinates in the workgroup: its wave and lane, and the lane's place in a 16 × 16
// f64 MFMA tile (i16 = the row / column within the tile, k4 = the k of a k-step).
struct ChainLane {
  int tid, wv, ln, i16, k4;
};

// Four interleaved partial sums of a[k]·b[k·sb] over k < K, combined by sum4: the summation order
// of every VALU dot product of the rebuild (the bands beside the MFMA tiles, x_in[U]).
template <int K>
__device__ __forceinline__ void dot4(const double* a, const double* b, int sb, double (&acc)[4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k & 3] = fma(a[k], b[k * sb], acc[k & 3]);
}
__device__ __forceinline__ double sum4(const double (&acc)[4]) {
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// ---- early loads --------------------------------------------------------------------------------
// Everything a rebuilding chunk loads comes in as 16-byte pieces (one buffer_load_dwordx4 each). The
// staged image (StageRec::im) has the LDS image's element order, so piece p goes to piece p of
// sh.im; the previous record's Z (|U| rows of ZC, the record's rows kZJ wide: ZC / 2 pieces a row)
// and Y (kZC × kMaxU contiguous) are pairs of neighbours. ChainLoads holds a thread's values in
// flight between issue_early_loads and land_rebuild_operands.
template <typename T, bool J>
struct ChainLoads {
  static constexpr int ZC = ChainSharedT<J>::ZC;
  static constexpr int kImPieces = static_cast<int>(sizeof(RebuildImage<T>) / 16);  // 954 (fp32) / 1 908
  static constexpr int kPerIm = (kImPieces + kChainThreads - 1) / kChainThreads;    // 4 / 8
  static constexpr int kZP = ZC / 2, kZPieces = kMaxU * kZP;                        // 560 (Joseph: 1 120)
  static constexpr int kPerZ = (kZPieces + kChainThreads - 1) / kChainThreads;      // 3 (Joseph: 5)
  static constexpr int kYPieces = kZC * kMaxU / 2;                                  // 560
  static constexpr int kPerY = (kYPieces + kChainThreads - 1) / kChainThreads;      // 3
  q16 vim[kPerIm], vz[kPerZ], vy[kPerY];
  double r0u, c0u, r0p, c0p, x2;  // raw row 0 / column 0 of Σ_in' at U and U', x'[U]
  double x0, x1, pa1, pa2, tq;    // the record's x[U'], Zx', a1, a2; t_map_odom
  int pflags;                     // the record's flags
};

// the previous record: Z', Y', x[U'], Zx' and its predict (through a descriptor: size 0 = zeros)
template <typename T, bool J>
__device__ __forceinline__ void load_prev_record(ChainLoads<T, J>& L, __amdgpu_buffer_rsrc_t rr,
                                                 int tid) {
  using CL = ChainLoads<T, J>;
  constexpr unsigned oZ = offsetof(ChunkRec, Z), oY = offsetof(ChunkRec, Y);
  const int tc = tid < kMaxU ? tid : 0;
#pragma unroll
  for (int i = 0; i < CL::kPerZ; ++i) {
    const int p = tid + i * kChainThreads, pz = p < CL::kZPieces ? p : 0;
    L.vz[i] = ld_q16(rr, oZ + 8u * ((pz / CL::kZP) * kZJ + 2 * (pz % CL::kZP)));
  }
#pragma unroll
  for (int i = 0; i < CL::kPerY; ++i) {
    const int p = tid + i * kChainThreads;
    L.vy[i] = ld_q16(rr, oY + 16u * (p < CL::kYPieces ? p : 0));
  }
  L.x0 = ld_f64(rr, offsetof(ChunkRec, xU) + 8u * tc, 0);
  L.x1 = ld_f64(rr, offsetof(ChunkRec, Zx) + 8u * tc, 0);
  L.pflags = static_cast<int>(__builtin_amdgcn_raw_buffer_load_b32(rr, offsetof(ChunkRec, flags), 0, 0));
  L.pa1 = ld_f64(rr, offsetof(ChunkRec, a1), 0);
  L.pa2 = ld_f64(rr, offsetof(ChunkRec, a2), 0);
}

// kLook with staged operands: the loads do not depend on A0's index sets, so they are issued
// before it and land during A0 (whose barrier orders LDS only). The image was staged by the
// k_stage two chunks back, right behind the Σ pass that wrote Σ_in': the same values as the
// gather of land_rebuild_operands, in the LDS image's layout (≈ 5 000 cycles less than the ≈ 1 900
// scattered lines of the gather through one CU). Issued unconditionally, through buffer descriptors
// of size 0 unless `early` (zeros, no access): a load under a branch is waited for at the branch's
// join on the path that skipped it — vmcnt(0) before A0's first use of `aj`.
template <typename T, bool J>
__device__ __forceinline__ void issue_early_loads(ChainLoads<T, J>& L, const StageRec<T>* sg,
                                                  const ChunkRec* rp, FilterCtl* ctl, int tid,
                                                  bool early) {
  using CL = ChainLoads<T, J>;
  const int tc = tid < kMaxU ? tid : 0;
  const auto rs = buf_rsrc(sg, early ? static_cast<unsigned>(sizeof(StageRec<T>)) : 0u);
  constexpr unsigned oIm = offsetof(StageRec<T>, im);
#pragma unroll
  for (int i = 0; i < CL::kPerIm; ++i) {
    const int p = tid + i * kChainThreads;
    L.vim[i] = ld_q16(rs, oIm + 16u * (p < CL::kImPieces ? p : 0));
  }
  load_prev_record(L, buf_rsrc(rp, early ? static_cast<unsigned>(sizeof(ChunkRec)) : 0u), tid);
  L.r0u = ld_f64(rs, offsetof(StageRec<T>, r0u) + 8u * tc, 0);
  L.c0u = ld_f64(rs, offsetof(StageRec<T>, c0u) + 8u * tc, 0);
  L.r0p = ld_f64(rs, offsetof(StageRec<T>, r0p) + 8u * tc, 0);
  L.c0p = ld_f64(rs, offsetof(StageRec<T>, c0p) + 8u * tc, 0);
  L.x2 = ld_f64(rs, offsetof(StageRec<T>, xg) + 8u * tc, 0);
  L.tq = ctl->tmo[tid < 3 ? tid : 0];
}

// ---- A0: index sets U (this chunk) and U' (kLook: the previous chunk, from the descriptor) --------
// Thread t ≥ 3 of an index set: the Σ column of its marker's landmark id, x for odd t − 3 and y
// for even (a bad id → slot 0's columns).
__device__ __forceinline__ bool bad_id(int id, int N) { return id < 0 || id >= N; }
__device__ __forceinline__ int column_of_id(int id, int N, int tid) {
  return (bad_id(id, N) ? 3 : 3 + 2 * id) + ((tid - 3) & 1);
}

// aj: the marker's associated id (k_assoc), for a marker whose descriptor id is negative.
template <bool J>
__device__ __forceinline__ void build_index_sets(ChainSharedT<J>& sh, const MsgDesc& d, int N, int aj,
                                                 bool look, int tid) {
  const int m = d.m;
  if (tid < kMaxU) {  // u[3+2c], u[4+2c] = the columns of marker c's landmark (bad id → slot 0's)
    int u = tid < 3 ? tid : 0;  // padding 0: loads stay in bounds
    if (tid >= 3 && tid < 3 + 2 * m) {
      const int c = (tid - 3) >> 1, idd = d.ids[c];
      const int id = idd >= 0 ? idd : aj;
      const bool bad = bad_id(id, N);
      u = column_of_id(id, N, tid);
      if (((tid - 3) & 1) == 0) {
        sh.skip[c] = bad ? 1 : 0;
        if (bad && idd >= 0) atomicOr(&sh.status, EKF_FLAG_RANGE_D);  // association: flagged already
      }
    }
    sh.u[tid] = u;
  }
  if (tid == 0) sh.nu_cnt = 3 + 2 * m;
  if (look && tid < kMaxU) {  // the previous chain's mapping of its ids (bad → slot 0)
    const int pm = d.prev_m;
    int u = 0;
    if (tid < 3) {
      u = tid;
    } else if (tid < 3 + 2 * pm) {
      u = column_of_id(d.prev_ids[(tid - 3) >> 1], N, tid);
    }
    sh.pv.u[tid] = u;
    if (tid == 0) {
      sh.pv.nu = 3 + 2 * pm;
      sh.pv.m = pm;
    }
  }
}

// ---- A1, kLook: the rebuild ---------------------------------------------------------------------
// Σ_in[U,U] = Σ_pred'[U,U] − K'·M' with Σ_pred' = A'·Σ_in'·A'ᵀ + Q̄' (the previous chunk's predict,
// if it had one), K'[a] = Σ_pred'[u_a, U']·Z', M'[:, b] = Y'·Σ_pred'[U', u_b]: the factor kernel's
// formulas evaluated at U only.
//
// The operands into LDS. Each thread issues all of its loads before its first LDS store: indices
// are clamped rather than predicated (a predicated load becomes a branch with its own wait), so the
// loads of a thread are in flight together instead of one memory round trip per loop iteration.
// Sp, xp: the previous chunk's Σ_in' and x' of this filter (a chain without a staged image gathers
// from them).
template <typename T, bool J>
__device__ __forceinline__ void land_rebuild_operands(ChainSharedT<J>& sh, ChainLoads<T, J>& L,
                                                      const T* Sp, const double* xp, int ld,
                                                      const ChunkRec* rp, FilterCtl* ctl, int tid,
                                                      int nu, int np, bool early) {
  using CL = ChainLoads<T, J>;
  constexpr int ZC = CL::ZC;
  static_assert(sizeof(sh.im) == 2 * sizeof(RebuildImage<float>) && alignof(decltype(sh.im)) >= 16 &&
                    (kZC * kMaxU) % 2 == 0 && ZC % 2 == 0,
                "the staged image and the record's Z / Y are copied in 16-byte pieces");
  const int tc = tid < kMaxU ? tid : 0;
  if (!early) {  // (early: the staged image and the record's values are in registers)
    load_prev_record(L, buf_rsrc(rp, static_cast<unsigned>(sizeof(ChunkRec))), tid);
    T vd[kRebPer], vr[kRebPer], vc[kRebPer];
#pragma unroll
    for (int i = 0; i < kRebPer; ++i) {
      const int e = tid + i * kChainThreads;
      const int a = min(e / kRebW, kMaxU - 1), b = min(e % kRebW, kMaxU - 1);  // clamped: in bounds
      const size_t ua = static_cast<size_t>(sh.u[a]) * ld, pa = static_cast<size_t>(sh.pv.u[b]);
      vd[i] = Sp[ua + sh.u[b]];
      vr[i] = Sp[ua + pa];
      vc[i] = Sp[pa * ld + sh.u[a]];
    }
    // raw row 0 / column 0 of Σ_in' at U and U' (for the previous predict), x'
    const int uu = sh.u[tc], pu = sh.pv.u[tc];
    L.r0u = static_cast<double>(Sp[uu]);
    L.c0u = static_cast<double>(Sp[static_cast<size_t>(uu) * ld]);
    L.r0p = static_cast<double>(Sp[pu]);
    L.c0p = static_cast<double>(Sp[static_cast<size_t>(pu) * ld]);
    L.x2 = xp[uu];
    L.tq = ctl->tmo[tid < 3 ? tid : 0];
    // the raw gather at the image's positions (what a staged chain's image holds)
    store_raw_image<T>(sh, vd, vr, vc, tid, nu, np);
  } else {
    // the staged image, piece p → piece p of sh.im (fp32: four values widened to two pieces)
    d2m* const im = reinterpret_cast<d2m*>(&sh.im);
#pragma unroll
    for (int i = 0; i < CL::kPerIm; ++i) {
      const int p = tid + i * kChainThreads;
      if (p < CL::kImPieces) {
        if constexpr (sizeof(T) == 8) {
          im[p] = __builtin_bit_cast(d2m, L.vim[i]);
        } else {
          const f4v w = __builtin_bit_cast(f4v, L.vim[i]);
          im[2 * p] = d2m{static_cast<double>(w.x), static_cast<double>(w.y)};
          im[2 * p + 1] = d2m{static_cast<double>(w.z), static_cast<double>(w.w)};
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CL::kPerZ; ++i) {
    const int p = tid + i * kChainThreads;
    const d2m w = __builtin_bit_cast(d2m, L.vz[i]);
    if (p < CL::kZPieces) {
      double* z = &sh.pv.Z[p / CL::kZP][2 * (p % CL::kZP)];
      z[0] = w.x;
      z[1] = w.y;
    }
  }
#pragma unroll
  for (int i = 0; i < CL::kPerY; ++i) {
    const int p = tid + i * kChainThreads, e0 = 2 * p, e1 = 2 * p + 1;
    const d2m w = __builtin_bit_cast(d2m, L.vy[i]);
    if (p < CL::kYPieces) {
      sh.pv.Y[e0 / kMaxU][e0 % kMaxU] = w.x;
      sh.pv.Y[e1 / kMaxU][e1 % kMaxU] = w.y;
    }
  }
  if (tid < ZC) sh.pv.Z[kMaxU][tid] = 0.0;  // the 36th k row / column
  if (tid < kZC) sh.pv.Y[tid][kMaxU] = 0.0;
  if (tid < kMaxU) {
    sh.pv.r0U[tid] = L.r0u;
    sh.pv.c0U[tid] = L.c0u;
    sh.pv.r0P[tid] = L.r0p;
    sh.pv.c0P[tid] = L.c0p;
    sh.pv.xU[tid] = L.x0;
    sh.pv.Zx[tid] = L.x1;
    sh.pv.xg[tid] = L.x2;
  }
  if (tid == 0) {
    sh.pv.first = (L.pflags & kFirst) != 0;
    sh.pv.joseph = (L.pflags & kJoseph) != 0;
    sh.pv.a1 = L.pa1;
    sh.pv.a2 = L.pa2;
  }
  if (tid < 3) sh.tmo[tid] = L.tq;
}

// Where each column of U sits in U' (pv.pos[a]: the first position k with u'_k = u_a; −1: none),
// for x_in[U]. One wave (wave 3, beside the other waves' previous predict: off every barrier's
// path), from the index sets: a landmark column is 3 + 2·slot + (x: 0, y: 1), so lane j < m' takes
// the previous marker j's slot, and a lane's own slot is compared with the 16 of them by
// v_readlane — the columns' comparison (a bad id's columns are slot 0's on both sides).
template <bool J>
__device__ __forceinline__ void map_U_into_prev(ChainSharedT<J>& sh, int ln, int nu) {
  const int pm = sh.pv.m;
  const int pslot = ln < pm ? (sh.pv.u[3 + 2 * min(ln, kMaxChunk - 1)] - 3) >> 1 : -1;
  const int l = min(ln, kMaxU - 1), u = sh.u[l];
  const int slot = (u - 3) >> 1, par = (u - 3) & 1;  // (a marker's; the pose is mapped below)
  int hit = -1;
#pragma unroll
  for (int c = kMaxChunk - 1; c >= 0; --c)
    hit = __builtin_amdgcn_readlane(pslot, c) == slot ? 3 + 2 * c + par : hit;
  // the pose sits at its own position; a padding row's column 0 at position 0 (never stored)
  if (ln < kMaxU) sh.pv.pos[ln] = l < 3 ? l : (l < nu ? hit : 0);
}

// Wave 3's x_in[U] of lane ln's row: the previous chunk's x[U'] where it has it (pv.pos), else
// x' + r'(i)·Zx'. Nothing reads it before the predict fold. Simple form: beside wave 3's K' / M'
// tiles, where it stands in for the band output the other waves have (one dot product each: wave 3
// reaches the barrier before them). Joseph form: in the P phase, whose tiles are waves 0–2's.
template <bool J>
__device__ __forceinline__ double prev_x_at_U(ChainSharedT<J>& sh, int ln) {
  const int l = ln < kMaxU ? ln : kMaxU - 1;
  const int pos = sh.pv.pos[l];
  double bacc[4] = {0.0, 0.0, 0.0, 0.0};
  dot4<kMaxU>(&sh.im.R[l][0], &sh.pv.Zx[0], 1, bacc);
  const double r = sum4(bacc);  // R[·][k ≥ |U'|] = 0
  return pos >= 0 ? sh.pv.xU[pos] : sh.pv.xg[l] + r;
}
template <bool J>
__device__ __forceinline__ void store_x_in(ChainSharedT<J>& sh, int ln, int nu, double xres) {
  // (lanes beyond store to the wave's junk slot: a value used under a branch is computed there)
  *(ln < nu ? &sh.xU[0][ln] : &sh.junk[3][ln]) = xres;
  if (ln < 3) sh.xpose[ln] = sh.pv.xU[ln];  // pose ∈ U' always
}

// A band output of the K' / M' phase as a VALU dot product (16 × 16 tiles there would be 13/16
// padding): bk: K'[brow][bcol] = R[brow]·Z'[:, bcol], else M'[brow][bcol] = Y'[brow]·C[:, bcol].
template <bool J>
__device__ __forceinline__ void km_band_dot(ChainSharedT<J>& sh, bool bk, int brow, int bcol,
                                            double (&bacc)[4]) {
  const double* ra = bk ? &sh.im.R[min(brow, kMaxU - 1)][0] : &sh.pv.Y[brow][0];
  const double* cb = bk ? &sh.pv.Z[0][bcol] : &sh.im.C[0][min(bcol, kMaxU)];
  const int sc = bk ? ChainSharedT<J>::ZC + 1 : kMaxU + 1;
  dot4<kMaxU + 1>(ra, cb, sc, bacc);
}

// K' = R·Z' (35 × 32) and M' = Y'·C (32 × 35) on f64 MFMA, simple form. Their 32 × 32 cores are 8
// tiles, two per wave; the 3-wide bands K'[32..34][·] and M'[·][32..34] are VALU dot products, one
// output per thread of waves 0–2, and wave 3 (W3) forms x_in[U] instead. Operand reads are
// unconditional (clamped rows / columns feed only discarded outputs, k ≥ |U'| is zero-padded in
// both operands, so every k-step runs: its MFMA adds exact zeros). A wave's tiles and its VALU work
// are one basic block (operand reads first, then two interleaved accumulation chains beside the dot
// product): the MFMA and VALU pipes overlap. The stores are unconditional too, through a selected
// address: a store under a branch took the dot product into the branch with it, behind the MFMAs.
template <bool W3>
__device__ __forceinline__ void rebuild_km_simple(ChainSharedT<false>& sh, const ChainLane& L, int nu,
                                                  int np, unsigned seq) {
  (void)seq;  // (diagnostic stamps)
  (void)np;
  const int tid = L.tid, wv = L.wv, i16 = L.i16, k4 = L.k4;
  double av[2][9], bv[2][9];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int tt = wv + 4 * q;  // 0..3 K' tiles, 4..7 M' tiles
    const bool kt = tt < 4;
    const int ti = (kt ? tt : tt - 4) >> 1, tj = (kt ? tt : tt - 4) & 1;
    // A: R[row][k] (K') or Y'[row][k] (M'), k contiguous; B: Z'[k][col] (stride kZC + 1) or
    // C[k][col] (stride kMaxU + 1)
    const double* pa = kt ? &sh.im.R[16 * ti + i16][0] : &sh.pv.Y[16 * ti + i16][0];
    const double* pb = kt ? &sh.pv.Z[0][16 * tj + i16] : &sh.im.C[0][16 * tj + i16];
    const int sb = kt ? kZC + 1 : kMaxU + 1;
#pragma unroll
    for (int s0 = 0; s0 < 9; ++s0) {
      av[q][s0] = pa[4 * s0 + k4];
      bv[q][s0] = pb[(4 * s0 + k4) * sb];
    }
  }
  // the VALU share: a band output (waves 0–2) or x_in[U] (wave 3)
  double bacc[4] = {0.0, 0.0, 0.0, 0.0};
  int brow = 0, bcol = 0;
  bool bk = false;
  double xres = 0.0;
  if (!W3) {
    if (tid < 96) {  // K'[32 + t/32][t%32]
      bk = true;
      brow = 32 + (tid >> 5);
      bcol = tid & 31;
    } else {  // M'[u/3][32 + u%3]
      const int u = tid - 96;
      brow = u / 3;
      bcol = 32 + (u - 3 * (u / 3));
    }
    km_band_dot(sh, bk, brow, bcol, bacc);
  } else {
    xres = prev_x_at_U(sh, L.ln);
  }
  d4 acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
  for (int s0 = 0; s0 < 9; ++s0)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[q] = mfma_f64(av[q][s0], bv[q][s0], acc[q]);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int tt = wv + 4 * q;
    const bool kt = tt < 4;
    const int ti = (kt ? tt : tt - 4) >> 1, tj = (kt ? tt : tt - 4) & 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * ti + k4 + 4 * r, col = 16 * tj + i16;
      *(kt ? &sh.pv.K[row][col] : &sh.pv.M[row][col]) = acc[q][r];
    }
  }
  EKF_STAMPW(30);  // (the wave's tiles stored)
  if (!W3)  // (an M' band column is 32..34 < kMaxU)
    *(bk ? &sh.pv.K[brow][bcol] : &sh.pv.M[brow][bcol]) = sum4(bacc);
  else
    store_x_in(sh, L.ln, nu, xres);
}

// Joseph form (ZC = 64): K' = R·Z' is 35 × 4m' (K' then V' columns), M' = Y'·C is 2m' × 35. Their
// 16 × 16 cores are 12 tiles, three per wave (one after another, each operand read waited for
// once); the bands K'[32..34][·] (192 outputs) and M'[·][32..34] (96) are VALU dot products of
// waves 0–2 (two per thread for the first 96); wave 3 (W3) has its tiles only.
template <bool W3>
__device__ __forceinline__ void rebuild_km_joseph(ChainSharedT<true>& sh, const ChainLane& L, int nu,
                                                  int np, unsigned seq) {
  (void)seq;  // (diagnostic stamps)
  (void)nu;
  (void)np;
  constexpr int ZC = ChainSharedT<true>::ZC;
  const int tid = L.tid, wv = L.wv, i16 = L.i16, k4 = L.k4;
#pragma unroll 1
  for (int q = 0; q < 3; ++q) {
    const int tt = wv + 4 * q;  // 0..7 K' tiles (2 × 4), 8..11 M' tiles (2 × 2)
    const bool kt = tt < 8;
    const int ti = kt ? tt >> 2 : (tt - 8) >> 1, tj = kt ? tt & 3 : (tt - 8) & 1;
    const double* pa = kt ? &sh.im.R[16 * ti + i16][0] : &sh.pv.Y[16 * ti + i16][0];
    const double* pb = kt ? &sh.pv.Z[0][16 * tj + i16] : &sh.im.C[0][16 * tj + i16];
    const int sb = kt ? ZC + 1 : kMaxU + 1;
    double av[9], bv[9];
#pragma unroll
    for (int s0 = 0; s0 < 9; ++s0) {
      av[s0] = pa[4 * s0 + k4];
      bv[s0] = pb[(4 * s0 + k4) * sb];
    }
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s0 = 0; s0 < 9; ++s0) acc = mfma_f64(av[s0], bv[s0], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // (a selected address, not a branch: rebuild_km_simple)
      const int row = 16 * ti + k4 + 4 * r, col = 16 * tj + i16;
      *(kt ? &sh.pv.K[row][col] : &sh.pv.M[row][col]) = acc[r];
    }
  }
  EKF_STAMPW(30);  // (the wave's tiles stored)
  if (!W3) {
#pragma unroll 1
    for (int t = tid; t < 288; t += 192) {
      const bool bk = t < 192;  // K'[32 + t/64][t%64], else M'[u/3][32 + u%3]
      const int u = t - 192;
      const int brow = bk ? 32 + (t >> 6) : u / 3, bcol = bk ? (t & 63) : 32 + u % 3;
      double bacc[4] = {0.0, 0.0, 0.0, 0.0};
      km_band_dot(sh, bk, brow, bcol, bacc);
      // (stored under a branch, unlike the tiles: without it this loop's reads were issued one
      // by one, each waited for before its FMA)
      const double v = sum4(bacc);
      if (bk) sh.pv.K[brow][bcol] = v;
      else if (bcol < kMaxU) sh.pv.M[brow][bcol] = v;
    }
  }
}

// P = D − K'·M' on the 48×48 padded block, simple form: 9 tiles over the 4 waves (K' columns and
// M' rows ≥ 2m' are zero because Z' / Y' are, so every k-step runs: their MFMAs add exact zeros).
// The 32 × 32 core of P on MFMA, one 16 × 16 tile per wave; the 3-wide bands (rows 32..34 and
// columns 32..34, 201 entries) as VALU dot products, one per thread, in the same basic block.
// Entries outside the block go to the wave's junk slot (a selected address: rebuild_km_simple).
__device__ __forceinline__ void rebuild_p_simple(ChainSharedT<false>& sh, const ChainLane& L,
                                                 int nu, unsigned seq) {
  (void)seq;  // (diagnostic stamps)
  auto& P = sh.im.D;
  const int tid = L.tid, wv = L.wv, i16 = L.i16, k4 = L.k4;
  const int ti = wv >> 1, tj = wv & 1;
  const int col = 16 * tj + i16, ar = 16 * ti + i16;
  double av[8], bv[8];
#pragma unroll
  for (int s0 = 0; s0 < 8; ++s0) {
    av[s0] = -sh.pv.K[ar][4 * s0 + k4];
    bv[s0] = sh.pv.M[4 * s0 + k4][col];
  }
  d4 acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = P[16 * ti + k4 + 4 * r][col];
  // band entry: t < 105 → rows 32..34 × columns 0..34, then rows 0..31 × columns 32..34
  const int t = tid < 201 ? tid : 200;
  const int brow = t < 105 ? 32 + t / 35 : (t - 105) / 3;
  const int bcol = t < 105 ? t - 35 * (t / 35) : 32 + (t - 105) - 3 * ((t - 105) / 3);
  const int br = min(brow, kMaxU - 1), bc = min(bcol, kMaxU - 1);
  double bs[4] = {0.0, 0.0, 0.0, 0.0};
  dot4<kZC>(&sh.pv.K[br][0], &sh.pv.M[0][bc], kMaxU + 1, bs);
  const double bv0 = P[br][bc];
#pragma unroll
  for (int s0 = 0; s0 < 8; ++s0) acc = mfma_f64(av[s0], bv[s0], acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * ti + k4 + 4 * r;
    *(row < nu && col < nu ? &P[row][col] : &sh.junk[wv][L.ln]) = acc[r];
  }
  EKF_STAMPW(34);  // (the wave's tile stored)
  *(tid < 201 && brow < nu && bcol < nu ? &P[brow][bcol] : &sh.junk[wv][L.ln]) = bv0 - sum4(bs);
}

// P = D − K'·M'full with M'full = [M' (rows 0..31); K'[:, 0..32)ᵀ (rows 32..63: a Joseph chunk
// before, its V'·K'ᵀ terms, V' = K' columns 32..63)] — zero beyond each part's rank 2m', and the
// K'ᵀ part zero after a simple-form chunk (its record's columns ≥ 32 are not V'). The 48 × 48 padded
// block as 9 tiles on f64 MFMA, k < 64 in 16 k-steps: waves 0–2 one row tile each (its K' rows read
// once) × the three column tiles, interleaved. Rows / columns ≥ kMaxU are clamped on read and never
// stored; a wave reads and writes only its own rows.
__device__ __forceinline__ void rebuild_p_joseph(ChainSharedT<true>& sh, const ChainLane& L,
                                                 int nu, unsigned seq) {
  (void)seq;  // (diagnostic stamps)
  auto& P = sh.im.D;
  const int wv = L.wv, i16 = L.i16, k4 = L.k4;
  if (wv < 3) {
    const bool pj = sh.pv.joseph != 0;
    const int ar = min(16 * wv + i16, kMaxU - 1);
    double av[16];
#pragma unroll
    for (int s0 = 0; s0 < 16; ++s0) av[s0] = -sh.pv.K[ar][4 * s0 + k4];
    d4 acc[3];
#pragma unroll
    for (int tj = 0; tj < 3; ++tj) {
      const int bc = min(16 * tj + i16, kMaxU - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[tj][r] = P[min(16 * wv + k4 + 4 * r, kMaxU - 1)][bc];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // k < 32 (M' rows), then k ≥ 32 (K'ᵀ)
      double bv[3][8];
#pragma unroll
      for (int tj = 0; tj < 3; ++tj) {
        const int bc = min(16 * tj + i16, kMaxU - 1);
#pragma unroll
        for (int s0 = 0; s0 < 8; ++s0)
          bv[tj][s0] = h == 0 ? sh.pv.M[4 * s0 + k4][bc] : (pj ? sh.pv.K[bc][4 * s0 + k4] : 0.0);
      }
#pragma unroll
      for (int s0 = 0; s0 < 8; ++s0)
#pragma unroll
        for (int tj = 0; tj < 3; ++tj) acc[tj] = mfma_f64(av[8 * h + s0], bv[tj][s0], acc[tj]);
    }
#pragma unroll
    for (int tj = 0; tj < 3; ++tj) {
      const int col = 16 * tj + i16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wv + k4 + 4 * r;
        *(row < nu && col < nu ? &P[row][col] : &sh.junk[wv][L.ln]) = acc[tj][r];
      }
    }
  }
  else {  // wave 3 has no tile: x_in[U]
    store_x_in(sh, L.ln, nu, prev_x_at_U(sh, L.ln));
  }
  EKF_STAMPW(34);  // (the wave's tiles stored)
}

// The predicted pose (slam.cpp:184-196) of a rebuilding chunk, from x' of the pose: one lane of
// wave 2, beside the other waves' P tiles.
template <bool J>
__device__ __forceinline__ void pick_predicted_pose(ChainSharedT<J>& sh, const MsgDesc& d, int ci) {
  if (sh.npose_ci == ci) {  // computed ahead by the chunk before (chain_wave3)
    sh.pose[0] = sh.npose[0];
    sh.pose[1] = sh.npose[1];
    sh.pose[2] = sh.npose[2];
    sh.a1 = sh.na1;
    sh.a2 = sh.na2;
  } else {
    double a1, a2;
    const double xp[3] = {sh.pv.xU[0], sh.pv.xU[1], sh.pv.xU[2]};
    predicted_pose(sh.tmo, d, xp, sh.pose, &a1, &a2);
    sh.a1 = a1;
    sh.a2 = a2;
  }
}

// The rebuild's phases in order: operands, the previous predict (and the map of U into U'), K' / M',
// P, the predicted pose.
template <typename T, bool J>
__device__ __forceinline__ void rebuild_block(ChainSharedT<J>& sh, const MsgDesc& d,
                                              ChainLoads<T, J>& loads, const T* Sp, const double* xp,
                                              int ld, const ChunkRec* rp, FilterCtl* ctl,
                                              const ChainLane& L, int nu, bool early, double q, int ci,
                                              unsigned seq) {
  (void)seq;  // (diagnostic stamps)
  const int np = sh.pv.nu;
  land_rebuild_operands(sh, loads, Sp, xp, ld, rp, ctl, L.tid, nu, np, early);
  __syncthreads();
  EKF_STAMP(21);
  // (wave 3's threads have no special entry: the map instead, not before)
  if (L.wv == 3)
    map_U_into_prev(sh, L.ln, nu);
  else
    predict_prev(sh, L.tid, nu, np, q);
  __syncthreads();

  EKF_STAMP(3);
  EKF_STAMP(4);
  if constexpr (!J)
    L.wv == 3 ? rebuild_km_simple<true>(sh, L, nu, np, seq)
              : rebuild_km_simple<false>(sh, L, nu, np, seq);
  else
    L.wv == 3 ? rebuild_km_joseph<true>(sh, L, nu, np, seq)
              : rebuild_km_joseph<false>(sh, L, nu, np, seq);
  EKF_STAMP(7);
  EKF_STAMPW(22);  // (each wave's end of the K' / M' phase)
  __syncthreads();
  EKF_STAMP(5);
  if constexpr (!J)
    rebuild_p_simple(sh, L, nu, seq);
  else
    rebuild_p_joseph(sh, L, nu, seq);
  EKF_STAMPW(26);  // (each wave's end of the P phase)
  EKF_STAMPT(10, 64);
  EKF_STAMPT(11, 128);
  EKF_STAMPT(13, 192);
  if (L.wv == 2 && L.ln == 0) {
    pick_predicted_pose(sh, d, ci);
    EKF_STAMPT(8, 128);
  }
  EKF_STAMPT(9, 192);  // (wave 3's end; its x_in[U]: K' / M' phase, Joseph form P phase)
}

// ---- A1, gathering: Σ_in[U, U], x[U] and the predicted pose from this chunk's own Σ_in / x ---------
// (every global load before the first LDS store, as in land_rebuild_operands)
template <typename T, bool J>
__device__ __forceinline__ void gather_block(ChainSharedT<J>& sh, const MsgDesc& d, const T* S,
                                             const double* xin, int ld, FilterCtl* ctl, int tid,
                                             int nu) {
  auto& P = sh.im.D;
  double vd[kRebPer];
#pragma unroll
  for (int i = 0; i < kRebPer; ++i) {
    const int e = tid + i * kChainThreads;
    const int a = min(e / kRebW, kMaxU - 1), b = min(e % kRebW, kMaxU - 1);
    vd[i] = static_cast<double>(S[static_cast<size_t>(sh.u[a]) * ld + sh.u[b]]);
  }
  const double xv = xin[sh.u[tid < nu ? tid : 0]];
  const double xq = xin[tid < 3 ? tid : 0];
  const double tq = ctl->tmo[tid < 3 ? tid : 0];
#pragma unroll
  for (int i = 0; i < kRebPer; ++i) {
    const int e = tid + i * kChainThreads;
    const int a = e / kRebW, b = e % kRebW;
    if (a < nu && b < nu) P[a][b] = vd[i];
  }
  if (tid < nu) sh.xU[0][tid] = xv;
  if (tid < 3) {
    sh.xpose[tid] = xq;
    sh.tmo[tid] = tq;
  }
  __syncthreads();
  if (tid == 192) {
    double a1, a2;
    predicted_pose(sh.tmo, d, sh.xpose, sh.pose, &a1, &a2);
    sh.a1 = a1;
    sh.a2 = a2;
  }
}

// ---- A3: x[U] pose, α, this chunk's predict folded in: P ← A P Aᵀ + Q̄ (slam.cpp:198) -----------
// α, row 0, column 0 to LDS for the record; the predict (slam.cpp:198) changes only the special
// entries (rows / columns 1, 2 and the pose diagonal, special_entry): one per thread, its raw
// value, row 0 and column 0 read before any is written.
template <bool J>
__device__ __forceinline__ void fold_predict(ChainSharedT<J>& sh, int tid, int nu, bool first,
                                             double q) {
  auto& P = sh.im.D;
  const double a1 = sh.a1, a2 = sh.a2, s00 = P[0][0];
  if (tid < nu) {
    if (tid < 3) sh.xU[0][tid] = sh.pose[tid];
    sh.alphaU[tid] = first ? alpha_of(sh.u[tid], a1, a2) : 0.0;
    sh.row0raw[tid] = P[0][tid];
    sh.col0raw[tid] = P[tid][0];
  }
  if (tid == 0) sh.s00 = s00;
  if (first) {
    int a, b;
    special_entry(min(tid, kSpec - 1), a, b);
    const bool ok = tid < kSpec && a < nu && b < nu;
    a = min(a, kMaxU - 1);
    b = min(b, kMaxU - 1);
    const double pr = P[a][b], r0 = P[0][b], c0 = P[a][0];
    lds_barrier();  // every raw read done before the first write
    const double ai = alpha_of(a, a1, a2), aj = alpha_of(b, a1, a2);
    double v = pr + ai * r0;
    v = v + (c0 + ai * s00) * aj;
    v = (a == b && a < 3) ? v + q : v;
    if (ok) P[a][b] = v;
  }
}

// ---- A2: the wave programs beside chain_wave0 (see k_chain) -------------------------------------
// What waves 1 and 2 share: a published factor (K, M or V of step k) at the step's five positions
// pA = {0, 1, 2, pj, pj+1}, the 2×2 product over pA that a history term needs, and the row of a
// 5×2 matrix that position `l` of U selects (zero off pA).
__device__ __forceinline__ void read_pA(const double (*fac)[2], int pj, double (&f0)[5],
                                        double (&f1)[5]) {
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const int pa = a < 3 ? a : pj + a - 3;
    f0[a] = fac[pa][0];
    f1[a] = fac[pa][1];
  }
}
// out (row-major 2×2) = Σ_a (x0[a], x1[a])ᵀ·(y0[a], y1[a])
__device__ __forceinline__ void prod_pA(const double (&x0)[5], const double (&x1)[5],
                                        const double (&y0)[5], const double (&y1)[5], double* out) {
  double c00 = 0.0, c01 = 0.0, c10 = 0.0, c11 = 0.0;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    c00 = fma(x0[a], y0[a], c00);
    c01 = fma(x0[a], y1[a], c01);
    c10 = fma(x1[a], y0[a], c10);
    c11 = fma(x1[a], y1[a], c11);
  }
  out[0] = c00;
  out[1] = c01;
  out[2] = c10;
  out[3] = c11;
}
__device__ __forceinline__ void select_pA(int l, int pj, const double (&g0)[5], const double (&g1)[5],
                                          double& r0, double& r1) {
  const int pos = l < 3 ? l : (l == pj ? 3 : (l == pj + 1 ? 4 : -1));
  r0 = r1 = 0.0;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    r0 = pos == a ? g0[a] : r0;
    r1 = pos == a ? g1[a] : r1;
  }
}

// Wave 3: P outside the cross (rows and columns ∉ the next marker's Bx), then the posterior
// t_map_odom and the next chunk's predicted pose.
// lane → column 3+(lane&31), rows 3.. of parity lane>>5. The lane's 16 entries stay in registers
// for the whole chunk: every step's rank-2 term is applied to all of them — also to those in the
// next marker's cross, which wave 0 updates (and stores) itself with the same operands in the same
// order, so the register copy keeps the block's bits — and only the entries outside that cross are
// stored (what wave 0 reads ahead, and the block's final state).
// A: the launch's arguments, for the next chunk's descriptor (chunk ci + 1 of nchunks, read in HBM
// under the test that there is one) and A.gather.
template <typename T, bool J>
__device__ __forceinline__ void chain_wave3(ChainSharedT<J>& sh, const MsgDesc& d,
                                            const PassArgs<T>& A, FilterCtl* ctl, int fy, int m,
                                            int nu, int lane, int ci, int nchunks, unsigned seq) {
  (void)seq;  // (diagnostic stamps)
  constexpr int JM = ChainSharedT<J>::JM;
  auto& P = sh.im.D;
  const int hb = lane & 31, hr = lane >> 5;
  const int b = min(3 + hb, kMaxU - 1);
  {  // (Joseph: V_c[a]·K_c[b] after the K·M term, as wave 0 does)
    double pv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) pv[i] = P[min(3 + hr + 2 * i, kMaxU - 1)][b];  // clamped rows
    for (int c = 0; c + 1 < m; ++c) {
      lds_wait_ge(&sh.pub, c + 1);
      EKF_STAMPT(192 + 2 * c, 192);
      const int nx = 5 + 2 * c, cj = min(c, JM - 1);
      const bool colok = 3 + hb < nu && b != nx && b != nx + 1;
      const double mb0 = sh.MU[c][b][0], mb1 = sh.MU[c][b][1];
      const double kb0 = J ? sh.KU[c][b][0] : 0.0, kb1 = J ? sh.KU[c][b][1] : 0.0;
      double k0[16], k1[16], w0[16], w1[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {  // clamped rows: unconditional reads, no per-row wait
        const int a = min(3 + hr + 2 * i, kMaxU - 1);
        k0[i] = sh.KU[c][a][0];
        k1[i] = sh.KU[c][a][1];
        if (J) {
          w0[i] = sh.VU[cj][a][0];
          w1[i] = sh.VU[cj][a][1];
        }
      }
      // every lane stores every row (masked-off entries to its junk slot): no divergent
      // branches, so the reads above are waited for once, not once per predicated store
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int a = 3 + hr + 2 * i;
        const bool ok = colok && a < nu && a != nx && a != nx + 1;
        double v = rank2_sub(pv[i], k0[i], k1[i], mb0, mb1);
        if (J) v = rank2_sub(v, w0[i], w1[i], kb0, kb1);
        pv[i] = v;
        *(ok ? &P[a][b] : &sh.junk[3][lane]) = v;
      }
      lds_publish(&sh.pdone, c + 1);
      EKF_STAMPT(193 + 2 * c, 192);
    }
  }
  // The posterior t_map_odom = T(x, y, θ)·t_odom_robot⁻¹ (slam.cpp:273-277) as soon as wave 0 has
  // published the last step (its x is stored before that), beside waves 1–2's last Z / Y and off
  // the epilogue (a pose composition's sin / cos on one lane)
  if (lane == 0 && (d.flags & kLast)) {
    lds_wait_ge(&sh.pub, m);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const Pose2 tmo = compose(Pose2{sh.xU[0][0], sh.xU[0][1], sh.xU[0][2]},
                              inverse(Pose2{d.odom[0], d.odom[1], d.odom[2]}));
    ctl->tmo[0] = tmo.theta;
    ctl->tmo[1] = tmo.x;
    ctl->tmo[2] = tmo.y;
    sh.tmo[0] = tmo.theta;
    sh.tmo[1] = tmo.x;
    sh.tmo[2] = tmo.y;
    if (A.trace) {  // the pose trace's record, behind the t_map_odom store (count: k_chain, step 4)
      const long long n = trace_append(A, A.f0 + fy, sh.trace_n, sh.xU[0][0], sh.xU[0][1],
                                       sh.xU[0][2], tmo.theta, tmo.x, tmo.y);
      sh.trace_n = n;
      A.trace_n[A.f0 + fy] = n;
    }
  }
  // ... and the next chunk's predicted pose (slam.cpp:184-196), beside waves 1–2's last Z / Y
  // instead of in its prologue: its inputs are this chunk's final pose (the record's x[U] there,
  // which the next chunk would read), the t_map_odom after this chunk (the word it would load)
  // and its descriptor's odometry — the same values, so the same bits
  if (lane == 0 && ci + 1 < nchunks) {
    const MsgDesc& nd = A.desc[static_cast<size_t>(ci + 1) * A.desc_stride + fy];
    const int nfl = nd.flags;
    const double od[3] = {nd.odom[0], nd.odom[1], nd.odom[2]};
    if ((nfl & kActive) && (nfl & kLook) && !A.gather) {
      lds_wait_ge(&sh.pub, m);
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      const double xp[3] = {sh.xU[0][0], sh.xU[0][1], sh.xU[0][2]};
      const double tm[3] = {sh.tmo[0], sh.tmo[1], sh.tmo[2]};
      double np_[3], a1, a2;
      predicted_pose(tm, nfl, od, xp, np_, &a1, &a2);
      sh.npose[0] = np_[0];
      sh.npose[1] = np_[1];
      sh.npose[2] = np_[2];
      sh.na1 = a1;
      sh.na2 = a2;
      sh.npose_ci = ci + 1;
    }
  }
}

// Wave 1's steps, simple form: lane k forms C_k, lane i its row of Z_c. Returns Σ_c Z_c ν_c of row
// `lane`, accumulated as the Z_c come (the record's Zx).
__device__ __forceinline__ double wave1_steps_simple(ChainSharedT<false>& sh,
                                                     __amdgpu_buffer_rsrc_t rr, int m, int nu,
                                                     int lane, unsigned seq) {
  (void)seq;  // (diagnostic stamps)
  constexpr int oZ = static_cast<int>(offsetof(ChunkRec, Z));
  const int li = lane < kMaxU ? lane : kMaxU - 1;
  double zxa = 0.0;
  for (int c = 0; c < m; ++c) {
    lds_wait_ge(&sh.pub, c + 1);
    const int pj = 3 + 2 * c;
    double H0[5], H1[5], Si[4], G0[5], G1[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      H0[a] = sh.Hs[c][0][a];
      H1[a] = sh.Hs[c][1][a];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) Si[k] = sh.Sis[c][k];
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      G0[a] = H0[a] * Si[0] + H1[a] * Si[2];
      G1[a] = H0[a] * Si[1] + H1[a] * Si[3];
    }
    {  // lane k < c: C_k (lanes ≥ c store to a junk slot: no divergent branch)
      double m0[5], m1[5];
      read_pA(sh.MU[lane < c ? lane : 0], pj, m0, m1);
      prod_pA(m0, m1, G0, G1, lane < c ? &sh.Cz[lane][0] : &sh.junk[1][0]);
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);  // (one wave: LDS keeps its order)
    {  // row li of Z_c
      double z0, z1;
      select_pA(li, pj, G0, G1, z0, z1);
      // the history in groups of 4 terms: a group's 12 LDS reads are issued together and
      // waited for once (one term per read-wait-FMA round trip was ≈ 135 cycles)
      int k = 0;
      for (; k + 4 <= c; k += 4) {
        double zz[4][2], cz[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          zz[q][0] = sh.Z[li][2 * (k + q)];
          zz[q][1] = sh.Z[li][2 * (k + q) + 1];
#pragma unroll
          for (int e = 0; e < 4; ++e) cz[q][e] = sh.Cz[k + q][e];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          z0 = fma(-zz[q][1], cz[q][2], fma(-zz[q][0], cz[q][0], z0));
          z1 = fma(-zz[q][1], cz[q][3], fma(-zz[q][0], cz[q][1], z1));
        }
      }
      for (; k < c; ++k) {
        const double zk0 = sh.Z[li][2 * k], zk1 = sh.Z[li][2 * k + 1];
        const double c00 = sh.Cz[k][0], c01 = sh.Cz[k][1], c10 = sh.Cz[k][2], c11 = sh.Cz[k][3];
        z0 = fma(-zk1, c10, fma(-zk0, c00, z0));
        z1 = fma(-zk1, c11, fma(-zk0, c01, z1));
      }
      const bool in = lane < nu;
      const double Z0 = in ? z0 : 0.0, Z1 = in ? z1 : 0.0;
      const double t = Z0 * sh.nu[c][0] + Z1 * sh.nu[c][1];
      zxa += t;
      if (lane < kMaxU) {
        sh.Z[lane][2 * c] = Z0;
        sh.Z[lane][2 * c + 1] = Z1;
        st_wt2(rr, oZ + 8 * (kZJ * lane + 2 * c), Z0, Z1);
      }
    }
    EKF_STAMPT(320 + c, 64);
  }
  return zxa;
}

// Wave 1's steps, Joseph form: Σ_c[i, U] = r_0(i)·Φ_c with Φ_{c+1} = Φ_c − Z_c·M_c[:, U] −
// Zv_c·K_c[U]ᵀ, so W_c = Φ_c[:, pA]·Hᵀ = E_c·Hᵀ − Σ_{k<c} (Z_k·C_k + Zv_k·C'_k), C_k = M_k[:, pA_c]·Hᵀ
// and C'_k = K_k[pA_c]ᵀ·Hᵀ (2×2 each); then Z_c = W_c·S_c⁻¹ (K_c = G_c·S⁻¹, G_c[i] = r_0(i)·W_c) and
// Zv_c = W_c − Z_c·S_c (V_c = G_c − K_c·S_c). One marker: Z_0 = E·Hᵀ·S⁻¹, as the simple form.
__device__ __forceinline__ double wave1_steps_joseph(ChainSharedT<true>& sh,
                                                     __amdgpu_buffer_rsrc_t rr, int m, int nu,
                                                     int lane, unsigned seq) {
  (void)seq;  // (diagnostic stamps)
  constexpr int oZ = static_cast<int>(offsetof(ChunkRec, Z));
  constexpr int cols = kZC;  // V_c in columns 32 + 2c.. (fixed: the rebuild's K'ᵀ rows start at 32)
  const int li = lane < kMaxU ? lane : kMaxU - 1;
  double zxa = 0.0;
  for (int c = 0; c < m && c < kMaxJoseph; ++c) {
    lds_wait_ge(&sh.pub, c + 1);
    EKF_STAMPT(460 + c, 64);
    const int pj = 3 + 2 * c;
    double H0[5], H1[5], Si[4], Sc[4];
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      H0[a] = sh.Hs[c][0][a];
      H1[a] = sh.Hs[c][1][a];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      Si[k] = sh.Sis[c][k];
      Sc[k] = sh.Ss[c][k];
    }
    {  // lane k < c: C_k and C'_k
      const int k = lane < c ? lane : 0;
      double m0[5], m1[5], q0[5], q1[5];
      read_pA(sh.MU[k], pj, m0, m1);
      read_pA(sh.KU[k], pj, q0, q1);
      prod_pA(m0, m1, H0, H1, lane < c ? &sh.Cz[lane][0] : &sh.junk[1][0]);
      prod_pA(q0, q1, H0, H1, lane < c ? &sh.Cv[lane][0] : &sh.junk[1][4]);
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);  // (one wave: LDS keeps its order)
    EKF_STAMPT(480 + c, 64);
    {  // row li of W_c, then of Z_c and Zv_c
      double w0, w1;
      select_pA(li, pj, H0, H1, w0, w1);
      // the history in groups of 4 terms, each group's 24 LDS reads issued together (one
      // read-wait round trip per term made this wave the chunk's last, ≈ 200 cycles a term)
      auto jterm = [&](const double* zz, const double* cz) {
        w0 = fma(-zz[1], cz[2], fma(-zz[0], cz[0], w0));
        w1 = fma(-zz[1], cz[3], fma(-zz[0], cz[1], w1));
        w0 = fma(-zz[3], cz[6], fma(-zz[2], cz[4], w0));
        w1 = fma(-zz[3], cz[7], fma(-zz[2], cz[5], w1));
      };
      int k = 0;
      for (; k + 4 <= c; k += 4) {
        double zz[4][4], cz[4][8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          zz[q][0] = sh.Z[li][2 * (k + q)];
          zz[q][1] = sh.Z[li][2 * (k + q) + 1];
          zz[q][2] = sh.Z[li][cols + 2 * (k + q)];
          zz[q][3] = sh.Z[li][cols + 2 * (k + q) + 1];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            cz[q][e] = sh.Cz[k + q][e];
            cz[q][4 + e] = sh.Cv[k + q][e];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 4; ++q) jterm(zz[q], cz[q]);
      }
      for (; k < c; ++k) {
        double zz[4], cz[8];
        zz[0] = sh.Z[li][2 * k];
        zz[1] = sh.Z[li][2 * k + 1];
        zz[2] = sh.Z[li][cols + 2 * k];
        zz[3] = sh.Z[li][cols + 2 * k + 1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          cz[e] = sh.Cz[k][e];
          cz[4 + e] = sh.Cv[k][e];
        }
        jterm(zz, cz);
      }
      const bool in = lane < nu;
      const double Z0 = in ? w0 * Si[0] + w1 * Si[2] : 0.0;
      const double Z1 = in ? w0 * Si[1] + w1 * Si[3] : 0.0;
      const double V0 = in ? w0 - (Z0 * Sc[0] + Z1 * Sc[2]) : 0.0;
      const double V1 = in ? w1 - (Z0 * Sc[1] + Z1 * Sc[3]) : 0.0;
      zxa += Z0 * sh.nu[c][0] + Z1 * sh.nu[c][1];
      if (lane < kMaxU) {
        sh.Z[lane][2 * c] = Z0;
        sh.Z[lane][2 * c + 1] = Z1;
        sh.Z[lane][cols + 2 * c] = V0;
        sh.Z[lane][cols + 2 * c + 1] = V1;
        st_wt2(rr, oZ + 8 * (kZJ * lane + 2 * c), Z0, Z1);
        st_wt2(rr, oZ + 8 * (kZJ * lane + cols + 2 * c), V0, V1);
      }
    }
    lds_publish(&sh.zdone, c + 1);  // (wave 2 reads Z_c, Zv_c)
    EKF_STAMPT(320 + c, 64);
  }
  return zxa;
}

// Wave 1: Z_c, K_c[i] = r_0(i)·Z_c for every row i.
// Σ_c[i, pA_c] = r_0(i)·(E_c − Σ_{k<c} Z_k·M_k[:, pA_c]) (E_c selects the positions pA_c), so
// Z_c = E_c·G − Σ_{k<c} Z_k·C_k with G = Hᵀ·S⁻¹ (5×2) and C_k = M_k[:, pA_c]·G (2×2): lane k
// forms C_k, lane i its row of Z_c — 4c FMAs a row instead of a |U|×|U| row map updated per
// step. The record parity this chunk writes was last written two chunks back: the prologue's
// poll (that chunk's Σ-pass epoch) has made the bulk stream done with it. Z_c goes to the
// record as soon as it is computed (write-through, off the chain's path).
template <bool J>
__device__ __forceinline__ void chain_wave1(ChainSharedT<J>& sh, ChunkRec* rec, int m, int nu,
                                            int lane, unsigned seq) {
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc(rec, 0, static_cast<int>(sizeof(ChunkRec)), 0x00020000);
  {  // columns ≥ 2m of the record's Z are zero (the factor kernel and a rebuilding chain read
     // them); Joseph: columns 2m..32 and 32 + 2m..64 (V in 32..32 + 2m)
    const int zw = kZC - 2 * m, nz = J ? 2 : 1;
    for (int e = lane; e < kMaxU * zw * nz; e += 64) {
      const int h = e >= kMaxU * zw ? 1 : 0, e2 = e - h * kMaxU * zw;
      const int b = e2 / zw, k = 2 * m + (e2 - b * zw) + kZC * h;
      st_wt(&rec->Z[b][k], 0.0);
    }
  }
  double zxa;
  if constexpr (!J)
    zxa = wave1_steps_simple(sh, rr, m, nu, lane, seq);
  else
    zxa = wave1_steps_joseph(sh, rr, m, nu, lane, seq);
  if (lane < kMaxU) sh.Zx[lane] = zxa;
}

// Wave 2: Y_c, M_c[:, j] = Y_c·c_0(j) for every column j; Y_c to the record at once.
// Σ_c[pA_c, j] = (E_cᵀ − Σ_{k<c} K_k[pA_c]·Y_k)·c_0(j), so Y_c = H·E_cᵀ − Σ_{k<c} D_k·Y_k with
// D_k = H·K_k[pA_c] (2×2): lane k forms D_k, lane j its column of Y_c.
// Joseph: Σ_{c+1}[·, j] also loses V_c·K_c[j]ᵀ, and K_c[j] = r_0(j)·Z_c = Z_cᵀ·c_0(j) (Σ_pred is
// symmetric in exact arithmetic; fp64 Σ exactly): Y_c = H·E_cᵀ − Σ_{k<c} (D_k·Y_k + D'_k·Z_kᵀ),
// D'_k = H·V_k[pA_c], with wave 1's Z_k (flag zdone).
template <bool J>
__device__ __forceinline__ void chain_wave2(ChainSharedT<J>& sh, ChunkRec* rec, int m, int nu,
                                            int lane, bool joseph, unsigned seq) {
  (void)seq;  // (diagnostic stamps)
  constexpr int JM = ChainSharedT<J>::JM;
  for (int e = lane; e < (kZC - 2 * m) * kMaxU; e += 64)  // rows ≥ 2m of the record's Y are zero
    st_wt(&(&rec->Y[2 * m][0])[e], 0.0);
  const int lj = lane < kMaxU ? lane : kMaxU - 1;
  for (int c = 0; c < m; ++c) {
    lds_wait_ge(&sh.pub, c + 1);
    EKF_STAMPT(400 + c, 128);
    if (joseph && c > 0) lds_wait_ge(&sh.zdone, min(c, kMaxJoseph));
    EKF_STAMPT(420 + c, 128);
    const int pj = 3 + 2 * c;
    double H0[5], H1[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      H0[a] = sh.Hs[c][0][a];
      H1[a] = sh.Hs[c][1][a];
    }
    {  // lane k < c: D_k (Joseph: and D'_k)
      const int k = lane < c ? lane : 0;
      double k0[5], k1[5];
      read_pA(sh.KU[k], pj, k0, k1);
      prod_pA(H0, H1, k0, k1, lane < c ? &sh.Dy[lane][0] : &sh.junk[2][0]);
      if (joseph) {
        const int kj = min(k, JM - 1);
        double v0[5], v1[5];
        read_pA(sh.VU[kj], pj, v0, v1);
        prod_pA(H0, H1, v0, v1, lane < c ? &sh.Dv[kj][0] : &sh.junk[2][4]);
      }
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    EKF_STAMPT(440 + c, 128);
    {  // column lj of Y_c
      double y0, y1;
      select_pA(lj, pj, H0, H1, y0, y1);
      int k0 = 0;
      if (joseph) {  // (uniform) groups of 4 terms with D'_k·Z_kᵀ, reads issued together
        for (; k0 + 4 <= c; k0 += 4) {
          double yy[4][4], dy[4][8];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int kj = min(k0 + q, JM - 1);
            yy[q][0] = sh.Y[2 * (k0 + q)][lj];
            yy[q][1] = sh.Y[2 * (k0 + q) + 1][lj];
            yy[q][2] = sh.Z[lj][2 * (k0 + q)];
            yy[q][3] = sh.Z[lj][2 * (k0 + q) + 1];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              dy[q][e] = sh.Dy[k0 + q][e];
              dy[q][4 + e] = sh.Dv[kj][e];
            }
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            y0 = fma(-dy[q][1], yy[q][1], fma(-dy[q][0], yy[q][0], y0));
            y1 = fma(-dy[q][3], yy[q][1], fma(-dy[q][2], yy[q][0], y1));
            y0 = fma(-dy[q][5], yy[q][3], fma(-dy[q][4], yy[q][2], y0));
            y1 = fma(-dy[q][7], yy[q][3], fma(-dy[q][6], yy[q][2], y1));
          }
        }
      } else {  // (uniform) groups of 4 terms, reads issued together (as wave 1's Z)
        for (; k0 + 4 <= c; k0 += 4) {
          double yy[4][2], dy[4][4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            yy[q][0] = sh.Y[2 * (k0 + q)][lj];
            yy[q][1] = sh.Y[2 * (k0 + q) + 1][lj];
#pragma unroll
            for (int e = 0; e < 4; ++e) dy[q][e] = sh.Dy[k0 + q][e];
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            y0 = fma(-dy[q][1], yy[q][1], fma(-dy[q][0], yy[q][0], y0));
            y1 = fma(-dy[q][3], yy[q][1], fma(-dy[q][2], yy[q][0], y1));
          }
        }
      }
#pragma unroll 4
      for (int k = k0; k < c; ++k) {
        const double yk0 = sh.Y[2 * k][lj], yk1 = sh.Y[2 * k + 1][lj];
        const double d00 = sh.Dy[k][0], d01 = sh.Dy[k][1], d10 = sh.Dy[k][2], d11 = sh.Dy[k][3];
        y0 = fma(-d01, yk1, fma(-d00, yk0, y0));
        y1 = fma(-d11, yk1, fma(-d10, yk0, y1));
        if (joseph) {
          const int kj = min(k, JM - 1);
          const double zk0 = sh.Z[lj][2 * k], zk1 = sh.Z[lj][2 * k + 1];
          const double e00 = sh.Dv[kj][0], e01 = sh.Dv[kj][1], e10 = sh.Dv[kj][2], e11 = sh.Dv[kj][3];
          y0 = fma(-e01, zk1, fma(-e00, zk0, y0));
          y1 = fma(-e11, zk1, fma(-e10, zk0, y1));
        }
      }
      if (lane < kMaxU) {
        const bool in = lane < nu;
        sh.Y[2 * c][lane] = in ? y0 : 0.0;
        sh.Y[2 * c + 1][lane] = in ? y1 : 0.0;
        st_wt(&rec->Y[2 * c][lane], in ? y0 : 0.0);
        st_wt(&rec->Y[2 * c + 1][lane], in ? y1 : 0.0);
      }
    }
    EKF_STAMPT(360 + c, 128);
  }
}

// ---- the fp32 pend patch -------------------------------------------------------------------------
// fp32 Σ: the last step's rank-2 term on the whole block (earlier steps are applied), the final
// Σ[U, U] in fp64, to the record (write-through) for the Σ pass's fp32 tiles (their U × U entries).
// Only a chunk that initialises a landmark has the 1e7 − (1e7 − δ) cancellation the patch is
// for (slam.cpp:130's prior has no cross terms; an untouched landmark's rows stay exact): a first
// sighting, or an association chunk (its new landmark is written by k_assoc). Other chunks keep
// the pass's own values and skip this (k_chain's `pend`).
template <bool J>
__device__ __forceinline__ void write_pend_patch(ChainSharedT<J>& sh, ChunkRec* rec, int m, int nu,
                                                 int tid, bool joseph) {
  constexpr int JM = ChainSharedT<J>::JM;
  auto& P = sh.im.D;
  const int c = max(m - 1, 0);
  for (int e = tid; e < kMaxU * kMaxU; e += blockDim.x) {
    const int a = e / kMaxU, b = e - a * kMaxU;
    double v = P[a][b];
    if (m > 0)
      v = rank2_sub(v, sh.KU[c][a][0], sh.KU[c][a][1], sh.MU[c][b][0], sh.MU[c][b][1]);
    if (m > 0 && joseph) {  // − V_c[a]·K_c[b]ᵀ
      const int cj = min(c, JM - 1);
      v = rank2_sub(v, sh.VU[cj][a][0], sh.VU[cj][a][1], sh.KU[c][b][0], sh.KU[c][b][1]);
    }
    if (a < nu && b < nu) st_wt(&rec->Pend[a][b], v);
  }
}

// ---- the record epilogue -------------------------------------------------------------------------
// Waves 0–2 hand the chunk to the factor kernel (and the next chain): the record, write-through.
// Its epoch is published at the next chunk's start (or the kernel's end): the stores drain behind
// the next prologue instead of stalling this one. The record parity's release (the bulk stream
// done with it) was awaited by the prologue's poll.
template <bool J>
__device__ __forceinline__ void write_record(ChainSharedT<J>& sh, const MsgDesc& d, ChunkRec* rec,
                                             FilterCtl* ctl, int m, int nu, int tid, bool pend) {
  const double* xfin = sh.xU[0];
  if (tid == 0 && sh.status) atomicOr(&ctl->status, sh.status);
  if (tid < kMaxU) {  // state weights: x_i += r_0(i)[U] · Σ_c Z_c ν_c
    const double zx = sh.Zx[tid];  // (wave 1's sum over the corrections)
    const bool in = tid < nu;
    st_wt(&rec->Zx[tid], zx);
    st_wt(&rec->u[tid], sh.u[tid]);
    st_wt(&rec->alphaU[tid], in ? sh.alphaU[tid] : 0.0);
    st_wt(&rec->row0raw[tid], in ? sh.row0raw[tid] : 0.0);
    st_wt(&rec->col0raw[tid], in ? sh.col0raw[tid] : 0.0);
    st_wt(&rec->xU[tid], in ? xfin[tid] : 0.0);
  }
  if (tid == 0) {
    st_wt(&rec->m, m);
    st_wt(&rec->nu, nu);
    st_wt(&rec->flags, d.flags | (pend ? kPendValid : 0));
    st_wt(&rec->a1, sh.a1);
    st_wt(&rec->a2, sh.a2);
    st_wt(&rec->s00, sh.s00);
  }
}

// One workgroup per filter, persistent over the `nchunks` chunks of a launch (descriptors
// A.desc[i·desc_stride + filter]): per chunk the m sequential corrections on the |U|×|U| block.
// Every chunk of a launch after the first rebuilds its block from the chunk before (kLook): the
// previous Σ_in (complete) and the record, the factor kernel's formulas at U. (Carrying the
// chain's own final block into the next chunk instead was 6 % faster but let the chain's block and
// the HBM Σ drift apart — two roundings of the 1e7-prior first sightings — until a survey replay
// went non-finite; the rebuild keeps every schedule bit-identical)
template <typename T, bool J>
__global__ __launch_bounds__(kChainThreads) void k_chain(PassArgs<T> A, int nchunks) {
  __shared__ ChainSharedT<J> sh;
  // The descriptor is read every step: keep it in LDS. Two buffers: a chunk's epilogue prefetches
  // the next one's (and computes its predicted pose from it).
  __shared__ MsgDesc sdesc[2];
  static_assert(sizeof(MsgDesc) % 16 == 0, "MsgDesc copied as uint4");
  const int fy = blockIdx.y;
  const int f = A.f0 + fy;
  const int tid = threadIdx.x;
  const int ld = A.ld;
  FilterCtl* ctl = A.ctl + f;
  // LDS starts as whatever the CU's previous kernel left (possibly NaN bit patterns): zero it once,
  // so padding rows / columns that feed MFMA or dot products as zeros really are zeros
  for (int e = tid; e < static_cast<int>(sizeof(sh) / 8); e += blockDim.x)
    reinterpret_cast<double*>(&sh)[e] = 0.0;
  // Every wave's zeroing stores must land before the one below: the word npose_ci lives in is
  // zeroed by a thread of another wave, and without the barrier that store could come after this
  // one (npose_ci = 0 made chunk 0 copy a never-computed predicted pose, (0, 0, 0)). The race
  // showed where the chain's waves run at different paces — on CUs shared with the bulk stream's
  // kernels (two streams without CU masks: > 32 filters with EKF_SERIAL=0), DESIGN.md §5.
  __syncthreads();
  if (tid == 0) sh.npose_ci = -1;  // (ordered before its first reader by the chunk loop's barriers)
  if (tid == 0) sh.trace_n = -1;   // (likewise)
  bool pre = false;        // sdesc[ci & 1] was prefetched by the previous chunk's epilogue
  unsigned pending = 0;    // chain epoch of the previous chunk, not yet published (its record
                           // stores are still in flight; see the epilogue)
  for (int ci = 0; ci < nchunks; ++ci) {
    // ---- 1. the descriptor ----
    if (!pre) {
      const MsgDesc& gd = A.desc[static_cast<size_t>(ci) * A.desc_stride + fy];
      // planned on the bulk stream beside this launch: the planner's count covers every descriptor
      if (ci == 0 && A.need_plan && tid == 0 && !epoch_wait_acquire(A.sync + kSyncPlan, A.need_plan))
        flag_timeout(&ctl->status, A.fatal);
      __syncthreads();
      if (threadIdx.x < sizeof(MsgDesc) / 16)
        reinterpret_cast<uint4*>(&sdesc[ci & 1])[threadIdx.x] =
            reinterpret_cast<const uint4*>(&gd)[threadIdx.x];
      __syncthreads();
    }
    pre = false;
    const MsgDesc& d = sdesc[ci & 1];
    auto& P = sh.im.D;
    (void)P;  // (EKF_DUMP_BLOCK)
    const bool active = (d.flags & kActive) != 0;
    const bool look = (d.flags & kLook) != 0 && !A.gather;
    // ---- 2. the pending epoch ----
    // Publish the previous chunk's record before this chunk waits on anything the bulk stream
    // produces (its factor kernel needs that record).
    if (pending) {
      drain_stores();
      __syncthreads();
      if (tid == 0) epoch_store(A.sync + kSyncChain + f, pending);
      pending = 0;
    }
    if (!active) continue;  // this filter sits the chunk out
    const unsigned seq = A.seq + static_cast<unsigned>(ci);
    // ---- 3. wait for the bulk stream ----
    // Σ_in / x / records a rebuilding chain reads come from the Σ pass two launches back (bulk
    // stream), and this record parity is free again once that pass is done (its factor kernel read
    // it); a chunk that gathers its own Σ_in needs the pass one back.
    const unsigned need = look ? (seq >= 2 ? seq - 1 : 0u) : seq;
    // A0's associated ids (k_assoc, earlier on this stream), loaded unconditionally (clamped) and
    // here, so that the barrier below completes them: under A0's branch the load was waited for,
    // vmcnt(0), together with every early load below
    const int cA = tid >= 3 && tid < 3 + 2 * d.m ? (tid - 3) >> 1 : 0;
    const int aj = ctl->assoc_j[min(max(d.assoc_slot + cA, 0), kMaxAssoc - 1)];
    // first_ready: the host joined the bulk stream before this launch, so every pass before it is
    // complete (epochs ≤ A.seq), published or not — the launch's second chunk needs the pass just
    // before the launch, whose epoch the flush that issued it did not publish (waiting for a later
    // epoch instead held that chunk until this launch's first pass: ≈ 27 µs)
    if (A.polls && need && tid == 0 && !(A.first_ready && need <= A.seq) &&
        !epoch_wait_acquire(A.sync + kSyncSigma, need))
      flag_timeout(&ctl->status, A.fatal);
    EKF_STAMP(305);
    // (Z, Φ are set up by wave 1 and Y, Ψ by wave 2 at the start of their step loops)
    if (tid == 0) sh.status = 0;
    __syncthreads();
    EKF_STAMP(0);
    const T* S = A.sig[d.parity] + f * A.sig_stride;  // this chunk's Σ_in and x_in (a gathering chunk)
    const double* xin = A.x[d.parity] + f * A.x_stride;
    const int m = d.m;
    const bool first = (d.flags & kFirst) != 0;
    // Joseph (≤ kMaxJoseph markers per chunk): Σ ← Σ − K_c·M_c − (Σ_cHᵀ − K_c·S_c)·K_cᵀ per step,
    // i.e. (I−KH)Σ(I−KH)ᵀ + K·R·Kᵀ expanded (slam.cpp:264-265's update in Joseph form). Row factor
    // V_c = G_c − K_c·S_c beside K_c, column factor K_cᵀ beside M_c: the record's Z carries V_c's
    // row map in columns 32 + 2c.. (kZC + 2c), the chain's block gets the term step by step.
    const bool joseph = J && (d.flags & kJoseph) != 0;
    // kLook: this chunk's Σ_in is still being written by the previous chunk's Σ pass. Rebuild what
    // the chain needs from the chunk before: Σ_in' (the other buffer, complete) and its record.
    const ChunkRec* rp = A.rec + static_cast<size_t>(d.parity ^ 1) * A.rec_stride + f;

    // ---- 4. the early loads (staged image, previous record) ----
    const bool early = look && (d.flags & kStageIn);
    ChainLoads<T, J> loads;
    issue_early_loads(loads, A.stage + static_cast<size_t>(d.parity) * A.rec_stride + f, rp, ctl,
                      tid, early);
    // pose trace: the filter's count, once per launch, by the lane that appends (chain_wave3).
    // Here, behind the poll of step 3, every earlier writer of this filter's t_map_odom — and so
    // of its count — is done: where gather_block / rebuild_block load FilterCtl::tmo.
    if (A.trace && tid == 3 * 64 && sh.trace_n < 0) sh.trace_n = A.trace_n[f];
    EKF_STAMP(14);

    // ---- 5. A0: the index sets ----
    build_index_sets(sh, d, A.N, aj, look, tid);
    lds_barrier();
    EKF_STAMP(1);
    const int nu = sh.nu_cnt;
    const ChainLane L = {tid, tid >> 6, tid & 63, tid & 15, (tid & 63) >> 4};

    // ---- 6. A1: Σ_in[U, U], x_in[U] and the predicted pose, rebuilt or gathered ----
    if (look)
      rebuild_block(sh, d, loads, A.sig[d.parity ^ 1] + f * A.sig_stride,
                    A.x[d.parity ^ 1] + f * A.x_stride, ld, rp, ctl, L, nu, early, A.q, ci, seq);
    else
      gather_block(sh, d, S, xin, ld, ctl, tid, nu);
    EKF_STAMP(6);

    // ---- 7. A3: the predict fold ----
    __syncthreads();
    fold_predict(sh, tid, nu, first, A.q);
    __syncthreads();
    EKF_STAMP(2);
    EKF_DUMP_BLOCK(seq);
    EKF_STAMP(18);

    // ---- 8. A2: the m corrections, one program per wave ----
    // The dependent chain (ẑ, H, S⁻¹, ν → K, M, x → next marker) runs on wave 0 alone, with no
    // workgroup barrier. After step c it publishes K_c, M_c, H_c, S_c⁻¹ and applies the step's rank-2
    // term only to the "cross" of the next marker (all rows × its 5 columns, its 5 rows × the later
    // columns) — the entries step c+1 reads. The other waves follow through LDS flags:
    //   wave 3  the rest of P (rows ∉ next, columns of markers ≥ c+2), one step behind wave 0;
    //   wave 1  Z_c = Φ_c[:, pA]·Hᵀ·S⁻¹, then Φ −= Z_c·M_c (live columns);
    //   wave 2  Y_c = H·Ψ_c[pA, :],      then Ψ −= K_c·Y_c (live rows).
    // Φ, Ψ, Z, Y feed only the factor kernel, so waves 1–2 may lag the chain freely. "Live" = what
    // later steps still read (pose and later markers).
    if (tid == 0) {
      sh.pub = 0;
      sh.pdone = 0;
      sh.zdone = 0;
      sh.any_init = 0;
    }
    if (pending) drain_stores();
    __syncthreads();
    if (pending) {
      if (tid == 0) epoch_store(A.sync + kSyncChain + f, pending);
      pending = 0;
    }
    EKF_STAMP(19);
    const bool pre_next = ci + 1 < nchunks;
    // this chunk's own record (waves 1–2 write Z, Y through; then the pend patch and the rest)
    ChunkRec* const rec = A.rec + static_cast<size_t>(d.parity) * A.rec_stride + f;
    if (L.wv == 0) {
      // A.chain_fast (the default): the lean program as far as the chunk's markers are common
      // cases, the generic one from the first that is not; EKF_CHAIN_FAST=0: the generic one from
      // step 0
      int c = 0;
      if (A.chain_fast) c = chain_wave0_lean<J>((LdsChain<J>*)(&sh), (LdsDesc*)(&d), m, nu, A.r, seq);
      if (c < m) chain_wave0<J>((LdsChain<J>*)(&sh), (LdsDesc*)(&d), c, m, nu, A.r, seq);
      if (tid == 0) {
        sh.n_lean += static_cast<unsigned>(c);
        sh.n_generic += static_cast<unsigned>(m - c);
      }
    } else if (L.wv == 3)
      chain_wave3(sh, d, A, ctl, fy, m, nu, L.ln, ci, nchunks, seq);
    else if (L.wv == 1)
      chain_wave1(sh, rec, m, nu, L.ln, seq);
    else
      chain_wave2(sh, rec, m, nu, L.ln, joseph, seq);
    __syncthreads();

    // ---- 9. the fp32 pend patch ----
    const bool pend = sizeof(T) == 4 && (sh.any_init || (d.flags & kNoInit));
    if (pend) write_pend_patch(sh, rec, m, nu, tid, joseph);
    __syncthreads();
    EKF_STAMP(12);

    // ---- 10. the record (waves 0–2), and the next chunk's descriptor prefetched ----
    // (wave 3 wrote the posterior t_map_odom after the last step, chain_wave3)
    if (L.wv != 3) {
      if (pre_next && tid >= 128 && tid < 128 + static_cast<int>(sizeof(MsgDesc) / 16))
        reinterpret_cast<uint4*>(&sdesc[(ci + 1) & 1])[tid - 128] =
            reinterpret_cast<const uint4*>(
                &A.desc[static_cast<size_t>(ci + 1) * A.desc_stride + fy])[tid - 128];
      write_record(sh, d, rec, ctl, m, nu, tid, pend);
      EKF_STAMP(16);
    }
    pending = seq + 1u;
    pre = pre_next;
    __syncthreads();
    EKF_STAMP(40);
    EKF_STAMPV(307, __builtin_amdgcn_s_memrealtime());
  }  // chunk loop
  if (pending) {
    drain_stores();
    __syncthreads();
    if (tid == 0) epoch_store(A.sync + kSyncChain + f, pending);
  }
  // the launch's step counts (a filter's chain launches are ordered: plain loads and stores)
  if (tid == 0 && (sh.n_lean | sh.n_generic)) {
    ctl->chain_steps[0] += sh.n_lean;
    ctl->chain_steps[1] += sh.n_generic;
  }
}
template <typename T>
hipError_t launch_chain(const PassArgs<T>& a, int nf, int nchunks, hipStream_t s, hipEvent_t e0,
                        hipEvent_t e1) {
  // (the Joseph form's instantiation: a handle's chunks are all of its form, ekf_set_joseph)
  launch(a.joseph ? k_chain<T, true> : k_chain<T, false>, dim3(1, nf), dim3(kChainThreads), s, e0,
         e1, a, nchunks);
  return hipGetLastError();
}
template hipError_t launch_chain<double>(const PassArgs<double>&, int, int, hipStream_t, hipEvent_t,
                                         hipEvent_t);
template hipError_t launch_chain<float>(const PassArgs<float>&, int, int, hipStream_t, hipEvent_t,
                                        hipEvent_t);

}  // namespace ekfslam
