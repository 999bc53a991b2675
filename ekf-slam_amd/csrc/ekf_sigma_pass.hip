// k_sigma_pass (gfx950 / CDNA4): the third kernel of a chunk (ekf_chain.hip's header has the
// three), the rank-(2+2m) update of the dense covariance from the factor kernel's Kcat / Mcat, with
// what runs right behind it on its stream: k_stage and the Σ-pass epoch. The pass's tile grid, for
// the launcher and the kernel alike, is sigma_grid.hpp's.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ekf_device.hpp"
#include "ekf_launch.hpp"
#include "ekf_math.hpp"
#include "sigma_grid.hpp"

namespace ekfslam {

#include "ekf_diag.hpp"  // (SIG_STAMP; empty in the product library)
#ifdef EKF_DIAG_STAMPS
__device__ unsigned long long g_sig_stamps[4096][5];
#endif

#include "ekf_sync.hpp"  // (hand-off protocol and buffer-descriptor helpers)

// ---- Σ pass on MFMA -------------------------------------------------------------------------
// Σ_out = Σ_in + Q̄ − Σ_k Kcat[k]ᵀ ⊗ Mcat[k], one tile per wave, four waves per workgroup.
//   fp32  32×32 tile, v_mfma_f32_32x32x2_f32: D[row = (r&3) + 8(r>>2) + 4(lane>>5)][col = lane&31]
//         → each load / store instruction covers 2 rows × 128 B
//   fp64  32×16 tile, two v_mfma_f64_16x16x4_f64 blocks: D[row = 16ti + (lane>>4) + 4r][col = lane&15]
//         → 4 rows × 128 B per instruction
// A/B lane maps: 16x16x4 A[i = lane&15][k = lane>>4]; 32x32x2 A[i = lane&31][k = lane>>5].
// Memory goes through buffer descriptors with 32-bit offsets (no 64-bit address per load):
//   - Σ: the wave's 32-row panel (up to row n); a row ≥ n lies past the end, a column ≥ n gets
//     the offset kOOB, so the range check returns 0 for its loads and drops its stores (no masks,
//     no waits);
//   - Kcat / Mcat: the factor rows are uniform (SGPR soffset), the lane's column in voffset.
// Order: operands (L2-hot) first, then Σ_in. The MFMAs start from zero as soon as the operands
// land and run while Σ_in is still in flight; Σ_in (+ Q̄) is added once, before the store.
typedef float f16v __attribute__((ext_vector_type(16)));
constexpr unsigned kOOB = 0x80000000u;  // voffset past any Σ panel descriptor (32·ld·w < 2 GiB)


template <typename T>
struct SigmaTile;

// The simple form's factor rank is at most 2 + 2·kMaxChunk = 34: 17 k-steps of the 32×32×2 MFMA.
// (kw, the rank rounded up to 4 for the fp64 tiles, would make it 18, the last one on the two zero
// rows 34–35.) A Joseph chunk's rank 2 + 4m ≤ 66 (kw ≤ 68) takes a second block of 17 k-steps
// (KB = 2): the operand registers are loaded again for it, so the tile keeps its register count.
constexpr int kSteps = (2 + 2 * kMaxChunk + 1) / 2;
static_assert(kMaxKW <= 4 * kSteps, "Joseph rank within two blocks of fp32 k-steps");
struct F32TileRegs {  // one fp32 tile's loads
  float a[kSteps], b[kSteps], sv[16];
};
template <>
struct SigmaTile<float> {
  static constexpr int kRows = 32, kCols = 32;
  // descriptors based at the wave's row panel: offsets stay 32-bit for any n (a filter's Σ may
  // exceed 4 GiB), and the records end at row n
  static __device__ __forceinline__ __amdgpu_buffer_rsrc_t panel(const float* S, int n, int ld,
                                                                 int R0) {
    return buf_rsrc(S + static_cast<size_t>(R0) * ld,
                    static_cast<unsigned>(min(n - R0, kRows)) * ld * 4u);
  }
  static __device__ __forceinline__ unsigned soff(int n, int ld, int C0, int lane) {
    const int col = C0 + (lane & 31);
    return col < n ? static_cast<unsigned>(4 * (lane >> 5) * ld + col) * 4u : kOOB;
  }
  // block kb: factor rows 2·kSteps·kb + 2s + (lane ≥ 32)
  static __device__ __forceinline__ void load_ops(F32TileRegs& g, const float* kc, const float* mc,
                                                  int n, int ldk, int R0, int C0, int lane,
                                                  int kb = 0) {
    const int kr = lane >> 5, kcol = lane & 31;
    const unsigned kbytes = static_cast<unsigned>(kMaxKW) * ldk * 4u;
    const auto rk = buf_rsrc(kc, kbytes), rm = buf_rsrc(mc, kbytes);
    const int k0 = 2 * kSteps * kb;
    const unsigned ko = static_cast<unsigned>((k0 + kr) * ldk + R0 + kcol) * 4u;
    const unsigned mo = static_cast<unsigned>((k0 + kr) * ldk + min(C0 + kcol, n - 1)) * 4u;
    const unsigned kstep = 2u * ldk * 4u;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      g.a[s] = ld_f32(rk, ko, s * kstep);
      g.b[s] = ld_f32(rm, mo, s * kstep);
    }
  }
  static __device__ __forceinline__ void load_sig(F32TileRegs& g, const float* Sin, int n, int ld,
                                                  int R0, int C0, int lane) {
    const auto rin = panel(Sin, n, ld, R0);
    const unsigned so = soff(n, ld, C0, lane);
    const unsigned rstride = static_cast<unsigned>(ld) * 4u;
#pragma unroll
    for (int r = 0; r < 16; ++r) g.sv[r] = ld_f32(rin, so + ((r & 3) + 8 * (r >> 2)) * rstride, 0);
  }
  // the MFMAs on the tile's operands, Σ_in − K·M (+ Q̄), the stores
  // pm (≠ null: the chunk's record holds the chain's fp64 Σ[U, U], kPendValid): the tile's patch
  // map (patch_map below) — the entries whose row and column are both in U take the record's value
  static __device__ __forceinline__ void finish(const F32TileRegs& g, float* Sout, int n, int ld,
                                                int kw, bool first, double qd, int R0, int C0,
                                                int lane, const int* pm = nullptr,
                                                const ChunkRec* rec = nullptr) {
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    mma(g, kw, 0, acc);
    store(g, acc, Sout, n, ld, first, qd, R0, C0, lane, pm, rec);
  }
  // the k-steps of one operand block (k0: its first factor row): every MFMA issued, factor rows
  // ≥ kw (stale) zeroed by a select — a branch per k-step let the compiler sink each operand load
  // into its branch behind a vmcnt(0)
  static __device__ __forceinline__ void mma(const F32TileRegs& g, int kw, int k0, f16v& acc) {
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const bool live = k0 + 2 * s < kw;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(live ? g.a[s] : 0.0f, live ? g.b[s] : 0.0f, acc,
                                                 0, 0, 0);
    }
  }
  // Joseph: the two operand blocks (the first loaded before Σ_in, the second after its MFMAs)
  static __device__ __forceinline__ void finish2(F32TileRegs& g, const float* kc, const float* mc,
                                                 int ldk, float* Sout, int n, int ld, int kw,
                                                 bool first, double qd, int R0, int C0, int lane,
                                                 const int* pm, const ChunkRec* rec) {
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    mma(g, kw, 0, acc);
    load_ops(g, kc, mc, n, ldk, R0, C0, lane, 1);
    mma(g, kw, 2 * kSteps, acc);
    store(g, acc, Sout, n, ld, first, qd, R0, C0, lane, pm, rec);
  }
  static __device__ __forceinline__ void store(const F32TileRegs& g, const f16v& acc, float* Sout,
                                               int n, int ld, bool first, double qd, int R0,
                                               int C0, int lane, const int* pm,
                                               const ChunkRec* rec) {
    const int kr = lane >> 5, col = C0 + (lane & 31);
    const auto rout = panel(Sout, n, ld, R0);
    const unsigned so = soff(n, ld, C0, lane);
    const unsigned rstride = static_cast<unsigned>(ld) * 4u;
    const float* sv = g.sv;
    SIG_STAMP(2);
    const float q = static_cast<float>(qd);
    if (!pm) {  // (two loops: the common one keeps the plain store sequence)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = R0 + (r & 3) + 8 * (r >> 2) + 4 * kr;
        float v = sv[r] - acc[r];
        if (first && row == col && row < 3) v += q;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout,
                                              so + ((r & 3) + 8 * (r >> 2)) * rstride, 0, 0);
      }
      return;
    }
    const int pc = pm[32 + (lane & 31)];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = (r & 3) + 8 * (r >> 2) + 4 * kr, row = R0 + rl;
      float v = sv[r] - acc[r];
      if (first && row == col && row < 3) v += q;
      const int pr = pm[rl];
      if (pr < kMaxU && pc < kMaxU) v = static_cast<float>(rec->Pend[pr][pc]);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout,
                                            so + ((r & 3) + 8 * (r >> 2)) * rstride, 0, 0);
    }
  }
};

// fp64 tile of 32 × 16·TJ: TJ = 2 for a few filters (more waves per filter), TJ = 4 for swarms
// (≥ 16 filters): the M operand rows are read once per 64 columns instead of per 32 — the
// operand loads are the pass's VMEM bottleneck there (swarm pass 589 → 564 µs; one filter's pass
// 5.2 → 7.6 µs, so it keeps TJ = 2)
// 2 = nt: the swarm's 2.2 GB of Σ stream through HBM once per message (≫ the 256 MB MALL), so its
// Σ_in loads and Σ_out stores skip cache retention — swarm 1.09e7 → 1.15e7 corrections/s
// (profiles/r2/r2z_*, two alternating runs each). The MALL-resident single-filter tiles keep the default.
#ifndef EKF_SIG_POL
#define EKF_SIG_POL 2
#endif
// Symmetric: Σ_out is symmetric (Σ_in + Q̄ − Kcatᵀ·Mcat is, the predict's A·Σ·Aᵀ and every
// correction's K·S·Kᵀ are), so an fp64 pass computes only the tiles holding an element on or above
// the diagonal (first tile column of tile row tr: ⌊32·tr / kCols⌋) and writes every element (r, c),
// r > c, as the mirror of (c, r): Σ_in is read in those tiles only (≈ 0.58 of Σ at the swarm's n),
// the MFMA work of the strictly-lower tiles is skipped, and Σ_out stays exactly symmetric. The
// mirror goes out through the wave's LDS (the tile transposed, then row by row: a direct
// transposed store is 16 rows × 32 B per instruction, measured 1.5× slower than the whole pass).
// Swarm pass 445 → 379 µs standalone, bit-identical in the upper triangle (tools/pass64_lab.hip).
constexpr int kTS = 34;  // transposed tile row stride (doubles; 16 B aligned rows)
template <int TJ_>
struct SigmaTile64 {
  static constexpr int TJ = TJ_;
  // cache policy of the swarm tile's Σ_in loads / Σ_out stores (the swarm's Σ streams through HBM)
  static constexpr int kPol = TJ == 4 ? EKF_SIG_POL : 0;
  static constexpr int kRows = 32, kCols = 16 * TJ;
  static constexpr int kLds = kCols * kTS;  // doubles of the wave's transposed tile
  // KB operand blocks of 36 factor rows (Joseph: 2, rank 2 + 4m ≤ 66; the second block's operands
  // reuse the first's registers after its MFMAs)
  template <int KB = 1>
  static __device__ __forceinline__ void run(const double* Sin, double* Sout, const double* kc,
                                             const double* mc, int n, int ld, int ldk, int kw,
                                             bool first, double q, int R0, int C0, int lane,
                                             double* tT) {
    const int kr = lane >> 4, kcol = lane & 15;
    // descriptors based at the wave's row panel: offsets stay 32-bit for any n (a filter's Σ
    // may exceed 4 GiB), and the records end at row n
    const size_t pbase = static_cast<size_t>(R0) * ld;
    const unsigned sbytes = static_cast<unsigned>(min(n - R0, kRows)) * ld * 8u;
    const unsigned kbytes = static_cast<unsigned>(kMaxKW) * ldk * 8u;
    const auto rin = buf_rsrc(Sin + pbase, sbytes), rout = buf_rsrc(Sout + pbase, sbytes);
    // the mirror: rows C0 … C0 + kCols − 1 of Σ_out from column R0
    const auto rmir = buf_rsrc(Sout + static_cast<size_t>(C0) * ld + R0,
                               static_cast<unsigned>(min(n - C0, kCols)) * ld * 8u);
    const auto rk = buf_rsrc(kc, kbytes), rm = buf_rsrc(mc, kbytes);
    double a[2][9], b[TJ][9], sv[2][TJ][4];
    const unsigned ko = static_cast<unsigned>(kr * ldk + R0 + kcol) * 8u;
    unsigned mo[TJ], so[TJ];
    const unsigned rstride = static_cast<unsigned>(ld) * 8u;
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
      const int col = C0 + 16 * tj + kcol;
      mo[tj] = static_cast<unsigned>(kr * ldk + min(col, n - 1)) * 8u;
      so[tj] = col < n ? static_cast<unsigned>(kr * ld + col) * 8u : kOOB;
    }
    const unsigned kstep = 4u * ldk * 8u;
    auto load_ops = [&](int kb) {
#pragma unroll
      for (int s = 0; s < 9; ++s) {
        a[0][s] = ld_f64(rk, ko, (9 * kb + s) * kstep);
        a[1][s] = ld_f64(rk, ko + 16 * 8, (9 * kb + s) * kstep);
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj) b[tj][s] = ld_f64(rm, mo[tj], (9 * kb + s) * kstep);
      }
    };
    load_ops(0);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sv[ti][tj][r] = __builtin_bit_cast(
              double, __builtin_amdgcn_raw_buffer_load_b64(rin, so[tj] + (16 * ti + 4 * r) * rstride, 0, kPol));
    d4 acc[2][TJ];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < TJ; ++tj) acc[ti][tj] = d4{0, 0, 0, 0};
    auto mma = [&](int kb) {
#pragma unroll
      for (int s = 0; s < 9; ++s) {  // unconditional, stale rows ≥ kw zeroed (see the fp32 tile)
        const bool live = 36 * kb + 4 * s < kw;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int tj = 0; tj < TJ; ++tj)
            acc[ti][tj] = mfma_f64(live ? a[ti][s] : 0.0, live ? b[tj][s] : 0.0, acc[ti][tj]);
      }
    };
    mma(0);
    if (KB == 2) {
      load_ops(1);
      mma(1);
    }
    SIG_STAMP(2);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rl = 16 * ti + kr + 4 * r, cl = 16 * tj + kcol;
          const int row = R0 + rl, col = C0 + cl;
          double v = sv[ti][tj][r] - acc[ti][tj][r];
          if (first && row == col && row < 3) v += q;
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, v), rout,
                                                col >= row ? so[tj] + (16 * ti + 4 * r) * rstride : kOOB,
                                                0, kPol);
          tT[cl * kTS + rl] = v;
        }
    // the mirror, two rows of the transposed tile per store (LDS in order within the wave)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const int rl = lane & 31;
#pragma unroll
    for (int i = 0; i < kCols / 2; ++i) {
      const int cl = 2 * i + (lane >> 5);
      const double v = tT[cl * kTS + rl];
      const int row = R0 + rl, col = C0 + cl;
      const unsigned mo2 = col > row && col < n ? static_cast<unsigned>(cl * ld + rl) * 8u : kOOB;
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, v), rmir, mo2, 0, kPol);
    }
  }
};
template <>
struct SigmaTile<double> : SigmaTile64<2> {};
// the tile a Σ pass of T runs: WIDE (swarms) takes the 32 × 64 fp64 tile
template <typename T, bool WIDE>
using PassTile = typename std::conditional<sizeof(T) == 8 && WIDE, SigmaTile64<4>, SigmaTile<T>>::type;
constexpr int kPassWaves = 4;  // waves (= tiles) per workgroup

// The fp32 tile's patch map, in the wave's 64 ints of LDS: pm[0..32) the first position in the
// chunk's U (rec->u[0..nu)) of each of the tile's rows R0 … R0 + 31, pm[32..64) of each of its
// columns C0 … C0 + 31; kMaxU (> any position) for a row / column not in U. Each lane brings one
// position of U; an index listed twice keeps its first position (atomicMin). Within the wave only:
// the fences order its LDS accesses, no barrier.
__device__ __forceinline__ const int* patch_map(int* map, const ChunkRec* rec, int R0, int C0,
                                                int lane) {
  map[lane] = kMaxU;
  const int nu = rec->nu, u = rec->u[min(lane, kMaxU - 1)];
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  if (lane < nu && u >= R0 && u < R0 + 32) atomicMin(&map[u - R0], lane);
  if (lane < nu && u >= C0 && u < C0 + 32) atomicMin(&map[32 + u - C0], lane);
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  return map;
}

// One fp32 tile (tr, tc) of filter A.f0 + fb. The operand loads depend only on the filter and the
// tile, so they go out before the descriptor's scalar round trips (flags, parity, m, then the Σ
// pointer it selects) instead of behind them (≈ 0.3 µs of a 9 µs pass, tools/pass_lab.hip).
// map: the wave's 64 ints of LDS (patch_map).
template <int KB>
__device__ __forceinline__ void pass_tile_f32(const PassArgs<float>& A, const MsgDesc& d, int fb,
                                              int tr, int tc, int lane, int* map) {
  using Tile = SigmaTile<float>;
  const int f = A.f0 + fb;
  const int R0 = tr * Tile::kRows, C0 = tc * Tile::kCols;
  // the patch test's record flags of both parities, issued with the operands (not a scalar round
  // trip behind the descriptor's parity: that wait cost ≈ 0.4 µs of the pass)
  const int rf0 = A.rec[f].flags, rf1 = A.rec[A.rec_stride + f].flags;
  F32TileRegs g;
  Tile::load_ops(g, A.kcat + f * A.km_stride, A.mcat + f * A.km_stride, A.n, A.ldk, R0, C0, lane);
  // keep the operand loads ahead of Σ_in's: the MFMAs then wait for vmcnt(16), not vmcnt(0)
  __builtin_amdgcn_sched_barrier(0);
  if (!(d.flags & kActive)) return;
  SIG_STAMP(1);
  const int kw = pass_kw((d.flags & kJoseph) != 0, d.m);
  Tile::load_sig(g, A.sig[d.parity] + f * A.sig_stride, A.n, A.ld, R0, C0, lane);
  // the fp32 patch: the chain's fp64 Σ[U, U] over this tile's entries there, for the chunks that
  // initialised a landmark (the pass's 1e7 − (1e7 − δ) at a first sighting — the reference's
  // prior, slam.cpp:130 — loses δ in fp32)
  const ChunkRec* rec = A.rec + static_cast<size_t>(d.parity) * A.rec_stride + f;
  const int* pm = nullptr;
  if ((d.parity ? rf1 : rf0) & kPendValid) pm = patch_map(map, rec, R0, C0, lane);  // wave-uniform
  float* Sout = A.sig[d.parity ^ 1] + f * A.sig_stride;
  const bool first = (d.flags & kFirst) != 0;
  if constexpr (KB == 1)
    Tile::finish(g, Sout, A.n, A.ld, kw, first, A.q, R0, C0, lane, pm, rec);
  else
    Tile::finish2(g, A.kcat + f * A.km_stride, A.mcat + f * A.km_stride, A.ldk, Sout, A.n, A.ld, kw,
                  first, A.q, R0, C0, lane, pm, rec);
}

// One fp64 tile (SigmaTile64) of filter A.f0 + fb. tT: the wave's Tile::kLds doubles of LDS.
template <typename Tile, int KB>
__device__ __forceinline__ void pass_tile_f64(const PassArgs<double>& A, const MsgDesc& d, int fb,
                                              int tr, int tc, int lane, double* tT) {
  if (!(d.flags & kActive)) return;
  SIG_STAMP(1);
  const int f = A.f0 + fb;
  // this filter's rank; rows beyond are stale
  const int kw = pass_kw((d.flags & kJoseph) != 0, d.m);
  Tile::template run<KB>(A.sig[d.parity] + f * A.sig_stride, A.sig[d.parity ^ 1] + f * A.sig_stride,
                         A.kcat + f * A.km_stride, A.mcat + f * A.km_stride, A.n, A.ld, A.ldk, kw,
                         (d.flags & kFirst) != 0, A.q, tr * Tile::kRows, tc * Tile::kCols, lane, tT);
}

// An explicit occupancy target (the one the registers allowed anyway: 2 waves/SIMD for the wide
// fp64 tile, 4–5 for the narrow one, 6–7 for fp32) makes the allocator keep the MFMA accumulators
// in VGPRs instead of AGPRs (no v_accvgpr_read before the Σ_in subtraction and the stores): swarm
// message 0.719 → 0.703 ms, N = 1024 fp64 pass 16.4 → 15.9 µs, fp32 unchanged
// (profiles/r3/p3r_vgpr_acc_ab.txt, two alternating runs each)
// As it stands: PassTile<float, true> is the very tile PassTile<float, false> is, yet the fp32
// swarm's instantiation k_sigma_pass<float, true, KB> is a kernel of its own with the target 2
// where the narrow fp32 one has 6. Whether that is intended is a performance question; the
// launcher's choice of instantiation (WIDE = many filters) is left as it is.
template <typename T, bool WIDE>
constexpr int kPassWavesPerEu = WIDE ? 2 : (sizeof(T) == 8 ? 4 : 6);
// KB: operand blocks of the rank (the Joseph form's instantiation: 2). G: sigma_grid() of this
// launch, the one the launcher sized its grid from.
template <typename T, bool WIDE, int KB>
__global__ __launch_bounds__(64 * kPassWaves)
__attribute__((amdgpu_waves_per_eu(kPassWavesPerEu<T, WIDE>))) void k_sigma_pass(PassArgs<T> A,
                                                                                 SigmaGrid G) {
  using Tile = PassTile<T, WIDE>;
  constexpr bool kSym = sizeof(T) == 8;  // fp64: the symmetric tiles (SigmaTile64)
  SIG_STAMP(0);
  __shared__ int cmap[kPassWaves][64];  // per wave: the fp32 tile's patch map
  __shared__ double tT[kPassWaves][kSym ? PassTile<double, WIDE>::kLds : 1];  // fp64: the mirror
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // The wave's filter and tile are sigma_grid_tile's. Two things only keep the scalar loads ahead
  // of it as few as they were (each is a dependent round trip before the wave's first vector
  // load; one more was + 0.5 % on the swarm's pass, profiles/r14/sigma_pass_grid/): the waves per
  // workgroup are the kernel's own constant instead of a field loaded from G, and the workgroup's
  // filter is resolved first, which brings the XCD-dealt grid's fields in with the first load.
  SigmaGrid g = G;
  g.wpb = kPassWaves;
  int b;
  if (sigma_grid_filter(g, blockIdx.x, blockIdx.y, b) < 0) return;
  const SigmaTileAt at = sigma_grid_tile<Tile::kCols, kSym>(g, blockIdx.x, blockIdx.y, wave);
  if (at.filter < 0) return;
  const MsgDesc& d = A.desc[at.filter];
  if constexpr (kSym)
    pass_tile_f64<Tile, KB>(A, d, at.filter, at.tr, at.tc, lane, tT[wave]);
  else
    pass_tile_f32<KB>(A, d, at.filter, at.tr, at.tc, lane, cmap[wave]);
  SIG_STAMP(3);
}

// Right behind the Σ pass on its stream, for chunks that stage (kStageOut, either dtype): the
// rebuild operands of the filter's chunk after next (StageRec), gathered from the Σ_out / x_out
// just completed — off the chain's critical path, where the same gather at the chain's start cost
// ≈ 10 µs of a 47 µs message (≈ 1 900 scattered lines through one CU). One workgroup per filter.
// fp32: the pass's tiles have already written the chain's fp64 Σ[U, U] over their entries
// (pass_tile_f32), so the Σ_out read here is the patched one, as the chain would gather it.
template <typename T>
__global__ __launch_bounds__(256) void k_stage(PassArgs<T> A) {
  const MsgDesc& d = A.desc[blockIdx.x];
  const int flags = d.flags;
  if (!(flags & kActive) || !(flags & kStageOut)) return;
  const int f = A.f0 + blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ int sgu[kStW], sgp[kStW];  // staged chain's U and U' (columns)
  // ---- one global round trip: the staged chunks' ids ----
  // threads 0 … 35: a = tid (U of the chunk after next); 64 … 99: a = tid − 64 (U', the next chunk's)
  const bool isp = tid >= 64;
  const int sa = isp ? tid - 64 : tid;
  const int sm = isp ? d.stg_pm : d.stg_m;
  const int sid = (isp ? d.stg_pids : d.stg_ids)[min(max(sa - 3, 0) >> 1, kMaxChunk - 1)];
  if (sa < kStW && (tid < kStW || (isp && tid < 64 + kStW))) {
    int col = 0;
    if (sa < 3) col = sa;
    else if (sa < 3 + 2 * sm && sa < kMaxU)
      // k_chain's A0 mapping: marker c → 3 + 2·id (+1), a bad id → slot 0's, padding → 0
      col = (sid < 0 || sid >= A.N ? 3 : 3 + 2 * sid) + ((sa - 3) & 1);
    (isp ? sgp : sgu)[sa] = col;
  }
  __syncthreads();
  // ---- stage: the chunk after next's rebuild operands (the second global round trip) ----
  const T* S = A.sig[d.parity ^ 1] + f * A.sig_stride;
  const double* xo = A.x[d.parity ^ 1] + f * A.x_stride;
  StageRec<T>* sg = A.stage + static_cast<size_t>(d.parity) * A.rec_stride + f;
  auto val = [&](int r, int c) -> T { return S[static_cast<size_t>(r) * A.ld + c]; };
  // The three blocks by image position (RebuildImage: the chain's LDS layout), entry e = row·36 +
  // column of each: D and R rows a over U, C rows k over U' with a along the row (the transposed
  // store the chain did). Loads unconditional (clamped), zeros selected after: a ≥ |U|, b ≥ |U|,
  // k ≥ |U'| and the padding slots.
  constexpr int kSPer = (kStW * kStW + 255) / 256;  // 6
  const int gnu = 3 + 2 * min(d.stg_m, kMaxChunk), gnp = 3 + 2 * min(d.stg_pm, kMaxChunk);
  T od[kSPer], orr[kSPer], oc[kSPer];
#pragma unroll
  for (int i = 0; i < kSPer; ++i) {
    const int e = min(tid + 256 * i, kStW * kStW - 1);
    const int r = e / kStW, c = e % kStW;
    const int a = min(r, kMaxU - 1), b = min(c, kMaxU - 1);
    const T vd = val(sgu[a], sgu[b]);
    const T vr = val(sgu[a], sgp[b]);
    const T vc = val(sgp[a], sgu[b]);  // C[k = r][a = c]
    od[i] = r < gnu && c < gnu ? vd : T(0);
    orr[i] = r < gnu && c < gnp ? vr : T(0);
    oc[i] = r < gnp && c < gnu ? vc : T(0);
  }
  const int t = min(tid, kMaxU - 1);  // (row / column 0: the pose θ)
  const T r0u = val(0, sgu[t]), c0u = val(sgu[t], 0);
  const T r0p = val(0, sgp[t]), c0p = val(sgp[t], 0);
  const double xg = xo[sgu[t]];
  if (tid < kStW) {
    sg->r0u[tid] = static_cast<double>(r0u);
    sg->c0u[tid] = static_cast<double>(c0u);
    sg->r0p[tid] = static_cast<double>(r0p);
    sg->c0p[tid] = static_cast<double>(c0p);
    sg->xg[tid] = xg;
  }
#pragma unroll
  for (int i = 0; i < kSPer; ++i) {
    const int e = tid + 256 * i;
    if (e < kMaxU * kStW) {
      (&sg->im.D[0][0])[e] = od[i];
      (&sg->im.R[0][0])[e] = orr[i];
    }
    if (e < kStW * kStW) (&sg->im.C[0][0])[e] = oc[i];
  }
}

// Σ-pass epoch for the chains on the other stream, launched right behind the Σ pass on its stream:
// the kernel boundary's release has written the pass's Σ_out (and the factor kernel's x, Kcat,
// Mcat) back before this store, so the pass itself keeps plain stores and no per-block release.
__global__ void k_sigma_epoch(unsigned* sync, unsigned epoch) {
  if (threadIdx.x == 0) epoch_store(sync + kSyncSigma, epoch);
}
// The pass with the WIDE or the narrow tile, on that tile's grid (fp64: the symmetric one).
template <typename T, bool WIDE>
static void launch_pass_tiles(const PassArgs<T>& a, int nf, hipStream_t s, hipEvent_t e0,
                              hipEvent_t e1) {
  using Tile = PassTile<T, WIDE>;
  const SigmaGrid g = sigma_grid(a.n, nf, Tile::kRows, Tile::kCols, sizeof(T) == 8, kPassWaves);
  launch(a.joseph ? k_sigma_pass<T, WIDE, 2> : k_sigma_pass<T, WIDE, 1>, dim3(g.grid_x, g.grid_y),
         dim3(64 * kPassWaves), s, e0, e1, a, g);
}
template <typename T>
hipError_t launch_sigma_pass(const PassArgs<T>& a, int nf, bool publish, bool stage, hipStream_t s,
                             hipEvent_t e0, hipEvent_t e1) {
  // the swarms' XCD-dealt grid goes with the wide fp64 tile
  if (nf >= kGridXcdFilters)
    launch_pass_tiles<T, true>(a, nf, s, e0, e1);
  else
    launch_pass_tiles<T, false>(a, nf, s, e0, e1);
  if (stage) hipLaunchKernelGGL(k_stage<T>, dim3(nf), dim3(256), 0, s, a);
  // the pass's epoch (otherwise published by the next chunk's factor kernel, PassArgs::pub_sigma)
  if (publish && a.polls)
    hipLaunchKernelGGL(k_sigma_epoch, dim3(1), dim3(64), 0, s, a.sync, a.seq + 1u);
  return hipGetLastError();
}
template hipError_t launch_sigma_pass<double>(const PassArgs<double>&, int, bool, bool, hipStream_t,
                                              hipEvent_t, hipEvent_t);
template hipError_t launch_sigma_pass<float>(const PassArgs<float>&, int, bool, bool, hipStream_t,
                                             hipEvent_t, hipEvent_t);

}  // namespace ekfslam

