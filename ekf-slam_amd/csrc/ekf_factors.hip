// k_factors (gfx950 / CDNA4): the second kernel of a chunk (ekf_chain.hip's header has the three).
// From the chain's record (ChunkRec) and Σ_in it builds the chunk's low-rank factors
// Kcat = Σ_pred[:, U]·Z and Mcat = Y·Σ_pred[U, :] for every row / column on f64 MFMA
// (v_mfma_f64_16x16x4f64), plus the new state x; the Σ pass (ekf_sigma_pass.hip) applies them.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ekf_device.hpp"
#include "ekf_launch.hpp"
#include "ekf_math.hpp"

namespace ekfslam {

#include "ekf_sync.hpp"  // (hand-off protocol and buffer-descriptor helpers)

template <bool J>
struct FactorSharedT {
  static constexpr int ZC = J ? kZJ : kZC;  // the record's Z columns in use (Joseph: Z and Zv)
  int u[kMaxU + 1];
  double alphaU[kMaxU], row0raw[kMaxU], col0raw[kMaxU], Zx[kMaxU], xU[kMaxU];
  double Z[kMaxU][ZC + 1];
  double Y[kZC][kMaxU + 1];
  double a1, a2, s00;
  int nu;
};

// The factor kernel's two halves: a chunk's record into LDS, then one wave's 16 indices of Kcat = R_pred·Z (rows) and
// Mcat = Y·C_pred (columns) on f64 MFMA, plus the new state.
// R_pred(i)[b] = Σ_pred[i][u_b], C_pred(j)[a] = Σ_pred[u_a][j].
template <bool J>
__device__ __forceinline__ void factor_record(const ChunkRec* rec, FactorSharedT<J>& sh, int tid) {
  constexpr int ZC = FactorSharedT<J>::ZC;
  {  // the record into LDS: every load of a thread issued before its first LDS store
    constexpr int kPer = (kMaxU * kZC + 255) / 256;  // 5
    constexpr int kPerZ = (kMaxU * ZC + 255) / 256;  // 5 (Joseph: 9)
    double vz[kPerZ], vy[kPer];
#pragma unroll
    for (int i = 0; i < kPerZ; ++i) {  // (the record's rows are kZJ wide)
      const int e = min(tid + 256 * i, kMaxU * ZC - 1);
      vz[i] = rec->Z[e / ZC][e % ZC];
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int e = min(tid + 256 * i, kMaxU * kZC - 1);
      vy[i] = (&rec->Y[0][0])[e];
    }
#pragma unroll
    for (int i = 0; i < kPerZ; ++i) {
      const int e = tid + 256 * i;
      if (e < kMaxU * ZC) {
        const int b = e / ZC, k = e - b * ZC;
        sh.Z[b][k] = vz[i];
      }
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int e = tid + 256 * i;
      if (e < kMaxU * kZC) {
        const int k2 = e / kMaxU, b2 = e - k2 * kMaxU;
        sh.Y[k2][b2] = vy[i];
      }
    }
  }
  if (tid < kMaxU) {
    sh.u[tid] = rec->u[tid];
    sh.alphaU[tid] = rec->alphaU[tid];
    sh.row0raw[tid] = rec->row0raw[tid];
    sh.col0raw[tid] = rec->col0raw[tid];
    sh.Zx[tid] = rec->Zx[tid];
    sh.xU[tid] = rec->xU[tid];
  }
  if (tid == 0) {
    sh.a1 = rec->a1;
    sh.a2 = rec->a2;
    sh.s00 = rec->s00;
    sh.nu = rec->nu;
  }
}

template <typename T, bool J>
__device__ __forceinline__ void factor_wave(const PassArgs<T>& A, const MsgDesc& d, int f, int wg,
                                            const FactorSharedT<J>& sh, int lane) {
  constexpr int NG = FactorSharedT<J>::ZC / 16;  // 16-column groups of Z: 2 (Joseph: 4)
  const int n = A.n, ld = A.ld, ldk = A.ldk;
  const T* S = A.sig[d.parity] + f * A.sig_stride;
  const double* xin = A.x[d.parity] + f * A.x_stride;
  double* xout = A.x[d.parity ^ 1] + f * A.x_stride;
  T* kc = A.kcat + f * A.km_stride;
  T* mc = A.mcat + f * A.km_stride;
  const bool first = (d.flags & kFirst) != 0;
  const bool joseph = J && (d.flags & kJoseph) != 0;
  // Joseph: Mcat rows 2 + 2m .. 2 + 4m − 1 hold K_c (the V_c·K_cᵀ term's column factor), written
  // by the row waves; the column waves leave them alone
  const int jk0 = joseph ? 2 * d.m : kZC, jk1 = joseph ? 4 * d.m : kZC;
  const int nu = sh.nu;
  const double* xfin = sh.xU;
  // ---- phase B: Kcat = R_pred·Z, Mcat = Y·C_pred on f64 MFMA, 16 rows (or columns) per wave ----
  // R_pred(i)[b] = Σ_pred[i][u_b], C_pred(j)[a] = Σ_pred[u_a][j] (predict folded in as above).
  const int row_tiles = (n + 15) / 16;
  const int ks = lane >> 4, l16 = lane & 15;
  const double s00 = sh.s00;
  // Mcat columns j = C0 + l16 of a wave from Σ_in[U, j] (raw) and Σ_in[0, j] (c0t)
  auto columns = [&](int j, const T (&raw)[9], T c0t) {
    const bool vj = j < n;
    const double c0raw = vj ? static_cast<double>(c0t) : 0.0;
    const double aj = first ? alpha_of(j, sh.a1, sh.a2) : 0.0;
    double bv[9];
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      const int k = 4 * s + ks;
      double v = (vj && k < nu) ? static_cast<double>(raw[s]) : 0.0;
      if (first && vj && k < nu) {
        v = v + sh.alphaU[k] * c0raw;
        v = v + (sh.col0raw[k] + sh.alphaU[k] * s00) * aj;
        if (sh.u[k] == j && j < 3) v += A.q;
      }
      bv[s] = v;
    }
    d4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      const int k = 4 * s + ks;
      const double y0 = k < kMaxU ? sh.Y[l16][k] : 0.0;
      const double y1 = k < kMaxU ? sh.Y[16 + l16][k] : 0.0;
      acc0 = mfma_f64(y0, bv[s], acc0);
      acc1 = mfma_f64(y1, bv[s], acc1);
    }
    if (vj && ks == 0) {
      mc[0 * ldk + j] = static_cast<T>(first ? c0raw : 0.0);
      mc[1 * ldk + j] = static_cast<T>(first ? aj : 0.0);
    }
    if (vj) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kr = ks + 4 * r;
        if (kr < jk0 || kr >= jk1) mc[(2 + kr) * ldk + j] = static_cast<T>(acc0[r]);
        if (16 + kr < jk0 || 16 + kr >= jk1) mc[(18 + kr) * ldk + j] = static_cast<T>(acc1[r]);
      }
    }
  };
  // fp64: Σ_in is symmetric, so a row wave's Σ_in[U, i] are also its columns' — one wave per 16
  // indices builds both Kcat rows and Mcat columns (half the waves and half the Σ_in reads of
  // separate row and column waves, the same values)
  constexpr bool merged = sizeof(T) == 8;
  if (wg < row_tiles) {
    const int R0 = wg * 16;
    const int i = R0 + l16;
    const bool vi = i < n;
    const T* rowp = S + static_cast<size_t>(vi ? i : 0) * ld;
    // every gather issued unconditionally (clamped index; padding u = 0 stays in bounds), then
    // masked: a predicated load would be a branch with its own wait, one round trip per load
    T raw[9];
    T r0t;
    if (sizeof(T) == 8) {
      // fp64 Σ is symmetric (the symmetric Σ pass mirrors every element below the diagonal), so
      // Σ_in[i, U] is read as Σ_in[U, i]: 16 consecutive i per row of U (128 B) instead of one
      // scattered element per lane and column of U
      r0t = S[vi ? i : 0];
#pragma unroll
      for (int s = 0; s < 9; ++s)
        raw[s] = S[static_cast<size_t>(sh.u[min(4 * s + ks, kMaxU - 1)]) * ld + (vi ? i : 0)];
    } else {
      r0t = rowp[0];
#pragma unroll
      for (int s = 0; s < 9; ++s) raw[s] = rowp[sh.u[min(4 * s + ks, kMaxU - 1)]];
    }
    const double r0raw = vi ? static_cast<double>(r0t) : 0.0;
    const double ai = first ? alpha_of(i, sh.a1, sh.a2) : 0.0;
    double av[9];
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      const int k = 4 * s + ks;
      double v = (vi && k < nu) ? static_cast<double>(raw[s]) : 0.0;
      if (first && vi && k < nu) {
        v = v + ai * sh.row0raw[k];
        v = v + (r0raw + ai * s00) * sh.alphaU[k];
        if (i == sh.u[k] && i < 3) v += A.q;
      }
      av[s] = v;
    }
    d4 acc[NG], acc2 = {0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = d4{0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      const int k = 4 * s + ks;
      const double zx = (k < kMaxU && l16 == 0) ? sh.Zx[k] : 0.0;
      // Zᵀ·R rather than R·Z: the lane then holds Kcat[c = ks + 4r][i = R0 + l16], so each store
      // covers 4 factor rows × 128 B instead of 16 rows × 32 B (the same products and sums)
#pragma unroll
      for (int g = 0; g < NG; ++g)
        acc[g] = mfma_f64(k < kMaxU ? sh.Z[k][16 * g + l16] : 0.0, av[s], acc[g]);
      acc2 = mfma_f64(zx, av[s], acc2);
    }
    if (vi && ks == 0) {  // the predict's two rank-1 factors (slam.cpp:198)
      kc[0 * ldk + i] = static_cast<T>(first ? -ai : 0.0);
      kc[1 * ldk + i] = static_cast<T>(first ? -(r0raw + ai * s00) : 0.0);
      // rows of U take the chain's x (first position of the row in U)
      int pos = kMaxU;
#pragma unroll
      for (int k = kMaxU - 1; k >= 0; --k) pos = (k < nu && sh.u[k] == i) ? k : pos;
      xout[i] = pos < nu ? xfin[pos] : xin[i] + acc2[0];
    }
    if (vi) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = 16 * g + ks + 4 * r;
          // Joseph: Z columns 0 .. 2m − 1 (the first two groups) are K, which is also the column
          // factor of the (ΣHᵀ − K·S)·Kᵀ term (Mcat rows 2 + 2m + c); columns 32 + c are V, Kcat
          // rows 2 + 2m + c — the rank-(2 + 4m) factors packed, zero columns not stored
          if (!joseph) {
            if (g < 2) kc[(2 + c) * ldk + i] = static_cast<T>(acc[g][r]);
          } else if (g < 2) {
            if (c < jk0) {
              kc[(2 + c) * ldk + i] = static_cast<T>(acc[g][r]);
              mc[(2 + jk0 + c) * ldk + i] = static_cast<T>(acc[g][r]);
            }
          } else if (c - kZC < jk0 + 2) {  // (+ the two zero rows up to kw = 4m + 4: the
            // pass reads them, and a longer chunk before may have left V rows there)
            kc[(2 + jk0 + c - kZC) * ldk + i] = static_cast<T>(acc[g][r]);
          }
        }
    }
    if (merged) columns(i, raw, r0t);
  } else if (!merged && wg < 2 * row_tiles) {
    const int C0 = (wg - row_tiles) * 16;
    const int j = C0 + l16;
    const bool vj = j < n;
    const int jj = vj ? j : 0;
    T raw[9];
    const T c0t = S[jj];
#pragma unroll
    for (int s = 0; s < 9; ++s)
      raw[s] = S[static_cast<size_t>(sh.u[min(4 * s + ks, kMaxU - 1)]) * ld + jj];
    columns(j, raw, c0t);
  }
}

// 16 rows or 16 columns per wave (fp64: both), per_filter workgroups of 4 waves per filter
template <typename T>
__host__ __device__ inline int factor_waves(const PassArgs<T>& a) {
  return (sizeof(T) == 8 ? 1 : 2) * ((a.n + 15) / 16);
}

template <typename T, bool J>
__global__ __launch_bounds__(256) void k_factors(PassArgs<T> A, int xcd_b, int nf) {
  __shared__ FactorSharedT<J> sh;
  // xcd_b = 0: grid (blocks per filter, filters). xcd_b = B > 0 (swarms): the Σ pass's XCD-aware
  // 1-D grid — block L on XCD L % 8 takes filter 8·⌊(L/8)/B⌋ + L % 8, block (L/8) % B — so a
  // filter's record is fetched into one L2 instead of eight. Placement only changes speed.
  int fb = blockIdx.y, bx = blockIdx.x;
  if (xcd_b > 0) {
    const int L = blockIdx.x, j = L >> 3;
    fb = (L & 7) + 8 * (j / xcd_b);
    bx = j % xcd_b;
  }
  // the previous chunk's Σ pass ended before this launch (same stream): its epoch, for the chains
  if (A.pub_sigma && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    epoch_store(A.sync + kSyncSigma, A.pub_sigma);
  if (fb >= nf) return;
  const MsgDesc& d = A.desc[fb];
  if (!(d.flags & kActive)) return;
  const int f = A.f0 + fb;
  const int tid = threadIdx.x;
  const ChunkRec* rec = A.rec + static_cast<size_t>(d.parity) * A.rec_stride + f;
  // the chain of this chunk runs on the other stream: wait for its record
  if (A.polls && tid == 0 && !epoch_wait_acquire(A.sync + kSyncChain + f, A.seq + 1u))
    flag_timeout(&A.ctl[f].status, A.fatal);
  drain_stores();
  __syncthreads();
  factor_record(rec, sh, tid);
  __syncthreads();
  factor_wave<T, J>(A, d, f, bx * (blockDim.x >> 6) + (tid >> 6), sh, tid & 63);
}
template <typename T>
hipError_t launch_factors(const PassArgs<T>& a, int nf, hipStream_t s, hipEvent_t e0,
                          hipEvent_t e1) {
  const int per_filter = (factor_waves(a) + 3) / 4;
  // (the Joseph form's instantiation: Z's 4m columns; a handle's chunks are all of its form)
  auto k = a.joseph ? k_factors<T, true> : k_factors<T, false>;
  if (nf >= 16) {  // XCD-aware 1-D grid, as the swarm's Σ pass
    launch(k, dim3(8 * ((nf + 7) / 8) * per_filter), dim3(256), s, e0, e1, a, per_filter, nf);
  } else {
    launch(k, dim3(per_filter, nf), dim3(256), s, e0, e1, a, 0, nf);
  }
  return hipGetLastError();
}
template hipError_t launch_factors<double>(const PassArgs<double>&, int, hipStream_t, hipEvent_t,
                                           hipEvent_t);
template hipError_t launch_factors<float>(const PassArgs<float>&, int, hipStream_t, hipEvent_t,
                                          hipEvent_t);

}  // namespace ekfslam
