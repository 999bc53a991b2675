// Phase stamps of the diagnostic library (make diag: EKF_DIAG_STAMPS, libekfslam_diag.so); in the
// product library every macro here is empty. A macro writes into a __device__ buffer that the one
// translation unit using it defines (with the reader the tools call): g_stamps and g_blocks in
// ekf_chain.hip, g_sig_stamps in ekf_sigma_pass.hip.
#pragma once

#ifdef EKF_DIAG_STAMPS
// tools/chain_stamps.py: s_memtime stamps of k_chain's block (0,0), thread 0 (or t), in a ring of
// the last four chunks (by seq & 3).
#define EKF_STAMP(i)                                                              \
  do {                                                                            \
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)                   \
      g_stamps[512 * (seq & 3) + (i)] = __builtin_amdgcn_s_memtime();             \
  } while (0)
#define EKF_STAMPT(i, t)                                                          \
  do {                                                                            \
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == (t))                 \
      g_stamps[512 * (seq & 3) + (i)] = __builtin_amdgcn_s_memtime();             \
  } while (0)
#define EKF_STAMPV(i, v)                                                          \
  do {                                                                            \
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)                   \
      g_stamps[512 * (seq & 3) + (i)] = (v);                                      \
  } while (0)
// one stamp per wave, by its lane 0: slot i + the wave's index
#define EKF_STAMPW(i)                                                             \
  do {                                                                            \
    if (blockIdx.x == 0 && blockIdx.y == 0 && (threadIdx.x & 63) == 0)            \
      g_stamps[512 * (seq & 3) + (i) + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
// tools/diag_blocks.py: filter 0's chain block Σ[U, U] and x[U] as the corrections start (predict
// folded in), per chunk sequence number mod 64.
#define EKF_DUMP_BLOCK(seq)                                                         \
  do {                                                                              \
    __syncthreads();                                                                \
    if (blockIdx.y == 0) {                                                          \
      for (int e = threadIdx.x; e < kMaxU * (kMaxU + 1); e += blockDim.x)           \
        (&g_blocks[(seq) & 63][0][0])[e] = (&P[0][0])[e];                             \
      if (threadIdx.x < kMaxU) g_blockx[(seq) & 63][threadIdx.x] = sh.xU[0][threadIdx.x]; \
    }                                                                               \
    __syncthreads();                                                                \
  } while (0)
// tools/sigma_bench.hip: s_memrealtime (100 MHz) per Σ-pass workgroup.
#define SIG_STAMP(i)                                                                   \
  do {                                                                                 \
    if (threadIdx.x == 0 && blockIdx.y == 0 && blockIdx.x < 4096) {                    \
      g_sig_stamps[blockIdx.x][i] = __builtin_amdgcn_s_memrealtime();                  \
      if (i == 0)                                                                      \
        g_sig_stamps[blockIdx.x][4] =                                                  \
            (static_cast<unsigned long long>(__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (15 << 11))) << 32) | \
            __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));                \
    }                                                                                  \
  } while (0)
#else
#define EKF_STAMP(i) \
  do {               \
  } while (0)
#define EKF_STAMPT(i, t) \
  do {                   \
  } while (0)
#define EKF_STAMPV(i, v) \
  do {                   \
  } while (0)
#define EKF_STAMPW(i) \
  do {                \
  } while (0)
#define EKF_DUMP_BLOCK(seq) \
  do {                      \
  } while (0)
#define SIG_STAMP(i) \
  do {               \
  } while (0)
#endif
