// ekf_copy_state (gfx950 / CDNA4): a filter's state from one handle into another on the device, an
// HBM-bound copy-and-convert over 64 × 64 tiles of the destination Σ.
//
// The padded source S'(a, b), a and b below the destination's n: the source element widened to
// fp64 where both are below the source's n, the destination's prior on the new diagonal entries,
// 0 everywhere else (so every column n..ld of the destination gets 0). Destination element (i, j):
//   straight tiles (fp32 and resident destinations)   S'(i, j)
//   SYM tiles (fp64 pipeline destinations)            S'(i, j) for i <= j, S'(j, i) below the
//     diagonal: the Σ pass relies on exact symmetry (ekf_set_state's rule, ekf_api.cpp).
// A tile below the diagonal therefore reads the source's transposed tile, row-major like any other,
// and transposes it through LDS; a diagonal tile selects (j, i) for i > j out of LDS.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ekf_device.hpp"
#include "ekf_launch.hpp"

namespace ekfslam {

namespace {

constexpr int kTile = kCopyTile;
// LDS row pitch in doubles: one 8-byte access width of padding. A transposed 8-byte read has lane l
// of a 32-lane group at double (c + l)·65 + r or, for the pair mapping below, at
// (c + 2·(l & 15))·65 + r + (l >> 4): the 8-byte slot (address mod 32) is l + const resp.
// 2·(l & 15) + (l >> 4) + const, 32 different slots either way (ds_read_b64 banks 64 dwords over
// each 32-lane half).
constexpr int kPitch = kTile + 1;

// E consecutive source elements from p (16-byte loads wherever E elements are 16 bytes or more)
template <typename Ts, int E>
__device__ __forceinline__ void load_run(const Ts* p, double (&v)[E]) {
  if constexpr (std::is_same<Ts, double>::value) {
#pragma unroll
    for (int e = 0; e < E; e += 2) {
      const double2 t = *reinterpret_cast<const double2*>(p + e);
      v[e] = t.x;
      v[e + 1] = t.y;
    }
  } else if constexpr (E == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x;
    v[1] = t.y;
    v[2] = t.z;
    v[3] = t.w;
  } else {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x;
    v[1] = t.y;
  }
}

// S'(a, b .. b + E − 1); b is a multiple of E, so a run that starts inside a source row ends inside
// its ld (a multiple of 16 elements).
template <typename Ts, int E>
__device__ __forceinline__ void padded_run(const CopyArgs& A, const Ts* src, int a, int b,
                                           double (&v)[E]) {
  const bool in = a < A.n_src && b < A.n_src;
  if (in) load_run<Ts, E>(src + static_cast<size_t>(a) * A.ld_src + b, v);
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (!in || b + e >= A.n_src) v[e] = (a == b + e && a >= A.n_src && a < A.n_dst) ? A.prior : 0.0;
}

template <typename Td, int E>
__device__ __forceinline__ void store_run(Td* p, const double (&v)[E]) {
  if constexpr (std::is_same<Td, double>::value) {
#pragma unroll
    for (int e = 0; e < E; e += 2) *reinterpret_cast<double2*>(p + e) = double2{v[e], v[e + 1]};
  } else {
    static_assert(E == 4, "an fp32 destination stores four elements, 16 bytes");
    *reinterpret_cast<float4*>(p) =
        float4{static_cast<float>(v[0]), static_cast<float>(v[1]), static_cast<float>(v[2]),
               static_cast<float>(v[3])};
  }
}

// x (n of the destination, the grown part 0), t_map_odom and the counter of one filter. The status
// word behind the counter, the decisions and the chain's counters stay as they are.
__device__ __forceinline__ void copy_small(const CopyArgs& A, int fs, int fd, int ps, int pd) {
  const double* xs = A.src_x[ps] + fs * A.src_x_stride;
  double* xd = A.dst_x[pd] + fd * A.dst_x_stride;
  for (int i = threadIdx.x; i < A.n_dst; i += blockDim.x) xd[i] = i < A.n_src ? xs[i] : 0.0;
  if (threadIdx.x == 0) {
    const FilterCtl* cs = A.src_ctl + fs;
    FilterCtl* cd = A.dst_ctl + fd;
    *reinterpret_cast<double2*>(cd->tmo) = *reinterpret_cast<const double2*>(cs->tmo);
    cd->tmo[2] = cs->tmo[2];
    cd->counter = cs->counter;
  }
}

}  // namespace

// Grid (tile column, tile row, block of destination filters), 256 threads. A workgroup builds its
// tile of S' once, in registers (16 fp64 values per thread), and stores it to each destination
// filter of its block: a fork reads Σ once per block of fpb filters, the other forms have fpb = 1.
template <typename Ts, typename Td, bool SYM>
__global__ __launch_bounds__(256) void k_copy_state(CopyArgs A) {
  const int tj = blockIdx.x, ti = blockIdx.y, t = threadIdx.x;
  const int k_lo = blockIdx.z * A.fpb, k_hi = min(k_lo + A.fpb, A.nf);
  // (the swarm form: fpb = 1, filter f from filter f)
  const int fs = A.src_f >= 0 ? A.src_f : A.dst_f0 + k_lo;
  const int ps = A.src_par[fs];
  const Ts* src = static_cast<const Ts*>(A.src_sig[ps]) + fs * A.src_sig_stride;
  // the run of E elements a thread holds per step, and its place in the tile. Straight: four
  // elements (one 16-byte store in fp32, two in fp64), 16 runs a row, 16 rows a step. SYM: a pair
  // (Td is double: 16 bytes); lanes l and l + 16 hold the same columns of two adjacent rows, so
  // that the transposed reads below fall on 32 different LDS slots.
  constexpr int E = SYM ? 2 : 4, STEPS = 16 / E;
  static_assert(!SYM || std::is_same<Td, double>::value, "SYM: fp64 pipeline destinations");
  int c, r0, dr;
  if constexpr (SYM) {
    const int l = t & 63;
    c = 2 * ((l & 15) + 16 * (l >> 5));
    r0 = 2 * (t >> 6) + ((l >> 4) & 1);
    dr = 8;
  } else {
    c = 4 * (t & 15);
    r0 = t >> 4;
    dr = 16;
  }
  // SYM below the diagonal: the source's tile (tj, ti), transposed on the way out
  const bool flip = SYM && ti > tj;
  const int R0 = (flip ? tj : ti) * kTile, C0 = (flip ? ti : tj) * kTile;
  double v[STEPS][E];
  // (a tile that lies wholly in the grown region reads nothing: padded_run's test is uniform there)
#pragma unroll
  for (int s = 0; s < STEPS; ++s) padded_run<Ts, E>(A, src, R0 + r0 + s * dr, C0 + c, v[s]);
  if constexpr (SYM) {
    if (ti >= tj) {  // (uniform over the workgroup)
      __shared__ double tile[kTile * kPitch];
#pragma unroll
      for (int s = 0; s < STEPS; ++s) {
        tile[(r0 + s * dr) * kPitch + c] = v[s][0];
        tile[(r0 + s * dr) * kPitch + c + 1] = v[s][1];
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < STEPS; ++s) {
        const int r = r0 + s * dr;
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (flip || r > c + e) v[s][e] = tile[(c + e) * kPitch + r];
      }
    }
  }
  const int i0 = ti * kTile + r0, j = tj * kTile + c;
  for (int k = k_lo; k < k_hi; ++k) {
    const int fd = A.dst_f0 + k;
    if (fd == A.skip) continue;  // a filter onto itself: untouched
    const int pd = A.dst_par[fd];
    Td* dst = static_cast<Td*>(A.dst_sig[pd]) + fd * A.dst_sig_stride;
    if (j < A.ld_dst) {
#pragma unroll
      for (int s = 0; s < STEPS; ++s) {
        const int i = i0 + s * dr;
        if (i < A.n_dst) store_run<Td, E>(dst + static_cast<size_t>(i) * A.ld_dst + j, v[s]);
      }
    }
    if (ti == 0 && tj == 0) copy_small(A, fs, fd, ps, pd);
  }
}

namespace {

template <typename Ts, typename Td, bool SYM>
hipError_t launch_one(const CopyArgs& a, hipStream_t s) {
  const dim3 grid((a.ld_dst + kTile - 1) / kTile, (a.n_dst + kTile - 1) / kTile,
                  (a.nf + a.fpb - 1) / a.fpb);
  hipLaunchKernelGGL((k_copy_state<Ts, Td, SYM>), grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_copy_state(const CopyArgs& a, bool src_f32, bool dst_f32, bool sym,
                             hipStream_t s) {
  if (a.nf < 1 || a.fpb < 1 || (sym && dst_f32) || (a.src_f < 0 && a.fpb != 1) ||
      (a.nf + a.fpb - 1) / a.fpb > 65535 || a.n_dst < a.n_src)
    return hipErrorInvalidValue;
  if (dst_f32)
    return src_f32 ? launch_one<float, float, false>(a, s) : launch_one<double, float, false>(a, s);
  if (sym)
    return src_f32 ? launch_one<float, double, true>(a, s) : launch_one<double, double, true>(a, s);
  return src_f32 ? launch_one<float, double, false>(a, s) : launch_one<double, double, false>(a, s);
}

}  // namespace ekfslam
