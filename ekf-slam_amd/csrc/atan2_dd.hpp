// atan2 in double-double arithmetic, rounded once: the bearing of a marker for the device planner
// of association replays (plan_assoc.hpp) and for the resident path's replays from device memory
// (stage_replay_block, ekf_resident.hip). The host planner takes its bearings from glibc's atan2,
// which is correctly rounded for all but about one argument in a thousand; ocml's on the device
// differs from it in the last bit far more often, and the landmark prior's
// 1e7 − (1e7 − δ) (slam.cpp:130) amplifies each such bit to ≈ 1e-9 on the state. Rounding an
// atan2 that is good to ≈ 2^-100 gives the correctly rounded value (short of a tie nobody will
// meet), so a device plan's bearings are the host plan's wherever glibc rounds correctly.
//
// t = min(|x|, |y|) / max(|x|, |y|) ∈ [0, 1]; θ_k = k/64 the table angle nearest atan(t); the point
// (max, min) rotated by −θ_k with sin θ_k, cos θ_k as double-double pairs (tools/gen_sincos_dd.py);
// τ = Y/X, |τ| ≤ 0.008, as a pair; atan τ = τ − τ³/3 + … with the tail (≤ 1.7e-7·τ) in plain
// doubles; the octant folded back with π and π/2 as pairs. Every product whose rounding error
// matters goes through fma and no other is contracted, so the host compiler and the device agree.
// Plain C++ with <math.h>: host compiler or hipcc.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EKF_DD_HD __host__ __device__
#else
#define EKF_DD_HD
#endif
// First statement of every function here: no product may be fused into a neighbouring sum. The
// error-free sums assume s = fl(a + b); a helper inlined next to a product would otherwise hand
// the compiler an a·b + c to contract (the device build contracts by default).
#if defined(__clang__)
#define EKF_DD_EXACT _Pragma("clang fp contract(off)")
#else
#define EKF_DD_EXACT
#endif

namespace ekfslam {
namespace dd {

struct Pair {
  double hi, lo;
};

EKF_DD_HD inline Pair two_sum(double a, double b) {
  EKF_DD_EXACT
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
EKF_DD_HD inline Pair quick_two_sum(double a, double b) {  // |a| ≥ |b|
  EKF_DD_EXACT
  const double s = a + b;
  return {s, b - (s - a)};
}
EKF_DD_HD inline Pair two_prod(double a, double b) {
  EKF_DD_EXACT
  const double p = a * b;
  return {p, fma(a, b, -p)};
}
EKF_DD_HD inline Pair add(Pair a, Pair b) {
  EKF_DD_EXACT
  Pair s = two_sum(a.hi, b.hi);
  const Pair t = two_sum(a.lo, b.lo);
  s = quick_two_sum(s.hi, s.lo + t.hi);
  return quick_two_sum(s.hi, s.lo + t.lo);
}
EKF_DD_HD inline Pair neg(Pair a) { return {-a.hi, -a.lo}; }
EKF_DD_HD inline Pair mul(double a, Pair b) {  // a·b
  EKF_DD_EXACT
  Pair p = two_prod(a, b.hi);
  p.lo = fma(a, b.lo, p.lo);
  return quick_two_sum(p.hi, p.lo);
}
EKF_DD_HD inline Pair div(Pair a, Pair b) {
  EKF_DD_EXACT
  const double q1 = a.hi / b.hi;
  const Pair r = add(a, neg(mul(q1, b)));
  const double q2 = r.hi / b.hi;
  const Pair r2 = add(r, neg(mul(q2, b)));
  const double q3 = r2.hi / b.hi;
  const Pair q = quick_two_sum(q1, q2);
  return add(q, Pair{q3, 0.0});
}

}  // namespace dd

EKF_DD_HD inline double atan2_rounded(double y, double x) {
  EKF_DD_EXACT
  // sin(k/64), cos(k/64) as (hi, lo) pairs, k = 0..51 (51/64 > π/4)
  constexpr double kSinCos[52][4] = {
      {0x0.0p+0, 0x0.0p+0, 0x1.0000000000000p+0, 0x0.0p+0},
      {0x1.fffaaaaeeeed5p-7, -0x1.2ab639a9f0776p-63, 0x1.fff000155549fp-1, 0x1.28a28a03a5ef3p-55},
      {0x1.ffeaaaeeee86fp-6, -0x1.cd406fb224ae2p-60, 0x1.ffc00155527d3p-1, -0x1.3b54492d89b5bp-55},
      {0x1.7fdc01032fba9p-5, -0x1.599bdf46e997ap-59, 0x1.ff7006bfdf99fp-1, -0x1.8b3b560648d5fp-56},
      {0x1.ffaaaeeed4edbp-5, -0x1.2d16d32684b69p-59, 0x1.ff0015549f4d3p-1, 0x1.328387b99426fp-55},
      {0x1.3facb12d1755bp-4, -0x1.921915299468bp-58, 0x1.fe7034129ef6fp-1, -0x1.cbf4337c96f97p-57},
      {0x1.7f701032550e4p-4, 0x1.afc2d1800501ap-60, 0x1.fdc06bf7e6b9bp-1, 0x1.31902b535f8dbp-55},
      {0x1.bf1b78568391dp-4, 0x1.e91841dea4cc8p-58, 0x1.fcf0c800e99b1p-1, 0x1.ea3d786d186acp-57},
      {0x1.feaaeee86ee36p-4, -0x1.afcb2bcc6f03bp-59, 0x1.fc015527d5bd3p-1, 0x1.b68f35094efb8p-55},
      {0x1.1f0d3d7afceafp-3, -0x1.6ef95099769a5p-57, 0x1.faf22263c4bd3p-1, -0x1.52ace133a2769p-58},
      {0x1.3eb312c5d66cbp-3, 0x1.47d666b66cb91p-57, 0x1.f9c340a7cc428p-1, 0x1.c5b6b063b7462p-55},
      {0x1.5e44fcfa126f3p-3, -0x1.6f443063f89b6p-57, 0x1.f874c2e1eecf6p-1, -0x1.c6514e1332b16p-55},
      {0x1.7dc102fbaf2b5p-3, 0x1.5ab50e23c97c3p-59, 0x1.f706bdf9ece1cp-1, -0x1.698c80c36dcb4p-55},
      {0x1.9d252d0cec312p-3, 0x1.9c43d80b1137dp-58, 0x1.f57948cff6797p-1, 0x1.e3a0d3e03b1d4p-57},
      {0x1.bc6f84edc6199p-3, 0x1.9c1a56a7b0cabp-57, 0x1.f3cc7c3b3d16ep-1, -0x1.21a3ad28a3494p-57},
      {0x1.db9e15fb5a5d0p-3, -0x1.32e20d6cc6fc2p-57, 0x1.f20073086649fp-1, 0x1.b940416c1984bp-56},
      {0x1.faaeed4f31577p-3, -0x1.15d88508e32b8p-57, 0x1.f01549f7deea1p-1, 0x1.d3c1e99e5cafdp-55},
      {0x1.0cd00cef36436p-2, -0x1.9fb0a0c93e2b4p-56, 0x1.ee0b1fbc0f11cp-1, -0x1.bfd2380bbc3b1p-59},
      {0x1.1c37d64c6b876p-2, 0x1.46076fe0dcff4p-56, 0x1.ebe214f76efa8p-1, -0x1.02f9f12ba543ep-55},
      {0x1.2b8ddc43eb49fp-2, 0x1.1553899f2d807p-57, 0x1.e99a4c3a7cd83p-1, -0x1.2264b1bc53ce8p-55},
      {0x1.3ad129769d3d8p-2, 0x1.03d550487839ap-63, 0x1.e733ea0193d40p-1, -0x1.6428b3546ce13p-55},
      {0x1.4a00c9b0f3d20p-2, 0x1.823ba6bb08eadp-56, 0x1.e4af14b2a449cp-1, -0x1.68ca02e8a6833p-55},
      {0x1.591bc9fa2f597p-2, 0x1.7c74bac3fe0cbp-57, 0x1.e20bf49acd6c1p-1, -0x1.660aec7ef636bp-58},
      {0x1.682138a38d7f7p-2, -0x1.d889202444aadp-56, 0x1.df4ab3ebd875ep-1, -0x1.e2d8a7e6736c4p-55},
      {0x1.7710255764214p-2, -0x1.6ead7314bb6cep-57, 0x1.dc6b7eb995912p-1, 0x1.4b364776dcd35p-58},
      {0x1.85e7a12826949p-2, 0x1.8a40e9b5face0p-56, 0x1.d96e82f71a9dcp-1, 0x1.ff61bd5d2039dp-55},
      {0x1.94a6be9f546c5p-2, -0x1.69ce13e683f58p-56, 0x1.d653f073e4040p-1, -0x1.76236434bec37p-55},
      {0x1.a34c91cc50ccap-2, -0x1.a310e3b50cecdp-58, 0x1.d31bf8d8d7c06p-1, 0x1.e60dd3089cbddp-56},
      {0x1.b1d8305321617p-2, -0x1.ae242cb99f519p-56, 0x1.cfc6cfa52ad9fp-1, 0x1.8b5b5508f2a0dp-55},
      {0x1.c048b17b140a3p-2, 0x1.19fe6757e9fa7p-57, 0x1.cc54aa2b2972ep-1, 0x1.4ee162ba83a98p-57},
      {0x1.ce9d2e3d4a51fp-2, -0x1.2fc8a12dae298p-57, 0x1.c8c5bf8ce1a84p-1, 0x1.ab3d1a1590123p-56},
      {0x1.dcd4c15329c9ap-2, 0x1.0d4c6e171fd9ap-56, 0x1.c51a48b8b175ep-1, -0x1.1bbb43b9aa880p-57},
      {0x1.eaee8744b05f0p-2, -0x1.789b43c9b027dp-58, 0x1.c1528065b7d50p-1, -0x1.892111312e828p-55},
      {0x1.f8e99e76abc97p-2, 0x1.9d950af2d00a3p-58, 0x1.bd6ea310294f5p-1, 0x1.31bbcc88c109dp-56},
      {0x1.0362939c69955p-1, -0x1.2d8cd78397b01p-55, 0x1.b96eeef58840ep-1, 0x1.45a3cc78fade0p-58},
      {0x1.0a4021e9e1001p-1, -0x1.6f643a13914f6p-55, 0x1.b553a410c104ep-1, 0x1.8ff7947027a15p-58},
      {0x1.110d0c4b69c3bp-1, 0x1.d918998809981p-55, 0x1.b11d04162a4c6p-1, 0x1.1dd561efbc0c2p-56},
      {0x1.17c8e5f2eedb0p-1, 0x1.35e57102e2488p-57, 0x1.accb526f69de5p-1, 0x1.8fb6a8dd6b6ccp-55},
      {0x1.1e7343236574cp-1, 0x1.22a3fa4f41d5ap-56, 0x1.a85ed4373e02dp-1, 0x1.9be06385ec792p-57},
      {0x1.250bb93788bbbp-1, 0x1.ea3d02457bccep-56, 0x1.a3d7d0352bdcfp-1, -0x1.68dbaeca19669p-55},
      {0x1.2b91dea88421ep-1, -0x1.fa371db216ab0p-55, 0x1.9f368ed912f85p-1, -0x1.1d200c5791606p-55},
      {0x1.32054b148bc4fp-1, 0x1.f6b42095a135bp-55, 0x1.9a7b5a36a6514p-1, 0x1.722cfcc9fa7a9p-55},
      {0x1.386597456282bp-1, -0x1.10fada93b07a8p-56, 0x1.95a67e00cb1fdp-1, -0x1.0befda21f862dp-55},
      {0x1.3eb25d36cd53ap-1, -0x1.be570e1570fc0p-58, 0x1.90b84784ddaf7p-1, -0x1.0feb10ab93b87p-56},
      {0x1.44eb381cf386bp-1, -0x1.3ed6c1e6a5505p-55, 0x1.8bb105a5dc900p-1, 0x1.863e03e9474c1p-55},
      {0x1.4b0fc46aab761p-1, 0x1.0da05738cc59cp-61, 0x1.869108d77a6c6p-1, 0x1.338ffe2bfe9ddp-56},
      {0x1.511f9fd7b351cp-1, -0x1.5c0e861c48831p-55, 0x1.8158a31916d5dp-1, -0x1.de8b90b8228dep-57},
      {0x1.571a6966d59b3p-1, 0x1.c843b4d0fb197p-58, 0x1.7c0827f09e54fp-1, -0x1.c73d6d72aee68p-57},
      {0x1.5cffc16bf8f0dp-1, 0x1.96cb370eb578ap-55, 0x1.769fec655211fp-1, -0x1.827d5cf8c68c5p-57},
      {0x1.62cf49921ac79p-1, -0x1.edd9855b6241ap-55, 0x1.712046fa77678p-1, 0x1.425b0a5029c81p-55},
      {0x1.6888a4e134b2fp-1, -0x1.6b7d37644d5e6p-55, 0x1.6b898fa9efb5dp-1, 0x1.15ac786ccf4b2p-56},
      {0x1.6e2b77c40bde1p-1, -0x1.0e729857fad53p-56, 0x1.65dc1fdeb8cbap-1, -0x1.97c1b47337c77p-58},
  };
  constexpr dd::Pair kPi{0x1.921fb54442d18p+1, 0x1.1a62633145c07p-53};
  constexpr dd::Pair kHalfPi{0x1.921fb54442d18p+0, 0x1.1a62633145c07p-54};
  const double ax = fabs(x), ay = fabs(y);
  const bool swap = ay > ax;
  const double mn = swap ? ax : ay, mx = swap ? ay : ax;
  // zeros, infinities, NaNs and ratios beyond the pairs' exponent range: libm's own cases
  if (!(mx > 0x1p-900) || !(mx < 0x1p+900) || !(mn > mx * 0x1p-100)) return atan2(y, x);
  int k = static_cast<int>(64.0 * atan2(mn, mx) + 0.5);
  k = k < 0 ? 0 : (k > 51 ? 51 : k);
  const dd::Pair s{kSinCos[k][0], kSinCos[k][1]}, c{kSinCos[k][2], kSinCos[k][3]};
  const dd::Pair X = dd::add(dd::mul(mx, c), dd::mul(mn, s));
  const dd::Pair Y = dd::add(dd::mul(mn, c), dd::neg(dd::mul(mx, s)));
  const dd::Pair tau = dd::div(Y, X);
  const double t = tau.hi, z = t * t;
  // atan τ − τ = τ³·(−1/3 + z/5 − z²/7 + z³/9 − z⁴/11 + z⁵/13)
  const double p = -1.0 / 3.0 + z * (1.0 / 5.0 + z * (-1.0 / 7.0 + z * (1.0 / 9.0 +
                   z * (-1.0 / 11.0 + z * (1.0 / 13.0)))));
  dd::Pair a = dd::add(dd::Pair{static_cast<double>(k) / 64.0, 0.0},
                       dd::add(tau, dd::Pair{t * z * p, 0.0}));
  if (swap) a = dd::add(kHalfPi, dd::neg(a));
  if (x < 0.0) a = dd::add(kPi, dd::neg(a));
  return copysign(a.hi, y);
}

}  // namespace ekfslam
