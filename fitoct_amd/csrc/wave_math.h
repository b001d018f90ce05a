// Device-resident NUTS, layer 3: one wave's arithmetic.  Cross-lane sums of doubles without
// LDS (DPP row operations, gfx950 permlane swaps), fma_v / fexp / frcp, the extended-range
// weights XF of the multinomial merges, and the Philox normal pair.
// Part of the sampler's one translation unit (nuts_device.hip includes the layers in order).
// All of it lives in namespace fitoct, which dev_common.h opens and only nuts_device.hip
// closes: parsed on its own, this header ends inside the open namespace.
#pragma once
#include "dev_common.h"

// ---------------------------------------------------------------------------
// cross-lane moves of doubles without LDS (DPP row ops, gfx950 permlane swaps)
// ---------------------------------------------------------------------------
constexpr int DPP_XOR1 = 0xB1;         // quad_perm(1,0,3,2)
constexpr int DPP_XOR2 = 0x4E;         // quad_perm(2,3,0,1)
constexpr int DPP_QREV = 0x1B;         // quad_perm(3,2,1,0): flip bits 0,1
constexpr int DPP_HALF_MIRROR = 0x141; // lane i <-> 7-i within 8: flip bits 0..2
constexpr int DPP_MIRROR = 0x140;      // lane i <-> 15-i within 16: flip bits 0..3

// (bound_ctrl: a disabled source lane reads 0, as the zero 'old' operand of update_dpp
// gave, without a v_mov of that zero before every DPP move)
template <int CTRL>
__device__ __forceinline__ double dpp(double x) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
// v_readlane of a double (lane index wave-uniform)
__device__ __forceinline__ double rl(double x, int l) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, l);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), l);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// a' = a with rows {1,3} (lanes 16-31, 48-63) replaced by b's rows {0,2};
// b' = b with rows {0,2} replaced by a's rows {1,3}.  Returns a' + b'.
__device__ __forceinline__ double swap16_add(double a, double b) {
  const uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
  const auto lo = __builtin_amdgcn_permlane16_swap((uint32_t)ua, (uint32_t)ub, false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((uint32_t)(ua >> 32), (uint32_t)(ub >> 32), false, false);
  const double a2 = __builtin_bit_cast(double, ((uint64_t)hi[0] << 32) | lo[0]);
  const double b2 = __builtin_bit_cast(double, ((uint64_t)hi[1] << 32) | lo[1]);
  return a2 + b2;
}
// same across the two 32-lane halves; b2: the swapped b, dead after the sum
__device__ __forceinline__ double swap32_add(double a, double b, double& b2) {
  const uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
  const auto lo = __builtin_amdgcn_permlane32_swap((uint32_t)ua, (uint32_t)ub, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((uint32_t)(ua >> 32), (uint32_t)(ub >> 32), false, false);
  const double a2 = __builtin_bit_cast(double, ((uint64_t)hi[0] << 32) | lo[0]);
  b2 = __builtin_bit_cast(double, ((uint64_t)hi[1] << 32) | lo[1]);
  return a2 + b2;
}
__device__ __forceinline__ double swap32_add(double a, double b) {
  double b2;
  return swap32_add(a, b, b2);
}

// butterfly sum over the wave; every lane ends with the bitwise-identical value
__device__ __forceinline__ double wave_sum(double x) {
  x += dpp<DPP_XOR1>(x);
  x += dpp<DPP_XOR2>(x);
  x += dpp<DPP_HALF_MIRROR>(x);
  x += dpp<DPP_MIRROR>(x);
  x = swap16_add(x, x);
  return swap32_add(x, x);
}
__device__ __forceinline__ void wave_sum2(double& a, double& b) {
  a += dpp<DPP_XOR1>(a);
  b += dpp<DPP_XOR1>(b);
  a += dpp<DPP_XOR2>(a);
  b += dpp<DPP_XOR2>(b);
  a += dpp<DPP_HALF_MIRROR>(a);
  b += dpp<DPP_HALF_MIRROR>(b);
  a += dpp<DPP_MIRROR>(a);
  b += dpp<DPP_MIRROR>(b);
  a = swap16_add(a, a);
  b = swap16_add(b, b);
  a = swap32_add(a, a);
  b = swap32_add(b, b);
}

// N independent butterfly sums, stage by stage (the DPP / permlane moves of the
// N values overlap instead of serialising N reductions)
template <int N>
__device__ __forceinline__ void wave_sum_n(double (&x)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] += dpp<DPP_XOR1>(x[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] += dpp<DPP_XOR2>(x[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] += dpp<DPP_HALF_MIRROR>(x[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] += dpp<DPP_MIRROR>(x[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = swap16_add(x[i], x[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = swap32_add(x[i], x[i]);
}

// exp on the sampler side: reduction by ln2 (hi/lo), Taylor degree 12 on
// |r| <= ln2/2, n = round(x log2 e) from the 1.5*2^52 shifter fed straight to
// v_ldexp_f64 (<= 2 ulp from the library exp, scripts/micro/acc.hip; no special
// cases: x is clamped to [-746, 710], where exp is 0 / inf either way).
// v_fma_f64 with all three operands in VGPRs.  In the sampler's code the compiler keeps
// fexp's coefficients in VGPRs (its SGPRs are spent) and forms p * r + c as a copy of c into
// the destination plus a v_fmac_f64: two VALU instructions per Horner step.  Same operation.
// Every sampler uses it (the migrating ones too since write_mp's single exp freed their
// registers; round 3 had to leave them out: profiles/r03_ab_fmav.txt).  The addend in an SGPR
// pair instead costs the migrating kernels 23-29 more spilled SGPRs for the same speed
// (profiles/r07_ab_sampler_valu.txt).
__device__ __forceinline__ double fma_v(double a, double b, double c) {
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ double fexp(double x) {
  x = fmin(fmax(x, -746.0), 710.0);
  const double SH = 6755399441055744.0;   // 1.5 * 2^52
  const double t = fma(x, 1.4426950408889634, SH);
  const double n = t - SH;
  const int ni = (int)(uint32_t)__builtin_bit_cast(uint64_t, t);
  double r = fma(-n, 6.93147180369123816490e-01, x);
  r = fma(-n, 1.90821492927058770002e-10, r);
  double p = 2.08767569878680989792e-09;   // 1/12!
  p = fma_v(p, r, 2.50521083854417187751e-08);
  p = fma_v(p, r, 2.75573192239858906526e-07);
  p = fma_v(p, r, 2.75573192239858906526e-06);
  p = fma_v(p, r, 2.48015873015873015873e-05);
  p = fma_v(p, r, 1.98412698412698412698e-04);
  p = fma_v(p, r, 1.38888888888888888889e-03);
  p = fma_v(p, r, 8.33333333333333333333e-03);
  p = fma_v(p, r, 4.16666666666666666667e-02);
  p = fma_v(p, r, 1.66666666666666666667e-01);
  p = fma_v(p, r, 0.5);
  p = fma_v(p, r, 1.0);
  p = fma_v(p, r, 1.0);
  return ldexp(p, ni);
}
// 1/x to <= 1 ulp: v_rcp_f64 and one Newton step (x finite, nonzero)
__device__ __forceinline__ double frcp(double x) {
  const double r = __builtin_amdgcn_rcp(x);
  return fma(r, fma(-x, r, 1.0), r);
}

// Multinomial trajectory weights exp(H0 - H) as extended-exponent floats
// m * 2^e (m in [1/2, 1) or 0): the merges of base_nuts (log_sum_exp of log
// weights, then u < exp(lsw_final - lsw_subtree)) become an add and a multiply,
// with no exp / log1p per merge and no overflow for any energy change.  The
// oracle (oracle/fitoct_oracle.c) uses the same representation.
struct XF {
  double m;
  int e;
};
__device__ __forceinline__ XF xf_norm(double m, int e) {
  int k;
  const double f = frexp(m, &k);
  return XF{f, f == 0.0 ? 0 : e + k};
}
__device__ __forceinline__ XF xf_exp(double x) {   // exp(x), x <= +inf; -inf -> 0
  if (x > -700.0 && x < 700.0) return xf_norm(fexp(x), 0);
  // above 1e8 (an energy drop no trajectory of a finite start reaches) the weight
  // saturates: the exponent stays within int, and so does the exponent difference of
  // two weights in xf_u_below (>= -1.45e9 - 1.45e8)
  if (!(x < 1.0e8)) x = 1.0e8;
  // below -1e9 (a divergent leaf: its weight is never merged) the exponent would not fit
  // an int; the weight is 0 to every digit the merges can resolve
  if (!(x > -1.0e9)) return XF{0.0, 0};
  const double k = floor(x * 1.4426950408889634);   // log2(e)
  return xf_norm(fexp(fma(-k, 0.6931471805599453, x)), (int)k);
}
__device__ __forceinline__ XF xf_add(XF a, XF b) {
  if (a.m == 0.0) return b;
  if (b.m == 0.0) return a;
  const int e = a.e > b.e ? a.e : b.e;
  return xf_norm(ldexp(a.m, a.e - e) + ldexp(b.m, b.e - e), e);
}
__device__ __forceinline__ bool xf_gt(XF a, XF b) {   // a > b (both >= 0)
  if (a.m == 0.0) return false;
  if (b.m == 0.0) return true;
  return a.e != b.e ? a.e > b.e : a.m > b.m;
}
__device__ __forceinline__ bool xf_u_below(double u, XF a, XF b) {   // u < a / b
  if (b.m == 0.0) return false;   // Stan: u < exp(-inf - -inf) = NaN is false
  return ldexp(u * b.m, b.e - a.e) < a.m;
}
__device__ __forceinline__ double xf_val(XF a) { return ldexp(a.m, a.e); }


__device__ __forceinline__ void normal_pair(RngKey k, uint32_t c0, uint32_t c1, uint32_t c2,
                                            uint32_t c3, double& n0, double& n1) {
  U4 c = {c0, c1, c2, c3};
  U4 r = philox4x32_10(c, k.k0, k.k1);
  const double u1 = u53(r.x, r.y), u2 = u53(r.z, r.w);
  const double rad = sqrt(-2.0 * log(1.0 - u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);   // angle 2*pi*u2; sinpi/cospi need no Payne-Hanek reduction
  n0 = rad * cs;
  n1 = rad * sn;
}
