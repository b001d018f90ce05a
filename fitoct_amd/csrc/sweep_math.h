// Device-resident NUTS, layer 4: the likelihood sweep's per-bin arithmetic.
//   * gradient waves: the N depth bins are strided over 256 lanes; each lane
//     keeps its bins' data resident in VGPRs for the whole run (read from HBM
//     once per tile, shared by all G chains; up to 8 bins per lane, or 16 in
//     the compact layout for arithmetic depth grids).  For the
//     built-in uniform-grid SE basis (MODE_POLY) the GP basis factorises as
//     K(x~_i, g_l) = a_i t_i^l b_l, so a bin needs 5 registers (c*x, y, 1/uy,
//     t, a) instead of a 16-wide basis row: dL_i = a_i P(t_i) by Horner on the
//     chain's coefficients c = b .* K^-1 yGP, and B^T h = K^-1 (b .* M) from
//     the moments M_l = sum_i h_i a_i t_i^l.  A user-supplied basis keeps its
//     rows in registers (MODE_ROWS, fp32) or streams them (MODE_STREAM).
//     Per chain a lane accumulates 4+NNP partial sums; a transposed butterfly
//     built from v_permlane32_swap / v_permlane16_swap / DPP row mirrors
//     reduces them across the wave (no LDS round trips), and 4 per-wave
//     partials land in LDS.
// Here: rcp_ / exp_ and the Estrin polynomials, the bin_* bodies, the moments of the
// factorised basis, the transposed reductions and the lanes' resident bins (Bins).
// NOT a stand-alone header: nuts_device.hip includes it, lds_layout.h and gradient_pass.h
// under "#pragma clang fp contract(on)" (the reason is given there).  Included anywhere
// else, without that pragma, the sweep would be contracted differently and its rounding,
// and with it the draws, would silently change.
// Part of the sampler's one translation unit (nuts_device.hip includes the layers in order).
// All of it lives in namespace fitoct, which dev_common.h opens and only nuts_device.hip
// closes: parsed on its own, this header ends inside the open namespace.
#pragma once
#include "wave_math.h"

// ---------------------------------------------------------------------------
// per-bin arithmetic (the likelihood sweep)
// ---------------------------------------------------------------------------
template <class R> __device__ __forceinline__ R rcp_(R x);
template <> __device__ __forceinline__ double rcp_<double>(double x) {
  const double r = __builtin_amdgcn_rcp(x);    // v_rcp_f64 (quarter rate)
  const double e = fma(-x, r, 1.0);
  return fma(r, e, r);   // one Newton step: <= 1 ulp from 1/x (scripts/micro/acc.hip)
}
template <> __device__ __forceinline__ float rcp_<float>(float x) {
  return __builtin_amdgcn_rcpf(x);
}
template <class R> __device__ __forceinline__ R exp_(R x);
// exp for the sweep: reduction by ln2 (hi/lo), Taylor degree 12 on |r| <= ln2/2,
// ldexp.  n = round(x log2 e) comes from the 1.5*2^52 shifter (its low word is n
// as an int, fed straight to v_ldexp_f64: no v_rndne / v_cvt_i32_f64, the latter
// half rate).  x is clamped at -746 (below it exp is 0 either way, and the shifter
// needs |x log2 e| < 2^51); arguments here are <= 0, underflow ends in 0 via ldexp.
template <> __device__ __forceinline__ double exp_<double>(double x) {
  x = fmax(x, -746.0);
  const double SH = 6755399441055744.0;   // 1.5 * 2^52
  const double t = fma(x, 1.4426950408889634, SH);
  const double n = t - SH;
  const int ni = (int)(uint32_t)__builtin_bit_cast(uint64_t, t);
  double r = fma(-n, 6.93147180369123816490e-01, x);
  r = fma(-n, 1.90821492927058770002e-10, r);
  double p = 2.08767569878680989792e-09;   // 1/12!
  p = fma(p, r, 2.50521083854417187751e-08);
  p = fma(p, r, 2.75573192239858906526e-07);
  p = fma(p, r, 2.75573192239858906526e-06);
  p = fma(p, r, 2.48015873015873015873e-05);
  p = fma(p, r, 1.98412698412698412698e-04);
  p = fma(p, r, 1.38888888888888888889e-03);
  p = fma(p, r, 8.33333333333333333333e-03);
  p = fma(p, r, 4.16666666666666666667e-02);
  p = fma(p, r, 1.66666666666666666667e-01);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, ni);
}
template <> __device__ __forceinline__ float exp_<float>(float x) { return __expf(x); }

// Estrin's scheme for sum_k c[k] t^k (k < N): pairs c[2j] + c[2j+1] t, then pairs of those
// with t^2, t^4, ...: dependency depth ceil(log2 N) + 1 FMAs instead of N - 1.
template <int N>
__device__ __forceinline__ double estrin(const double* c, double t) {
  constexpr int M = (N + 1) / 2;
  double v[M];
#pragma unroll
  for (int j = 0; j < M; ++j) v[j] = (2 * j + 1 < N) ? fma(c[2 * j + 1], t, c[2 * j]) : c[2 * j];
  double x = t * t;
#pragma unroll
  for (int n = M; n > 1; n = (n + 1) / 2) {
#pragma unroll
    for (int j = 0; j < n / 2; ++j) v[j] = fma(v[2 * j + 1], x, v[2 * j]);
    if (n & 1) v[n / 2] = v[n - 1];
    x = x * x;
  }
  return v[0];
}
// exp_<double>'s reduction and Taylor-12 polynomial, the polynomial by Estrin
__device__ __forceinline__ double exp_lat(double x) {
  x = fmax(x, -746.0);
  const double SH = 6755399441055744.0;   // 1.5 * 2^52
  const double t = fma(x, 1.4426950408889634, SH);
  const double n = t - SH;
  const int ni = (int)(uint32_t)__builtin_bit_cast(uint64_t, t);
  double r = fma(-n, 6.93147180369123816490e-01, x);
  r = fma(-n, 1.90821492927058770002e-10, r);
  constexpr double c[13] = {1.0, 1.0, 0.5, 1.66666666666666666667e-01,
                            4.16666666666666666667e-02, 8.33333333333333333333e-03,
                            1.38888888888888888889e-03, 1.98412698412698412698e-04,
                            2.48015873015873015873e-05, 2.75573192239858906526e-06,
                            2.75573192239858906526e-07, 2.50521083854417187751e-08,
                            2.08767569878680989792e-09};
  return ldexp(estrin<13>(c, r), ni);
}
// exp_ with a degree-11 polynomial: same reduction, one FMA fewer
__device__ __forceinline__ double exp11_(double x) {
  x = fmax(x, -746.0);
  const double SH = 6755399441055744.0;
  const double t = fma(x, 1.4426950408889634, SH);
  const double n = t - SH;
  const int ni = (int)(uint32_t)__builtin_bit_cast(uint64_t, t);
  double r = fma(-n, 6.93147180369123816490e-01, x);
  r = fma(-n, 1.90821492927058770002e-10, r);
  // degree-11 Chebyshev fit on |r| <= ln2/2 (scripts/micro/exp_fit.py): <= 1 ulp from the
  // correctly rounded exp, one FMA fewer than Taylor-12
  double p = 2.5110037605963777e-08;
  p = fma(p, r, 2.763263963904103e-07);
  p = fma(p, r, 2.755724091857897e-06);
  p = fma(p, r, 2.4801485482328494e-05);
  p = fma(p, r, 0.00019841269890047113);
  p = fma(p, r, 0.0013888888952314775);
  p = fma(p, r, 0.008333333333319601);
  p = fma(p, r, 0.0416666666664881);
  p = fma(p, r, 0.1666666666666668);
  p = fma(p, r, 0.5000000000000019);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, ni);
}

// Likelihood terms of one bin given its modulation dL (shared by every mode).
// acc: [0] sum d^2, [1] sum a, [2] sum a e, [3] sum w; returns h (adjoint seed of dL).
// yi = y / uy is staged per bin (plan_data.cpp stage), so d = (y - m) / uy is one FMA,
// and c x / L is formed once for the exponent and the theta3 weight.
// The non-physical guard (1 + dL <= 0 -> lp = -inf) is a per-lane running min
// (umin), applied once after the lane's bins (no per-bin selects).
template <class R, class A, int NA>
__device__ __forceinline__ R bin_tail(R iL, R cx, R yi, R isu, R th1, R th2, A (&acc)[NA]) {
  const R ciL = cx * iL;                                         // c x / L
  R e;                                                           // exp(-c x / L)
  if constexpr (sizeof(R) == 8) e = exp11_(-ciL);
  else e = exp_<R>(-ciL);
  const R m = fma(th2, e, th1);                                  // ui.R:88
  const R d = fma(-m, isu, yi);                                  // (y-m)/uy
  const R a = d * isu;                                           // dlp/dm * sigma^2
  const R ae = a * e;
  const R w = ae * ciL;
  acc[0] += (A)(d * d);
  acc[1] += (A)a;
  acc[2] += (A)ae;
  acc[3] += (A)w;
  return w * iL;                                                 // dlp/ddL / (th2 th3) * sigma^2
}
template <class R, class A, int NA, bool LAT = false>
__device__ __forceinline__ R bin_core(R u, R cx, R yi, R isu, R th1, R th2, R th3, A (&acc)[NA],
                                      R& umin) {   // u = 1 + dL
  umin = fmin(umin, u);
  const R L = th3 * u;                                           // decay length theta3*(1+dL)
  const R iL = rcp_<R>(L);
  const R ciL = cx * iL;                                         // c x / L
  R e;                                                           // exp(-c x / L)
  if constexpr (LAT && sizeof(R) == 8) e = exp_lat(-ciL);
  else e = exp_<R>(-ciL);
  const R m = fma(th2, e, th1);                                  // ui.R:88
  const R d = fma(-m, isu, yi);                                  // (y-m)/uy
  const R a = d * isu;                                           // dlp/dm * sigma^2
  const R ae = a * e;
  const R w = ae * ciL;
  acc[0] += (A)(d * d);
  acc[1] += (A)a;
  acc[2] += (A)ae;
  acc[3] += (A)w;
  return w * iL;                                                 // dlp/ddL / (th2 th3) * sigma^2
}

// MODE_POLY: dL = a P(t) with P = sum_l c_l t^l ; moments M_l += h a t^l
template <class R, int NNP, class A>
__device__ __forceinline__ void bin_poly(R cx, R y, R isu, R t, R av, R th1, R th2, R th3,
                                         const R (&cf)[NNP], A (&acc)[4 + NNP], R& umin) {
  R P = cf[NNP - 1];
#pragma unroll
  for (int k = NNP - 2; k >= 0; --k) P = fma(P, t, cf[k]);
  const R h = bin_core<R, A, 4 + NNP>(fma(av, P, R(1)), cx, y, isu, th1, th2, th3, acc, umin);
  R p = h * av;
  acc[4] += (A)p;
#pragma unroll
  for (int l = 1; l < NNP; ++l) {
    p *= t;
    acc[4 + l] += (A)p;
  }
}

// MODE_POLY on a uniform grid: the forward half of bin_poly; returns w = h a,
// the bin's weight in the moments (accumulated per lane by moments_geo).
template <class R, int NNP, class A, bool LAT = false>
__device__ __forceinline__ R bin_poly_fwd(R cx, R y, R isu, R t, R av, R th1, R th2, R th3,
                                          const R (&cf)[NNP], A (&acc)[4 + NNP], R& umin) {
  R P;
  if constexpr (LAT && sizeof(R) == 8) {
    P = estrin<NNP>(cf, t);
  } else {
    P = cf[NNP - 1];
#pragma unroll
    for (int k = NNP - 2; k >= 0; --k) P = fma(P, t, cf[k]);
  }
  return bin_core<R, A, 4 + NNP, LAT>(fma(av, P, R(1)), cx, y, isu, th1, th2, th3, acc, umin) * av;
}

// Two bins of bin_poly_fwd sharing one reciprocal: 1/L0 = L1 / (L0 L1), 1/L1 = L0 / (L0 L1)
// (one quarter-rate v_rcp_f64 and its Newton step for two bins, <= 3 ulp).
template <class R, int NNP, class A>
__device__ __forceinline__ void bin_poly_fwd2(R cx0, R y0, R isu0, R t0, R a0, R cx1, R y1,
                                              R isu1, R t1, R a1, R th1, R th2, R th3,
                                              const R (&cf)[NNP], A (&acc)[4 + NNP], R& umin,
                                              R& w0, R& w1) {
  R P0 = cf[NNP - 1], P1 = cf[NNP - 1];
#pragma unroll
  for (int k = NNP - 2; k >= 0; --k) {
    P0 = fma(P0, t0, cf[k]);
    P1 = fma(P1, t1, cf[k]);
  }
  const R u0 = R(1) + a0 * P0, u1 = R(1) + a1 * P1;
  umin = fmin(umin, fmin(u0, u1));
  const R L0 = th3 * u0, L1 = th3 * u1;
  const R ip = rcp_<R>(L0 * L1);
  w0 = bin_tail<R, A, 4 + NNP>(ip * L1, cx0, y0, isu0, th1, th2, acc) * a0;
  w1 = bin_tail<R, A, 4 + NNP>(ip * L0, cx1, y1, isu1, th1, th2, acc) * a1;
}

// Moments of one lane's BPT bins t_b = t0 R^b:  M_l = t0^l sum_b w_b (R^l)^b.
// BPT-1 FMAs + 2 multiplies per moment instead of 2 operations per bin and moment.
template <int BPT, int NNP>
__device__ __forceinline__ void moments_geo(KPc& P, double t0, const double (&w)[BPT],
                                            double (&acc)[4 + NNP]) {
  double pw = 1.0;
#pragma unroll
  for (int l = 0; l < NNP; ++l) {
    const double X = P.geo_R[l];
    double S = w[BPT - 1];
#pragma unroll
    for (int b = BPT - 2; b >= 0; --b) S = fma(S, X, w[b]);
    acc[4 + l] = pw * S;
    pw *= t0;
  }
}

// The same for one 8-bin half of a 16-bin lane (BPT 16): M_l += t0^l sum_b w_b (R^l)^b.
template <int NB, int NNP>
__device__ __forceinline__ void moments_geo_add(KPc& P, double t0, const double (&w)[NB],
                                                double (&acc)[4 + NNP]) {
  double pw = 1.0;
#pragma unroll
  for (int l = 0; l < NNP; ++l) {
    const double X = P.geo_R[l];
    double S = w[NB - 1];
#pragma unroll
    for (int b = NB - 2; b >= 0; --b) S = fma(S, X, w[b]);
    acc[4 + l] = fma(pw, S, acc[4 + l]);
    pw *= t0;
  }
}

// MODE_ROWS / MODE_STREAM: dL = B_i . yGP ; (B^T h)_k += B_ik h
// LAT (f64, 1-2 bins per lane: a latency-bound sweep): exp by Estrin's scheme (config 5 at
// one GPU +7 %, config 2 +-0; the dot product in three FMA chains as well measured config 5
// +10 % but config 2 -1.8 %, alone config 5 -8 %: profiles/r06_ab_rows.txt)
template <class R, int NNP, class A, bool LAT = false>
__device__ __forceinline__ void bin_rows(R cx, R y, R isu, const R (&Brow)[NNP], R th1, R th2,
                                         R th3, const R (&yg)[NNP], A (&acc)[4 + NNP], R& umin) {
  R dL = R(0);
#pragma unroll
  for (int k = 0; k < NNP; ++k) dL = fma(Brow[k], yg[k], dL);
  const R h = bin_core<R, A, 4 + NNP, LAT>(R(1) + dL, cx, y, isu, th1, th2, th3, acc, umin);
#pragma unroll
  for (int k = 0; k < NNP; ++k) acc[4 + k] = fma((A)Brow[k], (A)h, acc[4 + k]);
}

// Transposed butterfly over the wave: 32 values x 64 lanes -> lane l holds the
// full sum of value (l >> 1).  Each step halves the live values: lanes whose
// step bit is set keep the upper half.  Bits 5 and 4 use the gfx950 permlane
// swaps (no select needed), bits 3..1 DPP row mirrors (partner differs in the
// step bit and below), the final pair a quad swap.
template <int H, int CTRL, int NV>
__device__ __forceinline__ void tr_dpp(double (&v)[NV], bool up) {
#pragma unroll
  for (int i = 0; i < H; ++i) {
    const double send = up ? v[i] : v[i + H];
    const double keep = up ? v[i + H] : v[i];
    v[i] = keep + dpp<CTRL>(send);
  }
}
// The same transposed butterfly for 8 values (U-turn criteria): after it every
// lane of each 8-lane group holds the full sum of one value; returns whether all
// 8 sums are > 0 (one ballot).  ~3x fewer cross-lane steps than 8 butterflies.
__device__ __forceinline__ bool transpose_all_positive8(double (&v)[8], int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = swap32_add(v[i], v[i + 4]);
#pragma unroll
  for (int i = 0; i < 2; ++i) v[i] = swap16_add(v[i], v[i + 2]);
  tr_dpp<1, DPP_MIRROR>(v, (lane & 8) != 0);
  double x = v[0];
  x += dpp<DPP_XOR1>(x);
  x += dpp<DPP_XOR2>(x);
  x += dpp<DPP_HALF_MIRROR>(x);
  const uint64_t ok = __builtin_amdgcn_ballot_w64(x > 0.0);
  return ok == __builtin_amdgcn_read_exec();
}

// The transposed butterfly for any NV <= 32 values: halves the live values per
// step (ceil).  Returns the lane's total and, in idx, which value it is (-1: a
// padding lane).
// A value without a partner at a step belongs to the step's lower lanes alone: its
// slot in the upper lanes is padding.  A padding slot is only ever sent to, and
// summed in, padding slots (a lane receives the slot it keeps, whose index is the
// sender's), and padding lanes store nothing (idx = -1), so what a padding slot
// holds never reaches a result.  Such a value therefore needs no select and no
// zero partner: every lane adds its partner's copy to its own, which in the lower
// lanes is the same keep + received, same operands, same order, as with the
// selects (each 4 v_cndmask per step), and in the upper lanes a sum nobody reads.
// No x + 0.0 is formed in a lane that holds a value (before and after this form).
template <int H, int N, int CTRL, int NV>
__device__ __forceinline__ void tr_dpp_n(double (&v)[NV], bool up) {
#pragma unroll
  for (int i = 0; i < H; ++i) {
    if (i + H < N) {
      const double send = up ? v[i] : v[i + H];
      const double keep = up ? v[i + H] : v[i];
      v[i] = keep + dpp<CTRL>(send);
    } else {
      v[i] = v[i] + dpp<CTRL>(v[i]);
    }
  }
}
template <int NV>
__device__ __forceinline__ double transpose_reduce(double (&v)[NV], int lane, int& idx) {
  constexpr int c1 = (NV + 1) / 2, c2 = (c1 + 1) / 2, c3 = (c2 + 1) / 2, c4 = (c3 + 1) / 2;
  constexpr int c5 = (c4 + 1) / 2;
  static_assert(NV <= 32 && c5 == 1, "transpose_reduce: at most 32 values");
  // (odd NV: the last value's swap partner is the first pair's swapped operand, dead after
  // its sum, instead of a zero moved into a register pair for it: the lower half gets
  // a_low + a_high as before, the upper half is a padding slot)
  double spare = 0.0;
#pragma unroll
  for (int i = 0; i < c1; ++i) {
    if (i == 0 && c1 < NV) v[i] = swap32_add(v[i], v[i + c1], spare);
    else v[i] = swap32_add(v[i], i + c1 < NV ? v[i + c1] : spare);
  }
#pragma unroll
  for (int i = 0; i < c2; ++i) v[i] = swap16_add(v[i], i + c2 < c1 ? v[i + c2] : 0.0);
  tr_dpp_n<c3, c2, DPP_MIRROR>(v, (lane & 8) != 0);
  tr_dpp_n<c4, c3, DPP_HALF_MIRROR>(v, (lane & 4) != 0);
  tr_dpp_n<c5, c4, DPP_QREV>(v, (lane & 2) != 0);
  int i = (lane & 2) ? c5 : 0;
  bool ok = i < c4;
  i += (lane & 4) ? c4 : 0;
  ok = ok && i < c3;
  i += (lane & 8) ? c3 : 0;
  ok = ok && i < c2;
  i += (lane & 16) ? c2 : 0;
  ok = ok && i < c1;
  i += (lane & 32) ? c1 : 0;
  ok = ok && i < NV;
  idx = ok ? i : -1;
  return v[0] + dpp<DPP_XOR1>(v[0]);
}

// per-lane resident bin data
template <class R, int BPT, int NNP, int MODE>
struct Bins {
  static constexpr int NB = BPT > 0 ? BPT : 1;
  static constexpr int NR = MODE == MODE_POLY ? 2 : NNP;
  R cx[NB], y[NB], isu[NB];
  R row[NB][NR];
  __device__ void load(KPc& P, int tid) {
    if constexpr (BPT > 0) {
      const AS_GLB R* pcx = (const AS_GLB R*)P.cx;
      const AS_GLB R* py = (const AS_GLB R*)P.y;
      const AS_GLB R* pisu = (const AS_GLB R*)P.isu;
      const AS_GLB R* pB = (const AS_GLB R*)P.B;
      if constexpr (BPT == 16) {   // compact: y, 1/uy, a per bin; c*x and t of bin 0 only
        cx[0] = pcx[tid];
        row[0][0] = pB[2 * (size_t)tid];
#pragma unroll
        for (int b = 0; b < BPT; ++b) {
          const int i = tid + b * GT;
          y[b] = py[i];
          isu[b] = pisu[i];
          row[b][1] = pB[2 * (size_t)i + 1];
        }
      } else {
#pragma unroll
        for (int b = 0; b < BPT; ++b) {
          const int i = tid + b * GT;
          cx[b] = pcx[i];
          y[b] = py[i];
          isu[b] = pisu[i];
#pragma unroll
          for (int k = 0; k < NR; ++k) row[b][k] = pB[(size_t)i * NR + k];
        }
      }
    }
  }
};
