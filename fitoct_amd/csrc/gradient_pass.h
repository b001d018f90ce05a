// Device-resident NUTS, layer 6: the gradient waves' sweep of the likelihood and its
// hand-derived gradient over the lanes' resident bins (sweep_math.h), for the chains whose
// positions are staged in LDS; one partial sum per wave and slot lands in PART.
// Part of the sampler's one translation unit (nuts_device.hip includes the layers in order).
// All of it lives in namespace fitoct, which dev_common.h opens and only nuts_device.hip
// closes: parsed on its own, this header ends inside the open namespace.
// Compiled under nuts_device.hip's "#pragma clang fp contract(on)" (see sweep_math.h).
#pragma once
#include "sweep_math.h"
#include "lds_layout.h"

// The likelihood sweep of chains [cb, ce) of the tile (gradient waves only).
// PART[c][wave][0 .. 4+NNP) receives this wave's partial sums of chain c.
// LATR: the row-mode sweep's latency form (bin_rows LAT); every sampler and the logp kernel
// use it, so all paths keep computing the same gradient bit for bit.
template <class R, int BPT, int NNP, int MODE, bool LATR = false>
__device__ void gradient_pass(KPc& P, const Bins<R, BPT, NNP, MODE>& bins,
                              const AS_LDS double* mpall, AS_LDS double* part, const int* done,
                              int cb, int ce,
                              int tid, int lane, int wave) {
  FITOCT_MARK(gradient_pass);
  for (int c = cb; c < ce; ++c) {
    if (done[c]) continue;   // wave-uniform (LDS broadcast)
    const AS_LDS double* mp = mpall + c * MPW;
    const R th1 = (R)mp[0], th2 = (R)mp[1], th3 = (R)mp[2];
    R cf[NNP];   // POLY: c_l = b_l (K^-1 yGP)_l ; ROWS: yGP_k
#pragma unroll
    for (int k = 0; k < NNP; ++k) cf[k] = (R)mp[4 + k];
    double acc[4 + NNP];
#pragma unroll
    for (int k = 0; k < 4 + NNP; ++k) acc[k] = 0.0;
    R umin = R(1);
    if constexpr (BPT == 16) {   // MODE_POLY f64 on an arithmetic grid (host-checked)
      double cx0 = bins.cx[0], t0 = bins.row[0][0];
      const double tmax = P.geo_tmax;
      // opaque per sweep: c*x_b and t_b are formed inside the sweep, as the compact layout
      // intends, instead of being hoisted out of the sweep loop (32 more live doubles)
      asm volatile("" : "+v"(cx0), "+v"(t0));
      // the lane's bins in groups of NQ (moments per group: NQ weights live at a time);
      // one reciprocal per bin (pairs sharing one measured 3 % slower here)
      constexpr int NQ = BPT16_GROUP;
#pragma unroll
      for (int q = 0; q < 16 / NQ; ++q) {
        double w[NQ];
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
          const int bb = q * NQ + b;
          const double cxb = cx0 + P.geo_dcx[bb];
          const double tb = fmin(t0 * P.geo_R[bb], tmax);
          w[b] = bin_poly_fwd<R, NNP, double>(cxb, bins.y[bb], bins.isu[bb], tb,
                                              bins.row[bb][1], th1, th2, th3, cf, acc, umin);
        }
        moments_geo_add<NQ, NNP>(P, q ? t0 * P.geo_R[q * NQ] : t0, w, acc);
      }
    } else if constexpr (BPT > 0 && MODE == MODE_POLY && sizeof(R) == 8) {
      if (P.geo) {
        double w[BPT];
        // 8 bins per lane (the headline shape, N = 2048): bins in pairs sharing one
        // reciprocal, exp by a degree-11 polynomial (A/B: config 3 +1.7 %, configs 2 / 5
        // within noise; at 16 bins the pairs spill)
        if constexpr (BPT == 8) {
#pragma unroll
          for (int b = 0; b < BPT; b += 2)
            bin_poly_fwd2<R, NNP, double>(bins.cx[b], bins.y[b], bins.isu[b], bins.row[b][0],
                                          bins.row[b][1], bins.cx[b + 1], bins.y[b + 1],
                                          bins.isu[b + 1], bins.row[b + 1][0], bins.row[b + 1][1],
                                          th1, th2, th3, cf, acc, umin, w[b], w[b + 1]);
        } else {
          // sweeps of at most 2 bins per lane (N <= 512: configs 2 and 5) are latency-bound:
          // the basis polynomial and exp by Estrin's scheme (config 5 +1.8 %)
          constexpr bool LAT = BPT <= 2;
#pragma unroll
          for (int b = 0; b < BPT; ++b)
            w[b] = bin_poly_fwd<R, NNP, double, LAT>(bins.cx[b], bins.y[b], bins.isu[b],
                                                     bins.row[b][0], bins.row[b][1], th1, th2,
                                                     th3, cf, acc, umin);
        }
        moments_geo<BPT, NNP>(P, bins.row[0][0], w, acc);
      } else {
#pragma unroll
        for (int b = 0; b < BPT; ++b)
          bin_poly<R, NNP, double>(bins.cx[b], bins.y[b], bins.isu[b], bins.row[b][0],
                                   bins.row[b][1], th1, th2, th3, cf, acc, umin);
      }
    } else if constexpr (BPT > 0 && MODE == MODE_POLY) {
#pragma unroll
      for (int b = 0; b < BPT; ++b)
        bin_poly<R, NNP, double>(bins.cx[b], bins.y[b], bins.isu[b], bins.row[b][0],
                                 bins.row[b][1], th1, th2, th3, cf, acc, umin);
    } else if constexpr (BPT > 0) {
      // the few bins of one lane accumulate in R, the lane totals in f64
      constexpr bool ROWS_LAT = LATR && sizeof(R) == 8 && BPT <= 2;
      R racc[4 + NNP];
#pragma unroll
      for (int k = 0; k < 4 + NNP; ++k) racc[k] = R(0);
#pragma unroll
      for (int b = 0; b < BPT; ++b)
        bin_rows<R, NNP, R, ROWS_LAT>(bins.cx[b], bins.y[b], bins.isu[b], bins.row[b], th1, th2,
                                      th3, cf, racc, umin);
#pragma unroll
      for (int k = 0; k < 4 + NNP; ++k) acc[k] = (double)racc[k];
    } else {
      const AS_GLB R* pcx = (const AS_GLB R*)P.cx;
      const AS_GLB R* py = (const AS_GLB R*)P.y;
      const AS_GLB R* pisu = (const AS_GLB R*)P.isu;
      const AS_GLB R* pB = (const AS_GLB R*)P.B;
      for (int i = tid; i < P.n_pad; i += GT) {
        if constexpr (MODE == MODE_POLY) {
          bin_poly<R, NNP, double>(pcx[i], py[i], pisu[i], pB[2 * (size_t)i], pB[2 * (size_t)i + 1],
                                   th1, th2, th3, cf, acc, umin);
        } else {
          R row[NNP];
#pragma unroll
          for (int k = 0; k < NNP; ++k) row[k] = pB[(size_t)i * NNP + k];
          bin_rows<R, NNP, double>(pcx[i], py[i], pisu[i], row, th1, th2, th3, cf, acc, umin);
        }
      }
    }
    if (!(umin > R(0))) acc[0] = INFINITY;   // some bin has 1 + dL <= 0: lp = -inf
    int idx;
    FITOCT_MARK(sweep_reduce);
    const double r = transpose_reduce<4 + NNP>(acc, lane, idx);
    if (!(lane & 1) && idx >= 0) part[(c * NGW + wave) * NSLOT + idx] = r;
  }
}
