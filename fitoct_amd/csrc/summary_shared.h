// Pieces of the posterior summary and of the rank diagnostics that the host and the device must
// compute the same way (include/fitoct.h "posterior summary", "rank diagnostics"; DESIGN.md
// §4): the output-layout transform of stan_output.cpp, the order-preserving key and the type-7
// index arithmetic of the quantiles, Geyer's truncation rule of the effective sample size, and
// the inverse normal CDF of the rank normalisation.  Compiles for the host (g++) and,
// where marked FITOCT_HD, for the device (hipcc).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fitoct.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FITOCT_HD __host__ __device__
#else
#define FITOCT_HD
#endif

namespace fitoct {

// ---- output layout (Stan's order: parameters, transformed parameters, generated
// quantities; include/fitoct.h "Stan output") -------------------------------------------
// One output parameter column: where its value comes from.
enum Src { S_RAW = 0, S_LAMBDA_DATA, S_TAU, S_HS_LAMBDA, S_HS_YGP };
struct OutSpec {
  int src;
  int k;   // S_RAW: raw parameter index (0..D, D = br); S_HS_*: control point
};
// what the layout reads of a fitoct_problem
struct OutModel {
  int fam, Nn, D, prior_PD;
  double lambda_scale;
};

FITOCT_HD inline int out_n_params(const OutModel& m) {
  int n = m.D;
  if (m.fam == FITOCT_PRIOR_LASSO) n += 1;
  else if (m.fam == FITOCT_PRIOR_HORSESHOE) n += 1 + 2 * m.Nn;
  return n + (m.prior_PD ? 0 : 1);
}

// output parameter column i (0 <= i < out_n_params)
FITOCT_HD inline OutSpec out_spec(const OutModel& m, int i) {
  if (i < m.D) return {S_RAW, i};
  i -= m.D;
  if (m.fam == FITOCT_PRIOR_LASSO) {
    // ⚑ lassoPrior.stan has no lambda parameter: its penalty lambda_s is data
    // (lassoPrior.stan:4), exposed as the constant column `lambda`
    if (i == 0) return {S_LAMBDA_DATA, 0};
    i -= 1;
  } else if (m.fam == FITOCT_PRIOR_HORSESHOE) {
    // transformed parameters of horseShoePrior.stan:25-33, in declaration order
    if (i == 0) return {S_TAU, 0};
    i -= 1;
    if (i < m.Nn) return {S_HS_LAMBDA, i};
    i -= m.Nn;
    if (i < m.Nn) return {S_HS_YGP, i};
    i -= m.Nn;
  }
  return {S_RAW, m.D};   // br (plotExpGP.R:42-43: absent in a prior run)
}

// constrained raw parameters r[0..D-1], br r[D]  ->  the value of one output column
// (products and correctly rounded square roots only: the same bits on host and device)
FITOCT_HD inline double out_value(const OutModel& m, OutSpec c, const double* r) {
  const int Nn = m.Nn;
  // horseshoe raw order: theta[3] z[Nn] r1_global r2_global r1_local[Nn] r2_local[Nn] sigma
  switch (c.src) {
    case S_RAW: return r[c.k];
    case S_LAMBDA_DATA: return m.lambda_scale;
    case S_TAU: return r[3 + Nn] * sqrt(r[4 + Nn]);
    case S_HS_LAMBDA: return r[5 + Nn + c.k] * sqrt(r[5 + 2 * Nn + c.k]);
    default: {   // S_HS_YGP
      const double tau = r[3 + Nn] * sqrt(r[4 + Nn]);
      return r[3 + c.k] * (r[5 + Nn + c.k] * sqrt(r[5 + 2 * Nn + c.k])) * tau;
    }
  }
}

// ---- fitted curves (fitoct_expgp_curves, fitoct_curves_*: "posterior curves") -----------------
// Curve parameter k of a draw: theta.1..3 (k < 3), then yGP.(k - 2), as OUTPUT-layout columns.
FITOCT_HD inline OutSpec curve_param_spec(const OutModel& m, int k) {
  if (k < 3 || m.fam != FITOCT_PRIOR_HORSESHOE) return {S_RAW, k};
  return {S_HS_YGP, k - 3};
}
// One bin of one draw: dL_i = B_i . yGP,
// m_i = theta1 + theta2 exp(-c x_i / (theta3 (1 + dL_i))) (ui.R:88, synthData.R:22),
// resid_i = (y_i - m_i) / uy_i.  ncx = -c x_i; nn = 0 for the mono-exponential model.  The
// one copy of the loop body: the host routes and the device kernels differ only in exp and in
// the fma contraction of the device compile.
struct CurveBin {
  double dL, m, resid;
};
FITOCT_HD inline CurveBin curve_bin(const double* Brow, int nn, const double* ygp,
                                    const double* th, double ncx, double y, double uy) {
  double d = 0.0;
  for (int k = 0; k < nn; ++k) d += Brow[k] * ygp[k];
  const double mi = th[0] + th[1] * exp(ncx / (th[2] * (1.0 + d)));
  return {d, mi, (y - mi) / uy};
}

// ---- quantiles ----------------------------------------------------------------------------
// Order-preserving 64-bit key of a double: key(a) < key(b) as unsigned integers where a < b,
// with -0.0 below +0.0 (a total order, so that an order statistic is one bit pattern).
FITOCT_HD inline uint64_t order_key(double v) {
  uint64_t u;
  memcpy(&u, &v, sizeof u);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
FITOCT_HD inline double key_value(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  memcpy(&v, &u, sizeof v);
  return v;
}
// type-7 quantile of S sorted values at probability p: x[lo] + frac (x[hi] - x[lo])
struct QIndex {
  int64_t lo, hi;
  double frac;
};
FITOCT_HD inline QIndex quantile_index(int64_t S, double p) {
  const double h = (double)(S - 1) * p, fl = floor(h);
  QIndex q;
  q.lo = (int64_t)fl < S - 1 ? (int64_t)fl : S - 1;
  q.hi = q.lo + 1 < S ? q.lo + 1 : S - 1;
  q.frac = h - fl;
  return q;
}
// (called on the host only, by both routes: a device compile could contract it to an fma)
inline double quantile_lerp(double x_lo, double x_hi, double frac) {
  return frac > 0.0 ? x_lo + frac * (x_hi - x_lo) : x_lo;
}

// ---- diagnostics (stan::analyze, as printed by rstan::summary) ------------------------------
inline double mean_of(const double* x, int n) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += x[i];
  return s / n;
}
inline double var_of(const double* x, int n) {  // sample variance (n-1)
  const double m = mean_of(x, n);
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += (x[i] - m) * (x[i] - m);
  return s / (n - 1);
}

// potential scale reduction from the means cm[m] and sample variances cv[m] of m already
// split chains of n draws
inline double psr_moments(const double* cm, const double* cv, int m, int n) {
  const double B = n * var_of(cm, m);
  const double W = mean_of(cv, m);
  return sqrt((B / W + n - 1) / n);
}

// stan::analyze::compute_effective_sample_size on m already split chains of n draws, from
// their means cm[m], sample variances cvar[m] and acov_mean(lag): the mean over chains of
// the biased autocovariance at `lag` (each chain about its own mean).  Geyer's initial
// positive sequence, then the initial monotone sequence, then the 1/log10 floor.
template <class F>
double ess_moments(const double* cm, const double* cvar, int m, int n, F&& acov_mean) {
  const double mean_var = mean_of(cvar, m);
  double var_plus = mean_var * (n - 1) / n;
  if (m > 1) var_plus += var_of(cm, m);
  if (!(var_plus > 0.0)) return NAN;
  std::vector<double> rho(n + 2, 0.0);
  double rho_even = 1.0;
  double rho_odd = 1.0 - (mean_var - acov_mean(1)) / var_plus;
  rho[0] = 1.0;
  rho[1] = rho_odd;
  int t = 1;
  while (t < n - 4 && (rho_even + rho_odd) > 0.0) {
    rho_even = 1.0 - (mean_var - acov_mean(t + 1)) / var_plus;
    rho_odd = 1.0 - (mean_var - acov_mean(t + 2)) / var_plus;
    if ((rho_even + rho_odd) >= 0.0) {
      rho[t + 1] = rho_even;
      rho[t + 2] = rho_odd;
    }
    t += 2;
  }
  const int max_t = t;
  if (rho_even > 0.0) rho[max_t + 1] = rho_even;
  t = 1;
  while (t <= max_t - 2) {
    if (rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]) {
      rho[t + 1] = (rho[t - 1] + rho[t]) / 2.0;
      rho[t + 2] = rho[t + 1];
    }
    t += 2;
  }
  const double ess = (double)m * n;
  double tau = -1.0;
  for (int i = 0; i <= max_t; ++i) tau += 2.0 * rho[i];
  tau += rho[max_t + 1];
  tau = std::max(tau, 1.0 / log10(ess));
  return ess / tau;
}

// ---- rank diagnostics (rstan::monitor) ----------------------------------------------------------
// a NaN among sorted keys lies at an end: below key(-inf) or above key(+inf)
FITOCT_HD inline bool keys_hold_nan(uint64_t first, uint64_t last) {
  return first < 0x000fffffffffffffull || last > 0xfff0000000000000ull;
}
// Tail_ESS of the two indicator series: the smaller one, a NaN in either propagating
inline double tail_min(double a, double b) {
  return (a != a || b != b) ? NAN : std::min(a, b);
}

// ---- rank normalisation (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021) -----------------
// Phi^-1 of the fractional rank: the host diagnostics (host_model.cpp) and the device rank
// diagnostics (monitor_device.hip) compile this one copy.
FITOCT_HD inline double inv_normal_cdf(double p) {
  // Acklam's rational approximation + one Newton step (|err| < 1e-13)
  const double a[] = {-3.969683028665376e+01, 2.209460984245205e+02,
                      -2.759285104469687e+02, 1.383577518672690e+02,
                      -3.066479806614716e+01, 2.506628277459239e+00};
  const double b[] = {-5.447609879822406e+01, 1.615858368580409e+02,
                      -1.556989798598866e+02, 6.680131188771972e+01,
                      -1.328068155288572e+01};
  const double c[] = {-7.784894002430293e-03, -3.223964580411365e-01,
                      -2.400758277161838e+00, -2.549732539343734e+00,
                      4.374664141464968e+00, 2.938163982698783e+00};
  const double d[] = {7.784695709041462e-03, 3.224671290700398e-01,
                      2.445134137142996e+00, 3.754408661907416e+00};
  double q, r, x;
  if (p < 0.02425) {
    q = sqrt(-2 * log(p));
    x = (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) /
        ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1);
  } else if (p > 1 - 0.02425) {
    q = sqrt(-2 * log(1 - p));
    x = -(((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) /
        ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1);
  } else {
    q = p - 0.5;
    r = q * q;
    x = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
        (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1);
  }
  const double e = 0.5 * erfc(-x / sqrt(2.0)) - p;
  const double u = e * sqrt(2 * M_PI) * exp(x * x / 2);
  return x - u / (1 + x * u / 2);
}

}  // namespace fitoct
