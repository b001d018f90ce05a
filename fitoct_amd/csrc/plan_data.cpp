// The data plan (plan_data.h): argument checks of a problem, basis mode, bins per lane, the
// factorised basis, the geometric-grid ratios and the staged bytes.  Pure host arithmetic over
// the problem and the switches; fitoct_api.cpp uploads the result, batch.cpp plans a whole
// batch with it before anything is allocated.
#include "plan_data.h"

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>

#include "host_internal.h"

namespace fitoct {
namespace {

int check_problem(const fitoct_problem* p) {
  if (!p) return fail(FITOCT_E_ARG, "problem is NULL");
  if (p->N < 2) return fail(FITOCT_E_ARG, "N must be >= 2");
  if (p->N > FITOCT_MAX_BINS)
    return fail(FITOCT_E_ARG, "N must be <= FITOCT_MAX_BINS (" + std::to_string(FITOCT_MAX_BINS) + ")");
  if (!p->x || !p->y || !p->uy) return fail(FITOCT_E_ARG, "x, y, uy must be non-NULL");
  const bool mono = p->prior_type == FITOCT_MODEL_MONOEXP;
  if (!mono && (p->Nn < 2 || p->Nn > 24)) return fail(FITOCT_E_ARG, "Nn must be in [2, 24]");
  if (p->theta_prior != 0 && p->theta_prior != 1)
    return fail(FITOCT_E_ARG, "theta_prior must be 0 or 1");
  if (p->theta_prior == 1 && !mono)
    return fail(FITOCT_E_ARG, "theta_prior = 1 is the mono-exponential model's switch");
  if (p->theta_prior == 1 && !(p->lambda_scale > 0.0))
    return fail(FITOCT_E_ARG, "lambda_scale must be > 0");
  if (mono && p->prior_PD && p->theta_prior == 0)
    return fail(FITOCT_E_ARG, "the mono-exponential model has a flat prior: prior_PD must be 0");
  if (model_dim(p->prior_type, p->Nn) < 0) return fail(FITOCT_E_ARG, "unknown prior_type");
  if (p->data_type != 1 && p->data_type != 2) return fail(FITOCT_E_ARG, "data_type must be 1 or 2");
  for (int i = 0; i < p->N; ++i) {
    if (!isfinite(p->x[i]) || !isfinite(p->y[i]) || !(p->uy[i] > 0.0) || !isfinite(p->uy[i]))
      return fail(FITOCT_E_ARG, "x, y must be finite and uy > 0 at bin " + std::to_string(i));
  }
  if (!mono && !p->B) {   // x~ = (x - min x) / (max x - min x) (server.R:635)
    double xmin = p->x[0], xmax = p->x[0];
    for (int i = 1; i < p->N; ++i) {
      xmin = fmin(xmin, p->x[i]);
      xmax = fmax(xmax, p->x[i]);
    }
    if (!(xmax > xmin)) return fail(FITOCT_E_ARG, "x must not be constant");
  }
  for (int j = 0; j < 3; ++j)
    if (!(p->theta0[j] > 0.0)) return fail(FITOCT_E_ARG, "theta0 must be > 0");
  if (p->prior_type == FITOCT_PRIOR_NORMAL && !(p->lambda_rate > 0.0))
    return fail(FITOCT_E_ARG, "lambda_rate must be > 0");
  if (p->prior_type == FITOCT_PRIOR_LASSO && !(p->lambda_scale > 0.0))
    return fail(FITOCT_E_ARG, "lambda_scale must be > 0");
  if (p->prior_type == FITOCT_PRIOR_HORSESHOE && !(p->nu >= 1.0))
    return fail(FITOCT_E_ARG, "nu must be >= 1 (horseShoePrior.stan:13)");
  if (!(p->sigma_scale > 0.0)) return fail(FITOCT_E_ARG, "sigma_scale must be > 0");
  return FITOCT_OK;
}

int invert3(const double* S, double* Si) {
  const double a = S[0], b = S[1], c = S[2], d = S[3], e = S[4], f = S[5], g = S[6], h = S[7],
               i = S[8];
  const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const double det = a * A + b * B + c * C;
  if (!(fabs(det) > 0.0) || !isfinite(det)) return fail(FITOCT_E_ARG, "Sigma0 is singular");
  Si[0] = A / det;
  Si[1] = -(b * i - c * h) / det;
  Si[2] = (b * f - c * e) / det;
  Si[3] = B / det;
  Si[4] = (a * i - c * g) / det;
  Si[5] = -(a * f - c * d) / det;
  Si[6] = C / det;
  Si[7] = -(a * h - b * g) / det;
  Si[8] = (a * e - b * d) / det;
  if (!(A > 0.0) || !(det > 0.0)) return fail(FITOCT_E_ARG, "Sigma0 must be positive definite");
  return FITOCT_OK;
}

// Shapes: bins are strided over the GT = 256 lanes of a tile's gradient waves.  Up to max_bpt
// bins per lane keep their data in VGPRs for the whole run (0 = streamed from HBM/L2 every
// sweep): the factorised f64 basis holds 5 values per bin, so up to 8 bins per lane fit;
// explicit fp32 basis rows hold NNP + 3 values per bin, up to 4; f64 rows up to 2.
void choose_bins(int N, int max_bpt, int& bpt, int& n_pad) {
  bpt = 0;
  for (int b = 1; b <= max_bpt; b *= 2)
    if (N <= b * GT) { bpt = b; break; }
  n_pad = bpt ? bpt * GT : (N + GT - 1) / GT * GT;
}

// MODE_POLY factors of the SE basis on the uniform grid g_l = g_0 + l*dg:
//   K(x~_i, g_l) = a_i t_i^l b_l, a_i = exp(-(x~_i-g_0)^2/(2s2)),
//   t_i = exp((x~_i-g_0) dg/s2), b_l = exp(-(l dg)^2/(2s2)),
// and K^-1 = (K(xGP,xGP) + nugget I)^-1.  Accepted only if the factorised basis
// reproduces the Cholesky basis B to 1e-10 (relative to max|B|) and no power
// t^l (l < nnp) can overflow; otherwise the caller falls back to streamed rows.
bool build_poly(const fitoct_problem* p, const std::vector<double>& B, int nnp,
                std::vector<double>& ta, std::vector<double>& kinv, std::vector<double>& bv) {
  const int N = p->N, Nn = p->Nn;
  double xmin = p->x[0], xmax = p->x[0];
  for (int i = 1; i < N; ++i) {
    xmin = std::min(xmin, p->x[i]);
    xmax = std::max(xmax, p->x[i]);
  }
  const double rho = (p->rho > 0.0) ? p->rho : 1.0 / Nn;
  const double s2 = (p->kernel_conv == 0) ? rho * rho : 0.5 * rho * rho;
  double g0, dg;
  if (p->grid_type == FITOCT_GRID_INTERNAL) {
    const double dx = 1.0 / (Nn + 1);
    g0 = dx / 2;
    dg = (1.0 - dx) / (Nn - 1);
  } else {
    g0 = 0.0;
    dg = 1.0 / (Nn - 1);
  }
  ta.assign((size_t)2 * N, 0.0);
  for (int i = 0; i < N; ++i) {
    const double u = (p->x[i] - xmin) / (xmax - xmin) - g0;
    const double lt = u * dg / s2, la = -u * u / (2.0 * s2);
    if (fabs(lt) * (nnp - 1) > 650.0 || la < -650.0) return false;
    ta[2 * i] = exp(lt);
    ta[2 * i + 1] = exp(la);
  }
  bv.assign(Nn, 0.0);
  for (int l = 0; l < Nn; ++l) bv[l] = exp(-(l * dg) * (l * dg) / (2.0 * s2));
  // K^-1 by Cholesky
  std::vector<double> xg(Nn), L((size_t)Nn * Nn, 0.0);
  for (int k = 0; k < Nn; ++k) xg[k] = g0 + k * dg;
  for (int i = 0; i < Nn; ++i)
    for (int j = 0; j <= i; ++j) {
      const double d = xg[i] - xg[j];
      double sum = exp(-d * d / (2.0 * s2)) + (i == j ? p->nugget : 0.0);
      for (int k = 0; k < j; ++k) sum -= L[i * Nn + k] * L[j * Nn + k];
      if (i == j) {
        if (!(sum > 0.0)) return false;
        L[i * Nn + i] = sqrt(sum);
      } else {
        L[i * Nn + j] = sum / L[j * Nn + j];
      }
    }
  std::vector<double> Li((size_t)Nn * Nn, 0.0);  // L^-1 (lower)
  for (int j = 0; j < Nn; ++j) {
    Li[j * Nn + j] = 1.0 / L[j * Nn + j];
    for (int i = j + 1; i < Nn; ++i) {
      double sum = 0.0;
      for (int k = j; k < i; ++k) sum -= L[i * Nn + k] * Li[k * Nn + j];
      Li[i * Nn + j] = sum / L[i * Nn + i];
    }
  }
  kinv.assign((size_t)Nn * Nn, 0.0);
  for (int i = 0; i < Nn; ++i)
    for (int j = 0; j < Nn; ++j) {
      double sum = 0.0;
      for (int k = std::max(i, j); k < Nn; ++k) sum += Li[k * Nn + i] * Li[k * Nn + j];
      kinv[i * Nn + j] = sum;
    }
  // exactness check against the Cholesky basis
  double bmax = 0.0, err = 0.0;
  std::vector<double> row(Nn);
  for (int i = 0; i < N; ++i) {
    double tp = ta[2 * i + 1];
    for (int l = 0; l < Nn; ++l) {
      row[l] = tp * bv[l];
      tp *= ta[2 * i];
    }
    for (int k = 0; k < Nn; ++k) {
      double v = 0.0;
      for (int l = 0; l < Nn; ++l) v += row[l] * kinv[l * Nn + k];
      const double b = B[(size_t)i * Nn + k];
      bmax = std::max(bmax, fabs(b));
      err = std::max(err, fabs(v - b));
    }
  }
  return err <= 1e-10 * std::max(1.0, bmax);
}

// MODE_POLY with bins in registers: on an arithmetic depth grid the bins
// tid + b*GT of one lane have t = t_tid * R^b (t_i = exp(u_i dg / s2), u_i linear
// in i), which lets the sweep form a lane's moments by Horner in R^l
// (sweep_math.h moments_geo).  Accepted only if every x_i lies on the line
// through x_0 and x_{N-1} to 1e-12 of the range and no (R^l)^b can overflow.
bool geo_ratios(const fitoct_problem* p, int nnp, int bpt, double* R) {
  const int N = p->N, Nn = p->Nn;
  if (bpt < 2 || Nn < 2) return false;
  double xmin = p->x[0], xmax = p->x[0];
  for (int i = 1; i < N; ++i) {
    xmin = std::min(xmin, p->x[i]);
    xmax = std::max(xmax, p->x[i]);
  }
  const double range = xmax - xmin, step = (p->x[N - 1] - p->x[0]) / (N - 1);
  for (int i = 0; i < N; ++i)
    if (fabs(p->x[i] - (p->x[0] + i * step)) > 1e-12 * range) return false;
  const double rho = (p->rho > 0.0) ? p->rho : 1.0 / Nn;
  const double s2 = (p->kernel_conv == 0) ? rho * rho : 0.5 * rho * rho;
  const double dg = (p->grid_type == FITOCT_GRID_INTERNAL) ? (1.0 - 1.0 / (Nn + 1)) / (Nn - 1)
                                                           : 1.0 / (Nn - 1);
  const double logR = GT * (step / range) * dg / s2;
  if (fabs(logR) * (nnp - 1) * (bpt - 1) > 600.0) return false;
  if (bpt == 16) {   // c*x_b and t_b are formed in the kernel: x must be on the line to ~ulps
    for (int i = 0; i < N; ++i)
      if (fabs(p->x[i] - (p->x[0] + i * step)) > 4e-16 * std::max(fabs(xmin), fabs(xmax)) + 1e-300)
        return false;
    if (fabs(logR) * (bpt - 1) > 600.0) return false;
  }
  for (int l = 0; l < 24; ++l) R[l] = exp(l * logR);
  return true;
}

template <class R>
void stage(const fitoct_problem* p, const std::vector<double>& B, const std::vector<double>& ta,
           int mode, int n_pad, int nnp, std::vector<char>& out) {
  const size_t n = (size_t)n_pad;
  const int nr = (mode == MODE_POLY) ? 2 : nnp;
  out.assign(sizeof(R) * (3 * n + n * nr), 0);
  R* cx = (R*)out.data();
  R* y = cx + n;
  R* isu = y + n;
  R* Bp = isu + n;
  for (int i = 0; i < p->N; ++i) {
    cx[i] = (R)((double)p->data_type * p->x[i]);
    y[i] = (R)(p->y[i] / p->uy[i]);   // y / uy: the sweep forms (y - m) / uy as one FMA
    isu[i] = (R)(1.0 / p->uy[i]);
    if (mode == MODE_POLY) {
      Bp[2 * (size_t)i] = (R)ta[2 * (size_t)i];
      Bp[2 * (size_t)i + 1] = (R)ta[2 * (size_t)i + 1];
    } else {
      for (int k = 0; k < p->Nn; ++k) Bp[(size_t)i * nnp + k] = (R)B[(size_t)i * p->Nn + k];
    }
  }
}

}  // namespace

int plan_data(const fitoct_problem* p, int precision, const Switches& sw, int force_bpt,
              bool poly_only, DataPlan& dp) {
  int rc = check_problem(p);
  if (rc) return rc;
  dp = DataPlan();
  dp.mixed = (precision == FITOCT_PREC_MIXED);
  const int D = model_dim(p->prior_type, p->Nn);
  // NNP: padded control-point count of the kernel instantiation (15 = FitOCT's Nn,
  // ctrlParams.yaml:4, with no padding work in the sweep; 24 covers Nn = 16..24)
  dp.nnp = (p->Nn <= 15) ? 15 : 24;
  dp.ppl = (D <= WAVE) ? 1 : 2;
  if (dp.nnp == 15 && dp.ppl == 2) dp.nnp = 24;  // the (24, 2) instantiation covers it
  if (dp.nnp == 24) dp.ppl = 2;
  const bool mono = p->prior_type == FITOCT_MODEL_MONOEXP;
  std::vector<double> B, xg;
  if (mono) {
    // no GP term: a factorised basis of zeros (dL = 0); Nn = 0 inside the kernel
  } else if (p->B) {
    B.assign(p->B, p->B + (size_t)p->N * p->Nn);
  } else {
    rc = build_basis(p, B, xg);
    if (rc) return rc;
  }
  dp.h_xyu.assign(p->x, p->x + p->N);
  dp.h_xyu.insert(dp.h_xyu.end(), p->y, p->y + p->N);
  dp.h_xyu.insert(dp.h_xyu.end(), p->uy, p->uy + p->N);
  dp.h_B = B;
  // basis mode (see kernel_params.h BasisMode)
  std::vector<double> ta;
  int mode;
  bool rows_res = false;
  if (mono && !dp.mixed) {
    mode = MODE_POLY;
    ta.assign(2 * (size_t)p->N, 0.0);
  } else if (mono) {   // the mixed kernels are row-mode only: rows of zeros (dL = 0)
    mode = MODE_ROWS;
    B.assign((size_t)p->N * p->Nn, 0.0);
  } else if (dp.mixed) {
    mode = MODE_ROWS;
  } else {
    // N <= 512 (configs 2 and 5): the basis rows themselves, 1-2 bins of 15 doubles per lane
    // in the gradient waves' registers -- the sampler's leaf then has no K^-1 products
    // (write_mp, finish_grad) on its critical path.  Wider problems: the factorised basis.
    rows_res = !poly_only && p->N <= 2 * GT && dp.nnp == 15;
    const bool poly = !rows_res && !p->B && build_poly(p, B, dp.nnp, ta, dp.kinv, dp.bv);
    mode = poly ? MODE_POLY : MODE_ROWS;
  }
  // f64 rows (NNP doubles per bin) are streamed, but for N <= 512 (rows_res)
  int n_pad;
  choose_bins(p->N, mode == MODE_POLY ? 8 : dp.mixed ? 4 : rows_res ? 2 : 0, dp.bpt, n_pad);
  // N in (2048, 4096] on an arithmetic depth grid: 16 bins per lane in the compact
  // layout (y, 1/uy, a in registers; c*x and t formed from the lane's first bin)
  double R16[24];
  if (mode == MODE_POLY && !mono && !dp.mixed && dp.bpt == 0 && p->N <= 16 * GT &&
      force_bpt < 0 && !sw.no_geo &&
      geo_ratios(p, dp.nnp, 16, R16)) {
    dp.bpt = 16;
    n_pad = 16 * GT;
  }
  if (force_bpt >= 0 && force_bpt != dp.bpt) {   // batch: the batch's common bin layout
    if (force_bpt != 0 && force_bpt < dp.bpt) return fail(FITOCT_E_ARG, "bin layout too small");
    dp.bpt = force_bpt;
    n_pad = force_bpt ? force_bpt * GT : (p->N + GT - 1) / GT * GT;
  }
  if (dp.mixed) stage<float>(p, B, ta, mode, n_pad, dp.nnp, dp.staged);
  else stage<double>(p, B, ta, mode, n_pad, dp.nnp, dp.staged);
  KParams& k = dp.kp;
  k.mode = mode;
  k.N = p->N;
  k.n_pad = n_pad;
  k.geo = (mode == MODE_POLY && !mono && !dp.mixed && !sw.no_geo)
              ? geo_ratios(p, dp.nnp, dp.bpt, k.geo_R) : 0;
  if (dp.bpt == 16) {
    if (!k.geo) return fail(FITOCT_E_INTERNAL, "16-bin layout without a geometric grid");
    const double cstep = (double)p->data_type * (p->x[p->N - 1] - p->x[0]) / (p->N - 1);
    for (int b = 0; b < 16; ++b) k.geo_dcx[b] = (double)b * GT * cstep;
    k.geo_tmax = 0.0;
    for (int i = 0; i < p->N; ++i) k.geo_tmax = std::max(k.geo_tmax, ta[2 * (size_t)i]);
  }
  k.Nn = mono ? 0 : p->Nn;
  k.D = D;
  k.family = p->prior_type;
  k.prior_PD = p->prior_PD ? 1 : 0;
  for (int j = 0; j < 3; ++j) k.theta0[j] = p->theta0[j];
  if (mono) {
    for (int j = 0; j < 9; ++j) k.S0inv[j] = 0.0;
  } else {
    rc = invert3(p->Sigma0, k.S0inv);
    if (rc) return rc;
  }
  k.lambda_rate_eff = (p->lambda_conv == 0) ? 1.0 / p->lambda_rate : p->lambda_rate;
  k.lambda_scale = p->lambda_scale;
  k.nu = p->nu;
  k.sigma_scale = p->sigma_scale;
  k.sigma_scale_inv = 1.0 / p->sigma_scale;
  k.theta_rate = p->theta_prior == 1 ? 1.0 / p->lambda_scale : 0.0;
  return FITOCT_OK;
}

int plan_batch_data(const fitoct_problem* probs, int n_problems, int precision,
                    const Switches& sw, std::vector<DataPlan>& plans) {
  // one basis mode for the whole batch: resident rows only if every problem has N <= 512
  bool poly_only = false;
  for (int p = 0; p < n_problems; ++p) poly_only = poly_only || probs[p].N > 2 * GT;
  plans.assign(n_problems, DataPlan());
  for (int p = 0; p < n_problems; ++p) {
    if (probs[p].prior_type != probs[0].prior_type || probs[p].Nn != probs[0].Nn)
      return fail(FITOCT_E_ARG, "batch problems must share prior_type and Nn (problem " +
                                    std::to_string(p) + ")");
    const int rc = plan_data(&probs[p], precision, sw, -1, poly_only, plans[p]);
    if (rc) return fail(rc, "problem " + std::to_string(p) + ": " + g_last_error);
  }
  // one kernel instantiation and one LDS carve must serve every problem
  int bpt = 0;
  for (const DataPlan& d : plans) bpt = std::max(bpt, d.bpt == 0 ? 1 << 20 : d.bpt);
  for (const DataPlan& d : plans)
    if (d.kp.mode != plans[0].kp.mode || d.nnp != plans[0].nnp || d.ppl != plans[0].ppl)
      return fail(FITOCT_E_ARG, "batch problems plan to different kernels (basis mode)");
  // bins: every tile runs the batch's widest bin layout.  A problem planned with
  // fewer bins per lane is staged at the common n_pad (zero-weight padding).
  if (bpt == 1 << 20) bpt = 0;
  auto replan = [&](int to) -> int {
    for (int p = 0; p < n_problems; ++p) {
      if (plans[p].bpt == to) continue;
      DataPlan d;
      const int rc = plan_data(&probs[p], precision, sw, to, poly_only, d);
      if (rc) return rc;
      plans[p] = std::move(d);
    }
    return FITOCT_OK;
  };
  int rc = replan(bpt);
  // the 16-bin layout needs an arithmetic depth grid in every problem: else stream all
  if (rc && bpt == 16) rc = replan(0);
  return rc;
}

}  // namespace fitoct

namespace {
// 64-bit FNV-1a of a byte range
uint64_t fnv1a(const void* data, size_t bytes, uint64_t h = 0xcbf29ce484222325ULL) {
  const unsigned char* c = (const unsigned char*)data;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ c[i]) * 0x100000001b3ULL;
  return h;
}
fitoct::Switches switches_of(const int32_t* sw) {
  fitoct::Switches w;
  w.no_geo = sw[0], w.no_pair = sw[1], w.pair = sw[2], w.no_migrate = sw[3], w.no_spec = sw[4];
  w.no_bidi = sw[5], w.no_tail_bidi = sw[6], w.spec = sw[7], w.spec_live = sw[8];
  w.tail_left = sw[9], w.test_tail_idle_us = sw[10], w.test_pair_absent = sw[11];
  return w;
}
}  // namespace

// test entries (tests/test_plan_data.py): the data plan over a problem and explicit switches
// (`sw`: the Switches fields in declaration order, as int32).
// `ints`: mode, bpt, n_pad, nnp, ppl, mixed, N, Nn, D, family, prior_PD, geo, then the lengths
// of staged (bytes), kinv, bv, h_xyu, h_B.  `dbls`: theta0[3], lambda_rate_eff, lambda_scale,
// nu, sigma_scale, sigma_scale_inv, theta_rate, geo_tmax.  `digests`: FNV-1a of the staged
// bytes; kinv; bv; geo_R | geo_dcx | geo_tmax; S0inv.
extern "C" int32_t fitoct_internal_plan_data(const fitoct_problem* prob, int32_t precision,
                                             const int32_t* sw, int32_t force_bpt,
                                             int32_t poly_only, int64_t* ints, double* dbls,
                                             uint64_t* digests) {
  using namespace fitoct;
  return guarded(__func__, [&]() -> int32_t {
    DataPlan d;
    const int rc = plan_data(prob, precision, switches_of(sw), force_bpt, poly_only != 0, d);
    if (rc) return rc;
    const KParams& k = d.kp;
    const int64_t iv[17] = {k.mode, d.bpt, k.n_pad, d.nnp, d.ppl, d.mixed, k.N, k.Nn, k.D,
                            k.family, k.prior_PD, k.geo, (int64_t)d.staged.size(),
                            (int64_t)d.kinv.size(), (int64_t)d.bv.size(),
                            (int64_t)d.h_xyu.size(), (int64_t)d.h_B.size()};
    std::copy(iv, iv + 17, ints);
    const double dv[10] = {k.theta0[0], k.theta0[1], k.theta0[2], k.lambda_rate_eff,
                           k.lambda_scale, k.nu, k.sigma_scale, k.sigma_scale_inv, k.theta_rate,
                           k.geo_tmax};
    std::copy(dv, dv + 10, dbls);
    digests[0] = fnv1a(d.staged.data(), d.staged.size());
    digests[1] = fnv1a(d.kinv.data(), sizeof(double) * d.kinv.size());
    digests[2] = fnv1a(d.bv.data(), sizeof(double) * d.bv.size());
    digests[3] = fnv1a(&k.geo_tmax, sizeof k.geo_tmax,
                       fnv1a(k.geo_dcx, sizeof k.geo_dcx, fnv1a(k.geo_R, sizeof k.geo_R)));
    digests[4] = fnv1a(k.S0inv, sizeof k.S0inv);
    return FITOCT_OK;
  });
}

// ... and the batch's common layout over n problems: out[0] the common bpt, then mode, bpt and
// n_pad of every problem's final plan
extern "C" int32_t fitoct_internal_batch_layout(const fitoct_problem* probs, int32_t n,
                                                int32_t precision, const int32_t* sw,
                                                int64_t* out) {
  using namespace fitoct;
  return guarded(__func__, [&]() -> int32_t {
    std::vector<DataPlan> plans;
    const int rc = plan_batch_data(probs, n, precision, switches_of(sw), plans);
    if (rc) return rc;
    out[0] = plans[0].bpt;
    for (int p = 0; p < n; ++p) {
      out[1 + 3 * p] = plans[p].kp.mode;
      out[2 + 3 * p] = plans[p].bpt;
      out[3 + 3 * p] = plans[p].kp.n_pad;
    }
    return FITOCT_OK;
  });
}
