// Posterior summary of draws that stay in HBM (include/fitoct.h "posterior summary";
// DESIGN.md §4.9): rstan::summary(fit, pars)$summary -- mean, se_mean, sd, type-7 quantiles,
// n_eff, Rhat per output column -- computed on the device from the sampler's raw draws
// buffer, and the same computation on the host (fitoct_summary_host, on top of
// split_rhat_ess and std::nth_element) that the device route is tested against.
//
// Device route, per pass over a chunk of output columns (the first three kernels and Geyer's
// rounds live in summary_kernels.h, shared with monitor_device.hip):
//   stage_kernel    raw rows (contiguous, read coalesced through LDS) -> the output-layout
//                   transform (summary_shared.h, the copy stan_output.cpp uses) -> a
//                   column-major post-warmup staging buffer X[group][col][chain][n];
//   moments_kernel  one wave per (group, col, split chain): mean, then centred sum of
//                   squares, NaN and constant flags (butterfly reductions: a fixed order);
//   acov_kernel     per (group, col, block of 64 lags): biased autocovariance of every split
//                   chain about its own mean, averaged over the split chains in a fixed
//                   order.  The host applies Geyer's rule (ess_moments, shared with the host
//                   diagnostics) block by block and asks for the next block only for the
//                   columns that have not terminated;
//   qhist_kernel /  exact radix select over order-preserving 64-bit keys of the pooled
//   qselect_kernel  values: eight 8-bit passes, most significant byte first, for the up to
//                   2 n_probs order statistics of each (group, col) at once; histograms in
//                   LDS, merged with integer atomics; a one-wave kernel picks the digits.
// No floating-point atomics anywhere: the results are the same bit for bit from call to call.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fitoct.h"
#include "host_internal.h"
#include "plan_internal.h"
#include "summary_kernels.h"
#include "summary_shared.h"

namespace fitoct {
namespace {

// out row = mean, se_mean, sd, the quantiles, n_eff, Rhat
void put_row(const Shape& s, double* row, double mean, double sd, const double* q, double ess,
             double rhat) {
  row[0] = mean;
  row[1] = ess > 0.0 ? sd / sqrt(ess) : NAN;
  row[2] = sd;
  for (int i = 0; i < s.np; ++i) row[3 + i] = q[i];
  row[3 + s.np] = ess;
  row[4 + s.np] = rhat;
}
void nan_row(const Shape& s, double* row) {
  for (int i = 0; i < s.width; ++i) row[i] = NAN;
}

// ---- host route -----------------------------------------------------------------------------
int summary_host(const Shape& s, const double* draws, const fitoct_summary_config* cfg,
                 double* out) {
  std::vector<double> x((size_t)s.S), q((size_t)std::max(1, s.np));
  std::vector<uint64_t> keys;
  for (int g = 0; g < s.G; ++g) {
    OutModel m = s.model;
    m.lambda_scale = s.lscale[g];
    for (int j = 0; j < s.P; ++j) {
      double* row = out + ((size_t)g * s.P + j) * s.width;
      bool has_nan = false;
      for (int c = 0; c < s.C; ++c)
        for (int i = 0; i < s.n; ++i) {
          const double* raw = draws + (((size_t)g * s.C + c) * s.I + s.first + i) * s.W;
          const double v = column_value(m, j, raw);
          has_nan = has_nan || v != v;
          x[(size_t)c * s.n + i] = v;
        }
      if (has_nan) {
        nan_row(s, row);
        continue;
      }
      double rhat = NAN, ess = NAN;
      const int rc = split_rhat_ess(x.data(), s.C, s.n, &rhat, &ess);
      if (rc) return rc;
      double sum = 0.0, ssq = 0.0;
      for (int64_t i = 0; i < s.S; ++i) sum += x[i];
      const double mean = sum / (double)s.S;
      for (int64_t i = 0; i < s.S; ++i) ssq += (x[i] - mean) * (x[i] - mean);
      const double sd = sqrt(ssq / (double)(s.S - 1));
      if (s.np > 0) {   // order statistics by the total order of the keys (-0.0 < +0.0)
        keys.resize((size_t)s.S);
        for (int64_t i = 0; i < s.S; ++i) keys[i] = order_key(x[i]);
        for (int i = 0; i < s.np; ++i) {
          const QIndex qi = quantile_index(s.S, cfg->probs[i]);
          std::nth_element(keys.begin(), keys.begin() + qi.lo, keys.end());
          const double x_lo = key_value(keys[qi.lo]);
          // the next order statistic is the smallest key above position lo
          const double x_hi = qi.hi > qi.lo
                                  ? key_value(*std::min_element(keys.begin() + qi.hi, keys.end()))
                                  : x_lo;
          q[i] = quantile_lerp(x_lo, x_hi, qi.frac);
        }
      }
      put_row(s, row, mean, sd, q.data(), ess, rhat);
    }
  }
  return FITOCT_OK;
}

// ---- kernels: stage_kernel, moments_kernel, acov_kernel, qhist_kernel, qselect_kernel
// (summary_kernels.h, shared with monitor_device.hip and curves_device.hip) ------------------

// ---- device route ---------------------------------------------------------------------------
int summary_device(const Shape& s, const void* d_draws, const fitoct_summary_config* cfg,
                   hipStream_t st, double* out) {
  DeviceKeep keep;
  HIP_TRY(hipSetDevice(cfg->device));
  const int64_t col_bytes = (int64_t)s.G * s.S * (int64_t)sizeof(double);
  const int ncc_max = columns_per_pass(s, cfg, col_bytes);
  const int64_t pairs_max = (int64_t)s.G * ncc_max;
  const int rblocks = (s.n + STAGE_ROWS - 1) / STAGE_ROWS;
  const int nblk = qhist_blocks(s.S);
  const int64_t limit = (int64_t)1 << 31;
  if ((int64_t)rblocks * s.C * s.G >= limit || pairs_max * s.m >= limit ||
      pairs_max * nblk >= limit)
    return fail(FITOCT_E_ARG, "summary: shape too large for one launch (lower max_staging_bytes)");
  const int T = 2 * s.np;

  DevBuf X, lscale;
  EssBufs eb;
  SelectBufs sel;
  FITOCT_TRY(X.alloc((size_t)pairs_max * s.S * sizeof(double)));
  FITOCT_TRY(eb.alloc(pairs_max, s.m));
  FITOCT_TRY(lscale.alloc((size_t)s.G * sizeof(double)));
  if (T > 0) FITOCT_TRY(sel.alloc(pairs_max));
  HIP_TRY(hipMemcpyAsync(lscale.p, s.lscale.data(), sizeof(double) * s.G, hipMemcpyHostToDevice, st));

  // the order statistics every column needs: x[lo], x[hi] of each probability
  std::vector<QIndex> qidx(s.np);
  for (int i = 0; i < s.np; ++i) qidx[i] = quantile_index(s.S, cfg->probs[i]);
  const SelectRanks ranks(qidx, pairs_max);

  std::vector<double> h_mom, cm(s.m), cv(s.m), q((size_t)std::max(1, s.np));
  std::vector<int> h_flags;
  std::vector<unsigned long long> h_keys;
  for (int c0 = 0; c0 < s.P; c0 += ncc_max) {
    const int ncc = std::min(ncc_max, s.P - c0);
    const int64_t pairs = (int64_t)s.G * ncc;
    KShape k{s.G, s.C, s.I, s.W, s.first, s.n, s.h, s.m, c0, ncc, s.model};
    stage_kernel<<<dim3((unsigned)((int64_t)rblocks * s.C * s.G)), dim3(STAGE_THREADS),
                   sizeof(double) * STAGE_ROWS * (s.W | 1), st>>>(
        k, (const double*)d_draws, lscale.as<double>(), X.as<double>());
    HIP_TRY(hipGetLastError());
    FITOCT_TRY(queue_moments(k, X.as<double>(), pairs, eb, st, h_mom, h_flags));

    // quantiles: queued behind the moments, read back after the autocovariance rounds
    if (T > 0) FITOCT_TRY(queue_select(X.as<double>(), pairs, s.S, T, nblk, sel, ranks, st, h_keys));
    HIP_TRY(hipStreamSynchronize(st));

    // per pair: NaN / constant pattern, pooled mean and sd, Rhat; which pairs need n_eff
    struct Col {
      double mean = NAN, sd = NAN, rhat = NAN;
      bool has_nan = false, constant = false;
    };
    std::vector<Col> cols((size_t)pairs);
    std::vector<int> active;
    for (int64_t p = 0; p < pairs; ++p) {
      Col& c = cols[p];
      const double* mo = h_mom.data() + (size_t)p * s.m * 4;
      int fl = 0;
      for (int j = 0; j < s.m; ++j) fl |= h_flags[(size_t)p * s.m + j];
      c.has_nan = fl & 1;
      c.constant = !(fl & 2);
      if (c.has_nan) continue;
      pooled_mean_sd(mo, s.n, s.h, s.m, s.S, c.mean, c.sd);
      if (c.constant) continue;   // n_eff and Rhat are NaN (split_rhat_ess)
      for (int j = 0; j < s.m; ++j) {
        cm[j] = mo[4 * j];
        cv[j] = mo[4 * j + 1] / (s.h - 1);
      }
      c.rhat = psr_moments(cm.data(), cv.data(), s.m, s.h);
      active.push_back((int)p);
    }
    // n_eff: autocovariance in blocks of 64 lags, only for the columns still undecided
    std::vector<double> ess((size_t)pairs, NAN);
    FITOCT_TRY(ess_rounds(k, X.as<double>(), eb, st, h_mom, active, ess));
    for (int64_t p = 0; p < pairs; ++p) {
      const int g = (int)(p / ncc), j = c0 + (int)(p % ncc);
      double* row = out + ((size_t)g * s.P + j) * s.width;
      const Col& c = cols[p];
      if (c.has_nan) {
        nan_row(s, row);
        continue;
      }
      for (int i = 0; i < s.np; ++i)
        q[i] = quantile_lerp(key_value(h_keys[p * QT_MAX + 2 * i]),
                             key_value(h_keys[p * QT_MAX + 2 * i + 1]), qidx[i].frac);
      put_row(s, row, c.mean, c.sd, q.data(), ess[p], c.rhat);
    }
  }
  return FITOCT_OK;
}

int summary_device_checked(const fitoct_problem* probs, int n_groups, int chains, int iters_saved,
                           const void* d_draws, const fitoct_summary_config* cfg, void* stream,
                           double* out) {
  Shape s;
  FITOCT_TRY(check_args("summary", true, probs, n_groups, chains, iters_saved, d_draws, cfg, out, s));
  FITOCT_TRY(check_device("summary", cfg, d_draws));
  return summary_device(s, d_draws, cfg, (hipStream_t)stream, out);
}

}  // namespace
}  // namespace fitoct

using namespace fitoct;

extern "C" {

void fitoct_default_summary_config(fitoct_summary_config* cfg) {
  if (!cfg) return;
  *cfg = fitoct_summary_config{};
  const double p[5] = {0.025, 0.25, 0.5, 0.75, 0.975};   // rstan::summary's default probs
  cfg->n_probs = 5;
  for (int i = 0; i < 5; ++i) cfg->probs[i] = p[i];
}

int32_t fitoct_summary_width(int32_t n_probs) {
  if (n_probs < 0 || n_probs > MAX_PROBS) return fail(FITOCT_E_ARG, "n_probs must be in [0, 16]");
  return 5 + n_probs;
}

int32_t fitoct_summary_host(const fitoct_problem* probs, int32_t n_groups, int32_t chains,
                            int32_t iters_saved, const double* draws,
                            const fitoct_summary_config* cfg, double* out) {
  return guarded(__func__, [&]() -> int32_t {
    Shape s;
    const int rc = check_args("summary", true, probs, n_groups, chains, iters_saved, draws, cfg, out, s);
    return rc ? rc : summary_host(s, draws, cfg, out);
  });
}

int32_t fitoct_summary_device(const fitoct_problem* probs, int32_t n_groups, int32_t chains,
                              int32_t iters_saved, const void* d_draws,
                              const fitoct_summary_config* cfg, void* stream, double* out) {
  return guarded(__func__, [&]() -> int32_t {
    return summary_device_checked(probs, n_groups, chains, iters_saved, d_draws, cfg, stream, out);
  });
}

int32_t fitoct_plan_summary(fitoct_plan* pl, const fitoct_summary_config* cfg, double* out) {
  return guarded(__func__, [&]() -> int32_t {
    if (!pl || !cfg || !out) return fail(FITOCT_E_ARG, "summary: NULL argument");
    if (pl->launched)
      return fail(FITOCT_E_ARG, "plan is running: call fitoct_plan_wait first");
    if (!pl->ran) return fail(FITOCT_E_ARG, "plan has not run");
    const bool group = !pl->shards.empty();
    if (group && !pl->gather_dst)
      return fail(FITOCT_E_ARG, "the device-list run left its shards in per-device buffers: pass "
                                "a d_draws to the run, the summary needs the draws in one buffer");
    fitoct_summary_config c = *cfg;
    c.device = group ? pl->gather_dev : pl->cfg.device;
    return summary_device_checked(&pl->prob, 1, pl->kp.chains, pl->kp.iters_saved,
                                  group ? pl->gather_dst : (void*)pl->last_draws, &c, nullptr, out);
  });
}

int32_t fitoct_batch_summary(fitoct_batch* b, const fitoct_summary_config* cfg, double* out) {
  return guarded(__func__, [&]() -> int32_t {
    if (!b || !cfg || !out) return fail(FITOCT_E_ARG, "summary: NULL argument");
    if (!b->ran) return fail(FITOCT_E_ARG, "batch has not run");
    const bool group = !b->subs.empty();
    if (group && !b->gather_dst)
      return fail(FITOCT_E_ARG, "the device-list run left its files in per-device buffers: pass "
                                "a d_draws to the run, the summary needs the draws in one buffer");
    std::vector<fitoct_problem> probs;
    if (group) {
      for (const fitoct_batch* sb : b->subs)
        for (const fitoct_plan* pl : sb->plans) probs.push_back(pl->prob);
    } else {
      for (const fitoct_plan* pl : b->plans) probs.push_back(pl->prob);
    }
    const fitoct_plan* p0 = group ? b->subs[0]->plans[0] : b->plans[0];
    fitoct_summary_config c = *cfg;
    c.device = group ? b->gather_dev : b->cfg.device;
    return summary_device_checked(probs.data(), (int32_t)probs.size(), b->cfg.chains,
                                  p0->kp.iters_saved,
                                  group ? b->gather_dst : (void*)p0->last_draws, &c, nullptr, out);
  });
}

}  // extern "C"
