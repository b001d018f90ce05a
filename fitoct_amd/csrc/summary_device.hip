// Posterior summary of draws that stay in HBM (include/fitoct.h "posterior summary";
// DESIGN.md §4.9): rstan::summary(fit, pars)$summary -- mean, se_mean, sd, type-7 quantiles,
// n_eff, Rhat per output column -- computed on the device from the sampler's raw draws
// buffer, and the same computation on the host (fitoct_summary_host, on top of
// split_rhat_ess and std::nth_element) that the device route is tested against.
//
// Device route, per pass over a chunk of output columns, all of it the shared layer's
// (posterior_common.hip, which describes the kernels): queue_stage, queue_moments, queue_select
// for the quantiles, then on the host pair_row (a NaN row, or mean, sd and the quantiles), Rhat
// from the split chains' moments, and ess_rounds for n_eff.  This file launches no kernel of
// its own.  No floating-point atomics anywhere: the results are the same bit for bit from call
// to call.
#include "posterior_common.h"

namespace fitoct {
namespace {

// out row = mean, se_mean, sd, the quantiles, n_eff, Rhat; put_tail: what needs n_eff, once
// mean, sd and the quantiles stand in the row
void put_tail(const Shape& s, double* row, double ess, double rhat) {
  row[1] = ess > 0.0 ? row[2] / sqrt(ess) : NAN;
  row[3 + s.np] = ess;
  row[4 + s.np] = rhat;
}
void put_row(const Shape& s, double* row, double mean, double sd, const double* q, double ess,
             double rhat) {
  row[0] = mean;
  row[2] = sd;
  for (int i = 0; i < s.np; ++i) row[3 + i] = q[i];
  put_tail(s, row, ess, rhat);
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

// ---- device route ---------------------------------------------------------------------------
int summary_device(const Shape& s, const void* d_draws, const fitoct_summary_config* cfg,
                   hipStream_t st, double* out) {
  DeviceKeep keep;
  HIP_TRY(hipSetDevice(cfg->device));
  const int64_t col_bytes = (int64_t)s.G * s.S * (int64_t)sizeof(double);
  const int ncc_max = (int)items_per_pass(cfg, s.P, col_bytes);
  const int64_t pairs_max = (int64_t)s.G * ncc_max;
  const int nblk = qhist_blocks(s.S);
  const int64_t limit = (int64_t)1 << 31;
  if (row_grid(s) >= limit || pairs_max * s.m >= limit || pairs_max * nblk >= limit)
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
  const SelectRanks ranks(s, cfg, pairs_max);

  std::vector<double> h_mom, cm(s.m), cv(s.m);
  std::vector<int> h_flags;
  std::vector<unsigned long long> h_keys;
  for (int c0 = 0; c0 < s.P; c0 += ncc_max) {
    const int ncc = std::min(ncc_max, s.P - c0);
    const int64_t pairs = (int64_t)s.G * ncc;
    const KShape k = kshape(s, c0, ncc);
    FITOCT_TRY(queue_stage(k, d_draws, lscale.as<double>(), X.as<double>(), st));
    FITOCT_TRY(queue_moments(k, X.as<double>(), pairs, eb, st, h_mom, h_flags));
    // quantiles: queued behind the moments
    if (T > 0) FITOCT_TRY(queue_select(X.as<double>(), pairs, s.S, T, nblk, sel, ranks, st, h_keys));
    HIP_TRY(hipStreamSynchronize(st));

    // per pair: a NaN row, or mean, sd and the quantiles; Rhat; which pairs need n_eff
    auto row_of = [&](int64_t p) {
      return out + ((size_t)(p / ncc) * s.P + c0 + (int)(p % ncc)) * s.width;
    };
    std::vector<double> rhat((size_t)pairs, NAN), ess((size_t)pairs, NAN);
    std::vector<char> has_nan((size_t)pairs, 0);
    std::vector<int> active;
    for (int64_t p = 0; p < pairs; ++p) {
      bool constant = false;
      has_nan[p] = !pair_row(s, p, h_mom, h_flags, h_keys, ranks, false, row_of(p), s.width, 2,
                             &constant);
      if (has_nan[p] || constant) continue;   // constant: n_eff and Rhat are NaN (split_rhat_ess)
      split_moments(h_mom.data() + (size_t)p * s.m * 4, s.m, s.h, cm.data(), cv.data());
      rhat[p] = psr_moments(cm.data(), cv.data(), s.m, s.h);
      active.push_back((int)p);
    }
    // n_eff: autocovariance in blocks of 64 lags, only for the columns still undecided
    FITOCT_TRY(ess_rounds(k, X.as<double>(), eb, st, h_mom, active, ess));
    for (int64_t p = 0; p < pairs; ++p)
      if (!has_nan[p]) put_tail(s, row_of(p), ess[p], rhat[p]);
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

// the last run of a plan or of a batch (one body: on_last_run)
template <class Handle>
static int32_t last_run_summary(const char* fn, Handle* h, const fitoct_summary_config* cfg, double* out) {
  return guarded(fn, [&]() -> int32_t {
    return on_last_run(h, "summary", "the summary needs", cfg, out != nullptr,
                       [&](const Where& w, const fitoct_summary_config& c) {
                         return summary_device_checked(w.probs.data(), (int32_t)w.probs.size(), w.chains,
                                                       w.iters_saved, w.draws, &c, nullptr, out);
                       });
  });
}

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
  return last_run_summary(__func__, pl, cfg, out);
}

int32_t fitoct_batch_summary(fitoct_batch* b, const fitoct_summary_config* cfg, double* out) {
  return last_run_summary(__func__, b, cfg, out);
}

}  // extern "C"
