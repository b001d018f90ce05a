// Posterior summary of draws that stay in HBM (include/fitoct.h "posterior summary";
// DESIGN.md §4.9): rstan::summary(fit, pars)$summary -- mean, se_mean, sd, type-7 quantiles,
// n_eff, Rhat per output column -- computed on the device from the sampler's raw draws
// buffer, and the same computation on the host (fitoct_summary_host, on top of
// split_rhat_ess and std::nth_element) that the device route is tested against.
//
// Device route, per pass over a chunk of output columns:
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
#include "summary_shared.h"

namespace fitoct {
namespace {

constexpr int64_t DEFAULT_STAGING_BYTES = (int64_t)256 << 20;
constexpr int MAX_PROBS = 16;
constexpr int QT_MAX = 2 * MAX_PROBS;   // order statistics per column: x[lo], x[hi] per probability
constexpr int LAG_BLOCK = 64;           // lags per acov_kernel workgroup: one per lane
constexpr int STAGE_ROWS = 32;          // rows of one chain per stage_kernel workgroup
constexpr int STAGE_THREADS = 256;
constexpr int ACOV_WAVES = 4;
constexpr int ACOV_TILE = 512;          // series elements per LDS tile and wave
constexpr int QHIST_THREADS = 256;
constexpr int QHIST_PER_THREAD = 16;    // elements per thread and grid stride

// What a call computes: shapes checked by check_args.
struct Shape {
  int G = 0, C = 0, I = 0, W = 0;   // groups, chains, saved iterations, raw columns
  int first = 0, n = 0, h = 0, m = 0;   // skipped, post-warmup, half length, split chains
  int P = 0, np = 0, width = 0;     // output columns, probabilities, 5 + np
  int64_t S = 0;                    // pooled draws of one column
  OutModel model{};                 // lambda_scale: per group, in lscale
  std::vector<double> lscale;
};

int check_args(const fitoct_problem* probs, int n_groups, int chains, int iters_saved,
               const void* draws, const fitoct_summary_config* cfg, const double* out,
               Shape& s) {
  if (!probs || !cfg || !out || !draws)
    return fail(FITOCT_E_ARG, "summary: NULL argument (problems, draws, config or out)");
  if (n_groups < 1 || chains < 1 || iters_saved < 1)
    return fail(FITOCT_E_ARG, "summary: need n_groups, chains and iters_saved >= 1");
  if (chains > (1 << 30)) return fail(FITOCT_E_ARG, "summary: too many chains");
  const fitoct_problem& p0 = probs[0];
  const int D = model_dim(p0.prior_type, p0.Nn);
  if (D < 0) return fail(FITOCT_E_ARG, "summary: unknown prior_type");
  if (p0.prior_type != FITOCT_MODEL_MONOEXP && (p0.Nn < 2 || p0.Nn > 24))
    return fail(FITOCT_E_ARG, "summary: Nn must be in [2, 24]");
  for (int g = 1; g < n_groups; ++g)
    if (probs[g].prior_type != p0.prior_type || probs[g].Nn != p0.Nn ||
        (probs[g].prior_PD != 0) != (p0.prior_PD != 0))
      return fail(FITOCT_E_ARG, "summary: groups must share prior_type, Nn and prior_PD (group " +
                                    std::to_string(g) + ")");
  if (cfg->first_iter < 0) return fail(FITOCT_E_ARG, "summary: first_iter is negative");
  if ((int64_t)iters_saved - cfg->first_iter < 4)
    return fail(FITOCT_E_ARG, "summary: need >= 4 post-warmup iterations (iters_saved - first_iter)");
  if (cfg->n_probs < 0 || cfg->n_probs > MAX_PROBS)
    return fail(FITOCT_E_ARG, "summary: n_probs must be in [0, 16]");
  for (int i = 0; i < cfg->n_probs; ++i)
    if (!(cfg->probs[i] >= 0.0 && cfg->probs[i] <= 1.0))
      return fail(FITOCT_E_ARG, "summary: probs[" + std::to_string(i) + "] is not in [0, 1]");
  if (cfg->max_staging_bytes < 0)
    return fail(FITOCT_E_ARG, "summary: max_staging_bytes is negative");
  s.G = n_groups;
  s.C = chains;
  s.I = iters_saved;
  s.W = D + 8;
  s.first = cfg->first_iter;
  s.n = iters_saved - cfg->first_iter;
  s.h = s.n / 2;   // the middle draw is dropped when n is odd
  s.m = 2 * chains;
  s.model = {p0.prior_type, p0.Nn, D, p0.prior_PD ? 1 : 0, p0.lambda_scale};
  s.P = 7 + out_n_params(s.model);
  s.np = cfg->n_probs;
  s.width = 5 + s.np;
  s.S = (int64_t)chains * s.n;
  s.lscale.resize(n_groups);
  for (int g = 0; g < n_groups; ++g) s.lscale[g] = probs[g].lambda_scale;
  return FITOCT_OK;
}

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

// output column j of a raw row (7 sampler columns, then the parameter columns)
FITOCT_HD inline double column_value(const OutModel& m, int j, const double* raw) {
  return j < 7 ? raw[j] : out_value(m, out_spec(m, j - 7), raw + 7);
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

// ---- kernels --------------------------------------------------------------------------------
// What every kernel needs of the call (by value: a few words).
struct KShape {
  int G, C, I, W, first, n, h, m;
  int c0, ncc;          // this pass: first output column and number of columns
  OutModel model;
};

// X[pair = g * ncc + jc][chain][n]
__device__ inline const double* chain_series(const double* X, const KShape& k, int64_t pair,
                                             int chain) {
  return X + ((size_t)pair * k.C + chain) * k.n;
}

// one workgroup per (group, chain, block of STAGE_ROWS rows)
__global__ __launch_bounds__(STAGE_THREADS) void stage_kernel(KShape k, const double* draws,
                                                              const double* lscale, double* X) {
  extern __shared__ double tile[];   // [STAGE_ROWS][Wp], Wp odd: rows land on different banks
  const int Wp = k.W | 1;
  const int rblocks = (k.n + STAGE_ROWS - 1) / STAGE_ROWS;
  int64_t b = blockIdx.x;
  const int rb = (int)(b % rblocks);
  b /= rblocks;
  const int c = (int)(b % k.C), g = (int)(b / k.C);
  const int i0 = rb * STAGE_ROWS, rows = min(STAGE_ROWS, k.n - i0);
  const double* src = draws + (((size_t)g * k.C + c) * k.I + k.first + i0) * k.W;
  for (int t = threadIdx.x; t < rows * k.W; t += STAGE_THREADS) {
    const int r = t / k.W;
    tile[r * Wp + (t - r * k.W)] = src[t];
  }
  __syncthreads();
  OutModel m = k.model;
  m.lambda_scale = lscale[g];
  for (int t = threadIdx.x; t < k.ncc * STAGE_ROWS; t += STAGE_THREADS) {
    const int jc = t / STAGE_ROWS, r = t % STAGE_ROWS;
    if (r < rows)
      X[(((size_t)g * k.ncc + jc) * k.C + c) * k.n + i0 + r] =
          column_value(m, k.c0 + jc, tile + r * Wp);
  }
}

__device__ inline double wave_sum(double v) {   // butterfly: every lane gets the same bits
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// mom[pair][split chain][4] = mean, centred sum of squares, sum, the middle draw (first half of
// an odd-length chain; 0 otherwise); flags: bit 0 a NaN, bit 1 a value that differs from the
// chain's first draw.  One wave per (pair, split chain).
__global__ __launch_bounds__(64) void moments_kernel(KShape k, const double* X, double* mom,
                                                     int* flags) {
  const int64_t b = blockIdx.x;
  const int64_t pair = b / k.m;
  const int j = (int)(b % k.m), lane = threadIdx.x;
  const double* base = chain_series(X, k, pair, j >> 1);
  const double* x = base + ((j & 1) ? k.n - k.h : 0);
  const double first = base[0];
  double sum = 0.0;
  int f = 0;
  for (int i = lane; i < k.h; i += 64) {
    const double v = x[i];
    sum += v;
    f |= (v != v ? 1 : 0) | (v != first ? 2 : 0);
  }
  double mid = 0.0;
  if (!(j & 1) && (k.n & 1)) {
    mid = base[k.h];
    f |= (mid != mid ? 1 : 0) | (mid != first ? 2 : 0);
  }
  sum = wave_sum(sum);
  const double mean = sum / k.h;
  double ssq = 0.0;
  for (int i = lane; i < k.h; i += 64) {
    const double d = x[i] - mean;
    ssq += d * d;
  }
  ssq = wave_sum(ssq);
  const int any = (__ballot(f & 1) ? 1 : 0) | (__ballot(f & 2) ? 2 : 0);
  if (lane == 0) {
    double* o = mom + (size_t)b * 4;
    o[0] = mean;
    o[1] = ssq;
    o[2] = sum;
    o[3] = mid;
    flags[b] = any;
  }
}

// acov[a][l] for the a-th active pair: mean over split chains of the biased autocovariance
// at lag lag0 + l.  Wave w takes split chains w, w + 4, ...; lane l takes lag lag0 + l; each
// chain's sum runs over the series in order, the waves' partial means are added in wave order.
__global__ __launch_bounds__(ACOV_WAVES * 64) void acov_kernel(KShape k, const double* X,
                                                               const double* mom, const int* act,
                                                               int lag0, double* acov) {
  __shared__ double A[ACOV_WAVES][ACOV_TILE];                // centred x[i]
  __shared__ double B[ACOV_WAVES][ACOV_TILE + LAG_BLOCK];    // centred x[i + lag0 + l]
  __shared__ double part[ACOV_WAVES][LAG_BLOCK];
  const int64_t pair = act[blockIdx.x];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double tot = 0.0;
  for (int jb = 0; jb < k.m; jb += ACOV_WAVES) {   // (uniform trip count: barriers inside)
    const int j = jb + w;
    const bool on = j < k.m;
    const double* x = on ? chain_series(X, k, pair, j >> 1) + ((j & 1) ? k.n - k.h : 0) : nullptr;
    const double cm = on ? mom[((size_t)pair * k.m + j) * 4] : 0.0;
    double s = 0.0;
    for (int i0 = 0; i0 < k.h; i0 += ACOV_TILE) {
      for (int t = lane; t < ACOV_TILE; t += 64)
        A[w][t] = (on && i0 + t < k.h) ? x[i0 + t] - cm : 0.0;
      for (int t = lane; t < ACOV_TILE + LAG_BLOCK; t += 64) {
        const int64_t idx = (int64_t)i0 + lag0 + t;
        B[w][t] = (on && idx < k.h) ? x[idx] - cm : 0.0;
      }
      __syncthreads();
      for (int t = 0; t < ACOV_TILE; ++t) s += A[w][t] * B[w][t + lane];
      __syncthreads();
    }
    if (on) tot += s / k.h;
  }
  part[w][lane] = tot;
  __syncthreads();
  if (w == 0) {
    double v = part[0][lane];
    for (int q = 1; q < ACOV_WAVES; ++q) v += part[q][lane];
    acov[(size_t)blockIdx.x * LAG_BLOCK + lane] = v / k.m;
  }
}

// Radix-select state of one pair: T targets (order statistics), each with the key prefix found
// so far, its rank among the keys sharing that prefix, and the histogram slot of its prefix
// (targets with equal prefixes share one).
struct QState {
  int T;
  int64_t S;
  unsigned long long* hist;   // [pairs][QT_MAX][256]
  long long* rank;            // [pairs][QT_MAX]
  unsigned long long* pre;    // [pairs][QT_MAX] prefix of each target
  int* slot;                  // [pairs][QT_MAX]
  unsigned long long* uniq;   // [pairs][QT_MAX] distinct prefixes
  int* nuniq;                 // [pairs]
};

// digits of byte `pass` (0 = most significant) of the keys whose higher bytes equal a prefix
__global__ __launch_bounds__(QHIST_THREADS) void qhist_kernel(const double* X, QState q, int pass,
                                                              int nblk) {
  __shared__ unsigned int lh[QT_MAX * 256];
  __shared__ unsigned long long spre[QT_MAX];
  const int64_t pair = blockIdx.x / nblk;
  const int blk = blockIdx.x % nblk;
  const int U = q.nuniq[pair];
  for (int t = threadIdx.x; t < U * 256; t += QHIST_THREADS) lh[t] = 0u;
  if ((int)threadIdx.x < U) spre[threadIdx.x] = q.uniq[pair * QT_MAX + threadIdx.x];
  __syncthreads();
  const double* x = X + (size_t)pair * q.S;
  const int shift = 56 - 8 * pass;
  for (int64_t i = (int64_t)blk * QHIST_THREADS + threadIdx.x; i < q.S;
       i += (int64_t)nblk * QHIST_THREADS) {
    const unsigned long long key = order_key(x[i]);
    const unsigned int digit = (unsigned int)(key >> shift) & 255u;
    const unsigned long long hi = pass == 0 ? 0ull : key >> (shift + 8);
    for (int u = 0; u < U; ++u)
      if (hi == spre[u]) atomicAdd(&lh[u * 256 + digit], 1u);
  }
  __syncthreads();
  unsigned long long* H = q.hist + (size_t)pair * QT_MAX * 256;
  for (int t = threadIdx.x; t < U * 256; t += QHIST_THREADS)
    if (lh[t]) atomicAdd(&H[t], (unsigned long long)lh[t]);
}

// one wave per pair: each target walks its histogram to its digit; then the distinct prefixes
// are renumbered and the histograms cleared for the next pass
__global__ __launch_bounds__(64) void qselect_kernel(QState q) {
  const int64_t pair = blockIdx.x;
  unsigned long long* H = q.hist + (size_t)pair * QT_MAX * 256;
  const int t = threadIdx.x;
  if (t < q.T) {
    const unsigned long long* h = H + (size_t)q.slot[pair * QT_MAX + t] * 256;
    long long r = q.rank[pair * QT_MAX + t], cum = 0;
    int d = 0;
    for (; d < 255; ++d) {
      const long long c = (long long)h[d];
      if (r < cum + c) break;
      cum += c;
    }
    q.rank[pair * QT_MAX + t] = r - cum;
    q.pre[pair * QT_MAX + t] = (q.pre[pair * QT_MAX + t] << 8) | (unsigned long long)d;
  }
  __syncthreads();
  if (t == 0) {
    int U = 0;
    for (int a = 0; a < q.T; ++a) {
      const unsigned long long p = q.pre[pair * QT_MAX + a];
      int u = 0;
      while (u < U && q.uniq[pair * QT_MAX + u] != p) ++u;
      if (u == U) q.uniq[pair * QT_MAX + U++] = p;
      q.slot[pair * QT_MAX + a] = u;
    }
    q.nuniq[pair] = U;
  }
  for (int i = t; i < QT_MAX * 256; i += 64) H[i] = 0ull;
}

// ---- device route ---------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t bytes) {
    HIP_TRY(hipMalloc(&p, bytes ? bytes : 8));
    return FITOCT_OK;
  }
  template <class T>
  T* as() const {
    return (T*)p;
  }
};
// the calling thread's device is put back when the call returns
struct DeviceKeep {
  int dev = -1;
  DeviceKeep() {
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  }
  ~DeviceKeep() {
    if (dev >= 0) (void)hipSetDevice(dev);
  }
};
struct NeedLag {};   // Geyer's rule asked for a lag block that has not been computed yet

#define FITOCT_TRY(expr)          \
  do {                            \
    const int rc_ = (expr);       \
    if (rc_) return rc_;          \
  } while (0)

int summary_device(const Shape& s, const void* d_draws, const fitoct_summary_config* cfg,
                   hipStream_t st, double* out) {
  DeviceKeep keep;
  HIP_TRY(hipSetDevice(cfg->device));
  const int64_t col_bytes = (int64_t)s.G * s.S * (int64_t)sizeof(double);
  const int64_t cap = cfg->max_staging_bytes > 0 ? cfg->max_staging_bytes : DEFAULT_STAGING_BYTES;
  const int ncc_max = (int)std::max<int64_t>(1, std::min<int64_t>(s.P, cap / col_bytes));
  const int64_t pairs_max = (int64_t)s.G * ncc_max;
  const int rblocks = (s.n + STAGE_ROWS - 1) / STAGE_ROWS;
  const int nblk = (int)std::max<int64_t>(
      1, std::min<int64_t>(1024, (s.S + QHIST_THREADS * QHIST_PER_THREAD - 1) /
                                     (QHIST_THREADS * QHIST_PER_THREAD)));
  const int64_t limit = (int64_t)1 << 31;
  if ((int64_t)rblocks * s.C * s.G >= limit || pairs_max * s.m >= limit ||
      pairs_max * nblk >= limit)
    return fail(FITOCT_E_ARG, "summary: shape too large for one launch (lower max_staging_bytes)");
  const int T = 2 * s.np;

  DevBuf X, mom, flags, lscale, acov, act, hist, rank, pre, slot, uniq, nuniq;
  FITOCT_TRY(X.alloc((size_t)pairs_max * s.S * sizeof(double)));
  FITOCT_TRY(mom.alloc((size_t)pairs_max * s.m * 4 * sizeof(double)));
  FITOCT_TRY(flags.alloc((size_t)pairs_max * s.m * sizeof(int)));
  FITOCT_TRY(lscale.alloc((size_t)s.G * sizeof(double)));
  FITOCT_TRY(acov.alloc((size_t)pairs_max * LAG_BLOCK * sizeof(double)));
  FITOCT_TRY(act.alloc((size_t)pairs_max * sizeof(int)));
  if (T > 0) {
    FITOCT_TRY(hist.alloc((size_t)pairs_max * QT_MAX * 256 * sizeof(unsigned long long)));
    FITOCT_TRY(rank.alloc((size_t)pairs_max * QT_MAX * sizeof(long long)));
    FITOCT_TRY(pre.alloc((size_t)pairs_max * QT_MAX * sizeof(unsigned long long)));
    FITOCT_TRY(slot.alloc((size_t)pairs_max * QT_MAX * sizeof(int)));
    FITOCT_TRY(uniq.alloc((size_t)pairs_max * QT_MAX * sizeof(unsigned long long)));
    FITOCT_TRY(nuniq.alloc((size_t)pairs_max * sizeof(int)));
  }
  HIP_TRY(hipMemcpyAsync(lscale.p, s.lscale.data(), sizeof(double) * s.G, hipMemcpyHostToDevice, st));

  // the order statistics every column needs: x[lo], x[hi] of each probability
  std::vector<QIndex> qidx(s.np);
  std::vector<long long> rank0((size_t)pairs_max * QT_MAX, 0);
  std::vector<int> one((size_t)pairs_max, 1);
  for (int i = 0; i < s.np; ++i) {
    qidx[i] = quantile_index(s.S, cfg->probs[i]);
    for (int64_t p = 0; p < pairs_max; ++p) {
      rank0[p * QT_MAX + 2 * i] = qidx[i].lo;
      rank0[p * QT_MAX + 2 * i + 1] = qidx[i].hi;
    }
  }

  std::vector<double> h_mom, h_acov, cm(s.m), cv(s.m), q((size_t)std::max(1, s.np));
  std::vector<int> h_flags, h_act;
  std::vector<unsigned long long> h_keys;
  for (int c0 = 0; c0 < s.P; c0 += ncc_max) {
    const int ncc = std::min(ncc_max, s.P - c0);
    const int64_t pairs = (int64_t)s.G * ncc;
    KShape k{s.G, s.C, s.I, s.W, s.first, s.n, s.h, s.m, c0, ncc, s.model};
    stage_kernel<<<dim3((unsigned)((int64_t)rblocks * s.C * s.G)), dim3(STAGE_THREADS),
                   sizeof(double) * STAGE_ROWS * (s.W | 1), st>>>(
        k, (const double*)d_draws, lscale.as<double>(), X.as<double>());
    HIP_TRY(hipGetLastError());
    moments_kernel<<<dim3((unsigned)(pairs * s.m)), dim3(64), 0, st>>>(k, X.as<double>(),
                                                                       mom.as<double>(),
                                                                       flags.as<int>());
    HIP_TRY(hipGetLastError());
    h_mom.resize((size_t)pairs * s.m * 4);
    h_flags.resize((size_t)pairs * s.m);
    HIP_TRY(hipMemcpyAsync(h_mom.data(), mom.p, sizeof(double) * h_mom.size(),
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_flags.data(), flags.p, sizeof(int) * h_flags.size(),
                           hipMemcpyDeviceToHost, st));

    // quantiles: queued behind the moments, read back after the autocovariance rounds
    if (T > 0) {
      QState qs{T, s.S, hist.as<unsigned long long>(), rank.as<long long>(),
                pre.as<unsigned long long>(), slot.as<int>(), uniq.as<unsigned long long>(),
                nuniq.as<int>()};
      HIP_TRY(hipMemsetAsync(hist.p, 0, (size_t)pairs * QT_MAX * 256 * sizeof(unsigned long long), st));
      HIP_TRY(hipMemsetAsync(pre.p, 0, (size_t)pairs * QT_MAX * sizeof(unsigned long long), st));
      HIP_TRY(hipMemsetAsync(slot.p, 0, (size_t)pairs * QT_MAX * sizeof(int), st));
      HIP_TRY(hipMemsetAsync(uniq.p, 0, (size_t)pairs * QT_MAX * sizeof(unsigned long long), st));
      HIP_TRY(hipMemcpyAsync(rank.p, rank0.data(), (size_t)pairs * QT_MAX * sizeof(long long),
                             hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(nuniq.p, one.data(), (size_t)pairs * sizeof(int),
                             hipMemcpyHostToDevice, st));
      for (int pass = 0; pass < 8; ++pass) {
        qhist_kernel<<<dim3((unsigned)(pairs * nblk)), dim3(QHIST_THREADS), 0, st>>>(
            X.as<double>(), qs, pass, nblk);
        HIP_TRY(hipGetLastError());
        qselect_kernel<<<dim3((unsigned)pairs), dim3(64), 0, st>>>(qs);
        HIP_TRY(hipGetLastError());
      }
      h_keys.resize((size_t)pairs * QT_MAX);
      HIP_TRY(hipMemcpyAsync(h_keys.data(), pre.p, sizeof(unsigned long long) * h_keys.size(),
                             hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));

    // per pair: NaN / constant pattern, pooled mean and sd, Rhat; which pairs need n_eff
    struct Col {
      double mean = NAN, sd = NAN, rhat = NAN, ess = NAN;
      bool has_nan = false, constant = false, done = true;
      std::vector<double> acov;   // lag blocks computed so far
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
      double sum = 0.0;
      for (int j = 0; j < s.m; ++j) sum += mo[4 * j + 2];
      if (s.n & 1)
        for (int j = 0; j < s.m; j += 2) sum += mo[4 * j + 3];
      c.mean = sum / (double)s.S;
      // pooled centred sum of squares from the split chains' own (Chan et al.'s update)
      double ssq = 0.0;
      for (int j = 0; j < s.m; ++j) {
        const double d = mo[4 * j] - c.mean;
        ssq += mo[4 * j + 1] + s.h * (d * d);
      }
      if (s.n & 1)
        for (int j = 0; j < s.m; j += 2) {
          const double d = mo[4 * j + 3] - c.mean;
          ssq += d * d;
        }
      c.sd = sqrt(ssq / (double)(s.S - 1));
      if (c.constant) continue;   // n_eff and Rhat are NaN (split_rhat_ess)
      for (int j = 0; j < s.m; ++j) {
        cm[j] = mo[4 * j];
        cv[j] = mo[4 * j + 1] / (s.h - 1);
      }
      c.rhat = psr_moments(cm.data(), cv.data(), s.m, s.h);
      c.done = false;
      active.push_back((int)p);
    }
    // n_eff: autocovariance in blocks of 64 lags, only for the columns still undecided
    for (int lag0 = 0; !active.empty(); lag0 += LAG_BLOCK) {
      HIP_TRY(hipMemcpyAsync(act.p, active.data(), sizeof(int) * active.size(),
                             hipMemcpyHostToDevice, st));
      acov_kernel<<<dim3((unsigned)active.size()), dim3(ACOV_WAVES * 64), 0, st>>>(
          k, X.as<double>(), mom.as<double>(), act.as<int>(), lag0, acov.as<double>());
      HIP_TRY(hipGetLastError());
      h_acov.resize(active.size() * LAG_BLOCK);
      HIP_TRY(hipMemcpyAsync(h_acov.data(), acov.p, sizeof(double) * h_acov.size(),
                             hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      std::vector<int> still;
      for (size_t a = 0; a < active.size(); ++a) {
        Col& c = cols[active[a]];
        c.acov.insert(c.acov.end(), h_acov.begin() + a * LAG_BLOCK,
                      h_acov.begin() + (a + 1) * LAG_BLOCK);
        const double* mo = h_mom.data() + (size_t)active[a] * s.m * 4;
        for (int j = 0; j < s.m; ++j) {
          cm[j] = mo[4 * j];
          cv[j] = mo[4 * j + 1] / (s.h - 1);
        }
        try {
          c.ess = ess_moments(cm.data(), cv.data(), s.m, s.h, [&](int lag) {
            if (lag >= s.h) return 0.0;
            if ((size_t)lag >= c.acov.size()) throw NeedLag{};
            return c.acov[lag];
          });
          c.done = true;
        } catch (const NeedLag&) {
          still.push_back(active[a]);
        }
      }
      active.swap(still);
    }
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
      put_row(s, row, c.mean, c.sd, q.data(), c.ess, c.rhat);
    }
  }
  return FITOCT_OK;
}

int summary_device_checked(const fitoct_problem* probs, int n_groups, int chains, int iters_saved,
                           const void* d_draws, const fitoct_summary_config* cfg, void* stream,
                           double* out) {
  Shape s;
  FITOCT_TRY(check_args(probs, n_groups, chains, iters_saved, d_draws, cfg, out, s));
  if (cfg->device < 0) return fail(FITOCT_E_ARG, "summary: device is negative");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    return fail(FITOCT_E_NODEVICE, "no HIP device visible");
  }
  if (cfg->device >= ndev) return fail(FITOCT_E_ARG, "summary: device ordinal out of range");
  int bdev = -1;
  if (buffer_device(d_draws, bdev) != FITOCT_OK) {   // also a pointer the runtime does not know
    (void)hipGetLastError();
    return fail(FITOCT_E_ARG, "summary: d_draws must be a device buffer (hipMalloc)");
  }
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
    const int rc = check_args(probs, n_groups, chains, iters_saved, draws, cfg, out, s);
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
