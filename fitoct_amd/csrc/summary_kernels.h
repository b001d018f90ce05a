// What the device routes of the posterior summary (summary_device.hip), of the rank
// diagnostics (monitor_device.hip) and of the posterior curves (curves_device.hip) share
// (DESIGN.md §4): the argument checks and the shape arithmetic, the staging, moments and
// autocovariance kernels, the exact radix select of the quantiles with its set-up, the device
// buffers, the split of the output columns into passes, and the rounds of Geyer's rule over
// lag blocks.  Included by those translation units only; everything has internal linkage, so
// each object carries its own copy of the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fitoct.h"
#include "host_internal.h"
#include "summary_shared.h"

namespace fitoct {
namespace {

constexpr int64_t DEFAULT_STAGING_BYTES = (int64_t)256 << 20;
constexpr int MAX_PROBS = 16;
constexpr int LAG_BLOCK = 64;           // lags per acov_kernel workgroup: one per lane
constexpr int STAGE_ROWS = 32;          // rows of one chain per stage_kernel workgroup
constexpr int STAGE_THREADS = 256;
constexpr int ACOV_WAVES = 4;
constexpr int ACOV_TILE = 512;          // series elements per LDS tile and wave
constexpr int QT_MAX = 2 * MAX_PROBS;   // order statistics per column: x[lo], x[hi] per probability
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

// `who` names the caller in the messages ("summary", "monitor"); the rank diagnostics take no
// probabilities (with_probs false: n_probs and probs are not read, np = 0)
int check_args(const std::string& who, bool with_probs, const fitoct_problem* probs, int n_groups,
               int chains, int iters_saved, const void* draws, const fitoct_summary_config* cfg,
               const double* out, Shape& s) {
  if (!probs || !cfg || !out || !draws)
    return fail(FITOCT_E_ARG, who + ": NULL argument (problems, draws, config or out)");
  if (n_groups < 1 || chains < 1 || iters_saved < 1)
    return fail(FITOCT_E_ARG, who + ": need n_groups, chains and iters_saved >= 1");
  if (chains > (1 << 30)) return fail(FITOCT_E_ARG, who + ": too many chains");
  const fitoct_problem& p0 = probs[0];
  const int D = model_dim(p0.prior_type, p0.Nn);
  if (D < 0) return fail(FITOCT_E_ARG, who + ": unknown prior_type");
  if (p0.prior_type != FITOCT_MODEL_MONOEXP && (p0.Nn < 2 || p0.Nn > 24))
    return fail(FITOCT_E_ARG, who + ": Nn must be in [2, 24]");
  for (int g = 1; g < n_groups; ++g)
    if (probs[g].prior_type != p0.prior_type || probs[g].Nn != p0.Nn ||
        (probs[g].prior_PD != 0) != (p0.prior_PD != 0))
      return fail(FITOCT_E_ARG, who + ": groups must share prior_type, Nn and prior_PD (group " +
                                    std::to_string(g) + ")");
  if (cfg->first_iter < 0) return fail(FITOCT_E_ARG, who + ": first_iter is negative");
  if ((int64_t)iters_saved - cfg->first_iter < 4)
    return fail(FITOCT_E_ARG, who + ": need >= 4 post-warmup iterations (iters_saved - first_iter)");
  if (with_probs) {
    if (cfg->n_probs < 0 || cfg->n_probs > MAX_PROBS)
      return fail(FITOCT_E_ARG, who + ": n_probs must be in [0, 16]");
    for (int i = 0; i < cfg->n_probs; ++i)
      if (!(cfg->probs[i] >= 0.0 && cfg->probs[i] <= 1.0))
        return fail(FITOCT_E_ARG, who + ": probs[" + std::to_string(i) + "] is not in [0, 1]");
  }
  if (cfg->max_staging_bytes < 0)
    return fail(FITOCT_E_ARG, who + ": max_staging_bytes is negative");
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
  s.np = with_probs ? cfg->n_probs : 0;
  s.width = 5 + s.np;
  s.S = (int64_t)chains * s.n;
  s.lscale.resize(n_groups);
  for (int g = 0; g < n_groups; ++g) s.lscale[g] = probs[g].lambda_scale;
  return FITOCT_OK;
}

// the checks of a device route that need the runtime: the ordinal, and d_draws a device buffer
int check_device(const std::string& who, const fitoct_summary_config* cfg, const void* d_draws) {
  if (cfg->device < 0) return fail(FITOCT_E_ARG, who + ": device is negative");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    return fail(FITOCT_E_NODEVICE, "no HIP device visible");
  }
  if (cfg->device >= ndev) return fail(FITOCT_E_ARG, who + ": device ordinal out of range");
  int bdev = -1;
  if (buffer_device(d_draws, bdev) != FITOCT_OK) {   // also a pointer the runtime does not know
    (void)hipGetLastError();
    return fail(FITOCT_E_ARG, who + ": d_draws must be a device buffer (hipMalloc)");
  }
  return FITOCT_OK;
}

// output column j of a raw row (7 sampler columns, then the parameter columns)
FITOCT_HD inline double column_value(const OutModel& m, int j, const double* raw) {
  return j < 7 ? raw[j] : out_value(m, out_spec(m, j - 7), raw + 7);
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

// Output columns per pass: as many as the staging cap holds at bytes_per_column each (never
// less than one); the passes are c0 = 0, ncc_max, ... with min(ncc_max, P - c0) columns.
inline int columns_per_pass(const Shape& s, const fitoct_summary_config* cfg,
                            int64_t bytes_per_column) {
  const int64_t cap = cfg->max_staging_bytes > 0 ? cfg->max_staging_bytes : DEFAULT_STAGING_BYTES;
  return (int)std::max<int64_t>(1, std::min<int64_t>(s.P, cap / bytes_per_column));
}

// Device buffers of the moments and of Geyer's rounds, for up to pairs_max series sets.
struct EssBufs {
  DevBuf mom, flags, acov, act;
  int alloc(int64_t pairs_max, int m) {
    FITOCT_TRY(mom.alloc((size_t)pairs_max * m * 4 * sizeof(double)));
    FITOCT_TRY(flags.alloc((size_t)pairs_max * m * sizeof(int)));
    FITOCT_TRY(acov.alloc((size_t)pairs_max * LAG_BLOCK * sizeof(double)));
    FITOCT_TRY(act.alloc((size_t)pairs_max * sizeof(int)));
    return FITOCT_OK;
  }
};

// moments_kernel over X[pairs][k.C][k.n] and its read-back, queued on st (not synchronised)
inline int queue_moments(const KShape& k, const double* X, int64_t pairs, EssBufs& b,
                         hipStream_t st, std::vector<double>& h_mom, std::vector<int>& h_flags) {
  moments_kernel<<<dim3((unsigned)(pairs * k.m)), dim3(64), 0, st>>>(k, X, b.mom.as<double>(),
                                                                     b.flags.as<int>());
  HIP_TRY(hipGetLastError());
  h_mom.resize((size_t)pairs * k.m * 4);
  h_flags.resize((size_t)pairs * k.m);
  HIP_TRY(hipMemcpyAsync(h_mom.data(), b.mom.p, sizeof(double) * h_mom.size(),
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_flags.data(), b.flags.p, sizeof(int) * h_flags.size(),
                         hipMemcpyDeviceToHost, st));
  return FITOCT_OK;
}

// Pooled mean and sd (n - 1) of one pair from the moments of its m split chains of h draws
// (moments_kernel's rows mo[m][4]; S = m / 2 * n values): the sums are added in chain order,
// the centred sums of squares combined by Chan et al.'s update; the middle draw of an odd n
// is carried separately.
inline void pooled_mean_sd(const double* mo, int n, int h, int m, int64_t S, double& mean,
                           double& sd) {
  double sum = 0.0;
  for (int j = 0; j < m; ++j) sum += mo[4 * j + 2];
  if (n & 1)
    for (int j = 0; j < m; j += 2) sum += mo[4 * j + 3];
  mean = sum / (double)S;
  double ssq = 0.0;
  for (int j = 0; j < m; ++j) {
    const double d = mo[4 * j] - mean;
    ssq += mo[4 * j + 1] + h * (d * d);
  }
  if (n & 1)
    for (int j = 0; j < m; j += 2) {
      const double d = mo[4 * j + 3] - mean;
      ssq += d * d;
    }
  sd = sqrt(ssq / (double)(S - 1));
}

// n_eff of the pairs listed in `active` (ess[pair] is written): autocovariance in blocks of 64
// lags, Geyer's rule (ess_moments) on the host block by block, the next block only for the
// pairs that have not terminated.  h_mom: the moments of X (queue_moments, synchronised), still
// in b.mom on the device.
inline int ess_rounds(const KShape& k, const double* X, EssBufs& b, hipStream_t st,
                      const std::vector<double>& h_mom, std::vector<int> active,
                      std::vector<double>& ess) {
  std::vector<std::vector<double>> lags(active.size());   // lag blocks computed so far
  std::vector<int> slot(active.size());                   // active[a]'s entry of lags
  for (size_t a = 0; a < active.size(); ++a) slot[a] = (int)a;
  std::vector<double> h_acov, cm(k.m), cv(k.m);
  for (int lag0 = 0; !active.empty(); lag0 += LAG_BLOCK) {
    HIP_TRY(hipMemcpyAsync(b.act.p, active.data(), sizeof(int) * active.size(),
                           hipMemcpyHostToDevice, st));
    acov_kernel<<<dim3((unsigned)active.size()), dim3(ACOV_WAVES * 64), 0, st>>>(
        k, X, b.mom.as<double>(), b.act.as<int>(), lag0, b.acov.as<double>());
    HIP_TRY(hipGetLastError());
    h_acov.resize(active.size() * LAG_BLOCK);
    HIP_TRY(hipMemcpyAsync(h_acov.data(), b.acov.p, sizeof(double) * h_acov.size(),
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<int> still, still_slot;
    for (size_t a = 0; a < active.size(); ++a) {
      std::vector<double>& ac = lags[slot[a]];
      ac.insert(ac.end(), h_acov.begin() + a * LAG_BLOCK, h_acov.begin() + (a + 1) * LAG_BLOCK);
      const double* mo = h_mom.data() + (size_t)active[a] * k.m * 4;
      for (int j = 0; j < k.m; ++j) {
        cm[j] = mo[4 * j];
        cv[j] = mo[4 * j + 1] / (k.h - 1);
      }
      try {
        ess[active[a]] = ess_moments(cm.data(), cv.data(), k.m, k.h, [&](int lag) {
          if (lag >= k.h) return 0.0;
          if ((size_t)lag >= ac.size()) throw NeedLag{};
          return ac[lag];
        });
      } catch (const NeedLag&) {
        still.push_back(active[a]);
        still_slot.push_back(slot[a]);
      }
    }
    active.swap(still);
    slot.swap(still_slot);
  }
  return FITOCT_OK;
}

// ---- exact radix select (qhist_kernel / qselect_kernel) -------------------------------------
// Device buffers of the select, for up to pairs_max pairs.
struct SelectBufs {
  DevBuf hist, rank, pre, slot, uniq, nuniq;
  int alloc(int64_t pairs_max) {
    FITOCT_TRY(hist.alloc((size_t)pairs_max * QT_MAX * 256 * sizeof(unsigned long long)));
    FITOCT_TRY(rank.alloc((size_t)pairs_max * QT_MAX * sizeof(long long)));
    FITOCT_TRY(pre.alloc((size_t)pairs_max * QT_MAX * sizeof(unsigned long long)));
    FITOCT_TRY(slot.alloc((size_t)pairs_max * QT_MAX * sizeof(int)));
    FITOCT_TRY(uniq.alloc((size_t)pairs_max * QT_MAX * sizeof(unsigned long long)));
    FITOCT_TRY(nuniq.alloc((size_t)pairs_max * sizeof(int)));
    return FITOCT_OK;
  }
};
// The order statistics every pair needs, x[lo] and x[hi] of each probability, as the initial
// ranks of up to pairs_max pairs (and the one distinct prefix every pair starts with).
struct SelectRanks {
  std::vector<long long> rank0;
  std::vector<int> one;
  SelectRanks(const std::vector<QIndex>& qidx, int64_t pairs_max)
      : rank0((size_t)pairs_max * QT_MAX, 0), one((size_t)pairs_max, 1) {
    for (size_t i = 0; i < qidx.size(); ++i)
      for (int64_t p = 0; p < pairs_max; ++p) {
        rank0[p * QT_MAX + 2 * i] = qidx[i].lo;
        rank0[p * QT_MAX + 2 * i + 1] = qidx[i].hi;
      }
  }
};
// workgroups of qhist_kernel per pair
inline int qhist_blocks(int64_t S) {
  return (int)std::max<int64_t>(
      1, std::min<int64_t>(1024, (S + QHIST_THREADS * QHIST_PER_THREAD - 1) /
                                     (QHIST_THREADS * QHIST_PER_THREAD)));
}
// The eight passes over X[pairs][S] for T targets per pair and the read-back of the selected
// keys h_keys[pairs][QT_MAX], queued on st (not synchronised).
inline int queue_select(const double* X, int64_t pairs, int64_t S, int T, int nblk,
                        const SelectBufs& b, const SelectRanks& r, hipStream_t st,
                        std::vector<unsigned long long>& h_keys) {
  QState qs{T, S, b.hist.as<unsigned long long>(), b.rank.as<long long>(),
            b.pre.as<unsigned long long>(), b.slot.as<int>(), b.uniq.as<unsigned long long>(),
            b.nuniq.as<int>()};
  HIP_TRY(hipMemsetAsync(b.hist.p, 0, (size_t)pairs * QT_MAX * 256 * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(b.pre.p, 0, (size_t)pairs * QT_MAX * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(b.slot.p, 0, (size_t)pairs * QT_MAX * sizeof(int), st));
  HIP_TRY(hipMemsetAsync(b.uniq.p, 0, (size_t)pairs * QT_MAX * sizeof(unsigned long long), st));
  HIP_TRY(hipMemcpyAsync(b.rank.p, r.rank0.data(), (size_t)pairs * QT_MAX * sizeof(long long),
                         hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(b.nuniq.p, r.one.data(), (size_t)pairs * sizeof(int),
                         hipMemcpyHostToDevice, st));
  for (int pass = 0; pass < 8; ++pass) {
    qhist_kernel<<<dim3((unsigned)(pairs * nblk)), dim3(QHIST_THREADS), 0, st>>>(X, qs, pass, nblk);
    HIP_TRY(hipGetLastError());
    qselect_kernel<<<dim3((unsigned)pairs), dim3(64), 0, st>>>(qs);
    HIP_TRY(hipGetLastError());
  }
  h_keys.resize((size_t)pairs * QT_MAX);
  HIP_TRY(hipMemcpyAsync(h_keys.data(), b.pre.p, sizeof(unsigned long long) * h_keys.size(),
                         hipMemcpyDeviceToHost, st));
  return FITOCT_OK;
}

}  // namespace
}  // namespace fitoct
