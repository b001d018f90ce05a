// The one compiled copy of what the device routes of the posterior summary
// (summary_device.hip), of the rank diagnostics (monitor_device.hip) and of the posterior curves
// (curves_device.hip) share (posterior_common.h): the argument checks and the
// shape arithmetic, where a plan's or a batch's last run left its draws, the staging, moments
// and autocovariance kernels, the exact radix select of the quantiles with its set-up, the
// device buffers, the rounds of Geyer's rule over lag blocks, and the head of a table row.
//
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
#include "posterior_common.h"

namespace fitoct {

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

// ---- where the last run's draws lie (plan_internal.h) ----------------------------------------
fitoct_problem with_data(const fitoct_plan* pl) {
  fitoct_problem p = pl->prob;
  if (pl->h_xyu.size() == 3 * (size_t)p.N) {
    p.x = pl->h_xyu.data();
    p.y = p.x + p.N;
    p.uy = p.y + p.N;
  }
  p.B = pl->h_B.empty() ? nullptr : pl->h_B.data();
  return p;
}

int plan_where(fitoct_plan* pl, const char* needs, Where& w) {
  if (pl->launched) return fail(FITOCT_E_ARG, "plan is running: call fitoct_plan_wait first");
  if (!pl->ran) return fail(FITOCT_E_ARG, "plan has not run");
  const bool group = !pl->shards.empty();
  if (group && !pl->gather_dst)
    return fail(FITOCT_E_ARG, std::string("the device-list run left its shards in per-device "
                                          "buffers: pass a d_draws to the run, ") +
                                  needs + " the draws in one buffer");
  w.probs.push_back(with_data(pl));
  w.chains = pl->kp.chains;
  w.iters_saved = pl->kp.iters_saved;
  w.device = group ? pl->gather_dev : pl->cfg.device;
  w.draws = (const char*)(group ? pl->gather_dst : (void*)pl->last_draws);
  return FITOCT_OK;
}

int batch_where(fitoct_batch* b, const char* needs, Where& w) {
  if (!b->ran) return fail(FITOCT_E_ARG, "batch has not run");
  const bool group = !b->subs.empty();
  if (group && !b->gather_dst)
    return fail(FITOCT_E_ARG, std::string("the device-list run left its files in per-device "
                                          "buffers: pass a d_draws to the run, ") +
                                  needs + " the draws in one buffer");
  if (group) {
    for (const fitoct_batch* sb : b->subs)
      for (const fitoct_plan* pl : sb->plans) w.probs.push_back(with_data(pl));
  } else {
    for (const fitoct_plan* pl : b->plans) w.probs.push_back(with_data(pl));
  }
  const fitoct_plan* p0 = group ? b->subs[0]->plans[0] : b->plans[0];
  w.chains = b->cfg.chains;
  w.iters_saved = p0->kp.iters_saved;
  w.device = group ? b->gather_dev : b->cfg.device;
  w.draws = (const char*)(group ? b->gather_dst : (void*)p0->last_draws);
  w.group_bytes = sizeof(double) * (size_t)w.chains * w.iters_saved *
                  (model_dim(p0->prob.prior_type, p0->prob.Nn) + 8);
  return FITOCT_OK;
}

namespace {

constexpr int ACOV_WAVES = 4;
constexpr int ACOV_TILE = 512;          // series elements per LDS tile and wave
constexpr int QHIST_THREADS = 256;
constexpr int QHIST_PER_THREAD = 16;    // elements per thread and grid stride

// ---- kernels --------------------------------------------------------------------------------
// one workgroup per (group, chain, block of STAGE_ROWS rows)
__global__ __launch_bounds__(STAGE_THREADS) void stage_kernel(KShape k, const double* draws,
                                                              const double* lscale, double* X) {
  extern __shared__ double tile[];   // [STAGE_ROWS][Wp]
  const int Wp = k.W | 1;
  const RowBlock rb = load_row_tile(k, draws, tile);
  const int g = rb.g, c = rb.c, i0 = rb.i0, rows = rb.rows;
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

struct NeedLag {};   // Geyer's rule asked for a lag block that has not been computed yet

// Pooled mean and sd (n - 1) of one pair from the moments of its m split chains of h draws
// (moments_kernel's rows mo[m][4]; S = m / 2 * n values): the sums are added in chain order,
// the centred sums of squares combined by Chan et al.'s update; the middle draw of an odd n
// is carried separately.
void pooled_mean_sd(const double* mo, int n, int h, int m, int64_t S, double& mean, double& sd) {
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

}  // namespace

// ---- what the users queue -------------------------------------------------------------------
int queue_stage(const KShape& k, const void* d_draws, const double* lscale, double* X,
                hipStream_t st) {
  stage_kernel<<<dim3((unsigned)((int64_t)row_blocks(k.n) * k.C * k.G)), dim3(STAGE_THREADS),
                 row_tile_bytes(k.W), st>>>(k, (const double*)d_draws, lscale, X);
  HIP_TRY(hipGetLastError());
  return FITOCT_OK;
}

int EssBufs::alloc(int64_t pairs_max, int m) {
  FITOCT_TRY(mom.alloc((size_t)pairs_max * m * 4 * sizeof(double)));
  FITOCT_TRY(flags.alloc((size_t)pairs_max * m * sizeof(int)));
  FITOCT_TRY(acov.alloc((size_t)pairs_max * LAG_BLOCK * sizeof(double)));
  FITOCT_TRY(act.alloc((size_t)pairs_max * sizeof(int)));
  return FITOCT_OK;
}

int queue_moments(const KShape& k, const double* X, int64_t pairs, EssBufs& b, hipStream_t st,
                  std::vector<double>& h_mom, std::vector<int>& h_flags) {
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

int ess_rounds(const KShape& k, const double* X, EssBufs& b, hipStream_t st,
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
      split_moments(h_mom.data() + (size_t)active[a] * k.m * 4, k.m, k.h, cm.data(), cv.data());
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
int SelectBufs::alloc(int64_t pairs_max) {
  FITOCT_TRY(hist.alloc((size_t)pairs_max * QT_MAX * 256 * sizeof(unsigned long long)));
  FITOCT_TRY(rank.alloc((size_t)pairs_max * QT_MAX * sizeof(long long)));
  FITOCT_TRY(pre.alloc((size_t)pairs_max * QT_MAX * sizeof(unsigned long long)));
  FITOCT_TRY(slot.alloc((size_t)pairs_max * QT_MAX * sizeof(int)));
  FITOCT_TRY(uniq.alloc((size_t)pairs_max * QT_MAX * sizeof(unsigned long long)));
  FITOCT_TRY(nuniq.alloc((size_t)pairs_max * sizeof(int)));
  return FITOCT_OK;
}

SelectRanks::SelectRanks(const Shape& s, const fitoct_summary_config* cfg, int64_t pairs_max)
    : qidx(s.np), rank0((size_t)pairs_max * QT_MAX, 0), one((size_t)pairs_max, 1) {
  for (int i = 0; i < s.np; ++i) {
    qidx[i] = quantile_index(s.S, cfg->probs[i]);
    for (int64_t p = 0; p < pairs_max; ++p) {
      rank0[p * QT_MAX + 2 * i] = qidx[i].lo;
      rank0[p * QT_MAX + 2 * i + 1] = qidx[i].hi;
    }
  }
}

int qhist_blocks(int64_t S) {
  return (int)std::max<int64_t>(
      1, std::min<int64_t>(1024, (S + QHIST_THREADS * QHIST_PER_THREAD - 1) /
                                     (QHIST_THREADS * QHIST_PER_THREAD)));
}

int queue_select(const double* X, int64_t pairs, int64_t S, int T, int nblk, const SelectBufs& b,
                 const SelectRanks& r, hipStream_t st, std::vector<unsigned long long>& h_keys) {
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

// ---- rows -----------------------------------------------------------------------------------
bool pair_row(const Shape& s, int64_t p, const std::vector<double>& h_mom,
              const std::vector<int>& h_flags, const std::vector<unsigned long long>& h_keys,
              const SelectRanks& r, bool nan, double* row, int width, int sd_at, bool* constant) {
  int fl = nan ? 1 : 0;
  for (int j = 0; j < s.m; ++j) fl |= h_flags[(size_t)p * s.m + j];
  if (constant) *constant = !(fl & 2);
  if (fl & 1) {
    for (int i = 0; i < width; ++i) row[i] = NAN;
    return false;
  }
  pooled_mean_sd(h_mom.data() + (size_t)p * s.m * 4, s.n, s.h, s.m, s.S, row[0], row[sd_at]);
  for (int i = 0; i < s.np; ++i)
    row[sd_at + 1 + i] = quantile_lerp(key_value(h_keys[p * QT_MAX + 2 * i]),
                                       key_value(h_keys[p * QT_MAX + 2 * i + 1]), r.qidx[i].frac);
  return true;
}

}  // namespace fitoct
