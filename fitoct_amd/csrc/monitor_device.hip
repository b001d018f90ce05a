// Rank diagnostics of draws that stay in HBM (include/fitoct.h "rank diagnostics"; DESIGN.md
// §4): rstan::monitor's rank-normalised split R-hat, bulk ESS and tail ESS (Vehtari et al.
// 2021) per output column, computed on the device from the sampler's raw draws buffer, and the
// same computation on the host (fitoct_monitor_host, on top of host_model.cpp's monitor_column)
// that the device route is tested against.
//
// Device route, per pass over a chunk of output columns (queue_stage, queue_moments and
// ess_rounds: the shared layer, posterior_common.hip, which holds their kernels):
//   stage_kernel      raw rows -> X[pair][chain][n], the output-layout transform applied;
//   keys_kernel       the S = 2 chains h split draws of a pair, pooled in split-chain order, as
//                     order-preserving 64-bit keys (of x, or of |x - median|);
//   sort              keys only, exact.  S <= FITOCT_MONITOR_SORT_LDS_KEYS: sort_lds_kernel, one
//                     workgroup per pair, a bitonic network in LDS.  Larger: eight stable 8-bit
//                     radix passes, least significant byte first, over tiles of
//                     FITOCT_MONITOR_SORT_TILE keys: rhist_kernel (digit histogram of a tile in
//                     LDS, integer atomics), rscan_kernel (offsets of every digit and tile),
//                     rscatter_kernel (one wave per tile: a key's place among the wave's equal
//                     digits from ballots, so no atomics and a fixed order);
//   pick_kernel       the order statistics the host needs: both ends (a NaN lies there), the two
//                     middle keys (median), x[lo], x[hi] of q05 and q95;
//   rank_kernel       every draw finds the keys below and up to its own value by bisection of the
//                     sorted keys: average rank over ties (== on the values: -0.0 ties with
//                     +0.0), then z = Phi^-1((r - 3/8) / (S + 1/4)) at the draw's own position of
//                     Z[pair][split chain][h];
//   tail_kernel       the indicator series x <= q05 and x <= q95;
//   moments_kernel on z(x), both indicators and z(|x - median|), acov_kernel with Geyer's rule
//   on the host for the first three: the four series lie in one buffer, one launch serves all.
// No floating-point atomics anywhere, and no result depends on the order in which workgroups
// run: the results are the same bit for bit from call to call and for any max_staging_bytes.
#include "posterior_common.h"

namespace fitoct {
namespace {

constexpr int SORT_LDS_KEYS = FITOCT_MONITOR_SORT_LDS_KEYS;   // a power of two
constexpr int SORT_TILE = FITOCT_MONITOR_SORT_TILE;           // a multiple of 64
constexpr int SORT_THREADS = 256;
constexpr int ELEM_THREADS = 256;   // keys_kernel, rank_kernel, tail_kernel: one draw per thread
constexpr int N_PICKS = 8;
constexpr int N_PAR = 3;            // per pair: median, q05, q95
constexpr int N_SERIES = 4;         // z(x), x <= q05, x <= q95, z(|x - median|)
static_assert((SORT_LDS_KEYS & (SORT_LDS_KEYS - 1)) == 0 && SORT_TILE % 64 == 0, "sort shapes");

// ---- host route -----------------------------------------------------------------------------
int monitor_host(const Shape& s, const double* draws, double* out) {
  std::vector<double> x((size_t)s.S);
  for (int g = 0; g < s.G; ++g) {
    OutModel m = s.model;
    m.lambda_scale = s.lscale[g];
    for (int j = 0; j < s.P; ++j) {
      for (int c = 0; c < s.C; ++c)
        for (int i = 0; i < s.n; ++i)
          x[(size_t)c * s.n + i] = column_value(
              m, j, draws + (((size_t)g * s.C + c) * s.I + s.first + i) * s.W);
      FITOCT_TRY(monitor_column(x.data(), s.C, s.n, out + ((size_t)g * s.P + j) * 5));
    }
  }
  return FITOCT_OK;
}

// ---- kernels --------------------------------------------------------------------------------
// split draw e = j h + i (split chain j, position i) of a pair staged as X[pair][chain][n]
__device__ inline double split_value(const double* X, const KShape& k, int64_t pair, int64_t e) {
  const int j = (int)(e / k.h), i = (int)(e % k.h);
  return chain_series(X, k, pair, j >> 1)[((j & 1) ? k.n - k.h : 0) + i];
}

// K[pair][e] = key of the split draw (fold: of its distance to the pair's median, par[pair][0])
__global__ __launch_bounds__(ELEM_THREADS) void keys_kernel(KShape k, const double* X,
                                                            const double* par, int fold,
                                                            int64_t S, int nblk,
                                                            unsigned long long* K) {
  const int64_t pair = blockIdx.x / nblk;
  const int64_t e = (int64_t)(blockIdx.x % nblk) * ELEM_THREADS + threadIdx.x;
  if (e >= S) return;
  double v = split_value(X, k, pair, e);
  if (fold) v = fabs(v - par[pair * N_PAR]);
  K[(size_t)pair * S + e] = order_key(v);
}

// one workgroup per pair: bitonic sort of its S <= SORT_LDS_KEYS keys in LDS, padded to the
// next power of two Np with the largest key (the pads stay behind the S keys)
__global__ __launch_bounds__(SORT_THREADS) void sort_lds_kernel(int64_t S, int Np,
                                                                unsigned long long* K) {
  __shared__ unsigned long long a[SORT_LDS_KEYS];
  unsigned long long* key = K + (size_t)blockIdx.x * S;
  for (int t = threadIdx.x; t < Np; t += SORT_THREADS) a[t] = t < S ? key[t] : ~0ull;
  __syncthreads();
  for (int kk = 2; kk <= Np; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < Np / 2; t += SORT_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const unsigned long long u = a[i], v = a[p];
        if ((u > v) == ((i & kk) == 0)) {
          a[i] = v;
          a[p] = u;
        }
      }
      __syncthreads();
    }
  for (int t = threadIdx.x; t < S; t += SORT_THREADS) key[t] = a[t];
}

// Radix pass, step 1.  cnt[pair][tile][digit] = keys of the tile with that digit at `shift`.
__global__ __launch_bounds__(SORT_THREADS) void rhist_kernel(const unsigned long long* K,
                                                             int64_t S, int ntile, int shift,
                                                             unsigned int* cnt) {
  __shared__ unsigned int lh[256];
  const int64_t pair = blockIdx.x / ntile;
  const int tile = blockIdx.x % ntile;
  lh[threadIdx.x] = 0u;   // SORT_THREADS == 256
  __syncthreads();
  const unsigned long long* key = K + (size_t)pair * S;
  const int64_t e0 = (int64_t)tile * SORT_TILE;
  for (int t = threadIdx.x; t < SORT_TILE && e0 + t < S; t += SORT_THREADS)
    atomicAdd(&lh[(unsigned int)(key[e0 + t] >> shift) & 255u], 1u);
  __syncthreads();
  cnt[((size_t)pair * ntile + tile) * 256 + threadIdx.x] = lh[threadIdx.x];
}
static_assert(SORT_THREADS == 256, "rhist_kernel and rscan_kernel: one thread per digit");

// Step 2, one workgroup per pair, thread d for digit d: the counts become the place of the
// first key of every (digit, tile): all smaller digits first, then the digit's earlier tiles.
__global__ __launch_bounds__(SORT_THREADS) void rscan_kernel(int ntile, unsigned int* cnt) {
  __shared__ unsigned int tot[256];
  unsigned int* c = cnt + (size_t)blockIdx.x * ntile * 256 + threadIdx.x;   // c[256 t]: tile t
  unsigned int sum = 0u;
  for (int t = 0; t < ntile; ++t) sum += c[(size_t)256 * t];
  tot[threadIdx.x] = sum;
  __syncthreads();
  unsigned int base = 0u;
  for (int d = 0; d < (int)threadIdx.x; ++d) base += tot[d];
  for (int t = 0; t < ntile; ++t) {
    const unsigned int here = c[(size_t)256 * t];
    c[(size_t)256 * t] = base;
    base += here;
  }
}

// Step 3, one wave per tile: the keys go out in tile order behind the (digit, tile) offset.
// A key's place among the wave's 64 current keys with the same digit comes from eight ballots
// (one per digit bit); the running offsets live in LDS.  Stable, no atomics.
__global__ __launch_bounds__(64) void rscatter_kernel(const unsigned long long* K, int64_t S,
                                                      int ntile, int shift,
                                                      const unsigned int* cnt,
                                                      unsigned long long* out) {
  __shared__ unsigned int off[256];
  const int64_t pair = blockIdx.x / ntile;
  const int tile = blockIdx.x % ntile, lane = threadIdx.x;
  for (int d = lane; d < 256; d += 64) off[d] = cnt[((size_t)pair * ntile + tile) * 256 + d];
  __syncthreads();
  const unsigned long long* key = K + (size_t)pair * S;
  unsigned long long* dst = out + (size_t)pair * S;
  const int64_t e0 = (int64_t)tile * SORT_TILE;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int r = 0; r < SORT_TILE / 64; ++r) {   // (uniform trip count: barriers inside)
    const int64_t e = e0 + r * 64 + lane;
    const bool on = e < S;
    const unsigned long long kv = on ? key[e] : 0ull;
    const unsigned int digit = (unsigned int)(kv >> shift) & 255u;
    unsigned long long same = __ballot(on);
    for (int b = 0; b < 8; ++b) {
      const bool bit = (digit >> b) & 1u;
      const unsigned long long has = __ballot(on && bit);
      same &= bit ? has : ~has;
    }
    const unsigned int before = (unsigned int)__popcll(same & below);
    const unsigned int place = on ? off[digit] + before : 0u;
    __syncthreads();
    if (on && (int64_t)place < S) dst[place] = kv;   // (never false: the offsets sum to S)
    if (on && before == 0u) off[digit] = place + (unsigned int)__popcll(same);
    __syncthreads();
  }
}

// which sorted keys the host reads back
struct Picks {
  int64_t at[N_PICKS];
};
__global__ __launch_bounds__(64) void pick_kernel(const unsigned long long* K, int64_t S,
                                                  Picks pk, unsigned long long* picked) {
  if (threadIdx.x < N_PICKS)
    picked[(size_t)blockIdx.x * N_PICKS + threadIdx.x] =
        K[(size_t)blockIdx.x * S + pk.at[threadIdx.x]];
}

// keys of K[0..S) below q
__device__ inline int64_t keys_below(const unsigned long long* K, int64_t S,
                                     unsigned long long q) {
  int64_t lo = 0, hi = S;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (K[mid] < q) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Z[pair][e] = z of the split draw's average rank among the pair's sorted keys K (fold: of its
// distance to the median, whose keys K then holds)
__global__ __launch_bounds__(ELEM_THREADS) void rank_kernel(KShape k, const double* X,
                                                            const double* par, int fold,
                                                            int64_t S, int nblk,
                                                            const unsigned long long* K,
                                                            double* Z) {
  const int64_t pair = blockIdx.x / nblk;
  const int64_t e = (int64_t)(blockIdx.x % nblk) * ELEM_THREADS + threadIdx.x;
  if (e >= S) return;
  double v = split_value(X, k, pair, e);
  if (fold) v = fabs(v - par[pair * N_PAR]);
  // ties are decided by ==: both zeros form one run of the sorted keys (-0.0, then +0.0)
  const unsigned long long k_lo = order_key(v == 0.0 ? -0.0 : v);
  const unsigned long long k_hi = order_key(v == 0.0 ? 0.0 : v);
  const unsigned long long* key = K + (size_t)pair * S;
  const int64_t lower = keys_below(key, S, k_lo);   // keys below the run
  const int64_t upper = k_hi == ~0ull ? S : keys_below(key, S, k_hi + 1ull);   // through the run
  const double r = 0.5 * (double)(lower + upper - 1) + 1.0;
  Z[(size_t)pair * S + e] = inv_normal_cdf((r - 0.375) / ((double)S + 0.25));
}

// the indicator series of the tail quantiles par[pair][1] (q05) and par[pair][2] (q95)
__global__ __launch_bounds__(ELEM_THREADS) void tail_kernel(KShape k, const double* X,
                                                            const double* par, int64_t S,
                                                            int nblk, double* I05, double* I95) {
  const int64_t pair = blockIdx.x / nblk;
  const int64_t e = (int64_t)(blockIdx.x % nblk) * ELEM_THREADS + threadIdx.x;
  if (e >= S) return;
  const double v = split_value(X, k, pair, e);
  I05[(size_t)pair * S + e] = v <= par[pair * N_PAR + 1] ? 1.0 : 0.0;
  I95[(size_t)pair * S + e] = v <= par[pair * N_PAR + 2] ? 1.0 : 0.0;
}

// ---- device route ---------------------------------------------------------------------------
// exact sort of K[pairs][S], keys only; tmp and cnt: scratch of the multi-workgroup regime
int sort_keys(int64_t pairs, int64_t S, unsigned long long* K, unsigned long long* tmp,
              unsigned int* cnt, hipStream_t st) {
  if (S <= SORT_LDS_KEYS) {
    int Np = 2;
    while (Np < S) Np <<= 1;
    sort_lds_kernel<<<dim3((unsigned)pairs), dim3(SORT_THREADS), 0, st>>>(S, Np, K);
    HIP_TRY(hipGetLastError());
    return FITOCT_OK;
  }
  const int ntile = (int)((S + SORT_TILE - 1) / SORT_TILE);
  unsigned long long *src = K, *dst = tmp;
  for (int pass = 0; pass < 8; ++pass) {   // an even number of passes: the result is in K
    rhist_kernel<<<dim3((unsigned)(pairs * ntile)), dim3(SORT_THREADS), 0, st>>>(src, S, ntile,
                                                                                 8 * pass, cnt);
    HIP_TRY(hipGetLastError());
    rscan_kernel<<<dim3((unsigned)pairs), dim3(SORT_THREADS), 0, st>>>(ntile, cnt);
    HIP_TRY(hipGetLastError());
    rscatter_kernel<<<dim3((unsigned)(pairs * ntile)), dim3(64), 0, st>>>(src, S, ntile, 8 * pass,
                                                                          cnt, dst);
    HIP_TRY(hipGetLastError());
    std::swap(src, dst);
  }
  return FITOCT_OK;
}

int monitor_device(const Shape& s, const void* d_draws, const fitoct_summary_config* cfg,
                   hipStream_t st, double* out) {
  DeviceKeep keep;
  HIP_TRY(hipSetDevice(cfg->device));
  const int64_t S = (int64_t)s.m * s.h;   // pooled split draws of one column
  const int64_t col_bytes = (int64_t)s.G * s.S * (int64_t)sizeof(double);
  const int ncc_max = (int)items_per_pass(cfg, s.P, FITOCT_MONITOR_STAGING_BUFFERS * col_bytes);
  const int64_t pairs_max = (int64_t)s.G * ncc_max;
  const int64_t nblk = (S + ELEM_THREADS - 1) / ELEM_THREADS;
  const int64_t ntile = (S + SORT_TILE - 1) / SORT_TILE;
  const int64_t limit = (int64_t)1 << 31;
  // (the radix offsets and the average rank's lower + upper are 32- and 64-bit: S < 2^31)
  if (S >= limit || row_grid(s) >= limit || N_SERIES * pairs_max * s.m >= limit ||
      pairs_max * nblk >= limit || pairs_max * ntile * 256 >= limit)
    return fail(FITOCT_E_ARG, "monitor: shape too large for one launch (lower max_staging_bytes)");

  // X and six buffers of S values per pair: two of keys, and the four series z(x), x <= q05,
  // x <= q95, z(|x - median|) in one buffer ZS[series][pair][S], so that one moments_kernel and
  // one acov_kernel launch per lag block serve them all
  DevBuf X, KA, KB, ZS, lscale, cnt, picked, par;
  EssBufs eb;
  FITOCT_TRY(X.alloc((size_t)pairs_max * s.S * sizeof(double)));
  for (DevBuf* b : {&KA, &KB}) FITOCT_TRY(b->alloc((size_t)pairs_max * S * sizeof(double)));
  FITOCT_TRY(ZS.alloc((size_t)N_SERIES * pairs_max * S * sizeof(double)));
  FITOCT_TRY(lscale.alloc((size_t)s.G * sizeof(double)));
  FITOCT_TRY(cnt.alloc(S > SORT_LDS_KEYS ? (size_t)pairs_max * 256 * ntile * sizeof(unsigned int) : 0));
  FITOCT_TRY(picked.alloc((size_t)pairs_max * N_PICKS * sizeof(unsigned long long)));
  FITOCT_TRY(par.alloc((size_t)pairs_max * N_PAR * sizeof(double)));
  FITOCT_TRY(eb.alloc(N_SERIES * pairs_max, s.m));
  HIP_TRY(hipMemcpyAsync(lscale.p, s.lscale.data(), sizeof(double) * s.G, hipMemcpyHostToDevice, st));

  const QIndex q05 = quantile_index(S, 0.05), q95 = quantile_index(S, 0.95);
  const Picks pk{{0, S - 1, S / 2 - 1, S / 2, q05.lo, q05.hi, q95.lo, q95.hi}};
  std::vector<unsigned long long> h_picked;
  std::vector<double> h_par, mom, cm(s.m), cv(s.m);
  std::vector<int> flags;
  for (int c0 = 0; c0 < s.P; c0 += ncc_max) {
    const int ncc = std::min(ncc_max, s.P - c0);
    const int64_t pairs = (int64_t)s.G * ncc;
    const KShape k = kshape(s, c0, ncc);
    // Z[pair][split chain][h] read as whole chains of 2 h draws: the split halves are its rows
    KShape kz = k;
    kz.n = 2 * s.h;
    const dim3 egrid((unsigned)(pairs * nblk)), eblock(ELEM_THREADS);
    unsigned long long* keys = KA.as<unsigned long long>();
    // this pass's series: pair p of series q is "pair" q pairs + p of the moments and Geyer's rounds
    double* Z = ZS.as<double>();
    double *I05 = Z + (size_t)pairs * S, *I95 = Z + (size_t)2 * pairs * S,
           *ZF = Z + (size_t)3 * pairs * S;
    FITOCT_TRY(queue_stage(k, d_draws, lscale.as<double>(), X.as<double>(), st));

    // x: sort, the order statistics, z(x)
    keys_kernel<<<egrid, eblock, 0, st>>>(k, X.as<double>(), par.as<double>(), 0, S, (int)nblk, keys);
    HIP_TRY(hipGetLastError());
    FITOCT_TRY(sort_keys(pairs, S, keys, KB.as<unsigned long long>(), cnt.as<unsigned int>(), st));
    pick_kernel<<<dim3((unsigned)pairs), dim3(64), 0, st>>>(keys, S, pk,
                                                            picked.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    h_picked.resize((size_t)pairs * N_PICKS);
    HIP_TRY(hipMemcpyAsync(h_picked.data(), picked.p, sizeof(unsigned long long) * h_picked.size(),
                           hipMemcpyDeviceToHost, st));
    rank_kernel<<<egrid, eblock, 0, st>>>(k, X.as<double>(), par.as<double>(), 0, S, (int)nblk,
                                          keys, Z);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));

    // per pair: a NaN among the draws; the median and the tail quantiles
    std::vector<char> skip((size_t)pairs, 0);
    std::vector<int> active;
    h_par.assign((size_t)pairs * N_PAR, 0.0);
    for (int64_t p = 0; p < pairs; ++p) {
      const unsigned long long* q = h_picked.data() + (size_t)p * N_PICKS;
      skip[p] = keys_hold_nan(q[0], q[1]);
      if (skip[p]) continue;
      h_par[p * N_PAR] = 0.5 * (key_value(q[3]) + key_value(q[2]));
      h_par[p * N_PAR + 1] = quantile_lerp(key_value(q[4]), key_value(q[5]), q05.frac);
      h_par[p * N_PAR + 2] = quantile_lerp(key_value(q[6]), key_value(q[7]), q95.frac);
    }
    HIP_TRY(hipMemcpyAsync(par.p, h_par.data(), sizeof(double) * h_par.size(),
                           hipMemcpyHostToDevice, st));

    // the indicators; |x - median|: sort, z
    tail_kernel<<<egrid, eblock, 0, st>>>(k, X.as<double>(), par.as<double>(), S, (int)nblk,
                                          I05, I95);
    HIP_TRY(hipGetLastError());
    keys_kernel<<<egrid, eblock, 0, st>>>(k, X.as<double>(), par.as<double>(), 1, S, (int)nblk, keys);
    HIP_TRY(hipGetLastError());
    FITOCT_TRY(sort_keys(pairs, S, keys, KB.as<unsigned long long>(), cnt.as<unsigned int>(), st));
    rank_kernel<<<egrid, eblock, 0, st>>>(k, X.as<double>(), par.as<double>(), 1, S, (int)nblk,
                                          keys, ZF);
    HIP_TRY(hipGetLastError());

    FITOCT_TRY(queue_moments(kz, Z, N_SERIES * pairs, eb, st, mom, flags));
    HIP_TRY(hipStreamSynchronize(st));

    // every chain constant (in x as in z(x): bit 1 of no split chain's flags): a NaN row too
    for (int64_t p = 0; p < pairs; ++p) {
      int fl = 0;
      for (int j = 0; j < s.m; ++j) fl |= flags[(size_t)p * s.m + j];   // (series 0: z(x))
      skip[p] = skip[p] || !(fl & 2);
    }
    for (int q = 0; q < 3; ++q)   // n_eff of z(x) and of both indicators
      for (int64_t p = 0; p < pairs; ++p)
        if (!skip[p]) active.push_back((int)(q * pairs + p));
    std::vector<double> ess((size_t)N_SERIES * pairs, NAN);
    FITOCT_TRY(ess_rounds(kz, Z, eb, st, mom, active, ess));

    auto psr_of = [&](int64_t p) {   // p: series and pair
      split_moments(mom.data() + (size_t)p * s.m * 4, s.m, s.h, cm.data(), cv.data());
      return psr_moments(cm.data(), cv.data(), s.m, s.h);
    };
    for (int64_t p = 0; p < pairs; ++p) {
      const int g = (int)(p / ncc), j = c0 + (int)(p % ncc);
      double* row = out + ((size_t)g * s.P + j) * 5;
      if (skip[p]) {
        for (int i = 0; i < 5; ++i) row[i] = NAN;
        continue;
      }
      row[1] = psr_of(p);
      row[2] = psr_of(3 * pairs + p);
      row[0] = std::max(row[1], row[2]);
      row[3] = ess[p];
      row[4] = tail_min(ess[pairs + p], ess[2 * pairs + p]);
    }
  }
  return FITOCT_OK;
}

int monitor_device_checked(const fitoct_problem* probs, int n_groups, int chains, int iters_saved,
                           const void* d_draws, const fitoct_summary_config* cfg, void* stream,
                           double* out) {
  Shape s;
  FITOCT_TRY(check_args("monitor", false, probs, n_groups, chains, iters_saved, d_draws, cfg, out, s));
  FITOCT_TRY(check_device("monitor", cfg, d_draws));
  return monitor_device(s, d_draws, cfg, (hipStream_t)stream, out);
}

}  // namespace
}  // namespace fitoct

using namespace fitoct;

// the last run of a plan or of a batch (one body: on_last_run)
template <class Handle>
static int32_t last_run_monitor(const char* fn, Handle* h, const fitoct_summary_config* cfg, double* out) {
  return guarded(fn, [&]() -> int32_t {
    return on_last_run(h, "monitor", "the diagnostics need", cfg, out != nullptr,
                       [&](const Where& w, const fitoct_summary_config& c) {
                         return monitor_device_checked(w.probs.data(), (int32_t)w.probs.size(), w.chains,
                                                       w.iters_saved, w.draws, &c, nullptr, out);
                       });
  });
}

extern "C" {

int32_t fitoct_monitor_host(const fitoct_problem* probs, int32_t n_groups, int32_t chains,
                            int32_t iters_saved, const double* draws,
                            const fitoct_summary_config* cfg, double* out) {
  return guarded(__func__, [&]() -> int32_t {
    Shape s;
    const int rc = check_args("monitor", false, probs, n_groups, chains, iters_saved, draws, cfg, out, s);
    return rc ? rc : monitor_host(s, draws, out);
  });
}

int32_t fitoct_monitor_device(const fitoct_problem* probs, int32_t n_groups, int32_t chains,
                              int32_t iters_saved, const void* d_draws,
                              const fitoct_summary_config* cfg, void* stream, double* out) {
  return guarded(__func__, [&]() -> int32_t {
    return monitor_device_checked(probs, n_groups, chains, iters_saved, d_draws, cfg, stream, out);
  });
}

int32_t fitoct_plan_monitor(fitoct_plan* pl, const fitoct_summary_config* cfg, double* out) {
  return last_run_monitor(__func__, pl, cfg, out);
}

int32_t fitoct_batch_monitor(fitoct_batch* b, const fitoct_summary_config* cfg, double* out) {
  return last_run_monitor(__func__, b, cfg, out);
}

}  // extern "C"
