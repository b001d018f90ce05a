// The pairs plot of draws that stay in HBM (include/fitoct.h "pairs plot"):
// what pairs(fit, pars), rgumlib::SAPlot and FitOCTLib::plotPriPostAll reduce the draws to --
// per selected output column the marginal histogram, per couple of columns (a *panel*) the
// joint histogram, each with a second count plane of the divergent draws, and the correlation
// matrix -- and the same computation on the host (fitoct_pairs_host) that the device route is
// tested against.  Both routes share the argument checks, the edge builder (build_edges: the
// device never evaluates an edge formula), the bin rule (bin_code: comparisons against the edge
// array only, so the counts are exact) and the last step of the correlation (finish_corr).
//
// Device route:
//   ranges     the columns whose range is automatic are staged and selected by the shared layer
//              (queue_stage, queue_select), in passes of contiguous output columns under
//              max_staging_bytes; nothing is staged when every range is given;
//   digitise_kernel   one workgroup per (group, chain, block of STAGE_ROWS rows) reads the raw
//              rows once (load_row_tile), forms the selected column values and finds each
//              value's bin against the group's edges in LDS.  It writes one byte per (column,
//              draw), K[group][col][Sp] (the bin, or BIN_BELOW / BIN_ABOVE / BIN_NONE), one
//              byte per draw for the divergent flag, and per (group, column) the flags "holds a
//              NaN" and "holds two different values".  These bytes, (n_cols + 1) Sp per group,
//              lie outside max_staging_bytes;
//   marginal_kernel   hist1 and outside of one byte column: 16 bytes per lane, LDS counters,
//              one 64-bit integer atomic per non-empty counter and workgroup.  (The marginals
//              are counted from the bytes and not in digitise_kernel: its tile, the edges and
//              the counters of 64 columns x 64 bins x 2 planes do not fit 64 KiB of LDS.);
//   panel_kernel      one workgroup per (group, column a, up to PANELS_MAX columns b, share of
//              the draws) streams the byte columns, 16 bytes per lane in a grid-stride loop
//              over a capped grid, reads a's bytes once for its panels, counts into
//              LDS-private n_bins x n_bins grids of 32-bit words and flushes the non-empty
//              cells with 64-bit integer atomics;
//   mean_partial_kernel / cov_partial_kernel   the pooled means, then the centred
//              cross-products, from the raw rows: the row blocks of a group are split over a
//              number of workgroups fixed by the shape (corr_slabs), each loops over its
//              blocks in order and writes one slab; slab_sum_kernel adds the slabs in slab
//              order.  A call for the correlation alone selects and digitises nothing: the
//              mean pass forms the columns' flags.
// Integer atomics only, and a partition of the floating-point sums that depends on the shape
// alone: the results are the same bit for bit from call to call, for any max_staging_bytes and
// on any device.
#include "posterior_common.h"

namespace fitoct {
namespace {

constexpr int MAX_COLS = 64, MAX_BINS = 64;
// K's codes beside the bins 0 .. n_bins - 1: below lo, above hi, no bin (a NaN, no grid)
constexpr int BIN_BELOW = 253, BIN_ABOVE = 254, BIN_NONE = 255;
constexpr int FLAG_NAN = 1, FLAG_VARIES = 2;
constexpr int VEC = 16;                  // bytes of K per lane and load
constexpr int COUNT_THREADS = 256;       // marginal_kernel, panel_kernel
constexpr int MARGINAL_BLOCKS = 32;      // workgroups per byte column, at most
constexpr int PANELS_MAX = 8;            // panels sharing column a per workgroup, at most
constexpr int PANEL_LDS_BYTES = 32 << 10;    // a workgroup's grids (64 bins x 2 planes: one grid)
constexpr int LDS_LIMIT_BYTES = 64 << 10;    // every launch's dynamic LDS is checked against it
constexpr int PANEL_GRID = 1024;         // workgroups of one panels launch, about
constexpr int CORR_SLABS = 2048;         // partial slabs of one call, at most
constexpr int PROD_PER_THREAD = (MAX_COLS * (MAX_COLS + 1) / 2 + STAGE_THREADS - 1) / STAGE_THREADS;

// What a call computes beside Shape: checked by check_pairs_args.
struct PShape {
  int nc = 0, nb = 0, planes = 1, npan = 0;
  int cols[MAX_COLS] = {};
  uint64_t log_mask = 0;
  int64_t Sp = 0;   // S rounded up to VEC: the stride of a byte column
};

void pairs_sizes(int nc, int nb, int planes, int64_t G, int64_t sizes[5]) {
  sizes[0] = G * nc * (nb + 1);
  sizes[1] = G * nc * planes * nb;
  sizes[2] = G * nc * 2;
  sizes[3] = G * (nc * (nc - 1) / 2) * planes * nb * nb;
  sizes[4] = G * nc * nc;
}

int check_pairs_config(const fitoct_pairs_config* cfg) {
  if (!cfg) return fail(FITOCT_E_ARG, "pairs: NULL argument (config)");
  if (cfg->n_cols < 1 || cfg->n_cols > MAX_COLS)
    return fail(FITOCT_E_ARG, "pairs: n_cols must be in [1, 64]");
  if (cfg->n_bins < 2 || cfg->n_bins > MAX_BINS)
    return fail(FITOCT_E_ARG, "pairs: n_bins must be in [2, 64]");
  if (cfg->planes != 1 && cfg->planes != 2) return fail(FITOCT_E_ARG, "pairs: planes must be 1 or 2");
  return FITOCT_OK;
}

// sc: the summary's form of the call (the probabilities of the automatic ranges), what the
// shared layer reads
int check_pairs_args(const fitoct_problem* probs, int n_groups, int chains, int iters_saved,
                     const void* draws, const fitoct_pairs_config* cfg,
                     const fitoct_pairs_out* out, Shape& s, PShape& p, fitoct_summary_config& sc) {
  if (!cfg || !out) return fail(FITOCT_E_ARG, "pairs: NULL argument (problems, draws, config or out)");
  const double p_lo = cfg->range_probs[0], p_hi = cfg->range_probs[1];
  if (!(p_lo >= 0.0 && p_lo < p_hi && p_hi <= 1.0))
    return fail(FITOCT_E_ARG, "pairs: range_probs must satisfy 0 <= p_lo < p_hi <= 1");
  sc = fitoct_summary_config{};
  sc.first_iter = cfg->first_iter;
  sc.n_probs = 2;
  sc.probs[0] = p_lo;
  sc.probs[1] = p_hi;
  sc.max_staging_bytes = cfg->max_staging_bytes;
  sc.device = cfg->device;
  static const double some = 0.0;   // (the outputs are optional: check_args wants one)
  FITOCT_TRY(check_args("pairs", true, probs, n_groups, chains, iters_saved, draws, &sc, &some, s));
  FITOCT_TRY(check_pairs_config(cfg));
  p.nc = cfg->n_cols;
  p.nb = cfg->n_bins;
  p.planes = cfg->planes;
  p.npan = p.nc * (p.nc - 1) / 2;
  p.log_mask = cfg->log_mask;
  p.Sp = (s.S + VEC - 1) / VEC * VEC;
  for (int j = 0; j < p.nc; ++j) {
    const int c = cfg->cols[j];
    if (c < 0 || c >= s.P)
      return fail(FITOCT_E_ARG, "pairs: cols[" + std::to_string(j) + "] = " + std::to_string(c) +
                                    " is not in [0, " + std::to_string(s.P) + ")");
    for (int i = 0; i < j; ++i)
      if (cfg->cols[i] == c)
        return fail(FITOCT_E_ARG, "pairs: cols[" + std::to_string(j) + "] repeats column " +
                                      std::to_string(c));
    p.cols[j] = c;
  }
  if (p.nc < 64 && (cfg->log_mask >> p.nc) != 0)
    return fail(FITOCT_E_ARG, "pairs: log_mask has a bit at or above n_cols");
  if (!out->edges && !out->hist1 && !out->outside && !out->hist2 && !out->corr)
    return fail(FITOCT_E_ARG, "pairs: every output of out is NULL");
  return FITOCT_OK;
}

// ---- what both routes share --------------------------------------------------------------------
// the given range of (group, column) if both ends are finite numbers
bool given_range(const double* ranges, int64_t gj, double& lo, double& hi) {
  if (!ranges) return false;
  lo = ranges[2 * gj];
  hi = ranges[2 * gj + 1];
  return std::isfinite(lo) && std::isfinite(hi);
}

// e[0 .. nb]: the edges of one column; false and NaN edges where the column has no grid
bool build_edges(double lo, double hi, int nb, bool log_scale, double* e) {
  bool ok = std::isfinite(lo) && std::isfinite(hi) && lo < hi && (!log_scale || lo > 0.0);
  if (ok) {
    const double span = log_scale ? log(hi / lo) : hi - lo;
    e[0] = lo;
    e[nb] = hi;
    for (int k = 1; k < nb; ++k)
      e[k] = log_scale ? lo * exp(span * k / nb) : lo + span * ((double)k / nb);
    for (int k = 0; k < nb; ++k) ok = ok && e[k] < e[k + 1];
  }
  if (!ok)
    for (int k = 0; k <= nb; ++k) e[k] = NAN;
  return ok;
}

// numpy's rule for explicit edges: bin k holds e[k] <= v < e[k + 1], the last one v <= e[nb] too
FITOCT_HD inline int bin_code(const double* e, int nb, double v) {
  if (e[0] != e[0] || v != v) return BIN_NONE;
  if (v < e[0]) return BIN_BELOW;
  if (v > e[nb]) return BIN_ABOVE;
  int lo = 0, hi = nb;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (v >= e[mid]) lo = mid;
    else hi = mid;
  }
  return lo;
}

FITOCT_HD inline int panel_index(int nc, int a, int b) {   // a < b, lexicographic
  return a * nc - a * (a + 1) / 2 + (b - a - 1);
}

// corr[nc][nc] of one group from the centred cross-products cu (upper triangle by rows:
// (0,0) (0,1) .. (0,nc-1) (1,1) ..) and the columns' flags
void finish_corr(int nc, const double* cu, const int* flags, double* corr) {
  std::vector<double> root((size_t)nc);
  std::vector<char> bad((size_t)nc);
  std::vector<int> row0((size_t)nc);
  for (int a = 0, o = 0; a < nc; o += nc - a, ++a) row0[a] = o - a;   // cu[row0[a] + b]
  for (int a = 0; a < nc; ++a) {
    const double saa = cu[row0[a] + a];
    bad[a] = (flags[a] & FLAG_NAN) || !(flags[a] & FLAG_VARIES) || !(saa > 0.0) || !std::isfinite(saa);
    root[a] = sqrt(saa);
  }
  for (int a = 0; a < nc; ++a)
    for (int b = 0; b < nc; ++b) {
      double r = NAN;
      if (!bad[a] && !bad[b]) {
        const int lo = std::min(a, b), hi = std::max(a, b);
        r = a == b ? 1.0 : std::max(-1.0, std::min(1.0, cu[row0[lo] + hi] / (root[lo] * root[hi])));
      }
      corr[(size_t)a * nc + b] = r;
    }
}

// a NaN column has no grid: its edges are NaN, its counts 0
void blank_column(const PShape& p, int64_t gj, const fitoct_pairs_out* out) {
  if (out->edges) std::fill_n(out->edges + gj * (p.nb + 1), p.nb + 1, NAN);
  if (out->hist1) std::fill_n(out->hist1 + gj * p.planes * p.nb, p.planes * p.nb, (int64_t)0);
  if (out->outside) std::fill_n(out->outside + gj * 2, 2, (int64_t)0);
}

// ---- host route --------------------------------------------------------------------------------
int pairs_host(const Shape& s, const PShape& p, const fitoct_summary_config& sc,
               const double* draws, const double* ranges, const fitoct_pairs_out* out) {
  const int nc = p.nc, nb = p.nb, nb2 = nb * nb;
  const int64_t S = s.S;
  int64_t sizes[5];
  pairs_sizes(nc, nb, p.planes, s.G, sizes);
  if (out->hist1) std::fill_n(out->hist1, sizes[1], (int64_t)0);
  if (out->outside) std::fill_n(out->outside, sizes[2], (int64_t)0);
  if (out->hist2) std::fill_n(out->hist2, sizes[3], (int64_t)0);
  std::vector<double> V((size_t)nc * S), E((size_t)nc * (nb + 1)), mean((size_t)nc);
  std::vector<double> cu((size_t)nc * (nc + 1) / 2);
  std::vector<unsigned char> K((size_t)nc * S), dv((size_t)S);
  std::vector<int> flags((size_t)nc);
  std::vector<uint64_t> keys;
  const bool want_bins = out->hist1 || out->outside || out->hist2;
  for (int g = 0; g < s.G; ++g) {
    OutModel m = s.model;
    m.lambda_scale = s.lscale[g];
    // the column values of the pooled draws, the divergent flags, the columns' flags
    for (int c = 0; c < s.C; ++c)
      for (int i = 0; i < s.n; ++i) {
        const double* raw = draws + (((size_t)g * s.C + c) * s.I + s.first + i) * s.W;
        const int64_t d = (int64_t)c * s.n + i;
        dv[d] = raw[5] != 0.0 ? 1 : 0;
        for (int j = 0; j < nc; ++j) V[(size_t)j * S + d] = column_value(m, p.cols[j], raw);
      }
    for (int j = 0; j < nc; ++j) {
      const double* x = V.data() + (size_t)j * S;
      int f = 0;
      for (int64_t d = 0; d < S; ++d) f |= (x[d] != x[d] ? FLAG_NAN : 0) | (x[d] != x[0] ? FLAG_VARIES : 0);
      flags[j] = f;
    }
    // ranges and edges
    for (int j = 0; j < nc; ++j) {
      const int64_t gj = (int64_t)g * nc + j;
      const double* x = V.data() + (size_t)j * S;
      double r[2] = {NAN, NAN};
      if (!(flags[j] & FLAG_NAN) && !given_range(ranges, gj, r[0], r[1])) {
        // the summary's order statistics and interpolation (summary_host)
        keys.resize((size_t)S);
        for (int64_t d = 0; d < S; ++d) keys[d] = order_key(x[d]);
        for (int i = 0; i < 2; ++i) {
          const QIndex qi = quantile_index(S, sc.probs[i]);
          std::nth_element(keys.begin(), keys.begin() + qi.lo, keys.end());
          const double x_lo = key_value(keys[qi.lo]);
          const double x_hi = qi.hi > qi.lo
                                  ? key_value(*std::min_element(keys.begin() + qi.hi, keys.end()))
                                  : x_lo;
          r[i] = quantile_lerp(x_lo, x_hi, qi.frac);
        }
      }
      double* e = E.data() + (size_t)j * (nb + 1);
      const bool grid = !(flags[j] & FLAG_NAN) && build_edges(r[0], r[1], nb, (p.log_mask >> j) & 1, e);
      if (!grid) std::fill_n(e, nb + 1, NAN);
      if (out->edges) std::copy(e, e + nb + 1, out->edges + gj * (nb + 1));
      if (!want_bins) continue;
      unsigned char* k = K.data() + (size_t)j * S;
      for (int64_t d = 0; d < S; ++d) {
        const int code = bin_code(e, nb, x[d]);
        k[d] = (unsigned char)code;
        if (code < nb) {
          if (out->hist1) {
            ++out->hist1[(gj * p.planes) * nb + code];
            if (p.planes == 2 && dv[d]) ++out->hist1[(gj * p.planes + 1) * nb + code];
          }
        } else if (out->outside && code != BIN_NONE) {
          ++out->outside[gj * 2 + (code == BIN_ABOVE ? 1 : 0)];
        }
      }
    }
    // panels
    if (out->hist2)
      for (int a = 0; a < nc; ++a)
        for (int b = a + 1; b < nc; ++b) {
          int64_t* h = out->hist2 + (((int64_t)g * p.npan + panel_index(nc, a, b)) * p.planes) * nb2;
          const unsigned char *ka = K.data() + (size_t)a * S, *kb = K.data() + (size_t)b * S;
          for (int64_t d = 0; d < S; ++d)
            if (ka[d] < nb && kb[d] < nb) {
              ++h[ka[d] * nb + kb[d]];
              if (p.planes == 2 && dv[d]) ++h[nb2 + ka[d] * nb + kb[d]];
            }
        }
    // correlation: the pooled means, then the centred cross-products
    if (out->corr) {
      for (int j = 0; j < nc; ++j) {
        const double* x = V.data() + (size_t)j * S;
        double sum = 0.0;
        for (int64_t d = 0; d < S; ++d) sum += x[d];
        mean[j] = sum / (double)S;
      }
      for (int a = 0, o = 0; a < nc; ++a)
        for (int b = a; b < nc; ++b, ++o) {
          const double *xa = V.data() + (size_t)a * S, *xb = V.data() + (size_t)b * S;
          double acc = 0.0;
          for (int64_t d = 0; d < S; ++d) acc += (xa[d] - mean[a]) * (xb[d] - mean[b]);
          cu[o] = acc;
        }
      finish_corr(nc, cu.data(), flags.data(), out->corr + (size_t)g * nc * nc);
    }
  }
  return FITOCT_OK;
}

// ---- kernels -----------------------------------------------------------------------------------
// What the pairs kernels need of the call beside KShape (by value).
struct PDev {
  int nc, nb, planes, npan;
  int64_t S, Sp;
};
// the selected output columns, for the kernels that read the raw rows
struct Cols {
  int c[MAX_COLS];
};

// the raw row of group g's first pooled draw: what "holds two different values" compares with
__device__ inline const double* first_row(const KShape& k, const double* draws, int64_t g) {
  return draws + ((size_t)g * k.C * k.I + k.first) * k.W;
}

// One workgroup per (group, chain, block of STAGE_ROWS rows); dynamic LDS: the row tile, then
// the group's edges [nc][nb + 1].
__global__ __launch_bounds__(STAGE_THREADS) void digitise_kernel(
    KShape k, PDev p, Cols cols, const double* draws, const double* lscale, const double* edges,
    unsigned char* K, unsigned char* Dv, int* flags) {
  extern __shared__ double sm[];
  __shared__ int fl[MAX_COLS];
  __shared__ double first[MAX_COLS];   // the group's first pooled draw, per column
  const int Wp = k.W | 1, ne = p.nb + 1;
  double* tile = sm;
  double* ed = sm + STAGE_ROWS * Wp;
  if ((int)threadIdx.x < MAX_COLS) fl[threadIdx.x] = 0;
  const RowBlock rb = load_row_tile(k, draws, tile);
  OutModel m = k.model;
  m.lambda_scale = lscale[rb.g];
  for (int t = threadIdx.x; t < p.nc * ne; t += STAGE_THREADS)
    ed[t] = edges[(size_t)rb.g * p.nc * ne + t];
  if ((int)threadIdx.x < p.nc)
    first[threadIdx.x] = column_value(m, cols.c[threadIdx.x], first_row(k, draws, rb.g));
  __syncthreads();
  const int64_t d0 = (int64_t)rb.c * k.n + rb.i0;
  for (int t = threadIdx.x; t < p.nc * STAGE_ROWS; t += STAGE_THREADS) {
    const int jc = t / STAGE_ROWS, r = t % STAGE_ROWS;
    if (r >= rb.rows) continue;
    const double v = column_value(m, cols.c[jc], tile + r * Wp);
    const int f = (v != v ? FLAG_NAN : 0) | (v != first[jc] ? FLAG_VARIES : 0);
    if (f) atomicOr(&fl[jc], f);
    K[((size_t)rb.g * p.nc + jc) * p.Sp + d0 + r] = (unsigned char)bin_code(ed + jc * ne, p.nb, v);
  }
  if ((int)threadIdx.x < rb.rows)
    Dv[(size_t)rb.g * p.Sp + d0 + threadIdx.x] = tile[threadIdx.x * Wp + 5] != 0.0 ? 1 : 0;
  __syncthreads();
  if ((int)threadIdx.x < p.nc && fl[threadIdx.x])
    atomicOr(&flags[(size_t)rb.g * p.nc + threadIdx.x], fl[threadIdx.x]);
}

__device__ inline unsigned int byte_of(const uint4& v, int i) {
  const unsigned int w = i < 8 ? (i < 4 ? v.x : v.y) : (i < 12 ? v.z : v.w);
  return (w >> (8 * (i & 3))) & 255u;
}

// hist1[pair][plane][nb] and outside[pair][2] of the byte column pair = group * nc + column;
// `blocks` workgroups per column, each a grid-stride share of the column's 16-byte vectors
__global__ __launch_bounds__(COUNT_THREADS) void marginal_kernel(
    PDev p, int blocks, const unsigned char* K, const unsigned char* Dv, const int* flags,
    unsigned long long* hist1, unsigned long long* outside) {
  __shared__ unsigned int h[2][MAX_BINS + 2];   // per plane: the bins, then below, above
  const int64_t pair = blockIdx.x / blocks;
  const int blk = blockIdx.x % blocks;
  if (flags[pair] & FLAG_NAN) return;           // no grid: the counts stay 0
  for (int t = threadIdx.x; t < 2 * (MAX_BINS + 2); t += COUNT_THREADS) (&h[0][0])[t] = 0u;
  __syncthreads();
  const uint4* col = (const uint4*)(K + (size_t)pair * p.Sp);
  const uint4* div = (const uint4*)(Dv + (size_t)(pair / p.nc) * p.Sp);
  const int64_t nvec = p.Sp / VEC;
  for (int64_t v = (int64_t)blk * COUNT_THREADS + threadIdx.x; v < nvec;
       v += (int64_t)blocks * COUNT_THREADS) {
    const uint4 a = col[v];
    const uint4 d = p.planes == 2 ? div[v] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const unsigned int code = byte_of(a, i);
      if (code == (unsigned int)BIN_NONE) continue;
      const unsigned int slot = code < (unsigned int)p.nb ? code
                                                          : (unsigned int)p.nb + (code == (unsigned int)BIN_ABOVE ? 1u : 0u);
      atomicAdd(&h[0][slot], 1u);
      if (byte_of(d, i)) atomicAdd(&h[1][slot], 1u);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < p.planes * p.nb; t += COUNT_THREADS) {
    const unsigned int c = h[t / p.nb][t % p.nb];
    if (c) atomicAdd(&hist1[(size_t)pair * p.planes * p.nb + t], (unsigned long long)c);
  }
  if (threadIdx.x < 2 && h[0][p.nb + threadIdx.x])
    atomicAdd(&outside[(size_t)pair * 2 + threadIdx.x], (unsigned long long)h[0][p.nb + threadIdx.x]);
}

// The panels (a, b0 .. b0 + cnt) of one workgroup.
struct PanelItem {
  int a, b0, cnt;
};

// Workgroup (group, item, share): dynamic LDS cells[cnt][planes][nb * nb].
__global__ __launch_bounds__(COUNT_THREADS) void panel_kernel(
    PDev p, const PanelItem* items, int n_items, int shares, const unsigned char* K,
    const unsigned char* Dv, const int* flags, unsigned long long* hist2) {
  extern __shared__ unsigned int cells[];
  int64_t b = blockIdx.x;
  const int share = (int)(b % shares);
  b /= shares;
  const PanelItem it = items[b % n_items];
  const int64_t g = b / n_items;
  if (flags[g * p.nc + it.a] & FLAG_NAN) return;   // no grid: every panel of a stays 0
  const int nb2 = p.nb * p.nb, per = p.planes * nb2;
  for (int t = threadIdx.x; t < it.cnt * per; t += COUNT_THREADS) cells[t] = 0u;
  __syncthreads();
  const unsigned char* Kg = K + (size_t)g * p.nc * p.Sp;
  const uint4* ca = (const uint4*)(Kg + (size_t)it.a * p.Sp);
  const uint4* div = (const uint4*)(Dv + (size_t)g * p.Sp);
  const int64_t nvec = p.Sp / VEC;
  unsigned int blank = 0u;   // the columns b with no grid
  for (int q = 0; q < it.cnt; ++q)
    if (flags[g * p.nc + it.b0 + q] & FLAG_NAN) blank |= 1u << q;
  for (int64_t v = (int64_t)share * COUNT_THREADS + threadIdx.x; v < nvec;
       v += (int64_t)shares * COUNT_THREADS) {
    const uint4 a = ca[v];
    const uint4 d = p.planes == 2 ? div[v] : make_uint4(0u, 0u, 0u, 0u);
    for (int q = 0; q < it.cnt; ++q) {
      if (blank >> q & 1u) continue;
      const uint4 bb = ((const uint4*)(Kg + (size_t)(it.b0 + q) * p.Sp))[v];
      unsigned int* c = cells + (size_t)q * per;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const unsigned int ka = byte_of(a, i), kb = byte_of(bb, i);
        if (ka < (unsigned int)p.nb && kb < (unsigned int)p.nb) {
          atomicAdd(&c[ka * p.nb + kb], 1u);
          if (byte_of(d, i)) atomicAdd(&c[nb2 + ka * p.nb + kb], 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < it.cnt * per; t += COUNT_THREADS) {
    const int q = t / per, cell = t % per;
    if (cells[t])
      atomicAdd(&hist2[((size_t)g * p.npan + panel_index(p.nc, it.a, it.b0 + q)) * per + cell],
                (unsigned long long)cells[t]);
  }
}

// Slab `sl` of `slabs` takes the row blocks [sl * nblk / slabs, (sl + 1) * nblk / slabs) of its
// group's nblk = row_blocks(n) * chains, in order.
struct SlabRange {
  int64_t g, b0, b1, nblk;
};
__device__ inline SlabRange slab_range(const KShape& k, int slabs) {
  SlabRange r;
  r.g = blockIdx.x / slabs;
  const int64_t sl = blockIdx.x % slabs;
  r.nblk = (int64_t)row_blocks(k.n) * k.C;
  r.b0 = sl * r.nblk / slabs;
  r.b1 = (sl + 1) * r.nblk / slabs;
  return r;
}

// V[STAGE_ROWS][nc]: the selected column values of the tile's rows less `centre` (NULL: 0); the
// rows past the block's end are 0
__device__ inline void tile_values(const KShape& k, const PDev& p, const Cols& cols,
                                   const OutModel& m, const double* tile, int rows,
                                   const double* centre, double* V) {
  const int Wp = k.W | 1;
  for (int t = threadIdx.x; t < p.nc * STAGE_ROWS; t += STAGE_THREADS) {
    const int r = t / p.nc, jc = t % p.nc;
    V[t] = r < rows ? column_value(m, cols.c[jc], tile + r * Wp) - (centre ? centre[jc] : 0.0) : 0.0;
  }
}

// part[group][slab][nc]: the sums of the slab's draws; dynamic LDS: the row tile, then V.
// flags, if given (a call that digitises nothing): the columns' flags, as digitise_kernel's.
__global__ __launch_bounds__(STAGE_THREADS) void mean_partial_kernel(
    KShape k, PDev p, Cols cols, int slabs, const double* draws, const double* lscale,
    double* part, int* flags) {
  extern __shared__ double sm[];
  double* tile = sm;
  double* V = sm + STAGE_ROWS * (k.W | 1);
  const SlabRange sr = slab_range(k, slabs);
  OutModel m = k.model;
  m.lambda_scale = lscale[sr.g];
  const bool mine = (int)threadIdx.x < p.nc;
  const double v0 = mine ? column_value(m, cols.c[threadIdx.x], first_row(k, draws, sr.g)) : 0.0;
  double acc = 0.0;
  int f = 0;
  for (int64_t b = sr.b0; b < sr.b1; ++b) {
    const RowBlock rb = load_row_tile(k, draws, tile, sr.g * sr.nblk + b);
    tile_values(k, p, cols, m, tile, rb.rows, nullptr, V);
    __syncthreads();
    if (mine)
      for (int r = 0; r < rb.rows; ++r) {
        const double v = V[r * p.nc + threadIdx.x];
        acc += v;
        f |= (v != v ? FLAG_NAN : 0) | (v != v0 ? FLAG_VARIES : 0);
      }
    __syncthreads();
  }
  if (mine) part[(size_t)blockIdx.x * p.nc + threadIdx.x] = acc;
  if (mine && flags && f) atomicOr(&flags[sr.g * p.nc + threadIdx.x], f);
}

// part[group][slab][ne], ne = nc (nc + 1) / 2: the centred cross-products of the slab's draws,
// upper triangle by rows; thread t carries the entries t, t + STAGE_THREADS, ...
__global__ __launch_bounds__(STAGE_THREADS) void cov_partial_kernel(
    KShape k, PDev p, Cols cols, int slabs, const double* draws, const double* lscale,
    const double* mean, double* part) {
  extern __shared__ double sm[];
  double* tile = sm;
  double* V = sm + STAGE_ROWS * (k.W | 1);
  const SlabRange sr = slab_range(k, slabs);
  OutModel m = k.model;
  m.lambda_scale = lscale[sr.g];
  const int ne = p.nc * (p.nc + 1) / 2;
  int ea[PROD_PER_THREAD], eb[PROD_PER_THREAD];
  double acc[PROD_PER_THREAD];
#pragma unroll
  for (int q = 0; q < PROD_PER_THREAD; ++q) {
    int e = threadIdx.x + q * STAGE_THREADS, a = 0;
    acc[q] = 0.0;
    if (e >= ne) e = 0;   // (not stored)
    while (e >= p.nc - a) {
      e -= p.nc - a;
      ++a;
    }
    ea[q] = a;
    eb[q] = a + e;
  }
  const int nq = (ne - (int)threadIdx.x + STAGE_THREADS - 1) / STAGE_THREADS;   // this thread's entries
  const double* centre = mean + (size_t)sr.g * p.nc;
  for (int64_t b = sr.b0; b < sr.b1; ++b) {
    const RowBlock rb = load_row_tile(k, draws, tile, sr.g * sr.nblk + b);
    tile_values(k, p, cols, m, tile, rb.rows, centre, V);
    __syncthreads();
#pragma unroll 2
    for (int r = 0; r < STAGE_ROWS; ++r) {
      const double* v = V + r * p.nc;
#pragma unroll
      for (int q = 0; q < PROD_PER_THREAD; ++q)
        if (q < nq) acc[q] += v[ea[q]] * v[eb[q]];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < PROD_PER_THREAD; ++q)
    if ((int)threadIdx.x + q * STAGE_THREADS < ne)
      part[(size_t)blockIdx.x * ne + threadIdx.x + q * STAGE_THREADS] = acc[q];
}

// out[group][ne] = scale * the sum over the slabs, in slab order, of part[group][slab][ne]
__global__ __launch_bounds__(STAGE_THREADS) void slab_sum_kernel(int64_t total, int ne, int slabs,
                                                               double scale, const double* part,
                                                               double* out) {
  const int64_t t = (int64_t)blockIdx.x * STAGE_THREADS + threadIdx.x;
  if (t >= total) return;
  const int64_t g = t / ne;
  const int e = (int)(t % ne);
  double acc = 0.0;
  for (int sl = 0; sl < slabs; ++sl) acc += part[((size_t)g * slabs + sl) * ne + e];
  out[t] = acc * scale;
}

// ---- device route ------------------------------------------------------------------------------
// slabs per group: by the shape alone (never by the device)
int corr_slabs(const Shape& s) {
  const int64_t nblk = (int64_t)row_blocks(s.n) * s.C;
  return (int)std::max<int64_t>(1, std::min<int64_t>(nblk, CORR_SLABS / s.G));
}

// lo, hi [G][nc] of the columns whose range is automatic: staged and selected in passes of
// contiguous output columns under the staging cap (the summary's select and interpolation)
int auto_ranges(const Shape& s, const PShape& p, const fitoct_summary_config& sc,
                const void* d_draws, const double* ranges, const double* d_lscale, hipStream_t st,
                std::vector<double>& lo, std::vector<double>& hi) {
  std::vector<std::pair<int, int>> need;   // (output column, its place in the selection)
  for (int j = 0; j < p.nc; ++j)
    for (int g = 0; g < s.G; ++g) {
      const int64_t gj = (int64_t)g * p.nc + j;
      if (!given_range(ranges, gj, lo[gj], hi[gj])) {
        lo[gj] = hi[gj] = NAN;
        if (need.empty() || need.back().second != j) need.emplace_back(p.cols[j], j);
      }
    }
  if (need.empty()) return FITOCT_OK;
  std::sort(need.begin(), need.end());
  const int64_t col_bytes = (int64_t)s.G * s.S * (int64_t)sizeof(double);
  const int ncc_max = (int)items_per_pass(&sc, (int64_t)need.size(), col_bytes);
  const int64_t pairs_max = (int64_t)s.G * ncc_max;
  const int nblk = qhist_blocks(s.S);
  if (pairs_max * nblk >= ((int64_t)1 << 31))
    return fail(FITOCT_E_ARG, "pairs: shape too large for one launch (lower max_staging_bytes)");
  DevBuf X;
  SelectBufs sel;
  FITOCT_TRY(X.alloc((size_t)pairs_max * s.S * sizeof(double)));
  FITOCT_TRY(sel.alloc(pairs_max));
  const SelectRanks ranks(s, &sc, pairs_max);
  std::vector<unsigned long long> h_keys;
  for (size_t i0 = 0; i0 < need.size();) {
    // a pass: consecutive output columns, as many as the cap holds
    size_t i1 = i0 + 1;
    while (i1 < need.size() && (int)(i1 - i0) < ncc_max && need[i1].first == need[i1 - 1].first + 1)
      ++i1;
    const int ncc = (int)(i1 - i0);
    const int64_t pairs = (int64_t)s.G * ncc;
    FITOCT_TRY(queue_stage(kshape(s, need[i0].first, ncc), d_draws, d_lscale, X.as<double>(), st));
    FITOCT_TRY(queue_select(X.as<double>(), pairs, s.S, 4, nblk, sel, ranks, st, h_keys));
    HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < s.G; ++g)
      for (int i = 0; i < ncc; ++i) {
        const int64_t gj = (int64_t)g * p.nc + need[i0 + i].second;
        double a, b;
        if (given_range(ranges, gj, a, b)) continue;
        const unsigned long long* key = h_keys.data() + ((size_t)g * ncc + i) * QT_MAX;
        lo[gj] = quantile_lerp(key_value(key[0]), key_value(key[1]), ranks.qidx[0].frac);
        hi[gj] = quantile_lerp(key_value(key[2]), key_value(key[3]), ranks.qidx[1].frac);
      }
    i0 = i1;
  }
  return FITOCT_OK;
}

int pairs_device(const Shape& s, const PShape& p, const fitoct_summary_config& sc,
                 const void* d_draws, const double* ranges, hipStream_t st,
                 const fitoct_pairs_out* out) {
  DeviceKeep keep;
  HIP_TRY(hipSetDevice(sc.device));
  const int nc = p.nc, nb = p.nb, ne1 = nb + 1, nb2 = nb * nb;
  const int64_t G = s.G, GC = G * nc, limit = (int64_t)1 << 31;
  int64_t sizes[5];
  pairs_sizes(nc, nb, p.planes, G, sizes);
  const bool want_h1 = out->hist1 || out->outside, want_h2 = out->hist2 && p.npan > 0;
  // a call for the correlation alone needs no range, no edge and no byte
  const bool want_bins = out->edges || out->hist1 || out->outside || out->hist2;
  // the panels' work items and launch shape
  const int per_bytes = p.planes * nb2 * (int)sizeof(unsigned int);
  const int ppw = std::max(1, std::min(PANELS_MAX, PANEL_LDS_BYTES / per_bytes));
  std::vector<PanelItem> items;
  for (int a = 0; a + 1 < nc; ++a)
    for (int b0 = a + 1; b0 < nc; b0 += ppw) items.push_back({a, b0, std::min(ppw, nc - b0)});
  const int64_t nvec = p.Sp / VEC;
  const int64_t vec_blocks = (nvec + COUNT_THREADS - 1) / COUNT_THREADS;
  const int marg_blocks = (int)std::min<int64_t>(MARGINAL_BLOCKS, vec_blocks);
  const int64_t n_items = std::max<int64_t>(1, (int64_t)items.size());
  const int shares =
      (int)std::max<int64_t>(1, std::min<int64_t>(vec_blocks, PANEL_GRID / (G * n_items)));
  const int slabs = corr_slabs(s);
  const int ne = nc * (nc + 1) / 2;
  const size_t tile_bytes = row_tile_bytes(s.W);
  const size_t digitise_lds = tile_bytes + sizeof(double) * nc * ne1;
  const size_t panel_lds = (size_t)ppw * per_bytes;
  const size_t corr_lds = tile_bytes + sizeof(double) * STAGE_ROWS * nc;
  if (std::max({digitise_lds, panel_lds, corr_lds}) > (size_t)LDS_LIMIT_BYTES)
    return fail(FITOCT_E_INTERNAL, "pairs: a kernel's LDS exceeds 64 KiB");
  if (row_grid(s) >= limit || GC * marg_blocks >= limit || G * n_items * shares >= limit ||
      s.S >= limit)
    return fail(FITOCT_E_ARG, "pairs: shape too large for one launch");

  DevBuf lscale;
  FITOCT_TRY(lscale.alloc((size_t)G * sizeof(double)));
  HIP_TRY(hipMemcpyAsync(lscale.p, s.lscale.data(), sizeof(double) * G, hipMemcpyHostToDevice, st));

  const PDev pd{nc, nb, p.planes, p.npan, s.S, p.Sp};
  Cols cols{};
  std::copy(p.cols, p.cols + nc, cols.c);
  const KShape k = kshape(s);
  DevBuf dE, K, Dv, dflags;
  FITOCT_TRY(dflags.alloc((size_t)GC * sizeof(int)));
  HIP_TRY(hipMemsetAsync(dflags.p, 0, (size_t)GC * sizeof(int), st));
  std::vector<double> E;
  if (want_bins) {
    // ranges and edges
    std::vector<double> lo((size_t)GC), hi((size_t)GC);
    E.resize((size_t)sizes[0]);
    FITOCT_TRY(auto_ranges(s, p, sc, d_draws, ranges, lscale.as<double>(), st, lo, hi));
    for (int64_t gj = 0; gj < GC; ++gj)
      build_edges(lo[gj], hi[gj], nb, (p.log_mask >> (gj % nc)) & 1, E.data() + gj * ne1);
    // digitise
    FITOCT_TRY(dE.alloc(E.size() * sizeof(double)));
    FITOCT_TRY(K.alloc((size_t)GC * p.Sp));
    FITOCT_TRY(Dv.alloc((size_t)G * p.Sp));
    HIP_TRY(hipMemcpyAsync(dE.p, E.data(), E.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(K.p, BIN_NONE, (size_t)GC * p.Sp, st));   // (the pad bytes count nowhere)
    HIP_TRY(hipMemsetAsync(Dv.p, 0, (size_t)G * p.Sp, st));
    digitise_kernel<<<dim3((unsigned)row_grid(s)), dim3(STAGE_THREADS), digitise_lds, st>>>(
        k, pd, cols, (const double*)d_draws, lscale.as<double>(), dE.as<double>(),
        K.as<unsigned char>(), Dv.as<unsigned char>(), dflags.as<int>());
    HIP_TRY(hipGetLastError());
  }

  // marginals
  DevBuf dh1, dout;
  if (want_h1) {
    FITOCT_TRY(dh1.alloc((size_t)sizes[1] * sizeof(int64_t)));
    FITOCT_TRY(dout.alloc((size_t)sizes[2] * sizeof(int64_t)));
    HIP_TRY(hipMemsetAsync(dh1.p, 0, (size_t)sizes[1] * sizeof(int64_t), st));
    HIP_TRY(hipMemsetAsync(dout.p, 0, (size_t)sizes[2] * sizeof(int64_t), st));
    marginal_kernel<<<dim3((unsigned)(GC * marg_blocks)), dim3(COUNT_THREADS), 0, st>>>(
        pd, marg_blocks, K.as<unsigned char>(), Dv.as<unsigned char>(), dflags.as<int>(),
        dh1.as<unsigned long long>(), dout.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    if (out->hist1)
      HIP_TRY(hipMemcpyAsync(out->hist1, dh1.p, (size_t)sizes[1] * sizeof(int64_t),
                             hipMemcpyDeviceToHost, st));
    if (out->outside)
      HIP_TRY(hipMemcpyAsync(out->outside, dout.p, (size_t)sizes[2] * sizeof(int64_t),
                             hipMemcpyDeviceToHost, st));
  }

  // panels
  DevBuf dh2, ditems;
  if (want_h2) {
    FITOCT_TRY(dh2.alloc((size_t)sizes[3] * sizeof(int64_t)));
    FITOCT_TRY(ditems.alloc(items.size() * sizeof(PanelItem)));
    HIP_TRY(hipMemsetAsync(dh2.p, 0, (size_t)sizes[3] * sizeof(int64_t), st));
    HIP_TRY(hipMemcpyAsync(ditems.p, items.data(), items.size() * sizeof(PanelItem),
                           hipMemcpyHostToDevice, st));
    panel_kernel<<<dim3((unsigned)(G * n_items * shares)), dim3(COUNT_THREADS),
                   panel_lds, st>>>(
        pd, ditems.as<PanelItem>(), (int)n_items, shares, K.as<unsigned char>(),
        Dv.as<unsigned char>(), dflags.as<int>(), dh2.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out->hist2, dh2.p, (size_t)sizes[3] * sizeof(int64_t),
                           hipMemcpyDeviceToHost, st));
  }

  // correlation
  DevBuf part, dmean, dcu;
  std::vector<double> cu;
  if (out->corr) {
    FITOCT_TRY(part.alloc((size_t)G * slabs * ne * sizeof(double)));
    FITOCT_TRY(dmean.alloc((size_t)GC * sizeof(double)));
    FITOCT_TRY(dcu.alloc((size_t)G * ne * sizeof(double)));
    const dim3 grid((unsigned)(G * slabs));
    auto sum_grid = [](int64_t total) { return dim3((unsigned)((total + STAGE_THREADS - 1) / STAGE_THREADS)); };
    mean_partial_kernel<<<grid, dim3(STAGE_THREADS), corr_lds, st>>>(
        k, pd, cols, slabs, (const double*)d_draws, lscale.as<double>(), part.as<double>(),
        want_bins ? nullptr : dflags.as<int>());
    HIP_TRY(hipGetLastError());
    slab_sum_kernel<<<sum_grid(GC), dim3(STAGE_THREADS), 0, st>>>(GC, nc, slabs, 1.0 / (double)s.S,
                                                                  part.as<double>(), dmean.as<double>());
    HIP_TRY(hipGetLastError());
    cov_partial_kernel<<<grid, dim3(STAGE_THREADS), corr_lds, st>>>(
        k, pd, cols, slabs, (const double*)d_draws, lscale.as<double>(), dmean.as<double>(),
        part.as<double>());
    HIP_TRY(hipGetLastError());
    slab_sum_kernel<<<sum_grid(G * ne), dim3(STAGE_THREADS), 0, st>>>(G * ne, ne, slabs, 1.0,
                                                                      part.as<double>(), dcu.as<double>());
    HIP_TRY(hipGetLastError());
    cu.resize((size_t)G * ne);
    HIP_TRY(hipMemcpyAsync(cu.data(), dcu.p, cu.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  std::vector<int> flags((size_t)GC);
  HIP_TRY(hipMemcpyAsync(flags.data(), dflags.p, sizeof(int) * GC, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  if (out->edges) std::copy(E.begin(), E.end(), out->edges);
  for (int64_t gj = 0; gj < GC; ++gj)
    if (flags[gj] & FLAG_NAN) blank_column(p, gj, out);
  for (int g = 0; out->corr && g < s.G; ++g)
    finish_corr(nc, cu.data() + (size_t)g * ne, flags.data() + (size_t)g * nc,
                out->corr + (size_t)g * nc * nc);
  return FITOCT_OK;
}

int pairs_device_checked(const fitoct_problem* probs, int n_groups, int chains, int iters_saved,
                         const void* d_draws, const double* ranges, const fitoct_pairs_config* cfg,
                         void* stream, const fitoct_pairs_out* out) {
  Shape s;
  PShape p;
  fitoct_summary_config sc;
  FITOCT_TRY(check_pairs_args(probs, n_groups, chains, iters_saved, d_draws, cfg, out, s, p, sc));
  FITOCT_TRY(check_device("pairs", &sc, d_draws));
  return pairs_device(s, p, sc, d_draws, ranges, (hipStream_t)stream, out);
}

}  // namespace
}  // namespace fitoct

using namespace fitoct;

// the last run of a plan or of a batch (one body: on_last_run)
template <class Handle>
static int32_t last_run_pairs(const char* fn, Handle* h, const double* ranges, const fitoct_pairs_config* cfg, const fitoct_pairs_out* out) {
  return guarded(fn, [&]() -> int32_t {
    return on_last_run(h, "pairs", "the pairs plot needs", cfg, out != nullptr,
                       [&](const Where& w, const fitoct_pairs_config& c) {
                         return pairs_device_checked(w.probs.data(), (int32_t)w.probs.size(), w.chains,
                                                     w.iters_saved, w.draws, ranges, &c, nullptr, out);
                       });
  });
}

extern "C" {

void fitoct_default_pairs_config(fitoct_pairs_config* cfg) {
  if (!cfg) return;
  *cfg = fitoct_pairs_config{};
  cfg->n_bins = 32;
  cfg->planes = 1;
  cfg->range_probs[0] = 0.0;
  cfg->range_probs[1] = 1.0;
}

int32_t fitoct_pairs_sizes(const fitoct_pairs_config* cfg, int32_t n_groups, int64_t sizes[5]) {
  return guarded(__func__, [&]() -> int32_t {
    FITOCT_TRY(check_pairs_config(cfg));
    if (n_groups < 1 || !sizes) return fail(FITOCT_E_ARG, "pairs: need n_groups >= 1 and sizes");
    pairs_sizes(cfg->n_cols, cfg->n_bins, cfg->planes, n_groups, sizes);
    return FITOCT_OK;
  });
}

int32_t fitoct_pairs_host(const fitoct_problem* probs, int32_t n_groups, int32_t chains,
                          int32_t iters_saved, const double* draws, const double* ranges,
                          const fitoct_pairs_config* cfg, const fitoct_pairs_out* out) {
  return guarded(__func__, [&]() -> int32_t {
    Shape s;
    PShape p;
    fitoct_summary_config sc;
    FITOCT_TRY(check_pairs_args(probs, n_groups, chains, iters_saved, draws, cfg, out, s, p, sc));
    return pairs_host(s, p, sc, draws, ranges, out);
  });
}

int32_t fitoct_pairs_device(const fitoct_problem* probs, int32_t n_groups, int32_t chains,
                            int32_t iters_saved, const void* d_draws, const double* ranges,
                            const fitoct_pairs_config* cfg, void* stream,
                            const fitoct_pairs_out* out) {
  return guarded(__func__, [&]() -> int32_t {
    return pairs_device_checked(probs, n_groups, chains, iters_saved, d_draws, ranges, cfg, stream,
                                out);
  });
}

int32_t fitoct_plan_pairs(fitoct_plan* pl, const double* ranges, const fitoct_pairs_config* cfg,
                          const fitoct_pairs_out* out) {
  return last_run_pairs(__func__, pl, ranges, cfg, out);
}

int32_t fitoct_batch_pairs(fitoct_batch* b, const double* ranges, const fitoct_pairs_config* cfg,
                           const fitoct_pairs_out* out) {
  return last_run_pairs(__func__, b, ranges, cfg, out);
}

}  // extern "C"
