// Posterior bands of the fitted curves from draws that stay in HBM (include/fitoct.h
// "posterior curves"): per depth bin the mean, sd and type-7 quantiles of the
// decay-length modulation dL, the model curve m and the normalised residuals over the pooled
// post-warmup draws, and the curves of picked draws.  The host route (curves_host_group,
// stan_output.cpp) is the reference this one is tested against; both evaluate a bin with the
// one curve_bin of summary_shared.h.
//
// Device route:
//   params_kernel  once per call: raw rows (read coalesced through LDS: load_row_tile)
//                  -> Pm[group][S][3 + Nn], theta and yGP of every pooled draw in the OUTPUT
//                  layout's values, chain-major; a NaN among them flags its group;
//   curve_kernel   per pass: a workgroup takes 256 consecutive pooled draws of one group, each
//                  lane its draw's theta and yGP in registers, and loops over up to CURVE_CHUNK
//                  (quantity, bin) pairs whose basis rows, -c x, y and uy it staged in LDS
//                  (every lane reads the same word: a broadcast); lane s stores X[pair][s];
//   queue_moments, queue_select (the shared layer, posterior_common.hip) reduce
//                  X[pair][chain][n] exactly as the summary does; pair_row forms the rows.
//   curve_pick_kernel  one workgroup per (group, picked draw): the draw's curves over the
//                  bins and br = mean(resid^2), reduced in a fixed order.
// No floating-point atomics: the table is the same bytes from call to call and for any pass size.
#include "posterior_common.h"

namespace fitoct {
namespace {

constexpr int CURVE_THREADS = 256;      // pooled draws per curve_kernel workgroup
constexpr int CURVE_CHUNK = 64;         // pairs per curve_kernel workgroup
constexpr int CURVE_MAX_PAIRS = 4096;   // pairs per pass at most: bounds the select's histograms
constexpr int CURVE_ALL = FITOCT_CURVE_DL | FITOCT_CURVE_M | FITOCT_CURVE_RESID;

// What a curves call computes beyond the summary's Shape.
struct CShape {
  int what = 0, nq = 0, nn = 0, nnp = 0, npar = 3;   // nn: 0 for the mono-exponential model
  int qsel[3] = {0, 0, 0};            // the wanted quantities in order: 0 dL, 1 m, 2 resid
  std::vector<int> N;                 // bins of each group
  std::vector<int64_t> bin_off;       // [G + 1] bins before each group
  int64_t pairs = 0;                  // (group, quantity, bin) over all groups
};

int check_curve_args(const std::string& who, const fitoct_problem* probs, int n_groups, int chains,
                     int iters_saved, const void* draws, int what,
                     const fitoct_summary_config* cfg, const double* out, Shape& s, CShape& c) {
  FITOCT_TRY(check_args(who, true, probs, n_groups, chains, iters_saved, draws, cfg, out, s));
  if (what == 0 || (what & ~CURVE_ALL))
    return fail(FITOCT_E_ARG, who + ": what must be a non-empty set of FITOCT_CURVE_DL, _M, _RESID");
  if (s.S < 2) return fail(FITOCT_E_ARG, who + ": need >= 2 pooled draws");
  c.what = what;
  for (int b = 0; b < 3; ++b)
    if ((what >> b) & 1) c.qsel[c.nq++] = b;
  c.nn = s.model.fam == FITOCT_MODEL_MONOEXP ? 0 : s.model.Nn;
  c.nnp = c.nn == 0 ? 0 : c.nn <= 15 ? 15 : 24;
  c.npar = 3 + c.nn;
  c.bin_off.assign(1, 0);
  for (int g = 0; g < n_groups; ++g) {
    const fitoct_problem& p = probs[g];
    if (!p.x || !p.y || !p.uy || p.N < 2 || p.N > FITOCT_MAX_BINS)
      return fail(FITOCT_E_ARG, who + ": every problem needs x, y, uy and 2 <= N <= " +
                                    std::to_string(FITOCT_MAX_BINS) + " (group " +
                                    std::to_string(g) + ")");
    c.N.push_back(p.N);
    c.bin_off.push_back(c.bin_off.back() + p.N);
  }
  c.pairs = c.bin_off.back() * c.nq;
  return FITOCT_OK;
}

// the groups' bases [bins][nn] one after another: prob->B or as fitoct_build_basis builds it
int group_bases(const fitoct_problem* probs, const Shape& s, const CShape& c,
                std::vector<double>& B) {
  B.assign((size_t)c.bin_off.back() * c.nn, 0.0);
  if (c.nn == 0) return FITOCT_OK;
  std::vector<double> Bg, xg;
  for (int g = 0; g < s.G; ++g) {
    const double* src = probs[g].B;
    if (!src) {
      FITOCT_TRY(build_basis(&probs[g], Bg, xg));
      src = Bg.data();
    }
    std::copy(src, src + (size_t)c.N[g] * c.nn, B.begin() + (size_t)c.bin_off[g] * c.nn);
  }
  return FITOCT_OK;
}

int curves_host(const fitoct_problem* probs, const Shape& s, const CShape& c, const double* draws,
                const fitoct_summary_config* cfg, double* out) {
  std::vector<double> B;
  FITOCT_TRY(group_bases(probs, s, c, B));
  for (int g = 0; g < s.G; ++g)
    FITOCT_TRY(curves_host_group(&probs[g], B.data() + (size_t)c.bin_off[g] * c.nn, s.C, s.I,
                                 s.first, draws + (size_t)g * s.C * s.I * s.W, c.what, s.np,
                                 cfg->probs, out + (size_t)c.bin_off[g] * c.nq * (2 + s.np)));
  return FITOCT_OK;
}

// ---- kernels --------------------------------------------------------------------------------
// The groups' data on the device (by value to the kernels).
struct CurveData {
  const double* ncx;         // [bins] -c x
  const double* y;           // [bins]
  const double* uy;          // [bins]
  const double* B;           // [bins][nnp] basis rows, zero beyond nn
  const int64_t* bin_off;    // [G] bins before each group
  const int* gN;             // [G]
  const double* Pm;          // [G][S][npar]
  int64_t S;
  int npar, nn, nnp;
  int qsel[3];
};
// A workgroup's pairs: `count` consecutive pairs of group g from `first` (= quantity order * N +
// bin), stored from pair `xpair` of the pass's X.
struct Seg {
  int g, first, count, pad_;
  int64_t xpair;
};

// one workgroup per (group, chain, block of STAGE_ROWS rows)
__global__ __launch_bounds__(STAGE_THREADS) void params_kernel(KShape k, int npar,
                                                               const double* draws, double* Pm,
                                                               int* group_nan) {
  extern __shared__ double tile[];   // [STAGE_ROWS][Wp]
  const int Wp = k.W | 1;
  const RowBlock rb = load_row_tile(k, draws, tile);
  const int g = rb.g, c = rb.c, i0 = rb.i0, rows = rb.rows;
  // pooled draw s = chain * n + iteration; a row's npar values are contiguous
  double* dst = Pm + (((size_t)g * k.C + c) * k.n + i0) * npar;
  int bad = 0;
  for (int t = threadIdx.x; t < rows * npar; t += STAGE_THREADS) {
    const int r = t / npar, j = t - r * npar;
    const double v = out_value(k.model, curve_param_spec(k.model, j), tile + r * Wp + 7);
    bad |= v != v;
    dst[t] = v;
  }
  if (bad) atomicOr(&group_nan[g], 1);
}

template <int NNP>
__global__ __launch_bounds__(CURVE_THREADS) void curve_kernel(CurveData d, const Seg* segs,
                                                              int tiles, double* X) {
  constexpr int NB = NNP > 0 ? NNP : 1;
  __shared__ double sB[CURVE_CHUNK][NB];
  __shared__ double sx[CURVE_CHUNK], sy[CURVE_CHUNK], su[CURVE_CHUNK];
  __shared__ int sq[CURVE_CHUNK];
  const Seg sg = segs[blockIdx.x / tiles];
  const int tile = blockIdx.x % tiles;
  const int N = d.gN[sg.g];
  const int64_t b0 = d.bin_off[sg.g];
  for (int t = threadIdx.x; t < sg.count * NNP; t += CURVE_THREADS) {
    const int j = t / NB, kk = t - j * NB;
    sB[j][kk] = d.B[(size_t)(b0 + (sg.first + j) % N) * NB + kk];
  }
  if ((int)threadIdx.x < sg.count) {
    const int j = threadIdx.x, pr = sg.first + j;
    const int64_t bin = b0 + pr % N;
    sx[j] = d.ncx[bin];
    sy[j] = d.y[bin];
    su[j] = d.uy[bin];
    sq[j] = d.qsel[pr / N];
  }
  __syncthreads();
  const int64_t s = (int64_t)tile * CURVE_THREADS + threadIdx.x;
  if (s >= d.S) return;
  const double* pm = d.Pm + ((size_t)sg.g * d.S + s) * d.npar;
  double th[3], yg[NB];
  for (int kk = 0; kk < 3; ++kk) th[kk] = pm[kk];
#pragma unroll
  for (int kk = 0; kk < NNP; ++kk) yg[kk] = kk < d.nn ? pm[3 + kk] : 0.0;
  double* x = X + (size_t)sg.xpair * d.S + s;
  for (int j = 0; j < sg.count; ++j) {
    const CurveBin v = curve_bin(sB[j], NNP, yg, th, sx[j], sy[j], su[j]);
    const int q = sq[j];
    x[(size_t)j * d.S] = q == 0 ? v.dL : q == 1 ? v.m : v.resid;
  }
}

// one workgroup per (group, picked draw); par[G][n_pick][npar], the curves [n_pick][N_g] per
// group, br[G][n_pick]; each output NULL if not wanted
__global__ __launch_bounds__(CURVE_THREADS) void curve_pick_kernel(CurveData d, KShape k,
                                                                   const double* draws,
                                                                   const int64_t* pick, int n_pick,
                                                                   double* dL, double* m,
                                                                   double* resid, double* br,
                                                                   double* par) {
  __shared__ double prm[3 + 24];
  __shared__ double red[CURVE_THREADS];
  const int g = blockIdx.x / n_pick, j = blockIdx.x % n_pick;
  const int64_t s = pick[j];
  const int c = (int)(s / k.n), it = (int)(s % k.n);
  const double* raw = draws + (((size_t)g * k.C + c) * k.I + k.first + it) * k.W + 7;
  if ((int)threadIdx.x < d.npar) {
    const double v = out_value(k.model, curve_param_spec(k.model, threadIdx.x), raw);
    prm[threadIdx.x] = v;
    if (par) par[((size_t)g * n_pick + j) * d.npar + threadIdx.x] = v;
  }
  __syncthreads();
  const int N = d.gN[g];
  const int64_t b0 = d.bin_off[g];
  const size_t o = (size_t)b0 * n_pick + (size_t)j * N;
  double acc = 0.0;
  for (int i = threadIdx.x; i < N; i += CURVE_THREADS) {
    const CurveBin v = curve_bin(d.B + (size_t)(b0 + i) * d.nnp, d.nn, prm + 3, prm, d.ncx[b0 + i],
                                 d.y[b0 + i], d.uy[b0 + i]);
    acc += v.resid * v.resid;
    if (dL) dL[o + i] = v.dL;
    if (m) m[o + i] = v.m;
    if (resid) resid[o + i] = v.resid;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = CURVE_THREADS / 2; w > 0; w >>= 1) {   // a fixed tree: the same bits every call
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (br && threadIdx.x == 0) br[(size_t)g * n_pick + j] = red[0] / N;
}

// ---- device route ---------------------------------------------------------------------------
// the groups' data staged on the device
struct CurveDev {
  DevBuf ncx, y, uy, B, off, gN, Pm;
  CurveData d{};
  int stage(const fitoct_problem* probs, const Shape& s, const CShape& c, hipStream_t st) {
    std::vector<double> Bh;
    FITOCT_TRY(group_bases(probs, s, c, Bh));
    const int64_t bins = c.bin_off.back();
    const int nb = std::max(1, c.nnp);
    std::vector<double> h_ncx(bins), h_y(bins), h_uy(bins), h_B((size_t)bins * nb, 0.0);
    for (int g = 0; g < s.G; ++g) {
      const double cc = (double)probs[g].data_type;
      for (int i = 0; i < c.N[g]; ++i) {
        const int64_t b = c.bin_off[g] + i;
        h_ncx[b] = -cc * probs[g].x[i];
        h_y[b] = probs[g].y[i];
        h_uy[b] = probs[g].uy[i];
        for (int k = 0; k < c.nn; ++k) h_B[(size_t)b * nb + k] = Bh[(size_t)b * c.nn + k];
      }
    }
    FITOCT_TRY(ncx.alloc(sizeof(double) * bins));
    FITOCT_TRY(y.alloc(sizeof(double) * bins));
    FITOCT_TRY(uy.alloc(sizeof(double) * bins));
    FITOCT_TRY(B.alloc(sizeof(double) * h_B.size()));
    FITOCT_TRY(off.alloc(sizeof(int64_t) * s.G));
    FITOCT_TRY(gN.alloc(sizeof(int) * s.G));
    // (pageable host buffers: the copies below have completed when the calls return)
    HIP_TRY(hipMemcpyAsync(ncx.p, h_ncx.data(), sizeof(double) * bins, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(y.p, h_y.data(), sizeof(double) * bins, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(uy.p, h_uy.data(), sizeof(double) * bins, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(B.p, h_B.data(), sizeof(double) * h_B.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(off.p, c.bin_off.data(), sizeof(int64_t) * s.G, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(gN.p, c.N.data(), sizeof(int) * s.G, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    d = CurveData{ncx.as<double>(), y.as<double>(), uy.as<double>(), B.as<double>(),
                  off.as<int64_t>(), gN.as<int>(), nullptr, s.S, c.npar, c.nn, nb,
                  {c.qsel[0], c.qsel[1], c.qsel[2]}};
    return FITOCT_OK;
  }
};

int curves_device(const fitoct_problem* probs, const Shape& s, const CShape& c, const void* d_draws,
                  const fitoct_summary_config* cfg, hipStream_t st, double* out) {
  DeviceKeep keep;
  HIP_TRY(hipSetDevice(cfg->device));
  const int width = 2 + s.np, T = 2 * s.np;
  const int64_t ppp = items_per_pass(cfg, std::min<int64_t>(c.pairs, CURVE_MAX_PAIRS),
                                     s.S * (int64_t)sizeof(double));   // pairs of S doubles
  const int tiles = (int)((s.S + CURVE_THREADS - 1) / CURVE_THREADS);
  const int nblk = qhist_blocks(s.S);
  const int64_t limit = (int64_t)1 << 31;
  if (row_grid(s) >= limit || ppp * s.m >= limit || ppp * nblk >= limit ||
      (ppp + s.G) * tiles >= limit || s.S >= limit)
    return fail(FITOCT_E_ARG, "curves: shape too large for one launch (lower max_staging_bytes)");

  // every pass's workgroups: the pass's pairs cut at group borders and into chunks
  std::vector<Seg> segs;
  std::vector<size_t> pass_seg(1, 0);
  for (int64_t p0 = 0; p0 < c.pairs; p0 += ppp) {
    const int64_t p1 = std::min(c.pairs, p0 + ppp);
    int g = (int)(std::upper_bound(c.bin_off.begin(), c.bin_off.end(), p0 / c.nq) -
                  c.bin_off.begin()) - 1;
    for (int64_t p = p0; p < p1;) {
      while (c.bin_off[g + 1] * c.nq <= p) ++g;
      const int64_t gend = std::min(p1, c.bin_off[g + 1] * c.nq);
      const int cnt = (int)std::min<int64_t>(CURVE_CHUNK, gend - p);
      segs.push_back(Seg{g, (int)(p - c.bin_off[g] * c.nq), cnt, 0, p - p0});
      p += cnt;
    }
    pass_seg.push_back(segs.size());
  }

  CurveDev cd;
  DevBuf X, Pm, gnan, dsegs, mom, flags;
  SelectBufs sel;
  FITOCT_TRY(cd.stage(probs, s, c, st));
  FITOCT_TRY(Pm.alloc((size_t)s.G * s.S * c.npar * sizeof(double)));
  FITOCT_TRY(gnan.alloc((size_t)s.G * sizeof(int)));
  FITOCT_TRY(dsegs.alloc(segs.size() * sizeof(Seg)));
  FITOCT_TRY(X.alloc((size_t)ppp * s.S * sizeof(double)));
  EssBufs eb;   // the moments and their flags only
  FITOCT_TRY(eb.mom.alloc((size_t)ppp * s.m * 4 * sizeof(double)));
  FITOCT_TRY(eb.flags.alloc((size_t)ppp * s.m * sizeof(int)));
  if (T > 0) FITOCT_TRY(sel.alloc(ppp));
  cd.d.Pm = Pm.as<double>();
  const KShape k = kshape(s);

  std::vector<int> h_gnan(s.G);
  HIP_TRY(hipMemsetAsync(gnan.p, 0, (size_t)s.G * sizeof(int), st));
  HIP_TRY(hipMemcpyAsync(dsegs.p, segs.data(), segs.size() * sizeof(Seg), hipMemcpyHostToDevice, st));
  params_kernel<<<dim3((unsigned)row_grid(s)), dim3(STAGE_THREADS), row_tile_bytes(s.W), st>>>(
      k, c.npar, (const double*)d_draws, Pm.as<double>(), gnan.as<int>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h_gnan.data(), gnan.p, (size_t)s.G * sizeof(int), hipMemcpyDeviceToHost, st));

  const SelectRanks ranks(s, cfg, ppp);
  std::vector<double> h_mom;
  std::vector<int> h_flags;
  std::vector<unsigned long long> h_keys;
  for (size_t ps = 0; ps + 1 < pass_seg.size(); ++ps) {
    const int64_t p0 = (int64_t)ps * ppp, pairs = std::min(c.pairs, p0 + ppp) - p0;
    const Seg* sg = dsegs.as<Seg>() + pass_seg[ps];
    const dim3 grid((unsigned)((int64_t)(pass_seg[ps + 1] - pass_seg[ps]) * tiles));
    if (c.nnp == 0) curve_kernel<0><<<grid, dim3(CURVE_THREADS), 0, st>>>(cd.d, sg, tiles, X.as<double>());
    else if (c.nnp == 15) curve_kernel<15><<<grid, dim3(CURVE_THREADS), 0, st>>>(cd.d, sg, tiles, X.as<double>());
    else curve_kernel<24><<<grid, dim3(CURVE_THREADS), 0, st>>>(cd.d, sg, tiles, X.as<double>());
    HIP_TRY(hipGetLastError());
    FITOCT_TRY(queue_moments(k, X.as<double>(), pairs, eb, st, h_mom, h_flags));
    if (T > 0) FITOCT_TRY(queue_select(X.as<double>(), pairs, s.S, T, nblk, sel, ranks, st, h_keys));
    HIP_TRY(hipStreamSynchronize(st));

    int g = 0;
    for (int64_t p = 0; p < pairs; ++p) {
      while (c.bin_off[g + 1] * c.nq <= p0 + p) ++g;
      pair_row(s, p, h_mom, h_flags, h_keys, ranks, h_gnan[g] != 0, out + (size_t)(p0 + p) * width,
               width, 1);
    }
  }
  return FITOCT_OK;
}

// curves and parameters of picked draws; the outputs are host buffers, each NULL if not wanted
int curves_pick(const fitoct_problem* probs, const Shape& s, const CShape& c, const void* d_draws,
                const fitoct_summary_config* cfg, hipStream_t st, int n_pick, const int64_t* pick,
                double* dL, double* m, double* resid, double* br, double* theta, double* ygp) {
  if (n_pick == 0) return FITOCT_OK;
  DeviceKeep keep;
  HIP_TRY(hipSetDevice(cfg->device));
  if ((int64_t)s.G * n_pick >= ((int64_t)1 << 31))
    return fail(FITOCT_E_ARG, "curves: too many picked draws for one launch");
  CurveDev cd;
  FITOCT_TRY(cd.stage(probs, s, c, st));
  const size_t nc = (size_t)c.bin_off.back() * n_pick, nb = (size_t)s.G * n_pick;
  DevBuf dpick, ddL, dm, dr, dbr, dpar;
  FITOCT_TRY(dpick.alloc(sizeof(int64_t) * n_pick));
  if (dL) FITOCT_TRY(ddL.alloc(sizeof(double) * nc));
  if (m) FITOCT_TRY(dm.alloc(sizeof(double) * nc));
  if (resid) FITOCT_TRY(dr.alloc(sizeof(double) * nc));
  if (br) FITOCT_TRY(dbr.alloc(sizeof(double) * nb));
  const bool want_par = theta || ygp;
  if (want_par) FITOCT_TRY(dpar.alloc(sizeof(double) * nb * c.npar));
  HIP_TRY(hipMemcpyAsync(dpick.p, pick, sizeof(int64_t) * n_pick, hipMemcpyHostToDevice, st));
  curve_pick_kernel<<<dim3((unsigned)(s.G * n_pick)), dim3(CURVE_THREADS), 0, st>>>(
      cd.d, kshape(s), (const double*)d_draws, dpick.as<int64_t>(), n_pick,
      dL ? ddL.as<double>() : nullptr, m ? dm.as<double>() : nullptr,
      resid ? dr.as<double>() : nullptr, br ? dbr.as<double>() : nullptr,
      want_par ? dpar.as<double>() : nullptr);
  HIP_TRY(hipGetLastError());
  std::vector<double> h_par(want_par ? nb * c.npar : 0);
  if (dL) HIP_TRY(hipMemcpyAsync(dL, ddL.p, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
  if (m) HIP_TRY(hipMemcpyAsync(m, dm.p, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
  if (resid) HIP_TRY(hipMemcpyAsync(resid, dr.p, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
  if (br) HIP_TRY(hipMemcpyAsync(br, dbr.p, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
  if (want_par)
    HIP_TRY(hipMemcpyAsync(h_par.data(), dpar.p, sizeof(double) * h_par.size(),
                           hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (size_t r = 0; want_par && r < nb; ++r) {
    const double* pr = h_par.data() + r * c.npar;
    if (theta) std::copy(pr, pr + 3, theta + r * 3);
    if (ygp) std::copy(pr + 3, pr + 3 + c.nn, ygp + r * c.nn);
  }
  return FITOCT_OK;
}

int curves_device_checked(const fitoct_problem* probs, int n_groups, int chains, int iters_saved,
                          const void* d_draws, int what, const fitoct_summary_config* cfg,
                          void* stream, double* out) {
  Shape s;
  CShape c;
  FITOCT_TRY(check_curve_args("curves", probs, n_groups, chains, iters_saved, d_draws, what, cfg,
                              out, s, c));
  FITOCT_TRY(check_device("curves", cfg, d_draws));
  return curves_device(probs, s, c, d_draws, cfg, (hipStream_t)stream, out);
}

int curves_pick_checked(const fitoct_problem* probs, int n_groups, int chains, int iters_saved,
                        const void* d_draws, const fitoct_summary_config* cfg, void* stream,
                        int n_pick, const int64_t* pick, double* dL, double* m, double* resid,
                        double* br, double* theta, double* ygp) {
  Shape s;
  CShape c;
  if (!cfg) return fail(FITOCT_E_ARG, "curves pick: NULL argument (problems, draws, config or out)");
  fitoct_summary_config cq = *cfg;   // the probabilities play no part
  cq.n_probs = 0;
  static const double some = 0.0;    // (the outputs are optional: check_args wants one)
  FITOCT_TRY(check_curve_args("curves pick", probs, n_groups, chains, iters_saved, d_draws,
                              CURVE_ALL, &cq, &some, s, c));
  if (n_pick < 0 || (n_pick > 0 && !pick))
    return fail(FITOCT_E_ARG, "curves pick: n_pick is negative or pick is NULL");
  for (int j = 0; j < n_pick; ++j)
    if (pick[j] < 0 || pick[j] >= s.S)
      return fail(FITOCT_E_ARG, "curves pick: pick[" + std::to_string(j) + "] = " +
                                    std::to_string((long long)pick[j]) + " is not in [0, " +
                                    std::to_string((long long)s.S) + ")");
  FITOCT_TRY(check_device("curves pick", &cq, d_draws));
  return curves_pick(probs, s, c, d_draws, &cq, (hipStream_t)stream, n_pick, pick, dL, m, resid,
                     br, theta, ygp);
}

// ---- the last run of a plan or a batch (on_last_run: the refusals) ---------------------------
// the picked draws of a plan's run, or of group `group` of a batch's
template <class Handle>
int last_run_pick(const char* fn, Handle* h, int group, const fitoct_summary_config* cfg,
                  int n_pick, const int64_t* pick, double* dL, double* m, double* resid,
                  double* br, double* theta, double* ygp) {
  return guarded(fn, [&]() -> int32_t {
    return on_last_run(h, "curves pick", "the curves need", cfg, true,
                       [&](const Where& w, const fitoct_summary_config& c) {
                         if (group < 0 || group >= (int)w.probs.size())
                           return fail(FITOCT_E_ARG, "curves pick: group out of range");
                         return curves_pick_checked(
                             &w.probs[group], 1, w.chains, w.iters_saved,
                             w.draws + (size_t)group * w.group_bytes, &c, nullptr, n_pick, pick,
                             dL, m, resid, br, theta, ygp);
                       });
  });
}

template <class Handle>
int last_run_curves(const char* fn, Handle* h, int what, const fitoct_summary_config* cfg,
                    double* out) {
  return guarded(fn, [&]() -> int32_t {
    return on_last_run(h, "curves", "the curves need", cfg, out != nullptr,
                       [&](const Where& w, const fitoct_summary_config& c) {
                         return curves_device_checked(w.probs.data(), (int32_t)w.probs.size(),
                                                      w.chains, w.iters_saved, w.draws, what, &c,
                                                      nullptr, out);
                       });
  });
}

}  // namespace
}  // namespace fitoct

using namespace fitoct;

extern "C" {

int32_t fitoct_curves_width(int32_t n_probs) {
  if (n_probs < 0 || n_probs > MAX_PROBS) return fail(FITOCT_E_ARG, "n_probs must be in [0, 16]");
  return 2 + n_probs;
}

int32_t fitoct_curves_host(const fitoct_problem* probs, int32_t n_groups, int32_t chains,
                           int32_t iters_saved, const double* draws, int32_t what,
                           const fitoct_summary_config* cfg, double* out) {
  return guarded(__func__, [&]() -> int32_t {
    Shape s;
    CShape c;
    FITOCT_TRY(check_curve_args("curves", probs, n_groups, chains, iters_saved, draws, what, cfg,
                                out, s, c));
    return curves_host(probs, s, c, draws, cfg, out);
  });
}

int32_t fitoct_curves_device(const fitoct_problem* probs, int32_t n_groups, int32_t chains,
                             int32_t iters_saved, const void* d_draws, int32_t what,
                             const fitoct_summary_config* cfg, void* stream, double* out) {
  return guarded(__func__, [&]() -> int32_t {
    return curves_device_checked(probs, n_groups, chains, iters_saved, d_draws, what, cfg, stream,
                                 out);
  });
}

int32_t fitoct_plan_curves(fitoct_plan* pl, int32_t what, const fitoct_summary_config* cfg,
                           double* out) {
  return last_run_curves(__func__, pl, what, cfg, out);
}

int32_t fitoct_batch_curves(fitoct_batch* b, int32_t what, const fitoct_summary_config* cfg,
                            double* out) {
  return last_run_curves(__func__, b, what, cfg, out);
}

int32_t fitoct_curves_pick_device(const fitoct_problem* probs, int32_t n_groups, int32_t chains,
                                  int32_t iters_saved, const void* d_draws,
                                  const fitoct_summary_config* cfg, void* stream, int32_t n_pick,
                                  const int64_t* pick, double* dL, double* m, double* resid,
                                  double* br) {
  return guarded(__func__, [&]() -> int32_t {
    return curves_pick_checked(probs, n_groups, chains, iters_saved, d_draws, cfg, stream, n_pick,
                               pick, dL, m, resid, br, nullptr, nullptr);
  });
}

int32_t fitoct_plan_curves_pick(fitoct_plan* pl, const fitoct_summary_config* cfg, int32_t n_pick,
                                const int64_t* pick, double* dL, double* m, double* resid,
                                double* br) {
  return last_run_pick(__func__, pl, 0, cfg, n_pick, pick, dL, m, resid, br, nullptr, nullptr);
}

int32_t fitoct_batch_curves_pick(fitoct_batch* b, int32_t group, const fitoct_summary_config* cfg,
                                 int32_t n_pick, const int64_t* pick, double* dL, double* m,
                                 double* resid, double* br) {
  return last_run_pick(__func__, b, group, cfg, n_pick, pick, dL, m, resid, br, nullptr, nullptr);
}

int32_t fitoct_plan_curves_pick_params(fitoct_plan* pl, const fitoct_summary_config* cfg,
                                       int32_t n_pick, const int64_t* pick, double* theta,
                                       double* ygp) {
  return last_run_pick(__func__, pl, 0, cfg, n_pick, pick, nullptr, nullptr, nullptr, nullptr,
                       theta, ygp);
}

int32_t fitoct_batch_curves_pick_params(fitoct_batch* b, int32_t group,
                                        const fitoct_summary_config* cfg, int32_t n_pick,
                                        const int64_t* pick, double* theta, double* ygp) {
  return last_run_pick(__func__, b, group, cfg, n_pick, pick, nullptr, nullptr, nullptr, nullptr,
                       theta, ygp);
}

}  // extern "C"
