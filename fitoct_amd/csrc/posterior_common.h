// The interface of posterior_common.hip: what the device routes of the posterior summary
// (summary_device.hip), of the rank diagnostics (monitor_device.hip) and of the posterior curves
// (curves_device.hip) share.  The shared kernels -- staging, moments,
// autocovariance, the exact radix select -- are compiled once, in posterior_common.hip, and
// reached through the host functions declared here (queue_stage, queue_moments, queue_select,
// ess_rounds); no kernel is launched across translation units.  Beside the declarations this
// header holds plain structs, the constants the users' own kernels and buffers are sized by, and
// the small inline helpers those kernels need (KShape, chain_series, column_value,
// load_row_tile).
#pragma once
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

constexpr int64_t DEFAULT_STAGING_BYTES = (int64_t)256 << 20;
constexpr int MAX_PROBS = 16;
constexpr int LAG_BLOCK = 64;           // lags per acov_kernel workgroup: one per lane
constexpr int STAGE_ROWS = 32;          // rows of one chain per load_row_tile workgroup
constexpr int STAGE_THREADS = 256;
constexpr int QT_MAX = 2 * MAX_PROBS;   // order statistics per column: x[lo], x[hi] per probability

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
// probabilities (with_probs false: n_probs and probs are not read, np = 0).  Of a problem only
// prior_type, Nn, prior_PD and lambda_scale are read.
int check_args(const std::string& who, bool with_probs, const fitoct_problem* probs, int n_groups,
               int chains, int iters_saved, const void* draws, const fitoct_summary_config* cfg,
               const double* out, Shape& s);
// the checks of a device route that need the runtime: the ordinal, and d_draws a device buffer
int check_device(const std::string& who, const fitoct_summary_config* cfg, const void* d_draws);

// (where a plan's or a batch's last run left its draws: Where, plan_where, batch_where of
// plan_internal.h, defined in posterior_common.hip)

// The last run of a plan or a batch as the arguments of a *_device_checked entry: the NULL check
// (`who` names the table in its message; `rest`: the call's other required pointers are there),
// the refusals of plan_where / batch_where (`needs`), and the caller's config with the device
// of the draws in it.  f(where, config) makes the call; a plan is a run of one group.
inline int where_of(fitoct_plan* pl, const char* needs, Where& w) { return plan_where(pl, needs, w); }
inline int where_of(fitoct_batch* b, const char* needs, Where& w) { return batch_where(b, needs, w); }
template <class Handle, class Config, class F>
int on_last_run(Handle* h, const char* who, const char* needs, const Config* cfg, bool rest,
                F&& f) {
  if (!h || !cfg || !rest) return fail(FITOCT_E_ARG, std::string(who) + ": NULL argument");
  Where w;
  FITOCT_TRY(where_of(h, needs, w));
  Config c = *cfg;
  c.device = w.device;
  return f(w, c);
}

// ---- what the kernels share -----------------------------------------------------------------
// output column j of a raw row (7 sampler columns, then the parameter columns)
FITOCT_HD inline double column_value(const OutModel& m, int j, const double* raw) {
  return j < 7 ? raw[j] : out_value(m, out_spec(m, j - 7), raw + 7);
}

// What every kernel needs of the call (by value: a few words).
struct KShape {
  int G, C, I, W, first, n, h, m;
  int c0, ncc;          // this pass: first output column and number of columns
  OutModel model;
};
inline KShape kshape(const Shape& s, int c0 = 0, int ncc = 0) {
  return KShape{s.G, s.C, s.I, s.W, s.first, s.n, s.h, s.m, c0, ncc, s.model};
}

// X[pair = g * ncc + jc][chain][n]
__device__ inline const double* chain_series(const double* X, const KShape& k, int64_t pair,
                                             int chain) {
  return X + ((size_t)pair * k.C + chain) * k.n;
}

// A kernel that reads the raw rows (stage_kernel, params_kernel) runs one workgroup of
// STAGE_THREADS per (group, chain, block of STAGE_ROWS post-warmup rows), with row_tile_bytes
// of dynamic LDS.
FITOCT_HD inline int row_blocks(int n) { return (n + STAGE_ROWS - 1) / STAGE_ROWS; }
inline int64_t row_grid(const Shape& s) { return (int64_t)row_blocks(s.n) * s.C * s.G; }
inline size_t row_tile_bytes(int W) { return sizeof(double) * STAGE_ROWS * (W | 1); }
struct RowBlock {
  int g, c, i0, rows;   // group, chain, first post-warmup row, rows (< STAGE_ROWS at the end)
};
// The workgroup's rows, contiguous in `draws`, read coalesced into tile[r * Wp + col],
// Wp = k.W | 1 (odd: rows land on different banks); ends with the barrier.
// b: the row block, in 0 .. row_blocks(k.n) * k.C * k.G; a workgroup that loops over row blocks
// puts a barrier between its last read of the tile and the next load.
__device__ inline RowBlock load_row_tile(const KShape& k, const double* draws, double* tile,
                                         int64_t b) {
  const int Wp = k.W | 1;
  const int rblocks = row_blocks(k.n);
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
  return RowBlock{g, c, i0, rows};
}
__device__ inline RowBlock load_row_tile(const KShape& k, const double* draws, double* tile) {
  return load_row_tile(k, draws, tile, (int64_t)blockIdx.x);
}

// (device buffers: DevBuf; the caller's device put back: DeviceKeep -- plan_internal.h)

// Items (output columns, curve pairs) per pass: as many of `items` as the staging cap holds at
// bytes_per_item each (never less than one); the passes are i0 = 0, per, ... with
// min(per, items - i0) items.
inline int64_t items_per_pass(const fitoct_summary_config* cfg, int64_t items,
                              int64_t bytes_per_item) {
  const int64_t cap = cfg->max_staging_bytes > 0 ? cfg->max_staging_bytes : DEFAULT_STAGING_BYTES;
  return std::max<int64_t>(1, std::min<int64_t>(items, cap / bytes_per_item));
}

// stage_kernel on st: raw rows -> the output-layout transform -> X[group][k.ncc][chain][n], the
// columns k.c0 .. of this pass; lscale[G] on the device
int queue_stage(const KShape& k, const void* d_draws, const double* lscale, double* X,
                hipStream_t st);

// Device buffers of the moments and of Geyer's rounds, for up to pairs_max series sets.
struct EssBufs {
  DevBuf mom, flags, acov, act;
  int alloc(int64_t pairs_max, int m);
};
// moments_kernel over X[pairs][k.C][k.n] and its read-back, queued on st (not synchronised):
// h_mom[pair][split chain][4] = mean, centred sum of squares, sum, the middle draw (first half
// of an odd-length chain; 0 otherwise); h_flags: bit 0 a NaN, bit 1 a value that differs from
// the chain's first draw
int queue_moments(const KShape& k, const double* X, int64_t pairs, EssBufs& b, hipStream_t st,
                  std::vector<double>& h_mom, std::vector<int>& h_flags);
// the means cm[m] and sample variances cv[m] of a pair's split chains of h draws (psr_moments,
// ess_moments) from its moments rows mo[m][4]
inline void split_moments(const double* mo, int m, int h, double* cm, double* cv) {
  for (int j = 0; j < m; ++j) {
    cm[j] = mo[4 * j];
    cv[j] = mo[4 * j + 1] / (h - 1);
  }
}
// n_eff of the pairs listed in `active` (ess[pair] is written): autocovariance in blocks of 64
// lags, Geyer's rule (ess_moments) on the host block by block, the next block only for the
// pairs that have not terminated.  h_mom: the moments of X (queue_moments, synchronised), still
// in b.mom on the device.
int ess_rounds(const KShape& k, const double* X, EssBufs& b, hipStream_t st,
               const std::vector<double>& h_mom, std::vector<int> active,
               std::vector<double>& ess);

// ---- exact radix select ---------------------------------------------------------------------
// Device buffers of the select, for up to pairs_max pairs.
struct SelectBufs {
  DevBuf hist, rank, pre, slot, uniq, nuniq;
  int alloc(int64_t pairs_max);
};
// The type-7 indices of the call's probabilities over S pooled draws, and the order statistics
// every pair needs for them, x[lo] and x[hi] of each, as the initial ranks of up to pairs_max
// pairs (and the one distinct prefix every pair starts with).
struct SelectRanks {
  std::vector<QIndex> qidx;
  std::vector<long long> rank0;
  std::vector<int> one;
  SelectRanks(const Shape& s, const fitoct_summary_config* cfg, int64_t pairs_max);
};
// workgroups of the select's histogram kernel per pair
int qhist_blocks(int64_t S);
// The eight passes over X[pairs][S] for T targets per pair and the read-back of the selected
// keys h_keys[pairs][QT_MAX], queued on st (not synchronised).
int queue_select(const double* X, int64_t pairs, int64_t S, int T, int nblk, const SelectBufs& b,
                 const SelectRanks& r, hipStream_t st, std::vector<unsigned long long>& h_keys);

// ---- rows -----------------------------------------------------------------------------------
// The head of pair p's row from the moments, flags and selected keys of its pass (queue_moments,
// queue_select, synchronised).  A NaN among the pair's draws, or `nan` (the curves: a NaN among
// the group's parameters): row[0 .. width) = NaN, returns false.  Else row[0] = the pooled mean,
// row[sd_at] = the pooled sd (n - 1), row[sd_at + 1 ..] = the s.np quantiles, returns true.
// *constant, if given: every split chain held one value throughout.
bool pair_row(const Shape& s, int64_t p, const std::vector<double>& h_mom,
              const std::vector<int>& h_flags, const std::vector<unsigned long long>& h_keys,
              const SelectRanks& r, bool nan, double* row, int width, int sd_at,
              bool* constant = nullptr);

}  // namespace fitoct
