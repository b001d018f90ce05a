// C ABI of libfitoct (include/fitoct.h): the miscellaneous entries, the logp evaluator and the
// single-device plan -- argument checking, the upload of a data plan (plan_data.cpp), kernel
// dispatch and result download.  Batch mode: batch.cpp; device lists: multi_device.cpp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "fitoct.h"
#include "host_internal.h"
#include "kernel_params.h"
#include "plan_internal.h"

namespace fitoct {
int mig_img_words(int ppl);
}  // namespace fitoct

using namespace fitoct;


int fitoct::check_init(int C, int D, const double* q, const double* eps, const double* minv) {
  if (eps)
    for (int c = 0; c < C; ++c)
      if (!(eps[c] > 0.0 && eps[c] < INFINITY))
        return fail(FITOCT_E_ARG, "stepsize must be finite and > 0");
  if (minv)
    for (size_t i = 0; i < (size_t)C * D; ++i)
      if (!(minv[i] > 0.0 && minv[i] < INFINITY))
        return fail(FITOCT_E_ARG, "inv_metric must be finite and > 0");
  if (q)
    for (size_t i = 0; i < (size_t)C * D; ++i)
      if (!isfinite(q[i])) return fail(FITOCT_E_ARG, "q_init must be finite");
  return FITOCT_OK;
}

struct fitoct_evaluator {
  fitoct_plan* pl = nullptr;
  int capacity = 0, D = 0, cur_n = -1;
  long long evals = 0;
  double lp_const = 0.0;
  DevBuf d_q, d_out;
  std::vector<char> logmask;
  std::vector<double> host;
  ~fitoct_evaluator() { delete pl; }
};

namespace {

// The device side of a data plan (plan_data.cpp): check the device, upload the staged bytes and
// the factorised basis, and point the launch parameters at them.
int plan_common(fitoct_plan* pl, const fitoct_problem* p, DataPlan& dp, int chains, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(FITOCT_E_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(FITOCT_E_ARG, "device ordinal out of range");
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));

  pl->prob = *p;
  pl->prob.x = pl->prob.y = pl->prob.uy = pl->prob.B = nullptr;  // never keep caller pointers
  pl->mixed = dp.mixed;
  pl->bpt = dp.bpt;
  pl->nnp = dp.nnp;
  pl->ppl = dp.ppl;
  pl->h_xyu = std::move(dp.h_xyu);
  pl->h_B = std::move(dp.h_B);
  const std::vector<char>& staged = dp.staged;
  const size_t kbytes = sizeof(double) * (dp.kinv.size() + dp.bv.size());
  FITOCT_TRY(pl->d_data.alloc(staged.size() + kbytes + 16));
  char* d_data = pl->d_data.as<char>();
  HIP_TRY(hipMemcpy(d_data, staged.data(), staged.size(), hipMemcpyHostToDevice));
  double* dk = (double*)(d_data + (staged.size() + 15) / 16 * 16);
  KParams& k = pl->kp;
  k = dp.kp;
  if (k.mode == MODE_POLY) {
    HIP_TRY(hipMemcpy(dk, dp.kinv.data(), sizeof(double) * dp.kinv.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dk + dp.kinv.size(), dp.bv.data(), sizeof(double) * dp.bv.size(),
                      hipMemcpyHostToDevice));
  }
  const size_t rs = pl->mixed ? sizeof(float) : sizeof(double);
  k.cx = d_data;
  k.y = d_data + rs * k.n_pad;
  k.isu = d_data + 2 * rs * k.n_pad;
  k.B = d_data + 3 * rs * k.n_pad;
  k.Kinv = dk;
  k.bvec = dk + dp.kinv.size();
  k.chains = chains;
  pl->ncu = std::max(1, prop.multiProcessorCount);
  return FITOCT_OK;
}

}  // namespace

extern "C" {

int32_t fitoct_abi_version(void) { return FITOCT_ABI_VERSION; }

int32_t fitoct_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int32_t fitoct_struct_sizes(int32_t* problem, int32_t* config, int32_t* result, int32_t* info) {
  if (problem) *problem = (int32_t)sizeof(fitoct_problem);
  if (config) *config = (int32_t)sizeof(fitoct_config);
  if (result) *result = (int32_t)sizeof(fitoct_result);
  if (info) *info = (int32_t)sizeof(fitoct_plan_info);
  return FITOCT_OK;
}

void fitoct_default_config(fitoct_config* c) {
  if (!c) return;
  memset(c, 0, sizeof *c);
  c->chains = 4;  // server.R:469
  c->warmup = 500;
  c->samples = 1000;
  c->seed = 1234;
  c->adapt_delta = 0.8;
  c->max_treedepth = 10;
  c->adapt_engaged = 1;
  c->stepsize = 1.0;
  c->gamma = 0.05;
  c->kappa = 0.75;
  c->t0 = 10.0;
  c->init_buffer = 75;
  c->term_buffer = 50;
  c->window = 25;
  c->init_radius = 2.0;
  c->save_warmup = 1;
  c->precision = FITOCT_PREC_F64;
}

void fitoct_default_problem(fitoct_problem* p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->data_type = 2;
  p->Nn = 10;
  p->grid_type = FITOCT_GRID_INTERNAL;
  p->prior_type = FITOCT_PRIOR_NORMAL;
  p->lambda_rate = 0.1;
  p->lambda_scale = 10.0;
  p->nu = 1.0;
  p->sigma_scale = 10.0;
  p->nugget = 1e-9;
  p->theta0[0] = 1000.0;
  p->theta0[1] = 2000.0;
  p->theta0[2] = 300.0;
  for (int j = 0; j < 3; ++j) p->Sigma0[4 * j] = (0.05 * p->theta0[j]) * (0.05 * p->theta0[j]);
}

int32_t fitoct_dim(int32_t prior_type, int32_t Nn) { return model_dim(prior_type, Nn); }

int32_t fitoct_n_cols(int32_t prior_type, int32_t Nn) {
  const int D = model_dim(prior_type, Nn);
  return D < 0 ? -1 : D + 8;
}

int32_t fitoct_column_name(int32_t prior_type, int32_t Nn, int32_t i, char* buf, int32_t buflen) {
  return guarded(__func__, [&]() -> int32_t {
    const std::string s = column_name(prior_type, Nn, i);
    if (s.empty()) return fail(FITOCT_E_ARG, "column index out of range");
    if (!buf || buflen < (int32_t)s.size() + 1) return fail(FITOCT_E_ARG, "buffer too small");
    memcpy(buf, s.c_str(), s.size() + 1);
    return FITOCT_OK;
  });
}

int32_t fitoct_build_basis(const fitoct_problem* prob, double* B_out, double* xGP_out) {
  return guarded(__func__, [&]() -> int32_t {
    if (!prob || !B_out) return fail(FITOCT_E_ARG, "NULL argument");
    if (prob->N < 2 || !prob->x) return fail(FITOCT_E_ARG, "need x with N >= 2");
    std::vector<double> B, xg;
    const int rc = build_basis(prob, B, xg);
    if (rc) return rc;
    memcpy(B_out, B.data(), B.size() * sizeof(double));
    if (xGP_out) memcpy(xGP_out, xg.data(), xg.size() * sizeof(double));
    return FITOCT_OK;
  });
}

int32_t fitoct_evaluator_create(const fitoct_problem* prob, int32_t capacity, int32_t precision,
                                int32_t device, fitoct_evaluator** out) {
  return guarded(__func__, [&]() -> int32_t {
    if (!out) return fail(FITOCT_E_ARG, "out is NULL");
    *out = nullptr;
    if (capacity < 1) return fail(FITOCT_E_ARG, "capacity must be >= 1");
    const Switches sw = Switches::from_env();
    DataPlan dp;
    FITOCT_TRY(plan_data(prob, precision, sw, -1, false, dp));
    // released on every early return or exception until handed to the caller
    std::unique_ptr<fitoct_evaluator> ev(new fitoct_evaluator());
    fitoct_plan* pl = ev->pl = new fitoct_plan();
    pl->cfg.device = device;
    FITOCT_TRY(plan_common(pl, prob, dp, capacity, device));
    // the logp kernel takes the schedule's chains (points) per tile, nothing else
    int rc = FITOCT_OK;
    pl->sched = choose_schedule(pl->ppl, pl->kp.mode, capacity, 0, pl->ncu, 0, sw, &rc);
    if (rc) return rc;
    KParams& k = pl->kp;
    k.G = pl->sched.G;
    const int D = k.D;
    ev->capacity = capacity;
    ev->D = D;
    ev->lp_const = lp_constant(prob);
    ev->logmask.resize(D);
    for (int j = 0; j < D; ++j) ev->logmask[j] = log_transformed(prob->prior_type, prob->Nn, j);
    FITOCT_TRY(ev->d_q.alloc(sizeof(double) * (size_t)capacity * D));
    FITOCT_TRY(ev->d_out.alloc(sizeof(double) * (size_t)capacity * (D + 2)));
    FITOCT_TRY(pl->d_kp.alloc(sizeof(KParams)));
    k.q_in = ev->d_q.as<double>();
    k.grad_out = ev->d_out.as<double>();
    *out = ev.release();
    return FITOCT_OK;
  });
}

int32_t fitoct_evaluator_run(fitoct_evaluator* ev, int32_t n, const double* q, int32_t jacobian,
                             int32_t normalised, double* lp_out, double* grad_out,
                             double* sumr2_out) {
  return guarded(__func__, [&]() -> int32_t {
    if (!ev || !q || !lp_out) return fail(FITOCT_E_ARG, "bad buffers");
    if (n < 1 || n > ev->capacity) return fail(FITOCT_E_ARG, "n_points must be in [1, capacity]");
    fitoct_plan* pl = ev->pl;
    KParams& k = pl->kp;
    const int D = ev->D;
    HIP_TRY(hipSetDevice(pl->cfg.device));
    if (n != ev->cur_n) {  // outputs are laid out for n points: grad[n][D] | lp[n] | sumr2[n]
      k.chains = n;
      k.lp_out = ev->d_out.as<double>() + (size_t)n * D;
      k.s2_out = k.lp_out + n;
      HIP_TRY(hipMemcpy(pl->d_kp.p, &k, sizeof(KParams), hipMemcpyHostToDevice));
      ev->cur_n = n;
    }
    HIP_TRY(hipMemcpy(ev->d_q.p, q, sizeof(double) * (size_t)n * D, hipMemcpyHostToDevice));
    HIP_TRY(launch(true, pl->mixed, pl->bpt, pl->nnp, k, pl->d_kp.as<KParams>(), (n + k.G - 1) / k.G, 0));
    // one copy back of grad | lp | sumr2 (contiguous)
    ev->host.resize((size_t)n * (D + 2));
    HIP_TRY(hipMemcpy(ev->host.data(), ev->d_out.p, sizeof(double) * ev->host.size(),
                      hipMemcpyDeviceToHost));
    const double* g = ev->host.data();
    const double* lp = g + (size_t)n * D;
    for (int i = 0; i < n; ++i) {
      double v = lp[i];
      const double* qi = q + (size_t)i * D;
      if (!jacobian)
        for (int j = 0; j < D; ++j)
          if (ev->logmask[j]) v -= qi[j];
      if (normalised) v += ev->lp_const;
      lp_out[i] = isfinite(lp[i]) ? v : -INFINITY;
      if (grad_out)
        for (int j = 0; j < D; ++j)
          grad_out[(size_t)i * D + j] = g[(size_t)i * D + j] - ((!jacobian && ev->logmask[j]) ? 1.0 : 0.0);
      if (sumr2_out) sumr2_out[i] = lp[n + i];
    }
    ev->evals += n;
    return FITOCT_OK;
  });
}

void fitoct_evaluator_destroy(fitoct_evaluator* ev) { delete ev; }

int32_t fitoct_logp_grad(const fitoct_problem* prob, int32_t n_points, const double* q,
                         double* lp_out, double* grad_out, double* sumr2_out, int32_t precision,
                         int32_t device) {
  return guarded(__func__, [&]() -> int32_t {
    if (n_points < 1 || !q || !lp_out || !grad_out) return fail(FITOCT_E_ARG, "bad buffers");
    fitoct_evaluator* ev = nullptr;
    int rc = fitoct_evaluator_create(prob, n_points, precision, device, &ev);
    if (rc) return rc;
    rc = fitoct_evaluator_run(ev, n_points, q, 1, 0, lp_out, grad_out, sumr2_out);
    fitoct_evaluator_destroy(ev);
    return rc;
  });
}

int32_t fitoct_plan_create(const fitoct_problem* prob, const fitoct_config* cfg,
                           fitoct_plan** out) {
  return guarded(__func__, [&]() -> int32_t {
    if (!out) return fail(FITOCT_E_ARG, "out is NULL");
    *out = nullptr;
    if (!cfg) return fail(FITOCT_E_ARG, "config is NULL");
    if (cfg->chains < 1) return fail(FITOCT_E_ARG, "chains must be >= 1");
    std::vector<int> devs;
    const int rc = resolve_devices(cfg, cfg->chains, devs);
    if (rc) return rc;
    if (devs.size() > 1) return group_plan_create(prob, cfg, devs, out);
    fitoct_config c = *cfg;
    c.device = devs[0];
    c.n_devices = 0;
    FITOCT_TRY(check_config(&c));
    const Switches sw = Switches::from_env();
    DataPlan dp;
    FITOCT_TRY(plan_data(prob, c.precision, sw, -1, false, dp));
    return plan_create(prob, &c, sw, 0, dp, out);
  });
}

}  // extern "C"

int fitoct::PairBuffers::alloc(int tiles_, int ppl, const Switches& sw) {
  tiles = tiles_;
  // the start (q, p, g, minv + scalars), then two subtree record slots (5 vectors + 16 scalars)
  stride = (PAIR_START_DOUBLES + WAVE * ppl * 4 + 2 * (WAVE * ppl * 5 + 16) + 15) / 16 * 16;
  test_absent = sw.test_pair_absent ? 1 : 0;
  FITOCT_TRY(hdr.alloc(sizeof(int) * PAIR_HDR_INTS * (size_t)tiles));
  return buf.alloc(sizeof(double) * (size_t)stride * tiles);
}
void fitoct::PairBuffers::apply(KParams& k) const {
  k.pair = 1;
  k.pair_tiles = tiles;
  k.pair_stride = stride;
  k.pair_test_absent = test_absent;
  k.pair_hdr = hdr.as<int>();
  k.pair_buf = buf.as<double>();
}
int fitoct::PairBuffers::zero(hipStream_t st) const {
  HIP_TRY(hipMemsetAsync(hdr.p, 0, sizeof(int) * PAIR_HDR_INTS * (size_t)tiles, st));
  return FITOCT_OK;
}

int fitoct::check_config(const fitoct_config* cfg) {
  if (!cfg) return fail(FITOCT_E_ARG, "config is NULL");
  if (cfg->chains < 1) return fail(FITOCT_E_ARG, "chains must be >= 1");
  if (cfg->warmup < 0 || cfg->samples < 1) return fail(FITOCT_E_ARG, "warmup >= 0, samples >= 1");
  if (cfg->max_treedepth < 1 || cfg->max_treedepth > MAXDEPTH)
    return fail(FITOCT_E_ARG, "max_treedepth must be in [1, 16]");
  if (!(cfg->adapt_delta > 0.0 && cfg->adapt_delta < 1.0))
    return fail(FITOCT_E_ARG, "adapt_delta must be in (0, 1)");
  if (!(cfg->stepsize > 0.0)) return fail(FITOCT_E_ARG, "stepsize must be > 0");
  return FITOCT_OK;
}

// A plan: upload the data plan (plan_common), choose the launch schedule (schedule.cpp),
// allocate what it asks for and copy it into the kernel's parameters.
int fitoct::plan_create(const fitoct_problem* prob, const fitoct_config* cfg, const Switches& sw,
                        int g_chains, DataPlan& dp, fitoct_plan** out) {
  if (!out) return fail(FITOCT_E_ARG, "out is NULL");
  *out = nullptr;
  FITOCT_TRY(check_config(cfg));
  // released on every early return or exception until handed to the caller
  std::unique_ptr<fitoct_plan> guard(new fitoct_plan());
  fitoct_plan* pl = guard.get();
  FITOCT_TRY(plan_common(pl, prob, dp, cfg->chains, cfg->device));
  pl->cfg = *cfg;
  pl->sw = sw;
  KParams& k = pl->kp;
  // (a batch plans every problem's tiles from the batch's total chain count, and pairs its
  // tiles itself: fitoct_batch_create)
  int rc = FITOCT_OK;
  pl->sched = choose_schedule(pl->ppl, k.mode, cfg->chains, g_chains, pl->ncu, cfg->max_treedepth,
                              sw, &rc);
  if (rc) return rc;
  const Schedule& sc = pl->sched;
  k.G = sc.G;
  k.spec_live = sc.spec_live;
  k.spec = sc.spec;
  k.bidi = sc.bidi;
  k.tail_bidi = sc.tail_bidi;
  k.tail_left = sc.tail_left;
  k.tail_idle_ticks = sc.tail_idle_ticks;
  const int C = cfg->chains, D = k.D;
  k.chain_offset = cfg->chain_offset;
  k.warmup = cfg->warmup;
  k.samples = cfg->samples;
  k.max_depth = cfg->max_treedepth;
  k.save_warmup = cfg->save_warmup ? 1 : 0;
  k.adapt = cfg->adapt_engaged ? 1 : 0;
  k.seed = cfg->seed;
  k.adapt_delta = cfg->adapt_delta;
  k.gamma = cfg->gamma > 0 ? cfg->gamma : 0.05;
  k.kappa = cfg->kappa > 0 ? cfg->kappa : 0.75;
  k.t0 = cfg->t0 > 0 ? cfg->t0 : 10.0;
  k.stepsize0 = cfg->stepsize;
  k.init_radius = cfg->init_radius;
  k.init_buffer = cfg->init_buffer;
  k.term_buffer = cfg->term_buffer;
  k.base_window = cfg->window;
  const long long iters = (long long)cfg->warmup + cfg->samples;
  k.max_steps = iters * ((1LL << cfg->max_treedepth) + 1) + 4000LL * (cfg->warmup / 10 + 4) + 10000;
  k.iters_saved = cfg->save_warmup ? (int)iters : cfg->samples;
  k.ncols = D + 8;
  pl->draws_bytes = sizeof(double) * (size_t)C * k.iters_saved * k.ncols;
  const int vlen = WAVE * pl->ppl;
  // proposal pools: the chains', then the two-ended producers' (GMAX per tile; produce)
  const size_t pools = (size_t)C + (size_t)GMAX * sc.tiles;
  FITOCT_TRY(pl->d_stack.alloc(sizeof(double) * pools * (cfg->max_treedepth + 1) * POOL_VECS * vlen));
  FITOCT_TRY(pl->d_fin.alloc(sizeof(double) * (size_t)C * (1 + 2 * D)));
  FITOCT_TRY(pl->d_status.alloc(sizeof(int) * C));
  // [chains] leapfrogs per chain, then the launch's two-ended and paired transition counts
  FITOCT_TRY(pl->d_leap.alloc(sizeof(long long) * (C + 2)));
  FITOCT_TRY(pl->ev0.create());
  FITOCT_TRY(pl->ev1.create());
  k.stack = pl->d_stack.as<double>();
  k.fin_eps = pl->d_fin.as<double>();
  k.fin_minv = k.fin_eps + C;
  k.fin_q = k.fin_eps + C + (size_t)C * D;
  k.chain_status = pl->d_status.as<int>();
  k.leapfrogs = pl->d_leap.as<long long>();
  k.bidi_count = (unsigned long long*)(k.leapfrogs + C);
  k.pair_count = (unsigned long long*)(k.leapfrogs + C + 1);
  if (g_chains == 0) {   // progress / cancellation (fitoct_plan_poll / _cancel); batch: off
    const unsigned flags = hipHostMallocMapped | hipHostMallocCoherent;
    FITOCT_TRY(pl->h_prog.alloc(sizeof(int) * C, flags));
    FITOCT_TRY(pl->h_cancel.alloc(sizeof(int), flags));
    memset(pl->h_prog.p, 0, sizeof(int) * C);
    *pl->h_cancel.as<int>() = 0;
    int *dp_ = nullptr, *dc = nullptr;
    HIP_TRY(hipHostGetDevicePointer((void**)&dp_, pl->h_prog.p, 0));
    HIP_TRY(hipHostGetDevicePointer((void**)&dc, pl->h_cancel.p, 0));
    k.progress = dp_;
    k.cancel = dc;
  }
  if (sc.migrate) {   // the migration control block and the chain images in flight
    const int T = sc.tiles, words = mig_img_words(pl->ppl);
    pl->mig_bytes = sizeof(int) * (MIG_HDR + 2 * (size_t)T + (size_t)T * GMAX);
    FITOCT_TRY(pl->d_mig.alloc(pl->mig_bytes));
    FITOCT_TRY(pl->d_mig_img.alloc(sizeof(double) * (size_t)T * GMAX * words));
    k.mig = pl->d_mig.as<int>();
    k.mig_img = pl->d_mig_img.as<double>();
    k.mig_tiles = T;
    k.mig_img_words = words;
  }
  if (sc.pair) {
    FITOCT_TRY(pl->pairs.alloc(sc.tiles, pl->ppl, sw));
    pl->pairs.apply(k);
  }
  *out = guard.release();
  return FITOCT_OK;
}

extern "C" {

int32_t fitoct_plan_get_info(const fitoct_plan* pl, fitoct_plan_info* info) {
  return guarded(__func__, [&]() -> int32_t {
    if (!pl || !info) return fail(FITOCT_E_ARG, "NULL argument");
    if (!pl->shards.empty()) return group_plan_info(pl, info);
    info->dim = pl->kp.D;
    info->n_cols = pl->kp.ncols;
    info->iters_saved = pl->kp.iters_saved;
    info->chains = pl->kp.chains;
    const Schedule& sc = pl->sched;
    info->tiles = sc.tiles;
    info->chains_per_tile = sc.G;
    info->sampler = sc.sampler;
    info->n_devices = 1;
    info->bins_per_thread = pl->bpt;
    info->threads_per_tile = TPB;
    info->lds_bytes = sc.lds;
    info->n_pad = pl->kp.n_pad;
    info->draws_bytes = (int64_t)pl->draws_bytes;
    info->two_ended = sc.bidi ? 1 : sc.tail_bidi ? 2 : 0;
    info->ring_records = info->two_ended ? 1 : 0;   // (ABI 7: one subtree record per end)
    info->ring_records_in_levels = 0;
    info->paired = sc.pair ? 1 : 0;
    info->workgroups = sc.grid;
    info->basis_mode = pl->kp.mode;
    return FITOCT_OK;
  });
}

int32_t fitoct_plan_set_init(fitoct_plan* pl, const double* q_init, const double* stepsize,
                             const double* inv_metric) {
  return guarded(__func__, [&]() -> int32_t {
    if (!pl) return fail(FITOCT_E_ARG, "plan is NULL");
    if (!pl->shards.empty()) return group_plan_set_init(pl, q_init, stepsize, inv_metric);
    if (pl->launched) return fail(FITOCT_E_ARG, "plan is running: call fitoct_plan_wait first");
    const int C = pl->kp.chains, D = pl->kp.D;
    // checked on the host: the kernel takes every value as given
    const int ck = check_init(C, D, q_init, stepsize, inv_metric);
    if (ck) return ck;
    HIP_TRY(hipSetDevice(pl->cfg.device));
    if ((q_init || stepsize || inv_metric) && !pl->d_init.p)
      FITOCT_TRY(pl->d_init.alloc(sizeof(double) * (size_t)C * (1 + 2 * D)));
    double* d_eps = pl->d_init.as<double>();
    double* d_minv = d_eps ? d_eps + C : nullptr;
    double* d_q = d_eps ? d_eps + C + (size_t)C * D : nullptr;
    if (stepsize) HIP_TRY(hipMemcpy(d_eps, stepsize, sizeof(double) * C, hipMemcpyHostToDevice));
    if (inv_metric)
      HIP_TRY(hipMemcpy(d_minv, inv_metric, sizeof(double) * C * D, hipMemcpyHostToDevice));
    if (q_init) HIP_TRY(hipMemcpy(d_q, q_init, sizeof(double) * C * D, hipMemcpyHostToDevice));
    pl->kp.init_eps = stepsize ? d_eps : nullptr;
    pl->kp.init_minv = inv_metric ? d_minv : nullptr;
    pl->kp.init_q = q_init ? d_q : nullptr;
    return FITOCT_OK;
  });
}

int32_t fitoct_plan_launch(fitoct_plan* pl, void* d_draws, void* stream) {
  return guarded(__func__, [&]() -> int32_t {
    if (!pl) return fail(FITOCT_E_ARG, "plan is NULL");
    if (!pl->shards.empty()) return group_plan_launch(pl, d_draws, stream);
    if (pl->launched) return fail(FITOCT_E_ARG, "plan is running: call fitoct_plan_wait first");
    HIP_TRY(hipSetDevice(pl->cfg.device));
    if (pl->h_prog.p) {   // no launch of this plan is in flight: the kernel does not touch them
      memset(pl->h_prog.p, 0, sizeof(int) * pl->kp.chains);
      __atomic_store_n(pl->h_cancel.as<int>(), 0, __ATOMIC_SEQ_CST);
    }
    double* dst = (double*)d_draws;
    if (!dst) {
      if (!pl->d_draws.p) FITOCT_TRY(pl->d_draws.alloc(pl->draws_bytes));
      dst = pl->d_draws.as<double>();
    }
    hipStream_t st = (hipStream_t)stream;
    KParams k = pl->kp;
    k.draws = dst;
    HIP_TRY(hipMemsetAsync(pl->d_status.p, 0, sizeof(int) * k.chains, st));
    HIP_TRY(hipMemsetAsync(k.bidi_count, 0, 2 * sizeof(long long), st));   // + pair_count
    if (pl->d_mig.p) HIP_TRY(hipMemsetAsync(pl->d_mig.p, 0, pl->mig_bytes, st));
    if (pl->pairs.on()) FITOCT_TRY(pl->pairs.zero(st));
    if (stamps_requested(&k.bench_sweeps)) {   // diagnostic only
      const size_t bytes = sizeof(long long) * NSTAMP * pl->sched.tiles;
      if (!pl->d_stamps.p) FITOCT_TRY(pl->d_stamps.alloc(bytes));
      HIP_TRY(hipMemsetAsync(pl->d_stamps.p, 0, bytes, st));
      k.stamps = pl->d_stamps.as<long long>();
    }
    HIP_TRY(hipEventRecord(pl->ev0.p, st));
    if (!pl->d_kp.p) FITOCT_TRY(pl->d_kp.alloc(sizeof(KParams)));
    HIP_TRY(hipMemcpyAsync(pl->d_kp.p, &k, sizeof(KParams), hipMemcpyHostToDevice, st));
    HIP_TRY(launch(false, pl->mixed, pl->bpt, pl->nnp, k, pl->d_kp.as<KParams>(), pl->sched.grid,
                   st));
    HIP_TRY(hipEventRecord(pl->ev1.p, st));
    pl->last_draws = dst;
    pl->launched = true;
    pl->ran = false;
    return FITOCT_OK;
  });
}

int32_t fitoct_plan_poll(fitoct_plan* pl, int64_t* iterations_done, int64_t* iterations_total,
                         int32_t* finished) {
  return guarded(__func__, [&]() -> int32_t {
    if (!pl) return fail(FITOCT_E_ARG, "plan is NULL");
    if (!pl->shards.empty()) return group_plan_poll(pl, iterations_done, iterations_total, finished);
    const int C = pl->kp.chains;
    int64_t done = 0;
    const int* prog = pl->h_prog.as<int>();
    if (prog)
      for (int c = 0; c < C; ++c) done += __atomic_load_n(&prog[c], __ATOMIC_RELAXED);
    const int64_t total = (int64_t)C * (pl->kp.warmup + pl->kp.samples);
    int32_t fin = pl->ran ? 1 : 0;
    if (pl->launched) {
      HIP_TRY(hipSetDevice(pl->cfg.device));
      const hipError_t q = hipEventQuery(pl->ev1.p);
      if (q == hipSuccess) fin = 1;
      else if (q != hipErrorNotReady) HIP_TRY(q);
    }
    if (iterations_done) *iterations_done = (prog || !fin) ? done : total;
    if (iterations_total) *iterations_total = total;
    if (finished) *finished = fin;
    return FITOCT_OK;
  });
}

int32_t fitoct_plan_cancel(fitoct_plan* pl) {
  return guarded(__func__, [&]() -> int32_t {
    if (!pl) return fail(FITOCT_E_ARG, "plan is NULL");
    if (!pl->shards.empty()) return group_plan_cancel(pl);
    if (!pl->h_cancel.p) return fail(FITOCT_E_ARG, "this plan has no cancellation flag (batch plan)");
    __atomic_store_n(pl->h_cancel.as<int>(), 1, __ATOMIC_SEQ_CST);
    return FITOCT_OK;
  });
}

int32_t fitoct_plan_wait(fitoct_plan* pl) {
  return guarded(__func__, [&]() -> int32_t {
    if (!pl) return fail(FITOCT_E_ARG, "plan is NULL");
    if (!pl->shards.empty()) return group_plan_wait(pl);
    if (!pl->launched) return pl->ran ? FITOCT_OK : fail(FITOCT_E_ARG, "plan has not been launched");
    HIP_TRY(hipSetDevice(pl->cfg.device));
    pl->launched = false;
    HIP_TRY(hipEventSynchronize(pl->ev1.p));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, pl->ev0.p, pl->ev1.p));
    pl->kernel_ms = ms;
    if (pl->d_stamps.p && stamps_requested(nullptr)) {
      std::vector<long long> h((size_t)NSTAMP * pl->sched.tiles);
      HIP_TRY(hipMemcpy(h.data(), pl->d_stamps.p, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
      report_stamps(h.data(), pl->sched.tiles, pl->sched.bidi != 0);
    }
    pl->ran = true;
    return FITOCT_OK;
  });
}

int32_t fitoct_plan_run(fitoct_plan* pl, void* d_draws, void* stream) {
  return guarded(__func__, [&]() -> int32_t {
    const int32_t rc = fitoct_plan_launch(pl, d_draws, stream);
    return rc ? rc : fitoct_plan_wait(pl);
  });
}


int32_t fitoct_plan_download(fitoct_plan* pl, fitoct_result* res) {
  return guarded(__func__, [&]() -> int32_t {
    if (!pl || !res) return fail(FITOCT_E_ARG, "NULL argument");
    if (!pl->shards.empty()) return group_plan_download(pl, res);
    if (!pl->ran) return fail(FITOCT_E_ARG, "plan has not run");
    HIP_TRY(hipSetDevice(pl->cfg.device));
    const KParams& k = pl->kp;
    const int C = k.chains, D = k.D;
    res->n_cols = k.ncols;
    res->iters_saved = k.iters_saved;
    res->dim = D;
    res->kernel_ms = pl->kernel_ms;
    res->migrations = 0;
    if (pl->d_mig.p) HIP_TRY(hipMemcpy(&res->migrations, pl->d_mig.as<int>() + MIG_MOVES, sizeof(int),
                                       hipMemcpyDeviceToHost));
    if (res->draws) {
      const int64_t need = (int64_t)C * k.iters_saved * k.ncols;
      if (res->draws_capacity < need) return fail(FITOCT_E_ARG, "draws buffer too small");
      HIP_TRY(hipMemcpy(res->draws, pl->last_draws, pl->draws_bytes, hipMemcpyDeviceToHost));
    }
    if (res->stepsize) HIP_TRY(hipMemcpy(res->stepsize, k.fin_eps, sizeof(double) * C, hipMemcpyDeviceToHost));
    if (res->inv_metric)
      HIP_TRY(hipMemcpy(res->inv_metric, k.fin_minv, sizeof(double) * C * D, hipMemcpyDeviceToHost));
    if (res->last_q) HIP_TRY(hipMemcpy(res->last_q, k.fin_q, sizeof(double) * C * D, hipMemcpyDeviceToHost));
    std::vector<int> st(C);
    HIP_TRY(hipMemcpy(st.data(), k.chain_status, sizeof(int) * C, hipMemcpyDeviceToHost));
    if (res->chain_status) memcpy(res->chain_status, st.data(), sizeof(int) * C);
    const int bad = chain_outcome(C, D, st.data(), res->stepsize, res->inv_metric, res->last_q);
    std::vector<long long> lf(C);
    HIP_TRY(hipMemcpy(lf.data(), k.leapfrogs, sizeof(long long) * C, hipMemcpyDeviceToHost));
    long long tot = 0;
    for (long long v : lf) tot += v;
    res->total_leapfrogs = tot;
    long long nb = 0;
    HIP_TRY(hipMemcpy(&nb, k.bidi_count, sizeof(long long), hipMemcpyDeviceToHost));
    res->two_ended_transitions = nb;
    HIP_TRY(hipMemcpy(&nb, k.pair_count, sizeof(long long), hipMemcpyDeviceToHost));
    res->paired_transitions = nb;
    if (bad >= 0)
      return fail(st[bad], "chain " + std::to_string(k.chain_offset + bad) + " failed with status " +
                               std::to_string(st[bad]));
    return FITOCT_OK;
  });
}

void fitoct_plan_destroy(fitoct_plan* pl) { delete pl; }

int32_t fitoct_expgp_sample(const fitoct_problem* prob, const fitoct_config* cfg,
                            fitoct_result* res) {
  return guarded(__func__, [&]() -> int32_t {
    const auto t0 = std::chrono::steady_clock::now();
    if (cfg && cfg->chains >= 1) {   // several devices: one host thread per device
      std::vector<int> devs;
      const int rd = resolve_devices(cfg, cfg->chains, devs);
      if (rd) return rd;
      if (devs.size() > 1) {
        const int rg = group_sample(prob, cfg, devs, res);
        if (res)
          res->wall_ms = std::chrono::duration<double, std::milli>(
                             std::chrono::steady_clock::now() - t0).count();
        return rg;
      }
    }
    fitoct_plan* pl = nullptr;
    int rc = fitoct_plan_create(prob, cfg, &pl);
    if (rc) return rc;
    rc = fitoct_plan_run(pl, nullptr, nullptr);
    if (!rc && res) rc = fitoct_plan_download(pl, res);
    delete pl;
    if (res)
      res->wall_ms =
          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
  });
}

int32_t fitoct_split_rhat_ess(const double* x, int32_t chains, int32_t n, double* rhat,
                              double* ess) {
  return guarded(__func__, [&]() -> int32_t {
    if (!x) return fail(FITOCT_E_ARG, "x is NULL");
    return split_rhat_ess(x, chains, n, rhat, ess);
  });
}

int32_t fitoct_rank_rhat(const double* x, int32_t chains, int32_t n, double* rhat) {
  return guarded(__func__, [&]() -> int32_t {
    if (!x || !rhat) return fail(FITOCT_E_ARG, "NULL argument");
    return rank_rhat(x, chains, n, rhat);
  });
}

}  // extern "C"
