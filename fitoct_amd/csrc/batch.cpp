// Batch mode: many problems (FitOCT.R's per-file fitExpGP calls, FitOCT.R:70-124)
// sampled by ONE persistent launch.  Each problem keeps its own staged data,
// basis factors, pool and outputs (a fitoct_plan each); the kernel receives the
// array of their parameter blocks and a tile map {problem, first chain}, so a
// tile only ever holds one problem's chains.  Chain c of problem p is keyed as
// global chain cfg.chain_offset + p*chains + c: its draws are those of a single
// plan of that problem with chain_offset = cfg.chain_offset + p*chains.
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "fitoct.h"
#include "host_internal.h"
#include "kernel_params.h"
#include "plan_internal.h"

using namespace fitoct;

extern "C" {

int32_t fitoct_batch_create(const fitoct_problem* probs, int32_t n_problems,
                            const fitoct_config* cfg, fitoct_batch** out) {
  return guarded(__func__, [&]() -> int32_t {
    if (!out) return fail(FITOCT_E_ARG, "out is NULL");
    *out = nullptr;
    if (!probs || n_problems < 1) return fail(FITOCT_E_ARG, "need n_problems >= 1 problems");
    if (!cfg) return fail(FITOCT_E_ARG, "config is NULL");
    if (cfg->chains < 1) return fail(FITOCT_E_ARG, "chains must be >= 1");
    if ((int64_t)n_problems * cfg->chains > (int64_t)1 << 30)
      return fail(FITOCT_E_ARG, "too many chains in one batch");
    std::vector<int> devs;
    FITOCT_TRY(resolve_devices(cfg, n_problems, devs));
    if (devs.size() > 1) return group_batch_create(probs, n_problems, cfg, devs, out);
    std::unique_ptr<fitoct_batch> guard(new fitoct_batch());
    fitoct_batch* b = guard.get();
    b->cfg = *cfg;
    b->cfg.device = devs[0];
    b->cfg.n_devices = 0;
    b->n_problems = n_problems;
    b->sw = Switches::from_env();
    const int C = cfg->chains;
    if (check_config(cfg)) return fail(FITOCT_E_ARG, "problem 0: " + g_last_error);
    // every problem is planned on the host, at the batch's common bin layout, before anything
    // is allocated: one kernel instantiation and one LDS carve serve every problem
    std::vector<DataPlan> data;
    FITOCT_TRY(plan_batch_data(probs, n_problems, cfg->precision, b->sw, data));
    for (int p = 0; p < n_problems; ++p) {
      fitoct_config c = b->cfg;
      c.chain_offset = cfg->chain_offset + p * C;
      fitoct_plan* pl = nullptr;
      const int rc = plan_create(&probs[p], &c, b->sw, n_problems * C, data[p], &pl);
      if (rc) return fail(rc, "problem " + std::to_string(p) + ": " + g_last_error);
      b->plans.push_back(pl);
    }
    b->per_bytes = b->plans[0]->draws_bytes;
    std::vector<int> map;
    const int G = b->plans[0]->kp.G;
    for (int p = 0; p < n_problems; ++p)
      for (int c0 = 0; c0 < C; c0 += G) {
        map.push_back(p);
        map.push_back(c0);
      }
    b->tiles = (int)map.size() / 2;
    HIP_TRY(hipSetDevice(b->cfg.device));
    FITOCT_TRY(b->d_map.alloc(sizeof(int) * map.size()));
    HIP_TRY(hipMemcpy(b->d_map.p, map.data(), sizeof(int) * map.size(), hipMemcpyHostToDevice));
    FITOCT_TRY(b->d_kp.alloc(sizeof(KParams) * n_problems));
    // paired tiles over the whole batch (one-chain tiles: config 5's 4- and 8-GPU shares)
    const fitoct_plan* q0 = b->plans[0];
    if (want_pairs(q0->sched, q0->kp.mode, b->tiles, q0->ncu, b->sw))
      FITOCT_TRY(b->pairs.alloc(b->tiles, q0->ppl, b->sw));
    // cancellation flag (set by the multi-device layer when another device fails)
    FITOCT_TRY(b->h_cancel.alloc(sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
    *b->h_cancel.as<int>() = 0;
    HIP_TRY(hipHostGetDevicePointer((void**)&b->d_cancel, b->h_cancel.p, 0));
    FITOCT_TRY(b->ev0.create());
    FITOCT_TRY(b->ev1.create());
    *out = guard.release();
    return FITOCT_OK;
  });
}

int32_t fitoct_batch_get_info(const fitoct_batch* b, fitoct_plan_info* info) {
  return guarded(__func__, [&]() -> int32_t {
    if (!b || !info) return fail(FITOCT_E_ARG, "NULL argument");
    if (!b->subs.empty()) return group_batch_info(b, info);
    const int rc = fitoct_plan_get_info(b->plans[0], info);
    if (rc) return rc;
    info->chains = b->cfg.chains * (int)b->plans.size();
    info->tiles = b->tiles;
    info->paired = b->pairs.on() ? 1 : 0;
    info->workgroups = b->grid();
    info->basis_mode = b->plans.empty() ? 0 : b->plans[0]->kp.mode;
    info->draws_bytes = (int64_t)(b->per_bytes * b->plans.size());
    return FITOCT_OK;
  });
}

}  // extern "C"

int fitoct::batch_run_single(fitoct_batch* b, void* d_draws, void* stream) {
  HIP_TRY(hipSetDevice(b->cfg.device));
  const size_t P = b->plans.size();
  double* dst = (double*)d_draws;
  if (!dst) {
    if (!b->d_draws.p) FITOCT_TRY(b->d_draws.alloc(b->per_bytes * P));
    dst = b->d_draws.as<double>();
  }
  hipStream_t st = (hipStream_t)stream;
  std::vector<KParams> kp(P);
  for (size_t p = 0; p < P; ++p) {
    fitoct_plan* pl = b->plans[p];
    kp[p] = pl->kp;
    kp[p].draws = (double*)((char*)dst + b->per_bytes * p);
    kp[p].cancel = b->d_cancel;
    pl->last_draws = kp[p].draws;
    HIP_TRY(hipMemsetAsync(pl->d_status.p, 0, sizeof(int) * pl->kp.chains, st));
    HIP_TRY(hipMemsetAsync(pl->kp.bidi_count, 0, 2 * sizeof(long long), st));   // + pair_count
    // paired tiles: every problem's block names the batch's pairs
    if (b->pairs.on()) b->pairs.apply(kp[p]);
  }
  if (b->pairs.on()) FITOCT_TRY(b->pairs.zero(st));
  HIP_TRY(hipMemcpyAsync(b->d_kp.p, kp.data(), sizeof(KParams) * P, hipMemcpyHostToDevice, st));
  const fitoct_plan* p0 = b->plans[0];
  HIP_TRY(hipEventRecord(b->ev0.p, st));
  HIP_TRY(launch(false, p0->mixed, p0->bpt, p0->nnp, kp[0], b->d_kp.as<KParams>(), b->grid(), st,
                 b->d_map.as<int>()));
  HIP_TRY(hipEventRecord(b->ev1.p, st));
  HIP_TRY(hipEventSynchronize(b->ev1.p));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, b->ev0.p, b->ev1.p));
  b->kernel_ms = ms;
  for (fitoct_plan* pl : b->plans) {
    pl->kernel_ms = ms;
    pl->ran = true;
  }
  b->ran = true;
  return FITOCT_OK;
}

extern "C" {

int32_t fitoct_batch_run(fitoct_batch* b, void* d_draws, void* stream) {
  return guarded(__func__, [&]() -> int32_t {
    if (!b) return fail(FITOCT_E_ARG, "batch is NULL");
    if (!b->subs.empty()) return group_batch_run(b, d_draws, stream);
    if (b->h_cancel.p) __atomic_store_n(b->h_cancel.as<int>(), 0, __ATOMIC_SEQ_CST);
    return batch_run_single(b, d_draws, stream);
  });
}

int32_t fitoct_batch_download(fitoct_batch* b, int32_t problem, fitoct_result* res) {
  return guarded(__func__, [&]() -> int32_t {
    if (!b) return fail(FITOCT_E_ARG, "batch is NULL");
    if (problem < 0 || problem >= b->n_problems)
      return fail(FITOCT_E_ARG, "problem index out of range");
    if (!b->subs.empty()) return group_batch_download(b, problem, res);
    if (!b->ran) return fail(FITOCT_E_ARG, "batch has not run");
    return fitoct_plan_download(b->plans[problem], res);
  });
}

void fitoct_batch_destroy(fitoct_batch* b) { delete b; }

}  // extern "C"
