// Plan and batch objects behind the opaque handles of include/fitoct.h, with the small owning
// types their members are made of, shared by the single-device entry points (fitoct_api.cpp),
// batch mode (batch.cpp), the multi-device layer (multi_device.cpp) and the posterior tables.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "fitoct.h"
#include "host_internal.h"
#include "kernel_params.h"
#include "plan_data.h"
#include "schedule.h"

// a failed HIP call ends the enclosing function with FITOCT_E_HIP and its message
#define HIP_TRY(expr)                                                                 \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fitoct::fail(FITOCT_E_HIP,                                               \
                          std::string(#expr) + ": " + hipGetErrorString(e_));         \
  } while (0)

namespace fitoct {
// ---- owners: each releases what it created, cannot be copied and decides nothing ----
template <class T, hipError_t (*Release)(T)>
struct Owned {
  T p = nullptr;
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() {
    if (p) (void)Release(p);
  }
  template <class U>
  U* as() const {
    return (U*)p;
  }
};
struct DevBuf : Owned<void*, hipFree> {   // device memory
  int alloc(size_t bytes) {
    HIP_TRY(hipMalloc(&p, bytes ? bytes : 8));
    return FITOCT_OK;
  }
};
struct PinnedBuf : Owned<void*, hipHostFree> {   // host-pinned memory
  int alloc(size_t bytes, unsigned flags) {
    HIP_TRY(hipHostMalloc(&p, bytes, flags));
    return FITOCT_OK;
  }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
  int create(unsigned flags = hipEventDefault) {
    HIP_TRY(hipEventCreateWithFlags(&p, flags));
    return FITOCT_OK;
  }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
  int create(unsigned flags) {
    HIP_TRY(hipStreamCreateWithFlags(&p, flags));
    return FITOCT_OK;
  }
};
// The calling thread's HIP device is put back when the call returns (the entry points switch
// it; a caller such as PyTorch keeps its own notion of the current device).
struct DeviceKeep {
  int dev = -1;
  DeviceKeep() {
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  }
  ~DeviceKeep() {
    if (dev >= 0) (void)hipSetDevice(dev);
  }
};

#define FITOCT_TRY(expr)          \
  do {                            \
    const int rc_ = (expr);       \
    if (rc_) return rc_;          \
  } while (0)

// Paired tiles (KParams::pair_*): the pairs' hand-off words and buffers of one launch,
// owned by the plan (fitoct_api.cpp) or, over every problem's tiles, by the batch (batch.cpp)
struct PairBuffers {
  DevBuf hdr;   // int [tiles][PAIR_HDR_INTS] hand-off words, zeroed per launch
  DevBuf buf;   // double [tiles][stride] starts and subtree records
  int tiles = 0, stride = 0, test_absent = 0;
  bool on() const { return hdr.p != nullptr; }
  int alloc(int tiles, int ppl, const Switches& sw);
  void apply(KParams& k) const;      // every pair_* field of a launch's parameter block
  int zero(hipStream_t st) const;    // every word the pairs poll: before every launch
};
}  // namespace fitoct

struct fitoct_plan {
  fitoct_problem prob{};
  fitoct_config cfg{};
  fitoct::KParams kp{};      // (its pointers name the buffers below: none of them owns)
  fitoct::Switches sw{};     // the planner's environment switches at fitoct_plan_create
  fitoct::Schedule sched{};  // the launch schedule (schedule.cpp); a multi-device plan: tiles only
  int bpt = 0, nnp = 15, ppl = 1, ncu = 0;
  bool mixed = false;
  fitoct::DevBuf d_mig;       // int: chain-migration control block (see MigCtrl)
  fitoct::DevBuf d_mig_img;
  size_t mig_bytes = 0;
  size_t draws_bytes = 0;
  fitoct::DevBuf d_data;      // cx | y | isu | B  (type R), then K^-1 | b
  fitoct::DevBuf d_draws;     // double: internal draws buffer (lazily allocated)
  fitoct::DevBuf d_stack;
  fitoct::DevBuf d_fin;       // double: eps[C] | minv[C*D] | q[C*D]
  fitoct::DevBuf d_init;      // warm restart (fitoct_plan_set_init, lazy): eps[C] | minv[C*D] | q[C*D]
  fitoct::DevBuf d_status;    // int [chains]
  fitoct::DevBuf d_leap;      // long long [chains + 2]
  fitoct::DevBuf d_kp;        // KParams: device copy of the launch parameters (lazy)
  double* last_draws = nullptr;   // not owned: where the last launch wrote (d_draws or the caller's)
  double kernel_ms = 0.0;
  fitoct::Event ev0, ev1;
  bool ran = false;
  bool launched = false;      // fitoct_plan_launch issued, fitoct_plan_wait not yet
  fitoct::PinnedBuf h_prog;   // int [chains]: transitions done (kernel-written)
  fitoct::PinnedBuf h_cancel; // int: flag polled by the kernel
  fitoct::DevBuf d_stamps;    // long long: diagnostic stamps of the launch in flight (lazy)
  fitoct::PairBuffers pairs;  // paired tiles (sched.pair)
  // the plan's own host copies of x | y | uy and of the basis rows [N][Nn] (empty for the
  // mono-exponential model): what the posterior curves read of the problem (curves_device.hip)
  std::vector<double> h_xyu, h_B;

  // ---- multi-device plan (cfg.n_devices > 1; multi_device.cpp) ----
  // One single-device plan per device; shard r runs this plan's chains
  // [shard_off[r], shard_off[r] + shards[r]->kp.chains).  A multi-device plan holds no
  // device memory of its own: every entry point forwards to its shards.
  std::vector<fitoct_plan*> shards;   // owned
  std::vector<int> shard_off;
  void* gather_dst = nullptr;  // not owned: caller's d_draws of the launch in flight (or NULL)
  int gather_dev = -1;         // device holding gather_dst
  // a shard's own non-blocking stream (lazy): shards never wait on one another (nor on the
  // synchronous status reads and peer copies of other shards) through a default stream
  fitoct::Stream own_stream;

  ~fitoct_plan() {
    for (fitoct_plan* sh : shards) delete sh;
  }
};

struct fitoct_batch {
  std::vector<fitoct_plan*> plans;   // owned
  fitoct_config cfg{};
  int tiles = 0;
  size_t per_bytes = 0;       // draws bytes of one problem
  fitoct::DevBuf d_kp;        // KParams [n_problems]
  fitoct::DevBuf d_map;       // int [tiles][2]
  fitoct::DevBuf d_draws;     // internal [n_problems][chains][iters][cols] (lazy)
  double kernel_ms = 0.0;
  fitoct::Event ev0, ev1;
  bool ran = false;
  // host-pinned flag polled by every problem's chains (KParams::cancel): set by the
  // multi-device layer when another device's chain failed; cleared by each run
  fitoct::PinnedBuf h_cancel;
  int* d_cancel = nullptr;    // not owned: its device alias
  fitoct::Switches sw{};      // the planner's environment switches at fitoct_batch_create
  fitoct::PairBuffers pairs;  // paired tiles over the whole batch (every problem's KParams::pair_*)
  // blocks of the launch: the tiles, or with paired tiles a primary and a partner each
  int grid() const { return pairs.on() ? fitoct::pair_grid(tiles) : tiles; }

  // ---- multi-device batch: problems [sub_off[r], sub_off[r] + subs[r]->plans.size())
  // on sub-batch r, one device each (multi_device.cpp) ----
  std::vector<fitoct_batch*> subs;   // owned
  std::vector<int> sub_off;
  int n_problems = 0;
  fitoct::Stream own_stream;   // a sub-batch's own non-blocking stream (lazy)
  void* gather_dst = nullptr;  // not owned: caller's d_draws of the last multi-device run (or NULL)
  int gather_dev = -1;         // device holding gather_dst

  ~fitoct_batch() {
    for (fitoct_batch* sb : subs) delete sb;
    for (fitoct_plan* pl : plans) delete pl;
  }
};

namespace fitoct {

// the device list of a call: ordinals of the first min(n_devices, units) entries of
// cfg->devices (or {cfg->device} when n_devices == 0); FITOCT_E_ARG on a bad list
int resolve_devices(const fitoct_config* cfg, int units, std::vector<int>& devs);
// the device a caller's d_draws buffer lives on (FITOCT_E_ARG if it is not device memory)
int buffer_device(const void* p, int& dev);
// contiguous block partition of `total` units over `n` parts (part r: [off, off + cnt))
void block_range(int total, int n, int r, int& off, int& cnt);

// the sampler and the logp kernel, compiled once per prior family (nuts_device.hip,
// -DFITOCT_FAMILY)
hipError_t launch_family_0(bool logp, bool mixed, int bpt, int nnp, const KParams& P,
                           const KParams* dP, int tiles, hipStream_t st, const int* tile_map);
hipError_t launch_family_1(bool logp, bool mixed, int bpt, int nnp, const KParams& P,
                           const KParams* dP, int tiles, hipStream_t st, const int* tile_map);
hipError_t launch_family_2(bool logp, bool mixed, int bpt, int nnp, const KParams& P,
                           const KParams* dP, int tiles, hipStream_t st, const int* tile_map);
hipError_t launch_family_3(bool logp, bool mixed, int bpt, int nnp, const KParams& P,
                           const KParams* dP, int tiles, hipStream_t st, const int* tile_map);
inline hipError_t launch(bool logp, bool mixed, int bpt, int nnp, const KParams& P,
                         const KParams* dP, int tiles, hipStream_t st,
                         const int* tile_map = nullptr) {
  switch (P.family) {
    case 0: return launch_family_0(logp, mixed, bpt, nnp, P, dP, tiles, st, tile_map);
    case 1: return launch_family_1(logp, mixed, bpt, nnp, P, dP, tiles, st, tile_map);
    case 2: return launch_family_2(logp, mixed, bpt, nnp, P, dP, tiles, st, tile_map);
    case 3: return launch_family_3(logp, mixed, bpt, nnp, P, dP, tiles, st, tile_map);
    default: return hipErrorInvalidValue;
  }
}

// the sampler settings of a config, checked before anything is planned (fitoct_api.cpp)
int check_config(const fitoct_config* cfg);
// A single-device plan of a problem whose data plan is `dp` (consumed): the device, the upload,
// the launch schedule and what it asks for.  g_chains: the chain total of the batch the plan
// belongs to (0: a plan of its own).  On failure everything is released and *out stays NULL.
int plan_create(const fitoct_problem* prob, const fitoct_config* cfg, const Switches& sw,
                int g_chains, DataPlan& dp, fitoct_plan** out);

// multi-device forms of the plan / batch entry points (multi_device.cpp)
int group_plan_create(const fitoct_problem* prob, const fitoct_config* cfg,
                      const std::vector<int>& devs, fitoct_plan** out);
int group_plan_info(const fitoct_plan* pl, fitoct_plan_info* info);
int group_plan_set_init(fitoct_plan* pl, const double* q, const double* eps, const double* minv);
int group_plan_launch(fitoct_plan* pl, void* d_draws, void* stream);
int group_plan_poll(fitoct_plan* pl, int64_t* done, int64_t* total, int32_t* finished);
int group_plan_cancel(fitoct_plan* pl);
int group_plan_wait(fitoct_plan* pl);
int group_plan_download(fitoct_plan* pl, fitoct_result* res);
int group_sample(const fitoct_problem* prob, const fitoct_config* cfg,
                 const std::vector<int>& devs, fitoct_result* res);

int group_batch_create(const fitoct_problem* probs, int n_problems, const fitoct_config* cfg,
                       const std::vector<int>& devs, fitoct_batch** out);
int group_batch_info(const fitoct_batch* b, fitoct_plan_info* info);
int group_batch_run(fitoct_batch* b, void* d_draws, void* stream);
// a single-device batch's run (fitoct_batch_run without clearing the cancel flag)
int batch_run_single(fitoct_batch* b, void* d_draws, void* stream);
// warm-restart inputs of C chains checked on the host (fitoct_plan_set_init's rules)
int check_init(int C, int D, const double* q, const double* eps, const double* minv);
int group_batch_download(fitoct_batch* b, int problem, fitoct_result* res);

// ---- where the last run's draws lie (posterior_common.hip) ----
// What a plan's or a batch's last run left, as the arguments of a *_device entry of the
// posterior summary, the rank diagnostics or the posterior curves.  The problems carry the
// plans' own copies of x, y, uy and the basis (with_data): the curves read them; the summary and
// the rank diagnostics read prior_type, Nn, prior_PD and lambda_scale only (check_args), so one
// form serves all three.
struct Where {
  std::vector<fitoct_problem> probs;
  int chains = 0, iters_saved = 0, device = 0;
  const char* draws = nullptr;
  size_t group_bytes = 0;   // a batch: raw bytes of one problem's draws
};
// a plan's problem with the plan's own copies of x, y, uy and the basis behind it
fitoct_problem with_data(const fitoct_plan* pl);
// The refusals: a plan in flight, a plan or batch that has not run, a device-list run that left
// its parts in per-device buffers (`needs` names the caller in that message: "the summary needs",
// "the diagnostics need", "the curves need").
int plan_where(fitoct_plan* pl, const char* needs, Where& w);
int batch_where(fitoct_batch* b, const char* needs, Where& w);

}  // namespace fitoct
