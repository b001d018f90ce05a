// Device-resident NUTS for the FitOCT ExpGP posterior (gfx950 / MI355X).
//
// Replaces rstan::sampling + Stan's base_nuts / adapt_diag_e_nuts + the
// stanc-generated model with stan-math AD.
//
// Execution model ("tile" = one 512-thread workgroup of 8 waves, persistent for the
// whole run; kernel_params.h NW / NGW / GMAX):
//   * a tile owns G <= 4 chains.  Each chain is an explicit state machine (init
//     -> step-size search -> tree building -> adaptation -> next transition)
//     that consumes one gradient per leapfrog, so a chain that finishes its
//     trajectory starts its next transition at once: no chain waits for
//     another chain's tree.
//   * the 8 waves are specialised: waves 0..3 only run the likelihood sweep,
//     waves 4..7 only run NUTS (one chain each); waves w and w+4 share SIMD
//     w mod 4, so every SIMD holds one gradient wave and one NUTS wave.  The
//     roles meet in a dataflow pipeline through LDS: a NUTS wave enqueues its
//     chain's next position in a ring, the gradient waves drain the ring in
//     order and count their completions per chain, the NUTS wave resumes when
//     all 4 sweeps are in.  No barrier after start-up: each chain's sampler
//     latency hides behind the sweeps of the tile's other chains.
//   * gradient waves: the likelihood sweep over the lanes' resident bins (sweep_math.h,
//     gradient_pass.h).
//   * NUTS phase (wave 4+c drives chain c): lane k holds parameter k.  The wave sums the 4
//     partials, completes lp / grad with the priors and the log-Jacobians, and advances
//     the chain's state machine, Stan's recursive build_tree replayed one leaf per step
//     (chain.h: the action machine, the tree's records in LDS, the proposals' HBM pool).
//     Wave reductions are DPP/permlane butterflies (wave_math.h).
//   * workgroups communicate only to hand whole chains between tiles at transition
//     boundaries (chain migration, the MIG instantiation; the donor's side
//     in chain.h, the receiver's in tile_migrate.h).
//   * a tile of one chain (fewer chains than CUs) puts its three spare NUTS waves to work:
//     two producers leapfrog the trajectory's backward and forward ends at once and a
//     helper books the leaves in Stan's tree order (chain.h "two-ended trajectories";
//     the waves' roles and the paired tiles' bridge in nuts_kernel.h).
//
// Every layer has a header, included below in dependency order (DESIGN.md §4 has the map),
// and each opens with a description of its layer: dev_common.h, dev_global.h, wave_math.h;
// sweep_math.h, lds_layout.h, gradient_pass.h (the sweep's arithmetic, under its own
// contraction pragma); chain.h, tile_migrate.h, nuts_kernel.h.  This file keeps what is
// per translation unit: the order of the layers with the two pragmas, the log-density
// kernel, the family's instantiations and the launchers.  namespace fitoct opens in
// dev_common.h and closes at the end of this file.
//
// Random numbers are addressable Philox draws (philox.h), identical to the CPU
// oracle's, so short horizons of GPU and CPU chains coincide draw for draw.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "kernel_params.h"
#include "philox.h"

#include "dev_common.h"
#include "dev_global.h"
#include "wave_math.h"

// The sweep's arithmetic is contracted only where the source writes a * b + c as one
// expression (or calls fma): HIP's default, fast contraction across statements, let the
// backend fuse the same sweep differently in two kernel instantiations (the migrating and
// the plain sampler at 4 bins per lane, round 5), which broke the bitwise equality of
// their draws.  1 + a P(t) is written as an FMA (measured: hand-fusing the four per-bin sums
// as well costs config 5 7 %, scripts/gpu_r5_variants.sh); config 5 runs 1.7 % below the
// fast contraction, config 3 0.5 % (profiles/r05_ab_contract.txt).
#pragma clang fp contract(on)
#include "sweep_math.h"
#include "lds_layout.h"
#include "gradient_pass.h"

// (end of the sweep's arithmetic: the sampler's code below keeps HIP's default contraction)
#pragma clang fp contract(fast)
#include "chain.h"
#include "tile_migrate.h"
#include "nuts_kernel.h"
// One log density and gradient per chain at given positions (fitoct_logp_grad): the
// sampler's own start-up load, write_mp, sweep and finish_grad, once, with barriers between.
template <class R, int BPT, int NNP, int PPL, int MODE, int FAM>
__global__ void __launch_bounds__(TPB, 2) logp_kernel(const KParams* __restrict__ Pg) {
  KPc& P = *(KPc*)Pg;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lds<PPL> L{(AS_LDS char*)smem, P.G, Lds<PPL>::chain_bytes(P.max_depth)};
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = blockIdx.x * P.G;
  const int nct = min(P.G, P.chains - c0);
  __shared__ int done[GMAX];
  load_kinv<PPL, NNP, FAM>(P, L, tid);
  if (tid < GMAX) done[tid] = tid >= nct;
  __syncthreads();
  const int c = wave - NGW;
  if (wave >= NGW && c < nct) {
    Chain<PPL, NNP, FAM> ch(P, L, c, c0 + c, lane, nct);
    Vd<PPL> q;
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      const int k = s * WAVE + lane;
      q.a[s] = (k < P.D) ? ((const AS_GLB double*)P.q_in)[(size_t)(c0 + c) * P.D + k] : 0.0;
    }
    if (lane < NSLOT) ch.SUMS[lane] = 0.0;
    ch.write_mp(q);
    wave_fence();
  }
  __syncthreads();
  if (wave < NGW && P.prior_PD == 0) {
    Bins<R, BPT, NNP, MODE> bins;
    bins.load(P, tid);
    gradient_pass<R, BPT, NNP, MODE, true>(P, bins, L.mp(0), L.part(), done, 0, nct, tid, lane,
                                           wave);
  }
  __syncthreads();
  if (wave >= NGW && c < nct) {
    Chain<PPL, NNP, FAM> ch(P, L, c, c0 + c, lane, nct);
    ch.prior_part();
    wave_fence();
    Vd<PPL> g;
    double s0;
    const double lp = ch.finish_grad(g, s0);
    const size_t pt = (size_t)(c0 + c);
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      const int k = s * WAVE + lane;
      if (k < P.D) ((AS_GLB double*)P.grad_out)[pt * P.D + k] = g.a[s];
    }
    if (lane == 0) {
      ((AS_GLB double*)P.lp_out)[pt] = lp;
      if (P.s2_out) ((AS_GLB double*)P.s2_out)[pt] = s0;
    }
  }
}

// ---------------------------------------------------------------------------
// host-side dispatch over the template grid.  This file is compiled once per
// prior family (-DFITOCT_FAMILY=0/1/2, in parallel); the family is a template
// parameter of the sampler so that no family branch survives in its code.
// ---------------------------------------------------------------------------
#ifndef FITOCT_FAMILY
#error "compile with -DFITOCT_FAMILY=0|1|2"
#endif
#define FITOCT_CAT2(a, b) a##b
#define FITOCT_CAT(a, b) FITOCT_CAT2(a, b)

#if FITOCT_FAMILY == 0
int lds_bytes(int ppl, int G, int max_depth) {
  return ppl == 1 ? Lds<1>::bytes(G, max_depth) : Lds<2>::bytes(G, max_depth);
}
// doubles in a chain's migration image: its LDS region up to the tree levels
int mig_img_words(int ppl) {
  return ppl == 1 ? Lds<1>::chain_bytes(0) / 8 : Lds<2>::chain_bytes(0) / 8;
}
#endif

template <class R, int BPT, int NNP, int PPL, int MODE>
static hipError_t launch_t(bool logp, const KParams& P, const KParams* dP, int tiles,
                           hipStream_t st, const int* tile_map) {
  constexpr int F = FITOCT_FAMILY;
  // two-ended trajectories: 3 chain areas (the chain's and its two producers')
  const int lds = (!logp && P.bidi) ? Lds<PPL>::bytes(3, P.max_depth) : Lds<PPL>::bytes(P.G, P.max_depth);
  if (logp) {
    auto k = logp_kernel<R, BPT, NNP, PPL, MODE, F>;
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(k, dim3(tiles), dim3(TPB), lds, st, dP);
  } else {
    // three samplers: with migration, with speculative leaves (one chain per tile), plain
    // four samplers: with / without migration, with / without speculative leaves
    auto k = P.mig != nullptr
                 ? (P.spec ? nuts_kernel<R, BPT, NNP, PPL, MODE, F, true, true, false>
                           : nuts_kernel<R, BPT, NNP, PPL, MODE, F, true, false, false>)
             : P.spec ? (P.pair ? nuts_kernel<R, BPT, NNP, PPL, MODE, F, false, true, true>
                                : nuts_kernel<R, BPT, NNP, PPL, MODE, F, false, true, false>)
                      : nuts_kernel<R, BPT, NNP, PPL, MODE, F, false, false, false>;
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(k, dim3(tiles), dim3(TPB), lds, st, dP, tile_map);
  }
  return hipGetLastError();
}

template <class R, int NNP, int PPL, int MODE>
static hipError_t launch_m(bool logp, int bpt, const KParams& P, const KParams* dP, int tiles,
                           hipStream_t st, const int* tm) {
  switch (bpt) {
    case 0: return launch_t<R, 0, NNP, PPL, MODE>(logp, P, dP, tiles, st, tm);
    case 1: return launch_t<R, 1, NNP, PPL, MODE>(logp, P, dP, tiles, st, tm);
    case 2: return launch_t<R, 2, NNP, PPL, MODE>(logp, P, dP, tiles, st, tm);
    case 4: return launch_t<R, 4, NNP, PPL, MODE>(logp, P, dP, tiles, st, tm);
    case 8:
      if constexpr (MODE == MODE_POLY) return launch_t<R, 8, NNP, PPL, MODE>(logp, P, dP, tiles, st, tm);
      return hipErrorInvalidValue;
    case 16:   // compact geo layout, f64 only (N in (2048, 4096] on an arithmetic grid)
      if constexpr (MODE == MODE_POLY && sizeof(R) == 8)
        return launch_t<R, 16, NNP, PPL, MODE>(logp, P, dP, tiles, st, tm);
      return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
  }
}

template <int NNP, int PPL>
static hipError_t launch_n(bool logp, bool mixed, int bpt, const KParams& P, const KParams* dP,
                           int tiles, hipStream_t st, const int* tm) {
  if (!mixed) {
    if (P.mode == MODE_POLY)
      return launch_m<double, NNP, PPL, MODE_POLY>(logp, bpt, P, dP, tiles, st, tm);
    if constexpr (NNP == 15 && PPL == 1) {   // N <= 512: the rows in registers
      if (bpt == 1) return launch_t<double, 1, NNP, PPL, MODE_ROWS>(logp, P, dP, tiles, st, tm);
      if (bpt == 2) return launch_t<double, 2, NNP, PPL, MODE_ROWS>(logp, P, dP, tiles, st, tm);
    }
    if (bpt != 0) return hipErrorInvalidValue;
    return launch_t<double, 0, NNP, PPL, MODE_ROWS>(logp, P, dP, tiles, st, tm);
  }
  return launch_m<float, NNP, PPL, MODE_ROWS>(logp, bpt, P, dP, tiles, st, tm);
}

// P: host copy (shapes); dP: the same block already copied to device memory
hipError_t FITOCT_CAT(launch_family_, FITOCT_FAMILY)(bool logp, bool mixed, int bpt, int nnp,
                                                     const KParams& P, const KParams* dP,
                                                     int tiles, hipStream_t st,
                                                     const int* tile_map) {
  if (nnp == 15) return launch_n<15, 1>(logp, mixed, bpt, P, dP, tiles, st, tile_map);
  return launch_n<24, 2>(logp, mixed, bpt, P, dP, tiles, st, tile_map);
}

}  // namespace fitoct
