// Device-resident NUTS, layer 1: what every other layer of the sampler uses.  Address
// spaces, the names of a chain's LDS vectors / tree-level records / pool slots, the chain's
// scalars (ChainScalars), the two-ended trajectories' hand-off words (BdWord), the bounds
// of every wait (Patience) and the three orderings of a wave's LDS traffic.
//
// This header opens namespace fitoct for the whole translation unit: the layers after it
// (dev_global.h ... gradient_pass.h, then chain.h, tile_migrate.h, nuts_kernel.h) and the
// rest of nuts_device.hip, which includes them in order, are written inside it;
// nuts_device.hip closes it at its end.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "kernel_params.h"
#include "philox.h"

namespace fitoct {

// Explicit address spaces: LDS (3), global (1), constant (4).  Generic pointers
// would compile to FLAT instructions, which count in both vmcnt and lgkmcnt --
// every LDS wait would then also wait for the sampler's outstanding HBM stores.
#define AS_LDS __attribute__((address_space(3)))
#define AS_GLB __attribute__((address_space(1)))
#define AS_CST __attribute__((address_space(4)))
using KPc = const AS_CST KParams;

enum { FAM_NORMAL = 0, FAM_LASSO = 1, FAM_HORSESHOE = 2, FAM_MONO = 3 };
// (round 6: the A/B switches measured "off" or "rejected" in DESIGN.md §4 are gone from
// the kernel; what is left compiles to the measured defaults.  The only remaining build
// switches are the ordering fallbacks FITOCT_LOCAL_FENCE / FITOCT_LDS_INORDER and the
// profiling build FITOCT_PROFILE.)
// 16 bins per lane (config 4): moments are formed per group of 8 bins
constexpr int BPT16_GROUP = 8;

// Cycle stamps (FITOCT_STAMPS) exist only in a profiling build
// (FITOCT_PROFILE=1 python -m fitoct_amd.build): the production kernels carry
// no per-action timing code at all.
#ifndef FITOCT_PROFILE
#define FITOCT_PROFILE 0
#endif
constexpr bool kProfile = FITOCT_PROFILE != 0;
// -DFITOCT_ASM_MARKS: assembly comments at action boundaries, for per-action
// instruction counts in a -S listing (scripts/asm_actions.py); no code otherwise
#ifdef FITOCT_ASM_MARKS
#define FITOCT_MARK(name) asm volatile(";MARK " #name)
#else
#define FITOCT_MARK(name)
#endif
enum { ERR_INIT = -4, ERR_NUMERIC = -5, ERR_TIMEOUT = -6, ERR_CANCELLED = -8 };

// vectors kept in LDS per chain (lane-private elements)
enum VecId : int {
  V_CUR_Q, V_CUR_P, V_CUR_G,
  V_E0_Q, V_E0_P, V_E0_G,      // backward end of the trajectory
  V_E1_Q, V_E1_P, V_E1_G,      // forward end
  V_SMP_Q, V_SMP_G,            // z_sample (its momentum enters only the energy: smp_h)
  V_MINV, V_WF_M, V_WF_M2,     // metric + Welford
  V_RHO, V_PNEAR,              // trajectory momentum sum, near end of old trajectory
  V_QS, V_QE,                  // staged q and its constrained values (exp on positive params)
  V_PG, V_CA,                  // prior part of grad, likelihood coefficient (prior_part)
  NVEC
};
// U-turn record of one tree level (LDS)
enum LvlId : int { K_PBEG = 0, K_PEND = 1, K_RHO = 2, NLVL = 3 };
// proposal pool slot (HBM): q and g of a candidate sample.  Its momentum is dead once it is
// a candidate (the next transition draws a fresh one) except in the energy__ diagnostic,
// H(z_sample), which is the candidate leaf's own Hamiltonian h: kept as a scalar (pool_h)
enum PoolId : int { P_Q = 0, P_G = 1, NPOOL = POOL_VECS };
constexpr int NAUX = 96;   // per chain: yGP[32] | horseshoe lambda_j*tau [32] | FW_j [32]

struct ChainScalars {
  int state, t, depth, leaf, dir, n_leapfrog, divergent, init_attempt;
  int da_counter, win_counter, win_size, win_next, wf_n, ss_trial, ss_dir, ss_window;
  int status, win_on, init_buf, term_buf, pool_used, lsw_e, spec_we, pad2;
  int st_prop[MAXDEPTH];
  int st_w_e[MAXDEPTH];
  double H0, lsw_m, sum_metro, eps, eps_used, mu, s_bar, x_bar, ss_H0, lf_e;
  double cur_lp, cur_s2, smp_lp, smp_s2;
  double pr_lp, pr_is2, u_top, spec_wm;   // spec_wm, spec_we, spec_h: the speculative
                                          // path's booked leaf weight and energy
  int u_blk[MAXDEPTH];     // which block of 64 merge uniforms each level's ring holds (-1: none)
  double end_lp[2], end_s2[2];
  double st_w_m[MAXDEPTH];
  double pool_lp[MAXDEPTH + 1], pool_s2[MAXDEPTH + 1];
  long long leapfrogs;
  double spec_h;
  // Hamiltonian -lp + K(p) of each pool candidate and of the sample (energy__)
  double pool_h[MAXDEPTH + 1], smp_h;
  // the running subtree's sum of the leaves' acceptance terms (added to sum_metro when the
  // subtree ends, so two-ended trajectories can sum per subtree and stay bitwise equal)
  double sub_metro, pad_sm;
  long long prof[2][32];   // diagnostic build: cycles and calls per action
};
static_assert(sizeof(ChainScalars) % 16 == 0, "LDS carve alignment");

// two-ended trajectories (P.bidi): the tile's hand-off words in LDS.  BD_GEN: the transition
// (1..BD_GEN_MASK, -1: the chain has finished); BD_PROD + s: stream s's published leaves as
// (gen << 16) | count; BD_CONS + s: leaves of stream s the helper has booked; BD_END: the
// transition whose tree the helper has ended; BD_EXIT: producers that have left
// TW_*: who grows the ends -- the producers' NUTS slots (TW_SLOT, TW_SLOT + 1; a tile of
// one chain: 1, 2), the chain's slot and index (TW_CHAIN, TW_LC; written by bidi_begin);
// migrating tiles recruit producers at run time (TW_CLAIM: role bits claimed, TW_JOIN:
// producers in place; see receive_chain)
enum BdWord : int {
  BD_GEN = 0, BD_PROD = 1, BD_CONS = 3, BD_END = 5, BD_EXIT = 6,
  TW_CLAIM = 7, TW_JOIN = 8, TW_SLOT = 9, TW_CHAIN = 11, TW_LC = 12, TW_BUSY = 13, BD_N = 16
};
constexpr int BD_GEN_MASK = (1 << 15) - 1;
// BD_GEN | BD_ENDED: a migrating tile's chain has booked transition BD_GEN's tree to its end
// (its producers stop, and wait for the next transition or the launch's end)
constexpr int BD_ENDED = 1 << 20;
// (gen << 16) | v, the hand-off words that carry their transition.  Shifted unsigned: a paired
// tile's bridge forms it from BD_GEN | BD_ENDED too, whose bit 20 a signed shift would push
// past int's sign bit (undefined before C++20).  Same bits; the generation is not masked.
__device__ __forceinline__ int gen_word(int gen, int v) {
  return (int)(((unsigned)gen << 16) | (unsigned)v);
}
// a producer runs at most this many doublings past the booked one (lookahead 1 / 2 / 5
// measured -1.0 / -0.2 / +-0 % on config 2, profiles/r05_ab_stage.txt)
constexpr int BIDI_LOOK = 3;

constexpr long long SPIN_LIMIT = 1LL << 26;   // polls (~2 s) before a wait reads the clock
constexpr unsigned long long TICKS_PER_S = 100000000ULL;   // s_memrealtime: 100 MHz
// a wait for one leaf's work (a sweep, a booking, a producer's record): far above any real
// leaf (microseconds; a deep tree's whole trajectory is bounded separately, MIG_WAIT_TICKS)
constexpr unsigned long long LEAF_WAIT_TICKS = 30ULL * TICKS_PER_S;

// The hang guard of every wait in the kernel.  The first SPIN_LIMIT polls read no clock;
// past them the wait is bounded in REAL time (s_memrealtime), not in polls, so a slow
// sweep, a profiler or a deep tree never fails a healthy chain with ERR_TIMEOUT, and a
// fault still ends the launch.  expired(T) is true once T ticks passed since poll SPIN_LIMIT.
struct Patience {
  // polls so far, held at SPIN_LIMIT + 1 once the clock is read: 32 bits, so that a poll's
  // count and compare are scalar instructions (a 64-bit ordered compare is a VALU one)
  uint32_t n = 0;
  unsigned long long t0 = 0;
  __device__ __forceinline__ bool expired(unsigned long long ticks) {
    if (n < (uint32_t)SPIN_LIMIT) {
      ++n;
      return false;
    }
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    if (n == (uint32_t)SPIN_LIMIT) {
      t0 = t;
      n = (uint32_t)SPIN_LIMIT + 1;
    }
    __builtin_amdgcn_s_sleep(32);
    return t - t0 > ticks;
  }
};

__device__ __forceinline__ void wave_fence() {
  // orders this wave's LDS traffic: every earlier ds_* op has completed and the
  // compiler may not move memory accesses across this point.
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// A wave reading back what its own lanes just stored to LDS: the DS operations of one
// wave are performed in issue order (the AMDGPU memory model), so only the compiler must
// keep the order -- no wait for the stores to complete (FITOCT_LOCAL_FENCE=0: the full wait)
#ifndef FITOCT_LOCAL_FENCE
#define FITOCT_LOCAL_FENCE 1
#endif
__device__ __forceinline__ void wave_order() {
#if FITOCT_LOCAL_FENCE
  asm volatile("" ::: "memory");
#else
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
}
// A wave publishing LDS data to another wave of the tile by a later LDS store or atomic (a
// sweep's partial sums before grad_cnt, a position's MP before its ring entry, a leaf record
// before its count): the LDS performs one wave's DS operations in issue order, so a reader
// that sees the count and then reads the data sees the data.  FITOCT_LDS_INORDER=0: wait for
// the data stores to complete first (s_waitcnt lgkmcnt(0)).
#ifndef FITOCT_LDS_INORDER
#define FITOCT_LDS_INORDER 1
#endif
__device__ __forceinline__ void wave_publish() {
#if FITOCT_LDS_INORDER
  asm volatile("" ::: "memory");
#else
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
}
