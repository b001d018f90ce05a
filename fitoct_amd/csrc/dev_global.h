// Device-resident NUTS, layer 2: what crosses between workgroups or to the host.
// Agent-scope atomics for chain migration (MigView), system-scope accesses the host polls
// (progress, cancellation), and the paired tiles' hand-off words and sc1 accessors (x_*).
// Part of the sampler's one translation unit (nuts_device.hip includes the layers in order).
// All of it lives in namespace fitoct, which dev_common.h opens and only nuts_device.hip
// closes: parsed on its own, this header ends inside the open namespace.
#pragma once
#include "dev_common.h"

// ---------------------------------------------------------------------------
// chain migration between tiles: agent-scope atomics on global memory (the
// tiles of a launch sit on different XCDs, each with its own L2; release /
// acquire at agent scope write back / invalidate L2 as the gfx950 memory model
// requires).  Rare operations (at most one per transition), so generic pointers.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int g_load(AS_GLB int* p) {
  return __hip_atomic_load((int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int g_add(AS_GLB int* p, int v) {
  return __hip_atomic_fetch_add((int*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int g_or(AS_GLB int* p, int v) {
  return __hip_atomic_fetch_or((int*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int g_and(AS_GLB int* p, int v) {
  return __hip_atomic_fetch_and((int*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// run-time progress / cancellation: host-pinned fine-grained memory, read by the
// host while the kernel runs (system scope; at most one access per transition)
__device__ __forceinline__ void host_st(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ int host_ld(const int* p) {
  return __hip_atomic_load(const_cast<int*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ bool g_cas(AS_GLB int* p, int expect, int v) {
  return __hip_atomic_compare_exchange_strong((int*)p, &expect, v, __ATOMIC_RELAXED,
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
struct MigView {   // KParams::mig carved per MigCtrl
  AS_GLB int* hdr;
  AS_GLB int* load;
  AS_GLB int* fmask;
  AS_GLB int* mbox;
  __device__ MigView(int* base, int tiles)
      : hdr((AS_GLB int*)base), load((AS_GLB int*)base + MIG_HDR), fmask(load + tiles),
        mbox(fmask + tiles) {}
};
constexpr unsigned long long MIG_WAIT_TICKS = 120ULL * TICKS_PER_S;

// ---------------------------------------------------------------------------
// paired tiles (KParams::pair): the forward end of a one-chain tile's two-ended trajectories
// grows in a partner tile, with its own four gradient waves.  Everything crossing between
// the two workgroups is a write-through (sc1) agent-scope store, drained by the storing wave
// (s_waitcnt vmcnt(0)) before the one word that publishes it, and read with sc1 loads only
// (relaxed agent-scope atomics: global_load / global_store ... sc1, no L1 copy on either
// side), so no L2 write-back or invalidation is needed whichever XCDs the two tiles sit on.
// Per pair: PAIR_HDR_INTS hand-off words (zeroed before every launch), then in pair_buf
// the transition's start and one subtree record of the forward end.
// ---------------------------------------------------------------------------
enum PairHdr : int {
  // primary -> partner: the transition (its start is in pair_buf; -1: the chain finished),
  // the booking's records taken of the forward end and the booked depth, each (gen << 16) | v;
  // the chain's index and the transition's number t
  PH_GEN = 0, PH_CONS = 1, PH_DEPTH = 2, PH_LC = 3, PH_T = 4,
  PH_COUNT = 32,   // partner -> primary: (gen << 16) | forward-end subtree records published
  PH_STATE = 48    // PairState bits (both, atomics); PAIR_HDR_INTS words per pair (kernel_params.h)
};
// The pair's hand-shake: the primary marks START when it begins; the partner joins (START ->
// START | JOIN) only if the primary has begun, else marks LOCAL and leaves; the primary decides
// at its chain's first transition (START -> START | LOCAL unless the partner has joined).  So
// a partner that is not resident (a busy GPU) never holds up its primary, and a primary only
// ever waits for a partner that is running: the unpaired tile grows both ends itself.
enum PairState : int { PS_START = 1, PS_JOIN = 2, PS_LOCAL = 4 };
constexpr unsigned long long PAIR_JOIN_TICKS = 10000;   // 100 us (s_memrealtime: 100 MHz)
__device__ __forceinline__ void x_st(AS_GLB double* p, double v) {
  __hip_atomic_store((AS_GLB unsigned long long*)p, __builtin_bit_cast(unsigned long long, v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double x_ld(const AS_GLB double* p) {
  return __builtin_bit_cast(double, __hip_atomic_load((AS_GLB unsigned long long*)p,
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void x_sti(AS_GLB int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int x_ldi(AS_GLB int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// every sc1 store of this wave has reached memory (before the word that publishes them)
__device__ __forceinline__ void x_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
