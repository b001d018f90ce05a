// Device-resident NUTS, layer 8: what a tile's waves share before and between chains.
//   * the tile's start-up load (load_kinv: K^-1 and b zero-padded into LDS, the horseshoe's
//     lane-role block), which logp_kernel and nuts_kernel both run before their first sweep;
//   * the LDS hand-off primitives between the waves of one tile (lds_load, lds_load64, the
//     ring's length RINGN), which both kernels use as well;
//   * chain migration's receiving side (receive_chain): a NUTS wave whose slot is free posts
//     it, waits for a crowded tile's donation (Chain::try_donate, chain.h) and loads the
//     chain's image into the slot's LDS -- or, in the launch's tail, becomes a producer of a
//     lone chain's two-ended trajectories.
// Part of the sampler's one translation unit (nuts_device.hip includes the layers in order).
// All of it lives in namespace fitoct, which dev_common.h opens and only nuts_device.hip
// closes: parsed on its own, this header ends inside the open namespace.
// NOT a stand-alone header, and compiled under nuts_device.hip's second pragma,
// "#pragma clang fp contract(fast)" (HIP's default), not under the sweep's "on": include it
// only there, after chain.h (sweep_math.h needs the opposite regime and says why).
#pragma once

// ---------------------------------------------------------------------------
// the tile's start-up load (both kernels)
// ---------------------------------------------------------------------------
template <int PPL, int NNP, int FAM>
__device__ __forceinline__ void load_kinv(KPc& P, const Lds<PPL>& L, int tid) {
  if (P.mode == MODE_POLY) {  // zero-padded to NNP x NNP so the device loops are fixed-size
    const int Nn = P.Nn;
    for (int i = tid; i < KMAX * KMAX; i += TPB) {   // whole tile: no stale LDS is ever read
      const int r = i / NNP, c = i % NNP;
      L.kinv()[i] = (i < NNP * NNP && r < Nn && c < Nn) ? P.Kinv[r * Nn + c] : 0.0;
    }
    if (tid < NNP) L.bv()[tid] = (tid < Nn) ? P.bvec[tid] : 0.0;
  }
  // the lane-role block (read by the horseshoe's leaf path only): the first NUTS wave, once per tile
  if (FAM == FAM_HORSESHOE && (tid >> 6) == NGW) {
    const int lane = tid & (WAVE - 1);
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      const int k = s * WAVE + lane;
      const LaneRole r = lane_role<FAM>(k, P.D, P.Nn, P.nu);
      AS_LDS LaneRole* o = L.lane_roles() + k;
      o->aw = r.aw;
      o->cc = r.cc;
      o->soff = r.soff;
      o->aoff = r.aoff;
      o->kind = r.kind;
      o->pad = 0;
    }
  }
}

// LDS hand-off primitives between the waves of one tile (one CU: LDS is a
// single coherent memory, so a writer's ds ops completed under lgkmcnt(0) are
// visible to every later read of any wave).
__device__ __forceinline__ int lds_load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ unsigned long long lds_load64(const unsigned long long* p) {
  return __atomic_load_n(p, __ATOMIC_RELAXED);
}
constexpr int RINGN = 16;                 // hand-off ring: >= 2 * GMAX entries

// Migration receiver: post NUTS slot c of this tile as free and wait until a
// crowded tile hands a chain over (returns its chain index, image loaded into
// the slot's LDS) or every chain of the launch has finished (returns -1).
// Receivers wait only once every tile of the launch has started: then no tile
// is waiting for a CU, so waiting cannot starve one.  An idle wait longer than
// MIG_WAIT_TICKS withdraws the post (if no donor claimed it meanwhile).
// The launch's tail (P.tail_bidi; at most P.tail_left chains left unfinished): a receiver
// whose tile hosts exactly one live chain withdraws its post and becomes one of that chain's
// two producers of two-ended trajectories (returns -2 - end; one claim bit per end in
// TW_CLAIM, the slot in TW_SLOT + end, TW_JOIN counts producers in place).  A tile whose
// claims are taken keeps its other free slots posted.
template <int PPL>
__device__ int receive_chain(KPc& P, const Lds<PPL>& L, int c, int lane, volatile AS_LDS int* bd,
                             const AS_LDS int* live) {
  const MigView M(P.mig, P.mig_tiles);
  const int me = blockIdx.x;
  if (__builtin_amdgcn_readfirstlane(g_load(&M.hdr[MIG_STARTED])) < P.mig_tiles) return -1;
  if (lane == 0) {
    g_or(&M.fmask[me], 1 << c);
    g_add(&M.hdr[MIG_WAITING], 1);
  }
  AS_GLB int* box = &M.mbox[me * GMAX + c];
  unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  int m = 0;
  // Poll with relaxed loads and acquire once the mailbox is set: an agent-scope acquire
  // invalidates this XCD's L2, and up to hundreds of receivers wait at the end of a launch
  // (each poll an invalidation would evict every tile's proposal pools on the XCD).
  for (;;) {
    m = __builtin_amdgcn_readfirstlane(g_load(box));
    if (m != 0) break;
    const int done = __builtin_amdgcn_readfirstlane(g_load(&M.hdr[MIG_DONE]));
    if (done >= P.chains) return -1;
    const int lv = __builtin_amdgcn_readfirstlane(*(volatile const AS_LDS int*)live);
    if (P.tail_bidi && P.chains - done <= P.tail_left && lv == 1 &&
        __builtin_amdgcn_readfirstlane(bd[TW_CLAIM]) != 3) {
      int r = -1;
      if (lane == 0) {
        for (int k = 0; k < 2 && r < 0; ++k)
          if (((atomicOr((int*)&bd[TW_CLAIM], 1 << k) >> k) & 1) == 0) r = k;
        if (r >= 0) {
          if ((g_and(&M.fmask[me], ~(1 << c)) >> c) & 1) {   // withdrawn: no migrant comes here
            g_add(&M.hdr[MIG_WAITING], -1);
            bd[TW_SLOT + r] = c;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            atomicAdd((int*)&bd[TW_JOIN], 1);
          } else {   // a donor claimed this slot first: receive its chain, free the end
            atomicAnd((int*)&bd[TW_CLAIM], ~(1 << r));
            r = -1;
          }
        }
      }
      r = __builtin_amdgcn_readfirstlane(__shfl(r, 0));
      if (r >= 0) return -2 - r;
    }
      if (__builtin_amdgcn_s_memrealtime() - t0 > MIG_WAIT_TICKS) {
      int still = 0;   // withdraw the post unless a donor already claimed it
      if (lane == 0) {
        still = (g_and(&M.fmask[me], ~(1 << c)) >> c) & 1;
        if (still) g_add(&M.hdr[MIG_WAITING], -1);
      }
      if (__shfl(still, 0)) return -1;
      while ((m = __builtin_amdgcn_readfirstlane(g_load(box))) == 0) __builtin_amdgcn_s_sleep(8);
      break;
    }
    __builtin_amdgcn_s_sleep(32);
  }
  // pairs with the donor's release store of the mailbox: the image is visible from here
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (lane == 0) __hip_atomic_store((int*)box, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const AS_GLB double* src =
      (const AS_GLB double*)P.mig_img + (size_t)(me * GMAX + c) * P.mig_img_words;
  AS_LDS double* dst = (AS_LDS double*)L.chain(c);
  for (int i = lane; i < P.mig_img_words; i += WAVE) dst[i] = src[i];
  wave_fence();
  return m - 1;
}
