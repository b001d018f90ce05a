// Device-resident NUTS, layer 9: the sampler kernel.  nuts_kernel is one persistent tile of
// 8 specialised waves: it places the tile (batch tile_map, paired blocks), loads the lanes'
// bins and the tile's LDS (tile_migrate.h), and dispatches the waves to their roles --
//   * gradient waves 0..3: drain the ring of posted positions (gradient_pass.h);
//   * NUTS waves 4..7: one Chain each (chain.h), cycling run() -> post_sweep -> wait for the
//     4 partial sums; a free slot of a migrating tile waits in receive_chain;
//   * in a tile of one chain, the spare NUTS waves: the booking helper and the two producers
//     of two-ended trajectories, or, in a paired launch, the bridge waves (bridge_in,
//     bridge_out) that carry the forward end to and from the partner tile.
// The comment ahead of the kernel has the pipeline, batch mode and the paired tiles' layout.
// Part of the sampler's one translation unit (nuts_device.hip includes the layers in order).
// All of it lives in namespace fitoct, which dev_common.h opens and only nuts_device.hip
// closes: parsed on its own, this header ends inside the open namespace.
// NOT a stand-alone header, and compiled under nuts_device.hip's second pragma,
// "#pragma clang fp contract(fast)" (HIP's default), not under the sweep's "on": include it
// only there, after tile_migrate.h (sweep_math.h needs the opposite regime and says why).
#pragma once

// A NUTS wave's wait for its chain's sweeps: grad_cnt[c] reaching `want`.  The counter's
// address stays in one VGPR for the whole wait and the polled value goes through
// v_readfirstlane, so a poll is one LDS read, one lane read and scalar compares: no reload of
// a spilled address and no lane-mask loop around a wave-uniform count.  False: the wait expired.
__device__ __forceinline__ bool wait_sweeps(const int* cnt, const int want, Patience& w) {
  const AS_LDS int* p = (const AS_LDS int*)cnt;
  asm volatile("" : "+v"(p));
  const int n = __builtin_amdgcn_readfirstlane(want);   // (the slot's epoch is wave-uniform)
  while (__builtin_amdgcn_readfirstlane(__atomic_load_n(p, __ATOMIC_RELAXED)) < n) {
    if (w.expired(LEAF_WAIT_TICKS)) return false;
    __builtin_amdgcn_s_sleep(1);
  }
  return true;
}

// Dataflow pipeline inside a tile.  The NUTS wave of chain c writes the next
// position's parameters to MP[c] and enqueues c in an LDS ring (64-bit entries
// {sequence number, chain}); the gradient waves drain the ring in order, each
// sweeping its bins for that chain and bumping grad_cnt[c]; the NUTS wave waits
// until grad_cnt[c] reaches NGW * epoch and runs the sampler until it yields
// the next position.  Chains cycle independently (no barrier after start-up),
// so the sampler latency of one chain hides behind the sweeps of the others.
//
// Batch mode (fitoct_batch_*, FitOCT.R's loop over files): Pg is an array of
// parameter blocks, one per problem, and tile_map[2*tile] = {problem, first
// chain} places each tile; a tile never mixes problems, so every tile still
// keeps one problem's bins in registers.  tile_map == nullptr: one problem.
//
// Paired tiles (P.pair, one-chain tiles with two-ended trajectories, 2 x tiles <= CUs): block
// b is tile (b / 16) * 8 + b % 8 in the role (b / 8) % 2 -- 0: the primary, which hosts the
// chain, its helper and the backward end's producer; 1: its partner, which grows the forward
// end on its own gradient waves.  Blocks b and b + 8 (one XCD when blocks are dealt round-robin
// over the 8 XCDs; for speed only, the hand-off is correct on any placement) form a pair.
// PAIR: the paired launch (one-chain tiles with two-ended trajectories and partners; MIG =
// false, SPEC = true): its own instantiation, so that neither the bridges nor the partner's
// roles cost the unpaired kernels registers
template <class R, int BPT, int NNP, int PPL, int MODE, int FAM, bool MIG, bool SPEC, bool PAIR>
__global__ void __launch_bounds__(TPB, 2) nuts_kernel(const KParams* __restrict__ Pg,
                                                      const int* __restrict__ tile_map) {
  // the basis mode as a constant of the sampler's chain code (config 5 at one GPU +3 %), but
  // for the paired row-mode sampler, which reads it (config 2 +1.7 %: the compiler's schedule
  // of the producers; same-box A/B, profiles/r06_ab_rows.txt)
  constexpr int CMODE = (SPEC && PAIR && MODE == MODE_ROWS) ? -1 : MODE;
  int tix = blockIdx.x, role = 0;
  if constexpr (PAIR) {
    role = (tix >> 3) & 1;
    tix = ((tix >> 4) << 3) | (tix & 7);
    if (tix >= ((KPc*)Pg)->pair_tiles) return;   // the grid's padding to whole groups of 16
  }
  int pidx = 0, c0;
  if (tile_map) {
    const AS_CST int* tm = (const AS_CST int*)tile_map;
    pidx = __builtin_amdgcn_readfirstlane(tm[2 * tix]);
    c0 = __builtin_amdgcn_readfirstlane(tm[2 * tix + 1]);
  } else {
    c0 = tix * ((KPc*)Pg)->G;
  }
  KPc& P = *((KPc*)Pg + pidx);   // device-resident parameter block: uniform s_load reads
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // two-ended trajectories carve two more chain areas (the producers' slots 1, 2)
  const Lds<PPL> L{(AS_LDS char*)smem, P.bidi ? 3 : P.G, Lds<PPL>::chain_bytes(P.max_depth)};
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nct = min(P.G, P.chains - c0);
  __shared__ unsigned long long ring[RINGN];
  __shared__ int q_reserve, n_active, grad_cnt[GMAX];
  // post a sweep of chain slot s (lane 0 of the posting wave; its MP writes are in before):
  // sequence number from a ring-wide counter, one 64-bit store.  (Per-slot doorbells without
  // the atomic's return measured -3 to -6 %, gradient waves at priority 2-3 during sweeps
  // -16 to -19 % on config 2: profiles/r06_ab_rows.txt.)
  auto post_sweep = [&](const int s) {
    const unsigned rs = (unsigned)atomicAdd(&q_reserve, 1);
    __atomic_store_n(&ring[rs % RINGN], ((unsigned long long)rs << 32) | (unsigned)s, __ATOMIC_RELAXED);
  };
  __shared__ int bd[BD_N];   // two-ended trajectories' hand-off words (BdWord)
  __shared__ long long done_t[GMAX];   // profiling build: when the 8th wave finished chain c
  __shared__ long long start_min[GMAX], start_max[GMAX];
  // speculative leaves (P.spec, tiles of one or two chains): chain slot c's NUTS wave posts
  // a request for the bookkeeping of its leaf (deep: the leaf in HX[c]) or the prior part of
  // a speculated position; its helper wave (NUTS wave G + c) runs it and publishes the
  // request number it finished
  __shared__ int help_req[2], help_done[2], help_res[2], help_seen[2], help_gen[2], help_m[2],
      help_dead[2];
  const bool spec = SPEC;
  const bool helped = SPEC && !MIG && P.G <= 2;   // spare NUTS waves help the tile's chains
  const bool bidi = Chain<PPL, NNP, FAM, MIG, SPEC, CMODE>::kTwoEnded && helped &&
                   P.bidi != 0;   // ... and two producer waves
  __shared__ int live_chains;   // chains the tile hosts (speculation policy, Chain::live)
  // paired tiles: this pair's hand-off words and buffer; pair_on: the partner has joined
  // (partner tile: 1 = it grows the forward end, 0 = it leaves at once)
  const bool paired = PAIR && bidi;
  AS_GLB int* const xh = paired ? (AS_GLB int*)P.pair_hdr + (size_t)tix * PAIR_HDR_INTS : nullptr;
  AS_GLB double* const xb = paired ? (AS_GLB double*)P.pair_buf + (size_t)tix * P.pair_stride : nullptr;
  __shared__ int pair_on;

  load_kinv<PPL, NNP, FAM>(P, L, tid);
  if (tid == 0) {
    q_reserve = 0;
    n_active = nct;
    live_chains = nct;
    pair_on = 0;
    if (paired && role == 0 && nct > 0) __hip_atomic_fetch_or(xh + PH_STATE, PS_START, __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_AGENT);
    if (paired && role == 1) {
      // join once the primary has begun; give up (LOCAL) if it has not within PAIR_JOIN_TICKS
      // (the blocks of a launch start within a microsecond of each other on an idle chip; the
      // primary decides only at its chain's first transition, many gradients later)
      bool join = false;
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      for (int st = x_ldi(xh + PH_STATE); !P.pair_test_absent;) {
        if (st & PS_LOCAL) break;
        int expect = st & PS_START ? st : 0;
        const int want = st & PS_START ? st | PS_JOIN : PS_LOCAL;
        if (!(st & PS_START) && __builtin_amdgcn_s_memrealtime() - t0 < PAIR_JOIN_TICKS) {
          __builtin_amdgcn_s_sleep(2);
          st = x_ldi(xh + PH_STATE);
          continue;
        }
        if (__hip_atomic_compare_exchange_strong(xh + PH_STATE, &expect, want, __ATOMIC_RELAXED,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
          join = (want & PS_JOIN) != 0;
          break;
        }
        st = expect;   // the primary began (or decided) meanwhile: look again
      }
      if (!join) __hip_atomic_fetch_or(xh + PH_STATE, PS_LOCAL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pair_on = join ? 1 : 0;
      n_active = join ? 1 : 0;   // the partner's bridge wave ends its gradient waves
    }
  }
  if (tid < 2) {
    // (a partner tile has no backward-end producer: its helper serves producer 1 only)
    help_req[tid] = (role == 1 && tid == 0) ? -1 : 0;
    help_done[tid] = 0;
    help_res[tid] = 0;
    help_seen[tid] = 0;
    help_gen[tid] = 0;
    help_m[tid] = 0;
    help_dead[tid] = 0;
  }
  if (tid < GMAX) {
    grad_cnt[tid] = 0;
    done_t[tid] = 0;
    start_min[tid] = 0x7FFFFFFFFFFFFFFFLL;
    start_max[tid] = 0;
  }
  if (tid < RINGN) ring[tid] = ~0ULL;
  // (a tile of one chain: the producers' areas are NUTS slots 1 and 2)
  if (tid < BD_N) bd[tid] = (tid == TW_SLOT) ? 1 : (tid == TW_SLOT + 1) ? 2 : 0;
  if (MIG && P.mig != nullptr) {   // every slot of the tile may host migrants: all NUTS waves live
    if (tid == 0) {
      const MigView M(P.mig, P.mig_tiles);
      n_active = P.G;
      __hip_atomic_store((int*)&M.load[tix], nct, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add((int*)&M.hdr[MIG_STARTED], 1, __ATOMIC_RELAXED,   // a count: no data
                             __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();

  const bool stamp = kProfile && (P.stamps != nullptr) && role == 0 && lane == 0 && (wave == 0 || wave == NGW);
  const bool wstamp = kProfile && (P.stamps != nullptr) && role == 0 && lane == 0 && wave < NGW;
  long long t_wbusy = 0;
  long long t_busy = 0, n_items = 0, t_wait = 0, t_enq = 0, t_sweep = 0, t_notice = 0;
  long long t_st0 = 0, t_st1 = 0;
  long long t_begin = stamp ? (long long)__builtin_amdgcn_s_memtime() : 0;
  // tile timeline (profiling build): start, first chain finished, end, on the 100 MHz clock
  __shared__ long long first_done_rt;
  __shared__ int chains_done_here;
  const long long rt_begin = kProfile ? (long long)__builtin_amdgcn_s_memrealtime() : 0;
  if (kProfile && tid == 0) {
    first_done_rt = 0;
    chains_done_here = 0;
  }
  if (kProfile) __syncthreads();
  if (wave < NGW) {  // ------------------------- gradient waves
    Bins<R, BPT, NNP, MODE> bins;
    bins.load(P, tid);
    int zero_done[GMAX] = {0, 0, 0, 0};
    // profiling build: tile occupancy -- real time and sweeps by the tile's live chains
    // (0..4) at each ring entry (wave 0; the tail of a launch is its thinned-out tiles)
    long long occ_t[GMAX + 1] = {0, 0, 0, 0, 0}, occ_n[GMAX + 1] = {0, 0, 0, 0, 0};
    long long occ_last = kProfile ? (long long)__builtin_amdgcn_s_memrealtime() : 0;
    int occ_k = GMAX;
    for (unsigned h = 0;; ++h) {
      unsigned long long e;
      bool stop = false;
      Patience w;
      for (;;) {  // wait for ring entry h
        e = lds_load64(&ring[h % RINGN]);
        if ((unsigned)(e >> 32) == h) break;
        if (lds_load(&n_active) == 0) {
          stop = true;
          break;
        }
        // hang guard: with migration a tile may idle (receivers posted) until the launch's
        // last chain ends; without, its chains may pause between sweeps (a two-ended tree's
        // chain wave, init) but never for a leaf's wait bound
        if (w.expired(MIG_WAIT_TICKS + 10 * TICKS_PER_S)) {
          stop = true;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      if (stop) break;
      const int c = (int)(e & 0xFF);
      if (kProfile && wave == 0 && P.stamps != nullptr) {
        const long long now = (long long)__builtin_amdgcn_s_memrealtime();
        occ_t[occ_k] += now - occ_last;   // the interval since the last entry, at its count
        occ_last = now;
        occ_k = min(max(lds_load(&live_chains), 0), GMAX);
        ++occ_n[occ_k];
      }
      const long long s0 = stamp ? (long long)__builtin_amdgcn_s_memtime() : 0;
      const long long s0w = wstamp ? (long long)__builtin_amdgcn_s_memtime() : 0;
      if (kProfile && lane == 0) {   // sweep start spread over the 8 waves
        const unsigned long long t = (unsigned long long)__builtin_amdgcn_s_memtime();
        atomicMin((unsigned long long*)&start_min[c], t);
        atomicMax((unsigned long long*)&start_max[c], t);
      }
      if (P.prior_PD == 0)
        gradient_pass<R, BPT, NNP, MODE, true>(P, bins, L.mp(0), L.part(), zero_done, c, c + 1,
                                               tid, lane, wave);
      wave_publish();   // this wave's PART writes before its count
      if (wstamp) t_wbusy += (long long)__builtin_amdgcn_s_memtime() - s0w;
      if (lane == 0) {
        if (kProfile)   // latest finisher's time; LDS ops of a wave complete in order
          atomicMax((unsigned long long*)&done_t[c], (unsigned long long)__builtin_amdgcn_s_memtime());
        atomicAdd(&grad_cnt[c], 1);
      }
      if (stamp) {
        t_busy += (long long)__builtin_amdgcn_s_memtime() - s0;
        ++n_items;
      }
    }
    if (kProfile && role == 0 && wave == 0 && lane == 0 && P.stamps != nullptr) {
      AS_GLB long long* o = (AS_GLB long long*)P.stamps + (size_t)tix * NSTAMP;
      // (the interval after the last entry: the tile's live count now, normally 0 -- a
      // tile whose chains have finished waits for migrants, or the launch's end)
      occ_t[min(max(lds_load(&live_chains), 0), GMAX)] +=
          (long long)__builtin_amdgcn_s_memrealtime() - occ_last;
      for (int k = 0; k <= GMAX; ++k) {
        o[SS_OCC_TIME + k] = occ_t[k];
        o[SS_OCC_SWEEPS + k] = occ_n[k];
      }
    }
  } else {           // ------------------------- NUTS waves
    // the sampler is the latency-critical stage and shares each SIMD with two
    // throughput-bound gradient waves: let it win issue arbitration
    // (priority 2 / 1 / 0: -0.3 % / +-0 / -23 % on config 3)
    __builtin_amdgcn_s_setprio(3);
    const int c = wave - NGW;
    const bool mig = MIG && P.mig != nullptr;
    using Ch = Chain<PPL, NNP, FAM, MIG, SPEC, CMODE>;
    // Two-ended trajectories: producer of trajectory end s (0: backward, 1: forward) on NUTS
    // slot `slot` (its chain area holds the end's state, its subtree's levels and merge
    // uniforms, and its last subtree's record; its proposal pool is its own).  For every
    // transition g the chain starts (BD_GEN), it builds the subtrees of the doublings drawn in
    // direction s from the start outwards (Chain::sub_leaf), at most BIDI_LOOK doublings past
    // the one booked, and publishes one record per subtree once the booking has taken the
    // previous one.  `epoch`: the slot's sweeps so far (grad_cnt[slot] counts NGW per sweep).
    // Ends with BD_GEN < 0 (the tile's chain finished) or, in a migrating tile, with the launch.
    auto produce = [&](const int s, const int slot, long long epoch) {
      // helped: another wave books this end's leaves (serve: tiles of one chain -- the backward
      // end the booking helper; the forward end the partner tile's helper, or in an unpaired
      // row-mode tile the chain's wave while it waits for records), else the producer books them
      // itself (an unpaired tile with the factorised basis, whose registers have no room for the
      // chain's serving; a migrating launch's tail)
      const bool helped = !MIG && (s == 0 || PAIR || MODE == MODE_ROWS);
      int hreq = 0;   // leaves handed to the helper
      Ch pr(P, L, slot, c0, lane, nct);
      pr.bd = (volatile AS_LDS int*)bd;
      pr.pix = P.chains + (c0 / P.G) * GMAX + slot;   // its own proposal pool region
      int seen = 0;
      bool quit = false;
      // profiling build: cycles waiting for sweeps, for the lookahead / ring room, leaves,
      // and cycles inside trees
      long long pf_sw = 0, pf_may = 0, pf_n = 0, pf_tree = 0;
      // (and per leaf: finish_grad + end_update_p, staging the next leaf, the hand-over, prior_part)
      long long pf_fg = 0, pf_st = 0, pf_ho = 0, pf_pp = 0;
      auto pclk = [&]() -> long long { return kProfile ? (long long)__builtin_amdgcn_s_memtime() : 0; };
      while (!quit) {
        int g;
        {
          Patience w;
          int polls = 0;
          const unsigned long long t_idle = MIG ? __builtin_amdgcn_s_memrealtime() : 0;
          const unsigned long long idle_max = P.tail_idle_ticks ? P.tail_idle_ticks : MIG_WAIT_TICKS;
          while ((g = lds_load(&bd[BD_GEN])) == seen || (g > 0 && (g & BD_ENDED))) {
            if (MIG) {
              // a tail producer idle this long leaves -- but only once it holds TW_BUSY, so no
              // chain claims the pair while it withdraws its role (TW_JOIN, its TW_CLAIM bit):
              // a chain never waits for records of a producer that has gone.  While
              // a chain holds TW_BUSY its tree is under way and the producer stays.
              if (__builtin_amdgcn_s_memrealtime() - t_idle > idle_max) {
                int gone = 0;
                if (lane == 0 && atomicCAS((int*)&bd[TW_BUSY], 0, 2) == 0) {
                  atomicSub((int*)&bd[TW_JOIN], 1);
                  atomicAnd((int*)&bd[TW_CLAIM], ~(1 << s));
                  __atomic_store_n(&bd[TW_BUSY], 0, __ATOMIC_RELAXED);
                  gone = 1;
                }
                if (__builtin_amdgcn_readfirstlane(__shfl(gone, 0))) {
                  quit = true;
                  break;
                }
              }
            } else if (w.expired(MIG_WAIT_TICKS)) {
              quit = true;
              break;
            }
            if (MIG && (++polls & 255) == 0 &&
                __builtin_amdgcn_readfirstlane(g_load(&MigView(P.mig, P.mig_tiles).hdr[MIG_DONE])) >=
                    P.chains) {
              quit = true;
              break;
            }
            __builtin_amdgcn_s_sleep(MIG ? 8 : 1);
          }
        }
        if (quit || g < 0) break;
        seen = g;
        wave_fence();
        // the chain being grown: its key (direction draws) and its scalars (booked depth)
        const int lcg = lds_load(&bd[TW_LC]);
        pr.key = make_key(P.seed, (uint32_t)(P.chain_offset + lcg));
        const AS_LDS ChainScalars& S0 = L.cs(lds_load(&bd[TW_CHAIN]));
        Vd<PPL> q = pr.ld(V_E0_Q), p = pr.ld(V_E0_P), gr = pr.ld(V_E0_G);
        const Vd<PPL> minv = pr.ld(V_MINV);
        const double eps = pr.Sp->eps_used;
        const uint32_t t = (uint32_t)pr.uni(pr.Sp->t);
        // bit k: doubling k grows in direction s (act_begin_subtree's draws)
        const bool mine = lane < P.max_depth &&
                          ((uniform(pr.key, t, TAG_DIR, (uint32_t)lane, 0u) > 0.5) ? 1 : 0) == s;
        const unsigned long long dmask = __builtin_amdgcn_ballot_w64(mine);
        wave_fence();
        if (lds_load(&bd[BD_GEN]) != g) continue;   // the start was rewritten while read
        const double e = s ? eps : -eps;
        // this end's next doubling after depth d (-1: none)
        auto next_depth = [&](const int d) -> int {
          const unsigned long long r = d < 0 ? dmask : dmask & ~((2ULL << d) - 1);
          return r ? (int)__builtin_ctzll(r) : -1;
        };
        // may the subtree of depth d grow now: within BIDI_LOOK doublings of the booked depth.
        // Once true it stays true for the transition (the booked depth only grows)
        auto may = [&](const int d) -> bool {
          return d <= pr.uni(*(volatile const AS_LDS int*)&S0.depth) + BIDI_LOOK;
        };
        const long long pft0 = kProfile ? (long long)__builtin_amdgcn_s_memtime() : 0;
        auto wait_may = [&](const int d) -> bool {   // false: the tree ended
          Patience w;
          const long long pt = kProfile ? (long long)__builtin_amdgcn_s_memtime() : 0;
          for (;;) {
            if (lds_load(&bd[BD_GEN]) != g) {
              if (kProfile) pf_may += (long long)__builtin_amdgcn_s_memtime() - pt;
              return false;
            }
            if (may(d)) {
              if (kProfile) pf_may += (long long)__builtin_amdgcn_s_memtime() - pt;
              return true;
            }
            // the other end may grow for long (deep trees, large N).  In effect this wait
            // ends with BD_GEN: its bound outlasts the bound on the whole tree (MIG_WAIT_TICKS
            // from the tree's start), after which BD_GEN changes
            if (w.expired(2 * MIG_WAIT_TICKS)) return false;
            __builtin_amdgcn_s_sleep(1);
          }
        };
        // record m's slot is free once the booking has taken record m - RSLOTS
        auto wait_room = [&](const int m) -> bool {   // false: the tree ended
          Patience w;
          const long long pt = kProfile ? (long long)__builtin_amdgcn_s_memtime() : 0;
          for (;;) {
            if (lds_load(&bd[BD_GEN]) != g) return false;
            if (lds_load(&bd[BD_CONS + s]) >= m - Ch::RSLOTS + 1) {
              if (kProfile) pf_may += (long long)__builtin_amdgcn_s_memtime() - pt;
              return true;
            }
            if (w.expired(2 * MIG_WAIT_TICKS)) return false;
            __builtin_amdgcn_s_sleep(1);
          }
        };
        // expl_leapfrog from the last leaf of this end (begin_update_p, update_q), staged for
        // the gradient waves and enqueued; the position-only prior terms overlap the sweep
        Vd<PPL> p1, q1;
        auto stage = [&](const Vd<PPL>& qa, const Vd<PPL>& pa, const Vd<PPL>& ga) {
#pragma unroll
          for (int k = 0; k < PPL; ++k) {
            p1.a[k] = fma(0.5 * e, ga.a[k], pa.a[k]);
            q1.a[k] = fma(e, minv.a[k] * p1.a[k], qa.a[k]);
          }
          pr.write_mp(q1);
          if (lane == 0) post_sweep(slot);
          ++epoch;
        };
        int d = next_depth(-1);
        if (d < 0 || !wait_may(d)) continue;
        if (!helped) pr.sub_begin(d);   // (helped: the helper begins a subtree at its leaf 0)
        int m = 0;   // subtree records published this transition (not helped)
        int j = 0;   // the leaf in its sweep: leaf j of the subtree of depth d
        stage(q, p, gr);
        pr.prior_part();
        // a leaf is in its sweep here.  Once it is in, the next one (in this subtree, or the
        // first of this end's next subtree if that may grow already) is staged first and the
        // leaf's bookkeeping runs during that sweep: the next position depends only on this
        // leaf's q, p and g (if the bookkeeping ends the subtree, that sweep is dropped)
        for (;;) {
          bool late = false;
          Patience ws;
          const long long pt = kProfile ? (long long)__builtin_amdgcn_s_memtime() : 0;
          while (lds_load(&grad_cnt[slot]) < (int)(NGW * epoch)) {
            if (ws.expired(LEAF_WAIT_TICKS)) {
              late = true;
              break;
            }
            __builtin_amdgcn_s_sleep(1);
          }
          if (kProfile) {
            pf_sw += (long long)__builtin_amdgcn_s_memtime() - pt;
            ++pf_n;
          }
          if (late) {
            quit = true;
            break;
          }
          wave_fence();
          long long pc0 = pclk();
          // read with the partial sums (its latency hides in finish_grad's): a leaf the tree
          // no longer needs is dropped
          const int gen_now = lds_load(&bd[BD_GEN]);
          Vd<PPL> gn;
          double s2;
          const double lp = pr.finish_grad(gn, s2);
          Vd<PPL> pe;
#pragma unroll
          for (int k = 0; k < PPL; ++k) pe.a[k] = fma(0.5 * e, gn.a[k], p1.a[k]);   // end_update_p
          if (gen_now != g) break;   // the tree has ended: the leaf is not needed
          const Vd<PPL> qn = q1;
          const bool last = j == (1 << d) - 1;
          const int dn = last ? next_depth(d) : d;
          const bool nxt = !last || (dn >= 0 && may(dn));
          if (kProfile) {
            const long long pc1 = pclk();
            pf_fg += pc1 - pc0;
            pc0 = pc1;
          }
          if (nxt) stage(qn, pe, gn);
          if (kProfile) {
            const long long pc1 = pclk();
            pf_st += pc1 - pc0;
            pc0 = pc1;
          }
          if (helped) {
            // hand this leaf to the booking helper (two slots: once it has booked the leaf
            // before the previous one); stop when a booking cut its subtree (nothing later on
            // this end is needed)
            if (hreq > 0) {
              Patience wh;
              bool gone = false;
              while (lds_load(&help_done[s]) < hreq - 1) {
                if (lds_load(&bd[BD_GEN]) != g || wh.expired(LEAF_WAIT_TICKS)) {
                  gone = true;
                  break;
                }
                __builtin_amdgcn_s_sleep(1);
              }
              if (gone) break;
              const int res = lds_load(&help_res[s]);
              if ((res >> 2) == g && (res & 3) == Ch::SL_END) break;
            }
            AS_LDS double* X = L.px(s, (hreq + 1) & 1);
#pragma unroll
            for (int k = 0; k < PPL; ++k) {
              X[pr.idx(k)] = qn.a[k];
              X[Ch::VLEN + pr.idx(k)] = pe.a[k];
              X[2 * Ch::VLEN + pr.idx(k)] = gn.a[k];
            }
            if (lane == 0) {
              X[3 * Ch::VLEN] = lp;
              X[3 * Ch::VLEN + 1] = s2;
              X[3 * Ch::VLEN + 2] = (double)d;
              X[3 * Ch::VLEN + 3] = (double)j;
              X[3 * Ch::VLEN + 4] = (double)g;
            }
            wave_publish();   // the leaf lands before its request number
            ++hreq;
            if (lane == 0) __atomic_store_n(&help_req[s], hreq, __ATOMIC_RELAXED);
            if (kProfile) {
              const long long pc1 = pclk();
              pf_ho += pc1 - pc0;
              pc0 = pc1;
            }
            if (last) {
              if (dn < 0) break;   // this end has no further doubling in this tree
              if (!nxt) {
                if (!wait_may(dn)) break;
                stage(qn, pe, gn);
              }
              d = dn;
              j = 0;
            } else {
              ++j;
            }
            pr.prior_part();
            if (kProfile) pf_pp += pclk() - pc0;
            continue;
          }
          XF Tw{0.0, 0};
          int Tprop = -1;
          Vd<PPL> Tpb = pe, Trho = pe;
          double h = 0.0;
          const int r = pr.sub_leaf(qn, pe, gn, minv, lp, s2, Tw, Tprop, Tpb, Trho, h);
          if (r != Ch::SL_MID) {   // the subtree is complete (or cut): its record for the booking
            if (!wait_room(m)) break;
            const int fl = r == Ch::SL_DONE ? Ch::SR_VALID
                                            : pr.uni(pr.Sp->divergent) ? Ch::SR_DIVERGENT : 0;
            pr.sub_publish(s, m, fl, Tw, Tprop, Tpb, Trho, qn, pe, gn, lp, s2, h);
            wave_publish();   // the record lands before its count
            ++m;
            if (lane == 0) __atomic_store_n(&bd[BD_PROD + s], gen_word(g, m), __ATOMIC_RELAXED);
            if (r == Ch::SL_END || dn < 0) break;   // this end adds nothing more to the tree
            if (!nxt) {
              if (!wait_may(dn)) break;
              stage(qn, pe, gn);
            }
            d = dn;
            j = 0;
            pr.sub_begin(d);
          } else {
            ++j;
          }
          pr.prior_part();
        }
        if (kProfile) pf_tree += (long long)__builtin_amdgcn_s_memtime() - pft0;
      }
      if (helped && lane == 0) __atomic_store_n(&help_req[s], -1, __ATOMIC_RELAXED);   // its helper may leave
      if (kProfile && P.stamps != nullptr && lane == 0) {   // this end's producer (either tile)
        AS_GLB long long* o = (AS_GLB long long*)P.stamps + (size_t)tix * NSTAMP + SS_PRODUCER + 4 * s;
        o[0] = pf_sw;
        o[1] = pf_may;
        o[2] = pf_n;
        o[3] = pf_tree;
        AS_GLB long long* o2 = (AS_GLB long long*)P.stamps + (size_t)tix * NSTAMP + SS_PRODUCER_LEAF + 4 * s;
        o2[0] = pf_fg;
        o2[1] = pf_st;
        o2[2] = pf_ho;
        o2[3] = pf_pp;
      }
    };
    // Two-ended trajectories in a tile of one chain: the booking helper (NUTS wave 1 of the tile,
    // and of a partner tile) books the leaves its producers hand over -- Chain::sub_leaf on the
    // producer's own chain area, its subtree record once the subtree ends (when the booking has
    // taken the previous one) -- while the producer completes the next gradient and stages the
    // one after.  One request of producer s: 1 served, 0 none pending, -1 the producer is gone.
    // (help_seen / help_gen / help_m: requests served, and the transition and records published
    // of producer s, kept by the helper.)
    // nb (the chain's wave serving the forward end of an unpaired tile): serve a leaf only if its
    // subtree's record would find its slot free -- that wave alone frees the slots, so it must
    // never wait for one here.  0 then: not served (the request stays pending).
    auto serve = [&](const int s, const bool nb) -> int {
      const int rq0 = lds_load(&help_req[s]);
      if (rq0 < 0) return -1;
      const int rq = lds_load(&help_seen[s]) + 1;   // requests are served in order
      if (rq > rq0) return 0;
      wave_fence();   // the leaf after its request number
      Ch hc(P, L, 1 + s, c0, lane, nct);
      hc.bd = (volatile AS_LDS int*)bd;
      hc.pix = P.chains + (c0 / P.G) * GMAX + 1 + s;
      const AS_LDS double* X = L.px(s, rq & 1);
      Vd<PPL> q, pe, gg;
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        q.a[k] = X[hc.idx(k)];
        pe.a[k] = X[Ch::VLEN + hc.idx(k)];
        gg.a[k] = X[2 * Ch::VLEN + hc.idx(k)];
      }
      const double lp = X[3 * Ch::VLEN], s2 = X[3 * Ch::VLEN + 1];
      const int d = __builtin_amdgcn_readfirstlane((int)X[3 * Ch::VLEN + 2]);
      const int j = __builtin_amdgcn_readfirstlane((int)X[3 * Ch::VLEN + 3]);
      const int gen = __builtin_amdgcn_readfirstlane((int)X[3 * Ch::VLEN + 4]);
      int r = Ch::SL_END;
      // (else a leaf of a tree that has ended, or of a subtree a booking has cut: help_dead)
      if (lds_load(&bd[BD_GEN]) == gen &&
          !(lds_load(&help_gen[s]) == gen && lds_load(&help_dead[s]) == gen)) {
        hc.key = make_key(P.seed, (uint32_t)(P.chain_offset + lds_load(&bd[TW_LC])));
        int hm = lds_load(&help_m[s]);
        if (lds_load(&help_gen[s]) != gen) hm = 0;
        if (nb && lds_load(&bd[BD_CONS + s]) < hm - Ch::RSLOTS + 1) return 0;
        if (j == 0) hc.sub_begin(d);
        XF Tw{0.0, 0};
        int Tprop = -1;
        Vd<PPL> Tpb = pe, Trho = pe;
        double h = 0.0;
        r = hc.sub_leaf(q, pe, gg, hc.ld(V_MINV), lp, s2, Tw, Tprop, Tpb, Trho, h);
        if (r != Ch::SL_MID) {   // the subtree ended: its record, once the slot is free
          Patience w;
          bool room = true;
          while (lds_load(&bd[BD_CONS + s]) < hm - Ch::RSLOTS + 1) {
            if (lds_load(&bd[BD_GEN]) != gen || w.expired(2 * MIG_WAIT_TICKS)) {
              room = false;
              break;
            }
            __builtin_amdgcn_s_sleep(1);
          }
          if (room) {
            const int fl = r == Ch::SL_DONE ? Ch::SR_VALID
                                            : hc.uni(hc.Sp->divergent) ? Ch::SR_DIVERGENT : 0;
            hc.sub_publish(s, hm, fl, Tw, Tprop, Tpb, Trho, q, pe, gg, lp, s2, h);
            wave_publish();   // the record lands before its count
            ++hm;
            if (lane == 0) __atomic_store_n(&bd[BD_PROD + s], gen_word(gen, hm), __ATOMIC_RELAXED);
          } else {
            r = Ch::SL_END;
          }
        }
        if (lane == 0) {
          help_m[s] = hm;
          help_gen[s] = gen;
          if (r == Ch::SL_END) help_dead[s] = gen;
        }
      }
      wave_publish();   // the booking's LDS writes land before its result
      if (lane == 0) {
        help_seen[s] = rq;
        __atomic_store_n(&help_res[s], (gen << 2) | r, __ATOMIC_RELAXED);
        wave_publish();
        __atomic_store_n(&help_done[s], rq, __ATOMIC_RELAXED);
      }
      return 1;
    };
    // ---- paired tiles (P.pair): the bridge waves.  The forward end's producer runs unchanged
    // in the partner tile (NUTS wave 3, chain area 2); two bridge waves make the pair look like
    // one tile to it and to the primary's booking:
    //   bridge_in (primary, NUTS wave 3, where that producer would run): each transition's start
    //     (producer area 2, written by bidi_begin) and the end of each tree, and the booking's
    //     progress (records of the forward end taken, booked depth) out to the pair's words;
    //     the partner's subtree records in, into the primary's area 2, published as a local
    //     producer would (BD_PROD + 1);
    //   bridge_out (partner, NUTS wave 2): the start into the producer's area and BD_GEN; the
    //     booking's progress into BD_CONS + 1 and the depth the producer's lookahead reads;
    //     the producer's records out to the pair's record slot, then PH_COUNT.
    // A record reaches the booking only through both bridges, and the producer writes record
    // m only once the (mirrored, never larger) count of records booked is m, so one count
    // guards the record's three slots.  Counts and the booked depth carry their transition
    // (gen_word) and only grow within it.
    constexpr int QXD = Lds<PPL>::QX_DOUBLES;   // a record: Ch::RVEC vectors, then scalars
    constexpr int RVD = Ch::RVEC * Ch::VLEN;
    auto pair_start = [&]() { return xb; };
    // the pair's record slot k (the forward end's records m, k = m % 2): vectors, scalars
    auto pair_rec = [&](const int k) { return xb + 4 * Ch::VLEN + PAIR_START_DOUBLES + k * QXD; };
    // end 1's record slot k in this tile (Chain::rvec / rsc)
    auto fwd_vec = [&](const int k) -> AS_LDS double* {
      if constexpr (Ch::RSLOTS == 1) return L.vecs(2) + V_E1_Q * Ch::VLEN;
      else return L.qx0() + (2 + k) * QXD;
    };
    auto fwd_sc = [&](const int k) -> AS_LDS double* {
      if constexpr (Ch::RSLOTS == 1) return L.vecs(2) + V_RHO * Ch::VLEN;
      else return fwd_vec(k) + RVD;
    };
    auto bridge_in = [&]() -> bool {   // false: the pair did not form (grow the end here)
      {
        Patience w;   // the chain's first transition (or its end)
        while (lds_load(&bd[BD_GEN]) == 0 && !w.expired(MIG_WAIT_TICKS)) __builtin_amdgcn_s_sleep(1);
      }
      int st = 0;
      if (lane == 0) {
        int expect = PS_START;
        st = __hip_atomic_compare_exchange_strong(xh + PH_STATE, &expect, PS_START | PS_LOCAL,
                                                  __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT)
                 ? PS_START | PS_LOCAL
                 : expect;
      }
      st = __builtin_amdgcn_readfirstlane(__shfl(st, 0));
      if ((st & PS_LOCAL) || !(st & PS_JOIN)) return false;
      constexpr int VL = Ch::VLEN;
      AS_GLB double* const xs = pair_start();

      AS_LDS double* const av = L.vecs(2);        // producer area 2: the start, the record
      AS_LDS ChainScalars* const as = &L.cs(2);
      const volatile AS_LDS int* depth = (const volatile AS_LDS int*)&L.cs(0).depth;
      int seen = 0, copied = 0, last_cons = -1, last_depth = -1;
      Patience idle;
      for (;;) {
        const int g = lds_load(&bd[BD_GEN]);
        if (g != seen) {
          if (g < 0) {
            if (lane == 0) x_sti(xh + PH_GEN, -1);
            break;
          }
          if (!(g & BD_ENDED)) {   // a new transition: its start first
            wave_fence();   // the start after its number
#pragma unroll
            for (int s = 0; s < PPL; ++s) {
              const int k = s * WAVE + lane;
              x_st(xs + k, av[V_E0_Q * VL + k]);
              x_st(xs + VL + k, av[V_E0_P * VL + k]);
              x_st(xs + 2 * VL + k, av[V_E0_G * VL + k]);
              x_st(xs + 3 * VL + k, av[V_MINV * VL + k]);
            }
            if (lane == 0) {
              x_st(xs + 4 * VL, as->eps_used);
              x_st(xs + 4 * VL + 1, as->H0);
              x_sti(xh + PH_T, as->t);
              x_sti(xh + PH_LC, lds_load(&bd[TW_LC]));
            }
            x_drain();   // the start has reached memory before its number
          }
          if (lane == 0) {
            x_sti(xh + PH_GEN, g);   // (a tree's end: its number with BD_ENDED)
            if (!(g & BD_ENDED)) atomicAdd(P.pair_count, 1ULL);
          }
          seen = g;
          copied = 0;
          last_cons = last_depth = -1;
          idle = Patience{};
          continue;
        }
        // the booking's progress on the forward end, for the partner's lookahead and record slot
        const int cons = lds_load(&bd[BD_CONS + 1]);
        const int dep = *depth;
        if (lds_load(&bd[BD_GEN]) == seen) {
          if (lane == 0 && cons != last_cons) x_sti(xh + PH_CONS, gen_word(seen, cons));
          if (lane == 0 && dep != last_depth) x_sti(xh + PH_DEPTH, gen_word(seen, dep));
          last_cons = cons;
          last_depth = dep;
        }
        // the partner's next record of this transition
        const int pc = __builtin_amdgcn_readfirstlane(x_ldi(xh + PH_COUNT));
        if ((pc >> 16) == seen && (pc & 0xFFFF) > copied) {
          const int cnt = pc & 0xFFFF;
          for (int n = copied; n < cnt; ++n) {   // records n: the pair's slot -> end 1's slot
            const AS_GLB double* src = pair_rec(n & 1);
            AS_LDS double* dv = fwd_vec(n & 1);
            AS_LDS double* ds = fwd_sc(n & 1);
            for (int i = lane; i < QXD; i += WAVE) {
              const double v = x_ld(src + i);
              if (i < RVD) dv[i] = v;
              else ds[i - RVD] = v;
            }
          }
          wave_publish();   // the records land before their count
          copied = cnt;
          if (lane == 0) __atomic_store_n(&bd[BD_PROD + 1], gen_word(seen, copied), __ATOMIC_RELAXED);
          idle = Patience{};
          continue;
        }
        if (idle.expired(2 * MIG_WAIT_TICKS)) break;   // never, short of a fault
        __builtin_amdgcn_s_sleep(1);
      }
      if (lane == 0) __atomic_store_n(&help_req[1], -1, __ATOMIC_RELAXED);   // no producer 1 here
      return true;
    };
    auto bridge_out = [&]() {
      constexpr int VL = Ch::VLEN;
      AS_GLB double* const xs = pair_start();

      AS_LDS double* const av = L.vecs(2);        // the producer's area
      AS_LDS ChainScalars* const as = &L.cs(2);
      volatile AS_LDS int* depth = (volatile AS_LDS int*)&L.cs(0).depth;   // the producer's S0
      if (lane == 0) {
        bd[TW_CHAIN] = 0;
        *depth = 0;
      }
      int seen = 0, copied = 0;
      Patience idle;
      for (;;) {
        const int g = __builtin_amdgcn_readfirstlane(x_ldi(xh + PH_GEN));
        const int cw = __builtin_amdgcn_readfirstlane(x_ldi(xh + PH_CONS));
        const int dw = __builtin_amdgcn_readfirstlane(x_ldi(xh + PH_DEPTH));
        if (g != seen) {
          if (g < 0) break;
          if (!(g & BD_ENDED)) {   // a new transition: the start into the producer's area
#pragma unroll
            for (int s = 0; s < PPL; ++s) {
              const int k = s * WAVE + lane;
              av[V_E0_Q * VL + k] = x_ld(xs + k);
              av[V_E0_P * VL + k] = x_ld(xs + VL + k);
              av[V_E0_G * VL + k] = x_ld(xs + 2 * VL + k);
              av[V_MINV * VL + k] = x_ld(xs + 3 * VL + k);
            }
            if (lane == 0) {
              as->eps_used = x_ld(xs + 4 * VL);
              as->H0 = x_ld(xs + 4 * VL + 1);
              as->t = x_ldi(xh + PH_T);
              bd[TW_LC] = x_ldi(xh + PH_LC);
              bd[BD_CONS + 1] = 0;
              *depth = 0;
            }
          }
          wave_publish();   // the start lands before the transition's number
          if (lane == 0) __atomic_store_n(&bd[BD_GEN], g, __ATOMIC_RELAXED);
          seen = g;
          copied = 0;
          idle = Patience{};
          continue;
        }
        if (lane == 0) {   // the booking's progress: never lowered within the transition
          if ((cw >> 16) == seen && (cw & 0xFFFF) > bd[BD_CONS + 1]) bd[BD_CONS + 1] = cw & 0xFFFF;
          if ((dw >> 16) == seen && (dw & 0xFFFF) > *depth) *depth = dw & 0xFFFF;
        }
        const int pw = lds_load(&bd[BD_PROD + 1]);
        if ((pw >> 16) == seen && (pw & 0xFFFF) > copied) {
          const int cnt = pw & 0xFFFF;
          wave_fence();   // the records after their count
          for (int n = copied; n < cnt; ++n) {   // records n: end 1's slot -> the pair's slot
            const AS_LDS double* sv = fwd_vec(n & 1);
            const AS_LDS double* ss = fwd_sc(n & 1);
            AS_GLB double* dst = pair_rec(n & 1);
            for (int i = lane; i < QXD; i += WAVE) x_st(dst + i, i < RVD ? sv[i] : ss[i - RVD]);
          }
          x_drain();   // the records have reached memory before their count
          copied = cnt;
          if (lane == 0) x_sti(xh + PH_COUNT, gen_word(seen, copied));
          idle = Patience{};
          continue;
        }
        if (idle.expired(2 * MIG_WAIT_TICKS)) break;   // never, short of a fault
        __builtin_amdgcn_s_sleep(1);
      }
      // the chain has finished: stop the producer, let it drain its sweep, end the tile
      if (lane == 0) __atomic_store_n(&bd[BD_GEN], -1, __ATOMIC_RELAXED);
      {
        Patience w;
        while (lds_load(&bd[BD_EXIT]) < 1 && !w.expired(LEAF_WAIT_TICKS)) __builtin_amdgcn_s_sleep(1);
      }
      wave_fence();
      if (lane == 0) atomicSub(&n_active, 1);
    };
    if constexpr (PAIR) {
      if (role == 1 && pair_on && c == 2) bridge_out();   // partner tile: the bridge
    }
    if constexpr (SPEC && !MIG) {
      if (bidi && c == 1 && (role == 0 || pair_on)) {
        // the booking helper of producer 0 (a primary; in a paired launch also its producer 1
        // if the pair did not form) or 1 (a partner).  An unpaired launch's producer 1 books
        // its leaves itself (a helper serving both ends would pace both).
        constexpr bool both = PAIR;
        // below the producers and the sweep's NUTS neighbours: it has slack (4.1 k of a
        // producer's 5.8 k cycles per leaf, profiling build), and the gradient wave sharing its
        // SIMD is on a sweep's critical path (config 2: priority 2 / 1 +0.5 % over 3,
        // profiles/r06_ab_prio.txt)
        __builtin_amdgcn_s_setprio(2);
        Patience w;
        long long pf_busy = 0, pf_n = 0;   // profiling build: cycles booking, leaves booked
        for (int s = role;; s = (both && role == 0) ? s ^ 1 : s) {   // (one call site of serve)
          const long long pt = kProfile ? (long long)__builtin_amdgcn_s_memtime() : 0;
          const int a = serve(s, false);
          if (a > 0) {
            if (kProfile) {
              pf_busy += (long long)__builtin_amdgcn_s_memtime() - pt;
              ++pf_n;
            }
            w = Patience{};
            continue;
          }
          const bool alt = both && role == 0;
          if (a < 0 && (!alt || lds_load(&help_req[s ^ 1]) < 0)) break;   // producers gone
          if (!alt || s == 1) {
            if (w.expired(MIG_WAIT_TICKS)) break;   // never, short of a fault
            __builtin_amdgcn_s_sleep(1);
          }
        }
        if (kProfile && P.stamps != nullptr && lane == 0) {   // this tile's booking helper
          AS_GLB long long* o = (AS_GLB long long*)P.stamps + (size_t)tix * NSTAMP + SS_HELPER + 2 * role;
          o[0] = pf_busy;
          o[1] = pf_n;
        }
      }
    }
    // two-ended trajectories: producer of the backward (c = 2) / forward end (c = 3); paired
    // tiles: the forward end grows in the partner tile (its NUTS wave 3) and the primary's
    // wave 3 is the bridge.  (One call site: produce is inlined once.)
    if (bidi && c >= 2 && (role == 0 || (pair_on && c == 3))) {
      bool here = true;
      if constexpr (PAIR) {
        if (role == 0 && c == 3) here = !bridge_in();
      }
      if (here) produce(c - 2, c - 1, 0);
      wave_fence();
      if (lane == 0) atomicAdd(&bd[BD_EXIT], 1);
    }
    if (helped && !bidi && c >= P.G && c - P.G < nct) {   // the helper wave of chain slot c - G
      using Ch = Chain<PPL, NNP, FAM, MIG, SPEC, CMODE>;
      const int hs = c - P.G;
      Ch ch(P, L, hs, c0 + hs, lane, nct);
      int seen = 0;
      Patience w;
      for (;;) {
        const int r = lds_load(&help_req[hs]);
        if (r < 0) break;                       // the chain has finished
        if (r == seen) {
          // the chain releases its helper when it finishes (help_req = -1), however long
          // its gaps between speculated leaves (init, step-size searches): the hang guard
          // is in real time, not polls, as for migration receivers
          if (w.expired(MIG_WAIT_TICKS)) break;
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        w = Patience{};
        seen = r;
        wave_fence();   // the request's arguments are read after its number
        // book the handed-over leaf; publish its outcome, then the number
        const int res = ch.deep_book();
        wave_publish();
        if (lane == 0) {
          __atomic_store_n(&help_res[hs], res, __ATOMIC_RELAXED);
          wave_publish();
          __atomic_store_n(&help_done[hs], seen, __ATOMIC_RELAXED);
        }
      }
    }
    if (role == 0 && c < (mig ? P.G : nct)) {
      using Ch = Chain<PPL, NNP, FAM, MIG, SPEC, CMODE>;
      long long epoch = 0;     // this slot's hand-offs (grad_cnt[c] counts NGW per epoch)
      int lc = c < nct ? c0 + c : -1;
      int a = Ch::A_INIT_STATE;
      for (;;) {   // the slot's own chain, then (migration) chains handed over by other tiles
       if (lc >= 0) {
        Ch ch(P, L, c, lc, lane, nct);
        ch.live = (const AS_LDS int*)&live_chains;
        ch.bd = (volatile AS_LDS int*)bd;
        long long steps = 0;
        bool in_sweep = false;   // the last run() was A_PRIOR, overlapping the chain's sweep
        // ONE call site of the action machine (it is inlined once, not per caller)
        int hreq = 0;            // helper requests posted (speculative path)
        for (;;) {
          FITOCT_MARK(nuts_loop);
        const long long s0 = stamp ? (long long)__builtin_amdgcn_s_memtime() : 0;
        const int y = ch.run(a);
        if (Ch::kTwoEnded && y == Ch::A_BIDI_TREE) {   // the producers grow the subtrees
          const int g = lds_load(&bd[BD_GEN]);
          const bool late = false;
          // this wave books the trajectory level; in an unpaired tile it books the forward end's
          // leaves too while it waits for records
          ch.bidi_book_tree(g, [&]() -> bool {
            if constexpr (!PAIR && !MIG && MODE == MODE_ROWS) return serve(1, true) > 0;
            return false;
          });
          wave_publish();   // the producers stop growing this tree
          if (lane == 0) {
            __atomic_store_n(&bd[BD_GEN], g | BD_ENDED, __ATOMIC_RELAXED);
            __atomic_store_n(&bd[TW_BUSY], 0, __ATOMIC_RELAXED);   // (migrating tiles) another chain may claim them
          }
          wave_fence();   // the helper's bookkeeping is read after the end
          // the helper's booked leaves count toward the step bound like the chain's own
          steps += ch.uni(ch.Sp->n_leapfrog);
          if (late || ch.uni(ch.Sp->status) == ERR_TIMEOUT || steps > P.max_steps) {
            ch.Sp->status = ERR_TIMEOUT;
            a = Ch::A_FINISH;
          } else {
            a = Ch::A_END_TREE;
          }
          continue;
        }
        if (spec && y == Ch::A_SPEC_STAGED) {   // enqueue the speculated position, hand its prior part over
          if (++steps > P.max_steps) {
            ch.Sp->status = ERR_TIMEOUT;
            a = Ch::A_FINISH;
            continue;
          }
          if (lane == 0) {
            post_sweep(c);
            if (ch.deep) {
              wave_publish();   // the hand-off (HX) lands before the request number
              __atomic_store_n(&help_req[c], hreq + 1, __ATOMIC_RELAXED);
            }
          }
          if (stamp) t_enq = (long long)__builtin_amdgcn_s_memtime();
          if (ch.deep) {   // the helper books the leaf; this wave computes the next prior part
            ++hreq;
            ch.book_done = (volatile AS_LDS int*)&help_done[c];
            ch.book_res = (volatile AS_LDS int*)&help_res[c];
            ch.book_want = hreq;
            ++epoch;
            a = Ch::A_PRIOR;
            in_sweep = true;
            continue;
          }
          ++epoch;   // (no helper wave: this wave books the leaf during the sweep)
          a = Ch::A_SPEC_BOOK;
          continue;
        }
        if (spec && (y == Ch::A_SPEC_WAIT || y == Ch::A_SPEC_DISCARD)) {
          Patience w;
          const long long w0 = stamp ? (long long)__builtin_amdgcn_s_memtime() : 0;
          if (stamp) t_busy += w0 - s0;
          const bool late = !wait_sweeps(&grad_cnt[c], (int)(NGW * epoch), w);
          wave_fence();   // nothing of the next action is read before the sweep and the helper are done
          if (stamp) {
            const long long t1 = (long long)__builtin_amdgcn_s_memtime();
            t_wait += t1 - w0;
            t_sweep += done_t[c] - t_enq;
            t_st0 += start_min[c] - t_enq;
            t_st1 += start_max[c] - t_enq;
            start_min[c] = 0x7FFFFFFFFFFFFFFFLL;
            start_max[c] = 0;
            t_notice += t1 - (done_t[c] > w0 ? done_t[c] : w0);
            ++n_items;
          }
          if (late) {
            ch.Sp->status = ERR_TIMEOUT;
            a = Ch::A_FINISH;
          } else {
            a = (y == Ch::A_SPEC_WAIT) ? Ch::A_GRAD : Ch::A_END_TREE;
          }
          continue;
        }
        if (in_sweep) {
          in_sweep = false;
          bool late = false;
          Patience w;
          const long long w0 = stamp ? (long long)__builtin_amdgcn_s_memtime() : 0;
          // A NUTS wave waits at priority 3 on a SIMD it shares with a gradient wave.  When
          // the sweep is long (8+ bins per lane, or streamed bins) and the tile hosts
          // several chains, the wait is long and the sampler is not the bottleneck: poll
          // rarely, so the waiting wave leaves the SIMD's issue to the gradient wave.
          if (P.G >= 2 && (BPT >= 8 || BPT == 0)) {
            __builtin_amdgcn_s_setprio(0);
            late = !wait_sweeps(&grad_cnt[c], (int)(NGW * epoch), w);
            __builtin_amdgcn_s_setprio(3);
          } else {
            late = !wait_sweeps(&grad_cnt[c], (int)(NGW * epoch), w);
          }
          if (stamp) {
            const long long t1 = (long long)__builtin_amdgcn_s_memtime();
            t_wait += t1 - w0;
            t_sweep += done_t[c] - t_enq;            // enqueue -> 8th gradient wave done
            t_st0 += start_min[c] - t_enq;           // enqueue -> first wave starts
            t_st1 += start_max[c] - t_enq;           // enqueue -> last wave starts
            start_min[c] = 0x7FFFFFFFFFFFFFFFLL;
            start_max[c] = 0;
            t_notice += t1 - (done_t[c] > w0 ? done_t[c] : w0);
          }
          if (late) {
            ch.Sp->status = ERR_TIMEOUT;
            a = Ch::A_FINISH;
          } else {
            a = Ch::A_GRAD;
          }
          continue;
        }
        if (stamp) {
          t_busy += (long long)__builtin_amdgcn_s_memtime() - s0;
          ++n_items;
        }
        const int stt = __builtin_amdgcn_readfirstlane(ch.Sp->state);
        if (stt == ST_DONE || stt == ST_MOVED) {
          if (kProfile && lane == 0 && stt == ST_DONE) {
            atomicCAS((unsigned long long*)&first_done_rt, 0ULL,
                      (unsigned long long)__builtin_amdgcn_s_memrealtime());
            atomicAdd(&chains_done_here, 1);
          }
          if (helped && lane == 0) __atomic_store_n(&help_req[c], -1, __ATOMIC_RELAXED);   // release the helper
          if (bidi) {   // release the producers; they drain their sweeps
            if (kProfile && P.stamps != nullptr && lane == 0) {   // the booking's time
              AS_GLB long long* o = (AS_GLB long long*)P.stamps + (size_t)tix * NSTAMP;
              o[SS_BOOK_BUSY] = ch.pf_busy;
              o[SS_BOOK_WAIT] = ch.pf_wait;
              o[SS_BOOK_LEAVES] = ch.pf_n;
            }
            if (lane == 0) __atomic_store_n(&bd[BD_GEN], -1, __ATOMIC_RELAXED);
            Patience w;
            while (lds_load(&bd[BD_EXIT]) < 2 && !w.expired(LEAF_WAIT_TICKS)) __builtin_amdgcn_s_sleep(1);
          }
          if (spec && lane == 0) atomicSub(&live_chains, 1);
          break;
        }
        if (++steps > P.max_steps) {   // termination guarantee: report, never hang
          ch.Sp->status = ERR_TIMEOUT;
          a = Ch::A_FINISH;
          continue;
        }
        if constexpr (kProfile) {
          if (P.bench_sweeps > 0 && P.stamps != nullptr) {   // sweep-only measurement
            for (int r = 0; r < P.bench_sweeps; ++r) {
              if (lane == 0) post_sweep(c);
              ++epoch;
              while (lds_load(&grad_cnt[c]) < (int)(NGW * epoch)) __builtin_amdgcn_s_sleep(1);
            }
            ch.Sp->state = ST_DONE;
            break;
          }
        }
        // enqueue chain c: sequence number from a ring-wide counter, one 64-bit store
        if (lane == 0) post_sweep(c);
        if (stamp) t_enq = (long long)__builtin_amdgcn_s_memtime();
        ++epoch;
        // position-only work (prior terms, next merges' uniforms) overlaps the sweep
        a = Ch::A_PRIOR;
        in_sweep = true;
        }
        if (mig && lane == 0 && __builtin_amdgcn_readfirstlane(ch.Sp->state) == ST_DONE) {
          const MigView M(P.mig, P.mig_tiles);
          g_add(&M.load[blockIdx.x], -1);
          __hip_atomic_fetch_add((int*)&M.hdr[MIG_DONE], 1, __ATOMIC_RELAXED,   // a count: no data
                                 __HIP_MEMORY_SCOPE_AGENT);
        }
       }
        if (!mig) break;
        lc = receive_chain<PPL>(P, L, c, lane, (volatile AS_LDS int*)bd, (const AS_LDS int*)&live_chains);
        if constexpr (Ch::kTwoEnded) {
          if (lc <= -2) {   // recruited as a producer of the tile's lone chain (the tail)
            produce(-2 - lc, c, epoch);
            break;
          }
        }
        if (lc < 0) break;
        if (spec && lane == 0) atomicAdd(&live_chains, 1);
        a = Ch::A_START_TRANSITION;
      }
      wave_fence();
      if (lane == 0) atomicSub(&n_active, 1);
    }
  }
  if (wstamp) ((AS_GLB long long*)P.stamps)[(size_t)tix * NSTAMP + SS_WAVE_BUSY + wave] = t_wbusy;
  if (stamp) {
    AS_GLB long long* o = (AS_GLB long long*)P.stamps + (size_t)tix * NSTAMP;
    if (wave == 0) {
      o[SS_SWEEPS] = n_items;
      o[SS_GRAD_BUSY] = t_busy;
      o[SS_WALL] = (long long)__builtin_amdgcn_s_memtime() - t_begin;
      o[SS_RT_BEGIN] = rt_begin;
      o[SS_RT_END] = (long long)__builtin_amdgcn_s_memrealtime();
      o[SS_RT_FIRST_DONE] = first_done_rt;
      o[SS_CHAINS_DONE] = chains_done_here;
    } else {
      o[SS_NUTS_BUSY] = t_busy;
      o[SS_WAIT] = t_wait;
      o[SS_ENQ_TO_SWEPT] = t_sweep;
      o[SS_SWEPT_TO_RESUMED] = t_notice;
      o[SS_FIRST_START] = t_st0;
      o[SS_LAST_START] = t_st1;
      o[SS_ROUNDS] = n_items;
      for (int k = 0; k < 18; ++k) {
        o[SS_ACT_CYCLES + k] = L.cs(0).prof[0][k];
        o[SS_ACT_CALLS + k] = L.cs(0).prof[1][k];
      }
      for (int k = 0; k < 8; ++k) o[SS_SUB + k] = L.cs(0).prof[0][PROF_SUB + k];
      for (int k = 0; k < 4; ++k) o[SS_SUB_HI + k] = L.cs(0).prof[0][PROF_SUB + 8 + k];
    }
  }
}
