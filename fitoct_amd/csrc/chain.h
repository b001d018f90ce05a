// Device-resident NUTS, layer 7: the chain.  One NUTS wave drives one chain, lane k holding
// parameter k (Vd: a lane's PPL elements of a vector).  Chain is that wave's view of the
// chain's LDS area (lds_layout.h) and the sampler written as a flat action machine
// (Chain::Act, Chain::run): every action appears once, returns the next one, and A_YIELD
// hands the position staged by act_write_mp to the gradient waves (gradient_pass.h).  In
// source order:
//   * the lp / grad completion around a sweep: write_mp, prior_part, finish_grad;
//   * the actions: initialisation and the step-size search (act_init_*, act_ss_*), the
//     transition (act_start_transition, act_begin_subtree, act_leapfrog, act_grad), Stan's
//     recursive build_tree replayed one leaf per step (leaf_book, leaf_book_split: the U-turn
//     records of each tree level in LDS, the multinomial proposals in the HBM pool), the
//     end of a tree and the adaptation (act_end_tree, act_next_transition), act_finish;
//   * speculative leaves (the SPEC sampler): leaf_spec, act_spec_book, and the helper
//     wave's booking deep_book;
//   * two-ended trajectories (P.bidi, "two-ended trajectories" below has the argument why
//     the draws stay the same): the producers' subtrees (sub_begin, sub_leaf, sub_publish)
//     and the booking of the trajectory level from one record per subtree (bidi_begin,
//     bidi_book_tree; tail_ready / tail_claim in a migrating launch's tail);
//   * migration's donating side, try_donate (the receiving side is tile_migrate.h).
// The waves that run all this, and what they wait for, are nuts_kernel.h's.
// Part of the sampler's one translation unit (nuts_device.hip includes the layers in order).
// All of it lives in namespace fitoct, which dev_common.h opens and only nuts_device.hip
// closes: parsed on its own, this header ends inside the open namespace.
// NOT a stand-alone header, and compiled under nuts_device.hip's second pragma,
// "#pragma clang fp contract(fast)" (HIP's default), not under the sweep's "on": include it
// only there, after gradient_pass.h (sweep_math.h needs the opposite regime and says why).
#pragma once

// ---------------------------------------------------------------------------
// the chain (one wave; lane = parameter)
// ---------------------------------------------------------------------------
template <int PPL>
struct Vd {
  double a[PPL];
};

// MIG = false: a sampler built without chain migration (plans where it cannot
// run: one chain per tile, batch mode, FITOCT_NO_MIGRATE), so the receive loop
// and the donor check cost no registers in the NUTS waves
// SPEC = true: speculative leaves with a helper wave (one chain per tile, no migration)
// MODE_: the kernel's basis mode (MODE_POLY / MODE_ROWS) as a constant, or -1: read P.mode
template <int PPL, int NNP, int FAM, bool MIG = true, bool SPEC = false, int MODE_ = -1>
struct Chain {
  using V = Vd<PPL>;
  static constexpr int VLEN = WAVE * PPL;
  KPc* pp;   // laundered once per action: no kernarg load is hoisted across actions
  AS_LDS ChainScalars* Sp;
  AS_LDS double* Vb;
  AS_LDS double* SUMS;
  AS_LDS double* AUX;   // [0,32): yGP ; [32,64): horseshoe lambda_j * tau
  AS_LDS double* LV;    // [max_depth][NLVL][VLEN]
  AS_LDS double* RNG;   // [max_depth][WAVE]: level l's merge uniforms, one block of 64 merges
  AS_LDS double* MP;
  AS_LDS double* part;
  const AS_LDS double* Kinv;
  // this lane's row of K^-1 (lanes < NNP) held in VGPRs for the two K^-1 matvecs
  // of every leaf (write_mp, finish_grad): same arithmetic, no LDS reads on the
  // NUTS wave's critical path (configs 2 / 5 +2 %).  Not at NNP = 24 (it would spill).
  static constexpr bool KROW = NNP <= 16 && !MIG && MODE_ != MODE_ROWS;
  double krow[KROW ? NNP : 1];
  const AS_LDS double* bv;
  int lane, slot, lc, gid, nct;
  int pix;   // proposal pool region: the chain's (lc); a two-ended producer's own (produce)
  // speculative leaves (the SPEC sampler): always in a tile of one chain (with a helper
  // wave), else while the tile hosts <= P.spec_live live chains (the tail of a launch, when
  // the sweep no longer hides the sampler's latency; this wave then does the helper's part)
  static constexpr bool spec = SPEC;
  bool helped;   // ... with a helper wave (tiles of one or two chains, no migration)
  const AS_LDS int* live = nullptr;   // the tile's live-chain count (kernel-maintained)
  // a speculated leaf's values, kept from leaf_spec to act_spec_book (across the hand-off)
  // (the metric and the next subtree's start are re-read from LDS.)  The migrating
  // sampler, whose migration paths leave no registers to spare, also parks the leaf itself
  // in LDS, in slots dead from leaf_spec to the end of the bookkeeping: q in V_PG and g in
  // V_CA (there is no helper wave, so the next prior part is written only after the
  // bookkeeping), the end-updated p in V_CUR_G (where spec_weight reads it anyway).  No
  // LDS is added: the tile's LDS carve decides how many chains fit (G = 4 at depth 12).
  static constexpr bool KLDS = MIG;
  V k_q, k_pe, k_g;
  // (its lp / sum r^2 stay in Sp->cur_lp / cur_s2 until the bookkeeping)
  int k_dirn, k_dn, k_jn;
  uint32_t k_t;
  // deep speculation (tiles of one or two chains, helped): the helper books leaf k
  // (deep_book) while this wave completes gradient k + 1; this wave waits for booking k
  // (book_done >= book_want) only before it stages leaf k + 2, and reads its outcome from
  // book_res
  bool deep = false;
  AS_LDS double* HX = nullptr;
  volatile AS_LDS int* book_done = nullptr;
  volatile AS_LDS int* book_res = nullptr;
  int book_want = 0;
  // two-ended trajectories (P.bidi, deep tiles): the producer waves' chain areas (slots 1, 2:
  // backward, forward) and the tile's hand-off words BD_*
  // Compiled where it can run: tiles of one chain (deep speculation, spare waves from the
  // start), and migrating tiles in the launch's tail (a chain alone in its tile, with two
  // idle receivers recruited as producers: kernel and receive_chain, P.tail_bidi)
  static constexpr bool kTwoEnded = SPEC;
  bool bidi = false;
  volatile AS_LDS int* bd = nullptr;
  RngKey key;

  __device__ __forceinline__ Chain(KPc& P_, const Lds<PPL>& L, int slot_, int lc_, int lane_, int nct_)
      : pp(&P_), Sp(&L.cs(slot_)), Vb(L.vecs(slot_)), SUMS(L.sums(slot_)), AUX(L.aux(slot_)),
        LV(L.lvls(slot_)), RNG(L.lvls(slot_) + (size_t)P_.max_depth * NLVL * VLEN), MP(L.mp(slot_)),
        part(L.part()), Kinv(L.kinv()), bv(L.bv()),
        lane(lane_), slot(slot_), lc(lc_), nct(nct_) {
    // The chain area's base lives in ONE VGPR for the life of the chain, and the vectors, sums,
    // AUX and levels are constant offsets from it.  As wave-uniform SGPR values the compiler
    // copied the base into a VGPR in front of nearly every ds_ access to a chain scalar
    // (v_mov_b32 from the SGPR: 372 static copies in the headline kernel, 134 now), and kept
    // the four sub-bases in SGPRs of their own, spilled to VGPR lanes and reloaded per action.
    // Opaque to the compiler from here on (it may not treat the value as uniform again); the
    // alignment it could derive from the carve is stated instead, so that the 16-byte LDS reads
    // of AUX / SUMS stay single instructions.  Addresses only: no value changes.
    static_assert(sizeof(ChainScalars) % 16 == 0 && (NVEC * VLEN * 8) % 16 == 0 &&
                      (NSLOT * 8) % 16 == 0 && (NAUX * 8) % 16 == 0 &&
                      Lds<PPL>::head_bytes(1) % 16 == 0 && Lds<PPL>::head_bytes(2) % 16 == 0 &&
                      Lds<PPL>::chain_bytes(1) % 16 == 0 && Lds<PPL>::chain_bytes(2) % 16 == 0,
                  "chain areas are 16-byte aligned");
    asm volatile("" : "+v"(Sp));
    __builtin_assume(((uint32_t)(uintptr_t)Sp & 15u) == 0);
    Vb = (AS_LDS double*)((AS_LDS char*)Sp + sizeof(ChainScalars));
    SUMS = Vb + NVEC * VLEN;
    AUX = SUMS + NSLOT;
    LV = AUX + NAUX;
    gid = Pr().chain_offset + lc;
    pix = lc;
    // tiles of G <= 2 chains: NUTS wave G + c helps chain slot c (tile of one chain: wave 1)
    helped = SPEC && !MIG && P_.G <= 2;
    deep = helped;
    HX = L.hx(L.G <= 2 ? slot_ : 0);
    if (L.G == 3) QX0 = L.qx0();
    bidi = kTwoEnded && !MIG && deep && P_.bidi != 0;
    key = make_key(Pr().seed, (uint32_t)gid);
    if constexpr (KROW) {
      const int r = lane < NNP ? lane : 0;
#pragma unroll
      for (int k = 0; k < NNP; ++k) krow[k] = Kinv[r * NNP + k];
    }
  }
  __device__ __forceinline__ double kinv_row(int k) const {
    if constexpr (KROW) return krow[k];
    else return Kinv[lane * NNP + k];
  }

  __device__ __forceinline__ KPc& Pr() const { return *pp; }
  __device__ __forceinline__ bool is_poly() const {
    return MODE_ >= 0 ? MODE_ == MODE_POLY : Pr().mode == MODE_POLY;
  }
  // two-ended trajectories: producer k's chain area (NUTS slot bd[TW_SLOT + k] of this
  // tile: the chain areas are consecutive, chain_bytes apart), its scalars and vectors
  __device__ __forceinline__ AS_LDS char* parea(int k) const {
    const int sl = __builtin_amdgcn_readfirstlane(bd[TW_SLOT + k]);
    return (AS_LDS char*)Sp + (sl - slot) * Lds<PPL>::chain_bytes(Pr().max_depth);
  }
  __device__ __forceinline__ AS_LDS ChainScalars* psp(int k) const {
    return (AS_LDS ChainScalars*)parea(k);
  }
  __device__ __forceinline__ AS_LDS double* pvb(int k) const {
    return (AS_LDS double*)(parea(k) + sizeof(ChainScalars));
  }
  __device__ __forceinline__ int idx(int s) const { return s * WAVE + lane; }
  __device__ __forceinline__ bool ok(int s) const { return idx(s) < Pr().D; }
  __device__ __forceinline__ AS_LDS double* vec(int v) const { return Vb + v * VLEN; }
  __device__ __forceinline__ const AS_LDS double* QS() const { return Vb + V_QS * VLEN; }
  __device__ __forceinline__ const AS_LDS double* QE() const { return Vb + V_QE * VLEN; }
  __device__ __forceinline__ V ld(int v) const {
    V r;
#pragma unroll
    for (int s = 0; s < PPL; ++s) r.a[s] = vec(v)[idx(s)];
    return r;
  }
  __device__ __forceinline__ void st(int v, const V& x) const {
#pragma unroll
    for (int s = 0; s < PPL; ++s) vec(v)[idx(s)] = x.a[s];
  }
  __device__ __forceinline__ void copyv(int dst, int src) const { st(dst, ld(src)); }
  __device__ __forceinline__ AS_LDS double* lvl(int level, int which) const {
    return LV + ((size_t)level * NLVL + which) * VLEN;
  }
  __device__ __forceinline__ V lld(int level, int which) const {
    V r;
    const AS_LDS double* p = lvl(level, which);
#pragma unroll
    for (int s = 0; s < PPL; ++s) r.a[s] = p[idx(s)];
    return r;
  }
  __device__ __forceinline__ void lst(int level, int which, const V& x) const {
    AS_LDS double* p = lvl(level, which);
#pragma unroll
    for (int s = 0; s < PPL; ++s) p[idx(s)] = x.a[s];
  }
  __device__ __forceinline__ AS_GLB double* pslot(int sl, int which) const {
    // HBM [chain][max_depth+1][NPOOL][VLEN]; recomputed from the parameter block
    // on use (scalar ops) instead of holding a 64-bit pointer across actions
    const size_t base = ((size_t)pix * (Pr().max_depth + 1) + sl) * NPOOL + which;
    return (AS_GLB double*)Pr().stack + base * VLEN;
  }

  __device__ __forceinline__ double kin(const V& p, const V& minv) const {
    double x = 0.0;
#pragma unroll
    for (int s = 0; s < PPL; ++s) x += p.a[s] * minv.a[s] * p.a[s];
    return 0.5 * wave_sum(x);
  }
  // stan::mcmc::base_nuts::compute_criterion on p_sharp = minv .* p (symmetric)
  __device__ __forceinline__ bool crit(const V& pa, const V& pb, const V& rho,
                                       const V& minv) const {
    double x = 0.0, y = 0.0;
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      x += minv.a[s] * pb.a[s] * rho.a[s];
      y += minv.a[s] * pa.a[s] * rho.a[s];
    }
    wave_sum2(x, y);
    return x > 0.0 && y > 0.0;
  }
  // three compute_criterion calls of one merge, reduced together (6 dot products
  // in one interleaved butterfly; the conjunction is order-independent)
  __device__ __forceinline__ bool crit3(const V& a1, const V& b1, const V& r1, const V& a2,
                                        const V& b2, const V& r2, const V& a3, const V& b3,
                                        const V& r3, const V& minv) const {
    // slots 6, 7 pad the transposed reduction with a positive constant (lane 0)
    double x[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, lane == 0 ? 1.0 : 0.0, lane == 0 ? 1.0 : 0.0};
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      x[0] += minv.a[s] * b1.a[s] * r1.a[s];
      x[1] += minv.a[s] * a1.a[s] * r1.a[s];
      x[2] += minv.a[s] * b2.a[s] * r2.a[s];
      x[3] += minv.a[s] * a2.a[s] * r2.a[s];
      x[4] += minv.a[s] * b3.a[s] * r3.a[s];
      x[5] += minv.a[s] * a3.a[s] * r3.a[s];
    }
    return transpose_all_positive8(x, lane);
  }
  __device__ __forceinline__ bool is_log(int k) const { return k < 3 || k >= 3 + Pr().Nn; }
  // parameter k's lane-role record (the tile's block sits after b: a constant offset from Kinv)
  __device__ __forceinline__ const AS_LDS LaneRole* role(int k) const {
    return (const AS_LDS LaneRole*)((const AS_LDS char*)Kinv + Lds<PPL>::KBYTES) + k;
  }

  // ---------------- the point handed to the gradient phase ------------------
  // Stages q, caches its constrained values (QE) and, per family, yGP and the
  // horseshoe scales (AUX), then writes the gradient phase's parameters MP:
  // theta[3] and, per basis mode, yGP (rows) or c = b .* K^-1 yGP (poly).
  // (LDS exchange: on gfx950 a v_readlane assembly of yGP measured 3x slower.)
  __device__ void write_mp(const V& q) const {
    FITOCT_MARK(write_mp);
    long long ts = stamp0();
    const int Nn = Pr().Nn, D = Pr().D;
    const bool poly = is_poly();
    AS_LDS double* qs = vec(V_QS);
    AS_LDS double* qe = vec(V_QE);
#pragma unroll
    for (int s = 0; s < PPL; ++s) qs[idx(s)] = q.a[s];
    wave_order();   // q of every lane visible: the yGP lanes start at once, in parallel with
                    // the constrained values below
    if constexpr (FAM == FAM_HORSESHOE) {
      // Tests/horseShoePrior.stan:30-32 in the exponent: lambda_j tau =
      // r1_l sqrt(r2_l) r1_g sqrt(r2_g) = exp(u1_l + u2_l/2 + u1_g + u2_g/2)
      // The z_j lanes (3 + j) have no constrained value of their own to form, so lambda_j tau
      // is evaluated there: one exp per position serves both, each value through the same
      // function as before, and z_j is the lane's own q.
      const int j = lane - 3;
      const bool zl = (unsigned)j < (unsigned)Nn;
      const int jl = zl ? j : 0;
      const double a1 = qs[5 + Nn + jl], a2 = qs[5 + 2 * Nn + jl];
      const double g1 = qs[3 + Nn], g2 = qs[4 + Nn];
      const double ha = fma(0.5, a2, a1) + fma(0.5, g2, g1);
      double hl = 0.0;
#pragma unroll
      for (int s = 0; s < PPL; ++s) {
        const int k = idx(s);
        const double e = fexp((s == 0 && zl) ? ha : q.a[s]);
        const double ev = (k < D && is_log(k)) ? e : q.a[s];   // (not a z lane's)
        if (s == 0) hl = zl ? e : 0.0;
        qe[k] = ev;
        if (s == 0 && lane < 3) MP[lane] = ev;   // theta for the gradient waves
      }
      const double yv = zl ? q.a[0] * hl : 0.0;
      if ((unsigned)j < (unsigned)NNP) {
        AUX[j] = yv;
        AUX[32 + j] = hl;
        if (!poly) MP[4 + j] = yv;
      }
    } else {
      const int jl = lane < Nn ? lane : 0;
      const double u = qs[3 + jl];
#pragma unroll
      for (int s = 0; s < PPL; ++s) {
        const int k = idx(s);
        const double ev = (k < D && is_log(k)) ? fexp(q.a[s]) : q.a[s];
        qe[k] = ev;
        if (s == 0 && lane < 3) MP[lane] = ev;   // theta for the gradient waves
      }
      double yv = u, hl = 0.0;
      if (lane >= Nn) yv = hl = 0.0;
      if (lane < NNP) {
        AUX[lane] = yv;
        AUX[32 + lane] = hl;
        if (!poly) MP[4 + lane] = yv;
      }
    }
    sub(5, ts);
    if (poly) {  // c_l = b_l (K^-1 yGP)_l ; K^-1 padded to NNP x NNP
      wave_order();
      if (lane < NNP) {
        double c0 = 0.0, c1 = 0.0;   // two chains of FMAs: half the dependent latency
#pragma unroll
        for (int k = 0; k + 1 < NNP; k += 2) {
          c0 = fma(kinv_row(k), AUX[k], c0);
          c1 = fma(kinv_row(k + 1), AUX[k + 1], c1);
        }
        if constexpr ((NNP & 1) != 0) c0 = fma(kinv_row(NNP - 1), AUX[NNP - 1], c0);
        MP[4 + lane] = (c0 + c1) * bv[lane];
      }
    }
    sub(6, ts);
  }

  // The lp / grad completion is split so that everything depending only on the
  // staged position runs while the gradient waves sweep the bins (prior_part,
  // off the critical path), and only a few FMAs per lane remain once the bin
  // sums arrive (lik_part):
  //   grad_k = PG_k + CA_k * S[sidx(k)] + CB_k * famsum,   lp = pr_lp - 0.5 S0 pr_is2
  // with S = the bin sums after finish_grad's transform and famsum = sum_j FW_j S[4+j].
  // Which bin sum lane k's gradient needs: for the horseshoe, whose local scales make it a
  // comparison chain, the byte offset in the lane's role record (LaneRole::soff); the other
  // families' two comparisons stay in registers (the role read moved their kernels past the
  // SGPR-spill ceilings of tests/test_kernel_resources.py).
  __device__ __forceinline__ int sidx(int k) const {
    const int D = Pr().D, Nn = Pr().Nn;
    if (k < 3) return 1 + k;
    if (k == D - 1) return 0;
    if (k < 3 + Nn) return 4 + (k - 3);
    return 0;
  }
  __device__ __forceinline__ const AS_LDS double* sum_at(const AS_LDS double* S, int k,
                                                         int soff) const {
    if constexpr (FAM == FAM_HORSESHOE) return (const AS_LDS double*)((const AS_LDS char*)S + soff);
    else return S + sidx(k);
  }

  __device__ void prior_part() const {
    FITOCT_MARK(prior_part);
    const int D = Pr().D, Nn = Pr().Nn;
    constexpr int fam = FAM;
    const AS_LDS double* qs = QS();
    const AS_LDS double* qe = QE();
    const bool lik = (Pr().prior_PD == 0);
    constexpr bool mono = FAM == FAM_MONO;   // flat theta prior, sigma = 1 (fitMonoExp)
    const double th0 = qe[0], th1 = qe[1], th2 = qe[2];
    const double usig = mono ? 0.0 : qs[D - 1], sig = mono ? 1.0 : qe[D - 1];
    const double is2 = mono ? 1.0 : frcp(sig * sig);
    const double d0 = mono ? 0.0 : th0 - Pr().theta0[0], d1 = mono ? 0.0 : th1 - Pr().theta0[1],
                 d2 = mono ? 0.0 : th2 - Pr().theta0[2];
    const AS_CST double* Si = Pr().S0inv;
    const double Sd0 = Si[0] * d0 + Si[1] * d1 + Si[2] * d2;
    const double Sd1 = Si[3] * d0 + Si[4] * d1 + Si[5] * d2;
    const double Sd2t = Si[6] * d0 + Si[7] * d1 + Si[8] * d2;
    const double iss = Pr().sigma_scale_inv;   // 1 / sigma_scale (host division)
    const double gyf = lik ? th1 * th2 * is2 : 0.0;   // dlp/dyGP_k = gyf * S[4+k]
    // mono-exp with theta_prior = 1: theta_k ~ exponential(tr) (Tests/testGamma.R's model)
    const double tr = mono ? Pr().theta_rate : 0.0;
    double lpc = 0.0;
    if (lane == 0) {
      if (lik) lpc += -(double)Pr().N * usig;
      lpc += -0.5 * (d0 * Sd0 + d1 * Sd1 + d2 * Sd2t) + qs[0] + qs[1] + qs[2];
      if (mono) lpc += -tr * (th0 + th1 + th2);
      if (!mono) lpc += -0.5 * (sig * iss) * (sig * iss) + usig;
    }
    double ysum = 0.0;   // normal family: sum yGP^2
    if (fam == FAM_NORMAL) ysum = wave_sum(lane < Nn ? AUX[lane] * AUX[lane] : 0.0);
    if (fam == FAM_HORSESHOE && lane < Nn) AUX[64 + lane] = gyf * AUX[lane];   // FW_j
    V pg, ca;
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      const int k = idx(s);
      double gk = 0.0, ck = 0.0;
      if (k < D) {
        const double qk = qs[k];
        if (k < 3) {
          // th0 / th1 / th2 by lane.  Horseshoe: the lane's own read of the same word, no
          // selects (in the other families' kernels the read costs spilled SGPRs)
          const double thk = FAM == FAM_HORSESHOE ? qe[k] : (k == 0) ? th0 : (k == 1) ? th1 : th2;
          const double sdk = (k == 0) ? Sd0 : (k == 1) ? Sd1 : Sd2t;
          gk = 1.0 - thk * sdk;
          if (mono) gk -= tr * thk;
          if (lik) ck = (k == 2) ? th1 * is2 : thk * is2;
        } else if (mono) {
          // no other parameter
        } else if (k == D - 1) {
          gk = (lik ? -(double)Pr().N : 0.0) - (sig * iss) * (sig * iss) + 1.0;
          if (lik) ck = is2;
        } else if (fam == FAM_NORMAL) {
          // one reciprocal for the wave (lambda is the same on every lane) instead of an
          // IEEE division per term: no division latency on the sampler's path
          const double lam = qe[3 + Nn], il2 = frcp(lam * lam);
          if (k < 3 + Nn) {
            gk = -qk * il2;
            ck = gyf;
            lpc += -0.5 * qk * qk * il2;
          } else {  // lambda: lam * (-Nn / lam + ysum / lam^3 - rate) + 1
            const double rate = Pr().lambda_rate_eff;
            gk = -(double)Nn + ysum * il2 - rate * lam + 1.0;
            lpc += -(double)Nn * qk - rate * lam + qk;
          }
        } else if (fam == FAM_LASSO) {
          const double ls = Pr().lambda_scale;
          const double sg = (qk > 0.0) ? 1.0 : (qk < 0.0) ? -1.0 : 0.0;
          gk = -ls * sg - 2.0 * ls * qk;
          ck = gyf;
          lpc += -ls * fabs(qk) - ls * qk * qk;
        } else {  // horseshoe (Tests/horseShoePrior.stan:25-43), straight-line over lanes:
          //   z_j      : grad -q              lp -q^2/2
          //   r1 (g, l): grad 1 - e^2         lp -e^2/2 + q          (half-normal + log-Jacobian)
          //   r2 (g, l): grad c (1/e - 1)     lp -c (q + 1/e)        (InvGamma(c, c) + log-Jacobian,
          //                                                         c = 1/2 global, nu/2 local)
          // (which of the three a lane is, its shape c and where its coefficient's scale
          // sits in AUX: the lane's role record)
          const double ek = qe[k];
          const AS_LDS LaneRole* ro = role(k);
          const int kind = ro->kind;
          const bool tz = kind == RK_Z, tr1 = kind == RK_R1;
          const double cc = ro->cc;
          const double e2 = ek * ek, ie = frcp(ek);
          gk = tz ? -qk : tr1 ? 1.0 - e2 : cc * ie - cc;
          lpc += tz ? -0.5 * qk * qk : tr1 ? fma(-0.5, e2, qk) : -cc * (qk + ie);
          const double aw = ro->aw;
          ck = aw * gyf * *(const AS_LDS double*)((const AS_LDS char*)AUX + ro->aoff);
        }
      }
      pg.a[s] = gk;
      ca.a[s] = ck;
    }
    st(V_PG, pg);
    st(V_CA, ca);
    const double lp = wave_sum(lpc);
    if (lane == 0) {
      Sp->pr_lp = lp;
      Sp->pr_is2 = lik ? is2 : 0.0;
    }
  }

  // After the sweep: reduce the 8 waves' partial sums and complete lp / grad from
  // what prior_part left in LDS.  s0 = sum of squared residuals.  Two LDS round
  // trips: bin sums out (-> the K^-1 transform), transformed sums out (-> every
  // parameter lane); famsum is reduced straight from the transform's lanes.
  __device__ double finish_grad(V& g, double& s0) const {
    FITOCT_MARK(finish_grad);
    const int Nn = Pr().Nn, D = Pr().D;
    const bool lik = (Pr().prior_PD == 0), poly = is_poly();
    const V pg = ld(V_PG), ca = ld(V_CA);   // issued up front, used last
    const double pr_lp = Sp->pr_lp, pr_is2 = Sp->pr_is2;
    const double fw = (FAM == FAM_HORSESHOE && lane < Nn) ? AUX[64 + lane] : 0.0;
    double famsum = 0.0, S0 = 0.0;
    double srow[PPL];   // basis rows (MODE_ROWS): the bin sum each lane's gradient needs
    int soff[PPL];      // ... and its byte offset among the sums (the lane's role record)
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      srow[s] = 0.0;
      soff[s] = FAM == FAM_HORSESHOE ? role(idx(s))->soff : 0;
    }
    if (lik && !poly) {
      // each lane sums the partials of the sums it needs itself, in the SUMS path's order
      // (bitwise the same values): no store / wait / read-back before the gradient
      const AS_LDS double* pw = part + slot * NGW * NSLOT;
      double v = 0.0;
      const int jv = lane < NNP ? 4 + lane : 0;
#pragma unroll
      for (int w = 0; w < NGW; ++w) {
        S0 += pw[w * NSLOT];
        if (FAM == FAM_HORSESHOE) v += pw[w * NSLOT + jv];
#pragma unroll
        for (int s = 0; s < PPL; ++s)
          srow[s] += *sum_at(pw + w * NSLOT, idx(s), soff[s]);
      }
      if (FAM == FAM_HORSESHOE) famsum = wave_sum(lane < Nn ? fw * v : 0.0);
    } else if (lik) {
      double sl = 0.0;
      if (lane < 4 + NNP) {
#pragma unroll
        for (int w = 0; w < NGW; ++w) sl += part[(slot * NGW + w) * NSLOT + lane];
        if (poly && lane >= 4) sl *= bv[lane - 4];   // b .* M  (B^T h = K^-1 (b .* M))
        SUMS[lane] = sl;
      }
      S0 = rl(sl, 0);
      wave_order();
      double v = 0.0;
      if (lane < NNP) {
        if (poly) {
          double v1 = 0.0;
#pragma unroll
          for (int m = 0; m + 1 < NNP; m += 2) {
            v = fma(kinv_row(m), SUMS[4 + m], v);
            v1 = fma(kinv_row(m + 1), SUMS[4 + m + 1], v1);
          }
          if constexpr ((NNP & 1) != 0) v = fma(kinv_row(NNP - 1), SUMS[4 + NNP - 1], v);
          v += v1;
          SUMS[4 + lane] = v;   // every lane's reads above precede this store
        } else {
          v = SUMS[4 + lane];
        }
      }
      if (FAM == FAM_HORSESHOE) famsum = wave_sum(lane < Nn ? fw * v : 0.0);
      wave_order();
    }
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      const int k = idx(s);
      double gk = pg.a[s];
      if (lik && k < D) {
        gk = fma(ca.a[s], poly ? *sum_at(SUMS, k, soff[s]) : srow[s], gk);
        if (FAM == FAM_HORSESHOE && (k == 3 + Nn || k == 4 + Nn))
          gk = fma(k == 3 + Nn ? 1.0 : 0.5, famsum, gk);
      }
      g.a[s] = gk;
    }
    s0 = lik ? S0 : NAN;
    double lp = fma(-0.5 * S0, pr_is2, pr_lp);
    if ((lik && !(S0 <= DBL_MAX)) || !(fabs(lp) <= DBL_MAX)) lp = -INFINITY;
    return lp;
  }

  // ------------------------------ randomness --------------------------------
  __device__ V momentum(uint32_t tag, uint32_t c0, uint32_t c3, const V& minv) const {
    V p;
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      const int k = idx(s);
      double n0, n1;
      normal_pair(key, c0, tag, (uint32_t)(k >> 1), c3, n0, n1);
      const double n = (k & 1) ? n1 : n0;
      p.a[s] = (k < Pr().D) ? n / sqrt(minv.a[s]) : 0.0;
    }
    return p;
  }

  // =========================================================================
  // The sampler as a flat action machine.  Every action appears once in the
  // code and returns the next action; A_YIELD hands the position staged by
  // A_WRITE_MP to the gradient waves.  Values crossing actions live in LDS.
  // =========================================================================
  enum Act : int {
    A_YIELD = 0, A_GRAD, A_INIT_STATE, A_INIT_START, A_INIT_STEP, A_SS_BEGIN, A_SS_TRIAL,
    A_SS_STEP, A_SS_FINISH, A_START_TRANSITION, A_BEGIN_SUBTREE, A_LEAF, A_END_TREE,
    A_NEXT_TRANSITION, A_FINISH, A_LEAPFROG, A_WRITE_MP, A_PRIOR,
    // the speculative path (leaf_spec): A_SPEC_STAGED yields a staged position for the
    // kernel to enqueue and hand to the helper wave, A_SPEC_BOOK then does the leaf's
    // bookkeeping and yields A_SPEC_WAIT (wait for the sweep and the helper, then A_GRAD)
    // or A_SPEC_DISCARD (the trajectory ended: drain both, then A_END_TREE)
    A_SPEC_STAGED, A_SPEC_BOOK, A_SPEC_WAIT, A_SPEC_DISCARD,
    // two-ended trajectories: the producers and the helper grow and book the whole tree;
    // the chain's wave waits for its end, then A_END_TREE
    A_BIDI_TREE
  };
  enum LeafBook : int { LB_MID = 0, LB_NEXT = 1, LB_END = 2 };

  __device__ __forceinline__ int uni(int x) const { return __builtin_amdgcn_readfirstlane(x); }
  // diagnostic sub-action stamps (profiling build + FITOCT_STAMPS): cycles since t
  // into prof[0][PROF_SUB + i]
  __device__ __forceinline__ void sub(int i, long long& t) const {
    if (kProfile && Pr().stamps) {
      wave_fence();
      const long long n = (long long)__builtin_amdgcn_s_memtime();
      if (lane == 0) Sp->prof[0][PROF_SUB + i] += n - t;
      t = n;
    }
  }
  __device__ __forceinline__ long long stamp0() const {
    return (kProfile && Pr().stamps) ? (long long)__builtin_amdgcn_s_memtime() : 0;
  }

  // runs while the gradient waves sweep the staged position: the position-only
  // part of lp / grad, and the uniforms the coming leaf's merges will consume
  __device__ int act_prior() {
    FITOCT_MARK(act_prior);
    const bool tree = uni(Sp->state) == ST_TREE;
    if (deep) {   // the tree uniforms are the booking helper's (it owns the rings and Sp->leaf)
      prior_part();
      return A_YIELD;
    }
    prior_and_uniforms(tree, uni(Sp->depth), uni(Sp->leaf), (uint32_t)uni(Sp->t));
    return A_YIELD;
  }
  // The position-only part of lp / grad, and (tree building, leaf j of the subtree of
  // depth d) the uniforms that leaf's merges will consume.  Run by the chain's NUTS
  // wave (A_PRIOR) or, for a speculated leaf, by the tile's helper wave.
  __device__ void prior_and_uniforms(const bool tree, const int d, const int j,
                                     const uint32_t t) const {
    long long ts = stamp0();
    prior_part();
    sub(7, ts);
    if (tree) tree_uniforms(d, j, t);
  }
  // the uniforms leaf j of the subtree of depth d will consume in its merges (and the
  // top-level merge's, for the subtree's last leaf)
  __device__ void tree_uniforms(const int d, const int j, const uint32_t t) const {
    FITOCT_MARK(tree_uniforms);   // (what follows the inlined prior_part)
    {
      // Leaf j completes the merges of levels l < nm (trailing ones of j).
      // The k-th level-l merge of a subtree sits at leaf (k + 1) 2^(l+1) - 1; each
      // level keeps a ring of the uniforms of 64 consecutive merges, refilled a block
      // at a time by one Philox per lane (same counters as one draw per merge, so the
      // same numbers), i.e. one Philox pass per 64 merges instead of per leaf.
      const int nm = min(d, (int)__builtin_ctz(~(unsigned)j));
      for (int l = 0; l < nm; ++l) {
        const int blk = (j >> (l + 1)) >> 6;
        if (uni(Sp->u_blk[l]) != blk) {
          const int jj = ((((blk << 6) + lane) + 1) << (l + 1)) - 1;   // may pass the subtree's end: unused
          RNG[l * WAVE + lane] = uniform(key, t, TAG_MERGE | ((uint32_t)l << 8) | ((uint32_t)d << 16),
                                         (uint32_t)jj, 0u);
          if (lane == 0) Sp->u_blk[l] = blk;
        }
      }
      if (lane == WAVE - 1 && j == (1 << d) - 1)
        Sp->u_top = uniform(key, t, TAG_TOP, (uint32_t)d, 0u);
    }
  }

  // a gradient arrived for CUR_Q: complete lp / grad, store them, dispatch
  __device__ int act_grad() {
    FITOCT_MARK(act_grad);
    long long ts = stamp0();
    const int stt = uni(Sp->state);
    V g;
    double s0;
    if (stt == ST_TREE) {
      // the leaf's position, momentum and the metric are read while the bin sums reduce
      const V q = ld(V_CUR_Q), p = ld(V_CUR_P), minv = ld(V_MINV);
      const double lp = finish_grad(g, s0);
      FITOCT_MARK(act_grad_store);   // (what follows the inlined finish_grad)
      sub(4, ts);
      st(V_CUR_G, g);
      Sp->cur_lp = lp;
      Sp->cur_s2 = s0;
      if constexpr (spec) {   // per leaf: plain and speculative leaves leave the same state
        if (deep) {
          // leaf k - 1 is being booked by the helper: its outcome decides whether this leaf
          // belongs to the trajectory, and it sets the tree coordinates this leaf continues from
          const int w = wait_booking();
          if (w < 0) return A_FINISH;
          if (w == LB_END) return A_END_TREE;   // this (speculated) leaf is discarded
          return leaf_spec(q, p, g, minv, lp, s0);
        }
        if (helped || uni(__atomic_load_n(live, __ATOMIC_RELAXED)) <= Pr().spec_live)
          return leaf_spec(q, p, g, minv, lp, s0);
      }
      return leaf(q, p, g, minv, lp, s0);
    }
    const double lp = finish_grad(g, s0);
    sub(4, ts);
    st(V_CUR_G, g);
    Sp->cur_lp = lp;
    Sp->cur_s2 = s0;
    return stt == ST_STEPSIZE ? A_SS_STEP : A_INIT_STEP;
  }

  __device__ int act_init_state() {
    FITOCT_MARK(act_init_state);
    V one, zero;
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      one.a[s] = ok(s) ? 1.0 : 0.0;
      zero.a[s] = 0.0;
    }
    Sp->prof[lane >> 5][lane & 31] = 0;
#pragma unroll 1
    for (int v = 0; v < NVEC; ++v) st(v, zero);
    if (Pr().init_minv) {   // warm restart (fitoct_plan_set_init): the chain's metric
      V m;
#pragma unroll
      for (int s = 0; s < PPL; ++s)
        m.a[s] = ok(s) ? Pr().init_minv[(size_t)lc * Pr().D + idx(s)] : 0.0;
      st(V_MINV, m);
    } else {
      st(V_MINV, one);
    }
    if (lane < NSLOT) SUMS[lane] = 0.0;
    AUX[lane] = 0.0;
    Sp->status = 0;
    Sp->leapfrogs = 0;
    const double eps0 = Pr().init_eps ? Pr().init_eps[lc] : Pr().stepsize0;
    Sp->eps = eps0;
    Sp->mu = log(10.0 * eps0);
    Sp->da_counter = 0;
    Sp->s_bar = 0.0;
    Sp->x_bar = 0.0;
    // stan::mcmc::windowed_adaptation::set_window_params + restart
    const int W = Pr().warmup;
    int ib = Pr().init_buffer, tb = Pr().term_buffer, bw = Pr().base_window;
    Sp->win_on = (W >= 20) ? 1 : 0;
    if (W >= 20 && ib + bw + tb > W) {
      ib = (int)(0.15 * W);
      tb = (int)(0.1 * W);
      bw = W - (ib + tb);
    }
    Sp->init_buf = ib;
    Sp->term_buf = tb;
    Sp->win_counter = 0;
    Sp->win_size = bw;
    Sp->win_next = ib + bw - 1;
    Sp->wf_n = 0;
    Sp->t = 0;
    Sp->ss_window = 0;
    Sp->depth = 0;
    Sp->pool_used = 0;
    Sp->init_attempt = 0;
    return A_INIT_START;
  }

  __device__ int act_init_start() {
    FITOCT_MARK(act_init_start);
    const int Nn = Pr().Nn, attempt = uni(Sp->init_attempt);
    V q;
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      const int k = idx(s);
      double base = 0.0, w = 0.0;
      if (k < 3) {
        base = log(Pr().theta0[k]);
        w = 0.025;
      } else if (k < 3 + Nn) {
        w = 0.05;
      } else if (k < Pr().D) {
        w = 0.25;
        if (FAM == FAM_NORMAL && k == 3 + Nn) base = -log(Pr().lambda_rate_eff);
      }
      const double u = uniform(key, (uint32_t)attempt, TAG_INIT, (uint32_t)k, 0u);
      q.a[s] = (k < Pr().D) ? base + Pr().init_radius * w * (2.0 * u - 1.0) : 0.0;
      if (Pr().init_q && k < Pr().D) q.a[s] = Pr().init_q[(size_t)lc * Pr().D + k];   // warm restart
    }
    st(V_CUR_Q, q);
    Sp->state = ST_INIT;
    return A_WRITE_MP;
  }

  __device__ int act_init_step() {
    FITOCT_MARK(act_init_step);
    const V g = ld(V_CUR_G);
    double bad = 0.0;
#pragma unroll
    for (int s = 0; s < PPL; ++s)
      if (ok(s) && !(fabs(g.a[s]) <= DBL_MAX)) bad = 1.0;
    bad = wave_sum(bad);
    if (!(Sp->cur_lp > -INFINITY) || bad != 0.0) {
      if (Sp->init_attempt + 1 >= 100 || Pr().init_q) {   // a given start is not retried
        Sp->status = ERR_INIT;
        return A_FINISH;
      }
      Sp->init_attempt += 1;
      return A_INIT_START;
    }
    copyv(V_SMP_Q, V_CUR_Q);
    st(V_SMP_G, g);
    Sp->smp_lp = Sp->cur_lp;
    Sp->smp_s2 = Sp->cur_s2;
    return Pr().adapt ? A_SS_BEGIN : A_START_TRANSITION;
  }

  // --------------------- leapfrog (stan expl_leapfrog) -----------------------
  // A_LEAPFROG: begin_update_p + update_q from CUR with step Sp->lf_e
  __device__ int act_leapfrog() {
    FITOCT_MARK(act_leapfrog);
    return leapfrog_stage(ld(V_CUR_Q), ld(V_CUR_P), ld(V_CUR_G), ld(V_MINV), Sp->lf_e);
  }
  // begin_update_p + update_q from (q, p, g) in registers, then stage the new position
  // for the gradient waves (write_mp): the whole path to the next sweep without an LDS
  // round trip or an action dispatch
  __device__ int leapfrog_stage(V q, V p, const V& g, const V& minv, const double e) const {
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      p.a[s] = fma(0.5 * e, g.a[s], p.a[s]);        // p -= e/2 dphi/dq
      q.a[s] = fma(e, minv.a[s] * p.a[s], q.a[s]);  // q += e M^-1 p
    }
    st(V_CUR_P, p);
    st(V_CUR_Q, q);
    write_mp(q);
    FITOCT_MARK(leapfrog_staged);   // (what follows the inlined write_mp is the caller's)
    return A_YIELD;
  }
  __device__ int act_write_mp() {
    FITOCT_MARK(act_write_mp);
    long long ts = stamp0();
    write_mp(ld(V_CUR_Q));
    return A_YIELD;
  }
  // end_update_p with the gradient that just arrived
  __device__ V finish_leapfrog(double e) const {
    V p = ld(V_CUR_P);
    const V g = ld(V_CUR_G);
#pragma unroll
    for (int s = 0; s < PPL; ++s) p.a[s] = fma(0.5 * e, g.a[s], p.a[s]);
    st(V_CUR_P, p);
    return p;
  }

  // ----------------- base_hmc::init_stepsize as actions ----------------------
  __device__ int act_ss_begin() {
    FITOCT_MARK(act_ss_begin);
    const double eps = Sp->eps;
    if (eps == 0.0 || eps > 1e7 || isnan(eps)) return A_SS_FINISH;  // skipped like Stan
    Sp->ss_trial = 0;
    Sp->state = ST_STEPSIZE;
    return A_SS_TRIAL;
  }
  __device__ int act_ss_trial() {
    FITOCT_MARK(act_ss_trial);
    const V minv = ld(V_MINV);
    const V p = momentum(TAG_SSMOM, (uint32_t)uni(Sp->ss_window), (uint32_t)uni(Sp->ss_trial), minv);
    Sp->ss_H0 = -Sp->smp_lp + kin(p, minv);
    copyv(V_CUR_Q, V_SMP_Q);
    copyv(V_CUR_G, V_SMP_G);
    st(V_CUR_P, p);
    Sp->lf_e = Sp->eps;
    return A_LEAPFROG;
  }
  __device__ int act_ss_step() {
    FITOCT_MARK(act_ss_step);
    const V p = finish_leapfrog(Sp->eps);
    double h = -Sp->cur_lp + kin(p, ld(V_MINV));
    if (isnan(h)) h = INFINITY;
    const double dH = Sp->ss_H0 - h;
    const double L08 = -0.22314355131420976;  // log(0.8)
    if (Sp->ss_trial == 0) {
      Sp->ss_dir = (dH > L08) ? 1 : -1;
      Sp->ss_trial = 1;
      return A_SS_TRIAL;
    }
    if ((Sp->ss_dir == 1 && !(dH > L08)) || (Sp->ss_dir == -1 && !(dH < L08))) return A_SS_FINISH;
    Sp->eps = (Sp->ss_dir == 1) ? 2.0 * Sp->eps : 0.5 * Sp->eps;
    if (Sp->eps > 1e7 || Sp->eps == 0.0 || Sp->ss_trial > 2000) {
      Sp->status = ERR_NUMERIC;
      return A_FINISH;
    }
    Sp->ss_trial += 1;
    return A_SS_TRIAL;
  }
  __device__ int act_ss_finish() {
    FITOCT_MARK(act_ss_finish);
    if (uni(Sp->ss_window) == 0) return A_START_TRANSITION;
    // adapt_diag_e_nuts::transition after a metric update
    Sp->mu = log(10.0 * Sp->eps);
    Sp->da_counter = 0;
    Sp->s_bar = 0.0;
    Sp->x_bar = 0.0;
    return A_NEXT_TRANSITION;
  }

  // ------------------------------ transition --------------------------------
  __device__ int act_start_transition() {
    FITOCT_MARK(act_start_transition);
    Sp->state = ST_TREE;
    Sp->eps_used = Sp->eps;
    const V minv = ld(V_MINV);
    const V p = momentum(TAG_MOM, (uint32_t)uni(Sp->t), 0u, minv);
    Sp->H0 = -Sp->smp_lp + kin(p, minv);
    Sp->smp_h = Sp->H0;   // energy__ if no leaf replaces the initial point
    const V q = ld(V_SMP_Q), g = ld(V_SMP_G);
    st(V_E0_Q, q); st(V_E0_P, p); st(V_E0_G, g);
    st(V_E1_Q, q); st(V_E1_P, p); st(V_E1_G, g);
    Sp->end_lp[0] = Sp->end_lp[1] = Sp->smp_lp;
    Sp->end_s2[0] = Sp->end_s2[1] = Sp->smp_s2;
    st(V_RHO, p);
    Sp->lsw_m = 0.5;   // weight of the initial point: exp(0) = 0.5 * 2^1
    Sp->lsw_e = 1;
    Sp->n_leapfrog = 0;
    Sp->sum_metro = 0.0;
    Sp->depth = 0;
    Sp->divergent = 0;
    Sp->pool_used = 0;
    return A_BEGIN_SUBTREE;
  }

  __device__ int act_begin_subtree() {
    FITOCT_MARK(act_begin_subtree);
    if constexpr (kTwoEnded) {
      if (bidi) return bidi_begin();   // reached at depth 0 only: the helper books from there on
      if (MIG && tail_ready() && tail_claim()) return bidi_begin();   // (the chain's own wave books, kernel)
    }
    const int d = uni(Sp->depth);
    const double u = uniform(key, (uint32_t)uni(Sp->t), TAG_DIR, (uint32_t)d, 0u);
    const int dir = (u > 0.5) ? 1 : 0;
    Sp->dir = dir;
    const int eq = dir ? V_E1_Q : V_E0_Q;
    const V qe = ld(eq), pe = ld(eq + 1), ge = ld(eq + 2), minv = ld(V_MINV);
    st(V_PNEAR, pe);
    st(V_CUR_G, ge);
    Sp->cur_lp = Sp->end_lp[dir];
    Sp->cur_s2 = Sp->end_s2[dir];
    Sp->leaf = 0;
    Sp->sub_metro = 0.0;
    if (lane < MAXDEPTH) Sp->u_blk[lane] = -1;   // merge uniforms are per subtree (depth d)
    const double e = dir ? Sp->eps_used : -Sp->eps_used;
    Sp->lf_e = e;
    return leapfrog_stage(qe, pe, ge, minv, e);   // act_leapfrog + act_write_mp
  }

  // proposal pool: at most max_depth + 1 live slots (stack records + the running
  // subtree).  `used` is the slot bitmask, kept in registers by the caller.
  __device__ int pool_put(unsigned& used, const V& q, const V& g, double lp, double s2,
                          double h) const {
    const int sl = __builtin_ctz(~used);
    used |= 1u << sl;
    AS_GLB double* dq = pslot(sl, P_Q);
    AS_GLB double* dg = pslot(sl, P_G);
#pragma unroll
    for (int s = 0; s < PPL; ++s) {   // HBM stores, never waited on; D lanes only (the
      if (ok(s)) {                    // padding lanes of q, g are 0: top_merge reads 0)
        dq[idx(s)] = q.a[s];
        dg[idx(s)] = g.a[s];
      }
    }
    Sp->pool_lp[sl] = lp;
    Sp->pool_s2[sl] = s2;
    Sp->pool_h[sl] = h;
    return sl;
  }

  // one leaf of base_nuts::build_tree, followed by every merge it completes and,
  // when the subtree of depth d is complete, the top-level merge of the transition.
  // Chain scalars are read once into registers and written back once, so the
  // action costs a handful of LDS round trips instead of one per field.
  // Reached from act_grad (state ST_TREE) with the leaf's q, p (begin-updated), the
  // gradient just completed, the metric, lp and sum r^2 in registers.  A leaf inside
  // the subtree continues straight into the next leapfrog and stages its position
  // (act_leapfrog + act_write_mp with the same arithmetic, no LDS round trip or
  // dispatch between them).
  __device__ int leaf(const V& q, V p, const V& g, const V& minv, const double cur_lp,
                      const double cur_s2) {
    const double e = Sp->lf_e;
#pragma unroll
    for (int s = 0; s < PPL; ++s) p.a[s] = fma(0.5 * e, g.a[s], p.a[s]);   // end_update_p
    switch (leaf_book(q, p, g, minv, cur_lp, cur_s2)) {
      case LB_MID: return leapfrog_stage(q, p, g, minv, e);   // act_leapfrog + act_write_mp
      case LB_NEXT: return A_BEGIN_SUBTREE;
      default: return A_END_TREE;
    }
  }

  // Speculative leaf (tiles hosting one chain, with a helper wave): the next leaf's
  // position depends only on this leaf's (q, p, g) -- or, after the last leaf of a
  // subtree, on the trajectory end the next subtree grows from, whose direction is a
  // pre-addressed uniform -- not on the merges and U-turn checks.  So the next position
  // is staged and handed to the gradient waves first; the helper wave computes its prior
  // part while this wave does the bookkeeping of leaf j.  If the bookkeeping ends the
  // trajectory, the speculated sweep is drained and discarded.  Same arithmetic on the
  // same values as the plain path: draws are bitwise identical.
  __device__ int leaf_spec(const V& q, const V& p, const V& g, const V& minv, const double cur_lp,
                           const double cur_s2) {
    FITOCT_MARK(leaf_spec);
    const double e = Sp->lf_e;
    const int d = uni(Sp->depth), j = uni(Sp->leaf);
    const bool last = j == (1 << d) - 1;
    if (last && d + 1 >= Pr().max_depth) {   // the tree ends here at the latest: no speculation
      if (deep) tree_uniforms(d, j, (uint32_t)uni(Sp->t));   // the helper did not draw them
      return leaf(q, p, g, minv, cur_lp, cur_s2);
    }
    V pe;
#pragma unroll
    for (int s = 0; s < PPL; ++s) pe.a[s] = fma(0.5 * e, g.a[s], p.a[s]);   // end_update_p
    const int dir = uni(Sp->dir);
    int dirn = dir, dn = d, jn = j + 1;
    double en = e;
    V qs = q, ps = pe, gs = g;
    const uint32_t t = (uint32_t)uni(Sp->t);
    if (last) {   // act_begin_subtree of depth d + 1
      dn = d + 1;
      jn = 0;
      dirn = (uniform(key, t, TAG_DIR, (uint32_t)dn, 0u) > 0.5) ? 1 : 0;
      if (dirn != dir) {
        const int eq = dirn ? V_E1_Q : V_E0_Q;
        qs = ld(eq);
        ps = ld(eq + 1);
        gs = ld(eq + 2);
      }
      en = dirn ? Sp->eps_used : -Sp->eps_used;
    }
    leapfrog_stage(qs, ps, gs, minv, en);
    FITOCT_MARK(leaf_spec_park);
    if (deep) {   // hand leaf k to the booking helper (deep_book)
#pragma unroll
      for (int s = 0; s < PPL; ++s) {
        HX[idx(s)] = q.a[s];
        HX[VLEN + idx(s)] = pe.a[s];
        HX[2 * VLEN + idx(s)] = g.a[s];
      }
      if (lane == 0) {
        HX[3 * VLEN] = cur_lp;
        HX[3 * VLEN + 1] = cur_s2;
      }
      return A_SPEC_STAGED;
    }
    // for the helper (spec_weight): the booked leaf's end-updated momentum, in CUR_G's
    // slot (while a tree grows nothing reads CUR_G; begin_subtree rewrites it)
    st(V_CUR_G, pe);   // (its lp is Sp->cur_lp, set by act_grad)
    if constexpr (KLDS) {
      st(V_PG, q);
      st(V_CA, g);
    } else {
      k_q = q; k_pe = pe; k_g = g;
    }

    k_dirn = dirn; k_dn = dn; k_jn = jn; k_t = t;
    return A_SPEC_STAGED;   // the kernel enqueues the position and posts the helper
  }
  // the bookkeeping of the speculated leaf, while its successor is being swept
  __device__ int act_spec_book() {
    FITOCT_MARK(act_spec_book);
    spec_weight();   // (act_spec_book runs only without a helper wave: tiles of several chains)
    const int r = KLDS ? leaf_book_split(ld(V_PG), ld(V_CUR_G), ld(V_CA), ld(V_MINV), Sp->cur_lp,
                                         Sp->cur_s2)
                       : leaf_book_split(k_q, k_pe, k_g, ld(V_MINV), Sp->cur_lp, Sp->cur_s2);
    FITOCT_MARK(act_spec_book_next);   // (what follows the inlined leaf_book_split)
    if (r == LB_NEXT) {   // the rest of act_begin_subtree (the top merge set depth d + 1)
      // the next subtree grows from trajectory end k_dirn: the far end if the direction
      // changed (untouched by the top merge), else the end the top merge just set to this
      // leaf -- in both cases the (p, g) leaf_spec staged the next leapfrog from
      Sp->dir = k_dirn;
      const int eq = k_dirn ? V_E1_Q : V_E0_Q;
      st(V_PNEAR, ld(eq + 1));
      st(V_CUR_G, ld(eq + 2));
      Sp->cur_lp = Sp->end_lp[k_dirn];
      Sp->cur_s2 = Sp->end_s2[k_dirn];
      Sp->leaf = 0;
      Sp->sub_metro = 0.0;
      if (lane < MAXDEPTH) Sp->u_blk[lane] = -1;
      Sp->lf_e = k_dirn ? Sp->eps_used : -Sp->eps_used;
    }
    // without a helper, the next position's prior part follows the bookkeeping here
    if (r != LB_END) prior_and_uniforms(true, k_dn, k_jn, k_t);
    return r == LB_END ? A_SPEC_DISCARD : A_SPEC_WAIT;
  }

  // ---- the two steps of a leaf's booking that have one copy for every path (sub_leaf,
  // leaf_book, leaf_book_split, book_leaf): the leaf's energy and the push of a level's
  // record.  (The U-turn checks and the multinomial merge are still written out per path.)
  // a leaf's Hamiltonian -lp + K(p); NaN counts as +inf (a divergence)
  __device__ __forceinline__ double leaf_h(const double lp, const V& p, const V& minv) const {
    double h = -lp + kin(p, minv);
    if (isnan(h)) h = INFINITY;
    return h;
  }
  // ... and its multinomial weight exp(H0 - h), booked for leaf_book_split (spec_h, spec_w*)
  __device__ __forceinline__ void spec_weight(const double lp, const V& pe, const V& minv) const {
    const double h = leaf_h(lp, pe, minv);
    const XF w = xf_exp(Sp->H0 - h);
    Sp->spec_h = h;
    Sp->spec_wm = w.m;
    Sp->spec_we = w.e;
  }
  // push the running subtree T as level l's record (the init subtree of level l + 1); its
  // proposal, if it is still the leaf (q, g) itself (Tprop < 0), goes to the pool
  __device__ __forceinline__ void push_level(const int l, const V& Tpb, const V& p, const V& Trho,
                                             const XF Tw, const int Tprop, unsigned& used,
                                             const V& q, const V& g, const double cur_lp,
                                             const double cur_s2, const double h) const {
    lst(l, K_PBEG, Tpb);
    lst(l, K_PEND, p);
    lst(l, K_RHO, Trho);
    Sp->st_w_m[l] = Tw.m;
    Sp->st_w_e[l] = Tw.e;
    Sp->st_prop[l] = (Tprop < 0) ? pool_put(used, q, g, cur_lp, cur_s2, h) : Tprop;
  }

  // Deep speculation, run by the helper wave: the whole bookkeeping of the leaf the chain's
  // wave handed over in HX (act_spec_book's work with the weight computed here), with the
  // coordinates (depth, leaf, direction, step) in Sp advanced for the next leaf exactly as
  // act_spec_book advances them -- the chain's wave reads them only after waiting for this
  // booking.  Same operations on the same values as the plain path: same draws.
  __device__ __forceinline__ int deep_book() {
    V q, pe, g;
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      q.a[s] = HX[idx(s)];
      pe.a[s] = HX[VLEN + idx(s)];
      g.a[s] = HX[2 * VLEN + idx(s)];
    }
    return book_leaf(q, pe, g, HX[3 * VLEN], HX[3 * VLEN + 1]);
  }
  // ... of a leaf given by value (deep_book: from HX; bidi_book: from a producer's ring)
  __device__ __forceinline__ int book_leaf(const V& q, const V& pe, const V& g, const double lp, const double s2) {
    const int d = uni(Sp->depth), j = uni(Sp->leaf);
    const uint32_t t = (uint32_t)uni(Sp->t);
    tree_uniforms(d, j, t);
    const V minv = ld(V_MINV);
    spec_weight(lp, pe, minv);
    const int r = leaf_book_split(q, pe, g, minv, lp, s2);
    if (r == LB_NEXT) {   // act_begin_subtree's bookkeeping for the subtree of depth d + 1
      const int dirn = (uniform(key, t, TAG_DIR, (uint32_t)(d + 1), 0u) > 0.5) ? 1 : 0;
      Sp->dir = dirn;
      st(V_PNEAR, ld((dirn ? V_E1_Q : V_E0_Q) + 1));
      Sp->leaf = 0;
      Sp->sub_metro = 0.0;
      if (lane < MAXDEPTH) Sp->u_blk[lane] = -1;
      Sp->lf_e = dirn ? Sp->eps_used : -Sp->eps_used;
    }
    return r;
  }
  // the chain's wave: wait for the booking of the previous leaf (if one is outstanding);
  // its LB_* outcome, or -1 on a timeout (status set)
  __device__ int wait_booking() {
    if (book_want == 0) return LB_MID;
    long long ts = stamp0();   // profiling build: sub-stamp 8 = this wave's stall on the booking
    Patience w;
    while (*book_done < book_want) {
      if (w.expired(LEAF_WAIT_TICKS)) {
        Sp->status = ERR_TIMEOUT;
        return -1;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    wave_fence();   // the booking's LDS writes are visible from here
    sub(8, ts);
    const int r = uni(*book_res);
    book_want = 0;
    return r;
  }

  // ---------------- two-ended trajectories (P.bidi; tiles of one chain) ----------------
  // Stan's trajectory grows by doublings in directions drawn per depth (TAG_DIR); a doubling of
  // depth d builds a subtree of 2^d leaves from the trajectory end in its direction, and the
  // subtrees grown in one direction form one unbroken leapfrog chain from the transition's
  // start.  Everything base_nuts::build_tree does inside a subtree -- each leaf's weight and
  // divergence test, the multinomial merges, the U-turn checks of its levels, the subtree's
  // proposal -- depends only on that subtree's leaves.  So two producer waves (one per
  // direction, slots 1 and 2) build the subtrees of their direction whole, each in its own
  // chain area (levels, merge uniforms, proposal pool), at most BIDI_LOOK doublings past the
  // one booked, and the chain's wave books the trajectory level only, in tree order, from one
  // record per subtree (sub_publish): the top-level multinomial merge, the new end, the
  // trajectory-level U-turn checks.  The same operations on the same values as the one-ended
  // path (the acceptance statistic is summed per subtree on every path), so the same draws;
  // a transition takes about as long as its longer end, and the booking no longer paces it.
  enum SubRes : int { SL_MID = 0, SL_DONE = 1, SL_END = 2 };
  enum SubFlag : int { SR_VALID = 1, SR_DIVERGENT = 2 };
  // A subtree record: RVEC vectors -- the proposal's q and g, the end's (last leaf's)
  // momentum, the subtree's begin momentum and momentum sum -- and scalars RS_*.  Record m of
  // end s sits in slot m % RSLOTS: in a tile of one chain two slots per end (Lds::qx0, after
  // the hand-off slots), in a migrating tile (or at two parameters per lane) one, in vectors of
  // the producer's own area that a producer never uses (V_E1_Q .. V_SMP_G; the scalars in
  // V_RHO's).  Record m is written once the booking has taken record m - RSLOTS.
  static constexpr int RVEC = 5, RSLOTS = (MIG || PPL > 1) ? 1 : 2;
  enum RecVec : int { RV_SQ = 0, RV_SG, RV_EP, RV_PB, RV_RHO };
  enum RecSc : int { RS_SLP = 0, RS_SS2, RS_SH, RS_TWM, RS_METRO, RS_TWE, RS_N, RS_FLAGS, RS_DEPTH,
                     RS_N_ };
  AS_LDS double* QX0 = nullptr;   // the tile's record slots (tiles of one chain)
  __device__ __forceinline__ AS_LDS double* rvec(int s, int m) const {
    if constexpr (RSLOTS == 1) return pvb(s) + V_E1_Q * VLEN;
    else return QX0 + (size_t)(2 * s + (m & 1)) * Lds<PPL>::QX_DOUBLES;
  }
  __device__ __forceinline__ AS_LDS double* rsc(int s, int m) const {
    if constexpr (RSLOTS == 1) return pvb(s) + V_RHO * VLEN;
    else return rvec(s, m) + RVEC * VLEN;
  }
  __device__ __forceinline__ V pld(const AS_LDS double* base, int v) const {
    V r;
#pragma unroll
    for (int s = 0; s < PPL; ++s) r.a[s] = base[v * VLEN + idx(s)];
    return r;
  }
  // a migrating tile's chain, at the start of a transition (depth 0): two-ended when the tile
  // hosts one live chain, two idle receivers of the tile have become
  // producers and no other chain of the tile is growing a tree with them (TW_BUSY, claimed
  // by tail_claim, released when the tree is booked)
  __device__ __forceinline__ bool tail_ready() const {
    const int lv = uni(__atomic_load_n(live, __ATOMIC_RELAXED));
    return Pr().tail_bidi != 0 && uni(Sp->depth) == 0 && uni(bd[TW_JOIN]) >= 2 && lv == 1 &&
           uni(bd[TW_BUSY]) == 0;
  }
  __device__ __forceinline__ bool tail_claim() const {
    int ok = 0;
    if (lane == 0) ok = atomicCAS((int*)&bd[TW_BUSY], 0, 1) == 0;
    return uni(__shfl(ok, 0)) != 0;
  }
  // The chain's wave: book transition g's trajectory level in Stan's tree order from the
  // producers' subtree records (base_nuts::transition: the loop over depths; top_merge and
  // leaf_book's trajectory check on the record's values).  LB_END, with the status
  // ERR_TIMEOUT if a producer's record never came (a fault)
  // profiling build: this wave's cycles waiting for records / booking, subtrees booked
  long long pf_wait = 0, pf_busy = 0, pf_n = 0;
  template <class Idle>
  __device__ __forceinline__ int bidi_book_tree(const int g, Idle&& idle) {
    const uint32_t t = (uint32_t)uni(Sp->t);
    const V minv = ld(V_MINV);
    int m0 = 0, m1 = 0;
    for (;;) {
      const long long pt0 = kProfile ? (long long)__builtin_amdgcn_s_memtime() : 0;
      const int d = uni(Sp->depth);
      const int s = (uniform(key, t, TAG_DIR, (uint32_t)d, 0u) > 0.5) ? 1 : 0;
      const int m = s ? m1 : m0;
      bool lost = false;
      Patience wl;   // one subtree of the longer end: bounded by the whole tree's bound
      for (;;) {     // record m of end s published for this transition
        const int w = bd[BD_PROD + s];
        if ((w >> 16) == g && (w & 0xFFFF) > m) break;
        if (bd[BD_GEN] != g || wl.expired(MIG_WAIT_TICKS)) {   // never, short of a fault
          lost = true;
          break;
        }
        if (!idle()) __builtin_amdgcn_s_sleep(1);
      }
      if (lost) {
        Sp->status = ERR_TIMEOUT;
        return LB_END;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   // the record after its count
      const long long pt1 = kProfile ? (long long)__builtin_amdgcn_s_memtime() : 0;
      const AS_LDS double* RV = rvec(s, m);
      const AS_LDS double* SC = rsc(s, m);
      const int fl = uni((int)SC[RS_FLAGS]);
      Sp->n_leapfrog = uni(Sp->n_leapfrog) + uni((int)SC[RS_N]);
      Sp->sum_metro = Sp->sum_metro + SC[RS_METRO];
      if (fl & SR_DIVERGENT) Sp->divergent = 1;
      bool persist = false;
      if (fl & SR_VALID) {
        // top_merge: the sample, the trajectory's weight, the end, the depth
        const XF Tw{SC[RS_TWM], uni((int)SC[RS_TWE])};
        const XF Ww{Sp->lsw_m, Sp->lsw_e};
        const double u_top = uniform(key, t, TAG_TOP, (uint32_t)d, 0u);
        const bool take = xf_gt(Tw, Ww) || xf_u_below(u_top, Tw, Ww);
        if (take) {
          st(V_SMP_Q, pld(RV, RV_SQ));
          st(V_SMP_G, pld(RV, RV_SG));
          Sp->smp_lp = SC[RS_SLP];
          Sp->smp_s2 = SC[RS_SS2];
          Sp->smp_h = SC[RS_SH];
        }
        const XF Wn = xf_add(Ww, Tw);
        Sp->lsw_m = Wn.m;
        Sp->lsw_e = Wn.e;
        Sp->depth = d + 1;
        // the trajectory-level U-turn checks (leaf_book's, at the subtree's last leaf)
        const V pend = pld(RV, RV_EP), Tpb = pld(RV, RV_PB), Trho = pld(RV, RV_RHO);
        const int ef = s ? V_E1_P : V_E0_P;
        const V far = ld(s ? V_E0_P : V_E1_P), near = ld(ef), rho = ld(V_RHO);
        V rtot, rx, ry;
#pragma unroll
        for (int k = 0; k < PPL; ++k) {
          rtot.a[k] = rho.a[k] + Trho.a[k];
          rx.a[k] = rho.a[k] + Tpb.a[k];
          ry.a[k] = Trho.a[k] + near.a[k];
        }
        persist = crit3(far, pend, rtot, far, Tpb, rx, near, pend, ry, minv);
        st(ef, pend);
        st(V_RHO, rtot);
      }
      if (s) ++m1;
      else ++m0;
      wave_publish();   // the record's reads are done before the slot is released
      if (lane == 0) bd[BD_CONS + s] = m + 1;
      if (kProfile) {
        pf_wait += pt1 - pt0;
        pf_busy += (long long)__builtin_amdgcn_s_memtime() - pt1;
        ++pf_n;
      }
      if (!persist || d + 1 >= Pr().max_depth) return LB_END;
    }
  }
  // the chain's wave, at depth 0 of a transition: the start to both producers' slots, then
  // the transition's number (BD_GEN) releases them
  __device__ int bidi_begin() {
    const uint32_t t = (uint32_t)uni(Sp->t);
    const V q = ld(V_E0_Q), p = ld(V_E0_P), g = ld(V_E0_G), minv = ld(V_MINV);   // E0 = E1 = start
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      AS_LDS double* const pv = pvb(k);
      AS_LDS ChainScalars* const ps = psp(k);
#pragma unroll
      for (int s = 0; s < PPL; ++s) {
        pv[V_E0_Q * VLEN + idx(s)] = q.a[s];
        pv[V_E0_P * VLEN + idx(s)] = p.a[s];
        pv[V_E0_G * VLEN + idx(s)] = g.a[s];
        pv[V_MINV * VLEN + idx(s)] = minv.a[s];
      }
      if (lane == 0) {
        ps->eps_used = Sp->eps_used;
        ps->t = (int)t;
        ps->H0 = Sp->H0;
      }
    }
    if (lane == 0) {
      bd[BD_CONS] = 0;
      bd[BD_CONS + 1] = 0;
      bd[TW_CHAIN] = slot;   // the producers read the booked depth and the key from these
      bd[TW_LC] = lc;
    }
    wave_publish();   // every store above lands before the transition's number
    if (lane == 0) {
      bd[BD_GEN] = (bd[BD_GEN] & BD_GEN_MASK) % BD_GEN_MASK + 1;
      atomicAdd(Pr().bidi_count, 1ULL);
    }
    return A_BIDI_TREE;
  }
  // ---- the producer's side (run on the producer's own chain area) ----
  // a subtree of depth d begins (act_begin_subtree's bookkeeping, counts of this subtree)
  __device__ void sub_begin(const int d) {
    Sp->depth = d;
    Sp->leaf = 0;
    Sp->sub_metro = 0.0;
    Sp->n_leapfrog = 0;
    Sp->pool_used = 0;
    Sp->divergent = 0;
    if (lane < MAXDEPTH) Sp->u_blk[lane] = -1;
  }
  // One leaf of the producer's subtree (base_nuts::build_tree below the trajectory level):
  // leaf_book's weight, divergence test, merges, U-turn checks and push -- the same operations
  // on the same values.  At the subtree's last leaf (SL_DONE) its weight, proposal, begin
  // momentum and momentum sum are returned for sub_publish.  (q, p, g): the leaf with its
  // end-updated momentum.
  __device__ __forceinline__ int sub_leaf(const V& q, const V& p, const V& g, const V& minv, const double cur_lp,
                          const double cur_s2, XF& Tw_o, int& Tprop_o, V& Tpb_o, V& Trho_o,
                          double& h_o) {
    const double H0 = Sp->H0;
    const double sub_metro0 = Sp->sub_metro;
    const int d = uni(Sp->depth), j = uni(Sp->leaf), nlf = uni(Sp->n_leapfrog);
    unsigned used = (unsigned)uni(Sp->pool_used);
    Sp->n_leapfrog = nlf + 1;
    tree_uniforms(d, j, (uint32_t)uni(Sp->t));   // this leaf's merge uniforms
    const double h = leaf_h(cur_lp, p, minv);
    const double wl = H0 - h;
    const XF wleaf = xf_exp(wl);
    Sp->sub_metro = sub_metro0 + ((wl > 0.0) ? 1.0 : xf_val(wleaf));
    if (h - H0 > 1000.0) {   // divergent: the transition ends here
      Sp->divergent = 1;
      return SL_END;
    }
    V Tpb = p, Trho = p;
    XF Tw = wleaf;
    int Tprop = -1;   // -1: the current leaf; else a pool slot
#pragma unroll 1
    for (int l = 0; l < d; ++l) {
      if (((j >> l) & 1) == 0) {   // push T as the init subtree of level l+1
        push_level(l, Tpb, p, Trho, Tw, Tprop, used, q, g, cur_lp, cur_s2, h);
        break;
      }
      // merge init I = level l with final T (base_nuts::build_tree at depth l+1)
      const V Ipb = lld(l, K_PBEG), Ipe = lld(l, K_PEND), Irho = lld(l, K_RHO);
      const XF Iw{Sp->st_w_m[l], Sp->st_w_e[l]};
      const double um = RNG[l * WAVE + ((j >> (l + 1)) & (WAVE - 1))];
      const int Iprop = uni(Sp->st_prop[l]);
      const XF Sw = xf_add(Iw, Tw);
      const bool take_final = xf_gt(Tw, Sw) || xf_u_below(um, Tw, Sw);
      if (take_final) {
        used &= ~(1u << Iprop);
      } else {
        if (Tprop >= 0) used &= ~(1u << Tprop);
        Tprop = Iprop;
      }
      V rsub, rx, ry;
#pragma unroll
      for (int s = 0; s < PPL; ++s) {
        rsub.a[s] = Irho.a[s] + Trho.a[s];
        rx.a[s] = Irho.a[s] + Tpb.a[s];
        ry.a[s] = Trho.a[s] + Ipe.a[s];
      }
      const bool okc = crit3(Ipb, p, rsub, Ipb, Tpb, rx, Ipe, p, ry, minv);
      Tpb = Ipb;
      Trho = rsub;
      Tw = Sw;
      if (!okc) {
        Sp->pool_used = (int)used;
        return SL_END;
      }
    }
    Sp->pool_used = (int)used;
    if (j != (1 << d) - 1) {
      Sp->leaf = j + 1;
      return SL_MID;
    }
    Tw_o = Tw;
    Tprop_o = Tprop;
    Tpb_o = Tpb;
    Trho_o = Trho;
    h_o = h;
    return SL_DONE;
  }
  // record m of end s for the booking (its slot free: record m - RSLOTS was booked).
  // flags 0 / SR_DIVERGENT: an invalid subtree (only its counts matter)
  __device__ __forceinline__ void sub_publish(const int s, const int m, const int flags,
                                              const XF Tw, const int Tprop, const V& Tpb,
                                              const V& Trho, const V& q, const V& pe,
                                              const V& g, const double lp, const double s2,
                                              const double h) {
    AS_LDS double* const RV = rvec(s, m);
    AS_LDS double* const SC = rsc(s, m);
    if (flags & SR_VALID) {
      V sq = q, sg = g;
      double slp = lp, ss2 = s2, sh = h;
      if (Tprop >= 0) {   // the proposal is a pool slot (top_merge's read)
        const AS_GLB double* pq = pslot(Tprop, P_Q);
        const AS_GLB double* pg = pslot(Tprop, P_G);
#pragma unroll
        for (int k = 0; k < PPL; ++k) {
          sq.a[k] = ok(k) ? pq[idx(k)] : 0.0;
          sg.a[k] = ok(k) ? pg[idx(k)] : 0.0;
        }
        slp = Sp->pool_lp[Tprop];
        ss2 = Sp->pool_s2[Tprop];
        sh = Sp->pool_h[Tprop];
      }
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        RV[RV_SQ * VLEN + idx(k)] = sq.a[k];
        RV[RV_SG * VLEN + idx(k)] = sg.a[k];
        RV[RV_EP * VLEN + idx(k)] = pe.a[k];
        RV[RV_PB * VLEN + idx(k)] = Tpb.a[k];
        RV[RV_RHO * VLEN + idx(k)] = Trho.a[k];
      }
      if (lane == 0) {
        SC[RS_SLP] = slp;
        SC[RS_SS2] = ss2;
        SC[RS_SH] = sh;
        SC[RS_TWM] = Tw.m;
        SC[RS_TWE] = (double)Tw.e;
      }
    }
    if (lane == 0) {
      SC[RS_METRO] = Sp->sub_metro;
      SC[RS_N] = (double)Sp->n_leapfrog;
      SC[RS_FLAGS] = (double)flags;
      SC[RS_DEPTH] = (double)Sp->depth;
    }
  }

  // run by the helper wave for the leaf being booked: its Hamiltonian and multinomial
  // weight (leaf_book's first lines: leaf_h)
  __device__ void spec_weight() const {
    const V pe = ld(V_CUR_G), minv = ld(V_MINV);   // leaf_spec staged the momentum there
    spec_weight(Sp->cur_lp, pe, minv);
  }

  // base_nuts::transition's merge of the completed subtree of depth d (final weight Tw,
  // proposal Tprop: -1 = the leaf (q, p, g) itself, else a pool slot) into the trajectory
  // grown in direction dir: the new trajectory end, depth d + 1, the multinomial choice
  // of the sample (u_top drawn by act_prior) and the trajectory weight.  Shared by
  // leaf_book and leaf_book_split.
  __device__ __forceinline__ void top_merge(const V& q, const V& p, const V& g, const double cur_lp,
                                            const double cur_s2, const double h, const XF Tw,
                                            const int Tprop, unsigned used, const int dir,
                                            const int d) const {
    const XF Ww{Sp->lsw_m, Sp->lsw_e};
    const double u_top = Sp->u_top;
    const int eq = dir ? V_E1_Q : V_E0_Q;
    st(eq, q);
    st(eq + 1, p);
    st(eq + 2, g);
    Sp->end_lp[dir] = cur_lp;
    Sp->end_s2[dir] = cur_s2;
    Sp->depth = d + 1;
    const bool take = xf_gt(Tw, Ww) || xf_u_below(u_top, Tw, Ww);
    if (take) {
      if (Tprop < 0) {
        st(V_SMP_Q, q);
        st(V_SMP_G, g);
        Sp->smp_lp = cur_lp;
        Sp->smp_s2 = cur_s2;
        Sp->smp_h = h;
      } else {
        const AS_GLB double* sq = pslot(Tprop, P_Q);
        const AS_GLB double* sg = pslot(Tprop, P_G);
        V q2, g2;
#pragma unroll
        for (int s = 0; s < PPL; ++s) {
          q2.a[s] = ok(s) ? sq[idx(s)] : 0.0;
          g2.a[s] = ok(s) ? sg[idx(s)] : 0.0;
        }
        st(V_SMP_Q, q2);
        st(V_SMP_G, g2);
        Sp->smp_lp = Sp->pool_lp[Tprop];
        Sp->smp_s2 = Sp->pool_s2[Tprop];
        Sp->smp_h = Sp->pool_h[Tprop];
      }
    }
    if (Tprop >= 0) used &= ~(1u << Tprop);
    Sp->pool_used = (int)used;
    const XF Wn = xf_add(Ww, Tw);
    Sp->lsw_m = Wn.m;
    Sp->lsw_e = Wn.e;
  }

  // leaf_book for the speculative path, split so that the weight can come from the
  // helper wave: first every U-turn check the leaf completes (they need momenta only:
  // the running subtree's begin momentum and momentum sum follow the levels'
  // records whatever the multinomial choices), including the trajectory-level check
  // when the subtree ends; then, with the helper's weight, the divergence test, the
  // multinomial merges up to the first failing check, the push and the top-level
  // merge.  Same operations on the same values as leaf_book, so the same outcome.
  __device__ int leaf_book_split(const V& q, const V& p, const V& g, const V& minv,
                                 const double cur_lp, const double cur_s2) {
    FITOCT_MARK(act_leaf_split);
    long long ts = stamp0();
    const double H0 = Sp->H0;
    const double sub_metro0 = Sp->sub_metro;
    const int d = uni(Sp->depth), j = uni(Sp->leaf), nlf = uni(Sp->n_leapfrog);
    unsigned used = (unsigned)uni(Sp->pool_used);
    Sp->n_leapfrog = nlf + 1;
    const int nm = min(d, (int)__builtin_ctz(~(unsigned)j));   // merges this leaf completes
    const bool last = j == (1 << d) - 1;
    // phase A: U-turn checks
    V Tpb = p, Trho = p;
    int fail = nm;
#pragma unroll 1
    for (int l = 0; l < nm; ++l) {
      const V Ipb = lld(l, K_PBEG), Ipe = lld(l, K_PEND), Irho = lld(l, K_RHO);
      V rsub, rx, ry;
#pragma unroll
      for (int s = 0; s < PPL; ++s) {
        rsub.a[s] = Irho.a[s] + Trho.a[s];
        rx.a[s] = Irho.a[s] + Tpb.a[s];
        ry.a[s] = Trho.a[s] + Ipe.a[s];
      }
      const bool okc = crit3(Ipb, p, rsub, Ipb, Tpb, rx, Ipe, p, ry, minv);
      Tpb = Ipb;
      Trho = rsub;
      if (!okc) {
        fail = l;
        break;
      }
    }
    const int dir = uni(Sp->dir);
    V rtot;
    bool persist = false;
    if (last && fail == nm) {
      const V far = ld(dir ? V_E0_P : V_E1_P), near = ld(V_PNEAR), rho = ld(V_RHO);
      V rx, ry;
#pragma unroll
      for (int s = 0; s < PPL; ++s) {
        rtot.a[s] = rho.a[s] + Trho.a[s];
        rx.a[s] = rho.a[s] + Tpb.a[s];
        ry.a[s] = Trho.a[s] + near.a[s];
      }
      persist = crit3(far, p, rtot, far, Tpb, rx, near, p, ry, minv);
    }
    sub(2, ts);
    // phase B: the leaf's weight (book_leaf's, or this wave's own: act_spec_book)
    const double h = Sp->spec_h, wl = H0 - h;
    const XF wleaf{Sp->spec_wm, uni(Sp->spec_we)};
    const double sm = sub_metro0 + ((wl > 0.0) ? 1.0 : xf_val(wleaf));
    Sp->sub_metro = sm;
    sub(1, ts);
    if (h - H0 > 1000.0) {   // divergent: the transition ends here
      Sp->divergent = 1;
      Sp->sum_metro += sm;
      return LB_END;
    }
    XF Tw = wleaf;
    int Tprop = -1;   // -1: the current leaf (CUR); else a pool slot
    const int nmerge = fail < nm ? fail + 1 : nm;
#pragma unroll 1
    for (int l = 0; l < nmerge; ++l) {
      const XF Iw{Sp->st_w_m[l], Sp->st_w_e[l]};
      const double um = RNG[l * WAVE + ((j >> (l + 1)) & (WAVE - 1))];
      const int Iprop = uni(Sp->st_prop[l]);
      const XF Sw = xf_add(Iw, Tw);
      const bool take_final = xf_gt(Tw, Sw) || xf_u_below(um, Tw, Sw);
      if (take_final) {
        used &= ~(1u << Iprop);
      } else {
        if (Tprop >= 0) used &= ~(1u << Tprop);
        Tprop = Iprop;
      }
      Tw = Sw;
    }
    if (fail < nm) {
      Sp->pool_used = (int)used;
      Sp->sum_metro += sm;
      return LB_END;
    }
    if (nm < d) {   // push the running subtree as the init subtree of level nm + 1
      push_level(nm, Tpb, p, Trho, Tw, Tprop, used, q, g, cur_lp, cur_s2, h);
    }
    sub(0, ts);
    if (!last) {
      Sp->pool_used = (int)used;
      Sp->leaf = j + 1;
      return LB_MID;
    }
    // the subtree of depth d is complete and valid: top-level merge (base_nuts::transition)
    top_merge(q, p, g, cur_lp, cur_s2, h, Tw, Tprop, used, dir, d);
    Sp->sum_metro += sm;
    st(V_RHO, rtot);
    sub(3, ts);
    if (!persist || d + 1 >= Pr().max_depth) return LB_END;
    return LB_NEXT;
  }

  // one leaf of base_nuts::build_tree with the momentum already end-updated: weight,
  // divergence, every merge it completes and, when the subtree of depth d is complete,
  // the top-level merge of the transition.  Returns LB_MID (leaf j + 1 of this subtree
  // is next), LB_NEXT (a subtree of depth d + 1 is next) or LB_END.
  __device__ int leaf_book(const V& q, const V& p, const V& g, const V& minv, const double cur_lp,
                           const double cur_s2) {
    FITOCT_MARK(act_leaf);
    long long ts = stamp0();
    const double H0 = Sp->H0;
    const double sub_metro0 = Sp->sub_metro;
    const int d = uni(Sp->depth), j = uni(Sp->leaf), nlf = uni(Sp->n_leapfrog);
    unsigned used = (unsigned)uni(Sp->pool_used);
    Sp->n_leapfrog = nlf + 1;
    const double h = leaf_h(cur_lp, p, minv);
    sub(0, ts);
    const double wl = H0 - h;
    const XF wleaf = xf_exp(wl);
    // (Stan sums these over the trajectory's leaves in order; here per subtree, then the
    // subtrees' sums in tree order: a reassociation of the same terms, so that two-ended
    // trajectories, whose subtrees are booked by their producers, give the same bits)
    const double sm = sub_metro0 + ((wl > 0.0) ? 1.0 : xf_val(wleaf));
    Sp->sub_metro = sm;
    sub(1, ts);
    if (h - H0 > 1000.0) {   // divergent: the transition ends here
      Sp->divergent = 1;
      Sp->sum_metro += sm;
      return LB_END;
    }

    V Tpb = p, Trho = p;
    XF Tw = wleaf;
    int Tprop = -1;   // -1: the current leaf (CUR); else a pool slot
#pragma unroll 1
    for (int l = 0; l < d; ++l) {
      if (((j >> l) & 1) == 0) {   // push T as the init subtree of level l+1
        push_level(l, Tpb, p, Trho, Tw, Tprop, used, q, g, cur_lp, cur_s2, h);
        break;
      }
      // merge init I = level l with final T (base_nuts::build_tree at depth l+1)
      const V Ipb = lld(l, K_PBEG), Ipe = lld(l, K_PEND), Irho = lld(l, K_RHO);
      const XF Iw{Sp->st_w_m[l], Sp->st_w_e[l]};
      const double um = RNG[l * WAVE + ((j >> (l + 1)) & (WAVE - 1))];   // drawn by act_prior
      const int Iprop = uni(Sp->st_prop[l]);
      const XF Sw = xf_add(Iw, Tw);
      const bool take_final = xf_gt(Tw, Sw) || xf_u_below(um, Tw, Sw);
      if (take_final) {
        used &= ~(1u << Iprop);
      } else {
        if (Tprop >= 0) used &= ~(1u << Tprop);
        Tprop = Iprop;
      }
      V rsub, rx, ry;
#pragma unroll
      for (int s = 0; s < PPL; ++s) {
        rsub.a[s] = Irho.a[s] + Trho.a[s];
        rx.a[s] = Irho.a[s] + Tpb.a[s];
        ry.a[s] = Trho.a[s] + Ipe.a[s];
      }
      const bool okc = crit3(Ipb, p, rsub, Ipb, Tpb, rx, Ipe, p, ry, minv);
      Tpb = Ipb;
      Trho = rsub;
      Tw = Sw;
      if (!okc) {
        Sp->pool_used = (int)used;
        Sp->sum_metro += sm;
        return LB_END;
      }
    }
    sub(2, ts);
    if (j != (1 << d) - 1) {
      Sp->pool_used = (int)used;
      Sp->leaf = j + 1;
      return LB_MID;
    }
    // the subtree of depth d is complete and valid: top-level merge (base_nuts::transition)
    const int dir = uni(Sp->dir);
    top_merge(q, p, g, cur_lp, cur_s2, h, Tw, Tprop, used, dir, d);
    Sp->sum_metro += sm;
    const V far = ld(dir ? V_E0_P : V_E1_P), near = ld(V_PNEAR), rho = ld(V_RHO);
    V rtot, rx, ry;
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      rtot.a[s] = rho.a[s] + Trho.a[s];
      rx.a[s] = rho.a[s] + Tpb.a[s];
      ry.a[s] = Trho.a[s] + near.a[s];
    }
    const bool persist = crit3(far, p, rtot, far, Tpb, rx, near, p, ry, minv);
    st(V_RHO, rtot);
    sub(3, ts);
    if (!persist || d + 1 >= Pr().max_depth) return LB_END;
    return LB_NEXT;
  }

  // Draw records are written once and never read by the kernel: streaming (non-temporal)
  // stores, so the draws stream through L2 instead of evicting the proposal pools, whose
  // lines are rewritten at every other leaf (config 3: L2->memory writes 6.6x the draws
  // with ordinary stores, profiles/r03_pmc_traffic_config3.json).
  static __device__ __forceinline__ void st_draw(AS_GLB double* p, double v) {
    __builtin_nontemporal_store(v, p);
  }
  __device__ void write_draw(double accept, double energy) const {
    const int t = Sp->t, W = Pr().warmup;
    if (t < W && !Pr().save_warmup) return;
    const int it = Pr().save_warmup ? t : t - W;
    AS_GLB double* rec = (AS_GLB double*)Pr().draws + ((size_t)lc * Pr().iters_saved + it) * Pr().ncols;
    const V q = ld(V_SMP_Q);
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      const int k = idx(s);
      if (k < Pr().D) st_draw(&rec[7 + k], is_log(k) ? exp(q.a[s]) : q.a[s]);
    }
    if (lane < 8) {
      double v;
      switch (lane) {
        case 0: v = Sp->smp_lp; break;
        case 1: v = accept; break;
        case 2: v = Sp->eps_used; break;
        case 3: v = (double)Sp->depth; break;
        case 4: v = (double)Sp->n_leapfrog; break;
        case 5: v = (double)Sp->divergent; break;
        case 6: v = energy; break;
        default: v = (Pr().prior_PD == 0) ? Sp->smp_s2 / (double)Pr().N : NAN; break;
      }
      st_draw(&rec[lane < 7 ? lane : 7 + Pr().D], v);
    }
  }

  __device__ int act_end_tree() {
    FITOCT_MARK(act_end_tree);
    const double accept = Sp->sum_metro / (double)Sp->n_leapfrog;
    // energy__ = H(z_sample) (base_nuts::transition), the sample leaf's own -lp + K(p):
    // the same operations on the same values as -smp_lp + kin(p_sample)
    const double energy = Sp->smp_h;
    write_draw(accept, energy);
    Sp->leapfrogs += Sp->n_leapfrog;
    if (uni(Sp->t) < Pr().warmup && Pr().adapt) {
      learn_stepsize(accept);
      if (learn_variance()) {
        Sp->ss_window += 1;
        return A_SS_BEGIN;
      }
    }
    return A_NEXT_TRANSITION;
  }

  // stan::mcmc::stepsize_adaptation::learn_stepsize
  __device__ void learn_stepsize(double adapt_stat) {
    Sp->da_counter += 1;
    const double cnt = (double)Sp->da_counter;
    adapt_stat = adapt_stat > 1.0 ? 1.0 : adapt_stat;
    const double eta = 1.0 / (cnt + Pr().t0);
    Sp->s_bar = (1.0 - eta) * Sp->s_bar + eta * (Pr().adapt_delta - adapt_stat);
    const double x = Sp->mu - Sp->s_bar * sqrt(cnt) / Pr().gamma;
    const double x_eta = pow(cnt, -Pr().kappa);
    Sp->x_bar = (1.0 - x_eta) * Sp->x_bar + x_eta * x;
    Sp->eps = exp(x);
  }

  // stan::mcmc::var_adaptation::learn_variance + windowed_adaptation
  __device__ bool learn_variance() {
    const int W = Pr().warmup, cnt = uni(Sp->win_counter);
    const int tb = Sp->term_buf;
    if (Sp->win_on && cnt >= Sp->init_buf && cnt < W - tb && cnt != W) {
      Sp->wf_n += 1;
      const double n = (double)Sp->wf_n;
      const V q = ld(V_SMP_Q);
      V m = ld(V_WF_M), m2 = ld(V_WF_M2);
#pragma unroll
      for (int s = 0; s < PPL; ++s) {
        const double delta = q.a[s] - m.a[s];
        m.a[s] += delta / n;
        m2.a[s] += (q.a[s] - m.a[s]) * delta;
      }
      st(V_WF_M, m);
      st(V_WF_M2, m2);
    }
    if (Sp->win_on && cnt == Sp->win_next && cnt != W) {
      // compute_next_window
      const int last = W - tb - 1;
      if (Sp->win_next != last) {
        Sp->win_size *= 2;
        Sp->win_next = cnt + Sp->win_size;
        if (Sp->win_next != last) {
          const int boundary = Sp->win_next + 2 * Sp->win_size;
          if (boundary >= W - tb) Sp->win_next = last;
        }
      }
      const double n = (double)Sp->wf_n;
      V var = ld(V_MINV);
      const V m2 = ld(V_WF_M2);
      V zero;
#pragma unroll
      for (int s = 0; s < PPL; ++s) {
        zero.a[s] = 0.0;
        if (ok(s)) {
          if (Sp->wf_n > 1) var.a[s] = m2.a[s] / (n - 1.0);
          var.a[s] = (n / (n + 5.0)) * var.a[s] + 1e-3 * (5.0 / (n + 5.0));
        }
      }
      st(V_MINV, var);
      st(V_WF_M, zero);
      st(V_WF_M2, zero);
      Sp->wf_n = 0;
      Sp->win_counter = cnt + 1;
      return true;
    }
    Sp->win_counter = cnt + 1;
    return false;
  }

  __device__ int act_next_transition() {
    FITOCT_MARK(act_next_transition);
    Sp->t += 1;
    const int t = uni(Sp->t);
    // transitions done, for fitoct_plan_poll (replaces rstan's stan.log progress)
    if (Pr().progress != nullptr && lane == 0) host_st(Pr().progress + lc, t);
    if (t == Pr().warmup && Pr().adapt && Pr().warmup > 0) Sp->eps = exp(Sp->x_bar);  // complete_adaptation
    if (t >= Pr().warmup + Pr().samples) return A_FINISH;
    // fitoct_plan_cancel: stop at a transition boundary (checked every 8th transition)
    if (Pr().cancel != nullptr && (t & 7) == 0 && uni(host_ld(Pr().cancel)) != 0) {
      Sp->status = ERR_CANCELLED;
      return A_FINISH;
    }
    // a transition boundary: the chain's whole state is its LDS image (current
    // sample, metric, adaptation); hand it to an idle tile if this one is crowded
    if (MIG && Pr().mig != nullptr && t + 2 < Pr().warmup + Pr().samples && try_donate()) {
      Sp->state = ST_MOVED;
      return A_YIELD;
    }
    return A_START_TRANSITION;
  }

  // Work balance (the kernel ends with its slowest tile): a chain in a tile
  // hosting L chains moves to a posted free slot of a tile hosting <= L-2, if
  // any.  Its draws do not change: a chain's arithmetic is the same in every
  // tile of the launch (same bin-to-lane layout) and its random numbers are
  // addressed by (global chain id, iteration).
  __device__ bool try_donate() {
    KPc& P = Pr();
    const MigView M(P.mig, P.mig_tiles);
    if (uni(g_load(&M.hdr[MIG_WAITING])) <= 0) return false;
    const int me = blockIdx.x, T = P.mig_tiles;
    const int my = uni(g_load(&M.load[me]));
    if (my < 2) return false;
    int best = 0x7FFFFFFF;
    for (int i = lane; i < T; i += WAVE)
      if (g_load(&M.fmask[i]) != 0) best = min(best, (g_load(&M.load[i]) << 16) | i);
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) best = min(best, __shfl_xor(best, o));
    best = uni(best);
    if (best == 0x7FFFFFFF || (best >> 16) > my - 2) return false;
    const int tt = best & 0xFFFF;
    int slot = -1;
    if (lane == 0) {
      const int f = g_load(&M.fmask[tt]);
      if (f != 0) {
        const int b = __builtin_ctz(f);
        if (g_cas(&M.fmask[tt], f, f & ~(1 << b))) slot = b;
      }
    }
    slot = __shfl(slot, 0);
    slot = uni(slot);
    if (slot < 0) return false;
    if (lane == 0) {
      g_add(&M.load[tt], 1);
      g_add(&M.load[me], -1);
      g_add(&M.hdr[MIG_WAITING], -1);
      g_add(&M.hdr[MIG_MOVES], 1);
    }
    image_out(P.mig_img + (size_t)(tt * GMAX + slot) * P.mig_img_words);
    // one wave-wide release (the L2 write-back of every lane's image stores) publishes
    // the image to the receiver's XCD; the mailbox store itself is then relaxed
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane == 0)
      __hip_atomic_store((int*)&M.mbox[tt * GMAX + slot], lc + 1, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    return true;
  }
  // the chain's LDS state at a transition boundary (scalars, vectors, sums, aux;
  // the tree levels are dead between transitions) <-> a global image
  __device__ void image_out(double* dst) const {
    const AS_LDS double* src = (const AS_LDS double*)Sp;
    for (int i = lane; i < Pr().mig_img_words; i += WAVE) ((AS_GLB double*)dst)[i] = src[i];
  }

  __device__ int act_finish() {
    FITOCT_MARK(act_finish);
    Sp->state = ST_DONE;
    const V q = ld(V_SMP_Q), minv = ld(V_MINV);
#pragma unroll
    for (int s = 0; s < PPL; ++s) {
      const int k = idx(s);
      if (k < Pr().D) {
        if (Pr().fin_q) ((AS_GLB double*)Pr().fin_q)[(size_t)lc * Pr().D + k] = q.a[s];
        if (Pr().fin_minv) ((AS_GLB double*)Pr().fin_minv)[(size_t)lc * Pr().D + k] = minv.a[s];
      }
    }
    if (lane == 0) {
      if (Pr().fin_eps) ((AS_GLB double*)Pr().fin_eps)[lc] = Sp->eps;
      if (Pr().chain_status) ((AS_GLB int*)Pr().chain_status)[lc] = Sp->status;
      if (Pr().leapfrogs) ((AS_GLB long long*)Pr().leapfrogs)[lc] = Sp->leapfrogs;
    }
    return A_YIELD;
  }

  // run actions until the chain yields a position to the gradient waves (or finishes)
  __device__ __forceinline__ int run(int a) {
    for (;;) {
      FITOCT_MARK(dispatch);
      a = uni(a);
      // opaque per action: no jump threading across actions, and no address or
      // kernarg load hoisted out of the action loop (keeps register pressure local)
      {   // keep the block pointer provably wave-uniform (SGPRs) in every variant
        const uint64_t pv = (uint64_t)pp;
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)pv);
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(pv >> 32));
        pp = (KPc*)(((uint64_t)hi << 32) | lo);
      }
      asm volatile("" : "+s"(a), "+s"(pp));
      if (a == A_YIELD || a == A_SPEC_STAGED || a == A_SPEC_WAIT || a == A_SPEC_DISCARD ||
          (kTwoEnded && a == A_BIDI_TREE))
        break;
      const bool prof = kProfile && Pr().stamps != nullptr;
      const long long t0 = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
      const int a0 = a;
      switch (a) {
        case A_GRAD: a = act_grad(); break;
        case A_INIT_STATE: a = act_init_state(); break;
        case A_INIT_START: a = act_init_start(); break;
        case A_INIT_STEP: a = act_init_step(); break;
        case A_SS_BEGIN: a = act_ss_begin(); break;
        case A_SS_TRIAL: a = act_ss_trial(); break;
        case A_SS_STEP: a = act_ss_step(); break;
        case A_SS_FINISH: a = act_ss_finish(); break;
        case A_START_TRANSITION: a = act_start_transition(); break;
        case A_BEGIN_SUBTREE: a = act_begin_subtree(); break;
        case A_END_TREE: a = act_end_tree(); break;
        case A_NEXT_TRANSITION: a = act_next_transition(); break;
        case A_FINISH: a = act_finish(); break;
        case A_LEAPFROG: a = act_leapfrog(); break;
        case A_WRITE_MP: a = act_write_mp(); break;
        case A_PRIOR: a = act_prior(); break;
        case A_SPEC_BOOK: a = act_spec_book(); break;
        default: a = A_YIELD; break;
      }
      if (prof) {
        wave_fence();
        const int ai = (a0 == A_SPEC_BOOK) ? A_LEAF : a0;   // slot 11: the leaf's bookkeeping
        Sp->prof[0][ai] += (long long)__builtin_amdgcn_s_memtime() - t0;
        Sp->prof[1][ai] += 1;
      }
    }
    wave_publish();   // (the yielded position's MP before the kernel's ring entry)
    return a;
  }
};
