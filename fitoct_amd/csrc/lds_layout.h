// Device-resident NUTS, layer 5: the tile's LDS.  The per-lane roles written once at
// start-up (LaneRole) and the carve of the dynamic LDS block (Lds): K^-1, the staged
// positions, the sweep's partial sums, and per chain its scalars, vectors and tree levels.
// The host sizes the same carve (schedule.cpp lds_bytes).
// Part of the sampler's one translation unit (nuts_device.hip includes the layers in order).
// All of it lives in namespace fitoct, which dev_common.h opens and only nuts_device.hip
// closes: parsed on its own, this header ends inside the open namespace.
// Compiled under nuts_device.hip's "#pragma clang fp contract(on)" (see sweep_math.h).
#pragma once
#include "dev_common.h"

// What parameter k's lane needs on every leaf but which depends only on (k, D, Nn, family):
// fixed for the launch, so one NUTS wave writes it to LDS at start-up (load_kinv, before the
// tile's first barrier; read only after it) and the leaf path reads it back (a ds_read is no
// VALU issue) instead of re-deriving it from comparison chains.  Only a role, byte offsets
// and constant coefficients: every value they select between is still computed per leaf.
struct LaneRole {
  double aw;   // horseshoe: weight of the lane's likelihood coefficient (prior_part)
  double cc;   // horseshoe: the inverse-gamma shape of an r2 lane, 1/2 (global) or nu/2
  int soff;    // byte offset of the bin sum the lane's gradient needs (finish_grad)
  int aoff;    // horseshoe: byte offset in AUX of the scale / yGP its coefficient takes
  int kind;    // horseshoe: RK_Z (a z_j lane), RK_R1 (an r1 lane), RK_R2 (the rest)
  int pad;
};
enum RoleKind : int { RK_Z = 0, RK_R1 = 1, RK_R2 = 2 };
static_assert(sizeof(LaneRole) == 32, "LaneRole: 32 B per lane");

template <int FAM>
__device__ __forceinline__ LaneRole lane_role(int k, int D, int Nn, double nu) {
  LaneRole r;
  // which bin sum lane k's gradient needs.  Past D (padded lanes) it is not used:
  // finish_grad forms a gradient only under k < D.
  int si = 0;
  if (k < 3) si = 1 + k;
  else if (k == D - 1) si = 0;
  else if (k < 3 + Nn) si = 4 + (k - 3);
  else if (FAM == FAM_HORSESHOE && k >= 5 + Nn && k < D) {
    // local scale j of r1 (k = 5 + Nn + j) or r2 (k = 5 + 2 Nn + j)
    const int x = k - 5 - Nn;
    si = 4 + (x < Nn ? x : x - Nn);
  }
  r.soff = si * 8;
  // the horseshoe's lanes 3 <= k < D - 1 (prior_part), in the forms prior_part used per leaf
  const bool tz = k < 3 + Nn;
  const bool r1l = k >= 5 + Nn && k < 5 + 2 * Nn, r2l = k >= 5 + 2 * Nn;
  const bool tr1 = k == 3 + Nn || r1l;
  r.cc = (k == 4 + Nn) ? 0.5 : 0.5 * nu;
  const int ai = tz ? 32 + (k - 3) : r1l ? k - 5 - Nn : r2l ? k - 5 - 2 * Nn : 0;
  r.aw = (tz || r1l) ? 1.0 : r2l ? 0.5 : 0.0;
  r.aoff = (ai >= 0 && ai < NAUX ? ai : 0) * 8;   // (other lanes never read it: kept inside AUX)
  r.kind = tz ? RK_Z : tr1 ? RK_R1 : RK_R2;
  r.pad = 0;
  return r;
}

// LDS carve -----------------------------------------------------------------
// [ K^-1 (KMAX x KMAX, row stride NNP) | b (KMAX) | LaneRole[VLEN] | MP[GMAX][MPW] |
//   PART[G][NGW][NSLOT] |
//   G x chain{ ChainScalars | NVEC vectors | SUMS[NSLOT] | AUX[NAUX] | levels[max_depth][NLVL] } ]
template <int PPL>
struct Lds {
  static constexpr int VLEN = WAVE * PPL;
  static constexpr int KBYTES = (KMAX * KMAX + KMAX) * 8;
  static constexpr int RBYTES = VLEN * (int)sizeof(LaneRole);   // the lane-role block, after b
  static __host__ __device__ constexpr int head_bytes(int G) {
    return KBYTES + RBYTES + (GMAX * MPW + NGW * G * NSLOT) * 8;
  }
  static __host__ __device__ constexpr int chain_bytes(int max_depth) {
    // ... | levels[max_depth][NLVL][VLEN] | merge-uniform rings[max_depth][WAVE]
    return (int)sizeof(ChainScalars) +
           (NVEC * VLEN + NSLOT + NAUX + max_depth * NLVL * VLEN + max_depth * WAVE) * 8;
  }
  // tiles of one or two chains (deep speculation): per chain, the booked leaf's q,
  // end-updated p, g, lp and sum r^2, handed from the chain's wave to its helper wave
  static constexpr int HX_BYTES = ((3 * VLEN + 2) * 8 + 15) / 16 * 16;
  // two-ended trajectories (G = 3 areas: the chain's, two producers'): per producer, two
  // slots for the leaves it hands its booking helper (q, end-updated p, g, lp, sum r^2, depth,
  // leaf, transition)
  static constexpr int PX_BYTES = ((3 * VLEN + 8) * 8 + 15) / 16 * 16;
  // ... and per end, two slots for its subtree records (Chain::rvec): 5 vectors, 16 scalars
  // (one parameter per lane; at two, whose chain areas leave less room, one record slot per
  // end in the producer's own area)
  static constexpr int QX_DOUBLES = 5 * VLEN + 16;
  static constexpr int QX_SLOTS = PPL == 1 ? 4 : 0;
  static __host__ __device__ constexpr int bytes(int G, int max_depth) {
    return head_bytes(G) + G * chain_bytes(max_depth) +
           (G <= 2 ? G * HX_BYTES : G == 3 ? 4 * PX_BYTES + QX_SLOTS * QX_DOUBLES * 8 : 0);
  }
  AS_LDS char* base;
  int G, cb;
  __device__ AS_LDS double* kinv() const { return (AS_LDS double*)base; }
  __device__ AS_LDS double* bv() const { return (AS_LDS double*)base + KMAX * KMAX; }
  __device__ AS_LDS LaneRole* lane_roles() const { return (AS_LDS LaneRole*)(base + KBYTES); }
  __device__ AS_LDS double* mp(int c) const {
    return (AS_LDS double*)(base + KBYTES + RBYTES) + c * MPW;
  }
  __device__ AS_LDS double* part() const {
    return (AS_LDS double*)(base + KBYTES + RBYTES) + GMAX * MPW;
  }
  __device__ AS_LDS char* chain(int c) const { return base + head_bytes(G) + c * cb; }
  __device__ AS_LDS ChainScalars& cs(int c) const { return *(AS_LDS ChainScalars*)chain(c); }
  __device__ AS_LDS double* vecs(int c) const {
    return (AS_LDS double*)(chain(c) + sizeof(ChainScalars));
  }
  __device__ AS_LDS double* sums(int c) const { return vecs(c) + NVEC * VLEN; }
  __device__ AS_LDS double* aux(int c) const { return sums(c) + NSLOT; }
  __device__ AS_LDS double* lvls(int c) const { return aux(c) + NAUX; }
  // chain c's hand-off block (G <= 2)
  __device__ AS_LDS double* hx(int c = 0) const {
    return (AS_LDS double*)(base + head_bytes(G) + G * cb + c * HX_BYTES);
  }
  // producer s's hand-off slot k (two-ended trajectories, G = 3)
  __device__ AS_LDS double* px(int s, int k) const {
    return (AS_LDS double*)(base + head_bytes(G) + G * cb + (2 * s + k) * PX_BYTES);
  }
  // the record slots (end s, slot k = 2 s + k), after the hand-off slots
  __device__ AS_LDS double* qx0() const {
    return (AS_LDS double*)(base + head_bytes(G) + G * cb + 4 * PX_BYTES);
  }
};
