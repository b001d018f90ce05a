// The launch schedule (schedule.h): the single place where the sampler variant of a launch
// is decided.  Pure host arithmetic over the shape and the switches; the only functions
// called are lds_bytes (the kernel's LDS carve, lds_layout.h) and pair_grid.
#include "schedule.h"

#include <stdlib.h>

#include <algorithm>

#include "fitoct.h"
#include "host_internal.h"
#include "kernel_params.h"

namespace fitoct {

int lds_bytes(int ppl, int G, int max_depth);

Switches Switches::from_env() {
  auto set = [](const char* name) { return getenv(name) != nullptr; };
  Switches s;
  s.no_geo = set("FITOCT_NO_GEO");
  s.no_pair = set("FITOCT_NO_PAIR");
  s.pair = set("FITOCT_PAIR");
  s.no_migrate = set("FITOCT_NO_MIGRATE");
  s.no_spec = set("FITOCT_NO_SPEC");
  s.no_bidi = set("FITOCT_NO_BIDI");
  s.no_tail_bidi = set("FITOCT_NO_TAIL_BIDI");
  if (const char* e = getenv("FITOCT_SPEC")) s.spec = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("FITOCT_SPEC_LIVE")) s.spec_live = std::max(0, atoi(e));
  if (const char* e = getenv("FITOCT_TAIL_LEFT")) s.tail_left = std::max(0, atoi(e));
  if (const char* e = getenv("FITOCT_TEST_TAIL_IDLE_US"))   // test hook: producers give up early
    s.test_tail_idle_us = std::max(1, atoi(e));
  if (const char* e = getenv("FITOCT_TEST_PAIR_ABSENT"))    // test hook: partners never join
    s.test_pair_absent = atoi(e) != 0;
  return s;
}

// Migrating tiles of several chains speculate once they host <= this many live chains.
// Measured on config 3 at full length (profiles/r03_ab_spec_live.txt, two interleaved
// runs each): 0 (no speculation) 119.1 k draws/s, 1: 119.7-120.2 k, 2: 121.2-121.4 k,
// 3: 121.5-122.0 k, 4 (always): 119.5-120.3 k.  Tiles that do not migrate (batch mode,
// config 5) lose 7 % with any tail speculation (the speculative kernel's extra registers
// and per-leaf policy read), so they do not speculate.
constexpr int kSpecLiveMigrating = 3;

// (the kernel's static LDS comes on top of the carve: STATIC_LDS_RESERVE)
constexpr int kLdsBudget = 160 * 1024 - STATIC_LDS_RESERVE;

// Paired tiles (nuts_kernel.h "paired tiles"): a launch of one-chain tiles with two-ended
// trajectories whose 2 x tiles (in whole groups of 8 + 8 blocks) fit on the chip grows each
// trajectory's forward end in a partner tile with its own gradient waves, instead of sharing
// the tile's.  Same draws bit for bit: the partner runs the same producer on the same values.
// A partner that does not get a CU at launch leaves its primary to grow both ends (the pair's
// hand-shake), so this is safe on a shared GPU too.  FITOCT_NO_PAIR=1: off.
bool want_pairs(const Schedule& s, int mode, int tiles, int ncu, const Switches& sw) {
  if (!(s.bidi && s.G == 1 && pair_grid(tiles) <= ncu) || sw.no_pair) return false;
  // with the basis rows (N <= 512) an unpaired tile is faster (its chain's wave books the
  // forward end: config 2 253 k vs 245 k draws/s, profiles/r06_ab_unpaired.txt), so there the
  // pairing is on only with FITOCT_PAIR=1
  return mode == MODE_POLY || sw.pair;
}

Schedule choose_schedule(int ppl, int mode, int chains, int batch_chains, int ncu, int max_depth,
                         const Switches& sw, int* status) {
  Schedule s;
  *status = FITOCT_OK;
  // chains per tile: fill every CU with one tile first, then stack chains
  // (a batch plans every problem's tiles from the batch's total chain count)
  const int gc = batch_chains > 0 ? batch_chains : chains;
  int G = std::max(1, std::min(GMAX, (gc + ncu - 1) / ncu));
  while (G > 1 && lds_bytes(ppl, G, max_depth) > kLdsBudget) --G;
  if (lds_bytes(ppl, G, max_depth) > kLdsBudget) {
    *status = fail(FITOCT_E_ARG, "max_treedepth too large for the LDS budget");
    return s;
  }
  s.G = G;
  s.tiles = (chains + G - 1) / G;
  s.lds = lds_bytes(ppl, G, max_depth);
  // Chain migration (work balance): only when every tile of the launch is
  // co-resident (one tile per CU), so an idle tile waiting for a migrant never
  // keeps a pending tile off the chip; off in batch mode (a tile holds one
  // problem's bins) and with FITOCT_NO_MIGRATE.
  s.migrate = batch_chains == 0 && G >= 2 && s.tiles <= ncu && !sw.no_migrate;
  // Speculative leaves (chain.h leaf_spec).  A tile of one (two) chain(s) always
  // speculates, with a spare NUTS wave helping each chain (config 2 +4 %).  A tile of several chains
  // has no spare wave: while it hosts 4 live chains the sweep hides the sampler's latency
  // and speculation only adds work, so a migrating chain speculates only once its tile has
  // thinned out to <= kSpecLiveMigrating chains (the launch's tail, config 3 +2 %).  Draws
  // are the same bit for bit either way.  FITOCT_SPEC_LIVE=n overrides spec_live (0: never; GMAX:
  // always), FITOCT_SPEC=1 is FITOCT_SPEC_LIVE=GMAX (tests), FITOCT_NO_SPEC=1 builds the
  // plain sampler.
  {
    // (tiles of two chains without migration -- a batch of 257..512 chains, config 5's
    // per-GPU share at 2 GPUs -- have a spare NUTS wave per chain too: deep speculation)
    int live = s.migrate ? kSpecLiveMigrating : G <= 2 ? 1 : 0;
    if (sw.spec != -1) live = sw.spec != 0 ? GMAX : live;
    if (sw.spec_live != -1) live = sw.spec_live;
    if (sw.no_spec) live = 0;
    s.spec_live = std::max(0, std::min(live, GMAX));
    s.spec = s.spec_live > 0 ? 1 : 0;
  }
  // Two-ended trajectories (chain.h): tiles of one chain grow the trajectory's two
  // ends at once -- two spare NUTS waves build the subtrees of each direction whole, each in a
  // chain area of its own, and the chain's wave books the trajectory level from one record per
  // subtree.  Same draws bit for bit.  The three chain areas must fit, else the tile stays on
  // the one-ended path (at Nn 16..24 a chain area holds two parameters per lane: three of
  // them at max_treedepth 10 take ~181 KB of the 160 KB).  FITOCT_NO_BIDI=1: off.
  if (s.spec && G == 1 && !s.migrate && !sw.no_bidi) {
    const int base = lds_bytes(ppl, 3, max_depth);
    if (base <= kLdsBudget) {
      s.bidi = 1;
      s.lds = base;
    }
  }
  // Two-ended trajectories in the tail of a migrating launch (tile_migrate.h receive_chain):
  // the producers are idle receivers of the tile (their own chain areas: no LDS added).  Same
  // draws bit for bit.  FITOCT_NO_TAIL_BIDI=1: off; FITOCT_TAIL_LEFT=n: start at n unfinished
  // chains (default: every chain of the launch -- a chain alone in its tile goes two-ended
  // whenever two receivers are idle; one per tile measured 1 % slower on config 3).
  if (s.migrate && s.spec && !sw.no_tail_bidi) {
    s.tail_bidi = 1;
    // from the start (config 3: +1.0 % over one per tile, profiles/r05_ab_tail_left.txt)
    s.tail_left = sw.tail_left == -1 ? chains : std::max(0, sw.tail_left);
    s.tail_idle_ticks = 100ULL * (unsigned long long)sw.test_tail_idle_us;
  }
  s.pair = batch_chains == 0 && want_pairs(s, mode, s.tiles, ncu, sw);
  s.grid = s.pair ? pair_grid(s.tiles) : s.tiles;
  s.sampler = s.migrate ? (s.spec ? FITOCT_SAMPLER_MIGRATE_SPEC : FITOCT_SAMPLER_MIGRATE)
              : s.spec  ? FITOCT_SAMPLER_SPECULATIVE
                        : FITOCT_SAMPLER_PLAIN;
  return s;
}

}  // namespace fitoct

// test entry (tests/test_schedule.py): the planner over plain integers and explicit switches.
// `sw`: the Switches fields in declaration order, as int32.  `out`: G, tiles, lds, migrate,
// spec_live, spec, bidi, tail_bidi, tail_left, tail_idle_ticks, pair, grid, sampler, then for a
// batch (batch_chains > 0) whether its batch_chains / chains problems' tiles run paired,
// and their grid.
extern "C" int32_t fitoct_internal_schedule(int32_t ppl, int32_t mode, int32_t chains,
                                            int32_t batch_chains, int32_t ncu, int32_t max_depth,
                                            const int32_t* sw, int64_t* out) {
  using namespace fitoct;
  Switches w;
  w.no_geo = sw[0], w.no_pair = sw[1], w.pair = sw[2], w.no_migrate = sw[3], w.no_spec = sw[4];
  w.no_bidi = sw[5], w.no_tail_bidi = sw[6], w.spec = sw[7], w.spec_live = sw[8];
  w.tail_left = sw[9], w.test_tail_idle_us = sw[10], w.test_pair_absent = sw[11];
  int rc = FITOCT_OK;
  const Schedule s = choose_schedule(ppl, mode, chains, batch_chains, ncu, max_depth, w, &rc);
  if (rc) return rc;
  const int btiles = batch_chains > 0 ? batch_chains / chains * s.tiles : 0;
  const bool bpair = btiles > 0 && want_pairs(s, mode, btiles, ncu, w);
  const int64_t v[15] = {s.G, s.tiles, s.lds, s.migrate, s.spec_live, s.spec, s.bidi, s.tail_bidi,
                         s.tail_left, (int64_t)s.tail_idle_ticks, s.pair, s.grid, s.sampler,
                         bpair, bpair ? pair_grid(btiles) : btiles};
  std::copy(v, v + 15, out);
  return rc;
}
