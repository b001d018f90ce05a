// The launch schedule: which sampler variant a launch runs, decided in one pure function
// of the shape (schedule.cpp).  No HIP call and no environment read happens in the decision:
// the planner's environment switches are read once per fitoct_plan_create /
// fitoct_batch_create (Switches::from_env) and handed in.
#pragma once

namespace fitoct {

// every environment switch of the planner
struct Switches {
  bool no_geo = false;         // FITOCT_NO_GEO: no Horner-in-R^l moments, no 16-bin layout
  bool no_pair = false;        // FITOCT_NO_PAIR
  bool pair = false;           // FITOCT_PAIR: pair row-mode tiles too
  bool no_migrate = false;     // FITOCT_NO_MIGRATE
  bool no_spec = false;        // FITOCT_NO_SPEC: the plain sampler
  bool no_bidi = false;        // FITOCT_NO_BIDI
  bool no_tail_bidi = false;   // FITOCT_NO_TAIL_BIDI
  int spec = -1;               // FITOCT_SPEC: -1 unset, else atoi != 0
  int spec_live = -1;          // FITOCT_SPEC_LIVE: -1 unset, else max(0, atoi)
  int tail_left = -1;          // FITOCT_TAIL_LEFT: -1 unset, else max(0, atoi)
  int test_tail_idle_us = 0;   // FITOCT_TEST_TAIL_IDLE_US: 0 unset, else max(1, atoi)
  bool test_pair_absent = false;   // FITOCT_TEST_PAIR_ABSENT
  static Switches from_env();
};

struct Schedule {
  int G = 1, tiles = 0, lds = 0;   // chains per tile, tiles, dynamic LDS bytes of a tile
  bool migrate = false;            // chain migration between tiles
  int spec_live = 0, spec = 0;     // KParams::spec_live / spec
  int bidi = 0;                    // two-ended trajectories (tiles of one chain)
  int tail_bidi = 0, tail_left = 0;            // ... in a migrating launch's tail
  unsigned long long tail_idle_ticks = 0;
  bool pair = false;               // paired tiles
  int grid = 0;                    // blocks launched
  int sampler = 0;                 // FITOCT_SAMPLER_* (fitoct_plan_info::sampler)
};

// The schedule of `chains` chains of one problem: `ppl` parameters per lane, basis `mode`,
// `ncu` compute units, `batch_chains` the chain total of the batch the problem belongs to
// (0: a plan of its own).  A batch pairs its tiles itself (want_pairs over its tile total):
// its problems' schedules are unpaired.  *status: FITOCT_OK, or FITOCT_E_ARG with the
// message in fitoct_last_error().
Schedule choose_schedule(int ppl, int mode, int chains, int batch_chains, int ncu, int max_depth,
                         const Switches& sw, int* status);
// whether a launch of `tiles` tiles with this schedule runs paired tiles
bool want_pairs(const Schedule& s, int mode, int tiles, int ncu, const Switches& sw);

}  // namespace fitoct
