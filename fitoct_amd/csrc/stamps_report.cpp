// FITOCT_STAMPS: the report of a profiling build's cycle stamps (kernel_params.h StampSlot)
// on stderr.  scripts/stamps_*.py and the committed profiles/*stamps* files read these lines.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "host_internal.h"
#include "kernel_params.h"

namespace fitoct {

// the launch-time switches of the stamps (diagnostic only): FITOCT_STAMPS asks for them,
// FITOCT_BENCH_SWEEPS=n makes the launch a sweep-only measurement (KParams::bench_sweeps)
bool stamps_requested(int* bench_sweeps) {
  if (getenv("FITOCT_STAMPS") == nullptr) return false;
  if (bench_sweeps) {
    const char* e = getenv("FITOCT_BENCH_SWEEPS");
    *bench_sweeps = e ? atoi(e) : 0;
  }
  return true;
}

void report_stamps(const long long* h, int tiles, bool bidi) {
  auto tile = [&](int t) { return h + (size_t)NSTAMP * t; };
  double steps = 0, tg = 0, tn = 0, tt = 0, smax = 0, tw = 0, nw = 0, tsw = 0, tno = 0;
  double ts0 = 0, ts1 = 0;
  double act_t[18] = {0}, act_n[18] = {0};
  for (int t = 0; t < tiles; ++t) {
    const long long* o = tile(t);
    steps += o[SS_SWEEPS];
    tg += o[SS_GRAD_BUSY];
    tn += o[SS_NUTS_BUSY];
    tt += o[SS_WALL];
    tw += o[SS_WAIT];
    nw += o[SS_ROUNDS];
    tsw += o[SS_ENQ_TO_SWEPT];
    tno += o[SS_SWEPT_TO_RESUMED];
    ts0 += o[SS_FIRST_START];
    ts1 += o[SS_LAST_START];
    smax = std::max(smax, (double)o[SS_SWEEPS]);
    for (int a = 0; a < 18; ++a) {
      act_t[a] += o[SS_ACT_CYCLES + a];
      act_n[a] += o[SS_ACT_CALLS + a];
    }
  }
  double subt[12] = {0}, wb[8] = {0};
  for (int t = 0; t < tiles; ++t) {
    const long long* o = tile(t);
    for (int k = 0; k < 8; ++k) subt[k] += o[SS_SUB + k];
    for (int k = 0; k < 4; ++k) subt[8 + k] += o[SS_SUB_HI + k];
    for (int k = 0; k < 8; ++k) wb[k] += o[SS_WAVE_BUSY + k];
  }
  fprintf(stderr, "[fitoct stamps] gradient-wave busy per sweep by wave:");
  for (int k = 0; k < 8; ++k) fprintf(stderr, " %.0f", wb[k] / std::max(steps, 1.0));
  fprintf(stderr, "\n");
  // per gradient of chain 0 (act_n[1]: A_GRAD runs); a11 is the speculative path's
  // separate bookkeeping action (A_SPEC_BOOK)
  fprintf(stderr, "[fitoct stamps] sub-action cycles per gradient (chain 0): ");
  for (int k = 0; k < 12; ++k)
    if (subt[k] > 0) fprintf(stderr, "s%d:%.0f ", k, subt[k] / std::max(act_n[1], 1.0));
  fprintf(stderr, "\n");
  fprintf(stderr, "[fitoct stamps] per action (chain 0 of each tile): ");
  for (int a = 1; a < 18; ++a)
    if (act_n[a] > 0) fprintf(stderr, "a%d:%.0fx%.0f ", a, act_n[a] / tiles, act_t[a] / act_n[a]);
  fprintf(stderr, "\n");
  fprintf(stderr,
          "[fitoct stamps] tiles=%d mean sweeps/tile=%.0f max=%.0f | per sweep: grad-wave busy %.0f "
          "nuts-wave busy %.0f wall %.0f memtime ticks\n",
          tiles, steps / tiles, smax, tg / steps, tn / steps, tt / steps);
  fprintf(stderr,
          "[fitoct stamps] chain 0 per NUTS round: busy %.0f, waiting for its gradient %.0f "
          "(enqueue->sweep done %.0f, sweep done->resumed %.0f)\n",
          tn / std::max(nw, 1.0), tw / std::max(nw, 1.0), tsw / std::max(nw, 1.0),
          tno / std::max(nw, 1.0));
  fprintf(stderr, "[fitoct stamps] enqueue -> first wave starts %.0f, last wave starts %.0f\n",
          ts0 / std::max(nw, 1.0), ts1 / std::max(nw, 1.0));
  // tile timeline on the 100 MHz clock: how much of the launch the tiles sit idle at
  // the end (the kernel ends with its last tile)
  {
    long long t0 = LLONG_MAX, t1 = 0;
    std::vector<double> ends, firsts;
    for (int t = 0; t < tiles; ++t) {
      t0 = std::min(t0, tile(t)[SS_RT_BEGIN]);
      t1 = std::max(t1, tile(t)[SS_RT_END]);
    }
    const double span = std::max(1.0, (double)(t1 - t0));
    double done_sum = 0;
    for (int t = 0; t < tiles; ++t) {
      const long long* o = tile(t);
      ends.push_back((o[SS_RT_END] - t0) / span);
      if (o[SS_RT_FIRST_DONE] > 0) firsts.push_back((o[SS_RT_FIRST_DONE] - t0) / span);
      done_sum += o[SS_CHAINS_DONE];
    }
    std::sort(ends.begin(), ends.end());
    std::sort(firsts.begin(), firsts.end());
    auto q = [](const std::vector<double>& v, double f) {
      return v.empty() ? 0.0 : v[std::min(v.size() - 1, (size_t)(f * (v.size() - 1)))];
    };
    double mean_end = 0;
    for (double e : ends) mean_end += e;
    mean_end /= std::max<size_t>(1, ends.size());
    fprintf(stderr,
            "[fitoct stamps] tile ends (fraction of the launch): mean %.3f p10 %.3f p50 %.3f "
            "p90 %.3f | first chain done in a tile: p10 %.3f p50 %.3f p90 %.3f | chains "
            "finished %.0f, launch %.1f ms\n",
            mean_end, q(ends, 0.1), q(ends, 0.5), q(ends, 0.9), q(firsts, 0.1), q(firsts, 0.5),
            q(firsts, 0.9), done_sum, span / 1e5);
    // tile occupancy: share of all tiles' time, and of all sweeps, spent while a tile
    // hosted k live chains (k = 0..4; the launch's tail runs thinned-out tiles)
    double ot[GMAX + 1] = {0}, on[GMAX + 1] = {0}, st = 0, sn = 0;
    for (int t = 0; t < tiles; ++t)
      for (int k = 0; k <= GMAX; ++k) {
        ot[k] += tile(t)[SS_OCC_TIME + k];
        on[k] += tile(t)[SS_OCC_SWEEPS + k];
      }
    for (int k = 0; k <= GMAX; ++k) {
      st += ot[k];
      sn += on[k];
    }
    fprintf(stderr, "[fitoct stamps] tile occupancy (live chains k: share of tile time / of sweeps):");
    for (int k = 0; k <= GMAX; ++k)
      fprintf(stderr, " k=%d %.4f/%.4f", k, ot[k] / std::max(st, 1.0), on[k] / std::max(sn, 1.0));
    fprintf(stderr, "\n");
  }
  if (bidi) {   // two-ended roles (tiles of one chain; paired: the forward end's
                // producer runs in the partner tile)
    double hb = 0, hw = 0, hn = 0, hi = 0, pe[2][4] = {{0}};
    for (int t = 0; t < tiles; ++t) {
      const long long* o = tile(t);
      hb += o[SS_BOOK_BUSY];
      hw += o[SS_BOOK_WAIT];
      hn += o[SS_BOOK_LEAVES];
      hi += o[SS_BOOK_IDLE];
      for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 4; ++k) pe[s][k] += o[SS_PRODUCER + 4 * s + k];
    }
    fprintf(stderr,
            "[fitoct stamps] booking wave per booked leaf: busy %.0f, waiting for its record %.0f "
            "(leaves booked per tile %.0f, idle between trees %.0f per tile)\n",
            hb / std::max(hn, 1.0), hw / std::max(hn, 1.0), hn / tiles, hi / tiles);
    for (int s = 0; s < 2; ++s)
      fprintf(stderr,
              "[fitoct stamps] producer of end %d per produced leaf: waiting for its sweep %.0f, "
              "for lookahead / record slot %.0f, in trees %.0f (leaves per tile %.0f)\n",
              s, pe[s][0] / std::max(pe[s][2], 1.0), pe[s][1] / std::max(pe[s][2], 1.0),
              pe[s][3] / std::max(pe[s][2], 1.0), pe[s][2] / tiles);
    for (int s = 0; s < 2; ++s) {
      double q[4] = {0, 0, 0, 0}, n = 0;
      for (int t = 0; t < tiles; ++t) {
        for (int k = 0; k < 4; ++k) q[k] += tile(t)[SS_PRODUCER_LEAF + 4 * s + k];
        n += tile(t)[SS_PRODUCER + 4 * s + 2];   // the producer's leaves
      }
      fprintf(stderr,
              "[fitoct stamps] producer of end %d per leaf (helped): finish_grad %.0f, stage %.0f, "
              "hand-over %.0f, prior_part %.0f\n", s, q[0] / std::max(n, 1.0),
              q[1] / std::max(n, 1.0), q[2] / std::max(n, 1.0), q[3] / std::max(n, 1.0));
    }
    double hb2[2] = {0, 0}, hn2[2] = {0, 0};
    for (int t = 0; t < tiles; ++t)
      for (int r = 0; r < 2; ++r) {
        hb2[r] += tile(t)[SS_HELPER + 2 * r];
        hn2[r] += tile(t)[SS_HELPER + 2 * r + 1];
      }
    for (int r = 0; r < 2; ++r)
      if (hn2[r] > 0)
        fprintf(stderr,
                "[fitoct stamps] booking helper (%s tile): %.0f cycles per booked leaf, %.0f "
                "leaves per tile\n", r ? "partner" : "primary", hb2[r] / hn2[r], hn2[r] / tiles);
  }
}

}  // namespace fitoct

// test entry (tests/test_schedule.py): the report of a caller-made array
extern "C" void fitoct_internal_report_stamps(const long long* h, int32_t tiles, int32_t bidi) {
  fitoct::report_stamps(h, tiles, bidi != 0);
}
