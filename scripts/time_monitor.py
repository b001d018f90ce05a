"""Time the rank diagnostics (rank-normalised R-hat, bulk and tail ESS) on synthetic buffers
that lie in device memory, at two shapes:

* ``headline``: horseshoe Nn = 15, 1024 chains x 1000 post-warmup draws (1500 saved, 500
  skipped), one group -- few large segments, the multi-workgroup sort;
* ``config5``: 256 files x 4 chains x 100 draws -- many small segments, the LDS sort.

Per shape:

* the device route (``fitoct_monitor_device``, what ``Plan.monitor`` / ``Batch.monitor`` call
  below the handle): HIP events around the call, one warm-up call, the median of five;
* the route a caller had before: copy the draws to the host, materialise the output layout,
  ``fitoct_rank_rhat`` per column -- wall time, measured once (R-hat only: that route has no
  bulk or tail ESS).

Prints one JSON line per shape and, with ``--out``, writes them to that file (committed as
profiles/monitor_timing.json).

    python scripts/time_monitor.py [--shapes headline,config5] [--no-parent] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SHAPES = {   # groups, chains, saved iterations, skipped
    "headline": (1, 1024, 1500, 500),
    "config5": (256, 4, 100, 0),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,config5")
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    from time_summary import synthetic_draws

    from fitoct_amd.api import ExpGPProblem, monitor_device
    from fitoct_amd.stanfit import materialise, output_columns, rank_rhat
    xs = np.linspace(20.0, 500.0, 16)
    prob = ExpGPProblem(xs, 1000.0 + 0 * xs, 1.0 + 0 * xs, Nn=15, prior_type="horseshoe")
    names = output_columns(prob)
    lines = []
    for shape in a.shapes.split(","):
        G, chains, iters, first = SHAPES[shape]
        raw = synthetic_draws(torch, prob, G * chains, iters).reshape(G, chains, iters, -1)
        torch.cuda.synchronize()

        def once():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tab = monitor_device(raw.data_ptr(), [prob] * G, chains, iters, first_iter=first)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), tab
        once()   # warm-up: module load, allocator
        runs = [once() for _ in range(5)]
        ms = [r[0] for r in runs]
        table = runs[0][1]
        res = {"what": "rank diagnostics, device route vs download + fitoct_rank_rhat per column",
               "shape": {"name": shape, "groups": G, "chains": chains, "iters_saved": iters,
                         "first_iter": first, "raw_cols": prob.D + 8,
                         "output_cols": int(table.shape[1]), "draws_bytes": int(raw.numel() * 8)},
               "device_ms_median": statistics.median(ms), "device_ms": ms,
               "device_bitwise_repeatable": all(r[1].tobytes() == table.tobytes() for r in runs)}
        if not a.no_parent:
            t0 = time.perf_counter()
            host = raw.cpu().numpy()
            t1 = time.perf_counter()
            out = materialise(host, prob)[:, :, first:, :]
            t2 = time.perf_counter()
            rh = np.array([[rank_rhat(out[g, :, :, j]) for j in range(len(names))]
                           for g in range(G)])
            t3 = time.perf_counter()
            ok = ~np.isnan(table[:, :, 0])
            res.update({"parent_s": t3 - t0, "parent_copy_s": t1 - t0,
                        "parent_materialise_s": t2 - t1, "parent_rank_rhat_s": t3 - t2,
                        "parent_over_device": (t3 - t0) * 1e3 / statistics.median(ms),
                        "max_rel_diff_rhat": float(np.max(np.abs(table[:, :, 0][ok] - rh[ok]) /
                                                          rh[ok])),
                        "rank_rhat_max": float(np.max(table[:, :, 0][ok]))})
        print(json.dumps(res), flush=True)
        lines.append(res)
        del raw
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
