"""Time the pairs plot (the default ``pars``, 32 bins, two count planes) on synthetic horseshoe
draws, Nn = 15, that lie in device memory at the headline shape (1024 chains x 1000 post-warmup
draws of 1500 saved; N = 2048 plays no part: the table reads no data):

* the device route (``fitoct_pairs_device``, what ``Plan.pairs()`` calls on the draws where
  they lie): HIP events around the call, one warm-up call, the median of five, and the same for
  each part alone (``what=``: the ranges and digitising, the marginals, the panels, the
  correlation);
* the parent commit's route for the same numbers: copy the draws to the host, ``materialise``,
  then ``np.histogram``, ``np.histogram2d`` and ``np.corrcoef`` per plane; wall time, once.

Prints the split and one JSON line (committed as profiles/pairs_timing.json).

    python scripts/time_pairs.py [--chains 1024] [--no-host]
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

SETTINGS = dict(n_bins=32, planes=2)


def time_device(torch, raw, prob, chains, iters, first, what, repeats=5):
    from fitoct_amd.api import pairs_device

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t = pairs_device(raw.data_ptr(), prob, chains, iters, first_iter=first, what=what, **SETTINGS)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), t
    once()   # warm-up: module load, allocator
    runs = [once() for _ in range(repeats)]
    blob = [b"".join(r[1][w].tobytes() for w in what) for r in runs]
    return statistics.median(r[0] for r in runs), [r[0] for r in runs], len(set(blob)) == 1, runs[0][1]


def host_route(raw, prob, first, columns, lib_edges):
    """download + materialise + numpy, the parent commit's way to the same numbers (binned over
    the library's edges, so that the counts can be compared; its own minima and maxima are
    taken, and timed, all the same)."""
    from fitoct_amd.stanfit import materialise, output_columns
    t0 = time.perf_counter()
    host = raw[0].cpu().numpy()
    t1 = time.perf_counter()
    names = output_columns(prob)
    m = materialise(host, prob)[:, first:, :].reshape(-1, len(names))
    x = np.ascontiguousarray(m[:, [names.index(c) for c in columns]].T)
    div = host[:, first:, 5].reshape(-1) != 0
    t2 = time.perf_counter()
    ends = np.array([(v.min(), v.max()) for v in x])
    edges = lib_edges
    hist, panels = [], []
    for mask in (slice(None), div):
        hist.append([np.histogram(v[mask], bins=e)[0] for v, e in zip(x, edges)])
        panels.append([np.histogram2d(x[a][mask], x[b][mask], bins=[edges[a], edges[b]])[0]
                       for a in range(len(x)) for b in range(a + 1, len(x))])
    t3 = time.perf_counter()
    corr = np.corrcoef(x)
    t4 = time.perf_counter()
    return ({"copy_s": t1 - t0, "materialise_s": t2 - t1, "histograms_s": t3 - t2,
             "corrcoef_s": t4 - t3, "host_s": t4 - t0,
             "ranges_equal": bool(np.array_equal(ends, lib_edges[:, [0, -1]]))},
            np.array(hist), np.array(panels), corr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()

    import torch

    from fitoct_amd.api import PAIRS_WHAT
    from time_curves import problem, synthetic_draws
    prob = problem(2048, 15, 100)
    raw = synthetic_draws(torch, prob, 1, a.chains, a.iters)
    g = torch.Generator(device="cuda").manual_seed(9)   # 7.9 % divergent transitions
    raw[..., 5] = (torch.rand(raw.shape[:3], generator=g, device="cuda") < 0.079).double()
    torch.cuda.synchronize()
    args = (torch, raw, prob, a.chains, a.iters, a.warmup)

    full, ms, same, table = time_device(*args, PAIRS_WHAT)
    parts = {"ranges_digitise": ("edges",), "marginals": ("edges", "hist", "outside"),
             "panels": ("edges", "panels"), "corr": ("corr",)}
    split = {k: time_device(*args, w)[0] for k, w in parts.items()}
    for k in ("marginals", "panels"):
        split[k] -= split["ranges_digitise"]
    print(f"pairs: {full:.1f} ms; " + ", ".join(f"{k} {v:.1f} ms" for k, v in split.items()),
          file=sys.stderr)
    res = {"what": "pairs plot, device route vs download + materialise + numpy",
           "shape": {"groups": 1, "chains": a.chains, "iters_saved": a.iters, "first_iter": a.warmup,
                     "N": 2048, "Nn": 15, "family": "horseshoe", "columns": table["columns"],
                     "n_panels": int(table["panels"].shape[1]), "draws_bytes": int(raw.numel() * 8),
                     **SETTINGS},
           "device_ms_median": full, "device_ms": ms, "split_ms": split,
           "device_bitwise_repeatable": same}

    if not a.no_host:
        res["host"], hist, panels, corr = host_route(raw, prob, a.warmup, table["columns"],
                                                   table["edges"][0])
        res["host"]["counts_equal"] = bool(
            np.array_equal(hist.transpose(1, 0, 2), table["hist"][0]) and
            np.array_equal(panels.transpose(1, 0, 2, 3), table["panels"][0]))
        res["host"]["corr_max_abs_diff"] = float(np.nanmax(np.abs(corr - table["corr"][0])))
        res["speedup"] = res["host"]["host_s"] * 1e3 / full
    print(json.dumps(res))


if __name__ == "__main__":
    main()
