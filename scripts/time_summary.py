"""Time the posterior summary at the config-3 shape (1024 chains x 1500 saved iterations x 59
raw columns, horseshoe Nn = 15) on one synthetic buffer that lies in device memory:

* the device route (``fitoct_summary_device``): HIP events around the call, one warm-up call,
  the median of five;
* the parent commit's route on the same bytes: copy the draws to the host, materialise the
  output layout, ``StanFit.summary`` -- wall time, measured once.

Prints one JSON line (committed as profiles/summary_timing.json).

    python scripts/time_summary.py [--chains 1024] [--iters 1500] [--warmup 500] [--no-parent]
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


def synthetic_draws(torch, prob, chains, iters, seed=5):
    """Raw draws [chains, iters, D + 8] on the device: AR(1) series (phi from 0.1 to 0.9 over
    the columns), positive where the model's parameters are, plausible sampler columns."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    W = prob.D + 8
    phi = torch.linspace(0.1, 0.9, W, dtype=torch.float64, device="cuda")
    x = torch.empty((chains, iters, W), dtype=torch.float64, device="cuda")
    cur = torch.randn((chains, W), generator=g, dtype=torch.float64, device="cuda")
    for t in range(iters):
        cur = phi * cur + torch.sqrt(1 - phi * phi) * torch.randn(
            (chains, W), generator=g, dtype=torch.float64, device="cuda")
        x[:, t] = cur
    raw = torch.exp(0.3 * x)                       # parameters and br: positive
    raw[:, :, 0] = -50.0 + 3.0 * x[:, :, 0]        # lp__
    raw[:, :, 1] = torch.sigmoid(x[:, :, 1])       # accept_stat__
    raw[:, :, 2] = 0.1                             # stepsize__
    depth = torch.clamp(torch.round(3.0 + x[:, :, 3]), 1, 10)
    raw[:, :, 3] = depth                           # treedepth__
    raw[:, :, 4] = 2.0 ** depth - 1                # n_leapfrog__
    raw[:, :, 5] = 0.0                             # divergent__
    raw[:, :, 6] = 60.0 + 4.0 * x[:, :, 6]         # energy__
    return raw.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--no-parent", action="store_true")
    a = ap.parse_args()

    import torch

    from fitoct_amd.api import ExpGPProblem, summary_device
    from fitoct_amd.stanfit import StanFit, materialise, output_columns
    xs = np.linspace(20.0, 500.0, 16)
    prob = ExpGPProblem(xs, 1000.0 + 0 * xs, 1.0 + 0 * xs, Nn=15, prior_type="horseshoe")
    raw = synthetic_draws(torch, prob, a.chains, a.iters)
    torch.cuda.synchronize()

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tab = summary_device(raw.data_ptr(), prob, a.chains, a.iters, first_iter=a.warmup)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), tab
    once()   # warm-up: module load, allocator
    runs = [once() for _ in range(5)]
    ms = [r[0] for r in runs]
    table = runs[0][1][0]
    res = {"what": "posterior summary, device route vs the parent commit's host route",
           "shape": {"chains": a.chains, "iters_saved": a.iters, "first_iter": a.warmup,
                     "raw_cols": prob.D + 8, "output_cols": int(table.shape[0]),
                     "draws_bytes": int(raw.numel() * 8)},
           "device_ms_median": statistics.median(ms), "device_ms": ms,
           "device_bitwise_repeatable": all(r[1].tobytes() == runs[0][1].tobytes() for r in runs)}
    if not a.no_parent:
        t0 = time.perf_counter()
        host = raw.cpu().numpy()
        t1 = time.perf_counter()
        out = materialise(host, prob)
        t2 = time.perf_counter()
        rows = StanFit(out, output_columns(prob), a.warmup).summary()
        t3 = time.perf_counter()
        names = output_columns(prob)
        rel = max(abs(table[names.index(k)][0] - r["mean"]) / max(abs(r["mean"]), 1e-300)
                  for k, r in rows.items() if r["sd"] > 0)
        ess = max(abs(table[names.index(k)][-2] - r["n_eff"]) / r["n_eff"]
                  for k, r in rows.items() if r["n_eff"] == r["n_eff"])
        res.update({"parent_s": t3 - t0, "parent_copy_s": t1 - t0, "parent_materialise_s": t2 - t1,
                    "parent_summary_s": t3 - t2, "max_rel_diff_mean": rel,
                    "max_rel_diff_n_eff": ess})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
