"""Time the posterior curves (bands of dL, m and the residuals per depth bin; five
probabilities, all three quantities) on synthetic horseshoe draws, Nn = 15, that lie in device
memory:

* the device route (``fitoct_curves_device``) at the headline shape (1024 chains x 1000
  post-warmup draws of 1500 saved, N = 2048) and at config 5's shape (256 files x 4 chains x
  100 draws, N = 481): HIP events around the call, one warm-up call, the median of five.  The
  kernel split is by difference: a call without probabilities runs params_kernel,
  curve_kernel and moments_kernel only, the rest of a full call is the radix select;
* the parent commit's route, copy the draws to the host and evaluate there
  (``fitoct_curves_host``), wall time, measured once at ``--host-chains`` chains of the
  headline shape (the largest that finishes in about a minute).  Its evaluation and its
  selections are both linear in the number of draws, so the headline figure is that time
  scaled by chains / host-chains (reported as ``host_s_scaled``).

Prints the kernel split and one JSON line (committed as profiles/curves_timing.json;
DESIGN.md §5).

    python scripts/time_curves.py [--chains 1024] [--bins 2048] [--host-chains 512] [--no-host]
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

THETA = (40.0, 900.0, 150.0)


def problem(N, Nn, seed):
    from fitoct_amd.api import ExpGPProblem
    rng = np.random.default_rng(seed)
    x = np.linspace(20.0, 500.0, N)
    m = THETA[0] + THETA[1] * np.exp(-2 * x / (THETA[2] * (1 + 0.03 * np.sin(x / 60.0))))
    uy = 2.0 + 0.02 * m
    return ExpGPProblem(x, m + uy * rng.standard_normal(N), uy, Nn=Nn, prior_type="horseshoe")


def synthetic_draws(torch, prob, groups, chains, iters, seed=5):
    """Raw horseshoe draws [groups, chains, iters, D + 8] on the device: theta a few per cent
    around THETA, |yGP| = |z lambda tau| <= 0.05, everything else positive."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    D, Nn = prob.D, prob.Nn
    shape = (groups, chains, iters)

    def u(lo, hi, *tail):
        return lo + (hi - lo) * torch.rand(shape + tail, generator=g, dtype=torch.float64,
                                           device="cuda")
    raw = torch.exp(0.3 * torch.randn(shape + (D + 8,), generator=g, dtype=torch.float64,
                                      device="cuda"))
    th = torch.tensor(THETA, dtype=torch.float64, device="cuda")
    raw[..., 7:10] = th * (1 + 0.03 * torch.randn(shape + (3,), generator=g, dtype=torch.float64,
                                                  device="cuda"))
    p = raw[..., 7:7 + D]
    p[..., 3:3 + Nn] = u(-1, 1, Nn)
    p[..., 3 + Nn] = u(0.05, 0.25)
    p[..., 4 + Nn] = u(0.2, 1.0)
    p[..., 5 + Nn:5 + 2 * Nn] = u(0.0, 0.4, Nn)
    p[..., 5 + 2 * Nn:5 + 3 * Nn] = u(0.0, 0.25, Nn)
    return raw.contiguous()


def time_device(torch, raw, probs_list, chains, iters, first, probs):
    from fitoct_amd.api import curves_device

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tab = curves_device(raw.data_ptr(), probs_list, chains, iters, first_iter=first, probs=probs)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), tab
    once()   # warm-up: module load, allocator
    runs = [once() for _ in range(5)]
    ms = [r[0] for r in runs]
    same = all(r[1].tobytes() == runs[0][1].tobytes() for r in runs)
    return statistics.median(ms), ms, same, runs[0][1]


def device_shape(torch, name, groups, chains, iters, first, N, Nn):
    from fitoct_amd.api import DEFAULT_PROBS
    probs_list = [problem(N, Nn, 100 + g) for g in range(groups)]
    raw = synthetic_draws(torch, probs_list[0], groups, chains, iters)
    torch.cuda.synchronize()
    full, ms, same, table = time_device(torch, raw, probs_list, chains, iters, first, DEFAULT_PROBS)
    nosel, _, _, _ = time_device(torch, raw, probs_list, chains, iters, first, ())
    print(f"{name}: {full:.1f} ms = params + curve + moments kernels {nosel:.1f} ms "
          f"+ radix select {full - nosel:.1f} ms", file=sys.stderr)
    res = {"shape": {"groups": groups, "chains": chains, "iters_saved": iters, "first_iter": first,
                     "N": N, "Nn": Nn, "family": "horseshoe", "probs": list(DEFAULT_PROBS),
                     "what": ["dL", "m", "resid"], "draws_bytes": int(raw.numel() * 8)},
           "device_ms_median": full, "device_ms": ms,
           "split_ms": {"params_curve_moments": nosel, "radix_select": full - nosel},
           "device_bitwise_repeatable": same}
    return res, raw, probs_list, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--bins", type=int, default=2048)
    ap.add_argument("--host-chains", type=int, default=512)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()

    import torch

    from fitoct_amd.api import DEFAULT_PROBS, curves_host
    res = {"what": "posterior curves, device route vs download + fitoct_curves_host"}
    head, raw, probs_list, table = device_shape(torch, "headline", 1, a.chains, a.iters, a.warmup,
                                                a.bins, 15)
    res["headline"] = head
    if not a.no_host:
        hc = min(a.host_chains, a.chains)
        t0 = time.perf_counter()
        host_raw = raw[0, :hc].cpu().numpy()
        t1 = time.perf_counter()
        host = curves_host(host_raw, probs_list[0], a.warmup, DEFAULT_PROBS)
        t2 = time.perf_counter()
        scale = a.chains / hc
        res["host"] = {"chains": hc, "copy_s": t1 - t0, "curves_host_s": t2 - t1,
                       "host_s": t2 - t0, "scaling": "linear in chains",
                       "host_s_scaled": (t2 - t0) * scale}
        if hc == a.chains:
            res["host"]["max_abs_diff"] = float(np.max(np.abs(host - table)))
    del raw
    torch.cuda.empty_cache()
    res["config5"], _, _, _ = device_shape(torch, "config 5", 256, 4, 100, 0, 481, 15)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
