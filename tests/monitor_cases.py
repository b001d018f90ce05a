"""Cases and reference of the rank-diagnostics tests (test_monitor.py on the CPU,
test_gpu_monitor.py on the device): the synthetic raw buffers of summary_cases.py plus two of
their own, and a numpy / scipy restatement of ``rstan::monitor``'s rank-normalised split R-hat,
bulk ESS and tail ESS (Vehtari et al. 2021; include/fitoct.h "rank diagnostics"), written from
the definitions: ranks by ``scipy.stats.rankdata``, Phi^-1 by ``scipy.stats.norm.ppf``, every
ESS by ``summary_cases.geyer_margins`` so that the branch margins come with it.

Case ``i`` is one column longer than two workgroup-sorted segments and no multiple of either
sort constant of include/fitoct.h (read from the header, not guessed): the multi-workgroup
sort with a ragged last tile.  Case ``j`` is many small segments in one launch.
"""
from __future__ import annotations

import os
import re

import numpy as np
from scipy.stats import norm, rankdata

import summary_cases as SC
from summary_cases import Case, _problem, _rng, make_raw

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "fitoct.h")


def header_constant(name):
    return int(re.search(rf"#define {name} (\d+)", open(HEADER).read()).group(1))


SORT_LDS_KEYS = header_constant("FITOCT_MONITOR_SORT_LDS_KEYS")   # one workgroup sorts this many
SORT_TILE = header_constant("FITOCT_MONITOR_SORT_TILE")
STAGING_BUFFERS = header_constant("FITOCT_MONITOR_STAGING_BUFFERS")

KEYS = ("Rhat", "Rhat_bulk", "Rhat_fold", "Bulk_ESS", "Tail_ESS")
MIN_MARGIN = 1e-10


def case_i():
    """2 chains of n = 2 h draws, S = 4 h = 2 SORT_LDS_KEYS + 808 pooled values."""
    p = _problem("monoexp", 2)
    h = SORT_LDS_KEYS // 2 + 202
    return Case("i", [p], make_raw(p, _rng(31), 2, 2 * h, phis=0.6)[None])


def case_j():
    rng = _rng(32)
    ps = [_problem("normal", 15, lambda_rate=0.02 * (g + 1)) for g in range(40)]
    return Case("j", ps, np.stack([make_raw(p, rng, 4, 40) for p in ps]))


CASES = dict(SC.CASES, i=case_i, j=case_j)

# Columns whose ESS is not compared (their R-hats are): a Geyer branch of one of their 0/1
# indicator series is closer than 1e-10 to flipping.  With so few distinct autocovariances (in
# case j, 8 ones among 160 values) two sides of a comparison are often the same rational
# number, so no seed avoids it; test_monitor.py::test_branch_margins checks that these are all of them.
ESS_LEFT_OUT = {
    "c": [(0, "lambda")],
    "j": [(3, "lp__"), (4, "yGP.7"), (11, "yGP.15"), (13, "sigma"), (20, "yGP.14"),
          (22, "yGP.8"), (24, "yGP.13"), (25, "yGP.15"), (26, "sigma"), (30, "yGP.9")],
}


def pooled_size(case):
    _, chains, iters, _ = case.raw.shape
    return 2 * chains * ((iters - case.first_iter) // 2)


# ---- the definitions ---------------------------------------------------------------------------
def split_chains(x):
    """x[chains, n] -> [2 chains, h] in split-chain order; an odd n's middle draw is dropped."""
    n = x.shape[1]
    h = n // 2
    return np.stack([half for c in x for half in (c[:h], c[n - h:])])


def z_scores(v):
    S = v.size
    return norm.ppf((rankdata(v, method="average") - 0.375) / (S + 0.25))


def psr(ch):
    m, h = ch.shape
    B = h * ch.mean(1).var(ddof=1)
    W = ch.var(axis=1, ddof=1).mean()
    return float(np.sqrt((B / W + h - 1) / h))


def quantile7(srt, p):
    hh = (srt.size - 1) * p
    lo = int(np.floor(hh))
    hi = min(lo + 1, srt.size - 1)
    frac = hh - lo
    return srt[lo] + frac * (srt[hi] - srt[lo]) if frac > 0 else srt[lo]


def _ess(ch):
    """(n_eff, branch margin) of already split chains ch[m, h]; NaN for a constant series.
    geyer_margins splits what it is given: it gets chains of 2 h made of the halves."""
    if np.all(ch == ch.flat[0]):
        return float("nan"), np.inf
    m, h = ch.shape
    ess, margin, _ = SC.geyer_margins(ch.reshape(m // 2, 2 * h))
    return ess, margin


def reference_row(x):
    """x[chains, n] of one column -> (the five values, the smallest Geyer branch margin of the
    z series, the same of the two indicator series)."""
    ch = split_chains(np.asarray(x, float))
    m, h = ch.shape
    pooled = ch.reshape(-1)
    nan5 = np.full(5, np.nan)
    # every chain constant (all values equal, or a per-chain constant such as stepsize__): the
    # within-chain variance is zero and the R-hats would be rounding noise over zero
    if np.any(np.isnan(pooled)) or np.all(ch == ch[::2, :1].repeat(2, axis=0)):
        return nan5, np.inf, np.inf
    srt = np.sort(pooled)
    S = pooled.size
    med = 0.5 * (srt[S // 2 - 1] + srt[S // 2])        # S = 2 chains h is even
    z = z_scores(pooled).reshape(m, h)
    zf = z_scores(np.abs(pooled - med)).reshape(m, h)
    bulk, fold = psr(z), psr(zf)
    bulk_ess, z_margin = _ess(z)
    tails, t_margin = [], np.inf
    for p in (0.05, 0.95):
        e, mg = _ess((ch <= quantile7(srt, p)).astype(float))
        tails.append(e)
        t_margin = min(t_margin, mg)
    tail = float("nan") if np.any(np.isnan(tails)) else min(tails)
    return np.array([max(bulk, fold), bulk, fold, bulk_ess, tail]), z_margin, t_margin


def reference(case):
    """{(group, column name): (row, z margin, tail margin)} over every output column."""
    out = {}
    for g in range(len(case.probs_list)):
        fit, _ = SC.stanfit_rows(case, g)
        for col in fit.columns:
            out[g, col] = reference_row(SC.column(fit, col))
    return out


# ---- comparison --------------------------------------------------------------------------------
def check_row(row, want, what, ess=True):
    """One row of five against a reference row at the tolerances of summary_cases.check_row:
    the R-hats 1e-10 and the ESS 1e-8 relative, the NaN pattern identical.  ``ess`` False: a
    column whose Geyer margin is too small to compare an ESS (its R-hats still are)."""
    cols = range(5) if ess else range(3)
    for i in cols:
        assert np.isnan(row[i]) == np.isnan(want[i]), (what, KEYS[i], row, want)
        assert SC._close_or_both_nan(row[i], want[i], 1e-10 if i < 3 else 1e-8), \
            (what, KEYS[i], row[i], want[i])
