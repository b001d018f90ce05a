"""Synthetic raw-layout draws for the posterior-summary tests (test_summary.py on the CPU,
test_gpu_summary.py on the device), the numpy restatement of Geyer's rule with its branch
margins, and the comparison at the tolerances both files use.

A case is a raw buffer ``[groups, chains, iters_saved, D + 8]`` as the sampler writes it: seven
sampler columns, the D constrained parameters (AR(1) series in the unconstrained space, a
different phi per column, constrained by the library: ``exp`` on the log-transformed ones) and
``br``.  They are the smallest shapes at which each mechanism of the summary can go wrong.
The PCG64 seeds are chosen so that every Geyer branch of every compared column has a margin
of at least 1e-10 (``test_branch_margins``): a summation-order difference (about 1e-13) can
then never move the truncation lag.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from fitoct_amd import _lib
from fitoct_amd.api import DEFAULT_PROBS, ExpGPProblem
from fitoct_amd.stanfit import StanFit, materialise, output_columns

EPS = np.finfo(np.float64).eps


@dataclass
class Case:
    name: str
    probs_list: list            # one ExpGPProblem per group
    raw: np.ndarray             # [groups, chains, iters_saved, D + 8]
    first_iter: int = 0
    probs: tuple = DEFAULT_PROBS
    nan_rows: list = field(default_factory=list)   # (group, output column name) made NaN


def _problem(prior_type, Nn, **kw):
    x = np.linspace(20.0, 500.0, 16)
    return ExpGPProblem(x, 1000.0 + 0 * x, 1.0 + 0 * x, Nn=Nn, prior_type=prior_type, **kw)


def ar1(rng, chains, n, phi):
    """Stationary AR(1) with unit innovation variance, [chains, n]."""
    e = rng.standard_normal((chains, n))
    x = np.empty((chains, n))
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return x


def constrain(prob, q):
    q = np.ascontiguousarray(q, dtype=np.float64)
    out = np.empty_like(q)
    _lib.check(_lib.lib().fitoct_constrain(prob.family, prob.Nn, q.shape[0], _lib.dptr(q),
                                           _lib.dptr(out)))
    return out


def make_raw(prob, rng, chains, iters, phis=None, shift_chain=None):
    """One group's raw draws [chains, iters, D + 8]."""
    D = prob.D
    phis = np.linspace(0.1, 0.9, D) if phis is None else np.broadcast_to(phis, (D,))
    q = np.empty((chains, iters, D))
    for j in range(D):
        q[:, :, j] = 0.3 * np.sqrt(1 - phis[j] ** 2) * ar1(rng, chains, iters, phis[j])
    if shift_chain is not None:   # one chain off by 1.5 marginal sd in every coordinate
        q[shift_chain] += 1.5 * 0.3
    raw = np.empty((chains, iters, D + 8))
    raw[:, :, 7:7 + D] = constrain(prob, q.reshape(-1, D)).reshape(chains, iters, D)
    raw[:, :, 0] = -50.0 + 3.0 * ar1(rng, chains, iters, 0.5)            # lp__
    raw[:, :, 1] = rng.uniform(0.5, 1.0, (chains, iters))                # accept_stat__
    raw[:, :, 2] = rng.uniform(0.05, 0.2, (chains, 1))                   # stepsize__ (per chain)
    depth = rng.integers(1, 6, (chains, iters))
    raw[:, :, 3] = depth                                                 # treedepth__
    raw[:, :, 4] = 2.0 ** depth - 1                                      # n_leapfrog__
    raw[:, :, 5] = 0.0                                                   # divergent__
    raw[:, :, 6] = 60.0 + 4.0 * ar1(rng, chains, iters, 0.3)             # energy__
    raw[:, :, 7 + D] = np.exp(0.2 * ar1(rng, chains, iters, 0.4))        # br
    if prob.prior_PD:
        raw[:, :, 7 + D] = np.nan   # the sampler writes no br for a prior run
    return raw


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def case_a():
    p = _problem("horseshoe", 5)
    return Case("a", [p], make_raw(p, _rng(11), 4, 150)[None], first_iter=50)


def case_b():
    p = _problem("lasso", 4, lambda_scale=10.0)
    return Case("b", [p], make_raw(p, _rng(12), 3, 301, shift_chain=2)[None])


def case_c():
    rng = _rng(13)
    ps = [_problem("normal", 15, lambda_rate=0.05 * (g + 1)) for g in range(6)]
    raw = np.stack([make_raw(p, rng, 4, 40) for p in ps])
    raw[2, 1, 17, 7 + 4] = np.nan   # group 2, chain 1, iteration 17, parameter 4 (yGP.2)
    return Case("c", ps, raw, nan_rows=[(2, output_columns(ps[0])[7 + 4])])


def case_d():
    p = _problem("monoexp", 2)
    return Case("d", [p], make_raw(p, _rng(14), 2, 5000, phis=0.98)[None])


def case_e4():
    p = _problem("monoexp", 2)
    return Case("e4", [p], make_raw(p, _rng(15), 1, 4)[None])


def case_e5():
    p = _problem("monoexp", 2)
    return Case("e5", [p], make_raw(p, _rng(16), 1, 5)[None])


def case_g():
    p = _problem("horseshoe", 5, prior_PD=1)
    return Case("g", [p], make_raw(p, _rng(17), 4, 60)[None])


def case_h():
    p = _problem("normal", 3)
    rng = _rng(18)
    raw = make_raw(p, rng, 3, 101)
    raw[:, :, 3] = rng.integers(1, 4, (3, 101))   # heavy ties: three distinct values
    z = 1e-3 * ar1(rng, 3, 101, 0.2)              # crosses zero
    z[0, 5], z[1, 7], z[2, 9], z[0, 50] = -0.0, 0.0, 5e-324, -5e-324
    z[1, 60], z[2, 70], z[0, 80] = 1e-310, -1e-310, 0.0
    raw[:, :, 6] = z
    return Case("h", [p], raw[None], probs=(0.0, 0.025, 0.5, 0.975, 1.0))


CASES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d, "e4": case_e4, "e5": case_e5,
         "g": case_g, "h": case_h}


# ---- references --------------------------------------------------------------------------------
def stanfit_rows(case, g):
    """The parent route on group g: materialise, then StanFit.summary."""
    prob = case.probs_list[g]
    fit = StanFit(materialise(case.raw[g], prob), output_columns(prob), case.first_iter)
    return fit, fit.summary(probs=case.probs)


def column(fit, name):
    return fit.extract([name])[name]   # [chains, post-warmup n]


def geyer_margins(x):
    """Geyer's rule on x[chains, n] restated (as oracle/diag_np.py does, with the
    autocovariances by direct sums): (n_eff, smallest branch margin, truncation lag).  The
    margins: |rho_even + rho_odd| at every test of the initial positive sequence, the final
    |rho_even|, and every comparison of the initial monotone sequence."""
    x = np.asarray(x, float)
    n0 = x.shape[1]
    h = n0 // 2
    ch = np.concatenate([x[:, :h], x[:, n0 - h:]], axis=0)
    m, n = ch.shape
    c = ch - ch.mean(1, keepdims=True)
    acov = {}

    def ac(lag):
        if lag not in acov:
            acov[lag] = float(np.mean([np.dot(r[:n - lag], r[lag:]) / n for r in c])) if lag < n else 0.0
        return acov[lag]
    mean_var = float(np.mean(np.sum(c * c, 1) / (n - 1)))
    var_plus = mean_var * (n - 1) / n
    if m > 1:
        var_plus += ch.mean(1).var(ddof=1)
    margin = np.inf
    rho = np.zeros(n + 2)
    rho[0] = 1.0
    rho_even, rho_odd = 1.0, 1 - (mean_var - ac(1)) / var_plus
    rho[1] = rho_odd
    t = 1
    while t < n - 4:
        margin = min(margin, abs(rho_even + rho_odd))
        if not rho_even + rho_odd > 0:
            break
        rho_even = 1 - (mean_var - ac(t + 1)) / var_plus
        rho_odd = 1 - (mean_var - ac(t + 2)) / var_plus
        margin = min(margin, abs(rho_even + rho_odd))
        if rho_even + rho_odd >= 0:
            rho[t + 1], rho[t + 2] = rho_even, rho_odd
        t += 2
    max_t = t
    margin = min(margin, abs(rho_even))
    if rho_even > 0:
        rho[max_t + 1] = rho_even
    t = 1
    while t <= max_t - 2:
        margin = min(margin, abs((rho[t + 1] + rho[t + 2]) - (rho[t - 1] + rho[t])))
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = (rho[t - 1] + rho[t]) / 2
            rho[t + 2] = rho[t + 1]
        t += 2
    N = m * n
    tau = max(-1 + 2 * rho[:max_t + 1].sum() + rho[max_t + 1], 1 / np.log10(N))
    return float(N / tau), float(margin), max_t


# ---- comparison --------------------------------------------------------------------------------
def _close_or_both_nan(a, b, rel):
    if np.isnan(a) or np.isnan(b):
        return np.isnan(a) and np.isnan(b)
    return abs(a - b) <= rel * abs(b)


def check_row(row, want, flat, probs, what):
    """One table row (mean, se_mean, sd, quantiles, n_eff, Rhat) against a reference row given
    as the same sequence, at the tolerances of the summary's tests: Rhat 1e-10 and n_eff /
    se_mean 1e-8 relative (tests/test_abi.py); mean and sd within 4 S eps mean|x| (the
    worst-case bound of any summation order); quantiles within 4 eps max(|x_lo|, |x_hi|)."""
    np_ = len(probs)
    if np.all(np.isnan(want)):
        assert np.all(np.isnan(row)), (what, row)
        return
    S = flat.size
    tol = 4 * S * EPS * float(np.mean(np.abs(flat)))
    assert abs(row[0] - want[0]) <= tol, (what, "mean", row[0], want[0], tol)
    assert abs(row[2] - want[2]) <= tol, (what, "sd", row[2], want[2], tol)
    assert _close_or_both_nan(row[1], want[1], 1e-8), (what, "se_mean", row[1], want[1])
    assert _close_or_both_nan(row[3 + np_], want[3 + np_], 1e-8), (what, "n_eff", row[3 + np_],
                                                                  want[3 + np_])
    assert _close_or_both_nan(row[4 + np_], want[4 + np_], 1e-10), (what, "Rhat", row[4 + np_],
                                                                   want[4 + np_])
    srt = np.sort(flat)
    for i, p in enumerate(probs):
        hh = (S - 1) * p
        lo = int(np.floor(hh))
        hi = min(lo + 1, S - 1)
        qtol = 4 * EPS * max(abs(srt[lo]), abs(srt[hi]))
        assert abs(row[3 + i] - want[3 + i]) <= qtol, (what, f"q{p}", row[3 + i], want[3 + i])


def stanfit_row_values(r, probs):
    return np.array([r["mean"], r["se_mean"], r["sd"]] + [r[f"{100 * p:g}%"] for p in probs] +
                    [r["n_eff"], r["Rhat"]], dtype=np.float64)


def summary_config(case, max_staging_bytes=0, device=0):
    c = _lib.SummaryConfig()
    _lib.lib().fitoct_default_summary_config(C.byref(c))
    c.first_iter = case.first_iter
    c.n_probs = len(case.probs)
    for i, p in enumerate(case.probs):
        c.probs[i] = p
    c.max_staging_bytes = max_staging_bytes
    c.device = device
    return c
