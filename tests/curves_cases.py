"""Synthetic raw-layout draws for the posterior-curves tests (test_curves.py on the CPU,
test_gpu_curves.py on the device), the numpy restatement of the bands, and the bound both
files compare at.

A case is a raw buffer ``[groups, chains, iters_saved, D + 8]`` as the sampler writes it, with
theta a few per cent around the data's own decay and the GP coordinates drawn so that
``|yGP| <= 0.05`` (a real posterior's modulation is about +-0.1): ``1 + dL`` then stays away
from 0, which the bound needs (``test_bound_precondition``).  They are the smallest shapes at
which each mechanism of the curves can go wrong.

The bound is derived, not measured.  An order statistic, a mean and a type-7 quantile move by
at most sup_s |e_s| when every value moves by e_s, an sd by at most sqrt(S / (S - 1)) sup |e|.
Two correct evaluations of one draw's curves differ, with eps = 2^-53, by at most

    d_dL = (Nn + 2) eps sum_k |B_ik yGP_k|
    d_m  = theta2 e (|a| (4 eps + d_dL / (1 + dL)) + 4 eps) + 2 eps |m|     (a: exp's argument)
    d_r  = (d_m + eps |y - m|) / uy + eps |resid|

evaluated from the host's own per-draw curves (``fitoct_expgp_curves``); the bound of a bin is
8 times the maximum over the draws, for mean and sd plus the summation term
``4 S eps mean|value|`` of the summary's tests.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import numpy as np

from fitoct_amd import _lib
from fitoct_amd.api import CURVE_NAMES, DEFAULT_PROBS, ExpGPProblem, curves_blocks
from fitoct_amd.genquant import expgp_curves
from fitoct_amd.stanfit import materialise, output_columns

EPS = 2.0 ** -53
YGP_MAX = 0.05
THETA = np.array([40.0, 900.0, 150.0])


@dataclass
class Case:
    name: str
    probs_list: list            # one ExpGPProblem per group
    raw: np.ndarray             # [groups, chains, iters_saved, D + 8]
    first_iter: int = 0
    probs: tuple = DEFAULT_PROBS
    what: tuple = CURVE_NAMES
    nan_groups: tuple = ()


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def problem(prior_type, Nn, N, rng, **kw):
    """Data on the decay of THETA with a ripple and noise of sd uy."""
    x = np.linspace(20.0, 500.0, N)
    c = kw.get("dataType", 2)
    m = THETA[0] + THETA[1] * np.exp(-c * x / (THETA[2] * (1 + 0.03 * np.sin(x / 60.0))))
    uy = 2.0 + 0.02 * m
    return ExpGPProblem(x, m + uy * rng.standard_normal(N), uy, Nn=Nn, prior_type=prior_type, **kw)


def make_raw(prob, rng, chains, iters):
    """One group's raw draws [chains, iters, D + 8]: constrained values written directly."""
    D, Nn = prob.D, prob.Nn
    raw = np.empty((chains, iters, D + 8))
    raw[:, :, :7] = rng.standard_normal((chains, iters, 7))
    p = raw[:, :, 7:7 + D]
    p[...] = np.exp(0.3 * rng.standard_normal((chains, iters, D)))     # scales: positive
    p[:, :, :3] = THETA * (1 + 0.03 * rng.standard_normal((chains, iters, 3)))
    if prob.prior_type == "horseshoe":
        # raw order: theta[3] z[Nn] r1_global r2_global r1_local[Nn] r2_local[Nn] sigma;
        # yGP = z (r1_local sqrt(r2_local)) (r1_global sqrt(r2_global)), each factor bounded
        p[:, :, 3:3 + Nn] = rng.uniform(-1, 1, (chains, iters, Nn))
        p[:, :, 3 + Nn] = rng.uniform(0.05, 0.25, (chains, iters))
        p[:, :, 4 + Nn] = rng.uniform(0.2, 1.0, (chains, iters))
        p[:, :, 5 + Nn:5 + 2 * Nn] = rng.uniform(0.0, 0.4, (chains, iters, Nn))
        p[:, :, 5 + 2 * Nn:5 + 3 * Nn] = rng.uniform(0.0, 0.25, (chains, iters, Nn))
    elif prob.prior_type != "monoexp":
        p[:, :, 3:3 + Nn] = np.clip(0.02 * rng.standard_normal((chains, iters, Nn)),
                                    -YGP_MAX, YGP_MAX)
    raw[:, :, 7 + D] = np.exp(0.2 * rng.standard_normal((chains, iters)))   # br
    return raw


def case_a():
    rng = _rng(31)
    p = problem("horseshoe", 5, 37, rng)
    return Case("a", [p], make_raw(p, rng, 3, 151)[None], first_iter=50)


def case_b():
    rng = _rng(32)
    ps = []
    for g in range(6):
        kw = dict(dataType=1, kernel_conv=1) if g == 1 else {}
        ps.append(problem("normal", 15, 53 if g == 3 else 70, rng, **kw))
    ps[4] = dataclasses.replace(ps[4], B=0.9 * ps[4].basis()[0])   # a caller's basis
    return Case("b", ps, np.stack([make_raw(p, rng, 4, 40) for p in ps]))


def case_c():
    rng = _rng(33)
    p = problem("monoexp", 2, 16, rng)
    return Case("c", [p], make_raw(p, rng, 2, 60)[None])


def case_d():
    b = case_b()
    raw = b.raw.copy()
    raw[2, 1, 17, 7 + 3 + 6] = np.nan   # group 2, chain 1, iteration 17, yGP.7
    return Case("d", b.probs_list, raw, nan_groups=(2,))


def case_e():
    rng = _rng(35)
    p = problem("lasso", 24, 8, rng)
    return Case("e", [p], make_raw(p, rng, 8, 5000)[None])


PROBS16 = tuple(np.linspace(0.0, 1.0, 16))


def case_f(probs, what):
    a = case_a()
    return dataclasses.replace(a, name="f", probs=tuple(probs), what=tuple(what))


CASES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d, "e": case_e,
         "f-width2": lambda: case_f((), CURVE_NAMES),
         "f-16probs": lambda: case_f(PROBS16, CURVE_NAMES),
         "f-dL": lambda: case_f(DEFAULT_PROBS, ("dL",)),
         "f-m": lambda: case_f(DEFAULT_PROBS, ("m",)),
         "f-resid": lambda: case_f(DEFAULT_PROBS, ("resid",)),
         "f-dL-resid": lambda: case_f(DEFAULT_PROBS, ("dL", "resid"))}


# ---- references and the bound ------------------------------------------------------------------
def basis_of(prob):
    if prob.prior_type == "monoexp":
        return np.zeros((prob.N, 0))
    return prob.B if prob.B is not None else prob.basis()[0]


def pooled_params(case, g):
    """theta [S, 3] and yGP [S, Nn] of group g's pooled post-warmup draws, chain-major, as the
    OUTPUT layout has them (the library's materialise)."""
    prob = case.probs_list[g]
    names = output_columns(prob)
    rows = materialise(case.raw[g][:, case.first_iter:], prob)
    rows = rows.reshape(-1, rows.shape[-1])
    theta = rows[:, [names.index(f"theta.{k}") for k in (1, 2, 3)]]
    if prob.prior_type == "monoexp":
        return theta, np.zeros((rows.shape[0], 0))
    return theta, rows[:, [names.index(f"yGP.{k}") for k in range(1, prob.Nn + 1)]]


def draw_curves(prob, theta, ygp):
    """The host's own per-draw curves {dL, m, resid: [S, N]} (fitoct_expgp_curves)."""
    return expgp_curves(prob, theta, ygp, B=prob.B)


def value_bounds(prob, theta, ygp, cur):
    """Per-value difference of two correct evaluations, {dL, m, resid: [S, N]}."""
    B = basis_of(prob)
    Nn = B.shape[1]
    dL, m, r = cur["dL"], cur["m"], cur["resid"]
    d_dL = (Nn + 2) * EPS * (np.abs(ygp) @ np.abs(B).T) if Nn else np.zeros_like(dL)
    a = -float(prob.dataType) * prob.x[None, :] / (theta[:, 2:3] * (1 + dL))
    e = np.exp(a)
    d_m = np.abs(theta[:, 1:2]) * e * (np.abs(a) * (4 * EPS + d_dL / (1 + dL)) + 4 * EPS) \
        + 2 * EPS * np.abs(m)
    d_r = (d_m + EPS * np.abs(prob.y[None, :] - m)) / prob.uy[None, :] + EPS * np.abs(r)
    return {"dL": d_dL, "m": d_m, "resid": d_r}


def table_bounds(prob, theta, ygp, what, n_probs, cur=None):
    """The bound of every entry of one group's block [nq, N, 2 + n_probs]."""
    cur = draw_curves(prob, theta, ygp) if cur is None else cur
    vb = value_bounds(prob, theta, ygp, cur)
    S = theta.shape[0]
    out = np.empty((len(what), prob.N, 2 + n_probs))
    for q, name in enumerate(what):
        sup = 8 * np.max(vb[name], axis=0)
        summ = 4 * S * EPS * np.mean(np.abs(cur[name]), axis=0)
        out[q, :, 0] = sup + summ
        out[q, :, 1] = np.sqrt(S / (S - 1)) * sup + summ
        out[q, :, 2:] = sup[:, None]
    return out


def numpy_block(prob, theta, ygp, what, probs):
    """The bands restated in numpy: [nq, N, 2 + len(probs)]."""
    B = basis_of(prob)
    dL = ygp @ B.T if B.shape[1] else np.zeros((theta.shape[0], prob.N))
    m = theta[:, 0:1] + theta[:, 1:2] * np.exp(
        -float(prob.dataType) * prob.x[None, :] / (theta[:, 2:3] * (1 + dL)))
    vals = {"dL": dL, "m": m, "resid": (prob.y[None, :] - m) / prob.uy[None, :]}
    out = np.empty((len(what), prob.N, 2 + len(probs)))
    for q, name in enumerate(what):
        v = vals[name]
        out[q, :, 0] = v.mean(axis=0)
        out[q, :, 1] = v.std(axis=0, ddof=1)
        if probs:
            out[q, :, 2:] = np.quantile(v, probs, axis=0, method="linear").T
    if np.isnan(theta).any() or np.isnan(ygp).any():
        out[...] = np.nan
    return out


def ordered(what):
    return tuple(n for n in CURVE_NAMES if n in what)


def blocks(case, table):
    return curves_blocks(table, case.probs_list, case.what, case.probs)


def check_blocks(case, got, want, tag, report=None):
    """Every group's block of ``got`` against ``want`` (lists of [nq, N, w]): the same shape,
    the same NaN pattern, every entry within the bound.  ``report`` collects the largest ratio
    of difference to bound per quantity."""
    what = ordered(case.what)
    for g, prob in enumerate(case.probs_list):
        a, b = got[g], want[g]
        assert a.shape == b.shape == (len(what), prob.N, 2 + len(case.probs)), (tag, g, a.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (tag, g)
        if g in case.nan_groups:
            assert np.all(np.isnan(a)), (tag, g)
            continue
        theta, ygp = pooled_params(case, g)
        bound = table_bounds(prob, theta, ygp, what, len(case.probs))
        diff = np.abs(a - b)
        ratio = np.divide(diff, bound, out=np.where(diff > 0, np.inf, 0.0), where=bound > 0)
        for q, name in enumerate(what):
            worst = float(np.max(ratio[q]))
            print(f"{tag} group {g} {name}: largest difference / bound = {worst:.3g}")
            if report is not None:
                report[name] = max(report.get(name, 0.0), worst)
            assert worst <= 1.0, (tag, g, name, worst)


def summary_config(case, max_staging_bytes=0, device=0):
    from fitoct_amd.api import _summary_config
    return _summary_config(case.first_iter, case.probs, max_staging_bytes, device)
