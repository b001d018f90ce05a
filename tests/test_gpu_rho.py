"""HIP lp and grad lp over the GP length scale rho (rho_cases.CASES): every sweep and moments
path a plan can take as rho moves -- the factorised basis at 4, 8 and 16 bins per lane and
streamed, with and without the geometric moments, powers to e^400, and the row fallbacks
behind build_poly's overflow guard and accuracy gate -- each with its route asserted from a
plan's info, against the numpy model on a basis that does not come from the code under test.

Tier 1 (kappa2 <= 1e4): the exact basis (60 digits, rounded once), the tolerances of
test_gpu_logp.py unchanged, both precisions.
Tier 2, rows (kappa2 ~ 1e10): the library's own Cholesky basis handed to the numpy model only
-- the GPU problem keeps B = NULL, so route selection and staging are the library's; that
basis itself is held to the exact one by test_basis_rho.py.  f64.
Tier 2, factorised: the exact basis, the same tolerances plus a bracket: the reference is
re-evaluated on B +- dB S with dB = (3 Nn + 1 + E) eps kappa2 max|B| per entry (the Cholesky
solve's forward bound plus the relative rounding of a t^l b_l, whose exponents reach E) and
worst-case and random sign patterns S; the allowance per output is twice the largest
deviation.  The measured errors as fractions of it are printed (length scale).

No point of any case has a non-finite reference; none is skipped."""
from __future__ import annotations

import math

import numpy as np
import pytest

import rho_cases as R
from fitoct_amd import Plan, SamplerConfig, logp_grad
from oracle import model_np as M
from planner_env import switches
from test_gpu_logp import TOL

pytestmark = pytest.mark.gpu

TIER1 = [c for c in R.CASES if c.tier == "exact"]
TIER2_ROWS = [c for c in R.CASES if c.tier == "rows"]


def _route(prob):
    """(basis_mode, bins_per_thread) of a sampler plan for the problem, created, not run."""
    with switches(), Plan(prob, SamplerConfig(chains=4, warmup=10, samples=10)) as pl:
        return pl.info["basis_mode"], pl.info["bins_per_thread"]


def _gpu(prob, Q, prec):
    with switches():
        return logp_grad(prob, Q, prec)


def _errors(lp, g, s2, ref, Q):
    """Per point: (|lp - ref|, |g - ref| per coordinate, |sumr2 - ref|) and the references;
    every reference value must be finite."""
    out = []
    for i, q in enumerate(Q):
        rl, rg, rs = M.logp_grad(q, ref)
        assert math.isfinite(rl) and np.all(np.isfinite(rg)) and math.isfinite(rs), (i, rl, rs)
        out.append((abs(lp[i] - rl), np.abs(g[i] - rg), abs(s2[i] - rs), rl, rg, rs))
    return out


def _check(case, prec, lp, g, s2, ref, Q, allow=None):
    """The tolerances of test_gpu_logp._check, relative to 1 + |ref|, plus ``allow[i]`` =
    (lp, grad[D], sumr2) absolute allowances where given.  Returns the largest ratios of
    error to tolerance (lp, grad)."""
    tl, tg = TOL[prec]
    worst = [0.0, 0.0]
    for i, (el, eg, es, rl, rg, rs) in enumerate(_errors(lp, g, s2, ref, Q)):
        al, ag, as_ = allow[i] if allow else (0.0, 0.0, 0.0)
        print(f"rho {case.id} {prec} point {i}: lp err {el / (1 + abs(rl)):.2e} "
              f"grad err {(eg / (1 + np.abs(rg))).max():.2e}")
        assert el <= tl * (1 + abs(rl)) + al, (case.id, i, lp[i], rl)
        bad = eg - (tg * (1 + np.abs(rg)) + ag)
        assert bad.max() <= 0, (case.id, i, int(bad.argmax()), eg[bad.argmax()])
        assert es <= 10 * tl * (1 + abs(rs)) + as_, (case.id, i, s2[i], rs)
        worst[0] = max(worst[0], el / (tl * (1 + abs(rl)) + al))
        worst[1] = max(worst[1], float((eg / (tg * (1 + np.abs(rg)) + ag)).max()))
    return worst


@pytest.mark.parametrize("prec", ["f64", "mixed"])
@pytest.mark.parametrize("case", TIER1, ids=lambda c: c.id)
def test_tier1_exact_basis(case, prec):
    ex = case.exact()
    assert ex.kappa <= 1e4
    prob = case.problem()
    assert _route(prob) == (case.mode, case.bpt)
    Q = case.points(ex.bmax)
    _check(case, prec, *_gpu(prob, Q, prec), case.reference(ex.B), Q)


@pytest.mark.parametrize("case", TIER2_ROWS, ids=lambda c: c.id)
def test_tier2_rows_on_the_library_basis(case):
    prob = case.problem()
    assert prob.B is None
    assert _route(prob) == (case.mode, case.bpt) and case.mode == R.ROWS
    B, _ = prob.basis()
    Q = case.points(float(np.abs(B).max()))
    _check(case, "f64", *_gpu(prob, Q, "f64"), case.reference(B), Q)


# ---- tier 2, factorised: the bracket ---------------------------------------------------------
def _ygp(case, q):
    fam = M.FAMILIES[case.family]
    if fam == M.HORSESHOE:
        return M.horseshoe_ygp(M.constrain(q, fam, case.Nn), case.Nn)[0]
    return q[3:3 + case.Nn]


def bracket(case, ex, Q):
    """Per point the allowance (lp, grad[D], sumr2): twice the largest deviation of the
    reference over B +- dB S, S_ik = s_i sign(yGP_k): s = sign(d lp / d dL_i) (every entry's
    error pushes lp the same way; d lp / d dL_i has the sign of the residual y_i - m_i) and
    six fixed-seed random +-1 vectors."""
    dB = (3 * case.Nn + 1 + ex.E) * R.EPS * ex.kappa * ex.bmax
    d = case.data()
    rng = np.random.default_rng(20240229)
    rand = rng.choice([-1.0, 1.0], (6, case.N))
    allow = []
    for q in Q:
        ref = case.reference(ex.B)
        l0, g0, s0 = M.logp_grad(q, ref)
        y = _ygp(case, q)
        th = np.exp(q[0:3])
        m = th[0] + th[1] * np.exp(-2.0 * d["x"] / (th[2] * (1.0 + ex.B @ y)))
        dev = [0.0, np.zeros_like(g0), 0.0]
        for s in [np.sign(d["y"] - m)] + list(rand):
            for sg in (1.0, -1.0):
                S = sg * s[:, None] * np.sign(y)[None, :]
                l, g, s2 = M.logp_grad(q, case.reference(ex.B + dB * S))
                assert math.isfinite(l)
                dev = [max(dev[0], abs(l - l0)), np.maximum(dev[1], np.abs(g - g0)),
                       max(dev[2], abs(s2 - s0))]
        allow.append((2 * dev[0], 2 * dev[1], 2 * dev[2]))
    return dB, allow


def _fractions(lp, g, s2, ref, Q, allow):
    """Largest measured error as a fraction of the bracket's allowance alone (lp, grad), over
    the outputs the basis enters (a coordinate whose gradient does not depend on B has no
    allowance and is held by the plain tolerance)."""
    fl = fg = 0.0
    for (el, eg, es, *_), (al, ag, as_) in zip(_errors(lp, g, s2, ref, Q), allow):
        fl = max(fl, el / al)
        dep = ag > 0
        fg = max(fg, float((eg[dep] / ag[dep]).max()))
    return fl, fg


def test_tier2_factorised_streamed_wide():
    case = R.BY_ID["streamed_wide"]
    ex = case.exact()
    prob = case.problem()
    assert _route(prob) == (R.POLY, 0)
    Q = case.points(ex.bmax)
    dB, allow = bracket(case, ex, Q)
    ref = case.reference(ex.B)
    out = _gpu(prob, Q, "f64")
    print(f"rho streamed_wide: kappa2 {ex.kappa:.2e} E {ex.E:.1f} dB {dB:.2e}; error as a "
          f"fraction of the allowance: lp %.2e grad %.2e" % _fractions(*out, ref, Q, allow))
    _check(case, "f64", *out, ref, Q, allow)


def test_at_gate_route_recorded_and_both_routes_measured():
    """Nn = 12, internal grid, rho 0.19: the factorised basis reproduces the Cholesky one to
    about 7e-10 max|B|, next to build_poly's gate.  Whichever route the library takes is held
    to the exact reference within the bracket; the other route (reached, for the rows, by
    handing the library's own Cholesky basis to the GPU problem) is measured beside it."""
    case = R.BY_ID["at_gate"]
    ex = case.exact()
    prob = case.problem()
    mode, bpt = _route(prob)
    print(f"rho at_gate: route basis_mode {mode} bins_per_thread {bpt}, kappa2 {ex.kappa:.2e}")
    assert (mode, bpt) in ((R.POLY, 4), (R.ROWS, 0))
    Q = case.points(ex.bmax)
    dB, allow = bracket(case, ex, Q)
    ref = case.reference(ex.B)
    taken = _gpu(prob, Q, "f64")
    B, _ = prob.basis()
    rows_prob = case.problem(B=B)
    assert _route(rows_prob) == (R.ROWS, 0)
    rows = taken if mode == R.ROWS else _gpu(rows_prob, Q, "f64")
    print("rho at_gate: error vs the exact reference as a fraction of the allowance: "
          "route taken lp %.2e grad %.2e;" % _fractions(*taken, ref, Q, allow),
          "rows on the Cholesky basis lp %.2e grad %.2e" % _fractions(*rows, ref, Q, allow))
    # the rows route computes exactly its basis: tight against the numpy model on that basis
    _check(case, "f64", *rows, case.reference(B), Q)
    _check(case, "f64", *taken, ref, Q, allow)
