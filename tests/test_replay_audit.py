"""The replay auditor (tests/replay_audit.py) on the CPU: the C oracle's own runs audit
clean, every planted fault is caught by name, and the replay's own noise floor is
measured on the shapes the GPU tests replay (tests/replay_cases.py).

Planted faults.  A fault in stored columns trips every check those columns enter (a row
whose parameters are wrong cannot have the right lp__, br and replay at once), so each
fault is pinned by its whole signature: the exact set of finding names, where they sit and
which columns the replay reports -- no finding outside it -- and the signatures differ
from each other."""
from __future__ import annotations

import numpy as np
import pytest

import replay_audit as RA
import replay_cases as RC
from fitoct_amd import SamplerConfig
from oracle import nuts_c

NTHREADS = 16
CHAINS = 4

SMALL = {"normal": lambda: RC.prob("normal", 64, 6), "horseshoe": lambda: RC.prob("horseshoe", 64, 4),
         "lasso": lambda: RC.prob("lasso", 64, 6), "monoexp": lambda: RC.prob("monoexp", 64, 6)}

_runs = {}


def oracle_run(family, W):
    """One oracle run per (family, warmup), shared and never modified."""
    if (family, W) not in _runs:
        prob = SMALL[family]()
        cfg = SamplerConfig(chains=CHAINS, warmup=W, samples=60, seed=5)
        o = nuts_c.sample(prob, cfg, nthreads=NTHREADS)
        for a in o.values():
            a.setflags(write=False)
        _runs[family, W] = (prob, cfg, o)
    return _runs[family, W]


@pytest.mark.parametrize("W", [150, 300])
@pytest.mark.parametrize("family", list(SMALL))
def test_oracle_output_audits_clean(family, W):
    """W = 150: one metric window, W = 300: three.  No finding of any kind, and not one
    replayed transition disagrees (the replay starts from the rounded log(exp(q)) of the
    stored columns, the run itself from q)."""
    prob, cfg, o = oracle_run(family, W)
    a = RA.audit(prob, cfg, o["draws"], o["stepsize"], o["inv_metric"], nthreads=NTHREADS)
    assert a.window_ends == ((99,) if W == 150 else (99, 149, 249))
    assert a.replayed == CHAINS * (W + 60 - 1)
    assert not a.findings, (a.summary(), a.findings[:5])


def test_tree_rule_matches_the_oracle():
    """The rule the auditor applies to treedepth__ / n_leapfrog__ (replay_audit TREE RULE)
    is tight on the oracle's own rows: they hold a rejected last subtree (n_leapfrog__ >
    2^d - 1) as well as whole trees (n_leapfrog__ == 2^d - 1)."""
    _, _, o = oracle_run("horseshoe", 300)
    d, n, div = (o["draws"][:, :, j].ravel() for j in (3, 4, 5))
    ok = div == 0
    assert np.any(ok & (n == 2 ** d - 1)) and np.any(ok & (n > 2 ** d - 1))
    assert np.all(n[ok] <= 2 ** (d[ok] + 1) - 1) and np.all(n[ok] >= 2 ** d[ok] - 1)


def _audit(prob, cfg, draws, o, **kw):
    return RA.audit(prob, cfg, draws, kw.pop("stepsize", o["stepsize"]),
                    kw.pop("inv_metric", o["inv_metric"]), nthreads=NTHREADS, **kw)


def _where(a, name):
    return {(f.chain, f.t) for f in a.findings if f.name == name}


def _moved_row(draws, W, c, cond=lambda t: True):
    """A sampling-phase row of chain c whose transition moved the chain, with a moved row
    after it too."""
    for t in range(W + 2, draws.shape[1] - 2):
        if draws[c, t, 7] != draws[c, t - 1, 7] and draws[c, t + 1, 7] != draws[c, t, 7] and cond(t):
            return t
    raise AssertionError("no such row")


def test_planted_accept_stat_with_one_leaf_missing():
    prob, cfg, o = oracle_run("horseshoe", 300)
    d = o["draws"].copy()
    W = cfg.warmup
    n = d[:, W:, 4]
    sel = n >= 2           # (n - 1) / n of a one-leaf tree is 0: a different fault ("unmoved")
    d[:, W:, 1] = np.where(sel, d[:, W:, 1] * (n - 1) / n, d[:, W:, 1])
    a = _audit(prob, cfg, d, o)
    assert a.names() == {"replay"}
    assert all(f.cols == ("accept_stat__",) for f in a.findings)
    want = {(c, W + t) for c, t in zip(*np.nonzero(sel))}
    assert _where(a, "replay") == want and want


def test_planted_accept_stat_in_warmup_breaks_dual_averaging():
    """The same fault in the warmup rows: the stored step sizes no longer follow from the
    stored acceptance statistics."""
    prob, cfg, o = oracle_run("normal", 300)
    d = o["draws"].copy()
    # inside the second window (100..149), a tree of several leaves
    t = next(t for t in range(110, 140) if d[0, t, 4] >= 2)
    d[0, t, 1] *= (d[0, t, 4] - 1) / d[0, t, 4]
    a = _audit(prob, cfg, d, o, replay=False)
    assert a.names() == {"dual_averaging", "window_stepsize"}
    # every later step size of that window, and the search after its metric update (t = 149)
    # starts from another step size
    assert _where(a, "dual_averaging") == {(0, u) for u in range(t + 1, 150)}
    assert _where(a, "window_stepsize") == {(0, 150)}


def test_planted_lp_and_br_of_the_previous_row():
    prob, cfg, o = oracle_run("normal", 300)
    d = o["draws"].copy()
    D, W = prob.D, cfg.warmup
    # lp__ falls at that row: energy__ + (the larger, stale) lp__ stays positive
    t = _moved_row(d, W, 1, lambda t: d[1, t - 1, 0] > d[1, t, 0])
    d[1, t, 0], d[1, t, 7 + D] = d[1, t - 1, 0], d[1, t - 1, 7 + D]
    a = _audit(prob, cfg, d, o)
    assert a.names() == {"lp", "br", "replay"}
    assert _where(a, "lp") == _where(a, "br") == _where(a, "replay") == {(1, t)}
    assert a.replay_findings[0].cols == ("lp__", "br")


def test_planted_stepsize_shifted_by_one_iteration():
    prob, cfg, o = oracle_run("normal", 300)
    d = o["draws"].copy()
    W = cfg.warmup
    d[2, 1:, 2] = o["draws"][2, :-1, 2]
    a = _audit(prob, cfg, d, o)
    assert a.names() == {"dual_averaging", "window_stepsize", "final_stepsize",
                         "sampling_stepsize", "replay"}
    assert {c for f in a.findings for c in [f.chain]} == {2}
    # the step size of row W is still the last warmup one; the first after each metric
    # update is the one before the search
    assert _where(a, "sampling_stepsize") == {(2, W)}
    assert _where(a, "final_stepsize") == {(2, W), (2, -1)}   # -1: against the returned one
    assert _where(a, "window_stepsize") == {(2, e + 1) for e in a.window_ends}
    # the replay takes the row's own step size: that column agrees, the transition does not
    assert all("stepsize__" not in f.cols and 1 <= f.t <= W for f in a.replay_findings)
    assert len(a.replay_findings) > W // 2


def test_planted_metric_with_n_for_n_minus_1():
    prob, cfg, o = oracle_run("horseshoe", 300)
    n = 100.0             # the last window: iterations 150..249
    var = (o["inv_metric"] - 1e-3 * 5 / (n + 5)) * (n + 5) / n
    bad = (n / (n + 5)) * var * (n - 1) / n + 1e-3 * 5 / (n + 5)
    a = _audit(prob, cfg, o["draws"], o, inv_metric=bad, replay=False)
    assert a.names() == {"metric"}
    assert _where(a, "metric") == {(c, -1) for c in range(CHAINS)}


def test_planted_swap_of_two_ygp_columns():
    prob, cfg, o = oracle_run("normal", 300)
    d = o["draws"].copy()
    t = _moved_row(d, cfg.warmup, 3)
    d[3, t, [7 + 3, 7 + 4]] = d[3, t, [7 + 4, 7 + 3]]
    a = _audit(prob, cfg, d, o)
    assert a.names() == {"lp", "br", "replay"}
    assert _where(a, "lp") == _where(a, "br") == {(3, t)}
    # the row is not what the row before leads to, and leads nowhere near the row after
    assert _where(a, "replay") == {(3, t), (3, t + 1)}
    by_t = {f.t: f.cols for f in a.replay_findings}
    assert by_t[t] == ("yGP.1", "yGP.2")
    assert {"lp__", "yGP.1", "yGP.2"} <= set(by_t[t + 1])


def test_planted_treedepth_off_by_one():
    prob, cfg, o = oracle_run("horseshoe", 300)
    d = o["draws"].copy()
    W = cfg.warmup
    # a whole tree: n_leapfrog__ = 2^d - 1 cannot belong to depth d + 1
    t = next(t for t in range(W, d.shape[1]) if d[0, t, 4] == 2 ** d[0, t, 3] - 1 and d[0, t, 5] == 0)
    d[0, t, 3] += 1
    a = _audit(prob, cfg, d, o)
    assert a.names() == {"tree", "replay"}
    assert _where(a, "tree") == _where(a, "replay") == {(0, t)}
    assert a.replay_findings[0].cols == ("treedepth__",)


def test_planted_transition_of_another_chain():
    """Row t of chain 1 becomes the transition chain 2's random numbers make from the same
    state (same start, step size and metric): a consistent row that follows from the one
    before -- under the wrong key.  Only the replay can see it."""
    prob, cfg, o = oracle_run("normal", 300)
    d = o["draws"].copy()
    W = cfg.warmup
    t = W + 20
    q = RA.unconstrain(prob, d[1:2, t - 1, 7:7 + prob.D])
    d[1, t] = nuts_c.replay(prob, cfg, [2], [t], q, d[1, t, 2], o["inv_metric"][1:2])[0]
    assert not np.array_equal(d[1, t], o["draws"][1, t])
    a = _audit(prob, cfg, d, o)
    assert a.names() == {"replay"}
    # row t + 1 was made from the original row t
    assert _where(a, "replay") == {(1, t), (1, t + 1)}
    assert all("lp__" in f.cols and "theta.1" in f.cols for f in a.replay_findings)


# the replay's noise floor ------------------------------------------------------------------
NOISE, NOISE_SHARE = 1e-12, 0.002
SLOW = {"headline", "batch", "config2", "compact16", "streamed", "poly_one_chain",
        "user_basis_streamed"}          # more than a few seconds each on 16 threads


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.slow) if n in SLOW else n
                                  for n in RC.REPLAY])
def test_replay_noise_floor(name):
    """Every shape the GPU tests replay, on the oracle alone: run it, then replay every
    transition from a start moved by a relative 1e-12 (every stored parameter column of the
    row before, full magnitude, random sign) -- a stand-in for the per-leaf
    summation-order differences of another implementation.  At most 0.2 % of the transitions
    may then leave the 1e-6 of the comparison; that is what lets the GPU tests' 1 % cap hold
    for the reference alone.  A case that fails this gets a smaller max_treedepth, not a
    wider cap.  The measured table is in DESIGN.md (parity notes)."""
    case = RC.REPLAY[name]
    probs = case.make()
    n_rep = len(case.replayed())
    bad = total = 0
    worst = 0.0
    for p, prob in enumerate(probs if isinstance(probs, list) else [probs]):
        cfg = case.cfg(chains=n_rep, chain_offset=p * n_rep)
        o = nuts_c.sample(prob, cfg, nthreads=NTHREADS)
        clean = RA.audit(prob, cfg, o["draws"], o["stepsize"], o["inv_metric"], nthreads=NTHREADS)
        assert not clean.findings, (clean.summary(), clean.findings[:5])
        a = RA.audit(prob, cfg, o["draws"], o["stepsize"], o["inv_metric"], nthreads=NTHREADS,
                     start_noise=NOISE)
        assert not a.named("row", "adapt")
        bad, total = bad + len(a.replay_findings), total + a.replayed
        worst = max(worst, a.replay_max_rel)
    print(f"noise floor {name}: {bad} of {total} beyond 1e-6, largest agreeing {worst:.1e}")
    assert bad <= NOISE_SHARE * total, (bad, total)
