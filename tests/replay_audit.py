"""Audit of a sampler run against the C oracle, transition by transition (numpy only: no
GPU import; the draws may come from the HIP sampler or from the oracle itself).

One NUTS transition is a pure function of six inputs: chain id, iteration index, start
position, step size, inverse metric and the Philox key.  A run with ``save_warmup`` stores
every iteration's position and ``stepsize__``; the metric is the unit metric until the
first window closes and follows from the saved warmup positions afterwards.  So every
stored transition can be recomputed on its own by the oracle, starting from the audited
run's own previous draw: rounding noise then has one transition to grow in, not hundreds,
and a fault shared by every path of the sampler has nowhere to hide.

Three groups of checks, each yielding named :class:`Finding` s (none = clean):

``row`` -- a stored row's own consistency (every row, every chain)
    ``lp``                lp__ is the oracle's log density at the row's parameters, within
                          ``tl (1 + |lp|) + 4 eps sum_k |g_k| (1 + |q_k|)``: the log-density
                          tolerance of test_gpu_logp.py (tl = 1e-11 in f64, 1e-5 mixed) plus
                          the first-order term of the log(exp(q)) round trip the stored
                          columns force, g = the oracle's gradient
    ``br``                br is sumr2 / N within 10 times that tolerance (NaN under prior_PD)
    ``energy``            energy__ + lp__ >= -tol (the kinetic energy is not negative)
    ``tree``              treedepth__ and n_leapfrog__ fit together (see TREE RULE below)
    ``accept_range``      0 <= accept_stat__ <= 1
    ``sampling_stepsize`` stepsize__ is constant over the sampling phase and is the returned
                          step size
    ``unmoved``           accept_stat__ == 0 (no leaf carried any weight): parameters and lp__
                          equal the previous row exactly
``adapt`` -- Stan's adaptation recurrences restated from the oracle's run_chain, 1e-9 relative
    ``dual_averaging``    within a window, stepsize__[t+1] follows from accept_stat__[..t]
    ``window_stepsize``   the first stepsize__ after a metric update is the oracle's
                          init_stepsize from the run's own position, metric and step size
    ``final_stepsize``    stepsize__[W] and the returned step size are exp(x_bar)
    ``metric``            the returned inverse metric is n/(n+5) var + 1e-3 5/(n+5) of the
                          last window's saved positions (the earlier windows' metrics enter
                          ``window_stepsize`` and the replay)
``replay`` -- every transition t >= 1 of the listed chains recomputed from row t-1 with
    eps = stepsize__[t] and the metric in force at t; all D + 8 columns compared with row t
    at 1e-6 relative, NaN equal to NaN (test_gpu_sampler.first_mismatch's rule).  Skipped
    for mixed precision, where the f64 oracle is not the same chain.

TREE RULE.  base_nuts::transition counts a doubling in treedepth__ only once its subtree
came back valid, and counts the leaves of a subtree that did not in n_leapfrog__.  With d
doublings completed the trajectory holds 2^d - 1 leaves, and a further, rejected subtree adds
between 2 (the shortest span a U-turn check sees) and 2^d leaves.  So without a divergence
``2^d - 1 <= n_leapfrog__ <= 2^(d+1) - 1``, ``n_leapfrog__ != 2^d``, ``0 <= d <=
max_treedepth``, and ``n_leapfrog__ == 2^d - 1`` at d = max_treedepth.  (The oracle's own
runs hold rows such as d = 1, n = 3; a rule ``n <= 2^d - 1`` would reject them.)
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field

import numpy as np

from oracle import nuts_c

RTOL_ADAPT = 1e-9
RTOL_REPLAY = 1e-6
LP_TOL = {"f64": 1e-11, "mixed": 1e-5}      # test_gpu_logp.TOL, log density
EPS = np.finfo(float).eps
SAMPLER_COLS = ["lp__", "accept_stat__", "stepsize__", "treedepth__", "n_leapfrog__",
                "divergent__", "energy__"]
GROUP = {"lp": "row", "br": "row", "energy": "row", "tree": "row", "accept_range": "row",
         "sampling_stepsize": "row", "unmoved": "row", "dual_averaging": "adapt",
         "window_stepsize": "adapt", "final_stepsize": "adapt", "metric": "adapt",
         "replay": "replay"}


@dataclass
class Finding:
    name: str
    chain: int            # index into draws (not the global id)
    t: int                # stored iteration, -1: a per-chain result
    detail: str = ""
    cols: tuple = ()      # replay: the columns that disagree

    @property
    def group(self):
        return GROUP[self.name]


@dataclass
class Audit:
    findings: list = field(default_factory=list)
    replayed: int = 0                 # transitions replayed
    replay_max_per_chain: int = 0     # most disagreeing transitions in one chain
    replay_max_rel: float = 0.0       # largest column difference among agreeing transitions
    replay_max_accept: float = 0.0    # ... of accept_stat__ alone
    window_ends: tuple = ()           # iterations whose transition closed a metric window

    def named(self, *groups):
        return [f for f in self.findings if not groups or f.group in groups]

    def names(self):
        return {f.name for f in self.findings}

    @property
    def replay_findings(self):
        return [f for f in self.findings if f.name == "replay"]

    @property
    def replay_share(self):
        return len(self.replay_findings) / self.replayed if self.replayed else 0.0

    def summary(self):
        return (f"{len(self.named('row'))} row, {len(self.named('adapt'))} adaptation findings; "
                f"replay {len(self.replay_findings)}/{self.replayed} disagree "
                f"(at most {self.replay_max_per_chain} in a chain), largest agreeing difference "
                f"{self.replay_max_rel:.2e} (accept_stat__ {self.replay_max_accept:.2e})")


def unconstrain(prob, params):
    """Stored parameter columns [..., D] -> unconstrained q (theta, the prior's scales and
    sigma are stored exponentiated; yGP / z as they are)."""
    D = prob.D
    Nn = 0 if prob.prior_type == "monoexp" else prob.Nn
    k = np.arange(D)
    is_log = (k < 3) | (k >= 3 + Nn)
    q = np.array(params, dtype=np.float64, copy=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        q[..., is_log] = np.log(q[..., is_log])
    return q


def window_schedule(cfg):
    """(ib, tb, window ends): run_chain's restatement of windowed_adaptation -- the
    iterations t < W whose position enters the running variance are ib <= t < W - tb, and a
    metric update follows the transitions listed in ``ends``."""
    W = cfg.warmup
    ib, tb, bw = cfg.init_buffer, cfg.term_buffer, cfg.window
    if W < 20 or not cfg.adapt_engaged:
        return ib, tb, []
    if ib + bw + tb > W:
        ib, tb = int(0.15 * W), int(0.1 * W)
        bw = W - (ib + tb)
    ends, size, nxt, last = [], bw, ib + bw - 1, W - tb - 1
    for t in range(W):
        if t == nxt:
            ends.append(t)
            if nxt != last:
                size *= 2
                nxt = t + size
                if nxt != last and nxt + 2 * size >= W - tb:
                    nxt = last
    return ib, tb, ends


def _rel(a, b, floor=1e-300):
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


def _rows(prob, cfg, draws, stepsize, precision, out):
    C_, T, _ = draws.shape
    D, W = prob.D, cfg.warmup if cfg.save_warmup else 0
    q = unconstrain(prob, draws[:, :, 7:7 + D])
    lp, g, s2 = nuts_c.logp_grad(prob, q.reshape(-1, D))
    lp, g, s2 = lp.reshape(C_, T), g.reshape(C_, T, D), s2.reshape(C_, T)
    tol = LP_TOL[precision] * (1 + np.abs(lp)) + 4 * EPS * np.sum(np.abs(g) * (1 + np.abs(q)), axis=2)
    glp, acc, eps = draws[:, :, 0], draws[:, :, 1], draws[:, :, 2]
    d, n, div, en, br = (draws[:, :, 3], draws[:, :, 4], draws[:, :, 5], draws[:, :, 6],
                         draws[:, :, 7 + D])

    def add(name, mask, fmt):
        for c, t in zip(*np.nonzero(mask)):
            out.append(Finding(name, int(c), int(t), fmt(c, t)))

    add("lp", ~(np.abs(glp - lp) <= tol),
        lambda c, t: f"lp__ {glp[c, t]!r} oracle {lp[c, t]!r} tol {tol[c, t]:.3g}")
    if prob.prior_PD:
        add("br", ~np.isnan(br), lambda c, t: f"br {br[c, t]!r} under prior_PD")
    else:
        ref = s2 / prob.N
        add("br", ~(np.abs(br - ref) <= 10 * tol),
            lambda c, t: f"br {br[c, t]!r} oracle {ref[c, t]!r} tol {10 * tol[c, t]:.3g}")
    add("energy", ~(en + glp >= -tol), lambda c, t: f"energy__ + lp__ = {en[c, t] + glp[c, t]!r}")
    di = np.where(np.isfinite(d), d, -1).astype(np.int64)
    whole = (d == di) & (n == np.floor(n)) & (di >= 0) & (di <= cfg.max_treedepth)
    lo = np.ldexp(1.0, np.clip(di, 0, 62)) - 1
    fits = whole & (n >= np.maximum(lo, 1)) & (n <= 2 * lo + 1) & (n != lo + 1)
    fits &= (di < cfg.max_treedepth) | (n == lo)
    divergent = div == 1
    bad_tree = np.where(divergent, ~(whole & (n >= 1) & (n <= 2 * lo + 1)), ~fits)
    bad_tree |= ~((div == 0) | divergent)
    add("tree", bad_tree, lambda c, t: f"treedepth__ {d[c, t]} n_leapfrog__ {n[c, t]} "
                                       f"divergent__ {div[c, t]}")
    add("accept_range", ~((acc >= 0) & (acc <= 1)), lambda c, t: f"accept_stat__ {acc[c, t]!r}")
    if T > W:
        want = eps[:, W:W + 1] if stepsize is None else np.asarray(stepsize)[:, None]
        m = np.zeros((C_, T), bool)
        m[:, W:] = eps[:, W:] != want
        add("sampling_stepsize", m, lambda c, t: f"stepsize__ {eps[c, t]!r}, the run's "
                                                 f"{want[c, 0]!r}")
    stay = np.zeros((C_, T), bool)
    same = (draws[:, 1:, 7:7 + D] == draws[:, :-1, 7:7 + D]).all(axis=2) & (glp[:, 1:] == glp[:, :-1])
    stay[:, 1:] = (acc[:, 1:] == 0) & ~same
    add("unmoved", stay, lambda c, t: "accept_stat__ 0 but the row differs from the one before")
    return q


def _adapt(prob, cfg, draws, q, gids, stepsize, inv_metric, nthreads, out):
    """Restates run_chain's adaptation over all chains at once.  Returns the inverse metric
    in force at every stored iteration [C, T, D] (for the replay)."""
    C_, T, _ = draws.shape
    D, W = prob.D, cfg.warmup
    acc, eps = draws[:, :, 1], draws[:, :, 2]
    minv_at = np.ones((C_, T, D))
    if not (cfg.adapt_engaged and cfg.save_warmup and W > 0):
        if inv_metric is not None:
            minv_at[:] = np.asarray(inv_metric)[:, None, :]
        return minv_at, ()
    ib, tb, ends = window_schedule(cfg)

    def add(name, t, got, want):
        for c in np.nonzero(~(_rel(got, want) <= RTOL_ADAPT))[0]:
            out.append(Finding(name, int(c), t, f"{got[c]!r}, the recurrence gives {want[c]!r} "
                                                f"(rel {_rel(got, want)[c]:.3g})"))

    minv = np.ones((C_, D))
    mu = np.full(C_, np.log(10 * cfg.stepsize))
    s_bar, x_bar, x = np.zeros(C_), np.zeros(C_), np.zeros(C_)
    da_n, win_start, window = 0, ib, 0
    for t in range(W):
        minv_at[:, t] = minv
        # stepsize_adaptation::learn_stepsize
        da_n += 1
        eta = 1.0 / (da_n + cfg.t0)
        s_bar = (1 - eta) * s_bar + eta * (cfg.adapt_delta - np.minimum(acc[:, t], 1.0))
        x = mu - s_bar * np.sqrt(float(da_n)) / cfg.gamma
        xe = float(da_n) ** (-cfg.kappa)
        x_bar = (1 - xe) * x_bar + xe * x
        if t in ends:
            # var_adaptation::learn_variance: the window's positions are saved rows
            win = q[:, win_start:t + 1]
            n = win.shape[1]
            if n > 1:
                var = ((win - win.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (n - 1)
            else:
                var = minv
            minv = (n / (n + 5.0)) * var + 1e-3 * (5.0 / (n + 5.0))
            win_start, window = t + 1, window + 1
            first = nuts_c.replay_init_stepsize(prob, cfg, gids, window, q[:, t], np.exp(x), minv,
                                                nthreads)
            if t + 1 < T:
                add("window_stepsize", t + 1, eps[:, t + 1], first)
                mu = np.log(10 * eps[:, t + 1])
            s_bar, x_bar, da_n = np.zeros(C_), np.zeros(C_), 0
        elif t + 1 < W:
            add("dual_averaging", t + 1, eps[:, t + 1], np.exp(x))
    final = np.exp(x_bar)
    if T > W:
        add("final_stepsize", W, eps[:, W], final)
        if stepsize is not None:
            add("final_stepsize", -1, np.asarray(stepsize), final)
    minv_at[:, W:] = minv[:, None, :]
    if inv_metric is not None:
        got = np.asarray(inv_metric)
        for c in np.nonzero(~(_rel(got, minv) <= RTOL_ADAPT).all(axis=1))[0]:
            k = int(np.argmax(_rel(got[c], minv[c])))
            out.append(Finding("metric", int(c), -1, f"inv_metric[{k}] {got[c, k]!r}, the window's "
                                                     f"positions give {minv[c, k]!r}"))
    return minv_at, tuple(ends)


def _replay(prob, cfg, draws, q, gids, minv_at, chains, columns, nthreads, audit, start_noise):
    T = draws.shape[1]
    if T < 2 or not len(chains):
        return
    chains = np.asarray(chains, dtype=np.int64)
    ts = np.arange(1, T)
    cc, tt = np.meshgrid(chains, ts, indexing="ij")
    cc, tt = cc.ravel(), tt.ravel()
    first = 0 if cfg.save_warmup else cfg.warmup     # the stored row's iteration index
    start = q[cc, tt - 1]
    if start_noise:   # the replay's own noise floor: every stored start column moved by
        D = prob.D    # +-start_noise, relative, before it is unconstrained
        sign = np.random.default_rng(1).choice([-1.0, 1.0], start.shape)
        start = unconstrain(prob, draws[cc, tt - 1, 7:7 + D] * (1 + start_noise * sign))
    rows = nuts_c.replay(prob, cfg, gids[cc], tt + first, start, draws[cc, tt, 2],
                         minv_at[cc, tt], nthreads)
    got = draws[cc, tt]
    rel = np.abs(got - rows) / np.maximum(np.abs(rows), 1e-12)
    rel = np.where(np.isnan(got) & np.isnan(rows), 0.0, rel)
    bad = ~(rel <= RTOL_REPLAY)
    bad_row = bad.any(axis=1)
    audit.replayed = int(cc.size)
    good = rel[~bad_row]
    if good.size:
        audit.replay_max_rel = float(good.max())
        audit.replay_max_accept = float(good[:, 1].max())
    per_chain = np.bincount(np.searchsorted(chains, cc[bad_row]), minlength=len(chains))
    audit.replay_max_per_chain = int(per_chain.max())
    for i in np.nonzero(bad_row)[0]:
        cols = tuple(columns[j] for j in np.nonzero(bad[i])[0])
        j = int(np.nanargmax(np.where(bad[i], np.nan_to_num(rel[i], nan=np.inf), -1.0)))
        audit.findings.append(Finding(
            "replay", int(cc[i]), int(tt[i]),
            f"{columns[j]} {got[i, j]!r}, the oracle from row {tt[i] - 1} gives {rows[i, j]!r}; "
            f"treedepth__ {got[i, 3]:g} / {rows[i, 3]:g}", cols))


def audit(prob, cfg, draws, stepsize=None, inv_metric=None, chains=None, replay=True,
          nthreads=16, start_noise=0.0):
    """Audit the draws [chains, W + S, D + 8] of a ``save_warmup`` run of ``cfg`` on ``prob``
    (``cfg.chain_offset`` + the chain's index is its global id).  ``stepsize`` [chains] and
    ``inv_metric`` [chains, D]: the run's returned values, checked too if given.  ``chains``:
    the (sorted) chain indices to replay, default all; ``replay=False`` or mixed precision:
    row and adaptation checks only.  ``start_noise``: relative perturbation of every
    replay's start, i.e. of the stored parameter columns of row t-1 (a stand-in for the summation-order noise of another
    implementation; measures how far one transition amplifies it).  Returns an
    :class:`Audit`."""
    draws = np.asarray(draws, dtype=np.float64)
    C_, T, ncols = draws.shape
    if ncols != prob.D + 8:
        raise ValueError(f"draws have {ncols} columns, the problem {prob.D + 8}")
    if T != (cfg.warmup if cfg.save_warmup else 0) + cfg.samples:
        raise ValueError("draws do not hold the configured iterations")
    a = Audit()
    gids = (cfg.chain_offset + np.arange(C_)).astype(np.int32)
    cfg64 = dataclasses.replace(cfg, precision="f64", devices=())
    q = _rows(prob, cfg, draws, stepsize, cfg.precision, a.findings)
    minv_at, a.window_ends = _adapt(prob, cfg64, draws, q, gids, stepsize, inv_metric, nthreads,
                                    a.findings)
    if replay and cfg.precision == "f64":
        sel = np.arange(C_) if chains is None else np.sort(np.asarray(chains))
        _replay(prob, cfg64, draws, q, gids, minv_at, sel, SAMPLER_COLS + list(
            prob.column_names()[7:]), nthreads, a, start_noise)
    return a
