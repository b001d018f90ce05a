"""Cases and the numpy restatement for the pairs-plot tests (test_pairs.py on the CPU,
test_gpu_pairs.py on the device): include/fitoct.h "pairs plot".

The raw buffers are summary_cases' (``make_raw``, ``_problem``, ``_rng``), the smallest shapes at
which each mechanism can go wrong:

  p1   horseshoe Nn=5, 4 x 150, first_iter 50 (S = 400): all 40 columns, 7 bins, 2 planes;
       transformed columns, divergent__ = 1 on a seeded 10 % of the draws, automatic ranges
  p2   lasso Nn=4, 3 x 301 (S = 903: odd, no multiple of 16): five columns in a chosen order,
       64 bins, ranges at (0.05, 0.95); the constant ``lambda`` has no grid
  p3   normal Nn=15, 6 groups x 4 x 40, a NaN at group 2 / yGP.2: the default pars (22 columns,
       231 panels), 16 bins, 2 planes; p3c is the same buffer without the NaN
  p4a  monoexp 2 x 5000: one column, 2 bins, geometric edges (no panel at all)
  p4b  the same, two columns, 32 bins, geometric edges
  p5a  normal Nn=3, 3 x 101 with summary_cases.case_h's ties and signed zeros: treedepth__ over
       (1, 3) and energy__ over (0, its maximum), 2 bins
  p5b  the same, 5 bins
  p6   monoexp 1 x 4 (S = 4): two columns, 2 bins, the smallest accepted call
  p7   normal Nn=15, 3 groups x 4 x 6001 (S = 24004), the default pars, 32 bins, 2 planes: the
       sizes at which the device route's loops take more than one turn.  752 row blocks per
       group against 2048 / 3 = 682 slabs: a slab of the correlation spans one or two row
       blocks, the last block of a chain is short (6001 = 187 x 32 + 17); 66 panel work items x
       3 groups leave 1024 / 198 = 5 shares for 6 blocks of 256 sixteen-byte vectors, so the
       panels' grid-stride loop strides
  p8   monoexp 3 x 45001 (S = 135003 > 32 x 256 x 16): two columns, 64 bins, 2 planes: the
       marginals' grid-stride loop strides (33 blocks of vectors on 32 workgroups), the largest
       panel grid (32 KiB of LDS), 4221 row blocks on 2048 slabs
  p9   horseshoe Nn=24, 2 x 40: the first 64 columns, 64 bins: the largest edge array beside
       the widest row tile in the digitising kernel's LDS (55.6 KB)

The restatement takes the edges a call returned and counts with ``np.histogram`` /
``np.histogram2d`` on the ``materialise``d columns; the correlation is ``np.corrcoef``'s within
|dr| <= 8 S eps (1 + |mean_a| / sd_a) (1 + |mean_b| / sd_b): the rounding of a centred length-S
dot product and of its centring, whatever the order of summation.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass, field

import numpy as np

import summary_cases as SC
from fitoct_amd.stanfit import _base, materialise, output_columns

EPS = np.finfo(np.float64).eps


@dataclass
class Case:
    name: str
    probs_list: list            # one ExpGPProblem per group
    raw: np.ndarray             # [groups, chains, iters_saved, D + 8]
    first_iter: int = 0
    pars: tuple = None          # None: the default pars
    n_bins: int = 32
    planes: int = 1
    range_probs: tuple = (0.0, 1.0)
    ranges: dict = None         # {column name: (lo, hi)}
    log: tuple = ()
    nan_cols: list = field(default_factory=list)   # (group, column name) holding a NaN

    @property
    def S(self):
        return self.raw.shape[1] * (self.raw.shape[2] - self.first_iter)

    @property
    def exact_edges(self):
        """Both routes hold identical edges: no interpolated quantile is involved."""
        return tuple(self.range_probs) == (0.0, 1.0) or self.ranges is not None

    def kwargs(self):
        return dict(first_iter=self.first_iter, pars=self.pars, n_bins=self.n_bins,
                    planes=self.planes, range_probs=self.range_probs, ranges=self.ranges,
                    log=self.log)


def case_p1():
    a = SC.case_a()
    raw = a.raw.copy()
    rng = SC._rng(31)
    div = rng.random(raw.shape[:3]) < 0.10
    raw[..., 5] = div
    return Case("p1", a.probs_list, raw, first_iter=50, pars=tuple(output_columns(a.probs_list[0])),
                n_bins=7, planes=2)


def case_p2():
    b = SC.case_b()
    return Case("p2", b.probs_list, b.raw, pars=("lp__", "yGP.2", "theta.1", "lambda", "sigma"),
                n_bins=64, range_probs=(0.05, 0.95))


def _p3(with_nan):
    rng = SC._rng(13)   # summary_cases.case_c's buffer
    ps = [SC._problem("normal", 15, lambda_rate=0.05 * (g + 1)) for g in range(6)]
    raw = np.stack([SC.make_raw(p, rng, 4, 40) for p in ps])
    nan_cols = []
    if with_nan:
        raw[2, 1, 17, 7 + 4] = np.nan
        nan_cols = [(2, output_columns(ps[0])[7 + 4])]
    return Case("p3" if with_nan else "p3c", ps, raw, n_bins=16, planes=2, nan_cols=nan_cols)


def case_p3():
    return _p3(True)


def case_p3c():
    return _p3(False)


def case_p4a():
    d = SC.case_d()
    return Case("p4a", d.probs_list, d.raw, pars=("theta.1",), n_bins=2, log=("theta",))


def case_p4b():
    d = SC.case_d()
    return Case("p4b", d.probs_list, d.raw, pars=("theta.1", "theta.2"), n_bins=32, log=("theta",))


def _p5(name, n_bins):
    h = SC.case_h()
    top = float(np.max(h.raw[0, :, :, 6]))
    return Case(name, h.probs_list, h.raw, pars=("treedepth__", "energy__"), n_bins=n_bins,
                ranges={"treedepth__": (1.0, 3.0), "energy__": (0.0, top)})


def case_p5a():
    return _p5("p5a", 2)


def case_p5b():
    return _p5("p5b", 5)


def case_p6():
    e = SC.case_e4()
    return Case("p6", e.probs_list, e.raw, pars=("theta.1", "theta.3"), n_bins=2)


def _divergent(raw, seed):
    raw[..., 5] = SC._rng(seed).random(raw.shape[:3]) < 0.10
    return raw


def case_p7():
    rng = SC._rng(37)
    ps = [SC._problem("normal", 15, lambda_rate=0.05 * (g + 1)) for g in range(3)]
    raw = _divergent(np.stack([SC.make_raw(p, rng, 4, 6001) for p in ps]), 38)
    return Case("p7", ps, raw, n_bins=32, planes=2)


def case_p8():
    p = SC._problem("monoexp", 2)
    raw = _divergent(SC.make_raw(p, SC._rng(39), 3, 45001)[None], 40)
    return Case("p8", [p], raw, pars=("theta.1", "theta.2"), n_bins=64, planes=2)


def case_p9():
    p = SC._problem("horseshoe", 24)
    return Case("p9", [p], SC.make_raw(p, SC._rng(41), 2, 40)[None],
                pars=tuple(output_columns(p)[:64]), n_bins=64)


CASES = {"p1": case_p1, "p2": case_p2, "p3": case_p3, "p3c": case_p3c, "p4a": case_p4a,
         "p4b": case_p4b, "p5a": case_p5a, "p5b": case_p5b, "p6": case_p6, "p7": case_p7, "p8": case_p8, "p9": case_p9}
UNIT_RANGE = ("p1", "p3", "p3c", "p4a", "p4b", "p6", "p7", "p8", "p9")   # range_probs (0, 1), no explicit range


# ---- the restatement -----------------------------------------------------------------------------
def pooled(case, g):
    """(values [S, P] of group g's pooled post-warmup draws in the output layout, the output
    column names, divergent [S])."""
    prob = case.probs_list[g]
    names = output_columns(prob)
    m = materialise(case.raw[g], prob)[:, case.first_iter:, :].reshape(-1, len(names))
    div = case.raw[g][:, case.first_iter:, 5].reshape(-1) != 0
    return m, names, div


def formula_edges(lo, hi, nb, log):
    k = np.arange(nb + 1)
    return lo * np.exp(np.log(hi / lo) * k / nb) if log else lo + (hi - lo) * (k / nb)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_group(case, t, g, summary, what):
    """Group g of the tables ``t`` (api.pairs_host / pairs_device over the groups) against the
    definitions; ``summary`` is the same route's summary table [G, P, 7] at the case's
    range_probs.  Returns the largest correlation difference over its bound."""
    m, names, div = pooled(case, g)
    cols, S, nb = t["columns"], case.S, case.n_bins
    assert t["S"] == S
    idx = [names.index(c) for c in cols]
    logs = [c in case.log or _base(c) in case.log for c in cols]
    planes = [np.ones(S, bool), div][:case.planes]
    grid = []
    for j, c in enumerate(cols):
        v, e = m[:, idx[j]], t["edges"][g, j]
        tag = (what, g, c)
        given = (case.ranges or {}).get(c)
        lo, hi = given if given else summary[g, idx[j], 3:5]
        has_grid = (not np.isnan(v).any() and np.isfinite(lo) and np.isfinite(hi) and lo < hi
                    and not (logs[j] and lo <= 0))
        if has_grid:   # (strictly increasing edges: asserted below, every case's are)
            assert _bits(e[0]) == _bits(lo) and _bits(e[-1]) == _bits(hi), tag
            assert np.all(np.diff(e) > 0), tag
            want = formula_edges(lo, hi, nb, logs[j])
            assert np.all(np.abs(e - want) <= 4 * EPS * max(abs(lo), abs(hi))), (tag, e - want)
        else:
            assert np.all(np.isnan(e)), tag
        grid.append(has_grid)
        for pl, mask in enumerate(planes):
            want = np.histogram(v[mask], bins=e)[0] if has_grid else np.zeros(nb, np.int64)
            assert np.array_equal(t["hist"][g, j, pl], want), (tag, pl)
        out = (np.sum(v < e[0]), np.sum(v > e[-1])) if has_grid else (0, 0)
        assert tuple(t["outside"][g, j]) == out, tag
        if has_grid:
            assert t["hist"][g, j, 0].sum() + t["outside"][g, j].sum() == S, tag
    pn = 0
    for a in range(len(cols)):
        for b in range(a + 1, len(cols)):
            for pl, mask in enumerate(planes):
                got = t["panels"][g, pn, pl]
                if grid[a] and grid[b]:
                    want = np.histogram2d(m[mask, idx[a]], m[mask, idx[b]],
                                          bins=[t["edges"][g, a], t["edges"][g, b]])[0]
                    assert np.array_equal(got, want), (what, g, cols[a], cols[b], pl)
                    if case.name in UNIT_RANGE:   # the marginals of a panel are the columns'
                        assert np.array_equal(got.sum(axis=1), t["hist"][g, a, pl])
                        assert np.array_equal(got.sum(axis=0), t["hist"][g, b, pl])
                else:
                    assert not got.any(), (what, g, cols[a], cols[b], pl)
            pn += 1
    assert pn == t["panels"].shape[1]
    return check_corr(t["corr"][g], m[:, idx], f"{what} group {g}")


def no_corr(x):
    """The columns of x[S, n_cols] that have no correlation: a NaN, or zero variance."""
    return np.isnan(x).any(axis=0) | np.all(x == x[0], axis=0)


def corr_bound(x):
    """[n_cols, n_cols] bound of the correlation's rounding for the columns x[S, n_cols] (NaN
    where a column has no correlation)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(no_corr(x), np.nan, 1 + np.abs(x.mean(axis=0)) / x.std(axis=0))
    return 8 * x.shape[0] * EPS * np.outer(f, f)


def check_corr(corr, x, what, reference=None):
    """corr against np.corrcoef of x[S, n_cols] (or against ``reference``) within the bound;
    exact diagonal, bit symmetry, NaN exactly for the columns with a NaN or zero variance."""
    bound = corr_bound(x)
    none = no_corr(x)
    if reference is None:
        with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
            warnings.simplefilter("ignore")
            reference = np.atleast_2d(np.corrcoef(x.T))
    assert np.array_equal(np.isnan(corr), none[:, None] | none[None, :]), what
    assert np.array_equal(_bits(corr), _bits(corr.T)), what
    assert np.all(np.diag(corr)[~none] == 1.0), what
    ok = ~np.isnan(corr)
    ratio = float(np.max(np.abs(corr - reference)[ok] / bound[ok])) if ok.any() else 0.0
    print(f"{what}: largest correlation difference / bound = {ratio:.3g}")
    assert ratio <= 1.0, (what, ratio)
    return ratio


def check_case(case, t, summary, what):
    for g in range(len(case.probs_list)):
        check_group(case, t, g, summary, what)


INT_TABLES = ("hist", "outside", "panels")


def group_bytes(t, g):
    """Every block of group g, as bytes."""
    return b"".join(np.ascontiguousarray(t[w][g]).tobytes()
                    for w in ("edges",) + INT_TABLES + ("corr",))
