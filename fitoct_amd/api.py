"""Host-side mirror of FitOCTLib's ExpGP interface over the libfitoct C ABI.

``fitExpGP`` keeps the R signature used by the reference's callers
(FitOCT.R:110-124, priPost.R:2-16, ShinyInterface/server.R:408-426) -- same
argument names, meanings and defaults -- and returns the same list shape
``list(fit, method, xGP, prior_PD)`` (plotExpGP.R:29-32) as a dict whose ``fit``
is a :class:`fitoct_amd.stanfit.StanFit` (print / extract / as_matrix / summary
with Rhat and n_eff, as used at plotExpGP.R:7-50 and server.R:88-237).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import sys
import time
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import GRID, PREC, PRIOR, FitOCTError, check, dptr, lib


@dataclass
class ExpGPProblem:
    """Inputs of one ExpGP fit (fields of ``fitoct_problem``)."""

    x: np.ndarray
    y: np.ndarray
    uy: np.ndarray
    dataType: int = 2
    Nn: int = 10
    gridType: str = "internal"
    rho: float = 0.0                      # <= 0 -> 1/Nn
    theta0: np.ndarray = field(default_factory=lambda: np.array([1000.0, 2000.0, 300.0]))
    Sigma0: np.ndarray = None
    prior_type: str = "normal"
    lambda_rate: float = 0.1
    lambda_scale: float = 10.0
    nu: float = 1.0
    prior_PD: int = 0
    kernel_conv: int = 0
    lambda_conv: int = 0
    sigma_scale: float = 10.0
    nugget: float = 1e-9
    B: np.ndarray = None
    # monoexp only: 1 = theta_k ~ exponential(1/lambda_scale), Tests/testGamma.R's model
    # (the sampler's known answer, include/fitoct.h theta_prior)
    theta_prior: int = 0

    def __post_init__(self):
        self.x = np.ascontiguousarray(self.x, dtype=np.float64)
        self.y = np.ascontiguousarray(self.y, dtype=np.float64)
        self.uy = np.ascontiguousarray(self.uy, dtype=np.float64)
        if not (self.x.shape == self.y.shape == self.uy.shape) or self.x.ndim != 1:
            raise ValueError("x, y, uy must be 1-D arrays of equal length")
        self.theta0 = np.ascontiguousarray(self.theta0, dtype=np.float64).reshape(3)
        if self.Sigma0 is None:
            self.Sigma0 = np.diag((0.05 * self.theta0) ** 2)
        self.Sigma0 = np.ascontiguousarray(self.Sigma0, dtype=np.float64).reshape(3, 3)
        if self.B is not None:
            self.B = np.ascontiguousarray(self.B, dtype=np.float64).reshape(self.x.size, self.Nn)
        if self.gridType not in GRID:
            raise ValueError(f"gridType must be one of {list(GRID)}")
        if self.prior_type not in PRIOR:
            raise ValueError(f"prior_type must be one of {list(PRIOR)}")

    @property
    def N(self) -> int:
        return self.x.size

    @property
    def family(self) -> int:
        return PRIOR[self.prior_type]

    @property
    def D(self) -> int:
        return lib().fitoct_dim(self.family, self.Nn)

    def to_c(self) -> _lib.Problem:
        p = _lib.Problem()
        p.N = self.N
        p.x, p.y, p.uy = dptr(self.x), dptr(self.y), dptr(self.uy)
        p.data_type = int(self.dataType)
        p.Nn = int(self.Nn)
        p.grid_type = GRID[self.gridType]
        p.rho = float(self.rho if self.rho else 0.0)
        p.B = dptr(self.B) if self.B is not None else None
        p.theta0[:] = list(self.theta0)
        p.Sigma0[:] = list(self.Sigma0.ravel())
        p.prior_type = self.family
        p.lambda_rate = float(self.lambda_rate)
        p.lambda_scale = float(self.lambda_scale)
        p.nu = float(self.nu)
        p.prior_PD = int(self.prior_PD)
        p.kernel_conv = int(self.kernel_conv)
        p.lambda_conv = int(self.lambda_conv)
        p.sigma_scale = float(self.sigma_scale)
        p.nugget = float(self.nugget)
        p.theta_prior = int(self.theta_prior)
        return p

    def basis(self):
        """(B[N, Nn], xGP[Nn]) as built by the library (fp64 Cholesky, host)."""
        B = np.zeros((self.N, self.Nn))
        xg = np.zeros(self.Nn)
        p = self.to_c()
        check(lib().fitoct_build_basis(C.byref(p), dptr(B), dptr(xg)))
        return B, xg

    def column_names(self):
        return _lib.column_names(self.family, self.Nn)


@dataclass
class SamplerConfig:
    """``rstan::sampling`` controls (testGamma.R:42-47) + sharding."""

    chains: int = 4
    warmup: int = 500
    samples: int = 1000
    seed: int = 1234
    adapt_delta: float = 0.8
    max_treedepth: int = 10
    adapt_engaged: bool = True
    stepsize: float = 1.0
    gamma: float = 0.05
    kappa: float = 0.75
    t0: float = 10.0
    init_buffer: int = 75
    term_buffer: int = 50
    window: int = 25
    init_radius: float = 2.0
    save_warmup: bool = True
    precision: str = "f64"
    device: int = 0
    chain_offset: int = 0
    # device list (fitoct_config.devices): the chains are split into contiguous blocks
    # of global chain ids, one per device, each run by its own host thread in the
    # library; draws equal a one-device run bit for bit.  Empty: ``device`` alone.
    devices: tuple = ()

    def to_c(self) -> _lib.Config:
        c = _lib.Config()
        c.chains = int(self.chains)
        c.chain_offset = int(self.chain_offset)
        c.warmup = int(self.warmup)
        c.samples = int(self.samples)
        c.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        c.adapt_delta = float(self.adapt_delta)
        c.max_treedepth = int(self.max_treedepth)
        c.adapt_engaged = 1 if self.adapt_engaged else 0
        c.stepsize = float(self.stepsize)
        c.gamma, c.kappa, c.t0 = float(self.gamma), float(self.kappa), float(self.t0)
        c.init_buffer, c.term_buffer, c.window = (int(self.init_buffer), int(self.term_buffer),
                                                  int(self.window))
        c.init_radius = float(self.init_radius)
        c.save_warmup = 1 if self.save_warmup else 0
        c.precision = PREC[self.precision]
        c.device = int(self.device)
        devs = tuple(int(d) for d in self.devices)
        if len(devs) > _lib.MAX_DEVICES:
            raise ValueError(f"at most {_lib.MAX_DEVICES} devices per call")
        c.n_devices = len(devs)
        for i, d in enumerate(devs):
            c.devices[i] = d
        return c


def logp_grad(prob: ExpGPProblem, q: np.ndarray, precision: str = "f64", device: int = 0):
    """Batched log density / gradient on the GPU: q[P, D] -> (lp[P], grad[P, D], sumr2[P])."""
    q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float64)
    P, D = q.shape
    if D != prob.D:
        raise ValueError(f"q has {D} columns, model dimension is {prob.D}")
    lp = np.zeros(P)
    g = np.zeros((P, D))
    s2 = np.zeros(P)
    p = prob.to_c()
    check(lib().fitoct_logp_grad(C.byref(p), P, dptr(q), dptr(lp), dptr(g), dptr(s2),
                                 PREC[precision], device))
    return lp, g, s2


DEFAULT_PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)   # rstan::summary's probs


def _summary_config(first_iter, probs, max_staging_bytes=0, device=0) -> _lib.SummaryConfig:
    probs = tuple(float(p) for p in probs)
    if len(probs) > _lib.MAX_PROBS:
        raise ValueError(f"at most {_lib.MAX_PROBS} probabilities per summary")
    c = _lib.SummaryConfig()
    lib().fitoct_default_summary_config(C.byref(c))
    c.first_iter = int(first_iter)
    c.n_probs = len(probs)
    for i, p in enumerate(probs):
        c.probs[i] = p
    c.max_staging_bytes = int(max_staging_bytes)
    c.device = int(device)
    return c


def _problem_array(prob):
    probs = [prob] if isinstance(prob, ExpGPProblem) else list(prob)
    if not probs:
        raise ValueError("a summary needs at least one problem")
    arr = (_lib.Problem * len(probs))()
    for i, p in enumerate(probs):
        arr[i] = p.to_c()
    return probs, arr   # probs keeps the numpy buffers behind arr alive


def _post_warmup(cfg: SamplerConfig, first_iter):
    """The saved iterations a handle's table skips: the caller's, or the saved warmup."""
    if first_iter is None:
        return cfg.warmup if cfg.save_warmup else 0
    return first_iter


def _n_out(problem_c) -> int:
    """Rows of one group's summary or monitor table: 7 sampler columns, then the parameters."""
    return 7 + lib().fitoct_output_n_params(C.byref(problem_c))


def _host_draws(draws, ps) -> np.ndarray:
    """Host draws of the problems ``ps`` as ``[groups, chains, iters_saved, n_cols]``."""
    draws = np.ascontiguousarray(draws, dtype=np.float64)
    if draws.ndim == 3:
        draws = draws[None]
    if draws.ndim != 4 or draws.shape[0] != len(ps):
        raise ValueError("draws must be [groups, chains, iters_saved, n_cols], one problem per group")
    if draws.shape[3] != ps[0].D + 8:
        raise ValueError(f"draws have {draws.shape[3]} columns, the model has {ps[0].D + 8}")
    return draws


def _select_columns(prob: ExpGPProblem, pars):
    """(output column names, indices of the rows ``pars`` selects): names or base names
    (``"theta"`` -> ``theta.1`` ...) as in rstan, every row for None."""
    from .stanfit import _base, output_columns
    names = output_columns(prob)
    if pars is None:
        return names, list(range(len(names)))
    sel = []
    for p in ([pars] if isinstance(pars, str) else pars):
        hit = [i for i, c in enumerate(names) if c == p or _base(c) == p]
        if not hit:
            raise KeyError(f"no parameter {p!r} in the fit")
        sel += hit
    return names, sel


def summary_rows(table: np.ndarray, prob: ExpGPProblem, probs=DEFAULT_PROBS, pars=None) -> dict:
    """One group's summary table ``[P, 5 + len(probs)]`` (``fitoct_summary_*``) as the dict
    :meth:`fitoct_amd.stanfit.StanFit.summary` returns: ``{name: {"mean", "se_mean", "sd",
    "2.5%", ..., "n_eff", "Rhat"}}``, all-NaN rows omitted, ``pars`` selecting names or base
    names (``"theta"`` -> ``theta.1`` ...) as in rstan."""
    names, sel = _select_columns(prob, pars)
    keys = ["mean", "se_mean", "sd"] + [f"{100 * p:g}%" for p in probs] + ["n_eff", "Rhat"]
    return {names[i]: {k: float(v) for k, v in zip(keys, table[i])}
            for i in sel if not np.all(np.isnan(table[i]))}


def summary_device(d_draws: int, prob, chains: int, iters_saved: int, first_iter: int = 0,
                   probs=DEFAULT_PROBS, max_staging_bytes: int = 0, device: int = 0,
                   stream: int = 0) -> np.ndarray:
    """Posterior summary of draws that lie in device memory (``fitoct_summary_device``):
    ``d_draws`` is the device pointer (e.g. a gathered torch tensor's ``data_ptr()``) of raw
    sampler draws ``[groups][chains][iters_saved][n_cols]``, ``prob`` one problem or one per
    group.  Returns ``[groups, P, 5 + len(probs)]`` (rows: :func:`summary_rows`)."""
    ps, arr = _problem_array(prob)
    c = _summary_config(first_iter, probs, max_staging_bytes, device)
    out = np.empty((len(ps), _n_out(arr[0]), 5 + c.n_probs))
    check(lib().fitoct_summary_device(arr, len(ps), int(chains), int(iters_saved),
                                      C.c_void_p(d_draws or None), C.byref(c),
                                      C.c_void_p(stream or None), dptr(out)))
    return out


def summary_host(draws: np.ndarray, prob, first_iter: int = 0, probs=DEFAULT_PROBS) -> np.ndarray:
    """The same table computed on the host (``fitoct_summary_host``) from raw draws
    ``[chains, iters_saved, n_cols]`` or ``[groups, chains, iters_saved, n_cols]``."""
    ps, arr = _problem_array(prob)
    draws = _host_draws(draws, ps)
    c = _summary_config(first_iter, probs)
    out = np.empty((len(ps), _n_out(arr[0]), 5 + c.n_probs))
    check(lib().fitoct_summary_host(arr, len(ps), draws.shape[1], draws.shape[2], dptr(draws),
                                    C.byref(c), dptr(out)))
    return out


CURVE_NAMES = ("dL", "m", "resid")   # the order of a curves table's quantity blocks


def _curve_bits(what):
    names = [what] if isinstance(what, str) else list(what)
    bad = [w for w in names if w not in _lib.CURVE]
    if bad or not names:
        raise ValueError(f"what must name some of {CURVE_NAMES}, got {what!r}")
    bits = 0
    for w in names:
        bits |= _lib.CURVE[w]
    return bits


def curves_blocks(table: np.ndarray, probs_list, what, probs=DEFAULT_PROBS) -> list:
    """The packed table of ``fitoct_curves_*`` as one array ``[nq, N_g, 2 + len(probs)]`` per
    group (quantities in the order dL, m, resid, the wanted ones only)."""
    bits = what if isinstance(what, int) else _curve_bits(what)
    nq, w = bin(bits).count("1"), 2 + len(probs)
    out, o = [], 0
    for p in probs_list:
        out.append(table[o:o + nq * p.N * w].reshape(nq, p.N, w))
        o += nq * p.N * w
    return out


def curves_rows(block: np.ndarray, prob: ExpGPProblem, what, probs=DEFAULT_PROBS) -> dict:
    """One group's block ``[nq, N, 2 + len(probs)]`` as ``{"dL": {"mean": [N], "sd": [N],
    "2.5%": [N], ...}, "m": ..., "resid": ..., "x": x}``."""
    bits = what if isinstance(what, int) else _curve_bits(what)
    keys = ["mean", "sd"] + [f"{100 * p:g}%" for p in probs]
    names = [n for n in CURVE_NAMES if bits & _lib.CURVE[n]]
    rows = {n: {k: np.array(block[q, :, j]) for j, k in enumerate(keys)}
            for q, n in enumerate(names)}
    rows["x"] = prob.x.copy()
    return rows


def _curves_table(ps, what, c):
    bits = what if isinstance(what, int) else _curve_bits(what)
    nq = bin(bits).count("1") if 0 < bits < 8 else 3
    return bits, np.empty(sum(p.N for p in ps) * nq * (2 + c.n_probs))


def curves_device(d_draws: int, prob, chains: int, iters_saved: int, first_iter: int = 0,
                  probs=DEFAULT_PROBS, what=CURVE_NAMES, max_staging_bytes: int = 0,
                  device: int = 0, stream: int = 0) -> np.ndarray:
    """Posterior bands of the fitted curves of draws that lie in device memory
    (``fitoct_curves_device``; ``d_draws``, ``prob`` as :func:`summary_device`): per depth bin
    the mean, sd and quantiles of ``dL``, ``m`` and ``resid`` over the pooled post-warmup
    draws.  Returns the packed table (blocks: :func:`curves_blocks`)."""
    ps, arr = _problem_array(prob)
    c = _summary_config(first_iter, probs, max_staging_bytes, device)
    bits, out = _curves_table(ps, what, c)
    check(lib().fitoct_curves_device(arr, len(ps), int(chains), int(iters_saved),
                                     C.c_void_p(d_draws or None), bits, C.byref(c),
                                     C.c_void_p(stream or None), dptr(out)))
    return out


def curves_host(draws: np.ndarray, prob, first_iter: int = 0, probs=DEFAULT_PROBS,
                what=CURVE_NAMES) -> np.ndarray:
    """The same table computed on the host (``fitoct_curves_host``) from raw draws
    ``[chains, iters_saved, n_cols]`` or ``[groups, chains, iters_saved, n_cols]``."""
    ps, arr = _problem_array(prob)
    draws = _host_draws(draws, ps)
    c = _summary_config(first_iter, probs)
    bits, out = _curves_table(ps, what, c)
    check(lib().fitoct_curves_host(arr, len(ps), draws.shape[1], draws.shape[2], dptr(draws), bits,
                                   C.byref(c), dptr(out)))
    return out


def _pick_indices(draws, n, seed, S):
    """``generated_quantities``' selection: ``n`` of the S pooled draws at random, sorted, or
    the explicit flat indices ``draws``."""
    if draws is None:
        rng = np.random.default_rng(seed)
        draws = np.sort(rng.choice(S, size=min(n, S), replace=False))
    return np.ascontiguousarray(draws, dtype=np.int64).reshape(-1)


def _pick(prob, idx, call, call_params):
    """The dict of ``generated_quantities`` from the two pick entries of a plan or a batch."""
    k, N = idx.size, prob.N
    mono = prob.prior_type == "monoexp"
    dL, m, resid, br = np.empty((k, N)), np.empty((k, N)), np.empty((k, N)), np.empty(k)
    theta, ygp = np.empty((k, 3)), np.zeros((k, 0 if mono else prob.Nn))
    ip = idx.ctypes.data_as(_lib._lp)
    check(call(k, ip, dptr(dL), dptr(m), dptr(resid), dptr(br)))
    check(call_params(k, ip, dptr(theta), None if mono else dptr(ygp)))
    return {"dL": dL, "m": m, "resid": resid, "br": br, "index": idx, "theta": theta, "yGP": ygp}


MONITOR_KEYS = ("Rhat", "Rhat_bulk", "Rhat_fold", "Bulk_ESS", "Tail_ESS")


def monitor_rows(table: np.ndarray, prob: ExpGPProblem, pars=None) -> dict:
    """One group's rank-diagnostics table ``[P, 5]`` (``fitoct_monitor_*``) as ``{name: {"Rhat",
    "Rhat_bulk", "Rhat_fold", "Bulk_ESS", "Tail_ESS"}}`` (``Rhat`` the rank-normalised R-hat:
    the larger of bulk and folded), all-NaN rows omitted, ``pars`` as in :func:`summary_rows`."""
    names, sel = _select_columns(prob, pars)
    return {names[i]: {k: float(v) for k, v in zip(MONITOR_KEYS, table[i])}
            for i in sel if not np.all(np.isnan(table[i]))}


def monitor_device(d_draws: int, prob, chains: int, iters_saved: int, first_iter: int = 0,
                   max_staging_bytes: int = 0, device: int = 0, stream: int = 0) -> np.ndarray:
    """``rstan::monitor``'s rank diagnostics of draws that lie in device memory
    (``fitoct_monitor_device``; arguments as :func:`summary_device`): rank-normalised split
    R-hat (max, bulk, folded), bulk ESS and tail ESS per output column.  Returns
    ``[groups, P, 5]`` (rows: :func:`monitor_rows`)."""
    ps, arr = _problem_array(prob)
    c = _summary_config(first_iter, (), max_staging_bytes, device)
    out = np.empty((len(ps), _n_out(arr[0]), 5))
    check(lib().fitoct_monitor_device(arr, len(ps), int(chains), int(iters_saved),
                                      C.c_void_p(d_draws or None), C.byref(c),
                                      C.c_void_p(stream or None), dptr(out)))
    return out


def monitor_host(draws: np.ndarray, prob, first_iter: int = 0) -> np.ndarray:
    """The same table computed on the host (``fitoct_monitor_host``) from raw draws
    ``[chains, iters_saved, n_cols]`` or ``[groups, chains, iters_saved, n_cols]``."""
    ps, arr = _problem_array(prob)
    draws = _host_draws(draws, ps)
    c = _summary_config(first_iter, ())
    out = np.empty((len(ps), _n_out(arr[0]), 5))
    check(lib().fitoct_monitor_host(arr, len(ps), draws.shape[1], draws.shape[2], dptr(draws),
                                    C.byref(c), dptr(out)))
    return out


PAIRS_PARS = ("theta", "yGP", "lambda", "sigma", "br", "lp__")   # plotExpGP.R:41's pars
PAIRS_WHAT = ("edges", "hist", "outside", "panels", "corr")


def _pairs_config(prob: ExpGPProblem, first_iter, pars, n_bins, planes, range_probs, log,
                  max_staging_bytes=0, device=0):
    """(``fitoct_pairs_config``, names of the selected columns): ``pars`` and ``log`` select
    names or base names as :func:`_select_columns` does; the default ``pars`` are
    plotExpGP.R:41's, those the family has."""
    from .stanfit import _base
    names, _ = _select_columns(prob, None)
    if pars is None:
        pars = [p for p in PAIRS_PARS if any(c == p or _base(c) == p for c in names)]
    _, sel = _select_columns(prob, pars)
    if not 1 <= len(sel) <= _lib.MAX_PAIRS_COLS:
        raise ValueError(f"pairs takes 1..{_lib.MAX_PAIRS_COLS} columns, pars selects {len(sel)}")
    _, logsel = _select_columns(prob, log) if len(log) else (names, [])   # (those among pars)
    c = _lib.PairsConfig()
    lib().fitoct_default_pairs_config(C.byref(c))
    c.first_iter, c.n_cols = int(first_iter), len(sel)
    for j, i in enumerate(sel):
        c.cols[j] = i
        if i in logsel:
            c.log_mask |= 1 << j
    c.n_bins, c.planes = int(n_bins), int(planes)
    c.range_probs[0], c.range_probs[1] = float(range_probs[0]), float(range_probs[1])
    c.max_staging_bytes, c.device = int(max_staging_bytes), int(device)
    return c, [names[i] for i in sel]


def _pairs_ranges(ranges, columns, groups):
    """``ranges`` as ``[groups, n_cols, 2]`` (NaN: automatic) or None: an array of that shape
    (``[n_cols, 2]`` for every group), or ``{column name: (lo, hi)}``."""
    if ranges is None:
        return None
    if isinstance(ranges, dict):
        unknown = set(ranges) - set(columns)
        if unknown:
            raise KeyError(f"ranges names columns that pars does not select: {sorted(unknown)}")
        ranges = [ranges.get(n, (np.nan, np.nan)) for n in columns]
    r = np.asarray(ranges, dtype=np.float64)
    r = np.ascontiguousarray(np.broadcast_to(r, (groups, len(columns), 2)))
    return r


def _pairs_call(c, columns, groups, S, ranges, what, call) -> dict:
    """Allocate what ``what`` names of a pairs table, run ``call(ranges, config, out)`` (one of
    the ``fitoct_*pairs*`` entries) and return the arrays over the groups."""
    bad = [w for w in what if w not in PAIRS_WHAT]
    if bad or not len(what):
        raise ValueError(f"what must name some of {PAIRS_WHAT}, got {what!r}")
    nc, nb, pl = c.n_cols, c.n_bins, c.planes
    shapes = {"edges": (groups, nc, nb + 1), "hist": (groups, nc, pl, nb), "outside": (groups, nc, 2),
              "panels": (groups, nc * (nc - 1) // 2, pl, nb, nb), "corr": (groups, nc, nc)}
    t = {w: np.empty(shapes[w], dtype=np.float64 if w in ("edges", "corr") else np.int64)
         for w in PAIRS_WHAT if w in what}
    o = _lib.PairsOut()
    o.edges, o.corr = dptr(t.get("edges")), dptr(t.get("corr"))
    for field_, w in (("hist1", "hist"), ("outside", "outside"), ("hist2", "panels")):
        if w in t:
            setattr(o, field_, t[w].ctypes.data_as(_lib._lp))
    r = _pairs_ranges(ranges, columns, groups)
    check(call(dptr(r), C.byref(c), C.byref(o)))
    t["columns"], t["S"] = list(columns), int(S)
    return t


def pairs_rows(tables: dict, g: int = 0) -> dict:
    """Group ``g`` of a pairs table (:func:`pairs_device`, :func:`pairs_host`) as the dict
    :meth:`Plan.pairs` returns: ``{"columns": [...], "edges": [n_cols, nb + 1], "hist": [n_cols,
    planes, nb], "outside": [n_cols, 2], "panels": {(name_a, name_b): [planes, nb, nb]}, "corr":
    [n_cols, n_cols], "S": S}`` (the parts that were asked for)."""
    cols = tables["columns"]
    rows = {"columns": list(cols)}
    for w in ("edges", "hist", "outside", "corr"):
        if w in tables:
            rows[w] = tables[w][g]
    if "panels" in tables:
        names = [(a, b) for i, a in enumerate(cols) for b in cols[i + 1:]]
        rows["panels"] = {ab: tables["panels"][g][i] for i, ab in enumerate(names)}
    rows["S"] = tables["S"]
    return rows


def pairs_device(d_draws: int, prob, chains: int, iters_saved: int, first_iter: int = 0,
                 pars=None, n_bins: int = 32, planes: int = 1, range_probs=(0, 1), ranges=None,
                 log=(), what=PAIRS_WHAT, max_staging_bytes: int = 0, device: int = 0,
                 stream: int = 0) -> dict:
    """The pairs plot of draws that lie in device memory (``fitoct_pairs_device``; ``d_draws``,
    ``prob`` as :func:`summary_device`): per selected column the bin edges, the marginal
    histogram and the counts outside the range, per couple of columns the joint histogram, and
    the correlation matrix, over the pooled post-warmup draws; ``planes=2`` adds a second count
    plane of the divergent draws.  ``ranges``: explicit ``(lo, hi)`` per column (see
    :func:`_pairs_ranges`), else the quantiles at ``range_probs``; ``log`` names the columns
    with geometric edges.  Returns the arrays over the groups (one group: :func:`pairs_rows`)."""
    ps, arr = _problem_array(prob)
    c, columns = _pairs_config(ps[0], first_iter, pars, n_bins, planes, range_probs, log,
                               max_staging_bytes, device)
    return _pairs_call(c, columns, len(ps), int(chains) * (int(iters_saved) - int(first_iter)),
                       ranges, what,
                       lambda r, cp, op: lib().fitoct_pairs_device(
                           arr, len(ps), int(chains), int(iters_saved), C.c_void_p(d_draws or None),
                           r, cp, C.c_void_p(stream or None), op))


def pairs_host(draws: np.ndarray, prob, first_iter: int = 0, pars=None, n_bins: int = 32,
               planes: int = 1, range_probs=(0, 1), ranges=None, log=(), what=PAIRS_WHAT) -> dict:
    """The same table computed on the host (``fitoct_pairs_host``) from raw draws
    ``[chains, iters_saved, n_cols]`` or ``[groups, chains, iters_saved, n_cols]``."""
    ps, arr = _problem_array(prob)
    draws = _host_draws(draws, ps)
    c, columns = _pairs_config(ps[0], first_iter, pars, n_bins, planes, range_probs, log)
    return _pairs_call(c, columns, len(ps), draws.shape[1] * (draws.shape[2] - int(first_iter)),
                       ranges, what,
                       lambda r, cp, op: lib().fitoct_pairs_host(
                           arr, len(ps), draws.shape[1], draws.shape[2], dptr(draws), r, cp, op))


def pripost_marginals(prior, posterior, pars=None, n_bins: int = 32,
                      range_probs=(0.005, 0.995)) -> dict:
    """What ``FitOCTLib::plotPriPostAll(prior fit, posterior fit)`` draws (priPost.R:22): per
    column both runs have (``br`` is absent from a prior run), common bin edges and the two
    marginal count vectors.  ``prior`` and ``posterior`` are handles with a completed run
    (:class:`Plan`, or :class:`fitoct_amd.stanfit.StanFit`): each is asked for its automatic
    ranges at ``range_probs``, then both are binned over the union.  Returns ``{name: {"edges":
    [nb + 1], "prior": [nb], "posterior": [nb], "prior_outside": (below, above),
    "posterior_outside": ...}}``."""
    auto = [h.pairs(pars=pars, n_bins=n_bins, range_probs=range_probs, what=("edges",))
            for h in (prior, posterior)]
    common = [n for n in auto[0]["columns"] if n in auto[1]["columns"]]
    ranges = {}
    for n in common:
        e = [a["edges"][a["columns"].index(n)] for a in auto]
        ranges[n] = (np.fmin(e[0][0], e[1][0]), np.fmax(e[0][-1], e[1][-1]))   # NaN: no grid there
    both = [h.pairs(pars=common, n_bins=n_bins, ranges=ranges, what=("edges", "hist", "outside"))
            for h in (prior, posterior)]
    if both[0]["edges"].tobytes() != both[1]["edges"].tobytes():   # one builder, the same ranges
        raise RuntimeError("pripost_marginals: the two runs' edges differ")
    out = {}
    for j, n in enumerate(common):
        out[n] = {"edges": both[1]["edges"][j]}
        for side, t in zip(("prior", "posterior"), both):
            out[n][side] = t["hist"][j, 0]
            out[n][side + "_outside"] = tuple(int(v) for v in t["outside"][j])
    return out


@dataclass
class SampleOutput:
    draws: np.ndarray          # [chains, iters_saved, n_cols]
    columns: list
    warmup_saved: int          # leading warmup iterations included in draws
    stepsize: np.ndarray
    inv_metric: np.ndarray
    last_q: np.ndarray
    total_leapfrogs: int
    kernel_ms: float
    wall_ms: float
    chain_offset: int = 0
    migrations: int = 0        # chains handed between tiles (work balance)
    cfg: object = None         # the SamplerConfig of the run (Stan-CSV header)
    two_ended_transitions: int = 0   # transitions grown at both ends at once (no effect on draws)
    paired_transitions: int = 0      # ... whose forward end grew in a partner tile (no effect)


class _LastRun:
    """The posterior tables of a handle's last run, computed on the device from the draws where
    they lie: the bodies :class:`Plan` and :class:`Batch` share.  The handle gives ``_h``,
    ``cfg``, ``info``, its problems ``_probs`` with the first as a C struct ``_p0``, and the
    prefix of its entry points ``_entries`` ("fitoct_plan_" / "fitoct_batch_").  Every body
    returns one dict per problem, or with ``problem`` that problem's dict."""

    def _entry(self, name):
        return getattr(lib(), self._entries + name)

    def _each(self, problem, rows):
        if problem is not None:
            return rows(problem)
        return [rows(p) for p in range(len(self._probs))]

    def _summary(self, problem, pars, probs, first_iter, max_staging_bytes):
        c = _summary_config(_post_warmup(self.cfg, first_iter), probs, max_staging_bytes)
        out = np.empty((len(self._probs), _n_out(self._p0), 5 + c.n_probs))
        check(self._entry("summary")(self._h, C.byref(c), dptr(out)))
        return self._each(problem, lambda p: summary_rows(out[p], self._probs[p], probs, pars))

    def _monitor(self, problem, pars, first_iter, max_staging_bytes):
        c = _summary_config(_post_warmup(self.cfg, first_iter), (), max_staging_bytes)
        out = np.empty((len(self._probs), _n_out(self._p0), 5))
        check(self._entry("monitor")(self._h, C.byref(c), dptr(out)))
        return self._each(problem, lambda p: monitor_rows(out[p], self._probs[p], pars))

    def _curves(self, problem, what, probs, first_iter, max_staging_bytes):
        c = _summary_config(_post_warmup(self.cfg, first_iter), probs, max_staging_bytes)
        bits, out = _curves_table(self._probs, what, c)
        check(self._entry("curves")(self._h, bits, C.byref(c), dptr(out)))
        blocks = curves_blocks(out, self._probs, bits, probs)
        return self._each(problem, lambda p: curves_rows(blocks[p], self._probs[p], bits, probs))

    def _pairs(self, problem, chains, pars, n_bins, planes, range_probs, ranges, log, what,
               first_iter, max_staging_bytes):
        first_iter = _post_warmup(self.cfg, first_iter)
        c, columns = _pairs_config(self._probs[0], first_iter, pars, n_bins, planes, range_probs,
                                   log, max_staging_bytes)
        t = _pairs_call(c, columns, len(self._probs),
                        chains * (self.info["iters_saved"] - first_iter), ranges, what,
                        lambda r, cp, op: self._entry("pairs")(self._h, r, cp, op))
        return self._each(problem, lambda p: pairs_rows(t, p))

    def _curves_pick(self, problem, chains, draws, n, seed, first_iter, *lead):
        """``lead``: what the pick entries take between the handle and the config."""
        first_iter = _post_warmup(self.cfg, first_iter)
        idx = _pick_indices(draws, n, seed, chains * (self.info["iters_saved"] - first_iter))
        c = _summary_config(first_iter, ())
        pick, params = self._entry("curves_pick"), self._entry("curves_pick_params")
        return _pick(self._probs[problem], idx,
                     lambda k, ip, *o: pick(self._h, *lead, C.byref(c), k, ip, *o),
                     lambda k, ip, *o: params(self._h, *lead, C.byref(c), k, ip, *o))


class Plan(_LastRun):
    """A planned sampler run: inputs staged in HBM once, run many times."""

    _entries = "fitoct_plan_"

    def __init__(self, prob: ExpGPProblem, cfg: SamplerConfig):
        self.prob, self.cfg = prob, cfg
        self._p = prob.to_c()
        self._probs, self._p0 = [prob], self._p
        self._c = cfg.to_c()
        h = C.c_void_p()
        check(lib().fitoct_plan_create(C.byref(self._p), C.byref(self._c), C.byref(h)))
        self._h = h
        info = _lib.PlanInfo()
        check(lib().fitoct_plan_get_info(self._h, C.byref(info)))
        self.info = {f: getattr(info, f) for f, _ in _lib.PlanInfo._fields_}

    def run(self, d_draws: int = 0, stream: int = 0, progress=None, poll_s: float = 0.2):
        """Run on ``stream`` (hipStream_t as int); draws to the device buffer
        ``d_draws`` (int pointer, >= info['draws_bytes']) or a plan-internal one.

        ``progress(done, total)``, if given, is called from this thread every
        ``poll_s`` seconds while the kernel runs (done / total = transitions over all
        chains; this replaces rstan's stan.log progress, server.R:457-484).  A
        KeyboardInterrupt during the run cancels the chains at their next transition
        boundary, waits for the kernel to drain and re-raises: the R shim does the
        same around R_CheckUserInterrupt."""
        if progress is None:
            check(lib().fitoct_plan_run(self._h, C.c_void_p(d_draws or None),
                                        C.c_void_p(stream or None)))
            return
        self.launch(d_draws, stream)
        try:
            while True:
                done, total, finished = self.poll()
                progress(done, total)
                if finished:
                    break
                time.sleep(poll_s)
        except KeyboardInterrupt:
            self.cancel()
            self.wait()
            raise
        self.wait()

    def set_init(self, q_init=None, stepsize=None, inv_metric=None):
        """Warm restart (``fitoct_plan_set_init``): per-chain start position q_init
        [chains, D] (unconstrained), initial step size [chains] and diagonal inverse
        metric [chains, D] for the next runs; None keeps the default (jittered start
        around theta0, ``cfg.stepsize``, unit metric).  A previous run's ``last_q``,
        ``stepsize`` and ``inv_metric`` resume it (``adapt_engaged=False`` keeps them)."""
        C_, D = self.info["chains"], self.info["dim"]
        self._init = []   # kept alive only for the call (the library copies them)

        def arr(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))
            self._init.append(a)
            return dptr(a)
        check(lib().fitoct_plan_set_init(self._h, arr(q_init, (C_, D)), arr(stepsize, (C_,)),
                                         arr(inv_metric, (C_, D))))
        self._init = []

    def launch(self, d_draws: int = 0, stream: int = 0):
        """Enqueue the run and return at once (see :meth:`poll`, :meth:`wait`)."""
        check(lib().fitoct_plan_launch(self._h, C.c_void_p(d_draws or None),
                                       C.c_void_p(stream or None)))

    def poll(self):
        """(transitions done over all chains, chains * (warmup + samples), finished)."""
        d, t, f = C.c_int64(), C.c_int64(), C.c_int32()
        check(lib().fitoct_plan_poll(self._h, C.byref(d), C.byref(t), C.byref(f)))
        return int(d.value), int(t.value), bool(f.value)

    def cancel(self):
        """Ask every chain to stop at its next (8th) transition boundary; the run then
        reports FITOCT_E_CANCELLED from :meth:`download`."""
        check(lib().fitoct_plan_cancel(self._h))

    def wait(self):
        """Block until the launched run has drained."""
        check(lib().fitoct_plan_wait(self._h))

    def download(self, with_draws: bool = True) -> SampleOutput:
        """Copy results to the host.  ``with_draws=False`` leaves the draws in HBM
        (``SampleOutput.draws`` is None), e.g. when they are gathered over RCCL."""
        i = self.info
        C_, D = i["chains"], i["dim"]
        draws = np.empty((C_, i["iters_saved"], i["n_cols"])) if with_draws else None
        eps = np.empty(C_)
        minv = np.empty((C_, D))
        lq = np.empty((C_, D))
        st = np.zeros(C_, dtype=np.int32)
        r = _lib.Result()
        r.draws = dptr(draws)
        r.draws_capacity = draws.size if with_draws else 0
        r.stepsize, r.inv_metric, r.last_q = dptr(eps), dptr(minv), dptr(lq)
        r.chain_status = st.ctypes.data_as(C.POINTER(C.c_int32))
        check(lib().fitoct_plan_download(self._h, C.byref(r)))
        return SampleOutput(draws, self.prob.column_names(),
                            self.cfg.warmup if self.cfg.save_warmup else 0, eps, minv, lq,
                            int(r.total_leapfrogs), float(r.kernel_ms), 0.0,
                            self.cfg.chain_offset, int(r.migrations), self.cfg,
                            int(r.two_ended_transitions), int(r.paired_transitions))

    def summary(self, pars=None, probs=DEFAULT_PROBS, first_iter=None,
                max_staging_bytes: int = 0) -> dict:
        """``rstan::summary(fit, pars)$summary`` of the last run, computed on the device from
        the draws where they lie (the plan's buffer or the ``d_draws`` of the run; nothing is
        downloaded but the table): the dict of :meth:`fitoct_amd.stanfit.StanFit.summary`.
        ``first_iter`` (saved iterations to skip) defaults to the saved warmup."""
        return self._summary(0, pars, probs, first_iter, max_staging_bytes)

    def monitor(self, pars=None, first_iter=None, max_staging_bytes: int = 0) -> dict:
        """``rstan::monitor``'s rank diagnostics of the last run, computed on the device from
        the draws where they lie (as :meth:`summary`): the dict of :func:`monitor_rows`."""
        return self._monitor(0, pars, first_iter, max_staging_bytes)

    def curves(self, what=CURVE_NAMES, probs=DEFAULT_PROBS, first_iter=None,
               max_staging_bytes: int = 0) -> dict:
        """Posterior bands of the fitted curves of the last run (plotExpGP's plot), computed on
        the device from the draws where they lie: ``{"dL": {"mean": [N], "sd": [N], "2.5%":
        [N], ...}, "m": ..., "resid": ..., "x": x}`` for the quantities named in ``what``.
        ``first_iter`` defaults to the saved warmup."""
        return self._curves(0, what, probs, first_iter, max_staging_bytes)

    def pairs(self, pars=None, n_bins: int = 32, planes: int = 1, range_probs=(0, 1),
              ranges=None, log=(), what=PAIRS_WHAT, first_iter=None,
              max_staging_bytes: int = 0) -> dict:
        """The pairs plot of the last run (``pairs(fit, pars)``, ``SAPlot``), computed on the
        device from the draws where they lie: the dict of :func:`pairs_rows` -- bin edges,
        marginal and joint histograms (``planes=2``: a second plane of the divergent draws) and
        the correlation matrix of the columns ``pars`` selects (default: plotExpGP.R:41's).
        Arguments as :func:`pairs_device`; ``first_iter`` defaults to the saved warmup."""
        return self._pairs(0, self.info["chains"], pars, n_bins, planes, range_probs, ranges, log,
                           what, first_iter, max_staging_bytes)

    def curves_pick(self, draws=None, n=100, seed=None, first_iter=None) -> dict:
        """:func:`fitoct_amd.genquant.generated_quantities` without the download: dict(index,
        theta, yGP, dL, m, resid, br) of ``n`` post-warmup draws chosen at random (``seed``) or
        of the flat indices ``draws`` (chain * n_post + iteration), evaluated on the device."""
        return self._curves_pick(0, self.info["chains"], draws, n, seed, first_iter)

    def close(self):
        if getattr(self, "_h", None):
            lib().fitoct_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Batch(_LastRun):
    """Many problems (FitOCT.R's per-file fits, FitOCT.R:70-124) sampled by one
    launch (``fitoct_batch_*``).  Problem ``p``'s chains are global chains
    ``cfg.chain_offset + p*cfg.chains + c``, so its draws equal a :class:`Plan`
    of that problem with ``chain_offset = cfg.chain_offset + p*cfg.chains``."""

    _entries = "fitoct_batch_"

    def __init__(self, probs, cfg: SamplerConfig):
        self.probs, self.cfg = list(probs), cfg
        if not self.probs:
            raise ValueError("a batch needs at least one problem")
        arr = (_lib.Problem * len(self.probs))()
        for i, p in enumerate(self.probs):
            arr[i] = p.to_c()
        self._arr = arr    # the problems' numpy buffers stay referenced by self.probs
        self._probs, self._p0 = self.probs, arr[0]
        self._c = cfg.to_c()
        h = C.c_void_p()
        check(lib().fitoct_batch_create(arr, len(self.probs), C.byref(self._c), C.byref(h)))
        self._h = h
        info = _lib.PlanInfo()
        check(lib().fitoct_batch_get_info(self._h, C.byref(info)))
        self.info = {f: getattr(info, f) for f, _ in _lib.PlanInfo._fields_}

    def __len__(self):
        return len(self.probs)

    def run(self, d_draws: int = 0, stream: int = 0):
        """One launch for every problem; draws to ``d_draws`` (device pointer,
        >= info['draws_bytes'], layout [problem][chain][iter][col]) or internal."""
        check(lib().fitoct_batch_run(self._h, C.c_void_p(d_draws or None),
                                     C.c_void_p(stream or None)))

    def download(self, problem: int, with_draws: bool = True) -> SampleOutput:
        i, C_ = self.info, self.cfg.chains
        D = i["dim"]
        draws = np.empty((C_, i["iters_saved"], i["n_cols"])) if with_draws else None
        eps, minv, lq = np.empty(C_), np.empty((C_, D)), np.empty((C_, D))
        st = np.zeros(C_, dtype=np.int32)
        r = _lib.Result()
        r.draws = dptr(draws)
        r.draws_capacity = draws.size if with_draws else 0
        r.stepsize, r.inv_metric, r.last_q = dptr(eps), dptr(minv), dptr(lq)
        r.chain_status = st.ctypes.data_as(C.POINTER(C.c_int32))
        check(lib().fitoct_batch_download(self._h, int(problem), C.byref(r)))
        return SampleOutput(draws, self.probs[problem].column_names(),
                            self.cfg.warmup if self.cfg.save_warmup else 0, eps, minv, lq,
                            int(r.total_leapfrogs), float(r.kernel_ms), 0.0,
                            self.cfg.chain_offset + problem * C_, 0,
                            dataclasses.replace(self.cfg,
                                                chain_offset=self.cfg.chain_offset + problem * C_),
                            int(r.two_ended_transitions), int(r.paired_transitions))

    def summary(self, problem=None, pars=None, probs=DEFAULT_PROBS, first_iter=None,
                max_staging_bytes: int = 0):
        """Device summary of the last run (:meth:`Plan.summary`) of every file in one call: a
        list with one dict per problem, or problem ``problem``'s dict."""
        return self._summary(problem, pars, probs, first_iter, max_staging_bytes)

    def monitor(self, problem=None, pars=None, first_iter=None, max_staging_bytes: int = 0):
        """Device rank diagnostics of the last run (:meth:`Plan.monitor`) of every file in one
        call: a list with one dict per problem, or problem ``problem``'s dict."""
        return self._monitor(problem, pars, first_iter, max_staging_bytes)

    def curves(self, problem=None, what=CURVE_NAMES, probs=DEFAULT_PROBS, first_iter=None,
               max_staging_bytes: int = 0):
        """Posterior bands of the last run (:meth:`Plan.curves`) of every file in one call: a
        list with one dict per problem, or problem ``problem``'s dict."""
        return self._curves(problem, what, probs, first_iter, max_staging_bytes)

    def pairs(self, problem=None, pars=None, n_bins: int = 32, planes: int = 1,
              range_probs=(0, 1), ranges=None, log=(), what=PAIRS_WHAT, first_iter=None,
              max_staging_bytes: int = 0):
        """The pairs plot of the last run (:meth:`Plan.pairs`) of every file in one call: a
        list with one dict per problem, or problem ``problem``'s dict."""
        return self._pairs(problem, self.cfg.chains, pars, n_bins, planes, range_probs, ranges,
                           log, what, first_iter, max_staging_bytes)

    def curves_pick(self, problem: int, draws=None, n=100, seed=None, first_iter=None) -> dict:
        """:meth:`Plan.curves_pick` for problem ``problem`` of the last run."""
        g = int(problem)
        return self._curves_pick(g, self.cfg.chains, draws, n, seed, first_iter, g)

    def close(self):
        if getattr(self, "_h", None):
            lib().fitoct_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def sample_batch(probs, cfg: SamplerConfig):
    """One launch over every problem; returns one SampleOutput per problem."""
    t0 = time.perf_counter()
    with Batch(probs, cfg) as b:
        b.run()
        outs = [b.download(p) for p in range(len(b))]
    wall = (time.perf_counter() - t0) * 1e3
    for o in outs:
        o.wall_ms = wall
    return outs


def sample(prob: ExpGPProblem, cfg: SamplerConfig, progress=None,
           resume: SampleOutput | None = None) -> SampleOutput:
    """One-shot sampler run (plan + run + download); ``progress`` as in :meth:`Plan.run`.
    ``resume``: a previous run of the same chains whose last position, step size and
    inverse metric start this one (:meth:`Plan.set_init`)."""
    t0 = time.perf_counter()
    with Plan(prob, cfg) as pl:
        if resume is not None:
            pl.set_init(resume.last_q, resume.stepsize, resume.inv_metric)
        pl.run(progress=progress)
        out = pl.download()
    out.wall_ms = (time.perf_counter() - t0) * 1e3
    return out


def progress_printer(warmup, samples, stream=None):
    """rstan-format progress lines ("Chain k: Iteration: i / n [ p%]  (Warmup|Sampling)",
    ``fitoct_progress_line``: the overall fraction in the 4-serial-chains convention the
    Shiny server decodes, server.R:457-472) printed whenever the overall percentage
    changes -- the lines the R shim prints to R's stdout."""
    last = [-1]
    buf = C.create_string_buffer(160)

    def cb(done, total):
        if total <= 0:
            return
        pct = lib().fitoct_progress_line(int(done), int(total), int(warmup), int(samples), buf, 160)
        if pct < 0 or pct == last[0]:
            return
        last[0] = pct
        print(buf.value.decode(), file=stream or sys.stdout, flush=True)
    return cb


# --------------------------------------------------------------------------
# FitOCTLib-compatible entry point
# --------------------------------------------------------------------------
def fitExpGP(x, y, uy, dataType=2, Nn=10, gridType="internal", method="sample",
             theta0=None, Sigma0=None, lambda_rate=0.1, rho_scale=0.0, nb_warmup=500,
             nb_iter=1000, prior_PD=0, open_progress=False, *, nb_chains=4,
             prior_type="normal", lambda_scale=10.0, nu=1.0, adapt_delta=0.8,
             max_treedepth=10, seed=None, precision="f64", device=0, n_gpus=None,
             devices=None, refresh=1, **model_switches):
    """Drop-in for ``FitOCTLib::fitExpGP`` (FitOCT.R:110-124).

    ``nb_iter`` counts warmup + sampling iterations, as the callers pass
    ``nb_iter = nb_warmup + nb_sample`` (FitOCT.R:121).  ``rho_scale`` <= 0 means
    ``1/Nn`` (FitOCT.R:119).  Only ``method='sample'`` runs on the GPU; 'optim'
    and 'vb' run rstan::optimizing / rstan::vb natively over the same device
    density (:mod:`fitoct_amd.optim_vb`): ``fit`` is then an ``OptimFit``
    (``fit$par``, ``fit$hessian``) or a StanFit of ADVI draws.
    Progress lines are printed to stdout in rstan's format whatever
    ``open_progress`` is, as the R shim does (the Shiny server parses them from its
    stdout sink, server.R:391-393,457-484); ``refresh=0`` silences them.
    ``n_gpus`` (replaces ``options(mc.cores = detectCores())``,
    FitOCT.R:13): the chains are split over devices ``device .. device + n_gpus - 1``
    (the library runs one host thread per device; the draws do not depend on it);
    ``devices`` gives the ordinals explicitly instead (repeats allowed).
    Returns ``dict(fit, method, xGP, prior_PD, lasso)``.
    """
    from .stanfit import StanFit

    if method not in ("sample", "optim", "vb"):
        raise ValueError(f"method={method!r}: 'sample', 'optim' or 'vb' (FitOCT.R:42)")
    if theta0 is None:
        raise ValueError("theta0 is required (FitOCTLib::estimateExpPrior output)")
    nb_sample = int(nb_iter) - int(nb_warmup)
    if nb_sample < 1:
        raise ValueError("nb_iter must exceed nb_warmup")
    prob = ExpGPProblem(x, y, uy, dataType=dataType, Nn=Nn, gridType=gridType,
                        rho=rho_scale if rho_scale and rho_scale > 0 else 0.0, theta0=theta0,
                        Sigma0=Sigma0, prior_type=prior_type, lambda_rate=lambda_rate,
                        lambda_scale=lambda_scale, nu=nu, prior_PD=prior_PD, **model_switches)
    if seed is None:
        seed = int(np.random.SeedSequence().entropy & 0xFFFFFFFF)
    _, xGP = prob.basis()
    if method != "sample":
        from .genquant import expgp_curves
        from .optim_vb import optimizing, vb
        fit = (optimizing(prob, precision=precision, device=device) if method == "optim"
               else vb(prob, seed=seed, precision=precision, device=device))
        if method == "optim":   # fit$par$m / $resid / $dL (server.R:351,636)
            g = expgp_curves(prob, fit.par["theta"], fit.par["yGP"])
            for k in ("m", "resid", "dL"):
                fit.par[k] = g[k][0]
        return {"fit": fit, "method": method, "xGP": xGP, "prior_PD": prior_PD,
                "lasso": prior_type == "lasso"}
    if n_gpus is not None and not 1 <= int(n_gpus) <= 16:
        raise ValueError("fitExpGP: n_gpus must be in 1..16")   # as the R shim (fitoct_devices)
    if devices is None:
        devices = tuple(range(int(device), int(device) + int(n_gpus))) if n_gpus and n_gpus > 1 else ()
    cfg = SamplerConfig(chains=nb_chains, warmup=nb_warmup, samples=nb_sample, seed=seed,
                        adapt_delta=adapt_delta, max_treedepth=max_treedepth,
                        precision=precision, device=device, devices=devices)
    out = sample(prob, cfg, progress=progress_printer(nb_warmup, nb_sample) if refresh else None)
    fit = StanFit.from_output(out, prob)
    return {"fit": fit, "method": method, "xGP": xGP, "prior_PD": prior_PD,
            "lasso": prior_type == "lasso"}
