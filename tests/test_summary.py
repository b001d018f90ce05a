"""The posterior summary (include/fitoct.h "posterior summary") without a GPU: defaults and the
error contract of the six entries, the host route ``fitoct_summary_host`` against the
parent's route ``StanFit(materialise(raw)).summary()`` on the synthetic cases of
summary_cases.py, the branch-margin precondition that makes that comparison meaningful, and
the register gate of the new kernels.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import summary_cases as SC
from fitoct_amd import _lib
from fitoct_amd import build as B
from fitoct_amd.api import summary_host, summary_rows
from fitoct_amd.stanfit import output_columns

NO_DEVICE = _lib.lib().fitoct_device_count() < 1


@pytest.fixture(scope="module")
def cases():
    return {k: f() for k, f in SC.CASES.items()}


@pytest.fixture(scope="module")
def host_tables(cases):
    return {k: summary_host(c.raw, c.probs_list, c.first_iter, c.probs) for k, c in cases.items()}


# ---- defaults and error contract ----------------------------------------------------------------
def test_defaults_and_width():
    L = _lib.lib()
    c = _lib.SummaryConfig()
    L.fitoct_default_summary_config(C.byref(c))
    assert (c.first_iter, c.n_probs, c.max_staging_bytes, c.device) == (0, 5, 0, 0)
    assert list(c.probs)[:5] == [0.025, 0.25, 0.5, 0.75, 0.975]
    assert [L.fitoct_summary_width(k) for k in (0, 5, 16)] == [5, 10, 21]
    assert L.fitoct_summary_width(17) == -1 and L.fitoct_last_error()
    assert L.fitoct_summary_width(-1) == -1


def _call(entry, problems, chains=2, iters=10, draws=True, cfg=True, out=True, **cfg_kw):
    """One call of fitoct_summary_device / _host with host buffers -> (status, message)."""
    L = _lib.lib()
    arr = None
    if problems is not None:
        arr = (_lib.Problem * len(problems))()
        for i, p in enumerate(problems):
            arr[i] = p.to_c()
    c = _lib.SummaryConfig()
    L.fitoct_default_summary_config(C.byref(c))
    for k, v in cfg_kw.items():
        if k == "probs":
            c.n_probs = len(v)
            for i, p in enumerate(v):
                c.probs[i] = p
        else:
            setattr(c, k, v)
    G = len(problems) if problems else 1
    W = (problems[0].D if problems else 3) + 8
    raw = np.zeros((G, chains, max(iters, 1), W))
    res = np.zeros((G, 64, 21))
    cp = C.byref(c) if cfg else None
    if entry == "device":
        rc = L.fitoct_summary_device(arr, G, chains, iters, raw.ctypes.data if draws else None,
                                     cp, None, _lib.dptr(res) if out else None)
    else:
        rc = L.fitoct_summary_host(arr, G, chains, iters, _lib.dptr(raw) if draws else None, cp,
                                   _lib.dptr(res) if out else None)
    return rc, L.fitoct_last_error().decode()


BAD = {
    "too few post-warmup draws": dict(iters=10, first_iter=7),
    "three draws": dict(iters=3),
    "negative first_iter": dict(first_iter=-1),
    "n_probs below 0": dict(n_probs=-1),
    "n_probs above 16": dict(n_probs=17),
    "probability above 1": dict(probs=(0.5, 1.5)),
    "probability below 0": dict(probs=(-0.1,)),
    "probability NaN": dict(probs=(0.5, float("nan"))),
    "NULL draws": dict(draws=False),
    "NULL config": dict(cfg=False),
    "NULL out": dict(out=False),
    "no chains": dict(chains=0),
}


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors(entry, what):
    rc, msg = _call(entry, [SC._problem("normal", 5)], **BAD[what])
    assert rc == -1 and msg, (what, rc, msg)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_null_problems_and_mixed_groups(entry):
    rc, msg = _call(entry, None)
    assert rc == -1 and msg
    a = SC._problem("normal", 5)
    for other in (SC._problem("lasso", 5), SC._problem("normal", 6),
                  SC._problem("normal", 5, prior_PD=1)):
        rc, msg = _call(entry, [a, other])
        assert rc == -1 and "group" in msg, (rc, msg)
    rc, msg = _call(entry, [SC._problem("normal", 30)])
    assert rc == -1 and msg


def test_valid_call_needs_a_device():
    """Every check passes, then: no device -> FITOCT_E_NODEVICE; with one, the host pointer
    given as d_draws is refused (FITOCT_E_ARG) before any kernel runs."""
    rc, msg = _call("device", [SC._problem("normal", 5)])
    assert rc == (-3 if NO_DEVICE else -1) and msg
    rc, _ = _call("host", [SC._problem("normal", 5)])
    assert rc == 0


def test_plan_and_batch_summary_need_handles():
    L = _lib.lib()
    c = _lib.SummaryConfig()
    L.fitoct_default_summary_config(C.byref(c))
    out = np.zeros(64)
    assert L.fitoct_plan_summary(None, C.byref(c), _lib.dptr(out)) == -1 and L.fitoct_last_error()
    assert L.fitoct_batch_summary(None, C.byref(c), _lib.dptr(out)) == -1 and L.fitoct_last_error()


# ---- host route against the parent's route ------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.CASES))
def test_branch_margins(cases, name):
    """Precondition of the comparisons below and on the device: every Geyer branch of every
    column that has an n_eff is at least 1e-10 from flipping."""
    case = cases[name]
    deepest = 0
    for g in range(len(case.probs_list)):
        fit, rows = SC.stanfit_rows(case, g)
        for col, r in rows.items():
            if np.isnan(r["n_eff"]):
                continue
            ess, margin, max_t = SC.geyer_margins(SC.column(fit, col))
            assert margin >= 1e-10, (name, g, col, margin)
            assert ess == pytest.approx(r["n_eff"], rel=1e-8), (name, g, col)
            deepest = max(deepest, max_t)
    if name == "d":   # several blocks of 64 lags
        assert deepest > 300, deepest


@pytest.mark.parametrize("name", list(SC.CASES))
def test_host_summary_matches_stanfit(cases, host_tables, name):
    case, table = cases[name], host_tables[name]
    for g, prob in enumerate(case.probs_list):
        names = output_columns(prob)
        assert table.shape == (len(case.probs_list), len(names), 5 + len(case.probs))
        fit, rows = SC.stanfit_rows(case, g)
        for j, col in enumerate(names):
            flat = SC.column(fit, col).reshape(-1)
            if col not in rows:   # StanFit.summary omits an all-NaN column
                assert np.all(np.isnan(table[g, j])), (name, g, col)
                continue
            SC.check_row(table[g, j], SC.stanfit_row_values(rows[col], case.probs), flat,
                         case.probs, (name, g, col))


def test_case_properties(cases, host_tables):
    """What each case is there for shows in the table."""
    b, tb = cases["b"], host_tables["b"][0]
    names = output_columns(b.probs_list[0])
    lam = tb[names.index("lambda")]
    assert lam[0] == b.probs_list[0].lambda_scale and lam[2] == 0.0
    assert np.isnan(lam[1]) and np.isnan(lam[-1]) and np.isnan(lam[-2])
    assert tb[names.index("theta.1")][-1] > 1.1          # the shifted chain
    c, tc = cases["c"], host_tables["c"]
    names = output_columns(c.probs_list[0])
    (g_nan, col_nan), = c.nan_rows
    nan_rows = np.argwhere(np.all(np.isnan(tc), axis=2))
    assert nan_rows.tolist() == [[g_nan, names.index(col_nan)]]   # that row, that group only
    g = cases["g"]
    names = output_columns(g.probs_list[0])
    assert "br" not in names and host_tables["g"].shape[1] == len(names)
    assert not np.any(np.all(np.isnan(host_tables["g"][0]), axis=1))
    a = cases["a"]
    names = output_columns(a.probs_list[0])
    assert {"tau", "lambda.5", "yGP.5", "br"} <= set(names)
    h = cases["h"]
    names = output_columns(h.probs_list[0])
    q = host_tables["h"][0][names.index("treedepth__")][3:8]
    assert q[0] == 1.0 and q[-1] == 3.0 and set(q) <= {1.0, 2.0, 3.0}
    e = host_tables["h"][0][names.index("energy__")]
    flat = h.raw[0, :, :, 6].reshape(-1)
    assert e[3] == flat.min() and e[7] == flat.max()


def test_summary_rows_dict(cases, host_tables):
    """The dict form: StanFit.summary's keys, all-NaN rows omitted, pars by base name."""
    c = cases["c"]
    rows = summary_rows(host_tables["c"][2], c.probs_list[2], c.probs)
    assert c.nan_rows[0][1] not in rows and "theta.1" in rows
    assert list(rows["theta.1"]) == ["mean", "se_mean", "sd", "2.5%", "25%", "50%", "75%",
                                     "97.5%", "n_eff", "Rhat"]
    th = summary_rows(host_tables["c"][0], c.probs_list[0], c.probs, pars=["theta", "lp__"])
    assert list(th) == ["theta.1", "theta.2", "theta.3", "lp__"]
    with pytest.raises(KeyError):
        summary_rows(host_tables["c"][0], c.probs_list[0], c.probs, pars="nope")


# ---- register gate of the new object ------------------------------------------------------------
def test_summary_kernels_do_not_spill():
    """The -Rpass-analysis=kernel-resource-usage remarks fitoct_amd.build keeps beside the
    object of the shared layer, which holds the summary's kernels (the summary's own object
    has none): 0 spilled VGPRs and 0 scratch for every one of them (recompiled device-only for
    the remarks if the record is missing or stale)."""
    src = os.path.join(B.CSRC, "posterior_common.hip")
    path = os.path.join(B.OBJDIR, "posterior_common.resources.txt")
    if os.path.exists(path) and os.path.getmtime(path) >= B._newest_dep(src):
        text = open(path).read()
    else:
        out = os.path.join("/tmp", f"fitoct_resources_summary_{os.getpid()}.o")
        r = subprocess.run([B._hipcc(), *B._KERNEL, f"-I{B.INCLUDE}", f"-I{B.CSRC}",
                            "--cuda-device-only", "-c", src, "-o", out,
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        os.remove(out)
        text = r.stderr
    rows = B.kernel_resources(text)
    for kernel in ("stage_kernel", "moments_kernel", "acov_kernel", "qhist_kernel",
                   "qselect_kernel"):
        hit = [k for k in rows if kernel in k]
        assert len(hit) == 1, (kernel, list(rows))
        r = rows[hit[0]]
        assert r.get("VGPRs Spill", -1) == 0 and r.get("ScratchSize", -1) == 0, (kernel, r)
        assert r.get("LDS Size", 1 << 30) <= 64 * 1024, (kernel, r)
    assert len(rows) == 5, list(rows)   # the shared kernels, and nothing else, live here
    assert "posterior_common" in B.RECORDED and "summary_device" in B.RECORDED
