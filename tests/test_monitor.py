"""The rank diagnostics (include/fitoct.h "rank diagnostics") without a GPU: the host route
``fitoct_monitor_host`` against the numpy restatement of monitor_cases.py on every case, its
``Rhat`` against ``fitoct_rank_rhat`` bit for bit, the branch-margin precondition that makes the
ESS comparisons meaningful (here and on the device), the error contract of the four entries,
and the register gate of the new kernels.

One rule is wider than "every value equal": a column whose every chain is constant (the
sampler's ``stepsize__``) gives an all-NaN row, as it does in the summary.  Its within-chain
variance is zero, so its R-hats are rounding noise divided by zero (``fitoct_rank_rhat`` gives
about 1e15 on it, numpy 3e16): no route can agree with another on them.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import monitor_cases as MC
import summary_cases as SC
from fitoct_amd import _lib
from fitoct_amd import build as B
from fitoct_amd.api import monitor_host, monitor_rows
from fitoct_amd.stanfit import output_columns, rank_rhat

NO_DEVICE = _lib.lib().fitoct_device_count() < 1

ESS_LEFT_OUT = MC.ESS_LEFT_OUT   # named there: the columns whose ESS is not compared


@pytest.fixture(scope="module")
def cases():
    return {k: f() for k, f in MC.CASES.items()}


@pytest.fixture(scope="module")
def host_tables(cases):
    return {k: monitor_host(c.raw, c.probs_list, c.first_iter) for k, c in cases.items()}


@pytest.fixture(scope="module")
def refs(cases):
    return {k: MC.reference(c) for k, c in cases.items()}


# ---- precondition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MC.CASES))
def test_branch_margins(refs, name):
    """Every compared column's Geyer branches, on the z series and on both indicator series,
    are at least 1e-10 from flipping; the columns that miss it are exactly ESS_LEFT_OUT's, at
    most one in ten of the case."""
    low = [key for key, (_, zm, tm) in refs[name].items() if min(zm, tm) < MC.MIN_MARGIN]
    assert sorted(low) == sorted(ESS_LEFT_OUT.get(name, [])), (name, low)
    assert 10 * len(low) <= len(refs[name]), (name, len(low), len(refs[name]))
    if name in ("i", "j"):   # the new cases' z series hold it everywhere
        assert all(zm >= MC.MIN_MARGIN for _, zm, _ in refs[name].values())


# ---- host route against the restatement -----------------------------------------------------------
@pytest.mark.parametrize("name", list(MC.CASES))
def test_host_matches_restatement(cases, host_tables, refs, name):
    case, table = cases[name], host_tables[name]
    for g, prob in enumerate(case.probs_list):
        names = output_columns(prob)
        assert table.shape == (len(case.probs_list), len(names), 5)
        for j, col in enumerate(names):
            MC.check_row(table[g, j], refs[name][g, col][0], (name, g, col),
                         ess=(g, col) not in ESS_LEFT_OUT.get(name, []))


@pytest.mark.parametrize("name", list(MC.CASES))
def test_rhat_is_rank_rhat(cases, host_tables, name):
    """``Rhat`` equals fitoct_rank_rhat of the same column bit for bit; a NaN row is a column
    with a NaN or with every chain constant."""
    case, table = cases[name], host_tables[name]
    for g, prob in enumerate(case.probs_list):
        fit, _ = SC.stanfit_rows(case, g)
        for j, col in enumerate(output_columns(prob)):
            x = SC.column(fit, col)
            if np.isnan(table[g, j, 0]):
                ch = MC.split_chains(x).reshape(x.shape[0], -1)
                assert np.any(np.isnan(ch)) or np.all(ch == ch[:, :1]), (name, g, col)
                assert np.all(np.isnan(table[g, j]))
                continue
            assert np.float64(rank_rhat(x)).tobytes() == table[g, j, 0].tobytes(), (name, g, col)
            assert table[g, j, 0] == max(table[g, j, 1], table[g, j, 2])


def test_case_properties(cases, host_tables):
    """What each case is there for shows in the table."""
    b, tb = cases["b"], host_tables["b"][0]
    names = output_columns(b.probs_list[0])
    assert (b.raw.shape[2] - b.first_iter) % 2 == 1                     # a dropped middle draw
    assert tb[names.index("theta.1")][0] > 1.1                          # the shifted chain
    assert np.all(np.isnan(tb[names.index("lambda")]))                  # the lasso's constant
    c, tc = cases["c"], host_tables["c"]
    names = output_columns(c.probs_list[0])
    (g_nan, col_nan), = c.nan_rows
    nan_rows = np.argwhere(np.all(np.isnan(tc), axis=2)).tolist()
    want = sorted([[g, names.index("stepsize__")] for g in range(6)] +
                  [[g, names.index("divergent__")] for g in range(6)] +
                  [[g_nan, names.index(col_nan)]])
    assert nan_rows == want                                             # that row, that group only
    g = cases["g"]
    assert "br" not in output_columns(g.probs_list[0])
    h, th = cases["h"], host_tables["h"][0]
    names = output_columns(h.probs_list[0])
    tree = th[names.index("treedepth__")]
    assert not np.any(np.isnan(tree[:4])) and np.isnan(tree[4])         # x <= q95 = 3 is constant
    assert np.all(np.isnan(th[names.index("divergent__")]))
    assert not np.any(np.isnan(th[names.index("energy__")]))            # +-0 and subnormals
    S = MC.pooled_size(cases["i"])
    assert S > 2 * MC.SORT_LDS_KEYS and S % MC.SORT_LDS_KEYS and S % MC.SORT_TILE
    assert MC.pooled_size(cases["d"]) > MC.SORT_LDS_KEYS
    assert all(MC.pooled_size(cases[k]) <= MC.SORT_LDS_KEYS for k in "abcghj")
    assert cases["j"].raw.shape[:3] == (40, 4, 40)
    assert [MC.pooled_size(cases[k]) for k in ("e4", "e5")] == [4, 4]


def test_monitor_rows_dict(cases, host_tables):
    c = cases["c"]
    rows = monitor_rows(host_tables["c"][2], c.probs_list[2])
    assert c.nan_rows[0][1] not in rows and "stepsize__" not in rows and "theta.1" in rows
    assert list(rows["theta.1"]) == ["Rhat", "Rhat_bulk", "Rhat_fold", "Bulk_ESS", "Tail_ESS"]
    th = monitor_rows(host_tables["c"][0], c.probs_list[0], pars=["theta", "lp__"])
    assert list(th) == ["theta.1", "theta.2", "theta.3", "lp__"]
    with pytest.raises(KeyError):
        monitor_rows(host_tables["c"][0], c.probs_list[0], pars="nope")


# ---- error contract -------------------------------------------------------------------------------
def _call(entry, problems, chains=2, iters=10, draws=True, cfg=True, out=True, **cfg_kw):
    """One call of fitoct_monitor_device / _host with host buffers -> (status, message)."""
    L = _lib.lib()
    arr = None
    if problems is not None:
        arr = (_lib.Problem * len(problems))()
        for i, p in enumerate(problems):
            arr[i] = p.to_c()
    c = _lib.SummaryConfig()
    L.fitoct_default_summary_config(C.byref(c))
    for k, v in cfg_kw.items():
        setattr(c, k, v)
    G = len(problems) if problems else 1
    W = (problems[0].D if problems else 3) + 8
    raw = np.random.default_rng(1).standard_normal((G, chains, max(iters, 1), W))
    res = np.zeros((G, 64, 5))
    cp = C.byref(c) if cfg else None
    if entry == "device":
        rc = L.fitoct_monitor_device(arr, G, chains, iters, raw.ctypes.data if draws else None,
                                     cp, None, _lib.dptr(res) if out else None)
    else:
        rc = L.fitoct_monitor_host(arr, G, chains, iters, _lib.dptr(raw) if draws else None, cp,
                                   _lib.dptr(res) if out else None)
    return rc, L.fitoct_last_error().decode()


BAD = {
    "too few post-warmup draws": dict(iters=10, first_iter=7),
    "three draws": dict(iters=3),
    "negative first_iter": dict(first_iter=-1),
    "negative max_staging_bytes": dict(max_staging_bytes=-1),
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


def test_valid_call_needs_a_device_and_probs_are_ignored():
    """Every check passes, then: no device -> FITOCT_E_NODEVICE; with one, the host pointer
    given as d_draws is refused (FITOCT_E_ARG) before any kernel runs.  The probabilities of the
    shared config are not read."""
    rc, msg = _call("device", [SC._problem("normal", 5)])
    assert rc == (-3 if NO_DEVICE else -1) and msg
    assert _call("host", [SC._problem("normal", 5)])[0] == 0
    assert _call("host", [SC._problem("normal", 5)], n_probs=99)[0] == 0


def test_plan_and_batch_monitor_need_handles():
    L = _lib.lib()
    c = _lib.SummaryConfig()
    L.fitoct_default_summary_config(C.byref(c))
    out = np.zeros(64)
    assert L.fitoct_plan_monitor(None, C.byref(c), _lib.dptr(out)) == -1 and L.fitoct_last_error()
    assert L.fitoct_batch_monitor(None, C.byref(c), _lib.dptr(out)) == -1 and L.fitoct_last_error()


# ---- register gate of the new object --------------------------------------------------------------
KERNELS = ("keys_kernel", "sort_lds_kernel", "rhist_kernel", "rscan_kernel", "rscatter_kernel",
           "pick_kernel", "rank_kernel", "tail_kernel")
SHARED = ("stage_kernel", "moments_kernel", "acov_kernel")   # test_summary.py gates these


def test_monitor_kernels_do_not_spill():
    """The -Rpass-analysis=kernel-resource-usage remarks fitoct_amd.build keeps beside the
    monitor object: 0 spilled VGPRs and 0 scratch for every kernel of it (recompiled
    device-only for the remarks if the record is missing or stale), and the LDS sort within
    what one workgroup may declare."""
    src = os.path.join(B.CSRC, "monitor_device.hip")
    path = os.path.join(B.OBJDIR, "monitor_device.resources.txt")
    if os.path.exists(path) and os.path.getmtime(path) >= B._newest_dep(src):
        text = open(path).read()
    else:
        out = os.path.join("/tmp", f"fitoct_resources_monitor_{os.getpid()}.o")
        r = subprocess.run([B._hipcc(), *B._KERNEL, f"-I{B.INCLUDE}", f"-I{B.CSRC}",
                            "--cuda-device-only", "-c", src, "-o", out,
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        os.remove(out)
        text = r.stderr
    rows = B.kernel_resources(text)
    for kernel in KERNELS:
        hit = [k for k in rows if kernel in k]
        assert len(hit) == 1, (kernel, list(rows))
        r = rows[hit[0]]
        assert r.get("VGPRs Spill", -1) == 0 and r.get("ScratchSize", -1) == 0, (kernel, r)
        assert r.get("LDS Size", 1 << 30) <= 64 * 1024, (kernel, r)
    # one compiled copy of the shared kernels, in the shared layer's object
    assert not [k for k in rows if any(s in k for s in SHARED)], list(rows)
    lds = [rows[k]["LDS Size"] for k in rows if "sort_lds_kernel" in k][0]
    assert lds == 8 * MC.SORT_LDS_KEYS
    assert "monitor_device" in B.RECORDED
