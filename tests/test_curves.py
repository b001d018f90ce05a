"""The posterior curves (include/fitoct.h "posterior curves") without a GPU: the width, the error
contract of the entries (every refusal before any device call), the host route
``fitoct_curves_host`` against a numpy restatement within the derived bound of
curves_cases.py, the precondition of that bound, and the register gate of the new kernels.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import curves_cases as CC
from fitoct_amd import _lib
from fitoct_amd import build as B
from fitoct_amd.api import curves_host, curves_rows

NO_DEVICE = _lib.lib().fitoct_device_count() < 1


@pytest.fixture(scope="module")
def cases():
    return {k: f() for k, f in CC.CASES.items()}


@pytest.fixture(scope="module")
def host_tables(cases):
    return {k: curves_host(c.raw, c.probs_list, c.first_iter, c.probs, c.what)
            for k, c in cases.items()}


# ---- width and error contract -------------------------------------------------------------------
def test_width():
    L = _lib.lib()
    assert [L.fitoct_curves_width(k) for k in (0, 5, 16)] == [2, 7, 18]
    assert L.fitoct_curves_width(17) == -1 and L.fitoct_last_error()
    assert L.fitoct_curves_width(-1) == -1


def _prob(prior="normal", Nn=5, N=16, **kw):
    return CC.problem(prior, Nn, N, CC._rng(1), **kw)


def _call(entry, problems, chains=2, iters=10, draws=True, cfg=True, out=True, what=7,
          null=(), N=None, n_pick=2, pick=(0, 1), **cfg_kw):
    """One call of fitoct_curves_device / _host / _pick_device with host buffers ->
    (status, message)."""
    L = _lib.lib()
    arr = None
    if problems is not None:
        arr = (_lib.Problem * len(problems))()
        for i, p in enumerate(problems):
            arr[i] = p.to_c()
            for f in null:
                setattr(arr[i], f, None)
            if N is not None:
                arr[i].N = N
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
    res = np.zeros((G, 3, 64, 18))
    cp = C.byref(c) if cfg else None
    if entry == "device":
        rc = L.fitoct_curves_device(arr, G, chains, iters, raw.ctypes.data if draws else None,
                                    what, cp, None, _lib.dptr(res) if out else None)
    elif entry == "host":
        rc = L.fitoct_curves_host(arr, G, chains, iters, _lib.dptr(raw) if draws else None, what,
                                  cp, _lib.dptr(res) if out else None)
    else:
        idx = np.asarray(pick, dtype=np.int64)
        rc = L.fitoct_curves_pick_device(arr, G, chains, iters,
                                         raw.ctypes.data if draws else None, cp, None, n_pick,
                                         idx.ctypes.data_as(_lib._lp), _lib.dptr(res), None, None,
                                         None)
    return rc, L.fitoct_last_error().decode()


BAD = {
    "too few post-warmup draws": dict(iters=10, first_iter=7),
    "three draws": dict(iters=3),
    "negative first_iter": dict(first_iter=-1),
    "n_probs below 0": dict(n_probs=-1),
    "n_probs above 16": dict(n_probs=17),
    "probability above 1": dict(probs=(0.5, 1.5)),
    "probability NaN": dict(probs=(0.5, float("nan"))),
    "negative max_staging_bytes": dict(max_staging_bytes=-1),
    "NULL draws": dict(draws=False),
    "NULL config": dict(cfg=False),
    "NULL out": dict(out=False),
    "no chains": dict(chains=0),
    "what is 0": dict(what=0),
    "what has unknown bits": dict(what=8),
    "what is negative": dict(what=-1),
    "x is NULL": dict(null=("x",)),
    "y is NULL": dict(null=("y",)),
    "uy is NULL": dict(null=("uy",)),
    "N below 2": dict(N=1),
}


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors(entry, what):
    rc, msg = _call(entry, [_prob()], **BAD[what])
    assert rc == -1 and msg, (what, rc, msg)


@pytest.mark.parametrize("entry", ["device", "host", "pick"])
def test_null_problems_and_mixed_groups(entry):
    rc, msg = _call(entry, None)
    assert rc == -1 and msg
    a = _prob()
    for other in (_prob("lasso"), _prob(Nn=6), _prob(prior_PD=1)):
        rc, msg = _call(entry, [a, other])
        assert rc == -1 and "group" in msg, (rc, msg)


PICK_BAD = {
    "index at S": dict(pick=(0, 20)),
    "index below 0": dict(pick=(-1, 3)),
    "negative n_pick": dict(n_pick=-1),
    "x is NULL": dict(null=("x",)),
    "N below 2": dict(N=1),
    "too few post-warmup draws": dict(first_iter=7),
    "NULL draws": dict(draws=False),
    "NULL config": dict(cfg=False),
}


@pytest.mark.parametrize("what", list(PICK_BAD))
def test_pick_argument_errors(what):
    rc, msg = _call("pick", [_prob()], **PICK_BAD[what])   # S = 2 x 10 = 20
    assert rc == -1 and msg, (what, rc, msg)
    if what.startswith("index"):
        assert "pick[" in msg


def test_valid_call_needs_a_device():
    """Every check passes, then: no device -> FITOCT_E_NODEVICE; with one, the host pointer
    given as d_draws is refused (FITOCT_E_ARG) before any kernel runs."""
    for entry in ("device", "pick"):
        rc, msg = _call(entry, [_prob()])
        assert rc == (-3 if NO_DEVICE else -1) and msg, (entry, rc, msg)
    rc, _ = _call("host", [_prob()])
    assert rc == 0


def test_plan_and_batch_entries_need_handles():
    L = _lib.lib()
    c = _lib.SummaryConfig()
    L.fitoct_default_summary_config(C.byref(c))
    out = np.zeros(64)
    idx = np.zeros(1, dtype=np.int64).ctypes.data_as(_lib._lp)
    o = _lib.dptr(out)
    assert L.fitoct_plan_curves(None, 7, C.byref(c), o) == -1 and L.fitoct_last_error()
    assert L.fitoct_batch_curves(None, 7, C.byref(c), o) == -1 and L.fitoct_last_error()
    assert L.fitoct_plan_curves_pick(None, C.byref(c), 1, idx, o, None, None, None) == -1
    assert L.fitoct_batch_curves_pick(None, 0, C.byref(c), 1, idx, o, None, None, None) == -1
    assert L.fitoct_plan_curves_pick_params(None, C.byref(c), 1, idx, o, None) == -1
    assert L.fitoct_batch_curves_pick_params(None, 0, C.byref(c), 1, idx, o, None) == -1


# ---- host route against numpy -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.CASES))
def test_bound_precondition(cases, name):
    """The bound needs 1 + dL away from 0, and the cases keep |yGP| <= 0.05."""
    case = cases[name]
    for g, prob in enumerate(case.probs_list):
        if g in case.nan_groups:
            continue
        theta, ygp = CC.pooled_params(case, g)
        assert ygp.size == 0 or np.max(np.abs(ygp)) <= CC.YGP_MAX
        dL = CC.draw_curves(prob, theta, ygp)["dL"]
        assert np.min(1 + dL) >= 0.5, (name, g, np.min(1 + dL))


@pytest.mark.parametrize("name", list(CC.CASES))
def test_host_matches_numpy(cases, host_tables, name):
    case = cases[name]
    what = CC.ordered(case.what)
    want = []
    for g, prob in enumerate(case.probs_list):
        theta, ygp = CC.pooled_params(case, g)
        want.append(CC.numpy_block(prob, theta, ygp, what, case.probs))
    assert host_tables[name].size == sum(w.size for w in want)
    CC.check_blocks(case, CC.blocks(case, host_tables[name]), want, f"host/numpy {name}")


def test_case_properties(cases, host_tables):
    """What each case is there for shows in the table."""
    c = CC.blocks(cases["c"], host_tables["c"])[0]
    assert np.all(c[0] == 0.0) and not np.any(np.signbit(c[0]))   # monoexp: dL is exactly 0
    assert np.all(c[1][:, 1] > 0)
    b, d = CC.blocks(cases["b"], host_tables["b"]), CC.blocks(cases["d"], host_tables["d"])
    assert [x.shape[1] for x in b] == [70, 70, 70, 53, 70, 70]
    for g in range(6):
        if g == 2:
            assert np.all(np.isnan(d[g])) and not np.any(np.isnan(b[g]))
        else:   # a NaN blanks its own group and no other
            assert d[g].tobytes() == b[g].tobytes()
    a = CC.blocks(cases["a"], host_tables["a"])[0]
    for name, q in (("f-dL", 0), ("f-m", 1), ("f-resid", 2)):
        one = CC.blocks(cases[name], host_tables[name])[0]
        assert one.shape[0] == 1 and one[0].tobytes() == a[q].tobytes()
    two = CC.blocks(cases["f-dL-resid"], host_tables["f-dL-resid"])[0]
    assert two[0].tobytes() == a[0].tobytes() and two[1].tobytes() == a[2].tobytes()
    w2 = CC.blocks(cases["f-width2"], host_tables["f-width2"])[0]
    assert w2.shape[2] == 2 and w2.tobytes() == np.ascontiguousarray(a[:, :, :2]).tobytes()
    p16 = CC.blocks(cases["f-16probs"], host_tables["f-16probs"])[0]
    theta, ygp = CC.pooled_params(cases["a"], 0)
    m = CC.draw_curves(cases["a"].probs_list[0], theta, ygp)["m"]
    assert np.array_equal(p16[1][:, 2], m.min(axis=0)) and np.array_equal(p16[1][:, -1], m.max(axis=0))


def test_curves_rows_dict(cases, host_tables):
    case = cases["f-dL-resid"]
    rows = curves_rows(CC.blocks(case, host_tables["f-dL-resid"])[0], case.probs_list[0], case.what,
                       case.probs)
    assert list(rows) == ["dL", "resid", "x"]
    assert list(rows["dL"]) == ["mean", "sd", "2.5%", "25%", "50%", "75%", "97.5%"]
    assert rows["resid"]["50%"].shape == (37,) and np.array_equal(rows["x"], case.probs_list[0].x)
    with pytest.raises(ValueError):
        curves_host(case.raw, case.probs_list, what=("nope",))


def test_a_callers_basis_is_used(cases):
    """Case b's group 4 carries 0.9 x its built basis: its dL band is 0.9 x the built one's."""
    case = cases["b"]
    p = case.probs_list[4]
    own = curves_host(case.raw[4], p, what=("dL",))
    built = curves_host(case.raw[4], dataclasses.replace(p, B=None), what=("dL",))
    assert np.allclose(own, 0.9 * built, rtol=1e-12, atol=0) and not np.array_equal(own, built)


# ---- register gate of the new object ------------------------------------------------------------
def test_curves_kernels_do_not_spill():
    """The -Rpass-analysis=kernel-resource-usage remarks fitoct_amd.build keeps beside the
    curves object: 0 spilled VGPRs, 0 scratch and at most 64 KiB of LDS for every kernel of it
    (recompiled device-only for the remarks if the record is missing or stale)."""
    src = os.path.join(B.CSRC, "curves_device.hip")
    path = os.path.join(B.OBJDIR, "curves_device.resources.txt")
    if os.path.exists(path) and os.path.getmtime(path) >= B._newest_dep(src):
        text = open(path).read()
    else:
        out = os.path.join("/tmp", f"fitoct_resources_curves_{os.getpid()}.o")
        r = subprocess.run([B._hipcc(), *B._KERNEL, f"-I{B.INCLUDE}", f"-I{B.CSRC}",
                            "--cuda-device-only", "-c", src, "-o", out,
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        os.remove(out)
        text = r.stderr
    rows = B.kernel_resources(text)
    for kernel in ("params_kernel", "curve_pick_kernel", "curve_kernelILi0E", "curve_kernelILi15E",
                   "curve_kernelILi24E"):
        assert len([k for k in rows if kernel in k]) == 1, (kernel, list(rows))
    # the shared kernels (test_summary.py gates them) are the shared layer's object's alone
    assert len(rows) == 5, list(rows)
    for kernel, r in rows.items():
        assert r.get("VGPRs Spill", -1) == 0 and r.get("ScratchSize", -1) == 0, (kernel, r)
        assert r.get("LDS Size", 1 << 30) <= 64 * 1024, (kernel, r)
    assert "curves_device" in B.RECORDED
