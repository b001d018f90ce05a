"""The pairs plot (include/fitoct.h "pairs plot") without a GPU: the defaults, sizes and struct
layouts of the new entries, their error contract (every refusal before any device call), the
host route ``fitoct_pairs_host`` against the numpy restatement of pairs_cases.py, what each
case is there for, and the Python layer over host draws (``StanFit.pairs``,
``pripost_marginals``).
"""
from __future__ import annotations

import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import pairs_cases as PC
import summary_cases as SC
from fitoct_amd import _lib
from fitoct_amd import build as B
from fitoct_amd.api import (PAIRS_WHAT, pairs_device, pairs_host, pairs_rows, pripost_marginals,
                            summary_host)
from fitoct_amd.stanfit import StanFit, materialise, output_columns

NO_DEVICE = _lib.lib().fitoct_device_count() < 1


@pytest.fixture(scope="module")
def cases():
    return {k: f() for k, f in PC.CASES.items()}


@pytest.fixture(scope="module")
def host_tables(cases):
    return {k: pairs_host(c.raw, c.probs_list, **c.kwargs()) for k, c in cases.items()}


# ---- defaults, sizes, layouts -------------------------------------------------------------------
def test_defaults_and_sizes():
    L = _lib.lib()
    c = _lib.PairsConfig()
    c.n_cols, c.cols[5], c.log_mask, c.device = 9, 3, 7, 2
    L.fitoct_default_pairs_config(C.byref(c))
    assert (c.first_iter, c.n_cols, c.n_bins, c.planes, c.log_mask, c.max_staging_bytes,
            c.device) == (0, 0, 32, 1, 0, 0, 0)
    assert tuple(c.range_probs) == (0.0, 1.0) and not any(c.cols)
    sizes = (C.c_int64 * 5)()
    assert L.fitoct_pairs_sizes(C.byref(c), 1, sizes) == -1 and b"n_cols" in L.fitoct_last_error()
    c.n_cols, c.n_bins, c.planes = 5, 7, 2
    assert L.fitoct_pairs_sizes(C.byref(c), 3, sizes) == 0
    assert list(sizes) == [3 * 5 * 8, 3 * 5 * 2 * 7, 3 * 5 * 2, 3 * 10 * 2 * 49, 3 * 25]
    c.n_cols = 1
    assert L.fitoct_pairs_sizes(C.byref(c), 1, sizes) == 0 and sizes[3] == 0
    assert L.fitoct_pairs_sizes(C.byref(c), 0, sizes) == -1
    assert L.fitoct_pairs_sizes(None, 1, sizes) == -1


def test_struct_layouts_match_ctypes(tmp_path):
    """sizeof and every offsetof of the two new structs, as a C compiler lays the header out."""
    structs = {"fitoct_pairs_config": _lib.PairsConfig, "fitoct_pairs_out": _lib.PairsOut}
    lines = []
    for name, cls in structs.items():
        lines.append(f'printf("%zu", sizeof({name}));')
        lines += [f'printf(" %zu", offsetof({name}, {f}));' for f, _ in cls._fields_]
        lines.append('printf("\\n");')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fitoct.h"\n'
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = tmp_path / "layout"
    subprocess.run([cc, f"-I{B.INCLUDE}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    for line, cls in zip(out, structs.values()):
        want = [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
        assert [int(v) for v in line.split()] == want, cls


# ---- error contract -------------------------------------------------------------------------------
def _prob(prior="normal", Nn=5, **kw):
    return SC._problem(prior, Nn, **kw)


def _call(entry, problems, chains=2, iters=10, draws=True, cfg=True, out=True, outputs=PAIRS_WHAT,
          cols=(0, 7), **cfg_kw):
    """One call of fitoct_pairs_host / _device with host buffers -> (status, message)."""
    L = _lib.lib()
    arr = None
    if problems is not None:
        arr = (_lib.Problem * len(problems))()
        for i, p in enumerate(problems):
            arr[i] = p.to_c()
    c = _lib.PairsConfig()
    L.fitoct_default_pairs_config(C.byref(c))
    c.n_cols = len(cols)
    for j, v in enumerate(cols[:64]):
        c.cols[j] = v
    for k, v in cfg_kw.items():
        if k == "range_probs":
            c.range_probs[0], c.range_probs[1] = v
        else:
            setattr(c, k, v)
    G = len(problems) if problems else 1
    W = (problems[0].D if problems else 3) + 8
    raw = np.zeros((G, chains, max(iters, 1), W))
    bufs = {w: np.zeros(G * 64 * 65 * 2, dtype=np.float64 if w in ("edges", "corr") else np.int64)
            for w in outputs}
    o = _lib.PairsOut()
    for f, w in (("edges", "edges"), ("hist1", "hist"), ("outside", "outside"),
                 ("hist2", "panels"), ("corr", "corr")):
        if w in bufs:
            setattr(o, f, bufs[w].ctypes.data_as(_lib._dp if w in ("edges", "corr") else _lib._lp))
    cp, op = (C.byref(c) if cfg else None), (C.byref(o) if out else None)
    if entry == "device":
        rc = L.fitoct_pairs_device(arr, G, chains, iters, raw.ctypes.data if draws else None, None,
                                   cp, None, op)
    else:
        rc = L.fitoct_pairs_host(arr, G, chains, iters, _lib.dptr(raw) if draws else None, None,
                                 cp, op)
    return rc, L.fitoct_last_error().decode()


BAD = {   # what is wrong -> (the call, a word of the message)
    "too few post-warmup draws": (dict(iters=10, first_iter=7), "post-warmup"),
    "three draws": (dict(iters=3), "post-warmup"),
    "negative first_iter": (dict(first_iter=-1), "first_iter"),
    "negative max_staging_bytes": (dict(max_staging_bytes=-1), "max_staging_bytes"),
    "NULL draws": (dict(draws=False), "NULL"),
    "NULL config": (dict(cfg=False), "NULL"),
    "NULL out": (dict(out=False), "NULL"),
    "no chains": (dict(chains=0), "chains"),
    "n_cols 0": (dict(cols=()), "n_cols"),
    "n_cols 65": (dict(cols=tuple(range(64)), n_cols=65), "n_cols"),
    "column below 0": (dict(cols=(0, -1)), "cols[1]"),
    "column at P": (dict(cols=(len(output_columns(SC._problem("normal", 5))), 0)), "cols[0]"),
    "column repeated": (dict(cols=(3, 8, 3)), "cols[2]"),
    "n_bins 1": (dict(n_bins=1), "n_bins"),
    "n_bins 65": (dict(n_bins=65), "n_bins"),
    "planes 0": (dict(planes=0), "planes"),
    "planes 3": (dict(planes=3), "planes"),
    "p_lo negative": (dict(range_probs=(-0.1, 0.9)), "range_probs"),
    "p_hi above 1": (dict(range_probs=(0.1, 1.1)), "range_probs"),
    "p_lo equals p_hi": (dict(range_probs=(0.5, 0.5)), "range_probs"),
    "p_lo above p_hi": (dict(range_probs=(0.9, 0.1)), "range_probs"),
    "p_lo NaN": (dict(range_probs=(float("nan"), 0.9)), "range_probs"),
    "log_mask bit at n_cols": (dict(log_mask=1 << 2), "log_mask"),
    "every output NULL": (dict(outputs=()), "out"),
}


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors(entry, what):
    kw, word = BAD[what]
    rc, msg = _call(entry, [_prob()], **kw)
    assert rc == -1 and word in msg, (what, rc, msg)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_null_problems_and_mixed_groups(entry):
    rc, msg = _call(entry, None)
    assert rc == -1 and msg
    a = _prob()
    for other in (_prob("lasso"), _prob(Nn=6), _prob(prior_PD=1)):
        rc, msg = _call(entry, [a, other])
        assert rc == -1 and "group" in msg, (rc, msg)


def test_valid_call_needs_a_device():
    """Every check passes, then: no device -> FITOCT_E_NODEVICE; with one, the host pointer
    given as d_draws is refused (FITOCT_E_ARG) before any kernel runs."""
    rc, msg = _call("device", [_prob()])
    assert rc == (-3 if NO_DEVICE else -1) and msg, (rc, msg)
    for outputs in (PAIRS_WHAT, ("corr",), ("outside",)):
        rc, _ = _call("host", [_prob()], outputs=outputs, log_mask=3, cols=(0, 8))
        assert rc == 0
    rc, _ = _call("host", [_prob("horseshoe", 24)], cols=tuple(range(64)), n_bins=2)   # 64 columns
    assert rc == 0


def test_plan_and_batch_entries_need_handles():
    L = _lib.lib()
    c, o = _lib.PairsConfig(), _lib.PairsOut()
    L.fitoct_default_pairs_config(C.byref(c))
    assert L.fitoct_plan_pairs(None, None, C.byref(c), C.byref(o)) == -1 and L.fitoct_last_error()
    assert L.fitoct_batch_pairs(None, None, C.byref(c), C.byref(o)) == -1 and L.fitoct_last_error()


# ---- host route against numpy ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.CASES))
def test_host_matches_numpy(cases, host_tables, name):
    case = cases[name]
    summary = summary_host(case.raw, case.probs_list, case.first_iter, case.range_probs)
    PC.check_case(case, host_tables[name], summary, f"host/numpy {name}")


def test_case_properties(cases, host_tables):
    """What each case is there for shows in the tables."""
    t = host_tables["p1"]
    assert len(t["columns"]) == 40 and t["hist"].shape == (1, 40, 2, 7)
    assert 20 <= t["hist"][0, 0, 1].sum() <= 60 and t["hist"][0, 0, 0].sum() == 400   # ~10 % divergent
    t = host_tables["p2"]
    assert t["columns"] == ["lp__", "yGP.2", "theta.1", "lambda", "sigma"]
    lam = t["columns"].index("lambda")
    assert np.all(np.isnan(t["edges"][0, lam])) and not t["hist"][0, lam].any()
    assert np.all(t["outside"][0, [0, 1, 2, 4]] > 0) and not t["outside"][0, lam].any()
    assert np.all(np.isnan(t["corr"][0, lam])) and np.all(np.isnan(t["corr"][0, :, lam]))
    # p3: the NaN blanks yGP.2 of group 2 and touches no other group
    t, clean = host_tables["p3"], host_tables["p3c"]
    assert len(t["columns"]) == 22 and t["panels"].shape[:2] == (6, 231)
    y2 = t["columns"].index("yGP.2")
    for g in range(6):
        if g != 2:
            assert PC.group_bytes(t, g) == PC.group_bytes(clean, g), g
    assert np.all(np.isnan(t["edges"][2, y2])) and not t["hist"][2, y2].any()
    keep = [j for j in range(22) if j != y2]
    assert np.array_equal(t["hist"][2, keep], clean["hist"][2, keep])
    assert np.array_equal(t["corr"][2][np.ix_(keep, keep)].view(np.uint64),
                          clean["corr"][2][np.ix_(keep, keep)].view(np.uint64))
    # p4: no panel with one column; geometric edges
    t = host_tables["p4a"]
    assert t["panels"].shape == (1, 0, 1, 2, 2) and t["corr"].tolist() == [[[1.0]]]
    e = host_tables["p4b"]["edges"][0]
    assert np.allclose(e[:, 1:] / e[:, :-1], (e[:, -1:] / e[:, :1]) ** (1 / 32), rtol=1e-12, atol=0)
    # p5: values exactly on edges
    case = cases["p5a"]
    m, names, _ = PC.pooled(case, 0)
    depth, energy = m[:, names.index("treedepth__")], m[:, names.index("energy__")]
    t = host_tables["p5a"]
    assert t["edges"][0, 0].tolist() == [1.0, 2.0, 3.0]
    assert t["hist"][0, 0, 0].tolist() == [np.sum(depth == 1), np.sum(depth >= 2)]   # 2 opens bin 1
    assert not t["outside"][0, 0].any()                                               # 3 is inside
    t = host_tables["p5b"]
    zeros = np.sum(energy == 0)   # -0.0 and +0.0: bin 0
    assert zeros >= 3 and np.signbit(energy[energy == 0]).any()
    assert t["hist"][0, 1, 0][0] == np.sum((energy >= 0) & (energy < t["edges"][0, 1, 1]))
    assert t["outside"][0, 1].tolist() == [np.sum(energy < 0), 0] and np.sum(energy == -5e-324) == 1
    assert t["hist"][0, 1, 0][-1] >= 1   # the maximum falls in the closed last bin
    assert host_tables["p6"]["S"] == 4


def test_explicit_ranges_and_parts(cases):
    """Explicit ranges are the edges' ends; a NaN entry is automatic; ``what`` selects."""
    case = cases["p2"]
    auto = pairs_host(case.raw, case.probs_list, **case.kwargs())
    t = pairs_host(case.raw, case.probs_list, pars=case.pars, n_bins=8, what=("edges", "outside"),
                   range_probs=case.range_probs, ranges={"sigma": (0.5, 2.5), "lambda": (9.0, 11.0)})
    assert sorted(k for k in t if k in PAIRS_WHAT) == ["edges", "outside"]
    assert t["edges"][0, 4].tolist() == list(0.5 + 0.25 * np.arange(9))
    assert t["edges"][0, 3, [0, -1]].tolist() == [9.0, 11.0]           # a given range is a grid
    assert np.array_equal(t["edges"][0, :3, [0, -1]], auto["edges"][0, :3, [0, -1]])
    rows = pairs_rows(auto)
    assert list(rows["panels"])[:2] == [("lp__", "yGP.2"), ("lp__", "theta.1")]
    assert rows["panels"][("theta.1", "sigma")].shape == (1, 64, 64) and rows["S"] == 903
    with pytest.raises(KeyError):
        pairs_host(case.raw, case.probs_list, pars=("sigma",), log=("nope",))
    with pytest.raises(KeyError):
        pairs_host(case.raw, case.probs_list, pars=("sigma",), ranges={"theta.1": (0, 1)})
    with pytest.raises(ValueError):
        pairs_host(case.raw, case.probs_list, what=("nope",))
    with pytest.raises(_lib.FitOCTError):   # a host pointer, or no device
        pairs_device(case.raw.ctypes.data, case.probs_list, 3, 301)


# ---- the Python layer over host draws -------------------------------------------------------------
def _fit(case):
    prob = case.probs_list[0]
    return StanFit(materialise(case.raw[0], prob), output_columns(prob), case.first_iter,
                   source=("sample", prob, None, case.raw[0], 0.0))


def test_stanfit_pairs_default_pars():
    a = SC.case_a()
    rows = _fit(a).pairs(n_bins=7, planes=2)
    want = [c for c in output_columns(a.probs_list[0])
            if c.split(".")[0] in ("theta", "yGP", "lambda", "sigma", "br", "lp__")]
    assert sorted(rows["columns"]) == sorted(want) and rows["columns"][:3] == ["theta.1", "theta.2", "theta.3"]
    assert rows["columns"][-1] == "lp__" and rows["S"] == 400
    t = pairs_host(a.raw, a.probs_list, 50, n_bins=7, planes=2)
    for w in ("edges", "hist", "outside", "corr"):
        assert rows[w].tobytes() == t[w][0].tobytes(), w
    assert rows["panels"] == {} or all(
        np.array_equal(v, t["panels"][0, i]) for i, v in enumerate(rows["panels"].values()))
    with pytest.raises(ValueError):
        StanFit(np.zeros((1, 4, 2)), ["a", "b"], 0).pairs()


def test_pripost_marginals_on_host_fits():
    """plotPriPostAll: a prior run (no br) and a posterior run binned over common edges."""
    post, pri = SC.case_a(), SC.case_g()
    got = pripost_marginals(_fit(pri), _fit(post), n_bins=12)
    cols = _fit(pri).pairs(what=("edges",))["columns"]
    assert list(got) == cols and "br" not in got and "lp__" in got
    S = {"prior": 4 * 60, "posterior": 4 * 100}
    for name, r in got.items():
        assert r["edges"].shape == (13,) and np.all(np.diff(r["edges"]) > 0), name
        for side in ("prior", "posterior"):
            assert r[side].shape == (12,) and r[side].sum() + sum(r[side + "_outside"]) == S[side]
    # the union of the two automatic ranges
    e = [_fit(c).pairs(pars=("sigma",), range_probs=(0.005, 0.995), what=("edges",))["edges"][0]
         for c in (pri, post)]
    assert got["sigma"]["edges"][0] == min(e[0][0], e[1][0])
    assert got["sigma"]["edges"][-1] == max(e[0][-1], e[1][-1])
