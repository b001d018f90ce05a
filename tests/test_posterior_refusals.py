"""The argument refusals of the posterior tables' host entries (fitoct_summary_host,
fitoct_monitor_host, fitoct_curves_host) and of the functions that size a table
(fitoct_summary_width, fitoct_curves_width, fitoct_output_n_params), without a GPU: status and
``fitoct_last_error()`` text of every case equal, character for character, what
``tests/golden/posterior_refusals.json`` holds.  That file was recorded from the library before
the three tables' shared code moved into one translation unit
(``python tests/golden/record_posterior.py refusals``); the checks are one copy now, so a
message that changes changes for every entry at once, and this is where it shows.

A case an entry does not refuse (the rank diagnostics read no probabilities; only the curves
read ``what`` and the bins) is recorded with status 0 and an empty message.
"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import pytest

import summary_cases as SC
from fitoct_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "posterior_refusals.json")

ENTRIES = ("summary", "monitor", "curves")

# keyword arguments of call() per case
CASES = {
    "NULL problems": dict(problems=False),
    "NULL draws": dict(draws=False),
    "NULL config": dict(cfg=False),
    "NULL out": dict(out=False),
    "n_groups 0": dict(n_groups=0),
    "first_iter negative": dict(first_iter=-1),
    "three post-warmup draws": dict(iters=10, first_iter=7),
    "n_probs 17": dict(n_probs=17),
    "probability 1.5": dict(probs=(0.5, 1.5)),
    "mixed prior_type": dict(second="lasso"),
    "what 0": dict(what=0),
    "what 8": dict(what=8),
    "N 1": dict(N=1),
}

WIDTHS = {
    "fitoct_summary_width(17)": ("fitoct_summary_width", 17),
    "fitoct_summary_width(-1)": ("fitoct_summary_width", -1),
    "fitoct_curves_width(17)": ("fitoct_curves_width", 17),
    "fitoct_curves_width(-1)": ("fitoct_curves_width", -1),
    "fitoct_output_n_params(NULL)": ("fitoct_output_n_params", None),
}


def call(entry, problems=True, draws=True, cfg=True, out=True, n_groups=None, iters=10,
         second=None, what=7, N=None, **cfg_kw):
    """One call of fitoct_<entry>_host on zero draws -> [status, message] (message "" if 0)."""
    L = _lib.lib()
    ps = [SC._problem("normal", 5)] + ([SC._problem(second, 5)] if second else [])   # 16 bins
    arr = (_lib.Problem * len(ps))()
    for i, p in enumerate(ps):
        arr[i] = p.to_c()
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
    G = len(ps)
    raw = np.zeros((G, 2, iters, ps[0].D + 8))
    res = np.zeros((G, 3, 64, 21))
    args = [arr if problems else None, G if n_groups is None else n_groups, 2, iters,
            _lib.dptr(raw) if draws else None]
    if entry == "curves":
        args.append(what)
    args += [C.byref(c) if cfg else None, _lib.dptr(res) if out else None]
    rc = getattr(L, f"fitoct_{entry}_host")(*args)
    return [int(rc), L.fitoct_last_error().decode() if rc else ""]


def width(name):
    L = _lib.lib()
    fn, arg = WIDTHS[name]
    rc = getattr(L, fn)(arg)
    return [int(rc), L.fitoct_last_error().decode() if rc < 0 else ""]


def record() -> dict:
    out = {f"{e}: {k}": call(e, **kw) for e in ENTRIES for k, kw in CASES.items()}
    out.update({k: width(k) for k in WIDTHS})
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded) == sorted([f"{e}: {k}" for e in ENTRIES for k in CASES] + list(WIDTHS))
    # what the cases are there for: each is refused by at least one entry
    for k in CASES:
        assert any(recorded[f"{e}: {k}"][0] == -1 for e in ENTRIES), k


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("entry", ENTRIES)
def test_host_entry_refusal(recorded, entry, case):
    assert call(entry, **CASES[case]) == recorded[f"{entry}: {case}"]


@pytest.mark.parametrize("name", list(WIDTHS))
def test_width_refusal(recorded, name):
    assert width(name) == recorded[name]
