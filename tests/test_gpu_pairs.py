"""The pairs plot on the device (fitoct_pairs_device, Plan.pairs, Batch.pairs,
pripost_marginals): against the numpy restatement and the host route on the cases of
pairs_cases.py (counts exactly, the correlation within the derived bound), bit for bit across
calls and staging caps, on real runs through the buffers a run can leave its draws in, and the
refusals that come before any kernel is launched.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import pairs_cases as PC
from fitoct_amd import _lib
from fitoct_amd.api import (PAIRS_WHAT, Batch, ExpGPProblem, Plan, SamplerConfig, pairs_device,
                            pairs_host, pripost_marginals, summary_device)
from fitoct_amd.synth import default_prior, synth_decay

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return {k: f() for k, f in PC.CASES.items()}


@pytest.fixture(scope="module")
def on_device(cases):
    import torch
    return {k: torch.from_numpy(c.raw).to("cuda") for k, c in cases.items()}


def _device_tables(case, buf, **kw):
    _, C_, I, _ = case.raw.shape
    return pairs_device(buf.data_ptr(), case.probs_list, C_, I, **case.kwargs(), **kw)


def _all_bytes(case, t):
    return b"".join(PC.group_bytes(t, g) for g in range(len(case.probs_list)))


def _check_routes(case, dev, host, what):
    """Device against host: every integer output and the edges equal where no interpolated
    quantile is involved, the correlation within the bound."""
    assert dev["columns"] == host["columns"] and dev["S"] == host["S"]
    for g in range(len(case.probs_list)):
        if case.exact_edges:
            for w in ("edges",) + PC.INT_TABLES:
                assert dev[w][g].tobytes() == host[w][g].tobytes(), (what, g, w)
        m, names, _ = PC.pooled(case, g)
        x = m[:, [names.index(c) for c in dev["columns"]]]
        PC.check_corr(dev["corr"][g], x, f"{what} device/host group {g}", reference=host["corr"][g])


@pytest.mark.parametrize("name", list(PC.CASES))
def test_device_matches_numpy_and_host(cases, on_device, name):
    case, buf = cases[name], on_device[name]
    _, C_, I, _ = case.raw.shape
    dev = _device_tables(case, buf)
    summary = summary_device(buf.data_ptr(), case.probs_list, C_, I, case.first_iter,
                             case.range_probs)
    PC.check_case(case, dev, summary, f"device/numpy {name}")
    _check_routes(case, dev, pairs_host(case.raw, case.probs_list, **case.kwargs()), name)
    assert _all_bytes(case, _device_tables(case, buf)) == _all_bytes(case, dev)   # call to call


@pytest.mark.parametrize("name", ["p1", "p3"])
def test_staging_cap_does_not_change_a_bit(cases, on_device, name):
    """One column per select pass (never fewer) against all columns in one pass."""
    case, buf = cases[name], on_device[name]
    assert (_all_bytes(case, _device_tables(case, buf, max_staging_bytes=1)) ==
            _all_bytes(case, _device_tables(case, buf)))


def test_a_nan_blanks_its_own_group_only(cases, on_device):
    t, clean = (_device_tables(cases[k], on_device[k]) for k in ("p3", "p3c"))
    y2 = t["columns"].index("yGP.2")
    for g in range(6):
        if g != 2:
            assert PC.group_bytes(t, g) == PC.group_bytes(clean, g), g
    assert np.all(np.isnan(t["edges"][2, y2])) and not t["hist"][2, y2].any()
    assert np.all(np.isnan(t["corr"][2, y2]))


@pytest.mark.parametrize("name", ["p5b", "p2", "p3"])
def test_parts(cases, on_device, name):
    """Only the wanted outputs are computed, to the same bytes: p5b gives every range (no select
    at all); a call for the correlation alone digitises nothing and takes the columns' flags
    from the mean pass (p2's constant lambda, p3's NaN)."""
    case, buf = cases[name], on_device[name]
    full = _device_tables(case, buf)
    for what in (("corr",), ("outside",), ("panels", "edges")):
        part = _device_tables(case, buf, what=what)
        assert sorted(k for k in part if k in PAIRS_WHAT) == sorted(what)
        for w in what:
            assert part[w].tobytes() == full[w].tobytes(), w


# ---- real runs ----------------------------------------------------------------------------------
def _prob(prior, N, Nn, seed=3, **kw):
    t0, S0 = default_prior()
    d = synth_decay(N, "sincExp", seed)
    return ExpGPProblem(d["x"], d["y"], d["uy"], Nn=Nn, gridType="extremal", theta0=t0,
                        Sigma0=S0, prior_type=prior, **kw)


def _tables(rows):
    """A pairs dict of one problem back as tables over one group."""
    t = {w: rows[w][None] for w in ("edges", "hist", "outside", "corr")}
    t["panels"] = np.stack(list(rows["panels"].values()))[None]
    t["columns"], t["S"] = rows["columns"], rows["S"]
    return t


def _rows_bytes(rows):
    return PC.group_bytes(_tables(rows), 0)


@pytest.fixture(scope="module")
def horseshoe():
    return _prob("horseshoe", 97, 8), SamplerConfig(chains=8, warmup=50, samples=60, seed=21)


@pytest.mark.parametrize("save_warmup", [True, False])
def test_plan_pairs(horseshoe, save_warmup):
    prob, cfg = horseshoe
    with Plan(prob, dataclasses.replace(cfg, save_warmup=save_warmup)) as pl:
        pl.run()
        got = pl.pairs(planes=2)
        out = pl.download()
    first = 50 if save_warmup else 0
    assert got["S"] == 480 and got["columns"][-1] == "lp__" and "br" in got["columns"]
    assert list(got["panels"])[0] == ("theta.1", "theta.2")
    case = PC.Case("run", [prob], np.ascontiguousarray(out.draws)[None], first_iter=first, planes=2)
    host = pairs_host(out.draws, prob, first, planes=2)
    _check_routes(case, _tables(got), host, f"plan save_warmup={save_warmup}")


def test_plan_pairs_in_a_callers_buffer(horseshoe):
    """The run writes into the caller's d_draws; the table reads it there, and the direct entry
    on that buffer gives the same bytes."""
    import torch
    prob, cfg = horseshoe
    kw = dict(pars=("tau", "lambda", "lp__"), n_bins=8, planes=2, range_probs=(0.1, 0.9),
              log=("tau", "lambda"))
    with Plan(prob, cfg) as pl:
        buf = torch.full((pl.info["draws_bytes"] // 8,), float("nan"), dtype=torch.float64,
                         device="cuda")
        pl.run(d_draws=buf.data_ptr())
        got = pl.pairs(**kw)
        direct = pairs_device(buf.data_ptr(), prob, 8, pl.info["iters_saved"], first_iter=50, **kw)
        out = pl.download()
    assert got["columns"] == ["tau"] + [f"lambda.{k}" for k in range(1, 9)] + ["lp__"]
    assert _rows_bytes(got) == PC.group_bytes(direct, 0)
    case = PC.Case("run", [prob], np.ascontiguousarray(out.draws)[None], first_iter=50, **kw)
    host = pairs_host(out.draws, prob, 50, **kw)
    _check_routes(case, direct, host, "caller's buffer")
    summary = summary_device(buf.data_ptr(), prob, 8, pl.info["iters_saved"], 50, (0.1, 0.9))
    PC.check_case(case, direct, summary, "caller's buffer device/numpy")


def test_batch_pairs_equal_single_plans():
    """3 files x 4 chains, N = 481: each file's dict is a single plan's of that file, byte for
    byte, and problem= selects."""
    probs = [_prob("normal", 481, 10, seed=s) for s in (3, 4, 5)]
    cfg = SamplerConfig(chains=4, warmup=30, samples=30, seed=8)
    with Batch(probs, cfg) as b:
        b.run()
        got = b.pairs(planes=2, n_bins=16)
        one = b.pairs(problem=1, planes=2, n_bins=16)
    assert len(got) == 3 and _rows_bytes(one) == _rows_bytes(got[1])
    for p in range(3):
        with Plan(probs[p], dataclasses.replace(cfg, chain_offset=4 * p)) as pl:
            pl.run()
            single = pl.pairs(planes=2, n_bins=16)
        assert single["columns"] == got[p]["columns"]
        assert _rows_bytes(single) == _rows_bytes(got[p]), p


def test_pripost_marginals():
    """plotPriPostAll: a prior_PD = 1 plan and a prior_PD = 0 plan of the same problem."""
    cfg = SamplerConfig(chains=4, warmup=30, samples=40, seed=5)
    with Plan(_prob("normal", 97, 6, prior_PD=1), cfg) as pri, Plan(_prob("normal", 97, 6), cfg) as post:
        pri.run()
        post.run()
        got = pripost_marginals(pri, post, n_bins=10)
        cols = pri.pairs(what=("edges",))["columns"]
        ranges = {n: (r["edges"][0], r["edges"][-1]) for n, r in got.items()
                  if not np.isnan(r["edges"][0])}
        sides = [h.pairs(pars=list(ranges), n_bins=10, ranges=ranges, what=("edges",))["edges"]
                 for h in (pri, post)]
    assert sides[0].tobytes() == sides[1].tobytes()   # the edges are common, bit for bit
    assert sides[0].tobytes() == np.stack([got[n]["edges"] for n in ranges]).tobytes()
    assert list(got) == cols and "br" not in got and "sigma" in got
    for name, r in got.items():
        if np.all(np.isnan(r["edges"])):   # (a constant column has no grid on either side)
            continue
        assert r["edges"].shape == (11,) and np.all(np.diff(r["edges"]) > 0), name
        for side in ("prior", "posterior"):
            assert r[side].sum() + sum(r[side + "_outside"]) == 4 * 40, (name, side)


# ---- refusals (each before any kernel is launched) ----------------------------------------------
def test_refusals(horseshoe):
    prob, cfg = horseshoe
    with Plan(prob, cfg) as pl:
        with pytest.raises(_lib.FitOCTError) as ei:       # before any run
            pl.pairs()
        assert ei.value.code == -1 and "not run" in str(ei.value)
        pl.launch()
        with pytest.raises(_lib.FitOCTError) as ei:       # a launch is in flight
            pl.pairs()
        assert ei.value.code == -1 and "fitoct_plan_wait" in str(ei.value)
        pl.wait()
        assert "corr" in pl.pairs(what=("corr",))
        with pytest.raises(_lib.FitOCTError) as ei:
            pl.pairs(n_bins=65)
        assert ei.value.code == -1 and "n_bins" in str(ei.value)
    raw = np.zeros((2, 10, prob.D + 8))
    with pytest.raises(_lib.FitOCTError) as ei:           # a host pointer as d_draws
        pairs_device(raw.ctypes.data, prob, 2, 10)
    assert ei.value.code == -1 and "device buffer" in str(ei.value)
    with Plan(prob, dataclasses.replace(cfg, devices=(0, 0))) as pl:
        pl.run()                                          # shards stay in per-device buffers
        with pytest.raises(_lib.FitOCTError) as ei:
            pl.pairs()
        assert ei.value.code == -1 and "d_draws" in str(ei.value)
    with Batch([prob, prob], dataclasses.replace(cfg, chains=2)) as b:
        with pytest.raises(_lib.FitOCTError) as ei:
            b.pairs()
        assert ei.value.code == -1 and "not run" in str(ei.value)
