"""The posterior curves on the device (fitoct_curves_device, Plan.curves, Batch.curves, the pick
entries): against the host route on the synthetic cases of curves_cases.py within the derived
bound, bit for bit across pass sizes and calls, against the host route and
``genquant.expgp_curves`` on real runs through the buffers a run can leave its draws in, the
summary's table unchanged by the move of its select code, and the refusals that come before
any kernel is launched.
"""
from __future__ import annotations

import dataclasses
import os

import numpy as np
import pytest

import curves_cases as CC
import summary_cases as SC
from fitoct_amd import _lib
from fitoct_amd.api import (Batch, ExpGPProblem, Plan, SamplerConfig, curves_blocks,
                            curves_device, curves_host, summary_device)
from fitoct_amd.genquant import expgp_curves
from fitoct_amd.stanfit import materialise, output_columns
from fitoct_amd.synth import default_prior, synth_decay

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def cases():
    return {k: f() for k, f in CC.CASES.items()}


def _device_table(case, **kw):
    import torch
    t = torch.from_numpy(case.raw).to("cuda")
    _, C_, I, _ = case.raw.shape
    return curves_device(t.data_ptr(), case.probs_list, C_, I, case.first_iter, case.probs,
                         case.what, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_device_matches_host(cases, name):
    case = cases[name]
    host = curves_host(case.raw, case.probs_list, case.first_iter, case.probs, case.what)
    dev = _device_table(case)
    assert dev.shape == host.shape
    CC.check_blocks(case, CC.blocks(case, dev), CC.blocks(case, host), f"device/host {name}")
    again = _device_table(case)
    assert _bits(again).tobytes() == _bits(dev).tobytes()   # reproducible bit for bit
    if name == "c":
        assert np.all(CC.blocks(case, dev)[0][0] == 0.0)     # monoexp: dL is exactly 0
    if name == "d":   # the NaN blanks group 2; every other group is case b's, bit for bit
        b = CC.blocks(cases["b"], _device_table(cases["b"]))
        for g, blk in enumerate(CC.blocks(case, dev)):
            assert np.all(np.isnan(blk)) if g == 2 else blk.tobytes() == b[g].tobytes(), g


def test_passes_do_not_change_a_bit(cases):
    """Case b in one pass, with one pair per pass and with 7 pairs per pass."""
    case = cases["b"]
    one = _device_table(case)
    _, C_, I, _ = case.raw.shape
    pair_bytes = C_ * (I - case.first_iter) * 8
    each = _device_table(case, max_staging_bytes=1)   # never fewer than one pair per pass
    assert _bits(each).tobytes() == _bits(one).tobytes()
    seven = _device_table(case, max_staging_bytes=7 * pair_bytes + 5)
    assert _bits(seven).tobytes() == _bits(one).tobytes()


def test_summary_table_is_unchanged():
    """The summary's select kernels and their set-up moved to the shared header: its device
    table of summary_cases' case a is the bytes recorded before the move."""
    import torch
    case = SC.case_a()
    t = torch.from_numpy(case.raw).to("cuda")
    _, C_, I, _ = case.raw.shape
    table = summary_device(t.data_ptr(), case.probs_list, C_, I, case.first_iter, case.probs)
    want = np.load(os.path.join(GOLDEN, "summary_case_a.npy"))
    assert table.shape == want.shape
    assert _bits(table).tobytes() == _bits(want).tobytes()


def test_curves_table_is_unchanged(cases):
    """The curves' raw-row load, moments, select and row forming moved into the shared layer:
    the device table of case b, in one pass, is the bytes recorded before the move
    (tests/golden/record_posterior.py)."""
    table = _device_table(cases["b"])
    want = np.load(os.path.join(GOLDEN, "curves_case_b.npy"))
    assert table.shape == want.shape
    assert _bits(table).tobytes() == _bits(want).tobytes()


# ---- real runs ----------------------------------------------------------------------------------
def _prob(prior, N, Nn, seed=3):
    t0, S0 = default_prior()
    d = synth_decay(N, "sincExp", seed)
    return ExpGPProblem(d["x"], d["y"], d["uy"], Nn=Nn, gridType="extremal", theta0=t0,
                        Sigma0=S0, prior_type=prior)


def _run_case(prob, draws, first_iter, probs=CC.DEFAULT_PROBS):
    return CC.Case("run", [prob], np.ascontiguousarray(draws)[None], first_iter=first_iter,
                   probs=probs)


def _table_of(rows, probs=CC.DEFAULT_PROBS):
    """A curves dict back as one block [nq, N, 2 + len(probs)]."""
    keys = ["mean", "sd"] + [f"{100 * p:g}%" for p in probs]
    return np.stack([np.stack([rows[n][k] for k in keys], axis=1)
                     for n in CC.CURVE_NAMES if n in rows])


@pytest.fixture(scope="module")
def horseshoe():
    return _prob("horseshoe", 97, 8), SamplerConfig(chains=8, warmup=50, samples=60, seed=21)


@pytest.mark.parametrize("save_warmup", [True, False])
def test_plan_curves_and_pick(horseshoe, save_warmup):
    prob, cfg = horseshoe
    idx = [0, 59, 479]
    with Plan(prob, dataclasses.replace(cfg, save_warmup=save_warmup)) as pl:
        pl.run()
        got = pl.curves()
        picked = pl.curves_pick(draws=idx)
        out = pl.download()
    first = 50 if save_warmup else 0
    assert out.warmup_saved == first
    assert list(got) == ["dL", "m", "resid", "x"] and np.array_equal(got["x"], prob.x)
    case = _run_case(prob, out.draws, first)
    host = curves_host(out.draws, prob, first)
    CC.check_blocks(case, [_table_of(got)], CC.blocks(case, host), f"plan save_warmup={save_warmup}")
    # the picked draws: genquant.expgp_curves on the downloaded rows, within the bound per value
    theta, ygp = CC.pooled_params(case, 0)
    assert np.array_equal(picked["index"], idx)
    assert picked["theta"].tobytes() == np.ascontiguousarray(theta[idx]).tobytes()
    assert picked["yGP"].tobytes() == np.ascontiguousarray(ygp[idx]).tobytes()
    want = expgp_curves(prob, theta[idx], ygp[idx])
    vb = CC.value_bounds(prob, theta[idx], ygp[idx], want)
    for name in CC.CURVE_NAMES:
        assert picked[name].shape == (3, 97)
        ratio = np.max(np.abs(picked[name] - want[name]) / (8 * vb[name]))
        print(f"pick {name}: largest difference / bound = {ratio:.3g}")
        assert ratio <= 1.0, (name, ratio)
    stored = out.draws[:, first:, -1].reshape(-1)[idx]   # the sampler's own br column
    assert np.all(np.abs(picked["br"] - stored) <= 10 * 1e-11 * (1 + np.abs(stored))), \
        (picked["br"], stored)


def test_plan_curves_in_a_callers_buffer(horseshoe):
    """The run writes into the caller's d_draws; the bands read it there, and the direct entry
    on that buffer gives the same bytes."""
    import torch
    prob, cfg = horseshoe
    with Plan(prob, cfg) as pl:
        buf = torch.full((pl.info["draws_bytes"] // 8,), float("nan"), dtype=torch.float64,
                         device="cuda")
        pl.run(d_draws=buf.data_ptr())
        got = pl.curves(what=("m", "resid"), probs=(0.1, 0.9))
        direct = curves_device(buf.data_ptr(), prob, 8, pl.info["iters_saved"], first_iter=50,
                               probs=(0.1, 0.9), what=("m", "resid"))
        out = pl.download()
    assert list(got) == ["m", "resid", "x"] and list(got["m"]) == ["mean", "sd", "10%", "90%"]
    block = curves_blocks(direct, [prob], ("m", "resid"), (0.1, 0.9))[0]
    assert _bits(_table_of(got, (0.1, 0.9))).tobytes() == _bits(block).tobytes()
    case = dataclasses.replace(_run_case(prob, out.draws, 50, (0.1, 0.9)), what=("m", "resid"))
    host = curves_host(out.draws, prob, 50, (0.1, 0.9), ("m", "resid"))
    CC.check_blocks(case, [block], CC.blocks(case, host), "caller's buffer")


def test_batch_curves_equal_single_plans():
    """3 files x 4 chains, N = 481: each file's block is a single plan's of that file (the
    batch's draws are that plan's, bit for bit), and problem= selects the block."""
    probs = [_prob("normal", 481, 10, seed=s) for s in (3, 4, 5)]
    cfg = SamplerConfig(chains=4, warmup=30, samples=30, seed=8)
    with Batch(probs, cfg) as b:
        b.run()
        got = b.curves()
        one = b.curves(problem=1)
        pick = b.curves_pick(2, draws=[5, 100])
    assert len(got) == 3
    assert _bits(_table_of(one)).tobytes() == _bits(_table_of(got[1])).tobytes()
    for p in range(3):
        with Plan(probs[p], dataclasses.replace(cfg, chain_offset=4 * p)) as pl:
            pl.run()
            single = pl.curves()
            if p == 2:
                spick = pl.curves_pick(draws=[5, 100])
        assert _bits(_table_of(single)).tobytes() == _bits(_table_of(got[p])).tobytes(), p
    for k in ("dL", "m", "resid", "br", "theta", "yGP"):
        assert pick[k].tobytes() == spick[k].tobytes(), k


# ---- refusals (each before any kernel is launched) ----------------------------------------------
def test_refusals(horseshoe):
    prob, cfg = horseshoe
    with Plan(prob, cfg) as pl:
        for call in (pl.curves, lambda: pl.curves_pick(draws=[0])):
            with pytest.raises(_lib.FitOCTError) as ei:   # before any run
                call()
            assert ei.value.code == -1 and "not run" in str(ei.value)
        pl.launch()
        with pytest.raises(_lib.FitOCTError) as ei:       # a launch is in flight
            pl.curves()
        assert ei.value.code == -1 and "fitoct_plan_wait" in str(ei.value)
        pl.wait()
        assert "dL" in pl.curves(what="dL")
        with pytest.raises(_lib.FitOCTError) as ei:       # S = 8 x 60
            pl.curves_pick(draws=[480])
        assert ei.value.code == -1 and "pick[0]" in str(ei.value)
    raw = np.zeros((2, 10, prob.D + 8))
    with pytest.raises(_lib.FitOCTError) as ei:           # a host pointer as d_draws
        curves_device(raw.ctypes.data, prob, 2, 10)
    assert ei.value.code == -1 and "device buffer" in str(ei.value)
    with Plan(prob, dataclasses.replace(cfg, devices=(0, 0))) as pl:
        pl.run()                                          # shards stay in per-device buffers
        with pytest.raises(_lib.FitOCTError) as ei:
            pl.curves()
        assert ei.value.code == -1 and "d_draws" in str(ei.value)
    with Batch([prob, prob], dataclasses.replace(cfg, chains=2)) as b:
        with pytest.raises(_lib.FitOCTError) as ei:
            b.curves()
        assert ei.value.code == -1
