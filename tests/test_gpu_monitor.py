"""The rank diagnostics on the device (fitoct_monitor_device, Plan.monitor, Batch.monitor):
against the host route on the cases of monitor_cases.py (one-workgroup and multi-workgroup
sorts, heavy ties, NaN rows, many small segments), bit for bit across calls and column passes,
against the host route and ``rank_rhat`` of the downloaded draws on real runs through every
buffer a run can leave its draws in, and the refusals that come before any kernel is launched.
"""
from __future__ import annotations

import dataclasses
import os

import numpy as np
import pytest

import monitor_cases as MC
import summary_cases as SC
from fitoct_amd import _lib
from fitoct_amd.api import (Batch, ExpGPProblem, Plan, SamplerConfig, monitor_device,
                            monitor_host, monitor_rows)
from fitoct_amd.stanfit import StanFit, output_columns, rank_rhat
from fitoct_amd.synth import default_prior, synth_decay

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

@pytest.fixture(scope="module")
def cases():
    return {k: f() for k, f in MC.CASES.items()}


def _device_table(case, **kw):
    import torch
    t = torch.from_numpy(case.raw).to("cuda")
    _, C_, I, _ = case.raw.shape
    return monitor_device(t.data_ptr(), case.probs_list, C_, I, case.first_iter, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", list(MC.CASES))
def test_device_matches_host(cases, name):
    case = cases[name]
    host = monitor_host(case.raw, case.probs_list, case.first_iter)
    dev = _device_table(case)
    assert dev.shape == host.shape
    assert np.array_equal(np.isnan(dev), np.isnan(host)), name   # NaN rows and NaN Tail_ESS
    for g, prob in enumerate(case.probs_list):
        for j, col in enumerate(output_columns(prob)):
            MC.check_row(dev[g, j], host[g, j], (name, g, col),
                         ess=(g, col) not in MC.ESS_LEFT_OUT.get(name, []))
    again = _device_table(case)
    assert _bits(again).tobytes() == _bits(dev).tobytes()   # reproducible bit for bit
    if name == "b":
        names = output_columns(case.probs_list[0])
        assert dev[0, names.index("theta.1"), 0] > 1.1      # the shifted chain


@pytest.mark.parametrize("name", ["a", "i"])
def test_column_passes_do_not_change_a_bit(cases, name):
    """A staging cap of a third of the columns (three passes) and of less than one column (one
    column per pass), in both sort regimes."""
    case = cases[name]
    one = _device_table(case)
    G, C_, I, _ = case.raw.shape
    col_bytes = MC.STAGING_BUFFERS * G * C_ * (I - case.first_iter) * 8
    P = one.shape[1]
    third = -(-P // 3)
    assert 2 * third < P <= 3 * third
    three = _device_table(case, max_staging_bytes=third * col_bytes)
    assert _bits(three).tobytes() == _bits(one).tobytes()
    each = _device_table(case, max_staging_bytes=1)   # never less than one column per pass
    assert _bits(each).tobytes() == _bits(one).tobytes()


@pytest.mark.parametrize("name", ["a", "i"])
def test_monitor_table_is_unchanged(cases, name):
    """The staging, moments and autocovariance kernels moved into the shared layer's one
    translation unit: the device table, in both sort regimes, is the bytes recorded before the
    move (tests/golden/record_posterior.py)."""
    table = _device_table(cases[name])
    want = np.load(os.path.join(GOLDEN, f"monitor_case_{name}.npy"))
    assert table.shape == want.shape
    assert _bits(table).tobytes() == _bits(want).tobytes()


# ---- real runs ----------------------------------------------------------------------------------
def _prob(prior, N, Nn, seed=3):
    t0, S0 = default_prior()
    d = synth_decay(N, "sincExp", seed)
    return ExpGPProblem(d["x"], d["y"], d["uy"], Nn=Nn, gridType="extremal", theta0=t0,
                        Sigma0=S0, prior_type=prior)


def _same_as_stanfit(got, out, prob):
    """A device dict against the host route on the downloaded draws (R-hats 1e-10, ESS 1e-8,
    the same rows), and its Rhat against stanfit.rank_rhat of each column."""
    fit = StanFit.from_output(out, prob)
    want = fit.monitor()
    assert list(got) == list(want)
    for name in want:
        MC.check_row(np.array(list(got[name].values())), np.array(list(want[name].values())), name)
        r = rank_rhat(SC.column(fit, name))
        assert abs(got[name]["Rhat"] - r) <= 1e-10 * abs(r), (name, got[name]["Rhat"], r)


def _same_dict(a, b):
    assert list(a) == list(b)
    for name in a:
        va, vb = np.array(list(a[name].values())), np.array(list(b[name].values()))
        assert _bits(va).tobytes() == _bits(vb).tobytes(), (name, a[name], b[name])


@pytest.fixture(scope="module")
def lasso():
    return _prob("lasso", 64, 5), SamplerConfig(chains=8, warmup=60, samples=80, seed=21)


@pytest.mark.parametrize("save_warmup", [True, False])
def test_plan_monitor_equals_downloaded_monitor(lasso, save_warmup):
    prob, cfg = lasso
    with Plan(prob, dataclasses.replace(cfg, save_warmup=save_warmup)) as pl:
        pl.run()
        got = pl.monitor()
        out = pl.download()
        some = pl.monitor(pars=["theta", "lp__"])
    assert out.warmup_saved == (60 if save_warmup else 0)
    _same_as_stanfit(got, out, prob)
    assert "lambda" not in got and "stepsize__" not in got   # constant in every chain: NaN rows
    assert list(some) == ["theta.1", "theta.2", "theta.3", "lp__"]
    assert list(some["lp__"]) == list(MC.KEYS)
    assert some["theta.1"] == got["theta.1"]


@pytest.mark.parametrize("devices", [(), (0, 0)])
def test_plan_monitor_in_a_callers_buffer(lasso, devices):
    """The run writes (a device list: gathers) into the caller's d_draws; the diagnostics read
    it there."""
    import torch
    prob, cfg = lasso
    with Plan(prob, dataclasses.replace(cfg, devices=devices)) as pl:
        buf = torch.full((pl.info["draws_bytes"] // 8,), float("nan"), dtype=torch.float64,
                         device="cuda")
        pl.run(d_draws=buf.data_ptr())
        got = pl.monitor()
        out = pl.download()
        direct = monitor_device(buf.data_ptr(), prob, 8, pl.info["iters_saved"], first_iter=60)
    _same_as_stanfit(got, out, prob)
    _same_dict(monitor_rows(direct[0], prob), got)


def test_batch_monitor_equals_per_file_monitors():
    probs = [_prob("normal", 48, 5, seed=s) for s in (3, 4, 5)]
    cfg = SamplerConfig(chains=4, warmup=40, samples=40, seed=8)
    with Batch(probs, cfg) as b:
        b.run()
        got = b.monitor()
        one = b.monitor(problem=1, pars="yGP")
        outs = [b.download(p) for p in range(3)]
    assert len(got) == 3
    for p in range(3):
        _same_as_stanfit(got[p], outs[p], probs[p])
    assert list(one) == [f"yGP.{k}" for k in range(1, 6)]
    _same_dict({"yGP.2": one["yGP.2"]}, {"yGP.2": got[1]["yGP.2"]})


# ---- refusals (each before any kernel is launched) ----------------------------------------------
def test_refusals(lasso):
    prob, cfg = lasso
    with Plan(prob, cfg) as pl:
        with pytest.raises(_lib.FitOCTError) as ei:   # before any run
            pl.monitor()
        assert ei.value.code == -1 and "not run" in str(ei.value)
        pl.launch()
        with pytest.raises(_lib.FitOCTError) as ei:   # a launch is in flight
            pl.monitor()
        assert ei.value.code == -1 and "fitoct_plan_wait" in str(ei.value)
        pl.wait()
        assert "theta.1" in pl.monitor()
    raw = np.zeros((2, 10, prob.D + 8))
    with pytest.raises(_lib.FitOCTError) as ei:       # a host pointer as d_draws
        monitor_device(raw.ctypes.data, prob, 2, 10)
    assert ei.value.code == -1 and "device buffer" in str(ei.value)
    with Plan(prob, dataclasses.replace(cfg, devices=(0, 0))) as pl:
        pl.run()                                      # shards stay in per-device buffers
        with pytest.raises(_lib.FitOCTError) as ei:
            pl.monitor()
        assert ei.value.code == -1 and "d_draws" in str(ei.value)
    with Batch([prob, prob], dataclasses.replace(cfg, chains=2)) as b:
        with pytest.raises(_lib.FitOCTError) as ei:
            b.monitor()
        assert ei.value.code == -1
