"""The posterior summary on the device (fitoct_summary_device, Plan.summary, Batch.summary):
against the host route on the synthetic cases of summary_cases.py, against the parent's route
(download, materialise, StanFit.summary) on real runs through every buffer a run can leave its
draws in, and the refusals that come before any kernel is launched.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import summary_cases as SC
from fitoct_amd import _lib
from fitoct_amd.api import (Batch, ExpGPProblem, Plan, SamplerConfig, summary_device,
                            summary_host)
from fitoct_amd.stanfit import StanFit, output_columns
from fitoct_amd.synth import default_prior, synth_decay

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return {k: f() for k, f in SC.CASES.items()}


def _device_table(case, **kw):
    import torch
    t = torch.from_numpy(case.raw).to("cuda")
    _, C_, I, _ = case.raw.shape
    return summary_device(t.data_ptr(), case.probs_list, C_, I, case.first_iter, case.probs, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_device_matches_host(cases, name):
    case = cases[name]
    host = summary_host(case.raw, case.probs_list, case.first_iter, case.probs)
    dev = _device_table(case)
    assert dev.shape == host.shape
    np_ = len(case.probs)
    # the NaN / constant pattern is identical, all-NaN rows included
    assert np.array_equal(np.isnan(dev), np.isnan(host)), name
    for g, prob in enumerate(case.probs_list):
        names = output_columns(prob)
        fit, _ = SC.stanfit_rows(case, g)
        for j, col in enumerate(names):
            if np.all(np.isnan(host[g, j])):
                continue
            # quantiles: exact order statistics on both routes -> the same bits
            assert np.array_equal(_bits(dev[g, j, 3:3 + np_]), _bits(host[g, j, 3:3 + np_])), \
                (name, g, col, dev[g, j], host[g, j])
            SC.check_row(dev[g, j], host[g, j], SC.column(fit, col).reshape(-1), case.probs,
                         (name, g, col))
    again = _device_table(case)
    assert _bits(again).tobytes() == _bits(dev).tobytes()   # reproducible bit for bit


def test_column_passes_do_not_change_a_bit(cases):
    """Case f: case a with a staging cap of 15 of its 40 columns (three passes)."""
    case = cases["a"]
    one = _device_table(case)
    G, C_, I, _ = case.raw.shape
    col_bytes = G * C_ * (I - case.first_iter) * 8
    assert one.shape[1] == 40
    three = _device_table(case, max_staging_bytes=15 * col_bytes)
    assert _bits(three).tobytes() == _bits(one).tobytes()
    each = _device_table(case, max_staging_bytes=1)   # never less than one column per pass
    assert _bits(each).tobytes() == _bits(one).tobytes()


# ---- real runs ----------------------------------------------------------------------------------
def _prob(prior, N, Nn, seed=3):
    t0, S0 = default_prior()
    d = synth_decay(N, "sincExp", seed)
    return ExpGPProblem(d["x"], d["y"], d["uy"], Nn=Nn, gridType="extremal", theta0=t0,
                        Sigma0=S0, prior_type=prior)


def _same_as_stanfit(got, out, prob, probs=SC.DEFAULT_PROBS):
    fit = StanFit.from_output(out, prob)
    want = fit.summary(probs=probs)
    assert list(got) == list(want)
    for name in want:
        SC.check_row(SC.stanfit_row_values(got[name], probs),
                     SC.stanfit_row_values(want[name], probs),
                     SC.column(fit, name).reshape(-1), probs, name)


def _same_dict(a, b):
    """Two summary dicts hold the same numbers bit for bit (NaN entries included)."""
    assert list(a) == list(b)
    for name in a:
        assert list(a[name]) == list(b[name])
        va, vb = np.array(list(a[name].values())), np.array(list(b[name].values()))
        assert _bits(va).tobytes() == _bits(vb).tobytes(), (name, a[name], b[name])


@pytest.fixture(scope="module")
def lasso():
    return _prob("lasso", 64, 5), SamplerConfig(chains=8, warmup=60, samples=80, seed=21)


@pytest.mark.parametrize("save_warmup", [True, False])
def test_plan_summary_equals_downloaded_summary(lasso, save_warmup):
    prob, cfg = lasso
    with Plan(prob, dataclasses.replace(cfg, save_warmup=save_warmup)) as pl:
        pl.run()
        got = pl.summary()
        out = pl.download()
        some = pl.summary(pars=["theta", "lambda"], probs=(0.1, 0.9))
    assert out.warmup_saved == (60 if save_warmup else 0)
    _same_as_stanfit(got, out, prob)
    assert np.isnan(got["lambda"]["Rhat"]) and got["lambda"]["sd"] == 0.0
    assert list(some) == ["theta.1", "theta.2", "theta.3", "lambda"]
    assert list(some["theta.1"]) == ["mean", "se_mean", "sd", "10%", "90%", "n_eff", "Rhat"]
    assert some["theta.1"]["mean"] == got["theta.1"]["mean"]


@pytest.mark.parametrize("devices", [(), (0, 0)])
def test_plan_summary_in_a_callers_buffer(lasso, devices):
    """The run writes (a device list: gathers) into the caller's d_draws; the summary reads it
    there."""
    import torch
    prob, cfg = lasso
    with Plan(prob, dataclasses.replace(cfg, devices=devices)) as pl:
        buf = torch.full((pl.info["draws_bytes"] // 8,), float("nan"), dtype=torch.float64,
                         device="cuda")
        pl.run(d_draws=buf.data_ptr())
        got = pl.summary()
        out = pl.download()
        direct = summary_device(buf.data_ptr(), prob, 8, pl.info["iters_saved"], first_iter=60)
    _same_as_stanfit(got, out, prob)
    from fitoct_amd.api import summary_rows
    _same_dict(summary_rows(direct[0], prob), got)


@pytest.mark.parametrize("devices", [(), (0, 0)])
def test_batch_summary_equals_per_file_summaries(devices):
    """One device: the batch's own buffer.  A device list (files 2 + 1): the caller's buffer the
    sub-batches gather into; without one the files stay apart and the summary is refused."""
    import torch
    probs = [_prob("normal", 48, 5, seed=s) for s in (3, 4, 5)]
    cfg = SamplerConfig(chains=4, warmup=40, samples=40, seed=8, devices=devices)
    with Batch(probs, cfg) as b:
        b.run()
        if devices:
            with pytest.raises(_lib.FitOCTError) as ei:
                b.summary()
            assert ei.value.code == -1 and "d_draws" in str(ei.value)
            buf = torch.full((b.info["draws_bytes"] // 8,), float("nan"), dtype=torch.float64,
                             device="cuda")
            b.run(d_draws=buf.data_ptr())
        got = b.summary()
        one = b.summary(problem=1, pars="yGP")
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
            pl.summary()
        assert ei.value.code == -1 and "not run" in str(ei.value)
        pl.launch()
        with pytest.raises(_lib.FitOCTError) as ei:   # a launch is in flight
            pl.summary()
        assert ei.value.code == -1 and "fitoct_plan_wait" in str(ei.value)
        pl.wait()
        assert "theta.1" in pl.summary()
    raw = np.zeros((2, 10, prob.D + 8))
    with pytest.raises(_lib.FitOCTError) as ei:       # a host pointer as d_draws
        summary_device(raw.ctypes.data, prob, 2, 10)
    assert ei.value.code == -1 and "device buffer" in str(ei.value)
    with Plan(prob, dataclasses.replace(cfg, devices=(0, 0))) as pl:
        pl.run()                                      # shards stay in per-device buffers
        with pytest.raises(_lib.FitOCTError) as ei:
            pl.summary()
        assert ei.value.code == -1 and "d_draws" in str(ei.value)
    with Batch([prob, prob], dataclasses.replace(cfg, chains=2)) as b:
        with pytest.raises(_lib.FitOCTError) as ei:
            b.summary()
        assert ei.value.code == -1
