"""Every stored transition and adaptation step of the HIP sampler against the C oracle
(tests/replay_audit.py): one small launch per kernel instantiation with save_warmup on
(W = 150: the unit-metric phase, one metric window, the search after it, the term buffer;
S = 60 sampling iterations), then

* every stored row's own consistency (lp__, br, energy__, treedepth__ / n_leapfrog__,
  accept_stat__, stepsize__) -- zero findings;
* the adaptation recurrences (dual averaging, the step-size search after the metric
  update, exp(x_bar), the regularised Welford metric) at 1e-9 -- zero findings;
* the one-step replay: the oracle recomputes each transition t >= 1 of the listed chains
  from the sampler's own row t-1, step size and metric, and all D + 8 columns agree at 1e-6
  -- at most 1 % of the transitions disagree, at most 3 in any chain, and none at t = 1.
  (The oracle alone, replayed from starts moved by 1e-12, stays within 0.2 %:
  test_replay_audit.test_replay_noise_floor, same shapes.)

Unlike the leading-horizon and bitwise path-against-path tests, this sees the deep trees, the
transitions after a metric update, the sampling phase, and any fault the sampler's paths share.
The shapes are tests/replay_cases.py's; the measured figures are in DESIGN.md (parity notes)."""
from __future__ import annotations

import numpy as np
import pytest

import replay_audit as RA
import replay_cases as RC
from fitoct_amd import Batch
from planner_env import plan_run, switches

pytestmark = pytest.mark.gpu

NTHREADS = 16
SPECULATIVE, MIGRATE_SPEC = 2, 3      # FITOCT_SAMPLER_*
POLY, ROWS = 0, 1                     # fitoct_plan_info::basis_mode


def _launch(case, prob, **env):
    cfg = case.cfg()
    info, out = plan_run(prob, cfg, **env)
    return info, cfg, out


def _check(name, prob, cfg, out, chains=None, replay=True):
    a = RA.audit(prob, cfg, out.draws, out.stepsize, out.inv_metric, chains=chains, replay=replay,
                 nthreads=NTHREADS)
    print(f"replay audit {name}: {a.summary()}")
    for f in a.findings[:20]:
        print("   ", f)
    assert not a.named("row", "adapt"), a.named("row", "adapt")[:8]
    if not replay:
        assert a.replayed == 0
        return a
    n = len(out.draws) if chains is None else len(chains)
    assert a.replayed == n * (out.draws.shape[1] - 1)
    assert a.replay_share <= 0.01, a.summary()
    assert a.replay_max_per_chain <= 3, a.summary()
    assert not [f for f in a.replay_findings if f.t == 1]
    return a


@pytest.mark.parametrize("pair", [False, True], ids=["unpaired", "paired"])
def test_config2_row_tiles_of_one_chain(pair):
    """Config-2 shape: basis rows resident in the gradient waves, two-ended one-chain tiles,
    unpaired by default and paired with FITOCT_PAIR=1; trees to depth 10."""
    case = RC.REPLAY["config2"]
    prob = case.make()
    info, cfg, out = _launch(case, prob, **({"FITOCT_PAIR": "1"} if pair else {}))
    assert info["chains_per_tile"] == 1 and info["sampler"] == SPECULATIVE
    assert info["two_ended"] == 1 and info["basis_mode"] == ROWS and info["bins_per_thread"] == 2
    assert info["paired"] == int(pair)
    assert out.two_ended_transitions > 0 and (out.paired_transitions > 0) == pair
    _check("config2" + ("/paired" if pair else ""), prob, cfg, out)


def test_headline_migrating_tiles_of_four_chains():
    """The headline kernel: 1024 chains in migrating tiles of four (horseshoe lane roles from
    LDS, tail speculation, two-ended tails).  Every row and adaptation step of all 1024
    chains; the replay of 48 of them: the first 16, 16 spread evenly, the last 16."""
    case = RC.REPLAY["headline"]
    prob = case.make()
    info, cfg, out = _launch(case, prob)
    assert info["chains_per_tile"] == 4 and info["sampler"] == MIGRATE_SPEC
    assert info["basis_mode"] == POLY and info["bins_per_thread"] == 8 and info["two_ended"] == 2
    assert out.migrations > 0
    _check("headline", prob, cfg, out, chains=case.replayed())


def test_batch_of_files():
    """Config-5 shape: 6 files x 4 chains in one Batch launch, every chain of every file
    (file p's chains are global chains 4 p .. 4 p + 3)."""
    case = RC.REPLAY["batch"]
    probs = case.make()
    cfg = case.cfg()
    with switches(), Batch(probs, cfg) as b:
        b.run()
        info, outs = b.info, [b.download(p) for p in range(len(probs))]
    assert info["chains_per_tile"] == 1 and info["sampler"] == SPECULATIVE
    assert info["basis_mode"] == ROWS and info["two_ended"] == 1
    for p, (prob, out) in enumerate(zip(probs, outs)):
        assert out.cfg.chain_offset == p * case.chains
        _check(f"batch/file{p}", prob, out.cfg, out)


def test_factorised_basis_one_chain_tiles():
    case = RC.REPLAY["poly_one_chain"]
    prob = case.make()
    info, cfg, out = _launch(case, prob)
    assert info["chains_per_tile"] == 1 and info["sampler"] == SPECULATIVE
    assert info["basis_mode"] == POLY and info["two_ended"] == 1 and info["bins_per_thread"] == 4
    _check("poly_one_chain", prob, cfg, out)


@pytest.mark.parametrize("name", ["ppl2_normal", "ppl2_horseshoe"])
def test_two_parameters_per_lane(name):
    """Nn = 20 and the maximum Nn = 24 (D = 78 > 64 lanes): the (24, 2) instantiation."""
    case = RC.REPLAY[name]
    prob = case.make()
    info, cfg, out = _launch(case, prob)
    assert prob.Nn > 15 and info["chains_per_tile"] == 1 and info["sampler"] == SPECULATIVE
    assert info["basis_mode"] == POLY and info["two_ended"] == 1
    _check(name, prob, cfg, out)


def test_compact_sixteen_bins_per_lane_with_padding():
    case = RC.REPLAY["compact16"]
    prob = case.make()
    info, cfg, out = _launch(case, prob)
    assert info["bins_per_thread"] == 16 and info["n_pad"] == 4096 > prob.N
    assert info["chains_per_tile"] == 1 and info["basis_mode"] == POLY
    _check("compact16", prob, cfg, out)


def test_streamed_bins():
    """N = 8192: more bins than a tile keeps in registers, streamed at every sweep."""
    case = RC.REPLAY["streamed"]
    prob = case.make()
    info, cfg, out = _launch(case, prob)
    assert info["bins_per_thread"] == 0 and info["n_pad"] == 8192
    assert info["chains_per_tile"] == 1 and info["basis_mode"] == POLY
    _check("streamed", prob, cfg, out)


@pytest.mark.parametrize("name", ["amplitude_conv", "prior_pd", "monoexp", "minimum"])
def test_model_switches(name):
    """Model options the sampler kernel had only run statistically or not at all: dataType 1
    with the RMgauss kernel and rate conventions on the internal grid (Nn = 20), the prior
    predictive (prior_PD: br = NaN), the mono-exponential model, and the
    minimum shape N = 2, Nn = 2."""
    case = RC.REPLAY[name]
    prob = case.make()
    info, cfg, out = _launch(case, prob)
    assert info["chains_per_tile"] == 1 and info["sampler"] == SPECULATIVE
    if name == "prior_pd":
        assert np.isnan(out.draws[:, :, -1]).all()
    _check(name, prob, cfg, out)


@pytest.mark.parametrize("name,bpt", [("user_basis_streamed", 0), ("user_basis_resident", 2)])
def test_caller_supplied_basis(name, bpt):
    """A caller's B (not an SE basis: row mode whatever N): rows streamed at N = 1000,
    resident in the gradient waves at N = 300."""
    case = RC.REPLAY[name]
    prob = case.make()
    info, cfg, out = _launch(case, prob)
    assert info["basis_mode"] == ROWS and info["bins_per_thread"] == bpt
    assert info["chains_per_tile"] == 1 and info["sampler"] == SPECULATIVE
    _check(name, prob, cfg, out)


@pytest.mark.parametrize("name,mode,bpt", [("rho_wide", POLY, 4), ("rho_overflow_rows", ROWS, 0)])
def test_length_scale_other_than_the_default(name, mode, bpt):
    """rho away from 1/Nn (tests/rho_cases.py): rho 0.15 at Nn = 10, the factorised basis with
    the geometric moments; rho 0.03 at Nn = 15, where t^14 would overflow and the sampler
    runs the built-in basis through the streamed-rows fallback."""
    case = RC.REPLAY[name]
    prob = case.make()
    info, cfg, out = _launch(case, prob)
    assert prob.B is None and prob.rho != 1 / prob.Nn
    assert info["basis_mode"] == mode and info["bins_per_thread"] == bpt
    assert info["chains_per_tile"] == 1 and info["sampler"] == SPECULATIVE
    _check(name, prob, cfg, out)


@pytest.mark.parametrize("name", ["mixed_1024", "mixed_300"])
def test_mixed_precision_rows_and_adaptation(name):
    """precision = "mixed" (f32 sweep): the f64 oracle is not the same chain, so no replay;
    each row's lp__ / br within the mixed tolerances of test_gpu_logp.py, the adaptation
    arithmetic (f64 on the device) at 1e-9 from the run's own acceptance statistics."""
    case = RC.NO_REPLAY[name]
    prob = case.make()
    info, cfg, out = _launch(case, prob)
    assert cfg.precision == "mixed" and info["basis_mode"] == ROWS
    assert info["chains_per_tile"] == 1
    _check(name, prob, cfg, out, replay=False)


def test_hard_geometry_rows_and_adaptation():
    """adapt_delta 0.99, max_treedepth 12 on the horseshoe: trees too deep for the replay
    (already at max_treedepth 10 the oracle's own replay from starts moved by 1e-12 reaches
    the noise-floor cap), so rows and adaptation only -- at every tree depth the
    run reaches."""
    case = RC.NO_REPLAY["hard_geometry"]
    prob = case.make()
    info, cfg, out = _launch(case, prob)
    assert info["chains_per_tile"] == 1 and cfg.max_treedepth == 12
    assert out.draws[:, :, 3].max() >= 8
    _check("hard_geometry", prob, cfg, out, replay=False)
