"""Chain migration between tiles (work balance, chain.h try_donate / tile_migrate.h
receive_chain): a chain handed to another tile at a transition boundary must
produce exactly the draws it produces without migration (same arithmetic in
every tile, Philox addressed by global chain id and iteration), and the
hand-over must actually happen when tiles finish unevenly."""
from __future__ import annotations

import numpy as np
import pytest

from fitoct_amd import SamplerConfig
from planner_env import assert_same_run, plan_run
from test_gpu_sampler import _prob

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family,N", [("horseshoe", 512), ("normal", 2048), ("lasso", 1024)])
def test_migration_preserves_draws_bitwise(family, N):
    prob = _prob(family, N, 15)
    cfg = SamplerConfig(chains=1024, warmup=100, samples=100, seed=21, max_treedepth=7)
    info, a = plan_run(prob, cfg)
    _, b = plan_run(prob, cfg, FITOCT_NO_MIGRATE="1")
    assert info["chains_per_tile"] == 4
    assert b.migrations == 0
    assert a.migrations > 0, "no chain was handed over"
    assert_same_run(a, b)


@pytest.mark.parametrize("family,N,left", [("horseshoe", 2048, None),
                                           ("normal", 512, None),
                                           ("lasso", 1024, "256"),
                                           ("normal", 512, "512")])
def test_tail_two_ended_preserves_draws_bitwise(family, N, left):
    """The launch's tail (tile_migrate.h receive_chain, P.tail_bidi): once at most
    tail_left chains are unfinished (default: every chain of the launch; 256: one per
    tile), a chain alone in its migrating tile recruits two idle receivers of the tile as
    producers and grows both trajectory ends at once, booking the leaves itself.  Draws,
    step sizes, metrics, last positions and leapfrog counts equal those of the same launch
    without it (FITOCT_NO_TAIL_BIDI=1) and without migration at all, and the run reports
    two-ended transitions."""
    prob = _prob(family, N, 15)
    cfg = SamplerConfig(chains=1024, warmup=100, samples=100, seed=23, max_treedepth=8)
    info, a = plan_run(prob, cfg, FITOCT_TAIL_LEFT=left)
    _, b = plan_run(prob, cfg, FITOCT_NO_TAIL_BIDI="1")
    _, c = plan_run(prob, cfg, FITOCT_NO_MIGRATE="1")
    assert info["chains_per_tile"] == 4 and info["sampler"] == 3
    assert a.two_ended_transitions > 0, "no tail transition was two-ended"
    assert b.two_ended_transitions == 0 and c.two_ended_transitions == 0
    for x in (b, c):
        assert_same_run(a, x)


def test_tail_producer_that_gives_up_leaves_no_lone_chain_waiting():
    """a tail producer idle past its bound (FITOCT_TEST_TAIL_IDLE_US=20: 20 us
    instead of minutes) leaves its role only while it holds the tile's TW_BUSY word, and
    withdraws it (TW_JOIN, its TW_CLAIM bit), so a lone chain never claims a pair with a
    producer missing and then waits for records that no wave will write (ERR_TIMEOUT on a
    healthy chain).  Producers come and go all through the tail here: every chain finishes,
    with the draws of the launch without two-ended tails."""
    prob = _prob("horseshoe", 512, 15)
    cfg = SamplerConfig(chains=1024, warmup=100, samples=100, seed=29, max_treedepth=8)
    info, a = plan_run(prob, cfg, FITOCT_TEST_TAIL_IDLE_US="20")
    _, b = plan_run(prob, cfg, FITOCT_NO_TAIL_BIDI="1")
    assert info["two_ended"] == 2
    np.testing.assert_array_equal(a.draws, b.draws)
    np.testing.assert_array_equal(a.stepsize, b.stepsize)
    assert a.total_leapfrogs == b.total_leapfrogs
