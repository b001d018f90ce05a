"""The planner's environment switches for the GPU tests that compare sampler variants
(plain, speculative, two-ended, paired, migrating) bit for bit: one way to run "the planner's
defaults but for ...", and the equalities such a comparison asserts.  A plain module, used by
test_gpu_spec / _migration / _pair / _replay."""
from __future__ import annotations

import contextlib
import os

import numpy as np

from fitoct_amd import Plan

# every name Switches::from_env reads (csrc/schedule.cpp; test_schedule.py holds the two equal)
SWITCHES = ("FITOCT_NO_GEO", "FITOCT_NO_PAIR", "FITOCT_PAIR", "FITOCT_NO_MIGRATE",
            "FITOCT_NO_SPEC", "FITOCT_NO_BIDI", "FITOCT_NO_TAIL_BIDI", "FITOCT_SPEC",
            "FITOCT_SPEC_LIVE", "FITOCT_TAIL_LEFT", "FITOCT_TEST_TAIL_IDLE_US",
            "FITOCT_TEST_PAIR_ABSENT")


@contextlib.contextmanager
def switches(**env):
    """The planner's defaults (no switch set) but for ``env``; a value of None leaves its
    switch unset.  The caller's environment is back on exit, after an exception too."""
    unknown = set(env) - set(SWITCHES)
    assert not unknown, f"not a planner switch: {sorted(unknown)}"
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update({k: v for k, v in env.items() if v is not None})
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def plan_run(prob, cfg, **env):
    """(plan info, downloaded result) of one run of ``prob`` under ``switches(**env)``."""
    with switches(**env), Plan(prob, cfg) as pl:
        pl.run()
        return pl.info, pl.download()


def assert_same_run(a, b):
    """Two runs of the same chains, bit for bit: draws, step sizes, inverse metrics, last
    positions, total leapfrogs."""
    np.testing.assert_array_equal(a.draws, b.draws)
    np.testing.assert_array_equal(a.stepsize, b.stepsize)
    np.testing.assert_array_equal(a.inv_metric, b.inv_metric)
    np.testing.assert_array_equal(a.last_q, b.last_q)
    assert a.total_leapfrogs == b.total_leapfrogs
