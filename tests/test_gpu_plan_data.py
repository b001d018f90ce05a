"""The device plan is the host data plan: what ``fitoct_plan_get_info`` reports of a plan that
was created (not run) equals the answer of the pure host function (test_plan_data.py), and a
batch runs the layout the host function returns for it.

The batch case: problems of N = 300 and N = 2048 plan to one kernel at 8 factorised bins per
lane.  The N = 2048 problem plans to that layout on its own, so its draws in the batch equal,
as 64-bit patterns, a single plan with chain_offset 2.  The N = 300 problem reaches that layout
only inside a batch (alone it keeps its basis rows; no entry of the C ABI forces a layout on a
single plan), so its draws are compared, bit for bit, with the same problem's in a second batch
whose other file differs: a file's draws depend on its own layout and chain keys only."""
from __future__ import annotations

import numpy as np
import pytest

from fitoct_amd import Batch, Plan, SamplerConfig
from planner_env import assert_same_run, switches
from test_plan_data import PLANS, POLY, batch_layout, plan_data, prob

pytestmark = pytest.mark.gpu

ROWS_ON_DEVICE = ("test_gpu_replay config2 N=256", "test_gpu_batch N=513 factorised",
                  "test_gpu_replay headline N=2048 horseshoe", "test_gpu_sampler config4 N=4096",
                  "test_gpu_sampler config4 N=4096 off the grid", "N=5000 padded to the lanes")


@pytest.mark.parametrize("name", ROWS_ON_DEVICE)
def test_plan_info_is_the_host_plan(name):
    _, make, args, want = next(t for t in PLANS if t[0] == name)
    assert not args
    p = make()
    host = plan_data(p)
    assert host["rc"] == 0 and {k: host[k] for k in want} == want
    with switches(), Plan(p, SamplerConfig(chains=2, warmup=5, samples=5, max_treedepth=4)) as pl:
        info = pl.info
    assert (info["basis_mode"], info["bins_per_thread"], info["n_pad"], info["dim"]) == \
        (host["mode"], host["bpt"], host["n_pad"], host["D"])


def test_batch_runs_the_host_layout_bitwise():
    cfg = SamplerConfig(chains=2, warmup=5, samples=5, seed=11, max_treedepth=4)
    small, wide, other = prob(300), prob(2048), prob(2048, kind="sincExp2", seed=8)
    host = batch_layout([small, wide])
    assert host == dict(rc=0, bpt=8, plans=[[POLY, 8, 2048]] * 2)
    alone = plan_data(wide)
    assert (alone["mode"], alone["bpt"], alone["n_pad"]) == (POLY, 8, 2048)

    def run(probs):
        with switches(), Batch(probs, cfg) as b:
            info = b.info
            b.run()
            return info, [b.download(p) for p in range(len(probs))]

    info, outs = run([small, wide])
    assert (info["basis_mode"], info["bins_per_thread"], info["n_pad"]) == (POLY, 8, 2048)
    assert [o.chain_offset for o in outs] == [0, 2]
    with switches(), Plan(wide, SamplerConfig(**{**cfg.__dict__, "chain_offset": 2})) as pl:
        assert (pl.info["basis_mode"], pl.info["bins_per_thread"]) == (POLY, 8)
        pl.run()
        single = pl.download()
    assert_same_run(outs[1], single)
    assert outs[1].draws.view(np.uint64).tobytes() == single.draws.view(np.uint64).tobytes()
    _, outs2 = run([small, other])
    assert_same_run(outs[0], outs2[0])
    assert outs[0].draws.view(np.uint64).tobytes() == outs2[0].draws.view(np.uint64).tobytes()
    assert not np.array_equal(outs[1].draws, outs2[1].draws)

