"""The launch schedule (csrc/schedule.cpp) and the stamps report (csrc/stamps_report.cpp)
without a GPU.

``fitoct_internal_schedule`` runs the planner's pure decision -- chains per tile, migration,
speculation, two-ended trajectories, pairing, the grid -- over plain integers and explicit
switches (no environment read).  The expected schedules below are what the GPU tests
(test_gpu_pair / _spec / _migration / _batch) assert through ``fitoct_plan_get_info`` and what
DESIGN.md states for the BASELINE configs, on a 256-CU chip.
"""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fitoct_amd import _lib  # noqa: E402

POLY, ROWS = 0, 1                              # kernel_params.h BasisMode
PLAIN, MIGRATE, SPECULATIVE, MIGRATE_SPEC = 0, 1, 2, 3   # fitoct.h FITOCT_SAMPLER_*
GMAX, NSTAMP, NCU = 4, 108, 256
E_ARG = -1

SWITCHES = ("no_geo", "no_pair", "pair", "no_migrate", "no_spec", "no_bidi", "no_tail_bidi",
            "spec", "spec_live", "tail_left", "test_tail_idle_us", "test_pair_absent")
UNSET = dict.fromkeys(SWITCHES, 0) | {"spec": -1, "spec_live": -1, "tail_left": -1}
OUT = ("G", "tiles", "lds", "migrate", "spec_live", "spec", "bidi", "tail_bidi", "tail_left",
       "tail_idle_ticks", "pair", "grid", "sampler", "batch_pair", "batch_grid")


def schedule(mode, chains, batch_chains=0, ppl=1, depth=10, **switches):
    """(status, schedule as a dict)"""
    f = _lib.lib().fitoct_internal_schedule
    f.restype = C.c_int32
    sw = (C.c_int32 * len(SWITCHES))(*[int((UNSET | switches)[k]) for k in SWITCHES])
    out = (C.c_int64 * len(OUT))()
    rc = f(C.c_int32(ppl), C.c_int32(mode), C.c_int32(chains), C.c_int32(batch_chains),
           C.c_int32(NCU), C.c_int32(depth), sw, out)
    return rc, dict(zip(OUT, out))


CONFIG3 = dict(mode=POLY, chains=1024)     # horseshoe N = 2048, 1024 chains
CONFIG2 = dict(mode=ROWS, chains=128)      # normal N = 512, 128 chains
CONFIG5 = dict(mode=ROWS, chains=4, batch_chains=1024)   # 256 files x 4 chains in one batch
CONFIG5_SHARE = dict(mode=ROWS, chains=4, batch_chains=128)   # its 8-GPU share: 32 files

TABLE = [
    ("config 3", CONFIG3, {},
     dict(G=4, tiles=256, migrate=1, spec_live=3, spec=1, tail_bidi=1, tail_left=1024, bidi=0,
          tail_idle_ticks=0, pair=0, grid=256, sampler=MIGRATE_SPEC)),
    ("config 3 no_spec", CONFIG3, dict(no_spec=1),
     dict(sampler=MIGRATE, migrate=1, spec=0, spec_live=0, tail_bidi=0)),
    ("config 3 no_migrate", CONFIG3, dict(no_migrate=1),
     dict(G=4, migrate=0, spec_live=0, spec=0, tail_bidi=0, sampler=PLAIN)),
    ("config 3 no_migrate spec=1", CONFIG3, dict(no_migrate=1, spec=1),      # test_gpu_spec.py
     dict(G=4, migrate=0, spec_live=GMAX, spec=1, sampler=SPECULATIVE)),
    ("config 3 no_tail_bidi", CONFIG3, dict(no_tail_bidi=1),
     dict(tail_bidi=0, tail_left=0, sampler=MIGRATE_SPEC)),
    ("config 3 spec_live=9 clamps", CONFIG3, dict(spec_live=9), dict(spec_live=GMAX, spec=1)),
    ("config 3 spec_live=0", CONFIG3, dict(spec_live=0), dict(spec=0, sampler=MIGRATE)),
    ("config 3 spec=0 keeps the default", CONFIG3, dict(spec=0), dict(spec_live=3)),
    ("config 3 no_spec beats spec", CONFIG3, dict(spec=1, spec_live=2, no_spec=1),
     dict(spec_live=0, spec=0)),
    ("config 3 idle hook", CONFIG3, dict(test_tail_idle_us=7), dict(tail_idle_ticks=700)),
    ("config 3 tail_left=-5", CONFIG3, dict(tail_left=-5), dict(tail_bidi=1, tail_left=0)),
    ("config 3 tail_left=1", CONFIG3, dict(tail_left=1), dict(tail_bidi=1, tail_left=1)),
    ("config 2", CONFIG2, {},
     dict(G=1, tiles=128, migrate=0, spec=1, spec_live=1, bidi=1, tail_bidi=0, pair=0, grid=128,
          sampler=SPECULATIVE)),
    ("config 2 pair", CONFIG2, dict(pair=1), dict(bidi=1, pair=1, grid=256)),
    ("config 2 no_pair + pair", CONFIG2, dict(no_pair=1, pair=1), dict(pair=0, grid=128)),
    ("config 2 no_bidi", CONFIG2, dict(no_bidi=1),
     dict(bidi=0, spec=1, pair=0, sampler=SPECULATIVE)),
    # test_pairing_default_follows_the_basis_mode
    ("POLY 16 chains", dict(mode=POLY, chains=16), {}, dict(G=1, bidi=1, pair=1, grid=32)),
    ("ROWS 16 chains", dict(mode=ROWS, chains=16), {}, dict(G=1, bidi=1, pair=0, grid=16)),
    ("37 tiles", dict(mode=POLY, chains=37), {}, dict(tiles=37, pair=1, grid=80)),
    # test_pairs_off_where_twice_the_tiles_do_not_fit
    ("200 one-chain tiles", dict(mode=POLY, chains=200), {},
     dict(G=1, tiles=200, bidi=1, pair=0, grid=200)),
    ("128 POLY chains: the last paired count", dict(mode=POLY, chains=128), {},
     dict(pair=1, grid=256)),
    ("129 POLY chains", dict(mode=POLY, chains=129), {}, dict(G=1, bidi=1, pair=0, grid=129)),
    ("257 chains: two per tile, migrating", dict(mode=POLY, chains=257), {},
     dict(G=2, tiles=129, migrate=1, bidi=0, tail_bidi=1, sampler=MIGRATE_SPEC)),
    ("config 5", CONFIG5, {},
     dict(G=4, tiles=1, migrate=0, spec=0, bidi=0, pair=0, sampler=PLAIN, batch_pair=0,
          batch_grid=256)),
    # test_batch_of_one_chain_tiles_pairs_bitwise
    ("config 5 share", CONFIG5_SHARE, {},
     dict(G=1, tiles=4, bidi=1, pair=0, batch_pair=0, batch_grid=128)),
    ("config 5 share pair", CONFIG5_SHARE, dict(pair=1),
     dict(G=1, bidi=1, pair=0, batch_pair=1, batch_grid=256)),
    ("config 5 share no_pair", CONFIG5_SHARE, dict(no_pair=1, pair=1),
     dict(batch_pair=0, batch_grid=128)),
    ("config 5 at 2 GPUs: two chains per tile, deep speculation",
     dict(mode=ROWS, chains=4, batch_chains=512), {},
     dict(G=2, migrate=0, spec=1, spec_live=1, bidi=0, sampler=SPECULATIVE)),
    # test_two_ended_off_where_three_chain_areas_do_not_fit (Nn = 20: two parameters per lane)
    ("ppl 2 depth 10", dict(mode=ROWS, chains=4, ppl=2), {}, dict(G=1, spec=1, bidi=0, pair=0)),
]


@pytest.mark.parametrize("what,shape,switches,want", TABLE, ids=[t[0] for t in TABLE])
def test_schedule_table(what, shape, switches, want):
    rc, s = schedule(**shape, **switches)
    assert rc == 0
    assert {k: s[k] for k in want} == want, (what, s)
    assert s["tiles"] == -(-shape["chains"] // s["G"])
    if not s["pair"]:
        assert s["grid"] == s["tiles"]


def test_planner_env_lists_every_switch_the_planner_reads():
    """The GPU variant tests run "the planner's defaults but for ..." by clearing
    planner_env.SWITCHES: every name Switches::from_env passes to getenv (directly or through
    its ``set`` lambda) must be in it, or a new switch leaks into those comparisons."""
    import planner_env
    with open(os.path.join(ROOT, "fitoct_amd", "csrc", "schedule.cpp")) as f:
        read = re.findall(r'\b(?:getenv|set)\("(\w+)"\)', f.read())
    assert len(read) >= 12 and len(set(read)) == len(read)
    assert set(read) == set(planner_env.SWITCHES)
    assert planner_env.SWITCHES == tuple("FITOCT_" + k.upper() for k in SWITCHES)


def test_two_ended_tiles_carve_three_chain_areas():
    """config 2: lds = lds_bytes(1, 3, 10), the carve of a tile of three chains (768 chains);
    one-ended (no_bidi) it is the one-chain carve, which is smaller."""
    lds3 = schedule(ROWS, 768, no_migrate=1)[1]
    assert lds3["G"] == 3
    two = schedule(**CONFIG2)[1]
    one = schedule(**CONFIG2, no_bidi=1)[1]
    assert two["lds"] == lds3["lds"] <= 160 * 1024 - 1024
    assert 0 < one["lds"] < two["lds"]
    # two parameters per lane at depth 10: three areas do not fit, the tile keeps one
    assert schedule(ROWS, 4, ppl=2)[1]["lds"] <= 160 * 1024 - 1024


def test_depth_beyond_the_lds_budget_is_an_argument_error():
    rc, _ = schedule(POLY, 4, ppl=2, depth=64)
    assert rc == E_ARG
    assert b"max_treedepth too large for the LDS budget" in _lib.lib().fitoct_last_error()
    # chains per tile shrink before the plan gives up: depth 16 still runs, with fewer chains
    rc, s = schedule(POLY, 1024, ppl=2, depth=16)
    assert rc == 0 and 1 <= s["G"] < 4


# the planner inputs behind each row of test_kernel_resources.LAUNCHED, in its order
LAUNCHED_INPUTS = [
    (CONFIG3, {}),
    (CONFIG3, dict(no_spec=1)),
    (dict(mode=POLY, chains=1024), {}),                    # config 4
    (CONFIG2, dict(pair=1)),
    (CONFIG2, {}),
    (CONFIG5, {}),
    (CONFIG5_SHARE, dict(pair=1)),
    (dict(mode=ROWS, chains=4, batch_chains=256), {}),     # the 4-GPU share (8-GPU: 128)
]


def test_launched_table_names_what_the_planner_picks():
    """Every kernel named in test_kernel_resources.LAUNCHED is the instantiation the planner
    picks for that row's shape and switches: <..., MODE, FAM, MIG, SPEC, PAIR>."""
    from test_kernel_resources import LAUNCHED
    assert len(LAUNCHED) == len(LAUNCHED_INPUTS)
    for (what, _fam, kernel, _), (shape, switches) in zip(LAUNCHED, LAUNCHED_INPUTS):
        m = re.search(r"Li(\d+)ELi\d+ELb(\d)ELb(\d)ELb(\d)EEEv", kernel)
        mode, mig, spec, pair = (int(g) for g in m.groups())
        rc, s = schedule(**shape, **switches)
        assert rc == 0 and shape["mode"] == mode, what
        batch = shape.get("batch_chains", 0) > 0
        got = (s["migrate"], s["spec"], s["batch_pair"] if batch else s["pair"])
        assert got == (mig, spec, pair), (what, s)
    rc, s = schedule(mode=ROWS, chains=4, batch_chains=128)   # the 8-GPU share, same kernel
    assert (s["migrate"], s["spec"], s["batch_pair"]) == (0, 1, 0)


def _stamps(t, i):
    return (t + 1) * (1 + (i * 7919) % 1009) + t * i


# The report of a synthetic h[2][NSTAMP] with h[t][i] = _stamps(t, i), as the report code
# printed it while it still lived in fitoct_plan_wait (its arithmetic over the bare slot
# numbers).  By hand, e.g.: sweeps = h[0][0] + h[1][0] = 1 + 2 = 3; wave 0's busy cycles
# h[0][56] + h[1][56] = 514 + 1084 = 1598, per sweep 533; occupancy k = 0: time
# (h[.][72]: 84 + 240) / 9148 = 0.0354, sweeps (h[.][77]: 328 + 733) / 6779 = 0.1565.
REPORT = """\
[fitoct stamps] gradient-wave busy per sweep by wave: 533 380 227 75 931 778 626 473
[fitoct stamps] sub-action cycles per gradient (chain 0): s0:1 s1:1 s2:1 s3:1 s4:0 s5:2 s6:2 s7:1 s8:1 s9:1 s10:1 s11:0\x20
[fitoct stamps] per action (chain 0 of each tile): a1:788x0 a2:560x0 a3:330x4 a4:102x12 a5:1386x1 a6:1157x1 a7:928x1 a8:699x0 a9:470x0 a10:241x6 a11:1526x1 a12:1296x1 a13:1068x1 a14:838x1 a15:610x0 a16:380x4 a17:152x8\x20
[fitoct stamps] tiles=2 mean sweeps/tile=2 max=2 | per sweep: grad-wave busy 857 nuts-wave busy 705 wall 552 memtime ticks
[fitoct stamps] chain 0 per NUTS round: busy 1, waiting for its gradient 1 (enqueue->sweep done 1, sweep done->resumed 1)
[fitoct stamps] enqueue -> first wave starts 0, last wave starts 0
[fitoct stamps] tile ends (fraction of the launch): mean -0.819 p10 -2.638 p50 -2.638 p90 -2.638 | first chain done in a tile: p10 12.121 p50 12.121 p90 12.121 | chains finished 2614, launch 0.0 ms
[fitoct stamps] tile occupancy (live chains k: share of tile time / of sweeps): k=0 0.0354/0.1565 k=1 0.3162/0.0890 k=2 0.2662/0.0214 k=3 0.2161/0.4004 k=4 0.1660/0.3328
"""
REPORT_TWO_ENDED = """\
[fitoct stamps] booking wave per booked leaf: busy 0, waiting for its record 0 (leaves booked per tile 1496, idle between trees 1268 per tile)
[fitoct stamps] producer of end 0 per produced leaf: waiting for its sweep 2, for lookahead / record slot 1, in trees 1 (leaves per tile 580)
[fitoct stamps] producer of end 1 per produced leaf: waiting for its sweep 0, for lookahead / record slot 1, in trees 1 (leaves per tile 1178)
[fitoct stamps] producer of end 0 per leaf (helped): finish_grad 2, stage 2, hand-over 1, prior_part 1
[fitoct stamps] producer of end 1 per leaf (helped): finish_grad 0, stage 0, hand-over 1, prior_part 1
[fitoct stamps] booking helper (primary tile): 1 cycles per booked leaf, 491 leaves per tile
[fitoct stamps] booking helper (partner tile): 0 cycles per booked leaf, 1546 leaves per tile
"""


@pytest.mark.parametrize("bidi", [0, 1])
def test_stamps_report_lines(bidi, capfd):
    f = _lib.lib().fitoct_internal_report_stamps
    f.restype = None
    h = (C.c_longlong * (2 * NSTAMP))(*[_stamps(t, i) for t in range(2) for i in range(NSTAMP)])
    assert len(set(h)) > 200      # (nearly) every slot holds a value of its own
    capfd.readouterr()
    f(h, C.c_int32(2), C.c_int32(bidi))
    assert capfd.readouterr().err == REPORT + (REPORT_TWO_ENDED if bidi else "")
