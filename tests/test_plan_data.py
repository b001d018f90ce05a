"""The data plan (csrc/plan_data.cpp) without a GPU.

``fitoct_internal_plan_data`` runs the planner's pure decision of what a problem is staged as
-- basis mode, bins per lane, padding, the factorised basis, the geometric-grid ratios, the
staged bytes -- over a problem and explicit switches (no environment read, no device);
``fitoct_internal_batch_layout`` does the same for a batch's common bin layout.  The first
table restates what the GPU tests assert through ``fitoct_plan_get_info``; the second covers
the branches none of them asserts.  Every row's integers, doubles and FNV-1a digests (staged
bytes; K^-1; b; geo_R | geo_dcx | geo_tmax; S0inv) are also compared with
``golden/plan_data_parent.json``, recorded from the planning code as it stood inside
``plan_common`` before it moved: not a bit of what is staged may change.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fitoct_amd import ExpGPProblem, _lib  # noqa: E402
from fitoct_amd.synth import default_prior, synth_decay  # noqa: E402
import rho_cases  # noqa: E402
from test_schedule import SWITCHES, UNSET  # noqa: E402

POLY, ROWS = 0, 1          # kernel_params.h BasisMode
GT = 256                   # gradient lanes of a tile
E_ARG, E_INTERNAL = -1, -7
INTS = ("mode", "bpt", "n_pad", "nnp", "ppl", "mixed", "N", "Nn", "D", "family", "prior_PD",
        "geo", "staged_bytes", "kinv_len", "bv_len", "xyu_len", "B_len")
DBLS = ("theta0_0", "theta0_1", "theta0_2", "lambda_rate_eff", "lambda_scale", "nu",
        "sigma_scale", "sigma_scale_inv", "theta_rate", "geo_tmax")
DIGESTS = ("staged", "kinv", "bv", "geo", "S0inv")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "plan_data_parent.json")


def prob(N, family="normal", Nn=15, grid="extremal", kind="sincExp", seed=7, bend=False,
         user_B=False, **kw):
    """A synthetic decay on the arithmetic grid linspace(20, 500, N); ``bend`` moves one depth
    by 1e-9 of the range (off the grid for every geometric layout, 1e-12), ``user_B`` hands in
    a basis of the caller's."""
    t0, S0 = default_prior()
    d = synth_decay(N, kind, seed)
    x = d["x"].copy()
    if bend:
        x[N // 3] += 1e-9 * (x[-1] - x[0])
    B = np.random.default_rng(N).normal(0, 0.1, (N, Nn)) if user_B else None
    return ExpGPProblem(x, d["y"], d["uy"], Nn=Nn, gridType=grid, theta0=t0, Sigma0=S0,
                        prior_type=family, B=B, **kw)


def _switches(switches):
    return (C.c_int32 * len(SWITCHES))(*[int((UNSET | switches)[k]) for k in SWITCHES])


def _error(rc):
    return {"rc": rc, "error": _lib.lib().fitoct_last_error().decode()}


def plan_data(p, precision="f64", force_bpt=-1, poly_only=False, **switches):
    """The data plan of ExpGPProblem p as a dict: rc 0 with INTS, DBLS (hex) and DIGESTS, or
    the status with its message."""
    f = _lib.lib().fitoct_internal_plan_data
    f.restype = C.c_int32
    ints, dbls = (C.c_int64 * len(INTS))(), (C.c_double * len(DBLS))()
    dig = (C.c_uint64 * len(DIGESTS))()
    c = p.to_c()
    rc = f(C.byref(c), C.c_int32(_lib.PREC[precision]), _switches(switches),
           C.c_int32(force_bpt), C.c_int32(int(poly_only)), ints, dbls, dig)
    if rc:
        return _error(rc)
    return ({"rc": 0} | dict(zip(INTS, ints)) | {k: float(v).hex() for k, v in zip(DBLS, dbls)}
            | {"fnv_" + k: f"{v:016x}" for k, v in zip(DIGESTS, dig)})


def batch_layout(ps, precision="f64", **switches):
    """The common layout of a batch of ExpGPProblems: rc 0 with bpt and every problem's final
    (mode, bpt, n_pad), or the status with its message."""
    f = _lib.lib().fitoct_internal_batch_layout
    f.restype = C.c_int32
    arr = (_lib.Problem * len(ps))(*[p.to_c() for p in ps])
    out = (C.c_int64 * (1 + 3 * len(ps)))()
    rc = f(arr, C.c_int32(len(ps)), C.c_int32(_lib.PREC[precision]), _switches(switches), out)
    if rc:
        return _error(rc)
    return {"rc": 0, "bpt": out[0], "plans": [list(out[1 + 3 * i:4 + 3 * i]) for i in range(len(ps))]}


# (id, problem, arguments of plan_data, what the row must say)
# first: what GPU tests assert through fitoct_plan_get_info, each named after the test
PLANS = [
    ("test_gpu_replay config2 N=256", lambda: prob(256), {}, dict(mode=ROWS, bpt=1, n_pad=256)),
    ("test_gpu_replay config2 N=512", lambda: prob(512), {}, dict(mode=ROWS, bpt=2, n_pad=512)),
    ("test_gpu_batch N=513 factorised", lambda: prob(513), {}, dict(mode=POLY, bpt=4)),
    ("test_gpu_replay headline N=2048 horseshoe", lambda: prob(2048, "horseshoe"), {},
     dict(mode=POLY, bpt=8, n_pad=2048, geo=1)),
    ("test_gpu_sampler config4 N=4096", lambda: prob(4096), {},
     dict(mode=POLY, bpt=16, n_pad=4096, geo=1)),
    ("test_gpu_sampler config4 N=4096 no_geo", lambda: prob(4096), dict(no_geo=1),
     dict(mode=POLY, bpt=0, n_pad=4096, geo=0)),
    ("test_gpu_sampler config4 N=4096 off the grid", lambda: prob(4096, bend=True), {},
     dict(mode=POLY, bpt=0, n_pad=4096, geo=0)),
    ("test_gpu_replay compact16 N=3001 padded", lambda: prob(3001, "horseshoe"), {},
     dict(mode=POLY, bpt=16, n_pad=4096, geo=1)),
    ("test_gpu_replay streamed N=8192", lambda: prob(8192), {},
     dict(mode=POLY, bpt=0, n_pad=8192)),
    ("N=5000 padded to the lanes", lambda: prob(5000), {},
     dict(mode=POLY, bpt=0, n_pad=-(-5000 // GT) * GT)),
] + [
    ("rho_cases " + c.id, c.problem, {},
     {} if c.mode is None else dict(mode=c.mode, bpt=c.bpt)) for c in rho_cases.CASES
] + [
    # second: the branches no GPU test asserts directly
    ("mixed N=512", lambda: prob(512), dict(precision="mixed"),
     dict(mode=ROWS, mixed=1, bpt=2, n_pad=512)),
    ("mixed N=1024", lambda: prob(1024), dict(precision="mixed"),
     dict(mode=ROWS, mixed=1, bpt=4, n_pad=1024)),
    ("mixed N=2000 streamed", lambda: prob(2000), dict(precision="mixed"),
     dict(mode=ROWS, mixed=1, bpt=0, n_pad=2048)),
    ("caller's B N=300", lambda: prob(300, user_B=True), {}, dict(mode=ROWS, bpt=2, kinv_len=0)),
    ("caller's B N=2000", lambda: prob(2000, user_B=True), {}, dict(mode=ROWS, bpt=0, n_pad=2048)),
    ("Nn=9", lambda: prob(700, Nn=9), {}, dict(mode=POLY, nnp=15, ppl=1, Nn=9)),
    ("Nn=20", lambda: prob(700, Nn=20), {}, dict(mode=POLY, nnp=24, ppl=2, Nn=20)),
    ("monoexp f64", lambda: prob(700, "monoexp", Nn=10), {},
     dict(mode=POLY, Nn=0, D=3, bpt=4, kinv_len=0, B_len=0, geo=0)),
    ("monoexp mixed", lambda: prob(700, "monoexp", Nn=10), dict(precision="mixed"),
     dict(mode=ROWS, Nn=0, mixed=1, bpt=4)),
    ("force_bpt above the plan", lambda: prob(300), dict(force_bpt=4, poly_only=True),
     dict(mode=POLY, bpt=4, n_pad=1024)),
    ("force_bpt streamed", lambda: prob(300), dict(force_bpt=0, poly_only=True),
     dict(mode=POLY, bpt=0, n_pad=512)),
    ("force_bpt below the plan", lambda: prob(700), dict(force_bpt=2),
     dict(rc=E_ARG, error="bin layout too small")),
    ("force_bpt 16 on the grid", lambda: prob(2048), dict(force_bpt=16),
     dict(mode=POLY, bpt=16, n_pad=4096, geo=1)),
    ("force_bpt 16 off the grid", lambda: prob(2048, bend=True), dict(force_bpt=16),
     dict(rc=E_INTERNAL, error="16-bin layout without a geometric grid")),
]

# (id, problems, switches, what the row must say); plans: (mode, bpt, n_pad) per problem
BATCHES = [
    ("test_gpu_batch rows 481 + 200", lambda: [prob(481, seed=1), prob(200, kind="sincExp1", seed=2)],
     {}, dict(bpt=2, plans=[[ROWS, 2, 512], [ROWS, 2, 512]])),
    ("test_gpu_batch 481 + 700", lambda: [prob(481, seed=1), prob(700, kind="sincExp1", seed=2)],
     {}, dict(bpt=4, plans=[[POLY, 4, 1024], [POLY, 4, 1024]])),
    ("test_gpu_batch ragged 481 + 300 + 700",
     lambda: [prob(481, seed=1), prob(300, kind="sincExp1", seed=2), prob(700, kind="sincExp2", seed=3)],
     {}, dict(bpt=4, plans=[[POLY, 4, 1024]] * 3)),
    ("one streamed problem streams all", lambda: [prob(700), prob(5000)], {},
     dict(bpt=0, plans=[[POLY, 0, 768], [POLY, 0, 5120]])),
    ("16 bins for all on the grid", lambda: [prob(4096), prob(2048)], {},
     dict(bpt=16, plans=[[POLY, 16, 4096]] * 2)),
    ("16 bins fall back to streamed", lambda: [prob(4096), prob(2048, bend=True)], {},
     dict(bpt=0, plans=[[POLY, 0, 4096], [POLY, 0, 2048]])),
    ("different Nn", lambda: [prob(300), prob(300, Nn=10)], {},
     dict(rc=E_ARG, error="batch problems must share prior_type and Nn (problem 1)")),
    ("different family", lambda: [prob(300), prob(300), prob(300, "lasso")], {},
     dict(rc=E_ARG, error="batch problems must share prior_type and Nn (problem 2)")),
    ("different kernels", lambda: [prob(700), prob(700, user_B=True)], {},
     dict(rc=E_ARG, error="batch problems plan to different kernels (basis mode)")),
    ("a problem's own failure", lambda: [prob(300), prob(300, sigma_scale=0.0)], {},
     dict(rc=E_ARG, error="problem 1: sigma_scale must be > 0")),
]


def run_all():
    """every row's result, keyed by its id (what the golden file holds)"""
    rows = {"plan: " + name: plan_data(make(), **args) for name, make, args, _ in PLANS}
    rows.update({"batch: " + name: batch_layout(make(), **sw) for name, make, sw, _ in BATCHES})
    return rows


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name,make,args,want", PLANS, ids=[t[0] for t in PLANS])
def test_plan_data_table(name, make, args, want, golden):
    p = make()
    got = plan_data(p, **args)
    assert {k: got.get(k) for k in want} == want, (name, got)
    if got["rc"] == 0:
        mixed = args.get("precision") == "mixed"
        assert got["mixed"] == int(mixed) and got["N"] == p.N and got["xyu_len"] == 3 * p.N
        per_bin = 3 + (2 if got["mode"] == POLY else got["nnp"])
        assert got["staged_bytes"] == (4 if mixed else 8) * per_bin * got["n_pad"]
        assert got["n_pad"] % GT == 0 and got["n_pad"] >= p.N
        assert got["n_pad"] == (got["bpt"] * GT if got["bpt"] else -(-p.N // GT) * GT)
        if got["bpt"] == 16:
            assert got["geo"] == 1
    assert got == golden["plan: " + name]


@pytest.mark.parametrize("name,make,switches,want", BATCHES, ids=[t[0] for t in BATCHES])
def test_batch_layout_table(name, make, switches, want, golden):
    got = batch_layout(make(), **switches)
    assert {k: got.get(k) for k in want} == want, (name, got)
    assert got == golden["batch: " + name]


def test_golden_file_holds_exactly_the_tables(golden):
    assert set(golden) == ({"plan: " + t[0] for t in PLANS} | {"batch: " + t[0] for t in BATCHES})
    assert len(golden) == len(PLANS) + len(BATCHES)
