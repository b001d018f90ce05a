"""lp and grad lp bit for bit against a recording of the parent library.

Instruction-level work on the sweep's cross-lane reduction (``transpose_reduce``) and on
the leaf path (``write_mp``, ``prior_part``, ``finish_grad``) must leave every
floating-point operation, its operands and its order alone.  ``fitoct_logp_grad`` runs
the same ``gradient_pass``, ``prior_part`` and ``finish_grad`` as the sampler, so each
case evaluates 8 seeded positions and compares lp and the gradient exactly (the 64-bit
patterns) with ``tests/golden/reduce_bits_parent.npz``, recorded on an MI355X from the
library as it was before that work:

    python tests/golden/record_reduce_bits.py

The fixture holds the seeds and the recorded bits only; data and positions are
regenerated from the seeds.  Cases, one per reduction width and role layout:

* horseshoe, normal and lasso at Nn = 15 (19 sums), each at N = 2048 (8 bins per lane,
  paired bins), N = 300 (basis rows in registers, padding lanes) and N = 4096 (16 bins
  per lane);
* Nn = 20 (24 padded control points, 28 sums: odd counts at other steps of the reduction,
  two parameters per lane);
* the mono-exponential family at N = 256;
* horseshoe with ``prior_PD = 1`` (no sweep: the prior's part alone);
* horseshoe at positions where some bin has 1 + dL <= 0 (the sweep's ``acc[0] =
  INFINITY`` path): lp is -inf there, exactly as recorded.

``tests/test_gpu_logp.py`` pins the same paths to the oracle at 1e-11 / 1e-8.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fitoct_amd import ExpGPProblem, logp_grad   # noqa: E402
from fitoct_amd.synth import default_prior, synth_decay   # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "reduce_bits_parent.npz")
POINTS = 8
# name: (family, N, Nn, prior_PD, guard rows: positions whose yGP drives 1 + dL below 0)
CASES = {
    "horseshoe_N2048": ("horseshoe", 2048, 15, 0, False),
    "horseshoe_N300": ("horseshoe", 300, 15, 0, False),
    "horseshoe_N4096": ("horseshoe", 4096, 15, 0, False),
    "normal_N2048": ("normal", 2048, 15, 0, False),
    "normal_N300": ("normal", 300, 15, 0, False),
    "normal_N4096": ("normal", 4096, 15, 0, False),
    "lasso_N2048": ("lasso", 2048, 15, 0, False),
    "lasso_N300": ("lasso", 300, 15, 0, False),
    "lasso_N4096": ("lasso", 4096, 15, 0, False),
    "horseshoe_Nn20_N700": ("horseshoe", 700, 20, 0, False),
    "monoexp_N256": ("monoexp", 256, 2, 0, False),
    "horseshoe_N2048_priorPD": ("horseshoe", 2048, 15, 1, False),
    "horseshoe_N2048_guard": ("horseshoe", 2048, 15, 0, True),
}


def seeds(name):
    """(data seed, position seed) of a case: fixed by its place in the sorted case list."""
    i = sorted(CASES).index(name)
    return 100 + i, 200 + i


def problem_and_points(name, data_seed, point_seed):
    family, N, Nn, pd, guard = CASES[name]
    t0, S0 = default_prior()
    d = synth_decay(N, "sincExp", data_seed)
    if family == "monoexp":
        prob = ExpGPProblem(d["x"], d["y"], d["uy"], dataType=2, Nn=2, theta0=t0,
                            Sigma0=np.eye(3), prior_type="monoexp")
    else:
        prob = ExpGPProblem(d["x"], d["y"], d["uy"], dataType=2, Nn=Nn, gridType="extremal",
                            theta0=t0, Sigma0=S0, prior_type=family, prior_PD=pd)
    rng = np.random.default_rng(point_seed)
    q = rng.normal(0, 0.05, (POINTS, prob.D))   # small yGP: 1 + dL > 0 in every bin
    q[:, 0:3] = np.log(t0) + rng.normal(0, 0.02, (POINTS, 3))
    if family != "monoexp":
        q[:, -1] = rng.normal(0, 0.3, POINTS)
    if guard:   # every other position: z_j = -4 with unit scales, so yGP = -4 and 1 + dL < 0
        q[::2, 3:3 + Nn] = -4.0
        q[::2, 3 + Nn:-1] = 0.0
    return prob, q


def evaluate(name):
    ds, ps = seeds(name)
    prob, q = problem_and_points(name, ds, ps)
    lp, g, _ = logp_grad(prob, q, "f64")
    return (np.ascontiguousarray(lp, dtype=np.float64),
            np.ascontiguousarray(g, dtype=np.float64))


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(CASES))
def test_logp_grad_bits_equal_parent(name, recorded):
    assert tuple(int(v) for v in recorded[f"{name}/seeds"]) == seeds(name)
    lp, g = evaluate(name)
    ref_lp, ref_g = recorded[f"{name}/lp_bits"], recorded[f"{name}/grad_bits"]
    assert ref_lp.dtype == np.uint64 and ref_g.dtype == np.uint64
    assert ref_lp.shape == (POINTS,) and ref_g.shape == g.shape
    family, N, Nn, pd, guard = CASES[name]
    if guard:   # the recorded -inf rows are the guard rows, and only they
        want = np.zeros(POINTS, dtype=bool)
        want[::2] = True
        assert np.array_equal(ref_lp.view(np.float64) == -np.inf, want)
    else:
        assert np.all(np.isfinite(ref_lp.view(np.float64)))
    assert np.array_equal(lp.view(np.uint64), ref_lp), (
        f"{name}: lp differs from the parent's at positions "
        f"{np.flatnonzero(lp.view(np.uint64) != ref_lp).tolist()}")
    diff = g.view(np.uint64) != ref_g
    assert not diff.any(), (
        f"{name}: {int(diff.sum())} of {diff.size} gradient values differ from the parent's "
        f"(parameters {sorted(set(np.nonzero(diff)[1].tolist()))})")
