"""The sampler's results bit for bit against a recording of the parent library, at the
shapes where work on the leaf path's scalar traffic can go wrong and that
``tests/test_gpu_sampler_bits.py`` does not reach.

Moving lane masks, LDS sub-bases, per-lane roles and kernel parameters between SGPRs, VGPR
lanes and LDS must leave every floating-point operation, operand and order alone: draws,
step sizes, inverse metrics and last positions are compared as 64-bit patterns with
``tests/golden/leaf_scalar_bits_parent.npz``, recorded on an MI355X from the library as it
was before that work:

    python tests/test_gpu_leaf_scalar_bits.py --record

Cases (10 + 10 iterations, seed 31):

* horseshoe with Nn = 9 in the NNP = 15 kernel, N = 2048, 1024 chains in migrating tiles of
  four, max_treedepth 5: with Nn < NNP every ``lane < Nn`` / z-lane / role predicate and every
  padded AUX / MP slot differs from the Nn = 15 case.
* the headline shape (horseshoe N = 2048, Nn = 15, 1024 chains) at max_treedepth 12,
  adapt_delta 0.99: the full LDS carve, where anything added to the tile's head would push the
  tile from four chains to three.  ``chains_per_tile == 4`` is asserted from the plan before
  the run.
* lasso N = 4096 and normal N = 512 with 4 chains (max_treedepth 6): the families that keep
  their lane predicates in registers, through the helpers they share with the horseshoe.

A launch of 1024 chains stores its first and last four chains in full (two tiles of four) and
a SHA-256 of every chain's arrays.  (1024 chains make tiles of four on the 256 CUs of an
MI355X, the device the fixture was recorded on.)
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fitoct_amd import ExpGPProblem, Plan, SamplerConfig   # noqa: E402
from fitoct_amd.synth import default_prior, synth_decay   # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "leaf_scalar_bits_parent.npz")
FIELDS = ("draws", "stepsize", "inv_metric", "last_q")
# name: (family, N, Nn, chains, max_treedepth, adapt_delta, chains per tile, migrating)
CASES = {
    "horseshoe2048_nn9_mig": ("horseshoe", 2048, 9, 1024, 5, 0.8, 4, True),
    "horseshoe2048_depth12_mig": ("horseshoe", 2048, 15, 1024, 12, 0.99, 4, True),
    "lasso4096_c4": ("lasso", 4096, 15, 4, 6, 0.8, 1, False),
    "normal512_c4": ("normal", 512, 15, 4, 6, 0.8, 1, False),
}
KEEP = 8   # a launch of more chains stores its first and last four (two tiles of four)


def _run(name):
    family, N, Nn, chains, depth, delta, G, mig = CASES[name]
    t0, S0 = default_prior()
    d = synth_decay(N, "sincExp", 11)
    prob = ExpGPProblem(d["x"], d["y"], d["uy"], Nn=Nn, gridType="extremal", theta0=t0,
                        Sigma0=S0, prior_type=family)
    cfg = SamplerConfig(chains=chains, warmup=10, samples=10, seed=31, max_treedepth=depth,
                        adapt_delta=delta)
    with Plan(prob, cfg) as pl:
        info = pl.info
        assert info["chains_per_tile"] == G, info   # before the run: the LDS carve fits G chains
        if mig:
            assert info["sampler"] == 3, info   # FITOCT_SAMPLER_MIGRATE_SPEC
        pl.run()
        out = pl.download()
    return {f: np.ascontiguousarray(getattr(out, f), dtype=np.float64) for f in FIELDS}


def _kept(a):
    return a if a.shape[0] <= KEEP else np.concatenate([a[:KEEP // 2], a[-(KEEP // 2):]])


def _digest(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def _same_bits(a, b):
    """Exact equality of the stored 64-bit patterns (NaN payloads and signed zeros included)."""
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(CASES))
def test_leaf_scalar_bits_equal_parent(name, recorded):
    got = _run(name)
    for f in FIELDS:
        ref = recorded[f"{name}/{f}"]
        kept = _kept(got[f])
        assert ref.dtype == np.float64
        assert _same_bits(kept, ref), (
            f"{name}: {f} of the stored chains differs from the parent's in "
            f"{int(np.sum(kept.view(np.uint64) != ref.view(np.uint64)))} of {ref.size} values")
        assert _digest(got[f]) == str(recorded[f"{name}/{f}/sha256"]), (
            f"{name}: {f} differs from the parent's in a chain the fixture does not store")


def _record():
    out = {}
    for name in sorted(CASES):
        got = _run(name)
        for f in FIELDS:
            out[f"{name}/{f}"] = _kept(got[f])
            out[f"{name}/{f}/sha256"] = np.array(_digest(got[f]))
        print(name, {f: got[f].shape for f in FIELDS}, "finite draws:",
              bool(np.all(np.isfinite(got["draws"][:, :, 0]))))
    path = sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > 2 else FIXTURE
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if "--record" in sys.argv:
        _record()
