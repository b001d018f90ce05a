"""The sampler's results bit for bit against a recording of the parent library.

Instruction-level work on the NUTS waves (the form of the Horner steps of fexp, one exp
per position in write_mp, the bin-sum index without an integer division) must leave every
floating-point operation and its order alone: draws, step sizes, inverse metrics and last positions are
compared exactly (``np.array_equal``) with ``tests/golden/sampler_bits_parent.npz``, recorded on
an MI355X from the library as it was before that work:

    python tests/test_gpu_sampler_bits.py --record

Cases (20 + 20 iterations, max_treedepth 6, seed 31):

* horseshoe N = 2048 and lasso N = 4096 in migrating tiles of four chains: the headline's
  and config 4's kernel instantiations.  Chains per tile is ceil(chains / CUs) and
  nothing else selects it, so these two run 1024 chains (a launch of 8 chains is 8 tiles
  of one chain: another kernel).  The fixture holds the chains of two tiles (the first and
  the last, 8 chains) in full, and a SHA-256 of every chain's arrays: the whole launch is
  compared, within the size a committed fixture may have.
  (1024 chains make tiles of four on the 256 CUs of an MI355X, the device the fixture was
  recorded on; on another CU count the chains_per_tile assertion fails.)
* horseshoe N = 2048 with 1 and with 4 chains: the non-migrating speculative kernels, which
  share write_mp / prior_part with the above.
* normal N = 512, 4 chains: basis rows in registers (row mode).
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

FIXTURE = os.path.join(ROOT, "tests", "golden", "sampler_bits_parent.npz")
FIELDS = ("draws", "stepsize", "inv_metric", "last_q")
# name: (family, N, chains, chains per tile, migrating)
CASES = {
    "horseshoe2048_mig": ("horseshoe", 2048, 1024, 4, True),
    "lasso4096_mig": ("lasso", 4096, 1024, 4, True),
    "horseshoe2048_c1": ("horseshoe", 2048, 1, 1, False),
    "horseshoe2048_c4": ("horseshoe", 2048, 4, 1, False),
    "normal512_c4": ("normal", 512, 4, 1, False),
}
KEEP = 8   # a launch of more chains stores its first and last four (two tiles of four)


def _run(name):
    family, N, chains, G, mig = CASES[name]
    t0, S0 = default_prior()
    d = synth_decay(N, "sincExp", 11)
    prob = ExpGPProblem(d["x"], d["y"], d["uy"], Nn=15, gridType="extremal", theta0=t0,
                        Sigma0=S0, prior_type=family)
    cfg = SamplerConfig(chains=chains, warmup=20, samples=20, seed=31, max_treedepth=6)
    with Plan(prob, cfg) as pl:
        pl.run()
        info, out = pl.info, pl.download()
    assert info["chains_per_tile"] == G, info
    assert info["sampler"] == (3 if mig else 2), info   # FITOCT_SAMPLER_MIGRATE_SPEC / _SPECULATIVE
    return {f: np.ascontiguousarray(getattr(out, f), dtype=np.float64) for f in FIELDS}


def _kept(a):
    return a if a.shape[0] <= KEEP else np.concatenate([a[:KEEP // 2], a[-(KEEP // 2):]])


def _digest(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def _nan_equal_bits(a, b):
    """Exact equality of the stored bits (NaN payloads included)."""
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(CASES))
def test_sampler_bits_equal_parent(name, recorded):
    got = _run(name)
    for f in FIELDS:
        ref = recorded[f"{name}/{f}"]
        kept = _kept(got[f])
        assert ref.dtype == np.float64
        assert np.array_equal(kept, ref, equal_nan=True) and _nan_equal_bits(kept, ref), (
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
