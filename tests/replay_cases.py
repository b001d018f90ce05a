"""The shapes of the one-step replay audit (tests/replay_audit.py), shared by the GPU tests
(test_gpu_replay.py) and by the CPU test of the replay's own noise floor on the same
problems and configs (test_replay_audit.py).  No GPU import.

Each case is the smallest shape that still selects one instantiation of the sampler kernel.
Horseshoe cases run at max_treedepth <= 8, the others at <= 10: a transition amplifies a
start error the more the deeper its tree, and at max_treedepth 10 the horseshoe's replay
from starts moved by 1e-12 sits at the 0.2 % cap of the noise-floor test (parity
notes), where the replay compares at 1e-6."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from fitoct_amd import ExpGPProblem, SamplerConfig
from fitoct_amd.synth import default_prior, synth_decay

W, S = 150, 60


def prob(family, N, Nn, seed=11, mod="sincExp", grid="extremal", theta0=None, **kw):
    t0, S0 = default_prior()
    if theta0 is not None:
        t0 = np.asarray(theta0, dtype=np.float64)
        S0 = np.diag((0.05 * t0) ** 2)
    d = synth_decay(N, mod, seed)
    return ExpGPProblem(d["x"], d["y"], d["uy"], Nn=Nn, gridType=grid, theta0=t0, Sigma0=S0,
                        prior_type=family, **kw)


def bench_prob(family, N):
    """bench.py's synthetic input at a BASELINE config shape (test_gpu_sampler._bench_problem)."""
    return prob(family, N, 15, seed=1234, lambda_scale=10.0, nu=1.0)


def user_basis_prob(N):
    """The caller-supplied, non-SE basis of test_gpu_logp.test_user_basis_rows_mode."""
    from oracle import model_np as M
    t0, S0 = default_prior()
    d = synth_decay(N, "sincExp3", 5)
    B, _ = M.gp_basis(d["x"], 12, "extremal", 1 / 12)
    B = B * 0.9 + 0.01
    return ExpGPProblem(d["x"], d["y"], d["uy"], Nn=12, gridType="extremal", theta0=t0, Sigma0=S0,
                        prior_type="lasso", B=B)


@dataclass
class Case:
    make: object                  # () -> ExpGPProblem (or a list of them: a batch)
    chains: int                   # chains launched (per problem)
    depth: int
    replay: tuple = None          # chain indices replayed; None: every chain
    seed: int = 77
    extra: dict = field(default_factory=dict)   # further SamplerConfig fields

    def cfg(self, chains=None, **kw):
        return SamplerConfig(chains=self.chains if chains is None else chains, warmup=W, samples=S,
                             seed=self.seed, max_treedepth=self.depth, **{**self.extra, **kw})

    def replayed(self):
        return tuple(range(self.chains)) if self.replay is None else self.replay


HEADLINE_REPLAY = tuple(range(16)) + tuple(int(c) for c in np.linspace(16, 1007, 16)) \
    + tuple(range(1008, 1024))

# cases whose transitions are replayed (f64)
REPLAY = {
    "config2": Case(lambda: bench_prob("normal", 512), 24, 10),
    "headline": Case(lambda: bench_prob("horseshoe", 2048), 1024, 7, HEADLINE_REPLAY),
    "batch": Case(lambda: [prob("normal", 481, 15, seed=40 + f) for f in range(6)], 4, 10),
    "poly_one_chain": Case(lambda: prob("lasso", 1000, 12), 16, 8),
    "ppl2_normal": Case(lambda: prob("normal", 512, 20), 8, 6),
    "ppl2_horseshoe": Case(lambda: prob("horseshoe", 97, 24), 8, 6),
    "compact16": Case(lambda: prob("lasso", 3001, 15), 8, 7),
    "streamed": Case(lambda: prob("normal", 8192, 15), 4, 6),
    "amplitude_conv": Case(lambda: prob("horseshoe", 700, 20, grid="internal", dataType=1,
                                        kernel_conv=1, lambda_conv=1,
                                        theta0=[1000.0, 2000.0, 150.0]), 8, 8),
    "prior_pd": Case(lambda: prob("horseshoe", 481, 10, grid="internal", prior_PD=1), 8, 8),
    "monoexp": Case(lambda: prob("monoexp", 256, 10), 8, 10),
    "minimum": Case(lambda: prob("normal", 2, 2), 8, 10),
    "user_basis_streamed": Case(lambda: user_basis_prob(1000), 8, 10),
    "user_basis_resident": Case(lambda: user_basis_prob(300), 8, 10),
    # a length scale rho other than 1/Nn, both well conditioned (kappa2 4e3 and 1.3: the
    # oracle's own basis is the library's to ~1e-13, so the replay means what it says)
    "rho_wide": Case(lambda: prob("normal", 700, 10, grid="internal", rho=0.15), 8, 8),
    "rho_overflow_rows": Case(lambda: prob("normal", 1000, 15, rho=0.03), 8, 8),
}

# row and adaptation checks only
NO_REPLAY = {
    "mixed_1024": Case(lambda: prob("normal", 1024, 12, seed=4), 8, 10,
                       extra={"precision": "mixed"}),
    "mixed_300": Case(lambda: prob("normal", 300, 15), 8, 10, extra={"precision": "mixed"}),
    "hard_geometry": Case(lambda: prob("horseshoe", 300, 8), 16, 12,
                          extra={"adapt_delta": 0.99}),
}
