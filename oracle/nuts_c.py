"""ORACLE (test infrastructure only) -- ctypes wrapper of oracle/build/liboracle.so,
the C restatement of the ExpGP model and Stan's recursive NUTS (fitoct_oracle.c).

Parity status vs rstan: **parity unpinned** (see fitoct_oracle.c header).
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# FITOCT_SANITIZE=1: the ASan/UBSan build (make -C oracle sanitize) in oracle/build_san/
SANITIZE = os.environ.get("FITOCT_SANITIZE", "0") not in ("", "0")
BUILD_DIR = os.path.join(HERE, "build_san" if SANITIZE else "build")
LIB = os.path.join(BUILD_DIR, "liboracle.so")
_L = None


_BUILT = False


def build(force: bool = False) -> str:
    """make -C oracle (once per process; make tracks the sources)."""
    global _BUILT
    if force or not _BUILT:
        subprocess.run(["make", "-s", "-C", HERE] + (["sanitize"] if SANITIZE else [])
                       + (["-B"] if force else []), check=True)
        _BUILT = True
    return LIB


def lib():
    global _L
    if _L is None:
        build()
        from fitoct_amd import _lib as abi   # ABI struct layouts (include/fitoct.h)
        L = C.CDLL(LIB)
        dp = C.POINTER(C.c_double)
        L.oracle_basis.argtypes = [C.POINTER(abi.Problem), dp]
        L.oracle_logp_grad.argtypes = [C.POINTER(abi.Problem), C.c_int, dp, dp, dp, dp]
        L.oracle_sample.argtypes = [C.POINTER(abi.Problem), C.POINTER(abi.Config), dp, dp, dp,
                                    C.POINTER(C.c_longlong), C.c_int]
        L.oracle_philox.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_uint32)]
        L.oracle_normals.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_int, dp]
        L.oracle_sample_init.argtypes = [C.POINTER(abi.Problem), C.POINTER(abi.Config), dp, dp,
                                         dp, C.POINTER(C.c_longlong), C.c_int, dp, dp, dp]
        ip = C.POINTER(C.c_int32)
        L.oracle_replay.argtypes = [C.POINTER(abi.Problem), C.POINTER(abi.Config), C.c_int, ip, ip,
                                    dp, dp, dp, dp, C.c_int]
        L.oracle_replay_init_stepsize.argtypes = [C.POINTER(abi.Problem), C.POINTER(abi.Config),
                                                  C.c_int, ip, ip, dp, dp, dp, dp, C.c_int]
        _L = L
    return _L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def philox(ctr, key):
    c = (C.c_uint32 * 4)(*ctr)
    k = (C.c_uint32 * 2)(*key)
    o = (C.c_uint32 * 4)()
    lib().oracle_philox(c, k, o)
    return list(o)


def normals(seed, stream, tag, it, s, D):
    out = np.empty(D)
    lib().oracle_normals(seed, stream, tag, it, s, D, _dp(out))
    return out


def basis(prob):
    """prob: fitoct_amd.ExpGPProblem"""
    B = np.zeros((prob.N, prob.Nn))
    p = prob.to_c()
    assert lib().oracle_basis(C.byref(p), _dp(B)) == 0
    return B


def logp_grad(prob, q):
    q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float64)
    P, D = q.shape
    lp, g, s2 = np.zeros(P), np.zeros((P, D)), np.zeros(P)
    p = prob.to_c()
    assert lib().oracle_logp_grad(C.byref(p), P, _dp(q), _dp(lp), _dp(g), _dp(s2)) == 0
    return lp, g, s2


def sample(prob, cfg, nthreads: int = 0, q_init=None, init_stepsize=None, init_inv_metric=None):
    """prob: ExpGPProblem, cfg: SamplerConfig -> dict(draws, stepsize, inv_metric, leapfrogs).
    q_init [chains, D] / init_stepsize [chains] / init_inv_metric [chains, D]: the warm
    restart of fitoct_plan_set_init (None = the default start)."""
    D = prob.D
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64)
            for a in (q_init, init_stepsize, init_inv_metric)]
    iters = cfg.warmup + cfg.samples if cfg.save_warmup else cfg.samples
    draws = np.full((cfg.chains, iters, D + 8), np.nan)
    eps = np.zeros(cfg.chains)
    minv = np.zeros((cfg.chains, D))
    lf = np.zeros(cfg.chains, dtype=np.int64)
    p, c = prob.to_c(), cfg.to_c()
    rc = lib().oracle_sample_init(C.byref(p), C.byref(c), _dp(draws), _dp(eps), _dp(minv),
                                  lf.ctypes.data_as(C.POINTER(C.c_longlong)), int(nthreads),
                                  *[None if a is None else _dp(a) for a in arrs])
    if rc != 0:
        raise RuntimeError(f"oracle_sample failed with status {rc}")
    return {"draws": draws, "stepsize": eps, "inv_metric": minv, "leapfrogs": lf}


def _replay_args(prob, gid, idx, q, eps, minv):
    gid = np.ascontiguousarray(gid, dtype=np.int32)
    n = gid.size
    idx = np.ascontiguousarray(np.broadcast_to(np.asarray(idx, dtype=np.int32), (n,)))
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(n, prob.D)
    eps = np.ascontiguousarray(np.broadcast_to(np.asarray(eps, dtype=np.float64), (n,)))
    minv = np.ascontiguousarray(np.broadcast_to(np.asarray(minv, dtype=np.float64), (n, prob.D)))
    ip = C.POINTER(C.c_int32)
    return n, gid, idx, q, eps, minv, [gid.ctypes.data_as(ip), idx.ctypes.data_as(ip), _dp(q),
                                       _dp(eps), _dp(minv)]


def replay(prob, cfg, gid, t, q, eps, minv, nthreads: int = 0):
    """One transition per item: GLOBAL chain id gid[n] at iteration t[n] from the
    unconstrained position q[n, D] with step size eps[n] and inverse metric minv[n, D]
    -> rows[n, D + 8], each the row a run would store for that transition."""
    n, *keep, ptrs = _replay_args(prob, gid, t, q, eps, minv)
    rows = np.full((n, prob.D + 8), np.nan)
    p, c = prob.to_c(), cfg.to_c()
    rc = lib().oracle_replay(C.byref(p), C.byref(c), n, *ptrs, _dp(rows), int(nthreads))
    if rc != 0:
        raise RuntimeError(f"oracle_replay failed with status {rc}")
    return rows


def replay_init_stepsize(prob, cfg, gid, window, q, eps, minv, nthreads: int = 0):
    """The step-size search of chain gid[n] for its window[n]-th search (0: the run's
    start, k: after the k-th metric update) from position q[n, D], incoming step size
    eps[n] and inverse metric minv[n, D] -> the step sizes found [n]."""
    n, *keep, ptrs = _replay_args(prob, gid, window, q, eps, minv)
    out = np.full(n, np.nan)
    p, c = prob.to_c(), cfg.to_c()
    rc = lib().oracle_replay_init_stepsize(C.byref(p), C.byref(c), n, *ptrs, _dp(out),
                                           int(nthreads))
    if rc != 0:
        raise RuntimeError(f"oracle_replay_init_stepsize failed with status {rc}")
    return out
