"""The three double-precision GP bases -- fitoct_build_basis (the library, host only),
oracle_basis (the C oracle) and model_np.gp_basis -- against the exact basis
(rho_cases.exact_basis, 60 digits) over the length scales of rho_cases.CASES, and the way a
caller's rho_scale reaches fitoct_problem.rho.

The bound is derived, not tuned: a Cholesky solve's forward error, per entry
(3 Nn + 1) eps kappa2 max|B| (rho_cases.chol_bound).  The measured ratios to it are printed
and recorded in DESIGN.md §3 (length scale)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import rho_cases as R
from fitoct_amd import ExpGPProblem, _lib, api, pipeline
from fitoct_amd.synth import default_prior, synth_decay
from oracle import model_np as M
from oracle import nuts_c

N_DEPTHS = 97


def _design_problem(Nn, grid, rho, conv, N=N_DEPTHS):
    d = synth_decay(N, "sincExp", N + 3)
    t0, S0 = default_prior()
    return ExpGPProblem(d["x"], d["y"], d["uy"], Nn=Nn, gridType=grid, rho=rho, theta0=t0,
                        Sigma0=S0, kernel_conv=conv)


IMPLS = {
    "library": lambda p: p.basis()[0],
    "c_oracle": nuts_c.basis,
    "numpy": lambda p: M.gp_basis(p.x, p.Nn, p.gridType, p.rho, p.kernel_conv, p.nugget)[0],
}


@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("design", R.DESIGNS, ids=lambda d: f"Nn{d[0]}-{d[1][:3]}-rho{d[2]}-c{d[3]}")
def test_basis_within_the_cholesky_bound(design, impl):
    Nn, grid, rho, conv = design
    prob = _design_problem(*design)
    ex = R.exact_basis(prob.x, Nn, grid, rho, conv)
    err = float(np.abs(IMPLS[impl](prob) - ex.B).max())
    bound = R.chol_bound(Nn, ex)
    print(f"basis {impl} Nn={Nn} {grid} rho={rho} conv={conv}: kappa2 {ex.kappa:.2e} max|B| "
          f"{ex.bmax:.3g} err {err:.2e} = {err / bound:.3f} of the bound, "
          f"{err / (R.EPS * ex.kappa * ex.bmax):.3f} eps kappa2 max|B|")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_condition_numbers_of_the_table(case):
    """The kappa2 each case was chosen for, to a factor 3: a case cannot drift into another
    regime (well conditioned, at the gate, nugget-limited) unnoticed."""
    ex = case.exact(N_DEPTHS)
    assert case.kappa / 3 <= ex.kappa <= case.kappa * 3, (case.id, ex.kappa)


@pytest.mark.parametrize("design", R.DESIGNS, ids=lambda d: f"Nn{d[0]}-{d[1][:3]}-rho{d[2]}-c{d[3]}")
def test_interpolation_at_the_control_points(design):
    """At a control point K(x~, g) is a row of K(g, g), so the exact basis row is
    e_k - nugget (K + nugget I)^-1 e_k: the unit vector up to nugget ||K^-1||.  Checked on the
    exact basis independently of how it was computed (||K^-1||_2 <= kappa2 / ||K||_2 and
    ||K||_2 >= 1, the diagonal), and the library's basis agrees there within its bound."""
    Nn, grid, rho, conv = design
    xg = M.gp_grid(Nn, grid)
    # depths that are their own normalised image: the range ends 0 and 1 first and last
    x = np.concatenate([[0.0], xg, [1.0]])
    assert np.array_equal(M.normalize_depth(x)[1:-1], xg)
    ex = R.exact_basis(x, Nn, grid, rho, conv)
    unit = ex.B[1:-1] - np.eye(Nn)
    # nugget ||K^-1|| <= min(1, nugget kappa2); the control points as doubles sit eps / 2 from
    # the rationals, which moves a kernel row by at most eps / rho per entry
    slack = min(1.0, 1e-9 * ex.kappa) + Nn * R.EPS * ex.kappa / rho
    assert np.abs(unit).max() <= slack, (np.abs(unit).max(), slack)
    if ex.kappa < 1e3:       # the deviation is then the nugget term itself, visibly not zero
        assert 1e-10 < np.abs(unit).max()
    t0, S0 = default_prior()
    prob = ExpGPProblem(x, x, 1 + 0 * x, Nn=Nn, gridType=grid, rho=rho, theta0=t0, Sigma0=S0,
                        kernel_conv=conv)
    B, xgl = prob.basis()
    np.testing.assert_allclose(xgl, ex.xGP, rtol=0, atol=2 * R.EPS)
    assert np.abs(B - ex.B).max() <= R.chol_bound(Nn, ex)


# ---- rho_scale -> fitoct_problem.rho ---------------------------------------------------------
class _Captured(Exception):
    pass


def _capture_sample(monkeypatch):
    seen = {}

    def fake_sample(prob, cfg, progress=None, resume=None):
        seen["rho"] = prob.to_c().rho
        raise _Captured

    monkeypatch.setattr(api, "sample", fake_sample)
    return seen


@pytest.mark.parametrize("r", [0.03, 0.15, 0.5, 1.0])
def test_fitexpgp_passes_rho_scale_unchanged(monkeypatch, r):
    seen = _capture_sample(monkeypatch)
    d = synth_decay(64, "sincExp", 1)
    t0, _ = default_prior()
    with pytest.raises(_Captured):
        api.fitExpGP(d["x"], d["y"], d["uy"], Nn=8, theta0=t0, rho_scale=r, refresh=0)
    assert seen["rho"] == r


def test_fitexpgp_rho_scale_zero_is_one_over_nn(monkeypatch):
    """rho_scale = 0 (FitOCT.R:119): fitoct_problem.rho = 0, which the library reads as 1/Nn:
    the basis it builds is bit for bit the one of rho = 1/Nn."""
    seen = _capture_sample(monkeypatch)
    d = synth_decay(64, "sincExp", 1)
    t0, _ = default_prior()
    with pytest.raises(_Captured):
        api.fitExpGP(d["x"], d["y"], d["uy"], Nn=8, theta0=t0, rho_scale=0, refresh=0)
    assert seen["rho"] == 0.0
    p0 = ExpGPProblem(d["x"], d["y"], d["uy"], Nn=8, rho=0.0)
    p1 = ExpGPProblem(d["x"], d["y"], d["uy"], Nn=8, rho=1.0 / 8)
    p2 = ExpGPProblem(d["x"], d["y"], d["uy"], Nn=8, rho=0.3)
    assert np.array_equal(p0.basis()[0], p1.basis()[0])
    assert not np.array_equal(p0.basis()[0], p2.basis()[0])
    assert np.array_equal(nuts_c.basis(p0), nuts_c.basis(p1))


@pytest.mark.parametrize("r,want", [(0.03, 0.03), (0.15, 0.15), (0.5, 0.5), (0, 1.0 / 12),
                                    (None, 1.0 / 12)])
def test_pipeline_passes_rho_scale(r, want):
    d = synth_decay(64, "sincExp", 1)
    t0, S0 = default_prior()
    res = pipeline.FileResult("f", d["x"], d["y"], {"uy": d["uy"]}, {}, {},
                              prior={"theta0": t0, "Sigma0": S0})
    ctrl = pipeline.load_ctrl(rho_scale=r, Nn=12)
    p = pipeline._gp_problem(res, ctrl, 0, "normal")
    assert p.to_c().rho == want
    assert pipeline.load_ctrl()["rho_scale"] == 0.1          # FitOCT.R:47
    # the struct field is a plain double at the offset the library reads
    c = p.to_c()
    B = np.zeros((p.N, p.Nn))
    assert _lib.lib().fitoct_build_basis(C.byref(c), _lib.dptr(B), None) == 0
    ref, _ = M.gp_basis(p.x, 12, p.gridType, want)
    ex = R.exact_basis(p.x, 12, p.gridType, want)
    assert np.abs(B - ref).max() <= 2 * R.chol_bound(12, ex)
