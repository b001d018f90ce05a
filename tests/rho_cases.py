"""The GP length scale rho (fitoct_problem.rho: FitOCT.R's rho_scale, the Shiny app's slider)
away from its default 1/Nn: an exact basis and the table of cases shared by the CPU tests of
the three double-precision bases (test_basis_rho.py) and the GPU tests of lp and grad lp
(test_gpu_rho.py).  No GPU is needed to import or use this module.

rho decides which sweep a plan runs (the factorised basis K = a t^l b of build_poly, or
basis rows), which moments path (geo_ratios' guards), the dynamic range of the factors and
the conditioning of K(xGP, xGP) + nugget I.  Every case carries the route it is expected to
take; the expectations were derived from the guards' own formulas (length
scale) and each sits at least a decade from the gate or guard it depends on."""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction

import mpmath
import numpy as np

from fitoct_amd import ExpGPProblem
from fitoct_amd.synth import default_prior, synth_decay
from oracle import model_np as M

DPS = 60                              # decimal digits of the exact basis
FRAC_BITS = 256                       # fixed point of the final product (77 digits)
EPS = float(np.finfo(np.float64).eps)
POLY, ROWS = 0, 1                     # fitoct_plan_info::basis_mode


@dataclass(frozen=True)
class Exact:
    B: np.ndarray        # [N, Nn] the exact basis, rounded once to double
    kappa: float         # 2-norm condition number of the double K(xGP, xGP) + nugget I
    bmax: float          # max |B|
    E: float             # exponent range of the factorised evaluation a t^l b_l
    xGP: np.ndarray      # the control points, rounded to double


_exact = {}


def _grid(Nn, grid):
    """Control points as exact rationals (server.R:627-631)."""
    if grid == "extremal":
        return [Fraction(k, Nn - 1) for k in range(Nn)]
    dx = Fraction(1, Nn + 1)
    return [dx / 2 + (1 - dx) * Fraction(k, Nn - 1) for k in range(Nn)]


def _mpq(fr):
    return mpmath.mpf(fr.numerator) / mpmath.mpf(fr.denominator)


def _fixed(v):
    """mpf -> integer of FRAC_BITS fractional bits (truncated: 2^-256 relative to O(1))."""
    return int(mpmath.floor(mpmath.ldexp(v, FRAC_BITS)))


def exact_basis(x, Nn, grid, rho, kernel_conv=0, nugget=1e-9) -> Exact:
    """B = K(x~, g) (K(g, g) + nugget I)^-1 in 60-digit arithmetic (mpmath), rounded once to
    double: x~ the normalised depths of the doubles x, g the control points as exact
    rationals, s2 = rho^2 (kernel_conv 0: exp(-d^2 / (2 rho^2))) or rho^2 / 2 (kernel_conv 1:
    exp(-(d / rho)^2)) from the doubles rho and nugget.  The kernel values and the inverse
    are mpmath's; the final N x Nn x Nn product is formed on their 256-bit fixed-point images
    with Python integers, which is exact but for the 2^-256 of the images.  Cached per case."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    rho = float(rho) if rho else 1.0 / Nn
    key = (x.tobytes(), int(Nn), grid, rho, int(kernel_conv), float(nugget))
    if key in _exact:
        return _exact[key]
    with mpmath.workdps(DPS):
        mp = mpmath.mpf
        lo, hi = mp(float(x.min())), mp(float(x.max()))
        xt = [(mp(float(v)) - lo) / (hi - lo) for v in x]
        g = [_mpq(f) for f in _grid(Nn, grid)]
        s2 = mp(rho) ** 2 if kernel_conv == 0 else mp(rho) ** 2 / 2
        inv2s2 = 1 / (2 * s2)
        K = mpmath.matrix(Nn, Nn)
        for i in range(Nn):
            for j in range(Nn):
                K[i, j] = mpmath.exp(-(g[i] - g[j]) ** 2 * inv2s2) + (mp(float(nugget)) if i == j else 0)
        Kinv = mpmath.inverse(K)
        resid = mpmath.mnorm(K * Kinv - mpmath.eye(Nn), 1)
        assert resid < mp(10) ** -30, resid           # the inverse itself, to 30 digits
        Ki = np.array([[_fixed(Kinv[l, k]) for k in range(Nn)] for l in range(Nn)], dtype=object)
        Kx = np.array([[_fixed(mpmath.exp(-(u - gl) ** 2 * inv2s2)) for gl in g] for u in xt],
                      dtype=object)
        P = Kx.dot(Ki)                                # Python integers: exact
        B = np.array([[float(mpmath.ldexp(mp(int(v)), -2 * FRAC_BITS)) for v in row] for row in P])
        xg = np.array([float(v) for v in g])
    # the double matrix whose Cholesky factor every double-precision basis solves with
    d = xg[:, None] - xg[None, :]
    s2d = rho * rho if kernel_conv == 0 else 0.5 * rho * rho
    kappa = float(np.linalg.cond(np.exp(-d * d / (2 * s2d)) + nugget * np.eye(Nn), 2))
    # la, lt as build_poly forms them: a = exp(la), t = exp(lt), b_l = exp(-(l dg)^2 / (2 s2))
    g0, dg = xg[0], float(_grid(Nn, grid)[1] - _grid(Nn, grid)[0])
    u = M.normalize_depth(x) - g0
    E = float(np.max(u * u) / (2 * s2d) + (Nn - 1) * np.max(np.abs(u)) * dg / s2d
              + ((Nn - 1) * dg) ** 2 / (2 * s2d))
    B.setflags(write=False)
    xg.setflags(write=False)
    out = _exact[key] = Exact(B, kappa, float(np.abs(B).max()), E, xg)
    return out


@dataclass(frozen=True)
class RhoCase:
    id: str
    N: int
    family: str
    Nn: int
    grid: str
    rho: float
    conv: int
    kappa: float          # the condition number the case was chosen for (order of magnitude)
    mode: object          # expected basis_mode; None: not asserted
    bpt: object           # expected bins_per_thread
    tier: str             # "exact": tier 1; "rows": tier 2, own basis; "bracket": tier 2, bracket
    draw: int             # which draw of nine points the case uses (see points)

    def data(self):
        return synth_decay(self.N, "sincExp", self.N + 3)

    def kw(self):
        t0, S0 = default_prior()
        return dict(Nn=self.Nn, theta0=t0, Sigma0=S0, kernel_conv=self.conv, rho=self.rho)

    def problem(self, B=None):
        """The library's problem; B = None leaves the basis and the route to the library."""
        d = self.data()
        return ExpGPProblem(d["x"], d["y"], d["uy"], gridType=self.grid, prior_type=self.family,
                            B=B, **self.kw())

    def reference(self, B):
        """The numpy model on the basis it is handed."""
        d = self.data()
        return M.Problem(d["x"], d["y"], d["uy"], grid_type=self.grid,
                         family=M.FAMILIES[self.family], B=np.array(B), **self.kw())

    def exact(self, N=None):
        """The exact basis at the case's depths, or at N depths of the same range."""
        x = self.data()["x"] if N is None else synth_decay(N, "sincExp", N + 3)["x"]
        return exact_basis(x, self.Nn, self.grid, self.rho, self.conv)

    def points(self, bmax, P=9, spread=0.3):
        """Nine points as test_gpu_logp._points draws them, the yGP block (for the horseshoe
        its z factor, which enters yGP linearly) scaled by 1 / max(1, max|B|) so that
        1 + B yGP stays positive where the basis overshoots.  That scaling alone still leaves
        one point in ten or so with 1 + dL <= 0 somewhere (lp = -inf: nothing to compare), so
        a case's points are draw number ``draw`` of the generator seeded N + Nn + 1000 draw:
        the first draw whose nine points all have a finite lp on the exact basis, found once
        with the numpy model and fixed in the table (min(1 + dL) >= 0.029 over all of them;
        the tests assert that every reference value is finite)."""
        t0, _ = default_prior()
        D = M.dim(M.FAMILIES[self.family], self.Nn)
        rng = np.random.default_rng(self.N + self.Nn + 1000 * self.draw)
        q = rng.normal(0, spread, (P, D))
        q[:, 0:3] = np.log(t0) + rng.normal(0, 0.02, (P, 3))
        q[:, -1] = rng.normal(0, 0.3, P)
        q[:, 3:3 + self.Nn] /= max(1.0, bmax)
        return q


def _c(id, N, family, Nn, grid, rho, conv, kappa, mode, bpt, tier, draw):
    return RhoCase(id, N, family, Nn, {"int": "internal", "ext": "extremal"}[grid], rho, conv,
                   kappa, mode, bpt, tier, draw)


CASES = [
    # tier 1: kappa <= 1e4, exact basis, the suite's tolerances, both precisions
    _c("wide_poly4", 700, "normal", 10, "int", 0.15, 0, 4e3, POLY, 4, "exact", 6),
    _c("narrow_poly8", 2047, "lasso", 15, "ext", 0.05, 0, 5, POLY, 8, "exact", 0),       # t^14 ~ e^400
    _c("narrow_geo16", 3001, "horseshoe", 15, "ext", 0.05, 0, 5, POLY, 16, "exact", 2),  # geo guard 512 / 600
    _c("narrow_nogeo", 3001, "horseshoe", 15, "ext", 0.045, 0, 3, POLY, 0, "exact", 2),  # geo guard 632 > 600
    _c("overflow_rows", 1000, "normal", 15, "ext", 0.03, 0, 1.3, ROWS, 0, "exact", 0),   # lt 14 = 1111 > 650
    _c("narrow_resident", 300, "normal", 15, "ext", 0.03, 0, 1.3, ROWS, 2, "exact", 0),
    _c("conv1_poly", 700, "normal", 10, "ext", 0.20, 1, 5e2, POLY, 4, "exact", 0),       # s2 = rho^2 / 2
    _c("nn24_poly", 700, "horseshoe", 24, "int", 0.05, 0, 5e2, POLY, 4, "exact", 2),     # NNP 24, t^23 ~ e^377
    _c("few_wide", 1000, "lasso", 5, "ext", 0.5, 0, 3e3, POLY, 4, "exact", 0),
    _c("r01_2048", 2048, "horseshoe", 15, "ext", 0.1, 0, 4e3, POLY, 8, "exact", 2),      # FitOCT.R's default rho
    # tier 2
    _c("streamed_wide", 8192, "normal", 10, "ext", 0.2, 0, 6e4, POLY, 0, "bracket", 1),
    _c("ill_rows", 1000, "normal", 15, "int", 0.3, 0, 9e9, ROWS, 0, "rows", 1),          # gate refuses
    _c("ill_resident", 300, "normal", 15, "int", 0.3, 0, 9e9, ROWS, 2, "rows", 0),
    _c("ill_nn20", 700, "lasso", 20, "ext", 0.15, 0, 7e9, ROWS, 0, "rows", 2),
    _c("ill_nn24", 97, "horseshoe", 24, "ext", 0.1, 0, 2e9, ROWS, 0, "rows", 2),
    _c("at_gate", 700, "normal", 12, "int", 0.19, 0, 1.2e7, None, None, "bracket", 6),   # route recorded
]
BY_ID = {c.id: c for c in CASES}

# every (Nn, grid, rho, conv) of the table once
DESIGNS = sorted({(c.Nn, c.grid, c.rho, c.conv) for c in CASES})


def chol_bound(Nn, ex: Exact):
    """Forward-error bound of a Cholesky solve with the (Nn x Nn) matrix, per entry of B:
    (3 Nn + 1) eps kappa2 max|B| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd
    ed., Thm 10.4 with gamma_{3n+1})."""
    return (3 * Nn + 1) * EPS * ex.kappa * ex.bmax
