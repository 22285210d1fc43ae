"""Bounds and checks shared by the device tests of the single-vector operator sweeps (``test_gpu_stream_layout.py``,
``test_gpu_parity.py``, ``test_gpu_precond_minres.py``, ``test_gpu_shifted_minres.py``, ``test_gpu_sweep_two_launches.py``).
A plain module, imported as ``_block_cases`` is: no fixtures, no tests.  Every bound is stated where it is defined."""
import numpy as np

from eigensolvers_amd import feast as pf

EPS = np.finfo(float).eps


# ---------------------------------------------------------------- products
def product_bound(A, x):
    """Per-row bound of a product in any summation order: 4e-14 of the row's absolute sum."""
    return 4e-14 * (abs(A) @ np.abs(x)) + 1e-300


def fixed_point_term(A, x):
    """What the fixed-point accumulators (layout 5) add to ``product_bound``: 40 units of 2^-60 of max_i sum_j |a_ij| max|x|."""
    return 40 * 2.0 ** -60 * abs(A).sum(axis=1).max() * np.max(np.abs(x))


# ---------------------------------------------------------------- plain MINRES
def minres_opts(it=2000, tol=1e-10, **extra):
    d = {"linearSystemArgs": {"linearSolver": "minres", "linearIter": it, "linear_tol": tol}}
    d.update(extra)
    return d


def check_kernel_forms(label, fixed_order, x2, s2, x3, s3, xo, itn, istop):
    """KD riding on the next sweep (``x2``, ``s2``) against KD as its own kernel (``x3``, ``s3``) and against the oracle
    (``xo``, ``itn``, ``istop``): counts and stop codes equal, the two forms within 1e-7 ||x|| of each other and 1e-6 ||x|| of
    the oracle, and bit for bit where the layout fixes the order of a row's adds (``fixed_order``: layouts 1, 2, 3, 5
    without column splits; a scalar's summation tree does not depend on which kernel's prologue reduces it, common.h
    block_sum_partials)."""
    assert s2["iterations"] == s3["iterations"] == itn and s2["istop"] == s3["istop"] == istop, label
    scale = np.linalg.norm(xo)
    assert np.linalg.norm(x2 - x3) <= 1e-7 * scale, label                       # variant 4 adds a row in varying order
    assert np.linalg.norm(x2 - xo) <= 1e-6 * scale, label
    if fixed_order:
        np.testing.assert_array_equal(x2, x3)


# ---------------------------------------------------------------- Jacobi-preconditioned MINRES
def within(got, ref, bound):
    err = np.abs(np.asarray(got) - np.asarray(ref))
    assert (err <= bound).all(), f"max excess {np.max(err - bound):.3e}, {int((err > bound).sum())} elements"


def check_against_twin(label, Hh, b, sigma, rtol, W, tw, sign=1.0):
    """The solve ``W`` against the NumPy twin ``tw`` (``_precond_cases.twin``): iterations and istop equal, x within
    max(1e-9, 100 rtol) ||x||, rnorm within 5 %, Anorm within 1e-3, true residual <= 1.05 x the twin's + 1e-13."""
    xo, info, itn, istop, trace = tw
    st = W.last_solve_stats
    x = W.array
    r = np.linalg.norm(b - sign * (sigma * x - Hh @ x))
    ro = np.linalg.norm(b - sign * (sigma * xo - Hh @ xo))
    print(f"PMR {label}: iterations {st['iterations']} (twin {itn}), istop {st['istop']} ({istop}), |x - twin| / |x| = "
          f"{np.linalg.norm(x - xo) / np.linalg.norm(xo):.2e}, rnorm {st['rnorm']:.3e} ({trace[-1]['rnorm']:.3e}), Anorm "
          f"{st['Anorm']:.6e} ({trace[-1]['Anorm']:.6e}), true residual {r:.3e} ({ro:.3e})")
    assert st["preconditioner"] == "jacobi"
    assert st["iterations"] == itn and st["istop"] == istop
    within(x, xo, max(1e-9, 100 * rtol) * np.linalg.norm(xo))
    assert abs(st["rnorm"] - trace[-1]["rnorm"]) <= 0.05 * trace[-1]["rnorm"]
    assert r <= 1.05 * ro + 1e-13
    assert abs(st["Anorm"] - trace[-1]["Anorm"]) <= 1e-3 * trace[-1]["Anorm"]


# ---------------------------------------------------------------- shifted MINRES
REAL_SHIFT = 0.5


def contour_shifts():
    gk, _ = pf.quadraturePointsWeights(16, "legendre", positiveHalf=True)
    return [pf.contour_point(-0.21, 0.21, g)[1] for g in gk]


CONTOUR = contour_shifts()
SHIFT_SETS = {1: [CONTOUR[7]], 3: [CONTOUR[0], REAL_SHIFT, CONTOUR[5]], 8: CONTOUR[:3] + [REAL_SHIFT] + CONTOUR[4:],
              9: CONTOUR + [REAL_SHIFT]}                      # 9: two calls of the C entry (8 + 1)


def shifted_options(rtol, atol, maxiter=4000):
    return {"linearSystemArgs": {"linearSolver": "minres_shifted", "linearIter": maxiter, "linear_tol": rtol,
                                 "linear_atol": atol}}


def residual_bound(Hh, z, x, target):
    hinf = abs(Hh).sum(axis=1).max()
    return 1.01 * target + 100 * EPS * (abs(z) + hinf) * np.linalg.norm(x)


def true_residual(Hh, b, z, x, sign):
    return np.linalg.norm(b - sign * (z * x - Hh @ x))


def check_residuals(Hh, b, shifts, xs, sign, rtol, atol):
    target = max(atol, rtol * np.linalg.norm(b))
    for z, x in zip(shifts, xs):
        xa = x.array
        assert xa.dtype == np.complex128 and np.isfinite(xa).all()
        res = true_residual(Hh, b, z, xa, sign)
        assert res <= residual_bound(Hh, z, xa, target), (z, res, target)
