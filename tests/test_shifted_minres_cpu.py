"""Shifted MINRES on the CPU: the NumPy twin (``eigensolvers_amd.shifted_minres.shifted_minres_host``) - the
specification of the device kernels - against dense solves, and FEAST's vector-major path driven by the twin.

Shifts: the 8 upper-half-plane points of the 16-node Legendre contour on [-0.21, 0.21] (the recipe of
``test_feast_at_the_reference_comparable_inner_tolerance``) plus one real shift in the gap between the operator's
mid-spectrum cluster (|lambda| <= 0.2) and the rest of its spectrum (|lambda| >= 1)."""
import numpy as np
import pytest
import scipy.sparse as sp

import eigensolvers_amd as ea
from conftest import load_golden
from eigensolvers_amd import feast as pf
from eigensolvers_amd.shifted_minres import shifted_minres_host
from oracle.numpy_vector import RefVector

EPS = np.finfo(float).eps
REAL_SHIFT = 0.5
TOLS = [(1e-5, 1e-7), (1e-10, 1e-12)]


def contour_shifts():
    gk, _ = pf.quadraturePointsWeights(16, "legendre", positiveHalf=True)
    return [pf.contour_point(-0.21, 0.21, g)[1] for g in gk]


SHIFTS = contour_shifts() + [REAL_SHIFT]


def residual_bound(H, z, x, target):
    """The issue's bound: 1.01 * target plus the rounding of the check's own product."""
    hinf = abs(H).sum(axis=1).max()
    return 1.01 * target + 100 * EPS * (abs(z) + hinf) * np.linalg.norm(x)


def true_residual(H, b, z, x, sign):
    return np.linalg.norm(b - sign * (z * x - H @ x))


@pytest.fixture(scope="module")
def small():
    g = load_golden("feast_n100.npz")
    A = np.array(g["A"], dtype=float)
    b = np.random.default_rng(9).standard_normal(A.shape[0])
    return A, b / np.linalg.norm(b), np.linalg.eigvalsh(A)


@pytest.fixture(scope="module")
def rhs4000():
    b = np.random.default_rng(9).standard_normal(4000)
    return b / np.linalg.norm(b)


@pytest.mark.parametrize("rtol,atol", TOLS)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_twin_against_dense_solves_n100(small, sign, rtol, atol):
    A, b, lam = small
    # the contour of the tests above and the one around this problem's own window [160, 166]
    gk, _ = pf.quadraturePointsWeights(16, "legendre", positiveHalf=True)
    own = [pf.contour_point(160.0, 166.0, g)[1] for g in gk]
    for shifts in (SHIFTS, own):
        x, its, est, conv = shifted_minres_host(lambda v: A @ v, b, shifts, rtol, atol, 1000, sign)
        target = max(atol, rtol * np.linalg.norm(b))
        assert conv.all() and np.all(est <= target) and np.isfinite(x).all()
        for j, z in enumerate(shifts):
            res = true_residual(A, b, z, x[j], sign)
            assert res <= residual_bound(A, z, x[j], target), (z, res, target)
            exact = np.linalg.solve(sign * (z * np.eye(len(b)) - A), b.astype(complex))
            # error <= residual / distance to the spectrum
            assert np.linalg.norm(x[j] - exact) <= 10 * target / np.min(np.abs(z - lam)), (z, its[j])


@pytest.mark.parametrize("rtol,atol", TOLS)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_twin_residuals_on_the_generated_operator(gapped4000, rhs4000, sign, rtol, atol):
    H, b = gapped4000[0], rhs4000
    x, its, est, conv = shifted_minres_host(lambda v: H @ v, b, SHIFTS, rtol, atol, 4000, sign)
    target = max(atol, rtol)
    assert conv.all() and np.all(est <= target)
    for j, z in enumerate(SHIFTS):
        res = true_residual(H, b, z, x[j], sign)
        print(f"sign {sign:+.0f} rtol {rtol:g} z {z:.4f} its {its[j]} estimate {est[j]:.3e} true {res:.3e}")
        assert res <= residual_bound(H, z, x[j], target), (z, res, target)


def test_one_run_serves_all_shifts(gapped4000, rhs4000):
    H, b = gapped4000[0], rhs4000
    calls = [0]

    def matvec(v):
        calls[0] += 1
        return H @ v

    x, its, est, conv = shifted_minres_host(matvec, b, SHIFTS, 1e-5, 1e-7, 4000)
    assert calls[0] == its.max()                        # the products of the run = the slowest shift's steps
    assert len(set(its.tolist())) > 1                   # the shifts do stop at different steps
    for j in (0, 3, 7, 8):
        x1, it1, est1, conv1 = shifted_minres_host(lambda v: H @ v, b, [SHIFTS[j]], 1e-5, 1e-7, 4000)
        assert it1[0] == its[j] and est1[0] == est[j]
        assert np.array_equal(x1[0], x[j])              # the Lanczos run does not see the shifts: bit for bit


def test_breakdown_ends_in_one_step_with_the_exact_answer():
    h = np.linspace(-1.0, 1.0, 64)
    H = sp.diags(h).tocsr()
    b = np.zeros(64)
    b[3] = 2.0
    for sign in (1.0, -1.0):
        x, its, est, conv = shifted_minres_host(lambda v: H @ v, b, SHIFTS, 1e-10, 1e-12, 100, sign)
        assert np.all(its == 1) and conv.all() and np.all(est == 0.0)
        assert np.isfinite(x).all()
        for j, z in enumerate(SHIFTS):
            exact = sign * 2.0 / (z - h[3])
            assert abs(x[j, 3] - exact) <= 4 * EPS * abs(exact)
            assert np.count_nonzero(x[j]) == 1


def test_maxiter_leaves_every_shift_unconverged(gapped4000, rhs4000):
    H, b = gapped4000[0], rhs4000
    x, its, est, conv = shifted_minres_host(lambda v: H @ v, b, SHIFTS, 1e-12, 0.0, 5)
    assert not conv.any() and np.all(its == 5) and np.all(est > 1e-12)


def test_zero_right_hand_side():
    x, its, est, conv = shifted_minres_host(lambda v: v, np.zeros(7), SHIFTS[:2], 1e-5, 1e-7, 10)
    assert not x.any() and not its.any() and conv.all()


class TwinVector(RefVector):
    """The oracle's ndarray vector with the shared-Lanczos hook, so that the driver's vector-major path runs on the CPU."""
    calls = []

    @staticmethod
    def _solve_shifts(H, b, shifts, reverseGF=False):
        o = b.options["linearSystemArgs"]
        x, its, est, conv = shifted_minres_host(lambda v: H @ v, b.array, shifts, o["linear_tol"], o["linear_atol"],
                                                o["linearIter"], -1.0 if reverseGF else 1.0)
        TwinVector.calls.append(len(shifts))
        b.last_solve_stats = {"iterations": [int(i) for i in its], "estimates": [float(e) for e in est],
                              "products": int(its.max())}
        if not conv.all():
            raise UserWarning("Warning:: Iterative solver is not converged ")
        return [RefVector(x[j], b.options) for j in range(len(shifts))]


ea.AbstractVector.register(TwinVector)


def test_feast_vector_major_path_on_the_twin():
    """The golden run (gcrotmk at rtol 1e-2) stalls at its inner tolerance and answers to the reference's unit test:
    every eigenvalue of the window to 1e-4 absolute (test_feast_cpu.py, ``abs(e - nearest) <= 1e-4``).  That is the
    tolerance the golden values carry, so it is the one they are compared with here; the exact eigenvalues too."""
    g = load_golden("feast_n100.npz")
    A = g["A"]
    o = {"linearSystemArgs": {"linearSolver": "minres_shifted", "linearIter": 1000, "linear_tol": 1e-6, "linear_atol": 1e-10}}
    Y = [TwinVector(g["guess"][:, i].copy(), o) for i in range(6)]
    TwinVector.calls.clear()
    ev, Yf, st = pf.feastDiagonalization(A, Y, 8, "legendre", 160.0, 166.0, 1e-10, 20, writeOut=False)
    assert st["converged"]
    gold = pf.select_within_range(np.asarray(g["ev"]), 160.0, 166.0)[0]
    mine = pf.select_within_range(ev, 160.0, 166.0)[0]
    exact = pf.select_within_range(np.linalg.eigvalsh(A), 160.0, 166.0)[0]
    assert len(mine) == len(gold) == len(exact)
    np.testing.assert_allclose(mine, gold, rtol=0, atol=1e-4)
    np.testing.assert_allclose(mine, exact, rtol=0, atol=1e-4)
    rec = st["sharedLanczos"]
    assert len(rec) == st["outerIter"] + 1
    nvec = [6] + [int(g["nvec"])] * (len(rec) - 1)
    assert [r["solves"] for r in rec] == nvec[:len(rec)]
    assert len(TwinVector.calls) == sum(r["solves"] for r in rec)
    assert all(c == 4 for c in TwinVector.calls)                # 8 nodes = 4 contour points, all in one call
    for r in rec:
        assert len(r["products"]) == r["solves"] and len(r["iterations"]) == len(r["pairs"]) == 4 * r["solves"]
        assert all(p == max(i for (k, v), i in zip(r["pairs"], r["iterations"]) if v == vec)
                   for vec, p in enumerate(r["products"]))


def test_contour_pool_and_shared_lanczos_exclude_each_other():
    g = load_golden("feast_n100.npz")
    o = {"linearSystemArgs": {"linearSolver": "minres_shifted"}}
    Y = [TwinVector(g["guess"][:, i].copy(), o) for i in range(6)]
    with pytest.raises(ValueError):
        pf.feastDiagonalization(g["A"], Y, 8, "legendre", 160.0, 166.0, 1e-10, 2, writeOut=False, contourPool=True)


def test_the_default_path_is_untouched_without_the_solver_name():
    g = load_golden("feast_n100.npz")
    o = {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 1000, "linear_tol": 1e-2}}
    Y = [TwinVector(g["guess"][:, i].copy(), o) for i in range(6)]
    TwinVector.calls.clear()
    ev, Yf, st = pf.feastDiagonalization(g["A"], Y, 8, "legendre", 160.0, 166.0, 1e-10, 20, writeOut=False)
    assert "sharedLanczos" not in st and not TwinVector.calls
    np.testing.assert_allclose(ev, g["ev"], rtol=1e-9)
