"""The NumPy twin of the Jacobi-preconditioned MINRES against SciPy itself (``scipy.sparse.linalg.minres(A, b, M=...)``),
and the host statement of the preconditioner.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _precond_cases as pc
from eigensolvers_amd.generators import gapped_csr_host
from eigensolvers_amd.hip_vector import _preconditioner
from eigensolvers_amd.precond_minres import csr_diagonal_host, jacobi_inverse_host, minres_jacobi_host


def _scipy_with_m(H, b, sigma, minv, rtol, maxiter):
    n = len(b)
    A = spla.LinearOperator((n, n), matvec=pc.shifted(H, sigma), dtype=np.float64)
    calls = []
    x, info = spla.minres(A, b, M=sp.diags(minv), rtol=rtol, maxiter=maxiter, callback=lambda xk: calls.append(1))
    return x, info, len(calls)


def _plain_count(H, b, sigma, rtol, maxiter):
    n = len(b)
    calls = []
    spla.minres(spla.LinearOperator((n, n), matvec=pc.shifted(H, sigma), dtype=np.float64), b, rtol=rtol, maxiter=maxiter,
                callback=lambda xk: calls.append(1))
    return len(calls)


@pytest.fixture(scope="module")
def gapped16():
    return gapped_csr_host(4000, 16, seed=7), pc.unit_guess(4000)


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
def test_twin_equals_scipy_on_the_gapped_operator(gapped16, rtol):
    H, b = gapped16
    minv = jacobi_inverse_host(csr_diagonal_host(H), pc.SIGMA)
    xs, info, calls = _scipy_with_m(H, b, pc.SIGMA, minv, rtol, 2000)
    x, tinfo, itn, istop = minres_jacobi_host(pc.shifted(H, pc.SIGMA), b, minv, rtol=rtol, maxiter=2000)
    print(f"rtol {rtol:g}: SciPy {calls} iterations, twin {itn}, |x - x_scipy| / |x| = {np.linalg.norm(x - xs) / np.linalg.norm(xs):.2e}")
    assert info == 0 and tinfo == 0 and istop in (1, 2)
    assert itn == calls
    assert np.linalg.norm(x - xs) <= 1e-12 * np.linalg.norm(xs)
    if rtol == 1e-10:
        plain = _plain_count(H, b, pc.SIGMA, rtol, 2000)
        print(f"plain MINRES: {plain} iterations")
        assert itn == 17 and plain > 20 * itn            # the operator class this preconditioner is for


def test_twin_equals_scipy_on_the_dense_matrix_where_jacobi_buys_nothing():
    A = pc.dense_operator()
    b = pc.unit_guess(100)
    minv = jacobi_inverse_host(np.diag(A), pc.DENSE_SIGMA)
    xs, info, calls = _scipy_with_m(A, b, pc.DENSE_SIGMA, minv, 1e-8, 2000)
    x, tinfo, itn, istop = minres_jacobi_host(pc.shifted(A, pc.DENSE_SIGMA), b, minv, rtol=1e-8, maxiter=2000)
    plain = _plain_count(A, b, pc.DENSE_SIGMA, 1e-8, 2000)
    print(f"dense n = 100: SciPy with M {calls} iterations, twin {itn}, plain {plain}")
    assert info == 0 and tinfo == 0
    assert itn == calls
    assert np.linalg.norm(x - xs) <= 1e-12 * np.linalg.norm(xs)
    assert itn > 0.8 * plain                              # no diagonal dominance: nothing gained


@pytest.mark.parametrize("sigma,rtol", pc.DENSE_CASES)
def test_twin_is_determinate_at_the_shifts_of_the_device_tests_on_the_dense_matrix(sigma, rtol):
    """The device is compared with the twin on the dense matrix only where the twin does not depend on the order of the
    adds inside its own matrix product: three orders, same count, scalars and x equal to 1e-11 (observed: 1e-14)."""
    A = pc.dense_operator()
    b = pc.unit_guess(100)
    minv = jacobi_inverse_host(np.diag(A), sigma)
    C, At = sp.csr_matrix(A), np.ascontiguousarray(A.T)
    runs = []
    for mv in (lambda v: sigma * v - A @ v, lambda v: sigma * v - C @ v, lambda v: sigma * v - At.T @ v):
        tr = []
        x, info, itn, istop = minres_jacobi_host(mv, b, minv, rtol=rtol, maxiter=2000, trace=tr)
        runs.append((x, itn, istop, tr[-1]))
    x0, itn0, istop0, t0 = runs[0]
    assert itn0 < 60 and istop0 == 1
    for x, itn, istop, t in runs[1:]:
        assert (itn, istop) == (itn0, istop0)
        assert abs(t["Anorm"] - t0["Anorm"]) <= 1e-11 * t0["Anorm"] and abs(t["rnorm"] - t0["rnorm"]) <= 1e-11 * t0["rnorm"]
        assert np.linalg.norm(x - x0) <= 1e-11 * np.linalg.norm(x0)


def test_twin_equals_scipy_with_an_exact_diagonal_hit():
    H, hit, zero = pc.exact_hit_operator()
    b = pc.unit_guess(4001)
    d = csr_diagonal_host(H)
    assert d[hit] == pc.SIGMA and d[zero] == 0.0
    minv = jacobi_inverse_host(d, pc.SIGMA)
    xs, info, calls = _scipy_with_m(H, b, pc.SIGMA, minv, 1e-10, 2000)
    x, tinfo, itn, istop = minres_jacobi_host(pc.shifted(H, pc.SIGMA), b, minv, rtol=1e-10, maxiter=2000)
    print(f"exact hit: SciPy {calls} iterations, twin {itn}")
    assert info == 0 and itn == calls
    assert np.linalg.norm(x - xs) <= 1e-12 * np.linalg.norm(xs)


def test_twin_stops_at_the_iteration_limit_and_on_a_zero_right_hand_side(gapped16):
    H, b = gapped16
    minv = jacobi_inverse_host(csr_diagonal_host(H), pc.SIGMA)
    trace = []
    x, info, itn, istop = minres_jacobi_host(pc.shifted(H, pc.SIGMA), b, minv, rtol=1e-10, maxiter=5, trace=trace)
    assert (info, itn, istop) == (5, 5, 6) and len(trace) == 5 and trace[-1]["istop"] == 6
    x, info, itn, istop = minres_jacobi_host(pc.shifted(H, pc.SIGMA), np.zeros(4000), minv, rtol=1e-10, maxiter=5)
    assert not x.any() and (info, itn, istop) == (0, 0, 0)


def test_diagonal_sums_duplicates_and_gives_zero_without_an_entry():
    #   row 0: (0,0) twice; row 1: no diagonal; row 2: one stored zero on the diagonal
    A = sp.csr_matrix((np.array([1.5, 0.25, 2.0, 3.0, 0.0, 4.0]), np.array([0, 0, 2, 0, 2, 1]), np.array([0, 3, 4, 6])),
                      shape=(3, 3))
    assert A.nnz == 6                                     # duplicates kept as separate stored elements
    np.testing.assert_array_equal(csr_diagonal_host(A), [1.75, 0.0, 0.0])
    H = gapped_csr_host(3001, 16, seed=3)
    np.testing.assert_allclose(csr_diagonal_host(H), H.diagonal(), rtol=1e-15, atol=0)


def test_jacobi_inverse_floor():
    d = np.array([1.0, -3.0, 0.02, 0.5])
    minv = jacobi_inverse_host(d, 0.02)                   # t = 0.98, 3.02, 0, 0.48; floor 1e-8 * 3.02
    assert np.isfinite(minv).all()
    np.testing.assert_array_equal(minv, 1.0 / np.array([abs(0.02 - 1.0), abs(0.02 + 3.0), 1e-8 * abs(0.02 + 3.0), abs(0.02 - 0.5)]))
    with pytest.raises(ValueError, match="not finite"):
        jacobi_inverse_host(d, 0.02, 0.0)
    np.testing.assert_array_equal(jacobi_inverse_host(d, 0.1, 0.0), 1.0 / np.abs(0.1 - d))      # no hit: floor 0 is fine
    np.testing.assert_array_equal(jacobi_inverse_host(d, 0.02, 0.5), 1.0 / np.maximum(np.abs(0.02 - d), 0.5 * abs(0.02 + 3.0)))
    for bad in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            jacobi_inverse_host(d, 0.02, bad)
    with pytest.raises(ValueError, match="not finite"):
        jacobi_inverse_host(np.array([1.0, np.nan]), 0.02)
    with pytest.raises(ValueError, match="not finite"):
        jacobi_inverse_host(np.array([0.02, 0.02]), 0.02)                # every t is 0: a relative floor has nothing to scale


def _lsa(**kw):
    d = {"linearSolver": "minres", "linearIter": 100, "linear_tol": 1e-8}
    d.update(kw)
    return d


def test_option_validation_without_a_context():
    assert _preconditioner(_lsa()) is None
    assert _preconditioner(_lsa(preconditioner=None, linearSolver="gcrotmk")) is None
    assert _preconditioner(_lsa(preconditioner="jacobi"), 0.02) == "jacobi"
    with pytest.raises(ValueError, match="jacobi"):
        _preconditioner(_lsa(preconditioner="ilu"))
    for name in ("gcrotmk", "pardiso"):
        with pytest.raises(ValueError, match="minres"):
            _preconditioner(_lsa(preconditioner="jacobi", linearSolver=name))
    for name in ("minres_shifted", "lanczos_filter"):
        with pytest.raises(ValueError, match="shift invariance"):
            _preconditioner(_lsa(preconditioner="jacobi", linearSolver=name))
    with pytest.raises(ValueError, match="real shift"):
        _preconditioner(_lsa(preconditioner="jacobi"), 0.02 + 0.1j)
    with pytest.raises(ValueError, match="preconditionerFloor"):
        _preconditioner(_lsa(preconditioner="jacobi", preconditionerFloor=-1e-3), 0.02)
    with pytest.raises(NotImplementedError, match="x0"):
        _preconditioner(_lsa(preconditioner="jacobi"), 0.02, x0=object())

    class Ctx:
        collectives = True
    with pytest.raises(NotImplementedError, match="one GPU"):
        _preconditioner(_lsa(preconditioner="jacobi"), 0.02, None, Ctx())
