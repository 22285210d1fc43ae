"""GCROT's diagonal right preconditioner on the CPU: the NumPy twin of ``minv`` against an extended-precision evaluation,
the composed solve (the unchanged solver on ``v -> A (minv v)``, then ``x = minv u``) against SciPy's own
``gcrotmk(A, b, M=...)`` through the three drivers, and the option's validator."""
import numpy as np
import pytest
import scipy.sparse as sp

import _gcrot_precond_cases as gc
from _gcrot_precond_cases import NumpyOps
from eigensolvers_amd import hip_vector as hv
from eigensolvers_amd import jacobi_inverse_z_host
from eigensolvers_amd.gcrotmk import gcrotmk_device, gcrotmk_device_block, gcrotmk_device_pool
from eigensolvers_amd.precond_minres import csr_diagonal_host


# ---------------------------------------------------------------- 1. the twin of minv
@pytest.mark.parametrize("z", [0.02, 0.02 + 1e-12j, 0.02 + 0.05j, 0.05])
def test_twin_stays_within_its_derived_bound_of_the_extended_precision_value(z):
    """On the exact-hit operator (b): per element, relative, with the bound ``minv_reference`` derives from the twin's own
    operations.  z = 0.02 meets the hit exactly (``1 / g``); z = 0.02 + 1e-12j leaves it 1e-12 away (floored, the phase
    -i kept); the stored zero is an ordinary element."""
    H, hit, zero = gc.operator_b()
    d = csr_diagonal_host(H)
    assert d[hit] == 0.02 and d[zero] == 0.0
    minv = jacobi_inverse_z_host(d, z, gc.FLOOR)
    assert minv.dtype == (np.complex128 if complex(z).imag != 0 else np.float64)
    re, im, rel, kind = gc.minv_reference(d, z, gc.FLOOR)
    ratio = gc.minv_error_ratio(minv, d, z, gc.FLOOR)
    print(f"\nminv twin, z = {z}: max error / bound {ratio:.3f}, classes {np.bincount(kind, minlength=3).tolist()}, "
          f"largest bound {rel.max() / gc.U:.2f} u")
    assert ratio <= 1.0
    g = gc.FLOOR * float(np.max(np.abs(complex(z) - d)))
    if z == 0.02:
        assert kind[hit] == 2 and minv[hit] > 0 and abs(minv[hit] * g - 1) < 1e-14
    elif z == 0.02 + 1e-12j:
        assert kind[hit] == 1 and minv[hit].real == 0.0 and minv[hit].imag < 0 and abs(abs(minv[hit]) * g - 1) < 1e-14
    else:
        assert np.all(kind == 0)
    assert kind[zero] == 0 and abs(minv[zero] * complex(z) - 1) < 1e-14            # the stored zero: 1 / z


def test_twin_floor_classes_and_refusals():
    """A small diagonal with every class for a real and a complex z, and where the twin refuses."""
    d = np.array([1.0, -3.0, 0.02, 0.02 + 1e-11, 0.02 - 1e-11, 0.5])
    for z in (0.02, 0.02 + 1e-12j):
        kind = gc.minv_reference(d, z, 1e-8)[3]
        assert kind.tolist() == ([0, 0, 2, 1, 1, 0] if z == 0.02 else [0, 0, 1, 1, 1, 0])
        assert gc.minv_error_ratio(jacobi_inverse_z_host(d, z, 1e-8), d, z, 1e-8) <= 1.0
    minv = jacobi_inverse_z_host(d, 0.02, 1e-8)
    g = 1e-8 * 3.02
    assert minv[3] < 0 and minv[4] > 0 and minv[2] > 0                       # sign kept under the floor: m = z - d
    np.testing.assert_allclose(np.abs(minv[2:5]), 1 / g, rtol=1e-15)
    np.testing.assert_array_equal(jacobi_inverse_z_host(d, 0.1, 0.0), 1.0 / (0.1 - d))          # no hit: floor 0 is fine
    for z in (0.02, 0.02 + 0j):
        with pytest.raises(ValueError, match="not finite"):
            jacobi_inverse_z_host(d, z, 0.0)                                   # floor 0 with the hit
    assert np.all(np.isfinite(jacobi_inverse_z_host(d, 0.02 + 1e-12j, 0.0)))      # off the axis nothing is hit
    for z in (0.02, 0.02 + 0.05j):
        with pytest.raises(ValueError, match="not finite"):
            jacobi_inverse_z_host(np.array([1.0, np.nan]), z)
        with pytest.raises(ValueError, match="not finite"):
            jacobi_inverse_z_host(np.array([1.0, np.inf]), z)
    with pytest.raises(ValueError, match="not finite"):
        jacobi_inverse_z_host(np.array([0.02, 0.02]), 0.02)                  # every t is 0: a relative floor has nothing to scale
    for bad in (-1e-3, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="floor"):
            jacobi_inverse_z_host(d, 0.02, bad)


# ---------------------------------------------------------------- 2. the composed solve against SciPy with M
def _composed(H, z, sign=1.0):
    minv = jacobi_inverse_z_host(csr_diagonal_host(sp.csr_matrix(H)), z, gc.FLOOR)
    mv = gc.shifted_matvec(H, z, sign)
    return minv, (lambda v: mv(minv * v))


def _residual_slack(H, z, x, b):
    """2-norm of the rounding of the float64 evaluation of ``b - (z x - H x)``: per row u [(L + 2)(|H||x|) + 3 |z x| + |b|]."""
    L = np.diff(H.indptr)
    return float(np.linalg.norm(gc.U * ((L + 2) * (abs(H) @ np.abs(x)) + 3 * abs(z) * np.abs(x) + np.abs(b))))


def _check_against_scipy(name, z, j, x, info, products):
    H, b = gc.operator(name), gc.rhs(j)
    xs, infos, count = gc.scipy_solve(name, z, j)
    assert info == infos == 0
    assert abs(products - count) <= max(3, count // 50), (name, z, j, products, count)
    assert np.linalg.norm(x - xs) <= 1e-7 * np.linalg.norm(xs)
    res = np.linalg.norm(b - gc.shifted_matvec(H, z)(x))
    assert res <= max(gc.ATOL, gc.RTOL * np.linalg.norm(b)) + _residual_slack(H, z, x, b), (name, z, j, res)
    return count


@pytest.mark.parametrize("name", ["a", "c"])
def test_composed_solve_is_scipy_gcrotmk_with_M(name):
    """The single driver on ``v -> A (minv v)``, then ``x = minv u``: info, product count (to rounding), solution and true
    residual of ``scipy.sparse.linalg.gcrotmk(A, b, M=...)``, three shifts (the real one included), two right-hand sides."""
    H = gc.operator(name)
    for z in gc.SHIFTS:
        minv, mv = _composed(H, z)
        for j in (0, 1):
            u, info, stats = gcrotmk_device(None, mv, gc.rhs(j) + 0j, gc.N, rtol=gc.RTOL, atol=gc.ATOL, maxiter=1000,
                                            complex_pairs=True, ops=NumpyOps(gc.N))
            count = _check_against_scipy(name, z, j, minv * u, info, stats["matvecs"])
            print(f"\noperator ({name}) z = {z!r} rhs {j}: {stats['matvecs']} products, SciPy with M {count}")
            if name == "c":
                assert count > 45                               # past the first inner cycle: restarts and recycling are run


@pytest.mark.parametrize("name", ["a", "c"])
def test_lock_step_and_pool_drivers_on_the_composed_operator(name):
    """The same through ``gcrotmk_device_block`` (one shift) and ``gcrotmk_device_pool`` with a ``minv`` per tag."""
    H = gc.operator(name)
    n = gc.N
    z = gc.Z_COMPLEX
    minv, mv = _composed(H, z)
    sols = gcrotmk_device_block(None, lambda vs: [mv(v) for v in vs], [gc.rhs(j) + 0j for j in (0, 1)], n, rtol=gc.RTOL,
                                atol=gc.ATOL, maxiter=1000, complex_pairs=True, ops_factory=lambda: NumpyOps(n))
    for j, (u, info, stats) in enumerate(sols):
        _check_against_scipy(name, z, j, minv * u, info, stats["matvecs"])
    per_tag = {t: _composed(H, zz) for t, zz in enumerate(gc.SHIFTS)}
    jobs = [(gc.rhs(j) + 0j, t) for t in per_tag for j in (0, 1)]
    ps = {}
    seen = 0
    for i, tag, u, info, stats in gcrotmk_device_pool(
            None, lambda vs, tags: [per_tag[t][1](v) for v, t in zip(vs, tags)], jobs, n, 4, rtol=gc.RTOL, atol=gc.ATOL,
            maxiter=1000, complex_pairs=True, ops_factory=lambda: NumpyOps(n), pool_stats=ps):
        _check_against_scipy(name, gc.SHIFTS[tag], i % 2, per_tag[tag][0] * u, info, stats["matvecs"])
        seen += 1
    assert seen == len(jobs) and sum(k * v for k, v in ps["histogram"].items()) == sum(ps["products"])


def test_weak_dominance_operator_is_what_the_device_tests_need():
    """(c): the smallest multiple of 8 that takes SciPy's preconditioned solves past 45 products for both shifts while
    they stay under a quarter of the plain count (asserted when the operator is built)."""
    c = gc.weak_c()
    H = gc.operator_c()
    counts = [gc.scipy_solve("c", z, 0)[2] for z in (gc.Z_COMPLEX, gc.Z_REAL)]
    print(f"\nweak dominance: c = {c}, SciPy with M {counts} products")
    assert c % 8 == 0 and c > 8 and min(counts) > 45
    np.testing.assert_array_equal(H.diagonal(), gc.operator_a().diagonal())


# ---------------------------------------------------------------- 3. the validator
class _Ctx:
    def __init__(self, collectives=False, direct_only=False):
        self.collectives, self.direct_only = collectives, direct_only


def _operator(nrows=10, ncols=10, row_offset=0):
    H = hv.HipCsrOperator.__new__(hv.HipCsrOperator)              # attributes only: no device
    H.nrows, H.ncols, H.row_offset = nrows, ncols, row_offset
    return H


def _args(**kw):
    o = {"linearSolver": "gcrotmk", "linearIter": 100, "linear_tol": 1e-8, "linear_atol": 1e-12}
    o.update(kw)
    return o


def test_validator_refusals():
    V = hv._gcrot_preconditioner
    assert V(_args(gcrotPreconditioner="jacobi"), None, _Ctx(), _operator()) == hv.PRECONDITIONER_FLOOR_DEFAULT
    assert V(_args(gcrotPreconditioner="jacobi", preconditionerFloor=1e-3)) == 1e-3
    for bad in ("ilu", "Jacobi", True, 1):
        with pytest.raises(ValueError, match="gcrotPreconditioner"):
            V(_args(gcrotPreconditioner=bad))
    for solver in ("minres", "pardiso", "minres_shifted", "lanczos_filter"):
        with pytest.raises(ValueError, match="gcrotmk"):
            V(_args(gcrotPreconditioner="jacobi", linearSolver=solver))
    for bad in (-1.0, float("inf"), float("nan"), "1e-8", None):
        with pytest.raises(ValueError, match="preconditionerFloor"):
            V(_args(gcrotPreconditioner="jacobi", preconditionerFloor=bad))
    with pytest.raises(NotImplementedError, match="x0"):
        V(_args(gcrotPreconditioner="jacobi"), np.zeros(10))
    for ctx in (_Ctx(collectives=True), _Ctx(direct_only=True)):
        with pytest.raises(NotImplementedError, match="one GPU"):
            V(_args(gcrotPreconditioner="jacobi"), None, ctx)
    for H in (_operator(10, 20), _operator(10, 10, 5), np.eye(10), sp.identity(10, format="csr")):
        with pytest.raises(NotImplementedError, match="whole HipCsrOperator"):
            V(_args(gcrotPreconditioner="jacobi"), None, _Ctx(), H)


def test_without_the_key_nothing_new_is_seen():
    """Absent or None: the validator returns None whatever else is passed, and ``_preconditioner`` - MINRES's key - does
    what it did, its refusals of GCROT and of complex shifts included, with or without the new key in the dict."""
    V = hv._gcrot_preconditioner
    for o in (_args(), _args(gcrotPreconditioner=None), _args(linearSolver="minres"), _args(preconditionerFloor=-1.0)):
        assert V(o, np.zeros(3), _Ctx(collectives=True), object()) is None
    for extra in ({}, {"gcrotPreconditioner": None}, {"gcrotPreconditioner": "jacobi"}):
        assert hv._preconditioner(_args(**extra)) is None
        assert hv._preconditioner(_args(linearSolver="minres", preconditioner="jacobi", **extra), 0.02) == "jacobi"
        for solver in ("gcrotmk", "pardiso"):
            with pytest.raises(ValueError, match='linearSolver="minres" only'):
                hv._preconditioner(_args(linearSolver=solver, preconditioner="jacobi", **extra), 0.02)
        with pytest.raises(ValueError, match="takes no preconditioner here"):
            hv._preconditioner(_args(linearSolver="minres", preconditioner="jacobi", **extra), 0.02 + 0.05j)
