"""Operators, references and bounds shared by the tests of GCROT's diagonal right preconditioner
(``test_gcrot_precond_cpu.py``, ``test_gpu_gcrot_precond.py``).  A plain module, imported as ``_precond_cases`` is: no
fixtures, no tests."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import _precond_cases as pc
from eigensolvers_amd.generators import gapped_csr_host, guess_vector
from eigensolvers_amd.precond_gcrotmk import jacobi_inverse_z_host
from eigensolvers_amd.precond_minres import csr_diagonal_host
from test_gcrotmk_cpu import NumpyOps          # noqa: F401  (re-exported: the NumPy provider of the solver's vector operations)

LD = np.longdouble
U = 2.0 ** -53
ULD = float(np.finfo(LD).eps) / 2                  # 2^-64 where longdouble is the x87 format
N = 4001
Z_COMPLEX, Z_ON_AXIS, Z_REAL = 0.02 + 0.05j, complex(0.05), 0.05
SHIFTS = (Z_COMPLEX, Z_ON_AXIS, Z_REAL)            # the last one is a float: the real-shift GCROT
RTOL, ATOL = 1e-8, 1e-12
FLOOR = 1e-8

_cache = {}


def _once(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


# ---------------------------------------------------------------- operators
def operator_a():
    """(a) ``gapped_csr_host(4001, 16, seed=7)``: strongly diagonally dominant."""
    return _once("a", lambda: sp.csr_matrix(gapped_csr_host(N, 16, seed=7)))


def operator_b():
    """(b) its exact-hit form: ``(matrix, row with d_i == 0.02 exactly, row with a stored zero)``."""
    return _once("b", lambda: pc.exact_hit_operator(N, 0.02))


def _weak(c):
    A = operator_a()
    D = sp.diags(A.diagonal())
    return sp.csr_matrix(D + c * (A - D))


def weak_c():
    """The ``c`` of operator (c): the smallest multiple of 8 for which SciPy's own ``gcrotmk`` with ``M`` needs more than
    45 products for both z = 0.02+0.05j and z = 0.05 at rtol 1e-8 - (a) itself ends inside the first inner cycle, which
    tests neither restarts nor recycling."""
    def find():
        b = rhs(0)
        for c in range(8, 8 * 40, 8):
            H = _weak(c)
            if all(_scipy_solve(H, z, b)[2] > 45 for z in (Z_COMPLEX, Z_REAL)):
                return c
        raise AssertionError("no c up to 312 makes the preconditioned solves leave their first cycle")
    return _once("c value", find)


def operator_c():
    """(c) "weak dominance": ``D + c E``, D the diagonal of (a) and E the rest, ``c = weak_c()``.  Asserted here, on the
    CPU: with ``M`` both shifts need more than 45 products and at most a quarter of the plain count."""
    def build():
        c = weak_c()
        H = _weak(c)
        b = rhs(0)
        for z in (Z_COMPLEX, Z_REAL):
            count = _scipy_solve(H, z, b)[2]
            assert count > 45, (c, z, count)
            assert plain_count_exceeds(H, z, b, 4 * count), f"c = {c}, z = {z}: the plain solve needs fewer than 4 x {count} products"
        return H
    return _once("c", build)


def operator(name):
    return {"a": operator_a, "b": lambda: operator_b()[0], "c": operator_c}[name]()


def rhs(j, n=N):
    """Right-hand side j: the unit ``guess_vector(n, 1)`` for j = 0, unit normal vectors (seeded by j) after it."""
    def build():
        if j == 0:
            b = guess_vector(n, 1)
        else:
            b = np.random.default_rng([11, j]).standard_normal(n)
        b = b / np.linalg.norm(b)
        b.setflags(write=False)
        return b
    return _once(("rhs", j, n), build)


# ---------------------------------------------------------------- SciPy with M: the referee
def shifted_matvec(H, z, sign=1.0):
    """``v -> sign (z v - H v)``: the operator every reference here uses."""
    return lambda v: sign * (z * v - H @ v)


def _scipy_solve(H, z, b, sign=1.0, rtol=RTOL, atol=ATOL, maxiter=1000, floor=FLOOR, complex_rhs=False):
    cplx = isinstance(z, complex) or complex_rhs
    dtype = np.complex128 if cplx else np.float64
    n = H.shape[0]
    minv = jacobi_inverse_z_host(csr_diagonal_host(sp.csr_matrix(H)), z, floor)
    count = [0]
    mv = shifted_matvec(H, z, sign)

    def counted(v):
        count[0] += 1
        return mv(v)

    A = spl.LinearOperator((n, n), matvec=counted, dtype=dtype)
    M = spl.LinearOperator((n, n), matvec=lambda v: minv * v, dtype=dtype)
    x, info = spl.gcrotmk(A, b.astype(dtype), M=M, rtol=rtol, atol=atol, maxiter=maxiter)
    x.setflags(write=False)
    return x, info, count[0]


def scipy_solve(name, z, j, sign=1.0, complex_rhs=False):
    """``scipy.sparse.linalg.gcrotmk(A, b, M=diag(minv))`` (m = k = 20) on operator ``name``, right-hand side ``j``:
    ``(x, info, products of A)``, computed once per key and read-only."""
    key = ("scipy", name, z, isinstance(z, complex), j, sign, complex_rhs)
    b = rhs(j) * (1 + 0.5j) / abs(1 + 0.5j) if complex_rhs else rhs(j)
    return _once(key, lambda: _scipy_solve(operator(name), z, b, sign, complex_rhs=complex_rhs))


class _Enough(Exception):
    pass


def plain_count_exceeds(H, z, b, limit):
    """True when SciPy's plain ``gcrotmk`` (no ``M``) has not converged after ``limit`` products of A."""
    n = H.shape[0]
    dtype = np.complex128 if isinstance(z, complex) else np.float64
    count = [0]
    mv = shifted_matvec(H, z)

    def counted(v):
        count[0] += 1
        if count[0] > limit:
            raise _Enough()
        return mv(v)

    try:
        spl.gcrotmk(spl.LinearOperator((n, n), matvec=counted, dtype=dtype), b.astype(dtype), rtol=RTOL, atol=ATOL, maxiter=10000)
    except _Enough:
        return True
    return False


# ---------------------------------------------------------------- minv: extended-precision value and the twin's bound
_u = LD(U)          # the factors below are formed in longdouble: 1 + 2^-53 is not a float64


def minv_reference(d, z, floor):
    """``(re, im, rel, kind)``: the definition of ``minv`` (``jacobi_inverse_z_host``'s docstring) evaluated in longdouble
    on the float64 ``d``, the relative bound per element ``|got - ref| <= rel_i |ref_i|`` (complex modulus) that the
    twin's - and the kernel's - operations guarantee, and the class of each element (0: ``1 / m``, 1: floored with the
    phase kept, 2: ``t == 0``).

    Derivation (u = 2^-53; every operation listed in the twin rounds once; nothing is put on top):

    - ``mr' = rn(zr - d_i) = mr (1 + e)``, ``|e| <= u``: ``|m' - m| <= u |m|``, so ``1 / m' = (1 / m)(1 + f)`` with
      ``|1 + f| <= 1 / (1 - u)`` and the unit vector ``conj(m') / |m'|`` lies within ``2u`` of ``conj(m) / |m|``;
    - complex ``s' = |m'|^2 (1 + e_s)``, ``|e_s| <= (1 + u)^2 - 1`` (two products, one sum), and ``t' = sqrt(s')`` rounds
      once more: ``t' = |m'| (1 + e_t)``, ``1 + e_t`` within ``[(1 - e_s)(1 - u), (1 + u)^2]``; a real ``z`` has
      ``t' = |m'|`` exactly;
    - class 0, complex ``(mr' / s', -zi / s')``: one division per half, ``u`` in modulus:
      ``rel = (1 + u) / ((1 - e_s)(1 - u)) - 1``; real ``1 / mr'``: ``rel = (1 + u) / (1 - u) - 1``;
    - ``T' = max t'`` carries the relative error of one ``t'`` (times ``1 +- u`` for ``|m'|`` against ``|m|``) and
      ``g' = rn(floor T')`` one rounding more: ``g' = g (1 + e_g)``, ``1 + e_g >= lo_g``; complex
      ``lo_g = (1 - e_s)(1 - u)^3``, real ``lo_g = (1 - u)^2``;
    - class 2, ``1 / g'``: ``rel = (1 + u) / lo_g - 1``; class 1 real, ``copysign(1 / g', mr')``: the same (the sign of a
      rounded difference is the sign of the difference);
    - class 1 complex, ``((mr' / t') / g', (-zi / t') / g')``: two divisions per half, the phase's ``2u``:
      ``rel = (1 + u)^2 (1 + 2u) / ((1 - e_s)(1 - u) lo_g) - 1``;
    - the longdouble evaluation itself takes at most 8 operations per element: ``8 * 2^-64`` is added.

    An element whose ``t`` lies within these errors of ``g`` could fall into either class; the cases used avoid that."""
    z = complex(z)
    cplx = z.imag != 0.0
    d = np.asarray(d, dtype=np.float64)
    mr, zi = LD(z.real) - d.astype(LD), LD(z.imag)
    t = np.sqrt(mr * mr + zi * zi) if cplx else np.abs(mr)
    g = LD(floor) * t.max()
    kind = np.where(t >= g, 0, np.where(t > 0, 1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = mr * mr + zi * zi
        re = np.where(kind == 0, mr / s, np.where(kind == 1, mr / t / g, 1 / g))
        im = np.where(kind == 0, -zi / s, np.where(kind == 1, -zi / t / g, LD(0)))
    u = _u
    e_s = (1 + u) ** 2 - 1
    if cplx:
        lo_g = (1 - e_s) * (1 - u) ** 3
        rels = ((1 + u) / ((1 - e_s) * (1 - u)) - 1, (1 + u) ** 2 * (1 + 2 * u) / ((1 - e_s) * (1 - u) * lo_g) - 1, (1 + u) / lo_g - 1)
    else:
        lo_g = (1 - u) ** 2
        rels = ((1 + u) / (1 - u) - 1, (1 + u) / lo_g - 1, (1 + u) / lo_g - 1)
    rel = np.array([float(r) for r in rels])[kind] + 8 * ULD
    return re, im, rel, kind


def minv_error_ratio(got, d, z, floor):
    """max_i |got_i - ref_i| / (rel_i |ref_i|) for a ``minv`` (float64 or complex128 array); inf where it is not finite."""
    re, im, rel, _ = minv_reference(d, z, floor)
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        return float("inf")
    er, ei = got.real.astype(LD) - re, got.imag.astype(LD) - im
    err = np.sqrt(er * er + ei * ei)
    return float(np.max(err / (rel * np.sqrt(re * re + im * im))))


# ---------------------------------------------------------------- the element y = m x
def diag_mul_reference(mr, mi, xr, xi):
    """``(yr, yi, br, bi)``: ``(mr + i mi)(xr + i xi)`` in longdouble and the bound on each half of the float64 element
    ``yr = fma(-mi, xi, rn(mr xr))``, ``yi = fma(mi, xr, rn(mr xi))`` (``DiagMul::pair``).  ``mi`` None: a real ``m``,
    ``yr = rn(mr xr)``, ``yi = rn(mr xi)``.  ``xi`` None: the real element ``rn(m x)`` (``yi``, ``bi`` are None).

    With p = mr x (the rounded product) and q = mi x' (the fused one), ``fma(q, rn(p)) = (p (1 + e1) + q)(1 + e2)``,
    so ``|y - (p + q)| <= u |p| + u |p + q| + u^2 |p|``; without q it is ``u |p|``.  The longdouble evaluation rounds
    three times: ``3 * 2^-64 (|p| + |q|)`` is added.  Operands are kept where nothing underflows."""
    mr, xr = np.asarray(mr, dtype=LD), np.asarray(xr, dtype=LD)

    def half(p, q):
        y = p + q if q is not None else p
        ap, aq = np.abs(p), (np.abs(q) if q is not None else 0)
        b = (U * ap + U * np.abs(y) + U * U * ap) if q is not None else U * ap
        return y, (b + 3 * ULD * (ap + aq)).astype(np.float64)

    if xi is None:
        y, b = half(mr * xr, None)
        return y, None, b, None
    xi = np.asarray(xi, dtype=LD)
    if mi is None:
        yr, br = half(mr * xr, None)
        yi, bi = half(mr * xi, None)
    else:
        mi = np.asarray(mi, dtype=LD)
        yr, br = half(mr * xr, -mi * xi)
        yi, bi = half(mr * xi, mi * xr)
    return yr, yi, br, bi


def scaling_vectors(n, count, seed=5):
    """``count`` complex ``minv``-like vectors of length n as (re, im) rows whose magnitudes differ by orders between
    neighbours (1e-3, 1e2, 1e-1, 1e4, ... times ``exp(U(-2, 2))``): an operand that takes its neighbour's is off by far
    more than a bound.  Every third one is real (im None)."""
    rng = np.random.default_rng([seed, n])
    scales = (1e-3, 1e2, 1e-1, 1e4, 1.0, 1e-2)
    out = []
    for p in range(count):
        v = rng.standard_normal((2, n)) * np.exp(rng.uniform(-2, 2, (2, n))) * scales[p % len(scales)]
        out.append((np.ascontiguousarray(v[0]), None if p % 3 == 1 else np.ascontiguousarray(v[1])))
    return out


# ---------------------------------------------------------------- FEAST window
def feast_window():
    """``(lo, hi, eigenvalues inside)`` on operator (a): the 3 eigenvalues nearest 0.02 from a host ``eigvalsh``, the
    window's edges half way to the neighbours outside."""
    def build():
        ev = np.linalg.eigvalsh(operator_a().toarray())
        order = np.argsort(np.abs(ev - 0.02))[:3]
        i0, i1 = int(order.min()), int(order.max())
        assert i1 - i0 == 2 and i0 > 0 and i1 < len(ev) - 1
        lo, hi = 0.5 * (ev[i0 - 1] + ev[i0]), 0.5 * (ev[i1] + ev[i1 + 1])
        return float(lo), float(hi), ev[i0:i1 + 1].copy()
    return _once("window", build)
