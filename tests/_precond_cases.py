"""Operators and references shared by the tests of the Jacobi-preconditioned MINRES (``test_precond_minres_cpu.py``,
``test_gpu_precond_minres.py``).  A plain module, imported as ``_hiprec`` is: no fixtures, no tests."""
import numpy as np
import scipy.sparse as sp

from eigensolvers_amd.generators import dense_test_matrix, gapped_csr_host, guess_vector
from eigensolvers_amd.precond_minres import csr_diagonal_host, jacobi_inverse_host, minres_jacobi_host

SIGMA = 0.02
DENSE_SIGMA = 30.3
# (shift, rtol) of the device tests on the dense matrix: outside its spectrum, where the twin is determinate to rounding
# (test_gpu_precond_minres.py says why; test_precond_minres_cpu.py checks it)
DENSE_CASES = [(-20.0, 1e-10), (0.0, 1e-8)]


def unit_guess(n):
    b = guess_vector(n, 1)
    return b / np.linalg.norm(b)


def exact_hit_operator(n=4001, sigma=SIGMA):
    """``gapped_csr_host(n, 16, seed=7)`` with one diagonal entry set to ``sigma`` exactly and one to a STORED zero (rows
    that store their diagonal once, so the sums are those values exactly).  Returns (matrix, row of the hit, row of the zero)."""
    H = gapped_csr_host(n, 16, seed=7).copy()
    rows = np.repeat(np.arange(n), np.diff(H.indptr))
    on = np.flatnonzero(H.indices == rows)
    count = np.bincount(rows[on], minlength=n)
    single = np.flatnonzero(count == 1)
    hit, zero = int(single[len(single) // 3]), int(single[2 * len(single) // 3])
    pos = {int(rows[p]): int(p) for p in on}
    H.data[pos[hit]] = sigma
    H.data[pos[zero]] = 0.0
    assert H.nnz == len(H.data) and H.data[pos[zero]] == 0.0            # still stored
    return H, hit, zero


def dense_operator():
    return dense_test_matrix()[0]


def shifted(H, sigma, sign=1.0):
    """The matvec every reference here uses, so that twin and SciPy see the same operator bits."""
    return lambda v: sign * (sigma * v - H @ v)


_twins = {}


def twin(key, H, b, sigma, rtol, maxiter, floor=1e-8, sign=1.0):
    """``minres_jacobi_host`` on ``sign * (sigma I - H)``: (x, info, itn, istop, trace), computed once per key."""
    key = (key, sigma, rtol, maxiter, floor, sign)
    if key not in _twins:
        d = np.diag(H).copy() if isinstance(H, np.ndarray) else csr_diagonal_host(sp.csr_matrix(H))
        minv = jacobi_inverse_host(d, sigma, floor)
        trace = []
        x, info, itn, istop = minres_jacobi_host(shifted(H, sigma, sign), b, minv, rtol=rtol, maxiter=maxiter, trace=trace)
        x.setflags(write=False)
        _twins[key] = (x, info, itn, istop, trace)
    return _twins[key]
