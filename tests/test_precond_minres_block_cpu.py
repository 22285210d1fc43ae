"""The NumPy twin of the lock-step block form of the Jacobi-preconditioned MINRES (``precond_minres.minres_jacobi_block_host``,
the statement of ``csrc/minres_block_precond.hip``) against the single-vector twin ``minres_jacobi_host``, which
``test_precond_minres_cpu.py`` pins to SciPy, and once against ``scipy.sparse.linalg.minres(A, b, M=...)`` itself."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _precond_cases as pc
from eigensolvers_amd.generators import gapped_csr_host
from eigensolvers_amd.precond_minres import (csr_diagonal_host, jacobi_inverse_host, minres_jacobi_block_host,
                                             minres_jacobi_host)

N = 4000


def _columns():
    """unit_guess, five normalised random rows, e_1234 and a zero column: the columns of the device test."""
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((7, N))[:5]
    e = np.zeros(N)
    e[1234] = 1.0
    return np.stack([pc.unit_guess(N)] + [r / np.linalg.norm(r) for r in rows] + [e, np.zeros(N)], axis=1)


def _column_wise(mv):
    """A block product that IS the single product column by column (contiguous operands, so the same bits)."""
    return lambda V: np.stack([mv(np.ascontiguousarray(V[:, j])) for j in range(V.shape[1])], axis=1)


def test_block_twin_equals_the_single_twin_column_by_column():
    H = gapped_csr_host(N, 16, seed=7)
    minv = jacobi_inverse_host(csr_diagonal_host(H), pc.SIGMA)
    mv = pc.shifted(H, pc.SIGMA)
    B = _columns()
    for rtol, maxiter in ((1e-6, 2000), (1e-10, 2000), (1e-10, 5)):
        block = minres_jacobi_block_host(_column_wise(mv), B, minv, rtol=rtol, maxiter=maxiter)
        assert len(block) == B.shape[1]
        counts = []
        for j, (x, info, itn, istop) in enumerate(block):
            xs, infos, itns, istops = minres_jacobi_host(mv, B[:, j].copy(), minv, rtol=rtol, maxiter=maxiter)
            assert (info, itn, istop) == (infos, itns, istops), (rtol, maxiter, j)
            np.testing.assert_array_equal(x, xs)
            counts.append(itn)
        assert counts[-1] == 0 and not block[-1][0].any() and block[-1][3] == 0          # the zero column
        if maxiter == 5:
            assert all(r[1:] == (5, 5, 6) for r in block[:-1])
        else:
            assert len(set(counts[:-1])) > 1                                             # the columns stop at different iterations
            assert all(r[1] == 0 and r[3] in (1, 2) for r in block[:-1])


def test_one_column_against_scipy():
    H = gapped_csr_host(N, 16, seed=7)
    minv = jacobi_inverse_host(csr_diagonal_host(H), pc.SIGMA)
    mv = pc.shifted(H, pc.SIGMA)
    B = _columns()[:, :3]
    block = minres_jacobi_block_host(_column_wise(mv), B, minv, rtol=1e-10, maxiter=2000)
    A = spla.LinearOperator((N, N), matvec=mv, dtype=np.float64)
    count = [0]
    xs, info = spla.minres(A, B[:, 1], M=sp.diags(minv), rtol=1e-10, maxiter=2000,
                            callback=lambda xk: count.__setitem__(0, count[0] + 1))
    x, binfo, itn, istop = block[1]
    assert info == 0 and binfo == 0 and itn == count[0]
    assert np.linalg.norm(x - xs) <= 1e-12 * np.linalg.norm(xs)
