"""The Kronecker-sum operator's host side: the longdouble reference the GPU tests rest on, the explicit matrix behind
``to_scipy()``, the index convention, a known spectrum, and the refusals that need no device."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import _kron_cases as kc
from eigensolvers_amd import HipCsrOperator, HipKronSumOperator
from eigensolvers_amd.generators import coupled_oscillator_grid, sinc_dvr_harmonic

GRID = ((13, 10, 7), [(-5, 5), (-4.5, 4.5), (-4, 4)], [1.0, 1.3, 1.7])


def _dense_sum(factors, V):
    """((K_1 + K_2) + ...) + diag(V) from np.kron on dense arrays: the matrix stated without scipy.sparse."""
    dims = [T.shape[0] for T in factors]
    H = None
    for d, T in enumerate(factors):
        K = np.kron(np.kron(np.eye(kc.size(dims[:d])), T), np.eye(kc.size(dims[d + 1:])))
        H = K if H is None else H + K
    return H if V is None else H + np.diag(np.asarray(V).reshape(-1))


@pytest.mark.parametrize("dims", [(5,), (17, 3), (2, 3, 4, 5), (1, 8, 1, 5), (5, 4, 3, 6)])
@pytest.mark.parametrize("with_v", [False, True])
def test_explicit_matrix_and_longdouble_reference(dims, with_v):
    factors = kc.factors_for(dims, 1, symmetric=False)
    V = kc.diag_for(dims, 1) if with_v else None
    Hs = HipKronSumOperator.explicit_matrix(factors, V)
    assert sp.issparse(Hs) and Hs.shape == (kc.size(dims),) * 2
    np.testing.assert_array_equal(Hs.toarray(), _dense_sum(factors, V))
    x = kc.operand(kc.size(dims), 2)
    y, S = kc.kron_apply_ld(factors, V, x)
    # the CSR product against the reference: a row of at most sum n_d - D + 2 stored entries, inside the device bound
    ratio = kc.within(Hs @ x, y, kc.product_bound(dims, S))
    assert ratio < 0.5
    # S sums |a||x| term by term; the explicit matrix has merged the D diagonal terms of a row, so its |H||x| is no larger
    Sh = abs(Hs) @ np.abs(x)
    assert np.all(Sh <= np.asarray(S, dtype=float) * (1 + 1e-13))
    if len(dims) == 1 and not with_v:
        np.testing.assert_allclose(np.asarray(S, dtype=float), Sh, rtol=1e-13)


def test_index_convention_on_unit_vectors():
    dims = (3, 4, 2)
    factors = kc.factors_for(dims, 4, symmetric=False)
    V = kc.diag_for(dims, 4)
    for idx in itertools.product(*[range(n) for n in dims]):
        r = (idx[0] * dims[1] + idx[1]) * dims[2] + idx[2]
        e = np.zeros(kc.size(dims))
        e[r] = 1.0
        col = np.asarray(kc.kron_apply_ld(factors, V, e)[0], dtype=float).reshape(dims)
        want = np.zeros(dims)
        want[:, idx[1], idx[2]] += factors[0][:, idx[0]]           # T_d[i, k] takes x_k to y_i: not transposed
        want[idx[0], :, idx[2]] += factors[1][:, idx[1]]
        want[idx[0], idx[1], :] += factors[2][:, idx[2]]
        want[idx] += V[idx]
        np.testing.assert_allclose(col, want, rtol=0, atol=1e-13)
        np.testing.assert_allclose(HipKronSumOperator.explicit_matrix(factors, V)[:, [r]].toarray().reshape(dims), want, rtol=0, atol=1e-13)


def test_separable_spectrum_is_the_sums_of_the_factor_spectra():
    dims, ranges, freqs = GRID
    factors, V = coupled_oscillator_grid(dims, ranges, freqs, coupled=False)
    lam = np.linalg.eigvalsh(HipKronSumOperator.explicit_matrix(factors, V).toarray())
    parts = []
    for T, r, w in zip(factors, ranges, freqs):
        x = sinc_dvr_harmonic(T.shape[0], r)[1]
        parts.append(np.linalg.eigvalsh(T + np.diag((w * x) ** 2)))
    sums = np.sort(np.add.outer(np.add.outer(parts[0], parts[1]), parts[2]).reshape(-1))
    np.testing.assert_allclose(lam, sums, rtol=0, atol=5e-13 * np.max(np.abs(sums)))


def test_coupled_oscillator_grid():
    dims, ranges, freqs = GRID
    factors, V = coupled_oscillator_grid(dims, ranges, freqs)
    assert [T.shape for T in factors] == [(n, n) for n in dims] and V.shape == dims
    for T, n, r in zip(factors, dims, ranges):
        Hd, x = sinc_dvr_harmonic(n, r)
        np.testing.assert_array_equal(T, Hd - np.diag(x ** 2))
        np.testing.assert_array_equal(T, T.T)
    xs = [sinc_dvr_harmonic(n, r)[1] for n, r in zip(dims, ranges)]
    i = (3, 7, 2)
    p = [x[k] for x, k in zip(xs, i)]
    want = sum((w * q) ** 2 for w, q in zip(freqs, p)) + 0.3 * p[0] * p[1] * p[2] + 0.2 * p[0] ** 2 * p[2]
    assert abs(V[i] - want) <= 1e-13 * abs(want)
    with pytest.raises(ValueError):
        coupled_oscillator_grid((3, 4), ranges, freqs)


def test_refusals_that_need_no_device():
    T = np.eye(3)
    with pytest.raises(ValueError, match="not a square"):
        HipKronSumOperator.from_factors([np.ones((3, 4))])
    with pytest.raises(ValueError, match="not finite"):
        HipKronSumOperator.from_factors([T, np.array([[1.0, np.nan], [np.nan, 1.0]])])
    with pytest.raises(ValueError, match="not symmetric"):
        HipKronSumOperator.from_factors([T, np.array([[1.0, 2.0], [2.0 + 1e-10, 1.0]])])
    with pytest.raises(ValueError, match="1 to 8"):
        HipKronSumOperator.from_factors([])
    with pytest.raises(ValueError, match="1 to 8"):
        HipKronSumOperator.from_factors([T] * 9)
    with pytest.raises(ValueError, match="diag has shape"):
        HipKronSumOperator.from_factors([T, np.eye(2)], diag=np.zeros(5))
    with pytest.raises(ValueError, match="2\\^31"):
        HipKronSumOperator.from_factors([np.eye(200)] * 5)
    with pytest.raises(TypeError):
        HipKronSumOperator.from_factors([T * (1 + 1j)])
    with pytest.raises(TypeError):
        HipKronSumOperator.from_factors([T], diag=np.zeros(3) + 1j)
    # symmetric to 1e-12 * max|T| passes the check; shapes `dims` and (N,) of diag are both taken
    f, V = HipKronSumOperator._checked([T, np.array([[1.0, 2.0], [2.0 + 1e-13, 1.0]])], np.zeros((3, 2)), True)
    assert V.shape == (6,) and HipKronSumOperator._checked(f, np.zeros(6), True)[1].shape == (6,)
    assert issubclass(HipKronSumOperator, HipCsrOperator) and not HipKronSumOperator.supports_block_sweeps
    assert HipCsrOperator.supports_block_sweeps


def test_complex_input_is_refused_not_truncated():
    """A complex array used to lose its imaginary part on the way to float64 and give a wrong operator."""
    M = np.array([[1.0, 2.0 + 1.0j], [2.0 - 1.0j, 3.0]])
    with pytest.raises(TypeError, match="real fp64"):
        HipCsrOperator.from_dense(M)
    with pytest.raises(TypeError, match="real fp64"):
        HipCsrOperator.from_dense(M, layout="dense")
    with pytest.raises(TypeError, match="real fp64"):
        HipCsrOperator.from_csr_arrays([0, 1, 2], [0, 1], np.array([1.0 + 1j, 2.0]), 2)
    with pytest.raises(TypeError, match="real fp64"):
        HipCsrOperator.from_scipy(sp.csr_matrix(M))
