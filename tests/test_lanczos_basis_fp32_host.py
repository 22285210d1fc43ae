"""The host-side pieces of a Lanczos basis stored in fp32 (``eigensolvers_amd/lanczos_filter.py``): the NumPy twin of the
stored combination, ``lanczos_combine_stored_host``, against the twin of the prefix pass and against its own error bound,
the ``ValueError`` paths that need no device, and the slot size.

Every case fails without the feature: the names and arguments do not exist.

The bound.  Pass 2 forms ``q = sum_i g_i v_i``.  A stored element rounded to fp32 (to nearest even, normal range) carries
a relative error of at most 2^-24, so ``||q32 - q64||_2 <= 2^-24 sum_{i in stream} |g_i| ||v_i||`` with ``||v_i|| = 1``.  The
test takes ``||v_i||`` from the twin's own vectors and allows 0.1 % on top: that covers ``||v_i|| = 1`` only to rounding
and the fp64 roundings of the normalisation and the accumulation (at most ``m eps ||g||_1``, eight orders below the
bound).  It is derived, not measured."""
import importlib
import types

import numpy as np
import pytest
import scipy.sparse as sp

from _lanczos_cases import slot_bytes
from eigensolvers_amd.hip_vector import HipVector
from test_lanczos_prefix_host import NEAR, W8, Z8

lf = importlib.import_module("eigensolvers_amd.lanczos_filter")       # the package exports the function of the same name

N = 200


def operator200():
    """The twin operator of ``test_lanczos_prefix_host.py`` at n = 200: a random sparse symmetric matrix plus a diagonal
    +-(1..3) except 4 rows inside the contour's window."""
    rng = np.random.default_rng(5)
    R = sp.random(N, N, density=0.05, random_state=rng, format="csr")
    d = rng.choice([-1.0, 1.0], N) * rng.uniform(1.0, 3.0, N)
    d[::60] = np.linspace(-0.2, 0.2, len(d[::60]))
    return (0.05 * (R + R.T) + sp.diags(d)).tocsr()


@pytest.fixture(scope="module")
def twin_run():
    """(matvec, b, scalars of the twin's pass 1, its Lanczos vectors, the NC = 1 and NC = 2 tables), computed once."""
    H = operator200()
    b = np.random.default_rng(9).standard_normal(N)
    b /= np.linalg.norm(b)
    matvec = lambda v: H @ v
    sc = lf.lanczos_scalars_host(matvec, b, Z8, 1e-5, 1e-7, 4000)[0]
    m = len(sc.alphas)
    assert all(sc.converged) and m >= 12, m
    V = lf.lanczos_vectors_host(matvec, b, sc.alphas, sc.betas, m)
    y = lf.minres_coefficients(sc.alphas, sc.betas, Z8[NEAR], sc.iterations[NEAR])
    y = np.concatenate([y, np.zeros(m - len(y))])
    tables = {1: lf.filter_coefficients([sc], Z8, W8)[0], 2: np.stack([y.real, y.imag], axis=1)}
    assert tables[1].shape == (m, 1) and tables[2].shape == (m, 2)
    return matvec, b, sc, V, tables


def prefixes(m):
    return [1, 2, 3, m // 2, m]


@pytest.mark.parametrize("nc", [1, 2])
def test_fp64_storage_equals_the_prefix_twin_bit_for_bit(twin_run, nc):
    matvec, b, sc, V, tables = twin_run
    G, m = tables[nc], len(sc.alphas)
    for p in prefixes(m):
        want = lf.lanczos_combine_prefix_host(matvec, V[:p], sc.alphas, sc.betas, G)
        got = lf.lanczos_combine_stored_host(matvec, b, sc.alphas, sc.betas, G, p, np.float64)
        assert want.any() and got.shape == want.shape and np.array_equal(got, want), (p, np.abs(got - want).max())
    # a 1-D table is one combination; the default storage is fp64
    if nc == 1:
        assert np.array_equal(lf.lanczos_combine_stored_host(matvec, b, sc.alphas, sc.betas, G[:, 0], 4),
                              lf.lanczos_combine_prefix_host(matvec, V[:4], sc.alphas, sc.betas, G))
    for p in (0, m + 1):
        with pytest.raises(ValueError):
            lf.lanczos_combine_stored_host(matvec, b, sc.alphas, sc.betas, G, p, np.float64)


@pytest.mark.parametrize("nc", [1, 2])
def test_fp32_storage_obeys_the_rounding_bound(twin_run, nc):
    matvec, b, sc, V, tables = twin_run
    G, m = tables[nc], len(sc.alphas)
    vnorm = np.linalg.norm(V, axis=1)
    assert np.abs(vnorm - 1.0).max() < 1e-12
    for p in prefixes(m):
        q64 = lf.lanczos_combine_stored_host(matvec, b, sc.alphas, sc.betas, G, p, np.float64)
        q32 = lf.lanczos_combine_stored_host(matvec, b, sc.alphas, sc.betas, G, p, np.float32)
        stream = lf.prefix_split(m, p)[0]
        for c in range(nc):
            err = np.linalg.norm(q32[c] - q64[c])
            bound = 2.0 ** -24 * 1.001 * float(np.abs(G[:stream, c]) @ vnorm[:stream])
            print(f"STORED fp32 nc={nc} c={c} p={p} stream={stream} error {err:.3e} bound {bound:.3e}")
            assert err <= bound, (p, c, err, bound)
            if stream == 0:
                assert np.array_equal(q32[c], q64[c])
            elif np.abs(G[:stream, c]).max() > 0:
                assert err > 0.0, (p, c)                         # the storage really was narrower
    assert lf.prefix_split(m, 1)[0] == 0


def test_option_checks_that_need_no_device():
    assert lf.BASIS_PRECISIONS == ("fp64", "fp32")
    assert lf.BASIS_MODES == ("recompute", "keep")
    with pytest.raises(ValueError, match="fp16"):
        lf.lanczos_run(None, [], Z8, keepBasis=True, basisPrecision="fp16")
    with pytest.raises(ValueError, match="precision"):
        lf.lanczos_filter(None, [], Z8, W8, basis="keep", precision="single")
    with pytest.raises(ValueError, match="kept"):
        lf.lanczos_run(None, [], Z8, basisPrecision="fp32")
    with pytest.raises(ValueError, match="kept"):
        lf.lanczos_filter(None, [], Z8, W8, basis="recompute", precision="fp32")
    lsa = {"linearSolver": "lanczos_filter", "linearIter": 10, "linear_tol": 1e-5, "linear_atol": 1e-7}
    for o in ({"linearSystemArgs": lsa, "lanczosBasisPrecision": "fp32"},
              {"linearSystemArgs": lsa, "lanczosBasisPrecision": "fp32", "lanczosBasis": "recompute"}):
        with pytest.raises(ValueError, match="lanczosBasisPrecision"):
            HipVector._lanczos_filter(None, [types.SimpleNamespace(options=o)], Z8, W8)
    with pytest.raises(ValueError, match="half"):
        HipVector._lanczos_filter(None, [types.SimpleNamespace(options={"linearSystemArgs": lsa, "lanczosBasis": "keep",
                                                                        "lanczosBasisPrecision": "half"})], Z8, W8)


@pytest.mark.parametrize("n,k", [(100, 1), (1037, 3), (1037, 5), (4000, 8), (10_000_000, 8)])
def test_an_fp32_slot_is_half_the_bytes(n, k):
    assert lf.basis_slot_bytes(n, k) == lf.basis_slot_bytes(n, k, "fp64") == slot_bytes(n, k)
    assert 2 * lf.basis_slot_bytes(n, k, "fp32") == slot_bytes(n, k)
    with pytest.raises(ValueError):
        lf.basis_slot_bytes(n, k, "fp16")
    with pytest.raises(ValueError):
        lf.basis_slot_bytes(n, 9)
