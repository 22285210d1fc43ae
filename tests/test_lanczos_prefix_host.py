"""The host-side pieces of a Lanczos basis kept as a prefix (``eigensolvers_amd/lanczos_filter.py``): the bookkeeping
``prefix_split``, the NumPy twin of the tail pass against the twin of the product pass, and the ``ValueError`` paths that
need no device.

Every case fails without the feature: the names do not exist.

``lanczos_combine_prefix_host`` adds the same terms in the same order with the same NumPy expressions as
``lanczos_combine_host`` - the stream's terms from the stored vectors, which are the vectors the recurrence would have
rebuilt, then the recurrence itself - so the two are compared with ``array_equal`` (checked on the CPU: equal for every
case below, NC = 1 and NC = 2)."""
import importlib
import math
import types

import numpy as np
import pytest
import scipy.sparse as sp

from eigensolvers_amd import feast as pf
from eigensolvers_amd.hip_vector import HipVector

lf = importlib.import_module("eigensolvers_amd.lanczos_filter")       # the package exports the function of the same name


def contour(nc):
    """(shifts, FEAST's weights -0.5 w r phase) of the nc-node Legendre half contour of [-0.21, 0.21]."""
    gk, wk = pf.quadraturePointsWeights(nc, "legendre", positiveHalf=True)
    zs, ws = [], []
    for g, w in zip(gk, wk):
        theta, z = pf.contour_point(-0.21, 0.21, g)
        zs.append(z)
        ws.append(-0.5 * w * 0.21 * (math.cos(theta) + 1j * math.sin(theta)))
    return zs, ws


Z8, W8 = contour(16)
NEAR = int(np.argmin([abs(z.imag) for z in Z8]))


def odd_operator():
    """n = 1037: a random sparse symmetric matrix plus a diagonal +-(1..3) except 8 rows inside the contour's window."""
    n = 1037
    rng = np.random.default_rng(5)
    R = sp.random(n, n, density=0.01, random_state=rng, format="csr")
    d = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 3.0, n)
    d[::130] = np.linspace(-0.2, 0.2, len(d[::130]))
    return (0.05 * (R + R.T) + sp.diags(d)).tocsr()


def tridiagonal100():
    n = 100
    d = np.concatenate([np.linspace(-1.5, -1.0, n // 2), np.linspace(1.0, 1.5, n - n // 2)])
    return sp.diags([np.full(n - 1, 0.1), d, np.full(n - 1, 0.1)], [-1, 0, 1]).tocsr()


@pytest.fixture(scope="module", params=["odd1037", "tri100"])
def twin_run(request):
    """(matvec, b, scalars of the twin's pass 1, all its Lanczos vectors), computed once per operator."""
    H = odd_operator() if request.param == "odd1037" else tridiagonal100()
    b = np.random.default_rng(9).standard_normal(H.shape[0])
    b /= np.linalg.norm(b)
    matvec = lambda v: H @ v
    sc = lf.lanczos_scalars_host(matvec, b, Z8, 1e-5, 1e-7, 4000)[0]
    assert all(sc.converged) and len(sc.alphas) >= 12, len(sc.alphas)
    V = lf.lanczos_vectors_host(matvec, b, sc.alphas, sc.betas, len(sc.alphas))
    return matvec, b, sc, V


@pytest.mark.parametrize("p", [1, 2, 5])
def test_prefix_split(p):
    for m in (0, 1, p - 1, p, p + 1, 3 * p):
        stream, products = lf.prefix_split(m, p)
        if m > p:
            assert stream + products + 1 == m and stream == p - 1 and products == m - p, (m, p)
        else:
            assert products == 0 and stream == m, (m, p)
    assert lf.prefix_split(0, 0) == (0, 0)
    with pytest.raises(ValueError):
        lf.prefix_split(3, 0)
    with pytest.raises(ValueError):
        lf.prefix_split(-1, p)


def test_the_twins_vectors_are_those_of_its_pass_2(twin_run):
    matvec, b, sc, V = twin_run
    assert V.shape == (len(sc.alphas), b.size) and np.array_equal(V[0], b / sc.betas[0])
    # nearly orthonormal: these are Lanczos vectors, not just any vectors (short runs, little loss of orthogonality)
    assert np.abs(V[:10] @ V[:10].T - np.eye(10)).max() < 1e-8
    for p in (0, 1, 7):
        assert np.array_equal(lf.lanczos_vectors_host(matvec, b, sc.alphas, sc.betas, p), V[:p])
    with pytest.raises(ValueError):
        lf.lanczos_vectors_host(matvec, b, sc.alphas, sc.betas, len(sc.alphas) + 1)


@pytest.mark.parametrize("nc", [1, 2])
def test_combination_from_a_prefix_equals_the_product_pass_twin(twin_run, nc):
    matvec, b, sc, V = twin_run
    m = len(sc.alphas) - 5                                   # tables 5 terms short of the run: p = m + 5 vectors exist
    if nc == 1:
        G = lf.filter_coefficients([sc], Z8, W8)[0][:m]
    else:
        y = lf.minres_coefficients(sc.alphas, sc.betas, Z8[NEAR], sc.iterations[NEAR])
        y = np.concatenate([y, np.zeros(len(sc.alphas) - len(y))])[:m]
        G = np.stack([y.real, y.imag], axis=1)
    assert G.shape == (m, nc) and np.abs(G[-1]).max() > 0
    ref = lf.lanczos_combine_host(matvec, [b], [sc.alphas], [sc.betas], [G])[0]
    assert ref.shape == (nc, b.size) and ref.any()
    for p in (1, 2, 3, m - 1, m, m + 5):
        got = lf.lanczos_combine_prefix_host(matvec, V[:p], sc.alphas, sc.betas, G)
        assert got.shape == ref.shape and np.array_equal(got, ref), (p, m, np.abs(got - ref).max())
    # a 1-D table is one combination
    if nc == 1:
        assert np.array_equal(lf.lanczos_combine_prefix_host(matvec, V[:4], sc.alphas, sc.betas, G[:, 0]), ref)


def test_refusals_that_need_no_device():
    with pytest.raises(ValueError, match="[Pp]refix"):
        lf.lanczos_run(None, [], Z8, keepPrefix=True)
    with pytest.raises(ValueError, match="[Pp]refix"):
        lf.lanczos_run(None, [], Z8, keepBasis=False, keepPrefix=True)
    with pytest.raises(ValueError, match="[Pp]refix"):
        lf.lanczos_filter(None, [], Z8, W8, basis="recompute", prefix=True)
    lsa = {"linearSolver": "lanczos_filter", "linearIter": 10, "linear_tol": 1e-5, "linear_atol": 1e-7}
    for o in ({"linearSystemArgs": lsa, "lanczosBasisPrefix": True},
              {"linearSystemArgs": lsa, "lanczosBasisPrefix": True, "lanczosBasis": "recompute"}):
        with pytest.raises(ValueError, match="lanczosBasisPrefix"):
            HipVector._lanczos_filter(None, [types.SimpleNamespace(options=o)], Z8, W8)


def test_basis_modes_are_unchanged():
    assert lf.BASIS_MODES == ("recompute", "keep")
