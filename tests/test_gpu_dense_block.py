"""The opt-in dense layout of the block sweeps (``set_block_variant(3)``, csrc/dense_device.h ``dense_block_sweep<K>``): block
products of every interleave width, the lock-step block MINRES and the Lanczos filter.

Every test fails without the feature: ``set_block_variant(3)`` raises "unknown block variant".

The interleave width K follows from the number of operands, as in every block product: k <= 4 real operands take K = 4,
5..8 take K = 8; complex operands count twice (2 -> K = 4, 3..4 -> K = 8) and 5..8 of them share a 16-wide block when
HIPEIG_PAIR_BLOCK_WIDTH = 8.  The operand counts below put 1, K - 1 (K - 2 for complex operands) and K live columns into
each width the call can take.  Products are compared per column with the ``np.longdouble`` product within
``_sweep_cases.product_bound`` (a shift term counts as one more term of the row's absolute sum), and each is bit-identical
to itself with HIPEIG_DENSE_GRID = 1, where one workgroup walks every row group."""
import numpy as np
import pytest
import scipy.sparse as sp

from _lanczos_cases import W8, Z8, check_filter, device_columns, twin
from _sweep_cases import minres_opts, product_bound
from eigensolvers_amd import _lib

pytestmark = pytest.mark.gpu

LD = np.longdouble
SIGMA = 0.37
Z = 0.11 + 0.21j
REAL_COUNTS = (1, 3, 4, 5, 7, 8)             # K = 4: 1, 3, 4 live columns; K = 8: 5, 7, 8
PAIR_COUNTS = ((2, None), (3, None), (4, None), (5, "8"), (7, "8"), (8, "8"))     # K = 4: 4; K = 8: 6, 8; K = 16: 10, 14, 16


def _symmetric(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    return (A + A.T) / 2, rng.standard_normal((n, 16))


def _bufs(hip, cols):
    vs = [hip.HipVector(np.ascontiguousarray(c)) for c in cols]
    return vs, [v._buf for v in vs]


def _arrays(hip, bufs):
    return [hip.HipVector(b).array for b in bufs]


def _within(got, ref, bound, label):
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    assert (err <= bound).all(), (label, float(np.max(err / bound)))
    return float(np.max(err / bound))


def _block_products(hip, H, X, k):
    """(apply_block, apply_shifted_block +, apply_shifted_block -) of the first k columns, as host arrays."""
    keep, bufs = _bufs(hip, X[:, :k].T)
    out = [_arrays(hip, H.apply_block(bufs))]
    for reverse in (False, True):
        out.append(_arrays(hip, H.apply_shifted_block(SIGMA, bufs, reverse=reverse)))
    return out


def _pair_products(hip, H, X, npairs):
    """apply_shifted_pairs with one shift and with a shift per operand, on complex operands (columns 2p, 2p + 1)."""
    keep_r, re = _bufs(hip, X[:, 0:2 * npairs:2].T)
    keep_i, im = _bufs(hip, X[:, 1:2 * npairs:2].T)
    xs = list(zip(re, im))
    zs = [Z + 0.05 * p for p in range(npairs)]
    one = [(hip.HipVector(a).array, hip.HipVector(b).array) for a, b in H.apply_shifted_pairs(Z, xs)]
    per = [(hip.HipVector(a).array, hip.HipVector(b).array) for a, b in H.apply_shifted_pairs(zs, xs, reverse=True)]
    return one, per, zs


@pytest.mark.parametrize("n", [1, 3, 65, 129, 257, 1000])
def test_block_products_of_every_width(hip, monkeypatch, n):
    A, X = _symmetric(n, 300 + n)
    Al, Xl = A.astype(LD), X.astype(LD)
    AX = Al @ Xl
    H = hip.HipCsrOperator.from_dense(A)
    H.set_block_variant(3)
    monkeypatch.delenv("HIPEIG_DENSE_GRID", raising=False)
    monkeypatch.delenv("HIPEIG_PAIR_BLOCK_WIDTH", raising=False)
    worst = 0.0
    for k in REAL_COUNTS:
        got = _block_products(hip, H, X, k)
        assert H.block_info()["variant"] == "dense"
        for j in range(k):
            b0 = product_bound(abs(A), X[:, j])
            worst = max(worst, _within(got[0][j], AX[:, j], b0, ("apply_block", n, k, j)))
            for g, sign in zip(got[1:], (1.0, -1.0)):
                ref = LD(sign) * (LD(SIGMA) * Xl[:, j] - AX[:, j])
                worst = max(worst, _within(g[j], ref, b0 + 4e-14 * SIGMA * np.abs(X[:, j]), ("apply_shifted_block", n, k, j, sign)))
        monkeypatch.setenv("HIPEIG_DENSE_GRID", "1")
        again = _block_products(hip, H, X, k)
        monkeypatch.delenv("HIPEIG_DENSE_GRID")
        assert all(np.array_equal(a, b) for ga, gb in zip(got, again) for a, b in zip(ga, gb)), (n, k)
    for npairs, width in PAIR_COUNTS:
        if width:
            monkeypatch.setenv("HIPEIG_PAIR_BLOCK_WIDTH", width)
        one, per, zs = _pair_products(hip, H, X, npairs)
        assert H.block_info()["variant"] == "dense"
        for p in range(npairs):
            xr, xi = Xl[:, 2 * p], Xl[:, 2 * p + 1]
            for (gr, gi), z, sign in ((one[p], Z, 1.0), (per[p], zs[p], -1.0)):
                yr = LD(sign) * (LD(z.real) * xr - LD(z.imag) * xi - AX[:, 2 * p])
                yi = LD(sign) * (LD(z.real) * xi + LD(z.imag) * xr - AX[:, 2 * p + 1])
                extra = 4e-14 * abs(z) * (np.abs(X[:, 2 * p]) + np.abs(X[:, 2 * p + 1]))
                worst = max(worst, _within(gr, yr, product_bound(abs(A), X[:, 2 * p]) + extra, ("pairs re", n, npairs, p, sign)))
                worst = max(worst, _within(gi, yi, product_bound(abs(A), X[:, 2 * p + 1]) + extra, ("pairs im", n, npairs, p, sign)))
        monkeypatch.setenv("HIPEIG_DENSE_GRID", "1")
        one1, per1, _ = _pair_products(hip, H, X, npairs)
        monkeypatch.delenv("HIPEIG_DENSE_GRID")
        assert all(np.array_equal(a, b) for pa, pb in zip(one + per, one1 + per1) for a, b in zip(pa, pb)), (n, npairs)
        if width:
            monkeypatch.delenv("HIPEIG_PAIR_BLOCK_WIDTH")
    info = H.dense_info()
    assert info["bytes"] == n * info["ld"] * 8 and info["block_workgroups"] >= 1
    print(f"dense block products n={n}: max error / bound {worst:.3e}")


# ---------------------------------------------------------------- refusals
def _refused(hip, H, x, message):
    X = hip.HipVector(x, ctx=H.ctx)
    with pytest.raises(_lib.HipEigError, match=message):
        H.set_block_variant(3)
        H.apply_block([X._buf])
    H.set_block_variant(0)
    return hip.HipVector(H.apply_block([X._buf])[0], ctx=H.ctx).array


def test_block_variant_refused_on_a_row_slice_a_rectangle_and_a_loopback_context(hip):
    from eigensolvers_amd.distributed import LoopbackGroup
    A, X = _symmetric(129, 3)
    x = X[:, 0].copy()
    H = hip.HipCsrOperator.from_scipy(sp.csr_matrix(A), row_begin=32, row_end=97)
    y = _refused(hip, H, x, "whole square operator")
    assert (np.abs(y - (A @ x)[32:97]) <= product_bound(abs(A[32:97]), x)).all()
    M = sp.random(40, 129, density=0.3, random_state=np.random.default_rng(4), format="csr")
    H = hip.HipCsrOperator.from_csr_arrays(M.indptr, M.indices, M.data, 129)
    y = _refused(hip, H, x, "whole square operator")
    assert (np.abs(y - M @ x) <= product_bound(abs(M).toarray(), x)).all()
    grp = LoopbackGroup(1)
    try:
        H = hip.HipCsrOperator.from_dense(A, ctx=grp.contexts[0])
        y = _refused(hip, H, x, "communicator")
        assert (np.abs(y - A @ x) <= product_bound(abs(A), x)).all()
        del H
    finally:
        grp.close()


# ---------------------------------------------------------------- block MINRES and the Lanczos filter
def _operator257(inside=False):
    """Dense symmetric n = 257: diagonal +-(2..4), small off-diagonal part (|lambda| > 0.4); `inside`: seven diagonal
    entries moved into [-0.2, 0.2], so that the filter of the contour of [-0.21, 0.21] has something to keep."""
    n = 257
    rng = np.random.default_rng(257)
    R = rng.standard_normal((n, n))
    d = rng.choice([-1.0, 1.0], n) * rng.uniform(2.0, 4.0, n)
    if inside:
        d[::40] = np.linspace(-0.2, 0.2, len(d[::40]))
    A = 0.005 * (R + R.T)
    A[np.diag_indices(n)] = d
    return A


@pytest.mark.parametrize("k", [3, 8])
def test_block_minres_columns_equal_the_single_solves(hip, k):
    A = _operator257()
    n = A.shape[0]
    B = np.random.default_rng(k).standard_normal((n, k))
    B /= np.linalg.norm(B, axis=0)
    H = hip.HipCsrOperator.from_dense(A, layout="dense")
    vecs = [hip.HipVector(B[:, j].copy(), minres_opts(2000, 1e-10)) for j in range(k)]
    X = hip.HipVector.solveBlock(H, vecs, 0.0)
    assert H.block_info()["variant"] == "dense" and len(X) == k
    for j in range(k):
        single = hip.HipVector.solve(H, hip.HipVector(B[:, j].copy(), minres_opts(2000, 1e-10)), 0.0)
        assert H.last_variant() == "dense"
        st, ss = X[j].last_solve_stats, single.last_solve_stats
        print(f"dense block MINRES k={k} column {j}: iterations {st['iterations']} (single {ss['iterations']}), istop {st['istop']}")
        assert (st["iterations"], st["istop"]) == (ss["iterations"], ss["istop"]), j
        assert np.linalg.norm(X[j].array - single.array) <= 1e-7 * np.linalg.norm(single.array), j
        r = B[:, j] - (0.0 * X[j].array - A @ X[j].array)
        assert np.linalg.norm(r) <= 1e-9


def test_lanczos_filter_on_the_dense_layout(hip):
    """Eight columns, n = 257: each filtered vector within the filter test's bound (``_lanczos_cases.check_filter``) of the
    exact filter, and within the same bound of the run with the automatic block variant."""
    A = _operator257(inside=True)
    Hh = sp.csr_matrix(A)
    n = A.shape[0]
    B = np.random.default_rng(9).standard_normal((8, n))
    B /= np.linalg.norm(B, axis=1)[:, None]
    rtol, atol = 1e-10, 1e-12
    H = hip.HipCsrOperator.from_dense(A)
    qa = [q.array for q in hip.lanczos_filter(H, device_columns(hip, B, rtol, atol), Z8, W8)]
    assert H.block_info()["variant"] != "dense"
    H.set_block_variant(3)
    qd = [q.array for q in hip.lanczos_filter(H, device_columns(hip, B, rtol, atol), Z8, W8)]
    assert H.block_info()["variant"] == "dense"
    from _lanczos_cases import filter_bound, spectrum
    lam, U = spectrum("dense-layout-257", Hh)
    for r in range(8):
        its, est, conv, xnorms = twin(("dense-layout-257", r), Hh, B[r], Z8, rtol, atol, 1.0)
        assert conv.all()
        check_filter(f"dense layout column {r}", "dense-layout-257", Hh, B[r], qd[r], Z8, W8, xnorms, max(atol, rtol), 1.0)
        assert np.linalg.norm(qd[r] - qa[r]) <= filter_bound(Hh, lam, Z8, W8, xnorms, max(atol, rtol)), r
