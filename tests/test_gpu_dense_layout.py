"""The opt-in dense layout of the single-vector sweeps (``set_variant(6)``, csrc/dense.hip, csrc/dense_device.h): products,
fixed add order, refusals, the MINRES drivers that inherit the sweep through their row epilogues, and the reference's own
dense-``A`` test cases run with ``from_dense(A, layout="dense")``.

Every test fails without the feature: ``set_variant(6)`` raises "unknown variant" and ``from_dense`` has no ``layout``.

Products are compared with the ``np.longdouble`` product within ``_sweep_cases.product_bound``, 4e-14 of the row's absolute
sum; a shifted product counts ``|sigma x_i|`` as one more term of that sum.  The kernel's own worst case is
``(2 ceil(ncols / 128) + 6) * 2^-53`` of the sum (dense_device.h), below 2.5e-15 at these sizes: the bound is not tuned to it.
Sizes: odd n (a row start that is not 16-byte aligned without the padding), 63..65 and 127..129 (the lane step of 128
columns and its tail), 255 / 257, 1000 and 1023 (a row group that ends inside a workgroup)."""
import numpy as np
import pytest
import scipy.sparse as sp

import _precond_cases as pc
from _sweep_cases import SHIFT_SETS, check_against_twin, check_kernel_forms, check_residuals, minres_opts, product_bound, shifted_options
from conftest import load_golden
from eigensolvers_amd import _lib
from eigensolvers_amd import feast as pf
from eigensolvers_amd.generators import dense_test_matrix
from oracle.minres_ref import minres as minres_ref

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 257, 1000, 1023]
SIGMA = 0.37
LD = np.longdouble


def _symmetric(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    return (A + A.T) / 2, rng.standard_normal(n)


def _reference(A, x, sigma=0.0, sign=0.0):
    """A x, or sign (sigma x - A x), in extended precision."""
    y = A.astype(LD) @ x.astype(LD)
    return y if sign == 0 else LD(sign) * (LD(sigma) * x.astype(LD) - y)


def _within(got, ref, bound, label):
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    print(f"dense {label}: max error / bound {np.max(err / bound):.3e}")
    assert (err <= bound).all(), (label, float(np.max(err / bound)))


def _products(hip, H, x):
    """(A x, sigma x - A x, -(sigma x - A x)) of the operator as it is pinned."""
    X = hip.HipVector(x, ctx=H.ctx)
    out = [X.applyOp(H).array]
    for reverse in (False, True):
        y = H.ctx.alloc(H.nrows)
        H.apply_shifted(SIGMA, X._buf, y, reverse=reverse)
        out.append(hip.HipVector(y, ctx=H.ctx).array)
    return out


def _check_products(hip, H, A, absA, x, label):
    """All three products of the dense sweep against the extended-precision ones of the host matrix A."""
    H.set_variant(6)
    got = _products(hip, H, x)
    assert H.last_variant() == "dense"
    bound = product_bound(absA, x)
    _within(got[0], _reference(A, x), bound, f"{label} apply")
    for g, sign in zip(got[1:], (1.0, -1.0)):
        _within(g, _reference(A, x, SIGMA, sign), bound + 4e-14 * abs(SIGMA) * np.abs(x), f"{label} shifted {sign:+.0f}")
    return got


@pytest.mark.parametrize("n", SIZES)
def test_products_of_a_dense_symmetric_operator(hip, n):
    A, x = _symmetric(n, 100 + n)
    H = hip.HipCsrOperator.from_dense(A)
    before = H.device_bytes
    assert H.dense_info()["bytes"] == 0
    _check_products(hip, H, A, abs(A), x, f"n={n}")
    info = H.dense_info()
    assert info["rows"] == info["cols"] == n and info["ld"] >= n and (info["ld"] * 8) % 16 == 0
    assert info["bytes"] == n * info["ld"] * 8 and info["rows_per_wave"] >= 1
    assert info["workgroups"] == min(-(-n // (4 * info["rows_per_wave"])), 2048)
    assert H.device_bytes == before + info["bytes"]
    H.set_variant(0)                                                # the other layouts stay usable next to the copy
    np.testing.assert_allclose(hip.HipVector(x).applyOp(H).array, A @ x, rtol=0, atol=float(np.max(product_bound(abs(A), x))))


def test_from_dense_with_the_dense_layout_pins_both_variants(hip):
    A, x = _symmetric(65, 7)
    H = hip.HipCsrOperator.from_dense(A, layout="dense")
    y = hip.HipVector(x).applyOp(H).array
    assert H.last_variant() == "dense"
    _within(y, _reference(A, x), product_bound(abs(A), x), "from_dense(layout='dense')")
    ys = H.apply_block([hip.HipVector(x)._buf])
    assert H.block_info()["variant"] == "dense"
    _within(hip.HipVector(ys[0]).array, _reference(A, x), product_bound(abs(A), x), "from_dense(layout='dense') block")
    with pytest.raises(ValueError, match="layout"):
        hip.HipCsrOperator.from_dense(A, layout="rows")
    H0 = hip.HipCsrOperator.from_dense(A)                           # layout=None: the automatic choice, as before
    hip.HipVector(x).applyOp(H0)
    assert H0.last_variant() == "csr-stream" and H0.dense_info()["bytes"] == 0


def test_absent_entries_read_as_zero(hip):
    """A from_scipy operator of density 0.1 with empty rows."""
    n = 257
    rng = np.random.default_rng(31)
    R = sp.random(n, n, density=0.1, random_state=rng, format="lil")
    for r in (0, 5, 64, 200, 256):
        R[r, :] = 0
    R = R.tocsr()
    R.eliminate_zeros()
    assert (np.diff(R.indptr) == 0).sum() >= 5
    x = rng.standard_normal(n)
    H = hip.HipCsrOperator.from_scipy(R)
    got = _check_products(hip, H, R.toarray(), abs(R.toarray()), x, "scipy 0.1")
    empty = np.diff(R.indptr) == 0
    assert np.array_equal(got[0][empty], np.zeros(int(empty.sum())))


def test_duplicate_entries_and_unsorted_rows(hip):
    """Rows of 0..150 stored entries in random column order with repeats: more than one step of 64 per row, columns that
    recur inside a step and across steps.  The copy holds the sum of the entries stored at a position."""
    n = 130
    rng = np.random.default_rng(47)
    lens = rng.integers(0, 151, n)
    lens[3] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    col[rowptr[10]:rowptr[10] + min(lens[10], 70)] = 9            # one column many times, across a step boundary
    val = rng.standard_normal(len(col))
    rows = np.repeat(np.arange(n), lens)
    A = np.zeros((n, n))
    np.add.at(A, (rows, col), val)
    absA = np.zeros((n, n))
    np.add.at(absA, (rows, col), np.abs(val))
    assert (np.bincount(rows * n + col) > 1).any() and (np.diff(col[rowptr[1]:rowptr[2]]) < 0).any()
    x = rng.standard_normal(n)
    H = hip.HipCsrOperator.from_csr_arrays(rowptr, col, val, n)
    got = _check_products(hip, H, A, absA, x, "duplicates")
    H.set_variant(1)
    ref1 = _products(hip, H, x)
    assert H.last_variant() == "csr-vector"
    bound = product_bound(absA, x)
    for g, r in zip(got, ref1):
        assert (np.abs(g - r) <= bound + 4e-14 * abs(SIGMA) * np.abs(x)).all()


def test_pair_products_are_the_two_real_sweeps(hip):
    """Variant 6 takes the two-sweep form of the pair product: with a real shift the halves are the real products bit for
    bit; a complex shift adds the zi terms to them with the library's two-stream update (``hipeig_axpby``), so the halves
    are, bit for bit, the real shifted products followed by that update - and they meet the extended-precision bound."""
    n = 257
    A, xr = _symmetric(n, 5)
    xi = np.random.default_rng(6).standard_normal(n)
    H = hip.HipCsrOperator.from_dense(A, layout="dense")
    ctx = H.ctx
    Xr, Xi = hip.HipVector(xr), hip.HipVector(xi)

    def real(x, sigma=None):
        y = ctx.alloc(n)
        H.apply(x._buf, y) if sigma is None else H.apply_shifted(sigma, x._buf, y)
        return hip.HipVector(y).array

    yr, yi = ctx.alloc(n), ctx.alloc(n)
    H.apply_pair(Xr._buf, Xi._buf, yr, yi)
    assert not H.pair_info()["fused"] and H.last_variant() == "dense"
    assert np.array_equal(hip.HipVector(yr).array, real(Xr)) and np.array_equal(hip.HipVector(yi).array, real(Xi))
    H.apply_shifted_pair(SIGMA, Xr._buf, Xi._buf, yr, yi)
    assert np.array_equal(hip.HipVector(yr).array, real(Xr, SIGMA)) and np.array_equal(hip.HipVector(yi).array, real(Xi, SIGMA))
    z = SIGMA + 0.21j
    H.apply_shifted_pair(z, Xr._buf, Xi._buf, yr, yi)
    for reverse in (False, True):                                 # yr = s (zr xr - A xr) - s zi xi, yi = s (zr xi - A xi) + s zi xr
        sign = -1.0 if reverse else 1.0
        pr, pi, cr, ci = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
        H.apply_shifted_pair(z, Xr._buf, Xi._buf, pr, pi, reverse=reverse)
        H.apply_shifted(z.real, Xr._buf, cr, reverse=reverse)
        H.apply_shifted(z.real, Xi._buf, ci, reverse=reverse)
        _lib.call("hipeig_axpby", ctx.handle, n, -sign * z.imag, Xi._buf.ptr, 1.0, cr.ptr)
        _lib.call("hipeig_axpby", ctx.handle, n, sign * z.imag, Xr._buf.ptr, 1.0, ci.ptr)
        assert np.array_equal(hip.HipVector(pr).array, hip.HipVector(cr).array), reverse
        assert np.array_equal(hip.HipVector(pi).array, hip.HipVector(ci).array), reverse
    ref = LD(1) * (z.real * (xr.astype(LD)) - A.astype(LD) @ xr.astype(LD)) - LD(z.imag) * xi.astype(LD)
    imf = LD(1) * (z.real * (xi.astype(LD)) - A.astype(LD) @ xi.astype(LD)) + LD(z.imag) * xr.astype(LD)
    extra = 4e-14 * abs(z) * (np.abs(xr) + np.abs(xi))
    _within(hip.HipVector(yr).array, ref, product_bound(abs(A), xr) + extra, "pair re")
    _within(hip.HipVector(yi).array, imf, product_bound(abs(A), xi) + extra, "pair im")


def test_fixed_order_across_calls_and_grids(hip, monkeypatch):
    """n = 1000: 63 row groups.  The default grid gives every group its own workgroup; HIPEIG_DENSE_GRID = 1 and 3 make one
    and three workgroups walk them (the persistent loop).  The bits do not move."""
    n = 1000
    A, x = _symmetric(n, 77)
    H = hip.HipCsrOperator.from_dense(A, layout="dense")
    monkeypatch.delenv("HIPEIG_DENSE_GRID", raising=False)
    ref = _products(hip, H, x)
    assert H.dense_info()["workgroups"] == 63
    for a, b in zip(ref, _products(hip, H, x)):
        assert np.array_equal(a, b)
    for cap in (1, 3):
        monkeypatch.setenv("HIPEIG_DENSE_GRID", str(cap))
        got = _products(hip, H, x)
        assert H.dense_info()["workgroups"] == cap
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), cap


# ---------------------------------------------------------------- refusals
def _refused(hip, H, x, message):
    """set_variant(6) or the first product raises with `message`; the operator then works with the automatic choice."""
    X = hip.HipVector(x, ctx=H.ctx)
    with pytest.raises(_lib.HipEigError, match=message):
        H.set_variant(6)
        X.applyOp(H)
    H.set_variant(0)
    return X.applyOp(H).array


def test_refused_on_a_row_slice(hip):
    A, x = _symmetric(129, 3)
    H = hip.HipCsrOperator.from_scipy(sp.csr_matrix(A), row_begin=32, row_end=97)
    y = _refused(hip, H, x, "whole square operator")
    assert (np.abs(y - (A @ x)[32:97]) <= product_bound(abs(A[32:97]), x)).all()


def test_refused_on_a_rectangular_operator(hip):
    rng = np.random.default_rng(4)
    M = sp.random(40, 65, density=0.3, random_state=rng, format="csr")
    H = hip.HipCsrOperator.from_csr_arrays(M.indptr, M.indices, M.data, 65)
    x = rng.standard_normal(65)
    y = _refused(hip, H, x, "whole square operator")
    assert (np.abs(y - M @ x) <= product_bound(abs(M).toarray(), x)).all()


def test_refused_on_a_context_with_a_loopback_group(hip):
    from eigensolvers_amd.distributed import LoopbackGroup
    A, x = _symmetric(65, 9)
    grp = LoopbackGroup(1)
    try:
        H = hip.HipCsrOperator.from_dense(A, ctx=grp.contexts[0])
        y = _refused(hip, H, x, "communicator")
        assert H.dense_info()["bytes"] == 0
        assert (np.abs(y - A @ x) <= product_bound(abs(A), x)).all()
        del H
    finally:
        grp.close()


# ---------------------------------------------------------------- MINRES
def _dominant257():
    """Dense symmetric n = 257, diagonal +-(2..4), off-diagonal row sums ~1.5: diagonally dominant, |lambda| > 0.4, so
    sigma = 0, the real shift 0.5 and the contour of [-0.21, 0.21] all keep clear of the spectrum."""
    n = 257
    rng = np.random.default_rng(257)
    R = rng.standard_normal((n, n))
    d = rng.choice([-1.0, 1.0], n) * rng.uniform(2.0, 4.0, n)
    A = 0.005 * (R + R.T)
    A[np.diag_indices(n)] = d
    b = rng.standard_normal(n)
    return A, b / np.linalg.norm(b)


def _minres_cases():
    A100 = dense_test_matrix(100, 1212)[0]
    b100 = np.random.default_rng(100).standard_normal(100)
    A257, b257 = _dominant257()
    return [("dense100", A100, b100 / np.linalg.norm(b100), -20.0), ("dominant257", A257, b257, 0.0)]


@pytest.mark.parametrize("case", _minres_cases(), ids=lambda c: c[0])
def test_minres_counts_equal_the_oracle_and_the_kernel_forms_agree(hip, monkeypatch, case):
    name, A, b, sigma = case
    xo, info, itn, istop = minres_ref(lambda v: sigma * v - A @ v, b, rtol=1e-10, maxiter=2000)
    H = hip.HipCsrOperator.from_dense(A, layout="dense")

    def solve():
        W = hip.HipVector.solve(H, hip.HipVector(b.copy(), minres_opts(2000, 1e-10)), sigma)
        return W.array, W.last_solve_stats

    monkeypatch.delenv("HIPEIG_MINRES_FUSE_KD", raising=False)
    x2, s2 = solve()
    assert H.last_variant() == "dense"
    monkeypatch.setenv("HIPEIG_MINRES_FUSE_KD", "0")
    x3, s3 = solve()
    monkeypatch.delenv("HIPEIG_MINRES_FUSE_KD")
    print(f"dense MINRES {name}: iterations {s2['iterations']} / {s3['iterations']} (oracle {itn}), istop {s2['istop']} ({istop})")
    check_kernel_forms(name, True, x2, s2, x3, s3, xo, itn, istop)


def test_jacobi_preconditioned_minres_tracks_the_twin(hip):
    A, b = _dominant257()
    tw = pc.twin("dense-layout-257", A, b, 0.0, 1e-10, 2000)
    H = hip.HipCsrOperator.from_dense(A, layout="dense")
    opts = minres_opts(2000, 1e-10)
    opts["linearSystemArgs"]["preconditioner"] = "jacobi"
    W = hip.HipVector.solve(H, hip.HipVector(b.copy(), opts), 0.0)
    assert H.last_variant() == "dense"
    check_against_twin("dense layout n=257", A, b, 0.0, 1e-10, W, tw)


def test_shifted_minres_residuals(hip):
    A, b = _dominant257()
    H = hip.HipCsrOperator.from_dense(A, layout="dense")
    bd = hip.HipVector(b.copy(), shifted_options(1e-10, 1e-12))
    xs = hip.solve_shifts(H, bd, SHIFT_SETS[3])
    assert H.last_variant() == "dense" and len(xs) == 3
    check_residuals(sp.csr_matrix(A), b, SHIFT_SETS[3], xs, 1.0, 1e-10, 1e-12)


# ---------------------------------------------------------------- the reference's dense drivers
def test_reference_lanczos_unit_tests_with_the_dense_layout(hip):
    """The two Lanczos runs of test_reference_unit_tests_with_gcrotmk_on_device on from_dense(A, layout="dense")."""
    opt = lambda: {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 1000, "linear_tol": 1e-4}}
    g = load_golden("lanczos_n100_seed1212.npz")
    A, exact = dense_test_matrix(100, 1212)
    H = hip.HipCsrOperator.from_dense(A, layout="dense")
    ev, Y, st = hip.inexactLanczosDiagonalization(H, hip.HipVector(g["guess"].copy(), opt()), 30, 6, 4, 1e-6, writeOut=False)
    assert H.last_variant() == "dense"
    assert st["cumIter"] == int(g["cumIter"]) and st["isConverged"]
    np.testing.assert_allclose(ev[:2], g["ev"], rtol=1e-6)
    assert abs(hip.find_nearest(ev, 30)[1] - hip.find_nearest(exact, 30)[1]) <= 1e-4
    gb = load_golden("block3_degenerate.npz")
    Ab, _ = dense_test_matrix(100, 1212, gb["exact"])
    Hb = hip.HipCsrOperator.from_dense(Ab, layout="dense")
    v0 = [hip.HipVector(gb["guess"][:, i].copy(), opt()) for i in range(3)]
    ev, Y, st = hip.inexactLanczosDiagonalization(Hb, v0, gb["exact"][5] + 1.5, 6, 4, 1e-6, writeOut=False)
    assert Hb.last_variant() == "dense"
    assert st["cumIter"] == int(gb["cumIter"])
    np.testing.assert_allclose(ev[:3], gb["exact"][5:8], rtol=1e-6)


def test_reference_lindep_case_with_the_dense_layout(hip):
    """test_reference_lindep_test_case_on_device (dense n = 1200) on the dense layout, to that test's assertions."""
    import sys
    import warnings
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    from make_golden_r2 import LINDEP, lindep_case
    g = load_golden("lindep_dense_n1200.npz")
    A, y0 = lindep_case()
    H = hip.HipCsrOperator.from_dense(A, layout="dense")
    opt = lambda: {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": LINDEP["linearIter"], "linear_tol": LINDEP["linear_tol"]}}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev, Y, st = hip.inexactLanczosDiagonalization(H, hip.HipVector(y0.copy(), opt()), LINDEP["sigma"], LINDEP["L"], LINDEP["maxit"],
                                                      1e-12, writeOut=False)
    assert H.last_variant() == "dense" and H.dense_info()["bytes"] == 1200 * H.dense_info()["ld"] * 8
    assert st["isConverged"] and not st["lindep"] and st["outerIter"] == 0 and st["futileRestarts"] == 0
    assert abs(st["cumIter"] - int(g["cumIter_a"])) <= 2 and len(Y) == st["cumIter"] + 1
    np.testing.assert_allclose(ev[:3], g["ev_a"][:3], rtol=1e-9)
    exact = np.linspace(1, 400, 1200)
    assert abs(ev[0] - exact[np.argmin(np.abs(exact - 390))]) < 1e-6
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev, Y, st = hip.inexactLanczosDiagonalization(H, hip.HipVector(y0.copy(), opt()), LINDEP["sigma"], LINDEP["L"], LINDEP["maxit"],
                                                      1e-18, writeOut=False)
    assert (st["outerIter"], st["cumIter"], st["isConverged"]) == (int(g["outerIter_b"]), int(g["cumIter_b"]), False)
    assert np.all(np.isnan(ev)) and len(Y) == int(g["nvec_b"]) == st["innerIter"]


def test_feast_reference_problem_with_the_dense_layout(hip):
    """test_gpu_feast.py's n = 100 known-answer run on the dense layout, to that test's bounds."""
    g = load_golden("feast_n100.npz")
    A = g["A"]
    H = hip.HipCsrOperator.from_dense(A, layout="dense")
    opts = lambda: {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 1000, "linear_tol": 1e-2}}
    Y = [hip.HipVector(g["guess"][:, i].copy(), opts()) for i in range(6)]
    ev, Yf, st = pf.feastDiagonalization(H, Y, 8, "legendre", 160.0, 166.0, 1e-10, 20, writeOut=False)
    assert H.last_variant() == "dense"
    assert len(Yf) == int(g["nvec"]) and abs(st["outerIter"] - int(g["outerIter"])) <= 2
    exact = np.linalg.eigvalsh(A)
    inside = pf.select_within_range(exact, 160.0, 166.0)[0]
    found = pf.select_within_range(ev, 160.0, 166.0)[0]
    assert len(inside) == len(found) == 3
    np.testing.assert_allclose(found, inside, atol=1e-4)
    np.testing.assert_allclose(found, pf.select_within_range(g["ev"], 160.0, 166.0)[0], rtol=1e-6)
    np.testing.assert_allclose(hip.HipVector.overlapMatrix(Yf), np.eye(len(Yf)), atol=1e-5)
