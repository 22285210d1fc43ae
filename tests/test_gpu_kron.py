"""``HipKronSumOperator`` on the device: its products against integers (bit for bit) and against longdouble (row bound),
and the solvers it inherits against the oracle on the explicit matrix of the same operator (``to_scipy()``)."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import scipy.linalg as la
import scipy.sparse.linalg as spla

import _kron_cases as kc
import _precond_cases as pc
from conftest import REPO
from eigensolvers_amd import _lib
from eigensolvers_amd.generators import coupled_oscillator_grid, guess_vector, sinc_dvr_harmonic
from oracle import lanczos_ref
from oracle.minres_ref import minres as minres_ref
from oracle.numpy_vector import RefVector

pytestmark = pytest.mark.gpu

GRID = ((13, 10, 7), [(-5, 5), (-4.5, 4.5), (-4, 4)], [1.0, 1.3, 1.7])
COMBOS = [(with_v, symmetric) for with_v in (False, True) for symmetric in (True, False)]


def _opts(solver="minres", it=4000, tol=1e-10, **lsa):
    d = {"linearSolver": solver, "linearIter": it, "linear_tol": tol, "linear_atol": 1e-14}
    d.update(lsa)
    return {"linearSystemArgs": d}


def _operator(hip, dims, seed, with_v, symmetric, integer=False):
    factors = kc.factors_for(dims, seed, symmetric, integer)
    V = kc.diag_for(dims, seed, integer) if with_v else None
    return hip.HipKronSumOperator.from_factors(factors, diag=V, check=symmetric), factors, V


# ---------------------------------------------------------------------------------------------------- products
@pytest.mark.parametrize("dims", kc.SHAPES)
def test_integer_product_is_exact(hip, dims):
    """Integer factors, V and x in [-8, 8]: every partial sum is an integer far below 2^53, so any correct order of the
    adds gives the integer result bit for bit - lane maps and masks without a tolerance."""
    n = kc.size(dims)
    for with_v, symmetric in COMBOS:
        H, factors, V = _operator(hip, dims, 11, with_v, symmetric, integer=True)
        assert H.dims == tuple(dims) and H.shape == (n, n) and H.dtype == np.float64 and H.nnz == 0
        x = kc.operand(n, 5, integer=True)
        want = np.asarray(kc.kron_apply_ld(factors, V, x)[0], dtype=np.float64)
        X = hip.HipVector(x.copy())
        np.testing.assert_array_equal(X.applyOp(H).array, want)
        np.testing.assert_array_equal((H @ X).array, want)


@pytest.mark.parametrize("dims", kc.SHAPES)
def test_product_row_bound_and_kernel_forms(hip, dims):
    n = kc.size(dims)
    for with_v, symmetric in COMBOS:
        H, factors, V = _operator(hip, dims, 21, with_v, symmetric)
        x = kc.operand(n, 6)
        ref, S = kc.kron_apply_ld(factors, V, x)
        X = hip.HipVector(x.copy())
        Y = X.applyOp(H)
        ratio = kc.within(Y.array, ref, kc.product_bound(dims, S))
        print(f"dims {dims} V {with_v} sym {symmetric}: worst |err| / bound = {ratio:.3f}")
        # twice the same bits; the operand is untouched and the result is no alias of it
        np.testing.assert_array_equal(X.applyOp(H).array, Y.array)
        np.testing.assert_array_equal(X.array, x)
        assert Y._buf.ptr != X._buf.ptr
    info = H.kron_info()
    strides = [kc.size(dims[d + 1:]) for d in range(len(dims))]
    want = ["plain" if nd == 1 else "mfma-last" if s == 1 else "mfma" if s >= 16 else "plain" for nd, s in zip(dims, strides)]
    assert info["kernels"] == want and info["launches"] == len(dims) + 1 and info["modes"] == len(dims)
    assert info["padded"] == [((nd + 15) // 16 * 16, (nd + 3) // 4 * 4) for nd in dims]
    assert H.last_variant() == "kronecker-sum" and H.launches_per_apply() == 1
    assert H.device_bytes >= info["raw_bytes"] == 8 * n
    assert H.algorithmic_bytes() == (3 * len(dims) + 2) * 8 * n + 8 * sum(nd * nd for nd in dims)


@pytest.mark.parametrize("dims", kc.SHAPES)
def test_shifted_and_complex_products(hip, dims):
    n = kc.size(dims)
    H, factors, V = _operator(hip, dims, 31, True, False)
    xr, xi = kc.operand(n, 7), kc.operand(n, 8)
    (ar, Sr), (ai, Si) = kc.kron_apply_ld(factors, V, xr), kc.kron_apply_ld(factors, V, xi)
    Xr, Xi = hip.HipVector(xr.copy()), hip.HipVector(xi.copy())
    lr, li = np.asarray(xr, dtype=kc.LD), np.asarray(xi, dtype=kc.LD)
    ctx = Xr.ctx
    for sigma in (0.37, -25.0, 1e-3):
        for reverse in (False, True):
            s = -1.0 if reverse else 1.0
            out = ctx.alloc(n)
            H.apply_shifted(sigma, Xr._buf, out, reverse=reverse)
            kc.within(hip.HipVector(out).array, s * (kc.LD(sigma) * lr - ar), kc.shifted_bound(dims, Sr, sigma, xr))
    for z in (0.37 - 1.9j, 1e-3 + 1e2j, 0.3j):
        for reverse in (False, True):
            s = -1.0 if reverse else 1.0
            yr, yi = ctx.alloc(n), ctx.alloc(n)
            H.apply_shifted_pair(z, Xr._buf, Xi._buf, yr, yi, reverse=reverse)
            zr, zi = kc.LD(z.real), kc.LD(z.imag)
            kc.within(hip.HipVector(yr).array, s * (zr * lr - zi * li - ar), kc.pair_bound(dims, Sr, z.real, z.imag, xr, xi))
            kc.within(hip.HipVector(yi).array, s * (zr * li + zi * lr - ai), kc.pair_bound(dims, Si, z.real, z.imag, xi, xr))
    Z = hip.HipComplexVector(xr + 1j * xi).applyOp(H)
    kc.within(Z.re.array, ar, kc.product_bound(dims, Sr))
    kc.within(Z.im.array, ai, kc.product_bound(dims, Si))


@pytest.mark.parametrize("dims", kc.SHAPES)
def test_diagonal_equals_the_explicit_matrix(hip, dims):
    for with_v, symmetric in COMBOS:
        H, factors, V = _operator(hip, dims, 41, with_v, symmetric)
        np.testing.assert_array_equal(hip.HipVector(H.diagonal()).array, H.to_scipy().diagonal())
        assert H.diagonal() is H.diagonal()
    assert abs(H.to_scipy() - hip.HipKronSumOperator.explicit_matrix(factors, V)).max() == 0.0


def test_matrix_representation_and_block_loop(hip):
    dims = (7, 5, 9)
    H, factors, V = _operator(hip, dims, 51, True, True)
    Hs = H.to_scipy()
    Q = la.qr(np.random.default_rng(3).standard_normal((kc.size(dims), 4)), mode="economic")[0]
    vs = [hip.HipVector(Q[:, j].copy()) for j in range(4)]
    M = hip.HipVector.matrixRepresentation(H, vs)
    np.testing.assert_allclose(M, Q.T @ (Hs @ Q), rtol=0, atol=1e-12 * abs(Hs).sum(axis=1).max())
    M3 = hip.HipVector.matrixRepresentation(H, vs[:3])
    np.testing.assert_allclose(hip.HipVector.extendMatrixRepresentation(H, vs, M3), M, rtol=0, atol=1e-12 * abs(Hs).sum(axis=1).max())
    ys = H.apply_block([v._buf for v in vs])
    for v, y in zip(vs, ys):
        np.testing.assert_array_equal(hip.HipVector(y).array, v.applyOp(H).array)


# ---------------------------------------------------------------------------------------------------- solvers
@pytest.fixture(scope="module")
def grid(hip):
    dims, ranges, freqs = GRID
    factors, V = coupled_oscillator_grid(dims, ranges, freqs)
    H = hip.HipKronSumOperator.from_factors(factors, diag=V)
    Hs = H.to_scipy()
    lam = np.linalg.eigvalsh(Hs.toarray())
    sigma = 0.513 * lam[3] + 0.487 * lam[4]
    b = guess_vector(kc.size(dims), 1)
    b = b / np.linalg.norm(b)
    b.setflags(write=False)
    return {"H": H, "Hs": Hs, "lam": lam, "sigma": float(sigma), "b": b, "factors": factors, "V": V}


def _problem(hip, dims, grid):
    """(H, explicit matrix, sigma, b, factors, V): the fixture's grid, or the same oscillator on other dims."""
    if dims == GRID[0]:
        return grid["H"], grid["Hs"], grid["sigma"], grid["b"], grid["factors"], grid["V"]
    D = len(dims)
    # (17, 3): N = 51 and MINRES at rtol 1e-10 runs close to the exhaustion of the Krylov space, where the stopping quantity
    # moves by 20 % between two host roundings of the products; of the ranges (-4.5, 4.5), (-4, 4), (-3, 3) for its second
    # mode the last is the first whose count _count_is_posed accepts at both tolerances
    ranges = [(-5, 5), (-3, 3)] if dims == (17, 3) else [(-5, 5), (-4.5, 4.5), (-4, 4), (-3.5, 3.5)][:D]
    factors, V = coupled_oscillator_grid(dims, ranges, [1.0, 1.3, 1.7, 2.1][:D])
    H = hip.HipKronSumOperator.from_factors(factors, diag=V)
    Hs = H.to_scipy()
    lam = np.linalg.eigvalsh(Hs.toarray())
    b = guess_vector(kc.size(dims), 1)
    return H, Hs, float(0.513 * lam[3] + 0.487 * lam[4]), b / np.linalg.norm(b), factors, V


def _count_is_posed(Hs, factors, V, sigma, b, rtol, itn, istop):
    """The oracle's iteration count is a property of the problem, and not of the rounding of its products, where a second
    host rounding of H x (mode by mode in float64 instead of the CSR product) stops at the same iteration for the same
    reason AND the deciding quantity ``test1`` is further from ``rtol`` than the two roundings are from each other, at the
    stopping iteration (below) and at the one before (above).  Host only: the device is asked for the count afterwards."""
    ta, tb = [], []
    minres_ref(lambda v: sigma * v - Hs @ v, b, rtol=rtol, maxiter=4000, trace=ta)
    second = minres_ref(lambda v: sigma * v - kc.kron_apply_f64(factors, V, v), b, rtol=rtol, maxiter=4000, trace=tb)
    if second[2:] != (itn, istop) or istop != 1:
        return False
    stop, prev = (ta[-1]["test1"], tb[-1]["test1"]), (ta[-2]["test1"], tb[-2]["test1"])
    return max(stop) + abs(stop[0] - stop[1]) <= rtol and min(prev) - abs(prev[0] - prev[1]) > rtol


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("dims", [(13, 10, 7), (17, 3), (2, 3, 4, 5)])
def test_minres_tracks_the_oracle(hip, grid, monkeypatch, dims, rtol):
    H, Hs, sigma, b, factors, V = _problem(hip, dims, grid)
    trace = []
    xo, info, itn, istop = minres_ref(lambda v: sigma * v - Hs @ v, b, rtol=rtol, maxiter=4000, trace=trace)
    assert _count_is_posed(Hs, factors, V, sigma, b, rtol, itn, istop)
    W = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(tol=rtol)), sigma)
    st = W.last_solve_stats
    print(f"dims {dims} rtol {rtol}: iterations {st['iterations']} / oracle {itn}, istop {st['istop']} / {istop}")
    assert st["iterations"] == itn and st["istop"] == istop
    xtol = max(1e-9, 100 * rtol) * np.linalg.norm(xo)
    assert np.max(np.abs(W.array - xo)) <= xtol
    r = b - (sigma * W.array - Hs @ W.array)
    ro = b - (sigma * xo - Hs @ xo)
    assert np.linalg.norm(r) <= 1.05 * np.linalg.norm(ro) + 1e-13
    Wr = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(tol=rtol)), sigma, reverseGF=True)
    assert np.max(np.abs(Wr.array + xo)) <= xtol
    monkeypatch.setenv("HIPEIG_MINRES_FUSE_KD", "0")               # KD as its own kernel: same count, same iterate
    W3 = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(tol=rtol)), sigma)
    assert W3.last_solve_stats["iterations"] == itn and W3.last_solve_stats["istop"] == istop
    np.testing.assert_allclose(W3.array, W.array, rtol=0, atol=1e-12 * np.linalg.norm(xo))


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
def test_jacobi_minres_tracks_its_host_restatement(hip, grid, rtol):
    H, Hs, sigma, b = grid["H"], grid["Hs"], grid["sigma"], grid["b"]
    x, info, itn, istop, trace = pc.twin("kron_grid", Hs, b, sigma, rtol, 4000)
    W = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(tol=rtol, preconditioner="jacobi")), sigma)
    st = W.last_solve_stats
    print(f"jacobi rtol {rtol}: iterations {st['iterations']} / host {itn}, istop {st['istop']} / {istop}")
    assert st["iterations"] == itn and st["istop"] == istop and st["preconditioner"] == "jacobi"
    assert np.max(np.abs(W.array - x)) <= max(1e-9, 100 * rtol) * np.linalg.norm(x)


def test_shifted_minres_and_complex_right_hand_side(hip, grid):
    H, Hs, sigma, b = grid["H"], grid["Hs"], grid["sigma"], grid["b"]
    shifts = [sigma, sigma + 0.4j, sigma - 0.2 + 0.1j]
    xs = hip.solve_shifts(H, hip.HipVector(b.copy(), _opts("minres_shifted", tol=1e-8)), shifts)
    for z, x in zip(shifts, xs):
        assert np.linalg.norm(b - (z * x.array - Hs @ x.array)) <= 10 * 1e-8
    # a complex right-hand side with a real shift: MINRES on the two halves, each the oracle's solve of that half
    bc = b + 1j * np.roll(b, 5)
    W = hip.HipComplexVector.solve(H, hip.HipComplexVector(bc, _opts(tol=1e-10)), sigma)
    for half, got in ((bc.real, W.re), (bc.imag, W.im)):
        xo, info, itn, istop = minres_ref(lambda v: sigma * v - Hs @ v, half, rtol=1e-10, maxiter=4000)
        assert np.max(np.abs(got.array - xo)) <= max(1e-9, 100 * 1e-10) * np.linalg.norm(xo)


@pytest.mark.parametrize("shift", ["real", "complex"])
def test_gcrotmk(hip, grid, shift):
    """The residual on the explicit matrix, and the same solve through the CSR form of the operator: two GCROT runs that
    differ in the rounding of their products stop within a few steps of each other (the stopping test is looked at after
    every inner step and the residual falls by a bounded factor per step), so the product counts agree to 5 % + 2, and
    both solutions meet the same residual bound, so they agree to cond * rtol as in test_gcrotmk_tracks_scipy."""
    H, Hs, sigma, b = grid["H"], grid["Hs"], grid["sigma"], grid["b"]
    z = sigma if shift == "real" else sigma + 0.4j
    rtol = 1e-8
    W = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts("gcrotmk", tol=rtol)), z)
    x = W.array
    assert np.linalg.norm(b - (z * x - Hs @ x)) <= 10 * rtol * np.linalg.norm(b)
    Hc = hip.HipCsrOperator.from_scipy(Hs)
    Wc = hip.HipVector.solve(Hc, hip.HipVector(b.copy(), _opts("gcrotmk", tol=rtol)), z)
    n1, n2 = W.last_solve_stats["iterations"], Wc.last_solve_stats["iterations"]
    print(f"gcrotmk {shift}: products {n1} (Kronecker) / {n2} (CSR)")
    assert abs(n1 - n2) <= 0.05 * n2 + 2
    assert np.max(np.abs(x - Wc.array)) <= max(1e-9, 300 * rtol) * np.linalg.norm(Wc.array)
    if shift == "real":                                           # an initial guess
        W0 = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts("gcrotmk", tol=rtol)), z, x0=hip.HipVector(0.9 * x))
        assert np.linalg.norm(b - (z * W0.array - Hs @ W0.array)) <= 10 * rtol
        assert W0.last_solve_stats["iterations"] < n1


@pytest.mark.parametrize("solver,tol", [("minres", 1e-10), ("gcrotmk", 1e-8)])
def test_lanczos_single_vector(hip, grid, solver, tol):
    H, Hs, sigma, lam = grid["H"], grid["Hs"], grid["sigma"], grid["lam"]
    g = guess_vector(Hs.shape[0], 1)
    ev, Y, st = hip.inexactLanczosDiagonalization(H, hip.HipVector(g.copy(), _opts(solver, tol=tol)), sigma, 8, 10, 1e-12,
                                                  writeOut=False)
    evo, Yo, sto = lanczos_ref.inexact_lanczos(Hs, RefVector(g.copy(), _opts(solver, tol=tol)), sigma, 8, 10, 1e-12)
    near = lam[np.argmin(np.abs(lam - sigma))]
    print(f"lanczos {solver}: cumIter {st['cumIter']} / {sto['cumIter']}, converged {st['isConverged']} / {sto['isConverged']}, "
          f"|theta - lambda| / |lambda| = {abs(ev[0] - near) / abs(near):.2e} (oracle {abs(evo[0] - near) / abs(near):.2e})")
    assert st["cumIter"] == sto["cumIter"] and st["isConverged"] == sto["isConverged"]
    assert abs(ev[0] - near) <= 1e-10 * abs(near)


def test_lanczos_block_of_three_takes_the_one_by_one_path(hip, grid, monkeypatch):
    H, Hs, sigma = grid["H"], grid["Hs"], grid["sigma"]
    n = Hs.shape[0]
    Q = la.qr(np.random.default_rng(5).standard_normal((n, 3)), mode="economic")[0]
    called = []
    real_block = hip.HipVector._solve_block_minres
    monkeypatch.setattr(hip.HipVector, "_solve_block_minres", staticmethod(lambda *a, **k: called.append(1) or real_block(*a, **k)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev, Y, st = hip.inexactLanczosDiagonalization(H, [hip.HipVector(Q[:, i].copy(), _opts(tol=1e-10)) for i in range(3)],
                                                      sigma, 10, 4, 1e-10, writeOut=False)
        evo, Yo, sto = lanczos_ref.inexact_lanczos(Hs, [RefVector(Q[:, i].copy(), _opts(tol=1e-10)) for i in range(3)],
                                                   sigma, 10, 4, 1e-10)
    print(f"block lanczos: cumIter {st['cumIter']} / {sto['cumIter']}, converged {st['isConverged']} / {sto['isConverged']}, "
          f"max rel diff of five values {np.max(np.abs(ev[:5] - evo[:5]) / np.abs(evo[:5])):.2e}")
    assert not called
    assert st["cumIter"] == sto["cumIter"] and st["isConverged"] == sto["isConverged"] and sto["isConverged"]
    np.testing.assert_allclose(np.sort(ev)[:5], np.sort(evo)[:5], rtol=1e-10)


def test_separable_grid_gives_a_sum_of_factor_eigenvalues(hip):
    """A known answer with no CSR anywhere: without the coupling terms the spectrum is the sums of the factor spectra."""
    dims, ranges, freqs = GRID
    factors, V = coupled_oscillator_grid(dims, ranges, freqs, coupled=False)
    H = hip.HipKronSumOperator.from_factors(factors, diag=V)
    parts = [np.linalg.eigvalsh(T + np.diag((w * sinc_dvr_harmonic(T.shape[0], r)[1]) ** 2)) for T, r, w in zip(factors, ranges, freqs)]
    sums = np.sort(np.add.outer(np.add.outer(parts[0], parts[1]), parts[2]).reshape(-1))
    sigma = 0.513 * sums[3] + 0.487 * sums[4]
    g = guess_vector(kc.size(dims), 1)
    ev, Y, st = hip.inexactLanczosDiagonalization(H, hip.HipVector(g.copy(), _opts(tol=1e-10)), sigma, 8, 10, 1e-12, writeOut=False)
    near = sums[np.argmin(np.abs(sums - sigma))]
    assert st["isConverged"] and abs(ev[0] - near) <= 1e-10 * abs(near)


def test_feast_one_by_one_solves(hip, grid):
    H, Hs, lam = grid["H"], grid["Hs"], grid["lam"]
    n = Hs.shape[0]
    lo, hi = lam[0] - 0.5, 0.5 * (lam[2] + lam[3])
    Q = la.qr(np.random.default_rng(8).standard_normal((n, 5)), mode="economic")[0]
    Y0 = [hip.HipVector(Q[:, i].copy(), _opts("gcrotmk", tol=1e-8)) for i in range(5)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev, Y, st = hip.feastDiagonalization(H, Y0, 8, "legendre", lo, hi, 1e-9, 12, writeOut=False)
    ev = np.asarray(ev)
    inside = np.sort(ev[(ev >= lo) & (ev <= hi)])
    assert len(inside) == 3
    np.testing.assert_allclose(inside, lam[:3], atol=1e-4)                      # the bound of the reference's FEAST test


def test_lanczos_checkpoint_resume(hip, grid, tmp_path):
    """The product has one order of adds, so a run resumed from a checkpoint repeats the first run bit for bit."""
    H, sigma = grid["H"], grid["sigma"]
    g = guess_vector(H.nrows, 1)
    run = lambda **kw: hip.inexactLanczosDiagonalization(H, hip.HipVector(g.copy(), _opts(tol=1e-10)), sigma, 5, 6, 1e-12,
                                                         writeOut=False, **kw)
    d = str(tmp_path / "ck")
    ev, Y, st = run(checkpointDir=d, checkpointKeep=0)
    assert st["cumIter"] > 3
    ev2, Y2, st2 = run(resumeFrom=f"{d}/krylov_{3:06d}.npz")
    np.testing.assert_array_equal(ev2, ev)
    assert st2["cumIter"] == st["cumIter"]
    np.testing.assert_array_equal(Y2[0].array, Y[0].array)


# ---------------------------------------------------------------------------------------------------- refusals
def test_block_opt_ins_are_refused(hip, grid):
    H, sigma, b = grid["H"], grid["sigma"], grid["b"]
    n = len(b)
    bs = [hip.HipVector(np.roll(b, i).copy(), _opts(tol=1e-8, preconditioner="jacobi", preconditionerLockStep=True)) for i in range(3)]
    with pytest.raises(NotImplementedError, match="HipKronSumOperator"):
        hip.HipVector.solveBlock(H, bs, sigma)
    for call in (lambda: H.set_variant(2), lambda: H.set_block_variant(1), lambda: H.set_reproducible(True),
                 lambda: H.set_reduction("deterministic")):
        with pytest.raises(NotImplementedError, match="HipKronSumOperator"):
            call()
    Y0 = [hip.HipVector(np.roll(b, i).copy(), _opts("gcrotmk", tol=1e-8)) for i in range(2)]
    with pytest.raises(NotImplementedError, match="contourPool"):
        hip.feastDiagonalization(H, Y0, 8, "legendre", 0.0, 1.0, 1e-9, 2, writeOut=False, contourPool=True)
    Yf = [hip.HipVector(np.roll(b, i).copy(), _opts("lanczos_filter", tol=1e-8)) for i in range(2)]
    with pytest.raises(NotImplementedError, match="lanczos_filter"):
        hip.feastDiagonalization(H, Yf, 8, "legendre", 0.0, 1.0, 1e-9, 2, writeOut=False)
    # the C entry points of the block launchers: an error, not a zero product over the empty CSR arrays
    xs = [hip.HipVector(b.copy())._buf for _ in range(4)]
    ys = [xs[0].ctx.alloc(n) for _ in range(4)]
    from eigensolvers_amd.hip_vector import _ptr_table
    xt, k1 = _ptr_table(xs)
    yt, k2 = _ptr_table(ys)
    with pytest.raises(_lib.HipEigError, match="Kronecker"):
        _lib.call("hipeig_spmm", H.ctx.handle, H.handle, 4, xt, yt)
    with pytest.raises(_lib.HipEigError, match="Kronecker"):
        _lib.call("hipeig_csr_diagonal", H.ctx.handle, H.handle, ys[0].ptr)
    # the deterministic option of a vector is met as it stands; a larger factor than the kernels take is refused
    assert np.all(hip.HipVector(b.copy(), {"reduction": "deterministic"}).applyOp(H).array == hip.HipVector(b.copy()).applyOp(H).array)
    with pytest.raises(ValueError, match="1 <= n_d <= "):
        hip.HipKronSumOperator.from_factors([np.eye(H.kron_info()["max_factor"] + 1)])
    # automatic lock-step choices: one by one, with the single solve's results
    bs = [hip.HipVector(np.roll(b, i).copy(), _opts(tol=1e-8)) for i in range(3)]
    sols = hip.HipVector.solveBlock(H, bs, sigma)
    one = hip.HipVector.solve(H, hip.HipVector(np.roll(b, 1).copy(), _opts(tol=1e-8)), sigma)
    np.testing.assert_array_equal(sols[1].array, one.array)


def test_creation_under_forced_collectives_is_refused():
    """A context with a communicator (here one rank rehearsing the row partition) cannot create the operator.  A process of
    its own: the rehearsal flag is read when the communicator is attached."""
    code = (
        "import numpy as np, eigensolvers_amd as ea\n"
        "from eigensolvers_amd.distributed import LoopbackGroup\n"
        "g = LoopbackGroup(1)\n"
        "ctx = g.contexts[0]\n"
        "assert ctx.collectives\n"
        "try:\n"
        "    ea.HipKronSumOperator.from_factors([np.eye(4), np.eye(3)], ctx=ctx)\n"
        "except ValueError as e:\n"
        "    assert 'communicator' in str(e), e\n"
        "    print('refused')\n"
    )
    env = dict(os.environ, HIPEIG_FORCE_COLLECTIVES="1", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=REPO, timeout=120)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr
