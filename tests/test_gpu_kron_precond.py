"""The separable preconditioner of ``HipKronSumOperator`` on the device, through the public objects: every transform form
alone against integers (bit for bit) and against longdouble (row bound), the scale against its host statement, the
whole apply against longdouble, the preconditioned solves against their host twin, a Lanczos run, the refusals."""
import warnings

import numpy as np
import pytest

import _kron_cases as kc
import _kron_precond_cases as kp
from eigensolvers_amd.generators import guess_vector
from eigensolvers_amd.precond_minres import separable_scale_host

pytestmark = pytest.mark.gpu


def _opts(solver="minres", it=4000, tol=1e-10, **lsa):
    d = {"linearSolver": solver, "linearIter": it, "linear_tol": tol, "linear_atol": 1e-14}
    d.update(lsa)
    return {"linearSystemArgs": d}


def _down(hip, buf):
    return hip.HipVector(buf).array


def _with_bases(hip, dims, bases, seed=11):
    """An operator on ``dims`` (any factors) and its preconditioner with the given ``Q_d``; the eigenvalues play no part."""
    H = hip.HipKronSumOperator.from_factors(kc.factors_for(dims, seed))
    return H, H.separable_preconditioner(0.0, bases=bases, eigenvalues=[np.arange(1.0, n + 1.0) for n in dims])


# ---------------------------------------------------------------------------------------------------- one mode
@pytest.mark.parametrize("dims", kc.SHAPES)
def test_integer_transform_is_exact(hip, dims):
    """Integer ``Q`` and ``x`` in [-8, 8]: every partial sum is an integer far below 2^53, so any correct order of the adds
    gives the integer result bit for bit - lane maps, masks and the transposed copy without a tolerance."""
    n = kc.size(dims)
    bases = kc.factors_for(dims, 12, symmetric=False, integer=True)
    H, P = _with_bases(hip, dims, bases)
    x = kc.operand(n, 5, integer=True)
    X = hip.HipVector(x.copy())
    for d in range(len(dims)):
        for transpose in (False, True):
            want = np.asarray(kp.mode_apply_ld(bases[d], x, dims, d, transpose)[0], dtype=np.float64)
            got = P.transform(d, transpose, X._buf)
            np.testing.assert_array_equal(_down(hip, got), want)
            assert got.ptr != X._buf.ptr
    np.testing.assert_array_equal(X.array, x)


@pytest.mark.parametrize("dims", kc.SHAPES)
def test_transform_row_bound(hip, dims):
    n = kc.size(dims)
    bases = kc.factors_for(dims, 22, symmetric=False)
    H, P = _with_bases(hip, dims, bases)
    assert P.kernels() == kp.kernel_forms(dims)
    x = kc.operand(n, 6)
    X = hip.HipVector(x.copy())
    worst = 0.0
    for d in range(len(dims)):
        for transpose in (False, True):
            ref, S = kp.mode_apply_ld(bases[d], x, dims, d, transpose)
            got = _down(hip, P.transform(d, transpose, X._buf))
            worst = max(worst, kc.within(got, ref, kp.mode_bound(dims[d], S)))
            np.testing.assert_array_equal(_down(hip, P.transform(d, transpose, X._buf)), got)      # twice the same bits
    print(f"dims {dims} forms {P.kernels()}: worst |err| / bound = {worst:.3f}")


def test_all_three_forms_are_met(hip):
    met = set()
    for dims in kc.SHAPES:
        H, P = _with_bases(hip, dims, [np.eye(n) for n in dims])
        assert P.kernels() == kp.kernel_forms(dims) == H.kron_info()["kernels"]
        assert P.launches_per_apply == 2 * len(dims)
        met.update(P.kernels())
    assert met == {"mfma", "mfma-last", "plain"}


# ---------------------------------------------------------------------------------------------------- the scale
@pytest.mark.parametrize("dims", [(5,), (17, 3), (2, 3, 4, 5), (33, 20), (13, 10, 7)])
def test_scale_equals_the_host_statement(hip, dims):
    H = hip.HipKronSumOperator.from_factors(kc.factors_for(dims, 31), diag=kc.diag_for(dims, 31))
    for sigma, floor in ((0.37, 1e-8), (-2.5, 0.0), (0.37, 0.3)):
        P = H.separable_preconditioner(sigma, floor)
        np.testing.assert_array_equal(_down(hip, P.sinv()), separable_scale_host(P.eigenvalues, sigma, floor))
        assert P.sinv() is P.sinv() and H.separable_preconditioner(sigma, floor) is P
        assert P.device_bytes >= 8 * kc.size(dims) + 2 * 8 * sum(((n + 15) // 16 * 16) * ((n + 3) // 4 * 4) for n in dims)
    assert H.separable_preconditioner(1.0).bases is P.bases              # one decomposition per operator and potentials


def test_scale_refuses_an_exact_hit(hip):
    dims = (3, 4)
    H = hip.HipKronSumOperator.from_factors(kc.factors_for(dims, 32))
    lam = [np.array([1.0, 2.0, 4.0]), np.array([0.5, 8.0, 16.0, 32.0])]
    bases = [np.eye(3), np.eye(4)]
    with pytest.raises(ValueError, match="not finite"):
        H.separable_preconditioner(2.5, 0.0, bases=bases, eigenvalues=lam).sinv()           # Lam = 2 + 0.5 == sigma
    P = H.separable_preconditioner(2.5, 1e-3, bases=bases, eigenvalues=lam)
    np.testing.assert_array_equal(_down(hip, P.sinv()), separable_scale_host(lam, 2.5, 1e-3))


# ---------------------------------------------------------------------------------------------------- the apply
@pytest.mark.parametrize("dims", kc.SHAPES)
def test_apply_bound_symmetry_and_definiteness(hip, dims):
    n = kc.size(dims)
    H = hip.HipKronSumOperator.from_factors(kc.factors_for(dims, 41), diag=kc.diag_for(dims, 41))
    P = H.separable_preconditioner(0.37)
    sinv = separable_scale_host(P.eigenvalues, 0.37, 1e-8)
    smax = float(np.max(sinv))
    u, v = kc.operand(n, 8), kc.operand(n, 9)
    out = {}
    for name, r in (("u", u), ("v", v)):
        R = hip.HipVector(r.copy())
        z = _down(hip, P.apply(R._buf))
        ref = kp.apply_ld(P.bases, sinv, r)
        err = float(np.linalg.norm(np.asarray(z, dtype=kc.LD) - ref))
        bound = kp.apply_bound(dims, smax, np.linalg.norm(r))
        print(f"dims {dims} {name}: ||z - z_ld|| / bound = {err / bound:.3f}")
        assert err <= bound
        np.testing.assert_array_equal(R.array, r)
        assert float(np.dot(np.asarray(r, dtype=kc.LD), np.asarray(z, dtype=kc.LD))) > 0.0
        out[name] = (np.asarray(z, dtype=kc.LD), bound)
    (zu, bu), (zv, bv) = out["u"], out["v"]
    asym = abs(float(np.dot(np.asarray(u, dtype=kc.LD), zv) - np.dot(zu, np.asarray(v, dtype=kc.LD))))
    assert asym <= bv * np.linalg.norm(u) + bu * np.linalg.norm(v)
    # the operator's product is untouched by the applies that worked in its raw-sum buffer
    X = hip.HipVector(u.copy())
    y = X.applyOp(H).array
    P.apply(X._buf)
    np.testing.assert_array_equal(X.applyOp(H).array, y)


# ---------------------------------------------------------------------------------------------------- the solves
_operators = {}


def _device_problem(hip, dims):
    p = kp.problem(dims, solve=True)
    if dims not in _operators:
        _operators[dims] = hip.HipKronSumOperator.from_factors(p["factors"], diag=p["V"])
    return _operators[dims], p


@pytest.mark.parametrize("dims,rtol", kp.SOLVE_CASES)
def test_separable_minres_tracks_its_host_twin(hip, monkeypatch, dims, rtol):
    """Host twins (float64 / longdouble rounded): 19 / 19, 25 / 25, 11 / 11, 17 / 17, 17 / 17, 22 / 22, 20 / 20 iterations in
    the order of ``SOLVE_CASES``; ``_kron_precond_cases._ranges`` says which range the second mode of (17, 3) has here."""
    H, p = _device_problem(hip, dims)
    x, info, itn, istop, trace = kp.twin(dims, rtol, solve=True)
    other = kp.twin(dims, rtol, "ld", solve=True)
    print(f"dims {dims} rtol {rtol}: host twins {itn} / {other[2]} iterations, istop {istop} / {other[3]}, test1 at the stop "
          f"{trace[-1]['test1']:.3e} / {other[4][-1]['test1']:.3e}")
    assert kp.count_is_posed(dims, rtol)
    sigma, b = p["sigma"], p["b"]
    o = lambda: _opts(tol=rtol, preconditioner="separable")
    W = hip.HipVector.solve(H, hip.HipVector(b.copy(), o()), sigma)
    st = W.last_solve_stats
    print(f"dims {dims} rtol {rtol}: iterations {st['iterations']} / host {itn}, istop {st['istop']} / {istop}")
    assert st["iterations"] == itn and st["istop"] == istop and st["preconditioner"] == "separable"
    xtol = max(1e-9, 100 * rtol) * np.linalg.norm(x)
    assert np.max(np.abs(W.array - x)) <= xtol
    Wr = hip.HipVector.solve(H, hip.HipVector(b.copy(), o()), sigma, reverseGF=True)
    assert Wr.last_solve_stats["iterations"] == itn and np.max(np.abs(Wr.array + x)) <= xtol
    monkeypatch.setenv("HIPEIG_MINRES_FUSE_KD", "0")               # KD as its own kernel: same count, same iterate
    W3 = hip.HipVector.solve(H, hip.HipVector(b.copy(), o()), sigma)
    assert W3.last_solve_stats["iterations"] == itn and W3.last_solve_stats["istop"] == istop
    np.testing.assert_allclose(W3.array, W.array, rtol=0, atol=1e-12 * np.linalg.norm(x))


def test_given_potentials_and_zero_right_hand_side(hip):
    H, p = _device_problem(hip, kp.GRID)
    sigma, b = p["sigma"], p["b"]
    fit = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(tol=1e-8, preconditioner="separable")), sigma)
    same = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(tol=1e-8, preconditioner="separable",
                                                                preconditionerPotentials=p["potentials"])), sigma)
    np.testing.assert_array_equal(same.array, fit.array)            # the fit, handed over: the same decomposition bits
    bare = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(tol=1e-8, preconditioner="separable",
                                                                preconditionerPotentials=[np.zeros(n) for n in kp.GRID])), sigma)
    assert bare.last_solve_stats["iterations"] > 4 * fit.last_solve_stats["iterations"]
    zero = hip.HipVector.solve(H, hip.HipVector(np.zeros(len(b)), _opts(tol=1e-8, preconditioner="separable")), sigma)
    assert zero.last_solve_stats["iterations"] == 0 and not zero.array.any()


def test_lanczos_with_the_option(hip, monkeypatch):
    """The Ritz values compared are those the plain run determines: the ones that have reached an eigenvalue of the explicit
    matrix to 1e-9.  The others are set by the error of the inner solves, whichever solver makes it - once the wanted
    vector has converged, the next Lanczos vector is what the solve error leaves after orthogonalisation - and the plain
    run does not reproduce its own: the oracle at linear_tol 1e-10 / 1e-11 / 1e-13 returns 6.00710 / 6.00718 / 6.00719,
    9.14399 / 9.14220 / 9.14214 and 13.13425 / 13.12843 / 13.12818 beside 7.70805843 in all three (this run with the
    option: 6.00719, 9.14214, 13.12815).  They are printed."""
    H, p = _device_problem(hip, kp.GRID)
    sigma = p["sigma"]
    g = guess_vector(H.nrows, 1)
    seen = []
    decompositions = set(getattr(H, "_separable", {})) | {None}        # what other tests left on the shared operator, and the fit
    real_solve = hip.HipVector.solve

    def counting(*a, **k):
        w = real_solve(*a, **k)
        seen.append(dict(w.last_solve_stats))
        return w

    monkeypatch.setattr(hip.HipVector, "solve", staticmethod(counting))
    runs = {}
    for name, lsa in (("plain", {}), ("separable", {"preconditioner": "separable"})):
        del seen[:]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ev, Y, st = hip.inexactLanczosDiagonalization(H, hip.HipVector(g.copy(), _opts(tol=1e-10, **lsa)), sigma, 8, 10, 1e-12,
                                                          writeOut=False)
        runs[name] = (np.sort(np.asarray(ev)), st, list(seen))
    (ev0, st0, s0), (ev1, st1, s1) = runs["plain"], runs["separable"]
    inner0, inner1 = sum(s["iterations"] for s in s0), sum(s["iterations"] for s in s1)
    print(f"lanczos: inner iterations {inner0} plain / {inner1} separable over {len(s0)} / {len(s1)} solves")
    print(f"lanczos: Ritz values {ev0} plain / {ev1} separable")
    assert st0["isConverged"] and st1["isConverged"] and len(ev0) == len(ev1)
    lam = p["lam"]
    settled = [i for i, t in enumerate(ev0) if np.min(np.abs(lam - t)) <= 1e-9 * abs(t)]
    near = lam[np.argmin(np.abs(lam - sigma))]
    assert settled and any(abs(ev0[i] - near) <= 1e-9 * abs(near) for i in settled)
    np.testing.assert_allclose(ev1[settled], ev0[settled], rtol=1e-9)
    assert inner1 < inner0
    assert s1 and all(s.get("preconditioner") == "separable" for s in s1) and not any("preconditioner" in s for s in s0)
    assert set(H._separable) == decompositions                          # one decomposition for the whole run


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_and_leakage(hip):
    H, p = _device_problem(hip, kp.GRID)
    sigma, b = p["sigma"], p["b"]
    plain = lambda: hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(tol=1e-8)), sigma)
    jacobi = lambda: hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(tol=1e-8, preconditioner="jacobi")), sigma)
    before = plain().array, jacobi().array
    sep = lambda **kw: hip.HipVector(b.copy(), _opts(preconditioner="separable", **kw))
    Hc = hip.HipCsrOperator.from_scipy(p["Hs"])
    with pytest.raises(NotImplementedError, match="HipKronSumOperator"):
        hip.HipVector.solve(Hc, sep(), sigma)
    with pytest.raises(ValueError, match="real shift"):
        hip.HipVector.solve(H, sep(), sigma + 0.4j)
    with pytest.raises(ValueError, match="minres"):
        hip.HipVector.solve(H, sep(solver="gcrotmk"), sigma)
    with pytest.raises(ValueError, match="shift invariance"):
        hip.HipVector.solve(H, sep(solver="minres_shifted"), sigma)
    with pytest.raises(NotImplementedError, match="x0"):
        hip.HipVector.solve(H, sep(), sigma, x0=hip.HipVector(b.copy()))
    for bad in ([np.zeros(13), np.zeros(10)], [np.zeros(13), np.zeros(10), np.zeros(8)], np.zeros((13, 10, 7)), "fit"):
        with pytest.raises(ValueError, match="preconditionerPotentials"):
            hip.HipVector.solve(H, sep(preconditionerPotentials=bad), sigma)
    with pytest.raises(ValueError, match="together"):
        H.separable_preconditioner(sigma, bases=p["bases"])
    # solveBlock: one by one, with the single solve's bits
    one = hip.HipVector.solve(H, sep(tol=1e-8), sigma)
    sols = hip.HipVector.solveBlock(H, [sep(tol=1e-8) for _ in range(3)], sigma)
    for w in sols:
        np.testing.assert_array_equal(w.array, one.array)
        assert w.last_solve_stats["preconditioner"] == "separable"
    # a plain and a Jacobi solve after the separable ones: the bits they gave before
    np.testing.assert_array_equal(plain().array, before[0])
    np.testing.assert_array_equal(jacobi().array, before[1])
