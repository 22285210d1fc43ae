"""The two-pass Lanczos filter on the device (``csrc/lanczos_filter.hip`` behind ``eigensolvers_amd.lanczos_run``,
``eigensolvers_amd.lanczos_filter`` and FEAST's ``linearSolver="lanczos_filter"`` path) against the NumPy twins, the exact
filter from ``eigh`` and true residuals formed on the host.

Every case fails without the feature: the names do not exist.

The step bound against the twin (``STEPS ...`` lines under ``-s``) and the derived bound of the filtered vectors
(``FILTER ...``: the fraction of the bound a case uses) are stated in ``_lanczos_cases.py``, which holds the helpers."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from eigensolvers_amd.generators import gapped_params

from _lanczos_cases import (EPS, HI, LO, W8, Z8, build_problems, check_filter, check_steps, contour, device_columns, lf,
                            options, residual_bound, spectrum, twin)

pytestmark = pytest.mark.gpu

REAL_SHIFT = 0.5
NCOLS = 9
Z16, W16 = contour(32)
SETS = {"c8": (Z8, W8), "c8r": (Z8 + [REAL_SHIFT], W8 + [0.3 - 0.1j]), "c16": (Z16, W16)}


@pytest.fixture(scope="module")
def problems(hip):
    """name -> (host CSR, device operator, host right-hand sides [NCOLS, n]), built once."""
    return build_problems(hip, ("n100", "tri100", "gapped4000", "odd1037"), NCOLS)


# (problem, columns, block variant, sign, tolerances, shift set): every K of {1, 2, 3, 4, 5, 8, 9} with both block
# variants, both signs, both tolerance pairs, the three shift sets (16 points = more than 8 shifts in one run), the
# one-workgroup operator, and n = 1037 with K = 3 and K = 5, which pad the 4- and the 8-wide block.
CASES = [("gapped4000", 1, 1, 1.0, LO, "c8"), ("gapped4000", 1, 2, -1.0, HI, "c8r"),
         ("gapped4000", 2, 2, 1.0, LO, "c8r"), ("gapped4000", 2, 1, 1.0, HI, "c8"),
         ("gapped4000", 3, 1, -1.0, LO, "c8"), ("gapped4000", 3, 2, 1.0, HI, "c8"),
         ("gapped4000", 4, 2, 1.0, LO, "c16"), ("gapped4000", 4, 1, -1.0, HI, "c8r"),
         ("gapped4000", 5, 1, 1.0, LO, "c16"), ("gapped4000", 5, 2, 1.0, HI, "c8"),
         ("gapped4000", 8, 2, -1.0, LO, "c8"), ("gapped4000", 8, 1, 1.0, LO, "c8r"),
         ("gapped4000", 9, 1, 1.0, LO, "c8"), ("gapped4000", 9, 2, 1.0, LO, "c8"),
         ("odd1037", 3, 1, 1.0, HI, "c8r"), ("odd1037", 3, 2, -1.0, LO, "c8"),
         ("odd1037", 5, 2, 1.0, HI, "c8"), ("odd1037", 5, 1, -1.0, LO, "c16"),
         ("tri100", 1, 1, 1.0, HI, "c8r"), ("tri100", 8, 2, -1.0, HI, "c8r"), ("tri100", 9, 1, 1.0, LO, "c16")]


@pytest.mark.parametrize("name,K,variant,sign,tol,sset", CASES)
def test_step_counts_and_filter_error(hip, problems, name, K, variant, sign, tol, sset):
    Hh, Hd, B = problems[name]
    (rtol, atol), (zs, ws) = tol, SETS[sset]
    Hd.set_block_variant(variant)
    try:
        cols = device_columns(hip, B[:K], rtol, atol)
        qs = hip.lanczos_filter(Hd, cols, zs, ws, reverseGF=sign < 0)
    finally:
        Hd.set_block_variant(0)
    assert len(qs) == K and all(isinstance(q, hip.HipVector) and not isinstance(q, hip.HipComplexVector) for q in qs)
    target = max(atol, rtol)                                    # the columns have unit norm
    for r in range(K):
        st = cols[r].last_solve_stats
        its, est, conv, xnorms = twin((name, r), Hh, B[r], zs, rtol, atol, sign)
        assert conv.all() and len(st["iterations"]) == len(st["estimates"]) == len(zs)
        assert all(e <= target * (1 + 1e-12) for e in st["estimates"])
        label = f"{name} K={K} variant={variant} sign={sign:+.0f} rtol={rtol:g} {sset} column={r}"
        check_steps(label, st["iterations"], its)
        check_filter(label, name, Hh, B[r], qs[r].array, zs, ws, xnorms, target, sign)
    # block products: per group of 8 columns pass 1 takes the slowest column's steps, pass 2 one fewer
    for lo in range(0, K, 8):
        top = max(max(c.last_solve_stats["iterations"]) for c in cols[lo:lo + 8])
        for c in cols[lo:lo + 8]:
            st = c.last_solve_stats
            assert (st["products_pass1"], st["products_pass2"], st["products"]) == (top, top - 1, 2 * top - 1)


@pytest.mark.parametrize("name", ["n100", "gapped4000", "odd1037"])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_single_solutions_through_two_combinations(hip, problems, name, sign):
    """NC = 2 with (Re y, Im y) of one shift - the contour point nearest the real axis and the farthest - rebuilds that
    shift's iterate; its true residual answers to ``test_gpu_shifted_minres.py``'s bound."""
    Hh, Hd, B = problems[name]
    rtol, atol = LO if sign > 0 else HI
    K = 2
    run = hip.lanczos_run(Hd, device_columns(hip, B[:K], rtol, atol), Z8, reverseGF=sign < 0)
    assert run.converged and run.info == [0] * K
    for j in (int(np.argmin([abs(z.imag) for z in Z8])), int(np.argmax([abs(z.imag) for z in Z8]))):
        G = []
        for sc in run.scalars:
            y = lf.minres_coefficients(sc.alphas, sc.betas, Z8[j], sc.iterations[j], sign)
            G.append(np.stack([y.real, y.imag], axis=1))
        xs = run.combine(G)
        assert all(isinstance(x, hip.HipComplexVector) for x in xs)
        assert run.products_pass2 == [max(len(g) for g in G) - 1]
        for r, x in enumerate(xs):
            xa = x.array
            res = np.linalg.norm(B[r] - sign * (Z8[j] * xa - Hh @ xa))
            target = max(atol, rtol)
            print(f"RESIDUAL {name} sign={sign:+.0f} shift={j} column={r} true {res:.3e} target {target:.1e}")
            assert np.isfinite(xa).all() and res <= residual_bound(Hh, Z8[j], xa, target), (name, j, r, res)


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("variant", [1, 2])
def test_columns_do_not_see_each_other(hip, problems, monkeypatch, K, variant):
    """Column r of a K-column run against the one-column run at the same interleave width (the order in which a row's
    terms are added depends on the width; HIPEIG_LF_WIDTH=8 gives the one-column run the wide one): the row-owner sweep
    adds in a fixed order, so scalars, stop steps and the filtered vector are equal bit for bit; with the window-blocked
    sweep (LDS atomics) the stop steps are within the step bound."""
    Hh, Hd, B = problems["gapped4000"]
    rtol, atol = LO
    monkeypatch.delenv("HIPEIG_LF_WIDTH", raising=False)
    Hd.set_block_variant(variant)
    try:
        cols = device_columns(hip, B[:K], rtol, atol)
        run = hip.lanczos_run(Hd, cols, Z8)
        G = lf.filter_coefficients(run.scalars, Z8, W8)
        qs = [q.array for q in run.combine(G)]
        if K > 4:
            monkeypatch.setenv("HIPEIG_LF_WIDTH", "8")
        for r in sorted({0, K // 2, K - 1}):
            one = hip.lanczos_run(Hd, [cols[r]], Z8)
            a, b = run.scalars[r], one.scalars[0]
            if variant == 1:
                assert np.array_equal(a.iterations, b.iterations) and np.array_equal(a.estimates, b.estimates)
                assert np.array_equal(a.alphas, b.alphas) and np.array_equal(a.betas, b.betas)
                q1 = one.combine(lf.filter_coefficients(one.scalars, Z8, W8))[0].array
                assert np.array_equal(q1, qs[r])
            else:
                check_steps(f"gapped4000 K={K} variant=2 column={r} against the one-column run", a.iterations, b.iterations)
    finally:
        Hd.set_block_variant(0)


def test_masking_of_columns_that_stop_at_very_different_steps(hip, problems):
    """One block on n = 1037: a random column, a sum of 6 eigenvectors (its Krylov space is exhausted within 7 steps), a
    zero column (no step at all) and a second random column."""
    name = "odd1037"
    Hh, Hd, B = problems[name]
    lam, U = spectrum(name, Hh)
    few = U[:, [3, 200, 517, 518, 800, 1030]] @ np.array([1.0, -0.5, 0.7, 0.3, -1.2, 0.9])
    cols_h = np.array([B[0], few / np.linalg.norm(few), np.zeros(1037), B[1]])
    rtol, atol = LO
    twins = [twin((name, "masking", r), Hh, b, Z8, rtol, atol, 1.0) for r, b in enumerate(cols_h)]
    assert max(twins[1][0]) <= 7 and not twins[2][0].any()
    assert min(twins[0][0]) >= 10 * max(twins[1][0]) and min(twins[3][0]) >= 10 * max(twins[1][0])
    cols = device_columns(hip, cols_h, rtol, atol)
    qs = hip.lanczos_filter(Hd, cols, Z8, W8)
    for r in (0, 1, 3):
        its, est, conv, xnorms = twins[r]
        assert conv.all()
        check_steps(f"{name} masking column={r}", cols[r].last_solve_stats["iterations"], its)
        check_filter(f"{name} masking column={r}", name, Hh, cols_h[r], qs[r].array, Z8, W8, xnorms, max(atol, rtol), 1.0)
    assert cols[2].last_solve_stats["iterations"] == [0] * 8 and not qs[2].array.any()
    top = max(max(c.last_solve_stats["iterations"]) for c in cols)
    assert cols[1].last_solve_stats["products_pass1"] == top


def test_all_zero_columns_take_no_product(hip, problems):
    Hh, Hd, B = problems["gapped4000"]
    cols = device_columns(hip, np.zeros((2, 4000)), *LO)
    qs = hip.lanczos_filter(Hd, cols, Z8, W8)
    assert all(not q.array.any() for q in qs)
    assert all(c.last_solve_stats["products"] == 0 and c.last_solve_stats["iterations"] == [0] * 8 for c in cols)


@pytest.mark.parametrize("K", [3, 5])
def test_chunk_independence(hip, problems, monkeypatch, K):
    """The host looks at the state record every HIPEIG_LF_CHUNK steps (default 32); kernels enqueued past the stop return
    at once, so chunk 1 and chunk 32 give the same scalars and the same filtered vectors - row-owner sweep: bit for bit."""
    Hh, Hd, B = problems["odd1037"]
    Hd.set_block_variant(1)
    try:
        out = []
        for chunk in (None, "1"):
            monkeypatch.delenv("HIPEIG_LF_CHUNK", raising=False)
            if chunk:
                monkeypatch.setenv("HIPEIG_LF_CHUNK", chunk)
            cols = device_columns(hip, B[:K], *LO)
            run = hip.lanczos_run(Hd, cols, Z8)
            qs = run.combine(lf.filter_coefficients(run.scalars, Z8, W8))
            out.append((run, [q.array for q in qs]))
        (r0, q0), (r1, q1) = out
        assert r0.products_pass1 == r1.products_pass1 and len(set(map(tuple, (s.iterations for s in r0.scalars)))) > 1
        for a, b in zip(r0.scalars, r1.scalars):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert all(np.array_equal(x, y) for x, y in zip(q0, q1))
    finally:
        Hd.set_block_variant(0)


def test_step_limit_raises_and_reports_per_column(hip, problems):
    Hh, Hd, B = problems["gapped4000"]
    cols_h = np.array([B[0], np.zeros(4000), B[1]])
    cols = device_columns(hip, cols_h, 1e-12, 0.0, 5)
    run = hip.lanczos_run(Hd, cols, Z8 + [REAL_SHIFT])
    assert run.info == [5, 0, 5] and not run.converged and run.products_pass1 == [5]
    assert [list(s.iterations) for s in run.scalars] == [[5] * 9, [0] * 9, [5] * 9]
    assert [len(s.alphas) for s in run.scalars] == [5, 0, 5]
    with pytest.raises(UserWarning, match="Iterative solver is not converged"):
        hip.lanczos_filter(Hd, cols, Z8 + [REAL_SHIFT], W8 + [1.0])
    assert cols[0].last_solve_stats["iterations"] == [5] * 9 and cols[0].last_solve_stats["products_pass1"] == 5


def test_breakdown_ends_in_one_step_with_the_exact_answer(hip):
    h = np.linspace(-1.0, 1.0, 64)
    Hd = hip.HipCsrOperator.from_scipy(sp.diags(h).tocsr())
    b = np.zeros(64)
    b[3] = 2.0
    zs, ws = SETS["c8r"]
    for sign in (1.0, -1.0):
        cols = device_columns(hip, [b], 1e-10, 1e-12, 100)
        q = hip.lanczos_filter(Hd, cols, zs, ws, reverseGF=sign < 0)[0].array
        st = cols[0].last_solve_stats
        assert st["iterations"] == [1] * 9 and st["estimates"] == [0.0] * 9 and st["products"] == 1
        exact = sum((w * sign * 2.0 / (z - h[3])).real for z, w in zip(zs, ws))
        assert np.count_nonzero(q) == 1 and abs(q[3] - exact) <= 8 * EPS * sum(abs(w * 2.0 / (z - h[3])) for z, w in zip(zs, ws))


def test_refusals(hip, problems):
    Hh, Hd, B = problems["gapped4000"]
    cols = device_columns(hip, B[:2], *LO)
    with pytest.raises(NotImplementedError):
        hip.lanczos_filter(Hd, [hip.HipComplexVector(B[0] + 1j * B[1], options(*LO))], Z8, W8)
    with pytest.raises(NotImplementedError):
        hip.lanczos_run(Hd, cols + [hip.HipComplexVector(B[0] + 1j * B[1], options(*LO))], Z8)
    with pytest.raises(TypeError):
        hip.lanczos_filter(Hh, cols, Z8, W8)
    with pytest.raises(ValueError):
        hip.lanczos_run(Hd, cols, [0.1j * (k + 1) for k in range(33)])
    with pytest.raises(ValueError):
        hip.lanczos_filter(Hd, cols, Z8, W8[:3])
    with pytest.raises(NotImplementedError, match="filtered sums"):
        hip.HipVector.solve(Hd, cols[0], Z8[0])
    ctx = cols[0].ctx
    saved = ctx._force_collectives
    ctx._force_collectives = True            # what attach_comm records under HIPEIG_FORCE_COLLECTIVES=1
    try:
        assert ctx.collectives
        with pytest.raises(NotImplementedError, match="collectives"):
            hip.lanczos_filter(Hd, cols, Z8, W8)
        with pytest.raises(NotImplementedError, match="collectives"):
            hip.lanczos_run(Hd, cols, Z8)
    finally:
        ctx._force_collectives = saved
    with pytest.raises(ValueError, match="contourPool"):
        hip.feastDiagonalization(Hd, cols, 16, "legendre", -0.21, 0.21, 1e-4, 1, writeOut=False, contourPool=True)


def test_feast_end_to_end_with_the_lanczos_filter(hip):
    """The shared-Lanczos FEAST case of ``test_gpu_shifted_minres.py`` (config #5 at N = 2e4, rtol 1e-5) with both
    vector-major solvers: the same eigenvalues to that case's eConv, in the same number of FEAST iterations."""
    import scipy.linalg as la
    N, m0, eConv = 20_000, 16, 1e-4
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    Q = la.qr(np.random.default_rng(9).standard_normal((N, m0)), mode="economic")[0]
    out = {}
    for solver in ("minres_shifted", "lanczos_filter"):
        o = {"linearSystemArgs": {"linearSolver": solver, "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7}}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out[solver] = hip.feastDiagonalization(H, [hip.HipVector(Q[:, i].copy(), o) for i in range(m0)], 16, "legendre",
                                                   -0.21, 0.21, eConv, 12, writeOut=False)
    ev, Y, st = out["lanczos_filter"]
    ev_s, _, st_s = out["minres_shifted"]
    assert st["residual"] < eConv and st["outerIter"] == st_s["outerIter"]
    inside, inside_s = np.sort(ev[(ev > -0.21) & (ev < 0.21)]), np.sort(ev_s[(ev_s > -0.21) & (ev_s < 0.21)])
    assert len(inside) == len(inside_s) == 16
    assert np.sum(np.abs(inside - inside_s)) / np.sum(np.abs(inside_s)) < eConv
    targets = np.sort(gapped_params(N, 32, 7)["targets"])
    assert np.all(np.abs(inside - targets) < 2e-3)
    res = hip.true_residual_norms(H, ev, Y, m0)
    assert np.all(res < 1e-2), res
    rec = st["lanczosFilter"]
    assert len(rec) == st["outerIter"] + 1 and "sharedLanczos" not in st and "contourPool" not in st
    for r in rec:
        assert r["runs"] == 2 and len(r["products_pass1"]) == len(r["products_pass2"]) == 2      # 16 vectors = 2 groups of 8
        assert len(r["pairs"]) == len(r["steps"]) == 128
        assert sorted(map(tuple, r["pairs"])) == [(k, i) for k in range(8) for i in range(16)]
        for g in range(2):
            top = max(s for (k, i), s in zip(r["pairs"], r["steps"]) if i // 8 == g)
            assert r["products_pass1"][g] == top and r["products_pass2"][g] == top - 1
