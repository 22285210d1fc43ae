"""The kept Lanczos basis on the device (``csrc/lanczos_filter.hip``: ``hipeig_lanczos_block_scalars`` with ``basis_mode`` 1
and ``hipeig_lanczos_combine`` on its basis, behind ``lanczos_run(keepBasis=True)``, ``lanczos_filter(basis="keep")`` and
the ``HipVector`` option ``"lanczosBasis"``) against the two-pass path it replaces.

Every case fails without the feature: the names do not exist.

With the row-owner sweep (block variant 1) the kept path runs pass 1's kernels on pass 1's operands and the combination
puts every element through the product pass's operations in its order, so scalars and vectors are compared with
``array_equal``.  With the window-blocked sweep (variant 2, LDS atomics, add order not fixed) the checks are those of
``test_gpu_lanczos_filter.py`` (helpers and bounds: ``_lanczos_cases.py``): stop steps within ``STEP_DIFFERENCE_BOUND`` of the shifted-MINRES twin
(max(3, 2 * largest difference observed), EXPERIMENTS.md R9), the filtered vectors within the bound derived there from
the residual targets - ``||q - q_exact|| <= sum_j |c_j| (1.01 target + 100 eps (|z_j| + ||H||_inf) ||x_j||) /
dist(z_j, spectrum)`` against the ``eigh`` filter - and single solutions within its true-residual bound."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from _lanczos_cases import (EPS, FAR, HI, LO, NEAR, W8, Z8, arrays, block_variant, build_problems, check_filter, check_steps,
                            device_columns, lf, options, residual_bound, reusable_bytes, same_scalars,
                            single_solution_tables, slot_bytes, spectrum, twin)

pytestmark = pytest.mark.gpu

NCOLS = 16


@pytest.fixture(scope="module")
def problems(hip):
    """name -> (host CSR, device operator, host right-hand sides [NCOLS, n]), built once."""
    return build_problems(hip, ("tri100", "gapped4000", "odd1037"), NCOLS)


# ---- 1. pass 1 is unchanged ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,sign,tol", [("odd1037", 1, 1.0, HI), ("odd1037", 3, -1.0, LO), ("odd1037", 5, 1.0, LO),
                                             ("odd1037", 8, -1.0, HI), ("odd1037", 9, 1.0, LO),
                                             ("gapped4000", 1, -1.0, LO), ("gapped4000", 3, 1.0, LO),
                                             ("gapped4000", 5, -1.0, LO), ("gapped4000", 8, 1.0, LO),
                                             ("gapped4000", 9, -1.0, LO)])
def test_pass1_scalars_are_those_of_the_plain_run(hip, problems, name, K, sign, tol):
    Hh, Hd, B = problems[name]
    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:K], *tol)
        plain = hip.lanczos_run(Hd, cols, Z8, reverseGF=sign < 0)
        kept = hip.lanczos_run(Hd, cols, Z8, reverseGF=sign < 0, keepBasis=True)
    groups = (K + 7) // 8
    assert plain.basis_kept == [False] * groups and plain.basis_bytes == 0
    assert kept.basis_kept == [True] * groups and kept.converged
    assert same_scalars(plain.scalars, kept.scalars)
    assert plain.info == kept.info and plain.groups == kept.groups and plain.products_pass1 == kept.products_pass1
    # memory follows the steps taken: whole segments of 32 slots up to the group's last vector
    n = Hh.shape[0]
    expect = sum(-(-p // 32) * 32 * slot_bytes(n, hi - lo) for p, (lo, hi) in zip(kept.products_pass1, kept.groups))
    assert kept.basis_bytes == expect
    kept.release()
    assert kept.basis_kept == [False] * groups and kept.basis_bytes == 0


@pytest.mark.parametrize("name,K,sign", [("odd1037", 5, 1.0), ("odd1037", 3, -1.0), ("tri100", 8, 1.0)])
def test_pass1_steps_with_the_window_blocked_sweep(hip, problems, name, K, sign):
    Hh, Hd, B = problems[name]
    rtol, atol = LO
    with block_variant(Hd, 2):
        run = hip.lanczos_run(Hd, device_columns(hip, B[:K], rtol, atol), Z8, reverseGF=sign < 0, keepBasis=True)
    assert run.basis_kept == [True] and run.converged
    for r in range(K):
        its, est, conv, xnorms = twin((name, r), Hh, B[r], Z8, rtol, atol, sign)
        assert conv.all()
        check_steps(f"{name} K={K} variant=2 sign={sign:+.0f} kept column={r}", run.scalars[r].iterations, its)


# ---- 2. the combination equals the product pass ----------------------------------------------------------------------
@pytest.mark.parametrize("name,K,sign,tol", [("odd1037", 2, 1.0, HI), ("odd1037", 5, -1.0, LO), ("gapped4000", 8, 1.0, LO),
                                             ("tri100", 5, -1.0, HI)])
def test_combination_equals_the_product_pass(hip, problems, name, K, sign, tol):
    Hh, Hd, B = problems[name]
    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:K], *tol)
        plain = hip.lanczos_run(Hd, cols, Z8, reverseGF=sign < 0)
        kept = hip.lanczos_run(Hd, cols, Z8, reverseGF=sign < 0, keepBasis=True)
        assert kept.basis_kept == [True] and same_scalars(plain.scalars, kept.scalars)
        tables = [lf.filter_coefficients(plain.scalars, Z8, W8, sign), single_solution_tables(plain, NEAR, sign),
                  single_solution_tables(plain, FAR, sign)]
        for G in tables:
            a, b = plain.combine(G), kept.combine(G)
            assert plain.products_pass2 == [max(len(g) for g in G) - 1] and kept.products_pass2 == [0]
            if G[0].shape[1] == 2:
                assert all(isinstance(x, hip.HipComplexVector) for x in b)
            else:
                assert all(isinstance(x, hip.HipVector) and not isinstance(x, hip.HipComplexVector) for x in b)
            for r, (x, y) in enumerate(zip(arrays(a), arrays(b))):
                assert x.any() and np.array_equal(x, y), (name, K, r, G[0].shape)


@pytest.mark.parametrize("name,K,sign", [("odd1037", 5, 1.0), ("tri100", 2, -1.0)])
def test_filtered_vectors_with_the_window_blocked_sweep(hip, problems, name, K, sign):
    Hh, Hd, B = problems[name]
    rtol, atol = LO
    with block_variant(Hd, 2):
        cols = device_columns(hip, B[:K], rtol, atol)
        qs = hip.lanczos_filter(Hd, cols, Z8, W8, reverseGF=sign < 0, basis="keep")
    for r in range(K):
        st = cols[r].last_solve_stats
        assert st["basis"] == "kept" and st["products_pass2"] == 0 and st["products"] == st["products_pass1"]
        its, est, conv, xnorms = twin((name, r), Hh, B[r], Z8, rtol, atol, sign)
        check_filter(f"{name} K={K} variant=2 kept column={r}", name, Hh, B[r], qs[r].array, Z8, W8, xnorms,
                     max(atol, rtol), sign)


@pytest.mark.parametrize("name,sign,tol", [("gapped4000", 1.0, LO), ("odd1037", -1.0, HI)])
def test_single_solutions_with_the_window_blocked_sweep(hip, problems, name, sign, tol):
    Hh, Hd, B = problems[name]
    rtol, atol = tol
    K = 2
    with block_variant(Hd, 2):
        run = hip.lanczos_run(Hd, device_columns(hip, B[:K], rtol, atol), Z8, reverseGF=sign < 0, keepBasis=True)
        assert run.basis_kept == [True] and run.converged
        for j in (NEAR, FAR):
            xs = run.combine(single_solution_tables(run, j, sign))
            assert run.products_pass2 == [0]
            for r, x in enumerate(xs):
                xa = x.array
                res = np.linalg.norm(B[r] - sign * (Z8[j] * xa - Hh @ xa))
                target = max(atol, rtol)
                print(f"RESIDUAL {name} kept sign={sign:+.0f} shift={j} column={r} true {res:.3e} target {target:.1e}")
                assert np.isfinite(xa).all() and res <= residual_bound(Hh, Z8[j], xa, target), (name, j, r, res)


# ---- 3. many combinations, wide tables -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", [("odd1037", 5), ("gapped4000", 3)])
def test_many_combinations_and_wide_tables_from_one_run(hip, problems, name, K):
    Hh, Hd, B = problems[name]
    rng = np.random.default_rng(21)
    with block_variant(Hd, 1):
        run = hip.lanczos_run(Hd, device_columns(hip, B[:K], *LO), Z8, keepBasis=True)
        assert run.basis_kept == [True]
        p1 = list(run.products_pass1)
        wide = [rng.standard_normal((len(sc.alphas), 8)) for sc in run.scalars]
        out8 = run.combine(wide)
        assert run.products_pass2 == [0]
        out4 = run.combine([g[:, 2:6] for g in wide])
        assert run.products_pass2 == [0]
        out3 = run.combine([g[:, 5:8] for g in wide])
        assert run.products_pass2 == [0] and run.products_pass1 == p1
        assert all(len(o) == 8 for o in out8) and all(len(o) == 4 for o in out4) and all(len(o) == 3 for o in out3)
        for c in range(8):
            one = arrays(run.combine([g[:, c] for g in wide]))
            for r in range(K):
                assert one[r].any() and np.array_equal(out8[r][c].array, one[r]), (c, r)
                if 2 <= c < 6:
                    assert np.array_equal(out4[r][c - 2].array, one[r]), (c, r)
                if c >= 5:
                    assert np.array_equal(out3[r][c - 5].array, one[r]), (c, r)
        # the product pass does not take the wide table
        plain = hip.lanczos_run(Hd, device_columns(hip, B[:K], *LO), Z8)
        with pytest.raises(ValueError, match="NC = 1 or 2"):
            plain.combine(wide)


# ---- 4. masking ------------------------------------------------------------------------------------------------------
def test_masking_of_columns_that_stop_at_very_different_steps(hip, problems):
    """One block on n = 1037: a random column, a sum of 6 eigenvectors (its Krylov space is exhausted within 7 steps), a
    zero column (no step at all) and a second random column; then tables shorter than the steps run, an empty one, and
    one that is too long."""
    name = "odd1037"
    Hh, Hd, B = problems[name]
    lam, U = spectrum(name, Hh)
    few = U[:, [3, 200, 517, 518, 800, 1030]] @ np.array([1.0, -0.5, 0.7, 0.3, -1.2, 0.9])
    cols_h = np.array([B[0], few / np.linalg.norm(few), np.zeros(1037), B[1]])
    with block_variant(Hd, 1):
        cols = device_columns(hip, cols_h, *LO)
        plain = hip.lanczos_run(Hd, cols, Z8)
        kept = hip.lanczos_run(Hd, cols, Z8, keepBasis=True)
        assert kept.basis_kept == [True] and same_scalars(plain.scalars, kept.scalars)
        steps = [len(s.alphas) for s in kept.scalars]
        assert steps[2] == 0 and 1 <= steps[1] <= 8 and min(steps[0], steps[3]) >= 10 * steps[1]
        G = lf.filter_coefficients(kept.scalars, Z8, W8)
        full_p, full_k = arrays(plain.combine(G)), arrays(kept.combine(G))
        assert all(np.array_equal(x, y) for x, y in zip(full_p, full_k))
        assert not full_k[2].any() and full_k[1].any()
        # shorter than the steps run: 7 terms, 3 terms, none, all but one - and no term at all for the first column
        for cut in ([7, 3, 0, steps[3] - 1], [0, steps[1], 0, 1]):
            Gc = [g[:m] for g, m in zip(G, cut)]
            a, b = arrays(plain.combine(Gc)), arrays(kept.combine(Gc))
            assert kept.products_pass2 == [0] and plain.products_pass2 == [max(cut) - 1]
            for r in range(4):
                assert np.array_equal(a[r], b[r]) and bool(b[r].any()) == (cut[r] > 0), (cut, r)
        for r in (0, 1, 2):
            Gl = [g.copy() for g in G]
            Gl[r] = np.ones((steps[r] + 1, 1))
            with pytest.raises(ValueError, match=f"column {r}"):
                kept.combine(Gl)
    # against the exact filter, as the two-pass case
    for r in (0, 1, 3):
        its, est, conv, xnorms = twin((name, "masking", r), Hh, cols_h[r], Z8, *LO, 1.0)
        check_filter(f"{name} masking kept column={r}", name, Hh, cols_h[r], full_k[r], Z8, W8, xnorms, max(LO), 1.0)


def test_breakdown_ends_in_one_step_with_the_exact_answer(hip):
    h = np.linspace(-1.0, 1.0, 64)
    Hd = hip.HipCsrOperator.from_scipy(sp.diags(h).tocsr())
    b = np.zeros(64)
    b[3] = 2.0
    zs, ws = Z8 + [0.5], W8 + [0.3 - 0.1j]
    for sign in (1.0, -1.0):
        cols = device_columns(hip, [b], 1e-10, 1e-12, 100)
        q = hip.lanczos_filter(Hd, cols, zs, ws, reverseGF=sign < 0, basis="keep")[0].array
        st = cols[0].last_solve_stats
        assert st["iterations"] == [1] * 9 and st["estimates"] == [0.0] * 9
        assert st["products"] == 1 and st["products_pass2"] == 0 and st["basis"] == "kept"
        exact = sum((w * sign * 2.0 / (z - h[3])).real for z, w in zip(zs, ws))
        assert np.count_nonzero(q) == 1 and abs(q[3] - exact) <= 8 * EPS * sum(abs(w * 2.0 / (z - h[3])) for z, w in zip(zs, ws))


def test_all_zero_columns_keep_nothing_and_give_zeros(hip, problems):
    Hh, Hd, B = problems["gapped4000"]
    cols = device_columns(hip, np.zeros((2, 4000)), *LO)
    run = hip.lanczos_run(Hd, cols, Z8, keepBasis=True)
    assert run.basis_kept == [False] and run.products_pass1 == [0]
    assert all(not q.array.any() for q in run.combine([np.zeros((0, 1))] * 2))


# ---- 5. segment and chunk boundaries ---------------------------------------------------------------------------------
def test_segment_and_chunk_boundaries(hip, problems, monkeypatch):
    """A run of about 500 steps with 5 slots per segment (a hundred boundaries) and with the default 32, the state record
    looked at after every step and after every 32: the same scalars and the same combined vectors, bit for bit."""
    name, K = "gapped4000", 3
    Hh, Hd, B = problems[name]
    out = []
    with block_variant(Hd, 1):
        for seg, chunk in ((None, None), ("5", None), (None, "1"), ("5", "1")):
            monkeypatch.delenv("HIPEIG_LF_SEGMENT", raising=False)
            monkeypatch.delenv("HIPEIG_LF_CHUNK", raising=False)
            if seg:
                monkeypatch.setenv("HIPEIG_LF_SEGMENT", seg)
            if chunk:
                monkeypatch.setenv("HIPEIG_LF_CHUNK", chunk)
            run = hip.lanczos_run(Hd, device_columns(hip, B[:K], *LO), Z8, keepBasis=True)
            assert run.basis_kept == [True]
            p = run.products_pass1[0]
            assert run.basis_bytes == -(-p // int(seg or 32)) * int(seg or 32) * slot_bytes(4000, K)
            G = lf.filter_coefficients(run.scalars, Z8, W8)
            G2 = single_solution_tables(run, NEAR, 1.0)
            out.append((run.scalars, arrays(run.combine(G)), arrays(run.combine(G2))))
            run.release()
    assert 200 <= len(out[0][0][0].alphas) <= 1000
    for scalars, q, x in out[1:]:
        assert same_scalars(out[0][0], scalars)
        assert all(np.array_equal(a, b) for a, b in zip(out[0][1], q))
        assert all(np.array_equal(a, b) for a, b in zip(out[0][2], x))


# ---- 6. budget -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg,chunk", [(None, None), ("5", "1"), ("5", "4"), ("5", "7")])
def test_a_budget_of_ten_slots_falls_back_to_the_ring(hip, problems, monkeypatch, seg, chunk):
    """Room for about 10 slots on a run of about 100 steps.  With the default 32 slots per segment not even the first
    segment fits; with 5 per segment two fit and the run moves its two live vectors to the ring at step 9, 8 or 7 (chunk
    1, 4, 7: every position in the ring of three)."""
    name, K = "odd1037", 5
    Hh, Hd, B = problems[name]
    budget = 10 * slot_bytes(1037, K) + 100
    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:K], *LO)
        plain = hip.lanczos_run(Hd, cols, Z8)
        Gp = lf.filter_coefficients(plain.scalars, Z8, W8)
        qp = arrays(plain.combine(Gp))
        if seg:
            monkeypatch.setenv("HIPEIG_LF_SEGMENT", seg)
            monkeypatch.setenv("HIPEIG_LF_CHUNK", chunk)
        run = hip.lanczos_run(Hd, cols, Z8, keepBasis=True, basisBytes=budget)
        assert min(len(s.alphas) for s in run.scalars) > 50
        assert run.basis_kept == [False] and run.basis_bytes == 0
        assert same_scalars(plain.scalars, run.scalars) and run.products_pass1 == plain.products_pass1
        q = arrays(run.combine(Gp))
        assert run.products_pass2 == plain.products_pass2 == [max(len(g) for g in Gp) - 1]
        assert all(np.array_equal(a, b) for a, b in zip(qp, q))
        with pytest.raises(ValueError, match="NC = 1 or 2"):
            run.combine([np.ones((len(g), 4)) for g in Gp])
        qf = arrays(hip.lanczos_filter(Hd, cols, Z8, W8, basis="keep", basisBytes=budget))
        assert all(c.last_solve_stats["basis"] == "recomputed" for c in cols)
        assert all(c.last_solve_stats["products_pass2"] == c.last_solve_stats["products_pass1"] - 1 for c in cols)
        assert all(np.array_equal(a, b) for a, b in zip(qp, qf))


def test_a_budget_for_one_group_of_two(hip, problems):
    """16 columns = two groups of 8.  The budget holds either group's basis (its segments, and the one more a run
    allocates ahead of the chunk in which it stops) but not both: ``lanczos_filter`` works group by group and keeps both,
    one after the other; a ``lanczos_run`` holds the first while the second runs, so the second is not kept."""
    name = "odd1037"
    Hh, Hd, B = problems[name]
    seg_bytes = 32 * slot_bytes(1037, 8)
    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:16], *LO)
        peaks = []
        for lo in (0, 8):
            one = hip.lanczos_run(Hd, cols[lo:lo + 8], Z8, keepBasis=True)
            assert one.basis_kept == [True] and one.basis_bytes % seg_bytes == 0
            peaks.append(one.basis_bytes + seg_bytes)
            one.release()
        budget = max(peaks)
        plain = hip.lanczos_run(Hd, cols, Z8)
        G = lf.filter_coefficients(plain.scalars, Z8, W8)
        qp = arrays(plain.combine(G))
        qf = arrays(hip.lanczos_filter(Hd, cols, Z8, W8, basis="keep", basisBytes=budget))
        assert [c.last_solve_stats["basis"] for c in cols] == ["kept"] * 16
        assert [c.last_solve_stats["group"] for c in cols] == [0] * 8 + [1] * 8
        assert all(c.last_solve_stats["products_pass2"] == 0 for c in cols)
        assert all(np.array_equal(a, b) for a, b in zip(qp, qf))
        run = hip.lanczos_run(Hd, cols, Z8, keepBasis=True, basisBytes=budget)
        assert run.basis_kept == [True, False] and 0 < run.basis_bytes <= budget
        assert same_scalars(plain.scalars, run.scalars)
        q = arrays(run.combine(G))
        assert run.products_pass2 == [0, plain.products_pass2[1]]
        assert all(np.array_equal(a, b) for a, b in zip(qp, q))
        run.release()
        assert run.basis_bytes == 0 and run.basis_kept == [False, False]
        q = arrays(run.combine(G))
        assert run.products_pass2 == plain.products_pass2
        assert all(np.array_equal(a, b) for a, b in zip(qp, q))


def test_released_segments_are_handed_out_again(hip, problems):
    name, K = "odd1037", 3
    Hh, Hd, B = problems[name]
    cols = device_columns(hip, B[:K], *LO)
    ctx = cols[0].ctx
    run = hip.lanczos_run(Hd, cols, Z8, keepBasis=True)
    held, before = run.basis_bytes, reusable_bytes(ctx)
    run.release()
    assert held > 0 and reusable_bytes(ctx) == before + held
    again = hip.lanczos_run(Hd, cols, Z8, keepBasis=True)
    assert again.basis_bytes == held and reusable_bytes(ctx) <= before
    again.release()


# ---- 7. FEAST end to end ---------------------------------------------------------------------------------------------
def test_feast_end_to_end_with_the_kept_basis(hip):
    """Config #5 at N = 2e4 (``test_feast_end_to_end_with_the_lanczos_filter``) with the row-owner sweep: ``"lanczosBasis":
    "keep"`` gives the eigenvalues, the iteration count and the residual of ``"recompute"`` bit for bit."""
    import scipy.linalg as la
    N, m0, eConv = 20_000, 16, 1e-4
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    Q = la.qr(np.random.default_rng(9).standard_normal((N, m0)), mode="economic")[0]
    out = {}
    H.set_block_variant(1)
    try:
        for mode in ("recompute", "keep"):
            o = {"linearSystemArgs": {"linearSolver": "lanczos_filter", "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7},
                 "lanczosBasis": mode}
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out[mode] = hip.feastDiagonalization(H, [hip.HipVector(Q[:, i].copy(), o) for i in range(m0)], 16, "legendre",
                                                     -0.21, 0.21, eConv, 12, writeOut=False)
    finally:
        H.set_block_variant(0)
    (ev, Y, st), (ev_r, _, st_r) = out["keep"], out["recompute"]
    assert st["residual"] < eConv
    assert np.array_equal(ev, ev_r) and st["outerIter"] == st_r["outerIter"] and st["residual"] == st_r["residual"]
    assert len(st["lanczosFilter"]) == len(st_r["lanczosFilter"]) == st["outerIter"] + 1
    for rec, rec_r in zip(st["lanczosFilter"], st_r["lanczosFilter"]):
        assert rec["runs"] == 2 and rec["basis"] == ["kept"] * 2 and rec["products_pass2"] == [0] * 2
        assert rec_r["basis"] == ["recomputed"] * 2 and rec_r["products_pass2"] == [p - 1 for p in rec_r["products_pass1"]]
        assert rec["products_pass1"] == rec_r["products_pass1"] and rec["steps"] == rec_r["steps"]


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def test_refusals(hip, problems):
    Hh, Hd, B = problems["odd1037"]
    cols = device_columns(hip, B[:2], *LO)
    with pytest.raises(ValueError, match="basis"):
        hip.lanczos_filter(Hd, cols, Z8, W8, basis="kept")
    with pytest.raises(ValueError, match="basis"):
        hip.lanczos_filter(Hd, cols, Z8, W8, basis=None)
    with pytest.raises(ValueError, match="basisBytes"):
        hip.lanczos_run(Hd, cols, Z8, keepBasis=True, basisBytes=-1)
    bad = dict(options(*LO), lanczosBasis="always")
    with pytest.raises(ValueError, match="basis"):
        hip.feastDiagonalization(Hd, [hip.HipVector(b.copy(), bad) for b in B[:2]], 16, "legendre", -0.21, 0.21, 1e-4, 1,
                                 writeOut=False)
    keep = dict(options(*LO), lanczosBasis="keep", lanczosBasisBytes=123)
    v = hip.HipVector(B[0].copy(), keep)
    assert v.options["lanczosBasis"] == "keep" and v.options["lanczosBasisBytes"] == 123
    assert "lanczosBasis" not in cols[0].options
    with pytest.raises(NotImplementedError):
        hip.lanczos_filter(Hd, [hip.HipComplexVector(B[0] + 1j * B[1], options(*LO))], Z8, W8, basis="keep")
    with pytest.raises(NotImplementedError):
        hip.lanczos_run(Hd, cols + [hip.HipComplexVector(B[0] + 1j * B[1], options(*LO))], Z8, keepBasis=True)
    ctx = cols[0].ctx
    saved = ctx._force_collectives
    ctx._force_collectives = True            # what attach_comm records under HIPEIG_FORCE_COLLECTIVES=1
    try:
        assert ctx.collectives
        with pytest.raises(NotImplementedError, match="collectives"):
            hip.lanczos_filter(Hd, cols, Z8, W8, basis="keep")
        with pytest.raises(NotImplementedError, match="collectives"):
            hip.lanczos_run(Hd, cols, Z8, keepBasis=True)
    finally:
        ctx._force_collectives = saved
