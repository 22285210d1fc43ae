"""A Lanczos basis kept as a prefix on the device (``csrc/lanczos_filter.hip``: ``hipeig_lanczos_block_scalars`` with
``basis_mode`` 2 and ``hipeig_lanczos_combine`` on its basis, behind ``lanczos_run(keepBasis=True, keepPrefix=True)``,
``lanczos_filter(basis="keep", prefix=True)`` and the ``HipVector`` option ``"lanczosBasisPrefix"``) against the plain
two-pass path.

Every case fails without the feature: the names do not exist.

With the row-owner sweep (block variant 1) pass 1 runs the plain run's kernels on its operands whether a vector sits in
a slot or in the ring, and pass 2 puts every element through the product pass's operations in ascending order - the
stream for the terms ``i < p - 1``, the product loop from step ``p - 1`` - so scalars and vectors are compared with
``array_equal``.  With the window-blocked sweep (variant 2, LDS atomics, add order not fixed) the checks are those of
``test_gpu_lanczos_basis.py`` (helpers and bounds: ``_lanczos_cases.py``): stop steps within ``STEP_DIFFERENCE_BOUND`` of the shifted-MINRES twin and
the filtered vectors within ``||q - q_exact|| <= sum_j |c_j| (1.01 target + 100 eps (|z_j| + ||H||_inf) ||x_j||) /
dist(z_j, spectrum)`` against the ``eigh`` filter.  No tolerance is new."""
import warnings

import numpy as np
import pytest

from _lanczos_cases import (FAR, LO, NEAR, STEP_DIFFERENCE_BOUND, W8, Z8, all_equal, arrays, block_variant, build_problems,
                            device_columns, filter_bound, lf, options, reusable_bytes, same_scalars, single_solution_tables,
                            slot_bytes, spectrum, twin)

pytestmark = pytest.mark.gpu

NCOLS = 16


@pytest.fixture(scope="module")
def problems(hip):
    """name -> (host CSR, device operator, host right-hand sides [NCOLS, n]), built once."""
    return build_problems(hip, ("tri100", "gapped4000", "odd1037"), NCOLS)


def segments(monkeypatch, seg, chunk=None):
    monkeypatch.setenv("HIPEIG_LF_SEGMENT", str(seg))
    if chunk is None:
        monkeypatch.delenv("HIPEIG_LF_CHUNK", raising=False)
    else:
        monkeypatch.setenv("HIPEIG_LF_CHUNK", str(chunk))


@pytest.fixture(scope="module")
def odd5(hip, problems):
    """The plain run of odd1037's first 5 columns with the row-owner sweep, its NC = 1 and NC = 2 tables and what the
    product pass makes of them - the reference of the cases below, computed once."""
    Hh, Hd, B = problems["odd1037"]
    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:5], *LO)
        plain = hip.lanczos_run(Hd, cols, Z8)
        assert plain.converged and min(len(s.alphas) for s in plain.scalars) > 50
        tables = {"filter": lf.filter_coefficients(plain.scalars, Z8, W8), "near": single_solution_tables(plain, NEAR),
                  "far": single_solution_tables(plain, FAR)}
        combined = {key: arrays(plain.combine(G)) for key, G in tables.items()}
    return cols, plain, tables, combined


# ---- 1. + 2. the hand-over at every ring position and inside a chunk; the combination ----------------------------------
@pytest.mark.parametrize("seg,chunk,p", [("5", "1", 10), ("5", "4", 10), ("5", "7", 10), ("3", "32", 9)])
def test_hand_over_and_combination(hip, problems, odd5, monkeypatch, seg, chunk, p):
    """Room for 10 slots and 100 bytes on a run of about 100 steps: two segments of 5 or three of 3 stay and are written
    to their last slot; the run goes on in the ring from step p - 1, which with chunks of 1, 4, 7 and 32 steps falls on
    a chunk boundary, inside a chunk, and at every position of the ring of three."""
    Hh, Hd, B = problems["odd1037"]
    cols, plain, tables, combined = odd5
    budget = 10 * slot_bytes(1037, 5) + 100
    segments(monkeypatch, seg, chunk)
    with block_variant(Hd, 1):
        run = hip.lanczos_run(Hd, cols, Z8, keepBasis=True, keepPrefix=True, basisBytes=budget)
        assert same_scalars(plain.scalars, run.scalars) and run.info == plain.info
        assert run.products_pass1 == plain.products_pass1 and run.converged
        assert run.basis_vectors == [p] and run.basis_kept == [False]
        assert run.basis_bytes == (p // int(seg)) * int(seg) * slot_bytes(1037, 5)
        for key in ("filter", "near", "filter", "far", "near"):          # again, and with another table in between
            G = tables[key]
            out = run.combine(G)
            assert run.products_pass2 == [max(len(g) for g in G) - p]
            if G[0].shape[1] == 2:
                assert all(isinstance(x, hip.HipComplexVector) for x in out)
            got = arrays(out)
            assert all(x.any() for x in got) and all_equal(got, combined[key]), (key, seg, chunk)
        assert run.basis_vectors == [p]
        run.release()
        assert run.basis_vectors == [0] and run.basis_bytes == 0 and run.basis_kept == [False]
        for key in ("filter", "near"):
            got = arrays(run.combine(tables[key]))
            assert run.products_pass2 == [max(len(g) for g in tables[key]) - 1]
            assert all_equal(got, combined[key])


@pytest.mark.parametrize("p", [1, 2, 3])
def test_the_shortest_prefixes(hip, problems, odd5, monkeypatch, p):
    """Segments of one slot and room for p of them: where pass 2's plan without a basis and its plan behind a prefix
    meet - p = 1: no stream term, the recurrence starts at step 0 with r_0 from slot 0 and zeros for r_{-1}; p = 2: still
    no stream term, first product step 1; p = 3: one stream term."""
    Hh, Hd, B = problems["odd1037"]
    cols, plain, tables, combined = odd5
    segments(monkeypatch, 1)
    with block_variant(Hd, 1):
        run = hip.lanczos_run(Hd, cols, Z8, keepBasis=True, keepPrefix=True, basisBytes=p * slot_bytes(1037, 5) + 100)
        assert same_scalars(plain.scalars, run.scalars)
        assert run.basis_vectors == [p]
        for key in ("filter", "near"):
            G = tables[key]
            got = arrays(run.combine(G))
            assert run.products_pass2 == [max(len(g) for g in G) - p]
            assert all_equal(got, combined[key]), (key, p)
        run.release()


# ---- 3. masks around the seam ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["filter", "near"])
def test_masks_around_the_seam(hip, problems, odd5, monkeypatch, key):
    Hh, Hd, B = problems["odd1037"]
    cols, plain, tables, combined = odd5
    p = 10
    segments(monkeypatch, 5, 4)
    with block_variant(Hd, 1):
        run = hip.lanczos_run(Hd, cols, Z8, keepBasis=True, keepPrefix=True, basisBytes=10 * slot_bytes(1037, 5) + 100)
        assert run.basis_vectors == [p]
        G = tables[key]
        full = len(G[4])
        assert min(len(g) for g in G) > p + 1
        for cut, products in (([p - 2, p - 1, p, p + 1, full], full - p), ([p + 1, p, p - 1, p - 2, 0], 1),
                              ([p - 2, p - 1, p, p, 1], 0), ([0, 0, 3, 0, 0], 0), ([p + 2, 0, 0, 0, 0], 2)):
            Gc = [g[:m] for g, m in zip(G, cut)]
            want = arrays(plain.combine(Gc))
            got = arrays(run.combine(Gc))
            assert run.products_pass2 == [products], (cut, run.products_pass2)
            for r in range(5):
                assert np.array_equal(got[r], want[r]) and bool(got[r].any()) == (cut[r] > 0), (key, cut, r)
        Gl = [g.copy() for g in G]
        Gl[2] = np.ones((len(plain.scalars[2].alphas) + 1, G[2].shape[1]))
        with pytest.raises(ValueError, match="column 2"):
            run.combine(Gl)
        run.release()


# ---- 4. wide tables ----------------------------------------------------------------------------------------------------
def test_wide_tables_from_a_prefix(hip, problems, monkeypatch):
    """About 500 steps, three segments of 32 slots: NC = 4 and 8 take one call, 11 is split 8 + 2 + 1 and pays the tail
    three times; every column of the wide result is the product pass's NC = 1 result for that column of the table."""
    name, K, p = "gapped4000", 3, 96
    Hh, Hd, B = problems[name]
    monkeypatch.delenv("HIPEIG_LF_SEGMENT", raising=False)
    monkeypatch.delenv("HIPEIG_LF_CHUNK", raising=False)
    rng = np.random.default_rng(21)
    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:K], *LO)
        plain = hip.lanczos_run(Hd, cols, Z8)
        run = hip.lanczos_run(Hd, cols, Z8, keepBasis=True, keepPrefix=True, basisBytes=3 * 32 * slot_bytes(4000, K) + 8)
        assert same_scalars(plain.scalars, run.scalars)
        steps = [len(s.alphas) for s in run.scalars]
        assert 200 <= max(steps) <= 1000 and run.basis_vectors == [p] and run.basis_kept == [False]
        wide = [rng.standard_normal((m, 11)) for m in steps]
        tail = max(steps) - p
        one = [arrays(plain.combine([g[:, c] for g in wide])) for c in range(11)]
        for nc, calls in ((4, 1), (8, 1), (11, 3)):
            out = run.combine([g[:, :nc] for g in wide])
            assert run.products_pass2 == [tail * calls] and all(len(o) == nc for o in out)
            for r in range(K):
                for c in range(nc):
                    assert one[c][r].any() and np.array_equal(out[r][c].array, one[c][r]), (nc, r, c)
        run.release()
        none = hip.lanczos_run(Hd, cols, Z8, keepBasis=True, keepPrefix=True, basisBytes=0)
        assert none.basis_vectors == [0]
        with pytest.raises(ValueError, match="NC = 1 or 2"):
            none.combine([g[:, :4] for g in wide])


# ---- 5. enough budget and too little -----------------------------------------------------------------------------------
def test_enough_budget_and_too_little(hip, problems, odd5, monkeypatch):
    Hh, Hd, B = problems["odd1037"]
    cols, plain, tables, combined = odd5
    monkeypatch.delenv("HIPEIG_LF_SEGMENT", raising=False)
    monkeypatch.delenv("HIPEIG_LF_CHUNK", raising=False)
    with block_variant(Hd, 1):
        kept = hip.lanczos_run(Hd, cols, Z8, keepBasis=True)
        whole = hip.lanczos_run(Hd, cols, Z8, keepBasis=True, keepPrefix=True)
        assert whole.basis_kept == kept.basis_kept == [True] and whole.basis_vectors == whole.products_pass1
        assert whole.basis_bytes == kept.basis_bytes and same_scalars(plain.scalars, whole.scalars)
        for key in ("filter", "near"):
            a, b = arrays(kept.combine(tables[key])), arrays(whole.combine(tables[key]))
            assert kept.products_pass2 == whole.products_pass2 == [0]
            assert all_equal(a, b) and all_equal(b, combined[key])
        kept.release()
        whole.release()
        # a stop before the cap is a whole basis too: 4 segments of 32 hold the about 100 steps, the next would not fit
        capped = hip.lanczos_run(Hd, cols, Z8, keepBasis=True, keepPrefix=True, basisBytes=4 * 32 * slot_bytes(1037, 5) + 8)
        assert capped.basis_kept == [True] and capped.basis_vectors == capped.products_pass1
        assert all_equal(arrays(capped.combine(tables["filter"])), combined["filter"]) and capped.products_pass2 == [0]
        capped.release()
        small = hip.lanczos_run(Hd, cols, Z8, keepBasis=True, keepPrefix=True, basisBytes=32 * slot_bytes(1037, 5) - 8)
        assert small.basis_vectors == [0] and small._bases == [None] and small.basis_bytes == 0
        assert same_scalars(plain.scalars, small.scalars)
        assert all_equal(arrays(small.combine(tables["filter"])), combined["filter"])
        assert small.products_pass2 == [max(len(g) for g in tables["filter"]) - 1]


# ---- 6. the window-blocked sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,seg,nseg", [("odd1037", 5, 5, 4), ("tri100", 8, 3, 3)])
def test_prefix_with_the_window_blocked_sweep(hip, problems, monkeypatch, name, K, seg, nseg):
    Hh, Hd, B = problems[name]
    rtol, atol = LO
    n, p = Hh.shape[0], seg * nseg
    segments(monkeypatch, seg)
    with block_variant(Hd, 2):
        run = hip.lanczos_run(Hd, device_columns(hip, B[:K], *LO), Z8, keepBasis=True, keepPrefix=True,
                              basisBytes=nseg * seg * slot_bytes(n, K) + 8)
        assert run.converged and run.basis_vectors == [p] and run.basis_kept == [False]
        qs = arrays(run.combine(lf.filter_coefficients(run.scalars, Z8, W8)))
        assert run.products_pass2 == [run.products_pass1[0] - p] and run.products_pass2[0] > 0
        run.release()
    lam, U = spectrum(name, Hh)
    for r in range(K):
        its, est, conv, xnorms = twin((name, r), Hh, B[r], Z8, rtol, atol, 1.0)
        assert conv.all()
        diff = [int(d) - int(t) for d, t in zip(run.scalars[r].iterations, its)]
        print(f"STEPS {name} K={K} variant=2 prefix column={r} twin={list(map(int, its))} device-twin={diff}")
        assert max(abs(d) for d in diff) <= STEP_DIFFERENCE_BOUND, (name, r, diff)
        f = sum((w / (z - lam)).real for z, w in zip(Z8, W8))
        err = np.linalg.norm(qs[r] - U @ (f * (U.T @ B[r])))
        bound = filter_bound(Hh, lam, Z8, W8, xnorms, max(atol, rtol))
        print(f"FILTER {name} K={K} variant=2 prefix column={r} error {err:.3e} bound {bound:.3e} used {err / bound:.3f}")
        assert np.isfinite(qs[r]).all() and err <= bound, (name, r, err, bound)


# ---- 7. sixteen columns through lanczos_filter ---------------------------------------------------------------------------
def test_sixteen_columns_group_by_group(hip, problems, monkeypatch):
    """Two groups of 8 with room for 50 of their about 100 vectors each (10 segments of 5): both report ``"prefix"``, and
    the second group runs in the segments the first released."""
    Hh, Hd, B = problems["odd1037"]
    segments(monkeypatch, 5)
    p = 50
    budget = p * slot_bytes(1037, 8) + 8
    seen = []
    inner = lf.lanczos_run

    def recording(H, cols, *args, **kw):
        seen.append(reusable_bytes(cols[0].ctx))
        return inner(H, cols, *args, **kw)

    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:16], *LO)
        want = arrays(hip.lanczos_filter(Hd, cols, Z8, W8, basis="recompute"))
        monkeypatch.setattr(lf, "lanczos_run", recording)
        got = arrays(hip.lanczos_filter(Hd, cols, Z8, W8, basis="keep", prefix=True, basisBytes=budget))
        seen.append(reusable_bytes(cols[0].ctx))
    stats = [c.last_solve_stats for c in cols]
    assert [s["basis"] for s in stats] == ["prefix"] * 16 and [s["basis_vectors"] for s in stats] == [p] * 16
    assert [s["group"] for s in stats] == [0] * 8 + [1] * 8
    assert all(s["products_pass2"] == s["products_pass1"] - p and s["products_pass1"] > 60 for s in stats)
    assert all(s["products"] == s["products_pass1"] + s["products_pass2"] for s in stats)
    # reusable bytes before group 0, before group 1, at the end: group 0 leaves at most its 10 segments behind, group 1
    # takes exactly those and gives them back
    assert len(seen) == 3 and 0 <= seen[1] - seen[0] <= p * slot_bytes(1037, 8) and seen[2] == seen[1], seen
    assert all_equal(got, want)


# ---- 8. FEAST end to end -----------------------------------------------------------------------------------------------
def test_feast_end_to_end_with_a_prefix(hip):
    """Config #5 at N = 2e4 (``test_feast_end_to_end_with_the_kept_basis``) with the row-owner sweep and room for 6
    segments of 32 slots: the eigenvalues, the iteration count and the residual of ``"recompute"`` bit for bit.  A run of
    more than 192 steps holds a prefix and pays ``products_pass1 - 192`` products in pass 2.  As FEAST converges its runs
    get shorter (measured: pass 1 products per run 513, 511 in the first iteration, 536 .. 497 in the next three, then
    386 and 179, 150 and 84, 86 and 41): a run that stops within the 192 slots ends as a whole basis and reports
    ``"kept"`` with no product in pass 2 - so ``"prefix"`` is asserted for every run longer than the slots, not for every
    run."""
    import scipy.linalg as la
    N, m0, eConv = 20_000, 16, 1e-4
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    Q = la.qr(np.random.default_rng(9).standard_normal((N, m0)), mode="economic")[0]
    lsa = {"linearSolver": "lanczos_filter", "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7}
    modes = {"recompute": {"lanczosBasis": "recompute"},
             "prefix": {"lanczosBasis": "keep", "lanczosBasisPrefix": True, "lanczosBasisBytes": 6 * 32 * slot_bytes(N, 8)}}
    out = {}
    H.set_block_variant(1)
    try:
        for mode, extra in modes.items():
            o = dict(extra, linearSystemArgs=dict(lsa))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out[mode] = hip.feastDiagonalization(H, [hip.HipVector(Q[:, i].copy(), o) for i in range(m0)], 16, "legendre",
                                                     -0.21, 0.21, eConv, 12, writeOut=False)
    finally:
        H.set_block_variant(0)
    (ev, Y, st), (ev_r, _, st_r) = out["prefix"], out["recompute"]
    assert st["residual"] < eConv
    assert np.array_equal(ev, ev_r) and st["outerIter"] == st_r["outerIter"] and st["residual"] == st_r["residual"]
    assert len(st["lanczosFilter"]) == len(st_r["lanczosFilter"]) == st["outerIter"] + 1
    for it, (rec, rec_r) in enumerate(zip(st["lanczosFilter"], st_r["lanczosFilter"])):
        print(f"FEAST prefix iteration {it}: basis {rec['basis']} vectors {rec['basis_vectors']} products pass 1 "
              f"{rec['products_pass1']} pass 2 {rec['products_pass2']} (recompute: {rec_r['products_pass2']})")
    cap = 6 * 32
    for rec, rec_r in zip(st["lanczosFilter"], st_r["lanczosFilter"]):
        assert rec["runs"] == 2 and rec["products_pass1"] == rec_r["products_pass1"] and rec["steps"] == rec_r["steps"]
        assert rec["basis"] == ["prefix" if p1 > cap else "kept" for p1 in rec["products_pass1"]]
        assert rec["basis_vectors"] == [min(p1, cap) for p1 in rec["products_pass1"]]
        assert rec["products_pass2"] == [p1 - v for p1, v in zip(rec["products_pass1"], rec["basis_vectors"])]
        assert rec_r["basis"] == ["recomputed"] * 2 and rec_r["basis_vectors"] == [0] * 2
    # the tail really runs: the first iterations' runs take about 500 steps each
    assert st["lanczosFilter"][0]["basis"] == ["prefix"] * 2
    assert sum(rec["basis"].count("prefix") for rec in st["lanczosFilter"]) >= 2 * 2


def test_the_option_needs_the_kept_basis(hip, problems):
    Hh, Hd, B = problems["odd1037"]
    o = dict(options(*LO), lanczosBasisPrefix=True)
    v = hip.HipVector(B[0].copy(), o)
    assert v.options["lanczosBasisPrefix"] is True
    with pytest.raises(ValueError, match="lanczosBasisPrefix"):
        hip.feastDiagonalization(Hd, [hip.HipVector(b.copy(), o) for b in B[:2]], 16, "legendre", -0.21, 0.21, 1e-4, 1,
                                 writeOut=False)
    with pytest.raises(ValueError, match="[Pp]refix"):
        hip.lanczos_run(Hd, device_columns(hip, B[:2], *LO), Z8, keepPrefix=True)
