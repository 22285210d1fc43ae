"""A Lanczos basis stored in fp32 on the device (``csrc/lanczos_filter.hip``: ``hipeig_lanczos_block_scalars`` with
``basis_mode`` 3 and 4, ``hipeig_lanczos_combine`` on such a basis, ``hipeig_lanczos_basis_element_bytes``; behind
``lanczos_run(keepBasis=True, basisPrecision="fp32")``, ``lanczos_filter(basis="keep", precision="fp32")`` and the
``HipVector`` option ``"lanczosBasisPrecision"``) against the fp64 paths it sits beside.

Every case fails without the feature: the arguments, the option and the symbol do not exist.

Pass 1 is untouched: its recurrence runs in the fp64 ring on the plain run's operands, so with the row-owner sweep (block
variant 1) scalars are compared with ``same_scalars`` (bit for bit); with the window-blocked sweep (variant 2, add order
not fixed) stop steps stay within ``STEP_DIFFERENCE_BOUND`` of the shifted-MINRES twin, as everywhere.

Pass 2 differs from the fp64 basis's by the rounding of the stored elements alone: an element goes through the same
operations in the same order, and a stored element carries a relative error of at most 2^-24 (round to nearest even, normal
range), so per column and combination ``||q32 - q64|| <= 2^-24 sum_{i in stream} |G[i, c]| ||v_i||`` with ``||v_i|| = 1``.
``rounding_term`` is that sum with 0.1 % on top, which covers ``||v_i|| = 1`` only to rounding and the fp64 roundings of
the accumulation (at most ``m eps ||g||_1``, eight orders below the bound) - derived, not measured.  Where a test checks
against something else than the fp64 basis, its own derived bound (``_lanczos_cases.py``) gets this term added."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from _lanczos_cases import (EPS, FAR, HI, LO, NEAR, W8, Z8, all_equal, arrays, block_variant, build_problems, check_steps,
                            device_columns, exact_filter, filter_bound, lf, options, residual_bound, reusable_bytes,
                            same_scalars, single_solution_tables, slot_bytes, spectrum, twin)

pytestmark = pytest.mark.gpu

NCOLS = 16
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def problems(hip):
    """name -> (host CSR, device operator, host right-hand sides [NCOLS, n]), built once."""
    return build_problems(hip, ("tri100", "gapped4000", "odd1037"), NCOLS)


def rounding_term(G, stream=None):
    """Per combination: 2^-24 * 1.001 * sum_{i < stream} |G[i, c]| (every term when ``stream`` is None)."""
    G = np.asarray(G, dtype=float)
    G = G[:, None] if G.ndim == 1 else G
    return U32 * 1.001 * np.abs(G[:stream]).sum(axis=0)


def run32(hip, Hd, cols, sign=1.0, prefix=False, basisBytes=None):
    return hip.lanczos_run(Hd, cols, Z8, reverseGF=sign < 0, keepBasis=True, keepPrefix=prefix, basisBytes=basisBytes,
                           basisPrecision="fp32")


def element_bytes(run, g=0):
    from eigensolvers_amd import _lib
    out = C.c_int(-1)
    _lib.call("hipeig_lanczos_basis_element_bytes", run.B[0].ctx.handle, run._bases[g], C.byref(out))
    return out.value


def segments(monkeypatch, seg=None, chunk=None):
    for name, value in (("HIPEIG_LF_SEGMENT", seg), ("HIPEIG_LF_CHUNK", chunk)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def check_against_fp64(label, got, want, G, stream=None):
    """got / want: per column an array [n] (NC = 1), complex [n] (NC = 2) or a list of NC arrays."""
    for r, (x, y) in enumerate(zip(got, want)):
        nc = np.asarray(G[r]).shape[1]
        xs = [x] if nc == 1 else [x.real, x.imag] if nc == 2 else list(x)
        ys = [y] if nc == 1 else [y.real, y.imag] if nc == 2 else list(y)
        term = rounding_term(G[r], stream)
        for c in range(nc):
            err = np.linalg.norm(xs[c] - ys[c])
            print(f"FP32 {label} column={r} c={c} error {err:.3e} bound {term[c]:.3e}")
            assert np.isfinite(xs[c]).all() and err <= term[c], (label, r, c, err, term[c])


def wide(vs):
    """The arrays of a ``combine`` result, NC > 2 included."""
    return [[x.array for x in v] if isinstance(v, list) else v.array for v in vs]


@pytest.fixture(scope="module")
def odd5(hip, problems):
    """The plain run of odd1037's first 5 columns with the row-owner sweep, its NC = 1 and NC = 2 tables and what the
    product pass makes of them (which every fp64 basis repeats bit for bit) - the reference below, computed once."""
    Hh, Hd, B = problems["odd1037"]
    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:5], *LO)
        plain = hip.lanczos_run(Hd, cols, Z8)
        assert plain.converged and min(len(s.alphas) for s in plain.scalars) > 50
        tables = {"filter": lf.filter_coefficients(plain.scalars, Z8, W8), "near": single_solution_tables(plain, NEAR),
                  "far": single_solution_tables(plain, FAR)}
        combined = {key: arrays(plain.combine(G)) for key, G in tables.items()}
    return cols, plain, tables, combined


CASES = [("tri100", 8, 1.0, HI), ("odd1037", 3, -1.0, LO), ("odd1037", 5, 1.0, LO), ("gapped4000", 8, -1.0, LO)]


# ---- 1. pass 1 is unchanged ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,sign,tol", CASES)
def test_scalars_are_those_of_the_plain_run(hip, problems, monkeypatch, name, K, sign, tol):
    Hh, Hd, B = problems[name]
    n = Hh.shape[0]
    segments(monkeypatch)
    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:K], *tol)
        plain = hip.lanczos_run(Hd, cols, Z8, reverseGF=sign < 0)
        kept = run32(hip, Hd, cols, sign)
        part = run32(hip, Hd, cols, sign, prefix=True, basisBytes=32 * slot_bytes(n, K) // 2 + 8)
    p1 = plain.products_pass1[0]
    assert plain.basis_precision == "fp64" and kept.basis_precision == part.basis_precision == "fp32"
    for run in (kept, part):
        assert run.converged and same_scalars(plain.scalars, run.scalars)
        assert run.info == plain.info and run.groups == plain.groups and run.products_pass1 == plain.products_pass1
    # memory follows the steps taken: whole segments of 32 slots of n K floats up to the group's last vector
    assert kept.basis_kept == [True] and kept.basis_bytes == -(-p1 // 32) * 32 * slot_bytes(n, K) // 2
    # a prefix also holds its two fp64 hand-over vectors; a run that stopped within the slots is a whole basis and has none
    assert part.basis_vectors == [min(p1, 32)]
    assert part.basis_bytes == 32 * slot_bytes(n, K) // 2 + (2 * slot_bytes(n, K) if p1 > 32 else 0)
    assert element_bytes(kept) == element_bytes(part) == 4 and kept.basis_element_bytes == [4]
    kept.release()
    part.release()
    assert kept.basis_kept == [False] and kept.basis_bytes == 0 and kept.basis_element_bytes == [0]


@pytest.mark.parametrize("name,K,sign", [("odd1037", 5, 1.0), ("odd1037", 3, -1.0), ("tri100", 8, 1.0)])
def test_steps_with_the_window_blocked_sweep(hip, problems, monkeypatch, name, K, sign):
    Hh, Hd, B = problems[name]
    rtol, atol = LO
    segments(monkeypatch, 3)
    with block_variant(Hd, 2):
        runs = {"keep": run32(hip, Hd, device_columns(hip, B[:K], rtol, atol), sign),
                "prefix": run32(hip, Hd, device_columns(hip, B[:K], rtol, atol), sign, prefix=True,
                                basisBytes=9 * slot_bytes(Hh.shape[0], K) // 2 + 8)}
    assert runs["keep"].basis_kept == [True] and runs["prefix"].basis_vectors == [9]
    for mode, run in runs.items():
        assert run.converged
        for r in range(K):
            its, est, conv, xnorms = twin((name, r), Hh, B[r], Z8, rtol, atol, sign)
            assert conv.all()
            check_steps(f"{name} K={K} variant=2 sign={sign:+.0f} fp32 {mode} column={r}", run.scalars[r].iterations, its)
        run.release()


# ---- 2. the combination against the fp64 basis of the same run ---------------------------------------------------------
@pytest.mark.parametrize("name,K,sign,tol", CASES)
def test_combination_against_the_fp64_basis(hip, problems, monkeypatch, name, K, sign, tol):
    Hh, Hd, B = problems[name]
    segments(monkeypatch)
    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:K], *tol)
        k64 = hip.lanczos_run(Hd, cols, Z8, reverseGF=sign < 0, keepBasis=True)
        k32 = run32(hip, Hd, cols, sign)
        assert k64.basis_kept == k32.basis_kept == [True] and same_scalars(k64.scalars, k32.scalars)
        assert 2 * k32.basis_bytes == k64.basis_bytes > 0
        assert element_bytes(k32) == 4 and element_bytes(k64) == 8
        G = lf.filter_coefficients(k64.scalars, Z8, W8, sign)
        want, got = k64.combine(G), k32.combine(G)
        assert k32.products_pass2 == [0]
        assert all(isinstance(x, hip.HipVector) and not isinstance(x, hip.HipComplexVector) for x in got)
        got = arrays(got)
        assert all(x.any() for x in got)
        check_against_fp64(f"{name} K={K} sign={sign:+.0f} filter", got, arrays(want), G)
        # the basis is never written: a second call gives the same bits
        assert all_equal(arrays(k32.combine(G)), got)
        k64.release()
        k32.release()


# ---- 3. filtered vectors against the exact filter ----------------------------------------------------------------------
@pytest.mark.parametrize("name,K,sign,variant", [("odd1037", 5, 1.0, 1), ("odd1037", 3, -1.0, 2), ("tri100", 8, -1.0, 1),
                                                 ("tri100", 8, 1.0, 2), ("gapped4000", 8, 1.0, 2)])
def test_filtered_vectors(hip, problems, monkeypatch, name, K, sign, variant):
    Hh, Hd, B = problems[name]
    rtol, atol = LO
    segments(monkeypatch)
    with block_variant(Hd, variant):
        run = run32(hip, Hd, device_columns(hip, B[:K], rtol, atol), sign)
        assert run.basis_kept == [True] and run.converged
        G = lf.filter_coefficients(run.scalars, Z8, W8, sign)
        qs = arrays(run.combine(G))
        assert run.products_pass2 == [0]
        run.release()
    lam, U = spectrum(name, Hh)
    for r in range(K):
        its, est, conv, xnorms = twin((name, r), Hh, B[r], Z8, rtol, atol, sign)
        err = np.linalg.norm(qs[r] - exact_filter(lam, U, B[r], Z8, W8, sign))
        bound = filter_bound(Hh, lam, Z8, W8, xnorms, max(atol, rtol)) + rounding_term(G[r])[0]
        print(f"FILTER {name} K={K} variant={variant} fp32 column={r} error {err:.3e} bound {bound:.3e} used {err / bound:.3f}")
        assert np.isfinite(qs[r]).all() and err <= bound, (name, r, err, bound)


# ---- 4. single solutions through NC = 2 --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sign,tol,variant", [("gapped4000", 1.0, LO, 2), ("odd1037", -1.0, HI, 1)])
def test_single_solutions(hip, problems, monkeypatch, name, sign, tol, variant):
    Hh, Hd, B = problems[name]
    rtol, atol = tol
    K = 2
    hinf = abs(Hh).sum(axis=1).max()
    segments(monkeypatch)
    with block_variant(Hd, variant):
        run = run32(hip, Hd, device_columns(hip, B[:K], rtol, atol), sign)
        assert run.basis_kept == [True] and run.converged
        for j in (NEAR, FAR):
            Gj = single_solution_tables(run, j, sign)
            xs = run.combine(Gj)
            assert run.products_pass2 == [0] and all(isinstance(x, hip.HipComplexVector) for x in xs)
            for r, x in enumerate(xs):
                xa = x.array
                res = np.linalg.norm(B[r] - sign * (Z8[j] * xa - Hh @ xa))
                target = max(atol, rtol)
                bound = residual_bound(Hh, Z8[j], xa, target) + (abs(Z8[j]) + hinf) * U32 * np.hypot(Gj[r][:, 0], Gj[r][:, 1]).sum()
                print(f"RESIDUAL {name} fp32 sign={sign:+.0f} shift={j} column={r} true {res:.3e} bound {bound:.3e}")
                assert np.isfinite(xa).all() and res <= bound, (name, j, r, res, bound)
        run.release()


# ---- 5. masking ------------------------------------------------------------------------------------------------------
def test_masking_of_columns_that_stop_at_very_different_steps(hip, problems, monkeypatch):
    """The block of ``test_gpu_lanczos_basis.py``: a random column, a sum of 6 eigenvectors (its Krylov space is exhausted
    within 7 steps), a zero column (no step at all) and a second random column; then tables shorter than the steps run."""
    name = "odd1037"
    Hh, Hd, B = problems[name]
    lam, U = spectrum(name, Hh)
    few = U[:, [3, 200, 517, 518, 800, 1030]] @ np.array([1.0, -0.5, 0.7, 0.3, -1.2, 0.9])
    cols_h = np.array([B[0], few / np.linalg.norm(few), np.zeros(1037), B[1]])
    segments(monkeypatch)
    with block_variant(Hd, 1):
        cols = device_columns(hip, cols_h, *LO)
        k64 = hip.lanczos_run(Hd, cols, Z8, keepBasis=True)
        k32 = run32(hip, Hd, cols)
        assert k32.basis_kept == [True] and same_scalars(k64.scalars, k32.scalars)
        steps = [len(s.alphas) for s in k32.scalars]
        assert steps[2] == 0 and 1 <= steps[1] <= 8 and min(steps[0], steps[3]) >= 10 * steps[1]
        G = lf.filter_coefficients(k32.scalars, Z8, W8)
        full = arrays(k32.combine(G))
        check_against_fp64("masking full", full, arrays(k64.combine(G)), G)
        assert not full[2].any() and full[1].any()
        for cut in ([7, 3, 0, steps[3] - 1], [0, steps[1], 0, 1]):
            Gc = [g[:m] for g, m in zip(G, cut)]
            got = arrays(k32.combine(Gc))
            assert k32.products_pass2 == [0]
            check_against_fp64(f"masking cut={cut}", got, arrays(k64.combine(Gc)), Gc)
            for r in range(4):
                assert bool(got[r].any()) == (cut[r] > 0), (cut, r)
        Gl = [g.copy() for g in G]
        Gl[1] = np.ones((steps[1] + 1, 1))
        with pytest.raises(ValueError, match="column 1"):
            k32.combine(Gl)
        k64.release()
        k32.release()


def test_breakdown_ends_in_one_step_with_the_exact_answer(hip):
    """b = 2 e_3 on a diagonal operator: one step, and 2.0 is an fp32 number, so the stored vector is exact and the bound
    is the fp64 one of ``test_gpu_lanczos_basis.py``."""
    h = np.linspace(-1.0, 1.0, 64)
    Hd = hip.HipCsrOperator.from_scipy(sp.diags(h).tocsr())
    b = np.zeros(64)
    b[3] = 2.0
    zs, ws = Z8 + [0.5], W8 + [0.3 - 0.1j]
    for sign in (1.0, -1.0):
        cols = device_columns(hip, [b], 1e-10, 1e-12, 100)
        q = hip.lanczos_filter(Hd, cols, zs, ws, reverseGF=sign < 0, basis="keep", precision="fp32")[0].array
        st = cols[0].last_solve_stats
        assert st["iterations"] == [1] * 9 and st["estimates"] == [0.0] * 9
        assert st["products"] == 1 and st["products_pass2"] == 0 and st["basis"] == "kept" and st["basis_precision"] == "fp32"
        exact = sum((w * sign * 2.0 / (z - h[3])).real for z, w in zip(zs, ws))
        assert np.count_nonzero(q) == 1 and abs(q[3] - exact) <= 8 * EPS * sum(abs(w * 2.0 / (z - h[3])) for z, w in zip(zs, ws))


def test_all_zero_columns_keep_nothing_and_give_zeros(hip, problems):
    Hh, Hd, B = problems["gapped4000"]
    for prefix in (False, True):
        run = run32(hip, Hd, device_columns(hip, np.zeros((2, 4000)), *LO), prefix=prefix)
        assert run.basis_kept == [False] and run.products_pass1 == [0] and run.basis_bytes == 0
        assert all(not q.array.any() for q in run.combine([np.zeros((0, 1))] * 2))


# ---- 6. segment and chunk boundaries ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", [False, True])
def test_segment_and_chunk_boundaries(hip, problems, odd5, monkeypatch, prefix):
    """Segments of 1 and 3 slots, the state record looked at after every step and after every 5: the scalars and the
    combined vectors of the default segment and chunk in the same mode, bit for bit (``prefix``: mode 4 with room for the
    whole basis)."""
    Hh, Hd, B = problems["odd1037"]
    cols, plain, tables, combined = odd5
    out = []
    with block_variant(Hd, 1):
        for seg, chunk in ((None, None), (1, 1), (1, 5), (3, 1), (3, 5)):
            segments(monkeypatch, seg, chunk)
            run = run32(hip, Hd, cols, prefix=prefix)
            assert run.basis_kept == [True] and same_scalars(plain.scalars, run.scalars)
            p = run.products_pass1[0]
            assert run.basis_bytes == -(-p // (seg or 32)) * (seg or 32) * slot_bytes(1037, 5) // 2
            out.append((arrays(run.combine(tables["filter"])), arrays(run.combine(tables["near"]))))
            assert run.products_pass2 == [0]
            run.release()
    check_against_fp64("seams filter", out[0][0], combined["filter"], tables["filter"])
    for q, x in out[1:]:
        assert all_equal(out[0][0], q) and all_equal(out[0][1], x)


# ---- 7. budget -------------------------------------------------------------------------------------------------------
def test_a_budget_of_ten_fp64_slots(hip, problems, odd5, monkeypatch):
    """Room for ten fp64 slots and 100 bytes, 5 slots per segment, a run of about 100 steps: mode 4 holds four segments -
    twenty vectors; mode 3 cannot hold the run, frees what it had and finishes as the plain run."""
    Hh, Hd, B = problems["odd1037"]
    cols, plain, tables, combined = odd5
    budget = 10 * slot_bytes(1037, 5) + 100
    segments(monkeypatch, 5, 4)
    with block_variant(Hd, 1):
        part = run32(hip, Hd, cols, prefix=True, basisBytes=budget)
        assert part.basis_vectors == [20] and part.basis_kept == [False] and same_scalars(plain.scalars, part.scalars)
        assert part.basis_bytes == 20 * slot_bytes(1037, 5) // 2 + 2 * slot_bytes(1037, 5) and element_bytes(part) == 4
        part.release()
        none = run32(hip, Hd, cols, basisBytes=budget)
        assert none.basis_kept == [False] and none._bases == [None] and none.basis_bytes == 0 and none.basis_vectors == [0]
        assert same_scalars(plain.scalars, none.scalars) and none.products_pass1 == plain.products_pass1
        assert all_equal(arrays(none.combine(tables["filter"])), combined["filter"])
        assert none.products_pass2 == [max(len(g) for g in tables["filter"]) - 1]
        qf = arrays(hip.lanczos_filter(Hd, cols, Z8, W8, basis="keep", precision="fp32", basisBytes=budget))
        assert all(c.last_solve_stats["basis"] == "recomputed" and c.last_solve_stats["basis_precision"] == "fp32" for c in cols)
        assert all(c.last_solve_stats["products_pass2"] == c.last_solve_stats["products_pass1"] - 1 for c in cols)
        assert all_equal(qf, combined["filter"])


def test_released_segments_are_handed_out_again_at_the_fp32_size(hip, problems, monkeypatch):
    name, K = "odd1037", 3
    Hh, Hd, B = problems[name]
    segments(monkeypatch)
    cols = device_columns(hip, B[:K], *LO)
    ctx = cols[0].ctx
    run = run32(hip, Hd, cols)
    held, before = run.basis_bytes, reusable_bytes(ctx)
    assert held > 0 and held % (32 * slot_bytes(1037, K) // 2) == 0
    run.release()
    assert reusable_bytes(ctx) == before + held
    again = run32(hip, Hd, cols)
    assert again.basis_bytes == held and reusable_bytes(ctx) <= before
    again.release()


# ---- 8. the prefix and its hand-over vectors -----------------------------------------------------------------------------
@pytest.mark.parametrize("seg,chunk,p", [(1, None, 1), (1, None, 2), (1, None, 3), (1, 1, 3), (5, 4, 10), (3, 32, 9)])
def test_prefix_hand_over(hip, problems, odd5, monkeypatch, seg, chunk, p):
    """Room for p fp32 slots and 100 bytes.  Pass 2's recurrence restarts from the fp64 hand-over vectors, so only the
    stream's terms i < p - 1 carry a rounding: with p = 1 there is none and the result is the fp64 one bit for bit.  (5, 4, 10): the hand-over is made before step 9, inside the chunk of steps 8 .. 11; (3, 32, 9): inside the first
    chunk; chunk 1: at a chunk boundary."""
    Hh, Hd, B = problems["odd1037"]
    cols, plain, tables, combined = odd5
    segments(monkeypatch, seg, chunk)
    with block_variant(Hd, 1):
        run = run32(hip, Hd, cols, prefix=True, basisBytes=p * slot_bytes(1037, 5) // 2 + 100)
        assert same_scalars(plain.scalars, run.scalars) and run.info == plain.info and run.converged
        assert run.basis_vectors == [p] and run.basis_kept == [False] and element_bytes(run) == 4
        # the segments, and on top of the budget the two fp64 hand-over vectors - which are freed, not pooled, on release
        assert run.basis_bytes == p * slot_bytes(1037, 5) // 2 + 2 * slot_bytes(1037, 5)
        reusable = reusable_bytes(cols[0].ctx)
        for key in ("filter", "near", "filter"):                         # again: the basis and its hand-over are never written
            G = tables[key]
            mmax = max(len(g) for g in G)
            got = arrays(run.combine(G))
            stream, products = lf.prefix_split(mmax, p)
            assert run.products_pass2 == [products] and stream == p - 1 and products == mmax - p
            if stream == 0:
                assert all_equal(got, combined[key]), (key, p)
            else:
                check_against_fp64(f"prefix p={p} seg={seg} chunk={chunk} {key}", got, combined[key], G, stream)
                assert not all_equal(got, combined[key])                 # the stream really read fp32 slots
        run.release()
        assert run.basis_vectors == [0] and run.basis_bytes == 0
        assert reusable_bytes(cols[0].ctx) == reusable + p * slot_bytes(1037, 5) // 2
        assert all_equal(arrays(run.combine(tables["filter"])), combined["filter"])


# ---- 9. wide tables --------------------------------------------------------------------------------------------------
def test_wide_tables_from_one_run(hip, problems, monkeypatch):
    """NC = 8 takes one call, NC = 11 is split 8 + 2 + 1; every column of the table answers to the bound against the fp64
    basis, and the same column gives the same bits in whichever call it is served."""
    name, K = "odd1037", 5
    Hh, Hd, B = problems[name]
    rng = np.random.default_rng(21)
    segments(monkeypatch)
    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:K], *LO)
        k64 = hip.lanczos_run(Hd, cols, Z8, keepBasis=True)
        k32 = run32(hip, Hd, cols)
        assert k32.basis_kept == [True]
        table = [rng.standard_normal((len(sc.alphas), 11)) for sc in k32.scalars]
        out11, want11 = wide(k32.combine(table)), wide(k64.combine(table))
        assert k32.products_pass2 == [0] and all(len(o) == 11 for o in out11)
        check_against_fp64("wide NC=11", out11, want11, table)
        out8 = wide(k32.combine([g[:, :8] for g in table]))
        out4 = wide(k32.combine([g[:, 7:11] for g in table]))
        one = arrays(k32.combine([g[:, 10] for g in table]))
        for r in range(K):
            assert all(x.any() for x in out8[r]) and all_equal(out8[r], out11[r][:8]), r
            assert all_equal(out4[r], out11[r][7:11]) and np.array_equal(one[r], out11[r][10]), r
        k64.release()
        k32.release()


# ---- 10. sixteen columns through lanczos_filter ------------------------------------------------------------------------
def test_sixteen_columns_group_by_group(hip, problems, monkeypatch):
    """Two groups of 8.  The budget holds either group's fp32 basis (its segments and the one more a run allocates ahead
    of the chunk in which it stops) but not both: ``lanczos_filter`` works group by group, so both are kept, one after the
    other; one ``lanczos_run`` holds the first while the second runs, so the second is not kept."""
    Hh, Hd, B = problems["odd1037"]
    segments(monkeypatch)
    seg_bytes = 32 * slot_bytes(1037, 8) // 2
    with block_variant(Hd, 1):
        cols = device_columns(hip, B[:16], *LO)
        plain = hip.lanczos_run(Hd, cols, Z8)
        G = lf.filter_coefficients(plain.scalars, Z8, W8)
        want = arrays(plain.combine(G))
        peaks = []
        for lo in (0, 8):
            one = run32(hip, Hd, cols[lo:lo + 8])
            assert one.basis_kept == [True] and one.basis_bytes % seg_bytes == 0
            peaks.append(one.basis_bytes + seg_bytes)
            one.release()
        budget = max(peaks)
        got = arrays(hip.lanczos_filter(Hd, cols, Z8, W8, basis="keep", precision="fp32", basisBytes=budget))
        stats = [c.last_solve_stats for c in cols]
        assert [s["basis"] for s in stats] == ["kept"] * 16 and [s["basis_precision"] for s in stats] == ["fp32"] * 16
        assert [s["group"] for s in stats] == [0] * 8 + [1] * 8 and all(s["products_pass2"] == 0 for s in stats)
        check_against_fp64("sixteen columns", got, want, G)
        run = run32(hip, Hd, cols, basisBytes=budget)
        assert run.basis_kept == [True, False] and 0 < run.basis_bytes <= budget and run.basis_element_bytes == [4, 0]
        assert same_scalars(plain.scalars, run.scalars)
        q = arrays(run.combine(G))
        assert run.products_pass2 == [0, plain.products_pass2[1]]
        assert all_equal(q[:8], got[:8]) and all_equal(q[8:], want[8:])
        run.release()


# ---- 11. FEAST end to end --------------------------------------------------------------------------------------------
def test_feast_end_to_end_with_the_fp32_basis(hip):
    """Config #5 at N = 2e4, the problem of ``test_feast_end_to_end_with_the_kept_basis``, with the row-owner sweep and
    ``"lanczosBasisPrecision": "fp32"`` against ``"recompute"``.  That test compares eigenvalues bit for bit, which an fp64
    basis gives and a rounded one cannot; what takes its place here is tied to the 2^-24 model, step by step:

    * the filtered vectors of the first iteration, through the hook FEAST calls (``HipVector._lanczos_filter``, which reads
      the option): ``||q32_j - q64_j|| <= tau_j = 2^-24 * 1.001 * ||g_j||_1`` per subspace vector, as everywhere above;
    * the Ritz values after that iteration (``maxit=1``).  With ``E = Q32 - Q64``, ``||E||_F <= tau = ||(tau_j)||_2``, the
      Loewdin bases are the polar factors ``U``, ``U'`` of ``Q64``, ``Q32``, ``||U - U'||_F <= 2 ||E||_F / (sigma + sigma')``
      (Higham, the polar factor of a full-rank matrix) with ``sigma' >= sigma - tau`` the smallest singular values, the
      Ritz matrices differ by at most ``2 ||H||_2 ||U - U'||`` and Weyl's theorem carries that to every Ritz value:
      ``|theta_i - theta'_i| <= 4 ||H||_inf tau / (2 sigma - tau)``, plus ``100 eps ||H||_inf`` for the roundings of the
      two dense eigenproblems;
    * the whole run: converged, the same number of iterations, every run's basis kept in fp32 with no product in pass 2,
      and the first iteration - the same input vectors, pass 1 untouched - with ``recompute``'s products and stop steps
      exactly.  (FEAST corrects a filter's error from iteration to iteration, so the converged eigenvalues say little
      about the stream; measured: they differ by 6.4e-14.)"""
    import scipy.linalg as la
    from eigensolvers_amd.generators import gapped_csr_host
    N, m0, eConv = 20_000, 16, 1e-4
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    hinf = abs(gapped_csr_host(N, 32, seed=7)).sum(axis=1).max()
    Q = la.qr(np.random.default_rng(9).standard_normal((N, m0)), mode="economic")[0]
    lsa = {"linearSolver": "lanczos_filter", "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7}
    modes = {"recompute": {"lanczosBasis": "recompute"}, "fp32": {"lanczosBasis": "keep", "lanczosBasisPrecision": "fp32"}}

    def vectors(mode):
        o = dict(modes[mode], linearSystemArgs=dict(lsa))
        return [hip.HipVector(Q[:, i].copy(), o) for i in range(m0)]

    def feast(mode, maxit):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return hip.feastDiagonalization(H, vectors(mode), 16, "legendre", -0.21, 0.21, eConv, maxit, writeOut=False)

    H.set_block_variant(1)
    try:
        # the first iteration's filtered vectors, through FEAST's hook, and their coefficient tables
        Y32 = vectors("fp32")
        q64 = np.array(arrays(hip.HipVector._lanczos_filter(H, vectors("recompute"), Z8, W8))).T
        q32 = np.array(arrays(hip.HipVector._lanczos_filter(H, Y32, Z8, W8))).T
        assert [y.last_solve_stats["basis_precision"] for y in Y32] == ["fp32"] * m0
        G = lf.filter_coefficients(hip.lanczos_run(H, vectors("recompute"), Z8).scalars, Z8, W8)
        one, one_r = feast("fp32", 1), feast("recompute", 1)
        out, out_r = feast("fp32", 12), feast("recompute", 12)
    finally:
        H.set_block_variant(0)
    tau_j = np.array([rounding_term(g)[0] for g in G])
    err_j = np.linalg.norm(q32 - q64, axis=0)
    print("FEAST fp32 first filter: error / bound per vector", [f"{e / t:.3f}" for e, t in zip(err_j, tau_j)])
    assert np.isfinite(q32).all() and (err_j <= tau_j).all() and err_j.min() > 0.0, (err_j, tau_j)
    tau, sigma = float(np.linalg.norm(tau_j)), float(np.linalg.svd(q64, compute_uv=False)[-1])
    bound = 4.0 * hinf * tau / (2.0 * sigma - tau) + 100 * EPS * hinf
    diff = np.abs(np.asarray(one[0]) - np.asarray(one_r[0])).max()
    print(f"FEAST fp32 Ritz values after one iteration: difference {diff:.3e} bound {bound:.3e} (tau {tau:.3e} sigma {sigma:.3e})")
    assert sigma > tau and np.shape(one[0]) == np.shape(one_r[0]) == (m0,) and diff <= bound, (diff, bound)
    (ev, Y, st), (ev_r, _, st_r) = out, out_r
    print(f"FEAST fp32 iterations {st['outerIter']} / {st_r['outerIter']} change {st['residual']:.3e} / {st_r['residual']:.3e} "
          f"largest eigenvalue difference {np.abs(np.asarray(ev) - np.asarray(ev_r)).max():.3e}")
    assert st["residual"] < eConv and st["outerIter"] == st_r["outerIter"] and np.shape(ev) == np.shape(ev_r)
    assert len(st["lanczosFilter"]) == len(st_r["lanczosFilter"]) == st["outerIter"] + 1
    for rec, rec_r in zip(st["lanczosFilter"], st_r["lanczosFilter"]):
        assert rec["runs"] == 2 and rec["basis"] == ["kept"] * 2 and rec["products_pass2"] == [0] * 2
        assert rec["basis_precision"] == ["fp32"] * 2 and rec_r["basis_precision"] == ["fp64"] * 2
        assert rec_r["basis"] == ["recomputed"] * 2 and rec_r["products_pass2"] == [p - 1 for p in rec_r["products_pass1"]]
    first, first_r = st["lanczosFilter"][0], st_r["lanczosFilter"][0]
    assert first["products_pass1"] == first_r["products_pass1"] and first["steps"] == first_r["steps"]


# ---- 12. refusals ----------------------------------------------------------------------------------------------------
def scalars_call(Hd, cols, mode, budget=1 << 40):
    """``hipeig_lanczos_block_scalars`` at the C ABI with ``basis_mode = mode``; returns the basis handle."""
    from eigensolvers_amd import _lib
    from eigensolvers_amd.hip_vector import _ptr_table
    k, S, maxiter = len(cols), len(Z8), 40
    bt, keep = _ptr_table([b._buf for b in cols])
    dp = C.POINTER(C.c_double)
    zr, zi = (C.c_double * S)(*[z.real for z in Z8]), (C.c_double * S)(*[z.imag for z in Z8])
    alphas, betas = np.zeros((k, maxiter)), np.zeros((k, maxiter + 1))
    its, est, info, stats = (C.c_int * (k * S))(), (C.c_double * (k * S))(), (C.c_int * k)(), (C.c_double * (1 + k))()
    basis = C.c_void_p()
    _lib.call("hipeig_lanczos_block_scalars", cols[0].ctx.handle, Hd.handle, 1.0, k, bt, S, zr, zi, 1e-5, 1e-7, maxiter,
              alphas.ctypes.data_as(dp), betas.ctypes.data_as(dp), its, est, info, stats, mode, budget, C.byref(basis))
    return basis


def test_refusals(hip, problems):
    from eigensolvers_amd import _lib
    Hh, Hd, B = problems["odd1037"]
    Hh4, Hd4, B4 = problems["gapped4000"]
    cols = device_columns(hip, B[:5], *LO)
    ctx = cols[0].ctx
    for mode in (5, -1):
        with pytest.raises(_lib.HipEigError, match="basis mode"):
            scalars_call(Hd, cols, mode)
    with pytest.raises(_lib.HipEigError, match="byte budget"):
        scalars_call(Hd, cols, 3, budget=-1)
    handle = scalars_call(Hd, cols, 3)                                   # 40 steps: the step limit, a basis all the same
    assert handle.value
    out = C.c_int(-1)
    _lib.call("hipeig_lanczos_basis_element_bytes", ctx.handle, handle, C.byref(out))
    assert out.value == 4
    _lib.call("hipeig_lanczos_basis_element_bytes", ctx.handle, None, C.byref(out))
    assert out.value == 0
    with pytest.raises(_lib.HipEigError, match="null"):
        _lib.call("hipeig_lanczos_basis_element_bytes", ctx.handle, handle, None)
    # a basis kept for another column count, and for another operator
    fewer = hip.lanczos_run(Hd, cols[:3], Z8)
    other = hip.lanczos_run(Hd4, device_columns(hip, B4[:5], *LO), Z8)
    try:
        for run, what in ((fewer, "number of columns"), (other, "operator")):
            run._bases[0] = handle
            with pytest.raises(_lib.HipEigError, match=what):
                run.combine([np.ones((3, 1))] * len(run.B))
            run._bases[0] = None
    finally:
        fewer._bases[0] = other._bases[0] = None
        _lib.call("hipeig_lanczos_basis_release", ctx.handle, handle)
    with pytest.raises(ValueError, match="kept"):
        hip.lanczos_run(Hd, cols, Z8, basisPrecision="fp32")
    with pytest.raises(ValueError, match="precision"):
        hip.lanczos_filter(Hd, cols, Z8, W8, basis="keep", precision="fp16")
    bad = dict(options(*LO), lanczosBasisPrecision="fp32")
    v = hip.HipVector(B[0].copy(), bad)
    assert v.options["lanczosBasisPrecision"] == "fp32" and "lanczosBasisPrecision" not in cols[0].options
    with pytest.raises(ValueError, match="lanczosBasisPrecision"):
        hip.feastDiagonalization(Hd, [hip.HipVector(b.copy(), bad) for b in B[:2]], 16, "legendre", -0.21, 0.21, 1e-4, 1,
                                 writeOut=False)
