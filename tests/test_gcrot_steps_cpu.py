"""The reference of the GCROT step tests checked without a GPU (``_gcrot_steps.py``): the ``longdouble`` recurrence against
dense ``longdouble`` solves, the project's generator under every float64 summation order against it (``D``, ``D_SMALL``,
the invariants' constants), the planted faults, the margins of the exits and the two conditions on every primitive bound."""
import math

import numpy as np
import pytest

import _gcrot_steps as gs
import _hiprec as hp
import _minres_steps as ms
from test_hiprec_cpu import CUS, _emu_dot, _emu_lincomb, _fma

needs_extended = pytest.mark.skipif(not hp.EXTENDED, reason="longdouble is no wider than double on this machine")
LD, CLD = hp.LD, hp.CLD


# ---------------------------------------------------------------- Wide against a dense longdouble solve
def _dense_solve(A, b):
    """Gaussian elimination with partial pivoting, every operation in the dtype of ``A`` (longdouble / clongdouble)."""
    A, b = A.copy(), b.astype(A.dtype)
    n = len(b)
    for i in range(n):
        p = i + int(np.argmax(np.abs(A[i:, i])))
        if p != i:
            A[[i, p]], b[[i, p]] = A[[p, i]], b[[p, i]]
        for j in range(i + 1, n):
            f = A[j, i] / A[i, i]
            A[j, i:] -= f * A[i, i:]
            b[j] -= f * b[i]
    x = np.zeros(n, dtype=A.dtype)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - np.sum(A[i, i + 1:] * x[i + 1:])) / A[i, i]
    return x


@needs_extended
@pytest.mark.parametrize("opname", ["dense1", "dense2", "g63"])
@pytest.mark.parametrize("z", [gs.Z_REAL, gs.Z_PAIR], ids=["real", "pair"])
def test_wide_reaches_the_dense_solution_when_the_inner_space_reaches_n(opname, z):
    """One cycle whose inner space has n dimensions solves the system: the breakdown branch ends the loop at step n (on
    g63 the cycle is given m + k = 63 steps and ends there) and ``x`` is the dense ``longdouble`` solution to 2^-56 of
    ``max |x|`` - an eighth of the double rounding unit the runs are read in; the two ``longdouble`` solves themselves
    differ by the condition of g63 at z = 0.02, some 200, times 2^-64 - with ``r`` at that level too."""
    op = ms.operator(opname)
    pair = isinstance(z, complex)
    T = CLD if pair else LD
    b = ms.rhs(op.n, ms.SMALL_SEEDS.get(op.n))
    for sign in (1.0, -1.0):
        m, k = (gs.M_INNER, gs.K_OUTER) if op.n <= 2 else (op.n - 2, 2)
        run = gs.cycles(op, b, z, sign, m, k, 1, gs.Wide(pair))
        A = (LD(sign) * (T(z) * np.eye(op.n, dtype=T) - gs.stored(op).toarray().astype(T)))
        x = _dense_solve(A, b)
        assert run[0]["inner"] == run[0]["products"] == op.n
        assert float(np.max(np.abs(run[0]["x"] - x)) / np.max(np.abs(x))) <= 2.0 ** -56
        assert float(hp.nrm2(run[0]["r"])) <= 2.0 ** -56
    if op.n <= 2:
        assert gs.reference(gs.CASES[f"{opname} {'pair' if pair else 'real'}"])[0]["inner"] == op.n


def test_givens_least_squares_against_lstsq():
    """The rotations solve ``min ||e_1 - H y||``: float64 and complex128 Hessenberg matrices against ``numpy.linalg.lstsq``,
    the rotated matrix upper triangular with ``|R y| = |H y|``, the residual the norm of ``e_1 - H y``."""
    rng = np.random.default_rng(3)
    for T in (np.float64, np.complex128):
        for cols in (1, 2, 5):
            H = np.triu(rng.standard_normal((cols + 1, cols)) + (1j * rng.standard_normal((cols + 1, cols)) if T is np.complex128 else 0), -1)
            e1 = np.zeros(cols + 1, dtype=T)
            e1[0] = 1
            y, R, res = gs.givens_lstsq(H, T)
            want = np.linalg.lstsq(H, e1, rcond=None)[0]
            np.testing.assert_allclose(y, want, rtol=1e-12, atol=1e-14)
            assert np.allclose(np.tril(R, -1), 0) and np.allclose(R[-1], 0)
            assert np.linalg.norm(R @ y) == pytest.approx(np.linalg.norm(H @ y), rel=1e-12)
            assert res == pytest.approx(np.linalg.norm(e1 - H @ y), rel=1e-10)


# ---------------------------------------------------------------- D and the invariants' constants
def _worst_rows(table):
    worst = {}
    for (name, cyc, order), (d, q) in table.items():
        if d > worst.get(name, (0.0,))[0]:
            worst[name] = (d, cyc, order, q)
    return worst


@needs_extended
@pytest.mark.parametrize("small", [False, True], ids=["large", "small"])
def test_no_summation_order_deviates_by_more_than_D(small):
    """The project's generator on the NumPy provider, every order, against the ``longdouble`` recurrence: the committed
    constant is the measurement rounded up, not a loose cover of it."""
    Dm, table = gs.measured_deviation(small)
    for name, (d, cyc, order, q) in _worst_rows(table).items():
        print(f"GCROT-CPU {name}: {d:.2f} u ({q}, cycle {cyc}, {order})")
    const = gs.D_SMALL if small else gs.D
    print(f"GCROT-CPU {'D_SMALL' if small else 'D'} measured {Dm:.2f} u, constant {const}")
    assert 0.9 * const <= Dm <= const


@needs_extended
def test_invariants_of_the_float64_runs_stay_under_their_constants():
    inv, table = gs.measured_invariants()
    for q in gs.INVARIANTS:
        key = max(table, key=lambda kk: table[kk][q])
        print(f"GCROT-CPU invariant {q}: {inv[q]:.2f} u ({key[0]}, {key[1]}), constant {gs.INV[q]}")
        assert 0.9 * gs.INV[q] <= inv[q] <= gs.INV[q]


@needs_extended
def test_schedule_counts_and_the_restated_float64_form():
    """GCROT(3, 2) takes 5, 4, 3, 3, 3, 3 inner steps, a product each (21), in the reference and in the project's
    generator; the restated recurrence in float64 - the form the faults are planted in - is within D of the reference
    like the generator itself, so a fault's excess is the fault's."""
    for case in gs.CASES.values():
        ref = gs.reference(case)
        want = [5, 4, 3, 3, 3, 3][:case.ncycles] if case.op.n > 2 else [case.op.n]
        run = gs.run_double(case, "dot")
        for r in (ref, run):
            assert [rec["inner"] for rec in r] == want and [rec["products"] for rec in r] == want
        assert run.products == sum(want) + (1 if case.with_x0 else 0) and run.outer == run.info == case.ncycles
        plain = gs.cycles(case.op, case.b, case.z, case.sign, gs.M_INNER, gs.K_OUTER, case.ncycles, gs.Double("dot", case.pair),
                          x0=case.x0, minv=case.minv, fault="none")
        for g, r in zip(plain, ref):
            assert max(gs.deviations(g, r).values()) <= (gs.D_SMALL if case.small else gs.D), case.name
        assert gs.invariant_excess(gs.case_invariants(case, plain))[0] <= 1.0
    assert sum(rec["products"] for rec in gs.reference(gs.CASES["g1037 real sign=+1"])) == 21


# ---------------------------------------------------------------- planted faults
FAULT_CASES = ("g1037 real sign=+1", "g1037 pair sign=-1", "g20001 pair", "g1037 real x0", "g1037 pair x0", "g1037 real jacobi",
               "g1037 pair jacobi")


def _applies(fault, case):
    if fault == "r_is_b":
        return case.with_x0
    if fault == "no_final_M":
        return case.jacobi
    if fault == "gamma_unconj":
        return case.pair
    return True


def _first_cycle(fault, case):
    if fault == "y_unscaled" and case.with_x0:
        return 1                                      # ||b - A x0|| is 2.3, not 1: the scaling by beta acts at once
    if fault == "gamma_unconj" and case.with_x0:
        return 1                                      # b - A x0 is complex: c^T r is not the conjugate of the (real) gamma
    return gs.FIRST_ACTS[fault]


@needs_extended
@pytest.mark.parametrize("fault", [f for f in gs.FAULTS if f != "gamma_real"])
def test_planted_fault_exceeds_its_bound_at_the_first_cycle_it_acts_and_not_before(fault):
    """Per cycle the larger of (deviation / 8 D) and (invariant / 8 INV): at most 1 before the fault acts, above 1 at the
    first cycle it acts (recycling faults from cycle 2, the truncation fault from cycle 4) on every case read that far;
    ``no_final_M`` leaves every cycle alone and breaks the final ``x = M u``."""
    seen = 0
    for name in FAULT_CASES:
        case = gs.CASES[name]
        if not _applies(fault, case):
            continue
        ref = gs.reference(case)
        run = gs.run_double(case, "dot", fault=fault)
        inv = gs.case_invariants(case, run)
        size = [max(max(gs.deviations(g, r).values()) / case.bound, gs.invariant_excess([i])[0]) for g, r, i in zip(run, ref, inv)]
        final = gs.final_deviation(run.final, ref.final) / case.bound
        first = _first_cycle(fault, case)
        print(f"GCROT-CPU fault {fault} on {name}: per cycle {[f'{s:.3g}' for s in size]}, final {final:.3g}")
        if first is None:
            assert max(size) <= 1.0 and final > 1.0, (fault, name)
            seen += 1
            continue
        assert all(s <= 1.0 for s in size[:first - 1]), (fault, name, size)
        if len(size) >= first and not (case.jacobi and fault == "alpha_cx_only"):
            assert size[first - 1] > 1.0, (fault, name, size)
            seen += 1
    assert seen >= 2, fault


@needs_extended
def test_gamma_is_real_so_dropping_its_imaginary_part_is_no_fault():
    """``cx`` is the normalised projection of ``r`` on ``A [Z, U]``'s new direction (the least-squares problem minimises
    ``||r - V H y||``), so ``gamma = <cx, r> = ||P r||`` is real in exact arithmetic: in the reference its imaginary part
    is rounding (2^-60 of ``||r||``), and a run that drops it (``gamma_real``) stays within D at every cycle.  A wrong
    sign on the imaginary half of the conjugated product is therefore invisible to ANY check of a solve; it is caught
    where the operands are general, in the primitive checks."""
    for name in ("g1037 pair sign=+1", "g20001 pair", "g1037 pair x0"):
        case = gs.CASES[name]
        ref = gs.reference(case)
        for rec in ref:
            assert abs(float(rec["gamma"].imag)) <= 2.0 ** -60 * float(rec["r0"])
        run = gs.run_double(case, "dot", fault="gamma_real")
        assert all(max(gs.deviations(g, r).values()) <= gs.D for g, r in zip(run, ref))


# ---------------------------------------------------------------- exits
@needs_extended
@pytest.mark.parametrize("name", list(gs.EXITS))
def test_exits_have_a_margin_of_two_in_every_arithmetic(name):
    """Every decision of the solve is a factor of 2 from its threshold in ``longdouble`` and in every float64 order, all of
    them end alike, and the project's generator on the NumPy provider gives the same ``info``, cycles and product count."""
    e = gs.EXITS[name]
    ariths = [gs.Wide(e.pair)] + [gs.Double(o, e.pair) for o in gs.ORDERS]
    if e.raises is not None:
        for arith in ariths:
            with pytest.raises(e.raises, match="finite"):
                e.run(arith)
        with pytest.raises(e.raises, match="finite"):
            e.project(ariths[1])
        return
    ref = e.run(ariths[0])
    for arith in ariths:
        run = e.run(arith)
        margin = gs.exit_margin(run)
        print(f"GCROT-CPU exit {name} [{arith.name}]: info {run.info}, {len(run)} cycles, {run.products} products, margin {margin:.3g}")
        assert margin >= 2.0
        assert (run.info, run.outer, run.products, len(run)) == (ref.info, ref.outer, ref.products, len(ref))
        assert [rec["inner"] for rec in run] == [rec["inner"] for rec in ref]
        if arith is not ariths[0]:
            p = e.project(arith)
            assert (p.info, p.outer, p.products, len(p)) == (ref.info, ref.outer, ref.products, len(ref))
            assert gs.final_deviation(p.final, ref.final) <= gs.D if np.any(ref.final) else not np.any(p.final)
    expect = {"converges in cycle 3": (0, 3, 13), "maxiter": (2, 2, 9), "zero rhs": (0, 0, 0), "eigenvector": (0, 1, 2), "exact x0": (0, 0, 1)}
    assert (ref.info, len(ref), ref.products) == expect[name.rsplit(" ", 1)[0]]


# ---------------------------------------------------------------- the primitive bounds' two conditions
def _consts(n):
    return gs.grids(n, CUS)


def _pair_dot_emu(a, b, n, fault=None):
    import test_gpu_subspace_kernels as sk
    G = sk._grid_records(n, CUS)
    ar, ai, br, bi = a.real.copy(), a.imag.copy(), b.real.copy(), b.imag.copy()
    skip = fault == "odd tail"
    p = [_emu_dot(ar, br, G), _emu_dot(ai, br, G, skip_tail=skip)]
    q = [_emu_dot(ar, bi, G), _emu_dot(ai, bi, G, skip_tail=skip)]
    if fault == "not conjugated":
        return complex(p[0] - q[1], q[0] + p[1])
    return complex(p[0] + q[1], q[0] - p[1])


@needs_extended
@pytest.mark.parametrize("n", gs.LENGTHS)
def test_reduction_bounds_hold_four_times_over_and_seeded_faults_exceed_them(n):
    """Pair ``dot`` and ``nrm2`` (the real ones: ``test_hiprec_cpu.py``): the float64 emulation of the kernels' trees under
    a quarter; the unconjugated product, a skipped odd tail and a norm without its imaginary half above the bound."""
    import test_gpu_subspace_kernels as sk
    cdot, crec = _consts(n)
    G = sk._grid_records(n, CUS)
    a, b = gs.vectors(n, 2)
    got = _pair_dot_emu(a, b, n)
    assert max(gs.check_call("dot", (a, b), got, True, cdot, crec).values()) <= 0.25
    assert max(gs.check_call("dot", (a, b), _pair_dot_emu(a, b, n, "not conjugated"), True, cdot, crec).values()) > 1
    if n & 1 and n > 1:
        assert max(gs.check_call("dot", (a, b), _pair_dot_emu(a, b, n, "odd tail"), True, cdot, crec).values()) > 1
    re2, im2 = _emu_dot(a.real.copy(), a.real.copy(), G, final="threads"), _emu_dot(a.imag.copy(), a.imag.copy(), G, final="threads")
    assert gs.check_call("nrm2", (a,), math.sqrt(re2 + im2), True, cdot, crec)["pair nrm2"] <= 0.25
    assert gs.check_call("nrm2", (a,), math.sqrt(re2), True, cdot, crec)["pair nrm2"] > 1
    x = a.real.copy()
    assert gs.check_call("nrm2", (x,), math.sqrt(_emu_dot(x, x, G, final="threads")), False, cdot, crec)["nrm2"] <= 0.25
    assert gs.check_call("dot", (x, b.real.copy()), _emu_dot(x, b.real.copy(), G, final="threads"), False, cdot, crec)["dot"] <= 0.25


def _axpy_emu(alpha, x, y, fused, fault=None):
    """``_PairOps.axpy`` / ``_Ops.axpy`` as one or two ``hipeig_axpby`` per half; y None: ``scaled``."""
    def upd(a, xv, yv):
        return _fma(a, xv, yv) if fused else a * xv + yv
    alpha = complex(alpha)
    if not np.iscomplexobj(x):
        return upd(alpha.real, x, y)
    re = alpha.real * x.real if y is None else upd(alpha.real, x.real, y.real)
    im = alpha.real * x.imag if y is None else upd(alpha.real, x.imag, y.imag)
    if alpha.imag != 0.0:
        re = upd(alpha.imag if fault == "sign" else -alpha.imag, x.imag, re)
        im = upd(alpha.imag, x.real, im)
    return re + 1j * im


@needs_extended
@pytest.mark.parametrize("n", gs.LENGTHS)
def test_update_bounds_hold_for_fused_and_unfused_forms_and_seeded_faults_exceed_them(n):
    """``axpy``, complex ``axpy`` and ``scaled`` / ``scal`` for every scalar of the device test: the fused and the unfused
    float64 form under the bound (these are worst cases of one or two roundings, of which a correct evaluation can use
    half - the module docstring - so the margin of four does not exist here and is not asked); a wrong sign on the
    ``-ai x_im`` term, a skipped odd tail and a float32 scalar above it; real scalars bit for bit."""
    cdot, crec = _consts(n)
    x, y = gs.vectors(n, 2, seed=31)
    worst = 0.0
    for alpha in gs.SCALARS:
        cplx = complex(alpha).imag != 0.0
        for fused in (False, True):
            got = _axpy_emu(alpha, x, y, fused)
            worst = max(worst, max(gs.check_call("axpy", (alpha, x, y), got, True, cdot, crec).values()))
            if cplx:
                got = _axpy_emu(alpha, x, None, fused)
                for name in ("scaled", "scal"):
                    worst = max(worst, max(gs.check_call(name, (alpha, x), got, True, cdot, crec).values()))
            else:
                a = complex(alpha).real
                got = _axpy_emu(a, x.real.copy(), y.real.copy(), fused)
                worst = max(worst, gs.check_call("axpy", (a, x.real.copy(), y.real.copy()), got, False, cdot, crec)["axpy"])
        if cplx:
            assert max(gs.check_call("axpy", (alpha, x, y), _axpy_emu(alpha, x, y, True, "sign"), True, cdot, crec).values()) > 1
            assert max(gs.check_call("scaled", (alpha, x), _axpy_emu(alpha, x, None, True, "sign"), True, cdot, crec).values()) > 1
        else:
            a = complex(alpha).real
            assert gs.check_call("scaled", (alpha, x), a * x, True, cdot, crec)["scaled real scalar"] == 0.0
            assert gs.check_call("scal", (a, x.real.copy()), a * x.real, False, cdot, crec)["scal real scalar"] == 0.0
            bad = x / (1.0 / a) if a else x * 0.0 + 1e-300   # a division by the reciprocal is not the product
            if np.any(bad != a * x):
                assert gs.check_call("scaled", (alpha, x), bad, True, cdot, crec)["scaled real scalar"] == math.inf
        if complex(alpha) != 0:
            a32 = complex(np.complex64(alpha))
            if a32 != complex(alpha):
                assert max(gs.check_call("axpy", (alpha, x, y), _axpy_emu(a32, x, y, True), True, cdot, crec).values()) > 1
            if n & 1:
                bad = _axpy_emu(alpha, x, y, True)
                bad[-1] = y[-1]
                assert max(gs.check_call("axpy", (alpha, x, y), bad, True, cdot, crec).values()) > 1
    assert worst <= 1.0
    copy = x.copy()
    assert gs.check_call("copy", (x,), copy, True, cdot, crec)["copy"] == 0.0
    copy[n // 2] = np.nextafter(copy[n // 2].real, np.inf) + 1j * copy[n // 2].imag
    assert gs.check_call("copy", (x,), copy, True, cdot, crec)["copy"] == math.inf
    assert gs.check_call("zeros", (), np.zeros(n, dtype=complex), True, cdot, crec)["zeros"] == 0.0
    assert gs.check_call("zeros", (), -np.zeros(n), False, cdot, crec)["zeros"] == math.inf


@needs_extended
@pytest.mark.parametrize("n", [1, 3, 65, 1037])
def test_combine_bound_holds_four_times_over_and_the_chunk_fault_exceeds_it(n):
    """``_PairOps.combine`` over k' complex vectors is ``hipeig_lincomb`` over 2 k' real inputs (the 16-input chunks
    accumulate into the output): the float64 run under a quarter of ``c_lin(2 k')``; a second chunk that overwrites (live
    from k' = 9) and a coefficient table whose imaginary half lost its sign above it.  Real vectors: the same counts."""
    cdot, crec = _consts(n)
    for k in gs.COMBINE_COUNTS:
        V, cf = gs.vectors(n, k), gs.coefficients(k)
        parts = np.array([v.real for v in V] + [v.imag for v in V])
        c_re, c_im = np.concatenate([cf.real, -cf.imag]), np.concatenate([cf.imag, cf.real])
        got = _emu_lincomb(parts, c_re) + 1j * _emu_lincomb(parts, c_im)
        assert max(gs.check_call("combine", (cf, list(V)), got, True, cdot, crec).values()) <= 0.25, k
        bad = _emu_lincomb(parts, np.concatenate([cf.real, cf.imag])) + 1j * _emu_lincomb(parts, c_im)
        assert gs.check_call("combine", (cf, list(V)), bad, True, cdot, crec)["pair combine re"] > 1, k
        if 2 * k > 16:
            bad = _emu_lincomb(parts, c_re, "second chunk overwrites") + 1j * _emu_lincomb(parts, c_im)
            assert gs.check_call("combine", (cf, list(V)), bad, True, cdot, crec)["pair combine re"] > 1, k
        R = [v.real.copy() for v in V]
        got = _emu_lincomb(np.array(R), cf.real)
        assert gs.check_call("combine", (cf.real, R), got, False, cdot, crec)["combine"] <= 0.25, k
        if k > 16:
            bad = _emu_lincomb(np.array(R), cf.real, "second chunk overwrites")
            assert gs.check_call("combine", (cf.real, R), bad, False, cdot, crec)["combine"] > 1, k


def test_the_log_of_a_float64_run_passes_the_primitive_checks():
    """The NumPy provider's own calls - the log a device run's proxy records in the same form - pass ``check_log`` (its
    sums are NumPy's, not the kernels' trees: held to the bound, not to a quarter), and ``cycle_records`` cuts the log into
    the cycles the restated recurrence counts."""
    if not hp.EXTENDED:
        pytest.skip("longdouble is no wider than double on this machine")
    for name in ("g65 real", "g65 pair", "g1037 pair x0"):
        case = gs.CASES[name]
        run = gs.run_double(case, "dot")
        assert len(run) == case.ncycles
        worst = gs.check_log(run.log, case.pair, *_consts(case.op.n))
        assert worst and max(r for r, _ in worst.values()) <= 1.0, worst
        assert "copy" in worst and ("pair combine re" if case.pair else "combine") in worst
