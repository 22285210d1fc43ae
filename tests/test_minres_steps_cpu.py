"""The reference of the MINRES step tests checked without a GPU (``_minres_steps.py``): its float64 form against the
oracle, the NumPy twin and SciPy; the measured deviations ``D`` and ``D_LONG``; the planted faults; the margins of the exit
cases."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _hiprec as hp
import _minres_steps as ms
from eigensolvers_amd.precond_minres import csr_diagonal_host, jacobi_inverse_host, minres_jacobi_host
from oracle.minres_ref import minres as minres_ref

needs_extended = pytest.mark.skipif(not hp.EXTENDED, reason="longdouble is no wider than double on this machine")
TRACED = ("alfa", "beta", "rnorm", "ynorm", "Anorm", "test1", "test2")


def _matvec(case):
    A = case.op.A
    return lambda v: case.sign * (case.sigma * v - A @ v)


@pytest.mark.parametrize("name", ["g1037 sigma=0.02 sign=+1", "g1037 sigma=0.02 sign=-1", "g1037 sigma=0.0 sign=-1", "g65",
                                  "g20001", "g1037 column 1", "g1037 jacobi", "g20001 jacobi", "g1037 column 3 jacobi"])
def test_float64_form_is_the_oracle_and_the_twin_bit_for_bit(name):
    """``steps`` in float64 with ``np.dot`` evaluates the expressions of ``oracle/minres_ref.py`` (with ``minv`` those of
    ``minres_jacobi_host``) in their order, so ``x_k`` and every traced scalar are the same bits for k = 1 .. K."""
    case = ms.CASES[name]
    mine = ms.run_double(case, "dot")
    for k in range(1, case.nsteps + 1):
        trace = []
        if case.jacobi:
            x, info, itn, istop = minres_jacobi_host(_matvec(case), case.b, case.minv, rtol=0.0, maxiter=k, trace=trace)
        else:
            x, info, itn, istop = minres_ref(_matvec(case), case.b, rtol=0.0, maxiter=k, trace=trace)
        assert (itn, istop, info) == (k, 6, k)
        np.testing.assert_array_equal(x, mine[k - 1]["x"])
        for q in TRACED:
            assert trace[-1][q] == float(mine[k - 1][q]), (k, q)


@pytest.mark.parametrize("name", ["g1037 x0", "g20001 x0", "g1037 jacobi", "g20001 jacobi", "g1037 column 9 jacobi", "g1037 column 2"])
def test_float64_form_agrees_with_scipy(name):
    """``scipy.sparse.linalg.minres(A, b, x0=..., M=..., rtol=0, maxiter=k)`` within 4 u in the module's measure.  Not
    bit for bit: SciPy applies ``A`` and ``M`` through ``LinearOperator`` products and subtracts its (zero) shift, an order
    of evaluation that is its own."""
    case = ms.CASES[name]
    n = case.op.n
    A = spla.LinearOperator((n, n), matvec=_matvec(case), dtype=np.float64)
    M = None if case.minv is None else sp.diags(case.minv)
    mine = ms.run_double(case, "dot")
    for k in range(1, case.nsteps + 1):
        x, info = spla.minres(A, case.b, x0=None if case.x0 is None else case.x0.copy(), M=M, rtol=0.0, maxiter=k)
        assert info == k
        dev = ms.deviation(x, mine[k - 1]["x"])
        assert dev <= 4.0, (name, k, dev)
        if case.x0 is not None:                      # and the part the steps added, so that x0 cannot carry the agreement
            assert ms.deviation(x - case.x0, mine[k - 1]["x"] - case.x0) <= 4.0 * np.linalg.norm(x) / np.linalg.norm(x - case.x0)


@needs_extended
def test_no_summation_order_deviates_by_more_than_D():
    """``D``: the largest deviation of the four float64 orders from the ``longdouble`` run over the whole table, the
    iterate and the five scalar statistics; ``Acond`` (1 at step 1, a quotient of two gammas after) obeys it too."""
    Dm, table = ms.measured_deviation(stats=ms.STATS)
    worst = {}
    for (name, k, order), (d, q) in table.items():
        if d > worst.get(name, (0.0,))[0]:
            worst[name] = (d, k, order, q)
    for name, (d, k, order, q) in worst.items():
        print(f"STEPS-CPU {name}: {d:.2f} u ({q}, step {k}, {order})")
    print(f"STEPS-CPU D measured {Dm:.2f} u, constant {ms.D}")
    assert ms.D <= 16.0
    assert Dm <= ms.D
    assert Dm >= 0.5 * ms.D                           # the constant is the measurement, not a loose cover of it


@needs_extended
def test_the_scaled_column_deviates_as_an_unscaled_one():
    """Deviations are relative: the column the block tests scale by 1e-7 stays under D like every other."""
    case = ms.CASES[f"g1037 column {ms.SCALED_COLUMN}"]
    assert np.linalg.norm(case.b) < 1e-6
    ref = ms.reference(case)
    for order in ms.ORDERS:
        for g, r in zip(ms.run_double(case, order), ref):
            assert max(ms.step_deviations(g, r).values()) <= ms.D


def _applies(fault, case):
    return not ((fault == "z_prev" and not case.jacobi) or (fault == "ynorm_no_x0" and not case.with_x0)
                or (fault == "kc_tail" and not case.op.n & 1))


@needs_extended
@pytest.mark.parametrize("fault", ms.K_FAULTS)
def test_planted_fault_exceeds_8D(fault):
    """Every one-line fault is past ``8 D`` in some quantity at a step <= K on some case - and, for the faults that bear
    on a device configuration, on the case that configuration runs."""
    seen = {}
    for case in ms.CASES.values():
        if not _applies(fault, case):
            continue
        ref = ms.reference(case)
        for k, (g, r) in enumerate(zip(ms.run_double(case, "dot", fault=fault), ref), start=1):
            dev = ms.step_deviations(g, r, ms.STATS, case.scales(k, ref))
            q = max(dev, key=dev.get)
            if dev[q] > seen.get(case.name, (0.0,))[0]:
                seen[case.name] = (dev[q], k, q)
    caught = {name: v for name, v in seen.items() if v[0] > ms.FACTOR * ms.D}
    best = max(seen, key=lambda name: seen[name][0])
    print(f"STEPS-CPU fault {fault}: caught on {len(caught)} of {len(seen)} cases; largest {seen[best][0]:.3g} u "
          f"({seen[best][2]}, step {seen[best][1]}, {best})")
    assert caught, seen
    for name in ("g1037 sigma=0.02 sign=+1", "g20001", "g1037 jacobi", "g1037 x0"):
        if name in seen:
            assert name in caught, (fault, name, seen[name])


@needs_extended
def test_no_summation_order_deviates_by_more_than_D_LONG_at_the_long_steps():
    """``D_LONG``: ``D``'s definition over ``LONG_CASES`` and ``LONG_STEPS``, the four orders joined by the rank-ordered
    slab sums of 2 and 3 ranks; ``Acond`` obeys it too."""
    Dm, table = ms.measured_long_deviation(stats=ms.STATS)
    worst = {}
    for (name, k, order), (d, q) in table.items():
        if d > worst.get(name, (0.0,))[0]:
            worst[name] = (d, k, order, q)
    for name, (d, k, order, q) in worst.items():
        print(f"STEPS-CPU long {name}: {d:.2f} u ({q}, step {k}, {order})")
    print(f"STEPS-CPU D_LONG measured {Dm:.2f} u, constant {ms.D_LONG}")
    assert {k for _, k, _ in table} == set(ms.LONG_STEPS) and {n for n, _, _ in table} == set(ms.LONG_CASES)
    assert Dm <= ms.D_LONG <= 32.0


def test_slab_order_adds_the_ranks_sums_in_rank_order():
    x = ms.rhs(1037)
    y = ms.rhs(1037, 5)
    for P in (2, 3):
        acc = 0.0
        for r in range(P):
            lo, hi = ms.row_range(1037, P, r)
            acc += float(np.dot(x[lo:hi], y[lo:hi]))
        assert float(ms.Double("slabs", P).dot(x, y)) == acc
    assert [ms.row_range(1037, 3, r) for r in range(3)] == [(0, 346), (346, 692), (692, 1037)]
    assert float(ms.Double("slabs", 1).dot(x, y)) == float(np.dot(x, y))


@needs_extended
@pytest.mark.parametrize("fault", ms.LONG_FAULTS)
def test_planted_long_fault_exceeds_8_D_LONG(fault):
    """The faults of the row-partitioned path are past ``8 D_LONG`` at a step of ``LONG_STEPS`` on the case the group tests
    run; a lost update at the chunk boundary and a missing share at step 17 stay within ``8 D`` over steps 1 .. 4 - four
    steps cannot see them."""
    case = ms.CASES["g1037 sigma=0.02 sign=+1"]
    last = ms.LONG_STEPS[-1]
    ref = ms.reference(case, nsteps=last)
    got = ms.run_double(case, "dot", fault=fault, nsteps=last)
    dev = {k: max(ms.step_deviations(got[k - 1], ref[k - 1], ms.STATS).values()) for k in ms.LONG_STEPS}
    print(f"STEPS-CPU long fault {fault}: " + ", ".join(f"step {k}: {d:.3g} u" for k, d in dev.items()))
    assert any(d > ms.step_bound(k) for k, d in dev.items() if k > ms.K), dev
    if fault in ("kd_dropped_at_16", "yy_share_missing"):
        assert all(dev[k] <= ms.FACTOR * ms.D for k in range(1, ms.K + 1)), dev
    for k in ms.LONG_STEPS:
        assert ms.step_bound(k) == ms.FACTOR * (ms.D if k <= ms.K else ms.D_LONG)


def _twin_minv(e):
    return jacobi_inverse_host(csr_diagonal_host(e.H), e.sigma)


@pytest.mark.parametrize("name", list(ms.EXITS))
def test_exit_case_has_its_margin(name):
    """The oracle ends with the intended ``(itn, istop)`` under every summation order of its inner products; the deciding
    quantity is past its threshold by a factor >= 2 at the stop and short of it by >= 2 at every step before; a competing
    test that would overwrite the code is short of its threshold by >= 2 at the stop."""
    e = ms.EXITS[name]
    for order in ms.ORDERS:
        x, itn, istop, trace = ms.full_trace(e.matvec, e.b, e.rtol, e.maxiter, order=order)
        at_stop, before = ms.exit_margin(trace, e.decides)
        line = (f"STEPS-CPU exit {name} [{order}]: (itn, istop) = ({itn}, {istop}), {e.decides} past its threshold by "
                f"{at_stop:.3g}, short of it before by {before:.3g}")
        assert (itn, istop) == e.expect, line
        assert np.isfinite(x).all()
        assert at_stop >= 2.0 and before >= 2.0, line
        if name in ms.COMPETES:
            other, _ = ms.exit_margin(trace, ms.COMPETES[name])
            line += f", {ms.COMPETES[name]} short of its threshold by {1 / other:.3g}"
            assert other <= 0.5, line
        print(line)


def test_eigenvector_exit_in_the_preconditioned_twin():
    e = ms.EXITS["eigenvector n=64"]
    x, itn, istop, trace = ms.full_trace(e.matvec, e.b, e.rtol, e.maxiter, minv=_twin_minv(e))
    at_stop, before = ms.exit_margin(trace, "ratio")
    assert (itn, istop) == (1, -1) and at_stop >= 2.0
    j = int(np.flatnonzero(e.b)[0])
    assert np.count_nonzero(x) == 1
    assert ms.deviation(x[j], e.sign * e.b[j] / (ms.LD(e.sigma) - ms.LD(e.H.diagonal()[j]))) <= 4.0


def test_deviation_measure():
    a = np.array([1.0, 2.0, -3.0])
    assert ms.deviation(a, a) == 0.0
    assert ms.deviation(np.float64(1.0) + 2.0 ** -52, 1.0) == 2.0
    assert ms.deviation(np.array([1.0, np.nan]), np.array([1.0, 1.0])) == float("inf")
    assert ms.deviation(float("inf"), 1.0) == float("inf")
    b = a.copy()
    b[2] = np.nextafter(b[2], 0.0)                    # one ulp of 3 = 2^-51: 4 u / ||a||
    assert abs(ms.deviation(b, a) - 4.0 / np.linalg.norm(a)) < 1e-6
