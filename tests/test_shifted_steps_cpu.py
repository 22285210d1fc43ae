"""The reference of the shifted-MINRES step tests checked without a GPU (``_shifted_steps.py``): its ``longdouble`` run
against true residuals and a dense solve, the NumPy twin against it, the measured deviation ``D``, the planted faults and
the margins of the stop cases."""
import numpy as np
import pytest

import _hiprec as hp
import _shifted_steps as ss
from eigensolvers_amd.shifted_minres import shifted_minres_host

pytestmark = pytest.mark.skipif(not hp.EXTENDED, reason="longdouble is no wider than double on this machine")

# MINRES's |tau| IS the residual norm of its iterate; the longdouble run's own error is 2^-64 times a small factor, four
# orders below this
REFERENCE_TOL = 1e-15
ALL_CASES = list(ss.CASES.values()) + list(ss.STOPS.values())


def _true_residual(case, z, x):
    """``||b - sign (z x - H x)||`` in ``longdouble``."""
    op = case.op
    xw = np.asarray(x).astype(hp.CLD)
    Hx = hp.csr_matvec(op.rowptr, op.col, op.val, xw)[0]
    r = case.b.astype(ss.LD) - ss.LD(case.sign) * (hp.CLD(z) * xw - Hx)
    return hp.nrm2(r)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_reference_tau_is_the_true_residual(case):
    """Independently of the twin: at every step the reference's ``|tau_j|`` equals the residual norm of its iterate to
    1e-15 relative (at ``k == n``, where both are rounding residue, relative to ``beta1``).  A stop case is checked up to
    each shift's stop step, the steps the device tests read: beyond it ``|tau|`` falls to 1e-10 and below, where the
    rounding of the residual itself, 2^-64 ||b||, is no longer 1e-15 of it."""
    ref = ss.reference(case)
    worst = 0.0
    for k, rec in enumerate(ref, start=1):
        scale = case.tau_scale(k)
        for j, z in enumerate(case.shifts):
            if case.expect is not None and case.expect[j] is not None and k > case.expect[j]:
                continue
            res = _true_residual(case, z, rec["x"][j])
            rel = float(abs(res - rec["abstau"][j]) / (rec["abstau"][j] if scale is None else scale))
            worst = max(worst, rel)
            assert rel <= REFERENCE_TOL, (case.name, k, z, float(res), float(rec["abstau"][j]))
    print(f"STEPS-CPU {case.name}: | ||r|| - |tau| | / |tau| <= {worst:.2e}")


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_reference_is_the_dense_solve_at_step_n(sign):
    """n = 2: the Krylov space is the whole space at step 2, so ``x_2`` is the solution of the 2 x 2 system."""
    case = ss.CASES[f"dense2 sign={sign:+.0f}"]
    M = case.op.A.toarray().astype(hp.CLD)
    b = case.b.astype(hp.CLD)
    for j, z in enumerate(case.shifts):
        A = hp.CLD(sign) * (hp.CLD(z) * np.eye(2, dtype=hp.CLD) - M)
        det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
        x = np.array([A[1, 1] * b[0] - A[0, 1] * b[1], A[0, 0] * b[1] - A[1, 0] * b[0]]) / det
        assert ss.x_deviation(ss.reference(case)[1]["x"][j], x) * ss.U <= REFERENCE_TOL, (z, sign)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_twin_agrees_with_the_reference_step_by_step(case):
    """``shifted_minres_host`` with no tolerance and ``maxiter = k`` is step k: ``its == k``, ``x`` and ``estimates``
    within ``D`` of the reference."""
    A = case.op.A
    ref = ss.reference(case)
    worst = {"x": 0.0, "tau": 0.0}
    for k in range(1, case.nsteps + 1):
        x, its, est, conv = shifted_minres_host(lambda v: A @ v, case.b, case.shifts, 0.0, 0.0, k, case.sign)
        assert list(its) == [k] * len(case.shifts)
        dev = ss.step_deviations(case, k, x, est, ref)
        for q, d in dev.items():
            worst[q] = max(worst[q], d)
        assert max(dev.values()) <= ss.D, (case.name, k, dev)
    print(f"STEPS-CPU twin {case.name}: x {worst['x']:.2f} u, |tau| {worst['tau']:.2f} u (D = {ss.D:g})")


def test_no_summation_order_deviates_by_more_than_D():
    Dm, table = ss.measured_deviation()
    worst = {}
    for (name, k, order), (d, q) in table.items():
        if d > worst.get(name, (0.0,))[0]:
            worst[name] = (d, k, order, q)
    for name, (d, k, order, q) in worst.items():
        print(f"STEPS-CPU {name}: {d:.2f} u ({q}, step {k}, {order})")
    print(f"STEPS-CPU D measured {Dm:.2f} u, constant {ss.D}")
    assert ss.D <= 16.0
    assert Dm <= ss.D
    assert Dm >= 0.5 * ss.D                           # the constant is the measurement, not a loose cover of it
    assert ss.BOUND == ss.FACTOR * ss.D and ss.FACTOR == 8


@pytest.mark.parametrize("fault", ss.FAULTS)
def test_planted_fault_exceeds_8D(fault):
    """Every one-line fault is past ``8 D`` at a step <= K on some case - and on the g1037 and g20001 cases the device
    tests run (both odd, so the tail faults bear on them too)."""
    seen = {}
    for case in ss.CASES.values():
        if fault in ss.ODD_ONLY and not case.op.n & 1:
            continue
        ref = ss.reference(case)
        for k, g in enumerate(ss.run_double(case, "dot", fault=fault), start=1):
            dev = ss.step_deviations(case, k, g["x"], g["abstau"], ref)
            q = max(dev, key=dev.get)
            if dev[q] > seen.get(case.name, (0.0,))[0]:
                seen[case.name] = (dev[q], k, q)
    caught = {name: v for name, v in seen.items() if v[0] > ss.BOUND}
    best = max(seen, key=lambda name: seen[name][0])
    print(f"STEPS-CPU fault {fault}: caught on {len(caught)} of {len(seen)} cases; largest {seen[best][0]:.3g} u "
          f"({seen[best][2]}, step {seen[best][1]}, {best})")
    assert caught, seen
    for name in ("g1037 sign=+1", "g1037 sign=-1", "g20001 sign=+1"):
        assert name in caught, (fault, name, seen[name])


@pytest.mark.parametrize("fault", ss.UNOBSERVABLE)
def test_imaginary_part_of_d_carries_nothing(fault):
    """Why the wrong signs in ``Im d`` are not among ``FAULTS``: the triangular factor of ``sign (z I - T)`` is real, so
    ``r1i`` and ``Im d`` are rounding residue.  In the float64 form each of them moves an iterate by less than 1 u of its norm
    and no ``|tau|`` at all - below what the summation orders differ by, so no bound that a correct kernel meets can see it."""
    worst = 0.0
    for name in ("g65 sign=+1", "g1037 sign=-1", "g20001 sign=+1"):
        case = ss.CASES[name]
        for g, r in zip(ss.run_double(case, "dot", fault=fault), ss.run_double(case, "dot")):
            assert np.array_equal(g["abstau"], r["abstau"])
            worst = max(worst, max(ss.x_deviation(g["x"][j], r["x"][j]) for j in range(len(case.shifts))))
    print(f"STEPS-CPU {fault}: moves x by {worst:.3f} u at most")
    assert worst < 1.0


@pytest.mark.parametrize("name", list(ss.STOPS))
def test_stop_case_has_its_margin(name):
    """Under ``longdouble`` and every float64 summation order each shift stops at its expected step - or not at all - with
    ``|tau|`` a factor >= 2 from the target at every step that decides."""
    case = ss.STOPS[name]
    for arith in [ss.Wide] + [ss.Double(order) for order in ss.ORDERS]:
        margin, stops = ss.stop_margin(case, arith)
        line = f"STEPS-CPU stops {name} [{arith.name}]: stop steps {stops}, least margin {margin:.3g}"
        assert stops == case.expect, line
        assert margin >= 2.0, line
        print(line)
    stopped = [e for e in case.expect if e is not None]
    if name == "mixed":
        assert len(set(stopped)) >= 2 and max(stopped) <= 4 and None in case.expect
    else:
        assert len(stopped) == 8 and max(stopped) <= 5


@pytest.mark.parametrize("name", list(ss.STOPS))
def test_twin_stops_where_the_case_says(name):
    case = ss.STOPS[name]
    A = case.op.A
    ref = ss.reference(case)
    x, its, est, conv = shifted_minres_host(lambda v: A @ v, case.b, case.shifts, 0.0, case.target, ss.K, case.sign)
    assert list(its) == [ss.K if e is None else e for e in case.expect]
    assert list(conv) == [e is not None for e in case.expect]
    for j, k in enumerate(its):                       # frozen at its stop step: not step k + 1
        assert ss.x_deviation(x[j], ref[k - 1]["x"][j]) <= ss.D
        assert ss.tau_deviation(est[j], ref[k - 1]["abstau"][j]) <= ss.D


def test_measures():
    a = np.array([1.0 + 2.0j, -3.0j])
    assert ss.x_deviation(a, a) == 0.0
    b = a.copy()
    b[1] = complex(0.0, np.nextafter(-3.0, 0.0))      # one ulp of 3 = 2^-51: 4 u / ||a||
    assert abs(ss.x_deviation(b, a) - 4.0 / np.linalg.norm(a)) < 1e-6
    assert ss.x_deviation(np.array([1.0, complex(0.0, np.nan)]), np.array([1.0, 1.0])) == float("inf")
    assert ss.tau_deviation(1.0 + 2.0 ** -52, 1.0) == 2.0
    assert ss.tau_deviation(2.0 ** -52, 0.0, scale=2.0) == 1.0
    assert ss.tau_deviation(float("nan"), 1.0) == float("inf")
