"""Shifted MINRES on the device (``csrc/minres_shifts.hip`` behind ``eigensolvers_amd.solve_shifts``,
``HipVector.solve(linearSolver="minres_shifted")`` and FEAST's vector-major path) against the NumPy twin
``shifted_minres_host`` and against true residuals formed on the host with SciPy's product.

Every case fails without the feature: the solver name raises and ``solve_shifts`` does not exist.

Device against twin: the Lanczos recurrence amplifies rounding differences, so solutions are compared through their
residuals only, and the per-shift step counts may differ by a few: ``|device - twin| <= max(3, 2 * largest difference
observed)``.  The differences are printed (``STEPS ...`` lines under ``-s``); EXPERIMENTS.md R8-shifted holds what has been
observed: 0 on every case on an MI355X, so the bound is the rule's floor, 3 steps."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from _sweep_cases import (CONTOUR, EPS, REAL_SHIFT, SHIFT_SETS, check_residuals, residual_bound, shifted_options as options,
                          true_residual)
from conftest import load_golden
from eigensolvers_amd.generators import gapped_csr_host, gapped_params
from eigensolvers_amd.shifted_minres import shifted_minres_host

pytestmark = pytest.mark.gpu

TOLS = [(1e-5, 1e-7), (1e-10, 1e-12)]
STEP_DIFFERENCE_BOUND = 3          # max(3, 2 * largest difference observed), see the module docstring


def odd_operator():
    """n = 1037 (no tile, wave or vector width divides it): a random sparse symmetric matrix plus a diagonal of the
    generator's kind - +-(1..3) except 8 rows inside the contour's window - so that, as for the generated operators, the
    solves end well before n steps (a Lanczos run far beyond n steps counts its steps by its rounding errors)."""
    n = 1037
    rng = np.random.default_rng(5)
    R = sp.random(n, n, density=0.01, random_state=rng, format="csr")
    d = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 3.0, n)
    d[::130] = np.linspace(-0.2, 0.2, len(d[::130]))
    return (0.05 * (R + R.T) + sp.diags(d)).tocsr()


def host_operator(name):
    if name == "n100":
        return sp.csr_matrix(np.array(load_golden("feast_n100.npz")["A"], dtype=float))
    if name == "gapped4000":
        return gapped_csr_host(4000, 32, seed=7)
    return odd_operator()


@pytest.fixture(scope="module")
def problems(hip):
    """name -> (host CSR, device operator, host right-hand side), built once."""
    out = {}
    for name in ("n100", "gapped4000", "odd1037"):
        Hh = host_operator(name)
        Hd = hip.HipCsrOperator.generate(4000, 32, seed=7) if name == "gapped4000" else hip.HipCsrOperator.from_scipy(Hh)
        b = np.random.default_rng(9).standard_normal(Hh.shape[0])
        out[name] = (Hh, Hd, b / np.linalg.norm(b))
    return out


_twin_cache = {}


def twin(name, Hh, b, shifts, rtol, atol, sign, maxiter=4000):
    key = (name, tuple(shifts), rtol, atol, sign, maxiter)
    if key not in _twin_cache:
        _twin_cache[key] = shifted_minres_host(lambda v: Hh @ v, b, shifts, rtol, atol, maxiter, sign)
    return _twin_cache[key]


@pytest.mark.parametrize("rtol,atol", TOLS)
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("S", [1, 3, 8, 9])
@pytest.mark.parametrize("name", ["n100", "gapped4000", "odd1037"])
def test_residuals_and_step_counts(hip, problems, name, S, sign, rtol, atol):
    Hh, Hd, b = problems[name]
    shifts = SHIFT_SETS[S]
    bd = hip.HipVector(b.copy(), options(rtol, atol))
    xs = hip.solve_shifts(Hd, bd, shifts, reverseGF=sign < 0)
    assert len(xs) == S and all(isinstance(x, hip.HipComplexVector) for x in xs)
    check_residuals(Hh, b, shifts, xs, sign, rtol, atol)
    st = bd.last_solve_stats
    target = max(atol, rtol)
    assert len(st["iterations"]) == len(st["estimates"]) == S and all(e <= target * (1 + 1e-12) for e in st["estimates"])
    # one Lanczos run per call of the C entry: its products are the slowest shift's steps
    groups = [st["iterations"][i:i + 8] for i in range(0, S, 8)]
    assert st["products"] == sum(max(g) for g in groups)
    _, its, _, conv = twin(name, Hh, b, shifts, rtol, atol, sign)
    assert conv.all()
    diff = [d - t for d, t in zip(st["iterations"], its)]
    print(f"STEPS {name} S={S} sign={sign:+.0f} rtol={rtol:g} twin={list(map(int, its))} device-twin={diff}")
    assert max(abs(d) for d in diff) <= STEP_DIFFERENCE_BOUND, (diff, list(its))
    assert all(d <= np.ceil(1.1 * t) for d, t in zip(st["iterations"], its))     # more than the twin plus 10 % is a finding


@pytest.mark.parametrize("chunk", [None, "1"])
def test_shifts_do_not_see_each_other(hip, problems, monkeypatch, chunk):
    """CSR-stream (fixed add order): shift j of the 8-shift run is bit for bit the run with shift j alone - a stopped
    shift's x stays frozen while the others go on - and neither depends on how many steps the host enqueues between two
    looks at the state record (HIPEIG_MS_CHUNK, default 32)."""
    Hh, Hd, b = problems["gapped4000"]
    monkeypatch.delenv("HIPEIG_MS_CHUNK", raising=False)
    Hd.set_variant(2)
    try:
        bd = hip.HipVector(b.copy(), options(1e-5, 1e-7))
        ref = [(x.re.array, x.im.array) for x in hip.solve_shifts(Hd, bd, CONTOUR)]
        ref_its = list(bd.last_solve_stats["iterations"])
        assert len(set(ref_its)) > 1                        # they do stop at different steps
        if chunk is not None:
            monkeypatch.setenv("HIPEIG_MS_CHUNK", chunk)
            again = hip.solve_shifts(Hd, bd, CONTOUR)
            assert list(bd.last_solve_stats["iterations"]) == ref_its
            for (r, i), x in zip(ref, again):
                assert np.array_equal(r, x.re.array) and np.array_equal(i, x.im.array)
        for j, z in enumerate(CONTOUR):
            one = hip.solve_shifts(Hd, bd, [z])[0]
            assert bd.last_solve_stats["iterations"] == [ref_its[j]]
            assert bd.last_solve_stats["products"] == ref_its[j]
            assert np.array_equal(one.re.array, ref[j][0]) and np.array_equal(one.im.array, ref[j][1])
    finally:
        Hd.set_variant(0)


@pytest.fixture(scope="module")
def large(hip):
    N = 150_000
    Hd = hip.HipCsrOperator.generate(N, 32, seed=7)
    b = np.random.default_rng(11).standard_normal(N)
    return Hd, Hd.to_scipy(), b / np.linalg.norm(b)


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_reduction_paths_and_operator_layouts(hip, large, variant):
    """N = 150000, from the grid rules of ``hipeig_minres_shifts``: the CSR sweeps (variants 1, 2: one workgroup per row
    block of <= 2048 non-zeros, N * 32 / 2048 > 2000 of them) and the second kernel (8 elements per thread, N / 2048 = 74
    workgroups) both exceed one ticket group of 64, so the two-level finish of their reductions runs; the blocked copies
    (variants 3, 4) finish in one group.  Every operator layout feeds the same Lanczos epilogue.  The update pass carries
    no reduction.  The single-workgroup end is the tridiagonal n = 100 case below."""
    Hd, Hh, b = large
    shifts = SHIFT_SETS[3]
    Hd.set_variant(variant)
    try:
        bd = hip.HipVector(b.copy(), options(1e-5, 1e-7))
        xs = hip.solve_shifts(Hd, bd, shifts)
    finally:
        Hd.set_variant(0)
    check_residuals(Hh, b, shifts, xs, 1.0, 1e-5, 1e-7)


def test_single_workgroup(hip):
    """n = 100: the sweep, the second kernel and the update pass are one workgroup each.  A tridiagonal operator with the
    generator's kind of gap: its diagonal is +-(1..1.5) and its off-diagonal 0.1, so by Gershgorin no eigenvalue lies in
    (-0.8, 0.8) and every shift - the real one at 0.5 included - keeps 0.3 or more from the spectrum.  (A shift inside
    the spectrum of so small an operator is a nearly singular system: the twin itself then runs to three times n steps
    and misses the residual bound, which checks nothing of the device.)  The twin ends in 38 to 46 steps here, and the
    device answers to the same step-count rule as in ``test_residuals_and_step_counts``."""
    n = 100
    d = np.concatenate([np.linspace(-1.5, -1.0, n // 2), np.linspace(1.0, 1.5, n - n // 2)])
    Hh = sp.diags([np.full(n - 1, 0.1), d, np.full(n - 1, 0.1)], [-1, 0, 1]).tocsr()
    Hd = hip.HipCsrOperator.from_scipy(Hh)
    b = np.random.default_rng(12).standard_normal(n)
    shifts = CONTOUR + [REAL_SHIFT]
    bd = hip.HipVector(b.copy(), options(1e-10, 1e-12))
    xs = hip.solve_shifts(Hd, bd, shifts)
    check_residuals(Hh, b, shifts, xs, 1.0, 1e-10, 1e-12)
    xt, its, _, conv = twin("tridiagonal100", Hh, b, shifts, 1e-10, 1e-12, 1.0)
    assert conv.all() and max(its) < n // 2                  # the case itself is well posed: the twin ends well before n
    target = max(1e-12, 1e-10 * np.linalg.norm(b))
    assert all(true_residual(Hh, b, z, x, 1.0) <= residual_bound(Hh, z, x, target) for z, x in zip(shifts, xt))
    diff = [dv - t for dv, t in zip(bd.last_solve_stats["iterations"], its)]
    print(f"STEPS tridiagonal100 S=9 sign=+1 rtol=1e-10 twin={list(map(int, its))} device-twin={diff}")
    assert max(abs(dv) for dv in diff) <= STEP_DIFFERENCE_BOUND, (diff, list(its))


def test_breakdown_ends_in_one_step_with_the_exact_answer(hip):
    h = np.linspace(-1.0, 1.0, 64)
    Hd = hip.HipCsrOperator.from_scipy(sp.diags(h).tocsr())
    b = np.zeros(64)
    b[3] = 2.0
    shifts = CONTOUR + [REAL_SHIFT]
    for sign in (1.0, -1.0):
        bd = hip.HipVector(b.copy(), options(1e-10, 1e-12, 100))
        xs = hip.solve_shifts(Hd, bd, shifts, reverseGF=sign < 0)
        assert bd.last_solve_stats["iterations"] == [1] * 9 and bd.last_solve_stats["estimates"] == [0.0] * 9
        for z, x in zip(shifts, xs):
            xa = x.array
            exact = sign * 2.0 / (z - h[3])
            assert np.isfinite(xa).all() and np.count_nonzero(xa) == 1
            assert abs(xa[3] - exact) <= 4 * EPS * abs(exact)


def test_maxiter_raises_and_records_every_shift(hip, problems):
    Hh, Hd, b = problems["gapped4000"]
    bd = hip.HipVector(b.copy(), options(1e-12, 0.0, 5))
    with pytest.raises(UserWarning, match="Iterative solver is not converged"):
        hip.solve_shifts(Hd, bd, CONTOUR + [REAL_SHIFT])
    assert bd.last_solve_stats["iterations"] == [5] * 9
    assert bd.last_solve_stats["products"] == 10            # two calls of the C entry, 5 steps each


def test_zero_right_hand_side(hip, problems):
    Hh, Hd, b = problems["gapped4000"]
    bd = hip.HipVector(np.zeros(4000), options(1e-5, 1e-7))
    xs = hip.solve_shifts(Hd, bd, CONTOUR[:2])
    assert all(not x.array.any() for x in xs) and bd.last_solve_stats["products"] == 0


def test_hipvector_solve_with_the_new_name(hip, problems):
    Hh, Hd, b = problems["gapped4000"]
    for sign in (1.0, -1.0):
        bd = hip.HipVector(b.copy(), options(1e-10, 1e-12))
        x = hip.HipVector.solve(Hd, bd, CONTOUR[3], reverseGF=sign < 0)
        assert isinstance(x, hip.HipComplexVector)
        check_residuals(Hh, b, [CONTOUR[3]], [x], sign, 1e-10, 1e-12)
        assert len(bd.last_solve_stats["iterations"]) == 1
        xr = hip.HipVector.solve(Hd, bd, REAL_SHIFT, reverseGF=sign < 0)      # zi = 0 is a shift like any other
        assert isinstance(xr, hip.HipComplexVector)
        assert not xr.im.array.any()
        check_residuals(Hh, b, [REAL_SHIFT], [xr], sign, 1e-10, 1e-12)
    bd = hip.HipVector(b.copy(), options(1e-5, 1e-7))
    with pytest.raises(NotImplementedError):
        hip.HipVector.solve(Hd, bd, CONTOUR[0], x0=bd)
    with pytest.raises(NotImplementedError):
        hip.HipVector.solve(Hd, bd, REAL_SHIFT, x0=np.ones(4000))
    with pytest.raises(NotImplementedError):
        hip.HipVector.solve(Hd, hip.HipComplexVector(b + 1j * b, options(1e-5, 1e-7)), CONTOUR[0])
    with pytest.raises(NotImplementedError):
        hip.solve_shifts(Hd, hip.HipComplexVector(b + 1j * b, options(1e-5, 1e-7)), CONTOUR[:2])
    # solveBlock with this solver name: one by one, each with its shift
    bs = [hip.HipVector(b.copy(), options(1e-5, 1e-7)) for _ in range(3)]
    sols = hip.HipVector.solveBlock(Hd, bs, CONTOUR[2])
    assert all(isinstance(s, hip.HipComplexVector) for s in sols)
    check_residuals(Hh, b, [CONTOUR[2]] * 3, sols, 1.0, 1e-5, 1e-7)
    # the names the other paths rely on are untouched
    with pytest.raises(NotImplementedError):
        hip.HipVector.solve(Hd, hip.HipVector(b.copy(), {"linearSystemArgs": {"linearSolver": "minres"}}), CONTOUR[0])
    with pytest.raises(Exception, match="other than gcrotmk"):
        hip.HipVector.solve(Hd, hip.HipVector(b.copy(), {"linearSystemArgs": {"linearSolver": "minres_shift"}}), 0.5)


def test_a_context_with_collectives_is_refused(hip, problems):
    Hh, Hd, b = problems["gapped4000"]
    bd = hip.HipVector(b.copy(), options(1e-5, 1e-7))
    ctx = bd.ctx
    saved = ctx._force_collectives
    ctx._force_collectives = True            # what attach_comm records under HIPEIG_FORCE_COLLECTIVES=1
    try:
        assert ctx.collectives
        with pytest.raises(NotImplementedError, match="collectives"):
            hip.solve_shifts(Hd, bd, CONTOUR[:2])
    finally:
        ctx._force_collectives = saved


def test_feast_end_to_end_with_the_shared_lanczos_solver(hip):
    """``test_feast_at_the_reference_comparable_inner_tolerance``'s recipe (config #5 at N = 2e4, rtol 1e-5) and its
    assertions, with the vector-major path: 16 shared-Lanczos solves per FEAST iteration instead of 128 GCROT solves."""
    import scipy.linalg as la
    N, m0 = 20_000, 16
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    Q = la.qr(np.random.default_rng(9).standard_normal((N, m0)), mode="economic")[0]
    o = {"linearSystemArgs": {"linearSolver": "minres_shifted", "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7}}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev, Y, st = hip.feastDiagonalization(H, [hip.HipVector(Q[:, i].copy(), o) for i in range(m0)], 16, "legendre",
                                             -0.21, 0.21, 1e-4, 12, writeOut=False)
    assert st["residual"] < 1e-4 and 2 <= st["outerIter"] <= 10
    inside = np.sort(ev[(ev > -0.21) & (ev < 0.21)])
    targets = np.sort(gapped_params(N, 32, 7)["targets"])
    assert len(inside) == 16 and np.all(np.abs(inside - targets) < 2e-3)
    res = hip.true_residual_norms(H, ev, Y, m0)
    assert np.all(res < 1e-2), res
    rec = st["sharedLanczos"]
    assert len(rec) == st["outerIter"] + 1
    for r in rec:
        assert r["solves"] == 16 and len(r["products"]) == 16
        assert len(r["pairs"]) == len(r["iterations"]) == 128
        assert sorted(map(tuple, r["pairs"])) == [(k, i) for k in range(8) for i in range(16)]
        assert all(p == max(it for (k, i), it in zip(r["pairs"], r["iterations"]) if i == vec)
                   for vec, p in enumerate(r["products"]))
    assert "contourPool" not in st


def test_contour_pool_with_this_solver_is_refused(hip):
    H = hip.HipCsrOperator.generate(4000, 32, seed=7)
    o = options(1e-5, 1e-7)
    Y = [hip.HipVector(np.random.default_rng(i).standard_normal(4000), o) for i in range(2)]
    with pytest.raises(ValueError, match="contourPool"):
        hip.feastDiagonalization(H, Y, 16, "legendre", -0.21, 0.21, 1e-4, 1, writeOut=False, contourPool=True)
