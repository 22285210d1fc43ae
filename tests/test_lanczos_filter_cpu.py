"""The two-pass Lanczos filter on the CPU: the NumPy twin (``eigensolvers_amd.lanczos_filter``) - the specification of
``csrc/lanczos_filter.hip`` - against the shifted-MINRES twin and dense algebra, FEAST's filter path driven by the twin
through a stand-in backend, and the ``contourDeal="vector"`` deal.

Shifts: the 8 upper-half-plane points of the 16-node Legendre contour on [-0.21, 0.21], one set with the real shift 0.5
added, and the 16 points of the 32-node contour (more than 8 shifts in one run)."""
import importlib
import math

import numpy as np
import pytest
import scipy.sparse as sp

import eigensolvers_amd as ea
from conftest import load_golden
from eigensolvers_amd import feast as pf
from eigensolvers_amd.shifted_minres import shifted_minres_host
from oracle.numpy_vector import RefVector

lf = importlib.import_module("eigensolvers_amd.lanczos_filter")       # the package exports the function of the same name

EPS = np.finfo(float).eps
REAL_SHIFT = 0.5
TOLS = [(1e-5, 1e-7), (1e-10, 1e-12)]


def contour(nc, lo=-0.21, hi=0.21):
    """(shifts, FEAST's weights -0.5 w r phase) of the nc-node Legendre half contour."""
    gk, wk = pf.quadraturePointsWeights(nc, "legendre", positiveHalf=True)
    zs, ws = [], []
    for g, w in zip(gk, wk):
        theta, z = pf.contour_point(lo, hi, g)
        zs.append(z)
        ws.append(-0.5 * w * (hi - lo) * 0.5 * (math.cos(theta) + 1j * math.sin(theta)))
    return zs, ws


Z8, W8 = contour(16)
Z16, W16 = contour(32)
SETS = {"contour8": (Z8, W8), "contour8+real": (Z8 + [REAL_SHIFT], W8 + [0.3 - 0.1j]), "contour16": (Z16, W16)}


@pytest.fixture(scope="module")
def rhs4000():
    B = np.random.default_rng(9).standard_normal((2, 4000))
    return B / np.linalg.norm(B, axis=1)[:, None]


@pytest.mark.parametrize("rtol,atol", TOLS)
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("name", list(SETS))
def test_stop_steps_and_estimates_equal_the_shifted_minres_twin(gapped4000, rhs4000, name, sign, rtol, atol):
    """The same scalar recurrences in the same order: equal, not close.  With pass 2 repeating pass 1's expressions the
    filtered vector is the twin's ``sum_j Re(w_j x_j)`` to 1e-12, relative."""
    H, (zs, ws) = gapped4000[0], SETS[name]
    q, scalars = lf.lanczos_filter_host(lambda v: H @ v, rhs4000, zs, ws, rtol, atol, 4000, sign)
    for r, b in enumerate(rhs4000):
        x, its, est, conv = shifted_minres_host(lambda v: H @ v, b, zs, rtol, atol, 4000, sign)
        sc = scalars[r]
        assert conv.all() and np.array_equal(sc.iterations, its) and np.array_equal(sc.estimates, est)
        assert np.array_equal(sc.converged, conv)
        assert len(sc.alphas) == its.max() and len(sc.betas) == its.max() + 1 and sc.betas[0] == np.linalg.norm(b)
        ref = sum((w * xj).real for w, xj in zip(ws, x))
        err = np.linalg.norm(q[r] - ref) / np.linalg.norm(ref)
        print(f"{name} sign {sign:+.0f} rtol {rtol:g} column {r}: steps {its.min()}..{its.max()} relative difference {err:.2e}")
        assert err <= 1e-12


def test_columns_are_independent(gapped4000, rhs4000):
    H = gapped4000[0]
    both = lf.lanczos_scalars_host(lambda v: H @ v, rhs4000, Z8, 1e-5, 1e-7, 4000)
    one = lf.lanczos_scalars_host(lambda v: H @ v, rhs4000[1], Z8, 1e-5, 1e-7, 4000)
    assert len(both) == 2 and len(one) == 1
    for a, b in zip(both[1], one[0]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_coefficients_against_dense_least_squares_n100(sign):
    """``minres_coefficients`` (rotations + O(m) back substitution) against ``numpy.linalg.lstsq`` on the (m+1) x m shifted
    tridiagonal, to 1e-12 relative; the contour around this problem's own window [160, 166], and a real shift."""
    g = load_golden("feast_n100.npz")
    A = np.array(g["A"], dtype=float)
    b = np.random.default_rng(9).standard_normal(100)
    zs = contour(16, 160.0, 166.0)[0] + [150.3]
    sc = lf.lanczos_scalars_host(lambda v: A @ v, b, zs, 1e-6, 1e-10, 1000, sign)[0]
    assert sc.converged.all()
    worst = 0.0
    for z, m in zip(zs, sc.iterations):
        for mm in sorted({1, 2, 3, int(m) // 2, int(m)}):
            T = np.zeros((mm + 1, mm))
            T[np.arange(mm), np.arange(mm)] = sc.alphas[:mm]
            T[np.arange(1, mm + 1), np.arange(mm)] = sc.betas[1:mm + 1]
            T[np.arange(mm - 1), np.arange(1, mm)] = sc.betas[1:mm]
            M = sign * (z * np.eye(mm + 1, mm) - T)
            rhs = np.zeros(mm + 1, complex)
            rhs[0] = sc.betas[0]
            dense = np.linalg.lstsq(M, rhs, rcond=None)[0]
            y = lf.minres_coefficients(sc.alphas, sc.betas, z, mm, sign)
            assert y.shape == (mm,)
            worst = max(worst, np.linalg.norm(y - dense) / np.linalg.norm(dense))
    print(f"sign {sign:+.0f}: largest relative difference to the dense least-squares solve {worst:.2e}")
    assert worst <= 1e-12


def test_single_solution_through_two_combinations(gapped4000, rhs4000):
    """NC = 2 with (Re y, Im y) rebuilds one shift's iterate: its true residual meets the target as the twin's does."""
    H, b = gapped4000[0], rhs4000[0]
    sc = lf.lanczos_scalars_host(lambda v: H @ v, b, Z8, 1e-5, 1e-7, 4000)[0]
    for j in (0, 7):
        y = lf.minres_coefficients(sc.alphas, sc.betas, Z8[j], sc.iterations[j])
        parts = lf.lanczos_combine_host(lambda v: H @ v, b, [sc.alphas], [sc.betas], [np.stack([y.real, y.imag], axis=1)])[0]
        x = parts[0] + 1j * parts[1]
        res = np.linalg.norm(b - (Z8[j] * x - H @ x))
        hinf = abs(H.copy()).sum(axis=1).max()        # abs() puts its operand into canonical form IN PLACE: the fixture is shared
        assert res <= 1.01 * 1e-5 + 100 * EPS * (abs(Z8[j]) + hinf) * np.linalg.norm(x), (j, res)


def test_breakdown_gives_the_exact_answer_in_one_step():
    h = np.linspace(-1.0, 1.0, 64)
    H = sp.diags(h).tocsr()
    b = np.zeros(64)
    b[3] = 2.0
    zs, ws = SETS["contour8+real"]
    for sign in (1.0, -1.0):
        calls = [0]

        def matvec(v):
            calls[0] += 1
            return H @ v

        q, scalars = lf.lanczos_filter_host(matvec, b, zs, ws, 1e-10, 1e-12, 100, sign)
        sc = scalars[0]
        assert np.all(sc.iterations == 1) and sc.converged.all() and np.all(sc.estimates == 0.0)
        assert calls[0] == 1                                   # pass 1's one step; pass 2's only term needs no product
        exact = sum((w * sign * 2.0 / (z - h[3])).real for z, w in zip(zs, ws))
        assert np.count_nonzero(q[0]) == 1 and abs(q[0, 3] - exact) <= 8 * EPS * sum(abs(w * 2.0 / (z - h[3])) for z, w in zip(zs, ws))


def test_zero_column_and_step_limit(gapped4000, rhs4000):
    H = gapped4000[0]
    calls = [0]

    def matvec(v):
        calls[0] += 1
        return H @ v

    q, scalars = lf.lanczos_filter_host(matvec, np.zeros((1, 4000)), Z8, W8, 1e-5, 1e-7, 10)
    assert not q.any() and calls[0] == 0 and not scalars[0].iterations.any() and scalars[0].converged.all()
    assert len(scalars[0].alphas) == 0
    sc = lf.lanczos_scalars_host(matvec, rhs4000, Z8, 1e-12, 0.0, 5)
    assert all(not s.converged.any() and np.all(s.iterations == 5) and len(s.alphas) == 5 for s in sc)
    with pytest.raises(UserWarning, match="Iterative solver is not converged"):
        lf.lanczos_filter_host(matvec, rhs4000, Z8, W8, 1e-12, 0.0, 5)


class FilterVector(RefVector):
    """The oracle's ndarray vector with both vector-major hooks driven by the NumPy twins, so that FEAST's paths run on
    the CPU."""
    calls = []

    @staticmethod
    def _solve_shifts(H, b, shifts, reverseGF=False):
        o = b.options["linearSystemArgs"]
        x, its, est, conv = shifted_minres_host(lambda v: H @ v, b.array, shifts, o["linear_tol"], o["linear_atol"],
                                                o["linearIter"], -1.0 if reverseGF else 1.0)
        b.last_solve_stats = {"iterations": [int(i) for i in its], "estimates": [float(e) for e in est], "products": int(its.max())}
        return [RefVector(x[j], b.options) for j in range(len(shifts))]

    @staticmethod
    def _lanczos_filter(H, B, shifts, weights, reverseGF=False):
        o = B[0].options["linearSystemArgs"]
        q, scalars = lf.lanczos_filter_host(lambda v: H @ v, np.array([b.array for b in B]), shifts, weights,
                                            o["linear_tol"], o["linear_atol"], o["linearIter"], -1.0 if reverseGF else 1.0)
        FilterVector.calls.append((len(B), len(shifts)))
        for r, b in enumerate(B):
            m = int(scalars[r].iterations.max())
            b.last_solve_stats = {"iterations": [int(i) for i in scalars[r].iterations],
                                  "estimates": [float(e) for e in scalars[r].estimates], "products": 2 * m - 1,
                                  "products_pass1": m, "products_pass2": m - 1, "group": r}
        return [RefVector(q[r], B[r].options) for r in range(len(B))]


ea.AbstractVector.register(FilterVector)


def _feast_n100(solver, **kw):
    g = load_golden("feast_n100.npz")
    o = {"linearSystemArgs": {"linearSolver": solver, "linearIter": 1000, "linear_tol": 1e-6, "linear_atol": 1e-10}}
    Y = [FilterVector(g["guess"][:, i].copy(), o) for i in range(6)]
    return g, pf.feastDiagonalization(g["A"], Y, 8, "legendre", 160.0, 166.0, 1e-10, 20, writeOut=False, **kw)


def test_feast_filter_path_on_the_twin_agrees_with_the_shared_lanczos_path():
    FilterVector.calls.clear()
    g, (ev, Yf, st) = _feast_n100("lanczos_filter")
    _, (ev_s, _, st_s) = _feast_n100("minres_shifted")
    assert st["converged"] and st_s["converged"] and st["outerIter"] == st_s["outerIter"]
    assert len(ev) == len(ev_s)
    assert pf._eigenvalue_change_in_window(ev, ev_s, 160.0, 166.0) < 1e-10          # eConv of both runs
    exact = pf.select_within_range(np.linalg.eigvalsh(g["A"]), 160.0, 166.0)[0]
    np.testing.assert_allclose(pf.select_within_range(ev, 160.0, 166.0)[0], exact, rtol=0, atol=1e-4)
    rec = st["lanczosFilter"]
    assert "sharedLanczos" not in st and len(rec) == st["outerIter"] + 1
    assert len(FilterVector.calls) == len(rec)                  # ONE call per FEAST iteration
    assert all(s == 4 for _, s in FilterVector.calls)           # 8 nodes = 4 contour points, all in the call
    for r, (nvec, _) in zip(rec, FilterVector.calls):
        assert r["runs"] == nvec == len(r["products_pass1"]) == len(r["products_pass2"])
        assert len(r["pairs"]) == len(r["steps"]) == 4 * nvec
        assert sorted(map(tuple, r["pairs"])) == [(k, i) for k in range(4) for i in range(nvec)]
        for vec in range(nvec):
            top = max(s for (k, v), s in zip(r["pairs"], r["steps"]) if v == vec)
            assert r["products_pass1"][vec] == top and r["products_pass2"][vec] == top - 1


def test_contour_pool_with_the_filter_is_refused():
    with pytest.raises(ValueError, match="contourPool"):
        _feast_n100("lanczos_filter", contourPool=True)


def test_the_other_paths_do_not_take_the_filter():
    FilterVector.calls.clear()
    _, (ev, Yf, st) = _feast_n100("minres_shifted")
    assert "lanczosFilter" not in st and not FilterVector.calls


class _Comm:
    def __init__(self, rank, nranks):
        self.rank, self.nranks = rank, nranks


@pytest.mark.parametrize("nranks", [1, 2, 3, 5, 8])
def test_vector_deal(nranks):
    npoints, nsub = 4, 6
    full = pf._contour_pairs(npoints, nsub)
    per_rank = [pf._contour_pairs(npoints, nsub, _Comm(r, nranks), "vector") for r in range(nranks)]
    assert sorted(p for pr in per_rank for p in pr) == sorted(full)             # a partition of the full list
    assert sum(len(pr) for pr in per_rank) == len(full)
    for im0 in range(nsub):
        holders = [r for r, pr in enumerate(per_rank) if any(i == im0 for _, i in pr)]
        assert holders == [im0 % nranks]                                        # each vector on one rank ...
        assert sorted(k for k, i in per_rank[im0 % nranks] if i == im0) == list(range(npoints))    # ... with all its points
    with pytest.raises(ValueError, match="contourDeal"):
        pf._contour_pairs(npoints, nsub, _Comm(0, nranks), "vectors")


def test_feast_with_the_vector_deal_on_two_stand_in_ranks():
    """Two ranks run one after the other, their partial sums added by a recording all-reduce: the same eigenvalues as the
    undivided run, and no rank ran another's vector."""
    g = load_golden("feast_n100.npz")
    o = {"linearSystemArgs": {"linearSolver": "lanczos_filter", "linearIter": 1000, "linear_tol": 1e-6, "linear_atol": 1e-10}}
    nodes = [pf.contour_point(160.0, 166.0, gq) + (w,) for gq, w in zip(*pf.quadraturePointsWeights(8, "legendre"))]
    Y = [FilterVector(g["guess"][:, i].copy(), o) for i in range(6)]
    whole, _ = pf._lanczos_filter_sums(FilterVector, g["A"], Y, pf._contour_pairs(4, 6), nodes, 3.0, 1.0, {})
    parts = []
    for r in range(2):
        FilterVector.calls.clear()
        pairs = pf._contour_pairs(4, 6, _Comm(r, 2), "vector")
        Q, rec = pf._lanczos_filter_sums(FilterVector, g["A"], Y, pairs, nodes, 3.0, 1.0, {})
        assert FilterVector.calls == [(3, 4)] and rec["runs"] == 3
        assert [q is not None for q in Q] == [i % 2 == r for i in range(6)]
        parts.append(Q)
    for i in range(6):
        assert np.array_equal(parts[i % 2][i].array, whole[i].array)
