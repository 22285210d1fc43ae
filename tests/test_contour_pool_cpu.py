"""The always-full pool of contour solves on the CPU: the pool driver (eigensolvers_amd.gcrotmk.gcrotmk_device_pool) with
a NumPy provider of the vector operations - it only changes WHEN a solve's steps run, so every job gets exactly the
result of its single solve - its scheduling invariants, and the FEAST driver's pooled path (contourPool=True) and
balanced deal (contourDeal="balanced") on an ndarray backend whose solveBlock takes a shift per right-hand side.  The
solves of all contour points of a FEAST iteration are independent (feast.py:189-200)."""
import numpy as np
import pytest

import eigensolvers_amd as ea
from conftest import load_golden
from eigensolvers_amd import feast as pf
from eigensolvers_amd.gcrotmk import gcrotmk_device, gcrotmk_device_pool
from eigensolvers_amd.generators import gapped_csr_host
from oracle.numpy_vector import RefVector

ea.AbstractVector.register(RefVector)


class NumpyOps:
    """complex ndarrays in place of (re, im) device buffer pairs; the arithmetic of scipy's BLAS calls"""
    dtype = np.complex128

    def __init__(self, n):
        self.n = n

    def new(self):
        return np.empty(self.n, dtype=complex)

    def zeros(self):
        return np.zeros(self.n, dtype=complex)

    def copy(self, a):
        return a.copy()

    def dot(self, a, b):
        return np.vdot(a, b)

    def nrm2(self, a):
        return float(np.linalg.norm(a))

    def axpy(self, alpha, x, y):
        y += alpha * x

    def scal(self, alpha, x):
        x *= alpha

    def scaled(self, alpha, x):
        return alpha * x

    def arnoldi_step(self, vs, w):
        before = float(np.linalg.norm(w))
        h = np.zeros(len(vs), dtype=complex)
        for j, v in enumerate(vs):
            h[j] = np.vdot(v, w)
            w -= h[j] * v
        after = float(np.linalg.norm(w))
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = 1.0 / after
        if np.isfinite(alpha):
            w *= alpha
        return before, h, after

    def combine(self, coeffs, vecs):
        out = np.zeros(self.n, dtype=complex)
        for c, v in zip(coeffs, vecs):
            out += c * v
        return out


W = 4
SHIFTS = (0.02 + 0.05j, -0.01 + 0.11j, 0.03 + 0.2j)          # close to the real axis ... further off: unequal solves


@pytest.fixture(scope="module")
def pooled():
    """12 complex jobs with 3 shifts (point-major, as FEAST lists them) plus one zero right-hand side, W = 4: the single
    solves, what the pool handed out and every block product it asked for."""
    n = 1500
    H = gapped_csr_host(n, 16, seed=3)
    rng = np.random.default_rng(0)
    rhs = [(rng.standard_normal(n) + 0j) for _ in range(4)]
    rhs = [b / np.linalg.norm(b) for b in rhs]
    jobs = [(rhs[i], (k, i)) for k in range(3) for i in range(4)]          # tag = (shift index, vector index)
    jobs.insert(5, (np.zeros(n, dtype=complex), (1, "zero")))
    kw = dict(rtol=1e-7, atol=1e-12, maxiter=200, complex_pairs=True)

    def A(z):
        return lambda v: z * v - H @ v

    single = [gcrotmk_device(None, A(SHIFTS[tag[0]]), b, n, ops=NumpyOps(n), **kw) for b, tag in jobs]
    calls = []                                   # per block product: (tags, unstarted jobs left when it was asked for)
    started = [0]

    def factory():
        started[0] += 1
        return NumpyOps(n)

    def block_matvec(vs, tags):
        calls.append((list(tags), len(jobs) - started[0], [v.copy() for v in vs]))
        return [A(SHIFTS[t[0]])(v) for v, t in zip(vs, tags)]

    stats = {}
    handed = list(gcrotmk_device_pool(None, block_matvec, jobs, n, W, ops_factory=factory, pool_stats=stats, **kw))
    return n, jobs, single, handed, calls, stats


def test_pool_driver_is_the_single_solves_bit_for_bit(pooled):
    n, jobs, single, handed, calls, stats = pooled
    assert sorted(h[0] for h in handed) == list(range(len(jobs)))          # every job handed out, once
    for i, tag, x, info, st in handed:
        x1, info1, st1 = single[i]
        assert tag == jobs[i][1]
        assert info == info1 == 0 and st == st1
        np.testing.assert_array_equal(np.asarray(x), np.asarray(x1))
    zero = next(h for h in handed if h[1] == (1, "zero"))
    assert zero[4]["matvecs"] == 0 and not np.any(zero[2])
    # the shifts make unequal work: otherwise the pool would have nothing to refill
    its = [single[i][2]["matvecs"] for i in range(len(jobs)) if jobs[i][1][1] != "zero"]
    assert max(its) > 1.5 * min(its), its
    # solutions leave the pool as their solves end, not in job order
    assert [h[0] for h in handed] != sorted(h[0] for h in handed)


def test_pool_scheduling_invariants(pooled):
    n, jobs, single, handed, calls, stats = pooled
    hist = {}
    for tags, unstarted, vs in calls:
        assert 1 <= len(tags) <= W                                         # never more than W operands
        if len(tags) < W:
            assert unstarted == 0, (len(tags), unstarted)                  # a thin block only once the job list is empty
        assert len(set(tags)) == len(tags)
        hist[len(tags)] = hist.get(len(tags), 0) + 1
    assert stats["width"] == W and stats["jobs"] == len(jobs)
    assert stats["rounds"] == len(calls) and stats["histogram"] == hist
    # every operand reaches block_matvec with its own job's tag: a job's products are exactly the operands that came
    # with its tag, as many as its single solve needed
    per_tag = {}
    for tags, _, vs in calls:
        for t in tags:
            per_tag[t] = per_tag.get(t, 0) + 1
    for i, (b, tag) in enumerate(jobs):
        assert per_tag.get(tag, 0) == single[i][2]["matvecs"] == stats["products"][i]
        assert stats["outer"][i] == single[i][2]["outer"]
    assert "zero" not in {t[1] for tags, _, _ in calls for t in tags}      # the zero right-hand side asks for no product
    # the first operand a job sends is its normalised right-hand side: the tag travels with the right vector
    first = {}
    for tags, _, vs in calls:
        for t, v in zip(tags, vs):
            first.setdefault(t, v)
    for b, tag in jobs:
        if tag[1] != "zero":
            np.testing.assert_array_equal(first[tag], b / np.linalg.norm(b))
    # full blocks until the list is empty, then the tail: sum(len) = all products, and the pool beats one point at a time
    assert sum(len(t) for t, _, _ in calls) == sum(s[2]["matvecs"] for s in single)
    per_point = sum(max(single[i][2]["matvecs"] for i, (b, t) in enumerate(jobs) if t[0] == k) for k in range(3))
    assert stats["rounds"] < per_point


def test_pool_width_is_checked():
    with pytest.raises(ValueError):
        list(gcrotmk_device_pool(None, None, [], 10, 17))
    with pytest.raises(ValueError):
        list(gcrotmk_device_pool(None, None, [], 10, 0))
    stats = {}
    assert list(gcrotmk_device_pool(None, None, [], 10, 4, pool_stats=stats)) == [] and stats["rounds"] == 0


# ---- FEAST ------------------------------------------------------------------------------------------------------
class DenseVector(RefVector):
    """RefVector with a ``solveBlock`` hook that takes one shift or a shift per right-hand side: every solve is a direct
    dense solve, so two runs that ask for the same solves get the same bits whatever the order they are asked in."""
    reverse_delivery = False
    log = None                                   # per solveBlock call: (a shift per operand?, the operands' shifts)

    @staticmethod
    def _one(H, b, z):
        return RefVector(np.linalg.solve(z * np.eye(H.shape[0]) - H, b.array.astype(complex)), b.options)

    @staticmethod
    def solveBlock(H, bs, sigma, x0=None, opType="her", reverseGF=False, onSolution=None, poolStats=None):
        bs = list(bs)
        per_operand = np.ndim(sigma) > 0
        zs = list(sigma) if per_operand else [sigma] * len(bs)
        assert len(zs) == len(bs) and not reverseGF and x0 is None
        if DenseVector.log is not None:
            DenseVector.log.append((per_operand, list(zs)))
        sols = [DenseVector._one(H, b, complex(z)) for b, z in zip(bs, zs)]
        if onSolution is None:
            return sols
        order = range(len(bs) - 1, -1, -1) if DenseVector.reverse_delivery else range(len(bs))
        for i in order:
            onSolution(i, sols[i])
        if poolStats is not None and per_operand:
            poolStats.update({"width": 16, "rounds": 1, "histogram": {len(bs): 1}, "products": [1] * len(bs),
                              "outer": [0] * len(bs)})
        return [None] * len(bs)


ea.AbstractVector.register(DenseVector)


def _feast(cls, **kw):
    g = load_golden("feast_n100.npz")
    Y = [cls(g["guess"][:, i].copy(), {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 1000,
                                                             "linear_tol": 1e-2}}) for i in range(6)]
    ev, Yf, st = pf.feastDiagonalization(g["A"], Y, 8, "legendre", 160.0, 166.0, 1e-10, 20, writeOut=False, **kw)
    return g, ev, Yf, st


@pytest.mark.parametrize("reverse", [False, True])
def test_feast_with_the_pool_is_the_per_point_loop_bit_for_bit(monkeypatch, reverse):
    monkeypatch.setattr(DenseVector, "reverse_delivery", reverse)
    monkeypatch.setattr(DenseVector, "log", [])
    g, ev0, Y0, st0 = _feast(DenseVector)
    assert not any(per for per, zs in DenseVector.log) and "contourPool" not in st0        # off: one point per call
    monkeypatch.setattr(DenseVector, "log", [])
    g, ev1, Y1, st1 = _feast(DenseVector, contourPool=True)
    assert all(per for per, zs in DenseVector.log)                                         # on: a shift per operand
    assert len(DenseVector.log) == st1["outerIter"] + 1 == len(st1["contourPool"])         # one job list per iteration
    np.testing.assert_array_equal(ev1, ev0)
    assert st1["outerIter"] == st0["outerIter"] and len(Y1) == len(Y0)
    for a, b in zip(Y1, Y0):
        np.testing.assert_array_equal(a.array, b.array)
    # point-major job list over the current subspace: 4 half-contour points x the vectors of that iteration
    rec = st1["contourPool"][0]
    assert rec["pairs"] == [[k, i] for k in range(4) for i in range(6)] and len(rec["products"]) == 24
    assert len(st1["contourPool"][-1]["pairs"]) == 4 * len(Y1)
    exact = np.linalg.eigvalsh(g["A"])
    inside = exact[(exact >= 160.0) & (exact <= 166.0)]
    np.testing.assert_allclose(pf.select_within_range(ev1, 160.0, 166.0)[0], inside, rtol=1e-9)


def test_a_backend_without_the_capability_keeps_the_per_point_loop():
    g, ev, Yf, st = _feast(RefVector, contourPool=True)
    np.testing.assert_allclose(ev, g["ev"], rtol=1e-9)
    assert st["outerIter"] == int(g["outerIter"]) and len(Yf) == int(g["nvec"])
    assert "contourPool" not in st


class _Rank:
    def __init__(self, rank, nranks):
        self.rank, self.nranks = rank, nranks


@pytest.mark.parametrize("npoints,nsub,nranks", [(4, 6, 2), (8, 16, 2), (8, 15, 2), (3, 5, 2), (8, 16, 3)])
def test_the_balanced_deal_gives_every_rank_the_same_mix(npoints, nsub, nranks):
    every = [(k, i) for k in range(npoints) for i in range(nsub)]
    assert pf._contour_pairs(npoints, nsub) == every
    deal = [pf._contour_pairs(npoints, nsub, _Rank(r, nranks), "balanced") for r in range(nranks)]
    assert sorted(p for d in deal for p in d) == every                     # every pair once
    assert max(map(len, deal)) - min(map(len, deal)) <= 1
    for d in deal:
        assert d == sorted(d)                                              # point-major on every rank
    today = [pf._contour_pairs(npoints, nsub, _Rank(r, nranks), "point") for r in range(nranks)]
    for r in range(nranks):
        assert today[r] == [(k, i) for k, i in every if k % nranks == r]   # whole points, round robin
    with pytest.raises(ValueError):
        pf._contour_pairs(npoints, nsub, _Rank(0, nranks), "rows")


@pytest.mark.parametrize("deal", ["point", "balanced"])
@pytest.mark.parametrize("pool", [False, True])
def test_feast_over_two_fake_ranks_solves_its_share_of_the_deal(monkeypatch, deal, pool):
    """One FEAST iteration on each of two fake ranks (the all-reduce is the identity): what each rank solved is its
    share of the deal, with the pool and without it."""
    g = load_golden("feast_n100.npz")
    opts = {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 1000, "linear_tol": 1e-2}}
    solved = {}

    class Comm(_Rank):
        def allreduce(self, v):
            return v

    def run(comm):
        monkeypatch.setattr(DenseVector, "log", [])
        Y = [DenseVector(g["guess"][:, i].copy(), dict(opts)) for i in range(6)]
        ev, Yf, st = pf.feastDiagonalization(g["A"], Y, 8, "legendre", 160.0, 166.0, 1e-10, 1, writeOut=False,
                                             contourComm=comm, contourPool=pool, contourDeal=deal)
        solved[comm.rank] = sum(len(zs) for per, zs in DenseVector.log)
        return st

    st = [run(Comm(r, 2)) for r in range(2)]
    assert solved[0] + solved[1] == 24 and solved[0] == solved[1] == 12
    if pool:
        pairs = [tuple(p) for s in st for p in s["contourPool"][0]["pairs"]]
        assert sorted(pairs) == [(k, i) for k in range(4) for i in range(6)]
        for r, s in enumerate(st):
            assert [tuple(p) for p in s["contourPool"][0]["pairs"]] == pf._contour_pairs(4, 6, _Rank(r, 2), deal)
