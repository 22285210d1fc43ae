"""The always-full pool of contour solves on the GPU: the block product with a complex shift PER OPERAND
(hipeig_spmm_shift_pairs_z), HipVector.solveBlock with a shift per right-hand side, and feastDiagonalization with
contourPool=True, alone and over contour replicas with both deals.  The solves of all contour points of a FEAST iteration
are independent (feast.py:189-200); the pool only changes when a solve's steps run.  Bounds are those of the tests of the
single-shift paths (test_gpu_feast.py, test_gpu_loopback.py)."""
import warnings

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _shifts(rng, n):
    return [complex(rng.uniform(-0.2, 0.2), rng.uniform(0.02, 0.3)) for _ in range(n)]


def _check_against_single_products(hip, H, N, rng, cases):
    ctx = hip.HipContext.default()
    for npairs, reverse in cases:
        zs = _shifts(rng, npairs)
        xs = [(hip.HipVector(rng.standard_normal(N)), hip.HipVector(rng.standard_normal(N))) for _ in range(npairs)]
        ys = H.apply_shifted_pairs(zs, [(a._buf, b._buf) for a, b in xs], reverse=reverse)
        assert len(ys) == npairs
        for z, (xr, xi), (yr, yi) in zip(zs, xs, ys):
            rr, ri = ctx.alloc(N), ctx.alloc(N)
            H.apply_shifted_pair(z, xr._buf, xi._buf, rr, ri, reverse=reverse)
            ref = hip.HipVector(rr).array + 1j * hip.HipVector(ri).array
            got = hip.HipVector(yr).array + 1j * hip.HipVector(yi).array
            err, bound = np.max(np.abs(got - ref)), 1e-14 * np.max(np.abs(ref))
            print(f"N={N} npairs={npairs} reverse={reverse} z={z:.3f} err={err:.3e} bound={bound:.3e}")
            assert err <= bound


@pytest.mark.parametrize("N", [4000, 300_000])
def test_block_product_with_a_shift_per_operand_matches_the_single_products(hip, N):
    """1..6 operands (8-wide blocks, a 4-wide remainder, the one-operand fallback), both signs, every operand with its own
    shift, against hipeig_spmv_shift_pair with that operand's shift."""
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    _check_against_single_products(hip, H, N, np.random.default_rng(N),
                                   ((1, False), (2, True), (3, False), (4, False), (5, True), (6, False)))
    if N > 100_000:
        assert H.block_info()["variant"] == "column-window-blocked"


@pytest.mark.parametrize("variant", [1, 2])
def test_eight_operands_per_pass_with_a_shift_each(hip, monkeypatch, variant):
    """The 16-wide block (8 complex operands per pass) forced through its knob, both block kernels, 5..11 operands (a
    16-wide pass and remainders of every width), both signs."""
    N = 70_001
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    H.set_block_variant(variant)
    monkeypatch.setenv("HIPEIG_PAIR_BLOCK_WIDTH", "8")
    _check_against_single_products(hip, H, N, np.random.default_rng(variant), ((5, False), (7, True), (8, False), (11, False)))
    assert H.block_info()["variant"] == ("row-owner" if variant == 1 else "column-window-blocked")


@pytest.mark.parametrize("wide", ["4", "8"])
def test_equal_shifts_are_the_single_shift_product_bit_for_bit(hip, monkeypatch, wide):
    """All shifts equal, row-owner kernel (a row's terms are added in a fixed order): same K, same operator sum, same
    epilogue arithmetic as the one-shift product - the same bits, for every block width (4, 8 and 16 wide passes)."""
    N = 70_001
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    H.set_block_variant(1)
    monkeypatch.setenv("HIPEIG_PAIR_BLOCK_WIDTH", wide)
    rng = np.random.default_rng(5)
    z = -0.07 + 0.19j
    for npairs, reverse in ((2, False), (3, True), (4, False), (7, True), (8, False), (11, False)):
        xs = [(hip.HipVector(rng.standard_normal(N)), hip.HipVector(rng.standard_normal(N))) for _ in range(npairs)]
        bufs = [(a._buf, b._buf) for a, b in xs]
        one = H.apply_shifted_pairs(z, bufs, reverse=reverse)
        per = H.apply_shifted_pairs([z] * npairs, bufs, reverse=reverse)
        for (ar, ai), (br, bi) in zip(one, per):
            np.testing.assert_array_equal(hip.HipVector(br).array, hip.HipVector(ar).array)
            np.testing.assert_array_equal(hip.HipVector(bi).array, hip.HipVector(ai).array)
    assert H.block_info()["variant"] == "row-owner"
    with pytest.raises(ValueError):
        H.apply_shifted_pairs([z] * 3, bufs)


@pytest.mark.parametrize("cols", [1, 4])
def test_pooled_contour_solves_equal_the_single_solves(hip, cols):
    """6 right-hand sides x 2 contour points through solveBlock with a shift per right-hand side, pool width 4 forced: per
    solve the solution of the one-by-one solve to the solve tolerance, about the same number of products, true residual
    below the tolerance (the bounds of test_contour_solves_in_lock_step_equal_the_single_solves)."""
    N, points = 200_000, (0.02 + 0.05j, -0.03 + 0.12j)
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    rng = np.random.default_rng(2)
    o = {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 3000, "linear_tol": 1e-8, "linear_atol": 1e-12,
                              "arnoldiColumnsPerPass": cols}, "contourPoolWidth": 4}
    bs = [hip.HipVector(rng.standard_normal(N), o) for _ in range(6)]
    for b in bs:
        b.normalize()
    jobs = [(b, z) for z in points for b in bs]                       # point-major, as FEAST lists them
    one, its_one = [], []
    for b, z in jobs:
        one.append(hip.HipVector.solve(H, b, z))
        its_one.append(one[-1].last_solve_stats["iterations"])
    pool = {}
    blk = hip.HipVector.solveBlock(H, [b for b, z in jobs], [z for b, z in jobs], poolStats=pool)
    assert len(blk) == len(jobs)
    ctx = hip.HipContext.default()
    for j, ((b, z), w1, wb, it1) in enumerate(zip(jobs, one, blk, its_one)):
        assert isinstance(wb, hip.hip_vector.HipComplexVector)
        a1, ab = w1.array, wb.array
        rel = np.linalg.norm(ab - a1) / np.linalg.norm(a1)
        rr, ri = ctx.alloc(N), ctx.alloc(N)                           # true residual of the pooled solution
        H.apply_shifted_pair(z, wb.re._buf, wb.im._buf, rr, ri)
        res = np.linalg.norm(hip.HipVector(rr).array + 1j * hip.HipVector(ri).array - b.array)
        print(f"cols={cols} job={j} z={z} rel={rel:.3e} products={pool['products'][j]} single={it1} residual={res:.3e}")
        assert rel <= 1e-6
        assert abs(pool["products"][j] - it1) <= max(3, it1 // 20)
        assert res <= 5e-8
    # the pool's own record: width 4, never more, full blocks until the job list is empty
    assert pool["width"] == 4 and pool["jobs"] == 12 and max(pool["histogram"]) == 4
    assert sum(k * v for k, v in pool["histogram"].items()) == sum(pool["products"])
    assert pool["rounds"] == sum(pool["histogram"].values())
    thin = sum(v for k, v in pool["histogram"].items() if k < 4)
    assert thin <= max(pool["products"][-4:]) + 4          # thin blocks only while the last solves run out
    # handed out as the solves end: every index once, the returned list then holds nothing
    seen = []
    out = hip.HipVector.solveBlock(H, [b for b, z in jobs[:5]], [z for b, z in jobs[:5]],
                                   onSolution=lambda i, x: seen.append((i, x.last_solve_stats["iterations"])))
    assert out == [None] * 5 and sorted(i for i, _ in seen) == list(range(5))
    with pytest.raises(ValueError):
        hip.HipVector.solveBlock(H, bs[:3], [points[0]] * 2)


def _feast_n100(hip, ctx, comm=None, **kw):
    g = load_golden("feast_n100.npz")
    opts = {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 1000, "linear_tol": 1e-2}}
    opts.update(kw.pop("options", {}))
    A = hip.HipCsrOperator.from_dense(g["A"], ctx=ctx)
    Y = [hip.HipVector(g["guess"][:, i].copy(), dict(opts), ctx=ctx) for i in range(6)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev, Yf, st = hip.feastDiagonalization(A, Y, 8, "legendre", 160.0, 166.0, 1e-10, 20, writeOut=False,
                                             contourComm=comm, **kw)
    return g, ev, Yf, st


@pytest.mark.parametrize("width", [16, 5])
def test_feast_reference_problem_with_the_pool(hip, width):
    """The reference's own run (golden file) through HipVector with contourPool=True: window eigenvalues to rtol 1e-9,
    iteration count and vector count equal (the bounds of test_feast_contour_replicas, which regroups the same sums)."""
    g, ev, Yf, st = _feast_n100(hip, hip.HipContext.default(), contourPool=True, options={"contourPoolWidth": width})
    inside = (g["ev"] >= 160.0) & (g["ev"] <= 166.0)
    assert inside.sum() == 3
    print("width", width, "ev", ev[inside], "golden", g["ev"][inside], "outerIter", st["outerIter"])
    np.testing.assert_allclose(ev[inside], g["ev"][inside], rtol=1e-9)
    assert st["outerIter"] == int(g["outerIter"]) and len(Yf) == int(g["nvec"])
    recs = st["contourPool"]
    assert len(recs) == st["outerIter"] + 1
    for rec in recs:
        assert rec["width"] == width and max(rec["histogram"]) <= width
        assert len(rec["pairs"]) == len(rec["products"]) and rec["pairs"] == sorted(rec["pairs"])
        assert sum(k * v for k, v in rec["histogram"].items()) == sum(rec["products"])
    assert recs[0]["pairs"] == [[k, i] for k in range(4) for i in range(6)]


@pytest.mark.parametrize("deal", ["point", "balanced"])
def test_feast_contour_replicas_with_the_pool(hip, deal):
    """test_feast_contour_replicas' loopback run with P = 3 and the pool on every replica, both deals: same bounds."""
    from eigensolvers_amd.distributed import ContourReplicas, LoopbackGroup
    P = 3
    g, ev_s, Y_s, st_s = _feast_n100(hip, hip.HipContext.default())
    it_s, n_s = st_s["outerIter"], len(Y_s)
    grp = LoopbackGroup(P)
    try:
        def run(rank, ctx):
            _, ev, Yf, st = _feast_n100(hip, ctx, ContourReplicas(ctx), contourPool=True, contourDeal=deal)
            return ev, st["outerIter"], len(Yf), Yf[0].array, st["contourPool"]
        res = grp.run(run)
    finally:
        grp.close()
    inside = (ev_s >= 160.0) & (ev_s <= 166.0)
    assert inside.sum() == 3
    for ev, it, n, y0, recs in res:
        np.testing.assert_array_equal(ev, res[0][0])
        np.testing.assert_array_equal(y0, res[0][3])
        np.testing.assert_allclose(ev[inside], ev_s[inside], rtol=1e-9)
        np.testing.assert_allclose(ev[inside], g["ev"][inside], rtol=1e-9)
        np.testing.assert_allclose(ev, ev_s, rtol=1e-6)
        assert it == it_s == int(g["outerIter"]) and n == n_s == int(g["nvec"])
    first = [r[4][0]["pairs"] for r in res]                       # the deal of the first iteration: 4 points x 6 vectors
    assert sorted(p for f in first for p in f) == [[k, i] for k in range(4) for i in range(6)]
    if deal == "balanced":
        assert [len(f) for f in first] == [8, 8, 8]
    else:
        assert [len(f) for f in first] == [12, 6, 6]


def test_feast_at_the_usable_inner_tolerance_with_the_pool(hip):
    """The recipe of test_feast_at_the_reference_comparable_inner_tolerance (config #5 at N = 2e4, gcrotmk rtol 1e-5) with
    the pool: its assertions, and the iteration count of the pool-off run."""
    import scipy.linalg as la
    from eigensolvers_amd.generators import gapped_params
    N, m0 = 20_000, 16
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    Q = la.qr(np.random.default_rng(9).standard_normal((N, m0)), mode="economic")[0]
    o = {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7,
                              "arnoldiColumnsPerPass": 4}}
    runs = {}
    for pool in (False, True):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runs[pool] = hip.feastDiagonalization(H, [hip.HipVector(Q[:, i].copy(), o) for i in range(m0)], 16, "legendre",
                                                  -0.21, 0.21, 1e-4, 12, writeOut=False, contourPool=pool)
    ev, Y, st = runs[True]
    print("pool on: outerIter", st["outerIter"], "residual", st["residual"], "| off:", runs[False][2]["outerIter"],
          runs[False][2]["residual"])
    assert st["residual"] < 1e-4 and 2 <= st["outerIter"] <= 10
    inside = np.sort(ev[(ev > -0.21) & (ev < 0.21)])
    targets = np.sort(gapped_params(N, 32, 7)["targets"])
    assert len(inside) == 16 and np.all(np.abs(inside - targets) < 2e-3)
    res = hip.true_residual_norms(H, ev, Y, m0)
    assert np.all(res < 1e-2), res
    assert st["outerIter"] == runs[False][2]["outerIter"]
    assert "contourPool" not in runs[False][2] and len(st["contourPool"]) == st["outerIter"] + 1
    rec = st["contourPool"][0]
    assert rec["width"] == 16 and len(rec["pairs"]) == 8 * 16
    print("first iteration: rounds", rec["rounds"], "histogram", rec["histogram"], "products", sum(rec["products"]))
