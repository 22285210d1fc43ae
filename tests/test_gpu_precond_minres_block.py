"""The lock-step block form of the Jacobi-preconditioned MINRES (``linearSystemArgs["preconditionerLockStep"] = True``,
csrc/minres_block_precond.hip) against the per-column NumPy twin (``_precond_cases.twin``) with the bounds of
``test_gpu_precond_minres.py`` (``_sweep_cases.check_against_twin``): iterations and istop equal, x within
max(1e-9, 100 rtol) ||x||, rnorm within 5 %, Anorm within 1e-3, true residual <= 1.05 x the twin's + 1e-13.

Equal counts are a condition on the INPUTS: a block product adds a row in another order than the twin's, so a column whose
deciding test passes ``rtol`` by a hair may stop an iteration earlier or later on the device.  Every column used here is
checked on the host first (``_robust``): at the twin's stopping iteration and at the one before, both tests are at least
5 % away from ``rtol``."""
import ctypes as C
import warnings

import numpy as np
import pytest

import _precond_cases as pc
from _sweep_cases import check_against_twin
from eigensolvers_amd import _lib
from eigensolvers_amd.generators import gapped_csr_host, guess_vector
from eigensolvers_amd.hip_vector import _ptr_table

pytestmark = pytest.mark.gpu

N = 4000


def _opts(it=2000, tol=1e-10, lock=True, pre="jacobi", **lsa):
    d = {"linearSolver": "minres", "linearIter": it, "linear_tol": tol}
    if pre is not None:
        d["preconditioner"] = pre
    if lock is not None:
        d["preconditionerLockStep"] = lock
    d.update(lsa)
    return {"linearSystemArgs": d}


def _unit_rows(seed, rows, n, take):
    R = np.random.default_rng(seed).standard_normal((rows, n))[:take]
    return [r / np.linalg.norm(r) for r in R]


def _columns8():
    """unit_guess, the first five normalised rows of default_rng(3).standard_normal((7, N)), e_1234 and a zero column."""
    e = np.zeros(N)
    e[1234] = 1.0
    return [pc.unit_guess(N)] + _unit_rows(3, 7, N, 5) + [e, np.zeros(N)]


def _robust(label, tw, rtol):
    """The twin's stop is at least 5 % away from rtol in both tests, at the stopping iteration and at the one before."""
    trace = tw[4]
    last, before = trace[-1], trace[-2]
    assert last["istop"] in (1, 2), label
    deciding = last["test1"] if last["istop"] == 1 else last["test2"]
    assert deciding <= 0.95 * rtol, (label, deciding / rtol)
    for t in (last["test1"], last["test2"]):
        assert t <= 0.95 * rtol or t >= 1.05 * rtol, (label, t / rtol)
    assert min(before["test1"], before["test2"]) >= 1.05 * rtol, (label, before["test1"] / rtol, before["test2"] / rtol)


def _solve(hip, H, cols, sigma, rtol, it=2000, reverse=False, ctx=None, **lsa):
    vecs = [hip.HipVector(c.copy(), _opts(it, rtol, **lsa), ctx=ctx) for c in cols]
    return hip.HipVector.solveBlock(H, vecs, sigma, reverseGF=reverse), vecs


def _check_block(hip, name, Hh, H, cols, sigma, rtol, reverse=False):
    """One lock-step solve of ``cols`` against the per-column twins; returns the twins' iteration counts."""
    sign = -1.0 if reverse else 1.0
    twins = []
    for j, c in enumerate(cols):
        if c.any():
            twins.append(pc.twin((name, j), Hh, c, sigma, rtol, 2000, sign=sign))
            _robust(f"{name} column {j} rtol {rtol:g}", twins[-1], rtol)
        else:
            twins.append(None)
    X, vecs = _solve(hip, H, cols, sigma, rtol, reverse=reverse)
    assert len(X) == len(cols)
    for j, (x, tw) in enumerate(zip(X, twins)):
        st = x.last_solve_stats
        assert st["lockStep"] is True and st["preconditioner"] == "jacobi" and vecs[j].last_solve_stats is st
        if tw is None:
            assert st["iterations"] == 0 and not x.array.any()
        else:
            check_against_twin(f"{name} column {j} rtol {rtol:g} reverse {reverse}", Hh, cols[j], sigma, rtol, x, tw, sign=sign)
    return [tw[2] for tw in twins if tw is not None]


@pytest.fixture(scope="module")
def gapped16(hip):
    Hh = gapped_csr_host(N, 16, seed=7)
    return Hh, hip.HipCsrOperator.from_scipy(Hh)


# ---------------------------------------------------------------- 1. tracks the twin
@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("k", [8, 3])
def test_tracks_the_twin(hip, gapped16, k, rtol):
    """Fails without the feature: there is no hipeig_minres_block_jacobi and no "lockStep" in the stats."""
    Hh, H = gapped16
    cols = _columns8()[:k]
    counts = _check_block(hip, "g4000", Hh, H, cols, pc.SIGMA, rtol)
    assert len(set(counts)) > 1                                    # the columns stop at different iterations: masking runs
    if rtol == 1e-10:
        assert max(counts) > 16                                    # past the first chunk
    if k == 8 and rtol == 1e-10:
        _check_block(hip, "g4000", Hh, H, cols, pc.SIGMA, rtol, reverse=True)


# ---------------------------------------------------------------- 2. both block kernels
@pytest.mark.parametrize("variant,name", [(1, "row-owner"), (2, "column-window-blocked")])
def test_both_block_kernels(hip, variant, name):
    Hh = gapped_csr_host(N, 16, seed=7)
    H = hip.HipCsrOperator.from_scipy(Hh)
    H.set_block_variant(variant)
    for k in (8, 3):
        _check_block(hip, "g4000", Hh, H, _columns8()[:k], pc.SIGMA, 1e-10)
        assert H.block_info()["variant"] == name


# ---------------------------------------------------------------- 3. two sweep launches
@pytest.mark.parametrize("k", [8, 3])
def test_two_sweep_launches(hip, monkeypatch, k):
    """The geometry of test_gpu_block_two_launches.py: 8-row blocks, more of them than CUs, so the window-blocked sweep takes
    a second launch, whose partials lie behind the first's.  A wrong offset there breaks alfa in iteration 1."""
    monkeypatch.setenv("HIPEIG_BCOO_RW", "8")
    monkeypatch.setenv("HIPEIG_BCOO_WBITS", "9")
    Hh = gapped_csr_host(N, 16, seed=7)
    H = hip.HipCsrOperator.from_scipy(Hh)
    H.set_block_variant(2)
    _check_block(hip, "g4000", Hh, H, _columns8()[:k], pc.SIGMA, 1e-10)
    info = H.block_info()
    assert info["variant"] == "column-window-blocked"
    assert info["rows_per_block"] == 8
    assert info["row_blocks"] > H.ctx.device_info()["cus"]


# ---------------------------------------------------------------- 4. odd length and the floor
def test_odd_length_with_an_exact_diagonal_hit(hip):
    """n = 4001, one h_ii == sigma exactly (the floor of M) and one stored zero; k = 5 is the 8-wide interleave with padding."""
    Hh = pc.exact_hit_operator()[0]
    cols = [pc.unit_guess(4001)] + _unit_rows(5, 4, 4001, 4)
    counts = _check_block(hip, "hit4001", Hh, hip.HipCsrOperator.from_scipy(Hh), cols, pc.SIGMA, 1e-10)
    assert counts == [20] * 5


# ---------------------------------------------------------------- 5. less than one workgroup
def test_smaller_than_one_workgroup_on_the_dense_matrix(hip):
    A = pc.dense_operator()
    cols = _unit_rows(11, 3, 100, 3)
    counts = _check_block(hip, "dense100", A, hip.HipCsrOperator.from_dense(A), cols, -20.0, 1e-10)
    assert counts == [34, 35, 35]


# ---------------------------------------------------------------- 6. iteration limit
def test_iteration_limit(hip, gapped16):
    Hh, H = gapped16
    cols = _columns8()[:7]
    vecs = [hip.HipVector(c.copy(), _opts(5, 1e-10)) for c in cols]
    with pytest.raises(UserWarning, match="not converged"):
        hip.HipVector.solveBlock(H, vecs, pc.SIGMA)
    assert all(v.last_solve_stats["iterations"] == 5 and v.last_solve_stats["istop"] == 6 for v in vecs)
    # through the C entry
    ctx, k = vecs[0].ctx, len(vecs)
    outs = [ctx.alloc(N) for _ in vecs]
    bt, keep1 = _ptr_table([v._buf for v in vecs])
    xt, keep2 = _ptr_table(outs)
    info = (C.c_int * k)()
    stats = (C.c_double * (8 * k))()
    _lib.call("hipeig_minres_block_jacobi", ctx.handle, H.handle, pc.SIGMA, 1.0, k, bt, H.jacobi_inverse(pc.SIGMA).ptr, xt,
              1e-10, 5, info, stats)
    assert [info[j] for j in range(k)] == [5] * k
    assert [int(stats[8 * j + 1]) for j in range(k)] == [6] * k and [int(stats[8 * j]) for j in range(k)] == [5] * k


# ---------------------------------------------------------------- 7. chunk independence
def test_chunk_independence(hip, gapped16, monkeypatch):
    """The host looks at the records every HIPEIG_PMRB_CHUNK iterations; kernels enqueued past a column's stop leave it
    alone, so a look per iteration and the default give the same bits."""
    Hh, H = gapped16
    out = []
    for chunk in (None, "1"):
        monkeypatch.delenv("HIPEIG_PMRB_CHUNK", raising=False)
        if chunk:
            monkeypatch.setenv("HIPEIG_PMRB_CHUNK", chunk)
        X, _ = _solve(hip, H, _columns8(), pc.SIGMA, 1e-10)
        out.append([(x.array, x.last_solve_stats) for x in X])
    monkeypatch.delenv("HIPEIG_PMRB_CHUNK", raising=False)
    for (x0, s0), (x1, s1) in zip(*out):
        assert s0 == s1
        np.testing.assert_array_equal(x0, x1)


# ---------------------------------------------------------------- 8. neighbours untouched
def _neighbour_calls(hip, ctx):
    Hh = gapped_csr_host(N, 16, seed=7)
    H = hip.HipCsrOperator.from_scipy(Hh, ctx=ctx)
    Hx = pc.exact_hit_operator()[0]                                  # n = 4001: the seven plain blocks grow and move
    X = hip.HipCsrOperator.from_scipy(Hx, ctx=ctx)
    cols = _columns8()[:5]
    colsx = [pc.unit_guess(4001)] + _unit_rows(5, 4, 4001, 4)
    return {
        "plain block": lambda: [x.array for x in _solve(hip, H, cols, pc.SIGMA, 1e-8, ctx=ctx, pre=None, lock=None)[0]],
        "lock step": lambda: [x.array for x in _solve(hip, X, colsx, pc.SIGMA, 1e-10, ctx=ctx)[0]],
        "plain single": lambda: [hip.HipVector.solve(H, hip.HipVector(cols[1].copy(), _opts(2000, 1e-8, pre=None, lock=None), ctx=ctx),
                                                     pc.SIGMA).array],
    }


def test_neighbours_untouched(hip):
    """plain block -> lock-step Jacobi block -> plain block -> plain single on ONE context: the plain results are, bit
    for bit, those of the same calls on a fresh context."""
    fresh = {name: _neighbour_calls(hip, hip.HipContext(0))[name]() for name in ("plain block", "plain single")}
    calls = _neighbour_calls(hip, hip.HipContext(0))
    for name in ("plain block", "lock step", "plain block", "plain single"):
        got = calls[name]()
        assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in got)
        if name in fresh:
            assert len(got) == len(fresh[name])
            for g, r in zip(got, fresh[name]):
                np.testing.assert_array_equal(g, r)


@pytest.mark.parametrize("lock", [None, False])
def test_without_the_key_the_one_by_one_solves_run(hip, gapped16, lock):
    Hh, H = gapped16
    cols = _columns8()[:4]
    singles = [hip.HipVector.solve(H, hip.HipVector(c.copy(), _opts(2000, 1e-10, lock=None)), pc.SIGMA) for c in cols]
    block, _ = _solve(hip, H, cols, pc.SIGMA, 1e-10, lock=lock)
    for s, x in zip(singles, block):
        assert x.last_solve_stats == s.last_solve_stats and "lockStep" not in x.last_solve_stats
        np.testing.assert_array_equal(x.array, s.array)


# ---------------------------------------------------------------- 9. dispatch and refusals
def test_dispatch_and_refusals(hip, gapped16):
    Hh, H = gapped16
    cols = _columns8()[:3]
    with pytest.raises(ValueError, match="preconditionerLockStep"):
        _solve(hip, H, cols, pc.SIGMA, 1e-10, pre=None)
    with pytest.raises(ValueError, match="preconditionerLockStep"):
        hip.HipVector.solve(H, hip.HipVector(cols[0].copy(), _opts(pre=None)), pc.SIGMA)
    for bad in (1, "yes"):
        with pytest.raises(ValueError, match="bool"):
            hip.HipVector.solveBlock(H, [hip.HipVector(c.copy(), _opts(preconditionerLockStep=bad)) for c in cols], pc.SIGMA)
    # fewer right-hand sides than BLOCK_SOLVE_MIN, and a sequence of shifts: the one-by-one solves
    assert hip.HipVector.BLOCK_SOLVE_MIN == 3
    two, _ = _solve(hip, H, cols[:2], pc.SIGMA, 1e-10)
    seq, _ = _solve(hip, H, cols, [pc.SIGMA] * 3, 1e-10)
    singles = [hip.HipVector.solve(H, hip.HipVector(c.copy(), _opts(2000, 1e-10)), pc.SIGMA) for c in cols]
    for x, s in zip(two + seq, singles[:2] + singles):
        assert "lockStep" not in x.last_solve_stats and x.last_solve_stats == s.last_solve_stats
        np.testing.assert_array_equal(x.array, s.array)
    # the single solve's refusals
    vecs = [hip.HipVector(c.copy(), _opts()) for c in cols]
    with pytest.raises(NotImplementedError, match="x0"):
        hip.HipVector.solveBlock(H, vecs, pc.SIGMA, x0=hip.HipVector(cols[0].copy()))
    ctx = hip.HipContext()
    ctx._force_collectives = True                            # what attaching a communicator under HIPEIG_FORCE_COLLECTIVES leaves
    assert ctx.collectives
    with pytest.raises(NotImplementedError, match="one GPU"):
        hip.HipVector.solveBlock(hip.HipCsrOperator.from_scipy(Hh, ctx=ctx),
                                 [hip.HipVector(c.copy(), _opts(), ctx=ctx) for c in cols], pc.SIGMA)


# ---------------------------------------------------------------- 10. the driver
def test_lanczos_driver_with_a_block_of_three(hip, monkeypatch):
    """inexactLanczosDiagonalization needs no change: the option travels with the vectors.  A block of 3 on the gapped
    N = 4000 operator with the Jacobi key alone (one-by-one solves) and with both keys (lock step); the bound on the Ritz
    value is that of test_gpu_precond_minres.py::test_lanczos_driver_with_and_without_the_key, exact eigenvalues from the
    dense matrix.  L = 12: four blocks of three (the oracle converges with these arguments in 11 iterations)."""
    import scipy.linalg as la
    sigma = pc.SIGMA
    Hh = gapped_csr_host(N, 32, seed=7)
    lam = np.linalg.eigvalsh(Hh.toarray())
    exact = lam[np.argmin(np.abs(lam - sigma))]
    Hd = hip.HipCsrOperator.generate(N, 32, seed=7)
    Q = la.qr(np.stack([guess_vector(N, s) for s in (1, 2, 3)], axis=1), mode="economic")[0]
    seen = []
    real_block = hip.HipVector.solveBlock

    def recording(H, bs, s, *a, **k):
        xs = real_block(H, bs, s, *a, **k)
        seen.extend(x.last_solve_stats for x in xs)
        return xs

    monkeypatch.setattr(hip.HipVector, "solveBlock", staticmethod(recording))
    err = {}
    for lock in (None, True):
        seen.clear()
        v0 = [hip.HipVector(Q[:, j].copy(), _opts(2000, 1e-10, lock=lock)) for j in range(3)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ev, Y, st = hip.inexactLanczosDiagonalization(Hd, v0, sigma, 12, 10, 1e-13, writeOut=False)
        assert st["isConverged"]
        assert len(seen) >= 6 and all(s["preconditioner"] == "jacobi" for s in seen)
        assert all(s.get("lockStep") is (True if lock else None) for s in seen)
        near = ev[np.argmin(np.abs(np.asarray(ev) - exact))]
        err[lock] = abs(near - exact)
        print(f"LANCZOS block 3 lockStep={lock}: theta {near:.15f} exact {exact:.15f} error {err[lock]:.2e}, {len(seen)} solves, "
              f"{sum(s['iterations'] for s in seen)} inner iterations")
    assert err[True] <= max(10 * err[None], 1e-10 * abs(exact))
