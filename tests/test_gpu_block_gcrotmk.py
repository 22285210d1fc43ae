"""Lock-step GCROT solves with a REAL shift (HipVector.solveBlock -> _solve_real_block): the shifted block product
hipeig_spmm_shift, the real split / batched Arnoldi steps, and the solves and block Lanczos runs built on them.

The block Lanczos of the reference (inexact_Lanczos.py:319-320) solves the nBlock right-hand sides of an iteration on one
operator and one real shift; with linearSolver="gcrotmk" (the reference's own choice in every unit test) those solves now
advance together: one pass over the operator per block of products, the Arnoldi steps enqueued back to back.

Block product row bound (u = 2^-53, as asked of every product here): |y_i - y*_i| <= 1e-14 (|sigma| |x_i| + (|A| |x|)_i),
with y* the product in extended precision (tests/_hiprec.py).  Against hipeig_spmv_shift the shift term is rounded the
same way, so the two may differ only through the operator sum: by at most 1e-14 (|A| |x|)_i, and not at all on an
empty row."""
import ctypes as C
import gc
import os
import warnings

import numpy as np
import pytest
import scipy.linalg as la
import scipy.sparse as sp

import _hiprec as hp
from _product_cases import ragged_csr as _ragged_csr
from conftest import load_golden
from eigensolvers_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
PP = C.POINTER(C.c_void_p)


def _up(ctx, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    buf = ctx.alloc(a.size)
    _lib.call("hipeig_vec_upload", ctx.handle, buf.ptr, a.ctypes.data_as(C.c_void_p), a.size)
    return buf


def _down(ctx, buf):
    out = np.empty(buf.n)
    _lib.call("hipeig_vec_download", ctx.handle, out.ctypes.data_as(C.c_void_p), buf.ptr, buf.n)
    return out


def _gcrot_opts(it=3000, tol=1e-8, atol=1e-12, **extra):
    d = {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": it, "linear_tol": tol, "linear_atol": atol}}
    d.update(extra)
    return d


# ---------------------------------------------------------------- the shifted block product
def _check_shift_block(hip, ctx, H, csr, X, ks, sigma, variants, expect_auto):
    rowptr, col, val = csr
    n = len(rowptr) - 1
    Xd = [_up(ctx, x) for x in X]
    ref = []
    for x in X:
        ax, absax, _ = hp.csr_matvec(rowptr, col, val, x)
        xw = np.asarray(x, dtype=np.longdouble)
        ref.append((np.longdouble(sigma) * xw - ax, 1e-14 * (abs(sigma) * np.abs(x) + absax.astype(np.float64)),
                    1e-14 * absax.astype(np.float64)))
    empty = np.diff(rowptr) == 0
    singles = {}
    for sign in (1.0, -1.0):
        for j, x in enumerate(Xd):                          # hipeig_spmv_shift, column by column
            y = ctx.alloc(n)
            H.apply_shifted(sigma, x, y, reverse=sign < 0)
            singles[(sign, j)] = _down(ctx, y)
    for bv in variants:
        H.set_block_variant(bv)
        for k in ks:
            for sign in (1.0, -1.0):
                Y = H.apply_shifted_block(sigma, Xd[:k], reverse=sign < 0)
                if bv == 0:
                    assert H.block_info()["variant"] == expect_auto
                for j in range(k):
                    y = _down(ctx, Y[j])
                    yr, bound, bound_sum = ref[j]
                    err = np.abs(y.astype(np.longdouble) - np.longdouble(sign) * yr).astype(np.float64)
                    assert np.all(err <= bound), (f"variant {bv} k={k} sign={sign} column {j}: error / bound "
                                                  f"{float(np.max(err / bound)):.3g}")
                    d = np.abs(y - singles[(sign, j)])
                    assert np.all(d <= bound_sum), f"variant {bv} k={k} sign={sign} column {j}: differs beyond the operator sum"
                    np.testing.assert_array_equal(y[empty], singles[(sign, j)][empty])
    H.set_block_variant(0)


def test_shift_block_product_on_a_ragged_operator(hip):
    """k = 1 .. 11 operands (4-wide, 8-wide and 8 + remainder chunks), sign +-1, both block kernels and the automatic
    choice (row-owner here: the operand block fits one L2), odd N, empty / long / unsorted rows."""
    ctx = hip.HipContext.default()
    n = 3001
    csr = _ragged_csr(n, 11)
    H = hip.HipCsrOperator.from_csr_arrays(*csr, n)
    X = np.random.default_rng(3).standard_normal((11, n)) * np.exp(np.random.default_rng(4).uniform(-2, 2, (11, n)))
    _check_shift_block(hip, ctx, H, csr, X, range(1, 12), 0.37, (0, 1, 2), "row-owner")


def test_shift_block_product_on_a_window_blocked_operator(hip):
    """An operator large enough for the automatic choice to take the window-blocked kernel (fp64 LDS atomics: any order
    of the adds), odd N; and the same operator pinned to the row-owner kernel."""
    ctx = hip.HipContext.default()
    n = 100_003
    H = hip.HipCsrOperator.generate(n, 32, seed=7)
    A = H.to_scipy().tocsr()
    csr = (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data)
    X = np.random.default_rng(5).standard_normal((11, n))
    _check_shift_block(hip, ctx, H, csr, X, (1, 3, 4, 5, 8, 11), 0.02, (0,), "column-window-blocked")
    _check_shift_block(hip, ctx, H, csr, X, (8, 11), 0.02, (1,), None)


def test_shift_block_product_rejects_a_bad_sign(hip):
    ctx = hip.HipContext.default()
    H = hip.HipCsrOperator.generate(1000, 8, seed=7)
    x = _up(ctx, np.ones(1000))
    y = ctx.alloc(1000)
    xt = (C.c_void_p * 1)(x.ptr)
    yt = (C.c_void_p * 1)(y.ptr)
    with pytest.raises(_lib.HipEigError, match="sign"):
        _lib.call("hipeig_spmm_shift", ctx.handle, H.handle, 1, 0.1, 0.5, C.cast(xt, PP), C.cast(yt, PP))


# ---------------------------------------------------------------- real split and batched Arnoldi steps
def _orthonormal(rng, n, m):
    Q = rng.standard_normal((m, n))
    for _ in range(2):
        if m:
            Q = np.linalg.solve(np.linalg.cholesky(Q @ Q.T), Q)
    return np.ascontiguousarray(Q)


def _steps(rng, n, ms):
    out = []
    for s, m in enumerate(ms):
        if m > n // 2:
            V = rng.standard_normal((m, n))
            V /= np.linalg.norm(V, axis=1, keepdims=True)
        else:
            V = _orthonormal(rng, n, m)
        w = (V.T @ rng.standard_normal(m) if m else 0.0) + (1.0, 1e-4, 1e-8)[s % 3] * rng.standard_normal(n)
        out.append((V, w))
    return out


def _within_reference(got, V, w):
    """The forward-error bound of tests/test_gpu_orthogonalisation.py (c = 64 + 4m) for one real step."""
    nb, h, na, wo = got
    nb_r, h_r, na_r, w_r = hp.mgs(V, w)
    m = len(h_r)
    c = 64 + 4 * m
    vn = np.array([float(hp.nrm2(v)) for v in V])
    prefix = float(nb_r) + np.concatenate([[0.0], np.cumsum(np.abs(h_r.astype(np.float64)) * vn[:m])])
    S = prefix[m]
    if m:
        assert np.all(np.abs(np.asarray(h).astype(np.longdouble) - h_r).astype(np.float64) <= c * U * vn * prefix[:m])
    assert abs(nb - float(nb_r)) <= c * U * float(nb_r)
    assert abs(na - float(na_r)) <= c * U * S
    assert float(hp.nrm2(np.asarray(wo).astype(np.longdouble) - w_r)) <= c * U * S / float(na_r)


@pytest.mark.parametrize("cols", [1, 4])
def test_real_split_steps_on_side_streams(hip, monkeypatch, cols):
    """hipeig_arnoldi_step_begin / hipeig_arnoldi_step_end as the lock-step driver calls them: 16 slots begun before any
    is collected (8 side streams: slots s and s + 8 share one), 0 .. SPLIT_MAX_COLS columns, n > 8192.  Bit for bit the
    step hipeig_arnoldi_step_p runs on the compute stream, bit for bit the same with 1 and 8 side streams, within the
    high-precision reference's bound, and a product enqueued right after end(slot) reads the finished w."""
    from eigensolvers_amd.gcrotmk import _Ops
    n = 100_003
    ms = [0, 1, 3, 4, 5, 9, 13, 28, 40, 61, 64, 65, 99, _Ops.SPLIT_MAX_COLS]
    ms = (ms + ms)[:16]
    slots = _steps(np.random.default_rng(77), n, ms)
    results = {}
    for ns in (1, 8):
        monkeypatch.setenv("HIPEIG_ARNOLDI_STREAMS", str(ns))
        ctx = hip.HipContext()
        H = hip.HipCsrOperator.generate(n, 32, seed=7, ctx=ctx)
        H.set_variant(2)                              # a bitwise reproducible product
        opss = [_Ops(ctx, n, cols) for _ in slots]
        dev = [([_up(ctx, v) for v in V], _up(ctx, w)) for V, w in slots]
        ys = [ctx.alloc(n) for _ in slots]
        for s, (Vd, wd) in enumerate(dev):
            opss[s].arnoldi_begin(Vd, wd, s)
        scal = []
        for s, (Vd, wd) in enumerate(dev):
            scal.append(opss[s].arnoldi_end(len(Vd), s))
            H.apply_shifted(0.02, wd, ys[s])          # compute stream, no wait but end(s)
        out = []
        for s, (Vd, wd) in enumerate(dev):
            wv = _down(ctx, wd)
            y2 = ctx.alloc(n)
            H.apply_shifted(0.02, _up(ctx, wv), y2)
            np.testing.assert_array_equal(_down(ctx, ys[s]), _down(ctx, y2), err_msg=f"streams={ns} slot {s}: product read w early")
            out.append((scal[s][0], np.array(scal[s][1]), scal[s][2], wv))
        results[ns] = out
        if ns == 8:
            for s, (V, w) in enumerate(slots):
                Vd, _ = dev[s]
                wd = _up(ctx, w)
                nb, h, na = opss[s].arnoldi_step(Vd, wd)
                assert nb == out[s][0] and na == out[s][2], f"slot {s}: norms differ from the compute-stream step"
                np.testing.assert_array_equal(h, out[s][1], err_msg=f"slot {s}: coefficients")
                np.testing.assert_array_equal(_down(ctx, wd), out[s][3], err_msg=f"slot {s}: w")
        del H, opss, dev, ys
        ctx.synchronize()
        del ctx
        gc.collect()
    for s, (V, w) in enumerate(slots):
        a, b = results[1][s], results[8][s]
        assert a[0] == b[0] and a[2] == b[2], f"slot {s}: norms differ between 1 and 8 side streams"
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[3], b[3])
        _within_reference(b, V, w)


@pytest.mark.parametrize("n", [37, 4000, 8191, 8192])
def test_real_batched_steps(hip, n):
    """hipeig_arnoldi_step_batch_begin: 16 real steps of up to 64 columns in one launch, a workgroup each.  Where the
    single step is one workgroup too (the default at these lengths) the batch is it bit for bit; every step is within
    the high-precision reference's bound.  Longer vectors are declined (status 5, nothing done)."""
    from eigensolvers_amd.gcrotmk import _Ops
    ctx = hip.HipContext.default()
    ms = [0, 1, 2, 3, 4, 5, 7, 8, 9, 13, 20, 28, 40, 47, 61, _Ops.BATCH_MAX_COLS]
    steps = _steps(np.random.default_rng(n), n, ms)
    opss = [_Ops(ctx, n) for _ in steps]
    reqs = [([_up(ctx, v) for v in V], _up(ctx, w)) for V, w in steps]
    if os.environ.get("HIPEIG_MAPPED_SCALARS") == "0":
        assert not _Ops.arnoldi_begin_batch(opss, reqs)        # declined without the mapped scalar area
        return
    assert _Ops.arnoldi_begin_batch(opss, reqs)
    got = [opss[s].arnoldi_end(len(Vd), s) + (_down(ctx, wd),) for s, (Vd, wd) in enumerate(reqs)]
    single_is_one_wg = os.environ.get("HIPEIG_ARNOLDI_SMALL") != "0"
    for s, (V, w) in enumerate(steps):
        nb, h, na, wo = got[s]
        _within_reference((nb, h, na, wo), V, w)
        if single_is_one_wg:
            Vd = reqs[s][0]
            wd = _up(ctx, w)
            nb1, h1, na1 = opss[s].arnoldi_step(Vd, wd)
            assert nb1 == nb and na1 == na, f"step {s}: norms differ from the single step"
            np.testing.assert_array_equal(h1, h, err_msg=f"step {s}: coefficients")
            np.testing.assert_array_equal(_down(ctx, wd), wo, err_msg=f"step {s}: w")
    big = _Ops(ctx, 8193)
    wbig = ctx.alloc(8193)
    assert _Ops.arnoldi_begin_batch([big, big], [([], wbig), ([], wbig)]) is False


# ---------------------------------------------------------------- lock-step solves
@pytest.mark.parametrize("case", ["generate200k", "gapped4000"])
def test_real_shift_lock_step_is_the_one_by_one_solve_bit_for_bit(hip, gapped4000, case):
    """The lock-step solves against one-by-one device GCROT solves that apply the SAME product kernel: the row-owner
    block kernel, whose sum for a column depends only on the interleave width and on that column (blocks of <= 4 operands
    always take width 4, whatever else is in the block).  Every other piece - the split steps on the compute stream at
    N = 200k, the one-launch batch at N = 4000, dots, norms, combinations - is the single solve's kernel, so solutions,
    product counts and outer iterations are identical, bit for bit.  sigma = 0.02, ~6000 products per solve."""
    from eigensolvers_amd.gcrotmk import gcrotmk_device
    sigma = 0.02
    if case == "gapped4000":
        H = hip.HipCsrOperator.from_scipy(gapped4000[0])
        nrhs = 3
    else:
        H = hip.HipCsrOperator.generate(200_000, 32, seed=7)
        nrhs = hip.hip_vector.BLOCK_SOLVE_MIN_GCROT_LONG
    assert nrhs <= 4
    H.set_block_variant(1)
    N = H.nrows
    rng = np.random.default_rng(21)
    B = rng.standard_normal((nrhs, N))
    B /= np.linalg.norm(B, axis=1, keepdims=True)
    o = _gcrot_opts()
    ctx = hip.HipContext.default()
    bs = [hip.HipVector(b.copy(), o) for b in B]
    blk = hip.HipVector.solveBlock(H, bs, sigma)
    for b, wb in zip(bs, blk):
        x, info, st = gcrotmk_device(ctx, lambda v: H.apply_shifted_block(sigma, [v])[0], b._buf, N, rtol=1e-8, atol=1e-12,
                                     maxiter=3000)
        assert info == 0 and wb.last_solve_stats["lock_step"] is True
        assert wb.last_solve_stats["iterations"] == st["matvecs"] and wb.last_solve_stats["outer"] == st["outer"]
        np.testing.assert_array_equal(wb.array, hip.HipVector(x).array)


def test_real_shift_solves_in_lock_step_equal_the_single_solves(hip):
    """solveBlock with gcrotmk and a real shift runs the solves in lock step (block products, split Arnoldi steps); each
    right-hand side gets the solution of HipVector.solve to the solve tolerance, a true residual below the tolerance and
    ``lock_step`` in its stats; reverseGF gives -x; blockSolve = False is HipVector.solve bit for bit.

    The product COUNTS are compared exactly in the test above, against one-by-one solves on the same product kernel.
    Against HipVector.solve - a different kernel, other last bits in every product - they are not: sigma = 0.02 sits next
    to the operator's eigenvalue cluster, a solve takes ~6000 products (~150 restarted GCROT cycles), and over that many
    cycles the count follows the last bits of the products (10-15 % either way here).  The solutions agree to 1e-6 in norm
    (||b|| = 1: rtol 1e-8 times the condition at this shift).  The operator runs with reproducible kernels (reduction
    "deterministic") so that the comparison is the same on every run."""
    N, sigma = 200_000, 0.02
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    assert H.block_info()["variant"] == "none"
    rng = np.random.default_rng(2)
    B = rng.standard_normal((6, N))
    B /= np.linalg.norm(B, axis=1, keepdims=True)
    o = _gcrot_opts(reduction="deterministic")
    bs = [hip.HipVector(b.copy(), o) for b in B]
    one = [hip.HipVector.solve(H, b, sigma) for b in bs]
    assert H.block_info()["variant"] == "none"
    blk = hip.HipVector.solveBlock(H, bs, sigma)
    assert H.block_info()["variant"] != "none"                  # the solves issued block products
    ctx = hip.HipContext.default()
    for b, w1, wb in zip(bs, one, blk):
        assert isinstance(wb, hip.HipVector) and wb.last_solve_stats["lock_step"] is True
        assert b.last_solve_stats is wb.last_solve_stats
        a1, ab = w1.array, wb.array
        assert np.linalg.norm(ab - a1) <= 1e-6                  # ||b|| = 1; rtol 1e-8 times the condition at this shift
        r = ctx.alloc(N)                                        # true residual of the lock-step solution
        H.apply_shifted(sigma, wb._buf, r)
        assert np.linalg.norm(hip.HipVector(r).array - b.array) <= 1e-8 * 1.0001
    rev = hip.HipVector.solveBlock(H, bs, sigma, reverseGF=True)
    for wb, wr in zip(blk, rev):
        assert wr.last_solve_stats["lock_step"] is True
        assert np.linalg.norm(wr.array + wb.array) <= 1e-6
    # blockSolve = False: the one-by-one solves, bit for bit
    bs2 = [hip.HipVector(b.copy(), _gcrot_opts(reduction="deterministic", blockSolve=False)) for b in B[:3]]
    got = hip.HipVector.solveBlock(H, bs2, sigma)
    for g, w1 in zip(got, one):
        np.testing.assert_array_equal(g.array, w1.array)
        assert "lock_step" not in g.last_solve_stats


def test_real_shift_lock_step_with_cols_per_pass_four(hip):
    """arnoldiColumnsPerPass = 4 is honoured, on the default (fastest) kernels: both paths take the blocked Arnoldi
    sweep, every solution has a true residual below the tolerance, and the two agree to what that tolerance allows at
    this shift (cond * rtol: 1e-5 relative)."""
    N, sigma = 100_000, 0.02
    H = hip.HipCsrOperator.generate(N, 32, seed=7)
    rng = np.random.default_rng(9)
    o = _gcrot_opts(arnoldiColumnsPerPass=4)
    bs = [hip.HipVector(rng.standard_normal(N), o) for _ in range(4)]
    for b in bs:
        b.normalize()
    one = [hip.HipVector.solve(H, b, sigma) for b in bs]
    blk = hip.HipVector.solveBlock(H, bs, sigma)
    assert H.block_info()["variant"] == "column-window-blocked"
    ctx = hip.HipContext.default()
    for b, w1, wb in zip(bs, one, blk):
        assert wb.last_solve_stats["lock_step"] is True and "lock_step" not in w1.last_solve_stats
        assert np.linalg.norm(wb.array - w1.array) <= 1e-5 * np.linalg.norm(w1.array)
        for w in (w1, wb):
            r = ctx.alloc(N)
            H.apply_shifted(sigma, w._buf, r)
            assert np.linalg.norm(hip.HipVector(r).array - b.array) <= 1e-8 * 1.0001
    # fewer than BLOCK_SOLVE_MIN_GCROT_LONG right-hand sides of this length: the one-by-one solves
    few = hip.HipVector.solveBlock(H, bs[:hip.hip_vector.BLOCK_SOLVE_MIN_GCROT_LONG - 1], sigma)
    assert all("lock_step" not in w.last_solve_stats for w in few)


def test_non_converging_column_raises_after_every_solve_ran(hip):
    """One right-hand side of the block cannot converge in the outer iterations allowed, the others can (unit vectors
    of a diagonal operator: one product each): UserWarning, raised once all solves have run - every vector's stats set,
    and the converged ones those of their single solves."""
    n, sigma = 20_000, 0.0123
    d = np.linspace(-1.0, 1.0, n)
    H = hip.HipCsrOperator.from_scipy(sp.diags(d).tocsr())
    o = _gcrot_opts(it=2, tol=1e-10, atol=0.0)
    cols = []
    for k in (5, 777, 12_345):
        e = np.zeros(n)
        e[k] = 1.0
        cols.append(e)
    cols.insert(1, np.random.default_rng(1).standard_normal(n))
    bs = [hip.HipVector(c.copy(), o) for c in cols]
    with pytest.raises(UserWarning, match="not converged"):
        hip.HipVector.solveBlock(H, bs, sigma)
    for i, (b, c) in enumerate(zip(bs, cols)):
        st = b.last_solve_stats
        assert st is not None and st["lock_step"] is True
        if i != 1:
            w1 = hip.HipVector.solve(H, hip.HipVector(c.copy(), o), sigma)
            assert st["iterations"] == w1.last_solve_stats["iterations"] and st["outer"] == w1.last_solve_stats["outer"]
    with pytest.raises(UserWarning):
        hip.HipVector.solve(H, hip.HipVector(cols[1].copy(), o), sigma)


def test_collective_context_solves_one_by_one(hip, gapped4000, monkeypatch):
    """A one-rank communicator rehearsing the row-partitioned path (HIPEIG_FORCE_COLLECTIVES=1): products and reductions
    go through the collectives, which the split Arnoldi steps do not take - solveBlock solves one by one there, for a real
    and for a complex shift, instead of failing."""
    from eigensolvers_amd.distributed import LoopbackGroup
    monkeypatch.setenv("HIPEIG_FORCE_COLLECTIVES", "1")
    Hh, _ = gapped4000
    B = np.random.default_rng(4).standard_normal((2, 4000))
    B /= np.linalg.norm(B, axis=1, keepdims=True)
    grp = LoopbackGroup(1)

    def body(rank, ctx):
        assert ctx.collectives
        H = hip.HipCsrOperator.from_scipy(Hh, ctx=ctx)
        o = _gcrot_opts(tol=1e-6)
        real = hip.HipVector.solveBlock(H, [hip.HipVector(b.copy(), o, ctx=ctx) for b in B], 0.02)
        cplx = hip.HipVector.solveBlock(H, [hip.HipVector(b.copy(), o, ctx=ctx) for b in B], 0.02 + 0.05j)
        return [w.array for w in real], [w.last_solve_stats for w in real + cplx]

    try:
        (xs, stats), = grp.run(body)
    finally:
        grp.close()
    assert all("lock_step" not in st for st in stats)
    for b, x in zip(B, xs):
        assert np.linalg.norm(b - (0.02 * x - Hh @ x)) <= 1e-6 * 1.0001


# ---------------------------------------------------------------- block Lanczos through the lock-step solves
def test_reference_block3_run_takes_the_lock_step_path(hip, monkeypatch):
    """unittests/test_lanczosBlock.py as the reference runs it (dense n = 100, 3-fold degenerate level, nBlock = 3,
    gcrotmk rtol 1e-4) through the lock-step solves: the golden's cumIter, eigenvalues to 1e-6, the projector trace."""
    from eigensolvers_amd.generators import dense_test_matrix
    calls = []
    real = hip.HipVector._solve_real_block

    def counted(*a, **kw):
        calls.append(len(a[1]))
        return real(*a, **kw)

    monkeypatch.setattr(hip.HipVector, "_solve_real_block", staticmethod(counted))
    opt = lambda: {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 1000, "linear_tol": 1e-4}}
    gb = load_golden("block3_degenerate.npz")
    Ab, _ = dense_test_matrix(100, 1212, gb["exact"])
    v0 = [hip.HipVector(gb["guess"][:, i].copy(), opt()) for i in range(3)]
    ev, Y, st = hip.inexactLanczosDiagonalization(hip.HipCsrOperator.from_dense(Ab), v0, gb["exact"][5] + 1.5, 6, 4, 1e-6,
                                                  writeOut=False)
    assert calls and all(c == 3 for c in calls)
    assert st["cumIter"] == int(gb["cumIter"])
    np.testing.assert_allclose(ev[:3], gb["exact"][5:8], rtol=1e-6)
    w, V = np.linalg.eigh(Ab)
    lan = np.vstack([Y[i].array for i in range(3)]).T
    assert abs(np.abs(la.eigvals(lan.T @ V[:, 5:8])).sum() - 3) < 1e-6


def test_block8_gcrotmk_lanczos_lock_step_equals_one_by_one(hip, gapped4000):
    """Block-8 Lanczos on the gapped N = 4000 operator with gcrotmk: lock-step solves against blockSolve = False - the
    same cumulative iteration count, eigenvalues to 1e-10."""
    Hh, _ = gapped4000
    g = load_golden("gapped_csr_n4000_block8.npz")
    H = hip.HipCsrOperator.from_scipy(Hh)
    Q = la.qr(np.random.default_rng(5).standard_normal((4000, 8)), mode="economic")[0]
    runs = {}
    for block_solve in (True, False):
        v0 = [hip.HipVector(Q[:, i].copy(), _gcrot_opts(2000, 1e-10, 1e-12, blockSolve=block_solve)) for i in range(8)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ev, Y, st = hip.inexactLanczosDiagonalization(H, v0, 0.02, int(g["L"]), int(g["maxit"]), float(g["eConv"]),
                                                         writeOut=False)
        runs[block_solve] = (ev, st)
    (e1, s1), (e0, s0) = runs[True], runs[False]
    assert s1["cumIter"] == s0["cumIter"] and bool(s1["isConverged"]) == bool(s0["isConverged"])
    np.testing.assert_allclose(np.sort(e1[:8]), np.sort(e0[:8]), rtol=1e-10, atol=0)
