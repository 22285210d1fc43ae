"""The orthogonalisation kernels of the complex GCROT solves, and the block complex-shift product that feeds them,
against a high-precision reference (tests/_hiprec.py: the same operations in extended precision).

Forward-error bounds, u = 2^-53.  For an Arnoldi step of m columns V_0 .. V_{m-1} applied to w (sequential modified
Gram-Schmidt, SciPy's _fgmres; starred quantities are the reference's):

    |h_k - h*_k|     <= c u ||V_k|| (||w|| + sum_{l<k} |h*_l| ||V_l||)
    |nb - nb*|       <= c u nb*                                   (nb = ||w|| before the sweep)
    |na - na*|       <= c u S,   S = ||w|| + sum_l |h*_l| ||V_l||   (na = ||w|| after the sweep)
    ||w_out - w*||   <= c u S / na*                               (w_out = w / na)

with c = 64 + 4m.  Why these hold: every element of w is updated by one (real) or two (complex) roundings per column,
so after k columns the computed w differs from the exact one by at most ~2u (||w|| + sum_{l<k} |h_l| ||V_l||) in norm
(plus what the earlier coefficients' errors carry along, of the same order: each column's update is a projector or
close to one here).  A dot product of length n summed as the kernels sum it - a per-thread run of e terms, then a
64-lane wave tree (6 levels), a 4- or 16-wave workgroup stage and a last stage over the workgroups' partials (8 lanes
of <= 32 partials in order, a 3-level tree; or g partials read in order by every thread of the sequential sweep's next
launch) - has a relative error (to the sum of the magnitudes) of at most (e + 6 + 4 + g/8 + 3) u; for the longest
vector here (n = 2^20 + 1, blocked form: 256 workgroups of 256 threads, 8 element pairs per thread, so e <= 32 fma
terms of the complex real part) that is about 80 u if every rounding went the same way, and a few u in practice
(rounding errors add like a random walk).  64 u covers the reduction, 4 u per column the accumulated updates and the
Gram-matrix recovery of the blocked form (h_k = <V_k, w> - sum_{l<k} h_l G_kl: k <= 3 more roundings, each relative to
|h_l| ||V_k|| ||V_l||).  The reference's own error is ~2^-64 log2(n) relative and does not count.

A block complex-shift product row y_i = sign (z x_i - (A x)_i) with len_i stored entries is held to
    |y_i - y*_i| <= (len_i + 4) u ((|A| |x|)_i + |z| |x_i|),
the textbook bound of a sum of len_i products in any order plus the epilogue's three roundings.  Row by row: a wrong
value on a short or small row fails here even where it is far below the largest row.

Every test prints the largest ratio error / bound it saw per group (``-s`` shows it): how much of the bound is used.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import _hiprec as hp
from eigensolvers_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ARN_P = 4
MS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 28, 40]         # every residue modulo ARN_P, and the sizes GCROT(20, 20) reaches
DELTAS = [1.0, 1e-4, 1e-8]                       # w = V a + delta r: delta = 1e-8 is GCROT near convergence
SPLIT_MAX_COLS = 62


# ---------------------------------------------------------------- device helpers (any context)
def _up(ctx, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    buf = ctx.alloc(a.size)
    _lib.call("hipeig_vec_upload", ctx.handle, buf.ptr, a.ctypes.data_as(C.c_void_p), a.size)
    return buf


def _down(ctx, buf):
    out = np.empty(buf.n)
    _lib.call("hipeig_vec_download", ctx.handle, out.ctypes.data_as(C.c_void_p), buf.ptr, buf.n)
    return out


def _up_cols(ctx, V, pair):
    return [(_up(ctx, v.real), _up(ctx, v.imag)) for v in V] if pair else [_up(ctx, v) for v in V]


def _up_w(ctx, w, pair):
    return (_up(ctx, w.real), _up(ctx, w.imag)) if pair else _up(ctx, w)


def _down_w(ctx, w, pair):
    return _down(ctx, w[0]) + 1j * _down(ctx, w[1]) if pair else _down(ctx, w)


class _Worst:
    """Largest ratio error / bound per group; asserts every ratio <= 1."""

    def __init__(self, name):
        self.name, self.ratio = name, {}

    def check(self, group, err, bound, what):
        err = np.asarray(err, dtype=np.float64)
        bound = np.asarray(bound, dtype=np.float64)
        r = float(np.max(err / bound)) if err.size else 0.0
        assert np.all(err <= bound), f"{self.name} {what}: error / bound = {r:.3g} (max error {float(np.max(err)):.3e})"
        self.ratio[group] = max(self.ratio.get(group, 0.0), r)

    def report(self):
        print(f"\n[{self.name}] largest error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.ratio.items())))


def _check_step(worst, group, what, got, ref, vnorms, normalised=True):
    """got = (nb, h, na, w_out) of the device, ref = hp.mgs(...) of the same inputs; bounds of the module docstring."""
    nb, h, na, w = got
    nb_r, h_r, na_r, w_r = ref
    m = len(h_r)
    c = 64 + 4 * m
    ah = np.abs(h_r.astype(np.clongdouble)).astype(np.float64)
    nb_r, na_r = float(nb_r), float(na_r)
    prefix = nb_r + np.concatenate([[0.0], np.cumsum(ah * vnorms[:m])])          # ||w|| + sum_{l<k} |h*_l| ||V_l||
    S = prefix[m]
    if m:
        err_h = np.abs(np.asarray(h, dtype=np.complex128).astype(np.clongdouble) - h_r)
        worst.check(group + " h", err_h, c * U * vnorms[:m] * prefix[:m], f"{what} h")
    worst.check(group + " nb", abs(nb - nb_r), c * U * nb_r, f"{what} nb")
    worst.check(group + " na", abs(na - na_r), c * U * S, f"{what} na")
    err_w = float(hp.nrm2(np.asarray(w, dtype=np.complex128).astype(np.clongdouble) - w_r))
    worst.check(group + " w", err_w, c * U * S / (na_r if normalised else 1.0), f"{what} w")


def _orthonormal(rng, n, m, pair):
    """m orthonormal rows of length n (Cholesky QR twice: as orthonormal as Householder QR for a random matrix, and
    much faster at n = 2^20)."""
    Q = rng.standard_normal((m, n)) + (1j * rng.standard_normal((m, n)) if pair else 0.0)
    for _ in range(2):
        if m:
            L = np.linalg.cholesky(Q @ Q.conj().T)                 # Q Q^H = L L^H
            Q = np.linalg.solve(L, Q)
    return np.ascontiguousarray(Q)


def _skewed(Q, pair):
    """Columns far from orthonormal, so that the Gram correction of the blocked form carries weight: V_1 (and V_5, in
    the second block of ARN_P) take a complex multiple of their neighbour (the imaginary Gram terms are exercised only
    by a complex coupling), V_2 is scaled by 1e-3."""
    V = Q.copy()
    cpl = (0.3 + 0.4j) if pair else 0.3
    V[1] += cpl * V[0]
    if len(V) > 5:
        V[5] += cpl * V[4]
    V[2] *= 1e-3
    return V


# ---------------------------------------------------------------- sequential and blocked steps
@pytest.mark.parametrize("n", [8191, 8192, 8193, 100_003, (1 << 20) + 1])
@pytest.mark.parametrize("pair", [False, True], ids=["real", "pair"])
def test_arnoldi_step_against_the_high_precision_reference(hip, pair, n):
    """hipeig_arnoldi_step_p / hipeig_pair_arnoldi_step_p with cols_per_pass 1 (the sequential sweep; one workgroup up to
    n = 8192) and 4 (the blocked form beyond it; odd n: the scalar tail of arnoldi_block_kernel), m over every residue of
    ARN_P: orthonormal V with w = V a + delta r (delta = 1e-8: almost all of w cancels), then skewed V."""
    from eigensolvers_amd.gcrotmk import _Ops, _PairOps
    ctx = hip.HipContext.default()
    rng = np.random.default_rng(n + 7 * pair)
    mmax = max(MS)
    Q = _orthonormal(rng, n, mmax, pair)
    ops = {cols: (_PairOps if pair else _Ops)(ctx, n, cols) for cols in (1, 4)}
    worst = _Worst(f"arnoldi {'pair' if pair else 'real'} n={n}")

    def rnd(size):
        return rng.standard_normal(size) + (1j * rng.standard_normal(size) if pair else 0.0)

    def run(Vd, w, m, cols):
        wd = _up_w(ctx, w, pair)
        nb, h, na = ops[cols].arnoldi_step(Vd[:m], wd)
        return nb, h, na, _down_w(ctx, wd, pair)

    Qd = _up_cols(ctx, Q, pair)
    for delta in DELTAS:
        for m in MS:
            w = (Q[:m].T @ rnd(m) if m else np.zeros(n, dtype=Q.dtype)) + delta * rnd(n)
            ref = hp.mgs(Q[:m], w)
            vn = np.linalg.norm(Q[:m], axis=1)
            for cols in (1, 4):
                _check_step(worst, f"orth cols={cols}", f"delta={delta} m={m} cols={cols}", run(Qd, w, m, cols), ref, vn)
    V = _skewed(Q, pair)
    Vd = _up_cols(ctx, V, pair)
    w = V.T @ rnd(mmax) + rnd(n)
    vn = np.array([float(hp.nrm2(v)) for v in V])
    got = {(m, cols): run(Vd, w, m, cols) for m in MS for cols in (1, 4)}
    for m, ref in hp.mgs(V, w, checkpoints=set(MS)).items():
        for cols in (1, 4):
            _check_step(worst, f"skew cols={cols}", f"skewed m={m} cols={cols}", got[(m, cols)], ref, vn)
    worst.report()


# ---------------------------------------------------------------- the split form on side streams
def _split_slots(rng, n):
    ms = [0, 1, 3, 4, 5, 9, 13, 28, SPLIT_MAX_COLS]
    slots = []
    for s in range(16):
        m = ms[s % len(ms)]
        V = _orthonormal(rng, n, m, True)
        if s % 4 == 3 and m >= 3:
            V = _skewed(V, True)
        delta = DELTAS[s % 3]
        a = rng.standard_normal(m) + 1j * rng.standard_normal(m)
        w = (V.T @ a if m else 0.0) + delta * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        slots.append((V, w))
    return slots


def test_split_arnoldi_steps_on_side_streams(hip, monkeypatch):
    """hipeig_pair_arnoldi_step_begin / hipeig_arnoldi_step_end as gcrotmk_device_block calls them: 16 slots begun before
    any is collected (8 side streams: slots s and s + 8 share a stream, its workspace and its result record), blocked
    sweeps of 0 .. SPLIT_MAX_COLS columns.  Each slot: within the bounds of the reference; bit for bit the step
    hipeig_pair_arnoldi_step_p runs on the compute stream (same kernel, same grid); bit for bit the same with 1, 8 and 16
    side streams (the count is read once per context); and a product enqueued on the compute stream right after
    end(slot) reads the finished w (the ordering the split form's callers rely on)."""
    from eigensolvers_amd.gcrotmk import _PairOps
    n = 100_003
    rng = np.random.default_rng(1459)
    slots = _split_slots(rng, n)
    z = 0.02 + 0.05j
    worst = _Worst("split")
    results = {}
    for ns in (1, 8, 16):
        monkeypatch.setenv("HIPEIG_ARNOLDI_STREAMS", str(ns))
        ctx = hip.HipContext()
        H = hip.HipCsrOperator.generate(n, 32, seed=7, ctx=ctx)
        H.set_variant(2)                              # a bitwise reproducible product (fixed order of the adds)
        opss = [_PairOps(ctx, n, 4) for _ in slots]
        dev = [(_up_cols(ctx, V, True), _up_w(ctx, w, True)) for V, w in slots]
        ys = [(ctx.alloc(n), ctx.alloc(n)) for _ in slots]
        for s, (Vd, wd) in enumerate(dev):
            opss[s].arnoldi_begin(Vd, wd, s)
        scal = []
        for s, (Vd, wd) in enumerate(dev):
            scal.append(opss[s].arnoldi_end(len(Vd), s))
            H.apply_shifted_pair(z, wd[0], wd[1], ys[s][0], ys[s][1])     # compute stream, no wait but end(s)
        out = []
        for s, (Vd, wd) in enumerate(dev):
            wv = _down_w(ctx, wd, True)
            y2 = (ctx.alloc(n), ctx.alloc(n))
            H.apply_shifted_pair(z, _up(ctx, wv.real), _up(ctx, wv.imag), y2[0], y2[1])
            np.testing.assert_array_equal(_down_w(ctx, ys[s], True), _down_w(ctx, y2, True),
                                          err_msg=f"streams={ns} slot {s}: product read w before the step finished")
            out.append((scal[s][0], scal[s][1], scal[s][2], wv))
        results[ns] = out
        if ns == 8:                                   # the same steps on the compute stream
            for s, (V, w) in enumerate(slots):
                Vd, _ = dev[s]
                wd = _up_w(ctx, w, True)
                nb, h, na = opss[s].arnoldi_step(Vd, wd)
                assert nb == out[s][0] and na == out[s][2], f"slot {s}: norms differ from the compute-stream step"
                np.testing.assert_array_equal(h, out[s][1], err_msg=f"slot {s}: coefficients")
                np.testing.assert_array_equal(_down_w(ctx, wd, True), out[s][3], err_msg=f"slot {s}: w")
        del H, opss, dev, ys
        ctx.synchronize()
        del ctx
        gc.collect()
    for ns in (1, 16):
        for s in range(len(slots)):
            a, b = results[ns][s], results[8][s]
            assert a[0] == b[0] and a[2] == b[2], f"slot {s}: norms differ between 8 and {ns} side streams"
            np.testing.assert_array_equal(a[1], b[1], err_msg=f"slot {s}: coefficients, {ns} streams")
            np.testing.assert_array_equal(a[3], b[3], err_msg=f"slot {s}: w, {ns} streams")
    for s, (V, w) in enumerate(slots):
        vn = np.array([float(hp.nrm2(v)) for v in V])
        _check_step(worst, "side streams", f"slot {s} m={len(V)}", results[8][s], hp.mgs(V, w), vn)
    worst.report()


# ---------------------------------------------------------------- batched small steps
@pytest.mark.parametrize("n", [37, 4000, 8191, 8192])
def test_batched_small_steps_against_the_high_precision_reference(hip, n):
    """hipeig_pair_arnoldi_step_batch_begin: 16 steps of up to SPLIT_MAX_COLS columns in one launch, a workgroup each,
    against the reference (the existing test pins them to the single step; this pins both to the operation).  At n = 37
    the columns are unit vectors but not orthogonal (more of them than the dimension)."""
    import os
    from eigensolvers_amd.gcrotmk import _PairOps
    if os.environ.get("HIPEIG_MAPPED_SCALARS") == "0":
        pytest.skip("the batched form needs the mapped scalar area (it is declined without it: status 5)")
    ctx = hip.HipContext.default()
    rng = np.random.default_rng(n)
    ms = [0, 1, 2, 3, 4, 5, 7, 8, 9, 13, 20, 28, 40, 47, 61, SPLIT_MAX_COLS]
    worst = _Worst(f"batch n={n}")
    steps = []
    for s, m in enumerate(ms):
        if m > n // 2:
            V = rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))
            V /= np.linalg.norm(V, axis=1, keepdims=True)
        else:
            V = _orthonormal(rng, n, m, True)
        w = (V.T @ (rng.standard_normal(m) + 1j * rng.standard_normal(m)) if m else 0.0) + \
            DELTAS[s % 3] * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        steps.append((V, w))
    opss = [_PairOps(ctx, n) for _ in steps]
    reqs = [(_up_cols(ctx, V, True), _up_w(ctx, w, True)) for V, w in steps]
    assert _PairOps.arnoldi_begin_batch(opss, reqs)
    for s, ((V, w), (Vd, wd)) in enumerate(zip(steps, reqs)):
        nb, h, na = opss[s].arnoldi_end(len(Vd), s)
        vn = np.array([float(hp.nrm2(v)) for v in V])
        _check_step(worst, "batch", f"step {s} m={len(V)}", (nb, h, na, _down_w(ctx, wd, True)), hp.mgs(V, w), vn)
    worst.report()


# ---------------------------------------------------------------- MGS projections
@pytest.mark.parametrize("n", [1000, 100_003])
@pytest.mark.parametrize("pair", [False, True], ids=["real", "pair"])
def test_mgs_projection_against_the_high_precision_reference(hip, pair, n):
    """hipeig_mgs_project / hipeig_pair_mgs_project (w <- w - sum_j c_j V_j, coefficients taken one column after the
    other, no normalisation) for m = 0, 1, 5, 17, orthonormal and skewed columns, w close to span(V)."""
    ctx = hip.HipContext.default()
    rng = np.random.default_rng(n + pair)
    worst = _Worst(f"mgs_project {'pair' if pair else 'real'} n={n}")
    PP = C.POINTER(C.c_void_p)
    for skew in (False, True):
        for m in (0, 1, 5, 17):
            V = _orthonormal(rng, n, m, pair)
            if skew and m >= 3:
                V = _skewed(V, pair)
            a = rng.standard_normal(m) + (1j * rng.standard_normal(m) if pair else 0.0)
            r = rng.standard_normal(n) + (1j * rng.standard_normal(n) if pair else 0.0)
            w = (V.T @ a if m else 0.0) + 1e-8 * r
            Vd, wd = _up_cols(ctx, V, pair), _up_w(ctx, w, pair)
            coef = np.full(2 * m + 2, np.nan)
            if pair:
                tr = (C.c_void_p * max(m, 1))(*[v[0].ptr for v in Vd])
                ti = (C.c_void_p * max(m, 1))(*[v[1].ptr for v in Vd])
                _lib.call("hipeig_pair_mgs_project", ctx.handle, n, m, C.cast(tr, PP), C.cast(ti, PP), wd[0].ptr, wd[1].ptr,
                          coef.ctypes.data_as(C.POINTER(C.c_double)))
                h = coef[0:2 * m:2] + 1j * coef[1:2 * m:2]
            else:
                tab = (C.c_void_p * max(m, 1))(*[v.ptr for v in Vd])
                _lib.call("hipeig_mgs_project", ctx.handle, n, m, C.cast(tab, PP), wd.ptr,
                          coef.ctypes.data_as(C.POINTER(C.c_double)))
                h = coef[:m]
            wv = _down_w(ctx, wd, pair)
            if m == 0:
                np.testing.assert_array_equal(wv, w)                  # nothing to project against: w untouched
                continue
            nb_r, h_r, na_r, w_r = hp.mgs(V, w, normalise=False)
            vn = np.array([float(hp.nrm2(v)) for v in V])
            _check_step(worst, "skew" if skew else "orth", f"m={m} skew={skew}",
                        (float(nb_r), h, float(na_r), wv), (nb_r, h_r, na_r, w_r), vn, normalised=False)
    worst.report()


# ---------------------------------------------------------------- the partitioned sweep (an all-reduce per column)
@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("pair", [False, True], ids=["real", "pair"])
def test_partitioned_arnoldi_step_on_loopback_ranks(hip, pair, P):
    """The row-partitioned form of the step and of the projection (arnoldi.hip, arnoldi_partitioned: dot kernel,
    one-workgroup reduce, all-reduce, update kernel per column) on P loopback ranks with ragged row ranges of n = 1003:
    every rank uploads its rows and calls arnoldi_step with cols_per_pass 1 and 4 (a partitioned run takes the same
    sweep for both) and mgs_project.  Every rank returns the same scalars bit for bit, cols_per_pass 4 equals 1 bit for
    bit, and the concatenated w with the scalars is within the module's bounds of the extended-precision sweep."""
    from eigensolvers_amd.distributed import LoopbackGroup, row_range
    from eigensolvers_amd.gcrotmk import _Ops, _PairOps
    n = 1003
    rng = np.random.default_rng(1003 + 10 * P + pair)
    cases = []
    for skew in (False, True):
        for m in (0, 1, 5, 17):
            V = _orthonormal(rng, n, m, pair)
            if skew and m >= 3:
                V = _skewed(V, pair)
            a = rng.standard_normal(m) + (1j * rng.standard_normal(m) if pair else 0.0)
            r = rng.standard_normal(n) + (1j * rng.standard_normal(n) if pair else 0.0)
            cases.append((skew, m, V, (V.T @ a if m else 0.0) + 1e-8 * r))
    grp = LoopbackGroup(P)

    def body(rank, ctx):
        assert ctx.collectives
        b, e = row_range(n, P, rank)
        ops = {cols: (_PairOps if pair else _Ops)(ctx, e - b, cols) for cols in (1, 4)}
        out = []
        for skew, m, V, w in cases:
            Vd = _up_cols(ctx, V[:, b:e], pair)
            got = {}
            for cols in (1, 4):
                wd = _up_w(ctx, w[b:e], pair)
                nb, h, na = ops[cols].arnoldi_step(Vd, wd)
                got[cols] = (nb, np.array(h), na, _down_w(ctx, wd, pair))
            wd = _up_w(ctx, w[b:e], pair)
            got["mgs"] = (np.array(ops[1].mgs_project(Vd, wd)), _down_w(ctx, wd, pair))
            out.append(got)
        return out

    try:
        res = grp.run(body)
    finally:
        grp.close()
    worst = _Worst(f"partitioned {'pair' if pair else 'real'} P={P}")
    for k, (skew, m, V, w) in enumerate(cases):
        what = f"m={m} skew={skew}"
        for o in res:
            for cols in (1, 4):
                assert o[k][cols][0] == res[0][k][1][0] and o[k][cols][2] == res[0][k][1][2], f"{what} cols={cols}: norms differ"
                np.testing.assert_array_equal(o[k][cols][1], res[0][k][1][1], err_msg=f"{what} cols={cols}: coefficients differ")
                np.testing.assert_array_equal(o[k][cols][3], o[k][1][3], err_msg=f"{what}: w of cols_per_pass 4 differs from 1")
            np.testing.assert_array_equal(o[k]["mgs"][0], res[0][k]["mgs"][0], err_msg=f"{what}: projection coefficients differ")
        vn = np.array([float(hp.nrm2(v)) for v in V])
        group = "skew" if skew else "orth"
        nb, h, na, _ = res[0][k][1]
        _check_step(worst, f"step {group}", f"step {what}", (nb, h, na, np.concatenate([o[k][1][3] for o in res])),
                    hp.mgs(V, w), vn)
        wv = np.concatenate([o[k]["mgs"][1] for o in res])
        if m == 0:
            np.testing.assert_array_equal(wv, w)                      # nothing to project against: w untouched
            continue
        nb_r, h_r, na_r, w_r = hp.mgs(V, w, normalise=False)
        _check_step(worst, f"project {group}", f"project {what}", (float(nb_r), res[0][k]["mgs"][0], float(na_r), wv),
                    (nb_r, h_r, na_r, w_r), vn, normalised=False)
    worst.report()


# ---------------------------------------------------------------- block complex-shift product
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("variant", [1, 2])
def test_block_shift_product_row_by_row(hip, monkeypatch, variant, width):
    """hipeig_spmm_shift_pairs (through apply_shifted_pairs): y_p = sign (z x_p - A x_p) for 2 .. 11 complex operands -
    blocks 4, 8 and 16 wide - on the ragged operator (empty rows, a 2600-long row, duplicates, unsorted columns), both
    block kernels and both signs, each row against the extended-precision product."""
    from test_gpu_feast import _ragged_csr
    N = 70_001
    rng = np.random.default_rng(176 + variant)
    rowptr, col, val = _ragged_csr(rng, N, N)
    H = hip.HipCsrOperator.from_csr_arrays(rowptr, col, val, N)
    H.set_block_variant(variant)
    monkeypatch.setenv("HIPEIG_PAIR_BLOCK_WIDTH", str(width))
    ctx = hip.HipContext.default()
    z = -0.37 + 0.21j
    worst = _Worst(f"shift product variant={variant} width={width}")
    for npairs, reverse in ((2, False), (3, True), (4, False), (5, True), (8, False), (11, True)):
        xs = [rng.standard_normal(N) * np.exp(rng.uniform(-3, 3, N)) + 1j * rng.standard_normal(N) for _ in range(npairs)]
        xd = [(_up(ctx, x.real), _up(ctx, x.imag)) for x in xs]
        ys = H.apply_shifted_pairs(z, xd, reverse=reverse)
        sign = -1.0 if reverse else 1.0
        for p, (x, y) in enumerate(zip(xs, ys)):
            ax, absax, rowlen = hp.csr_matvec(rowptr, col, val, x)
            xw = x.astype(np.clongdouble)
            ref = sign * (np.clongdouble(z) * xw - ax)
            got = _down(ctx, y[0]) + 1j * _down(ctx, y[1])
            err = np.abs(got.astype(np.clongdouble) - ref).astype(np.float64)
            bound = (rowlen + 4) * U * (absax + abs(z) * np.abs(xw)).astype(np.float64)
            worst.check(f"npairs {npairs}", err, bound, f"npairs={npairs} operand {p} reverse={reverse}")
    assert H.block_info()["variant"] == ("row-owner" if variant == 1 else "column-window-blocked")
    worst.report()
