"""The device MINRES family held to extended precision over its first K = 4 steps, and pinned on its rare exits
(``_minres_steps.py`` holds the reference, the measure, the cases and the reasoning; ``test_minres_steps_cpu.py`` checks
them without a GPU).

A step is read by calling the C entry with ``rtol = 0`` and ``maxiter = k``: it returns ``x_k``, ``info == k`` and the
statistics of iteration k with ``istop == 6``.  Every deviation of ``x_k`` and of the six statistics from the
``longdouble`` run is held to ``8 D`` (``STEPS ...`` lines under ``-s`` print the observed ratios).  The exits run through
``HipVector.solve`` / ``solveBlock`` on the operators whose margins the CPU test has checked."""
import ctypes as C

import numpy as np
import pytest

import _hiprec as hp
import _minres_steps as ms
from eigensolvers_amd import _lib
from eigensolvers_amd.hip_vector import _ptr_table

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not hp.EXTENDED, reason="longdouble is no wider than double on this machine")]

BOUND = ms.FACTOR * ms.D
SMALL_WINDOWS = {"HIPEIG_TCOOW_RW": "64", "HIPEIG_TCOOW_WBITS": "10"}       # 64-row blocks, 1 Ki-column windows


# ---------------------------------------------------------------- reading steps
def _record(x, st, k, info, n=None):
    """``n``: the length of the system where step k == n ends its Krylov space.  There ``beta_{n+1}`` is 0 in exact
    arithmetic: at n = 1 every right-hand side is an eigenvector (``istop == -1``), and at n = 2 a residual that comes out
    as exactly 0 passes ``test <= rtol`` even with ``rtol = 0``.  Everywhere else the iteration limit is the stop."""
    got = (int(st[0]), int(st[1]), info)
    if k == n:
        assert got in ([(1, -1, 0)] if n == 1 else [(k, 6, k), (k, 1, 0), (k, 2, 0)]), (k, list(st), info)
    else:
        assert got == (k, 6, k), (k, list(st), info)
    return dict(x=x, rnorm=st[2], Anorm=st[3], ynorm=st[4], test1=st[5], test2=st[6], Acond=st[7])


def single_raw(hip, H, case, entry="hipeig_minres", minv=None, nsteps=None, rows=None, steps=None):
    """``[(k, x_k, statistics, info, collectives)]`` of the runs to the steps asked for: the library calls and nothing else,
    so that a rank of a group can make them (``rows = (lo, hi)``: the rank uploads its rows of ``b`` and ``x0`` and gets its
    rows of ``x_k`` back; no check is made here, a rank that raised would leave its peers waiting in a collective)."""
    ctx = H.ctx
    lo, hi = rows or (0, case.op.n)
    b = hip.HipVector(case.b[lo:hi].copy(), ctx=ctx)
    x0 = hip.HipVector(case.x0[lo:hi].copy(), ctx=ctx) if entry == "hipeig_minres_x0" else None
    out = []
    for k in (steps or range(1, (nsteps or case.nsteps) + 1)):
        xb = ctx.alloc(hi - lo)
        info = C.c_int(-1)
        st = (C.c_double * 8)()
        cs = (C.c_int64 * 4)()
        head = (ctx.handle, H.handle, float(case.sigma), float(case.sign), b._buf.ptr)
        tail = (xb.ptr, 0.0, k, C.byref(info), st)
        if entry == "hipeig_minres":
            _lib.call(entry, *head, *tail)
        elif entry == "hipeig_minres_x0":
            _lib.call(entry, *head, x0._buf.ptr, *tail)
        else:
            _lib.call(entry, *head, minv.ptr, *tail)
        _lib.call("hipeig_comm_stats", ctx.handle, cs)
        out.append((k, hip.HipVector(xb).array, list(st), info.value, int(cs[0])))
    return out


def single_steps(hip, H, case, entry="hipeig_minres", minv=None, nsteps=None, rows=None, steps=None):
    """Records of steps 1 .. K (or of ``steps``) of one of the single-vector entries on ``case``'s right-hand side."""
    raw = single_raw(hip, H, case, entry, minv, nsteps, rows, steps)
    return [_record(x, st, k, info, case.op.n) for k, x, st, info, _ in raw]


def block_raw(hip, H, cols, sigma, sign, minv=None, nsteps=ms.K, rows=None, steps=None):
    """``raw[j] = [(k, x_k, statistics, info, collectives)]`` of column j of the lock-step solve of ``cols`` (chunks of 8,
    as ``solveBlock`` cuts them), read as ``single_raw`` reads: library calls only, ``rows`` the rank's rows."""
    ctx = H.ctx
    lo, hi = rows or (0, len(cols[0]))
    raw = [[] for _ in cols]
    for i0 in range(0, len(cols), 8):
        chunk = [hip.HipVector(c[lo:hi].copy(), ctx=ctx) for c in cols[i0:i0 + 8]]
        kc = len(chunk)
        bt, keep1 = _ptr_table([b._buf for b in chunk])
        for k in (steps or range(1, nsteps + 1)):
            outs = [ctx.alloc(hi - lo) for _ in chunk]
            xt, keep2 = _ptr_table(outs)
            info = (C.c_int * kc)()
            st = (C.c_double * (8 * kc))()
            cs = (C.c_int64 * 4)()
            if minv is None:
                _lib.call("hipeig_minres_block", ctx.handle, H.handle, float(sigma), float(sign), kc, bt, xt, 0.0, k, info, st)
            else:
                _lib.call("hipeig_minres_block_jacobi", ctx.handle, H.handle, float(sigma), float(sign), kc, bt, minv.ptr, xt,
                          0.0, k, info, st)
            _lib.call("hipeig_comm_stats", ctx.handle, cs)
            for j in range(kc):
                raw[i0 + j].append((k, hip.HipVector(outs[j]).array, list(st[8 * j:8 * j + 8]), info[j], int(cs[0])))
    return raw


def block_records(cols, raw):
    """``recs[j][i]``: the record of the i-th step read of column j; a zero column was never started."""
    recs = [[] for _ in cols]
    for j, col in enumerate(cols):
        for k, x, st, info, _ in raw[j]:
            if not col.any():
                assert info == 0 and not x.any() and st[0] == 0
                recs[j].append(None)
            else:
                recs[j].append(_record(x, st, k, info))
    return recs


def block_steps(hip, H, cols, sigma, sign, minv=None, nsteps=ms.K, rows=None, steps=None):
    """``recs[j][k - 1]``: the record of step k of column j of the lock-step solve of ``cols`` (chunks of 8, as
    ``solveBlock`` cuts them)."""
    return block_records(cols, block_raw(hip, H, cols, sigma, sign, minv, nsteps, rows, steps))


def check_steps(label, case, recs, ref, x0=None, steps=None):
    """Every deviation of the records from the reference's is <= 8 D (past step K, where ``steps`` lists the steps the
    records were read at: <= 8 D_LONG); prints the largest ratio per quantity over the steps."""
    worst = {}
    ks = list(steps) if steps else list(range(1, len(recs) + 1))
    assert len(ks) == len(recs) and (steps is None or len(ref) >= ks[-1]), (label, ks, len(recs), len(ref))
    for k, g in zip(ks, recs):
        r = ref[k - 1]
        bound = ms.step_bound(k) if steps else BOUND
        dev = ms.step_deviations(g, r, ms.STATS, case.scales(k, ref))
        if x0 is not None:
            # x_k - x0 carries the roundings of x_k itself, u ||x_k|| each: relative to ||x_k - x0|| that many times more
            dx = r["x"] - x0.astype(ms.LD)
            dev["x-x0"] = ms.deviation(g["x"].astype(ms.LD) - x0.astype(ms.LD), dx) / max(1.0, float(hp.nrm2(r["x"]) / hp.nrm2(dx)))
        for q, d in dev.items():
            if not d / bound < worst.get(q, (-1.0, 0))[0]:
                worst[q] = (d / bound, k)
    what = f"8 D = {BOUND:g} u" + (f", past step {ms.K} 8 D_LONG = {ms.FACTOR * ms.D_LONG:g} u" if steps and ks[-1] > ms.K else "")
    print(f"STEPS {label}: largest deviation / ({what}): "
          + ", ".join(f"{q} {d:.3f} (step {k})" for q, (d, k) in worst.items()))
    bad = {q: v for q, v in worst.items() if not v[0] <= 1.0}
    assert not bad, (label, bad)
    return max(d for d, _ in worst.values())


_operators = {}


def device_operator(hip, name, fresh=False):
    """The device copy of ``ms.operator(name)``; ``fresh``: one of its own (a layout is built once, with the knobs then set)."""
    if fresh:
        return _upload(hip, name)
    if name not in _operators:
        _operators[name] = _upload(hip, name)
    H = _operators[name]
    H.set_variant(0)
    H.set_block_variant(0)
    return H


def _upload(hip, name):
    A = ms.operator(name).A
    return hip.HipCsrOperator.from_dense(A.toarray()) if name.startswith("dense") else hip.HipCsrOperator.from_scipy(A)


def device_minv(hip, H, case):
    """(device buffer, host copy) of ``hipeig_jacobi_inverse``: the reference runs on the device's own ``minv``."""
    buf = H.jacobi_inverse(case.sigma)
    return buf, hip.HipVector(buf).array


# ---------------------------------------------------------------- hipeig_minres
def test_plain_both_signs_and_two_shifts(hip):
    H = device_operator(hip, "g1037")
    for name in ("g1037 sigma=0.02 sign=+1", "g1037 sigma=0.02 sign=-1", "g1037 sigma=0.0 sign=+1", "g1037 sigma=0.0 sign=-1"):
        case = ms.CASES[name]
        check_steps(f"plain {name}", case, single_steps(hip, H, case), ms.reference(case))


@pytest.mark.parametrize("name", ["dense1", "dense2", "g63", "g64", "g65"])
def test_plain_small_n(hip, name):
    """n = 1, 2: one workgroup, ``n >> 1`` of 0 and 1, K limited to n; 63, 64, 65: around one wave, 65 with the tail
    branches of KC and KD (1037, odd too, runs in the test above)."""
    case = ms.CASES[name]
    for form in (None, "0"):
        with pytest.MonkeyPatch.context() as mp:
            if form:
                mp.setenv("HIPEIG_MINRES_FUSE_KD", form)
            recs = single_steps(hip, device_operator(hip, name), case)
        assert len(recs) == min(ms.K, case.op.n)
        check_steps(f"plain {name} n={case.op.n} fuse_kd={form or 1}", case, recs, ms.reference(case))


@pytest.mark.parametrize("variant", [1, 2])
def test_plain_n20001_more_than_64_row_blocks(hip, variant):
    """The two-level finish of the sweep's reduction."""
    case = ms.CASES["g20001"]
    H = device_operator(hip, "g20001")
    H.set_variant(variant)
    check_steps(f"plain g20001 layout {variant}", case, single_steps(hip, H, case), ms.reference(case))
    assert H.last_variant() == H.VARIANTS[variant]


def test_plain_n20001_more_than_64_workgroups_in_kc_and_kd(hip, monkeypatch):
    monkeypatch.setenv("HIPEIG_MR_PER_THREAD", "1")                       # 79 workgroups of 256 elements
    case = ms.CASES["g20001"]
    for form in (None, "0"):
        if form:
            monkeypatch.setenv("HIPEIG_MINRES_FUSE_KD", form)
        check_steps(f"plain g20001 per_thread=1 fuse_kd={form or 1}", case, single_steps(hip, device_operator(hip, "g20001"), case),
                    ms.reference(case))


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5])
def test_plain_layouts_and_kernel_forms(hip, variant, monkeypatch):
    """Every sweep layout the KA epilogue lives in, KD riding on the next sweep and as its own kernel; the two forms bit
    for bit where the layout fixes the order of a row's adds (``_sweep_cases.check_kernel_forms``: 1, 2, 3, 5)."""
    for name in ("g1037 sigma=0.02 sign=-1", "g20001"):
        case = ms.CASES[name]
        H = device_operator(hip, case.opname)
        H.set_variant(variant)
        forms = {}
        for form in (None, "0"):
            monkeypatch.delenv("HIPEIG_MINRES_FUSE_KD", raising=False)
            if form:
                monkeypatch.setenv("HIPEIG_MINRES_FUSE_KD", form)
            forms[form] = single_steps(hip, H, case)
            check_steps(f"plain {name} layout {variant} fuse_kd={form or 1}", case, forms[form], ms.reference(case))
        assert H.last_variant() == H.VARIANTS[variant]
        if variant in (1, 2, 3, 5):
            for a, b in zip(forms[None], forms["0"]):
                np.testing.assert_array_equal(a["x"], b["x"])
                assert [a[q] for q in ms.STATS] == [b[q] for q in ms.STATS]


def test_plain_column_split_sweep(hip, monkeypatch):
    """The epilogue in the combine launch of a column-split blocked sweep: three shares per row block, 1 Ki-column windows
    (20 of them at n = 20001)."""
    for k, v in SMALL_WINDOWS.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HIPEIG_TCOOW_CSPLIT", "3")
    case = ms.CASES["g20001"]
    H = device_operator(hip, "g20001", fresh=True)
    H.set_variant(4)
    for form in (None, "0"):
        if form:
            monkeypatch.setenv("HIPEIG_MINRES_FUSE_KD", form)
        check_steps(f"plain g20001 layout 4 csplit=3 fuse_kd={form or 1}", case, single_steps(hip, H, case), ms.reference(case))
    info = H.layout_info()
    assert info["column_splits"] == 3 and info["windows"] >= 3 and info["rows_per_block"] == 64, info


# ---------------------------------------------------------------- hipeig_minres_x0
@pytest.mark.parametrize("n", [1037, 20001])
def test_initial_guess(hip, n):
    """``ynorm`` includes ``x0``; ``x_k - x0`` is compared as well, so that a lost ``x0`` cannot hide in the norm."""
    case = ms.CASES[f"g{n} x0"]
    recs = single_steps(hip, device_operator(hip, case.opname), case, entry="hipeig_minres_x0")
    check_steps(f"x0 g{n}", case, recs, ms.reference(case), x0=case.x0)


# ---------------------------------------------------------------- hipeig_minres_jacobi
@pytest.mark.parametrize("n", [1037, 20001])
def test_jacobi(hip, n, monkeypatch):
    """Chunks of 2 iterations: a stand-alone KD, then an iteration with no pending KD, inside the four steps."""
    monkeypatch.setenv("HIPEIG_PMR_CHUNK", "2")
    case = ms.CASES[f"g{n} jacobi"]
    H = device_operator(hip, case.opname)
    buf, minv = device_minv(hip, H, case)
    recs = single_steps(hip, H, case, entry="hipeig_minres_jacobi", minv=buf)
    check_steps(f"jacobi g{n} chunk=2", case, recs, ms.reference(case, minv=minv))
    monkeypatch.delenv("HIPEIG_PMR_CHUNK")
    recs16 = single_steps(hip, H, case, entry="hipeig_minres_jacobi", minv=buf)
    check_steps(f"jacobi g{n} chunk=16", case, recs16, ms.reference(case, minv=minv))


# ---------------------------------------------------------------- the block forms
def _block(hip, k, variant, jacobi):
    cases = ms.block_cases(k, jacobi)
    H = device_operator(hip, "g1037")
    H.set_block_variant(variant)
    buf = minv = None
    if jacobi:
        buf, minv = device_minv(hip, H, cases[0])
    cols = [c.b for c in cases]
    assert np.linalg.norm(cols[ms.SCALED_COLUMN]) < 1e-6 < 0.3 < min(np.linalg.norm(c) for j, c in enumerate(cols) if j != ms.SCALED_COLUMN)
    recs = block_steps(hip, H, cols, 0.02, 1.0, minv=buf)
    name = ("jacobi " if jacobi else "") + f"block k={k} kernel {variant}"
    ratios = [check_steps(f"{name} column {j}", c, recs[j], ms.reference(c, minv=minv)) for j, c in enumerate(cases)]
    print(f"STEPS {name}: largest ratio over the columns {max(ratios):.3f}, scaled column {ratios[ms.SCALED_COLUMN]:.3f}")
    if variant == 1:
        # the run with that column alone: the other columns of its chunk zero (never started), same width, same slot
        for j in range(k):
            i0 = j - j % 8
            alone = [c if i0 + i == j else np.zeros_like(c) for i, c in enumerate(cols[i0:i0 + 8])]
            ra = block_steps(hip, H, alone, 0.02, 1.0, minv=buf)[j - i0]
            for a, b in zip(ra, recs[j]):
                np.testing.assert_array_equal(a["x"], b["x"], err_msg=f"{name} column {j}")
    assert H.block_info()["variant"] == H.BLOCK_VARIANTS[variant]


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("k", [3, 8, 11])
def test_block(hip, k, variant):
    """k = 3: the 4-wide interleave; 8: the 8-wide; 11: a chunk of 8 and one of 3.  Every column against its own reference,
    one column scaled by 1e-7; on the row-owner kernel every column bit for bit the run with that column alone."""
    _block(hip, k, variant, jacobi=False)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("k", [3, 8, 11])
def test_block_jacobi(hip, k, variant, monkeypatch):
    monkeypatch.setenv("HIPEIG_PMRB_CHUNK", "2")
    _block(hip, k, variant, jacobi=True)


# ---------------------------------------------------------------- exits
def _opts(e_or_it, tol=None, **lsa):
    it, tol = (e_or_it.maxiter, e_or_it.rtol) if tol is None else (e_or_it, tol)
    d = {"linearSolver": "minres", "linearIter": int(it), "linear_tol": float(tol)}
    d.update(lsa)
    return {"linearSystemArgs": d}


JACOBI = {"preconditioner": "jacobi"}
LOCKSTEP = {"preconditioner": "jacobi", "preconditionerLockStep": True}


def _ordinary64(j):
    g = np.random.default_rng([64, j]).standard_normal(64)
    return g / np.linalg.norm(g)


def _check_eigenvector_solution(e, x, st, label):
    j = int(np.flatnonzero(e.b)[0])
    assert (st["iterations"], st["istop"]) == (1, -1), (label, st)
    assert np.isfinite(x).all() and list(np.flatnonzero(x)) == [j], label
    exact = ms.LD(e.sign) * ms.LD(e.b[j]) / (ms.LD(e.sigma) - ms.LD(e.H.diagonal()[j]))
    dev = ms.deviation(x[j], exact)
    print(f"STEPS exit eigenvector {label}: x_j within {dev:.2f} u of sign c / (sigma - h_j)")
    assert dev <= 4.0, label


def _ordinary_solve(hip, e, ctx, lsa, k=0, block_variant=0):
    """One ordinary solve on the eigenvector case's operator in the given context (``k``: a block solve of k columns, which
    uses the block workspace): [(x, stats)] per column."""
    H = hip.HipCsrOperator.from_scipy(e.H, ctx=ctx)
    H.set_block_variant(block_variant)
    vecs = [hip.HipVector(_ordinary64(100 + j), _opts(200, 1e-10, **lsa), ctx=ctx) for j in range(max(k, 1))]
    X = hip.HipVector.solveBlock(H, vecs, e.sigma) if k else [hip.HipVector.solve(H, vecs[0], e.sigma)]
    return [(x.array, x.last_solve_stats) for x in X]


def _check_nothing_leaked(hip, e, ctx, lsa, label, k=0, block_variant=0):
    """The breakdown leaves non-finite values in the workspace rings (same lengths: nothing is reallocated); an ordinary
    solve after it on the same context gives the bits of the same solve on a fresh context."""
    same = _ordinary_solve(hip, e, ctx, lsa, k, block_variant)
    fresh = _ordinary_solve(hip, e, hip.HipContext(), lsa, k, block_variant)
    for (x, st), (xf, stf) in zip(same, fresh):
        assert np.isfinite(x).all() and st["istop"] in (1, 2), (label, st)
        np.testing.assert_array_equal(x, xf, err_msg=label)
        assert st == stf, label


@pytest.mark.parametrize("lsa", [{}, JACOBI], ids=["plain", "jacobi"])
@pytest.mark.parametrize("linear_iter", [1, 50])
@pytest.mark.parametrize("form", [None, "0"], ids=["kd-riding", "kd-own-kernel"])
def test_exit_right_hand_side_an_eigenvector(hip, form, linear_iter, lsa, monkeypatch):
    """``beta_2 == 0``: ``istop == -1`` after one iteration, no exception.  ``linearIter`` 1: the stand-alone KD ends the
    solve; 50: KD rides on the following sweep, which runs with ``s = 1 / 0`` on ``r2 = 0``."""
    if form:
        monkeypatch.setenv("HIPEIG_MINRES_FUSE_KD", form)
    e = ms.EXITS["eigenvector n=64"]
    ctx = hip.HipContext.default()
    H = hip.HipCsrOperator.from_scipy(e.H, ctx=ctx)
    W = hip.HipVector.solve(H, hip.HipVector(e.b.copy(), _opts(linear_iter, 1e-10, **lsa), ctx=ctx), e.sigma)
    label = f"{'jacobi' if lsa else 'plain'} fuse_kd={form or 1} linearIter={linear_iter}"
    _check_eigenvector_solution(e, W.array, W.last_solve_stats, label)
    _check_nothing_leaked(hip, e, ctx, lsa, label)


@pytest.mark.parametrize("kind", ["row-owner", "column-window-blocked", "jacobi-lock-step"])
@pytest.mark.parametrize("k,at", [(3, 2), (3, 1), (8, 5)])
def test_exit_eigenvector_column_in_a_block(hip, k, at, kind):
    """The eigenvector column stops after one iteration while the others run on: its iterate is the same bits at the end,
    the live columns equal the solves with that column alone (iterations, stop code, on the row-owner kernel bits).
    KD handles the columns in pairs and skips a pair that has stopped: column 2 of 3 shares its pair with the padding
    column, column 1 of 3 and column 5 of 8 with a live one, where only KD's per-column guard keeps the iterate."""
    e = ms.EXITS["eigenvector n=64"]
    lsa = LOCKSTEP if kind == "jacobi-lock-step" else {}
    ctx = hip.HipContext.default()
    H = hip.HipCsrOperator.from_scipy(e.H, ctx=ctx)
    H.set_block_variant(2 if kind == "column-window-blocked" else 1)
    cols = [e.b if j == at else _ordinary64(j) * (1.0 + 0.3 * j) for j in range(k)]

    def solve(cs):
        vecs = [hip.HipVector(c.copy(), _opts(200, 1e-10, **lsa), ctx=ctx) for c in cs]
        X = hip.HipVector.solveBlock(H, vecs, e.sigma)
        return [(x.array, x.last_solve_stats) for x in X]

    got = solve(cols)
    assert H.block_info()["variant"] == ("column-window-blocked" if kind == "column-window-blocked" else "row-owner")
    _check_eigenvector_solution(e, got[at][0], got[at][1], f"column {at} of {k}, {kind}")
    for j in range(k):
        xa, sa = solve([c if i == j else np.zeros(64) for i, c in enumerate(cols)])[j]
        x, st = got[j]
        assert (st["iterations"], st["istop"]) == (sa["iterations"], sa["istop"]), (j, st, sa)
        if j != at:
            assert st["istop"] in (1, 2) and st["iterations"] > 1
        if kind != "column-window-blocked" or j == at:
            np.testing.assert_array_equal(x, xa, err_msg=f"column {j} of {k}, {kind}")
        else:
            assert np.linalg.norm(x - xa) <= 1e-9 * np.linalg.norm(xa)
    _check_nothing_leaked(hip, e, ctx, lsa, f"block of {k}, {kind}", k=k, block_variant=2 if kind == "column-window-blocked" else 1)


def _oracle(e):
    x, itn, istop, trace = ms.full_trace(e.matvec, e.b, e.rtol, e.maxiter)
    assert (itn, istop) == e.expect
    return x, trace


def _check_exit(e, x, st, label):
    """``(iterations, istop)`` the oracle's; the statistics finite and on the oracle's side of the deciding threshold;
    where the operator is well conditioned (the ``1 + test1 <= 1`` cases at n = 1037) the iterate, ``Anorm`` and ``ynorm``
    within 8 D of the oracle's - ``rnorm``, ``test1`` and ``test2`` are rounding residue there."""
    xo, trace = _oracle(e)
    assert (st["iterations"], st["istop"]) == e.expect, (label, st)
    vals = [st[q] for q in ms.STATS]
    assert np.isfinite(vals).all() and np.isfinite(x).all(), (label, st)
    beta1 = float(np.linalg.norm(e.b))
    rec = dict(Anorm=st["Anorm"], ynorm=st["ynorm"], Acond=st["Acond"], test1=st["test1"], test2=st["test2"], beta1=beta1,
               epsx=st["Anorm"] * st["ynorm"] * ms.EPS, ratio=1.0)
    past, _ = ms.exit_margin([rec], e.decides)
    line = f"STEPS exit {label}: {e.expect}, {e.decides} past its threshold by {past:.3g}"
    assert past >= 1.0, (label, past)
    if e.name.startswith("1+test1 n=1037"):
        dev = {"x": ms.deviation(x, xo), "Anorm": ms.deviation(st["Anorm"], trace[-1]["Anorm"]),
               "ynorm": ms.deviation(st["ynorm"], trace[-1]["ynorm"])}
        line += ", deviation from the oracle / 8 D: " + ", ".join(f"{q} {d / BOUND:.3f}" for q, d in dev.items())
        print(line)
        assert max(dev.values()) <= BOUND, (label, dev)
    else:
        print(line)


@pytest.mark.parametrize("name", [n for n in ms.EXITS if n != "eigenvector n=64"])
def test_exit_codes_3_4_and_the_eps_level_test(hip, name, monkeypatch):
    """Through ``HipVector.solve`` in both kernel forms: no exception (``info == 0``)."""
    e = ms.EXITS[name]
    H = hip.HipCsrOperator.from_scipy(e.H)
    for form in (None, "0"):
        if form:
            monkeypatch.setenv("HIPEIG_MINRES_FUSE_KD", form)
        W = hip.HipVector.solve(H, hip.HipVector(e.b.copy(), _opts(e)), e.sigma, reverseGF=e.sign < 0)
        _check_exit(e, W.array, W.last_solve_stats, f"{name} fuse_kd={form or 1}")


BLOCK_EXITS = {"n=2": ("istop 3 n=2", "istop 4 n=2", None),
               "n=1037 d9": ("1+test1 n=1037 d9", "istop 3 n=1037", "zero", "1+test1 n=1037 d9"),
               "n=1037 d3": ("1+test1 n=1037 d3", "istop 4 n=1037", "1+test1 n=1037 d3")}


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("which", list(BLOCK_EXITS))
def test_exit_codes_side_by_side_in_a_block(hip, which, variant):
    """A column that exits with 3 or 4 beside columns that converge through ``1 + test1 <= 1`` (n = 2: beside an
    eigenvector column, ``istop == -1`` - every right-hand side with weight on both entries meets the tiny one); a case
    may stand in two slots; a zero column never starts."""
    names = BLOCK_EXITS[which]
    first = ms.EXITS[names[0]]
    H = hip.HipCsrOperator.from_scipy(first.H)
    H.set_block_variant(variant)
    n = len(first.b)
    cols = []
    for nm in names:
        if nm is None:
            cols.append(np.array([3.0, 0.0]))
        elif nm == "zero":
            cols.append(np.zeros(n))
        else:
            assert (ms.EXITS[nm].H != first.H).nnz == 0
            cols.append(ms.EXITS[nm].b)
    vecs = [hip.HipVector(c.copy(), _opts(first)) for c in cols]
    X = hip.HipVector.solveBlock(H, vecs, first.sigma, reverseGF=first.sign < 0)
    assert H.block_info()["variant"] == H.BLOCK_VARIANTS[variant]
    for j, (nm, x) in enumerate(zip(names, X)):
        st, xa = x.last_solve_stats, x.array
        label = f"block {which} kernel {variant} column {j}"
        if nm is None:
            assert (st["iterations"], st["istop"]) == (1, -1) and xa[1] == 0.0 and ms.deviation(xa[0], 3.0) <= 4.0, (label, st, xa)
        elif nm == "zero":
            assert st["iterations"] == 0 and not xa.any(), label
        else:
            _check_exit(ms.EXITS[nm], xa, st, label)
