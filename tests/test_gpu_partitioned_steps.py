"""The row-partitioned MINRES solves held to extended precision step by step, on loopback ranks of one GPU
(``LoopbackGroup``; ``_minres_steps.py`` holds the reference, the measure and the reasoning, ``test_gpu_minres_steps.py``
the helpers that read a step).

The partitioned solves are code of their own (minres.hip and minres_block.hip, ``dist``): the iterate update always rides
on the next sweep, every rank's share of ``<y,y>`` travels in a scalar slot of the operand exchange, ``<v,y>`` and the
lagged ``<x,x>`` share one all-reduce, chunks of 16 iterations follow each other with no flush - the pending update is
carried into the next chunk - and only the end of the solve runs the last update on its own.  A step is read as on one
GPU (``rtol = 0``, ``maxiter = k``), at the steps of ``ms.LONG_STEPS`` where the system allows it: 16 ends at a chunk
boundary, 17 and 18 carry a pending update across it, 32 ends at the second boundary, 33 crosses two.  Steps 1 .. 4 are
held to ``8 D``, the later ones to ``8 D_LONG``; the eight statistics must be the same bits on every rank.

Collectives.  A solve that ends at the iteration limit k has issued ``2 k + 2``, counted from the code and not from a
run.  One right-hand side (minres.hip): every iteration's sweep makes one operand exchange (``enqueue_ka``) and one
all-reduce of two doubles follows it (``enqueue_iteration``) - 2 k; nothing is issued at a chunk boundary; the end adds
the all-reduce of ``<y,y>`` in front of the stand-alone update (``enqueue_last_kd``) and that of its ``<x,x>``
(``enqueue_check``) - 2.  The block (minres_block.hip): per iteration the exchange of the operand block and one all-reduce
of 16 - 2 k; the end flush all-reduces ``red + 16`` and ``red + 24`` - 2.  What comes before the count is reset (``<b,b>``,
the product with an initial guess) is not in it.

Every body of a rank makes library calls and returns what they gave; nothing is asserted before every rank has returned
and the group is closed, and no call depends on the rank: a rank that raised or took another path would leave its peers
waiting in a collective.  Every rank holds at least one row (a rank without rows is a known limit)."""
import numpy as np
import pytest

import _hiprec as hp
import _minres_steps as ms
from _partition_cases import on_ranks
from eigensolvers_amd.distributed import row_range
from test_gpu_minres_steps import (BLOCK_EXITS, SMALL_WINDOWS, _check_eigenvector_solution, _check_exit, _opts, _record,
                                   block_raw, block_records, check_steps, single_raw)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not hp.EXTENDED, reason="longdouble is no wider than double on this machine")]

LONG = ms.LONG_STEPS


# ---------------------------------------------------------------- running on ranks (``on_ranks``: _partition_cases.py)
def rank_operator(hip, A, P, rank, ctx):
    lo, hi = row_range(A.shape[0], P, rank)
    return hip.HipCsrOperator.from_scipy(A, row_begin=lo, row_end=hi, ctx=ctx), (lo, hi)


def merge(raws, n):
    """The ranks' ``single_raw`` lists as one: the slices of ``x_k`` concatenated; the statistics, ``info`` and the
    collectives counted must be the same bits on every rank."""
    out = []
    for i, (k, _, st, info, coll) in enumerate(raws[0]):
        for r, raw in enumerate(raws[1:], start=1):
            assert np.array(raw[i][2]).tobytes() == np.array(st).tobytes(), (k, r, raw[i][2], st)
            assert (raw[i][0], raw[i][3], raw[i][4]) == (k, info, coll), (k, r)
        x = np.concatenate([raw[i][1] for raw in raws])
        assert x.shape == (n,)
        out.append((k, x, st, info, coll))
    return out


def records(merged, n=None):
    """Records of merged steps; a step that ended at the iteration limit k has issued 2 k + 2 collectives."""
    recs = []
    for k, x, st, info, coll in merged:
        recs.append(_record(x, st, k, info, n))
        if int(st[1]) == 6:
            assert coll == 2 * k + 2, (k, coll)
    return recs


def partitioned_single(hip, case, P, steps=None, entry="hipeig_minres", variant=0):
    """``(records, layout_info per rank, last_variant per rank)`` of the single-vector solve of ``case`` on P ranks."""
    A = case.op.A

    def body(rank, ctx):
        H, rows = rank_operator(hip, A, P, rank, ctx)
        H.set_variant(variant)
        raw = single_raw(hip, H, case, entry=entry, rows=rows, steps=steps)
        return raw, H.layout_info(), H.last_variant()

    res = on_ranks(P, body)
    return records(merge([r[0] for r in res], case.op.n), case.op.n), [r[1] for r in res], [r[2] for r in res]


# ---------------------------------------------------------------- one right-hand side
@pytest.mark.parametrize("P", [2, 3])
def test_plain_both_signs_at_the_long_steps(hip, P):
    """g1037 on 2 and 3 ranks (slabs 346 / 346 / 345: an odd tail on the last rank), both signs."""
    for name in ("g1037 sigma=0.02 sign=+1", "g1037 sigma=0.02 sign=-1"):
        case = ms.CASES[name]
        recs, _, _ = partitioned_single(hip, case, P, steps=LONG)
        check_steps(f"partitioned P={P} {name}", case, recs, ms.reference(case, nsteps=LONG[-1]), steps=LONG)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("name", ["g63", "g64", "g65"])
def test_small_systems_slabs_shorter_than_a_wave(hip, name, P):
    """Slabs of 21 .. 33 rows; K steps only: by step 34 these systems have nearly exhausted their Krylov space."""
    case = ms.CASES[name]
    recs, _, _ = partitioned_single(hip, case, P)
    assert len(recs) == ms.K
    check_steps(f"partitioned P={P} {name}", case, recs, ms.reference(case), steps=range(1, ms.K + 1))


def test_one_row_per_rank(hip):
    """n = 2 on two ranks; step 2 ends the Krylov space (``Case.scales``)."""
    case = ms.CASES["dense2"]
    recs, _, _ = partitioned_single(hip, case, 2)
    assert len(recs) == 2
    check_steps("partitioned P=2 dense2", case, recs, ms.reference(case), steps=(1, 2))


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5])
def test_every_sweep_layout_on_three_slabs(hip, variant):
    """g20001 on 3 ranks (slabs of 6667): every sweep layout the KA epilogue lives in, the riding KD with it."""
    case = ms.CASES["g20001"]
    recs, _, kinds = partitioned_single(hip, case, 3, steps=LONG, variant=variant)
    check_steps(f"partitioned P=3 g20001 layout {variant}", case, recs, ms.reference(case, nsteps=LONG[-1]), steps=LONG)
    assert kinds == [hip.HipCsrOperator.VARIANTS[variant]] * 3, kinds


def test_column_split_sweep_on_three_slabs(hip, monkeypatch):
    """Local and remote windows and three shares per row block: the combine launch carries the KA epilogue."""
    for k, v in SMALL_WINDOWS.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HIPEIG_TCOOW_CSPLIT", "3")
    case = ms.CASES["g20001"]
    recs, layouts, kinds = partitioned_single(hip, case, 3, steps=LONG, variant=4)
    check_steps("partitioned P=3 g20001 layout 4 csplit=3", case, recs, ms.reference(case, nsteps=LONG[-1]), steps=LONG)
    assert kinds == [hip.HipCsrOperator.VARIANTS[4]] * 3, kinds
    for info in layouts:
        assert info["column_splits"] == 3 and info["windows"] > 3 and info["rows_per_block"] == 64, info


@pytest.mark.parametrize("chunks", [2, 3])
def test_chunked_exchange_on_three_slabs(hip, chunks, monkeypatch):
    """The operand exchange cut into chunks: the scalar slots sit behind the last chunk, at a stride of their own
    (``cstride(nchunks - 1)``)."""
    monkeypatch.setenv("HIPEIG_GATHER_CHUNKS", str(chunks))
    for k, v in SMALL_WINDOWS.items():
        monkeypatch.setenv(k, v)
    case = ms.CASES["g20001"]
    recs, layouts, _ = partitioned_single(hip, case, 3, steps=LONG, variant=4)
    check_steps(f"partitioned P=3 g20001 exchange chunks={chunks}", case, recs, ms.reference(case, nsteps=LONG[-1]), steps=LONG)
    for info in layouts:
        assert info["exchange_chunks"] == chunks, info


def test_initial_guess_on_three_ranks(hip):
    """``hipeig_minres_x0`` starts from a partitioned product; ``x_k - x0`` is compared as well."""
    case = ms.CASES["g1037 x0"]
    recs, _, _ = partitioned_single(hip, case, 3, steps=LONG, entry="hipeig_minres_x0")
    check_steps("partitioned P=3 x0 g1037", case, recs, ms.reference(case, nsteps=LONG[-1]), x0=case.x0, steps=LONG)


# ---------------------------------------------------------------- the block
def partitioned_block(hip, cols, P, variant, steps):
    """``recs[j]``: the records of column j of the lock-step solve of ``cols`` on P ranks (g1037, sigma 0.02, sign +1)."""
    A = ms.operator("g1037").A

    def body(rank, ctx):
        H, rows = rank_operator(hip, A, P, rank, ctx)
        H.set_block_variant(variant)
        raw = block_raw(hip, H, cols, 0.02, 1.0, rows=rows, steps=steps)
        return raw, H.block_info()["variant"]

    res = on_ranks(P, body)
    assert [r[1] for r in res] == [hip.HipCsrOperator.BLOCK_VARIANTS[variant]] * P
    merged = [merge([r[0][j] for r in res], A.shape[0]) for j in range(len(cols))]
    for j, col in enumerate(cols):
        if col.any():
            records(merged[j])                                   # the collectives of the lock-step solve: 2 k + 2
    return block_records(cols, merged)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("k", [3, 8])
def test_block_at_the_long_steps(hip, k, variant, P):
    """The 4-wide and the 8-wide interleave, both block kernels: every column against its own reference, the column
    scaled by 1e-7 included."""
    cases = ms.block_cases(k)
    cols = [c.b for c in cases]
    assert np.linalg.norm(cols[ms.SCALED_COLUMN]) < 1e-6
    recs = partitioned_block(hip, cols, P, variant, LONG)
    name = f"partitioned P={P} block k={k} kernel {variant}"
    ratios = [check_steps(f"{name} column {j}", c, recs[j], ms.reference(c, nsteps=LONG[-1]), steps=LONG) for j, c in enumerate(cases)]
    print(f"STEPS {name}: largest ratio over the columns {max(ratios):.3f}, scaled column {ratios[ms.SCALED_COLUMN]:.3f}")


@pytest.mark.parametrize("variant", [1, 2])
def test_block_of_eight_with_a_zero_column(hip, variant):
    """A zero column is never started (``<b,b>`` is all-reduced: zero on every rank); its neighbours do not notice."""
    cases = ms.block_cases(8)
    zero = 5
    cols = [np.zeros_like(c.b) if j == zero else c.b for j, c in enumerate(cases)]
    recs = partitioned_block(hip, cols, 3, variant, LONG)
    assert recs[zero] == [None] * len(LONG)
    for j, c in enumerate(cases):
        if j != zero:
            check_steps(f"partitioned P=3 block of 8, column {zero} zero, kernel {variant}, column {j}", c, recs[j],
                        ms.reference(c, nsteps=LONG[-1]), steps=LONG)


# ---------------------------------------------------------------- exits
def _solve_on_ranks(hip, e, P, block_cols=None, block_variant=0):
    """``HipVector.solve`` (``block_cols``: ``solveBlock`` of these columns) of an exit case on P ranks:
    per rank ``[(slice of x, last_solve_stats, raised)]``, one entry per column."""
    def body(rank, ctx):
        H, (lo, hi) = rank_operator(hip, e.H, P, rank, ctx)
        H.set_block_variant(block_variant)
        vecs = [hip.HipVector(np.asarray(c)[lo:hi].copy(), _opts(e), ctx=ctx) for c in (block_cols or [e.b])]
        try:
            X = (hip.HipVector.solveBlock(H, vecs, e.sigma, reverseGF=e.sign < 0) if block_cols
                 else [hip.HipVector.solve(H, vecs[0], e.sigma, reverseGF=e.sign < 0)])
            return [(x.array, x.last_solve_stats, False) for x in X], H.block_info()["variant"]
        except UserWarning:                                      # not converged: the same on every rank, reported below
            return [(None, v.last_solve_stats, True) for v in vecs], H.block_info()["variant"]

    return on_ranks(P, body)


def _same_on_every_rank(res, label):
    """Every rank's statistics of every column are the same bits; returns ``[(x, stats)]`` per column."""
    def bits(st):
        return sorted((q, np.float64(v).tobytes()) for q, v in st.items())

    out = []
    for j, (_, st, raised) in enumerate(res[0][0]):
        assert not raised, (label, j, st)
        for r, (cols, _) in enumerate(res):
            assert not cols[j][2] and bits(cols[j][1]) == bits(st), (label, j, r, cols[j][1], st)
        out.append((np.concatenate([cols[j][0] for cols, _ in res]), st))
    return out


EXITS_ON_RANKS = [("eigenvector n=64", 2), ("istop 3 n=2", 2), ("istop 4 n=2", 2), ("1+test1 n=2", 2),
                  ("istop 3 n=1037", 3), ("1+test1 n=1037 d9", 3), ("istop 4 n=1037", 3), ("1+test1 n=1037 d3", 3)]


@pytest.mark.parametrize("name,P", EXITS_ON_RANKS)
def test_exits_on_ranks(hip, name, P):
    """Every rank reports the oracle's ``(itn, istop)``; the concatenated iterate is checked as on one GPU.  The
    partitioned run sees the stop of step K in KC of step K + 1: ``x`` must still be iterate K."""
    e = ms.EXITS[name]
    (x, st), = _same_on_every_rank(_solve_on_ranks(hip, e, P), name)
    assert "collectives" in st
    if name.startswith("eigenvector"):
        _check_eigenvector_solution(e, x, st, f"partitioned P={P}")
    else:
        _check_exit(e, x, st, f"partitioned P={P} {name}")


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("which", list(BLOCK_EXITS))
def test_exits_side_by_side_in_a_block_on_two_ranks(hip, which, variant):
    names = BLOCK_EXITS[which]
    first = ms.EXITS[names[0]]
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
    res = _solve_on_ranks(hip, first, 2, block_cols=cols, block_variant=variant)
    assert [kind for _, kind in res] == [hip.HipCsrOperator.BLOCK_VARIANTS[variant]] * 2
    for j, (nm, (xa, st)) in enumerate(zip(names, _same_on_every_rank(res, which))):
        label = f"partitioned P=2 block {which} kernel {variant} column {j}"
        if nm is None:
            assert (st["iterations"], st["istop"]) == (1, -1) and xa[1] == 0.0 and ms.deviation(xa[0], 3.0) <= 4.0, (label, st, xa)
        elif nm == "zero":
            assert st["iterations"] == 0 and not xa.any(), label
        else:
            _check_exit(ms.EXITS[nm], xa, st, label)
