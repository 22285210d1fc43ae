"""The row-partitioned operator products against an extended-precision reference, row by row, on loopback ranks of one
GPU (``LoopbackGroup``).

A rank's product is code of its own - the column remap into the chunk-major gathered operand, the chunked exchange, the
plan that sweeps own windows under the exchange and then what each chunk completes, accumulators handed on through
``yinit`` or combined from one set of slabs per launch, the interleaved block exchange - and what a row holds in the end
does not depend on the partition.  So every rank's slab is a ``pc.RealCase`` (``_partition_cases.slab_cases``) and every
row is held to the proven bounds of tests/_product_cases.py: ``shift_bound`` (layouts 1 to 4 and the block products),
``fixed_point_bound`` (layout 5), ``shift_pair_bound`` (the pair products, which a partitioned context runs as two real
sweeps and two ``axpby``).  The mark is 1.0, nothing is fitted.  tests/test_partitioned_product_cpu.py holds a float64
emulation of the same route to the same bounds and shows the faults they catch.

Which plan a case takes is said by the restatement of the layout code in tests/_partition_cases.py, fed with what
``layout_info()`` reports, and asserted per rank: a change of defaults cannot quietly turn the cases into something else.
The geometry is forced small (64-row units, 1024-column windows; blocks 37 rows x 512 columns) so that N = 9001 has 9 or
more windows.  The communicator reads ``HIPEIG_GATHER_CHUNKS`` / ``HIPEIG_OVERLAP`` when it is attached and a layout its
knobs when it is first built: the environment is set before the group exists.

Every body of a rank makes library calls and returns what they gave; nothing is asserted before every rank has returned
and the group is closed, and no call depends on the rank.  Every rank holds at least one row.  Each test prints its
largest error / bound (pytest -s).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _hiprec as hp
import _partition_cases as pt
import _product_cases as pc
from _partition_cases import on_ranks
from eigensolvers_amd import _lib
from test_gpu_real_products import REPEATABLE, SIGNS, _check

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not hp.EXTENDED, reason="longdouble is no wider than double on this machine")]

U = pc.U
KINDS = ("edge", "ragged")
PRODUCTS = [(0.0, 0.0)] + [(s, g) for s in pc.REAL_SHIFTS for g in SIGNS]


def _environment(monkeypatch, chunks=0, csplit=1, overlap=True):
    for k in pt.ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**pt.SWEEP_KNOBS, **pt.BLOCK_KNOBS}.items():
        monkeypatch.setenv(k, v)
    if chunks:
        monkeypatch.setenv("HIPEIG_GATHER_CHUNKS", str(chunks))
    if csplit > 1:
        monkeypatch.setenv("HIPEIG_TCOOW_CSPLIT", str(csplit))
    if not overlap:
        monkeypatch.setenv("HIPEIG_OVERLAP", "0")


def _operator(hip, case, ctx):
    return hip.HipCsrOperator.from_csr_arrays(*case.csr, case.ncols, case.row_offset, ctx=ctx)


def _products(hip, H, xl, layout, products=PRODUCTS, twice=False):
    """``{(sigma, sign): y}`` of one operator on one layout (``twice``: every product a second time under ``"again"``), with
    what the operator reports afterwards.  Library calls only."""
    ctx = H.ctx
    H.set_variant(layout)

    def product(sigma, sign):
        if sign == 0:
            return xl.applyOp(H).array
        y = ctx.alloc(H.nrows)
        H.apply_shifted(sigma, xl._buf, y, reverse=sign < 0)
        return hip.HipVector(y).array

    out = {"y": {p: product(*p) for p in products}}
    if twice:
        out["again"] = {p: product(*p) for p in products}
    out["variant"], out["info"] = H.last_variant(), H.layout_info()
    out["fixed"] = H.fixed_point_info() if layout == 5 else None
    return out


def _shape(sets, nchunks, overlap, fixed):
    launches = pt.plan(sets, nchunks, overlap, fixed)
    return "plain" if launches is None else "own windows" if sets[0] else "chunk sets only"


def _check_rank(hip, case, label, layout, got, splits, P, rank, expected, overlap=True, exact_fixed=True):
    """One rank's products of one layout against reference and bound on every row; the layout, the exchange and the
    window sets are those the case was written for.  Returns (largest error / bound, plan shape)."""
    gl, sets = expected
    stored = len(case.csr[1]) > 0
    V = hip.HipCsrOperator.VARIANTS
    label = f"rank {rank}, {label}"
    assert got["variant"] == V[layout if stored or layout < 3 else 2], f"{case.name}, {label}: {got['variant']}"
    info = got["info"]
    assert (info["exchange_chunks"], info["rows_per_rank_chunk"]) == (gl.nchunks, gl.h), f"{label}: {info}"
    shape = None
    if layout >= 4 and stored:
        assert (info["column_splits"], info["window_bits"], info["rows_per_block"]) == (splits, pt.WBITS, 64), f"{label}: {info}"
        assert info["windows"] == (gl.total() + (1 << pt.WBITS) - 1) >> pt.WBITS, f"{label}: {info}"
        assert pt.sets_from_info(info, P, rank, case.nrows) == sets[rank], f"{label}: {info}"
        shape = _shape(sets[rank], gl.nchunks, overlap, layout == 5)
    fixed = layout == 5 and stored
    if fixed:                                                # the scale first: a wrong X explains the rows it spoils
        R, Xmax = got["fixed"]
        Rh, Xh = pc.fixed_point_ingredients(case.csr[0], case.csr[2], case.x)
        assert Xmax == Xh, f"{case.name}, {label}: X = {Xmax!r}, max|x| over the operand = {Xh!r}"
        assert abs(R - Rh) <= int(case.lens.max()) * U * Rh, (case.name, label, R, Rh)
    worst = 0.0
    for (sigma, sign), y in got["y"].items():
        worst = max(worst, _check(case, label, sigma, sign, y, fixed, splits))
        if "again" in got and layout in REPEATABLE:
            assert np.array_equal(y, got["again"][(sigma, sign)]), \
                f"{case.name}, {label}, sigma={sigma} sign={sign:+.0f}: the second call differs"
    if fixed:
        if exact_fixed and splits == 1:
            sums = pc.fixed_point_sums(*case.csr, case.x, R)
            for (sigma, sign), y in got["y"].items():
                assert np.array_equal(y, pc.axpy_epilogue(sigma, sign, case.xl, sums)), \
                    f"{case.name}, {label}, sigma={sigma} sign={sign:+.0f}: not the integer arithmetic bit for bit"
    return worst, shape


# ================================================================ a. real products on ranks
def _geometries():
    out = []
    for partition in pt.PARTITIONS:
        for chunks, csplit, overlap in [(1, 1, True), (2, 1, True), (3, 1, True), (4, 1, True), (1, 3, True), (3, 3, True),
                                        (1, 1, False), (3, 1, False)]:
            out.append((partition, (4,), chunks, csplit, overlap))
    for partition in ("balanced3", "unequal3"):
        for chunks in (1, 3):
            out.append((partition, (1, 2, 3), chunks, 1, True))
            for csplit in (1, 3):
                out.append((partition, (5,), chunks, csplit, True))
    return out


def _gid(g):
    partition, layouts, chunks, csplit, overlap = g
    return f"{partition}-layout{''.join(map(str, layouts))}-{chunks}chunks" + (f"-{csplit}splits" if csplit > 1 else "") + \
        ("" if overlap else "-overlap0")


GEOMETRIES = _geometries()


def _expected_shapes(g):
    """Per rank the plan shape the restatement gives for a parametrised case at the forced geometry."""
    partition, layouts, chunks, csplit, overlap = g
    gl, sets = pt.expected_sets(partition, chunks, overlap)
    return [_shape(s, gl.nchunks, overlap, 5 in layouts) for s in sets]


# the parametrisation holds the three plans: own windows under the exchange, chunk sets alone, the plain exchange
_SHAPES = {_gid(g): _expected_shapes(g) for g in GEOMETRIES if g[1] == (4,)}
assert "own windows" in _SHAPES["balanced3-layout4-1chunks"]
assert set(_SHAPES["balanced3-layout4-3chunks"]) == {"chunk sets only"}
assert _SHAPES["unequal3-layout4-1chunks"][0] == "plain" and set(_SHAPES["tiny3-layout4-3chunks"]) == {"plain"}
assert set(_SHAPES["balanced3-layout4-1chunks-overlap0"]) == {"plain"}


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=_gid)
def test_real_products_on_ranks(hip, monkeypatch, geometry):
    """``applyOp`` and ``apply_shifted`` with every shift and both signs on each rank's slab of both operators: every row
    under its bound, empty rows bit for bit, the layout, the chunk and split counts and the window sets as expected;
    layouts 1, 2, 3 and 5 repeat bit for bit; layout 5's X is max|x| over the N operand entries, its R the slab's, and
    without splits its product the integer emulation."""
    partition, layouts, chunks, csplit, overlap = geometry
    _environment(monkeypatch, chunks, csplit, overlap)
    n, cuts = pt.PARTITIONS[partition]
    P = len(cuts) - 1
    expected = pt.expected_sets(partition, chunks, overlap)
    assert expected[0].nchunks == (1 if partition == "tiny3" else chunks)
    slabs = {kind: pt.cases(kind, partition) for kind in KINDS}

    def body(rank, ctx):
        out = {}
        for kind in KINDS:
            case = slabs[kind][rank]
            H = _operator(hip, case, ctx)
            xl = hip.HipVector(case.xl.copy(), ctx=ctx)
            out[kind] = {layout: _products(hip, H, xl, layout, twice=layout in REPEATABLE) for layout in layouts}
            out[kind]["operand"] = xl.array
        return out

    res = on_ranks(P, body)
    worst, shapes = {}, []
    for kind in KINDS:
        for rank, case in enumerate(slabs[kind]):
            assert np.array_equal(res[rank][kind]["operand"], case.xl), f"{case.name}: the operand changed"
            for layout in layouts:
                label = f"layout {layout}, {chunks} chunks, {csplit} splits" + ("" if overlap else ", no overlap")
                r, shape = _check_rank(hip, case, label, layout, res[rank][kind][layout], csplit, P, rank, expected, overlap)
                worst[(kind, layout)] = max(worst.get((kind, layout), 0.0), r)
                if kind == "edge" and layout >= 4:
                    shapes.append(shape)
    if layouts == (4,):                                      # a rank of one row that stores nothing has no blocked copy
        assert [s for s in shapes if s] == [s for s, c in zip(_SHAPES[_gid(geometry)], slabs["edge"]) if len(c.csr[1])]
    print(f"\npartitioned products, {_gid(geometry)}: max error / bound " +
          ", ".join(f"{k} layout {v} {r:.3f}" for (k, v), r in sorted(worst.items())) + f"; plans {shapes}")


# ================================================================ b. what is not operand stays out
@functools.lru_cache(maxsize=None)
def _symmetric():
    """``edge_matrix(9001)`` plus its transpose: an operator MINRES may be given."""
    A = pc.edge_matrix(pt.N, seed=pt.N)
    S = sp.csr_matrix(A + A.T)
    S.sort_indices()
    return S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data.copy()


def test_the_slots_of_a_minres_solve_stay_out_of_the_fixed_point_maximum(hip, monkeypatch):
    """A partitioned layout-5 MINRES solve leaves every rank's share of <y,y> in its scalar slot of the gathered buffer,
    and every later exchange carries the slots along.  A product of the same operator with an operand of order 1e-6
    must still take X = max|x| over the operand entries - exactly - and meet the integer emulation bit for bit."""
    partition, chunks = "balanced3", 3
    _environment(monkeypatch, chunks)
    n, cuts = pt.PARTITIONS[partition]
    P = len(cuts) - 1
    x = pc.real_operand(n, seed=5)
    small = x * 1e-6
    rhs = pt.slab_cases(_symmetric(), x, cuts, "symmetric edge")
    slabs = pt.slab_cases(_symmetric(), small, cuts, "symmetric edge, operand 1e-6")

    def body(rank, ctx):
        case = slabs[rank]
        H = _operator(hip, case, ctx)
        H.set_variant(5)
        b = hip.HipVector(rhs[rank].xl.copy(), ctx=ctx)
        xb = ctx.alloc(case.nrows)
        info, st = C.c_int(-1), (C.c_double * 8)()
        _lib.call("hipeig_minres", ctx.handle, H.handle, 0.02, 1.0, b._buf.ptr, xb.ptr, 0.0, 6, C.byref(info), st)
        solve_variant = H.last_variant()
        out = _products(hip, H, hip.HipVector(case.xl.copy(), ctx=ctx), 5, products=PRODUCTS[:3])
        out["solve"] = (solve_variant, int(st[0]), hip.HipVector(xb).array)
        return out

    res = on_ranks(P, body)
    expected = pt.expected_sets(partition, chunks)
    worst = 0.0
    for rank, case in enumerate(slabs):
        kind, itn, xk = res[rank]["solve"]
        assert kind == hip.HipCsrOperator.VARIANTS[5] and itn == 6 and np.all(np.isfinite(xk)) and xk.any(), (rank, kind, itn)
        r, _ = _check_rank(hip, case, "after a solve", 5, res[rank], 1, P, rank, expected)
        worst = max(worst, r)
    print(f"\npartitioned products, layout 5 after a MINRES solve, operand of order 1e-6: max error / bound {worst:.3f}")


B_CUTS = (0, 100, 3100, 6000)


def test_an_earlier_operators_operand_stays_out(hip, monkeypatch):
    """Two operators on the same contexts.  A (9001 rows, balanced, 1 chunk) runs one product with a NaN operand; B
    (6000 rows, unequal slabs, 2 chunks) needs no longer a buffer, so nothing is reallocated or cleared, and tails of its
    (rank, chunk) pieces - positions no exchange of B writes - lie where A's operand rows were.  B's products on every
    layout are finite and within their bounds, and layout 5's X is max|x| of B's operand exactly."""
    _environment(monkeypatch, 1)
    nA, cutsA = pt.PARTITIONS["balanced3"]
    P = len(cutsA) - 1
    countsA, countsB = pt.counts_of(cutsA), pt.counts_of(B_CUTS)
    glA, glB = pt.gather_layout(countsA, 1), pt.gather_layout(countsB, 2)
    assert glB.nchunks == 2 and glB.total() <= glA.total()              # B fits the buffer A sized: no new, zeroed one
    heldA = np.zeros(glA.total(), dtype=bool)
    heldA[pt.operand_positions(glA, countsA)] = True
    heldB = np.zeros(glB.total(), dtype=bool)
    heldB[pt.operand_positions(glB, countsB)] = True
    slotsB = np.zeros(glB.total(), dtype=bool)
    for r in range(P):
        slotsB[glB.slot(r):glB.slot(r) + pt.SLOT] = True
    stale = ~heldB & heldA[:glB.total()]
    assert stale.sum() >= 1000 and (stale & ~slotsB).any() and (stale & slotsB).any()       # tails and slots over A's rows
    slabsA = pt.cases("edge", "balanced3")
    slabsB = pt.slab_cases(pt.operator("edge", 6000), pc.real_operand(6000, seed=6), B_CUTS, "edge 6000 after a NaN operand")

    def body(rank, ctx):
        HA = _operator(hip, slabsA[rank], ctx)
        HA.set_variant(2)
        hip.HipVector(np.full(slabsA[rank].nrows, np.nan), ctx=ctx).applyOp(HA)
        ctx.set_gather_chunks(2)
        case = slabsB[rank]
        HB = _operator(hip, case, ctx)
        xl = hip.HipVector(case.xl.copy(), ctx=ctx)
        return {layout: _products(hip, HB, xl, layout, products=PRODUCTS[:3]) for layout in (1, 2, 3, 4, 5)}

    res = on_ranks(P, body)
    nwin = (glB.total() + (1 << pt.WBITS) - 1) >> pt.WBITS
    expected = (glB, [pt.window_sets(glB, r, countsB[r], pt.WBITS, nwin) for r in range(P)])
    worst = {}
    for rank, case in enumerate(slabsB):
        for layout in (1, 2, 3, 4, 5):
            r, _ = _check_rank(hip, case, f"layout {layout}", layout, res[rank][layout], 1, P, rank, expected)
            worst[layout] = max(worst.get(layout, 0.0), r)
    print("\npartitioned products, a second operator after a NaN operand: max error / bound " +
          ", ".join(f"layout {k} {v:.3f}" for k, v in sorted(worst.items())))


# ================================================================ c. pair products on ranks
@functools.lru_cache(maxsize=None)
def _pair_operands():
    return pc.complex_operands(pt.N, count=3, seed=8)


@functools.lru_cache(maxsize=None)
def _half_products(kind, partition, rank, p):
    case = pt.cases(kind, partition)[rank]
    return pc.half_products(*case.csr, *_pair_operands()[p])


def _check_pair(kind, partition, rank, p, z, sign, got, label):
    case = pt.cases(kind, partition)[rank]
    args = (*case.csr, *_pair_operands()[p], z, sign, case.row_offset, _half_products(kind, partition, rank, p))
    worst = 0.0
    for half, g, ref, b in zip(("re", "im"), got, pc.shift_pair_reference(*args), pc.shift_pair_bound(*args)):
        assert g.shape == b.shape
        r = pc.error_ratio(g, ref, b)
        assert r <= 1.0, f"{label}, operand {p}, z={complex(z)} sign={sign:+.0f}, {half} half: error / bound {r:.3g}"
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("partition", ["balanced3", "unequal3"])
@pytest.mark.parametrize("layout", [2, 4])
def test_pair_products_on_ranks(hip, monkeypatch, layout, partition):
    """``apply_shifted_pair``, and ``apply_shifted_pairs`` with one shift and with a shift per operand (a partitioned
    context takes the per-operand path for both: two real sweeps and two ``axpby``): every shift of ``pc.SHIFTS`` -
    ``zi = 0`` and ``z = 0`` among them - and both signs, both halves under ``shift_pair_bound`` with the slab's
    ``row_offset``, 2 chunks."""
    _environment(monkeypatch, 2)
    n, cuts = pt.PARTITIONS[partition]
    P = len(cuts) - 1
    ops = _pair_operands()
    rotations = [tuple(pc.SHIFTS[(i + j) % len(pc.SHIFTS)] for j in range(3)) for i in (0, 3)]

    def body(rank, ctx):
        case = pt.cases("ragged", partition)[rank]
        lo, hi = case.row_offset, case.row_offset + case.nrows
        H = _operator(hip, case, ctx)
        H.set_variant(layout)
        X = [(hip.HipVector(xr[lo:hi].copy(), ctx=ctx)._buf, hip.HipVector(xi[lo:hi].copy(), ctx=ctx)._buf) for xr, xi in ops]

        def host(y):
            return hip.HipVector(y[0]).array, hip.HipVector(y[1]).array

        out = {}
        for sign in SIGNS:
            for z in pc.SHIFTS:
                yr, yi = ctx.alloc(case.nrows), ctx.alloc(case.nrows)
                H.apply_shifted_pair(z, *X[0], yr, yi, reverse=sign < 0)
                out[("pair", z, sign)] = [host((yr, yi))]
                out[("pairs", z, sign)] = [host(y) for y in H.apply_shifted_pairs(z, X[:2], reverse=sign < 0)]
            for zs in rotations:
                out[("pairs_z", zs, sign)] = [host(y) for y in H.apply_shifted_pairs(list(zs), X, reverse=sign < 0)]
        return out, H.last_variant(), H.layout_info()

    res = on_ranks(P, body)
    gl = pt.expected_sets(partition, 2)[0]
    worst = {}
    for rank in range(P):
        out, kind, info = res[rank]
        assert kind == hip.HipCsrOperator.VARIANTS[layout] and info["exchange_chunks"] == gl.nchunks == 2, (rank, kind, info)
        for (form, z, sign), ys in out.items():
            for p, y in enumerate(ys):
                zp = z[p] if form == "pairs_z" else z
                r = _check_pair("ragged", partition, rank, p, zp, sign, y, f"ragged {partition} rank {rank} layout {layout} {form}")
                worst[form] = max(worst.get(form, 0.0), r)
    print(f"\npartitioned pair products, {partition}, layout {layout}, 2 chunks: max error / bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ================================================================ d. block products on ranks
WIDTHS = (3, 8, 11)                                          # a 4-wide pass, an 8-wide one, 8 + 3


@functools.lru_cache(maxsize=None)
def _block_cases(partition, column):
    n, cuts = pt.PARTITIONS[partition]
    return tuple(pt.slab_cases(pt.operator("ragged", n), pc.real_operand(n, seed=100 + column), cuts, f"ragged {partition} column {column}"))


@pytest.mark.parametrize("partition", ["balanced2", "balanced3", "unequal3"])
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("variant", [1, 2])
def test_block_products_on_ranks(hip, monkeypatch, variant, chunks, partition):
    """``apply_block`` and ``apply_shifted_block`` of 3, 8 and 11 operands (the interleaved block exchange, 4 and 8 wide):
    every column under ``shift_bound`` of its own operand, rows that store nothing hold the shift term alone, and the
    row-owner kernel repeats bit for bit."""
    _environment(monkeypatch, chunks)
    n, cuts = pt.PARTITIONS[partition]
    P = len(cuts) - 1
    products = [(0.0, 0.0)] + [(s, g) for s in pc.REAL_SHIFTS[:3] for g in SIGNS]

    def body(rank, ctx):
        cols = [_block_cases(partition, j)[rank] for j in range(max(WIDTHS))]
        H = _operator(hip, cols[0], ctx)
        H.set_block_variant(variant)
        X = [hip.HipVector(c.xl.copy(), ctx=ctx)._buf for c in cols]

        def product(k, sigma, sign):
            ys = H.apply_block(X[:k]) if sign == 0 else H.apply_shifted_block(sigma, X[:k], reverse=sign < 0)
            return [hip.HipVector(y).array for y in ys]

        out = {(k, p): product(k, *p) for k in WIDTHS for p in products}
        again = {(k, p): product(k, *p) for k in WIDTHS for p in products[:3]} if variant == 1 else {}
        return out, again, H.block_info(), H.layout_info()

    res = on_ranks(P, body)
    gl = pt.expected_sets(partition, chunks)[0]
    worst = {}
    for rank in range(P):
        out, again, binfo, info = res[rank]
        assert binfo["variant"] == hip.HipCsrOperator.BLOCK_VARIANTS[variant], (rank, binfo)
        if variant == 2:
            assert (binfo["rows_per_block"], binfo["windows"]) == (37, (gl.total() + 511) >> 9), (rank, binfo)
        assert (info["exchange_chunks"], info["rows_per_rank_chunk"]) == (gl.nchunks, gl.h) and gl.nchunks == chunks, (rank, info)
        for (k, (sigma, sign)), ys in out.items():
            assert len(ys) == k
            for j, y in enumerate(ys):
                case = _block_cases(partition, j)[rank]
                r = _check(case, f"block kernel {variant}, k={k}, {chunks} chunks", sigma, sign, y, False, 1)
                worst[k] = max(worst.get(k, 0.0), r)
        for key, ys in again.items():
            assert all(np.array_equal(a, b) for a, b in zip(ys, out[key])), f"rank {rank} {key}: the second call differs"
    print(f"\npartitioned block products, {partition}, kernel {variant}, {chunks} chunks: max error / bound " +
          ", ".join(f"k={k} {v:.3f}" for k, v in sorted(worst.items())))


# ================================================================ e. two operators alternating on one group
def test_two_operators_alternating_on_one_group(hip, monkeypatch):
    """Layout 4; A on 3 chunks (9001 rows, balanced: chunk sets only), B on 1 chunk (6000 rows, unequal slabs: own windows
    and, on the 100-row slab, the plain exchange).  The contexts' gathered buffer and partial-sum slabs are shared: products
    A, B, A, B are each within bound, so nothing of one layout reaches the other."""
    _environment(monkeypatch, 3)
    n, cuts = pt.PARTITIONS["balanced3"]
    P = len(cuts) - 1
    slabsA = pt.cases("ragged", "balanced3")
    slabsB = pt.slab_cases(pt.operator("edge", 6000), pc.real_operand(6000, seed=6), B_CUTS, "edge 6000, 1 chunk")
    products = PRODUCTS[:3]

    def body(rank, ctx):
        HA = _operator(hip, slabsA[rank], ctx)
        ctx.set_gather_chunks(1)
        HB = _operator(hip, slabsB[rank], ctx)
        xa = hip.HipVector(slabsA[rank].xl.copy(), ctx=ctx)
        xb = hip.HipVector(slabsB[rank].xl.copy(), ctx=ctx)
        return [_products(hip, H, x, 4, products=products) for H, x in ((HA, xa), (HB, xb), (HA, xa), (HB, xb))]

    res = on_ranks(P, body)
    countsB = pt.counts_of(B_CUTS)
    glB = pt.gather_layout(countsB, 1)
    nwinB = (glB.total() + (1 << pt.WBITS) - 1) >> pt.WBITS
    expected = [pt.expected_sets("balanced3", 3), (glB, [pt.window_sets(glB, r, countsB[r], pt.WBITS, nwinB) for r in range(P)])]
    worst, shapes = [0.0] * 4, []
    for rank in range(P):
        for i, got in enumerate(res[rank]):
            case = (slabsA, slabsB)[i % 2][rank]
            r, shape = _check_rank(hip, case, f"product {i}", 4, got, 1, P, rank, expected[i % 2])
            worst[i] = max(worst[i], r)
            shapes.append(shape)
    assert {"chunk sets only", "own windows", "plain"} == set(shapes), shapes
    print("\npartitioned products, two operators alternating: max error / bound A, B, A, B " + ", ".join(f"{w:.3f}" for w in worst))
