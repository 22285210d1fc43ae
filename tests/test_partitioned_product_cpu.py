"""The row-partitioned products without a GPU: the restated layout code of tests/_partition_cases.py held to its
properties, a float64 emulation of a rank's product through it held to the bounds the GPU tests use
(tests/test_gpu_partitioned_products.py), and the seeded faults those bounds and exact checks catch.

The emulation takes the route of the C++: the ranks' slices are scattered into a gathered buffer whose every other position
- scalar slots, tails of the (rank, chunk) pieces - is NaN, the slab's global columns are remapped, and the column windows
are swept launch by launch in the order of ``hipeig_tcoow_plan``: sums handed on from launch to launch (``yinit``), or with
column splits one set of slabs per launch and a combine that adds them all; layout 5 with integer accumulators on the
plain exchange.  A row's adds run in a random order (LDS atomics fix none).  A read of anything that is not operand gives
NaN, and ``pc.error_ratio`` turns NaN into inf.
"""
import numpy as np
import pytest

import _hiprec as hp
import _partition_cases as pt
import _product_cases as pc

pytestmark = pytest.mark.skipif(not hp.EXTENDED, reason="longdouble is no wider than double on this machine")

SIGNS = (1.0, -1.0)
PRODUCTS = [(0.0, 0.0)] + [(s, g) for s in pc.REAL_SHIFTS for g in SIGNS]


# ================================================================ layout properties
def _random_partitions(count=300):
    rng = np.random.default_rng(20)
    for _ in range(count):
        P = int(rng.integers(2, 9))
        kind = rng.integers(0, 3)
        if kind == 0:                                        # slabs of any length from 1 row upward
            counts = rng.integers(1, 3000, P)
        elif kind == 1:                                      # one-row and very short slabs next to long ones
            counts = np.where(rng.random(P) < 0.5, rng.integers(1, 20, P), rng.integers(500, 5000, P))
        else:                                                # lengths at multiples of 16 and of the window, +-1
            counts = rng.choice([16, 32, 1024, 2048, 3072], P) + rng.integers(-1, 2, P)
        yield [int(c) for c in counts], int(rng.integers(1, 5))


def _table_partitions():
    for name, (_, cuts) in pt.PARTITIONS.items():
        for chunks in (1, 2, 3, 4):
            yield pt.counts_of(cuts), chunks


def _check_layout(counts, asked, wbits_list=(10, 6)):
    label = f"counts {counts}, {asked} chunks asked"
    P = len(counts)
    gl = pt.gather_layout(counts, asked)
    total = gl.total()
    assert 1 <= gl.nchunks <= min(asked, pt.MAX_CHUNKS) and gl.h % 16 == 0 and gl.h * gl.nchunks >= max(counts), label
    assert gl.nchunks == 1 or max(counts) // gl.nchunks >= 16, label
    # pos is injective and below total(); the vectorised remap is the scalar owner search and pos
    pos = pt.operand_positions(gl, counts)
    assert len(np.unique(pos)) == sum(counts) and pos.min() >= 0 and pos.max() < total, label
    cuts = np.concatenate([[0], np.cumsum(counts)])
    probe = np.unique(np.clip(np.concatenate([cuts[:-1], cuts[1:] - 1, cuts[:-1] + 1, [0, cuts[-1] - 1]]), 0, cuts[-1] - 1))
    for j in probe:
        r = pt.owner(list(cuts), int(j))
        assert cuts[r] <= j < cuts[r + 1], (label, j, r)
        assert gl.pos(r, int(j - cuts[r])) == pos[j], (label, j, r)
    # slots: 16 doubles each, inside the buffer, disjoint from each other and from every operand position
    held = np.zeros(total, dtype=np.int32)
    held[pos] += 1
    for r in range(P):
        assert 0 <= gl.slot(r) and gl.slot(r) + pt.SLOT <= total, label
        held[gl.slot(r):gl.slot(r) + pt.SLOT] += 1
    assert held.max() == 1, label
    chunk_of = np.searchsorted(np.asarray(gl.cbase[1:gl.nchunks + 1]), np.arange(total), side="right")
    for wbits in wbits_list:
        W = 1 << wbits
        nwin = (total + W - 1) >> wbits
        for r in range(P):
            sets = pt.window_sets(gl, r, counts[r], wbits, nwin)
            assert len(sets) == 1 + gl.nchunks and all(len(s) <= pt.MAX_RUNS for s in sets), (label, r, sets)
            seen = np.zeros(nwin, dtype=np.int32)
            for s in sets:
                for lo, hi in s:
                    assert 0 <= lo < hi <= nwin, (label, r, sets)
                    seen[lo:hi] += 1
            assert np.all(seen == 1), (label, r, wbits, sets)                  # [0, nwin) exactly once
            own = np.zeros(total + W, dtype=bool)
            own[pos[cuts[r]:cuts[r + 1]]] = True
            for lo, hi in sets[0]:                                             # set 0: wholly the rank's own rows
                assert hi * W <= total and own[lo * W:hi * W].all(), (label, r, wbits, sets)
            for k in range(gl.nchunks):                                        # set 1 + k: nothing of a later chunk
                for lo, hi in sets[1 + k]:
                    assert chunk_of[min(hi * W, total) - 1] <= k, (label, r, wbits, k, sets)


def test_layout_properties_on_the_table():
    for counts, chunks in _table_partitions():
        _check_layout(counts, chunks)


def test_layout_properties_on_random_partitions():
    n = 0
    for counts, chunks in _random_partitions():
        _check_layout(counts, chunks)
        n += 1
    assert n == 300


def test_the_table_holds_the_three_plan_shapes():
    """What the GPU parametrisation relies on: an overlapped plan with own windows, a rank whose set 0 is empty while
    several chunk sets are not, and the fall-back to the plain exchange."""
    gl, sets = pt.expected_sets("balanced3", 1)
    assert (gl.nchunks, gl.h, gl.total()) == (1, 3008, 9072)
    assert sets[0] == [[(0, 2)], [(2, 9)]] and pt.plan(sets[0], 1) == [[(0, 2)], [(2, 9)]]
    gl, sets = pt.expected_sets("balanced3", 3)
    assert (gl.nchunks, gl.h) == (3, 1008) and gl.h < 1 << pt.WBITS
    for s in sets:
        assert s[0] == [] and sum(1 for q in s[1:] if q) == 3 and pt.plan(s, 3) == s[1:]
    gl, sets = pt.expected_sets("unequal3", 1)
    assert sets[0][0] == [] and pt.plan(sets[0], 1) is None and pt.plan(sets[1], 1) is not None      # the 17-row slab
    gl, sets = pt.expected_sets("tiny3", 3)
    assert gl.nchunks == 1 and all(pt.plan(s, 1) is None for s in sets)
    gl, sets = pt.expected_sets("unequal5", 4)
    assert gl.nchunks == 4 and all(pt.plan(s, 4) is not None for s in sets)
    assert all(pt.plan(s, 1, overlap=False) is None and pt.plan(s, 1, fixed=True) is None for s in pt.expected_sets("balanced3", 1)[1])


# ================================================================ a rank's product, emulated
class _Fault:
    """What a seeded fault changes; every field off gives the code as it is."""
    owner_off_by_one = last_stride_h = window_twice = window_dropped = combine_skips_launch = yinit_dropped = False
    shift_rows_off = xmax_over_buffer = False

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(self, k)
            setattr(self, k, v)


def _remap(gl, cuts, col, fault):
    offs = np.asarray(cuts, np.int64)
    col = np.asarray(col, np.int64)
    r = np.searchsorted(offs[1:-1], col, side="left" if fault.owner_off_by_one else "right")
    i = col - offs[r]
    c = np.minimum(i // gl.h, gl.nchunks - 1)
    stride = np.where((c == gl.nchunks - 1) & (not fault.last_stride_h), gl.h + pt.SLOT, gl.h)
    return np.asarray(gl.cbase, np.int64)[c] + r * stride + (i - c * gl.h)


def _in_runs(win, runs):
    m = np.zeros(len(win), dtype=bool)
    for lo, hi in runs:
        m |= (win >= lo) & (win < hi)
    return m


def _ordered_add(acc, rows, t, rng):
    """acc[rows] += t, one entry after the other in a random order."""
    p = rng.permutation(len(t))
    np.add.at(acc, rows[p], t[p])


def emulate(case, cuts, rank, chunks, sigma, sign, rng, fixed=False, csplit=1, overlap=True, fault=_Fault(), slot_value=None):
    """``(y, X, launches)`` of one rank's product on the forced geometry (1024-column windows)."""
    counts = pt.counts_of(cuts)
    gl = pt.gather_layout(counts, chunks, overlap)
    buf = pt.scatter(gl, counts, case.x)
    if slot_value is not None:
        for r in range(len(counts)):
            buf[gl.slot(r)] = slot_value
    rowptr, col, val = case.csr
    rows = np.repeat(np.arange(case.nrows), case.lens)
    g = _remap(gl, cuts, col, fault)
    win = g >> pt.WBITS
    nwin = (gl.total() + (1 << pt.WBITS) - 1) >> pt.WBITS
    launches = pt.plan(pt.window_sets(gl, rank, case.nrows, pt.WBITS, nwin), gl.nchunks, overlap, fixed) or [[(0, nwin)]]
    masks = [_in_runs(win, runs) for runs in launches]
    if fault.window_twice:
        masks[-1] = masks[-1] | (win == launches[0][0][0])
    if fault.window_dropped:
        masks[0] = masks[0] & (win != launches[0][0][0])
    t = val * buf[g]
    X = None
    if fixed:
        R = pc.fixed_point_ingredients(rowptr, val, case.x)[0]
        X = float(np.max(np.abs(buf[pt.operand_positions(gl, counts)])))
        if fault.xmax_over_buffer:
            X = float(np.nanmax(np.abs(buf)))
        S = pc.fixed_point_scale(R, X)
        stray = ~np.isfinite(t)                               # a read of something that is not operand: the row is lost
        ti = np.rint(np.where(stray, 0.0, t) * S).astype(np.int64)
        share = win % csplit
        sums = np.zeros(case.nrows)
        for s in range(csplit):
            acc = np.zeros(case.nrows, dtype=np.int64)
            m = masks[0] & (share == s)
            np.add.at(acc, rows[m], ti[m])
            sums = sums + acc.astype(np.float64) * (1.0 / S)
        sums[rows[stray & masks[0]]] = np.nan
    elif csplit == 1:
        sums = np.zeros(case.nrows)
        for i, m in enumerate(masks):
            if fault.yinit_dropped and i == len(masks) - 1:
                sums = np.zeros(case.nrows)
            _ordered_add(sums, rows[m], t[m], rng)
    else:
        share = win % csplit
        slabs = []
        for m in masks:
            for s in range(csplit):
                acc = np.zeros(case.nrows)
                ms = m & (share == s)
                _ordered_add(acc, rows[ms], t[ms], rng)
                slabs.append(acc)
        if fault.combine_skips_launch:
            slabs = slabs[csplit:]
        sums = np.zeros(case.nrows)
        for s in slabs:
            sums = sums + s
    xl = case.x[:case.nrows] if fault.shift_rows_off else case.xl
    return pc.axpy_epilogue(sigma, sign, xl, sums), X, launches


def _ratio(case, sigma, sign, y, fixed, csplit):
    return pc.error_ratio(y, case.reference(sigma, sign), case.bound(sigma, sign, fixed=fixed, column_splits=csplit))


GEOMETRIES = [(chunks, csplit, fixed, overlap) for chunks in (1, 2, 3, 4) for csplit in (1, 3) for fixed in (False, True)
              for overlap in (True,)] + [(1, 1, False, False), (3, 3, False, False)]


@pytest.mark.parametrize("partition", list(pt.PARTITIONS))
@pytest.mark.parametrize("kind", ["edge", "ragged"])
def test_emulated_products_stay_within_their_bounds(kind, partition):
    _, cuts = pt.PARTITIONS[partition]
    rng = np.random.default_rng(7)
    worst, shapes = 0.0, set()
    for rank, case in enumerate(pt.cases(kind, partition)):
        for chunks, csplit, fixed, overlap in GEOMETRIES:
            for sigma, sign in PRODUCTS:
                y, X, launches = emulate(case, cuts, rank, chunks, sigma, sign, rng, fixed, csplit, overlap)
                worst = max(worst, _ratio(case, sigma, sign, y, fixed, csplit))
                want = np.zeros(int(case.empty.sum())) if sign == 0 else (sign * sigma) * case.xl[case.empty]
                assert np.array_equal(y[case.empty], want)
                shapes.add(len(launches))
            if fixed:
                assert X == float(np.max(np.abs(case.x)))
                if csplit == 1:
                    y, _, _ = emulate(case, cuts, rank, chunks, 0.0, 0.0, rng, True)
                    assert np.array_equal(y, pc.fixed_point_sums(*case.csr, case.x, pc.fixed_point_ingredients(case.csr[0], case.csr[2], case.x)[0]))
    print(f"\nemulated partitioned products, {kind} {partition}: max error / bound {worst:.3f}; launches per plan {sorted(shapes)}")
    assert worst <= 1.0
    if partition != "tiny3":
        assert max(shapes) >= 3


# ================================================================ seeded faults
def _caught(case, cuts, rank, chunks, fault, fixed=False, csplit=1, products=PRODUCTS, **kw):
    """Every product the fault changes exceeds its bound; returns the smallest excess."""
    rng = np.random.default_rng(11)
    low = np.inf
    for sigma, sign in products:
        y, _, _ = emulate(case, cuts, rank, chunks, sigma, sign, rng, fixed, csplit, fault=fault, **kw)
        r = _ratio(case, sigma, sign, y, fixed, csplit)
        assert r > 1.0, (case.name, chunks, csplit, sigma, sign, r)
        low = min(low, r)
    return low


FLOAT_FAULTS = {
    # fault: (chunks, csplit, products it changes)
    "owner_off_by_one": (1, 1, PRODUCTS), "last_stride_h": (3, 1, PRODUCTS), "window_twice": (3, 1, PRODUCTS),
    "window_dropped": (1, 1, PRODUCTS), "combine_skips_launch": (3, 3, PRODUCTS), "yinit_dropped": (1, 1, PRODUCTS),
    "shift_rows_off": (1, 1, [(s, g) for s, g in PRODUCTS if s != 0.0]),
}


@pytest.mark.parametrize("name", list(FLOAT_FAULTS))
@pytest.mark.parametrize("partition", ["balanced3", "unequal3"])
def test_seeded_faults_exceed_the_bound(partition, name):
    chunks, csplit, products = FLOAT_FAULTS[name]
    _, cuts = pt.PARTITIONS[partition]
    rank = 1                                                 # a slab with a row_offset and peers on both sides
    case = pt.cases("edge", partition)[rank]
    _, _, launches = emulate(case, cuts, rank, chunks, 0.0, 0.0, np.random.default_rng(1), csplit=csplit)
    assert len(launches) >= 2, "the fault needs a plan of several launches"
    if name == "owner_off_by_one":
        assert np.isin(case.csr[1], cuts[1:-1]).any(), "no stored column at a slab boundary"
    low = _caught(case, cuts, rank, chunks, _Fault(**{name: True}), csplit=csplit, products=products)
    if name in ("owner_off_by_one", "last_stride_h", "shift_rows_off"):         # what layout 5 shares with the others
        low = min(low, _caught(case, cuts, rank, chunks, _Fault(**{name: True}), fixed=True, products=products))
    print(f"\nseeded fault {name} on {partition}: smallest error / bound {low:.3g}")


@pytest.mark.parametrize("partition", ["balanced3", "unequal3"])
def test_a_slot_value_in_the_operand_maximum_breaks_the_exact_checks(partition):
    """The shares of <y,y> a MINRES solve leaves in the slots (here 1e6) taken into X: X is no longer max|x|, the scale
    moves by 2^20 and the sums are no longer those of ``pc.fixed_point_sums``; with the maximum taken over the operand
    entries the slot value changes nothing."""
    _, cuts = pt.PARTITIONS[partition]
    rng = np.random.default_rng(3)
    for rank, case in enumerate(pt.cases("edge", partition)):
        R = pc.fixed_point_ingredients(case.csr[0], case.csr[2], case.x)[0]
        sums = pc.fixed_point_sums(*case.csr, case.x, R)
        y, X, _ = emulate(case, cuts, rank, 3, 0.0, 0.0, rng, fixed=True, slot_value=1e6)
        assert X == float(np.max(np.abs(case.x))) and np.array_equal(y, sums)
        y, X, _ = emulate(case, cuts, rank, 3, 0.0, 0.0, rng, fixed=True, slot_value=1e6, fault=_Fault(xmax_over_buffer=True))
        assert X == 1e6 and not np.array_equal(y, sums)
