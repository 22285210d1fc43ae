"""Reference and row bounds of the real products (tests/_product_cases.py), checked on the host.

The reference against exact rational arithmetic and each bound's formula by hand; then a float64 emulation of what each
sweep layout does with a row - an ``fma`` chain per lane and the ``__shfl_down`` tree (layout 1), rounded products, a sum
per lane and the same tree, or the whole-workgroup path of a row beyond 2048 entries (layout 2), adds in a random order
(layouts 3 and 4), shares of a unit's stream cut at multiples of 256 and added in order (column splits), the exact
integer arithmetic (layout 5, with and without splits) - on every operator and shift of the device test.  An emulation
must stay at or below 1.0 of its layout's bound on every row, and each seeded fault - injected here, in the emulation
only - must exceed it on at least one row, on every operator, for every layout's bound and every product the fault
changes.  fma(a, b, c) goes through the extended format where there is one (as in test_hiprec_cpu.py), else a * b + c.
"""
from fractions import Fraction

import numpy as np
import pytest

import _hiprec as hp
import _product_cases as pc

SIGNS = (1.0, -1.0)
PRODUCTS = [(0.0, 0.0)] + [(s, g) for s in pc.REAL_SHIFTS for g in SIGNS]       # (sigma, sign); sign 0: plain product
RW, WBITS, CSPLIT = 64, 10, 3                                                    # the forced geometry of the device test
KINDS = ("layout 1", "layout 2", "random order", "column splits", "fixed point", "fixed point, column splits")
CASES = [*pc.REAL_OPERATORS] + [lambda a=a: pc.tiny(*a) for a in pc.TINY]
CASE_IDS = [f.__name__ for f in pc.REAL_OPERATORS] + [f"tiny{n}{'' if st else 'empty'}" for n, st in pc.TINY]
FAULT_CASES = [*pc.REAL_OPERATORS, lambda: pc.tiny(65)]


def _fma(a, b, c):
    if not hp.EXTENDED:
        return a * b + c
    return (np.asarray(a, hp.LD) * np.asarray(b, hp.LD) + np.asarray(c, hp.LD)).astype(np.float64)


def _frac(v):
    return Fraction(*np.longdouble(v).as_integer_ratio())


# ---------------------------------------------------------------- reference and formulas
def test_reference_against_fractions():
    """n = 12 with an empty row, a duplicate column and unsorted columns; both signs and the plain product; rows 3..8 as a
    slab applied to the full-length operand."""
    rng = np.random.default_rng(12)
    n = 12
    lens = rng.integers(1, 6, n)
    lens[4], lens[7] = 0, 4
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([rng.choice(n, L, replace=False) for L in lens]).astype(np.int32)
    col[rowptr[7] + 1] = col[rowptr[7]]                                  # row 7 stores a column twice
    assert any(np.any(np.diff(col[rowptr[i]:rowptr[i + 1]]) < 0) for i in range(n))
    val = rng.standard_normal(rowptr[-1]) * np.exp(rng.uniform(-3, 3, rowptr[-1]))
    x = pc.real_operand(n)
    sigma = 0.37
    F = lambda v: Fraction(float(v))

    def exact(i, sign):
        ks = range(rowptr[i], rowptr[i + 1])
        s = sum((F(val[k]) * F(x[col[k]]) for k in ks), Fraction(0))
        mag = sum((abs(F(val[k]) * F(x[col[k]])) for k in ks), Fraction(0))
        if sign == 0:
            return s, mag
        return Fraction(int(sign)) * (F(sigma) * F(x[i]) - s), mag + abs(F(sigma) * F(x[i]))

    for sign in (1.0, -1.0, 0.0):
        y = pc.shift_reference(rowptr, col, val, x, sigma, sign)
        for i in range(n):
            e, mag = exact(i, sign)
            assert abs(_frac(y[i]) - e) <= 2.0 ** -60 * mag, (sign, i)
    assert pc.shift_reference(rowptr, col, val, x, sigma, 0.0)[4] == 0 and pc.shift_bound(rowptr, col, val, x, sigma, 0.0)[4] == 1e-300
    rp = rowptr[3:10] - rowptr[3]
    c, v = col[rowptr[3]:rowptr[9]], val[rowptr[3]:rowptr[9]]
    for sign in SIGNS:
        y = pc.shift_reference(rp, c, v, x, sigma, sign, row_offset=3)
        assert len(y) == len(pc.shift_bound(rp, c, v, x, sigma, sign, row_offset=3)) == 6
        assert len(pc.fixed_point_bound(rp, c, v, x, sigma, sign, row_offset=3)) == 6
        for i in range(6):
            e, mag = exact(i + 3, sign)
            assert abs(_frac(y[i]) - e) <= 2.0 ** -60 * mag


def test_bound_terms():
    """Each formula on a three-row operator by hand; an empty row's bound holds the shift term only."""
    rowptr, col, val = np.array([0, 2, 2, 3]), np.array([2, 0, 1]), np.array([2.0, -3.0, 0.5])
    x = np.array([1.0, -2.0, 4.0])
    u = 2.0 ** -53
    absx = [2 * 4 + 3 * 1, 0.0, 0.5 * 2]
    b = pc.shift_bound(rowptr, col, val, x, -3.0, 1.0)
    assert b[0] == pytest.approx(1.01 * u * (4 * absx[0] + 2 * 3 * 1), rel=1e-15)
    assert b[1] == pytest.approx(1.01 * u * 2 * 3 * 2, rel=1e-15)                        # empty row: the shift term alone
    assert b[2] == pytest.approx(1.01 * u * (3 * absx[2] + 2 * 3 * 4), rel=1e-15)
    p = pc.shift_bound(rowptr, col, val, x, -3.0, 0.0)
    assert p[0] == pytest.approx(1.01 * u * 3 * absx[0], rel=1e-15) and p[1] == 1e-300
    assert p[2] == pytest.approx(1.01 * u * 2 * absx[2], rel=1e-15)
    # a slab: the shift term reads the operand from row_offset on
    bs = pc.shift_bound(rowptr[:2], col[:2], val[:2], x, -3.0, -1.0, row_offset=2)
    assert bs[0] == pytest.approx(1.01 * u * (4 * absx[0] + 2 * 3 * 4), rel=1e-15)
    R, X = pc.fixed_point_ingredients(rowptr, val, x)
    assert (R, X) == (5.0, 4.0)
    q = 2.0 ** -60 * 20.0
    f = pc.fixed_point_bound(rowptr, col, val, x, -3.0, 1.0)
    assert f[0] == pytest.approx(1.01 * (1.0 * q + 3 * u * absx[0] + 2 * u * 3 * 1), rel=1e-15)
    assert f[1] == pytest.approx(1.01 * 2 * u * 3 * 2, rel=1e-15)
    assert f[2] == pytest.approx(1.01 * (0.5 * q + 3 * u * absx[2] + 2 * u * 3 * 4), rel=1e-15)
    fp = pc.fixed_point_bound(rowptr, col, val, x, -3.0, 0.0)
    assert fp[0] == pytest.approx(1.01 * (1.0 * q + 2 * u * absx[0]), rel=1e-15) and fp[1] == 1e-300
    f3 = pc.fixed_point_bound(rowptr, col, val, x, -3.0, 0.0, column_splits=3)           # shares: min(3, L_i)
    assert f3[0] == pytest.approx(1.01 * (1.0 * q + 3 * u * absx[0]), rel=1e-15)
    assert f3[2] == pytest.approx(1.01 * (0.5 * q + 2 * u * absx[2]), rel=1e-15) and f3[1] == 1e-300
    # the scale: one accumulator unit is at most 2^-60 R X, and the sums are the integer arithmetic
    for R_, X_ in ((5.0, 4.0), (1.0, 1.0), (0.999, 1.0), (3e5, 31.0)):
        S = pc.fixed_point_scale(R_, X_)
        assert 1.0 / S <= 2.0 ** -60 * R_ * X_ and R_ * X_ * S < 2.0 ** 61
    S = pc.fixed_point_scale(R, X)
    assert pc.fixed_point_sums(rowptr, col, val, x, R)[0] == float(int(np.rint(8.0 * S)) + int(np.rint(-3.0 * S))) / S
    assert np.array_equal(pc.axpy_epilogue(-3.0, -1.0, x, np.array([5.0, 0.0, -1.0])), 3.0 * x + np.array([5.0, 0.0, -1.0]))
    assert np.array_equal(pc.axpy_epilogue(9.0, 0.0, x, np.array([5.0, 0.0, -1.0])), [5.0, 0.0, -1.0])


@pytest.mark.parametrize("build", CASES, ids=CASE_IDS)
def test_operator_classes(build):
    """The builders' class asserts hold (they run inside the builders), columns are unsorted with duplicates kept, and
    the edge rows of ``stream_edges`` are where the CSR-stream kernel's blocks turn."""
    c = build()
    assert c.lanes == pc.lanes_per_row(c.csr[0]) and len(c.x) == c.ncols and len(c.xl) == c.nrows
    if c.name == "stream_edges":
        assert [int(c.lens[i]) for i in (0, 100, 101, 102, 3000, 3999)] == [0, 2048, 2049, 2047, 4097, 2049]
        assert np.all(c.lens[1500:2700] == 0) and c.nrows == 4000
    if c.name in ("lanes4", "lanes16", "lanes32", "lanes64", "stream_edges"):
        rp, col, _ = c.csr
        rows = np.flatnonzero(c.lens >= 30)[:50] if c.lens.max() >= 30 else np.flatnonzero(c.lens >= 2)
        assert any(np.any(np.diff(col[rp[i]:rp[i + 1]]) < 0) for i in rows)
        if c.lens.max() >= 30:
            assert any(len(set(col[rp[i]:rp[i + 1]])) < c.lens[i] for i in rows)


# ---------------------------------------------------------------- float64 emulation of the layouts
def _rows_of_entries(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def _lane_partials(csr, x, group, fused):
    """(n, group) lane partials: lane l of a row's group takes entries l, l + group, ... in order, as an fma chain
    (``csr_vector_sweep``) or as rounded products added to the lane's sum (``csr_stream_sweep``, LDS path)."""
    rowptr, col, val = csr
    n = len(rowptr) - 1
    L = np.diff(rowptr)
    S = np.zeros((n, group))
    lane = np.arange(group)
    for j in range(-(-int(L.max(initial=0)) // group)):
        act = np.flatnonzero(L > j * group)
        idx = rowptr[act, None] + j * group + lane
        mask = idx < rowptr[act + 1, None]
        idx = np.where(mask, idx, 0)
        v, xx, cur = val[idx], x[col[idx]], S[act]
        S[act] = np.where(mask, _fma(v, xx, cur) if fused else cur + v * xx, cur)
    return S


def _tree(S):
    """``group_reduce_sum``: v += __shfl_down(v, off) for off = group / 2 .. 1; lane 0 holds the sum."""
    S = S.copy()
    off = S.shape[1] >> 1
    while off:
        S[:, :off] += S[:, off:2 * off]
        off >>= 1
    return S[:, 0]


def _workgroup_row(v, xg):
    """A row beyond 2048 entries in ``csr_stream_sweep``: 256 fma chains with stride 256, ``wave_reduce_sum`` in each of
    the four waves, the four sums added in order (``block_reduce_sum``)."""
    S = np.zeros(256)
    for j in range(-(-len(v) // 256)):
        seg = slice(256 * j, min(256 * (j + 1), len(v)))
        k = seg.stop - seg.start
        S[:k] = _fma(v[seg], xg[seg], S[:k])
    w = _tree(S.reshape(4, 64))
    return ((w[0] + w[1]) + w[2]) + w[3]


def _lanes(csr, x, group, kind, drop_lane_rows=()):
    rowptr, col, val = csr
    S = _lane_partials(csr, x, group, fused=kind == "layout 1")
    for r in drop_lane_rows:
        S[r, group - 1] = 0.0                                            # fault: lane group - 1 never enters the tree
    out = _tree(S)
    if kind == "layout 2":
        for r in np.flatnonzero(np.diff(rowptr) > pc.STREAM_NNZ_PER_BLOCK):
            a, b = rowptr[r], rowptr[r + 1]
            out[r] = _workgroup_row(val[a:b], x[col[a:b]])
    return out


def _random_order(csr, x, rng, init=None):
    """Adds of a row in a random order into an accumulator that starts at zero (np.add.at adds in sequence)."""
    rowptr, col, val = csr
    out = np.zeros(len(rowptr) - 1) if init is None else init.copy()
    p = rng.permutation(len(col))
    np.add.at(out, _rows_of_entries(rowptr)[p], (val * x[col])[p])
    return out


def _shares(csr, rng):
    """(order, share, rows): the entries of every RW-row unit as one stream - window after window, any order inside a
    window - cut into CSPLIT shares at multiples of 256 (``tcoo_wg_sweep``: len * s / csplit & ~255, the last share to the
    end); ``share[k]``, ``rows[k]`` belong to entry ``order[k]``."""
    rowptr, col, _ = csr
    rows = _rows_of_entries(rowptr)
    unit = rows // RW
    order = np.lexsort((rng.random(len(col)), col >> WBITS, unit))
    u = unit[order]
    nunits = -(-(len(rowptr) - 1) // RW)
    length = np.bincount(u, minlength=nunits)
    start = np.concatenate([[0], np.cumsum(length)])[:-1]
    pos = np.arange(len(col)) - start[u]
    share = np.zeros(len(col), dtype=np.int64)
    for s in range(1, CSPLIT):
        share += pos >= ((length * s // CSPLIT) & ~255)[u]
    return order, share, rows[order]


def _column_splits(csr, x, rng):
    rowptr, col, val = csr
    order, share, rows = _shares(csr, rng)
    t = (val * x[col])[order]
    parts = np.zeros((CSPLIT, len(rowptr) - 1))
    for s in range(CSPLIT):
        np.add.at(parts[s], rows[share == s], t[share == s])
    out = parts[0].copy()
    for s in range(1, CSPLIT):                                           # tcoow_combine_sweep
        out = out + parts[s]
    return out


def _fixed_ints(csr, x, S):
    rowptr, col, val = csr
    out = np.zeros(len(rowptr) - 1, dtype=np.int64)
    np.add.at(out, _rows_of_entries(rowptr), pc.fixed_point_terms(col, val, x, S))
    return out


def _fixed(csr, x, S, init=None):
    ints = _fixed_ints(csr, x, S)
    return (ints if init is None else ints + init).astype(np.float64) * (1.0 / S)


def _fixed_splits(csr, x, S, rng):
    rowptr, col, val = csr
    order, share, rows = _shares(csr, rng)
    t = pc.fixed_point_terms(col, val, x, S)[order]
    out = None
    for s in range(CSPLIT):
        part = np.zeros(len(rowptr) - 1, dtype=np.int64)
        np.add.at(part, rows[share == s], t[share == s])
        part = part.astype(np.float64) * (1.0 / S)                      # every share leaves the sweep as a double
        out = part if out is None else out + part
    return out


def _scale(case):
    return pc.fixed_point_scale(*pc.fixed_point_ingredients(case.csr[0], case.csr[2], case.x))


def _emulate(kind, case, csr, rng, **fault):
    """Row sums of ``csr`` (the case's arrays, or a faulty copy of them) applied to the case's operand."""
    x = case.x
    if kind in ("layout 1", "layout 2"):
        return _lanes(csr, x, case.lanes, kind, **fault)
    if kind == "random order":
        return _random_order(csr, x, rng, **fault)
    if kind == "column splits":
        return _column_splits(csr, x, rng)
    if kind == "fixed point":
        return _fixed(csr, x, _scale(case), **fault)
    return _fixed_splits(csr, x, _scale(case), rng)


_CLEAN = {}


def _clean(case):
    if case.name not in _CLEAN:
        rng = np.random.default_rng(5)
        _CLEAN[case.name] = {kind: _emulate(kind, case, case.csr, rng) for kind in KINDS}
    return _CLEAN[case.name]


def _bound(case, kind, sigma, sign):
    if kind.startswith("fixed point"):
        return case.bound(sigma, sign, fixed=True, column_splits=CSPLIT if kind.endswith("splits") else 1)
    return case.bound(sigma, sign)


def _ratio(case, kind, sigma, sign, y):
    return pc.error_ratio(y, case.reference(sigma, sign), _bound(case, kind, sigma, sign))


@pytest.mark.parametrize("build", CASES, ids=CASE_IDS)
def test_emulated_layouts_stay_within_their_bounds(build):
    case = build()
    sums = _clean(case)
    worst = dict.fromkeys(KINDS, 0.0)
    for kind in KINDS:
        assert np.all(sums[kind][case.empty] == 0.0)
        for sigma, sign in PRODUCTS:
            y = pc.axpy_epilogue(sigma, sign, case.xl, sums[kind])
            worst[kind] = max(worst[kind], _ratio(case, kind, sigma, sign, y))
    print(f"\n{case.name} ({case.lanes} lanes), float64 emulation, max error / bound:", {k: round(v, 3) for k, v in worst.items()})
    for kind, r in worst.items():
        assert r <= 1.0, f"{case.name}, {kind}: the emulation reaches {r:.3g} of its bound"
    # the fixed-point sums of the bit-for-bit device check are the same integers
    R, X = pc.fixed_point_ingredients(case.csr[0], case.csr[2], case.x)
    assert np.array_equal(sums["fixed point"], pc.fixed_point_sums(*case.csr, case.x, R))


# ---------------------------------------------------------------- seeded faults
ROW_FAULTS = ["the last entry of a row dropped", "an entry added twice", "an entry gathered from column + 1",
              "an entry gathered from the next window (column +- 1024)", "an entry added to the neighbouring row"]
SUM_FAULTS = ["lane group - 1 of a full row left out of the tree", "an accumulator starts from the previous unit's row sum",
              "a stray add into an empty row"]
EPILOGUE_FAULTS = ["the shift term taken from row i + 1", "the shift's sign flipped", "a_self applied to the row sum"]


def _rebuild(csr, changed):
    """The arrays with the rows of ``changed`` ({row: (col, val)}) replaced."""
    rowptr, col, val = csr
    n = len(rowptr) - 1
    cs = [changed[i][0] if i in changed else col[rowptr[i]:rowptr[i + 1]] for i in range(n)]
    vs = [changed[i][1] if i in changed else val[rowptr[i]:rowptr[i + 1]] for i in range(n)]
    rp = np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
    return rp, np.concatenate(cs).astype(np.int32), np.concatenate(vs).astype(np.float64)


def _faulty_rows(case, fault, rng, group=None):
    """The arrays with ``fault`` in up to eight seeded rows (an entry of the row picked at random); None if the operator
    has no row the fault applies to."""
    rowptr, col, val = case.csr
    n, L = case.nrows, case.lens
    ok = L >= 1
    if fault == "an entry added to the neighbouring row":
        ok[-1] = False
    if fault == "an entry gathered from the next window (column +- 1024)" and case.ncols <= 2048:
        return None
    if group is not None:
        ok = (L >= group) & (L <= pc.STREAM_NNZ_PER_BLOCK)
    cand = np.flatnonzero(ok)
    if len(cand) == 0:
        return None
    rows = np.sort(rng.choice(cand, min(8, len(cand)), replace=False))
    if fault == "an entry added to the neighbouring row":
        rows = rows[np.concatenate([[True], np.diff(rows) > 1])]          # no picked row takes its neighbour's entry
    changed = {}
    for r in rows:
        c, v = col[rowptr[r]:rowptr[r + 1]].copy(), val[rowptr[r]:rowptr[r + 1]].copy()
        k = int(rng.integers(len(c)))
        if group is not None:
            keep = np.arange(len(c)) % group != group - 1
            c, v = c[keep], v[keep]
        elif fault == "the last entry of a row dropped":
            c, v = c[:-1], v[:-1]
        elif fault == "an entry added twice":
            c, v = np.append(c, c[k]), np.append(v, v[k])
        elif fault == "an entry gathered from column + 1":
            c[k] = c[k] + 1 if c[k] + 1 < case.ncols else c[k] - 1
        elif fault == "an entry gathered from the next window (column +- 1024)":
            c[k] = c[k] + 1024 if c[k] + 1024 < case.ncols else c[k] - 1024
        elif fault == "an entry added to the neighbouring row":
            c2, v2 = col[rowptr[r + 1]:rowptr[r + 2]], val[rowptr[r + 1]:rowptr[r + 2]]
            changed[r + 1] = (np.append(c2, c[k]), np.append(v2, v[k]))
            c, v = np.delete(c, k), np.delete(v, k)
        changed[r] = (c, v)
    return _rebuild(case.csr, changed), rows


def _assert_caught(case, kind, fault, sums, products=PRODUCTS, epilogue=pc.axpy_epilogue):
    lowest = float("inf")
    for sigma, sign in products:
        r = _ratio(case, kind, sigma, sign, epilogue(sigma, sign, case.xl, sums))
        assert r > 1.0, f"{case.name}, {kind}: '{fault}' passes at sigma={sigma} sign={sign:+.0f}: {r:.3g} of the bound"
        lowest = min(lowest, r)
    return lowest


@pytest.mark.parametrize("fault", ROW_FAULTS + SUM_FAULTS)
def test_faults_in_the_row_sum_exceed_every_bound(fault):
    """Every product - plain, and each shift with both signs - sees a fault of the row sum."""
    lowest = float("inf")
    for build in FAULT_CASES:
        case = build()
        clean = _clean(case)
        rng = np.random.default_rng(6)
        for kind in KINDS:
            if fault in ROW_FAULTS:
                bad = _faulty_rows(case, fault, rng)
                if bad is None:
                    continue
                sums = _emulate(kind, case, bad[0], rng)
            elif fault.startswith("lane group - 1"):
                if kind in ("layout 1", "layout 2"):
                    rows = np.flatnonzero((case.lens >= case.lanes) & (case.lens <= pc.STREAM_NNZ_PER_BLOCK))
                    sums = _emulate(kind, case, case.csr, rng, drop_lane_rows=rng.choice(rows, min(8, len(rows)), replace=False))
                else:                                                    # no lanes: the entries that lane would have taken
                    sums = _emulate(kind, case, _faulty_rows(case, fault, rng, group=case.lanes)[0], rng)
            elif fault.startswith("an accumulator starts"):
                if kind == "random order":
                    init = np.concatenate([np.zeros(RW), clean[kind][:-RW]])
                    sums = _emulate(kind, case, case.csr, rng, init=init)
                elif kind == "fixed point":
                    ints = _fixed_ints(case.csr, case.x, _scale(case))
                    sums = _emulate(kind, case, case.csr, rng, init=np.concatenate([np.zeros(RW, np.int64), ints[:-RW]]))
                else:
                    continue                                             # no accumulator that outlives a unit
            else:
                if not case.empty.any():
                    continue
                rows = np.flatnonzero(case.empty)
                k = rng.integers(len(case.csr[1]), size=len(rows))       # an entry of some other row lands in every empty row
                sums = clean[kind].copy()
                sums[rows] += case.csr[2][k] * case.x[case.csr[1][k]]
            lowest = min(lowest, _assert_caught(case, kind, fault, sums))
    assert np.isfinite(lowest)
    print(f"\n{fault}: lowest max error / bound over operators, layouts and products {lowest:.3g}")


def _epilogue_with(fault):
    def epi(sigma, sign, xl, s):
        a_self = sign * sigma
        if fault == "the shift term taken from row i + 1":
            return a_self * np.roll(xl, -1) + (-sign) * s
        if fault == "the shift's sign flipped":
            return (-a_self) * xl + (-sign) * s
        return a_self * s + (-sign) * s
    return epi


@pytest.mark.parametrize("fault", EPILOGUE_FAULTS)
def test_faults_in_the_epilogue_exceed_every_bound(fault):
    """The shifted products with sigma != 0 see a fault of the shift term (the plain product and sigma = 0 have none)."""
    products = [(s, g) for s, g in PRODUCTS if g != 0 and s != 0.0]
    assert len(products) == 8
    lowest = float("inf")
    for build in FAULT_CASES:
        case = build()
        for kind, sums in _clean(case).items():
            lowest = min(lowest, _assert_caught(case, kind, fault, sums, products, _epilogue_with(fault)))
    print(f"\n{fault}: lowest max error / bound over operators, layouts and products {lowest:.3g}")


@pytest.mark.parametrize("wbits,rw", [(22, 1024), (21, 2048)])
def test_the_entry_that_packs_to_the_padding_mark(wbits, rw):
    """The slab of the device test: the marked entry is the last of the last row, of order 1 on an operand element of
    order 1; the emulations stay within their bounds with it, and dropping it exceeds both bounds in every product."""
    case = pc.padding_mark_slab(wbits, rw)
    rowptr, col, val = case.csr
    assert case.nrows == rw and case.ncols == 1 << 22 and case.row_offset == 0
    assert (((rw - 1) << wbits) | int(col[-1] & ((1 << wbits) - 1))) == 0xFFFFFFFF and col[-1] >> wbits == 0
    assert val[-1] == 1.5 and case.x[col[-1]] == -0.75
    rng = np.random.default_rng(7)
    dropped = (np.concatenate([rowptr[:-1], [rowptr[-1] - 1]]), col[:-1], val[:-1])
    for kind in ("random order", "fixed point"):
        sums = _emulate(kind, case, case.csr, rng)
        for sigma, sign in PRODUCTS:
            assert _ratio(case, kind, sigma, sign, pc.axpy_epilogue(sigma, sign, case.xl, sums)) <= 1.0
        low = _assert_caught(case, kind, "the entry that packs to the padding mark dropped", _emulate(kind, case, dropped, rng))
        print(f"\n{case.name}, {kind}: the dropped entry is {low:.3g} of the bound at the least")
