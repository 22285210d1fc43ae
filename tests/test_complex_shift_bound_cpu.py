"""Reference and row bound of the complex-shift products (tests/_product_cases.py), checked on the host.

The reference against exact rational arithmetic; then a float64 emulation of the three forms the device runs - the fused
pair sweep, the block epilogues, the two real sweeps with their two ``axpby`` - with every row's terms added in a random
order.  The emulation must stay at or below the bound on every row (the bound is a worst case, so 1.0 is the mark, not a
fraction of it), and each seeded fault - injected here, in the emulation only - must exceed it on at least one row, for
every shift at which the fault changes the result.  fma(a, b, c) is emulated through the extended format where there is
one (as in test_hiprec_cpu.py), else as a * b + c.
"""
from fractions import Fraction

import numpy as np
import pytest

import _hiprec as hp
import _product_cases as pc

N = 3001
SIGNS = (1.0, -1.0)
P = 3                                                # operands the emulation runs on (of the GPU test's eleven)


def _fma(a, b, c):
    if not hp.EXTENDED:
        return a * b + c
    return (np.asarray(a, hp.LD) * np.asarray(b, hp.LD) + np.asarray(c, hp.LD)).astype(np.float64)


def _frac(v):
    return Fraction(*np.longdouble(v).as_integer_ratio())


# ---------------------------------------------------------------- the reference against fractions
def test_reference_against_fractions():
    """n = 12 with an empty row, a duplicate column and unsorted columns; one complex shift, both signs and the plain
    product; a slab of the same rows applied to the full-length operand."""
    rng = np.random.default_rng(12)
    n = 12
    lens = rng.integers(1, 6, n)
    lens[4], lens[7] = 0, 4
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([rng.choice(n, L, replace=False) for L in lens]).astype(np.int32)
    col[rowptr[7] + 1] = col[rowptr[7]]                                  # row 7 stores a column twice
    assert lens[7] >= 2 and any(np.any(np.diff(col[rowptr[i]:rowptr[i + 1]]) < 0) for i in range(n))
    val = rng.standard_normal(rowptr[-1]) * np.exp(rng.uniform(-3, 3, rowptr[-1]))
    xr, xi = pc.complex_operands(n, 1)[0]
    z = 0.37 - 1.9j
    F = lambda v: Fraction(float(v))

    def exact(i, sign):
        ks = range(rowptr[i], rowptr[i + 1])
        sr = sum((F(val[k]) * F(xr[col[k]]) for k in ks), Fraction(0))
        si = sum((F(val[k]) * F(xi[col[k]]) for k in ks), Fraction(0))
        mag = sum((abs(F(val[k])) * (abs(F(xr[col[k]])) + abs(F(xi[col[k]]))) for k in ks), Fraction(0))
        if sign == 0:
            return sr, si, mag
        vr, vi = F(xr[i]), F(xi[i])
        s = Fraction(int(sign))
        mag += (abs(F(z.real)) + abs(F(z.imag))) * (abs(vr) + abs(vi))
        return s * (F(z.real) * vr - F(z.imag) * vi - sr), s * (F(z.real) * vi + F(z.imag) * vr - si), mag

    for sign in (1.0, -1.0, 0.0):
        yr, yi = pc.shift_pair_reference(rowptr, col, val, xr, xi, z, sign)
        for i in range(n):
            er, ei, mag = exact(i, sign)
            assert abs(_frac(yr[i]) - er) <= 2.0 ** -60 * mag and abs(_frac(yi[i]) - ei) <= 2.0 ** -60 * mag, (sign, i)
    # rows 3..9 as a slab: the shift term comes from rows 3.. of the full-length operand
    rp = rowptr[3:10] - rowptr[3]
    c, v = col[rowptr[3]:rowptr[9]], val[rowptr[3]:rowptr[9]]
    yr, yi = pc.shift_pair_reference(rp, c, v, xr, xi, z, -1.0, row_offset=3)
    br, bi = pc.shift_pair_bound(rp, c, v, xr, xi, z, -1.0, row_offset=3)
    assert len(yr) == len(br) == 6
    for i in range(6):
        er, ei, mag = exact(i + 3, -1.0)
        assert abs(_frac(yr[i]) - er) <= 2.0 ** -60 * mag and abs(_frac(yi[i]) - ei) <= 2.0 ** -60 * mag


def test_bound_terms():
    """The formula itself on a three-row operator, and that an empty row's bound holds the shift terms only."""
    rowptr, col, val = np.array([0, 2, 2, 3]), np.array([2, 0, 1]), np.array([2.0, -3.0, 0.5])
    xr, xi = np.array([1.0, -2.0, 4.0]), np.array([0.5, 8.0, -1.0])
    z = -3.0 + 0.25j
    br, bi = pc.shift_pair_bound(rowptr, col, val, xr, xi, z, 1.0)
    u = 2.0 ** -53
    assert br[0] == pytest.approx(1.01 * u * (5 * (2 * 4 + 3 * 1) + 3 * 3 * 1 + 2 * 0.25 * 0.5), rel=1e-15)
    assert bi[0] == pytest.approx(1.01 * u * (5 * (2 * 1 + 3 * 0.5) + 3 * 3 * 0.5 + 2 * 0.25 * 1), rel=1e-15)
    assert br[1] == pytest.approx(1.01 * u * (3 * 3 * 2 + 2 * 0.25 * 8), rel=1e-15)          # empty row
    assert bi[2] == pytest.approx(1.01 * u * (4 * 0.5 * 8 + 3 * 3 * 1 + 2 * 0.25 * 4), rel=1e-15)
    p0r, p0i = pc.shift_pair_bound(rowptr, col, val, xr, xi, z, 0.0)
    assert p0r[1] == 1e-300 and p0i[1] == 1e-300 and p0r[0] == pytest.approx(1.01 * u * 5 * 11, rel=1e-15)
    assert pc.error_ratio(np.array([1.0, np.nan]), np.zeros(2, hp.LD), np.ones(2)) == float("inf")


def test_ragged_operator_options():
    """Without duplicates: the operator of the real-shift block tests, bit for bit; with them, every 5th row of two or
    more entries stores its first column twice and nothing else changes."""
    rp, c, v = pc.ragged_csr(N, 11)
    rp2, c2, v2 = pc.ragged_csr(N, 11, duplicates=True)
    L = np.diff(rp)
    assert N % 2 == 1 and np.sum(L == 0) >= N // 10 and np.sum(L == 300) == 7
    assert all(len(set(c[rp[i]:rp[i + 1]])) == L[i] for i in range(0, N, 97))
    assert np.array_equal(rp, rp2) and np.array_equal(v, v2)
    changed = np.flatnonzero(c != c2)
    rows = np.searchsorted(rp, changed, side="right") - 1
    assert len(changed) > 400 and np.all(rows % 5 == 0) and np.all(changed == rp[rows] + 1)
    assert np.array_equal(c2[changed], c2[changed - 1])
    assert np.any(L[rows] == 2) and np.any(L[rows] > 30)


# ---------------------------------------------------------------- float64 emulation of the three forms
def _row_sums(csr, x, rng, fault=None, fault_row=None):
    """A x in float64, the products of a row added one by one in a random order (the window-blocked kernels add with LDS
    atomics in any order; a fixed order is one of them)."""
    rowptr, col, val = csr
    out = np.zeros(len(rowptr) - 1)
    for i in range(len(out)):
        a, b = rowptr[i], rowptr[i + 1]
        if fault == "last entry of a long row dropped" and i == fault_row:
            b -= 1
        if a == b:
            continue
        t = (val[a:b] * x[col[a:b]])[rng.permutation(b - a)]
        if fault == "row sum in float32":
            out[i] = float(np.cumsum(t.astype(np.float32), dtype=np.float32)[-1])
        else:
            out[i] = np.cumsum(t)[-1]                                    # cumsum adds in sequence
    if fault == "row sum off by 64 ulp":
        out = out + 64.0 * np.spacing(out)
    return out


def _pair_epilogue(z, sign, vr, vi, sr, si):
    """PairEpilogue::row2 (spmv.hip)."""
    ar, ai, as_ = sign * z.real, sign * z.imag, (1.0 if sign == 0 else -sign)
    tr = ar * vr + as_ * sr                                              # add_rn(mul_rn, mul_rn): three roundings
    ti = ar * vi + as_ * si
    return _fma(-ai, vi, tr), _fma(ai, vr, ti)


def _block_epilogue(zs, sign, X, S, fault=None):
    """ShiftPairBlockEpilogue::elem / ShiftPairsZBlockEpilogue::elem (spmm.hip) on an interleaved block: columns
    (2p, 2p + 1) of X (operand rows) and S (row sums) are the halves of operand p, zs[p] its shift."""
    Y = np.empty_like(S)
    for j in range(S.shape[1]):
        p = j >> 1
        z = zs[(p + 1) % len(zs)] if fault == "operand p takes the shift of operand p + 1" else zs[p]
        ar, ai, as_ = sign * z.real, sign * z.imag, -sign
        vr, vi = X[:, j & ~1], X[:, (j & ~1) + 1]
        own = vi if j & 1 else vr
        t = ar * own + as_ * S[:, j]
        if j & 1:
            Y[:, j] = _fma(-ai if fault == "sign of the zi term flipped in the odd column" else ai, vr, t)
        else:
            Y[:, j] = _fma(-ai, vi, t)
    return Y


def _two_sweep(z, sign, vr, vi, sr, si):
    """launch_spmv_pair's second path: AxpyEpilogue::row per half, then axpby(-ai, xi, 1, yr) and axpby(ai, xr, 1, yi)
    with the product rounded on its own (the form with one more rounding; a contracted a * x + y is the fma above)."""
    ar, ai, as_ = sign * z.real, sign * z.imag, -sign

    def row(x, s):
        t = 0.0 if ar == 0.0 else ar * x
        return t + as_ * s

    yr, yi = row(vr, sr), row(vi, si)
    if ai != 0.0:
        yr = (-ai) * vi + 1.0 * yr
        yi = ai * vr + 1.0 * yi
    return yr, yi


@pytest.fixture(scope="module")
def case():
    csr = pc.ragged_csr(N, 11, duplicates=True)
    X = pc.complex_operands(N)[:P]
    prods = [pc.half_products(*csr, xr, xi) for xr, xi in X]
    rng = np.random.default_rng(5)
    sums = [(_row_sums(csr, xr, rng), _row_sums(csr, xi, rng)) for xr, xi in X]
    return csr, X, prods, sums


def _ratio(case, p, z, sign, yr, yi, rows=slice(None), row_offset=0):
    """max error / bound of an emulated result for operand p over ``rows`` of the operator (a slab: rows, and the operand
    rows the shift term reads start at row_offset)."""
    csr, X, prods, _ = case
    ref = pc.shift_pair_reference(*csr, *X[p], z, sign, products=prods[p])
    bnd = pc.shift_pair_bound(*csr, *X[p], z, sign, products=prods[p])
    return max(pc.error_ratio(yr, ref[0][rows], bnd[0][rows]), pc.error_ratio(yi, ref[1][rows], bnd[1][rows]))


def test_emulated_forms_stay_within_the_bound(case):
    csr, X, prods, sums = case
    worst = {"pair sweep": 0.0, "block": 0.0, "two sweeps": 0.0, "pair sweep, plain": 0.0}
    for k, z in enumerate(pc.SHIFTS):
        for sign in SIGNS:
            for p, ((xr, xi), (sr, si)) in enumerate(zip(X, sums)):
                worst["pair sweep"] = max(worst["pair sweep"], _ratio(case, p, z, sign, *_pair_epilogue(z, sign, xr, xi, sr, si)))
                worst["two sweeps"] = max(worst["two sweeps"], _ratio(case, p, z, sign, *_two_sweep(z, sign, xr, xi, sr, si)))
            zs = [pc.SHIFTS[(k + p) % len(pc.SHIFTS)] for p in range(P)]                # a shift per operand, cycled
            Y = _block_epilogue(zs, sign, np.column_stack([h for x in X for h in x]), np.column_stack([h for s in sums for h in s]))
            for p in range(P):
                worst["block"] = max(worst["block"], _ratio(case, p, zs[p], sign, Y[:, 2 * p], Y[:, 2 * p + 1]))
    for p, ((xr, xi), (sr, si)) in enumerate(zip(X, sums)):
        worst["pair sweep, plain"] = max(worst["pair sweep, plain"], _ratio(case, p, 0j, 0.0, *_pair_epilogue(0j, 0.0, xr, xi, sr, si)))
    print("float64 emulation, max error / bound:", {k: round(v, 3) for k, v in worst.items()})
    for form, r in worst.items():
        assert r <= 1.0, f"{form}: the float64 emulation reaches {r:.3g} of the bound"
    empty = np.diff(csr[0]) == 0                                         # empty rows: the shift term alone, nothing added
    yr, yi = _pair_epilogue(pc.SHIFTS[0], 1.0, *X[0], *sums[0])
    bad = yr.copy()
    bad[np.flatnonzero(empty)[3]] += 1e-12 * np.abs(X[0][0][np.flatnonzero(empty)[3]])
    assert _ratio(case, 0, pc.SHIFTS[0], 1.0, bad, yi) > 1.0


FAULTS = ["last entry of a long row dropped", "sign of the zi term flipped in the odd column",
          "operand p takes the shift of operand p + 1", "shift term read at row i - row_offset",
          "row sum in float32", "row sum off by 64 ulp"]


@pytest.mark.parametrize("fault", FAULTS)
def test_seeded_faults_exceed_the_bound(case, fault):
    csr, X, prods, sums = case
    nsh = len(pc.SHIFTS)
    lowest = float("inf")
    if fault in ("last entry of a long row dropped", "row sum in float32", "row sum off by 64 ulp"):
        long_row = int(np.flatnonzero(np.diff(csr[0]) == 300)[0])
        rng = np.random.default_rng(6)
        sr, si = (_row_sums(csr, h, rng, fault, long_row) for h in X[0])
        for z in pc.SHIFTS:
            for sign in SIGNS:
                for form in (_pair_epilogue, _two_sweep):
                    r = _ratio(case, 0, z, sign, *form(z, sign, *X[0], sr, si))
                    assert r > 1.0, f"{fault} passes at z={z} sign={sign} ({form.__name__}): {r:.3g}"
                    lowest = min(lowest, r)
    elif fault == "shift term read at row i - row_offset":
        off, end = 100, 2900
        rows = slice(off, end)
        for z in pc.SHIFTS:
            for sign in SIGNS:
                for p in range(P):
                    (xr, xi), (sr, si) = X[p], sums[p]
                    good = _pair_epilogue(z, sign, xr[rows], xi[rows], sr[rows], si[rows])
                    assert _ratio(case, p, z, sign, *good, rows=rows) <= 1.0
                    if z == 0:
                        continue                                          # no shift term: nothing to read wrongly
                    bad = _pair_epilogue(z, sign, xr[:end - off], xi[:end - off], sr[rows], si[rows])
                    r = _ratio(case, p, z, sign, *bad, rows=rows)
                    assert r > 1.0, f"{fault} passes at z={z} sign={sign} operand {p}: {r:.3g}"
                    lowest = min(lowest, r)
    else:
        Xb = np.column_stack([h for x in X for h in x])
        Sb = np.column_stack([h for s in sums for h in s])
        for k in range(nsh):
            zs = [pc.SHIFTS[(k + p) % nsh] for p in range(P)]
            for sign in SIGNS:
                Y = _block_epilogue(zs, sign, Xb, Sb, fault)
                for p in range(P):
                    if fault.startswith("sign of the zi term") and zs[p].imag == 0:
                        continue                                          # zi = 0: the flipped term is zero
                    assert zs[p] != zs[(p + 1) % P]
                    r = _ratio(case, p, zs[p], sign, Y[:, 2 * p], Y[:, 2 * p + 1])
                    assert r > 1.0, f"{fault} passes at z={zs[p]} sign={sign} operand {p}: {r:.3g}"
                    lowest = min(lowest, r)
    print(f"{fault}: lowest max error / bound over the shifts {lowest:.3g}")
