"""Operators, reference and row bound of the complex-shift products (a plain module: no fixtures, no tests).

The three entry points a FEAST contour solve takes its steps through - ``hipeig_spmv_shift_pair`` (fused pair sweep, or two
real sweeps and two ``axpby``), ``hipeig_spmm_shift_pairs`` and ``hipeig_spmm_shift_pairs_z`` (block epilogues of width 4, 8
and 16) - compute, for a complex operand x = xr + i xi, a complex shift z = zr + i zi and sign = +-1,

    yr = sign (zr xr - zi xi - A xr),      yi = sign (zr xi + zi xr - A xi)

and with sign = 0 the plain products (A xr, A xi).  ``shift_pair_reference`` evaluates that in ``np.longdouble`` and
``shift_pair_bound`` is the worst case of the float64 arithmetic the entry points perform, row by row.

The second half holds the same for the real single-vector products ``hipeig_spmv`` / ``hipeig_spmv_shift`` on the five
sweep layouts: ``shift_reference``, ``shift_bound`` (layouts 1 to 4), ``fixed_point_bound`` (layout 5), and the seeded
operators that put each sub-wave width, each row-block edge of the CSR-stream kernel and the tiny shapes of the blocked
layouts under them.
"""
import functools
import math

import numpy as np
import scipy.sparse as sp

import _hiprec as hp

U = 2.0 ** -53

# orders of magnitude apart from one entry to the next: an operand that takes its neighbour's shift is off by far more
# than a bound; zi = 0, zr = 0 and z = 0 each switch one term of the epilogue off; |z| >> |A| makes the operator sum the
# small part of the result
SHIFTS = (0.37 - 1.9j, 1e-3 + 1e2j, 25 + 0j, 0.3j, 0j, -0.07 + 0.19j)


def ragged_csr(n, seed, duplicates=False):
    """Odd n; empty rows, a few long rows (300 entries), the rest 0..40 entries; columns unsorted inside a row.
    ``duplicates``: every 5th row with at least two entries stores its first column twice (the second column index is
    overwritten with the first) - the arrays are meant to be kept as they are, without summing."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, n)
    lens[rng.choice(n, n // 10, replace=False)] = 0
    lens[rng.choice(n, 7, replace=False)] = 300
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([rng.choice(n, L, replace=False) for L in lens]).astype(np.int32)      # random order = unsorted
    val = rng.standard_normal(rowptr[-1]) * np.exp(rng.uniform(-3, 3, rowptr[-1]))
    if duplicates:
        rows = np.arange(0, n, 5)
        rows = rows[lens[rows] >= 2]
        col[rowptr[rows] + 1] = col[rowptr[rows]]
    return rowptr, col, val


def edge_matrix(N, seed):
    """Sparse rows of 0..40 non-zeros: row blocks of 64 rows give (block, window) tiles of a few to ~100 slots, i.e.
    shorter than 64 and than 256; rows 128..255 (two whole row blocks) and every 7th row are empty."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, N)
    lens[128:256] = 0
    lens[::7] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, N, int(rowptr[-1])).astype(np.int32)
    val = rng.standard_normal(int(rowptr[-1]))
    A = sp.csr_matrix((val, col, rowptr), shape=(N, N))
    A.sum_duplicates()
    A.sort_indices()
    return A


def complex_operands(n, count=11, seed=3):
    """``count`` complex operands of length n as (re, im) rows: standard_normal * exp(U(-2, 2)), element by element."""
    rng = np.random.default_rng([seed, n])
    X = rng.standard_normal((count, 2, n)) * np.exp(rng.uniform(-2, 2, (count, 2, n)))
    return [(np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1])) for x in X]


def half_products(rowptr, col, val, xr, xi):
    """What reference and bound need of the operator, taken once per operand (it does not depend on shift or sign):
    ``(A xr, (|A||xr|), A xi, (|A||xi|), L)`` in longdouble, L the stored entries per row."""
    ar, absr, L = hp.csr_matvec(rowptr, col, val, xr)
    ai, absi, _ = hp.csr_matvec(rowptr, col, val, xi)
    return ar, absr, ai, absi, L


def shift_pair_reference(rowptr, col, val, xr, xi, z, sign, row_offset=0, products=None):
    """``(yr, yi)`` in longdouble: sign (z x - A x) split into its halves, the plain products (A xr, A xi) for sign = 0.

    The CSR arrays hold the operator's rows; ``xr``, ``xi`` are full-length operands, of which the shift term takes rows
    ``row_offset ..`` (a row slab applied to a full-length operand).  ``products``: ``half_products`` of the same
    arguments, when the caller keeps them."""
    ar, _, ai, _, L = products if products is not None else half_products(rowptr, col, val, xr, xi)
    if sign == 0:
        return ar, ai
    n = len(L)
    z = complex(z)
    zr, zi, s = hp.LD(z.real), hp.LD(z.imag), hp.LD(sign)
    vr = np.asarray(xr, dtype=hp.LD)[row_offset:row_offset + n]
    vi = np.asarray(xi, dtype=hp.LD)[row_offset:row_offset + n]
    return s * (zr * vr - zi * vi - ar), s * (zr * vi + zi * vr - ai)


def shift_pair_bound(rowptr, col, val, xr, xi, z, sign, row_offset=0, products=None):
    """``(Br, Bi)``, float64: row bounds on ``|y - y*|`` for the real and the imaginary half.  With u = 2^-53, L_i the
    stored entries of row i and x' the other half of the operand, the real half's is

        B_i = 1.01 u [ (L_i + 3) (|A||xr|)_i + 3 |zr| |xr_i| + 2 |zi| |xi_i| ] + 1e-300

    and the imaginary half's the same with xr and xi exchanged; sign = 0 (plain product) has no shift terms.  It is the
    worst case of the arithmetic of ``PairEpilogue::row2``, ``ShiftPairBlockEpilogue::elem`` /
    ``ShiftPairsZBlockEpilogue::elem`` and of the two-sweep path (``AxpyEpilogue`` then ``axpby``), whatever the order
    of a row's adds:

    - every term of the row sum passes at most L_i roundings (its product, then at most L_i - 1 adds; L_i adds into an
      accumulator that starts at zero, the first of them exact): L_i u (|A||x|)_i;
    - t = rn(rn(ar x) + (-sign) s) adds u |zr x| for the product and u (|zr x| + (|A||x|)) for the sum;
    - the last step adds u (|zr x| + |zi x'| + (|A||x|)): one ``fma`` in the fused and the block forms; ``axpby`` in the
      two-sweep form, which may also round zi x' on its own - one more u |zi x'|;
    - the extra 1 in L_i + 3 and the factor 1.01 cover the second-order terms; 1e-300 keeps 0 <= 0 true where a ratio is
      formed.

    Proven, not fitted: no further safety factor belongs on it.  A row that stores nothing has no operator term, so a
    stray add into an empty row exceeds it."""
    _, absr, _, absi, L = products if products is not None else half_products(rowptr, col, val, xr, xi)
    n = len(L)
    Lf = L.astype(np.float64) + 3.0
    absr, absi = absr.astype(np.float64), absi.astype(np.float64)
    if sign == 0:
        return 1.01 * U * Lf * absr + 1e-300, 1.01 * U * Lf * absi + 1e-300
    z = complex(z)
    azr, azi = abs(z.real), abs(z.imag)
    vr = np.abs(np.asarray(xr, dtype=np.float64)[row_offset:row_offset + n])
    vi = np.abs(np.asarray(xi, dtype=np.float64)[row_offset:row_offset + n])
    return (1.01 * U * (Lf * absr + 3.0 * azr * vr + 2.0 * azi * vi) + 1e-300,
            1.01 * U * (Lf * absi + 3.0 * azr * vi + 2.0 * azi * vr) + 1e-300)


# ================================================================ the real products
# y = A x (``hipeig_spmv``) and y = sign (sigma x - A x) (``hipeig_spmv_shift``) on the five sweep layouts: 1 CSR-vector,
# 2 CSR-stream, 3 wave units, 4 workgroup units (fp64 LDS atomics), 5 workgroup units with fixed-point accumulators.
REAL_SHIFTS = (0.37, 1e3, 1e-3, 0.0, -25.0)          # orders of magnitude apart; 0.0 switches the shift term off

STREAM_NNZ_PER_BLOCK = 2048                          # SPMV_NNZ_PER_BLOCK: a longer row takes the whole-workgroup path


def lanes_per_row(rowptr):
    """The sub-wave width ``hipeig_csr_finalize`` picks from the mean row length."""
    n = len(rowptr) - 1
    mean = float(rowptr[-1]) / n if n else 0.0
    return 4 if mean < 6 else 8 if mean < 24 else 16 if mean < 96 else 32 if mean < 384 else 64


def shift_reference(rowptr, col, val, x, sigma, sign, row_offset=0, product=None):
    """``sign (sigma x[row_offset + i] - (A x)_i)`` in longdouble; the plain product ``A x`` for sign = 0.

    The CSR arrays hold the operator's rows (of a slab: rows ``row_offset ..`` of the square operator), ``x`` is the
    full-length operand.  ``product``: ``_hiprec.csr_matvec`` of the same arguments, when the caller keeps it."""
    ax, _, L = product if product is not None else hp.csr_matvec(rowptr, col, val, x)
    if sign == 0:
        return ax
    n = len(L)
    v = np.asarray(x, dtype=hp.LD)[row_offset:row_offset + n]
    return hp.LD(sign) * (hp.LD(sigma) * v - ax)


def shift_bound(rowptr, col, val, x, sigma, sign, row_offset=0, product=None):
    """Row bound, float64, on ``|y - y*|`` of the float64 sweeps (layouts 1 to 4).  With u = 2^-53 and L_i the stored
    entries of row i (a column stored twice counts twice),

        plain    B_i = 1.01 u (L_i + 1) (|A||x|)_i + 1e-300
        shifted  B_i = 1.01 u [ (L_i + 2) (|A||x|)_i + 2 |sigma| |x_i| ] + 1e-300

    whatever the order of a row's adds:

    - the row sum is a summation tree over the row's L_i products.  An add whose other operand is the 0.0 of an empty
      lane, an empty share or a fresh accumulator is exact, so the adds that round merge two non-empty sets of terms: at
      most L_i - 1 of them lie on a term's path, and with the rounding of its own product a term passes at most L_i
      roundings (fewer in the ``fma`` chains of layout 1 and of the whole-workgroup path of layout 2, where product and
      add round once).  The sum is off by at most gamma_L (|A||x|)_i, gamma_L = L u / (1 - L u);
    - that covers the lanes' chains with their ``__shfl_down`` tree, ``block_reduce_sum``, LDS atomics in any order, the
      shares of a column-split sweep added by ``tcoow_combine_sweep``, and accumulators handed on through ``yinit``: all
      of them are trees over the same terms;
    - plain product: ``AxpyEpilogue::row`` returns 0 + 1 * sum, both exact;
    - shifted: a_sum = -sign is exact; t = rn(a_self x_i) adds u |sigma x_i|, the final add u (|sigma x_i| + |sum|):
      2 u |sigma x_i| + u (|A||x|)_i;
    - the extra 1 in L_i + 1 / L_i + 2 and the factor 1.01 take the second-order terms (as in ``shift_pair_bound``);
      1e-300 keeps 0 <= 0 true where a ratio is formed and takes a product that underflows.

    Proven, not fitted: the mark is 1.0 and no safety factor belongs on top.  A row that stores nothing has the shift
    term alone, so a stray add into it exceeds the bound."""
    _, absx, L = product if product is not None else hp.csr_matvec(rowptr, col, val, x)
    Lf, absx = L.astype(np.float64), absx.astype(np.float64)
    if sign == 0:
        return 1.01 * U * (Lf + 1.0) * absx + 1e-300
    v = np.abs(np.asarray(x, dtype=np.float64)[row_offset:row_offset + len(L)])
    return 1.01 * U * ((Lf + 2.0) * absx + 2.0 * abs(float(sigma)) * v) + 1e-300


def fixed_point_ingredients(rowptr, val, x):
    """``(R, X)`` of the fixed-point sweep from the host arrays: R = max_i sum_j |a_ij| over the operator's rows (summed
    in longdouble), X = max |x| over the whole gathered operand."""
    rowptr = np.asarray(rowptr, np.int64)
    a = np.abs(np.asarray(val, dtype=hp.LD))
    full = np.diff(rowptr) > 0
    R = float(np.max(np.add.reduceat(a, rowptr[:-1][full]))) if full.any() else 0.0
    X = float(np.max(np.abs(x))) if len(x) else 0.0
    return R, X


def fixed_point_bound(rowptr, col, val, x, sigma, sign, row_offset=0, product=None, column_splits=1):
    """Row bound, float64, of layout 5 (``tcoo_wg_sweep<FIXED>``).  With q = 2^-60 R X (``fixed_point_ingredients``),
    u = 2^-53 and s_i = min(column_splits, L_i) the shares of row i that can hold an entry,

        plain    B_i = 1.01 [ (L_i / 2) q + (s_i + 1) u (|A||x|)_i ] + 1e-300
        shifted  B_i = 1.01 [ (L_i / 2) q + (s_i + 2) u (|A||x|)_i + 2 u |sigma| |x_i| ] + 1e-300

    - ``fixed_point_scale`` takes 2^e with v < 2^ex, e = 61 - ex, for v = rn(R' X), R' the device's row-sum maximum: one
      unit of the accumulators is 2^-e = 2^(ex - 61) <= 2 v 2^-61 = 2^-60 v, and v <= R X (1 + (L_max + 2) u), which the
      factor 1.01 takes;
    - a term is rn(a x) (u |a x|), scaled by a power of two (exact) and rounded to an integer by ``lds_add_i64_wg``:
      half a unit.  The integer adds are exact and cannot overflow (|sum| 2^e < 2^61 + L): (L_i / 2) 2^-e + u (|A||x|)_i;
    - int64 -> double rounds once, u |sum| <= u ((|A||x|)_i (1 + u) + (L_i / 2) 2^-e); the product with 2^-e is exact;
    - the epilogue is that of ``shift_bound``: nothing for the plain product, 2 u |sigma x_i| + u |sum| shifted;
    - column splits: every share is converted to double on its own - in total the same u (|A||x|)_i as the single
      conversion - and ``tcoow_combine_sweep`` adds the shares in double: the shares without an entry of the row are
      exact zeros, so at most s_i - 1 adds round, each by at most u (|A||x|)_i (1 + ...);
    - the header's (L_i / 2 + 1) 2^-60 R X is this bound's first term with the conversion counted as a whole unit; here
      the conversion is counted as what it is, u |sum|, so that a row without entries keeps the shift term alone.

    R and X come from the host arrays; that the device's own two numbers agree with them (X exactly, R to L_max u R) is
    checked where the device is."""
    _, absx, L = product if product is not None else hp.csr_matvec(rowptr, col, val, x)
    R, X = fixed_point_ingredients(rowptr, val, x)
    q = 2.0 ** -60 * R * X
    Lf, absx = L.astype(np.float64), absx.astype(np.float64)
    s = np.minimum(float(column_splits), Lf)
    if sign == 0:
        return 1.01 * (0.5 * Lf * q + (s + 1.0) * U * absx) + 1e-300
    v = np.abs(np.asarray(x, dtype=np.float64)[row_offset:row_offset + len(L)])
    return 1.01 * (0.5 * Lf * q + (s + 2.0) * U * absx + 2.0 * U * abs(float(sigma)) * v) + 1e-300


def fixed_point_scale(R, X):
    """2^e of ``fixed_point_scale`` (spmv_device.h) for finite R X > 0; 1.0 for R X = 0."""
    v = R * X
    return 2.0 ** (61 - math.frexp(v)[1]) if v > 0.0 else 1.0


def fixed_point_terms(col, val, x, S):
    """rint(rn(a x) S) per stored entry as int64: what ``lds_add_i64_wg`` adds (S a power of two, the product exact)."""
    x = np.asarray(x, np.float64)
    return np.rint(np.asarray(val, np.float64) * x[np.asarray(col, np.int64)] * S).astype(np.int64)


def fixed_point_sums(rowptr, col, val, x, R, X=None):
    """The row sums of layout 5 without column splits, bit for bit: the exact integer sum of rint(rn(a x) 2^e), converted
    to double once and scaled back.  ``R``: the row-sum maximum the scale is taken from (the device's, where its bits
    are to be met)."""
    rowptr = np.asarray(rowptr, np.int64)
    S = fixed_point_scale(R, (float(np.max(np.abs(x))) if len(x) else 0.0) if X is None else X)
    t = fixed_point_terms(col, val, x, S)
    out = np.zeros(len(rowptr) - 1, dtype=np.int64)
    full = np.diff(rowptr) > 0
    if full.any():
        out[full] = np.add.reduceat(t, rowptr[:-1][full])
    return out.astype(np.float64) * (1.0 / S)


def axpy_epilogue(sigma, sign, xl, s):
    """``AxpyEpilogue::row`` on whole arrays: rn(rn(a_self x_i) + a_sum s_i), a_self = sign sigma, a_sum = -sign (the
    plain product for sign = 0)."""
    if sign == 0:
        return 0.0 + 1.0 * s
    a_self = sign * sigma
    t = np.zeros_like(s) if a_self == 0.0 else a_self * xl
    return t + (-sign) * s


class RealCase:
    """An operator's rows as CSR arrays (of a slab: rows row_offset ..), its full-length operand, and the longdouble
    product of the two, taken once."""

    def __init__(self, name, csr, ncols, row_offset=0, x=None):
        self.name, self.ncols, self.row_offset = name, int(ncols), int(row_offset)
        self.csr = (np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int32), np.asarray(csr[2], np.float64))
        self.nrows = len(self.csr[0]) - 1
        self.lens = np.diff(self.csr[0])
        self.empty = self.lens == 0
        self.lanes = lanes_per_row(self.csr[0])
        self.x = real_operand(ncols, seed=self.nrows) if x is None else x
        self.xl = self.x[self.row_offset:self.row_offset + self.nrows]
        self._product = None

    @property
    def product(self):
        if self._product is None:
            self._product = hp.csr_matvec(*self.csr, self.x)
        return self._product

    def args(self, sigma, sign):
        return (*self.csr, self.x, sigma, sign, self.row_offset, self.product)

    def reference(self, sigma, sign):
        return shift_reference(*self.args(sigma, sign))

    def bound(self, sigma, sign, fixed=False, column_splits=1):
        if fixed:
            return fixed_point_bound(*self.args(sigma, sign), column_splits=column_splits)
        return shift_bound(*self.args(sigma, sign))


def real_operand(n, seed=3):
    """standard_normal * exp(U(-2, 2)), element by element."""
    rng = np.random.default_rng([seed, n, 17])
    return rng.standard_normal(n) * np.exp(rng.uniform(-2, 2, n))


def _random_rows(lens, ncols, rng):
    """Rows of the given lengths: columns integers(0, ncols) (unsorted, duplicates kept as stored), values
    standard_normal * exp(U(-3, 3))."""
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rowptr[-1])
    col = rng.integers(0, ncols, nnz).astype(np.int32)
    val = rng.standard_normal(nnz) * np.exp(rng.uniform(-3, 3, nnz))
    return rowptr, col, val


@functools.lru_cache(maxsize=None)
def lanes4():
    """1500 x 1500, rows of 0..4 entries: 4 lanes per row, 64 rows per workgroup pass."""
    rng = np.random.default_rng(404)
    c = RealCase("lanes4", _random_rows(rng.integers(0, 5, 1500), 1500, rng), 1500)
    assert c.lanes == 4 and c.empty.any() and np.any(c.lens == 4)
    return c


@functools.lru_cache(maxsize=None)
def lanes16():
    """1201 x 1201, rows of 30..90 entries, a tenth of the rows empty: 16 lanes."""
    rng = np.random.default_rng(1616)
    lens = rng.integers(30, 91, 1201)
    lens[rng.choice(1201, 120, replace=False)] = 0
    c = RealCase("lanes16", _random_rows(lens, 1201, rng), 1201)
    assert c.lanes == 16 and int(c.empty.sum()) == 120
    return c


@functools.lru_cache(maxsize=None)
def lanes32():
    """Rows 700..1299 of a 2000-column operator, 100..379 entries each: 32 lanes, a slab applied to the full operand."""
    rng = np.random.default_rng(3232)
    c = RealCase("lanes32", _random_rows(rng.integers(100, 380, 600), 2000, rng), 2000, 700)
    assert c.lanes == 32 and c.nrows == 600
    return c


@functools.lru_cache(maxsize=None)
def lanes64():
    """Rows 1000..1299 of a 3000-column operator, 384..900 entries each: 64 lanes, a slab."""
    rng = np.random.default_rng(6464)
    c = RealCase("lanes64", _random_rows(rng.integers(384, 901, 300), 3000, rng), 3000, 1000)
    assert c.lanes == 64 and c.nrows == 300
    return c


@functools.lru_cache(maxsize=None)
def stream_edges():
    """4000 x 4000, rows of 0..40 entries (8 lanes), and the row blocks of the CSR-stream kernel at their edges: row 0
    empty; rows 100 / 101 / 102 with 2048 / 2049 / 2047 entries (the largest row of the LDS path, the smallest of the
    whole-workgroup path, one below); row 3000 with 4097; rows 1500..2699 empty (the 1024-row cap closes a block, not the
    entry count); the last row with 2049."""
    rng = np.random.default_rng(2048)
    lens = rng.integers(0, 41, 4000)
    lens[0] = 0
    lens[100], lens[101], lens[102] = STREAM_NNZ_PER_BLOCK, STREAM_NNZ_PER_BLOCK + 1, STREAM_NNZ_PER_BLOCK - 1
    lens[3000] = 2 * STREAM_NNZ_PER_BLOCK + 1
    lens[1500:2700] = 0
    lens[3999] = STREAM_NNZ_PER_BLOCK + 1
    c = RealCase("stream_edges", _random_rows(lens, 4000, rng), 4000)
    assert c.lanes == 8 and np.all(c.empty[1500:2700]) and c.lens[-1] == 2049
    return c


@functools.lru_cache(maxsize=None)
def tiny(n, stored=True):
    """n = 1 (one entry, or nothing stored), 63, 64, 65 with rows of 0..5 entries: one unit of the blocked layouts partly
    or wholly beyond nrows, one window shorter than its nominal width."""
    rng = np.random.default_rng([n, 7])
    lens = np.array([1 if stored else 0]) if n == 1 else rng.integers(0, 6, n)
    c = RealCase(f"tiny n={n}" + ("" if stored else " (nothing stored)"), _random_rows(lens, n, rng), n)
    assert c.lanes == 4 and (n == 1 or (c.empty.any() and np.any(c.lens >= 4)))
    return c


@functools.lru_cache(maxsize=None)
def edge3001():
    """``edge_matrix(3001)`` as the stream-layout test builds it (8 lanes)."""
    A = edge_matrix(3001, seed=3001)
    c = RealCase("edge_matrix(3001)", (A.indptr, A.indices, A.data), 3001)
    assert c.lanes == 8
    return c


@functools.lru_cache(maxsize=None)
def ragged3001():
    """``ragged_csr(3001, 11, duplicates=True)``, the arrays as they are (8 lanes)."""
    c = RealCase("ragged_csr(3001)", ragged_csr(3001, 11, duplicates=True), 3001)
    assert c.lanes == 8
    return c


REAL_OPERATORS = (lanes4, lanes16, lanes32, lanes64, stream_edges, edge3001, ragged3001)
TINY = ((1, True), (1, False), (63, True), (64, True), (65, True))


@functools.lru_cache(maxsize=None)
def padding_mark_slab(wbits, rw):
    """``rw`` rows x 2^22 columns (row_offset 0), rows of 0..6 entries at random columns, and in local row rw - 1 one more
    entry at column 2^wbits - 1: with ``wbits`` window bits and ``rw`` rows per unit the wave-unit layout would pack it
    as (rw - 1) << wbits | 2^wbits - 1 = 0xFFFFFFFF, its sweep's mark for "no entry".  The entry and the operand element
    it meets are of order 1."""
    assert rw << wbits == 1 << 32
    ncols = 1 << 22
    rng = np.random.default_rng([wbits, rw])
    rowptr, col, val = _random_rows(rng.integers(0, 7, rw), ncols, rng)
    col = np.concatenate([col, [(1 << wbits) - 1]]).astype(np.int32)
    val = np.concatenate([val, [1.5]])
    rowptr = rowptr.copy()
    rowptr[-1] += 1
    x = real_operand(ncols, seed=wbits)
    x[(1 << wbits) - 1] = -0.75
    return RealCase(f"padding mark wbits={wbits} rw={rw}", (rowptr, col, val), ncols, 0, x)


def error_ratio(got, ref, bound):
    """max_i |got_i - ref_i| / bound_i, the difference taken in longdouble (NaN or inf in ``got`` gives inf)."""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got.astype(hp.LD) - ref).astype(np.float64)
    return float(np.max(err / bound)) if err.size else 0.0
