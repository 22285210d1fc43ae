"""Operators, reference and row bound of the complex-shift products (a plain module: no fixtures, no tests).

The three entry points a FEAST contour solve takes its steps through - ``hipeig_spmv_shift_pair`` (fused pair sweep, or two
real sweeps and two ``axpby``), ``hipeig_spmm_shift_pairs`` and ``hipeig_spmm_shift_pairs_z`` (block epilogues of width 4, 8
and 16) - compute, for a complex operand x = xr + i xi, a complex shift z = zr + i zi and sign = +-1,

    yr = sign (zr xr - zi xi - A xr),      yi = sign (zr xi + zi xr - A xi)

and with sign = 0 the plain products (A xr, A xi).  ``shift_pair_reference`` evaluates that in ``np.longdouble`` and
``shift_pair_bound`` is the worst case of the float64 arithmetic the entry points perform, row by row.
"""
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


def error_ratio(got, ref, bound):
    """max_i |got_i - ref_i| / bound_i, the difference taken in longdouble (NaN or inf in ``got`` gives inf)."""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got.astype(hp.LD) - ref).astype(np.float64)
    return float(np.max(err / bound)) if err.size else 0.0
