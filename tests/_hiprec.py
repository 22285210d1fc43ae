"""High-precision references for the kernel tests (a plain module, imported by the tests that need it).

Everything here is evaluated in ``np.longdouble`` / ``np.clongdouble``.  On x86-64 that is the 80-bit format with a
64-bit mantissa; NumPy's pairwise summation keeps the error of a sum of n terms near ``log2(n) * 2^-64`` relative to the
sum of their magnitudes, some 2000 times below the double rounding unit the kernels are held to.  Where ``longdouble``
is no wider than ``double`` (``np.finfo(np.longdouble).nmant < 63``), ``dot`` and ``nrm2`` take an exact form instead:
every product split into two doubles without error (Veltkamp / Dekker TwoProduct) and the terms added by ``math.fsum``.

``mgs`` is the sequential modified Gram-Schmidt sweep of SciPy's ``_fgmres`` as ``eigensolvers_amd.gcrotmk`` drives it
(``_Ops.arnoldi_step`` / ``_PairOps.arnoldi_step``): ``||w||``, then for each column ``h = <v, w>; w -= h v``, then
``||w||`` and ``w / ||w||`` - with the conjugated products of BLAS ``zdotc`` for complex columns.
"""
import math

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EXTENDED = np.finfo(np.longdouble).nmant >= 63      # x86-64: 63 stored fraction bits, a 64-bit mantissa

_SPLIT = float(2 ** 27 + 1)                          # Veltkamp's constant for binary64


def _two_product(a, b):
    """p, e with p + e == a * b exactly (a, b float64 arrays; Dekker's TwoProduct through Veltkamp splitting, no FMA)."""
    def split(x):
        t = _SPLIT * x
        hi = t - (t - x)
        return hi, x - hi
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _dot_exact(x, y):
    """sum(x * y) for float64 arrays, correctly rounded to float64 (every product exact as p + e, then math.fsum)."""
    p, e = _two_product(np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel())
    return math.fsum(np.concatenate([p, e]).tolist())


def _wide(x):
    x = np.asarray(x)
    return x.astype(CLD if np.iscomplexobj(x) else LD)


def dot(x, y):
    """conj(x) . y (zdotc for complex input) in extended precision; returns longdouble / clongdouble."""
    x, y = np.asarray(x), np.asarray(y)
    if not EXTENDED and x.dtype.itemsize <= 16 and y.dtype.itemsize <= 16:
        xr, xi = np.real(x).astype(np.float64), np.imag(x).astype(np.float64)
        yr, yi = np.real(y).astype(np.float64), np.imag(y).astype(np.float64)
        re = math.fsum([_dot_exact(xr, yr), _dot_exact(xi, yi)])
        if not (np.iscomplexobj(x) or np.iscomplexobj(y)):
            return LD(re)
        return CLD(complex(re, math.fsum([_dot_exact(xr, yi), -_dot_exact(xi, yr)])))
    xw, yw = _wide(x), _wide(y)
    return np.sum(np.conj(xw) * yw) if np.iscomplexobj(xw) else np.sum(xw * yw)


def nrm2(x):
    """||x||_2 in extended precision (longdouble)."""
    x = np.asarray(x)
    if not EXTENDED and x.dtype.itemsize <= 16:
        parts = [np.real(x).astype(np.float64), np.imag(x).astype(np.float64)]
        return LD(math.sqrt(math.fsum([_dot_exact(p, p) for p in parts])))
    xw = _wide(x)
    return np.sqrt(np.sum(xw.real * xw.real + xw.imag * xw.imag)) if np.iscomplexobj(xw) else np.sqrt(np.sum(xw * xw))


def mgs(V, w, normalise=True, checkpoints=None):
    """Sequential MGS of w against the rows of V (shape (m, n)), the whole sweep in extended precision.

    Returns ``(nb, h, na, w_out)``: ``||w||`` before, the m coefficients, ``||w||`` after and ``w / ||w||`` after (the
    projected ``w`` itself with ``normalise=False``, as ``hipeig_mgs_project`` leaves it).  With ``checkpoints`` (a set of
    column counts), returns ``{k: (nb, h[:k], na_k, w_out_k)}`` instead: the first k columns of a sweep ARE the sweep over
    k columns, so one pass serves every prefix."""
    V = np.asarray(V)
    m = V.shape[0]
    w = _wide(w)
    if np.iscomplexobj(V) and not np.iscomplexobj(w):
        w = w.astype(CLD)
    nb = nrm2(w)
    h = np.zeros(m, dtype=w.dtype)
    out = {}

    def record(k):
        na = nrm2(w)
        return nb, h[:k].copy(), na, (w / na if normalise else w.copy())

    want = set(checkpoints) if checkpoints is not None else {m}
    if 0 in want:
        out[0] = record(0)
    for j in range(m):
        v = _wide(V[j])
        c = dot(v, w)
        h[j] = c
        w -= c * v
        if j + 1 in want:
            out[j + 1] = record(j + 1)
    return out if checkpoints is not None else out[m]


def csr_matvec(rowptr, col, val, x):
    """y = A x for a CSR matrix (any row order of the columns, duplicates summed) in extended precision.

    Returns ``(y, absax, rowlen)``: the product, ``(|A| |x|)`` per row and the stored entries per row - what a row-wise
    forward-error bound of a float64 product needs."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    n = len(rowptr) - 1
    rowlen = np.diff(rowptr)
    xw = _wide(x)[col]
    vw = _wide(val)
    terms = vw * xw
    y = np.zeros(n, dtype=terms.dtype)
    absax = np.zeros(n, dtype=LD)
    full = rowlen > 0
    if full.any():                                   # row segments of the entry stream, each summed in order
        start = rowptr[:-1][full]
        y[full] = np.add.reduceat(terms, start)
        absax[full] = np.add.reduceat(np.abs(vw) * np.abs(xw), start)
    return y, absax, rowlen
