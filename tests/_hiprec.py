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


def _dots(Bw, aw):
    """[dot(b, a) for the rows b of Bw] as a longdouble array (real, already widened operands).  The sum runs along the
    contiguous axis, so NumPy adds pairwise (a longdouble matrix product would add in sequence)."""
    if not EXTENDED:
        return np.array([dot(b, aw) for b in Bw], dtype=LD).reshape(len(Bw))
    return np.sum(Bw * aw, axis=1) if len(Bw) else np.zeros(0, dtype=LD)


def orthonormalize_mgs(Q, x):
    """The reference's orthogonalize_against_set up to its lindep test (numpyVector.py:132-140) in extended precision: for
    each row q of Q (shape (m, n), in order)  t1 = x.q, t2 = q.q, x -= q (t1 / t2);  then ip = x.x.

    Returns ``(ip, x_projected, S)`` with the error scale S = ||x_0|| + sum_j |t1_j / t2_j| ||q_j||."""
    Q = np.asarray(Q, dtype=np.float64)
    xw = _wide(x).copy()
    S = nrm2(xw)
    for q in Q:
        qw = _wide(q)
        t1, t2 = dot(xw, qw), dot(qw, qw)
        coef = t1 / t2
        xw -= qw * coef
        S = S + abs(coef) * np.sqrt(t2)
    return dot(xw, xw), xw, S


def orthonormalize_cgs2(Q, x):
    """Two classical passes  c = Q x; x -= c^T Q  (all coefficients of a pass from the same x, no division by q.q) in
    extended precision, then ip = x.x.

    Returns ``(ip, x_projected, scales)``; ``scales[p]`` = (||x_p||, sum_j |c_j| ||q_j||, sum_j ||q_j||^2) for pass p, x_p
    being the vector the pass starts from."""
    Q = np.asarray(Q, dtype=np.float64)
    Qw = _wide(Q)
    xw = _wide(x).copy()
    qn2 = np.array([dot(q, q) for q in Qw], dtype=LD).reshape(len(Qw))
    qn = np.sqrt(qn2)
    scales = []
    for _ in range(2):
        c = _dots(Qw, xw)
        scales.append((nrm2(xw), np.sum(np.abs(c) * qn), np.sum(qn2)))
        for cj, qw in zip(c, Qw):
            xw -= cj * qw
    return dot(xw, xw), xw, scales


def gram(A, B):
    """A B^T and |A| |B|^T for row sets A (ma, n) and B (mb, n) in extended precision: ``(G, Gabs)``."""
    Aw, Bw = _wide(np.asarray(A, dtype=np.float64)), _wide(np.asarray(B, dtype=np.float64))
    aA, aB = np.abs(Aw), np.abs(Bw)
    G = np.empty((len(Aw), len(Bw)), dtype=LD)
    Gabs = np.empty_like(G)
    for i in range(len(Aw)):
        G[i] = _dots(Bw, Aw[i])
        Gabs[i] = _dots(aB, aA[i])
    return G, Gabs


def combine(V, C):
    """V^T C and |V|^T |C| for rows V (m, n) and coefficients C (m, k) in extended precision: ``(Y, Yabs)``, shape (n, k) -
    column c is sum_j C[j, c] V_j."""
    VT = np.ascontiguousarray(_wide(np.asarray(V, dtype=np.float64)).T)          # (n, m): the sum runs along a row
    Cw = _wide(np.asarray(C, dtype=np.float64))
    aVT, aC = np.abs(VT), np.abs(Cw)
    Y = np.empty((VT.shape[0], Cw.shape[1]), dtype=LD)
    Yabs = np.empty_like(Y)
    for c in range(Cw.shape[1]):
        Y[:, c] = _dots(VT, Cw[:, c])
        Yabs[:, c] = _dots(aVT, aC[:, c])
    return Y, Yabs


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
