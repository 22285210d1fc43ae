"""FEAST's filtered vector from two Lanczos passes, without any per-shift vector.  DESIGN.md section 3.6.

FEAST never looks at the solutions of its contour solves: it forms ``q = sum_k Re(c_k x_k)`` (feast.py:189-200) with
``sign*(z_k I - H) x_k = b``.  Every MINRES iterate ``x_k`` lies in the Krylov space of the same real Lanczos basis
``v_0, v_1, ...`` of ``(H, b)``, so ``q = sum_i g_i v_i`` with real ``g_i = Re(sum_k c_k y_{k,i})``, where ``y_k`` holds
the coefficients of shift k's iterate in that basis - numbers that follow from the Lanczos tridiagonal alone:

* pass 1 (``lanczos_scalars_host`` / ``hipeig_lanczos_block_scalars``) runs the Lanczos recurrence and the per-shift
  rotation recurrences of ``shifted_minres_host`` and keeps scalars only: ``alpha_i``, ``beta_i`` and the stop steps;
* the host turns them into ``g`` (``minres_coefficients``: the QR factors of the shifted tridiagonal, back substitution);
* pass 2 (``lanczos_combine_host`` / ``hipeig_lanczos_combine``) repeats the recurrence from the stored scalars -
  no dot products - and accumulates ``q += g_i v_i``.

With ``keepBasis`` / ``basis="keep"`` pass 1 keeps its vectors in device memory (``basis_mode`` 1) and pass 2, handed that
basis, is one stream over them: no second set of products, any number of combinations.  With ``keepPrefix`` /
``prefix=True`` on top (``basis_mode`` 2), a basis that outgrows its byte budget keeps its first ``p`` vectors: the stream
serves the terms ``i < p - 1`` and the recurrence restarts from the two last kept vectors, ``m - p`` products instead of
``m - 1``.  ``prefix_split`` is the plan of all three.  ``basisPrecision`` / ``precision="fp32"`` (``basis_mode`` 3 / 4)
stores that basis in fp32, twice the vectors per byte: pass 1, its scalars and the coefficients stay fp64 bit for bit, only
the copy pass 2 streams over is rounded (``lanczos_combine_stored_host`` states it and its error bound).

Both passes are an operator product plus a row epilogue, so up to 8 right-hand sides advance in lock step on the
interleaved block products of ``csrc/spmm_device.h``.  The ``*_host`` functions are the NumPy statement - the
specification the device code (``csrc/lanczos_filter.hip``) is tested against; ``lanczos_run`` / ``lanczos_filter`` are
the device entries.  Indices are 0-based: ``betas[0] = ||b||``, step i uses ``v_i``, yields ``alphas[i]`` and
``betas[i + 1]``, and ``v_{i+1} = (H v_i - alphas[i] v_i - betas[i] v_{i-1}) / betas[i+1]``.
"""
import collections
import ctypes as C
import math
import weakref

import numpy as np

__all__ = ["lanczos_scalars_host", "minres_coefficients", "filter_coefficients", "lanczos_combine_host",
           "lanczos_filter_host", "lanczos_run", "lanczos_filter", "LanczosRun", "LanczosScalars", "MAX_COLUMNS_PER_CALL",
           "MAX_SHIFTS_PER_RUN", "basis_budget", "split_combinations", "BASIS_MODES", "lanczos_vectors_host",
           "lanczos_combine_prefix_host", "prefix_split", "BASIS_PRECISIONS", "lanczos_combine_stored_host",
           "basis_slot_bytes"]

MAX_COLUMNS_PER_CALL = 8
MAX_SHIFTS_PER_RUN = 32
BASIS_MODES = ("recompute", "keep")
BASIS_PRECISIONS = ("fp64", "fp32")      # storage of a kept basis; the recurrence and its scalars are fp64 either way
BASIS_SAFETY = 0.9                       # share of the memory in sight a kept basis may take, as the contour pool's
BASIS_COMBINE_WIDTHS = (8, 4, 2, 1)      # combinations per column one hipeig_lanczos_combine call takes from a basis


def basis_budget(hbm_free, reusable, override=None, held=0):
    """Bytes the next group's kept basis may take.  Without ``override``: nine tenths of the free device memory plus the
    bytes of released bases the context hands out again (memory this run's earlier groups hold is no longer free, so it
    is counted already).  With ``override`` (``basisBytes``): that many bytes for the whole run, less the bytes ``held``
    by its earlier groups.  Never negative."""
    if override is not None:
        if int(override) < 0:
            raise ValueError("basisBytes must not be negative")
        return max(0, int(override) - int(held))
    return max(0, int(BASIS_SAFETY * (int(hbm_free) + int(reusable))))


def basis_slot_bytes(n, k, precision="fp64"):
    """Bytes of one slot - one Lanczos vector of a k-column group - of a kept basis: the interleaved block of width 4
    (k <= 4) or 8, padded to 32 elements, of 8-byte or (``"fp32"``) 4-byte elements."""
    if precision not in BASIS_PRECISIONS:
        raise ValueError(f"precision must be one of {BASIS_PRECISIONS}, not {precision!r}")
    if not 1 <= int(k) <= MAX_COLUMNS_PER_CALL:
        raise ValueError(f"1 to {MAX_COLUMNS_PER_CALL} columns per group")
    width = 4 if int(k) <= 4 else 8
    return (int(n) * width + 31) // 32 * 32 * (4 if precision == "fp32" else 8)


def split_combinations(nc):
    """``[(first, width), ...]``: the calls that serve a table of ``nc`` combinations per column from a kept basis, widest
    first (11 -> 8 + 2 + 1)."""
    nc = int(nc)
    if nc < 1:
        raise ValueError("at least one combination per column")
    out, lo = [], 0
    while lo < nc:
        w = next(w for w in BASIS_COMBINE_WIDTHS if w <= nc - lo)
        out.append((lo, w))
        lo += w
    return out


def prefix_split(m, p):
    """``(stream_terms, products)`` of a combination of ``m`` terms from a basis that holds the first ``p`` vectors.
    ``m <= p``: the stream takes all ``m`` terms, no product.  Otherwise the stream takes the terms ``i < p - 1``, the
    recurrence restarts from ``v_{p-2}``, ``v_{p-1}`` and runs the steps ``p - 1 .. m - 2`` - ``m - p`` products - and the
    last term needs none: ``stream_terms + products + 1 == m``."""
    m, p = int(m), int(p)
    if m < 0 or p < 0:
        raise ValueError("negative number of terms or vectors")
    if m <= p:
        return m, 0
    if p == 0:
        raise ValueError("a prefix holds at least one vector")
    return p - 1, m - p


def _checked_prefix(prefix, keeps, what):
    """``prefix`` only makes sense on top of a kept basis."""
    if prefix and not keeps:
        raise ValueError(f"{what}: keeping a prefix of the basis needs the basis to be kept")
    return bool(prefix)


def _checked_precision(value, keeps, what):
    """``value`` is one of ``BASIS_PRECISIONS``, and ``"fp32"`` only makes sense for a kept basis."""
    if value not in BASIS_PRECISIONS:
        raise ValueError(f"{what} must be one of {BASIS_PRECISIONS}, not {value!r}")
    if value == "fp32" and not keeps:
        raise ValueError(f"{what}: storing the basis in fp32 needs the basis to be kept")
    return value


def _checked_basis_mode(value, what):
    if value not in BASIS_MODES:
        raise ValueError(f"{what} must be one of {BASIS_MODES}, not {value!r}")
    return value


def _checked_tables(G, ncols, steps, kept):
    """The coefficient tables as contiguous ``[m_r, NC]`` arrays and NC; ``steps[r]``: the steps column r ran; ``kept``:
    every group holds its basis or at least a prefix of it (any NC), else the product pass has to serve some (NC = 1 or
    2)."""
    if len(G) != ncols:
        raise ValueError("one coefficient table per column")
    tabs = [np.asarray(g, dtype=np.float64) for g in G]
    tabs = [np.ascontiguousarray(t[:, None] if t.ndim == 1 else t) for t in tabs]
    nc = {t.shape[1] for t in tabs}
    if len(nc) != 1 or next(iter(nc)) < 1:
        raise ValueError("coefficient tables of one width, NC >= 1")
    nc = next(iter(nc))
    if nc not in (1, 2) and not kept:
        raise ValueError("coefficient tables of one width, NC = 1 or 2 (wider tables need a kept basis in every group)")
    for r, t in enumerate(tabs):
        if len(t) > steps[r]:
            raise ValueError(f"column {r}: {len(t)} coefficients but the run took {steps[r]} steps")
    return tabs, nc


def _release_bases(ctx, bases):
    from . import _lib
    for g, h in enumerate(bases):
        if h is not None:
            bases[g] = None
            _lib.call("hipeig_lanczos_basis_release", ctx.handle, h)

LanczosScalars = collections.namedtuple("LanczosScalars", "alphas betas iterations estimates converged")


def _scalars_one(matvec, b, zs, rtol, atol, maxiter, sign):
    """One column: the loop of ``shifted_minres_host`` - the same scalar expressions in the same order - without its
    ``d`` and ``x`` vectors."""
    S = zs.size
    its = np.zeros(S, dtype=int)
    beta1 = float(np.linalg.norm(b))
    if beta1 == 0.0:
        return LanczosScalars(np.zeros(0), np.zeros(1), its, np.zeros(S), np.ones(S, dtype=bool))
    target = max(atol, rtol * beta1)
    c1 = np.ones(S, complex)
    s1 = np.zeros(S, complex)
    c2 = np.ones(S, complex)
    s2 = np.zeros(S, complex)
    tau = np.full(S, beta1, complex)
    live = np.ones(S, dtype=bool)
    alphas, betas = [], [beta1]
    v_old, v, beta = np.zeros(b.size), b / beta1, 0.0
    for k in range(1, maxiter + 1):
        w = matvec(v) - beta * v_old
        alpha = float(v @ w)
        w = w - alpha * v
        beta_new = float(np.linalg.norm(w))
        alphas.append(alpha)
        betas.append(beta_new)
        for j in range(S):
            if not live[j]:
                continue
            t_up, t_d, t_lo = -sign * beta, sign * (zs[j] - alpha), -sign * beta_new
            tmp = c2[j] * t_up
            dd = -s1[j] * tmp + c1[j] * t_d
            nu = math.hypot(abs(dd), abs(t_lo))
            c, s = dd / nu, t_lo / nu
            tau[j] = -s * tau[j]
            c2[j], s2[j], c1[j], s1[j] = c1[j], s1[j], c, s
            its[j] = k
            if abs(tau[j]) <= target:
                live[j] = False
        if not live.any() or beta_new == 0.0:
            break
        v_old, v, beta = v, w / beta_new, beta_new
    return LanczosScalars(np.array(alphas), np.array(betas), its, np.abs(tau), ~live)


def lanczos_scalars_host(matvec, B, shifts, rtol, atol, maxiter, sign=1.0):
    """Pass 1 for every row of ``B`` (``[K, n]``, real): a list of ``LanczosScalars(alphas[m], betas[m + 1],
    iterations[S], estimates[S], converged[S])``, m the steps the column ran.  Stop rule, breakdown, ``maxiter`` and a zero
    right-hand side (m = 0, everything converged at once) as ``shifted_minres_host``; the columns are independent."""
    B = np.atleast_2d(np.asarray(B, dtype=np.float64))
    zs = np.asarray(shifts, dtype=complex).reshape(-1)
    return [_scalars_one(matvec, b, zs, rtol, atol, maxiter, sign) for b in B]


def _coefficients_batch(alphas, betas, zs, ms, sign):
    """``y[R, S, mmax]``: for column r (``alphas[r, :]``, ``betas[r, :]``, padded to ``mmax`` / ``mmax + 1``) and shift s
    the coefficients of the MINRES iterate at step ``ms[r, s]`` in the Lanczos basis, zero from that step on.  The
    rotation recurrence of the twin yields column k of R (``nu`` on the diagonal, ``r1``, ``r2`` above it) and entry k
    of ``Q^H beta_0 e_1`` (``conj(c_k) tau_{k-1}``); neither depends on where a shift stops, so one forward sweep serves
    all stop steps and the back substitution ``y_k = (t_k - r1_{k+1} y_{k+1} - r2_{k+2} y_{k+2}) / nu_k`` runs in O(m)."""
    alphas = np.asarray(alphas, dtype=np.float64)
    betas = np.asarray(betas, dtype=np.float64)
    ms = np.asarray(ms, dtype=int)
    R, S = ms.shape
    mmax = int(ms.max()) if ms.size else 0
    y = np.zeros((R, S, mmax), complex)
    if mmax == 0:
        return y
    z = np.asarray(zs, dtype=complex).reshape(1, S)
    nu = np.zeros((mmax, R, S))
    r1 = np.zeros((mmax, R, S), complex)
    r2 = np.zeros((mmax, R, S), complex)
    t = np.zeros((mmax, R, S), complex)
    c1 = np.ones((R, S), complex)
    s1 = np.zeros((R, S), complex)
    c2 = np.ones((R, S), complex)
    s2 = np.zeros((R, S), complex)
    tau = np.repeat(betas[:, :1].astype(complex), S, axis=1)
    with np.errstate(all="ignore"):                      # entries past a column's own steps are never used
        for k in range(mmax):
            t_up = (-sign * betas[:, k:k + 1]) if k else np.zeros((R, 1))
            t_d = sign * (z - alphas[:, k:k + 1])
            t_lo = -sign * betas[:, k + 1:k + 2]
            tmp = c2 * t_up
            r2[k] = np.conj(s2) * t_up
            r1[k] = np.conj(c1) * tmp + np.conj(s1) * t_d
            dd = -s1 * tmp + c1 * t_d
            nu[k] = np.hypot(np.abs(dd), np.abs(t_lo))
            c, s = dd / nu[k], t_lo / nu[k]
            t[k] = np.conj(c) * tau
            tau = -s * tau
            c2, s2, c1, s1 = c1, s1, c, s
        y1 = np.zeros((R, S), complex)                   # y_{k+1}, y_{k+2}
        y2 = np.zeros((R, S), complex)
        for k in range(mmax - 1, -1, -1):
            rhs = t[k].copy()
            if k + 1 < mmax:
                rhs -= np.where(ms > k + 1, r1[k + 1] * y1, 0.0)
            if k + 2 < mmax:
                rhs -= np.where(ms > k + 2, r2[k + 2] * y2, 0.0)
            yk = np.where(ms > k, rhs / nu[k], 0.0)
            y[:, :, k] = yk
            y1, y2 = yk, y1
    return y


def minres_coefficients(alphas, betas, z, m, sign=1.0):
    """``y`` (complex, length m): the MINRES iterate at step m of ``sign*(z I - H) x = b`` is ``sum_i y[i] v_i``."""
    m = int(m)
    a = np.zeros((1, m))
    bt = np.zeros((1, m + 1))
    a[0, :] = np.asarray(alphas, dtype=np.float64)[:m]
    bt[0, :] = np.asarray(betas, dtype=np.float64)[:m + 1]
    return _coefficients_batch(a, bt, [z], np.array([[m]]), sign)[0, 0]


def filter_coefficients(scalars, shifts, weights, sign=1.0):
    """``G[r]`` (``[m_r, 1]``, real) with ``G[r][i, 0] = Re(sum_j weights[j] y_{j,i})`` for every column of a pass-1 result
    (a list of records with ``alphas``, ``betas``, ``iterations``), each shift taken at its own stop step."""
    R = len(scalars)
    zs = np.asarray(shifts, dtype=complex).reshape(-1)
    w = np.asarray(weights, dtype=complex).reshape(-1)
    if w.size != zs.size:
        raise ValueError("one weight per shift")
    ms = np.array([[int(i) for i in sc.iterations] for sc in scalars], dtype=int).reshape(R, zs.size)
    mmax = int(ms.max()) if ms.size else 0
    a = np.zeros((R, mmax))
    bt = np.zeros((R, mmax + 1))
    for r, sc in enumerate(scalars):
        m = int(ms[r].max()) if zs.size else 0
        a[r, :m] = np.asarray(sc.alphas)[:m]
        bt[r, :m + 1] = np.asarray(sc.betas)[:m + 1]
    y = _coefficients_batch(a, bt, zs, ms, sign)
    g = np.einsum("j,rji->ri", w, y).real
    return [np.ascontiguousarray(g[r, :int(ms[r].max()) if zs.size else 0].reshape(-1, 1)) for r in range(R)]


def lanczos_combine_host(matvec, B, alphas, betas, G):
    """Pass 2: for every row r of ``B`` the ``[NC, n]`` array ``sum_i G[r][i, c] v_i`` (``G[r]``: ``[m_r, NC]``), the
    Lanczos vectors rebuilt from the stored scalars - no dot products; the last term needs no product."""
    B = np.atleast_2d(np.asarray(B, dtype=np.float64))
    out = []
    for r, b in enumerate(B):
        g = np.asarray(G[r], dtype=np.float64)
        g = g[:, None] if g.ndim == 1 else g
        m, nc = g.shape
        q = np.zeros((nc, b.size))
        if m:
            a, bt = np.asarray(alphas[r], dtype=np.float64), np.asarray(betas[r], dtype=np.float64)
            v_old, v = np.zeros(b.size), b / bt[0]
            for i in range(m):
                q += g[i][:, None] * v[None, :]
                if i + 1 < m:
                    # pass 1's expressions in pass 1's order: with the same products the vectors repeat bit for bit
                    w = matvec(v) - (bt[i] if i else 0.0) * v_old
                    w = w - a[i] * v
                    v_old, v = v, w / bt[i + 1]
        out.append(q)
    return out


def lanczos_vectors_host(matvec, b, alphas, betas, p):
    """``V[p, n]``: the first ``p`` Lanczos vectors of one column ``b`` as ``lanczos_combine_host`` rebuilds them from the
    scalars (its expressions, its order), ``p`` at most ``len(alphas)``, the steps the column ran."""
    b = np.asarray(b, dtype=np.float64)
    a, bt = np.asarray(alphas, dtype=np.float64), np.asarray(betas, dtype=np.float64)
    p = int(p)
    if not 0 <= p <= len(a):
        raise ValueError("0 to len(alphas) vectors")
    V = np.zeros((p, b.size))
    v_old, v = np.zeros(b.size), (b / bt[0] if p else b)
    for i in range(p):
        V[i] = v
        if i + 1 < p:
            w = matvec(v) - (bt[i] if i else 0.0) * v_old
            w = w - a[i] * v
            v_old, v = v, w / bt[i + 1]
    return V


def lanczos_combine_prefix_host(matvec, V, alphas, betas, G):
    """Pass 2 of one column from a prefix: ``V`` (``[p, n]``, p >= 1) holds its first p Lanczos vectors, ``G`` is ``[m]`` or
    ``[m, NC]``.  Returns ``[NC, n]``.  ``prefix_split(m, p)``: the terms it assigns to the stream come from ``V``, then the
    recurrence of ``lanczos_combine_host`` runs from ``V[p - 2]``, ``V[p - 1]`` - its expressions in its order, every
    term added in ascending i, so the result is ``lanczos_combine_host``'s bit for bit."""
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    g = np.asarray(G, dtype=np.float64)
    g = g[:, None] if g.ndim == 1 else g
    m, nc = g.shape
    p = len(V)
    q = np.zeros((nc, V.shape[1]))
    stream, products = prefix_split(m, p)
    for i in range(stream):
        q += g[i][:, None] * V[i][None, :]
    if m <= p:
        return q
    a, bt = np.asarray(alphas, dtype=np.float64), np.asarray(betas, dtype=np.float64)
    v_old, v = (V[p - 2] if p >= 2 else np.zeros(V.shape[1])), V[p - 1]
    for i in range(p - 1, m):
        q += g[i][:, None] * v[None, :]
        if i + 1 < m:
            w = matvec(v) - (bt[i] if i else 0.0) * v_old
            w = w - a[i] * v
            v_old, v = v, w / bt[i + 1]
    return q


def lanczos_combine_stored_host(matvec, b, alphas, betas, G, p, dtype=np.float64):
    """Pass 2 of one column from a basis stored in ``dtype``: the NumPy statement of ``basis_mode`` 3 / 4.  Returns
    ``[NC, n]`` (``G``: ``[m]`` or ``[m, NC]``).

    Pass 1's recurrence (the expressions of ``lanczos_combine_host``, fp64) leaves the un-normalised ``r_i = beta_i v_i``
    of the first ``p`` vectors (``r_0 = b``; ``1 <= p <= len(alphas)``) in an array of ``dtype``.  The terms
    ``prefix_split(m, p)`` assigns to the stream are formed from it as ``v = r_i / beta_i`` - the stored element widened to
    fp64, then this twin's own normalisation (the device multiplies by the ``1 / beta_i`` its pass 1 used) - and added in
    ascending i in fp64; the tail runs the recurrence in fp64 from the exact ``v_{p-2}``, ``v_{p-1}``, never from the
    stored copies.  With ``dtype=np.float64`` nothing is rounded and the result is ``lanczos_combine_prefix_host``'s bit
    for bit.

    With ``dtype=np.float32`` a stored element carries a relative error of at most 2^-24, so per combination c
    ``||q32 - q64||_2 <= 2^-24 sum_{i in stream} |G[i, c]| ||v_i||``, and ``||v_i|| = 1``.  Precondition: the vectors are
    stored un-normalised, so the bound holds while their elements stay in fp32's normal range (about 1e-38 .. 3e38 in
    magnitude; smaller ones lose relative accuracy, larger ones overflow).  ``||r_i|| = beta_i`` is of the size of
    ``||H||`` for i >= 1 and ``||b||`` for i = 0; FEAST's subspace vectors are normalised, so there the precondition is
    one on the operator's scale alone."""
    b = np.asarray(b, dtype=np.float64)
    a, bt = np.asarray(alphas, dtype=np.float64), np.asarray(betas, dtype=np.float64)
    g = np.asarray(G, dtype=np.float64)
    g = g[:, None] if g.ndim == 1 else g
    m, nc = g.shape
    p = int(p)
    if not 1 <= p <= len(a):
        raise ValueError("1 to len(alphas) vectors")
    R = np.zeros((p, b.size), dtype=dtype)
    R[0] = b
    v_old, v = np.zeros(b.size), b / bt[0]
    for i in range(p - 1):
        w = matvec(v) - (bt[i] if i else 0.0) * v_old
        w = w - a[i] * v
        R[i + 1] = w                                      # rounded to dtype here, to nearest even
        v_old, v = v, w / bt[i + 1]
    q = np.zeros((nc, b.size))
    stream, products = prefix_split(m, p)
    for i in range(stream):
        q += g[i][:, None] * (R[i].astype(np.float64) / bt[i])[None, :]
    if m <= p:
        return q
    for i in range(p - 1, m):                             # v_old, v are the exact v_{p-2}, v_{p-1}
        q += g[i][:, None] * v[None, :]
        if i + 1 < m:
            w = matvec(v) - (bt[i] if i else 0.0) * v_old
            w = w - a[i] * v
            v_old, v = v, w / bt[i + 1]
    return q


def lanczos_filter_host(matvec, B, shifts, weights, rtol, atol, maxiter, sign=1.0):
    """``(q[K, n], scalars)`` with ``q_r = sum_j Re(weights[j] x_{j,r})``, ``x_{j,r}`` the MINRES iterate of
    ``sign*(z_j I - H) x = B[r]`` at its own stop step; ``scalars`` is pass 1's result.  A shift still live at the step
    limit raises ``UserWarning``, as the device entry ``lanczos_filter`` does (``lanczos_scalars_host`` only reports)."""
    B = np.atleast_2d(np.asarray(B, dtype=np.float64))
    scalars = lanczos_scalars_host(matvec, B, shifts, rtol, atol, maxiter, sign)
    if not all(np.all(s.converged) for s in scalars):
        raise UserWarning("Warning:: Iterative solver is not converged ")
    G = filter_coefficients(scalars, shifts, weights, sign)
    q = lanczos_combine_host(matvec, B, [s.alphas for s in scalars], [s.betas for s in scalars], G)
    return np.array([x[0] for x in q]).reshape(len(B), -1), scalars


# ---- device ----------------------------------------------------------------------------------------------------------
class LanczosRun:
    """Pass 1's result for the columns ``B``: ``scalars[r]`` (a ``LanczosScalars``), ``info[r]`` (0, or the step limit when
    a shift of column r was still live there), ``groups`` (the column ranges of the calls of <= 8) and
    ``products_pass1[g]`` (block products of group g).  ``combine(G)`` is pass 2.  After ``lanczos_run(keepBasis=True)``
    ``basis_kept[g]`` tells whether group g's Lanczos vectors stayed in device memory, ``basis_bytes`` what they hold and
    ``release()`` gives them back; ``combine`` then streams over them instead of repeating the products.  With
    ``keepPrefix=True`` a group may hold only its first ``basis_vectors[g]`` vectors (``basis_kept[g]`` is then False);
    ``combine`` streams over those and repeats the products of the rest.  ``basis_precision`` is the storage asked for
    (``"fp64"`` or ``"fp32"``): ``combine`` is the same call either way."""

    def __init__(self, H, B, shifts, sign, basis_precision="fp64"):
        self.H, self.B, self.shifts, self.sign = H, list(B), list(shifts), sign
        self.basis_precision = basis_precision
        self.scalars, self.info, self.groups, self.products_pass1, self.products_pass2 = [], [], [], [], []
        self._bases = []                                  # per group: the basis handle, or None
        self._finalizer = weakref.finalize(self, _release_bases, self.B[0].ctx, self._bases)

    @property
    def converged(self):
        return all(i == 0 for i in self.info)

    @property
    def basis_vectors(self):
        """Lanczos vectors held per group: those of its longest column, 0 without a basis."""
        return [int(self._basis_info(g)[0]) if h is not None else 0 for g, h in enumerate(self._bases)]

    @property
    def basis_kept(self):
        """Per group: the whole basis is held (a prefix does not count)."""
        return [h is not None and v >= p for h, v, p in zip(self._bases, self.basis_vectors, self.products_pass1)]

    def _basis_info(self, g):
        from . import _lib
        info = (C.c_int64 * 8)()
        _lib.call("hipeig_lanczos_basis_info", self.B[0].ctx.handle, self._bases[g], info)
        return list(info)

    @property
    def basis_element_bytes(self):
        """Bytes of one stored element per group (8 or 4), 0 without a basis."""
        from . import _lib
        out = []
        for h in self._bases:
            nbytes = C.c_int(0)
            _lib.call("hipeig_lanczos_basis_element_bytes", self.B[0].ctx.handle, h, C.byref(nbytes))
            out.append(int(nbytes.value))
        return out

    @property
    def basis_bytes(self):
        """Bytes of device memory the kept bases hold."""
        return sum(self._basis_info(g)[1] for g, h in enumerate(self._bases) if h is not None)

    def release(self):
        """Give the kept bases back to the context (which reuses their segments); ``combine`` then takes the product pass."""
        _release_bases(self.B[0].ctx, self._bases)

    def combine(self, G):
        """``sum_i G[r][i, c] v_i`` for every column: ``G[r]`` of shape ``[m_r, NC]`` with ``m_r`` at most the steps
        column r ran.  NC = 1: a list of ``HipVector``; NC = 2: of ``HipComplexVector`` (c = 0 the real half, c = 1 the
        imaginary one); wider: a list of NC ``HipVector`` per column.  ``products_pass2[g]`` then holds the block products
        of group g: its largest ``m_r`` minus one - or 0 where the group's basis was kept: those groups are served by one
        stream over the stored vectors, any number of times, with NC up to 8 per call (wider tables are split).  A group
        that holds a prefix of p vectors is served the same way and adds ``prefix_split(mmax, p)[1]`` products per call
        of the split.  A group without a basis takes the product pass, which serves NC = 1 or 2 (``ValueError``
        otherwise)."""
        from . import _lib
        from .hip_vector import HipComplexVector, _ptr_table
        kept = bool(self._bases) and all(h is not None for h in self._bases)
        tabs, nc = _checked_tables(G, len(self.B), [len(s.alphas) for s in self.scalars], kept)
        ctx, n = self.B[0].ctx, len(self.B[0])
        out, self.products_pass2 = [], []
        dp = C.POINTER(C.c_double)
        for g, (lo, hi) in enumerate(self.groups):
            k = hi - lo
            basis = self._bases[g] if g < len(self._bases) else None
            m = (C.c_int * k)(*[len(tabs[r]) for r in range(lo, hi)])
            al = [np.ascontiguousarray(self.scalars[r].alphas, dtype=np.float64) for r in range(lo, hi)]
            be = [np.ascontiguousarray(self.scalars[r].betas, dtype=np.float64) for r in range(lo, hi)]
            pa = (dp * k)(*[a.ctypes.data_as(dp) for a in al])
            pb = (dp * k)(*[b.ctypes.data_as(dp) for b in be])
            bt, keep1 = _ptr_table([b._buf for b in self.B[lo:hi]])
            # products per call: 0 from a whole basis, all but the last term's without one
            expect = prefix_split(max(m), self._basis_info(g)[0])[1] if basis is not None else max(max(m) - 1, 0)
            cols = [[None] * nc for _ in range(k)]
            products, stats = 0, (C.c_double * 2)()
            for c0, w in split_combinations(nc):
                part = [np.ascontiguousarray(tabs[r][:, c0:c0 + w]) for r in range(lo, hi)]
                pg = (dp * k)(*[t.ctypes.data_as(dp) for t in part])
                bufs = [ctx.alloc(n) for _ in range(k * w)]
                qt, keep2 = _ptr_table(bufs)
                _lib.call("hipeig_lanczos_combine", ctx.handle, self.H.handle, basis, k, bt, m, pa, pb, w, pg, qt, stats)
                if int(stats[0]) != expect:
                    raise RuntimeError(f"pass 2 made {int(stats[0])} products, not {expect}")
                products += expect
                for j in range(k):
                    cols[j][c0:c0 + w] = [self.B[lo + j]._new(bufs[j * w + c]) for c in range(w)]
            self.products_pass2.append(products)
            for j in range(k):
                out.append(cols[j][0] if nc == 1 else HipComplexVector(*cols[j]) if nc == 2 else cols[j])
        return out


def _checked_inputs(H, B, what):
    from .hip_vector import HipComplexVector, HipCsrOperator, HipVector
    if not isinstance(H, HipCsrOperator):
        raise TypeError(f"{what} needs a HipCsrOperator (device-resident CSR)")
    B = list(B)
    if not B:
        raise ValueError(f"{what} needs at least one right-hand side")
    for b in B:
        if isinstance(b, HipComplexVector) or not isinstance(b, HipVector):
            raise NotImplementedError("the Lanczos filter takes real HipVector right-hand sides (the Lanczos run is real)")
    if B[0].ctx.collectives:
        raise NotImplementedError("the Lanczos filter runs on whole vectors on one GPU: a context with collectives "
                                  "(row partition, HIPEIG_FORCE_COLLECTIVES) is not supported")
    return B


def _default_basis_budget(ctx, basisBytes, held):
    """``basis_budget`` on the context's figures: free device memory and the bytes of released bases it would reuse."""
    from . import _lib
    if basisBytes is not None:
        return basis_budget(0, 0, basisBytes, held)
    info = (C.c_int64 * 8)()
    _lib.call("hipeig_lanczos_basis_info", ctx.handle, None, info)
    return basis_budget(ctx.device_info()["hbm_free"], info[5])


def lanczos_run(H, B, shifts, reverseGF=False, keepBasis=False, basisBytes=None, keepPrefix=False, basisPrecision="fp64"):
    """Pass 1 on the device (``hipeig_lanczos_block_scalars``) for the real ``HipVector``s ``B`` and up to 32 ``shifts``
    (real or complex) of ``sign*(z I - H)``, ``sign = -1`` with ``reverseGF``: a ``LanczosRun``.  More than 8 columns are
    grouped into calls of 8, each in lock step on block products.  Tolerances and the step limit come from
    ``B[0].options["linearSystemArgs"]`` as in ``solve_shifts``.  Nothing is raised here: ``run.info`` tells.

    ``keepBasis``: every group keeps its Lanczos vectors in device memory (``basis_mode`` 1, the same
    scalars) as long as the byte budget allows - ``basisBytes`` for the whole run, by default ``basis_budget`` of the free
    device memory.  A group whose basis does not fit finishes as a plain pass 1; ``run.basis_kept`` tells.

    ``keepPrefix`` (with ``keepBasis``): such a group keeps the vectors that fit instead (``basis_mode`` 2, again the same
    scalars); ``run.basis_vectors`` tells how many.

    ``basisPrecision="fp32"`` (with ``keepBasis``): the basis is stored in fp32 (``basis_mode`` 3, with ``keepPrefix`` 4) -
    twice the vectors per byte of budget.  The recurrence and its scalars are the plain run's; pass 1 writes ``4 n K`` more
    bytes per step, and ``combine`` differs from the fp64 basis's result by the rounding of the stored elements
    (``lanczos_combine_stored_host`` has the bound and its precondition)."""
    from . import _lib
    from .hip_vector import _ptr_table
    keepPrefix = _checked_prefix(keepPrefix, keepBasis, "lanczos_run(keepPrefix=True)")
    basisPrecision = _checked_precision(basisPrecision, keepBasis, "lanczos_run(basisPrecision)")
    B = _checked_inputs(H, B, "lanczos_run")
    if basisBytes is not None and int(basisBytes) < 0:
        raise ValueError("basisBytes must not be negative")
    zs = [complex(z) for z in np.asarray(shifts).reshape(-1)]
    if not 1 <= len(zs) <= MAX_SHIFTS_PER_RUN:
        raise ValueError(f"lanczos_run takes 1 to {MAX_SHIFTS_PER_RUN} shifts")
    ctx = B[0].ctx
    H.honour_reduction_option(B[0].options)
    o = B[0].options["linearSystemArgs"]
    rtol, atol, maxiter = float(o["linear_tol"]), float(o.get("linear_atol", 0.0)), int(o["linearIter"])
    sign = -1.0 if reverseGF else 1.0
    run = LanczosRun(H, B, zs, sign, basisPrecision)
    mode = (2 if keepPrefix else 1 if keepBasis else 0) + (2 if basisPrecision == "fp32" else 0)
    S = len(zs)
    zr = (C.c_double * S)(*[z.real for z in zs])
    zi = (C.c_double * S)(*[z.imag for z in zs])
    for lo in range(0, len(B), MAX_COLUMNS_PER_CALL):
        hi = min(lo + MAX_COLUMNS_PER_CALL, len(B))
        k = hi - lo
        bt, keep = _ptr_table([b._buf for b in B[lo:hi]])
        alphas = np.zeros((k, maxiter))
        betas = np.zeros((k, maxiter + 1))
        its = (C.c_int * (k * S))()
        est = (C.c_double * (k * S))()
        info = (C.c_int * k)()
        stats = (C.c_double * (1 + k))()
        dp = C.POINTER(C.c_double)
        basis = C.c_void_p()
        budget = _default_basis_budget(ctx, basisBytes, run.basis_bytes) if keepBasis else 0
        _lib.call("hipeig_lanczos_block_scalars", ctx.handle, H.handle, sign, k, bt, S, zr, zi, rtol, atol, maxiter,
                  alphas.ctypes.data_as(dp), betas.ctypes.data_as(dp), its, est, info, stats,
                  mode, budget, C.byref(basis))
        run._bases.append(C.c_void_p(basis.value) if basis.value else None)
        run.groups.append((lo, hi))
        run.products_pass1.append(int(stats[0]))
        for j in range(k):
            m = int(stats[1 + j])
            it = np.array(its[j * S:(j + 1) * S], dtype=int)
            run.scalars.append(LanczosScalars(alphas[j, :m].copy(), betas[j, :m + 1].copy(), it,
                                              np.array(est[j * S:(j + 1) * S]), np.array([info[j] == 0] * S)))
            run.info.append(int(info[j]))
    return run


def lanczos_filter(H, B, shifts, weights, reverseGF=False, basis="recompute", basisBytes=None, prefix=False,
                   precision="fp64"):
    """``[q_r]`` (``HipVector``) with ``q_r = sum_j Re(weights[j] x_{j,r})``, ``x_{j,r}`` the MINRES iterate of
    ``sign*(z_j I - H) x = B[r]`` at its own stop step - FEAST's filtered vectors with ``weights[j] = -0.5 w_j r phase_j`` -
    from two Lanczos passes on the device, no solution ever formed.  Every ``b.last_solve_stats`` = ``{"iterations":
    [per shift], "estimates": [|tau_j|], "products": block products of both passes of b's group, "products_pass1",
    "products_pass2", "basis": "kept" | "prefix" | "recomputed", "basis_vectors": vectors of the group held for pass 2, "basis_precision": "fp64" | "fp32"}``.  A shift still live at the step limit raises ``UserWarning`` as
    every other solver does.

    ``basis="keep"``: group by group - pass 1 with its vectors kept, coefficients, one stream over the vectors, release - so
    at most one group's basis is alive at a time and every group has the whole budget (``basisBytes``, default
    ``basis_budget``).  A group whose basis does not fit is served by the product pass and reports ``"recomputed"`` - or,
    with ``prefix=True``, keeps the vectors that fit, repeats only the products behind them and reports ``"prefix"``.
    ``precision="fp32"`` (with ``basis="keep"``) stores the basis in fp32, see ``lanczos_run``."""
    prefix = _checked_prefix(prefix, basis == "keep", "lanczos_filter(prefix=True)")
    precision = _checked_precision(precision, basis == "keep", "lanczos_filter(precision)")
    B = _checked_inputs(H, B, "lanczos_filter")
    _checked_basis_mode(basis, "basis")
    if len(np.asarray(weights).reshape(-1)) != len(np.asarray(shifts).reshape(-1)):
        raise ValueError("one weight per shift")
    if basis == "keep":
        spans = [(lo, min(lo + MAX_COLUMNS_PER_CALL, len(B))) for lo in range(0, len(B), MAX_COLUMNS_PER_CALL)]
    else:
        spans = [(0, len(B))]                                       # every group's pass 1 first, then every pass 2
    q, converged = [], True
    for first, (lo, hi) in enumerate(spans):
        run = lanczos_run(H, B[lo:hi], shifts, reverseGF=reverseGF, keepBasis=basis == "keep", basisBytes=basisBytes,
                          keepPrefix=prefix, basisPrecision=precision)
        try:
            G = filter_coefficients(run.scalars, run.shifts, weights, run.sign)
            part = run.combine(G) if run.converged else None
            kept, held = run.basis_kept, run.basis_vectors
        finally:
            run.release()
        converged = converged and part is not None
        for g, (glo, ghi) in enumerate(run.groups):
            p1 = run.products_pass1[g]
            p2 = run.products_pass2[g] if part is not None else 0
            for r in range(glo, ghi):
                b = B[lo + r]
                b.last_solve_stats = {"iterations": [int(i) for i in run.scalars[r].iterations],
                                      "estimates": [float(e) for e in run.scalars[r].estimates],
                                      "products": p1 + p2, "products_pass1": p1, "products_pass2": p2, "group": first + g,
                                      "basis": "kept" if kept[g] else "prefix" if held[g] else "recomputed",
                                      "basis_vectors": held[g], "basis_precision": precision}
                if part is not None:
                    part[r].last_solve_stats = b.last_solve_stats
        if part is not None:
            q.extend(part)
    if not converged:
        raise UserWarning("Warning:: Iterative solver is not converged ")
    return q
