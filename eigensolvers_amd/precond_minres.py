"""NumPy twin of the Jacobi-preconditioned device MINRES (``csrc/minres_precond.hip``).

``scipy.sparse.linalg.minres(A, b, M=...)`` (SciPy 1.15.3) restated for a diagonal ``M^-1 = diag(minv)`` in the order of
evaluation the device uses: ``z = minv * r2`` is a vector of its own, the Lanczos vector is ``v = z / beta`` and
``beta^2 = <r2, z>``; every scalar recurrence and stopping test is that of the plain solver.  The reference calls SciPy's
``minres`` without ``M`` (numpyVector.py:163), so this path has no counterpart there; SciPy itself is the referee
(``tests/test_precond_minres_cpu.py``).

``minres_jacobi_block_host`` is the lock-step block form (``csrc/minres_block_precond.hip``): the same recurrence for the
columns of an ``[n, k]`` array with one block product per iteration, every column masked once it has stopped.

``jacobi_inverse_host`` is the NumPy statement of ``hipeig_jacobi_inverse`` and ``csr_diagonal_host`` that of
``hipeig_csr_diagonal``.

The separable (fast-diagonalisation) preconditioner of ``HipKronSumOperator`` (``csrc/kron_precond.hip``):
``separable_fit_host`` is the additive least-squares fit of ``V``, ``separable_basis_host`` the decompositions
``T_d + diag(v_d) = Q_d diag(lam_d) Q_d^T``, ``separable_scale_host`` the statement of ``hipeig_kron_precond_scale``,
``separable_apply_host`` that of ``hipeig_kron_precond_apply`` and ``minres_precond_host`` the recurrence of
``minres_jacobi_host`` with any symmetric positive definite ``M^-1`` given as a function.
"""
import math

import numpy as np


def csr_diagonal_host(A):
    """``d_i`` = sum of the stored ``(i, i)`` entries of row ``i`` of a scipy CSR matrix in stored order (duplicate
    entries are separate stored elements), 0 where a row stores none."""
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    on = A.indices == rows
    d = np.zeros(n)
    np.add.at(d, rows[on], A.data[on])                   # unbuffered: adds in stored order
    return d


def jacobi_inverse_host(diag, sigma, floor=1e-8):
    """``minv_i = 1 / max(t_i, floor * max_j t_j)`` with ``t_i = |sigma - diag_i|``; ``floor`` is relative and ``>= 0``.
    Raises ``ValueError`` where an element would not be finite (a diagonal entry equal to ``sigma`` with ``floor = 0``, a
    non-finite diagonal entry)."""
    floor = float(floor)
    if not (0.0 <= floor < math.inf):
        raise ValueError(f"the relative floor must be finite and >= 0, got {floor!r}")
    t = np.abs(float(sigma) - np.asarray(diag, dtype=np.float64))
    if t.size == 0:
        return t
    tmax = math.inf if np.isnan(t).any() else float(t.max())
    tmin = float(np.nanmin(t))
    floor_abs = floor * tmax if tmax < math.inf else math.inf
    mmin = max(tmin, floor_abs)
    if not (tmax < math.inf) or not (floor_abs < math.inf) or not (mmin > 0.0) or not (1.0 / mmin < math.inf):
        raise ValueError(f"Jacobi preconditioner is not finite: max |sigma - d_i| = {tmax:g}, min = {tmin:g}, relative "
                         f"floor {floor:g} (a diagonal entry equal to sigma needs a floor > 0)")
    return 1.0 / np.maximum(t, floor_abs)


def separable_fit_host(V, dims):
    """The least-squares additive fit ``V ~ sum_d v_d[i_d]`` on the grid ``dims``: ``v_d[i]`` is the mean of ``V`` over all
    other modes at ``i_d = i``, minus ``(D - 1) / D`` times the grand mean (the constant is shared evenly, which fixes the
    one freedom of the fit).  An additive ``V`` is reproduced.  ``V = None`` gives zeros.  Returns ``D`` 1-D arrays."""
    dims = tuple(int(n) for n in dims)
    D = len(dims)
    if V is None:
        return [np.zeros(n) for n in dims]
    V = np.asarray(V, dtype=np.float64).reshape(dims)
    mean = float(V.mean())
    return [V.mean(axis=tuple(e for e in range(D) if e != d)) - (D - 1) / D * mean for d in range(D)]


def separable_basis_host(factors, potentials):
    """``(bases, eigenvalues)``: ``numpy.linalg.eigh(T_d + diag(v_d))`` mode by mode, ``T_d + diag(v_d) = Q_d diag(lam_d)
    Q_d^T``."""
    bases, eigenvalues = [], []
    for T, v in zip(factors, potentials):
        lam, Q = np.linalg.eigh(np.asarray(T, dtype=np.float64) + np.diag(np.asarray(v, dtype=np.float64)))
        bases.append(np.ascontiguousarray(Q))
        eigenvalues.append(np.ascontiguousarray(lam))
    return bases, eigenvalues


def separable_scale_host(eigenvalues, sigma, floor=1e-8):
    """``sinv`` of ``M^-1 = Q diag(sinv) Q^T``, flat in C order: ``Lam_r = ((lam_1[i_1] + lam_2[i_2]) + ...)``, one rounded
    add per mode in mode order, then ``jacobi_inverse_host`` with its relative floor and its refusals."""
    Lam = np.asarray(eigenvalues[0], dtype=np.float64)
    for lam in eigenvalues[1:]:
        Lam = np.add.outer(Lam, np.asarray(lam, dtype=np.float64))
    return jacobi_inverse_host(Lam.reshape(-1), sigma, floor)


def separable_apply_host(bases, sinv, x):
    """``Q (sinv (.) (Q^T x))`` with ``Q = Q_1 (x) ... (x) Q_D``, mode by mode with ``np.tensordot`` in the order of the
    device: the forward modes ``1..D`` (``Q_d^T``), the scale, the backward modes ``1..D`` (``Q_d``).  Works in the dtype
    of ``x`` (``np.longdouble`` for the references of the tests)."""
    dims = tuple(Q.shape[0] for Q in bases)
    X = np.asarray(x).reshape(dims)
    dt = X.dtype
    for d, Q in enumerate(bases):
        X = np.moveaxis(np.tensordot(np.asarray(Q, dtype=dt).T, X, axes=([1], [d])), 0, d)
    X = np.asarray(sinv, dtype=dt).reshape(dims) * X
    for d, Q in enumerate(bases):
        X = np.moveaxis(np.tensordot(np.asarray(Q, dtype=dt), X, axes=([1], [d])), 0, d)
    return X.reshape(-1)


def minres_precond_host(matvec, b, apply_minv, rtol=1e-5, maxiter=None, trace=None):
    """``scipy.sparse.linalg.minres(A, b, M=LinearOperator(apply_minv), rtol=rtol, maxiter=maxiter)`` from ``x = 0``: the
    recurrence of ``minres_jacobi_host`` with ``z = apply_minv(r2)`` in place of ``minv * r2``.

    Returns ``(x, info, itn, istop)``: ``info`` is ``maxiter`` when the iteration limit was the stopping reason
    (``istop == 6``) and 0 otherwise.  ``trace``, a list, receives one record of scalars per iteration.  ``rtol`` is tested
    in SciPy's preconditioned quantities: ``beta1 = sqrt(<b, M^-1 b>)``, ``rnorm = phibar`` in the ``M^-1`` norm."""
    b = np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    if maxiter is None:
        maxiter = 5 * n
    eps = np.finfo(np.float64).eps
    x = np.zeros(n)

    r2 = b.copy()
    z = apply_minv(r2)                                  # start kernel
    beta1 = float(np.dot(r2, z))
    if beta1 < 0:
        raise ValueError("indefinite preconditioner")
    if beta1 == 0.0:
        return x, 0, 0, 0
    beta1 = math.sqrt(beta1)

    oldb = 0.0
    beta = beta1
    dbar = 0.0
    epsln = 0.0
    phibar = beta1
    tnorm2 = 0.0
    gmax = 0.0
    gmin = np.finfo(np.float64).max
    cs = -1.0
    sn = 0.0
    w = np.zeros(n)
    w2 = np.zeros(n)
    r1 = r2
    istop = 0
    itn = 0

    while itn < maxiter:
        itn += 1
        s = 1.0 / beta
        v = s * z                                       # KA': the sweep gathers z
        y = matvec(v)
        if itn >= 2:
            y = y - (beta / oldb) * r1
        alfa = float(np.dot(v, y))
        y = y - (alfa / beta) * r2                      # KC'
        r1 = r2
        r2 = y
        z = apply_minv(r2)
        oldb = beta
        beta = float(np.dot(r2, z))
        if beta < 0:
            raise ValueError("non-symmetric matrix")
        beta = math.sqrt(beta)
        tnorm2 += alfa * alfa + oldb * oldb + beta * beta
        if itn == 1 and beta / beta1 <= 10 * eps:
            istop = -1

        oldeps = epsln
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln = sn * beta
        dbar = -cs * beta
        root = math.sqrt(gbar * gbar + dbar * dbar)

        gamma = max(math.sqrt(gbar * gbar + beta * beta), eps)
        cs = gbar / gamma
        sn = beta / gamma
        phi = cs * phibar
        phibar = sn * phibar

        denom = 1.0 / gamma                             # KD
        w1 = w2
        w2 = w
        w = (v - oldeps * w1 - delta * w2) * denom
        x = x + phi * w

        gmax = max(gmax, gamma)
        gmin = min(gmin, gamma)

        Anorm = math.sqrt(tnorm2)
        ynorm = math.sqrt(float(np.dot(x, x)))
        epsx = Anorm * ynorm * eps
        rnorm = phibar
        test1 = math.inf if (ynorm == 0 or Anorm == 0) else rnorm / (Anorm * ynorm)
        test2 = math.inf if Anorm == 0 else root / Anorm
        Acond = gmax / gmin

        if istop == 0:
            if 1 + test2 <= 1:
                istop = 2
            if 1 + test1 <= 1:
                istop = 1
            if itn >= maxiter:
                istop = 6
            if Acond >= 0.1 / eps:
                istop = 4
            if epsx >= beta1:
                istop = 3
            if test2 <= rtol:
                istop = 2
            if test1 <= rtol:
                istop = 1
        if trace is not None:
            trace.append(dict(itn=itn, alfa=alfa, beta=beta, rnorm=rnorm, ynorm=ynorm,
                              Anorm=Anorm, test1=test1, test2=test2, istop=istop))
        if istop != 0:
            break

    info = maxiter if istop == 6 else 0
    return x, info, itn, istop


def minres_jacobi_host(matvec, b, minv, rtol=1e-5, maxiter=None, trace=None):
    """``scipy.sparse.linalg.minres(A, b, M=diags(minv), rtol=rtol, maxiter=maxiter)`` from ``x = 0``:
    ``minres_precond_host`` with ``z = minv * r2``."""
    minv = np.asarray(minv, dtype=np.float64)
    return minres_precond_host(matvec, b, lambda r: minv * r, rtol, maxiter, trace)


def minres_jacobi_block_host(matvec_block, B, minv, rtol=1e-5, maxiter=None):
    """The lock-step block form of ``minres_jacobi_host`` (``csrc/minres_block_precond.hip``): the columns of ``B``
    (``[n, k]``) advance together, one ``matvec_block`` (``[n, k] -> [n, k]``) per iteration.  Every column keeps its own
    scalars and stopping tests; a column that has stopped (or whose ``<b, M^-1 b>`` is 0) is masked - its Lanczos vector is
    sent into the product as zeros and its iterate is no longer touched.  Returns one ``(x, info, itn, istop)`` per
    column: with a ``matvec_block`` that applies ``matvec`` column by column, the bits of ``minres_jacobi_host``."""
    B = np.asarray(B, dtype=np.float64)
    minv = np.asarray(minv, dtype=np.float64)
    n, k = B.shape
    if maxiter is None:
        maxiter = 5 * n
    eps = np.finfo(np.float64).eps

    def dots(P, Q, cols):                               # per column, on contiguous copies: the bits of the single twin's np.dot
        return {j: float(np.dot(np.ascontiguousarray(P[:, j]), np.ascontiguousarray(Q[:, j]))) for j in cols}

    X = np.zeros((n, k))
    R2 = B.copy()
    Z = minv[:, None] * R2                              # start kernel
    st = []
    for j, bz in dots(R2, Z, range(k)).items():
        if bz < 0:
            raise ValueError("indefinite preconditioner")
        beta1 = math.sqrt(bz)
        st.append(dict(live=bz != 0.0, beta1=beta1, oldb=0.0, beta=beta1, dbar=0.0, epsln=0.0, phibar=beta1, tnorm2=0.0,
                       gmax=0.0, gmin=np.finfo(np.float64).max, cs=-1.0, sn=0.0, istop=0, itn=0))
    W = np.zeros((n, k))
    W2 = np.zeros((n, k))
    R1 = R2
    itn = 0

    def coef(f):                                        # one coefficient per column, 0 for a masked one
        return np.array([f(S) if S["live"] else 0.0 for S in st])

    while itn < maxiter and any(S["live"] for S in st):
        itn += 1
        live = [j for j in range(k) if st[j]["live"]]
        V = coef(lambda S: 1.0 / S["beta"]) * Z         # KA': the sweep gathers Z
        Y = matvec_block(V)
        if itn >= 2:
            Y = Y - coef(lambda S: S["beta"] / S["oldb"]) * R1
        for j, alfa in dots(V, Y, live).items():
            st[j]["alfa"] = alfa
        Y = Y - coef(lambda S: S["alfa"] / S["beta"]) * R2     # KC'
        R1 = R2
        R2 = Y
        Z = minv[:, None] * R2
        yz = dots(R2, Z, live)
        oldeps, delta, denom, phi = np.zeros(k), np.zeros(k), np.zeros(k), np.zeros(k)
        for j in live:
            S = st[j]
            S["itn"] = itn
            S["oldb"] = S["beta"]
            if yz[j] < 0:
                raise ValueError("non-symmetric matrix")
            S["beta"] = math.sqrt(yz[j])
            alfa, oldb, beta = S["alfa"], S["oldb"], S["beta"]
            S["tnorm2"] += alfa * alfa + oldb * oldb + beta * beta
            if itn == 1 and beta / S["beta1"] <= 10 * eps:
                S["istop"] = -1
            oldeps[j] = S["epsln"]
            delta[j] = S["cs"] * S["dbar"] + S["sn"] * alfa
            gbar = S["sn"] * S["dbar"] - S["cs"] * alfa
            S["epsln"] = S["sn"] * beta
            S["dbar"] = -S["cs"] * beta
            S["root"] = math.sqrt(gbar * gbar + S["dbar"] * S["dbar"])
            gamma = max(math.sqrt(gbar * gbar + beta * beta), eps)
            S["cs"] = gbar / gamma
            S["sn"] = beta / gamma
            phi[j] = S["cs"] * S["phibar"]
            S["phibar"] = S["sn"] * S["phibar"]
            denom[j] = 1.0 / gamma
            S["gmax"] = max(S["gmax"], gamma)
            S["gmin"] = min(S["gmin"], gamma)
        W1 = W2                                         # KD
        W2 = W
        W = (V - oldeps * W1 - delta * W2) * denom
        X[:, live] = X[:, live] + phi[live] * W[:, live]
        for j, xx in dots(X, X, live).items():
            S = st[j]
            Anorm = math.sqrt(S["tnorm2"])
            ynorm = math.sqrt(xx)
            epsx = Anorm * ynorm * eps
            test1 = math.inf if (ynorm == 0 or Anorm == 0) else S["phibar"] / (Anorm * ynorm)
            test2 = math.inf if Anorm == 0 else S["root"] / Anorm
            Acond = S["gmax"] / S["gmin"]
            if S["istop"] == 0:
                if 1 + test2 <= 1:
                    S["istop"] = 2
                if 1 + test1 <= 1:
                    S["istop"] = 1
                if itn >= maxiter:
                    S["istop"] = 6
                if Acond >= 0.1 / eps:
                    S["istop"] = 4
                if epsx >= S["beta1"]:
                    S["istop"] = 3
                if test2 <= rtol:
                    S["istop"] = 2
                if test1 <= rtol:
                    S["istop"] = 1
            if S["istop"] != 0:
                S["live"] = False

    return [(X[:, j].copy(), maxiter if S["istop"] == 6 else 0, S["itn"], S["istop"]) for j, S in enumerate(st)]
