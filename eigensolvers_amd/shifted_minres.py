"""Shifted MINRES: ``sign*(z_j I - H) x_j = b`` for many shifts ``z_j`` from ONE Lanczos run on ``H``.

FEAST solves ``(z_k I - H) x_k = b`` for every contour point ``z_k`` with the same real right-hand side and the same
real symmetric ``H`` (feast.py:189-200).  The Krylov space ``K(H, b)`` does not depend on the shift, so one real Lanczos
recurrence - one operator product per step - serves all of them; each shift keeps a complex 2x2 rotation recurrence on
its shifted tridiagonal and a three-term update of its direction and solution vectors (MINRES; no Gram-Schmidt, no
restart, the residual norm ``|tau_j|`` of every shift minimal over the whole Krylov space).  DESIGN.md section 3.5.

``shifted_minres_host`` is the NumPy statement of the recurrences - the specification the device code
(``csrc/minres_shifts.hip``) is tested against; ``solve_shifts`` is the device entry.
"""
import ctypes as C
import math

import numpy as np

__all__ = ["shifted_minres_host", "solve_shifts", "MAX_SHIFTS_PER_CALL"]

MAX_SHIFTS_PER_CALL = 8


def shifted_minres_host(matvec, b, shifts, rtol, atol, maxiter, sign=1.0):
    """``x[S, n]`` (complex), ``iterations[S]``, ``estimates[S]`` (``|tau_j|``, the residual norm of the recurrence) and
    ``converged[S]`` for ``sign*(z_j I - H) x_j = b``; ``matvec(v) = H v`` with ``H`` real symmetric, ``b`` real.  Shift j
    stops after the step at which ``|tau_j| <= max(atol, rtol*||b||)`` (SciPy ``gcrotmk``'s criterion) and is not touched
    again; the run ends when no shift is live, after ``maxiter`` steps, or at a Lanczos breakdown (``beta_{k+1} = 0``,
    whose step is applied first and leaves ``tau_j = 0``).  The Lanczos recurrence does not see the shifts: shift j of an
    S-shift run is bit for bit the one-shift run."""
    b = np.asarray(b, dtype=np.float64)
    zs = np.asarray(shifts, dtype=complex).reshape(-1)
    n, S = b.size, zs.size
    x = np.zeros((S, n), complex)
    its = np.zeros(S, dtype=int)
    beta1 = float(np.linalg.norm(b))
    if beta1 == 0.0:
        return x, its, np.zeros(S), np.ones(S, dtype=bool)
    target = max(atol, rtol * beta1)
    d1 = np.zeros((S, n), complex)
    d2 = np.zeros((S, n), complex)
    c1 = np.ones(S, complex)
    s1 = np.zeros(S, complex)
    c2 = np.ones(S, complex)
    s2 = np.zeros(S, complex)
    tau = np.full(S, beta1, complex)
    live = np.ones(S, dtype=bool)
    v_old, v, beta = np.zeros(n), b / beta1, 0.0
    for k in range(1, maxiter + 1):
        w = matvec(v) - beta * v_old
        alpha = float(v @ w)
        w = w - alpha * v
        beta_new = float(np.linalg.norm(w))
        for j in range(S):
            if not live[j]:
                continue
            # column k of sign*(z I - T): above the diagonal, on it, below it
            t_up, t_d, t_lo = -sign * beta, sign * (zs[j] - alpha), -sign * beta_new
            r2 = np.conj(s2[j]) * t_up
            tmp = c2[j] * t_up
            r1 = np.conj(c1[j]) * tmp + np.conj(s1[j]) * t_d
            dd = -s1[j] * tmp + c1[j] * t_d
            nu = math.hypot(abs(dd), abs(t_lo))
            c, s = dd / nu, t_lo / nu                    # G = [[conj c, conj s], [-s, c]]
            d = (v - r1 * d1[j] - r2 * d2[j]) / nu
            x[j] += (np.conj(c) * tau[j]) * d
            tau[j] = -s * tau[j]
            d2[j], d1[j] = d1[j], d
            c2[j], s2[j], c1[j], s1[j] = c1[j], s1[j], c, s
            its[j] = k
            if abs(tau[j]) <= target:
                live[j] = False
        if not live.any() or beta_new == 0.0:
            break
        v_old, v, beta = v, w / beta_new, beta_new
    return x, its, np.abs(tau), ~live


def solve_shifts(H, b, shifts, reverseGF=False):
    """``[x_j]`` with ``sign*(z_j I - H) x_j = b`` for every shift in ``shifts`` (real or complex), on the device from
    one Lanczos run per group of 8 shifts (``hipeig_minres_shifts``); ``sign = -1`` with ``reverseGF``.  ``b`` is a real
    ``HipVector``; every solution is a ``HipComplexVector``, also for a real shift.  Tolerances and the step limit come
    from ``b.options["linearSystemArgs"]`` (``linear_tol``, ``linear_atol``, ``linearIter``); a shift still live at the
    limit raises ``UserWarning`` as every other solver does.  ``b.last_solve_stats`` = ``{"iterations": [per shift],
    "estimates": [|tau_j|], "products": operator products}`` (the products of the groups add up)."""
    from . import _lib
    from .hip_vector import HipComplexVector, HipCsrOperator, HipVector, _ptr_table
    if not isinstance(H, HipCsrOperator):
        raise TypeError("solve_shifts needs a HipCsrOperator (device-resident CSR)")
    if isinstance(b, HipComplexVector) or not isinstance(b, HipVector):
        raise NotImplementedError("shifted MINRES takes a real HipVector right-hand side (the Lanczos run is real)")
    ctx, n = b.ctx, len(b)
    if ctx.collectives:
        raise NotImplementedError("shifted MINRES runs on whole vectors on one GPU: a context with collectives "
                                  "(row partition, HIPEIG_FORCE_COLLECTIVES) is not supported")
    zs = [complex(z) for z in np.asarray(shifts).reshape(-1)]
    if not zs:
        raise ValueError("solve_shifts needs at least one shift")
    H.honour_reduction_option(b.options)
    o = b.options["linearSystemArgs"]
    rtol, atol, maxiter = float(o["linear_tol"]), float(o.get("linear_atol", 0.0)), int(o["linearIter"])
    out, iterations, estimates, products, failed = [], [], [], 0, False
    for i0 in range(0, len(zs), MAX_SHIFTS_PER_CALL):
        grp = zs[i0:i0 + MAX_SHIFTS_PER_CALL]
        S = len(grp)
        re = [ctx.alloc(n) for _ in grp]
        im = [ctx.alloc(n) for _ in grp]
        rt, keep1 = _ptr_table(re)
        it, keep2 = _ptr_table(im)
        zr = (C.c_double * S)(*[z.real for z in grp])
        zi = (C.c_double * S)(*[z.imag for z in grp])
        info = (C.c_int * S)()
        stats = (C.c_double * (4 * S))()
        _lib.call("hipeig_minres_shifts", ctx.handle, H.handle, -1.0 if reverseGF else 1.0, S, zr, zi, b._buf.ptr,
                  rt, it, rtol, atol, maxiter, info, stats)
        for j in range(S):
            out.append(HipComplexVector(b._new(re[j]), b._new(im[j])))
            iterations.append(int(stats[4 * j]))
            estimates.append(float(stats[4 * j + 1]))
            failed = failed or info[j] != 0
        products += int(stats[2])
    b.last_solve_stats = {"iterations": iterations, "estimates": estimates, "products": products}
    for x in out:
        x.last_solve_stats = b.last_solve_stats
    if failed:
        raise UserWarning("Warning:: Iterative solver is not converged ")
    return out
