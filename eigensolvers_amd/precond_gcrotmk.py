"""NumPy twin of GCROT's diagonal right preconditioner (``csrc/gcrot_precond.hip``).

``scipy.sparse.linalg.gcrotmk(A, b, M=...)`` (SciPy 1.15.3) applies ``M`` on the right - ``_fgmres``: ``z = M v``,
``w = A z`` - so with ``M = diag(minv)`` it is plain ``gcrotmk`` on the composed operator ``v -> A (minv * v)`` followed by
``x = minv * u``, and the residual it tests, ``b - A minv u``, is the true residual ``b - A x``.  The solver itself
(``gcrotmk.py``) is therefore not touched: the device path hands it the composed product and scales its result.  The
reference calls ``gcrotmk`` without ``M`` (numpyVector.py:161), so SciPy itself is the referee
(``tests/test_gcrot_precond_cpu.py``).

``jacobi_inverse_z_host`` states ``hipeig_jacobi_inverse_z`` in the same operations, ``diag_mul_host`` the element of
``hipeig_diag_mul`` / ``hipeig_pair_diag_mul`` to rounding (NumPy has no fused multiply-add, the device element uses one).
"""
import math

import numpy as np


def jacobi_inverse_z_host(diag, z, floor=1e-8):
    """``minv`` of ``M^-1 = diag(1 / (z - d_i))`` kept away from ``d_i == z``: with ``m_i = z - d_i``, ``t_i = |m_i|``,
    ``T = max_j t_j`` and ``g = floor * T``

    - ``1 / m_i`` where ``t_i >= g``,
    - the phase of ``1 / m_i`` at modulus ``1 / g`` where ``0 < t_i < g``,
    - ``1 / g`` where ``t_i == 0``.

    A real ``z`` (``complex(z).imag == 0``) gives a float64 array, a complex one a complex128 array.  The operations and
    their order are the device's: ``mr = rn(zr - d_i)``; real ``z``: ``t = |mr|``, ``1 / mr``, ``copysign(1 / g, mr)``;
    complex ``z``: ``s = rn(rn(mr mr) + rn(zi zi))``, ``t = sqrt(s)``, ``(mr / s, -zi / s)``, ``((mr / t) / g,
    (-zi / t) / g)``.  ``s`` is formed without scaling, so ``|z - d_i|`` is meant to stay within 1e-150 .. 1e150.

    Raises ``ValueError`` ("not finite") where an element would not be finite (a diagonal entry equal to ``z`` with
    ``floor = 0``), where ``diag`` holds a non-finite value and where every ``t_i`` is 0."""
    floor = float(floor)
    if not (0.0 <= floor < math.inf):
        raise ValueError(f"the relative floor must be finite and >= 0, got {floor!r}")
    z = complex(z)
    if not (math.isfinite(z.real) and math.isfinite(z.imag)):
        raise ValueError(f"z must be finite, got {z!r}")
    d = np.asarray(diag, dtype=np.float64)
    cplx = z.imag != 0.0
    mr = z.real - d
    if cplx:
        s = mr * mr + z.imag * z.imag
        t = np.sqrt(s)
    else:
        t = np.abs(mr)
    if t.size == 0:
        return t.astype(np.complex128) if cplx else t
    tmax = math.inf if np.isnan(t).any() else float(t.max())
    tmin = float(np.nanmin(t))
    g = floor * tmax if tmax < math.inf else math.inf
    mmin = max(tmin, g)
    if not (tmax < math.inf) or not (g < math.inf) or not (mmin > 0.0) or not (1.0 / mmin < math.inf):
        raise ValueError(f"Jacobi preconditioner is not finite: max |z - d_i| = {tmax:g}, min = {tmin:g}, relative "
                         f"floor {floor:g} (a diagonal entry equal to z needs a floor > 0)")
    g = np.float64(g)                                    # floor = 0: 1 / g is inf in a class that is then empty
    plain, zero = t >= g, t == 0.0
    low = ~plain & ~zero
    with np.errstate(divide="ignore", invalid="ignore"):
        if cplx:
            re = np.where(plain, mr / s, np.where(low, (mr / t) / g, 1.0 / g))
            im = np.where(plain, -z.imag / s, np.where(low, (-z.imag / t) / g, 0.0))
            return re + 1j * im
        return np.where(plain, 1.0 / mr, np.where(low, np.copysign(1.0 / g, mr), 1.0 / g))


def diag_mul_host(m, x):
    """``m * x`` element by element: what ``hipeig_diag_mul`` / ``hipeig_pair_diag_mul`` compute, to rounding."""
    return np.asarray(m) * np.asarray(x)


def composed_operator(matvec, minv):
    """``v -> A (minv * v)``: the product the unchanged solver is handed; its solution ``u`` gives ``x = minv * u``."""
    return lambda v: matvec(minv * v)
