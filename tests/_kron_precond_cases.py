"""Problems, references and bounds of the separable preconditioner of the Kronecker-sum operator
(``test_kron_precond_cpu.py``, ``test_gpu_kron_precond.py``).  A plain module: no fixtures, no tests, no device.

    M^-1 = Q S Q^T,  Q = Q_1 (x) ... (x) Q_D,  S = diag(sinv)

One mode.  An element of a transform is a sum of ``n_d`` products that each enter once, in an order the dims fix
(csrc/kron_precond_device.h): ``n_d`` products and ``n_d`` adds at most, the derivation of ``_kron_cases`` for a single
mode with nothing handed over from a launch before, so

    |z_i - (Q x)_i| <= gamma_{n_d + 2} sum_k |Q[i, k]| |x_k|.

The whole apply.  Each of the ``2 D`` steps errs by at most ``gamma_{n_d + 2} |Q_d| |x|`` row by row, in the 2-norm by
``gamma_{n_d + 2} sqrt(n_d) ||x||`` since ``|| |Q_d| ||_2 <= || Q_d ||_F = sqrt(n_d)``; the exact maps keep the norm up to
the one scaling, by ``s_max`` at most, which also rounds once (``u``, twice with the margin for its own input).  To first
order in ``u`` - the factor 1.01 pays for the rest, and for the stored ``Q`` being orthogonal to rounding only -

    ||z - M^-1 r||_2 <= 1.01 s_max ||r||_2 (2 sum_d gamma_{n_d + 2} sqrt(n_d) + 2 u).
"""
import numpy as np

import _kron_cases as kc
from eigensolvers_amd.generators import coupled_oscillator_grid, guess_vector
from eigensolvers_amd.hip_vector import HipKronSumOperator
from eigensolvers_amd.precond_minres import (minres_precond_host, separable_apply_host, separable_basis_host,
                                             separable_fit_host, separable_scale_host)

FLOOR = 1e-8
GRID = (13, 10, 7)
# (dims, rtol) of the solves: the grids of test_gpu_kron's MINRES cases at both tolerances, and (33, 20) - factors over two
# LDS row groups - at 1e-6
SOLVE_CASES = [((13, 10, 7), 1e-6), ((13, 10, 7), 1e-10), ((17, 3), 1e-6), ((17, 3), 1e-10), ((2, 3, 4, 5), 1e-6),
               ((2, 3, 4, 5), 1e-10), ((33, 20), 1e-6)]

_problems = {}
_twins = {}


def _ranges(dims, solve):
    """The ranges of ``test_gpu_kron._problem``.  (17, 3) is N = 51, where MINRES at rtol 1e-10 runs close to the exhaustion of
    the Krylov space; ``_problem`` took for its second mode the first of (-4.5, 4.5), (-4, 4), (-3, 3) at which the count of
    the PLAIN solve is posed at both tolerances, which is the last.  The count of the preconditioned solve is not posed
    there (22 iterations with float64 products and applies, 21 with longdouble ones: ``test1`` at iteration 21 is 1.2e-10
    and 5.7e-11), so the problems of the device solves (``solve=True``) take the first of the same three at which
    ``count_is_posed`` accepts both tolerances, by the same rule: (-4.5, 4.5), 11 and 17 iterations in both roundings."""
    D = len(dims)
    if dims == GRID:
        return [(-5, 5), (-4.5, 4.5), (-4, 4)]
    if dims == (17, 3) and not solve:
        return [(-5, 5), (-3, 3)]
    return [(-5, 5), (-4.5, 4.5), (-4, 4), (-3.5, 3.5)][:D]


def problem(dims, solve=False):
    """The oscillator grid of ``test_gpu_kron._problem`` on ``dims`` (its ranges and frequencies; ``solve``: see ``_ranges``),
    host only: a dict with the factors, V, the explicit matrix, the spectrum, sigma between the 4th and 5th level, the unit
    right-hand side and the parts of the preconditioner (potentials, bases, eigenvalues, sinv).  Built once; the arrays are
    read-only."""
    dims = tuple(dims)
    ranges = _ranges(dims, solve)
    key = (dims, tuple(ranges))
    if key not in _problems:
        D = len(dims)
        factors, V = coupled_oscillator_grid(dims, ranges, [1.0, 1.3, 1.7, 2.1][:D])
        Hs = HipKronSumOperator.explicit_matrix(factors, V)
        lam = np.linalg.eigvalsh(Hs.toarray())
        sigma = float(0.513 * lam[3] + 0.487 * lam[4])
        b = guess_vector(kc.size(dims), 1)
        b = b / np.linalg.norm(b)
        potentials = separable_fit_host(V, dims)
        bases, eigenvalues = separable_basis_host(factors, potentials)
        sinv = separable_scale_host(eigenvalues, sigma, FLOOR)
        for a in [b, sinv, lam] + list(bases) + list(eigenvalues):
            a.setflags(write=False)
        _problems[key] = dict(dims=dims, factors=factors, V=V, Hs=Hs, lam=lam, sigma=sigma, b=b, potentials=potentials,
                              bases=bases, eigenvalues=eigenvalues, sinv=sinv)
    return _problems[key]


def shifted(p):
    Hs, sigma = p["Hs"], p["sigma"]
    return lambda v: sigma * v - Hs @ v


def apply_f64(p):
    return lambda r: separable_apply_host(p["bases"], p["sinv"], r)


def apply_ld(bases, sinv, r):
    """The apply in longdouble from the same stored ``Q`` and ``sinv``."""
    return separable_apply_host(bases, np.asarray(sinv, dtype=kc.LD), np.asarray(r, dtype=kc.LD))


def twin(dims, rtol, rounding="f64", solve=False):
    """``minres_precond_host`` on ``problem(dims, solve)``: (x, info, itn, istop, trace), once per key.  ``"f64"``: float64
    products (the CSR matrix) and applies; ``"ld"``: longdouble products and applies, each rounded to float64 - a second
    host rounding of the same recurrence."""
    key = (tuple(dims), rtol, rounding, bool(solve))
    if key not in _twins:
        p = problem(dims, solve)
        if rounding == "f64":
            mv, ap = shifted(p), apply_f64(p)
        else:
            sigma = kc.LD(p["sigma"])
            mv = lambda v: np.asarray(sigma * np.asarray(v, dtype=kc.LD) - kc.kron_apply_ld(p["factors"], p["V"], v)[0], dtype=np.float64)
            ap = lambda r: np.asarray(apply_ld(p["bases"], p["sinv"], r), dtype=np.float64)
        trace = []
        x, info, itn, istop = minres_precond_host(mv, p["b"], ap, rtol=rtol, maxiter=4000, trace=trace)
        x.setflags(write=False)
        _twins[key] = (x, info, itn, istop, trace)
    return _twins[key]


def count_is_posed(dims, rtol):
    """Of the problems of the device solves, in the manner of ``test_gpu_kron._count_is_posed``: the twin's count is a property
    of the problem, not of the rounding of its products and applies, where the two host roundings stop at the same iteration
    with ``istop == 1`` AND ``test1`` is further from ``rtol`` than the two are from each other, at the stop (below) and one
    before (above)."""
    a, b = twin(dims, rtol, "f64", solve=True), twin(dims, rtol, "ld", solve=True)
    if a[2:4] != b[2:4] or a[3] != 1:
        return False
    ta, tb = a[4], b[4]
    stop, prev = (ta[-1]["test1"], tb[-1]["test1"]), (ta[-2]["test1"], tb[-2]["test1"])
    return max(stop) + abs(stop[0] - stop[1]) <= rtol and min(prev) - abs(prev[0] - prev[1]) > rtol


def mode_apply_ld(Q, x, dims, d, transpose):
    """``((I (x) Q (x) I) x, S)`` for mode ``d`` in longdouble, flat, ``S = (I (x) |Q| (x) I) |x|``; ``transpose``: ``Q^T``."""
    Ql = np.asarray(Q.T if transpose else Q, dtype=kc.LD)
    X = np.asarray(x, dtype=kc.LD).reshape(dims)
    z = np.moveaxis(np.tensordot(Ql, X, axes=([1], [d])), 0, d)
    S = np.moveaxis(np.tensordot(np.abs(Ql), np.abs(X), axes=([1], [d])), 0, d)
    return z.reshape(-1), S.reshape(-1)


def mode_bound(nd, S):
    return (kc.gamma(nd + 2) * S).astype(np.float64) + 1e-300


def apply_bound(dims, smax, rnorm):
    """The 2-norm bound of the whole apply (module docstring)."""
    return 1.01 * smax * rnorm * (2.0 * sum(kc.gamma(n + 2) * np.sqrt(n) for n in dims) + 2.0 * kc.U)


def kernel_forms(dims):
    strides = [kc.size(dims[d + 1:]) for d in range(len(dims))]
    return ["plain" if nd == 1 else "mfma-last" if s == 1 else "mfma" if s >= 16 else "plain" for nd, s in zip(dims, strides)]
