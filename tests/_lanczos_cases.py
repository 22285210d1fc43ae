"""Operators, references, bounds and small helpers shared by the device tests of the Lanczos filter
(``test_gpu_lanczos_filter.py``, ``test_gpu_lanczos_basis.py``, ``test_gpu_lanczos_prefix.py``).  A plain module, imported
as ``_hiprec`` is: no fixtures, no tests.

Device against twin: the Lanczos recurrence amplifies rounding differences, so the per-(column, shift) step counts may
differ by a few: ``|device - twin| <= max(3, 2 * largest difference observed)``, the rule of ``test_gpu_shifted_minres.py``.
EXPERIMENTS.md R9 holds what has been observed on an MI355X: 0 or +1 over 995 counts, so the bound is max(3, 2 * 1) = 3.

The filtered vectors answer to a derived bound, not a measured one: with ``q_exact = U f(Lambda) U^T b``,
``f(l) = sum_j Re(c_j sign / (z_j - l))``, and every MINRES iterate's residual at most its target,
``||q - q_exact|| <= sum_j |c_j| (1.01 target + 100 eps (|z_j| + ||H||_inf) ||x_j||) / dist(z_j, spectrum)``
(``||x_j||`` from the shifted-MINRES twin)."""
import ctypes as C
import importlib
import math

import numpy as np
import scipy.sparse as sp

from conftest import load_golden
from eigensolvers_amd import feast as pf
from eigensolvers_amd.generators import gapped_csr_host
from eigensolvers_amd.shifted_minres import shifted_minres_host

lf = importlib.import_module("eigensolvers_amd.lanczos_filter")       # the package exports the function of the same name

EPS = np.finfo(float).eps
LO, HI = (1e-5, 1e-7), (1e-10, 1e-12)
STEP_DIFFERENCE_BOUND = 3          # max(3, 2 * largest difference observed), see the module docstring


def contour(nc):
    """(shifts, FEAST's weights -0.5 w r phase) of the nc-node Legendre half contour of [-0.21, 0.21]."""
    gk, wk = pf.quadraturePointsWeights(nc, "legendre", positiveHalf=True)
    zs, ws = [], []
    for g, w in zip(gk, wk):
        theta, z = pf.contour_point(-0.21, 0.21, g)
        zs.append(z)
        ws.append(-0.5 * w * 0.21 * (math.cos(theta) + 1j * math.sin(theta)))
    return zs, ws


Z8, W8 = contour(16)
NEAR, FAR = int(np.argmin([abs(z.imag) for z in Z8])), int(np.argmax([abs(z.imag) for z in Z8]))


def odd_operator():
    """``test_gpu_shifted_minres.py``'s n = 1037 operator, restated (no tile, wave or vector width divides 1037): a random
    sparse symmetric matrix plus a diagonal of the generator's kind - +-(1..3) except 8 rows inside the contour's window."""
    n = 1037
    rng = np.random.default_rng(5)
    R = sp.random(n, n, density=0.01, random_state=rng, format="csr")
    d = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 3.0, n)
    d[::130] = np.linspace(-0.2, 0.2, len(d[::130]))
    return (0.05 * (R + R.T) + sp.diags(d)).tocsr()


def tridiagonal100():
    """The one-workgroup case of ``test_gpu_shifted_minres.py``: diagonal +-(1..1.5), off-diagonal 0.1, no eigenvalue in
    (-0.8, 0.8), so every shift - 0.5 included - keeps 0.3 or more from the spectrum and the twin ends well before n."""
    n = 100
    d = np.concatenate([np.linspace(-1.5, -1.0, n // 2), np.linspace(1.0, 1.5, n - n // 2)])
    return sp.diags([np.full(n - 1, 0.1), d, np.full(n - 1, 0.1)], [-1, 0, 1]).tocsr()


def host_operator(name):
    if name == "n100":
        return sp.csr_matrix(np.array(load_golden("feast_n100.npz")["A"], dtype=float))
    if name == "tri100":
        return tridiagonal100()
    if name == "gapped4000":
        return gapped_csr_host(4000, 32, seed=7)
    return odd_operator()


def build_problems(hip, names, ncols):
    """name -> (host CSR, device operator, host right-hand sides [ncols, n] of unit norm)."""
    out = {}
    for name in names:
        Hh = host_operator(name)
        Hd = hip.HipCsrOperator.generate(4000, 32, seed=7) if name == "gapped4000" else hip.HipCsrOperator.from_scipy(Hh)
        B = np.random.default_rng(9).standard_normal((ncols, Hh.shape[0]))
        out[name] = (Hh, Hd, B / np.linalg.norm(B, axis=1)[:, None])
    return out


_spectra = {}


def spectrum(name, Hh):
    if name not in _spectra:
        _spectra[name] = np.linalg.eigh(Hh.toarray())
    return _spectra[name]


_twin_cache = {}


def twin(key, Hh, b, shifts, rtol, atol, sign, maxiter=4000):
    """(steps, estimates, converged, ||x_j||) of the shifted-MINRES twin for one column, computed once per key and column."""
    key = (key, np.asarray(b, dtype=float).tobytes(), tuple(shifts), rtol, atol, sign, maxiter)
    if key not in _twin_cache:
        x, its, est, conv = shifted_minres_host(lambda v: Hh @ v, b, shifts, rtol, atol, maxiter, sign)
        _twin_cache[key] = (its, est, conv, np.linalg.norm(x, axis=1))
    return _twin_cache[key]


def options(rtol, atol, maxiter=4000):
    return {"linearSystemArgs": {"linearSolver": "lanczos_filter", "linearIter": maxiter, "linear_tol": rtol, "linear_atol": atol}}


def device_columns(hip, B, rtol, atol, maxiter=4000):
    o = options(rtol, atol, maxiter)
    return [hip.HipVector(np.array(b, dtype=float), o) for b in B]


def exact_filter(lam, U, b, zs, ws, sign):
    f = sum((w * sign / (z - lam)).real for z, w in zip(zs, ws))
    return U @ (f * (U.T @ b))


def filter_bound(Hh, lam, zs, ws, xnorms, target):
    hinf = abs(Hh).sum(axis=1).max()
    return sum(abs(w) * (1.01 * target + 100 * EPS * (abs(z) + hinf) * xn) / np.min(np.abs(z - lam))
               for z, w, xn in zip(zs, ws, xnorms))


def residual_bound(Hh, z, x, target):
    hinf = abs(Hh).sum(axis=1).max()
    return 1.01 * target + 100 * EPS * (abs(z) + hinf) * np.linalg.norm(x)


def check_steps(label, device_its, twin_its):
    diff = [int(d) - int(t) for d, t in zip(device_its, twin_its)]
    print(f"STEPS {label} twin={list(map(int, twin_its))} device-twin={diff}")
    assert max(abs(d) for d in diff) <= STEP_DIFFERENCE_BOUND, (label, diff, list(twin_its))
    assert all(d <= math.ceil(1.1 * t) for d, t in zip(device_its, twin_its)), (label, diff)


def check_filter(label, name, Hh, b, q, zs, ws, xnorms, target, sign):
    lam, U = spectrum(name, Hh)
    err = np.linalg.norm(q - exact_filter(lam, U, b, zs, ws, sign))
    bound = filter_bound(Hh, lam, zs, ws, xnorms, target)
    print(f"FILTER {label} error {err:.3e} bound {bound:.3e} used {err / bound:.3f}")
    assert np.isfinite(q).all() and err <= bound, (label, err, bound)


def same_scalars(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


def single_solution_tables(run, j, sign=1.0):
    """NC = 2 tables (Re y, Im y) of shift j's MINRES iterate, per column."""
    G = []
    for sc in run.scalars:
        y = lf.minres_coefficients(sc.alphas, sc.betas, Z8[j], sc.iterations[j], sign)
        G.append(np.stack([y.real, y.imag], axis=1))
    return G


def arrays(vs):
    return [v.array for v in vs]


def all_equal(xs, ys):
    return len(xs) == len(ys) and all(np.array_equal(x, y) for x, y in zip(xs, ys))


class block_variant:
    def __init__(self, Hd, variant):
        self.Hd, self.variant = Hd, variant

    def __enter__(self):
        self.Hd.set_block_variant(self.variant)

    def __exit__(self, *exc):
        self.Hd.set_block_variant(0)


def slot_bytes(n, k):
    """Bytes of one slot of a k-column group: the interleaved block, padded to 32 doubles."""
    K = 4 if k <= 4 else 8
    return ((n * K + 31) // 32 * 32) * 8


def reusable_bytes(ctx):
    """Bytes of released basis segments the context would hand out again."""
    from eigensolvers_amd import _lib
    info = (C.c_int64 * 8)()
    _lib.call("hipeig_lanczos_basis_info", ctx.handle, None, info)
    return info[5]
