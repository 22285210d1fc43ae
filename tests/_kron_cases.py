"""Shapes, operands, longdouble reference and row bound of the Kronecker-sum operator (a plain module: no fixtures, no tests).

    H = sum_d I (x) T_d (x) I + diag(V),   vector index in C order, last mode fastest.

``kron_apply_ld`` applies the factors mode by mode with ``np.tensordot`` in ``np.longdouble`` and returns, with the product,
the row sums ``S_r = |V_r x_r| + sum_d sum_k |T_d[i_d, k]| |x_..k..|`` the bound is stated in.

The bound.  A row of the device product is one sum of ``sum_d n_d + 1`` terms (the rounded product ``V_r x_r`` and one
term per factor entry), each entering once, in an order that the dims fix (csrc/kron_device.h).  Whatever that order, a
term passes at most ``m = sum_d n_d + D + 2`` roundings (its own product where it is not fused, and at most one add per
other term; D + 2 pays for the hand-over from launch to launch and the epilogue), so with ``u = 2^-53``

    |y_r - (H x)_r| <= gamma_m S_r,      gamma_m = m u / (1 - m u).

The longdouble reference itself is off by at most ``gamma_m`` at ``u = 2^-64``: 2^-11 of the bound.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble

# the smallest shapes at which a tile, a mask or a stride can go wrong: one mode; exactly one MFMA tile; a factor one past a
# tile over a short stride and the reverse; odd sizes in three modes; four modes with strides 60, 20, 5, 1; factors over two
# LDS row groups (33) with strides that are no multiple of 4 (33) or of 64 (20); singleton modes; the solver fixture's grid
SHAPES = [(5,), (16, 16), (17, 3), (3, 17), (7, 5, 9), (2, 3, 4, 5), (33, 20), (20, 33), (1, 8, 1, 5), (13, 10, 7)]


def gamma(m):
    return m * U / (1.0 - m * U)


def bound_terms(dims):
    return sum(dims) + len(dims) + 2


def size(dims):
    return int(np.prod(dims, dtype=np.int64))


def factors_for(dims, seed, symmetric=True, integer=False):
    rng = np.random.default_rng([seed, len(dims)] + list(dims))
    out = []
    for n in dims:
        T = rng.integers(-8, 9, (n, n)).astype(np.float64) if integer else rng.standard_normal((n, n)) * np.exp(rng.uniform(-2, 2, (n, n)))
        if symmetric:
            T = np.triu(T) + np.triu(T, 1).T
        out.append(np.ascontiguousarray(T))
    return out


def diag_for(dims, seed, integer=False):
    rng = np.random.default_rng([seed, 77] + list(dims))
    if integer:
        return rng.integers(-8, 9, dims).astype(np.float64)
    return rng.standard_normal(dims) * np.exp(rng.uniform(-2, 2, dims))


def operand(n, seed, integer=False):
    """standard_normal * exp(U(-2, 2)) element by element, as the operands of ``_product_cases``; or integers in [-8, 8]."""
    rng = np.random.default_rng([seed, 3, n])
    if integer:
        return rng.integers(-8, 9, n).astype(np.float64)
    return rng.standard_normal(n) * np.exp(rng.uniform(-2, 2, n))


def kron_apply_ld(factors, V, x):
    """``(H x, S)`` in longdouble, flat; ``V`` may be ``None``."""
    dims = tuple(T.shape[0] for T in factors)
    X = np.asarray(x, dtype=LD).reshape(dims)
    Xa = np.abs(X)
    y = np.zeros(dims, dtype=LD)
    S = np.zeros(dims, dtype=LD)
    if V is not None:
        Vl = np.asarray(V, dtype=LD).reshape(dims)
        y += Vl * X
        S += np.abs(Vl) * Xa
    for d, T in enumerate(factors):
        Tl = np.asarray(T, dtype=LD)
        y += np.moveaxis(np.tensordot(Tl, X, axes=([1], [d])), 0, d)
        S += np.moveaxis(np.tensordot(np.abs(Tl), Xa, axes=([1], [d])), 0, d)
    return y.reshape(-1), S.reshape(-1)


def kron_apply_f64(factors, V, x):
    """The same product in float64, mode by mode: a second host rounding of ``H x`` beside the CSR product."""
    dims = tuple(T.shape[0] for T in factors)
    X = np.asarray(x, dtype=np.float64).reshape(dims)
    y = np.zeros(dims) if V is None else np.asarray(V).reshape(dims) * X
    for d, T in enumerate(factors):
        y = y + np.moveaxis(np.tensordot(T, X, axes=([1], [d])), 0, d)
    return y.reshape(-1)


def product_bound(dims, S):
    return (gamma(bound_terms(dims)) * S).astype(np.float64) + 1e-300


def shifted_bound(dims, S, sigma, x):
    """``sign (sigma x - H x)`` as ``rn(rn(sigma x) - sum)``: the shift term is rounded twice, the sum once more."""
    m = bound_terms(dims)
    return (gamma(m + 1) * S + 2.02 * U * abs(sigma) * np.abs(x)).astype(np.float64) + 1e-300


def pair_bound(dims, S, zr, zi, x, xo):
    """One half of ``sign (z x - H x)`` as the real shifted sweep followed by the two-stream update with the other half
    ``xo``: the real shift term passes three roundings, the sum two more, the imaginary term two."""
    m = bound_terms(dims)
    return (gamma(m + 2) * S + 3.03 * U * abs(zr) * np.abs(x) + 2.02 * U * abs(zi) * np.abs(xo)).astype(np.float64) + 1e-300


def within(got, ref, bound):
    """``|got - ref| <= bound`` row by row; returns the largest ratio for the record."""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    ratio = float(np.max(err / bound))
    bad = ~(err <= bound)
    assert not bad.any(), f"{int(bad.sum())} rows over the bound, worst ratio {ratio:.3f} at row {int(np.argmax(err / bound))}"
    return ratio
