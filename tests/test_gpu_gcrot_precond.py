"""GCROT's diagonal right preconditioner on the GPU (``linearSystemArgs["gcrotPreconditioner"] = "jacobi"``): the element
``y = m x`` and ``minv`` against extended precision with their derived bounds, the block products that scale while they
pack against the unscaled products on the scaled operand (within the product's own row bound, and bit for bit on the
row-owner kernel), the solves through every path against SciPy's ``gcrotmk(A, b, M=...)``, and FEAST / block Lanczos end
to end with the key off and on.  Cases, references and bounds: ``_gcrot_precond_cases.py``, ``_product_cases.py``."""
import warnings

import numpy as np
import pytest
import scipy.linalg as la
import scipy.sparse as sp

import _gcrot_precond_cases as gc
import _hiprec as hp
import _product_cases as pc
from eigensolvers_amd import _lib, jacobi_inverse_z_host
from eigensolvers_amd.precond_minres import csr_diagonal_host

pytestmark = pytest.mark.gpu

SIGNS = (1.0, -1.0)


def _up(hip, a):
    return hip.HipVector(np.ascontiguousarray(a, dtype=np.float64))._buf


def _down(hip, buf):
    return hip.HipVector(buf).array


# ---------------------------------------------------------------- 4. the element y = m x
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4001])
def test_diag_mul_elements_against_extended_precision(hip, n):
    """hipeig_diag_mul and hipeig_pair_diag_mul (complex and real m), out of place and in place, operands and scalings
    spanning orders of magnitude: every element within the bound of ``DiagMul``'s own operations."""
    ctx = hip.HipContext.default()
    xs = pc.complex_operands(n, 3)
    ms = gc.scaling_vectors(n, 3)
    worst = 0.0
    for (xr, xi), (mr, mi) in zip(xs, ms):
        for in_place in (False, True):
            # real element
            yr_ref, _, br, _ = gc.diag_mul_reference(mr, None, xr, None)
            x, m_re = _up(hip, xr), _up(hip, mr)
            y = x if in_place else ctx.alloc(n)
            _lib.call("hipeig_diag_mul", ctx.handle, n, m_re.ptr, x.ptr, y.ptr)
            worst = max(worst, pc.error_ratio(_down(hip, y), yr_ref, br + 1e-300))
            if not in_place:
                np.testing.assert_array_equal(_down(hip, x), xr)
            # complex element, complex or real m
            yr_ref, yi_ref, br, bi = gc.diag_mul_reference(mr, mi, xr, xi)
            a, b = _up(hip, xr), _up(hip, xi)
            m_im = None if mi is None else _up(hip, mi)
            yr, yi = (a, b) if in_place else (ctx.alloc(n), ctx.alloc(n))
            _lib.call("hipeig_pair_diag_mul", ctx.handle, n, m_re.ptr, None if m_im is None else m_im.ptr,
                      a.ptr, b.ptr, yr.ptr, yi.ptr)
            worst = max(worst, pc.error_ratio(_down(hip, yr), yr_ref, br + 1e-300), pc.error_ratio(_down(hip, yi), yi_ref, bi + 1e-300))
    print(f"\ndiag_mul n = {n}: max error / bound {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------- 5. minv
def _device_minv(hip, d, z, floor, sentinel=None):
    """hipeig_jacobi_inverse_z on a host diagonal: complex128 / float64 array; ``sentinel``: what the outputs hold before."""
    ctx = hip.HipContext.default()
    n, z = len(d), complex(z)
    re = _up(hip, np.full(n, sentinel if sentinel is not None else 0.0))
    im = _up(hip, np.full(n, sentinel if sentinel is not None else 0.0)) if z.imag != 0 or sentinel is not None else None
    dd = _up(hip, d)
    try:
        _lib.call("hipeig_jacobi_inverse_z", ctx.handle, n, dd.ptr, z.real, z.imag, float(floor), re.ptr,
                  None if im is None else im.ptr)
    except _lib.HipEigError as exc:
        return exc, _down(hip, re), None if im is None else _down(hip, im)
    if z.imag != 0:
        return None, _down(hip, re) + 1j * _down(hip, im), None
    return None, _down(hip, re), None if im is None else _down(hip, im)


@pytest.mark.parametrize("z", [0.02, 0.02 + 1e-12j, 0.02 + 0.05j, 0.05])
def test_jacobi_inverse_z_stays_within_the_twin_s_bound(hip, z):
    """On the exact-hit operator (b), through HipCsrOperator.jacobi_inverse_z (the device diagonal): every element within
    the bound the twin's operations give of the extended-precision value; (None for the imaginary half of a real z)."""
    Hh, hit, zero = gc.operator_b()
    H = hip.HipCsrOperator.from_scipy(Hh)
    d = csr_diagonal_host(Hh)
    np.testing.assert_array_equal(_down(hip, H.diagonal()), d)
    re, im = H.jacobi_inverse_z(z, gc.FLOOR)
    assert (im is None) == (complex(z).imag == 0)
    got = _down(hip, re) if im is None else _down(hip, re) + 1j * _down(hip, im)
    ratio = gc.minv_error_ratio(got, d, z, gc.FLOOR)
    twin = jacobi_inverse_z_host(d, z, gc.FLOOR)
    print(f"\nminv device, z = {z}: max error / bound {ratio:.3f}; elements that differ from the twin: {int(np.sum(got != twin))}")
    assert ratio <= 1.0
    assert H.jacobi_inverse_z(z, gc.FLOOR)[0] is re                       # cached
    kind = gc.minv_reference(d, z, gc.FLOOR)[3]
    assert kind[hit] == {0.02: 2, 0.02 + 1e-12j: 1}.get(z, 0)


def test_jacobi_inverse_z_classes_refusals_and_cache(hip):
    """The small diagonal of the CPU test (every class, real and complex z) and the refusals: exactly where the twin
    refuses, with the "not finite" error, the output buffers left as they were."""
    d = np.array([1.0, -3.0, 0.02, 0.02 + 1e-11, 0.02 - 1e-11, 0.5])
    for z in (0.02, 0.02 + 1e-12j):
        exc, got, _ = _device_minv(hip, d, z, 1e-8)
        assert exc is None and gc.minv_error_ratio(got, d, z, 1e-8) <= 1.0
    exc, got, im = _device_minv(hip, d, 0.02, 1e-8, sentinel=7.0)           # a real z with an imaginary half given: zeros
    assert exc is None and np.all(im == 0.0) and gc.minv_error_ratio(got, d, 0.02, 1e-8) <= 1.0
    refused = [(d, 0.02, 0.0), (d, 0.02 + 0j, 0.0), (np.array([1.0, np.nan]), 0.02, 1e-8), (np.array([1.0, np.nan]), 0.02 + 0.05j, 1e-8),
               (np.array([1.0, np.inf]), 0.02 + 0.05j, 1e-8), (np.array([0.02, 0.02]), 0.02, 1e-8)]
    for dd, z, floor in refused:
        with pytest.raises(ValueError, match="not finite"):
            jacobi_inverse_z_host(dd, z, floor)
        exc, re, im = _device_minv(hip, dd, z, floor, sentinel=7.0)
        assert exc is not None and "not finite" in str(exc), (dd, z, floor)
        assert np.all(re == 7.0) and np.all(im == 7.0)                   # nothing written
    for dd, z, floor in ((d, 0.1, 0.0), (d, 0.02 + 1e-12j, 0.0)):           # the twin accepts: so does the device
        assert np.all(np.isfinite(jacobi_inverse_z_host(dd, z, floor)))
        exc, got, _ = _device_minv(hip, dd, z, floor)
        assert exc is None and gc.minv_error_ratio(got, dd, z, floor) <= 1.0
    # through the operator: ValueError, and the bounded cache
    Hh, _, _ = gc.operator_b()
    H = hip.HipCsrOperator.from_scipy(Hh)
    with pytest.raises(ValueError, match="not finite"):
        H.jacobi_inverse_z(0.02, 0.0)
    first = H.jacobi_inverse_z(0.3 + 0.1j)
    for k in range(H.JACOBI_Z_CACHE):
        H.jacobi_inverse_z(0.3 + 0.1j * (k + 2))
    assert len(H._jacobi_z) == H.JACOBI_Z_CACHE and H.jacobi_inverse_z(0.3 + 0.1j) is not first


# ---------------------------------------------------------------- 6. the block products that scale while they pack
class _Scaled:
    """A whole operator as CSR arrays, 9 complex operands, a scaling vector per operand, and - once per operand - the
    scaled operand as the device's own element produced it, with the half-products of the reference on it."""

    def __init__(self, hip, csr, n):
        self.csr, self.n = csr, n
        self.X = pc.complex_operands(n, 9)
        self.M = gc.scaling_vectors(n, 9)
        self.H = hip.HipCsrOperator.from_csr_arrays(*csr, n, 0)
        self.Xd = [(_up(hip, a), _up(hip, b)) for a, b in self.X]
        self.Md = [(_up(hip, a), None if b is None else _up(hip, b)) for a, b in self.M]
        self.Td, self.T, self.products = [], [], []
        for x, m in zip(self.Xd, self.Md):
            t = self.H.diag_mul(m, x)
            th = (_down(hip, t[0]), _down(hip, t[1]))
            self.Td.append(t); self.T.append(th)
            self.products.append(pc.half_products(*csr, *th))
        # real operands, one real scaling for all of them
        self.mreal = (self.Md[1][0], None)
        self.Rd = [x[0] for x in self.Xd]
        self.RTd = [self.H.diag_mul(self.mreal, x) for x in self.Rd]
        self.RT = [_down(hip, t) for t in self.RTd]
        self.rproducts = [pc.half_products(*csr, t, np.zeros(n)) for t in self.RT]

    def check(self, p, z, sign, y, hipmod, real=False):
        t = (self.RT[p], np.zeros(self.n)) if real else self.T[p]
        args = (*self.csr, *t, z, sign, 0, self.rproducts[p] if real else self.products[p])
        ref_r, ref_i = pc.shift_pair_reference(*args)
        br, bi = pc.shift_pair_bound(*args)
        if real:
            return pc.error_ratio(_down(hipmod, y), ref_r, br)
        return max(pc.error_ratio(_down(hipmod, y[0]), ref_r, br), pc.error_ratio(_down(hipmod, y[1]), ref_i, bi))


_SCALED = {}


def _scaled_case(hip, name):
    """Built once per operator, before any layout knob matters (the element kernels do not read them)."""
    if name not in _SCALED:
        if name == "ragged":
            _SCALED[name] = _Scaled(hip, pc.ragged_csr(3001, 11, duplicates=True), 3001)
        else:
            n = 64 * hip.HipContext.default().device_info()["cus"] + 3001
            A = pc.edge_matrix(n, seed=3)
            _SCALED[name] = _Scaled(hip, (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.copy()), n)
    return _SCALED[name]


def _fresh_operator(hip, case, monkeypatch, variant, width):
    """The layout geometry is read when a layout is first built: a new operator after the knobs are set."""
    monkeypatch.setenv("HIPEIG_BCOO_WBITS", "9")
    monkeypatch.setenv("HIPEIG_BCOO_RW", "37")
    monkeypatch.setenv("HIPEIG_PAIR_BLOCK_WIDTH", width)
    H = hip.HipCsrOperator.from_csr_arrays(*case.csr, case.n, 0)
    H.set_block_variant(variant)
    return H


@pytest.mark.parametrize("width", ["4", "8"])
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("name", ["ragged", "edge"])
def test_scaled_pair_products(hip, monkeypatch, name, variant, width):
    """hipeig_spmm_shift_pairs_zm: 1, 2, 3, 4, 5, 8, 9 operands (passes of width 4, 8, 16, a remainder chunk, the single
    fallback), both signs, a shift AND a scaling per operand that differ by orders between neighbours, some scalings real.
    (i) within the unscaled product's row bound evaluated at the scaled operand hipeig_pair_diag_mul writes; (ii) on the
    row-owner kernel bit for bit hipeig_spmm_shift_pairs_z on that operand."""
    case = _scaled_case(hip, name)
    H = _fresh_operator(hip, case, monkeypatch, variant, width)
    assert any(m[1] is None for m in case.Md) and any(m[1] is not None for m in case.Md)
    worst = 0.0
    for npairs in (1, 2, 3, 4, 5, 8, 9):
        for sign in SIGNS:
            zs = [pc.SHIFTS[(p + npairs) % len(pc.SHIFTS)] for p in range(npairs)]
            ys = H.apply_shifted_pairs_m(zs, case.Md[:npairs], case.Xd[:npairs], reverse=sign < 0)
            if variant == 1:
                plain = H.apply_shifted_pairs(zs, case.Td[:npairs], reverse=sign < 0)
            for p in range(npairs):
                r = case.check(p, zs[p], sign, ys[p], hip)
                assert r <= 1.0, f"{name} variant {variant} width {width} npairs {npairs} sign {sign:+.0f} operand {p}: error / bound {r:.3g}"
                worst = max(worst, r)
                if variant == 1:
                    for half in (0, 1):
                        np.testing.assert_array_equal(_down(hip, ys[p][half]), _down(hip, plain[p][half]))
            if npairs > 1:
                assert H.block_info()["variant"] == ("row-owner" if variant == 1 else "column-window-blocked")
    for a, b in zip(case.Xd, case.X):                                     # the operands were only read
        np.testing.assert_array_equal(_down(hip, a[0]), b[0])
    print(f"\nscaled pair products, {name} variant {variant} width {width}: max error / bound {worst:.3f}")


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("name", ["ragged", "edge"])
def test_scaled_real_products(hip, monkeypatch, name, variant):
    """hipeig_spmm_shift_m for k = 1, 3, 4, 5, 8, 9 real operands and one real scaling: the same two checks against
    hipeig_spmm_shift on hipeig_diag_mul's output."""
    case = _scaled_case(hip, name)
    H = _fresh_operator(hip, case, monkeypatch, variant, "4")
    worst = 0.0
    for k in (1, 3, 4, 5, 8, 9):
        for sign in SIGNS:
            sigma = (0.37, 25.0, -0.07, 1e-3)[(k + (sign < 0)) % 4]
            ys = H.apply_shifted_block_m(sigma, case.mreal, case.Rd[:k], reverse=sign < 0)
            if variant == 1:
                plain = H.apply_shifted_block(sigma, case.RTd[:k], reverse=sign < 0)
            for p in range(k):
                r = case.check(p, sigma, sign, ys[p], hip, real=True)
                assert r <= 1.0, f"{name} variant {variant} k {k} sign {sign:+.0f} operand {p}: error / bound {r:.3g}"
                worst = max(worst, r)
                if variant == 1:
                    np.testing.assert_array_equal(_down(hip, ys[p]), _down(hip, plain[p]))
            assert H.block_info()["variant"] == ("row-owner" if variant == 1 else "column-window-blocked")
    print(f"\nscaled real products, {name} variant {variant}: max error / bound {worst:.3f}")


def test_scaled_products_refuse_what_they_do_not_take(hip):
    case = _scaled_case(hip, "ragged")
    slab = hip.HipCsrOperator.from_scipy(sp.identity(100, format="csr"), 10, 90)
    x = _up(hip, np.ones(100))
    with pytest.raises(_lib.HipEigError, match="whole square operator"):
        slab.apply_shifted_block_m(0.5, (x, None), [x])
    with pytest.raises(_lib.HipEigError, match="whole square operator"):
        slab.apply_shifted_pairs_m([0.5j], [(x, None)], [(x, x)])
    with pytest.raises(ValueError):
        case.H.apply_shifted_pairs_m([0.5j] * 2, case.Md[:1], case.Xd[:1])


# ---------------------------------------------------------------- 7. the solves
def _options(key, maxiter=1000, **extra):
    lsa = {"linearSolver": "gcrotmk", "linearIter": maxiter, "linear_tol": gc.RTOL, "linear_atol": gc.ATOL}
    if key:
        lsa["gcrotPreconditioner"] = "jacobi"
    o = {"linearSystemArgs": lsa}
    o.update(extra)
    return o


_OPS = {}


def _csr(name):
    if name not in _OPS:
        A = sp.csr_matrix(gc.operator(name))
        _OPS[name] = (A, (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.copy()), csr_diagonal_host(A), abs(A).tocsr())
    return _OPS[name]


def _residual_check(name, z, sign, x, b, label):
    """True residual in longdouble against max(atol, rtol |b|) plus the 2-norm of the row bounds of the residual product
    the solver itself evaluated (at x, the scaled iterate) and of the final scaling's element bound pushed through
    |z| + |H|; (n + 4) u covers the solver's own norm and subtraction."""
    A, csr, d, Aabs = _csr(name)
    x = np.asarray(x, dtype=np.complex128)
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    products = pc.half_products(*csr, xr, xi)
    yr, yi = pc.shift_pair_reference(*csr, xr, xi, z, sign, 0, products)
    br, bi = pc.shift_pair_bound(*csr, xr, xi, z, sign, 0, products)
    b = np.asarray(b, dtype=np.complex128)
    res = float(np.sqrt(hp.nrm2(b.real.astype(hp.LD) - yr) ** 2 + hp.nrm2(b.imag.astype(hp.LD) - yi) ** 2))
    minv = jacobi_inverse_z_host(d, z, gc.FLOOR)
    u = x / minv
    mi = None if not np.iscomplexobj(minv) else minv.imag
    _, _, er, ei = gc.diag_mul_reference(minv.real, mi, u.real, u.imag)
    e = np.hypot(er, ei)
    pushed = abs(complex(z)) * e + Aabs @ e
    tol = max(gc.ATOL, gc.RTOL * float(np.linalg.norm(b)))
    allowed = tol * (1 + (len(b) + 4) * gc.U) + float(np.sqrt(np.sum(br ** 2) + np.sum(bi ** 2))) + float(np.linalg.norm(pushed))
    print(f"{label}: true residual {res:.3e}, allowed {allowed:.3e} (tolerance {tol:.1e})")
    assert res <= allowed, label
    return res


def _against_scipy(name, z, j, x, stats, label, sign=1.0, complex_rhs=False):
    xs, info, count = gc.scipy_solve(name, z, j, sign, complex_rhs)
    its = stats["iterations"]
    rel = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print(f"{label}: {its} products, SciPy with M {count}; |x - x_scipy| / |x_scipy| = {rel:.2e}")
    assert info == 0 and stats["preconditioner"] == "jacobi"
    assert abs(its - count) <= max(3, count // 20), label
    assert rel <= 1e-6, label
    b = gc.rhs(j) * (1 + 0.5j) / abs(1 + 0.5j) if complex_rhs else gc.rhs(j)
    _residual_check(name, z, sign, x, b, label)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_single_solves_follow_scipy_with_M(hip, name):
    """HipVector.solve with the key: the three shifts (complex, complex on the axis, real), reverseGF once and a complex
    right-hand side once, against SciPy's gcrotmk with M."""
    H = hip.HipCsrOperator.from_scipy(gc.operator(name))
    print()
    for z in gc.SHIFTS:
        b = hip.HipVector(gc.rhs(0).copy(), _options(True))
        x = hip.HipVector.solve(H, b, z)
        assert isinstance(x, hip.HipComplexVector) == isinstance(z, complex)
        assert b.last_solve_stats == x.last_solve_stats and "outer" in x.last_solve_stats
        _against_scipy(name, z, 0, x.array, x.last_solve_stats, f"({name}) single z = {z!r}")
    b = hip.HipVector(gc.rhs(1).copy(), _options(True))
    x = hip.HipVector.solve(H, b, gc.Z_COMPLEX, reverseGF=True)
    _against_scipy(name, gc.Z_COMPLEX, 1, x.array, x.last_solve_stats, f"({name}) single reverseGF", sign=-1.0)
    bc = hip.HipVector(gc.rhs(1) * (1 + 0.5j) / abs(1 + 0.5j), _options(True))
    assert isinstance(bc, hip.HipComplexVector)
    x = hip.HipVector.solve(H, bc, gc.Z_REAL)
    _against_scipy(name, gc.Z_REAL, 1, x.array, x.last_solve_stats, f"({name}) single complex right-hand side", complex_rhs=True)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_lock_step_and_pooled_solves_follow_scipy_with_M(hip, name):
    """solveBlock with the key: one contour point and 5 right-hand sides; the pool with 6 right-hand sides x 2 points,
    width 4 forced; the real block with 4 right-hand sides."""
    H = hip.HipCsrOperator.from_scipy(gc.operator(name))
    o = _options(True, contourPoolWidth=4)
    print()
    bs = [hip.HipVector(gc.rhs(j).copy(), o) for j in range(6)]
    xs = hip.HipVector.solveBlock(H, bs[:5], gc.Z_COMPLEX)
    for j, x in enumerate(xs):
        _against_scipy(name, gc.Z_COMPLEX, j, x.array, x.last_solve_stats, f"({name}) one point, rhs {j}")
    points = (gc.Z_COMPLEX, gc.Z_ON_AXIS)
    jobs = [(j, z) for z in points for j in range(6)]
    pool = {}
    xs = hip.HipVector.solveBlock(H, [bs[j] for j, z in jobs], [z for j, z in jobs], poolStats=pool)
    for i, ((j, z), x) in enumerate(zip(jobs, xs)):
        assert pool["products"][i] == x.last_solve_stats["iterations"]
        _against_scipy(name, z, j, x.array, x.last_solve_stats, f"({name}) pool z = {z!r} rhs {j}")
    assert pool["width"] == 4 and pool["jobs"] == 12 and max(pool["histogram"]) == 4
    assert sum(k * v for k, v in pool["histogram"].items()) == sum(pool["products"])
    assert pool["rounds"] == sum(pool["histogram"].values())
    thin = sum(v for k, v in pool["histogram"].items() if k < 4)
    assert thin <= max(pool["products"][-4:]) + 4
    xs = hip.HipVector.solveBlock(H, bs[:4], gc.Z_REAL)
    for j, x in enumerate(xs):
        assert x.last_solve_stats["lock_step"] is True
        _against_scipy(name, gc.Z_REAL, j, x.array, x.last_solve_stats, f"({name}) real block rhs {j}")


def test_the_key_halves_the_product_count_on_the_weakly_dominant_operator(hip):
    """On (c) the device's product count with the key is at most half its count without it, for a complex and for the real
    shift.  (Without the feature the key is ignored and the counts are equal.)"""
    H = hip.HipCsrOperator.from_scipy(gc.operator("c"))
    print()
    for z in (gc.Z_COMPLEX, gc.Z_REAL):
        counts = {}
        for key in (False, True):
            b = hip.HipVector(gc.rhs(0).copy(), _options(key, maxiter=10000))
            x = hip.HipVector.solve(H, b, z)
            counts[key] = x.last_solve_stats["iterations"]
            assert ("preconditioner" in x.last_solve_stats) == key
        print(f"(c) z = {z!r}: {counts[False]} products without the key, {counts[True]} with it")
        assert 2 * counts[True] <= counts[False]


def test_zero_right_hand_side_short_limit_and_refusals(hip):
    H = hip.HipCsrOperator.from_scipy(gc.operator("c"))
    o = _options(True)
    for z in (gc.Z_COMPLEX, gc.Z_REAL):
        x = hip.HipVector.solve(H, hip.HipVector(np.zeros(gc.N), o), z)
        assert np.all(x.array == 0) and x.last_solve_stats["iterations"] == 0
    xs = hip.HipVector.solveBlock(H, [hip.HipVector(np.zeros(gc.N), o), hip.HipVector(gc.rhs(0).copy(), o)], gc.Z_COMPLEX)
    assert np.all(xs[0].array == 0) and xs[0].last_solve_stats["iterations"] == 0 and xs[1].last_solve_stats["iterations"] > 45
    short = _options(True, maxiter=1)
    for z in (gc.Z_COMPLEX, gc.Z_REAL):
        b = hip.HipVector(gc.rhs(0).copy(), short)
        with pytest.raises(UserWarning, match="not converged"):
            hip.HipVector.solve(H, b, z)
        assert b.last_solve_stats["iterations"] > 0 and b.last_solve_stats["preconditioner"] == "jacobi"
    bs = [hip.HipVector(gc.rhs(j).copy(), short) for j in range(3)]
    with pytest.raises(UserWarning, match="not converged"):
        hip.HipVector.solveBlock(H, bs, gc.Z_COMPLEX)
    assert all(b.last_solve_stats["preconditioner"] == "jacobi" for b in bs)
    b = hip.HipVector(gc.rhs(0).copy(), o)
    with pytest.raises(NotImplementedError, match="x0"):
        hip.HipVector.solve(H, b, gc.Z_COMPLEX, x0=np.zeros(gc.N))
    with pytest.raises(ValueError, match="gcrotmk"):
        hip.HipVector.solve(H, hip.HipVector(gc.rhs(0).copy(), {"linearSystemArgs": {"linearSolver": "minres",
                                                                                      "gcrotPreconditioner": "jacobi"}}), 0.05)
    slab = hip.HipCsrOperator.from_scipy(gc.operator("c"), 0, 2000)
    with pytest.raises(NotImplementedError, match="whole HipCsrOperator"):
        hip.HipVector.solve(slab, b, gc.Z_COMPLEX)


# ---------------------------------------------------------------- 8. FEAST and block Lanczos end to end
def test_feast_with_the_key_off_and_on(hip):
    """FEAST on (a), a window of 3 eigenvalues around the cluster next to 0.02, gcrotmk at linear_tol 1e-8, key off and on,
    contourPool both ways: equal window counts, all converged with equal outerIter, and every in-window eigenvalue of the
    preconditioned run as close to the host eigvalsh value as twice the unpreconditioned run's distance + 1e-12 |theta|.
    Measured: about 105 s, nearly all of it the two runs WITHOUT the key (10 FEAST iterations of 14 plain solves of some
    thousand products each); 8 Legendre nodes instead of 4 took 223 s.  The runs with the key take about a second."""
    lo, hi, exact = gc.feast_window()
    H = hip.HipCsrOperator.from_scipy(gc.operator_a())
    m0 = 7                                               # the window's 3 and two neighbours on either side
    Q = la.qr(np.random.default_rng(9).standard_normal((gc.N, m0)), mode="economic")[0]
    runs = {}
    for pool in (False, True):
        for key in (False, True):
            o = _options(key, maxiter=20000)
            o["linearSystemArgs"]["arnoldiColumnsPerPass"] = 4
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ev, Y, st = hip.feastDiagonalization(H, [hip.HipVector(Q[:, i].copy(), o) for i in range(m0)], 4, "legendre", lo, hi,
                                                     1e-6, 12, writeOut=False, contourPool=pool)
            inside = np.sort(ev[(ev > lo) & (ev < hi)])
            runs[pool, key] = (inside, st)
            assert st["converged"], (pool, key, st["residual"])
            assert len(inside) == len(exact) == 3
    print()
    for pool in (False, True):
        (e0, s0), (e1, s1) = runs[pool, False], runs[pool, True]
        assert s0["outerIter"] == s1["outerIter"]
        d0, d1 = np.abs(e0 - exact), np.abs(e1 - exact)
        print(f"contourPool={pool}: outerIter {s1['outerIter']}; distance to eigvalsh, key off {d0}, key on {d1}")
        assert np.all(d1 <= 2 * d0 + 1e-12 * np.abs(exact))


def test_block_lanczos_with_the_key_off_and_on(hip):
    """One block-Lanczos run with linearSolver="gcrotmk" (nBlock 4, L = 6, one cycle) on (a), key off and on: equal cumIter, Ritz
    values to the 1e-10 relative the Lanczos goldens are held to."""
    H = hip.HipCsrOperator.from_scipy(gc.operator_a())
    Q = la.qr(np.random.default_rng(5).standard_normal((gc.N, 4)), mode="economic")[0]
    runs = {}
    for key in (False, True):
        lsa = {"linearSolver": "gcrotmk", "linearIter": 20000, "linear_tol": 1e-10, "linear_atol": 1e-12}
        if key:
            lsa["gcrotPreconditioner"] = "jacobi"
        v0 = [hip.HipVector(Q[:, i].copy(), {"linearSystemArgs": lsa}) for i in range(4)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ev, Y, st = hip.inexactLanczosDiagonalization(H, v0, 0.02, 6, 1, 1e-12, writeOut=False)
        runs[key] = (ev, st)
    (e0, s0), (e1, s1) = runs[False], runs[True]
    print(f"\nblock Lanczos: cumIter {s0['cumIter']} / {s1['cumIter']}, Ritz values {np.sort(e1[:4])}")
    assert s0["cumIter"] == s1["cumIter"] and bool(s0["isConverged"]) == bool(s1["isConverged"])
    assert np.all(np.isfinite(e0[:4])) and np.all(np.isfinite(e1[:4]))
    np.testing.assert_allclose(np.sort(e1[:4]), np.sort(e0[:4]), rtol=1e-10, atol=0)
