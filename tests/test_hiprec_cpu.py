"""The high-precision reference of the kernel tests (tests/_hiprec.py) against exact rational arithmetic."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _hiprec as hp
import test_gpu_subspace_kernels as sk        # the inputs, grids and bounds of the GPU cases (nothing there runs on import)


def _exact_dot(x, y):
    return sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(x, y)), Fraction(0))


def _rel(got, exact, scale):
    return abs(Fraction(float(got)) - exact) / scale if isinstance(got, float) else \
        abs(Fraction(*np.longdouble(got).as_integer_ratio()) - exact) / scale


def LDr(z):
    return np.longdouble(np.real(z)).as_integer_ratio()


def LDi(z):
    return np.longdouble(np.imag(z)).as_integer_ratio()


def test_cancelling_dot_product_that_float64_gets_wrong():
    """Products of order one whose exact sum is below the rounding unit: the last term cancels the float64 value of the
    others, so what is left is their rounding remainder.  float64 np.dot (any order of summation, with or without FMA)
    is wrong in its leading digit; the extended-precision and the exact forms are not."""
    rng = np.random.default_rng(2024)
    x, y = rng.standard_normal(100), rng.standard_normal(100)
    s = _exact_dot(x, y)
    x, y = np.append(x, -float(s)), np.append(y, 1.0)
    exact = _exact_dot(x, y)
    assert exact != 0 and abs(exact) < 1e-15
    assert abs(float(np.dot(x, y)) - float(exact)) > 0.5 * abs(float(exact))
    scale = _exact_dot(np.abs(x), np.abs(y))
    assert _rel(hp.dot(x, y), exact, scale) <= 8 * 2.0 ** -63
    assert Fraction(hp._dot_exact(x, y)) == Fraction(float(exact))                # correctly rounded, leading digit right


@pytest.mark.parametrize("n", [1, 2, 17, 1000])
def test_dot_and_nrm2_against_fractions(n):
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n)), rng.standard_normal(n)
    exact = _exact_dot(x, y)
    scale = _exact_dot(np.abs(x), np.abs(y))
    assert _rel(hp.dot(x, y), exact, scale) <= (math.log2(n) + 2) * 2.0 ** -63
    assert Fraction(hp._dot_exact(x, y)) == Fraction(float(exact))
    nn = _exact_dot(x, x)
    got = Fraction(*np.longdouble(hp.nrm2(x)).as_integer_ratio())
    assert abs(got * got - nn) / nn <= (math.log2(n) + 4) * 2.0 ** -63


def test_complex_dot_conjugates_the_first_argument():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(50) + 1j * rng.standard_normal(50)
    y = rng.standard_normal(50) + 1j * rng.standard_normal(50)
    re = _exact_dot(x.real, y.real) + _exact_dot(x.imag, y.imag)
    im = _exact_dot(x.real, y.imag) - _exact_dot(x.imag, y.real)
    d = hp.dot(x, y)
    scale = _exact_dot(np.abs(x), np.abs(y)) * 2
    assert _rel(d.real, re, scale) <= 2.0 ** -58 and _rel(d.imag, im, scale) <= 2.0 ** -58
    assert abs(complex(d) - np.vdot(x, y)) <= 1e-14 * float(scale)


@pytest.mark.parametrize("cplx", [False, True])
def test_mgs_against_fractions(cplx):
    """mgs: norm, sequential coefficients with the conjugated product, norm, normalised vector - compared with the same
    sweep in exact rational arithmetic (complex numbers as pairs of Fractions), w nearly in span(V)."""
    rng = np.random.default_rng(11 + cplx)
    n, m = 12, 3
    V = rng.standard_normal((m, n)) + (1j * rng.standard_normal((m, n)) if cplx else 0)
    w = V.T @ rng.standard_normal(m) + 1e-9 * rng.standard_normal(n)

    def F(z):
        return (Fraction(float(np.real(z))), Fraction(float(np.imag(z))))

    Vf = [[F(z) for z in row] for row in V]
    wf = [F(z) for z in w]
    hf = []
    for v in Vf:
        c = (sum((a[0] * b[0] + a[1] * b[1] for a, b in zip(v, wf)), Fraction(0)),
             sum((a[0] * b[1] - a[1] * b[0] for a, b in zip(v, wf)), Fraction(0)))
        hf.append(c)
        wf = [(b[0] - (c[0] * a[0] - c[1] * a[1]), b[1] - (c[0] * a[1] + c[1] * a[0])) for a, b in zip(v, wf)]
    na2 = sum((b[0] * b[0] + b[1] * b[1] for b in wf), Fraction(0))
    nb, h, na, wout = hp.mgs(V, w)
    hmax = max(abs(complex(float(c[0]), float(c[1]))) for c in hf)
    for got, c in zip(h, hf):
        assert abs(Fraction(*LDr(got)) - c[0]) <= 2.0 ** -58 * Fraction(hmax)
        if cplx:
            assert abs(Fraction(*LDi(got)) - c[1]) <= 2.0 ** -58 * Fraction(hmax)
    # the projected remainder is ~1e-9 of w: its norm still agrees to ~2^-64 / 1e-9 relative
    assert abs(Fraction(*np.longdouble(na).as_integer_ratio()) ** 2 - na2) / na2 <= 1e-8
    assert abs(float(na) - math.sqrt(float(na2))) <= 1e-9 * math.sqrt(float(na2))
    ref = np.array([complex(float(b[0]), float(b[1])) for b in wf]) / math.sqrt(float(na2))
    assert np.max(np.abs(wout.astype(complex) - ref)) <= 1e-8
    assert float(nb) == pytest.approx(np.linalg.norm(w), rel=1e-15)
    # checkpoints: every prefix of the sweep
    cps = hp.mgs(V, w, checkpoints={0, 1, 3})
    assert set(cps) == {0, 1, 3} and len(cps[1][1]) == 1 and cps[3][1][0] == h[0]
    assert float(cps[0][2]) == float(nb)
    # no normalisation: the projected vector itself
    _, _, na_p, wp = hp.mgs(V, w, normalise=False)
    assert np.max(np.abs((wp / na_p) - wout)) == 0


def test_csr_matvec_against_fractions():
    """Unsorted columns, duplicates and an empty row; complex operand."""
    rowptr = np.array([0, 3, 3, 7])
    col = np.array([2, 0, 2, 1, 1, 0, 2])
    val = np.array([1e10, 0.1, -1e10, 0.3, 1.0 / 3.0, -2.5, 7.0])
    x = np.array([1.0 / 3.0 + 0.5j, 2.0 / 7.0 - 1j, 0.123456789 + 1e-3j])
    y, absax, rowlen = hp.csr_matvec(rowptr, col, val, x)
    assert list(rowlen) == [3, 0, 4]
    assert y[1] == 0 and absax[1] == 0
    for i in (0, 2):
        ks = range(rowptr[i], rowptr[i + 1])
        ex_r = sum((Fraction(float(val[k])) * Fraction(float(x[col[k]].real)) for k in ks), Fraction(0))
        ex_i = sum((Fraction(float(val[k])) * Fraction(float(x[col[k]].imag)) for k in ks), Fraction(0))
        sc = float(absax[i])
        assert abs(Fraction(*LDr(y[i])) - ex_r) <= 2.0 ** -60 * Fraction(sc)
        assert abs(Fraction(*LDi(y[i])) - ex_i) <= 2.0 ** -60 * Fraction(sc)


def test_exact_fallback_matches_the_extended_form(monkeypatch):
    """The exact form that stands in where longdouble is plain double gives the same values to the extended rounding."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(300) + 1j * rng.standard_normal(300)
    y = rng.standard_normal(300) + 1j * rng.standard_normal(300)
    ext = complex(hp.dot(x, y)), float(hp.nrm2(x))
    monkeypatch.setattr(hp, "EXTENDED", False)
    ex = complex(hp.dot(x, y)), float(hp.nrm2(x))
    assert abs(ext[0] - ex[0]) <= 1e-15 * abs(ex[0]) and abs(ext[1] - ex[1]) <= 1e-16 * ex[1]
    assert float(hp.dot(x.real, y.real)) == hp._dot_exact(x.real, y.real)


# ---------------------------------------------------------------- references of the Lanczos-side subspace kernels
def _F(a):
    return [Fraction(float(v)) for v in a]


def _ld(v):
    return Fraction(*np.longdouble(v).as_integer_ratio())


def _small_rows(rng, m, n):
    return rng.standard_normal((m, n)) * 2.0 ** rng.integers(-10, 4, (m, 1))


def test_orthonormalize_mgs_against_fractions():
    """t1 = x.q, t2 = q.q, x -= q (t1 / t2) with columns that are neither unit nor orthogonal, x nearly in their span."""
    rng = np.random.default_rng(31)
    n, m = 11, 3
    Q = _small_rows(rng, m, n)
    Q[1] += 0.3 * Q[0]
    x = Q.T @ rng.standard_normal(m) + 1e-6 * rng.standard_normal(n)
    xf, S = _F(x), None
    x0n = math.sqrt(float(sum(v * v for v in xf)))
    S = Fraction(x0n)
    for q in Q:
        qf = _F(q)
        t1, t2 = sum(a * b for a, b in zip(xf, qf)), sum(a * a for a in qf)
        xf = [a - b * (t1 / t2) for a, b in zip(xf, qf)]
        S += abs(t1 / t2) * Fraction(math.sqrt(float(t2)))
    ipf = sum(v * v for v in xf)
    ip, xp, Sg = hp.orthonormalize_mgs(Q, x)
    scale = Fraction(float(S))
    assert max(abs(_ld(g) - e) for g, e in zip(xp, xf)) <= 2.0 ** -58 * scale
    assert abs(_ld(ip) - ipf) <= 2.0 ** -55 * scale * Fraction(math.sqrt(float(ipf)))
    assert abs(float(Sg) - float(S)) <= 1e-12 * float(S)
    ip0, x0, S0 = hp.orthonormalize_mgs(Q[:0], x)                       # no columns: x itself
    assert np.array_equal(x0.astype(np.float64), x) and float(S0) == pytest.approx(x0n, rel=1e-15)
    assert float(ip0) == pytest.approx(x0n ** 2, rel=1e-15)


def test_orthonormalize_cgs2_against_fractions():
    """Two passes, every coefficient of a pass from the vector the pass starts with, no division by q.q."""
    rng = np.random.default_rng(32)
    n, m = 9, 3
    Q = _small_rows(rng, m, n)
    x = Q.T @ rng.standard_normal(m) + rng.standard_normal(n)
    xf = _F(x)
    Qf = [_F(q) for q in Q]
    want = []
    for _ in range(2):
        c = [sum(a * b for a, b in zip(qf, xf)) for qf in Qf]
        want.append((math.sqrt(float(sum(v * v for v in xf))),
                     sum(abs(float(cj)) * math.sqrt(float(sum(a * a for a in qf))) for cj, qf in zip(c, Qf)),
                     float(sum(sum(a * a for a in qf) for qf in Qf))))
        xf = [v - sum(cj * qf[i] for cj, qf in zip(c, Qf)) for i, v in enumerate(xf)]
    ipf = sum(v * v for v in xf)
    ip, xp, scales = hp.orthonormalize_cgs2(Q, x)
    big = Fraction(max(abs(float(v)) for v in xf) + want[1][1] * (1 + want[1][2]) + want[0][1] * (1 + want[0][2]) ** 2)
    assert max(abs(_ld(g) - e) for g, e in zip(xp, xf)) <= 2.0 ** -57 * big
    assert abs(_ld(ip) - ipf) <= 2.0 ** -55 * big * big
    for got, exp in zip(scales, want):
        assert [float(v) for v in got] == pytest.approx(list(exp), rel=1e-12)
    ip0, x0, sc0 = hp.orthonormalize_cgs2(Q[:0], x)
    assert np.array_equal(x0.astype(np.float64), x) and float(sc0[0][1]) == 0 and float(sc0[1][2]) == 0


def test_gram_and_combine_against_fractions():
    rng = np.random.default_rng(33)
    A, B = _small_rows(rng, 3, 40), _small_rows(rng, 4, 40)
    G, Gabs = hp.gram(A, B)
    assert G.shape == Gabs.shape == (3, 4)
    for i in range(3):
        for j in range(4):
            mag = _exact_dot(np.abs(A[i]), np.abs(B[j]))
            assert abs(_ld(G[i, j]) - _exact_dot(A[i], B[j])) <= 2.0 ** -60 * mag
            assert abs(_ld(Gabs[i, j]) - mag) <= 2.0 ** -60 * mag
    V, Cm = _small_rows(rng, 5, 7), rng.standard_normal((5, 3))
    Y, Yabs = hp.combine(V, Cm)
    assert Y.shape == Yabs.shape == (7, 3)
    for i in range(7):
        for c in range(3):
            mag = _exact_dot(np.abs(V[:, i]), np.abs(Cm[:, c]))
            assert abs(_ld(Y[i, c]) - _exact_dot(V[:, i], Cm[:, c])) <= 2.0 ** -60 * mag
            assert abs(_ld(Yabs[i, c]) - mag) <= 2.0 ** -60 * mag


def test_new_references_agree_without_extended_precision(monkeypatch):
    rng = np.random.default_rng(34)
    Q, x = _small_rows(rng, 3, 50), rng.standard_normal(50)
    ext = (hp.orthonormalize_mgs(Q, x), hp.orthonormalize_cgs2(Q, x), hp.gram(Q, Q[:2]), hp.combine(Q, Q[:, :2]))
    monkeypatch.setattr(hp, "EXTENDED", False)
    ex = (hp.orthonormalize_mgs(Q, x), hp.orthonormalize_cgs2(Q, x), hp.gram(Q, Q[:2]), hp.combine(Q, Q[:, :2]))
    for a, b in zip(ext, ex):
        assert float(a[0] if np.ndim(a[0]) == 0 else 0) == pytest.approx(float(b[0] if np.ndim(b[0]) == 0 else 0), rel=1e-12)
    assert np.allclose(ext[0][1].astype(float), ex[0][1].astype(float), rtol=0, atol=1e-12)
    assert np.allclose(ext[2][0].astype(float), ex[2][0].astype(float), rtol=1e-13, atol=1e-13 * float(np.max(ext[2][1])))
    assert np.allclose(ext[3][0].astype(float), ex[3][0].astype(float), rtol=1e-13, atol=1e-13 * float(np.max(ext[3][1])))


# ---------------------------------------------------------------- the bounds of tests/test_gpu_subspace_kernels.py
# A float64 emulation of each kernel's algorithm and summation tree (blas1.hip) on the inputs of the GPU cases must stay
# under a quarter of the bound the GPU test applies, and each seeded fault - injected here, in the emulation only - must
# exceed it.  fma(a, b, c) is emulated through the extended format where there is one (a product of two doubles rounded to
# 64 bits first: off by 2^-11 of a rounding at most), else as a * b + c.
CUS = 256                                                               # the grids of an MI355X


def _fma(a, b, c):
    if not hp.EXTENDED:
        return a * b + c
    return (np.asarray(a, hp.LD) * np.asarray(b, hp.LD) + np.asarray(c, hp.LD)).astype(np.float64)


def _emu_tree(acc, G):
    """acc: one value per thread of G workgroups of 256 -> per-workgroup sums: the 64-lane shuffle tree, four waves in order."""
    v = acc.reshape(G, 4, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
    w = v[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _emu_records(part, skip=None):
    """finish_records: the <= 64 records of a group in order, then the group records in order (last axis: workgroups)."""
    G = part.shape[-1]
    groups = []
    for g0 in range(0, G, 64):
        s = np.zeros(part.shape[:-1])
        for b in range(g0, min(g0 + 64, G)):
            if b != skip:
                s = s + part[..., b]
        groups.append(s)
    tot = groups[0]
    for s in groups[1:]:
        tot = tot + s
    return tot


def _emu_dot(x, y, G, final="records", skip_tail=False, skip_record=None):
    n = len(x)
    n2, T = n // 2, 256 * G
    iters = -(-n2 // T)
    px, py = np.zeros((iters * T, 2)), np.zeros((iters * T, 2))
    px[:n2], py[:n2] = x[:2 * n2].reshape(n2, 2), y[:2 * n2].reshape(n2, 2)
    px, py = px.reshape(iters, T, 2), py.reshape(iters, T, 2)
    acc = np.zeros(T)
    for it in range(iters):
        acc = _fma(px[it, :, 1], py[it, :, 1], _fma(px[it, :, 0], py[it, :, 0], acc))
    if (n & 1) and not skip_tail:
        acc[0] = _fma(x[-1], y[-1], acc[0])
    part = _emu_tree(acc, G)
    if final == "records":
        return float(_emu_records(part, skip_record))
    pad = np.zeros(256 * -(-G // 256))                                   # hipeig_dot: the last workgroup's own tree
    pad[:G] = part
    t = np.zeros(256)
    for r in pad.reshape(-1, 256):
        t = t + r
    return float(_emu_tree(t, 1)[0])


def _emu_mgs(Q, x, G, fault=None):
    x = x.copy()
    for q in Q:
        t1, t2 = _emu_dot(x, q, G), _emu_dot(q, q, G)
        coef = t1 if fault == "t1 for t1/t2" else t1 / t2
        new = x + (-(q * coef))
        if fault == "update skips the odd tail":
            new[-1] = x[-1]
        x = new
    return _emu_dot(x, x, G, skip_tail=(fault == "dot skips the odd tail"),
                    skip_record=(64 if fault == "one of 65 records left out" else None)), x


def _emu_cgs2(Q, x, G, fault=None):
    x, m = x.copy(), len(Q)
    for _ in range(2):
        for j0 in range(0, m, 256):                                      # 256 columns per multi_dot / lincomb round
            c = [_emu_dot(q, x, G) for q in Q[j0:j0 + 256]]
            for j, cj in enumerate(c):
                if fault == "coefficients 16.. not applied" and j >= 16:
                    continue
                x = _fma(-cj, Q[j0 + j], x)
    return _emu_dot(x, x, G, final="threads"), x


def _emu_lincomb(V, c, fault=None):
    acc = np.zeros(V.shape[1])
    for j in range(len(V)):
        if fault == "second chunk overwrites" and j == 16:
            acc = np.zeros(V.shape[1])
        acc = _fma(c[j], V[j], acc)
    return acc


def _emu_gram(A, B, cus):
    """The MFMA kernel's order: per workgroup and wave 32 rows of every tile it takes in sequence, four waves, records."""
    n = A.shape[1]
    G, T = sk.gram_grid(n, cus)
    rows_pad = G * T * 128
    Ap, Bp = np.zeros((len(A), rows_pad)), np.zeros((len(B), rows_pad))
    Ap[:, :n], Bp[:, :n] = A, B
    Ap, Bp = Ap.reshape(len(A), T, G, 4, 32), Bp.reshape(len(B), T, G, 4, 32)      # tile t = pass * G + workgroup
    acc = np.zeros((len(A), len(B), G, 4))
    for t in range(T):
        for r in range(32):
            acc = acc + Ap[:, None, t, :, :, r] * Bp[None, :, t, :, :, r]
    part = ((acc[..., 0] + acc[..., 1]) + acc[..., 2]) + acc[..., 3]
    return _emu_records(part)


def _ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    return float(np.max(err / bound)) if err.size else 0.0


def _ortho_ratios(n, ms, per_thread=None, fault=None, only=None):
    """error / bound of the emulated hipeig_orthonormalize over the GPU test's cases at length n: {(method, quantity): max}."""
    G = sk._grid_records(n, CUS, per_thread)
    crec, cdot = sk.c_rec(n, G), sk.c_dot(n, G)
    cases = [c for c in sk.ortho_cases(n, ms) if only is None or (c[0], c[1]) == only]
    sets = sk.column_sets(n, max(c[2] for c in cases))
    out = {}
    for name, delta, m, idx in cases:
        V = sets[name]
        x = sk.operand(V, m, delta, idx)
        for tag, emu, ref in (("mgs", _emu_mgs, hp.orthonormalize_mgs), ("cgs2", _emu_cgs2, hp.orthonormalize_cgs2)):
            ip_r, x_r, scale = ref(V[:m], x)
            nb, xb, _ = sk.mgs_bounds(m, ip_r, scale) if tag == "mgs" else sk.cgs2_bounds(m, ip_r, scale, crec, cdot)
            ip, xo = emu(V[:m], x, G, fault)
            for key, r in ((("norm"), _ratio(abs(hp.LD(np.sqrt(ip)) - np.sqrt(ip_r)), nb)),
                           (("x"), _ratio(float(hp.nrm2(xo.astype(hp.LD) - x_r)), xb))):
                out[(tag, key)] = max(out.get((tag, key), 0.0), r)
    return out


@pytest.mark.parametrize("n,ms,per_thread", [(3, sk.MS, None), (255, sk.MS, None), (2049, sk.MS, None), (16640, [1, 3, 17], 1),
                                             (66561, [3, 17], None)])
def test_orthonormalize_bounds_hold_four_times_over_in_float64(n, ms, per_thread):
    for key, r in _ortho_ratios(n, ms, per_thread).items():
        assert r <= 0.25, f"n={n} {key}: the float64 emulation uses {r:.3g} of the bound"


def test_cgs2_bound_holds_four_times_over_beyond_256_columns():
    n, m = 2049, 257
    G = sk._grid_records(n, CUS)
    V = sk.column_sets(n, m)["scaled"]
    x = sk.operand(V, m, 1.0, 0)
    ip_r, x_r, scales = hp.orthonormalize_cgs2(V, x)
    nb, xb, _ = sk.cgs2_bounds(m, ip_r, scales, sk.c_rec(n, G), sk.c_dot(n, G))
    ip, xo = _emu_cgs2(V, x, G)
    assert abs(hp.LD(np.sqrt(ip)) - np.sqrt(ip_r)) <= 0.25 * nb
    assert float(hp.nrm2(xo.astype(hp.LD) - x_r)) <= 0.25 * xb


@pytest.mark.parametrize("fault,method,n,ms,per_thread,only", [
    ("update skips the odd tail", "mgs", 513, [3, 17], None, None),
    ("dot skips the odd tail", "mgs", 513, [3, 17], None, ("scaled", 1.0)),
    ("t1 for t1/t2", "mgs", 513, [1, 17], None, None),
    ("one of 65 records left out", "mgs", 66561, [3], None, ("scaled", 1.0)),
    ("coefficients 16.. not applied", "cgs2", 513, [17], None, None)])
def test_seeded_orthonormalize_faults_exceed_the_bounds(fault, method, n, ms, per_thread, only):
    """Each fault, in every case it is tried on, breaks the norm bound or the vector bound of its method."""
    for case in [c for c in sk.ortho_cases(n, ms) if only is None or (c[0], c[1]) == only]:
        r = _ortho_ratios(n, [case[2]], per_thread, fault, only=(case[0], case[1]))
        assert max(r[(method, "norm")], r[(method, "x")]) > 1, f"{fault} passes in case {case}: {r}"


@pytest.mark.parametrize("n", [64, 65, 127, 128, 129, 8192, 8193])
def test_gram_bound_holds_four_times_over_in_float64(n):
    rng = np.random.default_rng([n, 1])                                  # the rows of test_gram_blocks_element_by_element
    A, B = sk.rows(rng, 33, n), sk.rows(rng, 33, n)
    G_r, Gabs = hp.gram(A, B)
    bound = sk.c_gram(n, CUS) * sk.U * Gabs.astype(float)
    assert sk.c_gram(n, CUS) < 1e-13 / sk.U
    if n <= 128:
        assert sk.c_gram(n, CUS) == 35
    got = _emu_gram(A, B, CUS)
    assert _ratio(np.abs(got.astype(hp.LD) - G_r).astype(float), bound) <= 0.25
    # seeded faults: a 16 x 16 block transposed; the lower block of this non-symmetric call taken from the upper one
    for what in ("transposed", "mirrored"):
        bad = got.copy()
        if what == "transposed":
            bad[0:16, 16:32] = got[0:16, 16:32].T
        else:
            bad[16:32, 0:16] = got[0:16, 16:32].T
        assert _ratio(np.abs(bad.astype(hp.LD) - G_r).astype(float), bound) > 1, what


def test_gram_bound_with_several_tiles_per_workgroup():
    n = (1 << 14) + 129                                                  # 130 tiles on 32 workgroups: 5 tiles each, as
    cus = 32                                                             # 2050 tiles on an MI355X's grid take several
    assert sk.gram_grid(n, cus) == (32, 5) and sk.gram_grid((1 << 18) + 129, CUS)[1] > 1
    rng = np.random.default_rng([n, 4])
    A, B = sk.rows(rng, 3, n), sk.rows(rng, 17, n)
    G_r, Gabs = hp.gram(A, B)
    err = np.abs(_emu_gram(A, B, cus).astype(hp.LD) - G_r).astype(float)
    assert _ratio(err, sk.c_gram(n, cus) * sk.U * Gabs.astype(float)) <= 0.25


@pytest.mark.parametrize("n,per_thread", [(1, None), (3, None), (2049, None), (16640, 1)])
def test_multi_dot_bound_holds_four_times_over_in_float64(n, per_thread):
    rng = np.random.default_rng([n, 6])                                  # the rows of the GPU test
    Y, x = sk.rows(rng, 257, n), rng.standard_normal(n)
    G = sk._grid_records(n, CUS, per_thread)
    G_r, Gabs = hp.gram(Y, x[None, :])
    bound = sk.c_rec(n, G) * sk.U * Gabs[:, 0].astype(float)
    got = np.array([_emu_dot(y, x, G) for y in Y])
    assert _ratio(np.abs(got.astype(hp.LD) - G_r[:, 0]).astype(float), bound) <= 0.25
    if n & 1:
        bad = np.array([_emu_dot(y, x, G, skip_tail=True) for y in Y[:17]])
        assert np.all(np.abs(bad.astype(hp.LD) - G_r[:17, 0]).astype(float) > bound[:17])
    if G == 65:                                                          # (one element per thread: the upper half of the grid idles)
        bad = np.array([_emu_dot(y, x, G, skip_record=20) for y in Y[:17]])
        assert np.all(np.abs(bad.astype(hp.LD) - G_r[:17, 0]).astype(float) > bound[:17])


@pytest.mark.parametrize("n", [1, 3, 1025])
def test_lincomb_bounds_hold_four_times_over_in_float64(n):
    rng = np.random.default_rng([n, 7])                                  # the rows of the GPU test
    V, coef = sk.rows(rng, 33, n), rng.standard_normal(33) * 2.0 ** rng.integers(-3, 4, 33)
    for k in (1, 4, 5, 8, 9, 16, 17, 33):
        Y_r, Yabs = hp.combine(V[:k], coef[:k, None])
        bound = sk.c_lin(k) * sk.U * Yabs[:, 0].astype(float)
        err = np.abs(_emu_lincomb(V[:k], coef[:k]).astype(hp.LD) - Y_r[:, 0]).astype(float)
        assert _ratio(err, bound) <= 0.25, f"k={k}"
        if k == 17:
            bad = _emu_lincomb(V[:k], coef[:k], "second chunk overwrites")
            assert np.all(np.abs(bad.astype(hp.LD) - Y_r[:, 0]).astype(float) > bound)
    rng = np.random.default_rng([n, 8])
    V = sk.rows(rng, 40, n)
    Cw = rng.standard_normal((40, 36)) * 2.0 ** rng.integers(-3, 4, (40, 36))
    for m, k in ((1, 1), (5, 4), (9, 9), (17, 17), (40, 33)):
        Y_r, Yabs = hp.combine(V[:m], Cw[:m, :k])
        got = np.stack([_emu_lincomb(V[:m], Cw[:m, c]) for c in range(k)], axis=1)
        assert _ratio(np.abs(got.astype(hp.LD) - Y_r).astype(float), sk.c_lin(m) * sk.U * Yabs.astype(float)) <= 0.25, (m, k)


@pytest.mark.parametrize("n,per_thread", [(1, None), (2, None), (3, None), (511, None), (513, None), (16641, 1), (600001, 1)])
def test_dot_bound_holds_four_times_over_in_float64(n, per_thread):
    rng = np.random.default_rng([n, 9])                                  # the vectors of the GPU test
    x = rng.standard_normal(n) * 2.0 ** rng.integers(-10, 4, n)
    y = rng.standard_normal(n)
    G = sk._grid_records(n, CUS, per_thread)
    c = sk.c_dot(n, G)
    mag = float(hp.dot(np.abs(x), np.abs(y)))
    assert abs(hp.LD(_emu_dot(x, y, G, final="threads")) - hp.dot(x, y)) <= 0.25 * c * sk.U * mag
    nrm = math.sqrt(_emu_dot(x, x, G, final="threads"))
    assert abs(hp.LD(nrm) - hp.nrm2(x)) <= 0.25 * (c / 2 + 1) * sk.U * float(hp.nrm2(x))
    if n & 1 and n > 1:
        assert abs(hp.LD(_emu_dot(x, y, G, final="threads", skip_tail=True)) - hp.dot(x, y)) > c * sk.U * mag
