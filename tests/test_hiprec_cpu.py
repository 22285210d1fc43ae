"""The high-precision reference of the kernel tests (tests/_hiprec.py) against exact rational arithmetic."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _hiprec as hp


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
