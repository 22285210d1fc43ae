"""The real operator products of all five sweep layouts against an extended-precision reference, row by row.

``hipeig_spmv`` (y = A x) and ``hipeig_spmv_shift`` (y = sign (sigma x - A x)) on layout 1 (CSR-vector), 2 (CSR-stream),
3 (wave units, with and without the dense prefetch of the next x window), 4 (workgroup units, fp64 LDS atomics) and 5
(workgroup units, fixed-point accumulators), the last two also with column splits.  Every comparison is per row against
``shift_reference`` with ``shift_bound`` (layouts 1 to 4) or ``fixed_point_bound`` (layout 5) of tests/_product_cases.py:
the derivations are there, tests/test_real_product_bound_cpu.py holds a float64 emulation of every layout to them and
shows the faults they catch.  The operators put every sub-wave width (4, 8, 16, 32 and 64 lanes per row), the row blocks
of the CSR-stream kernel at their edges (rows of 2047, 2048, 2049 and 4097 entries, 1200 empty rows in a row, a long last
row), row slabs applied to a full-length operand and the tiny shapes n = 1, 63, 64, 65 under the bound.

The layout geometry is read from the environment when a layout is first built, so every geometry gets a fresh operator
after its knobs are set.  Each test prints the largest error / bound per (operator, layout, geometry) (pytest -s); nothing
is fitted to those numbers.
"""
import numpy as np
import pytest

import _product_cases as pc

pytestmark = pytest.mark.gpu

SIGNS = (1.0, -1.0)
KNOBS = ("HIPEIG_TCOO_RW", "HIPEIG_TCOO_WBITS", "HIPEIG_TCOO_PREFETCH", "HIPEIG_TCOOW_RW", "HIPEIG_TCOOW_WBITS",
         "HIPEIG_TCOOW_CSPLIT")
WAVE = {"HIPEIG_TCOO_RW": "64", "HIPEIG_TCOO_WBITS": "10"}
WG = {"HIPEIG_TCOOW_RW": "64", "HIPEIG_TCOOW_WBITS": "10"}
# (label, layout, knobs, layout_info fields the knobs set)
GEOMETRIES = [
    ("csr-vector", 1, {}, {}),
    ("csr-stream", 2, {}, {}),
    ("wave units 64 x 1024", 3, WAVE, {"rows_per_block": 64, "window_bits": 10}),
    ("wave units 64 x 1024, prefetch", 3, {**WAVE, "HIPEIG_TCOO_PREFETCH": "1"}, {"rows_per_block": 64, "window_bits": 10}),
    ("workgroup units 64 x 1024", 4, WG, {"rows_per_block": 64, "window_bits": 10, "column_splits": 1}),
    ("workgroup units 64 x 1024, 3 splits", 4, {**WG, "HIPEIG_TCOOW_CSPLIT": "3"},
     {"rows_per_block": 64, "window_bits": 10, "column_splits": 3}),
    ("fixed point 64 x 1024", 5, WG, {"rows_per_block": 64, "window_bits": 10, "column_splits": 1}),
    ("fixed point 64 x 1024, 3 splits", 5, {**WG, "HIPEIG_TCOOW_CSPLIT": "3"},
     {"rows_per_block": 64, "window_bits": 10, "column_splits": 3}),
]
AUTOMATIC = [("wave units, automatic", 3, {}, {}), ("workgroup units, automatic", 4, {}, {"column_splits": 1}),
             ("fixed point, automatic", 5, {}, {"column_splits": 1})]
REPEATABLE = (1, 2, 3, 5)                    # layouts that fix the order of a row's adds, or add integers
U = pc.U


def _set_knobs(monkeypatch, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def _worst_row(got, ref, bound):
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    row = int(np.argmax(np.where(np.isfinite(err), err / bound, np.inf)))
    return row, int(np.sum(~(err <= bound)))


def _check(case, label, sigma, sign, got, fixed, splits):
    """One product against reference and bound on every row; rows that store nothing hold the shift term's single
    rounding (adding +-0 is exact), 0.0 for the plain product."""
    ref, bound = case.reference(sigma, sign), case.bound(sigma, sign, fixed=fixed, column_splits=splits)
    assert got.shape == bound.shape
    r = pc.error_ratio(got, ref, bound)
    if r > 1.0:
        row, over = _worst_row(got, ref, bound)
        raise AssertionError(f"{case.name}, {label}, sigma={sigma} sign={sign:+.0f}: error / bound {r:.3g} at row {row} "
                             f"({case.lens[row]} entries; {over} rows over)")
    want = np.zeros(int(case.empty.sum())) if sign == 0 else (sign * sigma) * case.xl[case.empty]
    assert np.array_equal(got[case.empty], want), f"{case.name}, {label}, sigma={sigma} sign={sign:+.0f}: an empty row holds " \
                                                  "more than its shift term"
    return r


def _run_geometry(hip, monkeypatch, case, geometry, exact_fixed=False):
    """Every product of one (operator, geometry): applyOp, and apply_shifted with each shift and both signs.  Returns the
    largest error / bound."""
    label, layout, knobs, fields = geometry
    _set_knobs(monkeypatch, knobs)
    H = hip.HipCsrOperator.from_csr_arrays(*case.csr, case.ncols, case.row_offset)
    assert (H.nrows, H.ncols, H.row_offset, H.nnz) == (case.nrows, case.ncols, case.row_offset, len(case.csr[1]))
    H.set_variant(layout)
    X = hip.HipVector(case.x)
    ctx = H.ctx
    fixed, splits = layout == 5, int(knobs.get("HIPEIG_TCOOW_CSPLIT", 1))
    stored = H.nnz > 0

    def product(sigma, sign):
        if sign == 0:
            return X.applyOp(H).array
        y = ctx.alloc(case.nrows)
        H.apply_shifted(sigma, X._buf, y, reverse=sign < 0)
        return hip.HipVector(y).array

    got = product(0.0, 0.0)
    # the layout asked for is the layout taken; an operator that stores nothing has no blocked copy and streams
    assert H.last_variant() == H.VARIANTS[layout if stored or layout < 3 else 2], f"{case.name}, {label}: {H.last_variant()}"
    if stored:
        info = H.layout_info()
        assert {k: info[k] for k in fields} == fields, f"{case.name}, {label}: {info}"
    worst = _check(case, label, 0.0, 0.0, got, fixed and stored, splits)
    if layout in REPEATABLE:
        assert np.array_equal(got, product(0.0, 0.0)), f"{case.name}, {label}: the second call differs"
    if fixed and stored:
        R, Xmax = H.fixed_point_info()
        Rh, Xh = pc.fixed_point_ingredients(case.csr[0], case.csr[2], case.x)
        assert Xmax == Xh and abs(R - Rh) <= int(case.lens.max()) * U * Rh, (case.name, label, R, Rh, Xmax, Xh)
        if exact_fixed and splits == 1:
            sums = pc.fixed_point_sums(*case.csr, case.x, R)
            assert np.array_equal(got, sums), f"{case.name}, {label}: not the integer arithmetic bit for bit"
    for sigma in pc.REAL_SHIFTS:
        for sign in SIGNS:
            got = product(sigma, sign)
            worst = max(worst, _check(case, label, sigma, sign, got, fixed and stored, splits))
            if layout in REPEATABLE:
                assert np.array_equal(got, product(sigma, sign)), f"{case.name}, {label}: the second call differs"
            if fixed and stored and exact_fixed and splits == 1:
                assert np.array_equal(got, pc.axpy_epilogue(sigma, sign, case.xl, sums)), \
                    f"{case.name}, {label}, sigma={sigma} sign={sign:+.0f}: not the integer arithmetic bit for bit"
    assert np.array_equal(X.array, case.x), f"{case.name}, {label}: the operand changed"
    return worst


def _run(hip, monkeypatch, case, geometries, exact_fixed=False):
    worst = {g[0]: _run_geometry(hip, monkeypatch, case, g, exact_fixed) for g in geometries}
    print(f"\nreal products, {case.name} ({case.nrows} x {case.ncols}, {case.lanes} lanes): max error / bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_4_lanes_per_row(hip, monkeypatch):
    """1500 rows of 0..4 entries: 64 groups of 4 lanes per workgroup; layout 5 meets the integer emulation bit for bit."""
    _run(hip, monkeypatch, pc.lanes4(), GEOMETRIES, exact_fixed=True)


def test_16_lanes_per_row(hip, monkeypatch):
    """1201 rows of 30..90 entries, a tenth of them empty."""
    _run(hip, monkeypatch, pc.lanes16(), GEOMETRIES)


def test_32_lanes_per_row_on_a_slab(hip, monkeypatch):
    """Rows 700..1299 of 2000 columns, 100..379 entries each, applied to the full-length operand."""
    _run(hip, monkeypatch, pc.lanes32(), GEOMETRIES)


def test_64_lanes_per_row_on_a_slab(hip, monkeypatch):
    """Rows 1000..1299 of 3000 columns, 384..900 entries each: whole waves per row, 4 rows per workgroup pass."""
    _run(hip, monkeypatch, pc.lanes64(), GEOMETRIES)


def test_row_blocks_of_the_stream_kernel_at_their_edges(hip, monkeypatch):
    """Rows of 2048 (LDS path), 2049 (whole-workgroup path), 2047 and 4097 entries, 1200 empty rows in a row (the row
    cap closes the block), a 2049-entry last row; the blocked layouts also with their automatic geometry."""
    _run(hip, monkeypatch, pc.stream_edges(), GEOMETRIES + AUTOMATIC, exact_fixed=True)


@pytest.mark.parametrize("build", [pc.edge3001, pc.ragged3001], ids=["edge_matrix", "ragged_csr"])
def test_the_8_lane_operators_of_the_other_product_tests(hip, monkeypatch, build):
    _run(hip, monkeypatch, build(), GEOMETRIES)


@pytest.mark.parametrize("n,stored", pc.TINY, ids=[f"n={n}{'' if s else ', nothing stored'}" for n, s in pc.TINY])
def test_tiny_shapes(hip, monkeypatch, n, stored):
    """n = 1, 63, 64, 65: a unit of the blocked layouts partly beyond nrows, a window shorter than its nominal width."""
    _run(hip, monkeypatch, pc.tiny(n, stored), GEOMETRIES, exact_fixed=True)


@pytest.mark.parametrize("wbits,rw", [(22, 1024), (21, 2048)])
def test_the_entry_that_would_pack_to_the_padding_mark(hip, monkeypatch, wbits, rw):
    """Wave units asked for with rw << wbits = 2^32: local row rw - 1, column 2^wbits - 1 of a window would pack to
    0xFFFFFFFF, the sweep's mark for "no entry", and drop out of the product.  The builder keeps the rows per unit below
    2^(32 - wbits) - a multiple of 64, as the knob rounds them - so the entry stays in."""
    case = pc.padding_mark_slab(wbits, rw)
    _set_knobs(monkeypatch, {"HIPEIG_TCOO_WBITS": str(wbits), "HIPEIG_TCOO_RW": str(rw)})
    H = hip.HipCsrOperator.from_csr_arrays(*case.csr, case.ncols, case.row_offset)
    H.set_variant(3)
    X = hip.HipVector(case.x)
    got = X.applyOp(H).array
    assert H.last_variant() == H.VARIANTS[3]
    r = _check(case, f"wave units, {wbits} window bits", 0.0, 0.0, got, False, 1)
    print(f"\nreal products, {case.name}: max error / bound {r:.3f}")
    info = H.layout_info()
    assert info["window_bits"] == wbits and info["rows_per_block"] == rw - 64, info
    assert np.array_equal(got, X.applyOp(H).array)
