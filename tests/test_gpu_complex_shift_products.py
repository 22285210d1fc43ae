"""The complex-shift products of the FEAST contour solves against an extended-precision reference, row by row.

``hipeig_spmv_shift_pair`` (the fused pair sweep, or two real sweeps and two ``axpby``), ``hipeig_spmm_shift_pairs`` (one
shift per block, ``ShiftPairBlockEpilogue<4|8|16>``) and ``hipeig_spmm_shift_pairs_z`` (a shift per operand,
``ShiftPairsZBlockEpilogue<4|8|16>``).  Every comparison is per row and per half against ``shift_pair_reference`` with
``shift_pair_bound`` (tests/_product_cases.py: the bound's derivation is there, tests/test_complex_shift_bound_cpu.py holds
a float64 emulation to it and shows the faults it catches) - on operators with empty rows, 300-entry rows, unsorted and
duplicate columns, with several column windows and small row blocks forced, on more row blocks than CUs, on row slabs
applied to full-length operands, and with shifts that switch each term of the epilogue off or make the operator sum the
small part of the result.

The layout geometry is read from the environment when a layout is first built, so every test builds its own operator
after setting the knobs.  Each test prints the worst error / bound it met per form and block width (pytest -s).
"""
import numpy as np
import pytest
import scipy.sparse as sp

import _product_cases as pc
from _product_cases import SHIFTS, U
from test_gpu_stream_layout import SMALL_UNITS

pytestmark = pytest.mark.gpu

N = 3001
SIGNS = (1.0, -1.0)
_CASES = {}


class _Case:
    """An operator's rows as CSR arrays (of a slab: rows row_offset ..), the full-length operands, and the references
    and bounds on them: the half-products once per operand, a reference once per (operand, shift, sign)."""

    def __init__(self, csr, ncols, row_offset=0, count=11):
        self.csr, self.ncols, self.row_offset = csr, ncols, row_offset
        self.nrows = len(csr[0]) - 1
        self.X = pc.complex_operands(ncols, count)
        self.empty = np.diff(csr[0]) == 0
        self._products, self._refs = {}, {}

    def ref(self, p, z, sign):
        key = (p, complex(z), float(sign))
        if key not in self._refs:
            if p not in self._products:
                self._products[p] = pc.half_products(*self.csr, *self.X[p])
            args = (*self.csr, *self.X[p], z, sign, self.row_offset, self._products[p])
            self._refs[key] = pc.shift_pair_reference(*args) + pc.shift_pair_bound(*args)
        return self._refs[key]

    def operator(self, hip):
        return hip.HipCsrOperator.from_csr_arrays(*self.csr, self.ncols, self.row_offset)

    def upload(self, hip, count=None):
        return [(hip.HipVector(xr)._buf, hip.HipVector(xi)._buf) for xr, xi in self.X[:count]]


def _case(name, build):
    if name not in _CASES:
        _CASES[name] = build()
    return _CASES[name]


def _ragged():
    return _case("ragged", lambda: _Case(pc.ragged_csr(N, 11, duplicates=True), N))


def _summed(csr, n):
    A = sp.csr_matrix((csr[2].copy(), csr[1].copy(), csr[0].copy()), shape=(n, n))
    A.sum_duplicates()
    return A


def _rows_of(A, b, e, count=11):
    sl = A[b:e]
    return _Case((sl.indptr.astype(np.int64), sl.indices.astype(np.int32), sl.data.copy()), A.shape[1], b, count)


def _passes(npairs, wide):
    """Interleave width K of the pass each operand of an npairs call goes through (spmm_shift_pairs_impl's chunking)."""
    out, p0 = [], 0
    while p0 < npairs:
        left = npairs - p0
        np_ = min(left, 8) if (wide == 8 and left > 4) else min(left, 4)
        out += [4 if np_ <= 2 else 8 if np_ <= 4 else 16] * np_
        p0 += np_
    return out


class _Worst:
    """Worst error / bound per (form, K) of one test, printed when the test is through."""

    def __init__(self, title):
        self.title, self.r = title, {}

    def add(self, key, r):
        self.r[key] = max(self.r.get(key, 0.0), r)

    def report(self):
        print(f"\ncomplex-shift products, {self.title}: max error / bound " +
              ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.r.items())))


def _check(hip, case, label, p, z, sign, y, worst, key):
    """One operand's result (yr, yi buffers) against reference and bound on every row, both halves."""
    ref_r, ref_i, br, bi = case.ref(p, z, sign)
    got = [hip.HipVector(h).array for h in y]
    ratio = 0.0
    for half, g, ref, b in (("re", got[0], ref_r, br), ("im", got[1], ref_i, bi)):
        assert g.shape == b.shape
        r = pc.error_ratio(g, ref, b)
        ratio = max(ratio, r)
        if r > 1.0:
            err = np.abs(g.astype(np.longdouble) - ref).astype(np.float64)
            row = int(np.argmax(np.where(np.isfinite(err), err / b, np.inf)))
            raise AssertionError(f"{label} sign={sign:+.0f} operand {p} z={complex(z)} {half} half: worst error / bound "
                                 f"{r:.3g} at row {row} ({int(np.sum(~(err <= b)))} rows over)")
    worst.add(key, ratio)
    if sign != 0 and case.empty.any():
        # a row that stores nothing holds sign * z * x alone, to the roundings of the shift terms: nothing was added
        o, z = case.row_offset, complex(z)
        vr, vi = (np.abs(h[o:o + case.nrows])[case.empty] for h in case.X[p])
        for g, ref, own, other in ((got[0], ref_r, vr, vi), (got[1], ref_i, vi, vr)):
            err = np.abs(g[case.empty].astype(np.longdouble) - ref[case.empty]).astype(np.float64)
            assert np.all(err <= 1.01 * U * (3 * abs(z.real) * own + 2 * abs(z.imag) * other) + 1e-300), \
                f"{label} sign={sign:+.0f} operand {p} z={z}: an empty row holds more than its shift term"
    return ratio


def _shifts_for(npairs, sign, per_operand):
    """A shift per operand, cycled through the set so that neighbours differ by orders of magnitude; or one shift for the
    block, another for every (npairs, sign)."""
    if per_operand:
        return [SHIFTS[(p + npairs) % len(SHIFTS)] for p in range(npairs)]
    return [SHIFTS[(npairs + (0 if sign > 0 else 3)) % len(SHIFTS)]] * npairs


def _run_block_forms(hip, H, case, Xd, npairs_list, wide, worst, label, modes=(False, True), after=None):
    for npairs in npairs_list:
        Ks = _passes(npairs, wide)
        for sign in SIGNS:
            for per_operand in modes:
                zs = _shifts_for(npairs, sign, per_operand)
                ys = H.apply_shifted_pairs(zs if per_operand else zs[0], Xd[:npairs], reverse=sign < 0)
                if after is not None and npairs > 1:
                    after()
                form = "single pair" if npairs == 1 else "pairs_z" if per_operand else "pairs"
                for p in range(npairs):
                    K = 2 if npairs == 1 else Ks[p]
                    _check(hip, case, f"{label} {form} npairs={npairs} K={K}", p, zs[p], sign, ys[p], worst, f"{form} K={K}")


# ---------------------------------------------------------------- a. block forms on the ragged operator
@pytest.mark.parametrize("width", ["4", "8"])
@pytest.mark.parametrize("variant", [1, 2])
def test_block_forms_on_the_ragged_operator(hip, monkeypatch, variant, width):
    """n = 3001: empty, 300-entry, unsorted and duplicate-column rows; 1..11 operands (passes of width 4, 8 and 16, every
    remainder, the single-operand fallback), one shift and a shift per operand, both signs, both block kernels - the
    window-blocked one on 6 windows of 512 columns and 82 row blocks of 37 rows."""
    monkeypatch.setenv("HIPEIG_BCOO_WBITS", "9")
    monkeypatch.setenv("HIPEIG_BCOO_RW", "37")
    monkeypatch.setenv("HIPEIG_PAIR_BLOCK_WIDTH", width)
    case = _ragged()
    H = case.operator(hip)
    H.set_block_variant(variant)

    def geometry():
        info = H.block_info()
        if variant == 1:
            assert info["variant"] == "row-owner"
        else:
            assert info == {"variant": "column-window-blocked", "row_blocks": 82, "windows": 6, "rows_per_block": 37}

    worst = _Worst(f"ragged n={N} variant {variant} width {width}")
    _run_block_forms(hip, H, case, case.upload(hip), range(1, 12), int(width), worst, f"variant {variant} width {width}",
                     after=geometry)
    worst.report()
    wanted = {"4": {4, 8}, "8": {4, 8, 16}}[width]
    assert {k for k in worst.r if k.startswith("pairs_z")} == {f"pairs_z K={K}" for K in wanted}


def test_block_forms_with_the_automatic_kernel_choice(hip):
    """The same operator left to the automatic choice: the operand block fits one L2, so the row-owner kernel."""
    case = _ragged()
    H = case.operator(hip)
    worst = _Worst(f"ragged n={N} automatic")

    def picked():
        assert H.block_info()["variant"] == "row-owner"

    _run_block_forms(hip, H, case, case.upload(hip, 8), (2, 3, 8), 4, worst, "automatic", after=picked)
    worst.report()


# ---------------------------------------------------------------- b. a row slab applied to full-length operands
def _slab(raw):
    if raw:                                  # rows 100..2899 of the arrays as they are: duplicates and unsorted columns kept
        def build():
            rp, c, v = _ragged().csr
            return _Case((rp[100:2901] - rp[100], c[rp[100]:rp[2900]].copy(), v[rp[100]:rp[2900]].copy()), N, 100)
        return _case("ragged slab, raw arrays", build)
    return _case("ragged slab, summed", lambda: _rows_of(_summed(_ragged().csr, N), 100, 2900))


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("variant", [1, 2])
def test_block_forms_on_a_row_slab(hip, monkeypatch, variant, raw):
    """Rows 100..2899 applied to full-length operands: the sums gather from the whole block, the shift term reads the
    block from row 100 on.  from_scipy of the summed matrix, and the raw arrays with row_offset = 100."""
    monkeypatch.setenv("HIPEIG_BCOO_WBITS", "9")
    monkeypatch.setenv("HIPEIG_BCOO_RW", "37")
    monkeypatch.setenv("HIPEIG_PAIR_BLOCK_WIDTH", "8")
    case = _slab(raw)
    assert case.nrows == 2800 and case.row_offset == 100 and case.empty.any()
    H = case.operator(hip) if raw else hip.HipCsrOperator.from_scipy(_summed(_ragged().csr, N), 100, 2900)
    assert (H.nrows, H.ncols, H.row_offset) == (2800, N, 100)
    if not raw:
        A = H.to_scipy()
        assert np.array_equal(A.indptr, case.csr[0]) and np.array_equal(A.indices, case.csr[1]) and np.array_equal(A.data, case.csr[2])
    H.set_block_variant(variant)

    def geometry():
        info = H.block_info()
        if variant == 1:
            assert info["variant"] == "row-owner"
        else:
            assert info == {"variant": "column-window-blocked", "row_blocks": 76, "windows": 6, "rows_per_block": 37}

    worst = _Worst(f"slab rows 100..2899 variant {variant} {'raw' if raw else 'summed'}")
    _run_block_forms(hip, H, case, case.upload(hip, 8), (2, 4, 5, 8), 8, worst, f"slab variant {variant}", modes=(True,),
                     after=geometry)
    worst.report()


def _single_pair(hip, H, case, Xd, worst, label, key, fused, plain=True):
    """apply_shifted_pair with every shift of the set and both signs (an operand per shift), and the plain product."""
    ctx = H.ctx
    for k, z in enumerate(SHIFTS):
        for sign in SIGNS:
            y = (ctx.alloc(case.nrows), ctx.alloc(case.nrows))
            H.apply_shifted_pair(z, *Xd[k], *y, reverse=sign < 0)
            info = H.pair_info()
            assert info["fused"] == bool(fused), f"{label}: fused={info['fused']}"
            if fused and fused > 1:
                assert info["launches"] >= 2
            _check(hip, case, label, k, z, sign, y, worst, key)
    if plain:
        y = (ctx.alloc(case.nrows), ctx.alloc(case.nrows))
        H.apply_pair(*Xd[1], *y)
        assert H.pair_info()["fused"] == bool(fused)
        _check(hip, case, label + " plain product", 1, 0j, 0.0, y, worst, key + " plain")
        for h in y:
            assert np.all(hip.HipVector(h).array[case.empty] == 0.0)


@pytest.mark.parametrize("form", ["fused", "two sweeps"])
def test_single_pair_product_on_the_row_slab(hip, monkeypatch, form):
    """hipeig_spmv_shift_pair on the summed slab in both of its forms: the pair sweep (44 units of 64 rows, 3 windows) and
    the two real sweeps with their axpby on x + row_offset."""
    for k, v in SMALL_UNITS.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HIPEIG_PAIR_SWEEP", "1" if form == "fused" else "0")
    case = _slab(False)
    H = hip.HipCsrOperator.from_scipy(_summed(_ragged().csr, N), 100, 2900)
    if form == "fused":
        H.set_variant(4)
    worst = _Worst(f"slab rows 100..2899, single pair, {form}")
    _single_pair(hip, H, case, case.upload(hip, len(SHIFTS)), worst, f"slab {form}", form, fused=form == "fused")
    worst.report()


# ---------------------------------------------------------------- c. more row blocks than CUs
def test_block_forms_with_more_row_blocks_than_cus(hip, monkeypatch):
    """8-row blocks on n = 4001: 501 row blocks, a second sweep launch on anything with fewer CUs, for K = 4, 8 and 16."""
    monkeypatch.setenv("HIPEIG_BCOO_RW", "8")
    monkeypatch.setenv("HIPEIG_BCOO_WBITS", "9")
    monkeypatch.setenv("HIPEIG_PAIR_BLOCK_WIDTH", "8")
    n = 4001
    case = _case("ragged 4001", lambda: _Case(pc.ragged_csr(n, 5, duplicates=True), n))
    H = case.operator(hip)
    H.set_block_variant(2)

    def geometry():
        info = H.block_info()
        assert info == {"variant": "column-window-blocked", "row_blocks": 501, "windows": 8, "rows_per_block": 8}
        assert info["row_blocks"] > H.ctx.device_info()["cus"]

    worst = _Worst(f"ragged n={n}, 501 row blocks")
    _run_block_forms(hip, H, case, case.upload(hip), (2, 4, 8, 11), 8, worst, "two launches", modes=(True,), after=geometry)
    worst.report()
    assert set(worst.r) == {"pairs_z K=4", "pairs_z K=8", "pairs_z K=16"}


# ---------------------------------------------------------------- d. the pair sweep on small tiles, with shifts
def _edge_case(hip, slab):
    cus = hip.HipContext.default().device_info()["cus"]
    n = 64 * cus + 3001                                  # cus + 47 units of 64 rows: one workgroup per CU and launch -> two launches
    A = _case(("edge matrix", n), lambda: pc.edge_matrix(n, seed=3))
    b, e = (128, n - 37) if slab else (0, n)             # the slab keeps more than 64 * cus rows
    return A, b, e, _case(("edge", n, slab), lambda: _rows_of(A, b, e, len(SHIFTS)))


@pytest.mark.parametrize("slab", [False, True])
def test_fused_pair_sweep_with_shifts_on_small_tiles(hip, monkeypatch, slab):
    """spmv_tcoow_pair_kernel with a shift where it was only run plain: tiles shorter than a batch, empty rows and empty
    row blocks, 1 Ki-column windows - and a second launch (unit_begin > 0), on the whole operator and on a row slab."""
    for k, v in SMALL_UNITS.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HIPEIG_PAIR_SWEEP", "1")
    monkeypatch.setenv("HIPEIG_TCOOW_WG_PER_LAUNCH_CU", "1")
    A, b, e, case = _edge_case(hip, slab)
    H = hip.HipCsrOperator.from_scipy(A, b, e)
    H.set_variant(4)
    worst = _Worst(f"edge matrix n={A.shape[0]} rows {b}..{e - 1}, fused pair sweep")
    _single_pair(hip, H, case, case.upload(hip), worst, "fused pair sweep", "fused", fused=2)
    worst.report()


@pytest.mark.parametrize("variant", [1, 4])
def test_two_sweep_form_on_small_tiles(hip, monkeypatch, variant):
    """The same operator and shifts with the pair sweep switched off: two real sweeps (CSR-vector; TCOO-W in two launches)
    and two axpby, under the same bound."""
    for k, v in SMALL_UNITS.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HIPEIG_PAIR_SWEEP", "0")
    monkeypatch.setenv("HIPEIG_TCOOW_WG_PER_LAUNCH_CU", "1")
    A, b, e, case = _edge_case(hip, False)
    H = hip.HipCsrOperator.from_scipy(A)
    H.set_variant(variant)
    worst = _Worst(f"edge matrix n={A.shape[0]}, two sweeps, variant {variant}")
    _single_pair(hip, H, case, case.upload(hip), worst, f"two sweeps variant {variant}", "two sweeps", fused=0)
    assert H.last_variant() == H.VARIANTS[variant]
    if variant == 4:
        assert H.launches_per_apply() >= 2
    worst.report()


# ---------------------------------------------------------------- e. the window-blocked kernel chosen automatically
def test_block_forms_on_a_window_blocked_operator(hip):
    """generate(100 003, 32) with nothing pinned: the automatic choice takes the window-blocked kernel (fp64 LDS atomics)
    for 4 and 8 operands; the reference is built from the operator's own arrays."""
    n = 100_003
    H = hip.HipCsrOperator.generate(n, 32, seed=7)

    def build():
        A = H.to_scipy().tocsr()
        return _Case((A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data), n, 0, 8)

    case = _case("generated 100003", build)
    worst = _Worst(f"generated n={n}, automatic")

    def picked():
        assert H.block_info()["variant"] == "column-window-blocked"

    _run_block_forms(hip, H, case, case.upload(hip), (4, 8), 4, worst, "generated", modes=(True,), after=picked)
    worst.report()
