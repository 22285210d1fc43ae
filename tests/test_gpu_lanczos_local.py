"""The passes of the Lanczos filter (``csrc/lanczos_filter.hip``) against extended precision, relation by relation.

Everything a FEAST filtered vector is made of is pinned here to the same quantity in ``longdouble``: ``beta_0`` and
``v_0``, the three-term relation per element, ``alpha_i`` as ``<v_i, w*>``, ``||v_{i+1}||``, the ``|tau|`` estimates and
stop steps, and the sums ``sum_i G[i, c] v_i`` - all of them *local*, evaluated from the device's own vectors and
scalars, so each has a proven bound however far the basis has drifted.  Reference, bounds and their derivation:
``tests/_lanczos_local.py``; ``tests/test_lanczos_local_cpu.py`` holds the host twins to the bounds and shows the faults
they catch.  The device's vectors are read through ``LanczosRun.combine`` with slices of the identity, which is exact.

The runs are capped at 24 to 40 steps by ``linearIter`` (``run.info`` then reports the limit), which keeps every case at
seconds; one converged run provides the masks.  A kept basis holds pass 1's own vectors, so relations a to d apply with
either sweep.  The product pass rebuilds its vectors on every call; with the row-owner sweep every call rebuilds the same
ones, so relation b is checked across calls there, and with the window-blocked sweep (add order not fixed, two calls two
sequences) the ring is held to the rotation only - its scalars are those of the kept run, which is held to a to d.
A prefix is read with the row-owner sweep for the same reason.

Every test prints its largest error / bound ratio (``-s`` shows it).
"""
import numpy as np
import pytest

import _lanczos_local as ll
from _lanczos_cases import LO, Z8, arrays, block_variant, device_columns, lf, same_scalars

pytestmark = pytest.mark.gpu

KNOBS = ("HIPEIG_LF_WIDTH", "HIPEIG_LF_SEGMENT", "HIPEIG_LF_CHUNK", "HIPEIG_LF_PER_THREAD", "HIPEIG_LF_PROBE",
         "HIPEIG_BCOO_RW", "HIPEIG_BCOO_WBITS")
RELATIONS = ("a_beta0", "a_v0", "b", "c", "d")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _device_operator(hip, name):
    if name == "gapped4000":
        return hip.HipCsrOperator.generate(4000, 32, seed=7)
    return hip.HipCsrOperator.from_scipy(ll.operator(name).A)


@pytest.fixture(scope="module")
def ops(hip):
    """name -> (device operator, its rows as the reference reads them), built once with the default geometry."""
    out = {}
    for name in ("tri100", "odd1037", "gapped4000"):
        Hd = _device_operator(hip, name)
        out[name] = (Hd, ll.Operator(Hd.to_scipy()))
    return out


def _run(hip, Hd, B, sign, maxiter, **kw):
    return hip.lanczos_run(Hd, device_columns(hip, B, *LO, maxiter), Z8, reverseGF=sign < 0, **kw)


def _trees(Hd, n, K, variant):
    info = Hd.block_info()
    assert info["variant"] == ("row-owner" if variant == 1 else "column-window-blocked"), info
    return ll.sweep_trees(n, K, variant, Hd.ctx.device_info()["cus"], info["rows_per_block"], info["row_blocks"])


class _Worst(dict):
    def add(self, key, r):
        self[key] = max(self.get(key, 0.0), float(r))

    def report(self, title):
        print(f"\nlanczos local, {title}: max error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.items())))


def _check_relations(label, op, B, V, scalars, trees, worst, which="abcd"):
    for r, b in enumerate(B):
        rel = ll.local_relations(op, b, V[r], scalars[r].alphas, scalars[r].betas, trees, which)
        for key, v in rel.items():
            worst.add(key, v)
            assert v <= 1.0, f"{label} column {r}: relation {key} at {v:.3g} of its bound ({len(V[r])} vectors)"


def _check_rotation(label, scalars, sign, worst):
    compared = left = 0
    for r, sc in enumerate(scalars):
        w, c, l, bad = ll.rotation_check(sc, Z8, sign, *LO)
        worst.add("rotation", w)
        compared, left = compared + c, left + l
        assert w <= 1.0, f"{label} column {r}: an estimate off by {w:.3g} delta"
        assert not bad, f"{label} column {r}: stop steps of shifts {bad} are not the reference's ({list(sc.iterations)})"
    assert 20 * left <= compared + left, f"{label}: {left} of {compared + left} (column, shift) pairs left out"


# ---------------------------------------------------------------- a - d and the rotation on a kept basis
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("name,k,sign,cap,width", [c + (0,) for c in ll.CAPPED] + [("odd1037", 3, 1.0, 32, 8)])
def test_relations_on_the_kept_basis(hip, ops, monkeypatch, name, k, sign, cap, width, variant):
    """Pass 1's own vectors (basis_mode 1): relations a to d and the rotation, both sweeps, k = 1, 3, 5, 8 and k = 3 on
    the wide interleave, both signs."""
    if width:
        monkeypatch.setenv("HIPEIG_LF_WIDTH", str(width))
    Hd, op = ops[name]
    B = ll.columns(name, k)
    K = 8 if (k > 4 or width == 8) else 4
    worst = _Worst()
    with block_variant(Hd, variant):
        run = _run(hip, Hd, B, sign, cap, keepBasis=True)
        assert run.basis_kept == [True] and run.sign == sign
        assert all(i in (0, cap) for i in run.info) and all(1 <= len(s.alphas) <= cap for s in run.scalars)
        trees = _trees(Hd, op.n, K, variant)
        V = ll.read_vectors(run)
        run.release()
    label = f"{name} k={k} sign={sign:+.0f} variant {variant}"
    _check_relations(label, op, B, V, run.scalars, trees, worst)
    _check_rotation(label, run.scalars, sign, worst)
    worst.report(f"{label} K={K} kept basis, {max(len(v) for v in V)} steps, trees {trees}")


def test_relations_with_more_row_blocks_than_cus(hip, monkeypatch):
    """gapped4000 in 8-row blocks and 512-column windows: 500 row blocks, so a second sweep launch whose partials lie
    behind the first's, on anything with fewer CUs."""
    monkeypatch.setenv("HIPEIG_BCOO_RW", "8")
    monkeypatch.setenv("HIPEIG_BCOO_WBITS", "9")
    Hd = _device_operator(hip, "gapped4000")
    op = ll.Operator(Hd.to_scipy())
    B, sign, cap = ll.columns("gapped4000", 5), 1.0, 24
    worst = _Worst()
    with block_variant(Hd, 2):
        run = _run(hip, Hd, B, sign, cap, keepBasis=True)
        info = Hd.block_info()
        assert info["row_blocks"] == 500 and info["rows_per_block"] == 8 and info["windows"] == 8, info
        assert info["row_blocks"] > Hd.ctx.device_info()["cus"]
        trees = _trees(Hd, op.n, 8, 2)
        V = ll.read_vectors(run)
        run.release()
    _check_relations("500 row blocks", op, B, V, run.scalars, trees, worst)
    _check_rotation("500 row blocks", run.scalars, sign, worst)
    worst.report(f"gapped4000 k=5, 500 row blocks, trees {trees}")


# ---------------------------------------------------------------- the ring: the vectors the product pass rebuilds
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("name,k,sign,cap", [("tri100", 3, -1.0, 24), ("odd1037", 5, 1.0, 40), ("gapped4000", 8, 1.0, 33)])
def test_the_ring_and_the_product_pass(hip, ops, name, k, sign, cap, variant):
    """basis_mode 0: the rotation on the run's scalars; with the row-owner sweep also relation b on the vectors pass 2
    rebuilds, two per call."""
    Hd, op = ops[name]
    B = ll.columns(name, k)
    worst = _Worst()
    label = f"{name} k={k} sign={sign:+.0f} variant {variant} ring"
    with block_variant(Hd, variant):
        run = _run(hip, Hd, B, sign, cap)
        assert run.basis_vectors == [0]
        if variant == 1:
            V = ll.read_vectors(run)
            assert run.products_pass2 == [max(len(v) for v in V) - 1]
            _check_relations(label, op, B, V, run.scalars, _trees(Hd, op.n, 4 if k <= 4 else 8, 1), worst, which="b")
    _check_rotation(label, run.scalars, sign, worst)
    worst.report(label)


# ---------------------------------------------------------------- masks
@pytest.mark.parametrize("variant", [1, 2])
def test_masks(hip, ops, variant):
    """A random column, a sum of 6 eigenvectors and a zero column in one block, run to convergence: the relations hold up
    to each column's own last step (the second column's last steps lie next to a breakdown), a stopped column reads back
    as zeros (``read_vectors`` asserts it), and tables shorter than the steps run give the same vectors."""
    Hd, op = ops["odd1037"]
    B = ll.masking_columns()
    worst = _Worst()
    with block_variant(Hd, variant):
        run = _run(hip, Hd, B, 1.0, ll.MASKS_STEPS, keepBasis=True)
        assert run.converged and run.basis_kept == [True]
        steps = [len(s.alphas) for s in run.scalars]
        assert steps[0] >= 10 * steps[1] and 3 <= steps[1] <= 7 and steps[2] == 0, steps
        trees = _trees(Hd, op.n, 4, variant)
        V = ll.read_vectors(run)
        short = ll.read_vectors(run, [steps[0] // 2, steps[1] - 1, 0])
        G = ll.tables([steps[0] - 9, steps[1] - 2, 0], 3, seed=variant)
        q = run.combine(G)
        run.release()
    assert [len(v) for v in V] == steps
    for r in range(3):
        assert np.array_equal(short[r], V[r][:len(short[r])])
        worst.add("combination", ll.combine_check(V[r], G[r], np.array(arrays(q[r]))))
    assert worst["combination"] <= 1.0, worst
    label = f"masks variant {variant}"
    _check_relations(label, op, B, V, run.scalars, trees, worst)
    _check_rotation(label, run.scalars, 1.0, worst)
    worst.report(f"{label}, steps {steps}")


# ---------------------------------------------------------------- combinations
def _as_rows(out, nc):
    """``combine``'s result of one column as ``[NC, n]``."""
    if nc == 1:
        return out.array[None, :]
    if nc == 2:
        return np.array([out.re.array, out.im.array])
    return np.array(arrays(out))


def _check_combinations(label, run, V, ncs, worst, cuts=(0, 3), stream32=None):
    steps = [len(v) for v in V]
    for nc in ncs:
        for cut in cuts:
            ms = [max(m - cut * (r + 1), 0) for r, m in enumerate(steps)]        # cut > 0: every column ends elsewhere
            G = ll.tables(ms, nc, seed=cut)
            out = run.combine(G)
            for r in range(len(V)):
                s32 = 0 if stream32 is None else min(stream32, ms[r])
                ratio = ll.combine_check(V[r], G[r], _as_rows(out[r], nc), s32)
                worst.add(f"NC={nc}", ratio)
                assert ratio <= 1.0, f"{label} NC={nc} column {r} of {ms} terms: {ratio:.3g} of the bound"


PATHS = {"stream": (None, None), "product pass": (None, None), "prefix p=1": (1, 1), "prefix p=2": (1, 2), "prefix p=10": (5, 10)}


@pytest.mark.parametrize("path", list(PATHS))
def test_combinations(hip, ops, monkeypatch, path):
    """NC = 1, 2, 3, 8 and 11 (8 + 2 + 1) through the stream over a whole basis, the product pass (NC <= 2) and prefixes
    with the seam at p = 1, 2 and mid-run, full tables and tables that end at another step in every column; behind a
    prefix also relations a to d on what the stream and the recurrence behind the seam hand back."""
    name, k, sign, cap = "odd1037", 5, 1.0, 40
    Hd, op = ops[name]
    B = ll.columns(name, k)
    seg, p = PATHS[path]
    worst = _Worst()
    if seg:
        monkeypatch.setenv("HIPEIG_LF_SEGMENT", str(seg))
    with block_variant(Hd, 1):
        if path == "product pass":
            run = _run(hip, Hd, B, sign, cap)
        elif path == "stream":
            run = _run(hip, Hd, B, sign, cap, keepBasis=True)
            assert run.basis_kept == [True]
        else:
            run = _run(hip, Hd, B, sign, cap, keepBasis=True, keepPrefix=True, basisBytes=p * lf.basis_slot_bytes(op.n, k) + 100)
            assert run.basis_vectors == [p] and run.basis_kept == [False]
        V = ll.read_vectors(run)
        assert [len(v) for v in V] == [cap] * k
        if seg:
            assert run.products_pass2 == [cap - p]
            _check_relations(path, op, B, V, run.scalars, _trees(Hd, op.n, 8, 1), worst)
        _check_combinations(path, run, V, (1, 2) if path == "product pass" else (1, 2, 3, 8, 11), worst)
        run.release()
    worst.report(f"combinations, {path}")


@pytest.mark.parametrize("seg", [1, 3])
def test_the_stream_across_its_staging_boundary(hip, ops, monkeypatch, seg):
    """31, 32 and 33 terms from segments of 1 and 3 slots: the stream stages 32 steps of coefficients and slot pointers
    at a time (LF_BC_STEPS)."""
    name, k, sign, cap = "odd1037", 3, -1.0, 36
    Hd, op = ops[name]
    B = ll.columns(name, k)
    monkeypatch.setenv("HIPEIG_LF_SEGMENT", str(seg))
    worst = _Worst()
    with block_variant(Hd, 1):
        run = _run(hip, Hd, B, sign, cap, keepBasis=True)
        assert run.basis_kept == [True] and run.basis_vectors == [cap]
        V = ll.read_vectors(run)
        for m in (31, 32, 33):
            for nc in (1, 8):
                G = ll.tables([m, m - 1, m + 1], nc, seed=m)
                out = run.combine(G)
                assert run.products_pass2 == [0]
                for r in range(k):
                    ratio = ll.combine_check(V[r], G[r], _as_rows(out[r], nc))
                    worst.add(f"m={m}", ratio)
                    assert ratio <= 1.0, (seg, m, nc, r, ratio)
        run.release()
    worst.report(f"stream across the staging boundary, segments of {seg}")


# ---------------------------------------------------------------- the fp32 basis
@pytest.mark.parametrize("k", [3, 8])
def test_the_fp32_basis(hip, ops, monkeypatch, k):
    """basis_mode 3 and 4 with the row-owner sweep, whose fp64 run has the same vectors bit for bit: a stored vector read
    back against the fp64 one per element, the combination with the fp32 term on the stream's share, and behind a prefix
    the vectors from the seam on - rebuilt from the fp64 hand-over vectors - equal to the fp64 run's."""
    name, sign, cap, p = "odd1037", 1.0, 32, 10
    Hd, op = ops[name]
    B = ll.columns(name, k)
    worst = _Worst()
    with block_variant(Hd, 1):
        run64 = _run(hip, Hd, B, sign, cap, keepBasis=True)
        V64 = ll.read_vectors(run64)
        run64.release()
        run32 = _run(hip, Hd, B, sign, cap, keepBasis=True, basisPrecision="fp32")
        assert run32.basis_kept == [True] and run32.basis_element_bytes == [4] and same_scalars(run64.scalars, run32.scalars)
        V32 = ll.read_vectors(run32)
        for r in range(k):
            assert not np.array_equal(V32[r], V64[r])
            worst.add("stored", ll.stored_check(V32[r], V64[r]))
        assert worst["stored"] <= 1.0, worst
        _check_combinations("fp32 basis", run32, V64, (1, 3, 8), worst, stream32=cap)
        run32.release()
        monkeypatch.setenv("HIPEIG_LF_SEGMENT", "5")
        pre = _run(hip, Hd, B, sign, cap, keepBasis=True, keepPrefix=True, basisPrecision="fp32",
                   basisBytes=p * lf.basis_slot_bytes(op.n, k, "fp32") + 100)
        assert pre.basis_vectors == [p] and pre.basis_kept == [False] and same_scalars(run64.scalars, pre.scalars)
        Vp = ll.read_vectors(pre)
        assert pre.products_pass2 == [cap - p]
        for r in range(k):
            worst.add("stored, prefix", ll.stored_check(Vp[r][:p - 1], V64[r][:p - 1]))
            assert np.array_equal(Vp[r][p - 1:], V64[r][p - 1:]), f"column {r}: vectors behind the seam differ from the fp64 run's"
        assert worst["stored, prefix"] <= 1.0, worst
        _check_combinations("fp32 prefix", pre, V64, (2, 8), worst, stream32=p - 1)
        pre.release()
    worst.report(f"fp32 basis k={k}")
