"""The lane-major (index, value) stream of the workgroup-unit blocked layout (TCOO-W, variants 4 / 5 and the pair
sweep): every 256-slot batch is stored lane-major and every range a wave starts on begins on a batch boundary, so that
a lane loads its four indices with one 16-byte load and its four values with two.  These operators hit the edges of
that layout - tiles shorter than one instruction group or one batch, empty rows and empty row blocks, streams that end
inside a batch, column-split shares, the runs of the overlapped multi-rank sweep - and every product is checked
against the CSR-vector kernel (variant 1), which reads the plain CSR arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _product_cases import edge_matrix as _edge_matrix
from _sweep_cases import fixed_point_term, product_bound as _bound
from conftest import REPO
from eigensolvers_amd.distributed import LoopbackGroup, row_range

pytestmark = pytest.mark.gpu

SMALL_UNITS = {"HIPEIG_TCOOW_RW": "64", "HIPEIG_TCOOW_WBITS": "10", "HIPEIG_TCOOW_PAIR_RW": "64",
               "HIPEIG_TCOOW_PAIR_WBITS": "10"}


def _product(hip, H, x, variant):
    H.set_variant(variant)
    return hip.HipVector(x).applyOp(H).array


@pytest.mark.parametrize("N", [3001, 20000])
def test_small_tiles_empty_rows_and_units(hip, monkeypatch, N):
    for k, v in SMALL_UNITS.items():
        monkeypatch.setenv(k, v)
    A = _edge_matrix(N, seed=N)
    assert A.nnz % 256 != 0                                  # the stream ends inside a batch
    H = hip.HipCsrOperator.from_scipy(A)
    x = np.random.default_rng(1).standard_normal(N)
    ref = _product(hip, H, x, 1)
    y = _product(hip, H, x, 4)
    assert H.last_variant() == "column-window-blocked(workgroup)"
    lay = H.layout_info()
    assert lay["rows_per_block"] == 64 and lay["window_bits"] == 10 and lay["row_blocks"] == -(-N // 64)
    assert np.all(np.abs(y - ref) <= _bound(A, x))
    assert np.all(y[128:256] == 0.0) and np.all(y[::7] == 0.0)
    assert np.all(np.abs(ref - A @ x) <= _bound(A, x))
    # fused shift through the same sweep
    ctx = hip.HipContext.default()
    ys = ctx.alloc(N)
    H.apply_shifted(0.02, hip.HipVector(x)._buf, ys, reverse=True)
    assert np.all(np.abs(hip.HipVector(ys).array - (A @ x - 0.02 * x)) <= _bound(A, x) + 1e-16 * np.abs(x))


def test_pair_sweep_on_small_tiles(hip, monkeypatch):
    for k, v in SMALL_UNITS.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HIPEIG_PAIR_SWEEP", "1")
    N = 20000
    A = _edge_matrix(N, seed=3)
    H = hip.HipCsrOperator.from_scipy(A)
    rng = np.random.default_rng(2)
    xr, xi = rng.standard_normal(N), rng.standard_normal(N)
    ref_r, ref_i = _product(hip, H, xr, 1), _product(hip, H, xi, 1)
    H.set_variant(4)
    ctx = hip.HipContext.default()
    yr, yi = ctx.alloc(N), ctx.alloc(N)
    H.apply_pair(hip.HipVector(xr)._buf, hip.HipVector(xi)._buf, yr, yi)
    assert H.pair_info()["fused"], "the pair sweep was not taken"
    assert np.all(np.abs(hip.HipVector(yr).array - ref_r) <= _bound(A, xr))
    assert np.all(np.abs(hip.HipVector(yi).array - ref_i) <= _bound(A, xi))


def test_fixed_point_is_bitwise_equal_across_layout_builds(hip, monkeypatch):
    for k, v in SMALL_UNITS.items():
        monkeypatch.setenv(k, v)
    N = 20000
    A = _edge_matrix(N, seed=5)
    x = np.random.default_rng(4).standard_normal(N)
    outs = []
    for _ in range(2):                                       # two separately built layouts (atomic slot cursors)
        H = hip.HipCsrOperator.from_scipy(A)
        ref = _product(hip, H, x, 1)
        y = _product(hip, H, x, 5)
        assert H.last_variant() == "column-window-blocked(workgroup, fixed-point)"
        np.testing.assert_array_equal(y, _product(hip, H, x, 5))
        assert np.all(np.abs(y - ref) <= _bound(A, x) + fixed_point_term(A, x))
        outs.append(y)
    np.testing.assert_array_equal(outs[0], outs[1])


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import eigensolvers_amd as ea
N = int(sys.argv[2])
H = ea.HipCsrOperator.generate(N, 32, seed=9)
x = np.random.default_rng(8).standard_normal(N)
H.set_variant(1)
ref = ea.HipVector(x).applyOp(H).array
out = {}
for v in (4, 5):
    H.set_variant(v)
    y = ea.HipVector(x).applyOp(H).array
    out[f"err{v}"] = float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))
    out[f"layout{v}"] = H.layout_info()
print(json.dumps(out))
"""


@pytest.mark.parametrize("csplit", [2, 3, 5])
def test_column_split_shares_in_a_child_process(csplit):
    """Column splits through the environment of a fresh process: each workgroup's share of a row block's stream is cut
    at a batch multiple, whatever the number of shares."""
    env = dict(os.environ, HIPEIG_TCOOW_CSPLIT=str(csplit))
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO, "300000"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    o = json.loads(r.stdout.strip().splitlines()[-1])
    for v in (4, 5):
        assert o[f"layout{v}"]["column_splits"] == csplit
        assert o[f"err{v}"] < 1e-13, (v, o)


@pytest.mark.parametrize("csplit", [None, 3])
def test_loopback_ranks_with_small_windows(hip, monkeypatch, csplit):
    """Three loopback ranks, 1 Ki-column windows and 64-row blocks: every window of a slab starts a batch (any of them
    can begin a run of the overlapped plan), runs of local and remote windows are swept by separate launches."""
    N, P = 30011, 3
    for k, v in SMALL_UNITS.items():
        monkeypatch.setenv(k, v)
    if csplit:
        monkeypatch.setenv("HIPEIG_TCOOW_CSPLIT", str(csplit))
    A = _edge_matrix(N, seed=11)
    x = np.random.default_rng(12).standard_normal(N)
    ref = A @ x
    bound = _bound(A, x)
    grp = LoopbackGroup(P)

    def body(rank, ctx):
        b, e = row_range(N, P, rank)
        H = hip.HipCsrOperator.from_scipy(A, row_begin=b, row_end=e, ctx=ctx)
        out = {}
        for variant in (1, 4, 5):
            H.set_variant(variant)
            out[variant] = hip.HipVector(x[b:e], ctx=ctx).applyOp(H).array
        H.set_variant(4)
        out["layout"] = H.layout_info()
        return out

    try:
        res = grp.run(body)
    finally:
        grp.close()
    for r, o in enumerate(res):
        b, e = row_range(N, P, r)
        assert o["layout"]["column_splits"] == (csplit or 1)
        for variant in (1, 4):
            assert np.all(np.abs(o[variant] - ref[b:e]) <= bound[b:e]), (r, variant)
        assert np.all(np.abs(o[5] - ref[b:e]) <= bound[b:e] + fixed_point_term(A, x))


@pytest.mark.parametrize("N,nnz_row", [(1_000_000, 32), (10_000_000, 64)])
def test_padding_of_the_stream(hip, N, nnz_row):
    """Slots per non-zero of the stream (padding: bins kept inside one 64-lane instruction group, ~1.8 %, plus the
    batch-aligned row block starts) at the sizes of the inner solves and of the headline product."""
    H = hip.HipCsrOperator.generate(N, nnz_row, seed=7)
    H.set_variant(4)
    x = hip.HipVector(np.ones(N))
    x.applyOp(H)
    lay = H.layout_info()
    assert lay["variant"] == 4
    assert 1.0 < lay["padding"] <= 1.025, lay
