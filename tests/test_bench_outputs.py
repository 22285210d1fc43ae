"""`bench.py --dump-outputs DIR`: the product of the last timed step, y = sigma*x - H x, written as float64 - every row
while they fit the bound, beyond it a fixed seeded sample of rows - and a plain run whose JSON line carries the headline
figure alone (what takes runs of its own is behind --full)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_module", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dumped_rows_are_fixed_sorted_and_within_the_bound():
    from eigensolvers_amd import distributed as D
    bench = _bench_module()
    assert bench.dump_rows(bench.DUMP_MAX_VALUES) is None                    # small products are written whole
    N = 10_000_000                                                           # the headline size
    rows = bench.dump_rows(N)
    assert rows.size == bench.DUMP_MAX_VALUES and rows.size * 8 <= 64e6
    assert rows[0] >= 0 and rows[-1] < N and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, bench.dump_rows(N))                          # the same rows in every run
    parts = []                                                               # the ranks' shares, in rank order, are the sample
    for r in range(3):
        b, e = D.row_range(N, 3, r)
        parts.append(rows[(rows >= b) & (rows < e)])
    assert np.array_equal(np.concatenate(parts), rows)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_dumps_the_product_of_its_last_step(hip, tmp_path):
    bench = _bench_module()
    N, nnz_row, sigma = 4_500_000, 8, 0.02                                    # N > DUMP_MAX_VALUES: the sampled path
    r = subprocess.run([sys.executable, BENCH, "--n", str(N), "--nnz-row", str(nnz_row), "--sigma", str(sigma),
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "GB/s" and out["dtype"] == "f64" and out["higher_is_better"] is True
    assert not {"lanczos", "block8", "minres_n1e6", "cpu_baseline", "phases"} & set(out)
    assert "single_step_ms_median" not in out["roofline"] and "measured_stream_GBs" not in out["roofline"]

    assert sorted(os.listdir(tmp_path)) == ["y_sample.npy"]
    y = np.load(tmp_path / "y_sample.npy")
    rows = bench.dump_rows(N)
    assert y.dtype == np.float64 and y.shape == rows.shape
    Hs = hip.HipCsrOperator.generate(N, nnz_row, seed=7).to_scipy()[rows]    # bench.py's operator and operand
    x = np.random.default_rng(100).standard_normal(N)
    want = sigma * x[rows] - Hs @ x
    scale = abs(Hs) @ abs(x) + sigma * abs(x[rows])
    assert np.all(np.abs(y - want) <= 1e-13 * scale)
