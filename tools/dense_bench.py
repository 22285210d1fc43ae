#!/usr/bin/env python3
"""Dense layout timings (BASELINE config #1, the reference's dense-``A`` drivers): product, shifted product, one MINRES
iteration and the K = 8 block product of a dense symmetric operator, each with the automatic variant and with the dense
layout (variant 6 / block variant 3) on the SAME operator object in the same process.  HIP events, warm: ``--reps``
repetitions after ``--warmup``.  One JSON line per run; one n per process.

    python tools/dense_bench.py --n 8192  >> profiles/rNN_dense_layout.jsonl
    python tools/dense_bench.py --n 16384 >> profiles/rNN_dense_layout.jsonl
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_BYTES_PER_S = 8.0e12


def test_operator(n, seed=1212):
    """Symmetric, spectrum close to dense_test_matrix's linspace(1, 200, n) without its O(n^3) QR: that diagonal plus a
    symmetric random part of norm ~1, every entry non-zero."""
    import numpy as np
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n), dtype=np.float32).astype(np.float64)
    A += A.T
    A *= 0.25 / np.sqrt(n)
    A[np.diag_indices(n)] += np.linspace(1.0, 200.0, n)
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=-20.0)
    ap.add_argument("--rtol", type=float, default=1e-10)
    a = ap.parse_args()
    import numpy as np
    import eigensolvers_amd as ea
    ctx = ea.HipContext.default()
    n = a.n
    A = test_operator(n)
    H = ea.HipCsrOperator.from_dense(A)
    del A
    rng = np.random.default_rng(5)
    Q = rng.standard_normal((n, a.k))
    Q /= np.linalg.norm(Q, axis=0)
    opts = lambda: {"linearSystemArgs": {"linearSolver": "minres", "linearIter": 2000, "linear_tol": a.rtol}}
    X = [ea.HipVector(Q[:, j].copy(), opts()) for j in range(a.k)]
    y = ctx.alloc(n)
    alg = H.dense_algorithmic_bytes()
    out = {"n": n, "device": ctx.device_info()["name"], "reps": a.reps, "warmup": a.warmup, "k": a.k,
           "dense_algorithmic_bytes": alg, "csr_algorithmic_bytes": H.algorithmic_bytes()}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ctx.synchronize()
        ctx.timer_start()
        for _ in range(a.reps):
            fn()
        return ctx.timer_stop() / a.reps

    def solve_ms():
        """Milliseconds per MINRES iteration of one whole solve (set-up and the copies of the state record included)."""
        W = ea.HipVector.solve(H, X[0], a.sigma)                  # warm: workspaces, layouts
        ctx.synchronize()
        ctx.timer_start()
        W = ea.HipVector.solve(H, X[0], a.sigma)
        ms = ctx.timer_stop()
        its = W.last_solve_stats["iterations"]
        return ms / its, its, W.array

    results = {}
    for name, variant, block_variant in (("automatic", 0, 0), ("dense", 6, 3)):
        H.set_variant(variant)
        H.set_block_variant(block_variant)
        r = {}
        r["apply_ms"] = timed(lambda: H.apply(X[0]._buf, y))
        r["variant"] = H.last_variant()
        prod = ea.HipVector(y).array.copy()
        r["apply_shifted_ms"] = timed(lambda: H.apply_shifted(a.sigma, X[0]._buf, y))
        r["minres_iteration_ms"], r["minres_iterations"], sol = solve_ms()
        bufs = [x._buf for x in X]
        r["apply_block_ms_incl_pack_unpack"] = timed(lambda: H.apply_block(bufs))
        r["block_variant"] = H.block_info()["variant"]
        blk = ea.HipVector(H.apply_block(bufs)[a.k - 1]).array.copy()
        info = H.dense_info()                                     # refreshes device_bytes
        r["device_bytes"] = int(H.device_bytes)
        r["dense_copy_bytes"] = info["bytes"]
        r["workgroups"], r["block_workgroups"] = info["workgroups"], info["block_workgroups"]
        for key in ("apply_ms", "apply_shifted_ms"):
            r[key.replace("_ms", "_frac_of_8TBs")] = alg / (r[key] * 1e-3) / HBM_PEAK_BYTES_PER_S
        r["apply_block_frac_of_8TBs"] = (8 * n * n + 2 * 8 * n * a.k) / (r["apply_block_ms_incl_pack_unpack"] * 1e-3) / HBM_PEAK_BYTES_PER_S
        results[name] = (r, prod, sol, blk)
        out[name] = r
    (ra, pa, sa, ba), (rd, pd, sd, bd) = results["automatic"], results["dense"]
    out["max_rel_diff_product"] = float(np.max(np.abs(pa - pd)) / np.max(np.abs(pa)))
    out["max_rel_diff_block_product"] = float(np.max(np.abs(ba - bd)) / np.max(np.abs(ba)))
    out["max_rel_diff_solution"] = float(np.linalg.norm(sa - sd) / np.linalg.norm(sa))
    out["speedup_apply"] = ra["apply_ms"] / rd["apply_ms"]
    out["speedup_apply_block"] = ra["apply_block_ms_incl_pack_unpack"] / rd["apply_block_ms_incl_pack_unpack"]
    out["speedup_minres_iteration"] = ra["minres_iteration_ms"] / rd["minres_iteration_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
