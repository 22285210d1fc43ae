#!/usr/bin/env python3
"""Lock-step GCROT solves with a real shift (HipVector._solve_real_block, called directly: the widths below solveBlock's
dispatch threshold are measured too) against the one-by-one solves (HipVector.solve per right-hand side, what
options["blockSolve"] = False gives) on the same right-hand sides: wall time per block solve, products, operator passes
and device calls (products + Arnoldi step calls / batches).  The two modes alternate, one run of each per repetition, and
every row is printed (one JSON line) as soon as it is measured; the first line describes the device.

    python tools/gcrot_block_bench.py [--configs dense100,gapped4000,gen1e6 --blocks 3,8] > profiles/NN_gcrot_block.jsonl
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="dense100,gapped4000,gen1e6")
    ap.add_argument("--blocks", default="3,8")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import eigensolvers_amd as ea
    from eigensolvers_amd import gcrotmk as G
    from eigensolvers_amd.generators import dense_test_matrix, gapped_csr_host

    ctx = ea.HipContext.default()
    counts = {}

    def counting(owner, name, key):
        fn = getattr(owner, name)

        def wrapped(*args, **kw):
            counts[key] = counts.get(key, 0) + 1
            return fn(*args, **kw)
        setattr(owner, name, staticmethod(wrapped) if isinstance(owner.__dict__[name], staticmethod) else wrapped)

    counting(ea.HipCsrOperator, "apply_shifted", "single_products")
    counting(ea.HipCsrOperator, "apply_shifted_block", "block_products")
    counting(G._Ops, "arnoldi_step", "arnoldi_steps")
    counting(G._Ops, "arnoldi_begin", "arnoldi_split_steps")
    counting(G._Ops, "arnoldi_begin_batch", "arnoldi_batches")

    # (operator, shift, rtol) as the reference's tests and BASELINE's configurations use them
    def make(name):
        if name == "dense100":
            A, ev = dense_test_matrix(100, 1212)
            return ea.HipCsrOperator.from_dense(A), float(ev[5]) + 1.5, 1e-4
        if name == "gapped4000":
            return ea.HipCsrOperator.from_scipy(gapped_csr_host(4000, 32, seed=7)), 0.02, 1e-8
        if name == "gen1e6":
            return ea.HipCsrOperator.generate(1_000_000, 32, seed=7), 0.02, 1e-8
        raise SystemExit(f"unknown config {name}")

    print(json.dumps({"device": ctx.device_info()["name"], "reps": a.reps}), flush=True)
    for name in a.configs.split(","):
        H, sigma, rtol = make(name)
        n = H.nrows
        for k in [int(x) for x in a.blocks.split(",")]:
            Q = np.random.default_rng(5).standard_normal((n, k))
            Q /= np.linalg.norm(Q, axis=0)
            opts = {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 4000, "linear_tol": rtol, "linear_atol": 0.0}}
            bs = [ea.HipVector(Q[:, j].copy(), opts) for j in range(k)]
            runs = {
                "one_by_one": lambda: [ea.HipVector.solve(H, b, sigma) for b in bs],
                "lock_step": lambda: ea.HipVector._solve_real_block(H, bs, sigma, opts["linearSystemArgs"], False),
            }
            row = {"config": name, "N": n, "nnz": int(H.nnz), "nBlock": k, "sigma": sigma, "rtol": rtol}
            ts = {m: [] for m in runs}
            prods = {m: [] for m in runs}                   # products per repetition (the count moves with rounding)
            last = {}
            for m, fn in runs.items():                  # warm-up (layouts, workspaces)
                fn()
                ctx.synchronize()
            for rep in range(a.reps):
                order = list(runs) if rep % 2 == 0 else list(runs)[::-1]
                for m in order:
                    counts.clear()
                    t0 = time.perf_counter()
                    xs = runs[m]()
                    ctx.synchronize()
                    ts[m].append(time.perf_counter() - t0)
                    prods[m].append(sum(x.last_solve_stats["iterations"] for x in xs))
                    last[m] = (xs, dict(counts))
            for m in runs:
                xs, calls = last[m]
                if m == "lock_step":
                    assert all(x.last_solve_stats.get("lock_step") for x in xs)
                its = [x.last_solve_stats["iterations"] for x in xs]
                calls["device_calls"] = sum(calls.values())
                med = float(np.median(ts[m]))
                row[m] = {"seconds_median": med, "seconds": [round(t, 6) for t in ts[m]], "products": int(sum(its)),
                          "products_per_rep": prods[m], "iterations": its,
                          "us_per_product": round(1e6 * sum(ts[m]) / max(1, sum(prods[m])), 3),
                          "operator_passes": calls.get("block_products", 0) + calls.get("single_products", 0), **calls}
            row["speedup_lock_step"] = round(row["one_by_one"]["seconds_median"] / row["lock_step"]["seconds_median"], 3)
            row["speedup_per_product"] = round(row["one_by_one"]["us_per_product"] / row["lock_step"]["us_per_product"], 3)
            print(json.dumps(row), flush=True)
        del H


if __name__ == "__main__":
    main()
