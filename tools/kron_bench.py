#!/usr/bin/env python3
"""Kronecker-sum operator timings: product, shifted product and one MINRES iteration of the coupled oscillator on a
direct-product grid, through ``HipKronSumOperator`` and - where the explicit matrix fits - through the CSR path on
``HipCsrOperator.from_scipy(H.to_scipy())`` of the SAME operator in the same process.  HIP events, warm: ``--reps``
repetitions after ``--warmup``.  One JSON line per grid.

    python tools/kron_bench.py >> profiles/rNN_kron_sum.jsonl
    python tools/kron_bench.py --dims 64,64,64 --no-csr
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_BYTES_PER_S = 8.0e12
DEFAULT_GRIDS = ((100, 100, 100), (64, 64, 64), (32, 32, 32, 32))
CSR_MAX_NNZ = 1 << 30                     # the explicit matrix is built on the host: 12 bytes per entry there and on the device


def bench(dims, a):
    import numpy as np
    import eigensolvers_amd as ea
    from eigensolvers_amd.generators import coupled_oscillator_grid
    ctx = ea.HipContext.default()
    D = len(dims)
    ranges = [(-5.0 + 0.5 * d, 5.0 - 0.5 * d) for d in range(D)]
    freqs = [1.0 + 0.3 * d for d in range(D)]
    factors, V = coupled_oscillator_grid(dims, ranges, freqs)
    H = ea.HipKronSumOperator.from_factors(factors, diag=V)
    n = H.nrows
    opts = lambda: {"linearSystemArgs": {"linearSolver": "minres", "linearIter": a.iterations, "linear_tol": 1e-300}}
    rng = np.random.default_rng(5)
    x = rng.standard_normal(n)
    x /= np.linalg.norm(x)
    X = ea.HipVector(x, opts())
    y = ctx.alloc(n)
    sigma = float(np.min(V)) - 1.0                                  # below the spectrum: every iteration runs, none is special
    out = {"dims": list(dims), "n": n, "device": ctx.device_info()["name"], "reps": a.reps, "warmup": a.warmup,
           "kron_info": H.kron_info(), "kron_algorithmic_bytes": H.algorithmic_bytes()}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ctx.synchronize()
        ctx.timer_start()
        for _ in range(a.reps):
            fn()
        return ctx.timer_stop() / a.reps

    def iteration_ms(op):
        """Milliseconds per MINRES iteration of a solve that runs exactly ``--iterations`` of them (set-up included)."""
        ms = None
        for _ in range(2):                                        # the first solve allocates the workspaces
            try:
                ctx.synchronize()
                ctx.timer_start()
                ea.HipVector.solve(op, X, sigma)
            except UserWarning:
                pass
            ms = ctx.timer_stop()
        return ms / X.last_solve_stats["iterations"], X.last_solve_stats["iterations"]

    def measure(op, alg):
        r = {"apply_ms": timed(lambda: op.apply(X._buf, y))}
        prod = ea.HipVector(y).array.copy()
        r["apply_shifted_ms"] = timed(lambda: op.apply_shifted(sigma, X._buf, y))
        r["minres_iteration_ms"], r["minres_iterations"] = iteration_ms(op)
        r["variant"] = op.last_variant()
        r["device_bytes"] = int(op.device_bytes)
        for key in ("apply_ms", "apply_shifted_ms"):
            r[key.replace("_ms", "_frac_of_8TBs")] = alg / (r[key] * 1e-3) / HBM_PEAK_BYTES_PER_S
        return r, prod

    out["kron"], pk = measure(H, H.algorithmic_bytes())
    nnz = n * (sum(dims) - D + 1)
    if a.csr and nnz < CSR_MAX_NNZ:
        t0 = time.time()
        Hc = ea.HipCsrOperator.from_scipy(H.to_scipy())
        out["csr_build_host_s"] = round(time.time() - t0, 1)
        out["csr_nnz"] = int(Hc.nnz)
        out["csr_algorithmic_bytes"] = Hc.algorithmic_bytes()
        out["csr"], pc = measure(Hc, Hc.algorithmic_bytes())
        out["max_rel_diff_product"] = float(np.max(np.abs(pk - pc)) / np.max(np.abs(pc)))
        for key in ("apply_ms", "apply_shifted_ms", "minres_iteration_ms"):
            out["speedup_" + key[:-3]] = out["csr"][key] / out["kron"][key]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", action="append", help="a grid as n1,n2,...; may be repeated (default: the three documented grids)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--no-csr", dest="csr", action="store_false")
    a = ap.parse_args()
    grids = [tuple(int(t) for t in g.split(",")) for g in a.dims] if a.dims else DEFAULT_GRIDS
    for dims in grids:
        bench(dims, a)


if __name__ == "__main__":
    main()
