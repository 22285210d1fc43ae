#!/usr/bin/env python3
"""GCROT(m,k) with and without its diagonal right preconditioner (``linearSystemArgs["gcrotPreconditioner"]``) on one
MI355X, in the conventions of ``tools/precond_bench.py``: the two modes alternate inside every repetition, 3 repetitions,
medians and spread, host clock around the whole call (which ends in a device synchronise).  JSON lines:

  feast     one FEAST iteration (maxit = 1) of config #5's recipe (``tools/contour_pool_bench.py``: generated gapped
            operator, N = 1e6, 16 subspace vectors, 8 contour points, window [-0.21, 0.21], gcrotmk rtol 1e-5) through the
            contour pool, key off and on: wall seconds and the products of its 128 solves
  lanczos   the real-shift solves of one block Lanczos iteration (``solveBlock`` of ``--nblock`` seeded right-hand sides,
            sigma = 0.02, gcrotmk rtol 1e-8) on the same operator, key off and on: wall seconds and products per solve

Every measurement is a child process of its own under a time limit sized from the plain FEAST iteration (28.8 s in
README); a child that fails or runs out of time ends the run.  The generator is a best case for a diagonal preconditioner
(DESIGN.md 3.4b says where it loses).

usage: python tools/gcrot_precond_bench.py [--n 1000000] [--reps 3] [--what feast,lanczos] [--out profiles/FILE.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LIMITS = {"feast": 300, "lanczos": 300}          # seconds per child: operator build, one warm-up product, one measured call


def options(key, tol, atol):
    lsa = {"linearSolver": "gcrotmk", "linearIter": 4000, "linear_tol": tol, "linear_atol": atol, "arnoldiColumnsPerPass": 4}
    if key:
        lsa["gcrotPreconditioner"] = "jacobi"
    return {"linearSystemArgs": lsa}


def child(what, key, n, nblock):
    import numpy as np
    import scipy.linalg as la
    import eigensolvers_amd as ea
    ctx = ea.HipContext.default()
    H = ea.HipCsrOperator.generate(n, 32, seed=7)
    rng = np.random.default_rng(9)
    if what == "feast":
        m0 = 16
        Y0 = la.qr(rng.standard_normal((n, m0)), mode="economic")[0]
        Y = [ea.HipVector(Y0[:, i].copy(), options(key, 1e-5, 1e-7)) for i in range(m0)]
        Y[0].applyOp(H)                                    # layouts built outside the clock
        ctx.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ev, Yf, st = ea.feastDiagonalization(H, Y, 16, "legendre", -0.21, 0.21, 1e-4, 1, writeOut=False, contourPool=True)
        ctx.synchronize()
        dt = time.perf_counter() - t0
        rec = st["contourPool"][0]
        return {"seconds": round(dt, 3), "solves": len(rec["products"]), "products": int(sum(rec["products"])),
                "products_max_min": [int(max(rec["products"])), int(min(rec["products"]))], "rounds": int(rec["rounds"]),
                "width": rec["width"], "eigenvalues_in_window": int(np.sum((ev >= -0.21) & (ev <= 0.21)))}
    bs = [ea.HipVector(v / np.linalg.norm(v), options(key, 1e-8, 1e-12)) for v in rng.standard_normal((nblock, n))]
    bs[0].applyOp(H)
    ctx.synchronize()
    t0 = time.perf_counter()
    xs = ea.HipVector.solveBlock(H, bs, 0.02)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    return {"seconds": round(dt, 3), "solves": nblock, "products_per_solve": [x.last_solve_stats["iterations"] for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nblock", type=int, default=4)
    ap.add_argument("--what", default="feast,lanczos")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r22_gcrot_precond.jsonl"))
    ap.add_argument("--child", nargs=2, metavar=("WHAT", "KEY"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child[0], a.child[1] == "on", a.n, a.nblock)), flush=True)
        return 0
    import numpy as np
    out = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for what in a.what.split(","):
        runs = {"off": [], "on": []}
        for rep in range(a.reps):
            for mode in (("off", "on") if rep % 2 == 0 else ("on", "off")):
                cmd = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--nblock", str(a.nblock), "--child", what, mode]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[what])
                except subprocess.TimeoutExpired:
                    emit({"what": what, "mode": mode, "rep": rep, "error": f"no result within {LIMITS[what]} s"})
                    return 1
                if r.returncode != 0:
                    emit({"what": what, "mode": mode, "rep": rep, "error": r.stderr[-400:], "returncode": r.returncode})
                    return 1
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                runs[mode].append(rec)
                emit({"what": what, "N": a.n, "mode": mode, "rep": rep, **rec})
        sec = {m: [r["seconds"] for r in runs[m]] for m in runs}
        emit({"what": what + " summary", "N": a.n, "reps": a.reps,
              "seconds_median": {m: float(np.median(v)) for m, v in sec.items()},
              "seconds_min_max": {m: [min(v), max(v)] for m, v in sec.items()},
              "ratio_off_over_on": round(float(np.median(sec["off"]) / np.median(sec["on"])), 3)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
