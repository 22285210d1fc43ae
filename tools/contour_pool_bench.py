#!/usr/bin/env python3
"""One FEAST iteration (maxit = 1) of config #5's recipe (tools/bench_configs.py: the generated gapped operator, 16
subspace vectors, 16 Legendre nodes = 8 contour points, window [-0.21, 0.21], gcrotmk rtol 1e-5) with the contour pool
off (one contour point at a time, its solves in lock step) and on (all 128 solves through an always-full pool), the two
modes alternating.  One JSON line per run as soon as it is measured: wall seconds, products, block products by live
operands ("histogram"), rounds (block products); the first line describes the device.  The pool-off mode passes none of
the pool's keywords, so the same script measures a build that does not have them (--modes off).

    python tools/contour_pool_bench.py [--n 1000000 --reps 3 --modes off,on --width W] >> profiles/NN_contour_pool.jsonl

--replicas P: instead, one iteration over P loopback contour replicas on one GPU with the pool and each deal, reporting
per-replica product totals (max / mean is the load balance; busy times of threads sharing a GPU say nothing).
"""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m0", type=int, default=16)
    ap.add_argument("--nc", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--width", type=int, default=None, help="options['contourPoolWidth'] (default: the memory rule)")
    ap.add_argument("--cols", type=int, default=4, help="arnoldiColumnsPerPass")
    ap.add_argument("--label", default="")
    ap.add_argument("--replicas", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    import scipy.linalg as la
    import eigensolvers_amd as ea

    N, m0 = a.n, a.m0
    opt = {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7,
                                "arnoldiColumnsPerPass": a.cols}}
    if a.width is not None:
        opt["contourPoolWidth"] = a.width
    Y0 = la.qr(np.random.default_rng(9).standard_normal((N, m0)), mode="economic")[0]
    ctx = ea.HipContext.default()
    print(json.dumps({"device": ctx.device_info()["name"], "N": N, "m0": m0, "contour_points": a.nc // 2, "reps": a.reps,
                      "label": a.label}), flush=True)

    def iteration(H, c, **kw):
        Y = [ea.HipVector(Y0[:, i].copy(), dict(opt), ctx=c) for i in range(m0)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return ea.feastDiagonalization(H, Y, a.nc, "legendre", -0.21, 0.21, 1e-4, 1, writeOut=False, **kw)

    if a.replicas:
        from eigensolvers_amd.distributed import ContourReplicas, LoopbackGroup
        for deal in ("point", "balanced"):
            grp = LoopbackGroup(a.replicas)
            try:
                def run(rank, c):
                    comm = ContourReplicas(c)
                    H = ea.HipCsrOperator.generate(N, 32, seed=7, ctx=c)
                    ev, Yf, st = iteration(H, c, contourComm=comm, contourPool=True, contourDeal=deal)
                    rec = st["contourPool"][0] if st.get("contourPool") else {"products": [], "rounds": 0}
                    return int(sum(rec["products"])), int(rec["rounds"]), len(rec["products"])
                res = grp.run(run)
            finally:
                grp.close()
            tot = [r[0] for r in res]
            print(json.dumps({"label": a.label, "N": N, "replicas": a.replicas, "deal": deal, "products_per_replica": tot,
                              "rounds_per_replica": [r[1] for r in res], "solves_per_replica": [r[2] for r in res],
                              "max_over_mean": round(max(tot) / (sum(tot) / len(tot)), 4)}), flush=True)
        return

    H = ea.HipCsrOperator.generate(N, 32, seed=7)
    hist = {}
    inner = ea.HipCsrOperator.apply_shifted_pairs

    def counted(self, z, xs, reverse=False):
        hist[len(xs)] = hist.get(len(xs), 0) + 1
        return inner(self, z, xs, reverse=reverse)
    ea.HipCsrOperator.apply_shifted_pairs = counted

    modes = a.modes.split(",")
    for rep in range(a.reps):
        for mode in (modes if rep % 2 == 0 else modes[::-1]):
            hist.clear()
            ctx.synchronize()
            t0 = time.perf_counter()
            ev, Yf, st = iteration(H, ctx, **({"contourPool": True} if mode == "on" else {}))
            ctx.synchronize()
            dt = time.perf_counter() - t0
            row = {"label": a.label, "N": N, "mode": mode, "rep": rep, "seconds": round(dt, 3),
                   "products": int(sum(k * v for k, v in hist.items())), "rounds": int(sum(hist.values())),
                   "histogram": {str(k): hist[k] for k in sorted(hist)},
                   "eigenvalues_in_window": int(np.sum((ev >= -0.21) & (ev <= 0.21)))}
            if mode == "on":
                rec = st["contourPool"][0]
                row.update({"width": rec["width"], "pool_rounds": rec["rounds"],
                            "products_per_point": [int(sum(p for (k, i), p in zip(rec["pairs"], rec["products"]) if k == kk))
                                                   for kk in range(a.nc // 2)],
                            "products_max_min": [int(max(rec["products"])), int(min(rec["products"]))]})
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
