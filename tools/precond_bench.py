#!/usr/bin/env python3
"""Plain against Jacobi-preconditioned MINRES on one MI355X, in the class of BASELINE configuration #2.

For ``HipCsrOperator.generate(N, 65, seed)``, ``sigma = 0.02``, ``linear_tol = 1e-10`` and the seeded guess vector it
reports, as JSON lines (one record per line, ``"what"`` names it):

  solve        iterations, ms per solve and ms per iteration of the plain and the preconditioned solve: ``--reps``
               repetitions with the two modes alternating inside every repetition, after one warm-up solve each
  chunk        ms per iteration of the preconditioned solve with HIPEIG_PMR_CHUNK = 8 / 16 / 32 (alternating as well)
  floor        iterations of the preconditioned solve for preconditionerFloor = 0, 1e-8, 1e-3, 1e-2
  lanczos      one whole single-vector Lanczos run of configuration #2 (N = 1e6, 32 per row, L = 8, 6 cycles, eConv 1e-12)
               with and without the key: wall seconds and the inner iterations summed over its solves

Times are host clocks around work that ends in a device synchronise.  The generator is a best case for a diagonal
preconditioner (diagonal +-(1..10) plus a mid-spectrum cluster, off-diagonal row norm ~0.05): the iteration counts say
nothing about operators without diagonal dominance.

With ``--block K`` it measures the block solves instead (``"what": "block"`` and ``"block_chunk"``): ``solveBlock`` on
the same K seeded right-hand sides with ``linearSystemArgs["preconditionerLockStep"]`` off (the one-by-one preconditioned
solves) and on (the lock-step block form), the two modes alternating inside every repetition after one warm-up each -
ms per block of every repetition, medians and the per-column iteration counts - and the lock-step solve with
HIPEIG_PMRB_CHUNK = 8 / 16 / 32.  The records go to ``profiles/r19_jacobi_block.jsonl`` unless ``--out`` names another file.

usage: python tools/precond_bench.py [--sizes 1000000,10000000] [--reps 3] [--no-lanczos] [--block K] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import eigensolvers_amd as ea  # noqa: E402
from eigensolvers_amd.generators import guess_vector  # noqa: E402

SIGMA, RTOL = 0.02, 1e-10


def options(pre, floor=None, it=3000):
    lsa = {"linearSolver": "minres", "linearIter": it, "linear_tol": RTOL}
    if pre:
        lsa["preconditioner"] = "jacobi"
        if floor is not None:
            lsa["preconditionerFloor"] = floor
    return {"linearSystemArgs": lsa}


def timed_solve(H, b, opts):
    ctx = ea.HipContext.default()
    B = ea.HipVector(b, opts)
    ctx.synchronize()
    t = time.perf_counter()
    W = ea.HipVector.solve(H, B, SIGMA)
    ctx.synchronize()
    ms = (time.perf_counter() - t) * 1e3
    return W.last_solve_stats["iterations"], ms


def median(v):
    return float(np.median(v))


def solve_records(N, nnz_row, seed, reps, emit):
    H = ea.HipCsrOperator.generate(N, nnz_row, seed=seed)
    b = guess_vector(N, 1)
    b /= np.linalg.norm(b)
    modes = {"plain": options(False), "jacobi": options(True)}
    for o in modes.values():                                   # warm-up: code objects, layouts, workspaces, minv
        timed_solve(H, b, o)
    runs = {m: [] for m in modes}
    for _ in range(reps):
        for m, o in modes.items():                             # alternating
            runs[m].append(timed_solve(H, b, o))
    rec = {"what": "solve", "N": N, "nnz_row": nnz_row, "seed": seed, "sigma": SIGMA, "rtol": RTOL, "reps": reps,
           "kernel": H.last_variant()}
    for m, r in runs.items():
        its = [i for i, _ in r]
        rec[m] = {"iterations": its[0], "iterations_all_equal": len(set(its)) == 1,
                  "ms_per_solve": [round(ms, 4) for _, ms in r], "ms_per_solve_median": round(median([ms for _, ms in r]), 4),
                  "ms_per_iteration_median": round(median([ms / i for i, ms in r]), 5)}
    rec["per_iteration_ratio_jacobi_over_plain"] = round(rec["jacobi"]["ms_per_iteration_median"] / rec["plain"]["ms_per_iteration_median"], 4)
    rec["per_solve_ratio_plain_over_jacobi"] = round(rec["plain"]["ms_per_solve_median"] / rec["jacobi"]["ms_per_solve_median"], 3)
    # the byte model: a plain iteration moves 12 nnz + 4 (N + 1) + 8 N gathered + the element-wise streams (13 N doubles:
    # KA's epilogue r2 r1 y + KD's r1 w1 w2 w x(2), KC's r2 y(2)); the preconditioned one 24 N bytes more
    plain_bytes = 12.0 * H.nnz + 4.0 * (N + 1) + 8.0 * N + 13 * 8.0 * N
    rec["byte_model_ratio"] = round((plain_bytes + 24.0 * N) / plain_bytes, 4)
    emit(rec)

    chunks = ("8", "16", "32")
    per = {c: [] for c in chunks}
    for _ in range(reps):
        for c in chunks:
            os.environ["HIPEIG_PMR_CHUNK"] = c
            i, ms = timed_solve(H, b, modes["jacobi"])
            per[c].append(ms / i)
    del os.environ["HIPEIG_PMR_CHUNK"]
    emit({"what": "chunk", "N": N, "nnz_row": nnz_row, "reps": reps, "iterations": rec["jacobi"]["iterations"],
          "ms_per_iteration_median": {c: round(median(v), 5) for c, v in per.items()},
          "ms_per_iteration": {c: [round(x, 5) for x in v] for c, v in per.items()}})

    floors = {}
    for f in (0.0, 1e-8, 1e-3, 1e-2):
        try:
            floors[repr(f)] = timed_solve(H, b, options(True, f))[0]
        except ValueError as exc:
            floors[repr(f)] = f"ValueError: {exc}"[:120]
    emit({"what": "floor", "N": N, "nnz_row": nnz_row, "iterations_by_preconditionerFloor": floors})


def timed_block(H, cols, opts):
    ctx = ea.HipContext.default()
    B = [ea.HipVector(c, opts) for c in cols]
    ctx.synchronize()
    t = time.perf_counter()
    X = ea.HipVector.solveBlock(H, B, SIGMA)
    ctx.synchronize()
    ms = (time.perf_counter() - t) * 1e3
    return [x.last_solve_stats["iterations"] for x in X], bool(X[0].last_solve_stats.get("lockStep", False)), ms, X


def block_records(N, nnz_row, seed, K, reps, emit):
    H = ea.HipCsrOperator.generate(N, nnz_row, seed=seed)
    cols = []
    for j in range(K):
        b = guess_vector(N, j + 1)
        cols.append(b / np.linalg.norm(b))
    modes = {"one_by_one": options(True), "lock_step": options(True)}
    modes["lock_step"]["linearSystemArgs"]["preconditionerLockStep"] = True
    last = {}
    for m, o in modes.items():                                 # warm-up: code objects, layouts, workspaces, minv
        last[m] = timed_block(H, cols, o)[3]
    diff = [float(np.linalg.norm(a.array - b.array) / np.linalg.norm(b.array)) for a, b in zip(last["lock_step"], last["one_by_one"])]
    del last
    runs = {m: [] for m in modes}
    for _ in range(reps):
        for m, o in modes.items():                             # alternating
            runs[m].append(timed_block(H, cols, o)[:3])
    rec = {"what": "block", "N": N, "nnz_row": nnz_row, "seed": seed, "sigma": SIGMA, "rtol": RTOL, "reps": reps, "K": K,
           "block_kernel": H.block_info()["variant"], "x_difference_rel_max": max(diff)}
    for m, r in runs.items():
        assert all(lock == (m == "lock_step") for _, lock, _ in r), "the mode did not take its path"
        ms = [t for _, _, t in r]
        rec[m] = {"iterations": r[0][0], "iterations_all_equal": all(i == r[0][0] for i, _, _ in r),
                  "ms_per_block": [round(t, 4) for t in ms], "ms_per_block_median": round(median(ms), 4),
                  "ms_per_block_spread": round(max(ms) - min(ms), 4)}
    rec["ratio_one_by_one_over_lock_step"] = round(rec["one_by_one"]["ms_per_block_median"] / rec["lock_step"]["ms_per_block_median"], 3)
    emit(rec)

    chunks = ("8", "16", "32")
    per = {c: [] for c in chunks}
    for _ in range(reps):
        for c in chunks:
            os.environ["HIPEIG_PMRB_CHUNK"] = c
            per[c].append(timed_block(H, cols, modes["lock_step"])[2])
    del os.environ["HIPEIG_PMRB_CHUNK"]
    emit({"what": "block_chunk", "N": N, "nnz_row": nnz_row, "reps": reps, "K": K,
          "ms_per_block_median": {c: round(median(v), 4) for c, v in per.items()},
          "ms_per_block": {c: [round(x, 4) for x in v] for c, v in per.items()}})


def lanczos_records(emit):
    N = 1_000_000
    H = ea.HipCsrOperator.generate(N, 32, seed=7)
    real_solve = ea.HipVector.solve
    inner = []

    def counting(Hs, b, s, *a, **k):
        x = real_solve(Hs, b, s, *a, **k)
        inner.append(x.last_solve_stats["iterations"])
        return x

    ea.HipVector.solve = staticmethod(counting)
    try:
        rec = {"what": "lanczos", "N": N, "nnz_row": 32, "seed": 7, "L": 8, "maxit": 6, "eConv": 1e-12, "rtol": RTOL}
        for tag, pre in (("warmup", True), ("plain", False), ("jacobi", True)):
            inner.clear()
            v0 = ea.HipVector(guess_vector(N, 1).copy(), options(pre))
            ea.HipContext.default().synchronize()
            t = time.perf_counter()
            ev, Y, st = ea.inexactLanczosDiagonalization(H, v0, SIGMA, 8, 6, 1e-12, writeOut=False)
            ea.HipContext.default().synchronize()
            dt = time.perf_counter() - t
            if tag == "warmup":
                continue
            rec[tag] = {"seconds": round(dt, 3), "ritz": float(ev[0]), "converged": bool(st["isConverged"]),
                        "cumIter": st["cumIter"], "solves": len(inner), "inner_iterations": int(sum(inner)),
                        "true_residual_norm": float(ea.true_residual_norms(H, ev, Y, 1)[0])}
        rec["ritz_difference_rel"] = abs(rec["plain"]["ritz"] - rec["jacobi"]["ritz"]) / abs(rec["plain"]["ritz"])
        rec["wall_ratio_plain_over_jacobi"] = round(rec["plain"]["seconds"] / rec["jacobi"]["seconds"], 3)
        emit(rec)
    finally:
        ea.HipVector.solve = staticmethod(real_solve)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--nnz-row", type=int, default=65)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-lanczos", action="store_true")
    ap.add_argument("--block", type=int, default=0, help="measure solveBlock on this many right-hand sides instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.block and not a.out:
        a.out = os.path.join(REPO, "profiles", "r19_jacobi_block.jsonl")
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    info = ea.HipContext.default().device_info()
    emit({"what": "device", "info": info if isinstance(info, (dict, list, str)) else str(info)})
    for N in [int(s) for s in a.sizes.split(",") if s]:
        if a.block:
            block_records(N, a.nnz_row, a.seed, a.block, a.reps, emit)
        else:
            solve_records(N, a.nnz_row, a.seed, a.reps, emit)
    if not a.no_lanczos and not a.block:
        lanczos_records(emit)


if __name__ == "__main__":
    main()
