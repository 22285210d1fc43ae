#!/usr/bin/env python3
"""Plain, Jacobi and separable MINRES on the Kronecker-sum operator, one MI355X.

For ``coupled_oscillator_grid`` on every grid of ``--grids`` (ranges (-6, 6) per mode, frequencies 1.0 / 1.3 / 1.7 / 2.1),
``sigma = 0.513 lam[3] + 0.487 lam[4]`` (``eigsh`` on the device product), the normalised seeded guess vector and
``linear_tol = 1e-10`` it reports, as JSON lines (``"what"`` names the record):

  solve   iterations, ms per solve and ms per iteration of the three modes: ``--reps`` repetitions with the modes
          alternating inside every repetition, after one warm-up solve each (the decompositions and sinv are built there);
          medians and max - min
  apply   ms per ``M^-1 x`` alone and ms per ``H x`` alone from HIP events around 50 of them
  chunk   ms per solve of the separable mode with HIPEIG_KPMR_CHUNK = 4 / 8 / 16 (alternating as well)

Solve times are host clocks around work that ends in a device synchronise.  The records go to
``profiles/r22_kron_separable.jsonl`` unless ``--out`` names another file.

usage: python tools/kron_precond_bench.py [--grids 64x64x64,100x100x100,32x32x32x32] [--reps 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse.linalg as spla

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import eigensolvers_amd as ea  # noqa: E402
from eigensolvers_amd import _lib  # noqa: E402
from eigensolvers_amd.generators import coupled_oscillator_grid, guess_vector  # noqa: E402

RTOL = 1e-10
FREQS = [1.0, 1.3, 1.7, 2.1]
MODES = {"plain": None, "jacobi": "jacobi", "separable": "separable"}


def options(pre):
    lsa = {"linearSolver": "minres", "linearIter": 6000, "linear_tol": RTOL}
    if pre:
        lsa["preconditioner"] = pre
    return {"linearSystemArgs": lsa}


def timed_solve(H, b, sigma, pre):
    ctx = H.ctx
    B = ea.HipVector(b, options(pre))
    ctx.synchronize()
    t = time.perf_counter()
    W = ea.HipVector.solve(H, B, sigma)
    ctx.synchronize()
    return W.last_solve_stats["iterations"], (time.perf_counter() - t) * 1e3


def spread(v):
    return {"median": float(np.median(v)), "spread": float(np.max(v) - np.min(v)), "all": [round(float(t), 4) for t in v]}


def event_ms(ctx, fn, count=50):
    fn()
    ctx.synchronize()
    ms = C.c_float()
    _lib.call("hipeig_timer_start", ctx.handle)
    for _ in range(count):
        fn()
    _lib.call("hipeig_timer_stop", ctx.handle, C.byref(ms))
    return ms.value / count


def shift_between_levels(H):
    """``0.513 lam[3] + 0.487 lam[4]`` from the six lowest levels (Lanczos on the device product)."""
    n = H.nrows
    mv = lambda v: ea.HipVector(np.ascontiguousarray(v, dtype=np.float64).reshape(-1)).applyOp(H).array
    lam = np.sort(spla.eigsh(spla.LinearOperator((n, n), matvec=mv, dtype=np.float64), k=6, which="SA", tol=1e-10, ncv=48,
                             return_eigenvectors=False))
    return float(0.513 * lam[3] + 0.487 * lam[4])


def grid_records(dims, reps, emit):
    D = len(dims)
    factors, V = coupled_oscillator_grid(dims, [(-6, 6)] * D, FREQS[:D])
    H = ea.HipKronSumOperator.from_factors(factors, diag=V)
    ctx = H.ctx
    sigma = shift_between_levels(H)
    b = guess_vector(H.nrows, 1)
    b /= np.linalg.norm(b)
    base = {"dims": list(dims), "N": H.nrows, "sigma": sigma, "rtol": RTOL, "reps": reps}

    for pre in MODES.values():                                     # warm-up: code objects, workspaces, minv, Q_d and sinv
        timed_solve(H, b, sigma, pre)
    runs = {m: [] for m in MODES}
    for _ in range(reps):
        for m, pre in MODES.items():                               # alternating
            runs[m].append(timed_solve(H, b, sigma, pre))
    rec = dict(base, what="solve")
    for m, r in runs.items():
        its, ms = [i for i, _ in r], [t for _, t in r]
        rec[m] = {"iterations": its[0], "same_count": len(set(its)) == 1, "ms_per_solve": spread(ms),
                  "ms_per_iteration": float(np.median(ms)) / max(its[0], 1)}
    emit(rec)

    P = H.separable_preconditioner(sigma)
    x = ea.HipVector(b.copy())
    emit(dict(base, what="apply", launches_per_apply=P.launches_per_apply, kernels=P.kernels(),
              precond_device_bytes=P.device_bytes, model_bytes_per_apply=(4 * D + 3) * 8 * H.nrows,
              ms_per_apply=event_ms(ctx, lambda: P.apply(x._buf)), ms_per_product=event_ms(ctx, lambda: x.applyOp(H))))

    ladder = {c: [] for c in (4, 8, 16)}
    for _ in range(reps):
        for c in ladder:
            os.environ["HIPEIG_KPMR_CHUNK"] = str(c)
            ladder[c].append(timed_solve(H, b, sigma, "separable")[1])
    os.environ.pop("HIPEIG_KPMR_CHUNK", None)
    emit(dict(base, what="chunk", ms_per_solve={str(c): spread(v) for c, v in ladder.items()}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", default="64x64x64,100x100x100,32x32x32x32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r22_kron_separable.jsonl"))
    a = ap.parse_args()
    with open(a.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit({"what": "device", "info": ea.HipContext.default().device_info()})
        for g in a.grids.split(","):
            grid_records(tuple(int(n) for n in g.split("x")), a.reps, emit)


if __name__ == "__main__":
    main()
