#!/usr/bin/env python3
"""Parent against branch for the host side of the block sweeps (csrc/block_sweep_launch.h; EXPERIMENTS.md R17): every entry
point that launches a block sweep, at n = 4001, with the row-owner kernel (1), the window-blocked kernel (2) and the
window-blocked kernel on a geometry of 8-row blocks that takes two sweep launches (2x2).  One library per process:

    HIPEIG_LIB=/path/parent/libhipeig.so python tools/block_launcher_ab.py run parent_a.npz
    HIPEIG_LIB=/path/parent/libhipeig.so python tools/block_launcher_ab.py run parent_b.npz
    python tools/block_launcher_ab.py run branch.npz
    python tools/block_launcher_ab.py compare parent_a.npz parent_b.npz branch.npz [--jsonl out.jsonl]

compare: integer outputs (iteration counts, stop codes, steps) equal everywhere; kernel 1 adds a row's terms in a fixed
order, so every array equals the parent's bit for bit; kernel 2 adds them with fp64 LDS atomics in varying order, so the
parent's own run-to-run difference is the yardstick and the branch may differ from the parent by at most 4 times it (the
maximum of one pair of runs is itself a noisy sample).  Exit status 1 when a case misses."""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 4001
CONFIGS = {"1": (1, {}), "2": (2, {}), "2x2": (2, {"HIPEIG_BCOO_RW": "8", "HIPEIG_BCOO_WBITS": "9"})}


def contour(pf, nc=16):
    gk, wk = pf.quadraturePointsWeights(nc, "legendre", positiveHalf=True)
    zs, ws = [], []
    for g, w in zip(gk, wk):
        theta, z = pf.contour_point(-0.21, 0.21, g)
        zs.append(z)
        ws.append(-0.5 * w * 0.21 * (math.cos(theta) + 1j * math.sin(theta)))
    return zs, ws


def run(path):
    import importlib
    import eigensolvers_amd as ea
    from eigensolvers_amd import feast as pf
    from eigensolvers_amd.generators import gapped_csr_host
    lf = importlib.import_module("eigensolvers_amd.lanczos_filter")
    Hh = gapped_csr_host(N, 16, seed=7)
    rng = np.random.default_rng(11)
    X = rng.standard_normal((N, 16))
    X /= np.linalg.norm(X, axis=0)
    zs, ws = contour(pf)
    out = {}
    vec = lambda col, o=None: ea.HipVector(col.copy(), o) if o else ea.HipVector(col.copy())
    arr = lambda bufs: np.array([ea.HipVector(b).array for b in bufs])
    for name, (variant, env) in CONFIGS.items():
        os.environ.update(env)                                   # the geometry is read when a layout is first built
        try:
            H = ea.HipCsrOperator.from_scipy(Hh)
            H.set_block_variant(variant)
            put = lambda case, **kw: out.update({f"{name}/{case}/{k}": np.asarray(v) for k, v in kw.items()})
            for k in (3, 8):
                put(f"spmm_k{k}", y=arr(H.apply_block([vec(X[:, j])._buf for j in range(k)])))
            put("spmm_shift_k8", y=arr(H.apply_shifted_block(0.02, [vec(X[:, j])._buf for j in range(8)])))
            geometry = [H.block_info()[k] for k in ("row_blocks", "windows", "rows_per_block")] if variant == 2 else [0, 0, 0]
            assert name != "2x2" or geometry[0] > H.ctx.device_info()["cus"], "one sweep launch: nothing compared"
            for p in (4, 8):                                     # 4 complex operands: the 8-wide block; 8: the 16-wide one
                os.environ["HIPEIG_PAIR_BLOCK_WIDTH"] = "8" if p == 8 else "4"
                xs = [(vec(X[:, 2 * j])._buf, vec(X[:, 2 * j + 1])._buf) for j in range(p)]
                for case, z in ((f"pairs_p{p}", 0.02 + 0.1j), (f"pairs_z_p{p}", [0.02 * (j + 1) + 0.05j * (j + 1) for j in range(p)])):
                    ys = H.apply_shifted_pairs(z, xs)
                    put(case, re=arr([y[0] for y in ys]), im=arr([y[1] for y in ys]))
            os.environ.pop("HIPEIG_PAIR_BLOCK_WIDTH")
            for k in (3, 8):
                o = {"linearSystemArgs": {"linearSolver": "minres", "linearIter": 2000, "linear_tol": 1e-8}}
                S = ea.HipVector.solveBlock(H, [vec(X[:, j], o) for j in range(k)], 0.02)
                put(f"solve_k{k}", x=np.array([s.array for s in S]),
                    counts=np.array([[s.last_solve_stats["iterations"], s.last_solve_stats["istop"]] for s in S], dtype=np.int64))
            o = {"linearSystemArgs": {"linearSolver": "lanczos_filter", "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7}}
            for keep in (False, True):                           # pass 2 as product steps / as the stream over the kept basis
                r = ea.lanczos_run(H, [vec(X[:, j], o) for j in range(8)], zs, keepBasis=keep)
                try:
                    q = r.combine(lf.filter_coefficients(r.scalars, zs, ws))
                finally:
                    r.release()
                if not keep:
                    m = max(len(s.alphas) for s in r.scalars)
                    pad = lambda a, n: np.concatenate([a, np.zeros(n - len(a))])
                    put("lanczos_scalars", alphas=np.array([pad(s.alphas, m) for s in r.scalars]),
                        betas=np.array([pad(s.betas, m + 1) for s in r.scalars]),
                        counts=np.array([list(s.iterations) + [r.products_pass1[0], r.products_pass2[0]] for s in r.scalars], dtype=np.int64))
                put("lanczos_pass2_" + ("stream" if keep else "products"), q=np.array([v.array for v in q]))
            put("layout", counts=np.array([H.block_info()["variant"] == "column-window-blocked"] + geometry, dtype=np.int64))
        finally:
            for k in env:
                os.environ.pop(k)
    np.savez(path, **out)
    print(f"wrote {len(out)} arrays to {path}")


def rel(a, b):
    return 0.0 if a.shape == b.shape and np.array_equal(a, b) else float(np.max(np.abs(a - b)) / np.max(np.abs(a))) if a.shape == b.shape else math.inf


def compare(pa, pb, br, jsonl, fixed_order=lambda case: case.split("/")[0] == "1"):
    """``fixed_order(case)``: the case adds a row's terms in a fixed order, so it must reproduce the parent bit for bit."""
    A, B, C = np.load(pa), np.load(pb), np.load(br)
    assert set(A.files) == set(B.files) == set(C.files), "the runs hold different cases"
    rows, ok = [], True
    for case in sorted({k.rsplit("/", 1)[0] for k in A.files}):
        keys = [k for k in A.files if k.rsplit("/", 1)[0] == case]
        ints = [k for k in keys if A[k].dtype.kind == "i"]
        reals = [k for k in keys if A[k].dtype.kind != "i"]
        counts_equal = all(np.array_equal(A[k], C[k]) for k in ints)            # the branch against the parent's first run
        parent_counts_equal = all(np.array_equal(A[k], B[k]) for k in ints)     # the parent against itself
        yard = max([rel(A[k], B[k]) for k in reals], default=0.0)
        diff = max([rel(A[k], C[k]) for k in reals], default=0.0)
        fixed = fixed_order(case)
        good = counts_equal and (diff == 0.0 and yard == 0.0 if fixed else diff <= 4.0 * yard)
        ok = ok and good
        row = {"case": case, "counts_equal": bool(counts_equal), "parent_counts_equal": bool(parent_counts_equal), "parent_vs_parent": yard, "branch_vs_parent": diff,
               "criterion": "bit-equal" if fixed else "branch <= 4 x parent", "ok": bool(good)}
        if ints:
            row["counts"] = A[ints[0]].tolist()
            if not (counts_equal and parent_counts_equal):
                row["counts_parent_b"], row["counts_branch"] = B[ints[0]].tolist(), C[ints[0]].tolist()
        rows.append(row)
        print(f"{case:32s} counts {'equal' if counts_equal else 'DIFFER'} (parent-parent {'equal' if parent_counts_equal else 'DIFFER'})  parent-parent {yard:.2e}  branch-parent {diff:.2e}  "
              f"{'ok' if good else 'MISS'}")
    if jsonl:
        with open(jsonl, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    print("all cases ok" if ok else "MISSED")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("run").add_argument("out")
    c = sub.add_parser("compare")
    c.add_argument("parent_a")
    c.add_argument("parent_b")
    c.add_argument("branch")
    c.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    if a.cmd == "run":
        run(a.out)
        return 0
    return compare(a.parent_a, a.parent_b, a.branch, a.jsonl)


if __name__ == "__main__":
    sys.exit(main())
