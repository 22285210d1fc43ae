#!/usr/bin/env python3
"""Parent against branch for the host side of the single-vector sweeps (csrc/sweep_launch.h; EXPERIMENTS.md R18): the product,
the shifted product with both signs, the pair product on its two-sweep fallback and one plain MINRES solve, in sweep layouts
1, 2, 3, 4, 5 and 4 with three column splits (4c), at n = 4001 and on the two geometries of
tests/test_gpu_sweep_two_launches.py that take two sweep launches (n = 20000 for 4 / 5, n = 70001 for 3); and the product on
three loopback ranks with small windows (the raw launches of the overlapped plan).  One library per process:

    HIPEIG_LIB=/path/parent/libhipeig.so python tools/sweep_launcher_ab.py run parent_a.npz
    HIPEIG_LIB=/path/parent/libhipeig.so python tools/sweep_launcher_ab.py run parent_b.npz
    python tools/sweep_launcher_ab.py run branch.npz
    python tools/sweep_launcher_ab.py compare parent_a.npz parent_b.npz branch.npz [--jsonl out.jsonl]
    python tools/sweep_launcher_ab.py time          -> one JSON line: microseconds per back-to-back hipeig_spmv call

compare is block_launcher_ab.py's: integer outputs equal everywhere; layouts 1, 2, 3 and 5 add a row's terms in a fixed order,
so every array equals the parent's bit for bit; 4 and 4c add them with fp64 LDS atomics, so the branch may differ from the
parent by at most 4 times the parent's own run-to-run difference."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TCOOW_SMALL = {"HIPEIG_TCOOW_RW": "64", "HIPEIG_TCOOW_WBITS": "10"}
GEOMETRIES = {"n4001": (4001, {}),
              "n20000": (20000, dict(TCOOW_SMALL, HIPEIG_TCOOW_WG_PER_LAUNCH_CU="1")),
              "n70001": (70001, {"HIPEIG_TCOO_RW": "64", "HIPEIG_TCOO_WG_PER_CU": "1"})}
LAYOUTS = {"1": (1, {}), "2": (2, {}), "3": (3, {}), "4": (4, {}), "5": (5, {}), "4c": (4, {"HIPEIG_TCOOW_CSPLIT": "3"})}
FIXED_ORDER = ("1", "2", "3", "5")
SIGMA = 0.02


def fixed_order(case):
    return case.split("@")[0] in FIXED_ORDER


def unit_guess(n):
    from eigensolvers_amd.generators import guess_vector
    b = guess_vector(n, 1)
    return b / np.linalg.norm(b)


def run(path):
    import eigensolvers_amd as ea
    from eigensolvers_amd.distributed import LoopbackGroup, row_range
    from eigensolvers_amd.generators import gapped_csr_host
    ctx = ea.HipContext.default()
    out = {}
    for gname, (n, genv) in GEOMETRIES.items():
        Hh, b = gapped_csr_host(n, 16, seed=7), unit_guess(n)
        xi = np.random.default_rng(5).standard_normal(n)
        for lname, (variant, lenv) in LAYOUTS.items():
            env = dict(genv, **lenv)
            os.environ.update(env)                               # the geometry is read when a layout is first built
            try:
                H = ea.HipCsrOperator.from_scipy(Hh)
                H.set_variant(variant)
                put = lambda case, **kw: out.update({f"{lname}@{gname}/{case}/{k}": np.asarray(v) for k, v in kw.items()})
                x = ea.HipVector(b.copy())
                put("spmv", y=x.applyOp(H).array)
                for reverse in (False, True):
                    y = ctx.alloc(n)
                    H.apply_shifted(SIGMA, x._buf, y, reverse=reverse)
                    put("spmv_shift_" + ("minus" if reverse else "plus"), y=ea.HipVector(y).array)
                os.environ["HIPEIG_PAIR_SWEEP"] = "0"            # the two-sweep fallback: launch_spmv twice and two updates
                yr, yi = ctx.alloc(n), ctx.alloc(n)
                H.apply_shifted_pair(SIGMA + 0.11j, x._buf, ea.HipVector(xi.copy())._buf, yr, yi)
                os.environ.pop("HIPEIG_PAIR_SWEEP")
                assert not H.pair_info()["fused"]
                put("pair_fallback", re=ea.HipVector(yr).array, im=ea.HipVector(yi).array)
                o = {"linearSystemArgs": {"linearSolver": "minres", "linearIter": 3000, "linear_tol": 1e-8}}
                W = ea.HipVector.solve(H, ea.HipVector(b.copy(), o), SIGMA)
                put("minres", x=W.array, counts=np.array([W.last_solve_stats["iterations"], W.last_solve_stats["istop"]], dtype=np.int64))
                lay = H.layout_info()
                put("layout", counts=np.array([lay["variant"], H.launches_per_apply(), lay["rows_per_block"], lay["column_splits"]], dtype=np.int64))
                if (gname, lname) in (("n20000", "4"), ("n20000", "5"), ("n70001", "3")):
                    assert H.launches_per_apply() >= 2, "one sweep launch: nothing compared"
            finally:
                for k in env:
                    os.environ.pop(k)
    # three loopback ranks, 1 Ki-column windows and 64-row blocks: local and remote windows swept by separate raw launches
    n, P = 30011, 3
    Hh, b = gapped_csr_host(n, 16, seed=7), unit_guess(n)
    for lname in ("1", "4", "5", "4c"):
        variant, lenv = LAYOUTS[lname]
        env = dict(TCOOW_SMALL, **lenv)
        os.environ.update(env)
        grp = LoopbackGroup(P)

        def body(rank, rctx):
            r0, r1 = row_range(n, P, rank)
            H = ea.HipCsrOperator.from_scipy(Hh, row_begin=r0, row_end=r1, ctx=rctx)
            H.set_variant(variant)
            y = ea.HipVector(b[r0:r1].copy(), ctx=rctx).applyOp(H).array
            ys = rctx.alloc(r1 - r0)
            H.apply_shifted(SIGMA, ea.HipVector(b[r0:r1].copy(), ctx=rctx)._buf, ys)
            return y, ea.HipVector(ys, ctx=rctx).array, H.layout_info()

        try:
            res = grp.run(body)
        finally:
            grp.close()
            for k in env:
                os.environ.pop(k)
        out[f"{lname}@loopback3/spmv/y"] = np.concatenate([r[0] for r in res])
        out[f"{lname}@loopback3/spmv_shift_plus/y"] = np.concatenate([r[1] for r in res])
        out[f"{lname}@loopback3/layout/counts"] = np.array([[r[2]["variant"], r[2]["column_splits"], r[2]["exchange_chunks"]] for r in res], dtype=np.int64)
    np.savez(path, **out)
    print(f"wrote {len(out)} arrays to {path}")


def time_products(calls):
    """Back-to-back hipeig_spmv calls where the host side would show: a launch-bound product (n = 4000, CSR-stream) and the
    smallest size the automatic choice gives the workgroup-unit layout at this density (n = 300000, layout 4)."""
    import eigensolvers_amd as ea
    ctx = ea.HipContext.default()
    out = {"calls": calls}
    for n, variant in ((4000, 2), (300000, 4)):
        H = ea.HipCsrOperator.generate(n, 32, seed=7)
        H.set_variant(variant)
        x, y = ea.HipVector(np.ones(n))._buf, ctx.alloc(n)
        for _ in range(200):
            H.apply(x, y)
        ctx.synchronize()
        reps = []
        for _ in range(5):
            t0 = time.perf_counter()
            ctx.timer_start()
            for _ in range(calls):
                H.apply(x, y)
            ms = ctx.timer_stop()
            reps.append((ms * 1e3 / calls, (time.perf_counter() - t0) * 1e6 / calls))
        out[f"spmv_n{n}_layout{variant}_us"] = round(float(np.median([r[0] for r in reps])), 4)
        out[f"spmv_n{n}_layout{variant}_host_us"] = round(float(np.median([r[1] for r in reps])), 4)
        assert H.layout_info()["variant"] == variant
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("run").add_argument("out")
    c = sub.add_parser("compare")
    c.add_argument("parent_a")
    c.add_argument("parent_b")
    c.add_argument("branch")
    c.add_argument("--jsonl", default=None)
    sub.add_parser("time").add_argument("--calls", type=int, default=4000)
    a = ap.parse_args()
    if a.cmd == "run":
        run(a.out)
        return 0
    if a.cmd == "time":
        time_products(a.calls)
        return 0
    from block_launcher_ab import compare
    return compare(a.parent_a, a.parent_b, a.branch, a.jsonl, fixed_order=fixed_order)


if __name__ == "__main__":
    sys.exit(main())
