#!/usr/bin/env python3
"""One FEAST iteration (maxit = 1) of config #5's recipe (tools/bench_configs.py: the generated gapped operator, 16
subspace vectors, 16 Legendre nodes = 8 contour points, window [-0.21, 0.21], inner rtol 1e-5 / atol 1e-7) with the
``gcrotmk`` path as it stands (one contour point at a time, its 16 solves in lock step) and with
``linearSolver="minres_shifted"`` (one shared-Lanczos solve per subspace vector for all 8 points) and with
``linearSolver="lanczos_filter"`` (mode ``filter``: the filtered vectors from two Lanczos passes, 8 vectors in lock step
on block products, no per-shift vector) and with the same plus ``"lanczosBasis": "keep"`` (mode ``basis``: pass 1 keeps its
vectors in device memory and pass 2 is one stream over them) and with that plus ``"lanczosBasisPrefix": True`` (mode
``prefix``: a basis that outgrows the byte budget keeps the vectors that fit, and pass 2 repeats only the products behind
them) and with ``basis`` / ``prefix`` plus ``"lanczosBasisPrecision": "fp32"`` (modes ``basis32`` / ``prefix32``: the basis
stored in fp32, twice the vectors per byte), the modes alternating.  One JSON line per run as soon as it
is measured; the first line describes the device.

Then the per-phase split of one shared solve (``--phases``, default on): the whole 8-shift solve of the first subspace
vector timed with ``hipeig_timer_*``, and each of its three kernels alone (HIPEIG_MS_PROBE = 1 sweep / 2 second kernel /
3 update pass: that kernel launched ``--probe-steps`` times on a state record that does not advance), next to
``hipeig_spmv`` at the same size and to the update pass's byte model (8 n + 80 n per live shift).  For the ``filter`` mode:
one 8-column run with pass 1, the host's coefficients and pass 2 timed apart, pass 1's three kernels alone
(HIPEIG_LF_PROBE = 1 sweep / 2 second kernel / 3 scalar kernel), and the block sweep's time per column.  For the ``basis``
mode: one 8-column run with the keeping pass 1 and the combination from the kept basis timed apart - the combination's ms
per group and its TB/s against the byte model 8 n K m + 8 n K NC (m slots read, NC outputs written), for NC = 1, 2 and 8 -
and the bytes the basis holds.  For the ``basis32`` mode the same split on the fp32 basis (``basis32_phases``), byte model
4 n K m + 8 n K NC.

    python tools/shifted_feast_bench.py [--n 1000000 --reps 3 --modes gcrotmk,shifted,filter,basis,prefix,basis32,prefix32] >> profiles/NN_shifted_feast.jsonl

``--cpu``: instead, the NumPy twins on the host generator's operator (small N): products per shift of the shared-Lanczos
solver, and the two-pass filter's products and its difference from the former's sum; no timing claims;
``--cpu-gcrotmk`` adds SciPy ``gcrotmk``'s product counts for the same points.
"""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def contour(nc):
    from eigensolvers_amd import feast as pf
    gk, _ = pf.quadraturePointsWeights(nc, "legendre", positiveHalf=True)
    return [pf.contour_point(-0.21, 0.21, g)[1] for g in gk]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m0", type=int, default=16)
    ap.add_argument("--nc", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="gcrotmk,shifted")
    ap.add_argument("--cols", type=int, default=4, help="arnoldiColumnsPerPass of the gcrotmk mode")
    ap.add_argument("--phases", type=int, default=1)
    ap.add_argument("--probe-steps", type=int, default=200)
    ap.add_argument("--basis-bytes", type=int, default=None, help="byte budget of the basis and prefix modes (default: the library's rule)")
    ap.add_argument("--label", default="")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cpu-gcrotmk", action="store_true", help="with --cpu: also count SciPy gcrotmk's products per point")
    a = ap.parse_args()
    import numpy as np
    import scipy.linalg as la

    N, m0 = a.n, a.m0
    rng = np.random.default_rng(9)
    if a.cpu:
        from eigensolvers_amd.generators import gapped_csr_host
        from eigensolvers_amd.shifted_minres import shifted_minres_host
        H = gapped_csr_host(N, 32, seed=7)
        b = rng.standard_normal(N)
        b /= np.linalg.norm(b)
        t0 = time.perf_counter()
        x, its, est, conv = shifted_minres_host(lambda v: H @ v, b, contour(a.nc), 1e-5, 1e-7, 4000)
        print(json.dumps({"label": a.label, "N": N, "mode": "twin", "seconds": round(time.perf_counter() - t0, 3),
                          "iterations": [int(i) for i in its], "products": int(its.max()),
                          "converged": bool(conv.all())}), flush=True)
        import importlib
        import math
        from eigensolvers_amd import feast as pf
        lf = importlib.import_module("eigensolvers_amd.lanczos_filter")
        gk, wk = pf.quadraturePointsWeights(a.nc, "legendre", positiveHalf=True)
        ws = [-0.5 * w * 0.21 * (math.cos(pf.contour_point(-0.21, 0.21, g)[0]) + 1j * math.sin(pf.contour_point(-0.21, 0.21, g)[0]))
              for g, w in zip(gk, wk)]
        t0 = time.perf_counter()
        q, sc = lf.lanczos_filter_host(lambda v: H @ v, b, contour(a.nc), ws, 1e-5, 1e-7, 4000)
        ref = sum((w * xj).real for w, xj in zip(ws, x))
        m = int(sc[0].iterations.max())
        print(json.dumps({"label": a.label, "N": N, "mode": "filter_twin", "seconds": round(time.perf_counter() - t0, 3),
                          "iterations": [int(i) for i in sc[0].iterations], "products_pass1": m, "products_pass2": m - 1,
                          "relative_difference_to_twin_sum": float(np.linalg.norm(q[0] - ref) / np.linalg.norm(ref))}), flush=True)
        if a.cpu_gcrotmk:                                           # SciPy's gcrotmk, the reference's solver, point by point
            import scipy.sparse.linalg as spla
            cnt = []
            for z in contour(a.nc):
                c = [0]

                def mv(u, z=z, c=c):
                    c[0] += 1
                    return z * u - H @ u
                op = spla.LinearOperator((N, N), matvec=mv, dtype=complex)
                spla.gcrotmk(op, b.astype(complex), rtol=1e-5, atol=1e-7, maxiter=4000)
                cnt.append(c[0])
            print(json.dumps({"label": a.label, "N": N, "mode": "scipy_gcrotmk", "complex_products_per_point": cnt,
                              "complex_products": int(sum(cnt))}), flush=True)
        return

    import eigensolvers_amd as ea
    lsa = {"gcrotmk": {"linearSolver": "gcrotmk", "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7,
                       "arnoldiColumnsPerPass": a.cols},
           "shifted": {"linearSolver": "minres_shifted", "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7},
           "filter": {"linearSolver": "lanczos_filter", "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7},
           "basis": {"linearSolver": "lanczos_filter", "linearIter": 4000, "linear_tol": 1e-5, "linear_atol": 1e-7}}
    lsa["prefix"] = dict(lsa["basis"])
    lsa["basis32"], lsa["prefix32"] = dict(lsa["basis"]), dict(lsa["basis"])
    extra = {"basis": {"lanczosBasis": "keep"}, "prefix": {"lanczosBasis": "keep", "lanczosBasisPrefix": True}}
    extra["basis32"] = dict(extra["basis"], lanczosBasisPrecision="fp32")
    extra["prefix32"] = dict(extra["prefix"], lanczosBasisPrecision="fp32")
    if a.basis_bytes is not None:
        for mode in extra:
            extra[mode]["lanczosBasisBytes"] = a.basis_bytes
    Y0 = la.qr(rng.standard_normal((N, m0)), mode="economic")[0]
    ctx = ea.HipContext.default()
    print(json.dumps({"device": ctx.device_info()["name"], "N": N, "m0": m0, "contour_points": a.nc // 2, "reps": a.reps,
                      "label": a.label}), flush=True)
    H = ea.HipCsrOperator.generate(N, 32, seed=7)
    counts = {"pairs": 0, "single": 0}
    inner_pairs, inner_pair = ea.HipCsrOperator.apply_shifted_pairs, ea.HipCsrOperator.apply_shifted_pair

    def counted_pairs(self, z, xs, reverse=False):
        counts["pairs"] += len(xs)
        return inner_pairs(self, z, xs, reverse=reverse)

    def counted_pair(self, *args, **kw):
        counts["single"] += 1
        return inner_pair(self, *args, **kw)
    ea.HipCsrOperator.apply_shifted_pairs = counted_pairs
    ea.HipCsrOperator.apply_shifted_pair = counted_pair

    modes = [m for m in a.modes.split(",") if m]
    for rep in range(a.reps):
        for mode in (modes if rep % 2 == 0 else modes[::-1]):
            counts.update(pairs=0, single=0)
            Y = [ea.HipVector(Y0[:, i].copy(), dict(extra.get(mode, {}), linearSystemArgs=dict(lsa[mode])), ctx=ctx)
                 for i in range(m0)]
            ctx.synchronize()
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ev, Yf, st = ea.feastDiagonalization(H, Y, a.nc, "legendre", -0.21, 0.21, 1e-4, 1, writeOut=False)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            row = {"label": a.label, "N": N, "mode": mode, "rep": rep, "seconds": round(dt, 3),
                   "eigenvalues_in_window": int(np.sum((ev >= -0.21) & (ev <= 0.21)))}
            if mode == "shifted":
                rec = st["sharedLanczos"][0]
                row.update({"solves": rec["solves"], "real_products": int(sum(rec["products"])),
                            "products_per_vector": [int(p) for p in rec["products"]],
                            "iterations_per_point_min_max": [[int(min(i for (k, v), i in zip(rec["pairs"], rec["iterations"]) if k == kk)),
                                                              int(max(i for (k, v), i in zip(rec["pairs"], rec["iterations"]) if k == kk))]
                                                             for kk in range(a.nc // 2)]})
            elif mode in ("filter", "basis", "prefix", "basis32", "prefix32"):
                rec = st["lanczosFilter"][0]
                row.update({"runs": rec["runs"], "block_products_pass1": rec["products_pass1"],
                            "block_products_pass2": rec["products_pass2"], "basis": rec["basis"],
                            "basis_vectors": rec.get("basis_vectors"), "basis_precision": rec.get("basis_precision"),
                            "steps_per_point_min_max": [[int(min(i for (k, v), i in zip(rec["pairs"], rec["steps"]) if k == kk)),
                                                         int(max(i for (k, v), i in zip(rec["pairs"], rec["steps"]) if k == kk))]
                                                        for kk in range(a.nc // 2)]})
            else:
                row.update({"complex_products": counts["pairs"] + counts["single"]})
            print(json.dumps(row), flush=True)

    if a.phases and "shifted" in modes:
        zs = contour(a.nc)
        S = len(zs)
        b = ea.HipVector(Y0[:, 0].copy(), {"linearSystemArgs": dict(lsa["shifted"])}, ctx=ctx)
        os.environ.pop("HIPEIG_MS_PROBE", None)
        ea.solve_shifts(H, b, zs)                                   # warm (workspace, operator copy)
        ctx.timer_start()
        ea.solve_shifts(H, b, zs)
        whole_ms = ctx.timer_stop()
        st = b.last_solve_stats
        live_steps = int(sum(st["iterations"]))                    # shift-steps the update passes carried
        # hipeig_spmv at the same size, the yardstick of the sweep
        y = ctx.alloc(N)
        H.apply(b._buf, y)
        ctx.timer_start()
        for _ in range(a.probe_steps):
            H.apply(b._buf, y)
        spmv_ms = ctx.timer_stop() / a.probe_steps
        phase = {}
        bp = ea.HipVector(Y0[:, 0].copy(), {"linearSystemArgs": dict(lsa["shifted"], linearIter=a.probe_steps)}, ctx=ctx)
        for key, name in (("1", "sweep"), ("2", "second_kernel"), ("3", "update_pass")):
            os.environ["HIPEIG_MS_PROBE"] = key
            try:
                for timed in (False, True):
                    ctx.timer_start()
                    try:
                        ea.solve_shifts(H, bp, zs)
                    except UserWarning:
                        pass                                        # a probe run never converges
                    ms = ctx.timer_stop()
                phase[name] = ms / a.probe_steps
            finally:
                os.environ.pop("HIPEIG_MS_PROBE", None)
        upd_bytes = (8 + 80 * S) * N                                # all S shifts live in the probe
        print(json.dumps({"label": a.label, "N": N, "mode": "phases", "shifts": S, "products": st["products"],
                          "iterations": st["iterations"], "whole_solve_ms": round(whole_ms, 3),
                          "ms_per_step": round(whole_ms / st["products"], 5),
                          "mean_live_shifts": round(live_steps / st["products"], 3),
                          "probe_steps": a.probe_steps,
                          "sweep_ms": round(phase["sweep"], 5), "second_kernel_ms": round(phase["second_kernel"], 5),
                          "update_pass_ms_all_live": round(phase["update_pass"], 5),
                          "hipeig_spmv_ms": round(spmv_ms, 5),
                          "update_pass_TBps": round(upd_bytes / (phase["update_pass"] * 1e-3) / 1e12, 3),
                          "second_kernel_TBps": round(24 * N / (phase["second_kernel"] * 1e-3) / 1e12, 3)}), flush=True)

    if a.phases and "filter" in modes:
        import importlib
        import math
        from eigensolvers_amd import feast as pf
        lf = importlib.import_module("eigensolvers_amd.lanczos_filter")
        zs = contour(a.nc)
        gk, wk = pf.quadraturePointsWeights(a.nc, "legendre", positiveHalf=True)
        ws = [-0.5 * w * 0.21 * (math.cos(pf.contour_point(-0.21, 0.21, g)[0]) + 1j * math.sin(pf.contour_point(-0.21, 0.21, g)[0]))
              for g, w in zip(gk, wk)]
        K = min(8, m0)
        B = [ea.HipVector(Y0[:, i].copy(), {"linearSystemArgs": dict(lsa["filter"])}, ctx=ctx) for i in range(K)]
        os.environ.pop("HIPEIG_LF_PROBE", None)
        ea.lanczos_filter(H, B, zs, ws)                             # warm (workspace, operator copy)
        ctx.timer_start()
        run = ea.lanczos_run(H, B, zs)
        pass1_ms = ctx.timer_stop()
        t0 = time.perf_counter()
        G = lf.filter_coefficients(run.scalars, zs, ws)
        host_ms = (time.perf_counter() - t0) * 1e3
        ctx.timer_start()
        run.combine(G)
        pass2_ms = ctx.timer_stop()
        p1, p2 = run.products_pass1[0], run.products_pass2[0]
        y = ctx.alloc(N)
        H.apply(B[0]._buf, y)
        ctx.timer_start()
        for _ in range(a.probe_steps):
            H.apply(B[0]._buf, y)
        spmv_ms = ctx.timer_stop() / a.probe_steps
        phase = {}
        Bp = [ea.HipVector(Y0[:, i].copy(), {"linearSystemArgs": dict(lsa["filter"], linearIter=a.probe_steps)}, ctx=ctx)
              for i in range(K)]
        for key, name in (("1", "sweep"), ("2", "second_kernel"), ("3", "scalar_kernel")):
            os.environ["HIPEIG_LF_PROBE"] = key
            try:
                for timed in (False, True):
                    ctx.timer_start()
                    ea.lanczos_run(H, Bp, zs)                       # a probe run never converges; lanczos_run only reports
                    ms = ctx.timer_stop()
                phase[name] = ms / a.probe_steps
            finally:
                os.environ.pop("HIPEIG_LF_PROBE", None)
        print(json.dumps({"label": a.label, "N": N, "mode": "filter_phases", "columns": K, "shifts": len(zs),
                          "block_variant": H.block_info()["variant"],
                          "block_products_pass1": p1, "block_products_pass2": p2,
                          "pass1_ms": round(pass1_ms, 3), "host_coefficients_ms": round(host_ms, 3), "pass2_ms": round(pass2_ms, 3),
                          "pass1_ms_per_step": round(pass1_ms / p1, 5), "pass2_ms_per_step": round(pass2_ms / max(p2, 1), 5),
                          "probe_steps": a.probe_steps, "sweep_ms": round(phase["sweep"], 5),
                          "second_kernel_ms": round(phase["second_kernel"], 5), "scalar_kernel_ms": round(phase["scalar_kernel"], 5),
                          "sweep_ms_per_column": round(phase["sweep"] / K, 5), "hipeig_spmv_ms": round(spmv_ms, 5),
                          "second_kernel_TBps": round(24 * N * K / (phase["second_kernel"] * 1e-3) / 1e12, 3)}), flush=True)

    for precision, key in (("fp64", "basis"), ("fp32", "basis32")):
        if not (a.phases and key in modes):
            continue
        import importlib
        import math
        from eigensolvers_amd import feast as pf
        lf = importlib.import_module("eigensolvers_amd.lanczos_filter")
        zs = contour(a.nc)
        gk, wk = pf.quadraturePointsWeights(a.nc, "legendre", positiveHalf=True)
        ws = [-0.5 * w * 0.21 * (math.cos(pf.contour_point(-0.21, 0.21, g)[0]) + 1j * math.sin(pf.contour_point(-0.21, 0.21, g)[0]))
              for g, w in zip(gk, wk)]
        K = min(8, m0)
        B = [ea.HipVector(Y0[:, i].copy(), {"linearSystemArgs": dict(lsa["basis"])}, ctx=ctx) for i in range(K)]
        os.environ.pop("HIPEIG_LF_PROBE", None)
        ea.lanczos_filter(H, B, zs, ws, basis="keep", basisBytes=a.basis_bytes, precision=precision)   # warm (workspace, operator copy, reusable segments)
        ctx.timer_start()
        run = ea.lanczos_run(H, B, zs, keepBasis=True, basisBytes=a.basis_bytes, basisPrecision=precision)
        pass1_ms = ctx.timer_stop()
        kept, held = run.basis_kept, run.basis_bytes
        t0 = time.perf_counter()
        G = lf.filter_coefficients(run.scalars, zs, ws)
        host_ms = (time.perf_counter() - t0) * 1e3
        width = 4 if K <= 4 else 8
        m = max(len(g) for g in G)
        elem = 4.0 if precision == "fp32" else 8.0
        row = {"label": a.label, "N": N, "mode": key + "_phases", "columns": K, "shifts": len(zs),
               "basis_precision": precision,
               "block_variant": H.block_info()["variant"], "basis_kept": kept, "basis_bytes": held,
               "block_products_pass1": run.products_pass1[0], "pass1_keep_ms": round(pass1_ms, 3),
               "pass1_keep_ms_per_step": round(pass1_ms / run.products_pass1[0], 5),
               "host_coefficients_ms": round(host_ms, 3), "slots_read": m}
        rng2 = np.random.default_rng(3)
        for nc in (1, 2, 8):
            if nc > 2 and not all(kept):
                continue                                            # the product pass serves NC = 1 and 2 only
            Gn = G if nc == 1 else [np.repeat(g, nc, axis=1) * rng2.standard_normal((1, nc)) for g in G]
            times = []
            for _ in range(max(3, a.reps)):
                ctx.timer_start()
                run.combine(Gn)
                times.append(ctx.timer_stop())
            model = elem * N * width * m + 8.0 * N * width * nc
            best, med = min(times), sorted(times)[len(times) // 2]
            row.update({f"combine_nc{nc}_ms_per_group": [round(t, 3) for t in times],
                        f"combine_nc{nc}_ms_median": round(med, 3), f"combine_nc{nc}_model_bytes": int(model),
                        f"combine_nc{nc}_TBps_median": round(model / (med * 1e-3) / 1e12, 3),
                        f"combine_nc{nc}_TBps_best": round(model / (best * 1e-3) / 1e12, 3)})
            row[f"block_products_pass2_nc{nc}"] = run.products_pass2[0]
        run.release()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
