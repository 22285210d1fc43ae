"""Helpers shared by the device tests of the block path (``test_gpu_block.py``, ``test_gpu_block_two_launches.py``).  A plain
module, imported as ``_lanczos_cases`` is: no fixtures, no tests.

Tolerances: products 1e-14 of the row's absolute sum; per-column MINRES iteration counts and stop codes EQUAL to the
single-vector solve; iterates within max(1e-9, 100 rtol) ||x|| of the oracle (two correctly rounded MINRES runs agree to
the solve tolerance, see test_gpu_parity.py)."""
import numpy as np

from oracle.minres_ref import minres as minres_ref


def within(got, ref, bound):
    got, ref, bound = np.asarray(got), np.asarray(ref), np.asarray(bound)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    assert not bad.any(), f"max excess {np.max(err - bound):.3e} at {int(np.argmax(err - bound))}, {int(bad.sum())} elements"


def opts(it=2000, tol=1e-10, **extra):
    d = {"linearSystemArgs": {"linearSolver": "minres", "linearIter": it, "linear_tol": tol}}
    d.update(extra)
    return d


def block_solve(hip, H, B, sigma, it, tol, reverse=False):
    vecs = [hip.HipVector(B[:, j].copy(), opts(it, tol)) for j in range(B.shape[1])]
    out = hip.HipVector.solveBlock(H, vecs, sigma, reverseGF=reverse)
    return out, vecs


def check_block_solve(hip, H, Hh, B, X, vecs, rtol, sigma=0.02, it=2000):
    """Column j of the lock-step solve ``X`` of ``sigma - H`` against hipeig_minres on b_j alone and against the oracle:
    iteration count and stop code equal, iterate within the solve tolerance of both."""
    assert len(X) == B.shape[1]
    for j in range(B.shape[1]):
        st = X[j].last_solve_stats
        if not np.any(B[:, j]):
            assert st["iterations"] == 0 and np.all(X[j].array == 0.0)
            continue
        xo, info, itn, istop = minres_ref(lambda v: sigma * v - Hh @ v, B[:, j], rtol=rtol, maxiter=it)
        single = hip.HipVector.solve(H, hip.HipVector(B[:, j].copy(), opts(it, rtol)), sigma)
        ss = single.last_solve_stats
        assert (st["iterations"], st["istop"]) == (ss["iterations"], ss["istop"]), f"column {j}"
        assert (st["iterations"], st["istop"]) == (itn, istop), f"column {j} vs oracle"
        xtol = max(1e-9, 100 * rtol) * np.linalg.norm(xo)
        within(X[j].array, xo, xtol)
        within(X[j].array, single.array, xtol)
        assert abs(st["rnorm"] - ss["rnorm"]) <= 0.05 * ss["rnorm"] + 1e-300      # the estimate moves with the summation order
        assert vecs[j].last_solve_stats is st
