"""The single-vector operator sweep with MORE THAN ONE sweep launch, at a small shape (``csrc/sweep_launch.h``).

A blocked layout needs a second launch only when it has more workgroups' worth of row blocks than one launch holds; launch
``sw`` then starts at unit ``sw * gA`` (the wave-unit layout 3: ``sw * gA * 4``) and, in the solvers, leaves its per-workgroup
partial sums behind those of the launches before it.  With the automatic geometry that happens at full size only; here the
geometry is forced through the library's tuning knobs:

* layouts 4 and 5 (workgroup units, 5 with fixed-point accumulators): 64-row blocks, 1 Ki-column windows and one workgroup
  per CU and launch; n = 20000 gives 313 row blocks, two launches on anything with fewer than 313 CUs;
* layout 3 (wave units): 64-row units and one workgroup per CU and launch; n = 70001 gives 1094 units, four per workgroup,
  274 workgroups, two launches below 274 CUs.

The geometry is read from the environment when a layout is first built, so every test builds its own operator, and every
test asserts ``launches_per_apply() >= 2`` on it.  Operator ``gapped_csr_host(n, 16, seed=7)``, right-hand side the
normalised ``guess_vector(n, 1)``.  Every bound is that of the one-launch test of the same entry point
(``test_gpu_stream_layout.py``, ``test_gpu_parity.py``, ``test_gpu_precond_minres.py``, ``test_gpu_shifted_minres.py``)."""
import numpy as np
import pytest

import _precond_cases as pc
from _sweep_cases import (SHIFT_SETS, check_against_twin, check_kernel_forms, check_residuals, fixed_point_term, minres_opts,
                          product_bound, shifted_options)
from eigensolvers_amd.generators import gapped_csr_host
from oracle.minres_ref import minres as minres_ref

pytestmark = pytest.mark.gpu

SIGMA, RTOL, MAXITER = 0.02, 1e-8, 3000
GEOMETRY = {3: (70001, {"HIPEIG_TCOO_RW": "64", "HIPEIG_TCOO_WG_PER_CU": "1"}),
            4: (20000, {"HIPEIG_TCOOW_RW": "64", "HIPEIG_TCOOW_WBITS": "10", "HIPEIG_TCOOW_WG_PER_LAUNCH_CU": "1"})}
GEOMETRY[5] = GEOMETRY[4]

_problems = {}


def problem(n):
    """(host CSR, right-hand side, the oracle's plain solve), computed once per size and left unchanged."""
    if n not in _problems:
        Hh, b = gapped_csr_host(n, 16, seed=7), pc.unit_guess(n)
        xo, info, itn, istop = minres_ref(lambda v: SIGMA * v - Hh @ v, b, rtol=RTOL, maxiter=MAXITER)
        for a in (b, xo):
            a.setflags(write=False)
        _problems[n] = (Hh, b, (xo, itn, istop))
    return _problems[n]


@pytest.fixture(params=[3, 4, 5])
def two_launches(request, hip, monkeypatch):
    """(layout, host CSR, right-hand side, oracle solve, new_operator, check): ``new_operator()`` builds a fresh device
    operator pinned to the layout under the forced geometry; ``check(H)`` after a sweep asserts that it took two launches."""
    variant = request.param
    n, env = GEOMETRY[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    Hh, b, oracle = problem(n)

    def new_operator():
        H = hip.HipCsrOperator.from_scipy(Hh)
        H.set_variant(variant)
        return H

    def check(H):
        assert H.last_variant() == H.VARIANTS[variant]
        assert H.launches_per_apply() >= 2
        if variant in (4, 5):
            assert H.layout_info()["rows_per_block"] == 64

    return variant, Hh, b, oracle, new_operator, check


def test_product_and_shifted_product(hip, two_launches):
    """hipeig_spmv and hipeig_spmv_shift with both signs against the CSR-vector kernel (layout 1) on the same operator."""
    variant, Hh, b, _, new_operator, check = two_launches
    n = len(b)
    H = new_operator()
    ctx = hip.HipContext.default()
    x = hip.HipVector(b.copy())

    def products():
        out = [x.applyOp(H).array]
        for reverse in (False, True):
            ys = ctx.alloc(n)
            H.apply_shifted(SIGMA, x._buf, ys, reverse=reverse)
            out.append(hip.HipVector(ys).array)
        return out

    H.set_variant(1)
    refs = products()
    H.set_variant(variant)
    got = products()
    check(H)
    bound = product_bound(Hh, b) + (fixed_point_term(Hh, b) if variant == 5 else 0.0)
    used = [float(np.max(np.abs(g - r) / bound)) for g, r in zip(got, refs)]
    print(f"TWO-LAUNCH PRODUCT layout {variant}: largest |difference| / bound, product and the two shifted products: {used}")
    assert np.all(np.abs(got[0] - refs[0]) <= bound)
    for g, r in zip(got[1:], refs[1:]):
        assert np.all(np.abs(g - r) <= bound + 1e-16 * np.abs(b))
    assert np.all(np.abs(refs[0] - Hh @ b) <= product_bound(Hh, b))


def test_plain_minres_both_kernel_forms(hip, two_launches, monkeypatch):
    """The assertions of test_minres_two_and_three_kernel_forms_agree_in_every_sweep_layout.  A wrong partial offset of the
    second launch gives a wrong alfa in the first iteration; the count cannot survive that.  (The oracle ends with istop 1
    after 642 iterations at n = 20000 and 644 at n = 70001, and keeps both counts under other summation orders of its
    product.)"""
    variant, Hh, b, (xo, itn, istop), new_operator, check = two_launches
    out = []
    for form in (None, "0"):
        monkeypatch.delenv("HIPEIG_MINRES_FUSE_KD", raising=False)
        if form:
            monkeypatch.setenv("HIPEIG_MINRES_FUSE_KD", form)
        H = new_operator()
        W = hip.HipVector.solve(H, hip.HipVector(b.copy(), minres_opts(MAXITER, RTOL)), SIGMA)
        check(H)
        out.append((W.array, W.last_solve_stats))
    monkeypatch.delenv("HIPEIG_MINRES_FUSE_KD", raising=False)
    (x2, s2), (x3, s3) = out
    print(f"TWO-LAUNCH MINRES layout {variant}: iterations {s2['iterations']} / {s3['iterations']} (oracle {itn}), |x2 - x3| / |x| "
          f"{np.linalg.norm(x2 - x3) / np.linalg.norm(xo):.2e}, |x2 - oracle| / |x| {np.linalg.norm(x2 - xo) / np.linalg.norm(xo):.2e}")
    check_kernel_forms(f"layout {variant}", variant in (3, 5), x2, s2, x3, s3, xo, itn, istop)


def test_jacobi_minres(hip, two_launches):
    variant, Hh, b, _, new_operator, check = two_launches
    tw = pc.twin(f"two-launch g{len(b)}", Hh, b, SIGMA, RTOL, MAXITER)
    H = new_operator()
    o = minres_opts(MAXITER, RTOL)
    o["linearSystemArgs"]["preconditioner"] = "jacobi"
    W = hip.HipVector.solve(H, hip.HipVector(b.copy(), o), SIGMA)
    check(H)
    check_against_twin(f"two launches, layout {variant}", Hh, b, SIGMA, RTOL, W, tw)


def test_shifted_minres(hip, two_launches):
    variant, Hh, b, _, new_operator, check = two_launches
    shifts = SHIFT_SETS[3]
    H = new_operator()
    xs = hip.solve_shifts(H, hip.HipVector(b.copy(), shifted_options(1e-5, 1e-7)), shifts)
    check(H)
    check_residuals(Hh, b, shifts, xs, 1.0, 1e-5, 1e-7)
