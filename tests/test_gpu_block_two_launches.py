"""The window-blocked block sweep with MORE THAN ONE sweep launch, at a small shape (``csrc/block_sweep_launch.h``).

A window-blocked layout needs a second launch only when it has more row blocks than the device has CUs; launch ``sw`` then
starts at row block ``sw * gA`` and, in the solvers, leaves its per-workgroup partial sums behind those of the launches
before it.  With the automatic geometry that happens from N ~ 6.5e5 on; here the geometry is forced through the library's
tuning knobs to its own lower limit of 8 rows per block (``hipeig_block_pick_variant``): n = 4000 gives 500 row blocks
(and 8 column windows of 512), two launches on anything with fewer than 500 CUs.  The layout geometry is read from the
environment when the layout is first built, so every test builds its own operator.

Every bound is that of the one-launch test of the same entry point (``test_gpu_block.py``, ``test_gpu_lanczos_filter.py``)."""
import numpy as np
import pytest

from _block_cases import block_solve, check_block_solve, within
from _lanczos_cases import EPS, LO, W8, Z8, check_filter, check_steps, device_columns, host_operator, lf, twin

pytestmark = pytest.mark.gpu

N = 4000


@pytest.fixture
def two_launches(hip, gapped4000, monkeypatch):
    """(host CSR, fresh device operator pinned to the window-blocked kernel, check): ``check()`` after a block call asserts
    that the call ran on 8-row blocks and that there are more of them than CUs - the condition for a second launch."""
    monkeypatch.setenv("HIPEIG_BCOO_RW", "8")
    monkeypatch.setenv("HIPEIG_BCOO_WBITS", "9")
    Hh, _ = gapped4000
    H = hip.HipCsrOperator.from_scipy(Hh)
    H.set_block_variant(2)

    def check():
        info = H.block_info()
        assert info["variant"] == "column-window-blocked"
        assert info["rows_per_block"] == 8
        assert info["row_blocks"] > H.ctx.device_info()["cus"]
        return info

    return Hh, H, check


def test_product_and_shifted_product(hip, two_launches):
    """hipeig_spmm, k = 5 and 8 (the 8-wide block), and hipeig_spmm_shift - the same host path with another epilogue."""
    Hh, H, check = two_launches
    rng = np.random.default_rng(3)
    Habs = np.abs(Hh)
    for k in (5, 8):
        Xh = rng.standard_normal((N, k))
        Y = H.apply_block([hip.HipVector(Xh[:, j].copy())._buf for j in range(k)])
        info = check()
        assert info["row_blocks"] == N // 8 and info["windows"] == (N + 511) // 512
        ref, bound = Hh @ Xh, 1e-14 * (Habs @ np.abs(Xh))
        for j in range(k):
            within(hip.HipVector(Y[j]).array, ref[:, j], bound[:, j])
        # y = rn(rn(sigma x) + rn(-(H x))): the product's bound, half an ulp of the shift term, half an ulp of the result
        sigma = 0.02
        Ys = H.apply_shifted_block(sigma, [hip.HipVector(Xh[:, j].copy())._buf for j in range(k)])
        check()
        refs = sigma * Xh - ref
        bounds = bound + EPS * (np.abs(sigma * Xh) + np.abs(refs))
        for j in range(k):
            within(hip.HipVector(Ys[j]).array, refs[:, j], bounds[:, j])


@pytest.mark.parametrize("k", [8, 3])
def test_block_minres(hip, two_launches, k):
    """hipeig_minres_block on both interleave widths: the assertions of test_block_minres_equals_the_single_solves.  A
    wrong partial offset of the second launch gives a wrong alfa in the first iteration; the counts cannot survive that."""
    Hh, H, check = two_launches
    rtol = 1e-8
    rng = np.random.default_rng(17 + k)
    B = rng.standard_normal((N, k))
    B /= np.linalg.norm(B, axis=0)
    X, vecs = block_solve(hip, H, B, 0.02, 2000, rtol)
    check()
    check_block_solve(hip, H, Hh, B, X, vecs, rtol)


@pytest.mark.parametrize("keep", [True, False])
def test_lanczos_filter_both_passes(hip, two_launches, keep):
    """lanczos_run + combine with 8 columns: pass 1's sweep, and pass 2 as the stream over a kept basis (keep) or - ring of
    three, nothing kept - as the product steps, the second kernel that goes through the launcher."""
    Hh, H, check = two_launches
    name, K = "gapped4000", 8
    assert abs(Hh - host_operator(name)).max() == 0.0          # the spectrum and the twins are cached under this name
    rtol, atol = LO
    B = np.random.default_rng(9).standard_normal((K, N))
    B /= np.linalg.norm(B, axis=1)[:, None]
    cols = device_columns(hip, B, rtol, atol)
    run = hip.lanczos_run(H, cols, Z8, keepBasis=keep)
    check()
    try:
        assert run.converged and run.basis_kept == [keep]
        qs = run.combine(lf.filter_coefficients(run.scalars, Z8, W8))
    finally:
        run.release()
    check()
    if not keep:
        assert run.products_pass2 == [run.products_pass1[0] - 1]          # the product steps really ran
    for r in range(K):
        its, est, conv, xnorms = twin((name, r), Hh, B[r], Z8, rtol, atol, 1.0)
        assert conv.all()
        label = f"{name} two launches K={K} keep={keep} column={r}"
        check_steps(label, run.scalars[r].iterations, its)
        check_filter(label, name, Hh, B[r], qs[r].array, Z8, W8, xnorms, max(atol, rtol), 1.0)
