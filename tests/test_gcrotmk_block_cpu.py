"""The lock-step GCROT driver (eigensolvers_amd.gcrotmk.gcrotmk_device_block) with REAL operands, as HipVector's
lock-step solves of a real shift drive it (the nBlock solves of one block Lanczos iteration, inexact_Lanczos.py:319-320),
on the CPU with a NumPy provider of the vector operations: the driver only changes WHEN things run, so every right-hand
side gets exactly the result of its single solve."""
import numpy as np

from eigensolvers_amd.gcrotmk import gcrotmk_device, gcrotmk_device_block
from eigensolvers_amd.generators import gapped_csr_host


class Buf(np.ndarray):
    """an ndarray that is its own "device pointer" (the solver fills x = 0 through hipeig_vec_fill(ptr))"""
    ptr = property(lambda self: self)


class RealNumpyOps:
    """float64 ndarrays in place of device buffers"""

    def __init__(self, n):
        self.n = n

    def new(self):
        return np.empty(self.n).view(Buf)

    def copy(self, a):
        return a.copy()

    def dot(self, a, b):
        return float(np.dot(a, b))

    def nrm2(self, a):
        return float(np.linalg.norm(a))

    def axpy(self, alpha, x, y):
        y += alpha * x

    def scal(self, alpha, x):
        x *= alpha

    def scaled(self, alpha, x):
        return alpha * x

    def arnoldi_step(self, vs, w):
        before = float(np.linalg.norm(w))
        h = np.zeros(len(vs))
        for j, v in enumerate(vs):
            h[j] = np.dot(v, w)
            w -= h[j] * v
        after = float(np.linalg.norm(w))
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = 1.0 / after
        if np.isfinite(alpha):
            w *= alpha
        return before, h, after

    def combine(self, coeffs, vecs):
        out = np.zeros(self.n)
        for c, v in zip(coeffs, vecs):
            out += c * v
        return out


class _Ctx:
    handle = None


def test_real_lock_step_driver_is_the_single_solves_bit_for_bit(monkeypatch):
    from eigensolvers_amd import gcrotmk as G
    monkeypatch.setattr(G._lib, "call", lambda name, h, ptr, n, val: ptr.fill(val))     # hipeig_vec_fill of x = 0
    n, sigma = 600, 0.02
    H = gapped_csr_host(n, 12, seed=3)
    A = lambda v: sigma * v - H @ v
    bs = [np.random.default_rng(s).standard_normal(n) for s in range(5)]
    bs.insert(2, np.zeros(n))                                  # a zero right-hand side drops out without a product

    single = [gcrotmk_device(_Ctx(), A, b.view(Buf), n, rtol=1e-8, atol=1e-12, maxiter=300, ops=RealNumpyOps(n)) for b in bs]
    sizes = []

    def block_matvec(vs):
        sizes.append(len(vs))
        return [A(v) for v in vs]

    block = gcrotmk_device_block(_Ctx(), block_matvec, [b.view(Buf) for b in bs], n, rtol=1e-8, atol=1e-12, maxiter=300,
                                 ops_factory=lambda: RealNumpyOps(n))
    for (x1, i1, s1), (xb, ib, sb) in zip(single, block):
        assert i1 == ib and s1 == sb
        np.testing.assert_array_equal(np.asarray(x1), np.asarray(xb))
    assert block[2][2]["matvecs"] == 0 and not np.any(np.asarray(block[2][0]))
    assert sizes[0] == len(bs) - 1 and max(sizes) == len(bs) - 1 and min(sizes) >= 1
