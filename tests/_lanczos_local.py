"""Local relations of the Lanczos filter's passes (``csrc/lanczos_filter.hip``) against extended precision: reference,
bounds and their derivation.  A plain module, imported as ``_hiprec`` is: no fixtures, no tests.

A Lanczos recurrence amplifies rounding, so a device run cannot be held to a reference run step by step.  One step can:
whatever the vectors have drifted to, ``beta_{i+1} v_{i+1} = H v_i - alpha_i v_i - beta_i v_{i-1}`` holds to a few
roundings per element (Paige).  Everything here is therefore evaluated in ``longdouble`` from the *device's own*
``v_{i-1}, v_i, v_{i+1}, alpha_i, beta_i, beta_{i+1}``.  u = 2^-53; starred quantities are the reference's.

Reading the device's vectors.  ``LanczosRun.combine`` with tables that are slices of the identity returns
``v_i = rn(s_i r_i)``, ``s_i = rn(1 / beta_i)``, of the un-normalised ``r_i`` the device holds, exactly: the stream forms
``fma(1.0, v, 0.0)`` and ``fma(0.0, v, a)`` for every other term, the product pass the same on ``Q``.  It is the ``v`` the
sweep epilogue forms for ``<v, w>`` and the one every combination is built from.  A kept basis serves 8 slices per call,
the product pass 2 (``read_vectors``).

What an element goes through (``LfScalarsEpilogue::elem``, then ``lf_kc_kernel``; ``LfCombineEpilogue::elem`` is the
same expression), with ``c1 = rn(beta_i / beta_{i-1})``, ``c = rn(alpha_i / beta_i)``:

    sum     = sum_j H_rj r_i[j]                          L_row roundings, whatever the order of the row's adds
    r_{i+1} = fma(-c, r_i, fma(-c1, r_{i-1}, rn(s_i sum)))

``r_i[j] = v_i[j] / (s_i (1 + d_j))`` with ``|d_j| <= u``, so ``s_i`` cancels in ``s_i sum`` and the operator term of
``w* = H v_i - beta_i v_{i-1}`` carries 1 (d_j) + L_row (the sum: every term passes its product and at most L_row - 1
adds that are not adds of zero, in any tree) + 1 (the ``mul_rn``) roundings, then the two ``fma``'s: L_row + 4.
``c1 r_{i-1} = beta_i v_{i-1}`` to the roundings of the division, of ``s_{i-1}`` and of ``d``, then two ``fma``'s: 5.
``c r_i = alpha_i v_i`` likewise with one ``fma``: 4.  Reading ``v_{i+1}`` multiplies by ``s_{i+1}``: 2 more on everything.
So with ``c_vec(L) = L + 7`` and 1.01 for the second-order terms

 a  |beta_0 - ||b||*| <= 1.01 (c_dot / 2 + 1) u ||b||*           hipeig_dot's tree (``c_dot``), a square root
    |v_0 - b / beta_0| <= 2.01 u |b / beta_0|                     two roundings per element
 b  |beta_{i+1} v_{i+1} - (w* - alpha_i v_i)| <= 1.01 c_vec(L_row) u (|H||v_i| + beta_i |v_{i-1}| + |alpha_i||v_i|)_row
    in the multiplied form - no division by beta_{i+1} - so a step next to a breakdown stays checkable.
 c  |alpha_i - <v_i, w*>| <= 1.01 [c_vw u sum |v_i| (|w*| + e_w) + sum |v_i| e_w],
    e_w = u ((L_row + 3) |H||v_i| + 4 beta_i |v_{i-1}|)_row  the error of the sweep's own w (relation b without KC)
 d  | ||v_{i+1}||* - 1 | <= 1.01 (c_ww / 2 + 3) u          the <w, w> sum, the square root, 1 / beta, the readout

``c_vw`` and ``c_ww`` are the depths of the two reduction trees (``sweep_trees``): the additions the most travelled term
goes through, read off the code.

    sweep, row-owner   a wave owns the rows wave, wave + nwaves, ..: ceil(n / (4 G)) fma's in a thread, G =
                       min(ceil(n / 4), 8 CUs, 2048) workgroups; block_reduce_cols: log2(64 / K) shuffles, 3 adds of the
                       four waves
    sweep, window-bl.  a workgroup owns rows_per_block rows; which thread takes which element is fixed, the worst order
                       over the workgroup's whole share is taken anyway: rows_per_block
    KC                 ceil(n K / 2 / (256 G_E)) fma's, G_E = grid_for(n K / 2, 32); block_reduce_pairs:
                       log2(128 / K) shuffles, 3 adds
    the records        block_sum_partials_cols over P records of K: ceil(P K / 256) adds in a thread, log2(64 / K)
                       shuffles, 3 adds.  P = G, G_E, or for the window-blocked sweep its launches' workgroups, at most
                       twice the row blocks (records of workgroups past the last block hold zeros)

The grid formulas are mirrored only to size the bounds.

Rotation.  ``rotation`` runs the recurrence of ``lf_scalar_kernel`` / ``_scalars_one`` on given ``alphas``, ``betas`` in
any complex type.  In ``clongdouble`` on the device's scalars it is the reference of ``estimates`` (``|tau*|`` at the
reported step, relative ``DELTA``) and of ``iterations`` (the first step with ``|tau*_k| <= target``).  ``DELTA`` is 8
times the largest relative deviation of the float64 recurrence from the ``clongdouble`` one over the cases below
(``measured_rotation_deviation``; EXPERIMENTS.md holds the figure): the device splits real and imaginary parts and takes
``hypot(hypot())``, other roundings at the same conditioning.  The equality of the steps is a condition on the inputs: a
(column, shift) whose ``|tau*_k|`` comes within ``2 DELTA`` relative of the target at or before its stop is left out, no
more than 1 in 20 per test, and none on the host twin's scalars (``test_lanczos_local_cpu.py``).

Combination.  ``combine(G)`` against ``hp.combine(V_device, G)`` per element: one ``mul_rn`` (the readout's own), m
``fma``'s in ascending order, contraction off: ``(m + 2) u Yabs``.  From an fp32 basis the terms the stream serves add
``2^-24 (1 + 2^-20) Yabs_stream``; a stored vector read back obeys ``|v32 - v64| <= 2^-24 (1 + 2^-20) |v64|``, the
readout's rounding included.  ``tables`` draws the coefficients from a seeded ``standard_normal`` with magnitudes spread
over 2^-8 .. 2^4 across the steps, so every term matters, the last included.
"""
import math

import numpy as np

import _hiprec as hp
from _lanczos_cases import LO, host_operator, lf

U = 2.0 ** -53
U32 = 2.0 ** -24 * (1.0 + 2.0 ** -20)
TINY = 1e-300
LD, CLD = hp.LD, hp.CLD
MEASURED_DEVIATION = 30.4        # in u: measured_rotation_deviation over the cases below (the masking block's 102 steps)
DELTA = 8 * MEASURED_DEVIATION * U
ASSUMED_CUS = 256                # an MI355X; the CPU test sizes its trees with it

# the inputs of the device test (tests/test_gpu_lanczos_local.py); the CPU test holds the host twins to the same bounds
# on them.  (operator, columns, sign, step limit): the limit keeps a case at seconds, the tolerances are LO's
CAPPED = (("tri100", 1, 1.0, 24), ("tri100", 3, -1.0, 24), ("tri100", 8, 1.0, 24),
          ("odd1037", 1, -1.0, 32), ("odd1037", 3, 1.0, 32), ("odd1037", 5, 1.0, 40), ("odd1037", 8, -1.0, 32),
          ("gapped4000", 3, 1.0, 24), ("gapped4000", 5, -1.0, 24), ("gapped4000", 8, 1.0, 33))
MASKS_STEPS = 400                # the converged run of the masking block (odd1037, tolerances LO)


class Operator:
    """A host CSR matrix as the arrays ``hp.csr_matvec`` takes."""

    def __init__(self, A):
        A = A.tocsr()
        self.n = A.shape[0]
        self.rowptr, self.col, self.val = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64)
        self.A = A

    def wide(self, v):
        """``(H v, |H||v|, L)`` in longdouble."""
        return hp.csr_matvec(self.rowptr, self.col, self.val, v)

    def matvec(self, v):
        return self.A @ v


_operators = {}


def operator(name):
    if name not in _operators:
        _operators[name] = Operator(host_operator(name))
    return _operators[name]


def columns(name, k):
    """``[k, n]`` right-hand sides: seeded normal entries, norms 0.4 .. 3.2 apart by a factor 1.35 from column to column,
    so that no ``beta_0`` is 1 and a neighbour's ``1 / beta`` is off by a third."""
    n = operator(name).n
    B = np.random.default_rng([9, n]).standard_normal((8, n))
    B *= (0.4 * 1.35 ** np.arange(8) / np.linalg.norm(B, axis=1))[:, None]
    return np.ascontiguousarray(B[:k])


def masking_columns():
    """The block of ``test_masking_of_columns_that_stop_at_very_different_steps``: a random column, a sum of 6
    eigenvectors (its Krylov space is exhausted within 7 steps) and a zero column."""
    Hh = host_operator("odd1037")
    lam, Q = np.linalg.eigh(Hh.toarray())
    few = Q[:, [3, 200, 517, 518, 800, 1030]] @ np.array([1.0, -0.5, 0.7, 0.3, -1.2, 0.9])
    return np.array([columns("odd1037", 1)[0], few / np.linalg.norm(few), np.zeros(1037)])


# ---------------------------------------------------------------- reduction trees
def _records_tree(P, K):
    return -(-P * K // 256) + int(math.log2(64 // K)) + 3


def dot_tree(n, cus):
    """``c_dot`` of hipeig_dot (tests/test_gpu_subspace_kernels.py derives it)."""
    G = int(min(max(max(n // 8192, min(n // 1024, 2 * cus)), 1), 2048))
    return 2 * -(-(n // 2) // (256 * G)) + (n & 1) + 9 + -(-G // 256) + 9


def sweep_trees(n, K, variant, cus, rows_per_block=0, row_blocks=0, per_thread=32):
    """``{"vw", "ww", "dot"}``: the depths of the trees behind ``alpha`` (sweep), ``beta`` (KC) and ``beta_0``."""
    if variant == 1:
        G = max(1, min((n + 3) // 4, 8 * cus, 2048))
        vw = -(-n // (4 * G)) + int(math.log2(64 // K)) + 3 + _records_tree(G, K)
    else:
        vw = rows_per_block + _records_tree(min(2 * row_blocks, 2048), K)
    ne = n * (K // 2)
    GE = int(min(max(-(-ne // (256 * per_thread)), 1), 2048))
    ww = -(-ne // (256 * GE)) + int(math.log2(128 // K)) + 3 + _records_tree(GE, K)
    return {"vw": vw, "ww": ww, "dot": dot_tree(n, cus)}


# ---------------------------------------------------------------- a - d
def _ratio(err, bound):
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    if not np.all(np.isfinite(err)):
        return float("inf")
    return float(np.max(err / bound)) if err.size else 0.0


def local_relations(op, b, V, alphas, betas, trees, which="abcd"):
    """Largest error / bound per relation of one column: ``V[m, n]`` are its vectors ``v_0 .. v_{m-1}`` as read,
    ``alphas``, ``betas`` its scalars (at least m and m + 1 of them).  Step i enters relation c when ``v_i`` is there,
    relations b and d when ``v_{i+1}`` is.  Returns ``{"a_beta0", "a_v0", "b", "c", "d"}`` (0.0 where nothing was
    checked)."""
    out = {"a_beta0": 0.0, "a_v0": 0.0, "b": 0.0, "c": 0.0, "d": 0.0}
    m = len(V)
    if m == 0:
        return out
    if "a" in which:
        nb = hp.nrm2(b)
        out["a_beta0"] = _ratio(abs(LD(betas[0]) - nb), 1.01 * (trees["dot"] / 2 + 1) * U * nb)
        ref = np.asarray(b, dtype=LD) / LD(betas[0])
        out["a_v0"] = _ratio(np.abs(V[0].astype(LD) - ref), 2.01 * U * np.abs(ref) + TINY)
    vold = np.zeros(op.n, dtype=LD)
    for i in range(m):
        vi = V[i].astype(LD)
        hv, absax, L = op.wide(V[i])
        bi = LD(betas[i]) if i else LD(0)
        wstar = hv - bi * vold
        avi, avold = np.abs(vi), np.abs(vold)
        if "c" in which:
            ew = U * ((L + 3) * absax + 4 * bi * avold)
            bound = 1.01 * (trees["vw"] * U * np.sum(avi * (np.abs(wstar) + ew)) + np.sum(avi * ew)) + TINY
            out["c"] = max(out["c"], _ratio(abs(LD(alphas[i]) - np.sum(vi * wstar)), bound))
        if i + 1 < m:
            a = LD(alphas[i])
            if "b" in which:
                bound = 1.01 * U * (L + 7) * (absax + bi * avold + abs(a) * avi) + TINY
                out["b"] = max(out["b"], _ratio(np.abs(LD(betas[i + 1]) * V[i + 1].astype(LD) - (wstar - a * vi)), bound))
            if "d" in which:
                out["d"] = max(out["d"], _ratio(abs(hp.nrm2(V[i + 1]) - 1), 1.01 * (trees["ww"] / 2 + 3) * U))
        vold = vi
    return out


# ---------------------------------------------------------------- rotation
def rotation(alphas, betas, zs, sign, dtype=CLD, fault=None):
    """``|tau_k|`` for k = 1 .. m and every shift, ``[m, S]``: the recurrence of ``_scalars_one`` (its expressions in its
    order) on the given scalars in the complex type ``dtype``, no shift ever stopped.  ``fault``: ``"c2"`` leaves ``c2``
    at its start value, ``"tau"`` updates ``tau`` with ``c`` instead of ``-s`` (the CPU test's seeded faults)."""
    real = np.float64 if dtype == np.complex128 else LD
    al, be = np.asarray(alphas, dtype=real), np.asarray(betas, dtype=real)
    z = np.asarray(zs, dtype=complex).astype(dtype)
    S, m = z.size, len(al)
    sg = real(sign)
    c1, s1, c2 = np.ones(S, dtype), np.zeros(S, dtype), np.ones(S, dtype)
    tau = np.full(S, be[0] if len(be) else 0, dtype)
    out = np.zeros((m, S), dtype=real)
    for k in range(m):
        t_up = -sg * be[k] if k else real(0)
        t_d = sg * (z - al[k])
        t_lo = -sg * be[k + 1]
        tmp = c2 * t_up
        dd = -s1 * tmp + c1 * t_d
        nu = np.hypot(np.abs(dd), np.abs(t_lo))
        c, s = dd / nu, (t_lo / nu).astype(dtype)
        tau = (c if fault == "tau" else -s) * tau
        if fault != "c2":
            c2 = c1
        c1, s1 = c, s
        out[k] = np.abs(tau)
    return out


def rotation_check(sc, zs, sign, rtol, atol, delta=DELTA, tau=None):
    """One column's ``estimates`` and ``iterations`` against the ``clongdouble`` recurrence on its own scalars:
    ``(worst estimate error / (delta |tau*|), shifts compared for equality, shifts left out, mismatches)``.  ``tau``: the
    recurrence's result when the caller has it (the CPU test hands in a faulty one's counterpart)."""
    m = len(sc.alphas)
    if m == 0:
        return 0.0, 0, 0, [j for j, it in enumerate(sc.iterations) if it != 0 or sc.estimates[j] != 0.0]
    if tau is None:
        tau = rotation(sc.alphas, sc.betas, zs, sign)
    target = max(atol, rtol * float(sc.betas[0]))
    worst, compared, left, bad = 0.0, 0, 0, []
    for j in range(tau.shape[1]):
        hits = np.nonzero(tau[:, j] <= target)[0]
        stop = int(hits[0]) + 1 if len(hits) else m
        k = int(sc.iterations[j])
        if not 1 <= k <= m:
            bad.append(j)
            continue
        worst = max(worst, float(abs(LD(sc.estimates[j]) - tau[k - 1, j]) / (delta * tau[k - 1, j])))
        if np.any(np.abs(tau[:stop, j] - target) <= 2 * delta * target):
            left += 1
            continue
        compared += 1
        if k != stop:
            bad.append(j)
    return worst, compared, left, bad


def measured_rotation_deviation(cases):
    """Largest relative deviation of the float64 recurrence from the ``clongdouble`` one, in units of u, over
    ``(alphas, betas, zs, sign)`` cases."""
    worst = 0.0
    for al, be, zs, sign in cases:
        if len(al) == 0:
            continue
        ref = rotation(al, be, zs, sign, CLD)
        got = rotation(al, be, zs, sign, np.complex128)
        worst = max(worst, float(np.max(np.abs(got.astype(LD) - ref) / ref)) / U)
    return worst


# ---------------------------------------------------------------- combination
def tables(steps, nc, seed=0):
    """One ``[m_r, nc]`` table per column: seeded normal entries times ``2^e``, e a seeded permutation of an even spread
    over -8 .. 4 across the steps - no term is negligible because of where it stands, the last included."""
    rng = np.random.default_rng([31, seed, nc])
    out = []
    for m in steps:
        e = rng.permutation(np.linspace(-8.0, 4.0, m)) if m else np.zeros(0)
        g = rng.standard_normal((m, nc))
        g[np.abs(g) < 0.1] = 0.5                       # no coefficient small by accident either
        out.append(g * (2.0 ** e)[:, None])
    return out


def combine_check(V, G, q, stream32=0):
    """Largest error / bound of one column's combinations ``q[NC, n]`` against ``hp.combine(V[:m], G)``, ``V`` its fp64
    vectors as read.  ``stream32``: the leading terms that came from an fp32 basis."""
    G = np.asarray(G, dtype=np.float64)
    m = len(G)
    q = np.asarray(q, dtype=np.float64)
    if m == 0:
        return 0.0 if not q.any() else float("inf")
    Y, Yabs = hp.combine(V[:m], G)
    bound = (m + 2) * U * Yabs + TINY
    if stream32:
        bound = bound + U32 * hp.combine(V[:stream32], G[:stream32])[1]
    if not np.all(np.isfinite(q)):
        return float("inf")
    return _ratio(np.abs(q.T.astype(LD) - Y), bound)


def stored_check(V32, V64):
    """Largest ``|v32 - v64| / (2^-24 (1 + 2^-20) |v64|)`` of vectors read from an fp32 basis against the fp64 ones."""
    V64 = np.asarray(V64, dtype=np.float64)
    return _ratio(np.abs(np.asarray(V32, dtype=LD) - V64.astype(LD)), U32 * np.abs(V64).astype(LD) + TINY)


# ---------------------------------------------------------------- the device's vectors
def read_vectors(run, steps=None):
    """The device's ``v_0 .. v_{m_r - 1}`` of every column of a ``LanczosRun``, ``[m_r, n]`` each, read through
    ``combine`` with slices of the identity: 8 vectors per call where every group holds a basis (or a prefix), else 2.
    ``steps[r]`` (default: the steps column r ran) limits ``m_r``.  A column whose table has ended while the others go on
    must read back as zeros; that is asserted here."""
    ran = [len(s.alphas) for s in run.scalars]
    ms = ran if steps is None else [min(int(s), r) for s, r in zip(steps, ran)]
    kept = bool(run._bases) and all(h is not None for h in run._bases)
    nc = 8 if kept else 2
    n = len(run.B[0])
    V = [np.zeros((m, n)) for m in ms]
    for i0 in range(0, max(ms, default=0), nc):
        G = []
        for m in ms:
            g = np.zeros((min(m, i0 + nc), nc))
            for c in range(nc):
                if i0 + c < len(g):
                    g[i0 + c, c] = 1.0
            G.append(g)
        out = run.combine(G)
        for r, m in enumerate(ms):
            parts = [out[r].re, out[r].im] if nc == 2 else out[r]
            for c in range(nc):
                a = parts[c].array
                if i0 + c < m:
                    V[r][i0 + c] = a
                else:
                    assert not a.any(), f"column {r}: slice {i0 + c} past its {m} terms is not zero"
    return V


def twin_column(op, b, zs, sign, maxiter, rtol=LO[0], atol=LO[1]):
    """The host twin's ``(scalars, V[m, n])`` of one column."""
    sc = lf.lanczos_scalars_host(op.matvec, b[None, :], zs, rtol, atol, maxiter, sign)[0]
    m = len(sc.alphas)
    V = lf.lanczos_vectors_host(op.matvec, b, sc.alphas, sc.betas, m) if m else np.zeros((0, op.n))
    return sc, V
