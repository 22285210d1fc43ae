"""The subspace kernels of the inexact-Lanczos loop - hipeig_orthonormalize (sequential MGS and CGS2), hipeig_gram,
hipeig_multi_dot, hipeig_lincomb, hipeig_lincomb_block, hipeig_dot / hipeig_nrm2 - against the same operations in extended
precision (tests/_hiprec.py), at the sizes where each kernel changes path: odd tails, one tile +- 1, the step from 64 to
65 workgroups (two-level record sums), the 2048-workgroup cap, the 16-column chunks and the 256-column cap.

Data: rows with norms spread over 2^-10 .. 2^3 in a seeded random order and seeded normal entries, so that no two columns
or rows are interchangeable and q.q is never 1.

Forward-error bounds, u = 2^-53; starred quantities are the reference's.

Reductions.  Every dot product here is summed by a fixed tree.  An error bound of a sum is (number of additions the most
travelled term goes through) * u * (sum of the magnitudes), so the constant is the depth of the tree:

    e       the per-thread run: a thread of a grid of G workgroups of 256 takes ceil((n // 2) / (256 G)) element pairs,
            two fma terms each, one after the other (and thread 0 the odd tail): e = 2 ceil((n // 2) / (256 G)) + (n & 1)
    6       the 64-lane wave tree
    3       the four waves of a workgroup, added in order
    R(G)    the workgroups' records: <= 64 records of a group in order, min(G, 64) - 1 additions, then the <= 32 group
            records in order, ceil(G / 64) - 1 additions (finish_records; where lanes share a value their partial sums are
            again added in order, never deeper than the plain run)

    c_rec(n, G) = e + 9 + R(G)                  hipeig_multi_dot and the passes of CGS2
    c_dot(n, G) = e + 9 + ceil(G / 256) + 9     hipeig_dot: the last workgroup's 256 threads each add their share of the
                                                partials in order, then the wave tree and the four waves again

G is what grid_records() of blas1.hip takes for n, the device's CU count and the *_PER_THREAD knob (mirrored in
_grid_records below; it only sizes the bound).

    multi_dot   |d_j - d*_j|        <= c_rec u (|Y_j| . |x|)
    dot         |d - d*|            <= c_dot u (|x| . |y|)
    nrm2        |nrm - nrm*|        <= (c_dot / 2 + 1) u nrm*        (square root: half the relative error, one rounding)

Gram.  A workgroup of the MFMA kernel takes T tiles of 128 rows; each of its four waves adds 32 rows per tile into one
accumulator, 8 instructions of 4 terms, in sequence: 32 T terms.  Then the four waves (3) and the records as above, with
G = min(tiles, workgroups the launch allows) and T = ceil(tiles / G); the launch allows at least min(CUs, 512), which is
what the bound assumes (more workgroups only make T smaller):

    c_gram = 32 T + 3 + R(G),       |G_ij - G*_ij| <= c_gram u (|A_i| . |B_j|)

For one tile (n <= 128) that is 35 u, for 65 tiles 99 u: below the 1e-13 (900 u) the older tests allow.  Below 64 rows or 3
columns hipeig_gram runs multi_dot sweeps and c_rec applies.

Linear combinations.  out_i = sum_j c_j V_j[i] is a run of k fma's in order (chunks of 16 accumulate into the output):
k roundings, each relative to the partial sum it produces.  Short runs come close to that worst case - with row norms
spread over 2^13 one term dominates and every rounding is relative to the same large partial sum; a float64 run of k = 4
reaches 2.6 u - so there is no random-walk allowance to take off, and the margin of four over a float64 run that every
bound here is held to makes the constant

    c_lin = 4 (k + 1),              |out_i - out*_i| <= c_lin u (sum_j |c_j| |V_j[i]|)

(lincomb_block: the m inputs take the place of k.)

Sequential MGS (method 0), m columns: c = 64 + 4 m and S = ||x_0|| + sum_j |t1*_j / t2*_j| ||q_j||, the shape and the
constant test_gpu_orthogonalisation.py justifies for the same reduction tree and the same two roundings per element and
column:

    |sqrt(ip) - sqrt(ip*)| <= c u S,   ||x - x*|| <= c u S  (lindep exit, x not normalised),   c u S / sqrt(ip*) (normalised)

CGS2 (method 1).  One pass computes c = Q x and x' = x - sum_j c_j q_j.  Against the exact pass on the same x it errs by
    (m + 4) u (||x|| + sum_j |c_j| ||q_j||)        the m fma's of each element, and
    c_rec u ||x|| sum_j ||q_j||^2                  the coefficients' own errors |dc_j| <= c_rec u ||q_j|| ||x||, each
                                                   carried into x' by q_j - with columns of norm 7 this term is the larger.
Call the sum E(x).  The second pass starts from the first's result, so it also maps the first pass's error through
I - Q^T Q, whose norm is at most 1 + sum_j ||q_j||^2:

    ||x - x*||  <=  E2 = (1 + sum ||q_j||^2) E(x_0) + E(x_1*)
    |sqrt(ip) - sqrt(ip*)|  <=  N = E2 + (c_dot / 2 + 2) u sqrt(ip*)
    normalised:  ||x / sqrt(ip) - x* / sqrt(ip*)||  <=  (E2 + N + 2 u sqrt(ip*)) / sqrt(ip*)

tests/test_hiprec_cpu.py holds every bound to two conditions without a GPU: a float64 emulation of the kernel's algorithm
and tree on these inputs stays under a quarter of it, and each of a list of seeded faults exceeds it.

Every test prints the largest ratio error / bound it saw per group (``-s`` shows it).
"""
import ctypes as C

import numpy as np
import pytest

import _hiprec as hp
from eigensolvers_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MS = [0, 1, 2, 3, 16, 17, 33]
DELTAS = [1.0, 1e-4, 1e-8]
KNOBS = ("HIPEIG_MGS_PER_THREAD", "HIPEIG_MULTIDOT_PER_THREAD", "HIPEIG_DOT_PER_THREAD")
PP = C.POINTER(C.c_void_p)
DP = C.POINTER(C.c_double)


# ---------------------------------------------------------------- grids and constants (see the module docstring)
def _grid_records(n, cus, per_thread=None):
    """grid_records() of blas1.hip: the workgroups of a kernel that ends in a record sum."""
    g = max(n // 8192, min(n // 1024, 2 * cus))
    if per_thread:
        g = n // (256 * per_thread)
    return int(min(max(g, 1), 2048))


def _run(n, G):
    return 2 * -(-(n // 2) // (256 * G)) + (n & 1)


def _records(G):
    return (min(G, 64) - 1) + (-(-G // 64) - 1)


def c_rec(n, G):
    return _run(n, G) + 9 + _records(G)


def c_dot(n, G):
    return _run(n, G) + 9 + -(-G // 256) + 9


def gram_grid(n, cus):
    """(G, T) the Gram bound assumes: workgroups and tiles per workgroup."""
    tiles = -(-n // 128)
    G = min(tiles, cus, 512)
    return G, -(-tiles // G)


def c_gram(n, cus):
    G, T = gram_grid(n, cus)
    return 32 * T + 3 + _records(G)


def c_lin(k):
    return 4 * (k + 1)


def mgs_bounds(m, ip_ref, S):
    """(norm, x un-normalised, x normalised) bounds of the sequential sweep."""
    b = (64 + 4 * m) * U * float(S)
    return b, b, b / float(np.sqrt(ip_ref))


def cgs2_bounds(m, ip_ref, scales, crec, cdot):
    """(norm, x un-normalised, x normalised) bounds of the two classical passes; scales as hp.orthonormalize_cgs2 returns."""
    (x0, cq0, q2), (x1, cq1, _) = [tuple(float(v) for v in s) for s in scales]

    def E(xn, cq):
        return U * ((m + 4) * (xn + cq) + crec * xn * q2)

    E2 = (1.0 + q2) * E(x0, cq0) + E(x1, cq1)
    s = float(np.sqrt(ip_ref))
    N = E2 + (cdot / 2 + 2) * U * s
    return N, E2, (E2 + N + 2 * U * s) / s


# ---------------------------------------------------------------- data
def _norms(rng, m):
    return 2.0 ** rng.permutation(np.linspace(-10.0, 3.0, m)) if m else np.zeros(0)


def rows(rng, m, n):
    """m rows of length n: normal entries, row norms ~ sqrt(n) 2^-10 .. sqrt(n) 2^3 in a random order."""
    return np.ascontiguousarray(rng.standard_normal((m, n)) * _norms(rng, m)[:, None])


def _orthonormal(rng, n, m):
    Q = rng.standard_normal((m, n))
    for _ in range(2):
        if m:
            Q = np.linalg.solve(np.linalg.cholesky(Q @ Q.T), Q)
    return np.ascontiguousarray(Q)


def column_sets(n, mmax, seed=0):
    """{"scaled": orthogonal rows of norms 2^-10 .. 2^3 (q.q != 1), "skewed": the same with V[1] += 0.3 V[0] and
    V[2] *= 1e-3 (sequential != classical)}, each of shape (mmax, n); the sets of fewer columns are their prefixes."""
    rng = np.random.default_rng([n, mmax, seed])
    scaled = _orthonormal(rng, n, mmax) * _norms(rng, mmax)[:, None]
    skewed = scaled.copy()
    if mmax > 1:
        skewed[1] += 0.3 * skewed[0]
    if mmax > 2:
        skewed[2] *= 1e-3
    return {"scaled": np.ascontiguousarray(scaled), "skewed": skewed}


def operand(V, m, delta, idx):
    """x = a^T V[:m] + delta r."""
    n = V.shape[1]
    rng = np.random.default_rng([n, m, idx])
    a, r = rng.standard_normal(m), rng.standard_normal(n)
    return (V[:m].T @ a if m else np.zeros(n)) + delta * r


def ortho_cases(n, ms):
    """(set name, delta, m, index) of the orthonormalize cases at length n: the scaled set with every delta (there the
    sequential projection really cancels), the skewed set with delta = 1 where it differs from the scaled one."""
    out = []
    for m in ms:
        if m >= n:
            continue
        out += [("scaled", d, m, i) for i, d in enumerate(DELTAS)]
        if m >= 2:
            out.append(("skewed", 1.0, m, 3))
    return out


def mixed_alias_cases():
    """The Gram calls whose tables coincide in part (rows of A, rows of B): a 32 x 32 block with equal tables in a call
    that is not symmetric, with and without a second block row, and equal tables but for one pointer."""
    return {"40x40 first 32 shared": (list(range(40)), [("A", j) for j in range(32)] + [("B", j) for j in range(32, 40)]),
            "32x40 first 32 shared": (list(range(32)), [("A", j) for j in range(32)] + [("B", j) for j in range(32, 40)]),
            "33x33 all but B[5]": (list(range(33)), [("B", 5) if j == 5 else ("A", j) for j in range(33)])}


# ---------------------------------------------------------------- device helpers
def _up(ctx, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    buf = ctx.alloc(a.size)
    _lib.call("hipeig_vec_upload", ctx.handle, buf.ptr, a.ctypes.data_as(C.c_void_p), a.size)
    return buf


def _down(ctx, buf):
    out = np.empty(buf.n)
    _lib.call("hipeig_vec_download", ctx.handle, out.ctypes.data_as(C.c_void_p), buf.ptr, buf.n)
    return out


def _table(bufs):
    arr = (C.c_void_p * max(len(bufs), 1))(*[b.ptr for b in bufs])
    return C.cast(arr, PP), arr


def _cus(ctx):
    return int(ctx.device_info()["cus"])


class _Worst:
    """Largest ratio error / bound per group; asserts every ratio <= 1 (a zero bound asks for a zero error)."""

    def __init__(self, name):
        self.name, self.ratio = name, {}

    def check(self, group, err, bound, what):
        err = np.asarray(err, dtype=np.float64)
        bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        r = float(np.max(ratio)) if err.size else 0.0
        assert np.all(err <= bound), f"{self.name} {what}: error / bound = {r:.3g} (max error {float(np.max(err)):.3e})"
        self.ratio[group] = max(self.ratio.get(group, 0.0), r)

    def report(self):
        print(f"\n[{self.name}] largest error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.ratio.items())))


def _err(got, ref):
    """|got - ref| element-wise, the difference taken in extended precision."""
    return np.abs(np.asarray(got, dtype=np.float64).astype(hp.LD) - ref).astype(np.float64)


def _norm_err(got, ref):
    return float(hp.nrm2(np.asarray(got, dtype=np.float64).astype(hp.LD) - ref))


# ---------------------------------------------------------------- a. hipeig_orthonormalize
def _orthonormalize(ctx, n, Vd, m, x, lindep, method):
    xd = _up(ctx, x)
    tab, keep = _table(Vd[:m])
    ip, dep = C.c_double(np.nan), C.c_int(-1)
    _lib.call("hipeig_orthonormalize", ctx.handle, n, m, tab, xd.ptr, float(lindep), method, C.byref(ip), C.byref(dep))
    return float(ip.value), int(dep.value), _down(ctx, xd)


def _check_orthonormalize(ctx, worst, n, ms, per_thread=None):
    cus = _cus(ctx)
    G = _grid_records(n, cus, per_thread)
    crec, cdot = c_rec(n, G), c_dot(n, G)
    cases = ortho_cases(n, ms)
    mmax = max([c[2] for c in cases])
    sets = column_sets(n, mmax)
    dev = {name: [_up(ctx, v) for v in V] for name, V in sets.items()}
    for name, delta, m, idx in cases:
        V = sets[name]
        x = operand(V, m, delta, idx)
        refs = {0: hp.orthonormalize_mgs(V[:m], x), 1: hp.orthonormalize_cgs2(V[:m], x)}
        for method, tag in ((0, "mgs"), (1, "cgs2")):
            ip_r, x_r, scale = refs[method]
            nb, xb, xnb = mgs_bounds(m, ip_r, scale) if method == 0 else cgs2_bounds(m, ip_r, scale, crec, cdot)
            s_r = np.sqrt(ip_r)
            what = f"{tag} {name} delta={delta} m={m}"
            ip, dep, xo = _orthonormalize(ctx, n, dev[name], m, x, float(ip_r) / 4, method)
            assert dep == 0, f"{what}: reported linearly dependent at lindep = ip* / 4 (innerprod {ip}, ip* {float(ip_r)})"
            worst.check(f"{tag} norm", abs(hp.LD(np.sqrt(ip)) - s_r), nb, what + " norm")
            worst.check(f"{tag} x normalised", _norm_err(xo, x_r / s_r), xnb, what + " x normalised")
            ip2, dep, xo = _orthonormalize(ctx, n, dev[name], m, x, 4 * float(ip_r), method)
            assert dep == 1, f"{what}: not reported linearly dependent at lindep = 4 ip* (innerprod {ip2})"
            assert ip2 == ip, f"{what}: innerprod depends on lindep"
            worst.check(f"{tag} x at the lindep exit", _norm_err(xo, x_r), xb, what + " x at the lindep exit")
    for name, V in sets.items():
        for j, buf in enumerate(dev[name]):
            np.testing.assert_array_equal(_down(ctx, buf), V[j], err_msg=f"{name} column {j} was written to")


@pytest.mark.parametrize("n", [1, 2, 3, 255, 513, 2047, 2049, 66559, 66561, 100003])
def test_orthonormalize_against_the_high_precision_reference(hip, n):
    """hipeig_orthonormalize, both methods, m = 0 .. 33 < n: the returned inner product, the normalised x, the x the lindep
    exit leaves behind, and the columns untouched.  Odd n: the tails of mgs_sweep_kernel, multi_dot_kernel, lincomb_kernel
    and dot_kernel; 66559 / 66561: 64 and 65 workgroups, one- and two-level record sums; m = 17, 33: CGS2's 16-column
    chunks with their coefficient offsets."""
    ctx = hip.HipContext.default()
    worst = _Worst(f"orthonormalize n={n}")
    _check_orthonormalize(ctx, worst, n, MS)
    worst.report()


def test_cgs2_beyond_the_256_column_cap(hip):
    """CGS2 with m = 257 at n = 2049: a second multi_dot / lincomb round for column 256 within each pass.  That round takes
    its coefficient from the x the first 256 columns have already been removed from; the columns here are orthogonal, so
    it is the coefficient of the classical pass up to the columns' own orthogonality (~u ||q_i|| ||q_j||, inside the
    bound's first term)."""
    ctx = hip.HipContext.default()
    n, m = 2049, 257
    G = _grid_records(n, _cus(ctx))
    V = column_sets(n, m)["scaled"]
    Vd = [_up(ctx, v) for v in V]
    x = operand(V, m, 1.0, 0)
    ip_r, x_r, scales = hp.orthonormalize_cgs2(V, x)
    nb, xb, xnb = cgs2_bounds(m, ip_r, scales, c_rec(n, G), c_dot(n, G))
    worst = _Worst("cgs2 m=257")
    ip, dep, xo = _orthonormalize(ctx, n, Vd, m, x, float(ip_r) / 4, 1)
    assert dep == 0
    worst.check("norm", abs(hp.LD(np.sqrt(ip)) - np.sqrt(ip_r)), nb, "norm")
    worst.check("x normalised", _norm_err(xo, x_r / np.sqrt(ip_r)), xnb, "x normalised")
    ip, dep, xo = _orthonormalize(ctx, n, Vd, m, x, 4 * float(ip_r), 1)
    assert dep == 1
    worst.check("x at the lindep exit", _norm_err(xo, x_r), xb, "x at the lindep exit")
    worst.report()


@pytest.mark.parametrize("n", [16640, 32769, 600001])
def test_orthonormalize_on_forced_record_grids(hip, monkeypatch, n):
    """One element pair per thread (the *_PER_THREAD knobs, read per call): 16640 -> 65 workgroups, two groups, the last of
    one record; 32769 -> 128 workgroups and an odd tail; 600001 -> the 2048-workgroup cap, 32 groups."""
    for k in KNOBS:
        monkeypatch.setenv(k, "1")
    ctx = hip.HipContext.default()
    assert _grid_records(n, _cus(ctx), 1) == {16640: 65, 32769: 128, 600001: 2048}[n]
    worst = _Worst(f"orthonormalize, forced grid, n={n}")
    _check_orthonormalize(ctx, worst, n, [1, 3, 17], per_thread=1)
    worst.report()


@pytest.mark.parametrize("method", ["mgs", "cgs2"])
def test_orthogonalize_against_set_through_hipvector(hip, method):
    """HipVector.orthogonalize_against_set: a normalised vector within the bound, None at the lindep exit, x untouched."""
    ctx = hip.HipContext.default()
    n, m = 2049, 17
    G = _grid_records(n, _cus(ctx))
    V = column_sets(n, m)["skewed"]
    x = operand(V, m, 1.0, 3)
    opts = {"orthogonalization": method}
    qs = [hip.HipVector(v.copy(), opts) for v in V]
    X = hip.HipVector(x.copy(), opts)
    if method == "mgs":
        ip_r, x_r, S = hp.orthonormalize_mgs(V, x)
        xnb = mgs_bounds(m, ip_r, S)[2]
    else:
        ip_r, x_r, scales = hp.orthonormalize_cgs2(V, x)
        xnb = cgs2_bounds(m, ip_r, scales, c_rec(n, G), c_dot(n, G))[2]
    worst = _Worst(f"orthogonalize_against_set {method}")
    out = hip.HipVector.orthogonalize_against_set(X, qs, lindep=float(ip_r) / 4)
    worst.check("x normalised", _norm_err(out.array, x_r / np.sqrt(ip_r)), xnb, "x normalised")
    assert hip.HipVector.orthogonalize_against_set(X, qs, lindep=4 * float(ip_r)) is None
    np.testing.assert_array_equal(X.array, x)
    worst.report()


# ---------------------------------------------------------------- b. hipeig_gram
def _gram(ctx, n, Ad, Bd):
    ta, ka = _table(Ad)
    tb, kb = _table(Bd)
    out = np.full((len(Ad), len(Bd)), np.nan)
    _lib.call("hipeig_gram", ctx.handle, n, len(Ad), ta, len(Bd), tb, out.ctypes.data_as(DP))
    return out


def _gram_const(n, ma, mb, cus):
    if ma < 3 or mb < 3 or n < 64:
        return c_rec(n, _grid_records(n, cus))
    return c_gram(n, cus)


GRAM_SHAPES = [(3, 3), (3, 17), (16, 17), (17, 3), (32, 33), (33, 32)]


@pytest.mark.parametrize("n", [64, 65, 127, 128, 129, 8192, 8193, 30011])
def test_gram_blocks_element_by_element(hip, n):
    """hipeig_gram with distinct tables, every accumulator shape (1x1, 1x2, 2x1, 2x2, a second 32-column pass either way)
    at the first MFMA size, one tile +- 1 (the r + 1 < n / r < n tail of the fetch) and 64 / 65 workgroups."""
    ctx = hip.HipContext.default()
    rng = np.random.default_rng([n, 1])
    A, B = rows(rng, 33, n), rows(rng, 33, n)
    Ad, Bd = [_up(ctx, v) for v in A], [_up(ctx, v) for v in B]
    G_r, Gabs = hp.gram(A, B)
    worst = _Worst(f"gram n={n}")
    for ma, mb in GRAM_SHAPES:
        got = _gram(ctx, n, Ad[:ma], Bd[:mb])
        worst.check(f"{ma}x{mb}", _err(got, G_r[:ma, :mb]), _gram_const(n, ma, mb, _cus(ctx)) * U * Gabs[:ma, :mb].astype(float),
                    f"{ma}x{mb}")
    worst.report()


@pytest.mark.parametrize("n", [129, 8193])
def test_symmetric_gram(hip, n):
    """The same table twice, up to 100 columns: the SAME kernels, the skipped lower blocks mirrored inside a pass and the
    skipped lower passes mirrored between passes.  Exactly symmetric."""
    ctx = hip.HipContext.default()
    rng = np.random.default_rng([n, 2])
    A = rows(rng, 100, n)
    Ad = [_up(ctx, v) for v in A]
    G_r, Gabs = hp.gram(A, A)
    worst = _Worst(f"symmetric gram n={n}")
    for m in (3, 16, 17, 32, 33, 65, 100):
        S = _gram(ctx, n, Ad[:m], Ad[:m])
        np.testing.assert_array_equal(S, S.T, err_msg=f"m={m}: not symmetric bit for bit")
        worst.check(f"m={m}", _err(S, G_r[:m, :m]), c_gram(n, _cus(ctx)) * U * Gabs[:m, :m].astype(float), f"m={m}")
    worst.report()


def test_gram_with_partly_shared_tables(hip):
    """32 x 32 blocks whose tables coincide inside calls that are not symmetric: the SAME<2,2> kernel, its lower 16 x 16
    block taken from the transposed upper one on the host, next to blocks that are computed in full."""
    ctx = hip.HipContext.default()
    n = 8193
    rng = np.random.default_rng([n, 3])
    A, Bx = rows(rng, 40, n), rows(rng, 40, n)
    dev = {"A": [_up(ctx, v) for v in A], "B": [_up(ctx, v) for v in Bx]}
    both = np.concatenate([A, Bx])
    G_r, Gabs = hp.gram(A, both)
    worst = _Worst("gram, partly shared tables")
    for name, (ia, jb) in mixed_alias_cases().items():
        cols = [j if s == "A" else 40 + j for s, j in jb]
        got = _gram(ctx, n, [dev["A"][i] for i in ia], [dev[s][j] for s, j in jb])
        ref, mag = G_r[np.ix_(ia, cols)], Gabs[np.ix_(ia, cols)].astype(float)
        worst.check(name, _err(got, ref), c_gram(n, _cus(ctx)) * U * mag, name)
    worst.report()


def test_gram_with_several_tiles_per_workgroup_and_below_the_mfma_size(hip):
    """n = 2^18 + 129: 2050 tiles, more than any launch has workgroups, a last tile of one row.  n = 63: the multi_dot
    fallback fills the same out[i * mb + j] layout."""
    ctx = hip.HipContext.default()
    worst = _Worst("gram, long and short")
    for n, ma, mb in (((1 << 18) + 129, 3, 17), (63, 5, 5)):
        rng = np.random.default_rng([n, 4])
        A, B = rows(rng, ma, n), rows(rng, mb, n)
        got = _gram(ctx, n, [_up(ctx, v) for v in A], [_up(ctx, v) for v in B])
        G_r, Gabs = hp.gram(A, B)
        worst.check(f"n={n}", _err(got, G_r), _gram_const(n, ma, mb, _cus(ctx)) * U * Gabs.astype(float), f"n={n}")
    worst.report()


@pytest.mark.parametrize("m", [2, 3, 65])
def test_overlap_matrices_through_hipvector(hip, m):
    """overlapMatrix, extendOverlapMatrix and _multi_dot: the bounds of the kernels they call."""
    ctx = hip.HipContext.default()
    n = 8193
    cus = _cus(ctx)
    rng = np.random.default_rng([n, m, 5])
    A = rows(rng, m, n)
    V = [hip.HipVector(v.copy()) for v in A]
    G_r, Gabs = hp.gram(A, A)
    Gabs = Gabs.astype(float)
    crec = c_rec(n, _grid_records(n, cus))
    worst = _Worst(f"overlap m={m}")
    S = hip.HipVector.overlapMatrix(V)
    np.testing.assert_array_equal(S, S.T)
    worst.check("overlapMatrix", _err(S, G_r), _gram_const(n, m, m, cus) * U * Gabs, "overlapMatrix")
    d = hip.HipVector._multi_dot(V, V[-1])
    worst.check("_multi_dot", _err(d, G_r[:, -1]), crec * U * Gabs[:, -1], "_multi_dot")
    Sx = hip.HipVector.extendOverlapMatrix(V, S[:m - 1, :m - 1])
    np.testing.assert_array_equal(Sx[:m - 1, :m - 1], S[:m - 1, :m - 1])
    np.testing.assert_array_equal(Sx, Sx.T)
    worst.check("extendOverlapMatrix", _err(Sx[:, -1], G_r[:, -1]), crec * U * Gabs[:, -1], "extendOverlapMatrix")
    worst.report()


# ---------------------------------------------------------------- c. multi_dot, lincomb, lincomb_block, dot
@pytest.mark.parametrize("n,per_thread", [(1, None), (3, None), (2049, None), (16640, 1)])
def test_multi_dot_against_the_high_precision_reference(hip, monkeypatch, n, per_thread):
    """hipeig_multi_dot for m = 1 .. 257: 16-column launches, the second call past 256 columns (out + done)."""
    if per_thread:
        monkeypatch.setenv("HIPEIG_MULTIDOT_PER_THREAD", str(per_thread))
    ctx = hip.HipContext.default()
    rng = np.random.default_rng([n, 6])
    Y, x = rows(rng, 257, n), rng.standard_normal(n)
    Yd, xd = [_up(ctx, v) for v in Y], _up(ctx, x)
    G_r, Gabs = hp.gram(Y, x[None, :])
    c = c_rec(n, _grid_records(n, _cus(ctx), per_thread))
    worst = _Worst(f"multi_dot n={n}")
    for m in (1, 16, 17, 256, 257):
        tab, keep = _table(Yd[:m])
        out = np.full(m + 1, np.nan)
        _lib.call("hipeig_multi_dot", ctx.handle, n, m, tab, xd.ptr, out.ctypes.data_as(DP))
        assert np.isnan(out[m]), "wrote past the m results"
        worst.check(f"m={m}", _err(out[:m], G_r[:m, 0]), c * U * Gabs[:m, 0].astype(float), f"m={m}")
    worst.report()


@pytest.mark.parametrize("n", [1, 3, 1025])
def test_lincomb_against_the_high_precision_reference(hip, n):
    """hipeig_lincomb for k = 1 .. 33: the 4-, 8- and 16-wide kernels, and chunks past 16 that accumulate into the output
    (stale contents of the output must not show: it is filled with a large value first)."""
    ctx = hip.HipContext.default()
    rng = np.random.default_rng([n, 7])
    V, coef = rows(rng, 33, n), rng.standard_normal(33) * 2.0 ** rng.integers(-3, 4, 33)
    Vd = [_up(ctx, v) for v in V]
    worst = _Worst(f"lincomb n={n}")
    for k in (1, 4, 5, 8, 9, 16, 17, 33):
        out = _up(ctx, np.full(n, 1e30))
        tab, keep = _table(Vd[:k])
        cf = np.ascontiguousarray(coef[:k])
        _lib.call("hipeig_lincomb", ctx.handle, n, k, cf.ctypes.data_as(DP), tab, out.ptr)
        Y_r, Yabs = hp.combine(V[:k], coef[:k, None])
        worst.check(f"k={k}", _err(_down(ctx, out), Y_r[:, 0]), c_lin(k) * U * Yabs[:, 0].astype(float), f"k={k}")
    for j, buf in enumerate(Vd):
        np.testing.assert_array_equal(_down(ctx, buf), V[j], err_msg=f"input {j} was written to")
    worst.report()


@pytest.mark.parametrize("n", [1, 3, 1025])
def test_lincomb_block_against_the_high_precision_reference(hip, n):
    """hipeig_lincomb_block for k = 1 .. 33 outputs of m = 1 .. 40 inputs (the 4-, 8- and 16-wide kernels, several output
    passes, the odd tail written by thread c < k of each pass), also with the coefficients a column slice of a wider
    matrix (ldc > k)."""
    ctx = hip.HipContext.default()
    rng = np.random.default_rng([n, 8])
    V = rows(rng, 40, n)
    Cw = rng.standard_normal((40, 36)) * 2.0 ** rng.integers(-3, 4, (40, 36))
    Vd = [_up(ctx, v) for v in V]
    worst = _Worst(f"lincomb_block n={n}")
    for m, k in ((1, 1), (5, 4), (5, 5), (9, 8), (9, 9), (17, 16), (17, 17), (40, 33)):
        tab, keep = _table(Vd[:m])
        for c0, tag in ((0, "ldc=k"), (2, "ldc>k")):
            Cm = np.ascontiguousarray(Cw[:m, :k]) if c0 == 0 else Cw          # the slice Cw[:m, c0:c0 + k] of the wide matrix
            ldc = Cm.shape[1]
            ptr = C.cast(C.c_void_p(Cm.ctypes.data + 8 * c0), DP)
            outs = [_up(ctx, np.full(n, 1e30)) for _ in range(k)]
            otab, okeep = _table(outs)
            _lib.call("hipeig_lincomb_block", ctx.handle, n, m, k, ptr, ldc, tab, otab)
            Y_r, Yabs = hp.combine(V[:m], Cw[:m, c0:c0 + k])
            got = np.stack([_down(ctx, o) for o in outs], axis=1)
            worst.check(f"{m}x{k} {tag}", _err(got, Y_r), c_lin(m) * U * Yabs.astype(float), f"m={m} k={k} {tag}")
    for j, buf in enumerate(Vd):
        np.testing.assert_array_equal(_down(ctx, buf), V[j], err_msg=f"input {j} was written to")
    worst.report()


@pytest.mark.parametrize("n,per_thread", [(0, None), (1, None), (2, None), (3, None), (511, None), (513, None),
                                          (16641, 1), (600001, 1)])
def test_dot_and_nrm2_against_the_high_precision_reference(hip, monkeypatch, n, per_thread):
    """hipeig_dot / hipeig_nrm2 from the empty vector up, and on forced grids of 65 and 2048 workgroups with an odd tail."""
    if per_thread:
        monkeypatch.setenv("HIPEIG_DOT_PER_THREAD", str(per_thread))
    ctx = hip.HipContext.default()
    G = _grid_records(n, _cus(ctx), per_thread)
    if per_thread:
        assert G == {16641: 65, 600001: 2048}[n]
    rng = np.random.default_rng([n, 9])
    x = rng.standard_normal(n) * 2.0 ** rng.integers(-10, 4, n)
    y = rng.standard_normal(n)
    xd, yd = _up(ctx, x), _up(ctx, y)
    d, nr = C.c_double(np.nan), C.c_double(np.nan)
    _lib.call("hipeig_dot", ctx.handle, n, xd.ptr, yd.ptr, C.byref(d))
    _lib.call("hipeig_nrm2", ctx.handle, n, xd.ptr, C.byref(nr))
    worst = _Worst(f"dot n={n}")
    c = c_dot(n, G)
    worst.check("dot", abs(hp.LD(d.value) - hp.dot(x, y)), c * U * float(hp.dot(np.abs(x), np.abs(y))), "dot")
    worst.check("nrm2", abs(hp.LD(nr.value) - hp.nrm2(x)), (c / 2 + 1) * U * float(hp.nrm2(x)), "nrm2")
    worst.report()
