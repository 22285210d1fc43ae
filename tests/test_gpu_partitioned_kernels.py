"""The row-partitioned Arnoldi step, the projection and the sums of blas1.hip on loopback ranks of one GPU, against the
same operations in extended precision (``_hiprec.py``), with the bounds of the single-GPU tests
(``test_gpu_orthogonalisation.py``, ``test_gpu_subspace_kernels.py``) evaluated for this path.

Arnoldi step and projection (arnoldi.hip, ``ArnPlan::PARTITIONED``).  Per column a rank runs ``mgsp_dot_kernel`` on
``grid_for(n_r, 4)`` - g = ceil(n_r / 1024) workgroups of 256 threads, a thread takes at most ceil(n_r / (256 g)) <= 4
elements in order, one fma each (a pair: two, so <= 8 terms), then the 64-lane wave tree (6) and the four waves in order
(3) - then the one-workgroup ``mgsp_reduce_kernel``: every thread adds its ceil(g / 256) partials in order (1 here, 8 at
the cap of 2048 workgroups), the wave tree and the four waves again (9); the all-reduce adds the P ranks' sums in rank
order (P - 1).  The most travelled term goes through

    8 + 9 + ceil(g / 256) + 9 + (P - 1)  =  28 .. 36 additions  (P <= 3),

under the 64 the constant ``c = 64 + 4 m`` of ``_check_step`` allows for the reduction, so that constant stands;
``arnoldi_sumsq`` (the norms) has the same tree with two terms per element of a pair.  ``_depth`` evaluates the count for
the shapes run and the test asserts it.

Sums (``hipeig_dot``, ``hipeig_nrm2``, ``hipeig_multi_dot``, ``hipeig_gram``, ``hipeig_orthonormalize``).  A rank runs the
single-GPU kernel on its slab of n_r rows and the records are all-reduced, so the constant of a sum is that of
``test_gpu_subspace_kernels.py`` for the slab length, the largest over the ranks, plus the P - 1 additions of the rank
sum; it multiplies u times the sum of the magnitudes over the whole vector.  The sequential sweep of
``hipeig_orthonormalize`` keeps ``c = 64 + 4 m``: its reduction is ``c_rec(n_r, G) + P - 1`` deep, 63 at the most here
(asserted).

Coefficients, norms and sums must be the same bits on every rank.  A rank's body makes library calls and returns their
results; every check comes after all ranks have returned and the group is closed."""
import ctypes as C

import numpy as np
import pytest

import _hiprec as hp
import test_gpu_subspace_kernels as sk
from eigensolvers_amd import _lib
from eigensolvers_amd.distributed import LoopbackGroup, row_range
from eigensolvers_amd.gcrotmk import _Ops, _mgs_project, _name, _parts, _scalars, _tables, _unpack
from test_gpu_orthogonalisation import _Worst, _check_step, _down_w, _orthonormal, _skewed, _up_cols, _up_w

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MS = (0, 1, 4, 9, 28)
DELTAS = (1.0, 1e-8)
SHAPES = [(1037, 2), (1037, 3), (100_003, 2), (100_003, 3)]


def on_ranks(P, body):
    grp = LoopbackGroup(P)
    try:
        return grp.run(body)
    finally:
        grp.close()


def _slabs(n, P):
    return [row_range(n, P, r) for r in range(P)]


def _same_bits(values, what):
    first = np.asarray(values[0])
    for r, v in enumerate(values[1:], start=1):
        assert np.asarray(v).tobytes() == first.tobytes(), f"{what}: rank {r} differs from rank 0 ({v} vs {values[0]})"


# ---------------------------------------------------------------- Arnoldi step and projection
def _depth(n_r, P, pair):
    """Additions the most travelled term of a partitioned dot goes through (module docstring)."""
    g = min(max(-(-n_r // 1024), 1), 2048)
    e = -(-n_r // (256 * g))
    return (2 if pair else 1) * e + 9 + -(-g // 256) + 9 + (P - 1)


def _step(ctx, n_r, Vd, wd, pair):
    """``hipeig_arnoldi_step`` / ``hipeig_pair_arnoldi_step``: the raw record [nb^2, h .., na^2]."""
    out, ptr = _scalars(len(Vd), pair, 2)
    _lib.call(_name("arnoldi_step", pair), ctx.handle, n_r, len(Vd), *_tables(Vd, pair), *_parts(wd, pair), ptr)
    return out


@pytest.mark.parametrize("n,P", SHAPES)
@pytest.mark.parametrize("pair", [False, True], ids=["real", "pair"])
def test_partitioned_arnoldi_step_and_projection(hip, pair, n, P):
    """m over 0 .. 28 columns, w = V a + delta r with delta 1 and 1e-8 (almost all of w cancels) on orthonormal columns,
    then skewed columns; slabs of 345 .. 50002 rows, ragged, one workgroup and 49 per dot."""
    rng = np.random.default_rng([n, P, int(pair)])
    mmax = max(MS)
    Q = _orthonormal(rng, n, mmax, pair)
    V = _skewed(Q, pair)

    def rnd(size):
        return rng.standard_normal(size) + (1j * rng.standard_normal(size) if pair else 0.0)

    cases = [("orth", Q, m, (Q[:m].T @ rnd(m) if m else np.zeros(n, dtype=Q.dtype)) + delta * rnd(n), f"delta={delta} m={m}")
             for delta in DELTAS for m in MS]
    wsk = V.T @ rnd(mmax) + rnd(n)
    cases += [("skew", V, m, wsk, f"skewed m={m}") for m in MS]
    for lo, hi in _slabs(n, P):
        assert hi > lo and _depth(hi - lo, P, pair) <= 64, (lo, hi, _depth(hi - lo, P, pair))

    def body(rank, ctx):
        lo, hi = row_range(n, P, rank)
        dev = {"orth": _up_cols(ctx, Q[:, lo:hi], pair), "skew": _up_cols(ctx, V[:, lo:hi], pair)}
        ops = _Ops(ctx, hi - lo)
        out = []
        for kind, _, m, w, _ in cases:
            wd = _up_w(ctx, w[lo:hi], pair)
            rec = _step(ctx, hi - lo, dev[kind][:m], wd, pair)
            ws = _down_w(ctx, wd, pair)
            wd = _up_w(ctx, w[lo:hi], pair)
            coef = np.array(_mgs_project(ops, pair, dev[kind][:m], wd))
            out.append((rec, ws, coef, _down_w(ctx, wd, pair)))
        return out

    res = on_ranks(P, body)
    worst = _Worst(f"partitioned arnoldi {'pair' if pair else 'real'} n={n} P={P}")
    vnorms = {"orth": np.linalg.norm(Q, axis=1), "skew": np.array([float(hp.nrm2(v)) for v in V])}
    skew_step = hp.mgs(V, wsk, checkpoints=set(MS))
    skew_proj = hp.mgs(V, wsk, normalise=False, checkpoints=set(MS))
    for i, (kind, cols, m, w, what) in enumerate(cases):
        _same_bits([o[i][0] for o in res], f"{what}: step scalars")
        _same_bits([o[i][2] for o in res], f"{what}: projection coefficients")
        nb, h, na = _unpack(res[0][i][0], m, pair)
        ref = skew_step[m] if kind == "skew" else hp.mgs(cols[:m], w)
        _check_step(worst, f"step {kind}", f"step {what}", (nb, h, na, np.concatenate([o[i][1] for o in res])), ref, vnorms[kind])
        wv = np.concatenate([o[i][3] for o in res])
        if m == 0:
            np.testing.assert_array_equal(wv, w)                      # nothing to project against: w untouched
            continue
        nb_r, h_r, na_r, w_r = skew_proj[m] if kind == "skew" else hp.mgs(cols[:m], w, normalise=False)
        _check_step(worst, f"project {kind}", f"project {what}", (float(nb_r), res[0][i][2], float(na_r), wv),
                    (nb_r, h_r, na_r, w_r), vnorms[kind], normalised=False)
    worst.report()


# ---------------------------------------------------------------- sums
def _const(fn, n, P, *args):
    """A single-GPU constant evaluated for every slab, the largest, plus the P - 1 additions of the rank sum."""
    return max(fn(hi - lo, *args) for lo, hi in _slabs(n, P)) + (P - 1)


def _c_rec(n_r, cus):
    return sk.c_rec(n_r, sk._grid_records(n_r, cus))


def _c_dot(n_r, cus):
    return sk.c_dot(n_r, sk._grid_records(n_r, cus))


@pytest.mark.parametrize("n,P", SHAPES)
def test_partitioned_dot_nrm2_multi_dot_and_gram(hip, n, P):
    """Rows with norms spread over 2^-10 .. 2^3 (the recipe of the single-GPU test); multi_dot of 1, 5 and 17 columns (a
    second 16-column launch), Gram blocks of 5 x 9 and 16 x 16."""
    cus = sk._cus(hip.HipContext.default())
    rng = np.random.default_rng([n, P, 2])
    x = rng.standard_normal(n) * 2.0 ** rng.integers(-10, 4, n)
    y = rng.standard_normal(n)
    Y = sk.rows(rng, 17, n)
    A, B = sk.rows(rng, 16, n), sk.rows(rng, 16, n)

    def body(rank, ctx):
        lo, hi = row_range(n, P, rank)
        nr = hi - lo
        xd, yd = sk._up(ctx, x[lo:hi]), sk._up(ctx, y[lo:hi])
        d, nrm = C.c_double(np.nan), C.c_double(np.nan)
        _lib.call("hipeig_dot", ctx.handle, nr, xd.ptr, yd.ptr, C.byref(d))
        _lib.call("hipeig_nrm2", ctx.handle, nr, xd.ptr, C.byref(nrm))
        out = {"dot": d.value, "nrm2": nrm.value}
        Yd = [sk._up(ctx, v[lo:hi]) for v in Y]
        for m in (1, 5, 17):
            tab, keep = sk._table(Yd[:m])
            md = np.full(m + 1, np.nan)
            _lib.call("hipeig_multi_dot", ctx.handle, nr, m, tab, yd.ptr, md.ctypes.data_as(sk.DP))
            out[f"multi_dot {m}"] = md
        Ad, Bd = [sk._up(ctx, v[lo:hi]) for v in A], [sk._up(ctx, v[lo:hi]) for v in B]
        for ma, mb in ((5, 9), (16, 16)):
            out[f"gram {ma}x{mb}"] = sk._gram(ctx, nr, Ad[:ma], Bd[:mb])
        return out

    res = on_ranks(P, body)
    for key in res[0]:
        _same_bits([o[key] for o in res], key)
    got = res[0]
    worst = _Worst(f"partitioned sums n={n} P={P}")
    cdot = _const(_c_dot, n, P, cus)
    worst.check("dot", abs(hp.LD(got["dot"]) - hp.dot(x, y)), cdot * U * float(hp.dot(np.abs(x), np.abs(y))), "dot")
    worst.check("nrm2", abs(hp.LD(got["nrm2"]) - hp.nrm2(x)), (cdot / 2 + 1) * U * float(hp.nrm2(x)), "nrm2")
    G_r, Gabs = hp.gram(Y, y[None, :])
    crec = _const(_c_rec, n, P, cus)
    for m in (1, 5, 17):
        md = got[f"multi_dot {m}"]
        assert np.isnan(md[m]), "wrote past the m results"
        worst.check(f"multi_dot m={m}", sk._err(md[:m], G_r[:m, 0]), crec * U * Gabs[:m, 0].astype(float), f"multi_dot m={m}")
    G_r, Gabs = hp.gram(A, B)
    for ma, mb in ((5, 9), (16, 16)):
        cg = _const(lambda nr: sk._gram_const(nr, ma, mb, cus), n, P)
        worst.check(f"gram {ma}x{mb}", sk._err(got[f"gram {ma}x{mb}"], G_r[:ma, :mb]), cg * U * Gabs[:ma, :mb].astype(float),
                    f"gram {ma}x{mb}")
    worst.report()


@pytest.mark.parametrize("n,P", SHAPES)
def test_partitioned_orthonormalize(hip, n, P):
    """``hipeig_orthonormalize``, both methods, m = 0, 1, 7: the sequential sweep all-reduces a two-double slot per column
    (``t1``, ``t2``), CGS2 its coefficient records; the returned inner product, the normalised x and the x the lindep exit
    leaves behind, as on one GPU."""
    cus = sk._cus(hip.HipContext.default())
    crec, cdot = _const(_c_rec, n, P, cus), _const(_c_dot, n, P, cus)
    assert crec <= 64, crec                                          # what mgs_bounds' 64 + 4 m allows for the reduction
    cases = sk.ortho_cases(n, [0, 1, 7])
    sets = sk.column_sets(n, 7)
    runs = []
    for name, delta, m, idx in cases:
        x = sk.operand(sets[name], m, delta, idx)
        refs = {0: hp.orthonormalize_mgs(sets[name][:m], x), 1: hp.orthonormalize_cgs2(sets[name][:m], x)}
        for method in (0, 1):
            runs.append((name, delta, m, x, method, refs[method]))

    def body(rank, ctx):
        lo, hi = row_range(n, P, rank)
        dev = {name: [sk._up(ctx, v[lo:hi]) for v in V] for name, V in sets.items()}
        out = []
        for name, delta, m, x, method, (ip_r, _, _) in runs:
            keep = sk._orthonormalize(ctx, hi - lo, dev[name], m, x[lo:hi], float(ip_r) / 4, method)
            exit_ = sk._orthonormalize(ctx, hi - lo, dev[name], m, x[lo:hi], 4 * float(ip_r), method)
            out.append((keep, exit_))
        cols = {name: [sk._down(ctx, b) for b in bufs] for name, bufs in dev.items()}
        return out, cols

    res = on_ranks(P, body)
    worst = _Worst(f"partitioned orthonormalize n={n} P={P}")
    for i, (name, delta, m, x, method, (ip_r, x_r, scale)) in enumerate(runs):
        tag = "mgs" if method == 0 else "cgs2"
        what = f"{tag} {name} delta={delta} m={m}"
        _same_bits([o[0][i][0][0] for o in res], what + ": innerprod")
        nb, xb, xnb = sk.mgs_bounds(m, ip_r, scale) if method == 0 else sk.cgs2_bounds(m, ip_r, scale, crec, cdot)
        s_r = np.sqrt(ip_r)
        ip, dep, _ = res[0][0][i][0]
        assert [o[0][i][0][1] for o in res] == [0] * P, f"{what}: reported linearly dependent at lindep = ip* / 4 (innerprod {ip})"
        xo = np.concatenate([o[0][i][0][2] for o in res])
        worst.check(f"{tag} norm", abs(hp.LD(np.sqrt(ip)) - s_r), nb, what + " norm")
        worst.check(f"{tag} x normalised", sk._norm_err(xo, x_r / s_r), xnb, what + " x normalised")
        ip2 = res[0][0][i][1][0]
        assert [o[0][i][1][1] for o in res] == [1] * P, f"{what}: not reported linearly dependent at lindep = 4 ip*"
        assert ip2 == ip, f"{what}: innerprod depends on lindep"
        xo = np.concatenate([o[0][i][1][2] for o in res])
        worst.check(f"{tag} x at the lindep exit", sk._norm_err(xo, x_r), xb, what + " x at the lindep exit")
    for name, V in sets.items():
        for j in range(len(V)):
            np.testing.assert_array_equal(np.concatenate([o[1][name][j] for o in res]), V[j], err_msg=f"{name} column {j} was written to")
    worst.report()
