"""The Jacobi-preconditioned device MINRES (``linearSystemArgs["preconditioner"] = "jacobi"``, csrc/minres.hip, csrc/minres_precond.hip)
against its NumPy twin, which ``test_precond_minres_cpu.py`` pins to ``scipy.sparse.linalg.minres(A, b, M=...)``.

Tolerances are those of ``test_gpu_parity.py::test_minres_tracks_the_oracle`` with the twin in the oracle's place:
iterations and istop equal, x within max(1e-9, 100 rtol) ||x||, rnorm within 5 %, Anorm within 1e-3, true residual
<= 1.05 x the twin's + 1e-13.  The true residual is never compared with the UNpreconditioned solve's: rtol is tested in
the M^-1 norm, so with an exact diagonal hit the preconditioned 2-norm residual is legitimately larger."""
import numpy as np
import pytest
import scipy.sparse as sp

import _precond_cases as pc
from _sweep_cases import check_against_twin as _check_against_twin, within as _within
from eigensolvers_amd.generators import gapped_csr_host, guess_vector
from eigensolvers_amd.precond_minres import csr_diagonal_host, jacobi_inverse_host

pytestmark = pytest.mark.gpu


def _opts(it=2000, tol=1e-10, pre="jacobi", **lsa):
    d = {"linearSolver": "minres", "linearIter": it, "linear_tol": tol}
    if pre is not None:
        d["preconditioner"] = pre
    d.update(lsa)
    return {"linearSystemArgs": d}


# ---------------------------------------------------------------- N = 4000: tracks the twin
@pytest.fixture(scope="module")
def gapped16(hip):
    Hh = gapped_csr_host(4000, 16, seed=7)
    return Hh, hip.HipCsrOperator.from_scipy(Hh), pc.unit_guess(4000)


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
def test_tracks_the_twin(hip, gapped16, rtol):
    """Fails without the feature: the key is ignored there and the solve takes 664 iterations, not 17."""
    Hh, H, b = gapped16
    tw = pc.twin("g4000", Hh, b, pc.SIGMA, rtol, 2000)
    B = hip.HipVector(b.copy(), _opts(2000, rtol))
    W = hip.HipVector.solve(H, B, pc.SIGMA)
    assert B.last_solve_stats is W.last_solve_stats
    _check_against_twin(f"g4000 rtol {rtol:g}", Hh, b, pc.SIGMA, rtol, W, tw)
    assert W.last_solve_stats["iterations"] < 40
    # reverse Green's function: only the sign flips, M is the same
    Wr = hip.HipVector.solve(H, B, pc.SIGMA, reverseGF=True)
    assert Wr.last_solve_stats["iterations"] == tw[2]
    _within(Wr.array, -tw[0], max(1e-9, 100 * rtol) * np.linalg.norm(tw[0]))
    # the derived vector carries the key (options travel with the vectors)
    assert W.options["linearSystemArgs"]["preconditioner"] == "jacobi"
    assert W._new(W._buf).options["linearSystemArgs"] is B.options["linearSystemArgs"]


def test_without_the_key_the_plain_solver_runs(hip, gapped16):
    Hh, H, b = gapped16
    W0 = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(2000, 1e-10, pre=None)), pc.SIGMA)
    W1 = hip.HipVector.solve(H, hip.HipVector(b.copy(), {"linearSystemArgs": {"linearSolver": "minres", "linearIter": 2000,
                                                                              "linear_tol": 1e-10, "preconditioner": None}}), pc.SIGMA)
    assert "preconditioner" not in W0.last_solve_stats and "preconditioner" not in W1.last_solve_stats
    assert W0.last_solve_stats["iterations"] == W1.last_solve_stats["iterations"] > 300
    np.testing.assert_array_equal(W0.array, W1.array)


# ---------------------------------------------------------------- every layout, both kernel forms
@pytest.fixture(scope="module")
def gapped300k():
    n = 300_000                                                # three column windows of the blocked layouts
    Hh = gapped_csr_host(n, 16, seed=7)
    b = pc.unit_guess(n)
    return Hh, b, pc.twin("g300k", Hh, b, pc.SIGMA, 1e-8, 3000)


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5])
def test_every_layout_both_kernel_forms(hip, gapped300k, monkeypatch, variant):
    """KD riding on the next sweep (default) against KD as its own kernel (HIPEIG_MINRES_FUSE_KD=0): counts and stop codes
    are the twin's in every sweep layout, and the two forms agree bit for bit wherever the layout fixes the order of a
    row's adds (1, 2, 3 and the fixed-point 5; the fp64 LDS atomics of 4 add a row in varying order, as in the plain
    solver's test of the same name)."""
    Hh, b, tw = gapped300k
    H = hip.HipCsrOperator.from_scipy(Hh)
    H.set_variant(variant)
    out = []
    for form in (None, "0"):
        monkeypatch.delenv("HIPEIG_MINRES_FUSE_KD", raising=False)
        if form:
            monkeypatch.setenv("HIPEIG_MINRES_FUSE_KD", form)
        W = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(3000, 1e-8)), pc.SIGMA)
        assert H.last_variant() == H.VARIANTS[variant]
        _check_against_twin(f"g300k variant {variant} fuse {form}", Hh, b, pc.SIGMA, 1e-8, W, tw)
        out.append(W.array)
    monkeypatch.delenv("HIPEIG_MINRES_FUSE_KD", raising=False)
    assert tw[2] <= 20
    if variant == 4:
        assert np.linalg.norm(out[0] - out[1]) <= 1e-7 * np.linalg.norm(tw[0])
    else:
        np.testing.assert_array_equal(out[0], out[1])


# ---------------------------------------------------------------- smallest shapes where the kernels can go wrong
def test_odd_length_with_an_exact_diagonal_hit(hip):
    """n = 4001 (the double2 tail of the element-wise kernels), one h_ii == sigma exactly (the floor) and one stored zero."""
    Hh, hit, zero = pc.exact_hit_operator()
    b = pc.unit_guess(4001)
    H = hip.HipCsrOperator.from_scipy(Hh)
    d = hip.HipVector(H.diagonal()).array
    np.testing.assert_array_equal(d, csr_diagonal_host(Hh))
    assert d[hit] == pc.SIGMA and d[zero] == 0.0
    minv = hip.HipVector(H.jacobi_inverse(pc.SIGMA)).array
    assert np.isfinite(minv).all()
    np.testing.assert_allclose(minv, jacobi_inverse_host(d, pc.SIGMA), rtol=4e-16, atol=0)
    assert H.jacobi_inverse(pc.SIGMA) is H.jacobi_inverse(pc.SIGMA)                  # cached per (sigma, floor)
    tw = pc.twin("hit4001", Hh, b, pc.SIGMA, 1e-10, 2000)
    W = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(2000, 1e-10)), pc.SIGMA)
    _check_against_twin("hit4001", Hh, b, pc.SIGMA, 1e-10, W, tw)
    # floor 0 with the exact hit: an error, not a division by zero
    with pytest.raises(ValueError, match="not finite"):
        hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(2000, 1e-10, preconditionerFloor=0.0)), pc.SIGMA)
    # another floor is another M: the twin with that floor is the reference
    tw3 = pc.twin("hit4001", Hh, b, pc.SIGMA, 1e-10, 2000, floor=1e-3)
    W3 = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(2000, 1e-10, preconditionerFloor=1e-3)), pc.SIGMA)
    _check_against_twin("hit4001 floor 1e-3", Hh, b, pc.SIGMA, 1e-10, W3, tw3)


def test_diagonal_with_duplicate_entries(hip):
    """Duplicate (i, i) entries are separate stored elements: the device sums them in stored order like the host."""
    Hh = gapped_csr_host(4001, 16, seed=7).tocoo()
    extra = np.arange(0, 4001, 7)
    rows = np.concatenate([Hh.row, extra, extra[::2]])
    cols = np.concatenate([Hh.col, extra, extra[::2]])
    vals = np.concatenate([Hh.data, 0.125 + 1e-3 * extra, -0.5 + 1e-4 * extra[::2]])
    order = np.argsort(rows, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=4001))])
    A = sp.csr_matrix((vals[order], cols[order], indptr), shape=(4001, 4001))
    assert A.nnz == len(vals)
    ref = csr_diagonal_host(A)
    assert np.abs(ref - gapped_csr_host(4001, 16, seed=7).diagonal()).max() > 0.1
    H = hip.HipCsrOperator.from_scipy(A)
    assert H.nnz == len(vals)
    np.testing.assert_array_equal(hip.HipVector(H.diagonal()).array, ref)
    empty = sp.csr_matrix((np.array([1.0, 2.0, 2.0]), np.array([1, 0, 2]), np.array([0, 1, 2, 3])), shape=(3, 3))   # row 0, 1: no diagonal
    np.testing.assert_array_equal(hip.HipVector(hip.HipCsrOperator.from_scipy(empty).diagonal()).array, [0.0, 0.0, 2.0])


# Shifts of the n = 100 case.  A comparison with the twin means something only while the twin itself is determinate, and on
# this matrix that is a question of the shift: at sigma = 30.3 (inside the spectrum 1..200; test_precond_minres_cpu.py pins the
# twin to SciPy there, same product bits) the solve needs 103 iterations on n = 100, the Lanczos vectors lose orthogonality
# near iteration 80, and the twin ALONE - same code, only the order of the adds inside its matrix product changed (dense
# ``A @ v``, CSR product, ``A.T.T @ v``) - gives Anorm 13.8245 / 13.8165 / 13.7902 at 1e-8 (2.5e-3, against this file's
# bound of 1e-3) and 79 / 80 / 82 iterations at 1e-3: no reference exists there to the tolerances of this file.  Outside the
# spectrum the same three twins agree to rounding - sigma = -20 at 1e-10: 35 iterations each, Anorm to 4e-16, rnorm to
# 3e-15, x to 7e-16 ||x||; sigma = 0 at 1e-8: 54 iterations each, 2e-16 / 7e-15 / 6e-15 - eleven orders inside the bounds,
# so these are the cases (pc.DENSE_CASES; test_precond_minres_cpu.py checks that agreement): 35 and 54 iterations cross the
# chunk boundaries at 16, 32 and 48.
@pytest.mark.parametrize("sigma,rtol", pc.DENSE_CASES)
def test_smaller_than_one_workgroup_on_the_dense_matrix(hip, sigma, rtol):
    """n = 100 through from_dense, the reference's dense matrix: every kernel runs on less than one workgroup's worth of
    rows (one partial per reduction, the last-workgroup ticket taken by the only workgroup)."""
    A = pc.dense_operator()
    b = pc.unit_guess(100)
    tw = pc.twin("dense100", A, b, sigma, rtol, 2000)
    assert tw[2] in (35, 54) and tw[3] == 1
    H = hip.HipCsrOperator.from_dense(A)
    np.testing.assert_array_equal(hip.HipVector(H.diagonal()).array, np.diag(A))
    W = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(2000, rtol)), sigma)
    _check_against_twin(f"dense100 sigma {sigma:g}", A, b, sigma, rtol, W, tw)


def test_zero_right_hand_side_and_iteration_limit(hip, gapped16):
    Hh, H, b = gapped16
    W = hip.HipVector.solve(H, hip.HipVector(np.zeros(4000), _opts()), pc.SIGMA)
    assert not W.array.any() and W.last_solve_stats["iterations"] == 0
    need = pc.twin("g4000", Hh, b, pc.SIGMA, 1e-10, 2000)[2]
    B = hip.HipVector(b.copy(), _opts(need - 5, 1e-10))
    with pytest.raises(UserWarning, match="not converged"):
        hip.HipVector.solve(H, B, pc.SIGMA)
    assert B.last_solve_stats["iterations"] == need - 5 and B.last_solve_stats["istop"] == 6


def test_chunk_independence(hip, gapped16, monkeypatch):
    """The host looks at the state record every HIPEIG_PMR_CHUNK iterations; kernels enqueued past the stop return at once,
    so chunk 1 (every KD its own kernel, a look per iteration) and the default give the same bits."""
    Hh, H, b = gapped16
    out = []
    for chunk in (None, "1", "5"):
        monkeypatch.delenv("HIPEIG_PMR_CHUNK", raising=False)
        if chunk:
            monkeypatch.setenv("HIPEIG_PMR_CHUNK", chunk)
        W = hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(2000, 1e-10)), pc.SIGMA)
        out.append((W.array, W.last_solve_stats["iterations"], W.last_solve_stats["istop"]))
    monkeypatch.delenv("HIPEIG_PMR_CHUNK", raising=False)
    for x, itn, istop in out[1:]:
        assert (itn, istop) == out[0][1:]
        np.testing.assert_array_equal(x, out[0][0])


# ---------------------------------------------------------------- one workspace for the plain and the preconditioned solve
_SHIFTS = [0.02 + 0.1j, 0.3 + 0.1j, -0.2 + 0.05j]


def _workspace_calls(hip, ctx):
    """The solves that share the context's MINRES workspace, each as a function of nothing returning its arrays: a plain
    solve (7 vectors of 4000), a Jacobi solve (9 of 4001: the buffer grows and moves), a three-shift solve (which borrows the
    partial-sum areas and totals of both)."""
    Hh, b = gapped_csr_host(4000, 16, seed=7), pc.unit_guess(4000)
    Hx, bx = pc.exact_hit_operator()[0], pc.unit_guess(4001)
    H = hip.HipCsrOperator.from_scipy(Hh, ctx=ctx)
    X = hip.HipCsrOperator.from_scipy(Hx, ctx=ctx)
    so = {"linearSystemArgs": {"linearSolver": "minres_shifted", "linearIter": 2000, "linear_tol": 1e-8, "linear_atol": 0.0}}
    return {
        "plain": lambda: [hip.HipVector.solve(H, hip.HipVector(b.copy(), _opts(2000, 1e-10, pre=None), ctx=ctx), pc.SIGMA).array],
        "jacobi": lambda: [hip.HipVector.solve(X, hip.HipVector(bx.copy(), _opts(2000, 1e-10), ctx=ctx), pc.SIGMA).array],
        "shifted": lambda: [x.array for x in hip.HipVector._solve_shifts(H, hip.HipVector(b.copy(), so, ctx=ctx), _SHIFTS)],
    }


@pytest.fixture(scope="module")
def workspace_refs(hip):
    """Every call of ``_workspace_calls`` made first on a fresh context of its own."""
    return {name: _workspace_calls(hip, hip.HipContext(0))[name]() for name in ("plain", "jacobi", "shifted")}


@pytest.mark.parametrize("fresh", [False, True])
def test_shared_workspace_plain_launches(hip, workspace_refs, fresh):
    """Plain -> Jacobi -> plain -> shifted -> Jacobi on ONE context gives, call by call, the bits of the same call made
    first on a fresh context: on the default context (whatever ran there before) and on a new one, where the Jacobi solve
    grows the workspace from 7 x 4000 to 9 x 4032 doubles under the plain solve's feet."""
    calls = _workspace_calls(hip, hip.HipContext(0) if fresh else hip.HipContext.default())
    for name in ("plain", "jacobi", "plain", "shifted", "jacobi"):
        got = calls[name]()
        assert len(got) == len(workspace_refs[name])
        for g, r in zip(got, workspace_refs[name]):
            assert np.isfinite(g).all() and np.abs(g).max() > 0
            np.testing.assert_array_equal(g, r)


def _slack_solves(hip, ctx):
    """A plain solve at n = 4100 and two larger solves (n = 5000) that would fit in the slack a 9-vector workspace of 4001
    leaves a 7-vector solve: an ``x0`` that is the exact solution, which returns before any iteration, and a whole solve."""
    Ha, ba = gapped_csr_host(4100, 16, seed=7), pc.unit_guess(4100)
    Hb, bb = gapped_csr_host(5000, 16, seed=7), pc.unit_guess(5000)
    A = hip.HipCsrOperator.from_scipy(Ha, ctx=ctx)
    B = hip.HipCsrOperator.from_scipy(Hb, ctx=ctx)
    D = hip.HipCsrOperator.from_scipy(sp.identity(5000, format="csr") * 2.0, ctx=ctx)
    o = _opts(2000, 1e-10, pre=None)

    def exact_guess():                                          # (0 I - 2 I) x = -2 x0 with x0 given: r1 = b - A x0 = 0 exactly
        W = hip.HipVector.solve(D, hip.HipVector(-2.0 * bb, o, ctx=ctx), 0.0, x0=hip.HipVector(bb.copy(), ctx=ctx))
        assert W.last_solve_stats["iterations"] == 0
        np.testing.assert_array_equal(W.array, bb)

    return {"small": lambda: hip.HipVector.solve(A, hip.HipVector(ba.copy(), o, ctx=ctx), pc.SIGMA).array,
            "large": lambda: hip.HipVector.solve(B, hip.HipVector(bb.copy(), o, ctx=ctx), pc.SIGMA).array,
            "exact_guess": exact_guess}


def test_shared_workspace_under_graph_replay(hip, workspace_refs, monkeypatch):
    """HIPEIG_GRAPH=1 (read when a context is created): the plain solve's captured chunk has the workspace pointer and the
    vectors' stride baked in, and the Jacobi solve in between moves that workspace.  The replay after the move must give
    the bits of the replay before it and of the plain launches; the Jacobi solve never replays and gives its plain-launch
    bits.  Then larger solves that fit in the slack of the 9-vector buffer run between two replays of a smaller one - one
    of them leaves before it captures anything - and the smaller solve must still give its plain-launch bits."""
    plain = _slack_solves(hip, hip.HipContext(0))
    ref_small, ref_large = plain["small"](), plain["large"]()
    monkeypatch.setenv("HIPEIG_GRAPH", "1")
    ctx = hip.HipContext(0)
    calls = _workspace_calls(hip, ctx)
    first, jac, second = calls["plain"](), calls["jacobi"](), calls["plain"]()
    np.testing.assert_array_equal(second[0], first[0])
    np.testing.assert_array_equal(second[0], workspace_refs["plain"][0])
    np.testing.assert_array_equal(jac[0], workspace_refs["jacobi"][0])
    slack = _slack_solves(hip, ctx)
    np.testing.assert_array_equal(slack["small"](), ref_small)
    slack["exact_guess"]()
    np.testing.assert_array_equal(slack["small"](), ref_small)
    np.testing.assert_array_equal(slack["large"](), ref_large)
    np.testing.assert_array_equal(slack["small"](), ref_small)


# ---------------------------------------------------------------- refusals
def test_refusals(hip, gapped16):
    Hh, H, b = gapped16
    solve = hip.HipVector.solve
    with pytest.raises(ValueError, match="jacobi"):
        solve(H, hip.HipVector(b.copy(), _opts(pre="ssor")), pc.SIGMA)
    for name in ("gcrotmk", "pardiso"):
        with pytest.raises(ValueError, match="minres"):
            solve(H, hip.HipVector(b.copy(), _opts(linearSolver=name, linear_atol=1e-8)), pc.SIGMA)
    for name in ("minres_shifted", "lanczos_filter"):
        with pytest.raises(ValueError, match="shift invariance"):
            solve(H, hip.HipVector(b.copy(), _opts(linearSolver=name, linear_atol=1e-8)), pc.SIGMA)
    with pytest.raises(ValueError, match="shift invariance"):
        hip.HipVector._solve_shifts(H, hip.HipVector(b.copy(), _opts(linearSolver="minres_shifted", linear_atol=1e-8)), [pc.SIGMA])
    with pytest.raises(ValueError, match="shift invariance"):
        hip.HipVector._lanczos_filter(H, [hip.HipVector(b.copy(), _opts(linearSolver="lanczos_filter", linear_atol=1e-8))],
                                      [0.1 + 0.1j], [1.0 + 0.0j])
    with pytest.raises(ValueError, match="real shift"):
        solve(H, hip.HipVector(b.copy(), _opts()), pc.SIGMA + 0.1j)
    with pytest.raises(ValueError, match="real shift"):
        hip.HipVector.solveBlock(H, [hip.HipVector(b.copy(), _opts())] * 2, [pc.SIGMA + 0.1j, pc.SIGMA - 0.1j])
    with pytest.raises(ValueError, match="preconditionerFloor"):
        solve(H, hip.HipVector(b.copy(), _opts(preconditionerFloor=-1.0)), pc.SIGMA)
    with pytest.raises(NotImplementedError, match="x0"):
        solve(H, hip.HipVector(b.copy(), _opts()), pc.SIGMA, x0=hip.HipVector(b.copy()))
    ctx = hip.HipContext()
    ctx._force_collectives = True                            # what attaching a communicator under HIPEIG_FORCE_COLLECTIVES leaves
    assert ctx.collectives
    with pytest.raises(NotImplementedError, match="one GPU"):
        solve(hip.HipCsrOperator.from_scipy(Hh, ctx=ctx), hip.HipVector(b.copy(), _opts(), ctx=ctx), pc.SIGMA)


def test_solve_block_takes_the_one_by_one_solves(hip, gapped16):
    Hh, H, b = gapped16
    rng = np.random.default_rng(3)
    cols = [b] + [v / np.linalg.norm(v) for v in rng.standard_normal((7, 4000))]
    o = _opts(2000, 1e-10)
    singles = [hip.HipVector.solve(H, hip.HipVector(c.copy(), o), pc.SIGMA) for c in cols]
    block = hip.HipVector.solveBlock(H, [hip.HipVector(c.copy(), o) for c in cols], pc.SIGMA)
    assert len(block) == 8
    for s, x in zip(singles, block):
        assert x.last_solve_stats == s.last_solve_stats and x.last_solve_stats["preconditioner"] == "jacobi"
        np.testing.assert_array_equal(x.array, s.array)


# ---------------------------------------------------------------- the driver
def test_lanczos_driver_with_and_without_the_key(hip, monkeypatch):
    """inexactLanczosDiagonalization needs no change: the option travels with the vectors (restarts included).  The gapped
    N = 4000 single-vector case of _lanczos_cases.py (``gapped4000``); exact eigenvalues from the dense matrix."""
    N, sigma = 4000, pc.SIGMA
    Hh = gapped_csr_host(N, 32, seed=7)
    lam = np.linalg.eigvalsh(Hh.toarray())
    exact = lam[np.argmin(np.abs(lam - sigma))]
    Hd = hip.HipCsrOperator.generate(N, 32, seed=7)
    g = guess_vector(N, 1)
    inner = []
    real_solve = hip.HipVector.solve

    def counting(H, b, s, *a, **k):
        x = real_solve(H, b, s, *a, **k)
        inner.append((x.last_solve_stats["iterations"], x.last_solve_stats.get("preconditioner")))
        return x

    monkeypatch.setattr(hip.HipVector, "solve", staticmethod(counting))
    res = {}
    for pre in (None, "jacobi"):
        inner.clear()
        ev, Y, st = hip.inexactLanczosDiagonalization(Hd, hip.HipVector(g.copy(), _opts(2000, 1e-10, pre=pre)), sigma, 8, 10,
                                                      1e-13, writeOut=False)
        assert st["isConverged"]
        assert all(p == pre for _, p in inner) and len(inner) >= 7
        assert Y[0].options["linearSystemArgs"].get("preconditioner") == pre
        res[pre] = (abs(ev[0] - exact), sum(i for i, _ in inner), len(inner))
        print(f"LANCZOS preconditioner={pre}: theta {ev[0]:.15f} exact {exact:.15f} error {res[pre][0]:.2e}, "
              f"{res[pre][2]} solves, {res[pre][1]} inner iterations")
    assert res["jacobi"][0] <= max(10 * res[None][0], 1e-10 * abs(exact))
    assert res["jacobi"][1] < res[None][1]
