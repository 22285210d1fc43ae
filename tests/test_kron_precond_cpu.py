"""Host side of the separable preconditioner of the Kronecker-sum operator: the additive fit, the twin against SciPy's
``minres(A, b, M=...)``, the iteration counts it buys, and the refusals that need no device."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import _kron_cases as kc
import _kron_precond_cases as kp
from eigensolvers_amd.generators import coupled_oscillator_grid
from eigensolvers_amd.hip_vector import _preconditioner
from eigensolvers_amd.precond_minres import (jacobi_inverse_host, minres_jacobi_host, minres_precond_host,
                                             separable_apply_host, separable_basis_host, separable_fit_host,
                                             separable_scale_host)
from oracle.minres_ref import minres as minres_ref


def test_fit_reproduces_an_additive_potential():
    dims, ranges, freqs = kp.GRID, [(-5, 5), (-4.5, 4.5), (-4, 4)], [1.0, 1.3, 1.7]
    factors, V = coupled_oscillator_grid(dims, ranges, freqs, coupled=False)
    V = np.asarray(V).reshape(dims)
    v = separable_fit_host(V, dims)
    assert [a.shape for a in v] == [(n,) for n in dims]
    fit = v[0][:, None, None] + v[1][None, :, None] + v[2][None, None, :]
    assert np.max(np.abs(fit - V)) <= 1e-13 * np.max(np.abs(V))
    # a coupled V is not reproduced, but the fit is the least-squares one: the residual has no additive part left
    factors, Vc = coupled_oscillator_grid(dims, ranges, freqs)
    Vc = np.asarray(Vc).reshape(dims)
    vc = separable_fit_host(Vc, dims)
    res = Vc - (vc[0][:, None, None] + vc[1][None, :, None] + vc[2][None, None, :])
    assert np.max(np.abs(res)) > 1e-3 * np.max(np.abs(Vc))
    for again in separable_fit_host(res, dims):
        assert np.max(np.abs(again)) <= 1e-12 * np.max(np.abs(Vc))
    assert all(np.array_equal(a, np.zeros(n)) for a, n in zip(separable_fit_host(None, dims), dims))


def test_basis_scale_and_apply_are_what_they_say():
    p = kp.problem((2, 3, 4, 5))
    for T, v, Q, lam in zip(p["factors"], p["potentials"], p["bases"], p["eigenvalues"]):
        A = T + np.diag(v)
        assert np.max(np.abs(Q @ np.diag(lam) @ Q.T - A)) <= 1e-12 * np.max(np.abs(A))
    Lam = np.zeros(p["dims"])
    for d, lam in enumerate(p["eigenvalues"]):                      # mode order, one rounded add per mode
        shape = [1] * len(p["dims"])
        shape[d] = -1
        Lam = lam.reshape(shape) if d == 0 else Lam + lam.reshape(shape)
    np.testing.assert_array_equal(p["sinv"], jacobi_inverse_host(np.broadcast_to(Lam, p["dims"]).reshape(-1), p["sigma"], kp.FLOOR))
    Qfull = p["bases"][0]
    for Q in p["bases"][1:]:
        Qfull = np.kron(Qfull, Q)
    M = Qfull @ np.diag(p["sinv"]) @ Qfull.T
    r = kc.operand(kc.size(p["dims"]), 3)
    np.testing.assert_allclose(separable_apply_host(p["bases"], p["sinv"], r), M @ r, rtol=0, atol=1e-13 * np.max(p["sinv"]) * np.linalg.norm(r))
    assert np.all(np.linalg.eigvalsh(M) > 0)


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("dims", [(13, 10, 7), (17, 3), (2, 3, 4, 5)])
def test_twin_equals_scipy(dims, rtol):
    p = kp.problem(dims)
    n = kc.size(dims)
    x, info, itn, istop, trace = kp.twin(dims, rtol)
    count = []
    xs, infos = spla.minres(spla.LinearOperator((n, n), matvec=kp.shifted(p), dtype=np.float64), p["b"],
                            M=spla.LinearOperator((n, n), matvec=kp.apply_f64(p), dtype=np.float64), rtol=rtol, maxiter=4000,
                            callback=lambda xk: count.append(1))
    print(f"dims {dims} rtol {rtol}: twin {itn} iterations (istop {istop}), SciPy {len(count)}")
    assert info == infos == 0 and itn == len(count) and istop == 1
    assert np.max(np.abs(x - xs)) <= 1e-12 * np.linalg.norm(xs)


def test_jacobi_twin_is_the_general_twin_with_a_diagonal():
    p = kp.problem((17, 3))
    minv = jacobi_inverse_host(p["Hs"].diagonal(), p["sigma"], kp.FLOOR)
    a = minres_jacobi_host(kp.shifted(p), p["b"], minv, rtol=1e-8, maxiter=400)
    b = minres_precond_host(kp.shifted(p), p["b"], lambda r: minv * r, rtol=1e-8, maxiter=400)
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1:] == b[1:]


def test_counts_on_the_fixture_grid():
    """plain 129, Jacobi 54, the factors alone 564, the factors with the additive fit of V 25: the 1-D potentials are
    what makes it a preconditioner."""
    p = kp.problem(kp.GRID)
    rtol = 1e-10
    plain = minres_ref(kp.shifted(p), p["b"], rtol=rtol, maxiter=4000)[2]
    minv = jacobi_inverse_host(p["Hs"].diagonal(), p["sigma"], kp.FLOOR)
    jacobi = minres_jacobi_host(kp.shifted(p), p["b"], minv, rtol=rtol, maxiter=4000)[2]
    bases0, lam0 = separable_basis_host(p["factors"], separable_fit_host(None, p["dims"]))
    sinv0 = separable_scale_host(lam0, p["sigma"], kp.FLOOR)
    bare = minres_precond_host(kp.shifted(p), p["b"], lambda r: separable_apply_host(bases0, sinv0, r), rtol=rtol, maxiter=4000)[2]
    sep = kp.twin(kp.GRID, rtol)[2]
    print(f"MINRES iterations on {kp.GRID} at rtol {rtol}: plain {plain}, Jacobi {jacobi}, separable without potentials {bare}, "
          f"separable {sep}")
    # 129 and 25 are posed (test_gpu_kron._count_is_posed, kp.count_is_posed) and pinned; the Jacobi count and the one
    # without potentials move by a few with the rounding of the products (52 here, 53 with SciPy on the explicit shifted
    # matrix, 54 counted elsewhere; 566 against 564), so only their order is
    assert plain == 129 and sep == 25
    assert sep < jacobi < plain < bare
    assert abs(jacobi - 54) <= 3 and abs(bare - 564) <= 6                 # 5 % and 1 %: the table, to what rounding moves it


def _lsa(**kw):
    d = {"linearSolver": "minres", "linearIter": 100, "linear_tol": 1e-8}
    d.update(kw)
    return d


def test_refusals_without_a_device():
    assert _preconditioner(_lsa(preconditioner="separable"), 0.02) == "separable"
    assert _preconditioner(_lsa(preconditioner="separable", preconditionerPotentials=None), 0.02) == "separable"
    assert _preconditioner(_lsa(preconditioner="separable", preconditionerPotentials=[np.zeros(3), np.zeros(4)]), 0.02) == "separable"
    for bad in (np.zeros((3, 4)), "fit", [np.zeros((2, 2))], [3.0], 1.0, [np.zeros(3) + 1j]):
        with pytest.raises(ValueError, match="preconditionerPotentials"):
            _preconditioner(_lsa(preconditioner="separable", preconditionerPotentials=bad), 0.02)
    with pytest.raises(ValueError, match="separable"):
        _preconditioner(_lsa(preconditioner="ilu"))
    for name in ("gcrotmk", "pardiso"):
        with pytest.raises(ValueError, match="minres"):
            _preconditioner(_lsa(preconditioner="separable", linearSolver=name))
    for name in ("minres_shifted", "lanczos_filter"):
        with pytest.raises(ValueError, match="shift invariance"):
            _preconditioner(_lsa(preconditioner="separable", linearSolver=name))
    with pytest.raises(ValueError, match="real shift"):
        _preconditioner(_lsa(preconditioner="separable"), 0.02 + 0.1j)
    with pytest.raises(ValueError, match="preconditionerFloor"):
        _preconditioner(_lsa(preconditioner="separable", preconditionerFloor=np.inf), 0.02)
    with pytest.raises(ValueError, match="preconditionerLockStep"):
        _preconditioner(_lsa(preconditioner="separable", preconditionerLockStep=True), 0.02)
    with pytest.raises(NotImplementedError, match="x0"):
        _preconditioner(_lsa(preconditioner="separable"), 0.02, x0=object())

    class Ctx:
        collectives = True
    with pytest.raises(NotImplementedError, match="one GPU"):
        _preconditioner(_lsa(preconditioner="separable"), 0.02, None, Ctx())
    with pytest.raises(NotImplementedError, match="HipKronSumOperator"):
        _preconditioner(_lsa(preconditioner="separable"), 0.02, None, None, H=object())
    with pytest.raises(ValueError, match="not finite"):
        separable_scale_host([np.array([1.0, 2.0]), np.array([0.5, 4.0])], 2.5, 0.0)          # Lam = 2 + 0.5 == sigma
