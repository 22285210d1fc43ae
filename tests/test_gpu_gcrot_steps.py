"""Device GCROT(m,k) held to extended precision, cycle by cycle and call by call (``_gcrot_steps.py`` has the reference,
the measure ``D``, the invariants, the derivation of every primitive bound and the exits; ``test_gcrot_steps_cpu.py``
validates all of it without a GPU).

``gcrotmk_device`` takes a provider of the vector operations.  ``Recording`` wraps the real ``_Ops`` / ``_PairOps``: it
forwards every call (``dtype`` and ``cols_per_pass`` included) and downloads the operands and the result of each.  One
run then gives two kinds of check:

(a) the trajectory: per cycle ``x``, ``r``, ``c``, ``u``, ``beta``, ``alpha``, ``gamma`` within ``8 D`` of the
    ``longdouble`` run, the invariants within 8 x their constants, inner step and product counts, ``info`` and ``stats``
    equal to the reference's;
(b) every primitive call against ``longdouble`` on the device's own inputs, within its derived bound - a local relation,
    so a failure names the call and nothing is amplified.

Every test prints what the device used of each bound (``-s`` shows it; EXPERIMENTS.md records it)."""
import numpy as np
import pytest
import scipy.sparse as sp

import _gcrot_precond_cases as gc
import _gcrot_steps as gs
import _hiprec as hp
import _minres_steps as ms
import _product_cases as pc
import _sweep_cases as sw
from eigensolvers_amd.gcrotmk import _Ops, _PairOps, gcrotmk_device
from test_gpu_orthogonalisation import _check_step, _down, _up, _Worst

pytestmark = pytest.mark.gpu
LD = hp.LD


# ---------------------------------------------------------------- device helpers
def _upv(ctx, a, pair):
    a = np.asarray(a)
    return (_up(ctx, a.real), _up(ctx, a.imag if np.iscomplexobj(a) else np.zeros(len(a)))) if pair else _up(ctx, a)


def _downv(ctx, v, pair):
    return _down(ctx, v[0]) + 1j * _down(ctx, v[1]) if pair else _down(ctx, v)


class Recording:
    """A provider that forwards to the device provider ``ops`` and logs ``(name, inputs, result)`` of every call with host
    copies, in the form ``_gcrot_steps.HostOps`` logs them.  Anything else (``dtype``, ``cols_per_pass``, ``new`` ...) is
    the wrapped provider's own."""

    def __init__(self, ops, ctx, pair, log):
        self._ops, self._ctx, self._pair, self.log = ops, ctx, pair, log

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def _d(self, v):
        return _downv(self._ctx, v, self._pair)

    def zeros(self):
        out = self._ops.zeros()
        self.log.append(("zeros", (), self._d(out)))
        return out

    def copy(self, a):
        out = self._ops.copy(a)
        self.log.append(("copy", (self._d(a),), self._d(out)))
        return out

    def dot(self, a, b):
        out = self._ops.dot(a, b)
        self.log.append(("dot", (self._d(a), self._d(b)), out))
        return out

    def nrm2(self, a):
        out = self._ops.nrm2(a)
        self.log.append(("nrm2", (self._d(a),), out))
        return out

    def axpy(self, alpha, x, y):
        before = self._d(y)
        self._ops.axpy(alpha, x, y)
        self.log.append(("axpy", (alpha, self._d(x), before), self._d(y)))

    def scal(self, alpha, x):
        before = self._d(x)
        self._ops.scal(alpha, x)
        self.log.append(("scal", (alpha, before), self._d(x)))

    def scaled(self, alpha, x):
        out = self._ops.scaled(alpha, x)
        self.log.append(("scaled", (alpha, self._d(x)), self._d(out)))
        return out

    def arnoldi_step(self, vs, w):
        before = self._d(w)
        nb, h, na = self._ops.arnoldi_step(vs, w)
        self.log.append(("arnoldi_step", ([self._d(v) for v in vs], before), (nb, np.array(h), na, self._d(w))))
        return nb, h, na

    def combine(self, coeffs, vecs):
        out = self._ops.combine(coeffs, vecs)
        self.log.append(("combine", (np.array(coeffs), [self._d(v) for v in vecs]), self._d(out)))
        return out


_OPERATORS = {}


def _operator(hip, op):
    """``(device operator, CSR arrays)`` of an ``ms.Operator``, uploaded once."""
    if id(op) not in _OPERATORS:
        A = gs.stored(op).copy()                      # a copy: the stored order stays what the CPU twins multiply with
        A.sort_indices()
        _OPERATORS[id(op)] = (hip.HipCsrOperator.from_scipy(A), (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.copy()))
    return _OPERATORS[id(op)]


def _solve(hip, op, b, z, sign, pair, cols, maxiter, x0=None, jacobi=False, rtol=0.0, atol=0.0):
    """GCROT(3, 2) through ``gcrotmk_device`` on the recording provider, products as ``HipVector.solve`` makes them:
    ``(x buffers, info, stats, log, minv buffers, minv host)``."""
    ctx = hip.HipContext.default()
    H, _ = _operator(hip, op)
    n, reverse = op.n, sign < 0
    log = []
    minv = H.jacobi_inverse_z(z, gs.FLOOR) if jacobi else None
    minv_h = None
    if jacobi:
        minv_h = _down(ctx, minv[0]) + (1j * _down(ctx, minv[1]) if minv[1] is not None else 0.0)

    def matvec(v):
        if pair:
            if minv is not None:
                out = H.apply_shifted_pairs_m([z], [minv], [v], reverse=reverse)[0]
            else:
                out = (ctx.alloc(n), ctx.alloc(n))
                H.apply_shifted_pair(z, v[0], v[1], out[0], out[1], reverse=reverse)
        else:
            out = ctx.alloc(n)
            if minv is not None:
                H.apply_shifted_m(z, minv, v, out, reverse=reverse)
            else:
                H.apply_shifted(z, v, out, reverse=reverse)
        log.append(("mv", (_downv(ctx, v, pair),), _downv(ctx, out, pair)))
        return out

    ops = Recording((_PairOps if pair else _Ops)(ctx, n, cols), ctx, pair, log)
    assert ops.cols_per_pass == cols and (ops.dtype == np.complex128 if pair else not hasattr(ops, "dtype"))
    x, info, stats = gcrotmk_device(ctx, matvec, _upv(ctx, b, pair), n, rtol=rtol, atol=atol, maxiter=maxiter, m=gs.M_INNER,
                                    k=gs.K_OUTER, complex_pairs=pair, x0=None if x0 is None else _upv(ctx, x0, pair), ops=ops)
    return x, info, stats, log, minv, minv_h


# ---------------------------------------------------------------- (b) the calls the primitive table does not cover
def _check_arnoldi(worst, log, pair):
    for i, (name, ins, res) in enumerate(log):
        if name != "arnoldi_step":
            continue
        V, w = ins
        V = np.array(V)
        nb, h, na, w_out = res
        with np.errstate(divide="ignore"):
            normalised = bool(np.isfinite(1.0 / np.float64(na)))   # an exact zero stays unnormalised (the breakdown step)
        ref = hp.mgs(V, w, normalise=normalised)
        vn = np.array([float(hp.nrm2(v)) for v in V])
        _check_step(worst, "arnoldi", f"call {i} ({len(V)} columns)", (nb, h, na, w_out), ref, vn, normalised=normalised)


def _check_products(worst, log, op, csr, z, sign, pair, minv):
    """Plain products: the bounds of their own tests on the device's operand.  Jacobi products: the same at the scaled
    operand ``t* = minv x`` in longdouble, plus the scaling element's bound ``e`` pushed through the operator,
    ``|z| e + |H| e`` per half."""
    n = op.n
    Habs = abs(gs.stored(op).copy()).tocsr()
    for i, (name, ins, res) in enumerate(log):
        if name != "mv":
            continue
        x = ins[0]
        if pair:
            xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
            push_r = push_i = 0.0
            if minv is not None:
                mi = np.ascontiguousarray(minv.imag) if np.iscomplexobj(minv) else None
                xr, xi, er, ei = gc.diag_mul_reference(np.ascontiguousarray(minv.real), mi, xr, xi)
                push_r = abs(z.real) * er + abs(z.imag) * ei + Habs @ er
                push_i = abs(z.real) * ei + abs(z.imag) * er + Habs @ ei
            products = pc.half_products(*csr, xr, xi)
            ref_r, ref_i = pc.shift_pair_reference(*csr, xr, xi, z, sign, 0, products)
            br, bi = pc.shift_pair_bound(*csr, xr, xi, z, sign, 0, products)
            worst.check("product", np.abs(res.real.astype(LD) - ref_r).astype(float), br + push_r, f"call {i} re")
            worst.check("product", np.abs(res.imag.astype(LD) - ref_i).astype(float), bi + push_i, f"call {i} im")
        else:
            t, push = x.astype(LD), 0.0
            if minv is not None:
                t, _, e, _ = gc.diag_mul_reference(minv, None, x, None)
                push = abs(z) * e + Habs @ e
            ref = LD(sign) * (LD(z) * t - hp.csr_matvec(*csr, t)[0])
            shifted = sp.csr_matrix(sign * (z * sp.identity(n) - gs.stored(op)))
            worst.check("product", np.abs(res.astype(LD) - ref).astype(float), sw.product_bound(shifted, t.astype(float)) + push, f"call {i}")


def _check_primitives(worst, log, pair, n, cus):
    for label, (ratio, i) in gs.check_log(log, pair, *gs.grids(n, cus)).items():
        worst.check(label, ratio, 1.0, f"{label}, call {i} ({log[i][0]})")


# ---------------------------------------------------------------- (a) + (b): the step cases
def _step_params():
    out = []
    for tag in ("real", "pair"):
        out += [(f"g1037 {tag} sign={s}", cols) for s in ("+1", "-1") for cols in (1, 4)]
        out += [(f"g20001 {tag}", 1), (f"g20001 {tag}", 4), (f"g1037 {tag} x0", 1), (f"g1037 {tag} jacobi", 4)]
        out += [(f"{name} {tag}", cols) for name in ("g63", "g64", "g65", "dense1", "dense2") for cols in (1, 4)]
    return out


@pytest.mark.parametrize("name,cols", _step_params())
def test_cycles_and_every_call_against_extended_precision(hip, name, cols):
    case = gs.CASES[name]
    ctx = hip.HipContext.default()
    cus = int(ctx.device_info()["cus"])
    _, csr = _operator(hip, case.op)
    H = _operator(hip, case.op)[0]
    x, info, stats, log, minv, minv_h = _solve(hip, case.op, case.b, case.z, case.sign, case.pair, cols, case.ncycles,
                                               x0=case.x0, jacobi=case.jacobi)
    worst = _Worst(f"gcrot steps {name} cols={cols}")
    # (a) the trajectory
    ref = gs.reference(case, minv=minv_h)
    run = gs.cycle_records(log)
    assert len(run) == len(ref) == case.ncycles
    assert info == case.ncycles and stats["outer"] == case.ncycles
    assert stats["matvecs"] == sum(1 for e in log if e[0] == "mv") == sum(r["products"] for r in ref) + (1 if case.with_x0 else 0)
    for cyc, (g, r) in enumerate(zip(run, ref), start=1):
        assert (g["inner"], g["products"]) == (r["inner"], r["products"]), f"cycle {cyc}"
        for q, d in gs.deviations(g, r).items():
            worst.check(f"8D {q}", d, case.bound, f"cycle {cyc} {q}: {d:.1f} u")
    for cyc, inv in enumerate(gs.case_invariants(case, run, minv=minv_h), start=1):
        for q in gs.INVARIANTS:
            worst.check(f"inv {q}", inv[q], gs.FACTOR * gs.INV[q], f"cycle {cyc} invariant {q}: {inv[q]:.2f} u")
    np.testing.assert_array_equal(_downv(ctx, x, case.pair), run[-1]["x"])
    if case.jacobi:
        H.diag_mul(minv, x, x)                               # x = M u, as HipVector.solve ends
    worst.check("8D final", gs.final_deviation(_downv(ctx, x, case.pair), ref.final), case.bound, "final x")
    # (b) every call
    _check_primitives(worst, log, case.pair, case.op.n, cus)
    _check_arnoldi(worst, log, case.pair)
    _check_products(worst, log, case.op, csr, case.z, case.sign, case.pair, minv_h)
    worst.report()


# ---------------------------------------------------------------- 3. the primitives outside a solve
@pytest.mark.parametrize("pair", [False, True], ids=["real", "pair"])
@pytest.mark.parametrize("n", gs.LENGTHS)
def test_vector_operations_against_extended_precision(hip, n, pair):
    """``_Ops`` / ``_PairOps`` alone on operands spanning orders of magnitude: ``dot``, ``nrm2``, ``copy``, ``zeros``,
    ``axpy`` / ``scal`` / ``scaled`` with every scalar (real providers take the real ones) and ``combine`` over 1 .. 31
    vectors (2 .. 62 real inputs of ``hipeig_lincomb`` for pairs: its 4-, 8- and 16-wide kernels, one, two and four
    chunks), each within its derived bound, the inputs bit for bit unchanged after every call."""
    ctx = hip.HipContext.default()
    cus = int(ctx.device_info()["cus"])
    ops = (_PairOps if pair else _Ops)(ctx, n)
    log = []
    rec = Recording(ops, ctx, pair, log)
    worst = _Worst(f"vector operations {'pair' if pair else 'real'} n={n}")
    V = gs.vectors(n, max(gs.COMBINE_COUNTS))
    if not pair:
        V = np.ascontiguousarray(V.real)
    dev = [_upv(ctx, v, pair) for v in V]

    def unchanged(idx, what):
        for j in idx:
            assert _downv(ctx, dev[j], pair).tobytes() == V[j].tobytes(), f"{what}: input {j} changed"

    rec.dot(dev[0], dev[1]); unchanged((0, 1), "dot")
    rec.dot(dev[2], dev[2])
    rec.nrm2(dev[3]); unchanged((3,), "nrm2")
    rec.copy(dev[4]); unchanged((4,), "copy")
    if pair:
        rec.zeros()
    for alpha in gs.SCALARS:
        if not pair and complex(alpha).imag != 0.0:
            continue
        a = alpha if pair else complex(alpha).real
        y = rec.copy(dev[5])
        rec.axpy(a, dev[6], y); unchanged((5, 6), f"axpy {alpha}")
        rec.scaled(a, dev[7]); unchanged((7,), f"scaled {alpha}")
        y = rec.copy(dev[7])
        rec.scal(a, y); unchanged((7,), f"scal {alpha}")
    for k in gs.COMBINE_COUNTS:
        cf = gs.coefficients(k)
        rec.combine(cf if pair else np.ascontiguousarray(cf.real), dev[:k]); unchanged(range(k), f"combine {k}")
    _check_primitives(worst, log, pair, n, cus)
    if pair:
        assert {"pair axpy re", "pair axpy real scalar re", "pair scal re", "pair scaled im", "scal real scalar", "pair combine im",
                "pair dot im", "pair nrm2", "copy", "zeros"} <= set(worst.ratio)
    else:
        assert {"axpy", "scal real scalar", "scaled real scalar", "combine", "dot", "nrm2", "copy"} <= set(worst.ratio)
    worst.report()


# ---------------------------------------------------------------- 4. exits
@pytest.mark.parametrize("name", list(gs.EXITS))
def test_exits_end_where_the_reference_ends(hip, name):
    """``info``, ``stats["outer"]`` and ``stats["matvecs"]`` of the reference (whose decisions all have a margin of 2, so
    rounding cannot move them), the number of cycles and their inner steps, and the iterate within ``8 D``."""
    e = gs.EXITS[name]
    ctx = hip.HipContext.default()
    if e.raises is not None:
        with pytest.raises(e.raises, match="finite"):
            _solve(hip, e.op, e.b, e.z, e.sign, e.pair, 1, e.maxiter, x0=e.x0, rtol=e.rtol, atol=e.atol)
        return
    ref = e.run(gs.Wide(e.pair))
    x, info, stats, log, _, _ = _solve(hip, e.op, e.b, e.z, e.sign, e.pair, 1, e.maxiter, x0=e.x0, rtol=e.rtol, atol=e.atol)
    run = gs.cycle_records(log)
    products = sum(1 for entry in log if entry[0] == "mv")
    print(f"\nGCROT-GPU exit {name}: info {info}, outer {stats['outer']}, {products} products, {len(run)} cycles")
    assert (info, stats["outer"], stats["matvecs"], products) == (ref.info, ref.outer, ref.products, ref.products)
    assert [r["inner"] for r in run] == [r["inner"] for r in ref]
    got = _downv(ctx, x, e.pair)
    if np.any(ref.final):
        d = gs.final_deviation(got, ref.final)
        print(f"GCROT-GPU exit {name}: iterate {d:.1f} u of {gs.FACTOR * gs.D:.0f}")
        assert d <= gs.FACTOR * gs.D
    else:
        assert not np.any(got)
        assert products == 0 and not any(entry[0] == "arnoldi_step" for entry in log)
    worst = _Worst(f"exit {name}")
    _check_primitives(worst, log, e.pair, e.op.n, int(ctx.device_info()["cus"]))


@pytest.mark.parametrize("z", [gs.Z_REAL, gs.Z_PAIR], ids=["real", "pair"])
def test_solve_raises_when_maxiter_is_reached(hip, z):
    """``HipVector.solve`` turns ``info = maxiter`` into ``UserWarning`` (one cycle of GCROT(20, 20) cannot reach 1e-30)."""
    H, _ = _operator(hip, ms.operator("g1037"))
    opts = {"linearSystemArgs": {"linearSolver": "gcrotmk", "linearIter": 1, "linear_tol": 1e-30, "linear_atol": 0.0}}
    b = hip.HipVector(ms.rhs(1037).copy(), opts)
    with pytest.raises(UserWarning, match="not converged"):
        hip.HipVector.solve(H, b, z)
    assert b.last_solve_stats["outer"] == 1 and b.last_solve_stats["iterations"] == 40
