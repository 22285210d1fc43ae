"""The outer cycles of GCROT(m,k) and the vector operations it is assembled from, against extended precision: reference,
deviation measure, cases, primitive bounds and exits (``test_gcrot_steps_cpu.py``, ``test_gpu_gcrot_steps.py``).  A plain
module, imported as ``_minres_steps`` is: no fixtures, no tests.

GCROT repairs itself - it recomputes ``r = b - A x`` before it accepts convergence and minimises again over a fresh Krylov
space every cycle - so a wrong outer update still converges, with more products, and a whole solve held to SciPy sees
nothing.  Its first cycles on a well-conditioned system can be held to a reference run: GCROT(3, 2) over ``NCYCLES = 6``
cycles takes 5, 4, 3, 3, 3, 3 inner steps (21 products); cycle 2 projects against one ``c``, cycle 3 against two, cycles 4
to 6 delete the oldest pair, so every term of the recurrence is live and the truncation has happened three times.

``cycles`` restates SciPy 1.15.3's ``gcrotmk`` for ``sign (z I - H) x = b`` in the operation order of
``eigensolvers_amd/gcrotmk.py`` - sequential MGS against ``[C, V]``, the Hessenberg least squares, ``ux`` and ``cx``, the
scaling by ``alpha``, ``gamma``, the updates of ``r`` and ``x``, ``truncate='oldest'`` - and runs it in two arithmetics:

``Wide``        ``longdouble`` / ``clongdouble`` throughout, the reference.  Products, inner products and the MGS sweep go
                through ``_hiprec`` (``csr_matvec``, ``dot``, ``nrm2``, ``mgs``); a linear combination is the plain sum in
                ``longdouble`` (``_hiprec.combine`` takes float64 rows only; k + 1 roundings of 2^-64 do not count).  The
                least-squares problem is solved by Givens rotations written here, in ``longdouble``: neither the project's
                ``_fgmres`` nor SciPy's ``qr_insert`` / ``lstsq`` is called, the reference is independent of what it judges.
``Double(o)``   float64 with the inner products summed in order ``o`` (``_minres_steps.ORDERS``).  Without a fault it is
                the PROJECT'S OWN generator (``gcrotmk._gcrotmk``) driven with a NumPy provider (``HostOps``) whose calls
                are logged and cut into cycles (``cycle_records``) exactly as a device run's are; with ``fault=`` it is the
                restated recurrence in float64, where the one-line faults of ``FAULTS`` can be planted.

``D`` is the largest deviation of any ``Double`` run from ``Wide`` over ``CASES`` x cycles x orders x quantities in units
of u = 2^-53 of the quantity's scale (``deviations``): ``x`` element-wise over ``max |x*|``, ``r`` (2-norm) and ``gamma``
over ``||r*||`` at the cycle's start, ``c`` (2-norm) over 1, ``u`` element-wise over ``max |u*|``, ``beta`` and ``alpha``
relative.  A device run differs from the float64 forms in summation order and fused operations only; it is held to
``8 D``, the factor of the Lanczos filter's rotation recurrence.  ``measured_deviation`` computes it; the
committed constant is that figure rounded up (EXPERIMENTS.md has the table).

The small systems are read over fewer cycles.  On ``dense1`` / ``dense2`` the Krylov space is exhausted at step n of cycle
1 (the breakdown branch, ``h_last <= eps ||w||``, ends the inner loop and ``w`` - an exact zero - stays unnormalised):
after it ``r`` is rounding noise and there is nothing to compare, so they are read over cycle 1.  n = 63, 64, 65 are read
over ``SMALL_CYCLES = 5`` cycles (18 products; recycling and two truncations are live): at cycle 6 their float64 orders
spread to 450 u (g63, complex shift), past anything the large systems show, and would set the constant for everybody.
They keep a constant of their own, ``D_SMALL``, so that neither group passes with the other's slack.  The Jacobi cases are
read over ``JACOBI_CYCLES = 1``: on the strongly diagonally dominant g1037 the preconditioned residual falls to 1e-5
(real shift) and 4e-7 (complex) in the first cycle's five steps, so cycle 2 starts from ``r / ||r||`` with a relative
error of ``u / 1e-6`` and its ``c`` and ``u`` deviate by 1e5 .. 1e7 u between float64 orders - amplification by
convergence, which is what the step tests stay clear of.  The preconditioner enters through the product and the final
``x = M u`` only, and both are live in cycle 1.

Invariants, free of amplification (``invariants``): at the end of every cycle, from the run's OWN vectors, in longdouble:
``| ||c_i|| - 1 |``, ``|C^H C - I|``, ``||c - A u|| / (||A|| ||u||)`` (``||A||`` the infinity norm of the shifted, scaled
operator), ``||C^H r|| / ||r||`` (the ``||r||`` the cycle started from, the scale ``r`` and ``gamma`` are read in: where a
cycle exhausts the Krylov space the new ``r`` is rounding noise or an exact zero) and ``||(b - A x) - r|| / ||b||``.  Each
is held to 8 x the largest value the ``Double`` runs give (``INV``, one constant per invariant - no invariant passes with
another's slack - measured by ``measured_invariants``).

Primitive bounds (``check_call``): every call a provider receives, against longdouble on ITS OWN inputs - a local
relation, nothing is amplified, so the bounds are derived and not fitted (u = 2^-53, starred = longdouble):

real ``dot``      ``c_dot u (|x| . |y|)`` and ``nrm2`` ``(c_dot / 2 + 1) u nrm*``: ``test_gpu_subspace_kernels.py``.
pair ``dot``      ``conj(a) . b = (ar.br + ai.bi) + i (ar.bi - ai.br)``: each half is two ``hipeig_multi_dot`` results
                  (``c_rec u`` of their magnitude sums) and one add (u of the sum, itself at most the magnitude sums):
                  ``(c_rec + 1) u`` x (the sum of the two magnitude sums).
pair ``nrm2``     ``sqrt(re.re + im.im)``: two ``hipeig_dot`` of positive terms (``c_dot u`` relative each), an add (u),
                  a square root (half the relative error, one rounding): ``((c_dot + 1) / 2 + 1) u nrm*``.
``axpy``          ``hipeig_axpby`` with b = 1, ``y_i <- a x_i + y_i``: unfused ``rn(rn(a x) + y)`` errs by
                  ``u |a x| + u |a x + y| (1 + u)``, fused by ``u |a x + y|``; ``2 u (|a x_i| + |y_i|)`` covers both.
complex ``axpy``  a real-scalar update per half, then - ``alpha.imag != 0`` - a second one on its result:
                  ``2 u (|ai x'| + |t|) + (error of t)`` with ``|t| <= (1 + 2u)(|ar x| + |y|)``: two updates in sequence,
                  ``4 u (|ar x_i| + |ai x'_i| + |y_i|)`` (x' the other half of x).  A scalar with zero imaginary part: one
                  update, ``2 u``.
complex ``scaled``, ``scal``   ``rn(ar x)`` (u) then one update (2 u of its operands): within the same two-kernel
                  ``4 u (|ar x_i| + |ai x'_i|)``; ``scal`` copies that result back, exactly.
real scalar       ``scal`` / ``scaled``: one multiplication per element, bit-equal to the float64 product.
``combine``       ``c_lin = 4 (k + 1)`` of ``test_gpu_subspace_kernels.py`` with k the number of REAL inputs
                  (``_PairOps.combine`` runs ``hipeig_lincomb`` over the k' real parts followed by the k' imaginary
                  parts: k = 2 k'): ``c_lin u sum_j |c_j| |V_j[i]|``.
``copy``, ``zeros``   bit-exact.

The axpy-type bounds are worst cases of one or two roundings per element: a single correct rounding can use half of
them, so no float64 evaluation stays under a quarter; the CPU test holds the fused and the unfused form under the bound
itself there, and under a quarter for every bound that contains a reduction or a run of k terms.

``arnoldi_step`` and the operator products are held to the bounds their own tests derive
(``test_gpu_orthogonalisation._check_step``, ``_product_cases.shift_pair_bound``, ``_sweep_cases.product_bound``; the
Jacobi products add the scaling element's bound, ``_gcrot_precond_cases.diag_mul_reference``, pushed through ``|A|``).

The exits (``EXITS``) are chosen as ``_minres_steps.EXITS`` are: in ``Wide`` and in every ``Double`` order every decision
of the solve - ``beta`` against ``beta_tol`` at each cycle, the least-squares residual against the inner tolerance at each
inner step - lies a factor of 2 at least from its threshold (``exit_margin``), so device rounding cannot move the exit.
"""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _hiprec as hp
import _minres_steps as ms
from eigensolvers_amd.gcrotmk import gcrotmk_device
from eigensolvers_amd.precond_gcrotmk import jacobi_inverse_z_host
from eigensolvers_amd.precond_minres import csr_diagonal_host

U = 2.0 ** -53
EPS = float(np.finfo(np.float64).eps)
LD, CLD = hp.LD, hp.CLD
FACTOR = 8
ORDERS = ms.ORDERS
M_INNER, K_OUTER, NCYCLES, SMALL_CYCLES, JACOBI_CYCLES = 3, 2, 6, 5, 1
Z_REAL, Z_PAIR = 0.02, 0.02 + 0.05j
FLOOR = 1e-8
X0_NORM = 0.35
QUANTITIES = ("x", "r", "c", "u", "beta", "alpha", "gamma")
INVARIANTS = ("c_norm", "c_gram", "c_is_Au", "c_perp_r", "true_r")
D = 300.0                        # in u: measured_deviation over the g1037 / g20001 cases gives 293.7 (EXPERIMENTS.md)
D_SMALL = 260.0                  # in u: the same over g63, g64, g65 (5 cycles) and dense1, dense2 (1 cycle): 257.2
# in u: measured_invariants over all cases gives 2.49, 5.79, 4.41, 16.32, 16.97 (EXPERIMENTS.md)
INV = {"c_norm": 2.5, "c_gram": 5.8, "c_is_Au": 4.5, "c_perp_r": 16.5, "true_r": 17.0}
FAULTS = ("gamma_real", "gamma_unconj", "by_sign", "cx_from_Ry", "alpha_cx_only", "delete_newest", "B_from_V", "y_unscaled",
          "r_is_b", "no_final_M")
# the first cycle at which a fault changes anything on a real right-hand side with beta_1 = 1 (the CPU test asserts:
# passes before, exceeds at it).  gamma_real never does: gamma is real in exact arithmetic (the CPU test shows it).
# gamma_unconj: r is real in cycle 1, so c^T r is the conjugate of a real number there.
FIRST_ACTS = {"gamma_real": None, "gamma_unconj": 2, "by_sign": 2, "cx_from_Ry": 1, "alpha_cx_only": 1, "delete_newest": 4,
              "B_from_V": 2, "y_unscaled": 2, "r_is_b": 1, "no_final_M": None}


# ---------------------------------------------------------------- arithmetics
_stored_form = {}


def stored(op):
    """The operator as a scipy CSR matrix in its STORED entry order, private to this module: ``op.A`` is shared with other
    test modules, and a scipy call that sorts it in place (``abs``, ``sort_indices``) changes the order in which
    ``op.A @ v`` adds a row - and with it every float64 figure measured here."""
    if id(op) not in _stored_form:
        _stored_form[id(op)] = (op, sp.csr_matrix((op.val.copy(), op.col.copy(), op.rowptr.copy()), shape=(op.n, op.n)))
    return _stored_form[id(op)][1]


class Wide:
    """``longdouble`` / ``clongdouble`` throughout: the reference."""
    name = "longdouble"

    def __init__(self, cplx):
        self.cplx, self.T, self.R = cplx, (CLD if cplx else LD), LD

    @staticmethod
    def matvec(op, v):
        return hp.csr_matvec(op.rowptr, op.col, op.val, v)[0]

    @staticmethod
    def dot(x, y):
        return hp.dot(x, y)

    @staticmethod
    def nrm2(x):
        return hp.nrm2(x)

    def mgs(self, V, w):
        nb, h, na, w = hp.mgs(np.asarray(V), w, normalise=False)
        return nb, h, na, w

    def combine(self, coeffs, vecs):
        out = np.zeros(len(vecs[0]), dtype=self.T)
        for c, v in zip(coeffs, vecs):
            out = out + self.T(c) * v
        return out


class Double:
    """float64 / complex128 with the inner products (conjugated, as ``zdotc``) summed in ``order``; the product is
    scipy's; the MGS sweep and the combinations run column by column as the NumPy providers of the CPU tests do."""

    def __init__(self, order, cplx):
        assert order in ORDERS
        self.name, self.cplx = order, cplx
        self.T, self.R = (np.complex128 if cplx else np.float64), np.float64

    @staticmethod
    def matvec(op, v):
        return stored(op) @ v

    def _sum(self, t):
        if self.name == "fsum":
            return math.fsum(t.tolist())
        return float(np.sum(t))

    def dot(self, x, y):
        x, y = np.asarray(x), np.asarray(y)
        if self.name in ("dot", "reversed"):
            if self.name == "reversed":
                x, y = np.ascontiguousarray(x[::-1]), np.ascontiguousarray(y[::-1])
            d = np.vdot(x, y)
        else:
            t = np.conj(x) * y
            d = complex(self._sum(t.real), self._sum(t.imag)) if np.iscomplexobj(t) else self._sum(t)
        return self.T(d) if self.cplx else np.float64(np.real(d))

    def nrm2(self, x):
        return np.float64(math.sqrt(float(np.real(self.dot(x, x)))))

    def mgs(self, V, w):
        w = w.copy()
        nb = self.nrm2(w)
        h = np.zeros(len(V), dtype=self.T)
        for j, v in enumerate(V):
            h[j] = self.dot(v, w)
            w -= h[j] * v
        return nb, h, self.nrm2(w), w

    def combine(self, coeffs, vecs):
        out = np.zeros(len(vecs[0]), dtype=self.T)
        for c, v in zip(coeffs, vecs):
            out += c * v
        return out


# ---------------------------------------------------------------- the least-squares problem
def givens_lstsq(H, T):
    """``min_y ||e_1 - H y||`` for an upper Hessenberg ``H`` of shape (j + 2, j + 1) by Givens rotations, every operation
    in ``T``: returns ``(y, R, res)`` - the minimiser, the rotated matrix ``G H`` (upper triangular, last row zero) and
    ``|g_{j+1}|``, the residual.  A rotation is ``[[c, s], [-conj(s), c]]`` with real c."""
    H = np.array(H, dtype=T)
    rows, cols = H.shape
    g = np.zeros(rows, dtype=T)
    g[0] = 1
    for i in range(cols):
        a, b = H[i, i], H[i + 1, i]
        d = np.sqrt(abs(a) * abs(a) + abs(b) * abs(b))
        if d == 0:
            continue
        if abs(a) == 0:
            c, s = abs(a) * 0, np.conj(b) / abs(b)
        else:
            c, s = abs(a) / d, (a / abs(a)) * np.conj(b) / d
        top, bot = H[i].copy(), H[i + 1].copy()
        H[i], H[i + 1] = c * top + s * bot, -np.conj(s) * top + c * bot
        H[i + 1, i] = 0
        g[i], g[i + 1] = c * g[i] + s * g[i + 1], -np.conj(s) * g[i] + c * g[i + 1]
    y = np.zeros(cols, dtype=T)
    for i in range(cols - 1, -1, -1):
        y[i] = (g[i] - np.dot(H[i, i + 1:cols], y[i + 1:])) / H[i, i]
    return y, H, abs(g[cols])


# ---------------------------------------------------------------- the recurrence
class Run(list):
    """The per-cycle records of a run, with ``final`` (``x``, or ``M x`` with ``minv``), ``info``, ``outer``, ``products``
    (every operator application) and ``decisions`` ((kind, value / threshold, taken) of every stopping test)."""
    final = info = outer = products = None
    decisions = ()


def cycles(op, b, z, sign, m, k, ncycles, arith, x0=None, minv=None, fault=None, rtol=None, atol=0.0):
    """``ncycles`` outer cycles of GCROT(m,k) on ``sign (z I - H) x = b``, every operation in ``arith``.  ``minv``: SciPy's
    right preconditioner ``M = diag(minv)`` - the recurrence runs on ``A M`` and ``final = M x``.  ``x0``: ``r = b - A x0``.
    ``rtol`` None: no convergence test (the step tests); else SciPy's tests as ``gcrotmk.py`` makes them, ``ncycles`` being
    ``maxiter``.  ``arith``: ``Wide(cplx)`` or ``Double(order, cplx)``; ``Double`` without ``fault`` and without ``rtol``
    drives the project's generator (``run_project``).  Returns a ``Run`` of dicts ``x``, ``r``, ``c``, ``u`` (copies),
    ``beta``, ``alpha``, ``gamma``, ``inner`` (steps), ``products`` (of the cycle), ``r0`` (``||r||`` at its start)."""
    if isinstance(arith, Double) and fault is None and rtol is None:
        return run_project(op, b, z, sign, m, k, ncycles, arith, x0=x0, minv=minv)
    T, R = arith.T, arith.R
    sg, zz = R(sign), (T(z) if arith.cplx else R(np.real(z)))
    b = np.asarray(b).astype(T)
    mv = None if minv is None else np.asarray(minv).astype(T)
    run = Run()
    run.products, run.decisions = 0, []
    stopping = rtol is not None

    def A(v):
        run.products += 1
        v = v if mv is None else mv * v
        return sg * (zz * v - arith.matvec(op, v))

    def decide(kind, value, threshold):
        taken = bool(value <= threshold) if kind == "beta" else bool(value < threshold)
        run.decisions.append((kind, math.inf if threshold == 0 else float(value) / float(threshold), taken))
        return taken

    def finish(info, outer):
        run.final = x if (mv is None or fault == "no_final_M") else mv * x
        run.info, run.outer = info, outer
        return run

    with np.errstate(all="ignore"):
        if x0 is None:
            x = np.zeros(op.n, dtype=T)
            r = b.copy()
        else:
            x = np.asarray(x0).astype(T)
            r = b.copy() if fault == "r_is_b" else b - A(x)
        b_norm = arith.nrm2(b)
        if stopping:
            if not np.isfinite(b_norm):
                raise ValueError("RHS must contain only finite numbers")
            atol = max(float(atol), float(rtol) * float(b_norm))
            if b_norm == 0:
                x = b.copy()
                return finish(0, 0)
        CU = []
        for cyc in range(ncycles):
            beta = arith.nrm2(r)
            if stopping:
                beta_tol = max(atol, rtol * float(b_norm))
                if decide("beta", beta, beta_tol) and (cyc > 0 or CU):
                    r = b - A(x)
                    beta = arith.nrm2(r)
                    decide("beta", beta, beta_tol)
                if beta <= beta_tol:
                    return finish(0, 0)
            before = run.products
            ml = m + max(k - len(CU), 0)
            cs = [c for c, _ in CU]
            us = [u for _, u in CU]
            vs = [(R(1) / beta) * r]
            B = np.zeros((len(cs), ml), dtype=T)
            H = np.zeros((ml + 1, ml), dtype=T)
            for j in range(ml):
                w = A(vs[-1])
                nb, h, na, w = arith.mgs(cs + vs, w)
                if np.isfinite(R(1) / na):
                    w = (R(1) / na) * w
                if fault == "B_from_V":
                    wrong = h[len(cs):2 * len(cs)]
                    B[:len(wrong), j] = wrong
                else:
                    B[:, j] = h[:len(cs)]
                H[:j + 1, j] = h[len(cs):]
                H[j + 1, j] = na
                vs.append(w)
                breakdown = not (na > EPS * nb)
                y, Rm, res = givens_lstsq(H[:j + 2, :j + 1], T)
                if breakdown or (stopping and decide("inner", res, atol / float(beta))):
                    break
            nj = j + 1
            if fault != "y_unscaled":
                y = y * beta
            by = B[:, :nj] @ y
            ux = arith.combine(np.concatenate([y, by if fault == "by_sign" else -by]), vs[:nj] + us)
            hy = (Rm if fault == "cx_from_Ry" else H[:nj + 1, :nj]) @ y
            cx = arith.combine(hy, vs[:nj + 1])
            alpha = R(1) / arith.nrm2(cx)
            cx = alpha * cx
            if fault != "alpha_cx_only":
                ux = alpha * ux
            if fault == "gamma_unconj":
                gamma = arith.dot(np.conj(cx), r)
            else:
                gamma = arith.dot(cx, r)
            if fault == "gamma_real":
                gamma = T(np.real(gamma))
            r0 = beta
            r = r - gamma * cx
            x = x + gamma * ux
            while len(CU) >= k and CU:
                del CU[-1 if fault == "delete_newest" else 0]
            CU.append((cx, ux))
            run.append(dict(x=x.copy(), r=r.copy(), c=cx.copy(), u=ux.copy(), beta=beta, alpha=alpha, gamma=gamma,
                            inner=nj, products=run.products - before, r0=r0))
        return finish(ncycles if stopping else 0, ncycles)


# ---------------------------------------------------------------- the project's generator, logged
class HostOps:
    """The vector operations ``gcrotmk._gcrotmk`` asks of its provider, on float64 / complex128 ndarrays in ``arith``.
    Every call is logged as ``(name, inputs, result)`` with copies, as the device tests' recording proxy logs them."""

    def __init__(self, n, arith, log):
        self.n, self.arith, self.log, self.cols_per_pass = n, arith, log, 1
        if arith.cplx:
            self.dtype = np.complex128

    def new(self):
        return np.empty(self.n, dtype=self.arith.T)

    def zeros(self):
        out = np.zeros(self.n, dtype=self.arith.T)
        self.log.append(("zeros", (), out.copy()))
        return out

    def copy(self, a):
        self.log.append(("copy", (a.copy(),), a.copy()))
        return a.copy()

    def dot(self, a, b):
        d = self.arith.dot(a, b)
        d = complex(d) if self.arith.cplx else float(d)
        self.log.append(("dot", (a.copy(), b.copy()), d))
        return d

    def nrm2(self, a):
        d = float(self.arith.nrm2(a))
        self.log.append(("nrm2", (a.copy(),), d))
        return d

    def axpy(self, alpha, x, y):
        before = y.copy()
        y += self.arith.T(alpha) * x
        self.log.append(("axpy", (alpha, x.copy(), before), y.copy()))

    def scal(self, alpha, x):
        before = x.copy()
        x *= self.arith.T(alpha)
        self.log.append(("scal", (alpha, before), x.copy()))

    def scaled(self, alpha, x):
        out = self.arith.T(alpha) * x
        self.log.append(("scaled", (alpha, x.copy()), out.copy()))
        return out

    def arnoldi_step(self, vs, w):
        before = w.copy()
        nb, h, na, out = self.arith.mgs(vs, w)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / na
        w[:] = out * inv if np.isfinite(inv) else out
        self.log.append(("arnoldi_step", ([v.copy() for v in vs], before), (float(nb), h.copy(), float(na), w.copy())))
        return float(nb), h, float(na)

    def combine(self, coeffs, vecs):
        out = self.arith.combine(coeffs, vecs)
        self.log.append(("combine", (np.array(coeffs), [v.copy() for v in vecs]), out.copy()))
        return out


def cycle_records(log):
    """Cut the call log of one solve into per-cycle records (the keys ``cycles`` returns).  ``_gcrotmk`` calls ``dot``
    once per cycle, for ``gamma = <c, r>``; the two ``axpy`` after it update ``r`` and ``x``; the ``nrm2`` before the
    cycle's ``scaled`` is ``beta``, the one after its two ``combine`` is ``1 / alpha``.  ``("mv", ...)`` entries are the
    operator applications."""
    out, inner, products = Run(), 0, 0
    beta = last_nrm2 = pending = None
    for name, ins, res in log:
        if name == "mv":
            products += 1
        elif name == "nrm2":
            last_nrm2 = res
        elif name == "scaled":
            beta, inner, products = last_nrm2, 0, 0
        elif name == "arnoldi_step":
            inner += 1
        elif name == "dot":
            pending = dict(c=ins[0], gamma=res, beta=beta, alpha=1 / last_nrm2, inner=inner, products=products, r0=beta)
        elif name == "axpy" and pending is not None:
            if "r" not in pending:
                pending["r"] = res
            else:
                pending["u"], pending["x"] = ins[1], res
                out.append(pending)
                pending = None
    return out


def shifted(op, z, sign, minv=None):
    """``v -> sign (z v - H v)`` on float64 / complex128 arrays (``minv``: applied to ``v`` first)."""
    A = stored(op)

    def mv(v):
        v = v if minv is None else minv * v
        return sign * (z * v - A @ v)
    return mv


def run_project(op, b, z, sign, m, k, ncycles, arith, x0=None, minv=None, rtol=0.0, atol=0.0):
    """``gcrotmk_device`` (the project's generator and driver) on the host provider in ``arith``: the ``Run`` its log gives,
    with ``info``, ``outer`` (``stats["outer"]``), ``products`` (``stats["matvecs"]``), ``final`` and ``log``.  The real
    path is driven with ``complex_pairs=True`` too: the flag only chooses ``ops.zeros()`` for ``x = 0`` where the real
    device path fills a buffer through the library; the provider's ``dtype`` decides the arithmetic."""
    log = []
    T = arith.T
    zz = T(z) if arith.cplx else np.float64(np.real(z))
    mvec = None if minv is None else np.asarray(minv).astype(T)
    apply = shifted(op, zz, np.float64(sign), mvec)

    def matvec(v):
        out = apply(v)
        log.append(("mv", (v.copy(),), out.copy()))
        return out

    ops = HostOps(op.n, arith, log)
    x, info, stats = gcrotmk_device(None, matvec, np.asarray(b).astype(T), op.n, rtol=rtol, atol=atol, maxiter=ncycles, m=m, k=k,
                                    complex_pairs=True, x0=None if x0 is None else np.asarray(x0).astype(T), ops=ops)
    run = cycle_records(log)
    run.info, run.outer, run.products, run.log = info, stats["outer"], stats["matvecs"], log
    run.final = x if mvec is None else mvec * x
    return run


# ---------------------------------------------------------------- deviations and invariants
def _w(a):
    a = np.asarray(a)
    return a.astype(CLD if np.iscomplexobj(a) else LD)


def deviations(got, ref):
    """``{quantity: deviation in u}`` of one cycle's record against the reference's (the scales of the module docstring);
    ``inf`` where ``got`` is not finite."""
    out = {}
    scale = {"x": np.max(np.abs(_w(ref["x"]))), "u": np.max(np.abs(_w(ref["u"]))), "r": LD(ref["r0"]), "gamma": LD(ref["r0"]),
             "c": LD(1), "beta": abs(LD(ref["beta"])), "alpha": abs(LD(ref["alpha"]))}
    for q in QUANTITIES:
        g, r = _w(got[q]), _w(ref[q])
        if not np.all(np.isfinite(g)):
            out[q] = float("inf")
        elif q in ("x", "u"):
            out[q] = float(np.max(np.abs(g - r)) / scale[q]) / U
        elif q in ("r", "c"):
            out[q] = float(hp.nrm2(g - r) / scale[q]) / U
        else:
            out[q] = float(abs(g - r) / scale[q]) / U
    return out


def operator_norm(op, z, minv=None):
    """The infinity norm of ``(z I - H) diag(minv)``, bounded by ``(|z| + ||H||_inf) max |minv|``: a scale, not a figure."""
    rows = np.repeat(np.arange(op.n), np.diff(op.rowptr))     # from the arrays: abs(op.A) would sort the shared matrix in place
    h = float(np.bincount(rows, weights=np.abs(op.val), minlength=op.n).max())
    return (abs(complex(z)) + h) * (1.0 if minv is None else float(np.max(np.abs(minv))))


def invariants(run, op, b, z, sign, k, minv=None):
    """Per cycle ``{invariant: value in u}`` from the run's own vectors, evaluated in longdouble (module docstring)."""
    cplx = any(np.iscomplexobj(rec["x"]) for rec in run)
    wide = Wide(cplx)
    zz = CLD(z) if cplx else LD(np.real(z))
    mvw = None if minv is None else _w(minv)
    bw = _w(b)
    anorm = LD(operator_norm(op, z, minv))

    def A(v):
        v = _w(v) if mvw is None else mvw * _w(v)
        return LD(sign) * (zz * v - wide.matvec(op, v))

    out, CU = [], []
    for rec in run:
        while len(CU) >= k and CU:
            del CU[0]
        CU.append(_w(rec["c"]))
        c, u, r, x = _w(rec["c"]), _w(rec["u"]), _w(rec["r"]), _w(rec["x"])
        G = np.array([[hp.dot(a, d) for d in CU] for a in CU])
        inv = {"c_norm": max(abs(hp.nrm2(a) - 1) for a in CU),
               "c_gram": np.max(np.abs(G - np.eye(len(CU)))),
               "c_is_Au": hp.nrm2(c - A(u)) / (anorm * hp.nrm2(u)),
               "c_perp_r": np.sqrt(sum(abs(hp.dot(a, r)) ** 2 for a in CU)) / LD(rec["r0"]),
               "true_r": hp.nrm2((bw - A(x)) - r) / hp.nrm2(bw)}
        out.append({q: float(v) / U for q, v in inv.items()})
    return out


# ---------------------------------------------------------------- the case table
class Case:
    """Operator, right-hand side, shift, sign and - where used - ``minv`` / ``x0`` of one run of ``ncycles`` cycles."""

    def __init__(self, name, opname, z=Z_REAL, sign=1.0, ncycles=NCYCLES, jacobi=False, x0=False, small=False):
        self.name, self.opname, self.z, self.sign, self.ncycles = name, opname, z, sign, ncycles
        self.jacobi, self.with_x0, self.small = jacobi, x0, small
        self.pair = isinstance(z, complex)

    @property
    def op(self):
        return ms.operator(self.opname)

    @property
    def b(self):
        return ms.rhs(self.op.n, ms.SMALL_SEEDS.get(self.op.n))

    @property
    def minv(self):
        """The host statement of ``hipeig_jacobi_inverse_z`` (the device test hands the device's own to the reference)."""
        return jacobi_inverse_z_host(csr_diagonal_host(stored(self.op)), self.z, FLOOR) if self.jacobi else None

    @property
    def x0(self):
        if not self.with_x0:
            return None
        n = self.op.n
        rng = np.random.default_rng([13, n])
        g = rng.standard_normal(n) + (1j * rng.standard_normal(n) if self.pair else 0.0)
        return g * (X0_NORM / np.linalg.norm(g))

    @property
    def bound(self):
        return FACTOR * (D_SMALL if self.small else D)


def _cases():
    out = []
    for z, tag in ((Z_REAL, "real"), (Z_PAIR, "pair")):
        for sign in (1.0, -1.0):
            out.append(Case(f"g1037 {tag} sign={sign:+.0f}", "g1037", z, sign))
        out.append(Case(f"g20001 {tag}", "g20001", z))
        out.append(Case(f"g1037 {tag} x0", "g1037", z, x0=True))
        out.append(Case(f"g1037 {tag} jacobi", "g1037", z, ncycles=JACOBI_CYCLES, jacobi=True))
        for n in (63, 64, 65):
            out.append(Case(f"g{n} {tag}", f"g{n}", z, ncycles=SMALL_CYCLES, small=True))
        for n in (1, 2):
            out.append(Case(f"dense{n} {tag}", f"dense{n}", z, ncycles=1, small=True))
    return {c.name: c for c in out}


CASES = _cases()
_refs = {}


def reference(case, minv=None, fault=None):
    """The ``Wide`` run of a case, computed once and left unchanged.  ``minv``: the device's own inverse diagonal in place
    of the host statement's (keyed by its bytes)."""
    if not hp.EXTENDED:
        raise RuntimeError("longdouble is no wider than double here")
    key = (case.name, None if minv is None else np.asarray(minv).tobytes())
    if key not in _refs:
        run = cycles(case.op, case.b, case.z, case.sign, M_INNER, K_OUTER, case.ncycles, Wide(case.pair), x0=case.x0,
                     minv=case.minv if minv is None else minv)
        for rec in run:
            for q in ("x", "r", "c", "u"):
                rec[q].setflags(write=False)
        _refs[key] = run
    return _refs[key]


def run_double(case, order="dot", fault=None):
    return cycles(case.op, case.b, case.z, case.sign, M_INNER, K_OUTER, case.ncycles, Double(order, case.pair), x0=case.x0,
                  minv=case.minv, fault=fault)


def final_deviation(got, ref):
    """``final`` (``x``, ``M x`` with a preconditioner) element-wise over ``max |final*|``, in u."""
    g, r = _w(got), _w(ref)
    return float(np.max(np.abs(g - r)) / np.max(np.abs(r))) / U if np.all(np.isfinite(g)) else float("inf")


def measured_deviation(small):
    """``(D, table)`` over the large (``small`` False) or the small cases: the largest deviation of any float64 order from
    the ``longdouble`` run; ``table[(case, cycle, order)]`` = (largest deviation, its quantity)."""
    table = {}
    for case in CASES.values():
        if case.small != small:
            continue
        ref = reference(case)
        for order in ORDERS:
            run = run_double(case, order)
            assert len(run) == len(ref)
            for cyc, (g, r) in enumerate(zip(run, ref), start=1):
                dev = deviations(g, r)
                q = max(dev, key=dev.get)
                table[(case.name, cyc, order)] = (dev[q], q)
            table[(case.name, "final", order)] = (final_deviation(run.final, ref.final), "final")
    return max(v[0] for v in table.values()), table


def measured_invariants():
    """``({invariant: largest value in u}, table)`` over all cases, cycles and float64 orders;
    ``table[(case, order)]`` = {invariant: largest over the cycles}."""
    table = {}
    for case in CASES.values():
        for order in ORDERS:
            inv = case_invariants(case, run_double(case, order))
            table[(case.name, order)] = {q: max(rec[q] for rec in inv) for q in INVARIANTS}
    return {q: max(t[q] for t in table.values()) for q in INVARIANTS}, table


def case_invariants(case, run, minv=None):
    return invariants(run, case.op, case.b, case.z, case.sign, K_OUTER, case.minv if minv is None else minv)


def invariant_excess(inv):
    """The largest ``value / (8 INV)`` over the cycles' invariants, with its name and cycle: ``(ratio, name, cycle)``."""
    worst = (0.0, None, None)
    for cyc, rec in enumerate(inv, start=1):
        for q in INVARIANTS:
            ratio = rec[q] / (FACTOR * INV[q])
            if ratio > worst[0]:
                worst = (ratio, q, cyc)
    return worst


# ---------------------------------------------------------------- the primitives against longdouble on their own inputs
def grids(n, cus):
    """``(c_dot, c_rec)`` of ``test_gpu_subspace_kernels.py`` at length n on a device of ``cus`` compute units."""
    import test_gpu_subspace_kernels as sk
    G = sk._grid_records(n, cus)
    return sk.c_dot(n, G), sk.c_rec(n, G)


def _ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    bound = np.broadcast_to(bound, err.shape)
    if not np.all(np.isfinite(err)):
        return float("inf")
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if err.size else 0.0


def _halves(a):
    a = np.asarray(a)
    return (np.ascontiguousarray(a.real, dtype=np.float64), np.ascontiguousarray(a.imag, dtype=np.float64) if np.iscomplexobj(a) else None)


def _err(got, ref):
    return np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref).astype(np.float64)


def _mag(x, y):
    return float(hp.dot(np.abs(x), np.abs(y)))


def _axpy_half(a1, x1, a2, x2, y):
    """One half of a (complex) axpy / scaled: ``a1 x1 + a2 x2 + y`` in longdouble and the magnitudes' sum.  ``y`` None: 0."""
    ref = LD(a1) * x1.astype(LD)
    mag = np.abs(ref)
    if a2 is not None:
        t = LD(a2) * x2.astype(LD)
        ref, mag = ref + t, mag + np.abs(t)
    if y is not None:
        ref, mag = ref + y.astype(LD), mag + np.abs(y.astype(LD))
    return ref, mag.astype(np.float64)


def check_call(name, ins, res, pair, cdot, crec):
    """``{label: error / bound}`` of one logged provider call (``(name, ins, res)`` as ``HostOps`` and the device proxy log
    them; complex vectors as complex128 arrays) against longdouble on its own inputs.  ``cdot``, ``crec``: ``grids(n, cus)``.
    A ratio above 1 is a failure; the bit-exact relations give 0 or inf.  ``arnoldi_step`` and ``mv`` are not handled here."""
    out = {}
    if name in ("copy", "zeros"):
        want = ins[0] if name == "copy" else np.zeros_like(res)
        out[name] = 0.0 if np.asarray(res).tobytes() == np.asarray(want).tobytes() else float("inf")
    elif name == "dot":
        a, b = ins
        if not pair:
            out["dot"] = _ratio(abs(LD(res) - hp.dot(a, b)), cdot * U * _mag(a, b))
        else:
            (ar, ai), (br, bi) = _halves(a), _halves(b)
            ref = hp.dot(a, b)
            out["pair dot re"] = _ratio(abs(LD(res.real) - ref.real), (crec + 1) * U * (_mag(ar, br) + _mag(ai, bi)))
            out["pair dot im"] = _ratio(abs(LD(res.imag) - ref.imag), (crec + 1) * U * (_mag(ar, bi) + _mag(ai, br)))
    elif name == "nrm2":
        ref = hp.nrm2(ins[0])
        c = ((cdot + 1) / 2 + 1) if pair else (cdot / 2 + 1)
        out["pair nrm2" if pair else "nrm2"] = _ratio(abs(LD(res) - ref), c * U * float(ref))
    elif name == "axpy":
        alpha, x, y = ins
        alpha = complex(alpha)
        (xr, xi), (yr, yi), (gr, gi) = _halves(x), _halves(y), _halves(res)
        if not pair:
            ref, mag = _axpy_half(alpha.real, xr, None, None, yr)
            out["axpy"] = _ratio(_err(gr, ref), 2 * U * mag)
        elif alpha.imag == 0.0:
            for tag, xh, yh, gh in (("re", xr, yr, gr), ("im", xi, yi, gi)):
                ref, mag = _axpy_half(alpha.real, xh, None, None, yh)
                out[f"pair axpy real scalar {tag}"] = _ratio(_err(gh, ref), 2 * U * mag)
        else:
            ref, mag = _axpy_half(alpha.real, xr, -alpha.imag, xi, yr)
            out["pair axpy re"] = _ratio(_err(gr, ref), 4 * U * mag)
            ref, mag = _axpy_half(alpha.real, xi, alpha.imag, xr, yi)
            out["pair axpy im"] = _ratio(_err(gi, ref), 4 * U * mag)
    elif name in ("scal", "scaled"):
        alpha, x = ins
        alpha = complex(alpha)
        (xr, xi), (gr, gi) = _halves(x), _halves(res)
        if alpha.imag == 0.0:
            same = np.array_equal(gr, alpha.real * xr) and (xi is None or np.array_equal(gi, alpha.real * xi))
            out[f"{name} real scalar"] = 0.0 if same else float("inf")
        else:
            ref, mag = _axpy_half(alpha.real, xr, -alpha.imag, xi, None)
            out[f"pair {name} re"] = _ratio(_err(gr, ref), 4 * U * mag)
            ref, mag = _axpy_half(alpha.real, xi, alpha.imag, xr, None)
            out[f"pair {name} im"] = _ratio(_err(gi, ref), 4 * U * mag)
    elif name == "combine":
        import test_gpu_subspace_kernels as sk
        coeffs, vecs = ins
        cf = np.asarray(coeffs)
        gr, gi = _halves(res)
        if not pair:
            Y, Yabs = hp.combine(np.array(vecs, dtype=np.float64), np.asarray(cf.real, dtype=np.float64)[:, None])
            out["combine"] = _ratio(_err(gr, Y[:, 0]), sk.c_lin(len(vecs)) * U * Yabs[:, 0].astype(np.float64))
        else:
            parts = np.array([np.real(v) for v in vecs] + [np.imag(v) for v in vecs], dtype=np.float64)
            C2 = np.stack([np.concatenate([cf.real, -cf.imag]), np.concatenate([cf.imag, cf.real])], axis=1)
            Y, Yabs = hp.combine(parts, C2)
            c = sk.c_lin(2 * len(vecs))
            out["pair combine re"] = _ratio(_err(gr, Y[:, 0]), c * U * Yabs[:, 0].astype(np.float64))
            out["pair combine im"] = _ratio(_err(gi, Y[:, 1]), c * U * Yabs[:, 1].astype(np.float64))
    else:
        raise KeyError(name)
    return out


def check_log(log, pair, cdot, crec):
    """``{label: (largest error / bound, index of the call)}`` over the provider calls of a log ``check_call`` handles."""
    worst = {}
    for i, (name, ins, res) in enumerate(log):
        if name in ("mv", "arnoldi_step"):
            continue
        for label, r in check_call(name, ins, res, pair, cdot, crec).items():
            if r >= worst.get(label, (-1.0, None))[0]:
                worst[label] = (r, i)
    return worst


# ---------------------------------------------------------------- primitives outside a solve
LENGTHS = (1, 2, 3, 63, 64, 65, 1037)
SCALARS = (0.0, 1.5, complex(-0.3, 0.0), 0.7 - 1.9j, 1e-3 + 1e2j)
COMBINE_COUNTS = (1, 2, 8, 9, 17, 31)


def vectors(n, count, seed=21):
    """``count`` complex vectors of length n whose halves span orders of magnitude element by element and vector by vector
    (no two interchangeable): complex128 rows."""
    rng = np.random.default_rng([seed, n, count])
    V = rng.standard_normal((count, 2, n)) * np.exp(rng.uniform(-2, 2, (count, 2, n))) * 2.0 ** rng.integers(-6, 5, (count, 1, 1))
    return V[:, 0] + 1j * V[:, 1]


def coefficients(count, seed=22):
    rng = np.random.default_rng([seed, count])
    return (rng.standard_normal(count) + 1j * rng.standard_normal(count)) * 2.0 ** rng.integers(-3, 4, count)


# ---------------------------------------------------------------- exits
class Exit:
    """A solve with SciPy's stopping tests on: operator (an ``ms.Operator``), ``b``, ``z``, ``sign``, ``rtol``, ``atol``,
    ``maxiter``, ``x0``; ``raises``: the exception the solve must raise instead of returning."""

    def __init__(self, name, op, b, z=Z_REAL, sign=1.0, rtol=1e-8, atol=0.0, maxiter=20, x0=None, raises=None):
        self.name, self.op, self.b, self.z, self.sign = name, op, np.asarray(b, dtype=np.float64), z, sign
        self.rtol, self.atol, self.maxiter, self.x0, self.raises = rtol, atol, maxiter, x0, raises
        self.pair = isinstance(z, complex)

    def run(self, arith):
        return cycles(self.op, self.b, self.z, self.sign, M_INNER, K_OUTER, self.maxiter, arith, x0=self.x0,
                      rtol=self.rtol, atol=self.atol)

    def project(self, arith):
        return run_project(self.op, self.b, self.z, self.sign, M_INNER, K_OUTER, self.maxiter, arith, x0=self.x0,
                           rtol=self.rtol, atol=self.atol)


def exit_margin(run):
    """The least factor by which any decision of the run is away from its threshold (``inf`` with none)."""
    out = math.inf
    for kind, ratio, taken in run.decisions:
        if ratio == 0 or not math.isfinite(ratio):
            continue
        out = min(out, 1.0 / ratio if taken else ratio)
    return out


# On g1037 the least-squares residual falls by less than a factor of 2 a step (z = 0.02 lies next to a cluster), so no
# tolerance has a margin of 2 on both sides of a step there.  On a diagonal operator with its spectrum spread over [1, 2]
# (condition 2 after the shift) it falls by 5 to 6 a step, and this tolerance is passed at step 3 of cycle 3, a factor
# of 2 at least from the residuals on either side (the CPU test asserts it).
SPREAD = ms.Operator(sp.diags(np.linspace(1.0, 2.0, 1037)).tocsr())
CONVERGES_RTOL = 4e-9


def _exact_x0(op, z, sign, b):
    n = op.n
    A = sp.csc_matrix(sign * (z * sp.identity(n) - stored(op)))
    return spla.spsolve(A, b.astype(A.dtype))


def _exits():
    g = ms.operator("g1037")
    b = ms.rhs(1037)
    H64 = ms.Operator(sp.diags(np.linspace(-1.0, 1.0, 64) + 0.3).tocsr())
    e3 = np.zeros(64)
    e3[3] = 2.0
    nonfinite = b.copy()
    nonfinite[5] = np.inf
    out = []
    for z, tag in ((Z_REAL, "real"), (Z_PAIR, "pair")):
        out += [Exit(f"converges in cycle 3 {tag}", SPREAD, b, z, rtol=CONVERGES_RTOL),
                Exit(f"maxiter {tag}", g, b, z, rtol=1e-12, maxiter=2),
                Exit(f"zero rhs {tag}", g, np.zeros(1037), z),
                Exit(f"eigenvector {tag}", H64, e3, z, rtol=1e-10),
                Exit(f"exact x0 {tag}", g, b, z, x0=_exact_x0(g, z, 1.0, b)),
                Exit(f"non-finite rhs {tag}", g, nonfinite, z, raises=ValueError)]
    return {e.name: e for e in out}


EXITS = _exits()
