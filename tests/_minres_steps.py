"""The first steps and the rare exits of MINRES against extended precision: reference, deviation measure and cases
(``test_minres_steps_cpu.py``, ``test_gpu_minres_steps.py``).  A plain module, imported as ``_hiprec`` is: no fixtures, no
tests.

A MINRES run amplifies rounding as it converges, so a device run cannot be held to a reference run to the end.  Its first
``K = 4`` steps can: on a well-conditioned system nothing has been amplified yet, and by step 4 every term of the
recurrence is live - ``use_r1`` from step 2, ``oldeps`` from step 3, the R and W rings (period 3) and the Z ring (period 2)
have wrapped.  ``steps`` is SciPy 1.15.3's recurrence in the order of ``oracle/minres_ref.py`` for ``sign (sigma I - H)``,
written once and run in two arithmetics: ``Wide`` (``longdouble``, products and sums through ``_hiprec``) is the reference,
``Double(order)`` (float64 with a chosen summation order of the inner products) measures what a correct float64 evaluation
deviates by.  ``D`` is the largest such deviation over ``CASES``, steps 1 .. K, every order, the iterate and the five
scalar statistics, in units of u = 2^-53 (``measured_deviation``; EXPERIMENTS.md holds the table).  A device run differs from
the float64 forms in summation order and fused operations only, each of which moves a sum by no more than the orders
measured do; it is held to ``8 D``, the factor of the Lanczos filter's rotation recurrence.

``fault`` plants the one-line faults the CPU test must see exceed ``8 D`` (``FAULTS``).

The row-partitioned solves (``test_gpu_partitioned_steps.py``) are read further: they enqueue chunks of 16 iterations with
no flush between two chunks, so what can go wrong there - a pending iterate update lost at a boundary, a share of ``<y,y>``
missing at one step - does not exist within four steps.  On the well-conditioned g1037 / g20001 systems the ``longdouble``
run can still be held at ``LONG_STEPS``: 16 ends at a chunk boundary, 17 and 18 carry one pending update across it, 32 ends
at the second boundary, 33 crosses two.  ``D_LONG`` is ``D``'s definition over ``LONG_CASES`` x ``LONG_STEPS``, with the
orders joined by ``Double("slabs", P)`` - the sum in rank order of the ranks' own sums, as the loopback all-reduce adds; a
device run is held to ``8 D_LONG`` there, by the reasoning of ``8 D``.  The small systems (n = 63, 64, 65) nearly exhaust
their Krylov space by step 34 (the orders disagree by 5e3 .. 1e6 u): they are read over K steps only.  ``LONG_FAULTS`` are
the faults of that path; two of them pass at steps 1 .. 4, which is why four steps are not enough.

The exit cases (``EXITS``) are operators on which the oracle stops with the rare codes by a factor of 2 at least
(``exit_margin``), so that device rounding cannot move the step.
"""
import math

import numpy as np
import scipy.sparse as sp

import _hiprec as hp
from eigensolvers_amd.distributed import row_range
from eigensolvers_amd.generators import gapped_csr_host
from eigensolvers_amd.precond_minres import csr_diagonal_host, jacobi_inverse_host

U = 2.0 ** -53
EPS = float(np.finfo(np.float64).eps)
LD = hp.LD
K = 4
STATS = ("rnorm", "Anorm", "ynorm", "test1", "test2", "Acond")
D = 13.0                         # in u: measured_deviation over CASES gives 12.84 (EXPERIMENTS.md); the condition on the table is D <= 16
FACTOR = 8
ORDERS = ("dot", "pairwise", "reversed", "fsum")
K_FAULTS = ("swap_w", "c1_inverted", "kc_tail", "phi_old", "alfa_f32", "dbar_sign", "z_prev", "ynorm_no_x0")
LONG_FAULTS = ("ynorm_lagged", "kd_dropped_at_16", "yy_share_missing")     # of the row-partitioned path, seen at LONG_STEPS
FAULTS = K_FAULTS + LONG_FAULTS
LONG_STEPS = (1, 2, 3, 4, 16, 17, 18, 32, 33)
LONG_ORDERS = ORDERS + (("slabs", 2), ("slabs", 3))
D_LONG = 23.0                   # in u: measured_long_deviation gives 22.83 (EXPERIMENTS.md); the condition on the table is D_LONG <= 32


# ---------------------------------------------------------------- operators
class Operator:
    """A host CSR matrix: the arrays ``hp.csr_matvec`` takes and the scipy matrix the float64 forms multiply with."""

    def __init__(self, A):
        A = sp.csr_matrix(A)
        self.n = A.shape[0]
        self.rowptr, self.col, self.val = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64)
        self.A = A


def _dense(n):
    """Small dense symmetric operators for n = 1, 2: entries that are no powers of two, sigma = 0.02 well off the spectrum."""
    M = np.array([[0.7, -0.3], [-0.3, -1.1]])[:n, :n]
    return sp.csr_matrix(M)


_operators = {}


def operator(name):
    """``"g<n>"``: ``gapped_csr_host(n, 16, seed=7)``; ``"dense<n>"``: the small dense ones."""
    if name not in _operators:
        if name.startswith("dense"):
            A = _dense(int(name[5:]))
        else:
            A = gapped_csr_host(int(name[1:]), 16, seed=7)
        _operators[name] = Operator(A)
    return _operators[name]


# ---------------------------------------------------------------- arithmetics
class Wide:
    """``longdouble`` throughout: the reference."""
    name = "longdouble"
    real = LD

    @staticmethod
    def matvec(op, v):
        return hp.csr_matvec(op.rowptr, op.col, op.val, v)[0]

    @staticmethod
    def dot(x, y):
        return hp.dot(x, y)


class Double:
    """float64 with the inner products summed in ``order``; the product is scipy's (a row's terms in stored order).
    ``Double("slabs", P)``: the sum, in rank order, of ``np.dot`` over the ``row_range`` slabs of P ranks."""
    real = np.float64

    def __init__(self, order="dot", P=None):
        assert order in ORDERS or (order == "slabs" and P >= 1)
        self.name, self.P = order, P

    @staticmethod
    def matvec(op, v):
        return op.A @ v

    def dot(self, x, y):
        if self.name == "slabs":
            acc = np.float64(0.0)
            for r in range(self.P):
                lo, hi = row_range(len(x), self.P, r)
                acc = acc + np.float64(np.dot(x[lo:hi], y[lo:hi]))
            return acc
        if self.name == "dot":
            return np.float64(np.dot(x, y))
        if self.name == "pairwise":
            return np.float64(np.sum(x * y))
        if self.name == "reversed":
            return np.float64(np.dot(np.ascontiguousarray(x[::-1]), np.ascontiguousarray(y[::-1])))
        return np.float64(math.fsum((x * y).tolist()))


# ---------------------------------------------------------------- the recurrence
def steps(op, b, sigma, sign, nsteps, arith, minv=None, x0=None, fault=None):
    """``nsteps`` iterations of SciPy's MINRES on ``sign (sigma I - H) x = b`` with no stopping test, every operation in
    ``arith.real``.  ``minv``: SciPy's ``M`` as the diagonal of its inverse (``z = minv (.) r2``, ``beta^2 = <r2, z>``).
    ``x0``: ``r1 = b - A x0``, the iterate and ``ynorm`` start from it.  Returns one dict per step: ``x`` (a copy), ``alfa``,
    ``beta`` (``beta_{k+1}``) and the six statistics."""
    T = arith.real
    one = T(1)
    sg, sm = T(sign), T(sigma)
    b = np.asarray(b, dtype=np.float64).astype(T)
    mv = None if minv is None else np.asarray(minv, dtype=np.float64).astype(T)

    def A(v):
        return sg * (sm * v - arith.matvec(op, v))

    def sqrt(v):
        return np.sqrt(T(v))

    out = []
    with np.errstate(all="ignore"):
        if x0 is None:
            x = np.zeros(op.n, dtype=T)
            r1 = b.copy()
        else:
            x = np.asarray(x0, dtype=np.float64).astype(T)
            r1 = b - A(x)
        xstart = x.copy()
        y = r1 if mv is None else mv * r1
        beta1 = sqrt(arith.dot(r1, y))
        oldb, beta, dbar, epsln, phibar, tnorm2 = T(0), beta1, T(0), T(0), beta1, T(0)
        gmax, gmin = T(0), T(np.finfo(np.float64).max)
        cs, sn = T(-1), T(0)
        w = np.zeros(op.n, dtype=T)
        w2 = np.zeros(op.n, dtype=T)
        r2 = r1
        z = y
        for itn in range(1, nsteps + 1):
            s = one / beta
            v = s * z
            y = A(v)
            if itn >= 2:
                y = y - ((oldb / beta) if fault == "c1_inverted" else (beta / oldb)) * r1
            alfa = T(arith.dot(v, y))
            if fault == "alfa_f32":
                alfa = T(np.float32(alfa))
            yn = y - (alfa / beta) * r2
            if fault == "kc_tail" and op.n & 1:
                yn[-1] = y[-1]
            r1 = r2
            r2 = yn
            zprev = z
            z = r2 if mv is None else mv * r2
            oldb = beta
            if fault == "yy_share_missing" and itn == 17:              # the third of three slabs never arrived
                cut = row_range(op.n, 3, 1)[1]
                beta = sqrt(arith.dot(r2[:cut], z[:cut]))
            else:
                beta = sqrt(abs(arith.dot(r2, zprev))) if fault == "z_prev" else sqrt(arith.dot(r2, z))
            tnorm2 = tnorm2 + (alfa * alfa + oldb * oldb + beta * beta)

            oldeps = epsln
            delta = cs * dbar + sn * alfa
            gbar = sn * dbar - cs * alfa
            epsln = sn * beta
            dbar = cs * beta if fault == "dbar_sign" else -cs * beta
            root = sqrt(gbar * gbar + dbar * dbar)

            gamma = max(sqrt(gbar * gbar + beta * beta), T(EPS))
            cs_old = cs
            cs = gbar / gamma
            sn = beta / gamma
            phi = (cs_old if fault == "phi_old" else cs) * phibar
            phibar = sn * phibar

            denom = one / gamma
            w1 = w2
            w2 = w
            if fault == "swap_w":
                w = (v - oldeps * w2 - delta * w1) * denom
            else:
                w = (v - oldeps * w1 - delta * w2) * denom
            xlag = x
            if not (fault == "kd_dropped_at_16" and itn == 16):
                x = x + phi * w

            gmax = max(gmax, gamma)
            gmin = min(gmin, gamma)

            Anorm = sqrt(tnorm2)
            xn = (x - xstart) if fault == "ynorm_no_x0" else xlag if fault == "ynorm_lagged" else x
            ynorm = sqrt(arith.dot(xn, xn))
            rnorm = phibar
            out.append(dict(x=x.copy(), alfa=alfa, beta=beta, rnorm=rnorm, Anorm=Anorm, ynorm=ynorm,
                            test1=rnorm / (Anorm * ynorm), test2=root / Anorm, Acond=gmax / gmin))
    return out


# ---------------------------------------------------------------- the deviation measure
def deviation(got, ref):
    """In units of u, the difference taken in ``longdouble``: ``||got - ref||_2 / ||ref||_2`` for vectors,
    ``|got - ref| / |ref|`` for scalars; ``inf`` for a non-finite ``got``."""
    g = np.asarray(got).astype(LD)
    r = np.asarray(ref).astype(LD)
    if not np.all(np.isfinite(g)):
        return float("inf")
    if g.ndim:
        return float(hp.nrm2(g - r) / hp.nrm2(r)) / U
    return float(abs(g - r) / abs(r)) / U


def step_deviations(got, ref, stats=STATS, scales=None):
    """``{"x": .., stat: ..}`` of one step's record ``got`` (a dict as ``steps`` returns, float64 or wider) against the
    reference's record ``ref``.  ``scales[stat]``: that statistic is 0 in exact arithmetic at this step
    (``Case.scales``), so its error is taken relative to the given scale instead of its own value."""
    out = {"x": deviation(got["x"], ref["x"])}
    for q in stats:
        if scales and q in scales:
            g = LD(got[q])
            out[q] = float(abs(g - LD(ref[q])) / LD(scales[q])) / U if np.isfinite(g) else float("inf")
        else:
            out[q] = deviation(got[q], ref[q])
    return out


# ---------------------------------------------------------------- the case table
class Case:
    """Operator, right-hand side, shift, sign and - where used - ``minv`` / ``x0`` of one run of K (or n, if smaller) steps."""

    def __init__(self, name, opname, sigma=0.02, sign=1.0, seed=None, norm=1.0, jacobi=False, x0=False):
        self.name, self.opname, self.sigma, self.sign = name, opname, sigma, sign
        self.seed, self.norm, self.jacobi, self.with_x0 = seed, norm, jacobi, x0

    @property
    def op(self):
        return operator(self.opname)

    @property
    def nsteps(self):
        return min(K, self.op.n)

    @property
    def b(self):
        return rhs(self.op.n, self.seed) * self.norm

    def scales(self, k, ref):
        """Step ``k == n`` of an n-dimensional system ends the Krylov space: ``beta_{n+1}`` and with it ``rnorm`` and
        ``test1`` are 0 in exact arithmetic and pure rounding in any other, so the two are held to ``8 D u`` of the scale
        they fell from - ``beta1`` and ``beta1 / (Anorm ynorm)`` - not of their own value.  ``ref``: the reference's
        records.  ``None`` at every other step."""
        if k != self.op.n:
            return None
        beta1 = hp.nrm2(self.b)
        return {"rnorm": beta1, "test1": beta1 / (LD(ref[k - 1]["Anorm"]) * LD(ref[k - 1]["ynorm"]))}

    @property
    def minv(self):
        """The host statement of ``hipeig_jacobi_inverse`` (the device test hands the device's own to the reference)."""
        return jacobi_inverse_host(csr_diagonal_host(self.op.A), self.sigma) if self.jacobi else None

    @property
    def x0(self):
        if not self.with_x0:
            return None
        n = self.op.n
        g = np.random.default_rng([11, n]).standard_normal(n)
        return g * (X0_NORM / np.linalg.norm(g))


X0_NORM = 0.35        # ||x_4|| of the g1037 / g20001 cases is 0.2 .. 0.5: a guess of comparable norm
NCOLS = 11
# Right-hand sides are chosen, not taken blindly: alfa_1 = <v, A v> is a sum of both signs (the diagonal is +-(1 .. 10)), and
# where it cancels the float64 orders themselves disagree by 20 .. 150 u at step 1.  These seeds of default_rng([9, n, seed])
# keep every order within 13 u of the longdouble run, plain and preconditioned (EXPERIMENTS.md).
COLUMN_SEEDS = (0, 5, 16, 23, 26, 37, 20, 21, 35, 2)
SMALL_SEEDS = {63: 6, 64: 7, 65: 2}
JACOBI_SEED_20001 = 2

_rhs = {}


def rhs(n, seed=None):
    """A seeded right-hand side of norm 1: ``default_rng(9).standard_normal(n)`` (``seed`` None), else
    ``default_rng([9, n, seed])``; fixed entries for n <= 2."""
    if (n, seed) not in _rhs:
        if n <= 2:
            g = np.array([0.6, -1.3][:n])
        else:
            g = np.random.default_rng(9 if seed is None else [9, n, seed]).standard_normal(n)
        g = g / np.linalg.norm(g)
        g.setflags(write=False)
        _rhs[(n, seed)] = g
    return _rhs[(n, seed)]


SCALED_COLUMN, SCALE = 1, 1e-7     # the block tests scale this column: its deviations are relative and must not move


def column_norm(j):
    """Column 0 has norm 1; the others 0.4 .. 3.2 apart by a factor 1.26, so that no two ``1 / beta`` agree."""
    return 1.0 if j == 0 else 0.4 * 1.26 ** (j - 1) * (SCALE if j == SCALED_COLUMN else 1.0)


def _cases():
    out = []
    for sigma in (0.02, 0.0):
        for sign in (1.0, -1.0):
            out.append(Case(f"g1037 sigma={sigma} sign={sign:+.0f}", "g1037", sigma, sign))
    out += [Case("dense1", "dense1"), Case("dense2", "dense2")]
    for n, seed in SMALL_SEEDS.items():
        out.append(Case(f"g{n}", f"g{n}", seed=seed))
    out.append(Case("g20001", "g20001"))
    for n in (1037, 20001):
        out.append(Case(f"g{n} x0", f"g{n}", x0=True))
    out.append(Case("g1037 jacobi", "g1037", jacobi=True))
    out.append(Case("g20001 jacobi", "g20001", seed=JACOBI_SEED_20001, jacobi=True))
    for j in range(1, NCOLS):
        out.append(Case(f"g1037 column {j}", "g1037", seed=COLUMN_SEEDS[j - 1], norm=column_norm(j)))
        out.append(Case(f"g1037 column {j} jacobi", "g1037", seed=COLUMN_SEEDS[j - 1], norm=column_norm(j), jacobi=True))
    return {c.name: c for c in out}


CASES = _cases()
LONG_CASES = ("g1037 sigma=0.02 sign=+1", "g1037 sigma=0.02 sign=-1", "g1037 x0", "g20001") + tuple(f"g1037 column {j}" for j in range(1, 8))


def block_cases(k, jacobi=False):
    """The k columns of a block test: column 0 is the single-vector case's ``b``."""
    first = CASES["g1037 jacobi" if jacobi else "g1037 sigma=0.02 sign=+1"]
    return [first] + [CASES[f"g1037 column {j}" + (" jacobi" if jacobi else "")] for j in range(1, k)]


_refs = {}


def reference(case, minv=None, nsteps=None):
    """The ``longdouble`` run of a case, computed once and left unchanged.  ``minv``: the device's own inverse diagonal in
    place of the host statement's (keyed by its bytes).  ``nsteps``: that many steps instead of ``case.nsteps`` (a case of
    ``LONG_CASES`` is run to the last of ``LONG_STEPS`` the first time, so no record is ever computed twice)."""
    if not hp.EXTENDED:
        raise RuntimeError("longdouble is no wider than double here")
    mv = case.minv if minv is None else minv
    key = (case.name, None if minv is None else minv.tobytes())
    want = case.nsteps if nsteps is None else nsteps
    if key not in _refs or len(_refs[key]) < want:
        run = max(want, LONG_STEPS[-1]) if case.name in LONG_CASES else want
        _refs[key] = steps(case.op, case.b, case.sigma, case.sign, run, Wide, minv=mv, x0=case.x0)
        for rec in _refs[key]:
            rec["x"].setflags(write=False)
    return _refs[key][:want]


def run_double(case, order="dot", fault=None, nsteps=None):
    """``order``: one of ``ORDERS``, or ``("slabs", P)``."""
    arith = Double(*order) if isinstance(order, tuple) else Double(order)
    return steps(case.op, case.b, case.sigma, case.sign, nsteps or case.nsteps, arith, minv=case.minv, x0=case.x0, fault=fault)


def measured_deviation(cases=None, stats=STATS[:5]):
    """``(D, table)``: the largest deviation of any float64 order from the ``longdouble`` run over the cases, steps and the
    iterate and ``stats``; ``table[(case, step, order)]`` = (largest deviation, its quantity)."""
    table = {}
    for case in (CASES.values() if cases is None else cases):
        ref = reference(case)
        for order in ORDERS:
            for k, (g, r) in enumerate(zip(run_double(case, order), ref), start=1):
                dev = step_deviations(g, r, stats, case.scales(k, ref))
                q = max(dev, key=dev.get)
                table[(case.name, k, order)] = (dev[q], q)
    return max(v[0] for v in table.values()), table


def measured_long_deviation(cases=None, stats=STATS[:5]):
    """``measured_deviation`` over ``LONG_CASES`` (or ``cases``), the steps of ``LONG_STEPS`` and ``LONG_ORDERS``:
    ``(D_LONG, table)``."""
    table = {}
    last = LONG_STEPS[-1]
    for case in ([CASES[name] for name in LONG_CASES] if cases is None else cases):
        ref = reference(case, nsteps=last)
        for order in LONG_ORDERS:
            got = run_double(case, order, nsteps=last)
            for k in LONG_STEPS:
                dev = step_deviations(got[k - 1], ref[k - 1], stats)
                q = max(dev, key=dev.get)
                table[(case.name, k, order if isinstance(order, str) else f"slabs of {order[1]}")] = (dev[q], q)
    return max(v[0] for v in table.values()), table


def step_bound(k):
    """What a device record of step k is held to, in u: ``8 D`` over the first K steps, ``8 D_LONG`` after."""
    return FACTOR * (D if k <= K else D_LONG)


# ---------------------------------------------------------------- exits
class Exit:
    """An operator on which the oracle stops with a rare code: ``H`` (scipy CSR), ``b``, ``sigma``, ``sign``, ``rtol``,
    ``maxiter``, the expected ``(itn, istop)`` and the deciding quantity (``exit_margin``)."""

    def __init__(self, name, H, b, sigma, sign, rtol, maxiter, expect, decides):
        self.name, self.H, self.b, self.sigma, self.sign = name, sp.csr_matrix(H), np.asarray(b, dtype=np.float64), sigma, sign
        self.rtol, self.maxiter, self.expect, self.decides = rtol, maxiter, expect, decides

    def matvec(self, v):
        return self.sign * (self.sigma * v - self.H @ v)


def full_trace(matvec, b, rtol, maxiter, minv=None, order="dot"):
    """The oracle (with ``minv`` the NumPy twin) run with the quantities the stopping tests decide on added to its trace:
    ``(x, itn, istop, trace)``; ``trace[k]`` gains ``Acond``, ``epsx``, ``beta1`` and ``ratio`` (``beta / beta1``).
    ``order``: the summation order of the oracle's inner products (``ORDERS``; the twin has ``np.dot`` only)."""
    from eigensolvers_amd.precond_minres import minres_jacobi_host
    from oracle.minres_ref import minres
    trace = []
    if minv is None:
        dot = Double(order).dot
        x, info, itn, istop = minres(matvec, b, rtol=rtol, maxiter=maxiter, trace=trace, dot=lambda p, q: float(dot(p, q)))
        beta1 = math.sqrt(float(dot(b, b)))
    else:
        x, info, itn, istop = minres_jacobi_host(matvec, b, minv, rtol=rtol, maxiter=maxiter, trace=trace)
        beta1 = math.sqrt(float(np.dot(b, minv * b)))
    # gamma_k from the scalars of the trace: the recurrence of the rotation (the oracle's expressions in its order)
    cs, sn, dbar, gmax, gmin = -1.0, 0.0, 0.0, 0.0, float(np.finfo(np.float64).max)
    for t in trace:
        gbar = sn * dbar - cs * t["alfa"]
        dbar = -cs * t["beta"]
        gamma = max(math.sqrt(gbar * gbar + t["beta"] * t["beta"]), EPS)
        cs, sn = gbar / gamma, t["beta"] / gamma
        gmax, gmin = max(gmax, gamma), min(gmin, gamma)
        t.update(Acond=gmax / gmin, epsx=t["Anorm"] * t["ynorm"] * EPS, beta1=beta1, ratio=t["beta"] / beta1)
    return x, itn, istop, trace


def exit_margin(trace, decides):
    """``(at_stop, before)``: by which factor the deciding quantity is past its threshold at the last step of ``trace``,
    and the least factor by which it is short of it at the steps before (``inf`` with no step before).  ``decides``:
    ``"epsx"`` (against ``beta1``, istop 3), ``"Acond"`` (against ``0.1 / eps``, 4), ``"test1"`` / ``"test2"`` (against
    ``eps``: ``1 + test <= 1`` holds for ``test <= eps / 2``, so the threshold taken is ``eps / 2``), ``"ratio"``
    (``beta / beta1`` against ``10 eps``, -1; decided at step 1 only)."""
    def past(t):
        if decides == "epsx":
            return t["epsx"] / t["beta1"]
        if decides == "Acond":
            return t["Acond"] / (0.1 / EPS)
        if decides == "ratio":
            return math.inf if t["ratio"] == 0 else 10 * EPS / t["ratio"]
        return math.inf if t[decides] == 0 else (EPS / 2) / t[decides]
    before = [1.0 / past(t) if past(t) > 0 else math.inf for t in trace[:-1]]
    return past(trace[-1]), (min(before) if before else math.inf)


def _cyclic_diagonal(values, tiny_at=None, tiny=1e-16, n=1037):
    d = np.asarray(values, dtype=np.float64)[np.arange(n) % len(values)].copy()
    if tiny_at is not None:
        d[tiny_at] = tiny
    return sp.diags(d).tocsr()


TINY_ROW = 518


def _exit_rhs(bj, n=1037):
    """A seeded unit vector with its component on the tiny entry set to ``bj``: that component decides the exit."""
    g = np.random.default_rng(5).standard_normal(n)
    g /= np.linalg.norm(g)
    g[TINY_ROW] = bj
    return g


def _exits():
    """Every case runs ``A = H`` (sigma = 0, sign = -1) with rtol = 0 but the eigenvector case.  The n = 1037 operators
    are diagonal with nine (``d9``) or three (``d3``) distinct values in [1, 2] and one tiny entry (1e-16, 1e-18): a
    right-hand side with weight on that entry meets it once the other values are resolved and its iterate explodes (istop
    3, or 4 where the weight is small), one without never sees it and converges to rounding level (``1 + test1 <= 1``).
    How far the iterate explodes is decided by the rounding residue in ``gamma``, so the weights are chosen for a margin
    under every summation order of ``ORDERS``: with a weight of 1 on the d9 operator one order stops at step 12, not 10."""
    H64 = sp.diags(np.linspace(-1.0, 1.0, 64) + 0.3).tocsr()
    e3 = np.zeros(64)
    e3[3] = 2.0
    H2 = sp.diags([1.0, 1e-17]).tocsr()
    d9 = _cyclic_diagonal(np.linspace(1.0, 2.0, 9), TINY_ROW)
    d3 = _cyclic_diagonal(np.linspace(1.0, 2.0, 3), TINY_ROW, tiny=1e-18)
    out = [Exit("eigenvector n=64", H64, e3, 0.02, 1.0, 1e-10, 50, (1, -1), "ratio"),
           Exit("istop 3 n=2", H2, [1.0, 10.0], 0.0, -1.0, 0.0, 100, (2, 3), "epsx"),
           Exit("istop 4 n=2", H2, [1.0, 0.5], 0.0, -1.0, 0.0, 100, (2, 4), "Acond"),
           Exit("1+test1 n=2", sp.diags([1.0, 1e-3]).tocsr(), [1.0, 3.0], 0.0, -1.0, 0.0, 100, (2, 1), "test1"),
           Exit("istop 3 n=1037", d9, _exit_rhs(30.0), 0.0, -1.0, 0.0, 100, (10, 3), "epsx"),
           Exit("1+test1 n=1037 d9", d9, _exit_rhs(0.0), 0.0, -1.0, 0.0, 100, (9, 1), "test1"),
           Exit("istop 4 n=1037", d3, _exit_rhs(0.1), 0.0, -1.0, 0.0, 100, (4, 4), "Acond"),
           Exit("1+test1 n=1037 d3", d3, _exit_rhs(0.0), 0.0, -1.0, 0.0, 100, (3, 1), "test1")]
    return {e.name: e for e in out}


EXITS = _exits()
# what may not be past its threshold where another code is expected: istop 4 is overwritten by 3 when epsx >= beta1
COMPETES = {"istop 4 n=2": "epsx", "istop 4 n=1037": "epsx"}
