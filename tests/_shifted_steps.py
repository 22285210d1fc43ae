"""The first steps and the per-shift stops of shifted MINRES against extended precision: reference, cases, faults and
margins (``test_shifted_steps_cpu.py``, ``test_gpu_shifted_steps.py``).  A plain module, imported as ``_minres_steps`` is:
no fixtures, no tests.  Arithmetics, operators, right-hand sides and the deviation measure are ``_minres_steps``'s.

``steps`` is the recurrence of ``shifted_minres_host`` - one real Lanczos run, per shift a complex rotation recurrence and
a three-term update of direction and iterate - written once, without a stopping test, and run in two arithmetics:
``Wide`` (``longdouble`` / ``clongdouble``) is the reference, ``Double(order)`` measures what a correct float64 evaluation
deviates by.  ``K = 6``: step k of the device reads ``r_k`` from ring slot ``k % 3``, writes ``d_k`` over slot ``k & 1`` and
reads state record ``k & 1``; the pair has period 6, and by step 3 every term is live (``t_up`` from step 2, ``c2`` / ``s2``
from step 3), so six steps visit every phase of the rings.

The measure, per shift and step, in u = 2^-53: the relative 2-norm deviation of the complex iterate and the relative
deviation of ``|tau_j|`` (at step ``k == n``, where ``|tau|`` is 0 in exact arithmetic, relative to ``beta1``).  ``D`` is the
largest deviation of any float64 order from the ``longdouble`` run over ``CASES``, steps 1 .. K, every shift and both
quantities (``measured_deviation``; EXPERIMENTS.md holds the table); the device is held to ``FACTOR * D``.

``STOPS`` are runs on g1037 in which far shifts stop inside the first six steps while contour shifts go on: every
``|tau|`` is a factor of 2 at least away from the target at every step that decides (``stop_margin``), under every
summation order, so that device rounding cannot move a stop.
"""
import math

import numpy as np

import _hiprec as hp
from _minres_steps import FACTOR, LD, ORDERS, U, Double, Operator, Wide, deviation, operator, rhs  # noqa: F401
from _sweep_cases import CONTOUR, REAL_SHIFT

K = 6
D = 12.0                         # in u: measured_deviation over CASES gives 11.26 (EXPERIMENTS.md); the condition on the table is D <= 16
BOUND = FACTOR * D
SHIFTS = CONTOUR + [REAL_SHIFT]  # 9: two calls of the C entry (8 + 1)
FAULTS = ("swap_d", "c1_not_conjugated", "g_not_conjugated", "t_up_next_beta", "c2_not_rotated", "c2_frozen", "kc_tail",
          "ku_tail", "v_old_beta", "alpha_f32")
ODD_ONLY = ("kc_tail", "ku_tail")
# Not among them: a wrong sign in the imaginary part of ``d`` (on ``r1i * d1r`` or ``r1r * d1i``).  ``r1``, ``r2`` and ``nu`` are the
# entries of the triangular factor R of ``sign (z I - T)``; ``R^H R = |z|^2 I - 2 Re(z) T + T^2`` is real and R has the positive
# diagonal ``nu``, so R is that matrix's real Cholesky factor, and with it ``d_k`` (a column of ``V R^-1``) is real: ``r1i`` and
# ``Im d`` are 0 in exact arithmetic and rounding residue (1e-16 of their real parts) in any other.  Planted in ``steps``,
# either sign moves no iterate by more than 0.43 u of its norm and no ``|tau|`` at all (``test_shifted_steps_cpu.py``): no result
# can show a fault in these terms.
UNOBSERVABLE = ("d_imag_r1i", "d_imag_r1r")


# ---------------------------------------------------------------- the recurrence
def steps(op, b, shifts, sign, nsteps, arith, fault=None):
    """``nsteps`` steps of shifted MINRES on ``sign (z_j I - H) x_j = b`` with no stopping test (no ``live``, no break on
    ``beta == 0``), every operation in ``arith.real`` and the matching complex type.  The rotation's ``s = t_lo / nu`` is
    real, as on the device; ``nu = sqrt(|dd|^2 + t_lo^2)``.  Returns one dict per step: ``x`` (shape ``(S, n)``, complex, a
    copy), ``tau`` (complex per shift), ``abstau``, ``alpha`` and ``beta`` (``beta_{k+1}``)."""
    T = arith.real
    CT = hp.CLD if T is LD else np.complex128
    sg = T(sign)
    zs = np.asarray(shifts, dtype=complex).reshape(-1).astype(CT)
    S, n = zs.size, op.n
    b = np.asarray(b, dtype=np.float64).astype(T)
    out = []
    with np.errstate(all="ignore"):
        beta1 = np.sqrt(T(arith.dot(b, b)))
        x = np.zeros((S, n), dtype=CT)
        d1 = np.zeros((S, n), dtype=CT)
        d2 = np.zeros((S, n), dtype=CT)
        c1 = np.ones(S, dtype=CT)
        c2 = np.ones(S, dtype=CT)
        s1 = np.zeros(S, dtype=T)
        s2 = np.zeros(S, dtype=T)
        tau = np.full(S, beta1, dtype=CT)
        v_old, v, beta, beta_old = np.zeros(n, dtype=T), b / beta1, T(0), beta1
        for k in range(1, nsteps + 1):
            w = arith.matvec(op, v) - beta * v_old
            alpha = T(arith.dot(v, w))
            if fault == "alpha_f32":
                alpha = T(np.float32(alpha))
            wn = w - alpha * v
            if fault == "kc_tail" and n & 1:
                wn[-1] = w[-1]
            w = wn
            beta_new = np.sqrt(T(arith.dot(w, w)))
            for j in range(S):
                # column k of sign (z I - T): above the diagonal, on it, below it
                t_up = -sg * (beta_new if fault == "t_up_next_beta" and k > 1 else beta)
                t_d = sg * (zs[j] - alpha)
                t_lo = -sg * beta_new
                cc, ss = (c1[j], s1[j]) if fault == "c2_not_rotated" else (c2[j], s2[j])
                r2 = ss * t_up
                tmp = cc * t_up
                r1 = (c1[j] if fault == "c1_not_conjugated" else np.conj(c1[j])) * tmp + s1[j] * t_d
                dd = -s1[j] * tmp + c1[j] * t_d
                nu = np.sqrt(dd.real * dd.real + dd.imag * dd.imag + t_lo * t_lo)
                c, s = dd / nu, t_lo / nu                # G = [[conj c, s], [-s, c]]
                if fault == "swap_d":
                    d = (v - r1 * d2[j] - r2 * d1[j]) / nu
                else:
                    d = (v - r1 * d1[j] - r2 * d2[j]) / nu
                if fault == "d_imag_r1i":                # Im d = (- r1i d1r - r1r d1i - r2 d2i) / nu with + r1i d1r
                    d = d + CT(2j) * (r1.imag * d1[j].real) / nu
                if fault == "d_imag_r1r":                # ... with + r1r d1i
                    d = d + CT(2j) * (r1.real * d1[j].imag) / nu
                g = (c if fault == "g_not_conjugated" else np.conj(c)) * tau[j]
                xn = x[j] + g * d
                if fault == "ku_tail" and n & 1:         # d_k is written over d_{k-2}: the skipped element keeps that
                    d[-1] = d2[j][-1]
                    xn[-1] = x[j][-1]
                x[j] = xn
                tau[j] = -s * tau[j]
                d2[j], d1[j] = d1[j], d
                if fault != "c2_frozen":
                    c2[j], s2[j] = c1[j], s1[j]
                c1[j], s1[j] = c, s
            out.append(dict(x=x.copy(), tau=tau.copy(), abstau=np.abs(tau), alpha=alpha, beta=beta_new))
            v_old, v = v, w / (beta_old if fault == "v_old_beta" else beta_new)
            beta_old, beta = beta_new, beta_new
    return out


# ---------------------------------------------------------------- the measure
def x_deviation(got, ref):
    """``deviation`` of a complex vector: the relative 2-norm over real and imaginary parts."""
    g, r = np.asarray(got), np.asarray(ref)
    return deviation(np.concatenate([g.real, g.imag]), np.concatenate([r.real, r.imag]))


def tau_deviation(got, ref, scale=None):
    """``| |tau| - ref | / ref`` in u; relative to ``scale`` where given (step ``k == n``: ``beta1``)."""
    g = LD(got)
    if not np.isfinite(g):
        return float("inf")
    return float(abs(g - LD(ref)) / (LD(ref) if scale is None else LD(scale))) / U


def step_deviations(case, k, x, abstau, ref, shifts=None):
    """``{"x": .., "tau": ..}``: the largest deviation over the shifts (``shifts``: their indices in the case's list, all
    by default) of ``x[i]`` and ``abstau[i]`` from step ``k`` of the reference's records ``ref``."""
    idx = range(len(case.shifts)) if shifts is None else shifts
    r = ref[k - 1]
    scale = case.tau_scale(k)
    return {"x": max(x_deviation(x[i], r["x"][j]) for i, j in enumerate(idx)),
            "tau": max(tau_deviation(abstau[i], r["abstau"][j], scale) for i, j in enumerate(idx))}


# ---------------------------------------------------------------- the case table
class Case:
    """Operator, right-hand side, shifts and sign of one run of K (or n, if smaller) steps.  With ``target`` a stop case:
    ``expect[j]`` is the step shift j stops at, ``None`` for a shift still live after ``K`` steps."""

    def __init__(self, name, opname, sign=1.0, seed=None, shifts=SHIFTS, target=None, expect=None):
        self.name, self.opname, self.sign, self.seed = name, opname, sign, seed
        self.shifts, self.target, self.expect = list(shifts), target, expect

    @property
    def op(self):
        return operator(self.opname)

    @property
    def nsteps(self):
        return min(K, self.op.n)

    @property
    def b(self):
        return rhs(self.op.n, self.seed)

    def tau_scale(self, k):
        """Step ``k == n`` ends the Krylov space: ``|tau|`` is 0 in exact arithmetic, so it is held relative to ``beta1``."""
        return hp.nrm2(self.b) if k == self.op.n else None


# Right-hand sides are chosen, not taken blindly (as _minres_steps.COLUMN_SEEDS): alpha_1 = <v, H v> cancels between the
# diagonal's two signs, and where it does the float64 orders themselves disagree by more than 16 u.  rhs(65) gives 17.4 u
# and rhs(65, 2) 19.1 u; rhs(65, 1) 7.2 u (EXPERIMENTS.md).
SEEDS = {"g63": None, "g64": None, "g65": 1, "g1037": None, "g20001": None, "dense1": None, "dense2": None}


def _cases():
    out = []
    for opname, seed in SEEDS.items():
        for sign in (1.0, -1.0):
            out.append(Case(f"{opname} sign={sign:+.0f}", opname, sign, seed))
    return {c.name: c for c in out}


CASES = _cases()

# Far shifts on g1037 (||H|| is about 10): |tau| falls by roughly |z| / ||H|| per step, the contour shifts' stay above 0.35.
TARGET = 2.5e-3
FAR = [60.0, 30j, 20 - 20j]
MIXED_SHIFTS = [CONTOUR[0], FAR[0], CONTOUR[3], FAR[1], FAR[2], CONTOUR[7], REAL_SHIFT, 200j]
MIXED_EXPECT = [None, 3, None, 4, 4, None, None, 2]
ALL_STOP_SHIFTS = FAR + [-70 + 10j, 45 + 45j, 200j, -200.0, -28j]
ALL_STOP_EXPECT = [3, 4, 4, 3, 3, 2, 2, 4]
STOPS = {"mixed": Case("stops mixed", "g1037", 1.0, None, MIXED_SHIFTS, TARGET, MIXED_EXPECT),
         "all-stop": Case("stops all", "g1037", 1.0, None, ALL_STOP_SHIFTS, TARGET, ALL_STOP_EXPECT)}

_refs = {}


def reference(case):
    """The ``longdouble`` run of a case, computed once and left unchanged."""
    if not hp.EXTENDED:
        raise RuntimeError("longdouble is no wider than double here")
    if case.name not in _refs:
        _refs[case.name] = steps(case.op, case.b, case.shifts, case.sign, case.nsteps, Wide)
        for rec in _refs[case.name]:
            for a in rec.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return _refs[case.name]


def run_double(case, order="dot", fault=None):
    return steps(case.op, case.b, case.shifts, case.sign, case.nsteps, Double(order), fault=fault)


def measured_deviation(cases=None):
    """``(D, table)``: the largest deviation of any float64 order from the ``longdouble`` run over the cases, steps,
    shifts and both quantities; ``table[(case, step, order)]`` = (largest deviation, its quantity)."""
    table = {}
    for case in (CASES.values() if cases is None else cases):
        ref = reference(case)
        for order in ORDERS:
            for k, g in enumerate(run_double(case, order), start=1):
                dev = step_deviations(case, k, g["x"], g["abstau"], ref)
                q = max(dev, key=dev.get)
                table[(case.name, k, order)] = (dev[q], q)
    return max(v[0] for v in table.values()), table


# ---------------------------------------------------------------- stops
def stop_margin(case, arith=Wide):
    """``(margin, stops)`` of a stop case under ``arith``.  For a shift that stops, the smaller of the factor by which
    ``|tau|`` is below the target at its stop step and the least factor by which it is above it at the steps before; for a
    shift that must not stop, the least factor above the target over steps 1 .. K.  ``margin`` is the least over the
    shifts; ``stops[j]`` is the first step at which ``|tau_j| <= target`` (``None``: none up to K)."""
    recs = reference(case) if arith is Wide else steps(case.op, case.b, case.shifts, case.sign, K, arith)
    margin, stops = math.inf, []
    for j in range(len(case.shifts)):
        t = [float(r["abstau"][j]) for r in recs]
        at = next((k for k, v in enumerate(t, start=1) if v <= case.target), None)
        stops.append(at)
        want = case.expect[j]
        before = t if want is None else t[:want - 1]
        m = min([v / case.target for v in before], default=math.inf)
        if want is not None:
            m = min(m, case.target / t[want - 1] if t[want - 1] > 0 else math.inf)
        margin = min(margin, m)
    return margin, stops
