"""FEAST contour-integration eigensolver on the ``AbstractVector`` surface.

Drop-in for the reference's ``feastDiagonalization`` (feast.py:126-244; Polizzi, PRB 79, 115112):
all eigenpairs of a Hermitian operator inside [eMin, eMax] from a subspace that is filtered by a
Gauss quadrature of the resolvent along a half contour, one shifted linear solve
``(z_k I - A) q = y`` per (contour point, subspace vector), followed by a Rayleigh-Ritz step in
the Loewdin-orthonormalised filtered space.  Backend-agnostic like the Lanczos driver: only
``solve`` (with a complex shift), scalar multiplication, ``real``, ``linearCombination``,
``overlapMatrix`` and ``matrixRepresentation`` of ``type(Y[0])`` are used.

Multi-GPU ("replicas"): with ``contourComm`` the contour points are dealt round
robin to the ranks, every rank holding the whole operator and whole vectors; the only exchange is
one SUM all-reduce per filtered vector after the quadrature loop (in place of the serial
accumulation of ``updateQ``).  All ranks then carry out the same Rayleigh-Ritz step on identical data.

Quadrature: only nodes with positive abscissa are kept (``positiveHalf``), so ``nc`` nodes mean
``nc/2`` solves per vector (util_funcs.py:146-166).  The reference's ``trapezoidal`` rule is
restated with its quirks (off-by-one abscissae, weights (b-a)/(nc+1); util_funcs.py:14-27).
"""
import math
import time
import warnings

import numpy as np
from scipy import special

from .subspace import basisTransformation, loewdin_transform, ritz_pairs

__all__ = ["feastDiagonalization", "quadraturePointsWeights", "calculateQuadrature", "updateQ",
           "select_within_range", "contour_point"]


def _trapezoidal(nc):                                         # util_funcs.py:14-27, quirks kept
    a, b = -1.0, 1.0
    dx = (b - a) / nc
    pts = np.array([a + dx * (i - 1) for i in range(nc)])
    return pts, np.full(nc, (b - a) / (nc + 1))


def quadraturePointsWeights(nc, quad, positiveHalf=True):
    """Nodes and weights on [-1, 1] (util_funcs.py:146-166)."""
    if quad == "legendre":
        gk, wk = special.roots_legendre(nc)
    elif quad == "hermite":
        gk, wk = special.roots_hermite(nc)
    elif quad == "trapezoidal":
        gk, wk = _trapezoidal(nc)
    else:
        raise ValueError(f"unknown quadrature {quad!r}")
    if positiveHalf:
        keep = gk > 0.0
        gk, wk = gk[keep], wk[keep]
    return gk, wk


def select_within_range(values, lo, hi):
    """(values inside [lo, hi], their indices) - util_funcs.py:112-125."""
    idx = [i for i, v in enumerate(values) if lo <= v <= hi]
    return np.array([values[i] for i in idx]), idx


def _eigenvalue_change_in_window(ev, reference, lo, hi):
    """util_funcs.py:249-289 with an eigenvalue range: compare only pairs whose REFERENCE value
    lies in the window (all pairs when none does)."""
    if lo > hi:
        warnings.warn("emin is greater than emax. Moving forward with swapped values")
        lo, hi = hi, lo
    idx = select_within_range(reference, lo, hi)[1]
    if len(idx) >= 1:
        reference, ev = reference[idx], ev[idx]
    num = sum(abs(r - e) for r, e in zip(reference, ev))
    den = sum(abs(e) for e in ev)
    return num / den


def contour_point(eMin, eMax, g, contourEllipseFactor=1.0):
    """Angle and complex node for abscissa g (feast.py:191-195, Polizzi eq. 13)."""
    theta = -(math.pi * 0.5) * (g - 1)
    radius = (eMax - eMin) * 0.5
    z = (eMin + eMax) * 0.5 + radius * (math.cos(theta) + contourEllipseFactor * 1.0j * math.sin(theta))
    return theta, z


def calculateQuadrature(Amat, guess_b, z, radius, angle, weight, contourEllipseFactor):
    """One quadrature term -0.5 w r Re{ e^{i theta} (z - A)^{-1} b } (feast.py:45-103)."""
    b = guess_b
    cls = b.__class__
    if abs(z.imag) < 1e-15:
        opType, z = "her", z.real
    else:
        opType = "gen"
    phase = contourEllipseFactor * math.cos(angle) + math.sin(angle) * 1j
    if b.hasExactAddition:
        Qe = cls.solve(Amat, b, z, opType=opType)
        return cls.real((-0.50 * weight * radius * phase) * Qe)
    mult = -0.25 * weight * radius                             # Polizzi (12): both half planes
    p1 = cls.solve(Amat, b, z, opType=opType)
    p2 = cls.solve(Amat, b, z.conjugate(), opType=opType)
    return cls.linearCombination([p1, p2], [mult * phase, mult * phase.conjugate()])


def _quadrature_terms_block(cls, Amat, guesses, z, radius, angle, weight, contourEllipseFactor):
    """The quadrature terms of ONE contour point for all guesses through the backend's block solve hook, when it has one
    (``HipVector.solveBlock``: the solves share operator and shift, feast.py:198-200, so they can advance in lock step on
    block products).  Same arithmetic per vector as ``calculateQuadrature``; ``None`` = take the one-by-one path."""
    b0 = guesses[0]
    if (not hasattr(cls, "solveBlock") or not b0.hasExactAddition or len(guesses) < 2
            or not getattr(b0, "options", {}).get("blockSolve", True)):
        return None
    if abs(z.imag) < 1e-15:
        opType, z = "her", z.real
    else:
        opType = "gen"
    phase = contourEllipseFactor * math.cos(angle) + math.sin(angle) * 1j
    sols = cls.solveBlock(Amat, list(guesses), z, opType=opType)
    return [cls.real((-0.50 * weight * radius * phase) * Qe) for Qe in sols]


def _contour_pairs(npoints, nsub, contourComm=None, contourDeal="point"):
    """The (contour point, subspace vector) pairs this rank solves, in point-major order.  ``"point"``: whole contour
    points round robin (point k on rank ``k % nranks``); ``"balanced"``: pair ``k*nsub + im0`` round robin, so that every
    rank gets the same mix of points (the points of a contour differ several-fold in the products their solves need);
    ``"vector"``: subspace vector ``im0`` with ALL its contour points on rank ``im0 % nranks`` - for the vector-major
    solvers, whose Lanczos run per vector every rank would otherwise repeat."""
    if contourDeal not in ("point", "balanced", "vector"):
        raise ValueError(f"unknown contourDeal {contourDeal!r} ('point', 'balanced' or 'vector')")
    pairs = [(k, im0) for k in range(npoints) for im0 in range(nsub)]
    if contourComm is None:
        return pairs
    nr, r = contourComm.nranks, contourComm.rank
    if contourDeal == "balanced":
        return [(k, im0) for k, im0 in pairs if (k * nsub + im0) % nr == r]
    if contourDeal == "vector":
        return [(k, im0) for k, im0 in pairs if im0 % nr == r]
    return [(k, im0) for k, im0 in pairs if k % nr == r]


def _takes_shift_per_operand(cls, b0):
    """The backend's ``solveBlock`` takes one shift per right-hand side and hands each solution out as its solve ends
    (``HipVector.solveBlock(..., onSolution=, poolStats=)``)."""
    import inspect
    hook = getattr(cls, "solveBlock", None)
    if hook is None or not b0.hasExactAddition or not getattr(b0, "options", {}).get("blockSolve", True):
        return False
    try:
        return "onSolution" in inspect.signature(hook).parameters
    except (TypeError, ValueError):
        return False


def _pooled_contour_sums(cls, A, Y, pairs, nodes, radius, contourEllipseFactor, status):
    """The filtered vectors of one FEAST iteration with ALL contour solves of this rank handed to the backend as one job
    list (the solves of different contour points are independent, feast.py:189-200; the backend keeps an always-full
    pool of them alive).  ``nodes[k] = (theta, z, weight)``.  Every finished solution becomes its quadrature term with
    the arithmetic of ``_quadrature_terms_block`` and is added to ``Q[im0]`` in ASCENDING point order - a term that
    arrives before its predecessor waits - so that, given identical solves, ``Q`` is bit for bit the per-point loop's.
    A real node keeps today's path; its terms take their place in the same order.  Returns (Q, pool record or None)."""
    nsub = len(Y)
    Q = [None] * nsub
    order = [[k for k, i in pairs if i == im0] for im0 in range(nsub)]
    held = [dict() for _ in range(nsub)]
    taken = [0] * nsub

    def arrive(k, im0, term):
        held[im0][k] = term
        while taken[im0] < len(order[im0]) and order[im0][taken[im0]] in held[im0]:
            nxt = held[im0].pop(order[im0][taken[im0]])
            updateQ(Q, im0, nxt, 0 if Q[im0] is None else 1)
            taken[im0] += 1

    jobs = []
    for k, im0 in pairs:
        theta, z, weight = nodes[k]
        if abs(z.imag) < 1e-15:
            status["quadrature"] = k
            arrive(k, im0, calculateQuadrature(A, Y[im0], z, radius, theta, weight, contourEllipseFactor))
        else:
            jobs.append((k, im0))
    record = {}
    if jobs:
        def on_solution(j, Qe):
            k, im0 = jobs[j]
            theta, z, weight = nodes[k]
            status["quadrature"] = k
            phase = contourEllipseFactor * math.cos(theta) + math.sin(theta) * 1j
            arrive(k, im0, cls.real((-0.50 * weight * radius * phase) * Qe))

        cls.solveBlock(A, [Y[im0] for k, im0 in jobs], [nodes[k][1] for k, im0 in jobs], opType="gen",
                       onSolution=on_solution, poolStats=record)
    if not record:
        return Q, None
    return Q, {"width": record["width"], "rounds": record["rounds"],
               "histogram": dict(sorted(record["histogram"].items())), "pairs": [list(p) for p in jobs],
               "products": list(record["products"]), "outer": list(record["outer"])}


def _shares_lanczos(cls, b0):
    """The vector-major path: the backend solves all contour points of one right-hand side from one Lanczos run
    (``cls._solve_shifts``) and the vectors ask for it (``linearSolver="minres_shifted"``)."""
    lsa = getattr(b0, "options", {}).get("linearSystemArgs", {})
    return lsa.get("linearSolver") == "minres_shifted" and hasattr(cls, "_solve_shifts") and b0.hasExactAddition


def _shared_lanczos_sums(cls, A, Y, pairs, nodes, radius, contourEllipseFactor, status):
    """The filtered vectors of one FEAST iteration vector by vector: ONE ``cls._solve_shifts`` call per subspace vector
    with all complex contour points this rank holds for it (``pairs`` grouped by ``im0``) - the Krylov space of
    ``(z_k I - A) x = Y[im0]`` does not depend on ``z_k``.  Real nodes go through ``calculateQuadrature``.  The terms are
    formed with the arithmetic of ``_quadrature_terms_block`` and added in ascending point order, as
    ``_pooled_contour_sums`` does.  Returns (Q, record): the products per vector and the iterations per (point, vector)."""
    nsub = len(Y)
    Q = [None] * nsub
    record = {"solves": 0, "products": [], "pairs": [], "iterations": []}
    for im0 in range(nsub):
        points = sorted(k for k, i in pairs if i == im0)
        if not points:
            continue
        shifted = [k for k in points if abs(nodes[k][1].imag) >= 1e-15]
        sols = {}
        if shifted:
            xs = cls._solve_shifts(A, Y[im0], [nodes[k][1] for k in shifted])
            sols = dict(zip(shifted, xs))
            stats = getattr(Y[im0], "last_solve_stats", None) or {}
            record["solves"] += 1
            record["products"].append(stats.get("products"))
            its = stats.get("iterations") or [None] * len(shifted)
            for k, n_it in zip(shifted, its):
                record["pairs"].append([k, im0])
                record["iterations"].append(n_it)
        for k in points:
            theta, z, weight = nodes[k]
            status["quadrature"] = k
            if k in sols:
                phase = contourEllipseFactor * math.cos(theta) + math.sin(theta) * 1j
                term = cls.real((-0.50 * weight * radius * phase) * sols.pop(k))
            else:
                term = calculateQuadrature(A, Y[im0], z, radius, theta, weight, contourEllipseFactor)
            updateQ(Q, im0, term, 0 if Q[im0] is None else 1)
    return Q, record


def _filters_lanczos(cls, b0):
    """The two-pass path: the backend forms ``sum_k Re(c_k x_k)`` for a set of right-hand sides without the solutions
    (``cls._lanczos_filter``) and the vectors ask for it (``linearSolver="lanczos_filter"``)."""
    lsa = getattr(b0, "options", {}).get("linearSystemArgs", {})
    return lsa.get("linearSolver") == "lanczos_filter" and hasattr(cls, "_lanczos_filter") and b0.hasExactAddition


def _lanczos_filter_sums(cls, A, Y, pairs, nodes, radius, contourEllipseFactor, status):
    """The filtered vectors of one FEAST iteration from ``cls._lanczos_filter``: all subspace vectors this rank holds go
    through ONE call, with this rank's contour points as shifts and ``-0.5 w r phase`` as weights - real nodes included,
    the recurrence takes a real z as well.  (Vectors that hold different points - ``contourDeal="balanced"`` - take one
    call per distinct set.)  Returns (Q, record): the backend's runs (groups of right-hand sides that advanced in lock
    step), the block products of each pass per run, whether the run's Lanczos basis was ``"kept"``, held as a ``"prefix"``
    or ``"recomputed"`` for pass 2, the vectors it held (``"basis_vectors"``) and in which precision
    (``"basis_precision"``), and the steps per (point, vector)."""
    nsub = len(Y)
    Q = [None] * nsub
    record = {"runs": 0, "products_pass1": [], "products_pass2": [], "basis": [], "basis_vectors": [],
              "basis_precision": [], "pairs": [], "steps": []}
    by_points = {}
    for im0 in range(nsub):
        points = tuple(sorted(k for k, i in pairs if i == im0))
        if points:
            by_points.setdefault(points, []).append(im0)
    for points, vecs in by_points.items():
        shifts, weights = [], []
        for k in points:
            theta, z, weight = nodes[k]
            phase = contourEllipseFactor * math.cos(theta) + math.sin(theta) * 1j
            shifts.append(z.real if abs(z.imag) < 1e-15 else z)
            weights.append(-0.50 * weight * radius * phase)
        status["quadrature"] = points[-1]
        qs = cls._lanczos_filter(A, [Y[im0] for im0 in vecs], shifts, weights)
        seen = set()
        for im0, q in zip(vecs, qs):
            Q[im0] = q
            stats = getattr(Y[im0], "last_solve_stats", None) or {}
            group = stats.get("group", len(seen))
            if group not in seen:
                seen.add(group)
                record["runs"] += 1
                record["products_pass1"].append(stats.get("products_pass1"))
                record["products_pass2"].append(stats.get("products_pass2"))
                record["basis"].append(stats.get("basis"))
                record["basis_vectors"].append(stats.get("basis_vectors"))
                record["basis_precision"].append(stats.get("basis_precision"))
            its = stats.get("iterations") or [None] * len(points)
            for k, n_it in zip(points, its):
                record["pairs"].append([k, im0])
                record["steps"].append(n_it)
    return Q, record


def updateQ(Q, im0, Qquad_k, k):
    """Accumulate the k-th quadrature term into the im0-th filtered vector (feast.py:105-121)."""
    if k == 0:
        Q[im0] = Qquad_k
    else:
        Q[im0] = Qquad_k.__class__.linearCombination([Q[im0], Qquad_k], [1.0, 1.0])
    return Q


def feastDiagonalization(A, Y, nc, quad, eMin, eMax, eConv, maxit, contourEllipseFactor=1.0,
                         writeOut=True, eShift=0.0, convertUnit="au", outFileName=None,
                         summaryFileName=None, contourComm=None, contourPool=False, contourDeal="point"):
    """Arguments and returns as the reference (feast.py:126-165): ``(ev, Y, status)``.

    ``contourComm`` (not in the reference): an object with ``rank``, ``nranks`` and
    ``allreduce(vector) -> vector`` (e.g. ``distributed.ContourReplicas``); contour point k is then
    solved on rank ``k % nranks`` only.

    ``contourPool`` (not in the reference): hand the solves of ALL contour points of an iteration to the backend as one
    job list, when its ``solveBlock`` takes a shift per right-hand side (``HipVector``: an always-full pool of lock-step
    solves instead of one contour point at a time).  The sums are formed in the per-point loop's order;
    ``status["contourPool"]`` then holds, per FEAST iteration, the pool's width, rounds, block products by live
    operands and the products of every (point, vector) solve.  Other backends keep the per-point loop.
    With ``linearSolver="minres_shifted"`` on a backend that has ``_solve_shifts`` (``HipVector``) the iteration runs vector
    by vector instead: one shared-Lanczos solve per subspace vector for all of this rank's complex contour points
    (``shifted_minres.solve_shifts``); ``status["sharedLanczos"]`` holds, per FEAST iteration, the number of such solves,
    their products and the iterations of every (point, vector).  Not together with ``contourPool``.
    With ``linearSolver="lanczos_filter"`` on a backend that has ``_lanczos_filter`` (``HipVector``) all of this rank's
    subspace vectors go through ONE call that returns the filtered sums themselves from two Lanczos passes, no solution
    formed (``lanczos_filter.lanczos_filter``); ``status["lanczosFilter"]`` holds, per FEAST iteration, the runs, the block
    products of each pass and the steps of every (point, vector).  Not together with ``contourPool`` either.
    ``contourDeal``: how ``contourComm`` deals the work, ``"point"`` (above), ``"balanced"`` (the pair
    ``k*nsub + im0`` goes to rank ``(k*nsub + im0) % nranks``: every rank gets the same mix of points) or ``"vector"``
    (vector ``im0`` with all its points on rank ``im0 % nranks``: no rank repeats another's Lanczos run)."""
    if convertUnit != "au":
        raise NotImplementedError("unit conversion needs the reference's in-house `util` module")
    cls = type(Y[0])
    nsub = len(Y)
    shared = _shares_lanczos(cls, Y[0])
    filtered = _filters_lanczos(cls, Y[0])
    if contourPool or filtered:
        from .hip_vector import _need_block_sweeps
        _need_block_sweeps(A, "contourPool=True" if contourPool else "linearSolver='lanczos_filter'")
    if filtered and contourPool:
        raise ValueError("contourPool=True pools GCROT solves; linearSolver='lanczos_filter' forms the filtered vectors of "
                         "all contour points from two Lanczos passes - use one or the other")
    if shared and contourPool:
        raise ValueError("contourPool=True pools GCROT solves; linearSolver='minres_shifted' already serves all contour "
                         "points of a vector from one Lanczos run - use one or the other")
    assert eMax > eMin
    radius = (eMax - eMin) * 0.5
    gk, wk = quadraturePointsWeights(nc, quad, positiveHalf=True)
    status = {"flagAddition": Y[0].hasExactAddition, "outerIter": 0, "quadrature": 0, "isConverged": False,
              "phase": 1, "residual": None, "startTime": time.time(), "runTime": 0.0, "converged": False}
    summary = open(summaryFileName or "summary_feast.out", "w") if writeOut else None
    if summary:
        summary.write("startingPoint\n")
    ev, ref_ev = None, None
    for it in range(maxit):
        status["outerIter"] = it
        Q = [None] * nsub
        pairs = _contour_pairs(len(gk), nsub, contourComm, contourDeal)
        if shared:
            nodes = [contour_point(eMin, eMax, g, contourEllipseFactor) + (w,) for g, w in zip(gk, wk)]
            Q, record = _shared_lanczos_sums(cls, A, Y[:nsub], pairs, nodes, radius, contourEllipseFactor, status)
            status.setdefault("sharedLanczos", []).append(record)
            pairs = []
        if filtered:
            nodes = [contour_point(eMin, eMax, g, contourEllipseFactor) + (w,) for g, w in zip(gk, wk)]
            Q, record = _lanczos_filter_sums(cls, A, Y[:nsub], pairs, nodes, radius, contourEllipseFactor, status)
            status.setdefault("lanczosFilter", []).append(record)
            pairs = []
        if contourPool and pairs and _takes_shift_per_operand(cls, Y[0]):
            nodes = [contour_point(eMin, eMax, g, contourEllipseFactor) + (w,) for g, w in zip(gk, wk)]
            Q, record = _pooled_contour_sums(cls, A, Y[:nsub], pairs, nodes, radius, contourEllipseFactor, status)
            if record is not None:
                status.setdefault("contourPool", []).append(record)
            pairs = []
        for k in range(len(gk)):
            mine = [im0 for kk, im0 in pairs if kk == k]
            if not mine:
                continue
            status["quadrature"] = k
            theta, z = contour_point(eMin, eMax, gk[k], contourEllipseFactor)
            terms = _quadrature_terms_block(cls, A, [Y[im0] for im0 in mine], z, radius, theta, wk[k], contourEllipseFactor)
            for j, im0 in enumerate(mine):
                term = terms[j] if terms is not None else \
                    calculateQuadrature(A, Y[im0], z, radius, theta, wk[k], contourEllipseFactor)
                Q = updateQ(Q, im0, term, 0 if Q[im0] is None else 1)
        if contourComm is not None:
            for im0 in range(nsub):
                mine = Q[im0] if Q[im0] is not None else 0.0 * Y[im0]      # a rank without contour points
                Q[im0] = contourComm.allreduce(mine)
        # Rayleigh-Ritz in the Loewdin-orthonormalised filtered space (feast.py:203-215)
        S = cls.overlapMatrix(Q)
        Hm = cls.matrixRepresentation(A, Q)
        independent, X = loewdin_transform(S)
        status["lindep"] = not independent
        ev, U = ritz_pairs(X, Hm)
        Y = basisTransformation(Q, X @ U)
        if it != 0:
            if len(ref_ev) > len(ev):
                ref_ev = ref_ev[np.argmin(np.abs(ref_ev[:, None] - ev[None, :]), axis=0)]
            elif len(ref_ev) < len(ev):
                raise RuntimeError(f"ref_ev={ref_ev} but ev={ev}. Enlarged space?")
            residual = _eigenvalue_change_in_window(ev, ref_ev, eMin, eMax)
            status["runTime"] = time.time() - status["startTime"]
            status["residual"] = residual
            if summary:
                summary.write("{:>4} ".format(it) + " ".join(f"{e - eShift:.10f}" for e in ev)
                              + f" {residual:5.4e} {status['runTime']:.2f}\n")
                summary.flush()
            if residual < eConv:
                status["converged"] = True        # (the reference's "isConverged" key is never updated; kept so)
                break
        if nsub != len(Y):
            warnings.warn(f"Alert! Got {nsub - len(Y)} dependent vectors")
        nsub = len(Y)
        ref_ev = ev
    if summary:
        summary.write("endingPoint\n")
        summary.close()
    return ev, Y, status
