#!/usr/bin/env python3
"""Shift-and-invert Lanczos for one interior state of three coupled oscillators on a direct-product sinc-DVR grid, with
the Hamiltonian kept in its factored form  H = sum_d I (x) T_d (x) I + diag(V)  (``HipKronSumOperator``): the products run
factor by factor on the matrix cores and the explicit matrix is never formed on the device.  The grid is small enough for
dense ``eigh`` of the explicit matrix, which the eigenvalue is printed against.  ``--separable`` runs the inner MINRES solves
with the fast-diagonalisation preconditioner of the operator (``linearSystemArgs["preconditioner"] = "separable"``)."""
import os
import sys

import numpy as np
import scipy.linalg as la

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eigensolvers_amd as ea  # noqa: E402
from eigensolvers_amd.generators import coupled_oscillator_grid, guess_vector  # noqa: E402

dims = (13, 10, 7)
factors, V = coupled_oscillator_grid(dims, [(-5, 5), (-4.5, 4.5), (-4, 4)], [1.0, 1.3, 1.7])
H = ea.HipKronSumOperator.from_factors(factors, diag=V)
evEigh = la.eigvalsh(H.to_scipy().toarray())
sigma = 0.513 * evEigh[3] + 0.487 * evEigh[4]                   # between two interior states
options = {"linearSystemArgs": {"linearSolver": "minres", "linearIter": 4000, "linear_tol": 1e-10}}
if "--separable" in sys.argv[1:]:
    options["linearSystemArgs"]["preconditioner"] = "separable"
Y0 = ea.HipVector(guess_vector(H.nrows, 1), options)
ev, Y, status = ea.inexactLanczosDiagonalization(H, Y0, sigma, 8, 10, 1e-12, writeOut=False)
exact = evEigh[ea.find_nearest(evEigh, sigma)[0]]
print("kernels per mode:", H.kron_info()["kernels"], "bytes per product:", H.algorithmic_bytes())
print("eigenvalue:", ev[0], "dense eigh:", exact, "difference:", abs(ev[0] - exact), "converged:", status["isConverged"],
      "cumIter:", status["cumIter"])
