"""eigensolvers_amd - MI355X-native backend for the inexact-Lanczos shift-and-invert path.

Public surface (mirrors the reference's module-level names for this path):

    from eigensolvers_amd import (AbstractVector, HipVector, HipCsrOperator, HipKronSumOperator, HipContext,
                                  inexactLanczosDiagonalization)

``HipVector`` plugs into ``inexactLanczosDiagonalization`` exactly where the reference's
``NumpyVector`` does; all arithmetic runs in hand-written gfx950 kernels behind the C ABI
of ``include/hipeig.h`` (``libhipeig.so``).  Importing this package does not touch the
GPU; creating a ``HipContext`` / ``HipVector`` does, and fails loudly without one.
"""
from .abstract_vector import AbstractVector, LINDEP_DEFAULT_VALUE
from .hip_vector import HipComplexVector, HipContext, HipCsrOperator, HipKronSumOperator, HipVector
from .checkpoint import latest_checkpoint, load_checkpoint, save_checkpoint
from .feast import feastDiagonalization
from .lanczos import inexactLanczosDiagonalization, KrylovSpace, true_residual_norms
from .lanczos_filter import lanczos_filter, lanczos_filter_host, lanczos_run
from .precond_minres import (csr_diagonal_host, jacobi_inverse_host, minres_jacobi_block_host, minres_jacobi_host,
                             minres_precond_host, separable_apply_host, separable_basis_host, separable_fit_host,
                             separable_scale_host)
from .precond_gcrotmk import jacobi_inverse_z_host
from .shifted_minres import shifted_minres_host, solve_shifts
from .subspace import (basisTransformation, find_nearest, get_pick_function_close_to_sigma,
                       get_pick_function_maxOvlp)

__all__ = ["AbstractVector", "LINDEP_DEFAULT_VALUE", "HipContext", "HipCsrOperator", "HipKronSumOperator", "HipVector",
           "HipComplexVector",
           "feastDiagonalization", "latest_checkpoint", "load_checkpoint", "save_checkpoint",
           "inexactLanczosDiagonalization", "KrylovSpace", "true_residual_norms",
           "basisTransformation", "find_nearest", "get_pick_function_close_to_sigma",
           "get_pick_function_maxOvlp", "shifted_minres_host", "solve_shifts",
           "lanczos_filter", "lanczos_filter_host", "lanczos_run",
           "csr_diagonal_host", "jacobi_inverse_host", "minres_jacobi_host", "minres_jacobi_block_host",
           "jacobi_inverse_z_host", "minres_precond_host", "separable_apply_host", "separable_basis_host",
           "separable_fit_host", "separable_scale_host"]
__version__ = "0.1.0"
