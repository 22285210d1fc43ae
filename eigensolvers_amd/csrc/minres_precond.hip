// The Jacobi preconditioner of the device MINRES: M^-1 = diag(minv), minv_i = 1 / max(|sigma - h_ii|, floor), for SciPy
// 1.15.3's scipy.sparse.linalg.minres(A, b, M=...).  The reference passes no M (numpyVector.py:163), so this path has no
// counterpart there: it is opt-in (linearSystemArgs["preconditioner"]).  Here: the diagonal, its inverse and the start of
// a preconditioned solve; the iteration is the plain solver's with its PRECOND kernels (minres.hip).
#include <math.h>
#include "common.h"
#include "minres_device.h"

// ---- the diagonal and its inverse ---------------------------------------------------------------------------------------
// d_i = sum of the stored (i, i) entries of local row i in stored order (duplicates are separate stored elements), 0 when
// there is none.  One thread per row.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
csr_diagonal_kernel(int64_t nrows, int64_t row_offset, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                    const double* __restrict__ val, double* __restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows) return;
  const int64_t dc = row_offset + i;
  double s = 0.0;
  for (int32_t j = rowptr[i]; j < rowptr[i + 1]; ++j)
    if ((int64_t)col[j] == dc) s += val[j];
  d[i] = s;
}

extern "C" int hipeig_csr_diagonal(hipeig_ctx* c, hipeig_csr* A, double* d) {
  HIPEIG_REQUIRE(d != nullptr, "null output");
  HIPEIG_REQUIRE(!hipeig_kron_raw(A), "a Kronecker-sum operator stores no CSR entries: its diagonal is hipeig_kron_diagonal's");
  HIPEIG_REQUIRE(A->col_stride == 0, "the diagonal is taken from global column indices (one GPU, or a row slice before the columns are remapped)");
  if (A->nrows == 0) return 0;
  const int64_t g = (A->nrows + HIPEIG_BLOCK - 1) / HIPEIG_BLOCK;
  hipLaunchKernelGGL(csr_diagonal_kernel, dim3((unsigned)g), dim3(HIPEIG_BLOCK), 0, c->stream, A->nrows, A->row_offset,
                     A->d_rowptr, A->d_col, A->d_val, d);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// t_i = |sigma - d_i|: max_i and min_i, finished in the last workgroup (common.h).  A NaN counts as +inf in the maximum,
// which is how the host sees it (fmax would drop it).  part: 2 * gridDim.x doubles, out[0] = max, out[1] = min.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
jacobi_range_kernel(int64_t n, const double* __restrict__ d, double sigma, double* __restrict__ part, unsigned* counter,
                    double* __restrict__ out) {
  __shared__ double lds[8];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double mx = 0.0, mn = INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double t = fabs(sigma - d[i]);
    if (t != t) t = INFINITY;
    mx = fmax(mx, t); mn = fmin(mn, t);
  }
  block_reduce_maxmin(mx, mn, lds);
  if (threadIdx.x == 0) { store_partial(part + blockIdx.x, mx); store_partial(part + gridDim.x + blockIdx.x, mn); }
  if (last_block_ticket(counter, gridDim.x, blockIdx.x)) {
    mx = 0.0; mn = INFINITY;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x) {
      mx = fmax(mx, __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      mn = fmin(mn, __hip_atomic_load(part + gridDim.x + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    block_reduce_maxmin(mx, mn, lds);
    if (threadIdx.x == 0) { out[0] = mx; out[1] = mn; }
    release_ticket_counter(counter);
  }
}

__global__ void __launch_bounds__(HIPEIG_BLOCK)
jacobi_inverse_kernel(int64_t n, const double* __restrict__ d, double sigma, double floor_abs, double* __restrict__ minv) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    minv[i] = 1.0 / fmax(fabs(sigma - d[i]), floor_abs);
}

extern "C" int hipeig_jacobi_inverse(hipeig_ctx* c, int64_t n, const double* d, double sigma, double floor_rel, double* minv) {
  HIPEIG_REQUIRE(d != nullptr && minv != nullptr, "null vector");
  HIPEIG_REQUIRE(floor_rel >= 0.0 && floor_rel < INFINITY, "the relative floor must be finite and >= 0");
  if (n <= 0) return 0;
  const int g = grid_for(n, 8);
  double* tot = c->d_scalars + SC_MINRES_TOT;
  hipLaunchKernelGGL(jacobi_range_kernel, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, d, sigma, c->d_partials, c->d_counters, tot);
  HIPEIG_CHECK(hipGetLastError());
  HIPEIG_CHECK(hipMemcpyAsync(c->h_scalars, tot, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (hipeig_sync_checked(c)) return 4;
  const double tmax = c->h_scalars[0], tmin = c->h_scalars[1];
  const double floor_abs = floor_rel * tmax;
  const double mmin = fmax(tmin, floor_abs);            // the smallest m_i = max(t_i, floor)
  if (!(tmax < INFINITY) || !(floor_abs < INFINITY) || !(mmin > 0.0) || !(1.0 / mmin < INFINITY)) {
    hipeig_set_error("Jacobi preconditioner is not finite: max |sigma - d_i| = %g, min = %g, relative floor %g (a diagonal "
                     "entry equal to sigma needs a floor > 0)", tmax, tmin, floor_rel);
    return 3;
  }
  hipLaunchKernelGGL(jacobi_inverse_kernel, dim3(grid_stream(n)), dim3(HIPEIG_BLOCK), 0, c->stream, n, d, sigma, floor_abs, minv);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// z_0 = minv (.) b, r2_0 = b and <b, z_0>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
pmr_start_kernel(int64_t n, const double* __restrict__ b, const double* __restrict__ minv, double* __restrict__ r2,
                 double* __restrict__ z, MinresRed rc) {
  __shared__ double red[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double bv = b[i];
    const double zv = mul_rn(minv[i], bv);
    r2[i] = bv; z[i] = zv;
    acc = fma(bv, zv, acc);
  }
  acc = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) store_partial(rc.part + blockIdx.x, acc);
  if (last_block_ticket(rc.counter, rc.tickets, blockIdx.x)) {
    const double bz = sum_partials_agent(rc.base, rc.count, red);
    if (threadIdx.x == 0) *rc.tot = bz;
    release_ticket_counter(rc.counter);
  }
}

// Start of a preconditioned solve (minres_solve, minres.hip): r2_0 = b, z_0 = minv (.) b and beta1^2 = <b, z_0> on the host.
int hipeig_pmr_start(hipeig_ctx* c, int64_t n, const double* b, const double* minv, double* r2, double* z, int grid,
                     const MinresRed& rc, double* bz_out) {
  hipLaunchKernelGGL(pmr_start_kernel, dim3(grid), dim3(HIPEIG_BLOCK), 0, c->stream, n, b, minv, r2, z, rc);
  HIPEIG_CHECK(hipGetLastError());
  HIPEIG_CHECK(hipMemcpyAsync(c->h_scalars, rc.tot, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (hipeig_sync_checked(c)) return 4;
  const double bz = c->h_scalars[0];
  HIPEIG_REQUIRE(bz >= 0.0, "indefinite preconditioner: <b, M^-1 b> < 0 (or not a number)");
  *bz_out = bz;
  return 0;
}
