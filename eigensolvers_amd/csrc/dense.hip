// The dense copy of an operator (public variant 6, block variant 3): one more co-resident copy of the local rows, row-major
// fp64 with zero padding, built on the device from the CSR arrays on first use.  The sweeps live in dense_device.h; the
// launchers (sweep_launch.h, block_sweep_launch.h) reserve the copy and size the grids through the functions below.
// The layout is never a fallback and never falls back: an operator or context it does not take is refused with a message.
#include "dense_device.h"

// The fill kernel's loads and stores of the copy go past the CU's L1: the lane that last wrote a position need not be the
// one that reads it next.
__device__ __forceinline__ double dense_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void dense_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One wave per row, 64 stored entries per step.  a[r][c] receives the sum of the entries stored at (r, c) in stored order
// (what the CSR product adds up, hipeig.h at hipeig_csr_create); positions without an entry keep the zero of the memset.
// No floating-point atomics: inside a step the first lane that holds a column adds the later ones of that column in
// order; steps follow each other in program order, each behind the stores of the one before.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
dense_fill_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const double* __restrict__ val,
                  int64_t nrows, int64_t ld, double* a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < nrows; r += nwaves) {
    double* arow = a + r * ld;
    const int s = rowptr[r], e = rowptr[r + 1];
    for (int p0 = s; p0 < e; p0 += 64) {
      const int p = p0 + lane;
      const bool ok = p < e;
      const int cc = ok ? col[p] : -1;
      const double v = ok ? val[p] : 0.0;
      const int before = __shfl_up(cc, 1, 64);
      const bool ascending = !ok || lane == 0 || before < cc;
      if (__ballot(!ascending) == 0) {                           // strictly ascending columns: no column twice in this step
        if (ok) dense_store(arow + cc, dense_load(arow + cc) + v);
      } else {
        bool first = ok;
        double sum = ok ? dense_load(arow + cc) + v : 0.0;
        for (int k = 0; k < 64; ++k) {
          const int ck = __shfl(cc, k, 64);
          const double vk = __shfl(v, k, 64);
          if (ok && ck == cc) {
            if (k < lane) first = false;
            else if (k > lane) sum += vk;
          }
        }
        if (first) dense_store(arow + cc, sum);
      }
      wait_for_my_stores();                                      // a later step may hold the same column in another lane
    }
  }
}

// Why this operator / context cannot take the dense layout (error set, 2), or 0.  `c` may be null: the checks an operator
// allows on its own (hipeig_csr_set_variant has no context).
int hipeig_dense_refusal(const hipeig_ctx* c, const hipeig_csr* A) {
  if (c && (c->collectives || c->comm || c->loop || c->direct)) {
    hipeig_set_error("the dense layout does not take a context with a communicator (collectives or direct exchange)");
    return 2;
  }
  if (A->row_offset != 0 || A->nrows != A->ncols || A->col_stride != 0) {
    hipeig_set_error("the dense layout needs a whole square operator: rows %lld, columns %lld, row offset %lld%s",
                     (long long)A->nrows, (long long)A->ncols, (long long)A->row_offset,
                     A->col_stride != 0 ? ", remapped columns" : "");
    return 2;
  }
  return 0;
}

// Builds the copy unless it exists (idempotent).  0 on success; 2 refused; 1 on a failure.  Nothing stays allocated after
// either of the latter.
int hipeig_dense_reserve(hipeig_ctx* c, hipeig_csr* A) {
  if (const int rc = hipeig_dense_refusal(c, A)) return rc;
  if (A->d_dense) return 0;
  const int64_t ld = (A->ncols + DENSE_LD_ALIGN - 1) / DENSE_LD_ALIGN * DENSE_LD_ALIGN;
  const int64_t bytes = A->nrows * ld * (int64_t)sizeof(double);
  if (bytes == 0) { A->dense_ld = ld; return 0; }                // no rows: no sweep is ever launched
  size_t free_b = 0, total_b = 0;
  HIPEIG_CHECK(hipMemGetInfo(&free_b, &total_b));
  if ((uint64_t)bytes > (uint64_t)free_b) {
    hipeig_set_error("the dense copy (%lld bytes) does not fit the free device memory (%lld bytes)", (long long)bytes, (long long)free_b);
    return 2;
  }
  double* a = nullptr;
  auto build = [&]() -> int {
    HIPEIG_CHECK(hipMalloc((void**)&a, (size_t)bytes));
    HIPEIG_CHECK(hipMemsetAsync(a, 0, (size_t)bytes, c->stream));
    if (A->nnz > 0) {
      const int64_t want = (A->nrows + 3) / 4;                   // a wave per row
      const int grid = (int)(want < 8 * (int64_t)c->num_cu ? want : 8 * (int64_t)c->num_cu);
      hipLaunchKernelGGL(dense_fill_kernel, dim3(grid < 1 ? 1 : grid), dim3(HIPEIG_BLOCK), 0, c->stream, A->d_rowptr, A->d_col, A->d_val,
                         A->nrows, ld, a);
      HIPEIG_CHECK(hipGetLastError());
    }
    HIPEIG_CHECK(hipStreamSynchronize(c->stream));
    return 0;
  };
  if (const int rc = build()) {
    if (a) hipFree(a);
    return rc;
  }
  A->d_dense = a; A->dense_ld = ld; A->dense_bytes = bytes;
  A->bytes += bytes;
  return 0;
}

void hipeig_dense_free(hipeig_csr* A) {
  if (A->d_dense) hipFree(A->d_dense);
  A->d_dense = nullptr; A->dense_bytes = 0;
}

DenseView hipeig_dense_view(const hipeig_csr* A) {
  DenseView d;
  d.a = A->d_dense; d.nrows = A->nrows; d.ncols = A->ncols; d.ld = A->dense_ld;
  return d;
}

// Persistent grid of a dense sweep whose workgroups take `rows_per_wg` rows per step: one workgroup per row group, at most
// HIPEIG_MAX_PARTIALS, at most HIPEIG_DENSE_GRID (tuning knob, read per launch; what lets a small operator reach the
// persistent loop).  The grid never changes a bit of the result (dense_device.h).
int hipeig_dense_grid(const hipeig_csr* A, int rows_per_wg) {
  int64_t g = (A->nrows + rows_per_wg - 1) / rows_per_wg;
  if (g > HIPEIG_MAX_PARTIALS) g = HIPEIG_MAX_PARTIALS;
  if (const char* e = getenv("HIPEIG_DENSE_GRID")) {
    const int64_t cap = atoll(e);
    if (cap >= 1 && cap < g) g = cap;
  }
  return g < 1 ? 1 : (int)g;
}

extern "C" int hipeig_csr_dense_info(hipeig_csr* A, int64_t out[8]) {
  HIPEIG_REQUIRE(A && out, "null argument");
  memset(out, 0, 8 * sizeof(int64_t));
  out[0] = A->nrows; out[1] = A->ncols;
  out[2] = A->d_dense ? A->dense_ld : (A->ncols + DENSE_LD_ALIGN - 1) / DENSE_LD_ALIGN * DENSE_LD_ALIGN;
  out[3] = A->dense_bytes;
  out[4] = DENSE_ROWS_PER_WAVE;
  out[5] = A->dense_grid_vec; out[6] = A->dense_grid_blk;
  return 0;
}
