// Host side of the Kronecker-sum operator (public variant 7; kernels in kron_device.h).  The handle is an hipeig_csr with
// nnz = 0 and a zeroed row pointer - a stray CSR reader sees an empty matrix, not a null pointer - whose `kron` record
// holds the dims, the padded device copies of the factors, V and the raw-sum buffer.  sweep_launch.h runs the product of
// a sweep into that buffer (hipeig_kron_product) and carries the caller's row epilogue over it with the combine launch of
// the column-split TCOO-W sweep, so the single-vector solvers inherit the operator without a kernel of their own.  Block
// sweeps are not built: block_sweep_launch.h refuses the handle.  Never a fallback, and nothing falls back from it.
#include <vector>
#include "kron_device.h"

struct KronRecord {
  int D;
  int64_t N;
  KronMode mode[KRON_MAX_MODES];
  int form[KRON_MAX_MODES];              // 1 inner MFMA, 2 last-mode MFMA, 3 plain FMA
  double* d_t[KRON_MAX_MODES];
  double* d_tdiag;                       // the factors' diagonals, mode after mode
  int32_t diag_off[KRON_MAX_MODES];
  double* d_v;                           // null without V
  double* d_raw;                         // N raw sums of the product under way
  int64_t bytes;
};

static void kron_free(KronRecord* k) {
  if (!k) return;
  for (int d = 0; d < KRON_MAX_MODES; ++d)
    if (k->d_t[d]) hipFree(k->d_t[d]);
  if (k->d_tdiag) hipFree(k->d_tdiag);
  if (k->d_v) hipFree(k->d_v);
  if (k->d_raw) hipFree(k->d_raw);
  free(k);
}

double* hipeig_kron_raw(const hipeig_csr* A) { return A->kron ? A->kron->d_raw : nullptr; }

static size_t kron_last_lds(const KronMode& m) { return (size_t)(KRON_SLAB + 16 * KRON_IT) * (m.kpad + 2) * sizeof(double); }
static size_t kron_inner_lds(const KronMode& m) { return (size_t)(16 * KRON_IT) * (m.kpad + 2) * sizeof(double); }

// raw = V .* x + sum_d (I (x) T_d (x) I) x on the compute stream: one launch per mode, in ascending order.
int hipeig_kron_product(hipeig_ctx* c, hipeig_csr* A, const double* x) {
  KronRecord* k = A->kron;
  HIPEIG_REQUIRE(k != nullptr, "not a Kronecker-sum operator");
  HIPEIG_REQUIRE(x != k->d_raw, "the operand must not be the operator's raw buffer");
  for (int d = 0; d < k->D; ++d) {
    const KronMode& m = k->mode[d];
    const int first = d == 0 ? 1 : 0;
    const int groups = (m.npad + 16 * KRON_IT - 1) / (16 * KRON_IT);
    if (k->form[d] == 1) {
      const int64_t items = m.no * ((m.s + 63) >> 6);
      const int vec2 = (m.s % 2 == 0 && (uintptr_t)x % 16 == 0) ? 1 : 0;       // the raw buffer is an allocation of its own
      hipLaunchKernelGGL(kron_inner_mfma_kernel, dim3((unsigned)((items + 3) / 4), groups), dim3(HIPEIG_BLOCK), kron_inner_lds(m),
                         c->stream, m, x, (const double*)k->d_v, k->d_raw, first, vec2);
    } else if (k->form[d] == 2) {
      hipLaunchKernelGGL(kron_last_mfma_kernel, dim3((unsigned)((m.no + KRON_SLAB - 1) / KRON_SLAB), groups), dim3(HIPEIG_BLOCK),
                         kron_last_lds(m), c->stream, m, x, (const double*)k->d_v, k->d_raw, first);
    } else {
      hipLaunchKernelGGL(kron_plain_kernel, dim3(grid_stream(2 * k->N)), dim3(HIPEIG_BLOCK), 0, c->stream, m, k->N, x,
                         (const double*)k->d_v, k->d_raw, first);
    }
  }
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

extern "C" int hipeig_kron_create(hipeig_ctx* c, int D, const int64_t* dims, const double* const* factors, const double* diag,
                                  hipeig_csr** out) {
  HIPEIG_REQUIRE(c && dims && factors && out, "null argument");
  if (c->collectives || c->comm || c->loop || c->direct) {
    hipeig_set_error("the Kronecker-sum operator does not take a context with a communicator (row partition, collectives or "
                     "direct exchange)");
    return 2;
  }
  if (D < 1 || D > KRON_MAX_MODES) {
    hipeig_set_error("the Kronecker-sum operator takes 1 to %d modes, got %d", KRON_MAX_MODES, D);
    return 2;
  }
  int64_t N = 1;
  for (int d = 0; d < D; ++d) {
    HIPEIG_REQUIRE(factors[d] != nullptr, "null factor");
    if (dims[d] < 1 || dims[d] > KRON_MAX_N) {
      hipeig_set_error("factor %d is %lld x %lld: the Kronecker kernels take 1 <= n_d <= %d", d + 1, (long long)dims[d],
                       (long long)dims[d], KRON_MAX_N);
      return 2;
    }
    N *= dims[d];
    if (N >= ((int64_t)1 << 31)) {
      hipeig_set_error("the product of the dims must stay below 2^31");
      return 2;
    }
  }
  hipeig_csr* A = (hipeig_csr*)calloc(1, sizeof(hipeig_csr));
  KronRecord* k = (KronRecord*)calloc(1, sizeof(KronRecord));
  if (!A || !k) { free(A); free(k); hipeig_set_error("out of host memory"); return 1; }
  A->kron = k;
  auto build = [&]() -> int {
    A->nrows = A->ncols = N; A->nnz = 0; A->row_offset = 0;
    A->gather_len = N; A->lanes_per_row = 4; A->n_row_blocks = 0;
    A->variant = 7;                                              // pinned: hipeig_csr_pick_variant hands a pinned variant on unchanged
    HIPEIG_CHECK(hipMalloc((void**)&A->d_rowptr, (size_t)(N + 1) * sizeof(int32_t)));
    HIPEIG_CHECK(hipMemsetAsync(A->d_rowptr, 0, (size_t)(N + 1) * sizeof(int32_t), c->stream));
    HIPEIG_CHECK(hipMalloc((void**)&A->d_col, sizeof(int32_t)));
    HIPEIG_CHECK(hipMalloc((void**)&A->d_val, sizeof(double)));
    HIPEIG_CHECK(hipMalloc((void**)&A->d_row_blocks, sizeof(int32_t)));
    HIPEIG_CHECK(hipMemsetAsync(A->d_row_blocks, 0, sizeof(int32_t), c->stream));
    k->D = D; k->N = N;
    int64_t bytes = (N + 1) * 4 + 4 + 8 + 4;
    std::vector<double> tdiag;
    std::vector<std::vector<double>> padded((size_t)D);         // outlive the asynchronous uploads
    int64_t o = 1;
    for (int d = 0; d < D; ++d) {
      const int n = (int)dims[d];
      KronMode& m = k->mode[d];
      m.n = n; m.npad = (n + 15) / 16 * 16; m.kpad = (n + 3) / 4 * 4;
      m.no = o; m.s = N / (o * n);
      o *= n;
      k->form[d] = (n == 1) ? 3 : (m.s == 1) ? 2 : (m.s >= 16) ? 1 : 3;
      std::vector<double>& p = padded[d];
      p.assign((size_t)m.npad * m.kpad, 0.0);
      for (int i = 0; i < n; ++i)
        for (int q = 0; q < n; ++q) p[(size_t)i * m.kpad + q] = factors[d][(size_t)i * n + q];
      k->diag_off[d] = (int32_t)tdiag.size();
      for (int i = 0; i < n; ++i) tdiag.push_back(factors[d][(size_t)i * n + i]);
      HIPEIG_CHECK(hipMalloc((void**)&k->d_t[d], p.size() * sizeof(double)));
      HIPEIG_CHECK(hipMemcpyAsync(k->d_t[d], p.data(), p.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
      m.t = k->d_t[d];
      bytes += (int64_t)p.size() * 8;
    }
    HIPEIG_CHECK(hipMalloc((void**)&k->d_tdiag, tdiag.size() * sizeof(double)));
    HIPEIG_CHECK(hipMemcpyAsync(k->d_tdiag, tdiag.data(), tdiag.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    bytes += (int64_t)tdiag.size() * 8;
    if (diag) {
      HIPEIG_CHECK(hipMalloc((void**)&k->d_v, (size_t)N * sizeof(double)));
      HIPEIG_CHECK(hipMemcpyAsync(k->d_v, diag, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
      bytes += N * 8;
    }
    HIPEIG_CHECK(hipMalloc((void**)&k->d_raw, (size_t)N * sizeof(double)));
    bytes += N * 8;
    HIPEIG_CHECK(hipFuncSetAttribute((const void*)kron_last_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPEIG_CHECK(hipStreamSynchronize(c->stream));
    k->bytes = bytes;
    A->bytes = bytes;
    return 0;
  };
  if (const int rc = build()) {
    hipeig_kron_destroy(c, A);
    return rc;
  }
  *out = A;
  return 0;
}

extern "C" int hipeig_kron_destroy(hipeig_ctx* c, hipeig_csr* A) {
  if (!A) return 0;
  hipStreamSynchronize(c->stream);
  kron_free(A->kron);
  A->kron = nullptr;
  return hipeig_csr_destroy(c, A);
}

// out[0] = modes, [1] = N, [2] = kernel launches per product (one per mode + the combine launch that carries the epilogue),
// [3] = device bytes, [4] = bytes of the raw-sum buffer, [5] = largest factor the kernels take; per mode d (0-based):
// out[8 + 4 d] = kernel form (1 inner MFMA, 2 last-mode MFMA, 3 plain FMA), [9 + 4 d] = n_d, [10 + 4 d] = padded rows,
// [11 + 4 d] = padded columns.
extern "C" int hipeig_kron_info(hipeig_csr* A, int64_t out[40]) {
  HIPEIG_REQUIRE(A && out, "null argument");
  HIPEIG_REQUIRE(A->kron != nullptr, "not a Kronecker-sum operator");
  const KronRecord* k = A->kron;
  memset(out, 0, 40 * sizeof(int64_t));
  out[0] = k->D; out[1] = k->N; out[2] = k->D + 1; out[3] = k->bytes; out[4] = k->N * 8; out[5] = KRON_MAX_N;
  for (int d = 0; d < k->D; ++d) {
    out[8 + 4 * d] = k->form[d]; out[9 + 4 * d] = k->mode[d].n; out[10 + 4 * d] = k->mode[d].npad; out[11 + 4 * d] = k->mode[d].kpad;
  }
  return 0;
}

extern "C" int hipeig_kron_diagonal(hipeig_ctx* c, hipeig_csr* A, double* d) {
  HIPEIG_REQUIRE(c && A && d, "null argument");
  HIPEIG_REQUIRE(A->kron != nullptr, "not a Kronecker-sum operator");
  const KronRecord* k = A->kron;
  KronDiagArgs a;
  memset(&a, 0, sizeof(a));
  a.D = k->D;
  for (int e = 0; e < k->D; ++e) { a.n[e] = k->mode[e].n; a.off[e] = k->diag_off[e]; }
  a.td = k->d_tdiag; a.v = k->d_v;
  hipLaunchKernelGGL(kron_diagonal_kernel, dim3(grid_stream(2 * k->N)), dim3(HIPEIG_BLOCK), 0, c->stream, a, k->N, d);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}
