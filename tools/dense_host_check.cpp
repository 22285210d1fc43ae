// Host-side walk through the dense layout's set-up for a sanitizer build.  First, on hand-made records and without any
// device call: the variant checks, every refusal, the grid and the info record.  Then, where there is a GPU: a 5 x 5
// operator from CSR arrays with a repeated and an unsorted entry, variant 6 and block variant 3 asked for, the refusals that need no device (a rectangular and an
// offset operator), a product, the info record, destroy.  Every call is allowed to fail - without a GPU the first device
// call does - and the program still releases what it holds and returns 0: what a sanitizer reports is the finding.
//
//   make -C eigensolvers_amd/csrc hostcheck && tools/dense_host_check      (plain build: keeps it in step with common.h)
// Under the host sanitizers, with the objects in a directory D outside the tree:
//   S="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Xarch_host -fsanitize=address,undefined"
//   for f in eigensolvers_amd/csrc/*.hip tools/dense_host_check.cpp; do hipcc $S -c $f -o D/$(basename $f).obj; done
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined D/*.obj -ldl -o D/dense_host_check && D/dense_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../eigensolvers_amd/csrc/common.h"      // hipeig.h and the internal records, for the part that needs no device

static void report(const char* what, int rc) {
  std::printf("%-34s rc=%d%s%s\n", what, rc, rc ? "  " : "", rc ? hipeig_last_error() : "");
}

// The argument checks, the refusals, the grid and the bookkeeping on hand-made records.  These records own no device
// memory (their CSR pointers are null), so nothing here may get past a refusal: every reserve below is one that refuses
// before its first device call, and a reserve that would build the copy is left to main()'s real operator.
static void host_only() {
  hipeig_csr* A = (hipeig_csr*)calloc(1, sizeof(hipeig_csr));
  hipeig_ctx* c = (hipeig_ctx*)calloc(1, sizeof(hipeig_ctx));
  if (!A || !c) { free(A); free(c); return; }
  int64_t info[8];
  A->nrows = 5; A->ncols = 5; A->nnz = 9;
  report("host: set_variant(6), square", hipeig_csr_set_variant(A, 6));
  report("host: set_block_variant(3)", hipeig_csr_set_block_variant(A, 3));
  report("host: set_variant(7)", hipeig_csr_set_variant(A, 7));
  report("host: set_block_variant(4)", hipeig_csr_set_block_variant(A, 4));
  report("host: dense_info before a build", hipeig_csr_dense_info(A, info));
  std::printf("rows %lld cols %lld ld %lld bytes %lld\n", (long long)info[0], (long long)info[1], (long long)info[2], (long long)info[3]);
  report("host: dense_info(null)", hipeig_csr_dense_info(nullptr, info));
  setenv("HIPEIG_DENSE_GRID", "3", 1);
  A->nrows = A->ncols = 1000;
  std::printf("grid of 1000 rows, 16 per workgroup, cap 3: %d\n", hipeig_dense_grid(A, 16));
  unsetenv("HIPEIG_DENSE_GRID");
  std::printf("the same without the cap: %d\n", hipeig_dense_grid(A, 16));
  A->nrows = 46340;
  std::printf("46340 rows: %d\n", hipeig_dense_grid(A, 16));
  A->nrows = 3;                                               // rectangular
  report("host: set_variant(6), 3 x 1000", hipeig_csr_set_variant(A, 6));
  A->nrows = A->ncols = 5; A->row_offset = 2;                 // a slice
  report("host: set_block_variant(3), offset", hipeig_csr_set_block_variant(A, 3));
  A->row_offset = 0; A->col_stride = 8;                       // remapped columns
  report("host: reserve, remapped columns", hipeig_dense_reserve(c, A));
  A->col_stride = 0; c->collectives = 1;
  report("host: reserve, collectives", hipeig_dense_reserve(c, A));
  c->collectives = 0; c->loop = (void*)c;
  report("host: reserve, loopback group", hipeig_dense_reserve(c, A));
  c->loop = nullptr;
  report("host: dense_info after", hipeig_csr_dense_info(A, info));
  hipeig_dense_free(A);                                       // nothing was built: a no-op, twice
  hipeig_dense_free(A);
  free(A); free(c);
}

int main() {
  host_only();
  hipeig_ctx* ctx = nullptr;
  int rc = hipeig_ctx_create(0, &ctx);
  report("hipeig_ctx_create", rc);
  if (rc || !ctx) {
    std::printf("no device context: the operator path on the device does not run here\n");
    return 0;
  }
  // row 1 stores column 3 twice, row 2 stores its columns in descending order, row 4 is empty
  const int64_t rowptr[6] = {0, 2, 5, 8, 9, 9};
  const int32_t col[9] = {0, 4, 3, 1, 3, 4, 2, 0, 3};
  const double val[9] = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0};
  hipeig_csr* A = nullptr;
  rc = hipeig_csr_create(ctx, 5, 5, 0, rowptr, col, val, &A);
  report("hipeig_csr_create 5 x 5", rc);
  if (!rc && A) {
    report("hipeig_csr_set_variant(6)", hipeig_csr_set_variant(A, 6));
    report("hipeig_csr_set_block_variant(3)", hipeig_csr_set_block_variant(A, 3));
    report("hipeig_csr_set_variant(7)", hipeig_csr_set_variant(A, 7));
    double *x = nullptr, *y = nullptr;
    if (hipMalloc((void**)&x, 5 * sizeof(double)) == hipSuccess && hipMalloc((void**)&y, 5 * sizeof(double)) == hipSuccess) {
      const double hx[5] = {1.0, 1.0, 1.0, 1.0, 1.0};
      double hy[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      (void)hipMemcpy(x, hx, sizeof(hx), hipMemcpyHostToDevice);
      report("hipeig_spmv, dense", hipeig_spmv(ctx, A, x, y));
      hipeig_ctx_sync(ctx);
      (void)hipMemcpy(hy, y, sizeof(hy), hipMemcpyDeviceToHost);
      std::printf("y = %g %g %g %g %g (expected 3 12 21 9 0)\n", hy[0], hy[1], hy[2], hy[3], hy[4]);
    }
    if (x) (void)hipFree(x);
    if (y) (void)hipFree(y);
    int64_t info[8];
    report("hipeig_csr_dense_info", hipeig_csr_dense_info(A, info));
    std::printf("rows %lld cols %lld ld %lld bytes %lld\n", (long long)info[0], (long long)info[1], (long long)info[2], (long long)info[3]);
    report("hipeig_csr_destroy", hipeig_csr_destroy(ctx, A));
  }
  // refused from the operator alone: 3 rows of 5 columns, and 3 rows starting at row 2
  const int64_t rp3[4] = {0, 1, 2, 3};
  const int32_t c3[3] = {0, 1, 2};
  const double v3[3] = {1.0, 1.0, 1.0};
  for (int64_t offset : {(int64_t)0, (int64_t)2}) {
    hipeig_csr* B = nullptr;
    rc = hipeig_csr_create(ctx, 3, 5, offset, rp3, c3, v3, &B);
    report("hipeig_csr_create 3 x 5", rc);
    if (!rc && B) {
      report("  set_variant(6), refused", hipeig_csr_set_variant(B, 6));
      report("  set_block_variant(3), refused", hipeig_csr_set_block_variant(B, 3));
      report("  set_variant(0)", hipeig_csr_set_variant(B, 0));
      report("  hipeig_csr_destroy", hipeig_csr_destroy(ctx, B));
    }
  }
  report("hipeig_ctx_destroy", hipeig_ctx_destroy(ctx));
  return 0;
}
