// Lock-step block form of the Jacobi-preconditioned MINRES (opt-in: linearSystemArgs["preconditionerLockStep"]; recurrence,
// byte model and limits: DESIGN.md 3.2b): the right-hand sides of one block-Lanczos iteration, each running the recurrence
// of the preconditioned single solve (minres.hip, PRECOND) on interleaved [row][K] blocks, one block product per iteration.
// The Lanczos vectors are built from Z = minv (.) R2 (minv a plain length-n vector, broadcast along a row) and
// beta_j^2 = <r2_j, z_j>; Z_k is materialised as a ring of two blocks.  One iteration = three kernels:
//   KA'  minres_block_ka_kernel with Z_k where the plain solve passes R2: the gathered operand and the rows of V = s Z_k
//   KC'  Y -= (alfa/beta) R2 ; Z_{k+1} = minv (.) Y                          + partials <y_j, z_{k+1,j}>
//   KD   minres_block_kd_kernel with Z_k where the plain solve passes the old R2 (V = s_old Z_k)
// Records, stopping tests, masking of stopped columns and the host loop are the plain block driver's (minres_block.hip).
// One GPU, whole vectors, x0 = 0.
#include <stdlib.h>
#include "minres_block_device.h"

// Z0 = minv (.) R2 and per-workgroup partials of <r2_j, z0_j>.  One double2 (operands 2(t % (K/2)) and the next of row
// t / (K/2)) per thread and step.
template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
pmrb_start_kernel(int64_t n, const double* __restrict__ r2, const double* __restrict__ minv, double* __restrict__ z,
                  double* __restrict__ partials) {
  __shared__ double red[HIPEIG_BLOCK / 64 * K];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;           // multiple of K/2: operand pair fixed per thread
  const double2* r22 = reinterpret_cast<const double2*>(r2);
  double2* z2 = reinterpret_cast<double2*>(z);
  double a0 = 0.0, a1 = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * (K / 2); t += stride) {
    const double m = minv[t / (K / 2)];
    const double2 rv = r22[t];
    double2 zv;
    zv.x = mul_rn(m, rv.x); zv.y = mul_rn(m, rv.y);
    z2[t] = zv;
    a0 = fma(rv.x, zv.x, a0); a1 = fma(rv.y, zv.y, a1);
  }
  block_reduce_pairs<K>(a0, a1, red, partials + (size_t)blockIdx.x * K);
}

// KC': minres_block_kc_kernel's update of Y, then z_new = minv (.) y and <y_j, z_new_j> where the plain kernel leaves
// <y_j, y_j>.  A stopped column has coefficient 0: its z is rewritten from an unchanged y and never read again.  Once every
// column has stopped the kernel returns before it streams, as KA and KD do.
template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
pmrb_kc_kernel(int64_t n, MinresArgs a, const MinresState* __restrict__ Sin, MinresState* __restrict__ Sout,
               const double* __restrict__ r2, const double* __restrict__ minv, double* __restrict__ y,
               double* __restrict__ znext, double* __restrict__ partials) {
  __shared__ double red[HIPEIG_BLOCK / 64 * K];
  __shared__ double sh_c[K];
  __shared__ int sh_live;
  const double alfa = sum_or_value_cols<K>(a.pA, a.nA, red);
  if (threadIdx.x == 0) sh_live = 0;
  __syncthreads();
  if (threadIdx.x < K) {
    MinresState S = Sin[threadIdx.x];
    if (!S.done) S.alfa = alfa;
    if (blockIdx.x == 0) Sout[threadIdx.x] = S;
    sh_c[threadIdx.x] = S.done ? 0.0 : S.alfa / S.beta;
    if (!S.done) atomicOr(&sh_live, 1);
  }
  __syncthreads();
  if (!sh_live) return;                                   // every column has stopped: the rest of the chunk streams nothing
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;           // multiple of K/2: operand pair fixed per thread
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j0 = (int)(t0 % (K / 2)) * 2;
  const double c0 = sh_c[j0], c1 = sh_c[j0 + 1];
  const double2* r22 = reinterpret_cast<const double2*>(r2);
  double2* y2 = reinterpret_cast<double2*>(y);
  double2* z2 = reinterpret_cast<double2*>(znext);
  double a0 = 0.0, a1 = 0.0;
  for (int64_t t = t0; t < n * (K / 2); t += stride) {
    const double m = minv[t / (K / 2)];
    const double2 rv = r22[t];
    double2 yv = y2[t], zv;
    yv.x -= c0 * rv.x; yv.y -= c1 * rv.y;
    zv.x = mul_rn(m, yv.x); zv.y = mul_rn(m, yv.y);
    y2[t] = yv; z2[t] = zv;
    a0 = fma(yv.x, zv.x, a0); a1 = fma(yv.y, zv.y, a1);
  }
  block_reduce_pairs<K>(a0, a1, red, partials + (size_t)blockIdx.x * K);
}

template <int K>
static int minres_block_jacobi_impl(hipeig_ctx* c, hipeig_csr* A, double sigma, double sign, int k,
                                    const double* const* b, const double* minv, double* const* x, double rtol,
                                    int maxiter, int* info, double* out_stats) {
  HIPEIG_REQUIRE(k >= 1 && k <= K, "more right-hand sides than the interleave width");
  const int64_t n = A->nrows;
  for (int j = 0; j < k; ++j) {
    info[j] = 0;
    HIPEIG_REQUIRE(b[j] != x[j], "x must not alias b");
  }
  if (out_stats) memset(out_stats, 0, (size_t)k * 8 * sizeof(double));
  if (n == 0) return 0;

  // workspace: the plain block solve's seven blocks (R[3], W[3], the iterate), sized, strided and cleared as there, and the
  // ring of two Z blocks in its own buffer
  const int64_t nb = n * K;
  if (const int rc = minres_block_reserve_states(c)) return rc;
  if (const int rc = minres_block_reserve_blocks(c, nb)) return rc;
  if (c->mrbz_ws_n < nb) {
    if (c->mrbz_ws) HIPEIG_CHECK(hipFree(c->mrbz_ws));
    c->mrbz_ws = nullptr; c->mrbz_ws_n = 0;
    HIPEIG_CHECK(hipMalloc((void**)&c->mrbz_ws, (size_t)nb * 2 * sizeof(double)));
    c->mrbz_ws_n = nb;
  }
  double* R[3] = {c->mrb_ws, c->mrb_ws + c->mrb_ws_n, c->mrb_ws + 2 * c->mrb_ws_n};
  double* W[3] = {c->mrb_ws + 3 * c->mrb_ws_n, c->mrb_ws + 4 * c->mrb_ws_n, c->mrb_ws + 5 * c->mrb_ws_n};
  double* xw = c->mrb_ws + 6 * c->mrb_ws_n;
  double* Z[2] = {c->mrbz_ws, c->mrbz_ws + c->mrbz_ws_n};

  int per_thread = 32;                                   // the element-wise grid of the plain block solve (minres_block.hip)
  if (const char* e = getenv("HIPEIG_MRB_PER_THREAD")) per_thread = atoi(e) > 0 ? atoi(e) : 32;
  const int gE = grid_for(n * (K / 2), per_thread);
  double* pA = c->d_partials;
  double* pC = c->d_partials + BLOCK_PART_STRIDE;
  double* pD = c->d_partials + 2 * BLOCK_PART_STRIDE;
  HIPEIG_REQUIRE(c->partials_doubles >= (size_t)3 * BLOCK_PART_STRIDE, "partial-sum workspace too small");

  // start: R2 = B, Z0 = minv (.) B and beta1_j^2 = <b_j, z0_j> - all K sums in one copy and one synchronisation
  if (hipeig_block_pack(c, K, n, k, b, R[0])) return 1;
  HIPEIG_CHECK(hipMemsetAsync(R[1], 0, (size_t)c->mrb_ws_n * 6 * sizeof(double), c->stream));
  double* bz = c->d_scalars + SC_COMM;                   // the block solves' record area; no all-reduce runs here
  hipLaunchKernelGGL(pmrb_start_kernel<K>, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, R[0], minv, Z[0], pC);
  hipLaunchKernelGGL(sum_partials_cols_kernel<K>, dim3(1), dim3(HIPEIG_BLOCK), 0, c->stream, pC, gE, bz);
  HIPEIG_CHECK(hipGetLastError());
  HIPEIG_CHECK(hipMemcpyAsync(c->h_scalars, bz, K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (hipeig_sync_checked(c)) return 4;
  MinresState* h = c->h_mrb_state;
  int live = 0;
  for (int j = 0; j < K; ++j) {
    const double bzj = j < k ? c->h_scalars[j] : 0.0;
    HIPEIG_REQUIRE(bzj >= 0.0, "indefinite preconditioner: <b, M^-1 b> < 0 (or not a number)");
    if (bzj > 0.0) { minres_init_state(&h[j], bzj); ++live; }
    else {                                   // padding column, or beta1 == 0: the exact solution is x0 = 0
      memset(&h[j], 0, sizeof(MinresState));
      h[j].done = 1;
    }
  }
  if (live == 0) {
    for (int j = 0; j < k; ++j) if (hipeig_vec_fill(c, x[j], n, 0.0)) return 1;
    return 0;
  }
  MinresState* V = c->d_mrb_state;
  HIPEIG_CHECK(hipMemcpyAsync(V, h, K * sizeof(MinresState), hipMemcpyHostToDevice, c->stream));
  if (hipeig_sync_checked(c)) return 4;       // the pinned records are rewritten by the first copy-back

  BlockSweepPlan plan;
  if (const int rc = block_sweep_plan_build<K>(c, A, 1, &plan)) return rc;
  if (const int rc = block_sweep_set_lds_limit(plan, minres_block_ka_kernel<2, K>)) return rc;
  MinresArgs a;
  a.sigma = sigma; a.sign = sign; a.rtol = rtol; a.maxiter = maxiter; a.sC = 0;
  a.pA = pA; a.nA = plan.nPA;
  a.pC = pC; a.nC = gE;
  a.pD = pD; a.nD = gE;
  c->mr_collectives = 0;

  auto enqueue_iteration = [&](int it) {
    double* r2 = R[it % 3];
    double* yb = R[(it + 1) % 3];
    double* r1 = R[(it + 2) % 3];
    double* zk = Z[it % 2];
    double* znext = Z[(it + 1) % 2];
    block_sweep_launch(c, plan, [&](auto v, int grid, int threads, size_t lds, const BcooView& tv, int off) {
      hipLaunchKernelGGL((minres_block_ka_kernel<decltype(v)::value, K>), dim3(grid), dim3(threads), lds, c->stream,
                         tv, plan.dview, A->d_rowptr, A->d_col, A->d_val, n, zk, a, V + 0, V + 8, zk, r1, yb, pA + (size_t)off * K);
    });
    hipLaunchKernelGGL(pmrb_kc_kernel<K>, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, a, V + 8, V + 16, r2, minv, yb, znext, pC);
    // KD runs behind KC', which has written Z_{k+1} into the other half of the ring
    hipLaunchKernelGGL(minres_block_kd_kernel<K>, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, a, V + 16, V + 0,
                       zk, W[(it + 1) % 3], W[(it + 2) % 3], W[it % 3], xw, pD);
  };

  // a preconditioned solve is about 20 iterations, and every iteration enqueued past the last stop is four idle launches:
  // 8 / 16 / 32 measured 14.25 / 14.37 / 14.36 ms per block of 8 at N = 1e6
  int chunk = 8;
  if (const char* e = getenv("HIPEIG_PMRB_CHUNK")) chunk = atoi(e) > 0 ? atoi(e) : 8;
  int it = 0;
  bool all_done = false;
  while (it < maxiter && !all_done) {
    const int iend = (it + chunk < maxiter) ? it + chunk : maxiter;
    for (; it < iend; ++it) enqueue_iteration(it);
    HIPEIG_CHECK(hipGetLastError());
    hipLaunchKernelGGL(minres_block_check_kernel<K>, dim3(1), dim3(HIPEIG_BLOCK), 0, c->stream, a, V + 0);
    HIPEIG_CHECK(hipMemcpyAsync(h, V, K * sizeof(MinresState), hipMemcpyDeviceToHost, c->stream));
    if (hipeig_sync_checked(c)) return 4;
    all_done = true;
    for (int j = 0; j < K; ++j) all_done = all_done && h[j].done;
  }
  HIPEIG_REQUIRE(all_done, "block MINRES left the iteration loop without a stop code in every column");
  if (hipeig_block_unpack(c, K, n, k, xw, x)) return 1;
  for (int j = 0; j < k; ++j) {
    info[j] = (h[j].istop == 6) ? maxiter : 0;
    if (out_stats) {
      double* st = out_stats + (size_t)j * 8;
      st[0] = h[j].itn; st[1] = h[j].istop; st[2] = h[j].rnorm; st[3] = h[j].Anorm;
      st[4] = h[j].ynorm; st[5] = h[j].test1; st[6] = h[j].test2; st[7] = h[j].Acond;
    }
  }
  return 0;
}

extern "C" int hipeig_minres_block_jacobi(hipeig_ctx* c, hipeig_csr* A, double sigma, double sign, int k,
                                          const double* const* b, const double* minv, double* const* x, double rtol,
                                          int maxiter, int* info, double* out_stats) {
  HIPEIG_REQUIRE(info != nullptr && b != nullptr && x != nullptr, "null argument");
  HIPEIG_REQUIRE(k >= 1 && k <= BCOO_KMAX, "a block solve takes 1..8 right-hand sides");
  HIPEIG_REQUIRE(sign == 1.0 || sign == -1.0, "sign must be +1 or -1");
  HIPEIG_REQUIRE(maxiter >= 1, "maxiter must be positive");
  HIPEIG_REQUIRE(minv != nullptr, "null preconditioner");
  HIPEIG_REQUIRE(!c->collectives, "the preconditioned solve runs on one GPU (whole vectors, no row partition)");
  HIPEIG_REQUIRE(A->nrows == A->ncols && A->row_offset == 0 && A->col_stride == 0, "the preconditioned solve needs a square operator");
  // blocks of <= 4 use the narrow interleave, as hipeig_minres_block
  if (k <= 4) return minres_block_jacobi_impl<4>(c, A, sigma, sign, k, b, minv, x, rtol, maxiter, info, out_stats);
  return minres_block_jacobi_impl<8>(c, A, sigma, sign, k, b, minv, x, rtol, maxiter, info, out_stats);
}
