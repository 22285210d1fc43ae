// Lock-step block MINRES: the nBlock inner solves of one block-Lanczos iteration
// (inexact_Lanczos.py:319-320 calls typeClass.solve once per block vector, on the same operator
// and shift; feast.py:189-201 does the same for the m0 right-hand sides of a contour point)
// advanced TOGETHER, one tall-skinny block product per iteration instead of nBlock operator sweeps.
//
// Every column runs exactly the recurrences of the single-vector driver (minres.hip; the scalar
// code is shared through minres_device.h): its own MinresState record, its own stopping tests in
// SciPy's order, its own iteration count.  A column that has stopped is masked: its iterate is no
// longer touched, so what is returned for it is the iterate of the iteration it stopped at, as
// scipy.sparse.linalg.minres (numpyVector.py:163) would return it.  All vectors are interleaved
// blocks ([row][8]); one iteration = three kernels like the single-vector driver (minres_block_device.h, shared with
// the Jacobi-preconditioned block driver, minres_block_precond.hip):
//   KA  Y = A V - (beta/oldb) R1, V = R2/beta    (block product, fused)  + partials <v_j, y_j>
//   KC  Y -= (alfa/beta) R2                                               + partials <y_j, y_j>
//   KD  W = (V - oldeps W1 - delta W2)/gamma ; X += phi W                  + partials <x_j, x_j>
#include "minres_block_device.h"

template <int K>
static int minres_block_impl(hipeig_ctx* c, hipeig_csr* A, double sigma, double sign, int k,
                             const double* const* b, double* const* x, double rtol, int maxiter,
                             int* info, double* out_stats) {
  HIPEIG_REQUIRE(info != nullptr && b != nullptr && x != nullptr, "null argument");
  HIPEIG_REQUIRE(k >= 1 && k <= K, "more right-hand sides than the interleave width");
  HIPEIG_REQUIRE(sign == 1.0 || sign == -1.0, "sign must be +1 or -1");
  HIPEIG_REQUIRE(maxiter >= 1, "maxiter must be positive");
  HIPEIG_REQUIRE(c->collectives || A->nrows == A->ncols, "the inner solve needs a square operator (or a row partition)");
  const int64_t n = A->nrows;
  for (int j = 0; j < k; ++j) {
    info[j] = 0;
    HIPEIG_REQUIRE(b[j] != x[j], "x must not alias b");
  }
  if (out_stats) memset(out_stats, 0, (size_t)k * 8 * sizeof(double));
  if (n == 0) return 0;

  // recurrence records: <b_j, b_j> with the same reduction as the single-vector driver
  if (const int rc = minres_block_reserve_states(c)) return rc;
  MinresState* h = c->h_mrb_state;
  int live = 0;
  for (int j = 0; j < K; ++j) {
    double bb = 0.0;
    if (j < k && hipeig_dot(c, n, b[j], b[j], &bb)) return 1;
    if (bb > 0.0) { minres_init_state(&h[j], bb); ++live; }
    else {                                   // padding column, or beta1 == 0: the exact solution is x0 = 0
      memset(&h[j], 0, sizeof(MinresState));
      h[j].done = 1;
    }
  }
  if (live == 0) {
    for (int j = 0; j < k; ++j) if (hipeig_vec_fill(c, x[j], n, 0.0)) return 1;
    return 0;
  }

  // workspace: R[3] (r1, r2, y rotate), W[3] (w1, w2, w rotate) and the iterate block
  const int64_t nb = n * K;
  if (const int rc = minres_block_reserve_blocks(c, nb)) return rc;
  double* R[3] = {c->mrb_ws, c->mrb_ws + c->mrb_ws_n, c->mrb_ws + 2 * c->mrb_ws_n};
  double* W[3] = {c->mrb_ws + 3 * c->mrb_ws_n, c->mrb_ws + 4 * c->mrb_ws_n, c->mrb_ws + 5 * c->mrb_ws_n};
  double* xw = c->mrb_ws + 6 * c->mrb_ws_n;
  if (hipeig_block_pack(c, K, n, k, b, R[0])) return 1;
  HIPEIG_CHECK(hipMemsetAsync(R[1], 0, (size_t)c->mrb_ws_n * 6 * sizeof(double), c->stream));
  MinresState* V = c->d_mrb_state;
  HIPEIG_CHECK(hipMemcpyAsync(V, h, K * sizeof(MinresState), hipMemcpyHostToDevice, c->stream));
  if (hipeig_sync_checked(c)) return 4;       // the pinned records are rewritten by the first copy-back

  BlockSweepPlan plan;
  if (const int rc = block_sweep_plan_build<K>(c, A, 1, &plan)) return rc;
  if (const int rc = block_sweep_set_lds_limit(plan, minres_block_ka_kernel<2, K>, minres_block_ka_kernel<2, K, 1>)) return rc;
  // element-wise kernels: every workgroup sums the previous kernel's gE x K partials in its prologue, so FEWER, fatter
  // workgroups pay twice (less prologue traffic, fewer partials).  Measured (tools/experiments/mrb_grid_sweep.sh, N = 1e6,
  // K = 8, ms per block iteration): 4 / 8 / 16 / 32 / 64 items per thread -> 0.483 / 0.483 / 0.469 / 0.463 / 0.496.
  int per_thread = 32;
  if (const char* e = getenv("HIPEIG_MRB_PER_THREAD")) per_thread = atoi(e) > 0 ? atoi(e) : 32;
  const int gE = grid_for(n * (K / 2), per_thread);
  double* pA = c->d_partials;
  double* pC = c->d_partials + BLOCK_PART_STRIDE;
  double* pD = c->d_partials + 2 * BLOCK_PART_STRIDE;
  HIPEIG_REQUIRE(c->partials_doubles >= (size_t)3 * BLOCK_PART_STRIDE, "partial-sum workspace too small");
  const bool dist = c->collectives != 0;
  // row-partitioned run: reduced records of 8 - [0..7] <v,y>, [8..15] <x,x> (ONE all-reduce), [16..23] / [24..31] the
  // end-of-solve flush
  double* red = c->d_scalars + SC_COMM;
  MinresArgs a;
  a.sigma = sigma; a.sign = sign; a.rtol = rtol; a.maxiter = maxiter; a.sC = 0;
  const int nPA = plan.nPA;                              // records of <v_j,y_j> partials one sweep leaves in pA
  a.pA = dist ? red + 0 : pA; a.nA = dist ? 1 : nPA;
  a.pC = pC; a.nC = gE;
  a.pD = dist ? red + 8 : pD; a.nD = dist ? 1 : gE;
  double* slot = nullptr;
  MinresArgs a_kd = a;                                  // KD of a partitioned run: <y_j,y_j> as one share per rank from the exchange's slots
  if (dist) {
    HIPEIG_CHECK(hipMemsetAsync(red, 0, 32 * sizeof(double), c->stream));
    if (hipeig_block_reserve(c, A->gl, K)) return 1;
    slot = hipeig_gather_block_slot(c, A->gl, K);
    HIPEIG_REQUIRE(slot != nullptr, "no block exchange buffer");
    a_kd.pC = c->xb_full + A->gl.slot(0) * K; a_kd.nC = c->nranks; a_kd.sC = A->gl.cstride(A->gl.nchunks - 1) * K;
  }
  c->mr_collectives = 0;

  auto launch_ka = [&](const double* xg, double* r2, double* r1, double* yb, bool late) {
    block_sweep_launch(c, plan, [&](auto v, int grid, int threads, size_t lds, const BcooView& tv, int off) {
      if (late) hipLaunchKernelGGL((minres_block_ka_kernel<decltype(v)::value, K, 1>), dim3(grid), dim3(threads), lds, c->stream,
                                   tv, plan.dview, A->d_rowptr, A->d_col, A->d_val, n, xg, a, V + 0, V + 8, r2, r1, yb, pA + (size_t)off * K);
      else hipLaunchKernelGGL((minres_block_ka_kernel<decltype(v)::value, K>), dim3(grid), dim3(threads), lds, c->stream,
                              tv, plan.dview, A->d_rowptr, A->d_col, A->d_val, n, xg, a, V + 0, V + 8, r2, r1, yb, pA + (size_t)off * K);
    });
  };
  // KD of iteration `it` (buffers of that iteration)
  auto launch_kd = [&](int it, const MinresArgs& ak) {
    hipLaunchKernelGGL(minres_block_kd_kernel<K>, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, ak, V + 16, V + 0,
                       R[it % 3], W[(it + 1) % 3], W[(it + 2) % 3], W[it % 3], xw, pD);
  };

  auto enqueue_iteration = [&](int it) -> int {
    double* r2 = R[it % 3];
    double* yb = R[(it + 1) % 3];
    double* r1 = R[(it + 2) % 3];
    const double* xg = nullptr;
    if (hipeig_block_allgather(c, A, K, r2, &xg)) return 4;
    if (dist) {
      // Two collectives per iteration, as for one right-hand side (minres.hip): the exchange of the operand block carries
      // every rank's shares of <y_j,y_j> (so beta is the directly reduced norm of the updated y, not <y,y> - alfa^2), and
      // one all-reduce carries <v_j,y_j> together with the <x_j,x_j> of the KD that ran just before the sweep.
      ++c->mr_collectives;
      if (it > 0) launch_kd(it - 1, a_kd);
      else HIPEIG_CHECK(hipMemsetAsync(pD, 0, (size_t)gE * K * sizeof(double), c->stream));
      launch_ka(xg, r2, r1, yb, true);
      hipLaunchKernelGGL(sum_two_records_kernel<K>, dim3(2), dim3(HIPEIG_BLOCK), 0, c->stream, pA, nPA, pD, gE, red);
      if (hipeig_allreduce_sum(c, red, 16)) return 4;
      ++c->mr_collectives;
      hipLaunchKernelGGL(minres_block_kc_kernel<K>, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, a, V + 8, V + 16, r2, yb, pC, it > 0 ? 1 : 0);
      hipLaunchKernelGGL(sum_partials_cols_kernel<K>, dim3(1), dim3(HIPEIG_BLOCK), 0, c->stream, pC, gE, slot);   // travels with the next exchange
      return 0;
    }
    launch_ka(xg, r2, r1, yb, false);
    hipLaunchKernelGGL(minres_block_kc_kernel<K>, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, a, V + 8, V + 16, r2, yb, pC, 0);
    launch_kd(it, a);
    return 0;
  };

  const int chunk = 16;
  int it = 0;
  bool all_done = false;
  while (it < maxiter && !all_done) {
    const int iend = (it + chunk < maxiter) ? it + chunk : maxiter;
    for (; it < iend; ++it) {
      const int rc = enqueue_iteration(it);
      if (rc) return rc;
    }
    HIPEIG_CHECK(hipGetLastError());
    if (dist && iend < maxiter) {
      // no flush at a chunk boundary: the records KC left hold the tests of the iteration before; the pending KD runs at
      // the start of the next chunk
      HIPEIG_CHECK(hipMemcpyAsync(h, V + 16, K * sizeof(MinresState), hipMemcpyDeviceToHost, c->stream));
    } else {
      MinresArgs ac = a;
      if (dist) {
        // end of the solve: the last KD and the last tests on their own (their sums have not travelled: two small all-reduces)
        HIPEIG_CHECK(hipMemcpyAsync(red + 16, slot, K * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        if (hipeig_allreduce_sum(c, red + 16, K)) return 4;
        ++c->mr_collectives;
        MinresArgs ak = a;
        ak.pC = red + 16; ak.nC = 1; ak.sC = 0;
        launch_kd(iend - 1, ak);
        hipLaunchKernelGGL(sum_partials_cols_kernel<K>, dim3(1), dim3(HIPEIG_BLOCK), 0, c->stream, pD, gE, red + 24);
        if (hipeig_allreduce_sum(c, red + 24, K)) return 4;
        ++c->mr_collectives;
        ac.pD = red + 24;
      }
      hipLaunchKernelGGL(minres_block_check_kernel<K>, dim3(1), dim3(HIPEIG_BLOCK), 0, c->stream, ac, V + 0);
      HIPEIG_CHECK(hipMemcpyAsync(h, V, K * sizeof(MinresState), hipMemcpyDeviceToHost, c->stream));
    }
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

extern "C" int hipeig_minres_block(hipeig_ctx* c, hipeig_csr* A, double sigma, double sign, int k,
                                   const double* const* b, double* const* x, double rtol, int maxiter,
                                   int* info, double* out_stats) {
  HIPEIG_REQUIRE(k >= 1 && k <= BCOO_KMAX, "a block solve takes 1..8 right-hand sides");
  // blocks of <= 4 use the narrow interleave: twice the accumulator rows per workgroup, half the vector traffic
  if (k <= 4) return minres_block_impl<4>(c, A, sigma, sign, k, b, x, rtol, maxiter, info, out_stats);
  return minres_block_impl<8>(c, A, sigma, sign, k, b, x, rtol, maxiter, info, out_stats);
}
