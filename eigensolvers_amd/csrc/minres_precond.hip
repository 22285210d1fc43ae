// Jacobi-preconditioned device MINRES for sign*(sigma*I - H) x = b: SciPy 1.15.3's scipy.sparse.linalg.minres(A, b, M=...)
// with the diagonal M^-1 = diag(minv), minv_i = 1 / max(|sigma - h_ii|, floor).  The reference passes no M
// (numpyVector.py:163), so this path has no counterpart there: it is opt-in (linearSystemArgs["preconditioner"]).
//
// SciPy's recurrence with M differs from the plain one in ONE vector: the Lanczos vector is built from y = M^-1 r2
// instead of r2, and beta^2 = <r2, M^-1 r2> instead of <r2, r2>.  z_k = minv (.) r2_k is materialised, so the sweep still
// gathers from one vector, and the scalar side (minres_device.h) is the plain solver's, unchanged:
//   start  z_0 = minv (.) b                                                  + <b, z_0>  (= beta1^2)
//   KA'    y = A v - (beta/oldb) r1,  v = z_k/beta     (operator sweep gathering z_k) + <v,y>
//   KC'    y -= (alfa/beta) r2 ; z_{k+1} = minv (.) y                        + <y, z_{k+1}>  (= beta_{k+1}^2)
//   KD     w = (v - oldeps*w1 - delta*w2)/gamma ; x += phi*w                 + <x,x>
// KD(k-1) rides on the sweep of KA'(k) as in minres.hip; its v is s_old*z_{k-1}, one stream more than there, where r1
// served for both.  A ring of two z buffers suffices: z_{k-1} has been consumed by that KD before KC'(k) overwrites it.
// HIPEIG_MINRES_FUSE_KD=0 keeps the three-kernel form; both forms evaluate the same expressions in the same order.
//
// One GPU, whole vectors, no initial guess, no hipGraph: a solve is tens of iterations, so nothing is left to amortise.
// Bytes per iteration: those of minres.hip + 24 N (KC' reads minv and writes z, the riding KD reads z_{k-1}; the KA'
// epilogue reads z_k where KA read r2).
#include <math.h>
#include "spmv_device.h"

CsrView hipeig_csr_view(const hipeig_csr* A);
TcooView hipeig_tcoo_view(const hipeig_csr* A, const BlockedLayout& L);
int hipeig_tcoow_run_plan(hipeig_ctx* c, hipeig_csr* A, const double* x_local, int fixed, TcooView* last, bool* has_last,
                          const double** xg, int* ncombine);
int hipeig_tcoow_reserve(hipeig_ctx* c, const hipeig_csr* A);
SweepGrid hipeig_sweep_grid(const hipeig_csr* A, int variant);
int hipeig_csr_pick_variant(hipeig_ctx* c, hipeig_csr* A);
size_t hipeig_tcoo_lds_bytes(const hipeig_csr* A);

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
  HIPEIG_REQUIRE(A->col_stride == 0, "the diagonal is taken from global column indices (one GPU, or a row slice before the columns are remapped)");
  if (A->nrows == 0) return 0;
  const int64_t g = (A->nrows + HIPEIG_BLOCK - 1) / HIPEIG_BLOCK;
  hipLaunchKernelGGL(csr_diagonal_kernel, dim3((unsigned)g), dim3(HIPEIG_BLOCK), 0, c->stream, A->nrows, A->row_offset,
                     A->d_rowptr, A->d_col, A->d_val, d);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// max and min over the workgroup (exact, order-free); valid in thread 0.  lds: 8 doubles.
__device__ __forceinline__ void block_reduce_maxmin(double& mx, double& mn, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mx = fmax(mx, __shfl_xor(mx, off, 64));
    mn = fmin(mn, __shfl_xor(mn, off, 64));
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { lds[wid] = mx; lds[4 + wid] = mn; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) { mx = fmax(mx, lds[w]); mn = fmin(mn, lds[4 + w]); }
  __syncthreads();
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

// ---- the iteration ----------------------------------------------------------------------------------------------------
// Row epilogue of KA': v = s*z_k[r]; y = sign*(sigma*v - s*sum) - (beta/oldb)*r1[r]; <v,y>; and the KD of the iteration
// before, whose v is s_old*z_{k-1}[r].
struct PmrRowEpilogue {
  double sigma, sign, s, c1;
  int use_r1;
  const double* __restrict__ z;     // local slice of z_k (v = s*z)
  const double* __restrict__ r1;
  double* __restrict__ y;
  int do_kd;
  MinresKd kd;
  const double* __restrict__ zold;  // z_{k-1}
  const double* __restrict__ w1;
  const double* __restrict__ w2;
  double* __restrict__ w;
  double* __restrict__ x;
  double* xx;                       // running <x,x> of this thread
  __device__ __forceinline__ void row(int64_t r, double sum, double& acc) const {
    const double v = s * z[r];
    double yv = sign * (mul_rn(sigma, v) - s * sum);
    if (use_r1) yv -= c1 * r1[r];
    y[r] = yv;
    acc = fma(v, yv, acc);
    if (do_kd) {
      double wn, xv = x[r];
      kd.apply(zold[r], w1[r], w2[r], wn, xv);
      w[r] = wn; x[r] = xv;
      *xx = fma(xv, xv, *xx);
    }
  }
};

struct PmrKdArgs {
  int do_kd;
  const double* zold;
  const double* w1;
  const double* w2;
  double* w;
  double* x;
  MinresRed red;                    // <x,x>: partials laid out like the launch's <v,y> partials
};

// VARIANT 1-4: the operator sweep of that layout; FIXED = 1 (VARIANT 4 only): fixed-point accumulators (public variant 5).
template <int VARIANT, int FIXED = 0>
__global__ void __launch_bounds__(VARIANT == 4 ? TCOOW_THREADS : HIPEIG_BLOCK)
pmr_ka_kernel(CsrView A, TcooView T, const double* __restrict__ xg, MinresArgs a, const MinresState* __restrict__ Sin,
              MinresState* __restrict__ Sout, const double* __restrict__ z, const double* __restrict__ r1,
              double* __restrict__ y, MinresRed ra, PmrKdArgs kda) {
  __shared__ double prod[VARIANT == 2 ? SPMV_NNZ_PER_BLOCK : 8];
  __shared__ double red[16];
  extern __shared__ double tcoo_lds[];
  MinresState S = *Sin;
  PmrRowEpilogue epi;
  epi.do_kd = 0;
  if (kda.do_kd) {
    // Sin is the record KC' left: the scalar half of KD happens here, its vector half in the epilogue
    if (!S.done) {
      const double bb = minres_yy(a);
      epi.kd.s_old = S.s;
      minres_advance(S, bb);
      epi.kd.oldeps = S.oldeps; epi.kd.delta = S.delta; epi.kd.denom = S.denom; epi.kd.phi = S.phi;
      epi.do_kd = 1;
    }
  } else {
    const double xx = (S.itn > 0 && !S.done) ? a.pD[0] : 0.0;
    minres_tests(S, xx, a);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *Sout = S;
  if (S.done) return;
  epi.sigma = a.sigma; epi.sign = a.sign; epi.s = S.s;
  epi.use_r1 = S.itn >= 1;
  epi.c1 = epi.use_r1 ? S.beta / S.oldb : 0.0;
  epi.z = z; epi.r1 = r1; epi.y = y;
  double acc = 0.0, acc_xx = 0.0;
  epi.zold = kda.zold; epi.w1 = kda.w1; epi.w2 = kda.w2; epi.w = kda.w; epi.x = kda.x; epi.xx = &acc_xx;
  if (VARIANT == 4) tcoo_wg_sweep<PmrRowEpilogue, FIXED>(T, xg, epi, acc, tcoo_lds, red);
  else if (VARIANT == 3) tcoo_sweep(T, xg, epi, acc, tcoo_lds);
  else if (VARIANT == 2) csr_stream_sweep(A, xg, epi, acc, prod);
  else csr_vector_sweep(A, xg, epi, acc);
  acc = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) store_partial(ra.part + blockIdx.x, acc);
  if (kda.do_kd) {                                           // uniform: every workgroup saw the same record
    acc_xx = block_reduce_sum(acc_xx, red);
    if (threadIdx.x == 0) store_partial(kda.red.part + blockIdx.x, acc_xx);
  }
  if (last_block_ticket(ra.counter, ra.tickets, (unsigned)(ra.part - ra.base) + blockIdx.x)) {
    const double vy = sum_partials_agent(ra.base, ra.count, red);
    const double xx = kda.do_kd ? sum_partials_agent(kda.red.base, kda.red.count, red) : 0.0;
    if (threadIdx.x == 0) {
      *ra.tot = vy;
      if (kda.do_kd) *kda.red.tot = xx;
    }
    release_ticket_counter(ra.counter);
  }
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

// y -= (alfa/beta) r2 ; z_{k+1} = minv (.) y ; <y, z_{k+1}>; with test_prev the stopping tests of the previous iteration
// first (its KD rode on the sweep before this kernel and has left <x,x>).
__global__ void __launch_bounds__(HIPEIG_BLOCK)
pmr_kc_kernel(int64_t n, MinresArgs a, const MinresState* __restrict__ Sin, MinresState* __restrict__ Sout,
              const double* __restrict__ r2, const double* __restrict__ minv, double* __restrict__ y,
              double* __restrict__ znext, MinresRed rc, int test_prev) {
  __shared__ double red[4];
  MinresState S = *Sin;
  if (test_prev && !S.done) {
    const double xx = S.itn > 0 ? a.pD[0] : 0.0;
    minres_tests(S, xx, a);
  }
  if (S.done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *Sout = S;
    return;
  }
  S.alfa = a.pA[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) *Sout = S;
  const double nc = -(S.alfa / S.beta);
  const int64_t n2 = n >> 1;
  const double2* r22 = reinterpret_cast<const double2*>(r2);
  const double2* m2 = reinterpret_cast<const double2*>(minv);
  double2* y2 = reinterpret_cast<double2*>(y);
  double2* z2 = reinterpret_cast<double2*>(znext);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  {
    // explicit fused / separately rounded operations: the vector body and the tail round alike
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      const double2 rv = r22[i], mv = m2[i];
      double2 yv = y2[i], zv;
      yv.x = fma(nc, rv.x, yv.x); yv.y = fma(nc, rv.y, yv.y);
      zv.x = mv.x * yv.x; zv.y = mv.y * yv.y;
      y2[i] = yv; z2[i] = zv;
      acc = fma(yv.x, zv.x, acc); acc = fma(yv.y, zv.y, acc);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
      const double yv = fma(nc, r2[n - 1], y[n - 1]);
      const double zv = minv[n - 1] * yv;
      y[n - 1] = yv; znext[n - 1] = zv;
      acc = fma(yv, zv, acc);
    }
  }
  acc = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) store_partial(rc.part + blockIdx.x, acc);
  if (last_block_ticket(rc.counter, rc.tickets, blockIdx.x)) {
    const double yz = sum_partials_agent(rc.base, rc.count, red);
    if (threadIdx.x == 0) *rc.tot = yz;
    release_ticket_counter(rc.counter);
  }
}

// KD as its own kernel: the three-kernel form, and the last iteration of a chunk (nothing follows to ride on).
__global__ void __launch_bounds__(HIPEIG_BLOCK)
pmr_kd_kernel(int64_t n, MinresArgs a, const MinresState* __restrict__ Sin, MinresState* __restrict__ Sout,
              const double* __restrict__ zold, const double* __restrict__ w1, const double* __restrict__ w2,
              double* __restrict__ w, double* __restrict__ x, MinresRed rd) {
  __shared__ double red[4];
  MinresState S = *Sin;
  if (S.done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *Sout = S;
    return;
  }
  const double bb = minres_yy(a);
  const double s_old = S.s;
  minres_advance(S, bb);      // scalar recurrences (every thread, identical)
  if (blockIdx.x == 0 && threadIdx.x == 0) *Sout = S;
  const MinresKd kd{s_old, S.oldeps, S.delta, S.denom, S.phi};
  const int64_t n2 = n >> 1;
  const double2* z2 = reinterpret_cast<const double2*>(zold);
  const double2* w12 = reinterpret_cast<const double2*>(w1);
  const double2* w22 = reinterpret_cast<const double2*>(w2);
  double2* wn2 = reinterpret_cast<double2*>(w);
  double2* x2 = reinterpret_cast<double2*>(x);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    const double2 zv = z2[i], a1 = w12[i], a2 = w22[i];
    double2 xv = x2[i], wn;
    kd.apply(zv.x, a1.x, a2.x, wn.x, xv.x);
    kd.apply(zv.y, a1.y, a2.y, wn.y, xv.y);
    wn2[i] = wn;
    x2[i] = xv;
    acc = fma(xv.x, xv.x, acc); acc = fma(xv.y, xv.y, acc);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    double wn, xv = x[i];
    kd.apply(zold[i], w1[i], w2[i], wn, xv);
    w[i] = wn; x[i] = xv;
    acc = fma(xv, xv, acc);
  }
  acc = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) store_partial(rd.part + blockIdx.x, acc);
  if (last_block_ticket(rd.counter, rd.tickets, blockIdx.x)) {
    const double xx = sum_partials_agent(rd.base, rd.count, red);
    if (threadIdx.x == 0) *rd.tot = xx;
    release_ticket_counter(rd.counter);
  }
}

// End-of-chunk evaluation of the stopping tests (what KA''s prologue would do next).
__global__ void pmr_check_kernel(MinresArgs a, MinresState* __restrict__ S0) {
  MinresState S = *S0;
  const double xx = (S.itn > 0 && !S.done) ? a.pD[0] : 0.0;
  minres_tests(S, xx, a);
  if (threadIdx.x == 0) *S0 = S;
}

extern "C" int hipeig_minres_jacobi(hipeig_ctx* c, hipeig_csr* A, double sigma, double sign, const double* b,
                                    const double* minv, double* x, double rtol, int maxiter, int* info,
                                    double out_stats[8]) {
  HIPEIG_REQUIRE(info != nullptr, "null info");
  HIPEIG_REQUIRE(sign == 1.0 || sign == -1.0, "sign must be +1 or -1");
  HIPEIG_REQUIRE(maxiter >= 1, "maxiter must be positive");
  HIPEIG_REQUIRE(b != x, "x must not alias b");
  HIPEIG_REQUIRE(minv != nullptr && ((uintptr_t)minv & 15) == 0, "minv must be a 16-byte aligned device vector");
  HIPEIG_REQUIRE(!c->collectives, "the preconditioned solve runs on one GPU (whole vectors, no row partition)");
  HIPEIG_REQUIRE(A->nrows == A->ncols && A->row_offset == 0 && A->col_stride == 0, "the preconditioned solve needs a square operator");
  const int64_t n = A->nrows;
  *info = 0;
  if (out_stats) memset(out_stats, 0, 8 * sizeof(double));
  if (n == 0) return 0;

  // workspace: R[3] (r1, r2, y rotate), W[3] (w1, w2, w rotate), the iterate xw and the ring Z[2] of z = minv (.) r2
  if (c->pmr_ws_n < n) {
    if (c->pmr_ws) HIPEIG_CHECK(hipFree(c->pmr_ws));
    c->pmr_ws = nullptr; c->pmr_ws_n = 0;
    const int64_t np = (n + 31) & ~(int64_t)31;
    HIPEIG_CHECK(hipMalloc((void**)&c->pmr_ws, (size_t)np * 9 * sizeof(double)));
    c->pmr_ws_n = n;
  }
  const int64_t npad = (c->pmr_ws_n + 31) & ~(int64_t)31;
  double* ws = c->pmr_ws;
  double* R[3] = {ws, ws + npad, ws + 2 * npad};
  double* W[3] = {ws + 3 * npad, ws + 4 * npad, ws + 5 * npad};
  double* xw = ws + 6 * npad;
  double* Z[2] = {ws + 7 * npad, ws + 8 * npad};
  HIPEIG_CHECK(hipMemsetAsync(W[0], 0, (size_t)npad * 4 * sizeof(double), c->stream));   // W[0..2] and xw

  int per_thread = 24;       // the element-wise grids of minres.hip (measured there)
  if (const char* e = getenv("HIPEIG_MR_PER_THREAD")) per_thread = atoi(e) > 0 ? atoi(e) : 24;     // tuning knob
  const int gE = grid_wide(n, per_thread);
  double* pA = c->d_partials;
  double* pC = c->d_partials + HIPEIG_WIDE_PARTIALS;
  double* pD = c->d_partials + 2 * HIPEIG_WIDE_PARTIALS;
  double* tot = c->d_scalars + SC_MINRES_TOT;                         // [0] <v,y>, [1] <x,x>, [2] <y,z>
  unsigned* cntA = c->d_counters + 0;
  unsigned* cntC = c->d_counters + HIPEIG_TICKET_WORDS;
  unsigned* cntD = c->d_counters + 2 * HIPEIG_TICKET_WORDS;
  HIPEIG_CHECK(hipMemsetAsync(tot, 0, 8 * sizeof(double), c->stream));
  const MinresRed redC{pC, pC, gE, (unsigned)gE, cntC, tot + 2, nullptr};
  const MinresRed redD{pD, pD, gE, (unsigned)gE, cntD, tot + 1, nullptr};

  // start: r2_0 = b, z_0 = minv (.) b, beta1^2 = <b, z_0>
  hipLaunchKernelGGL(pmr_start_kernel, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, b, minv, R[0], Z[0], redC);
  HIPEIG_CHECK(hipGetLastError());
  HIPEIG_CHECK(hipMemcpyAsync(c->h_scalars, tot + 2, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (hipeig_sync_checked(c)) return 4;
  const double bz = c->h_scalars[0];
  HIPEIG_REQUIRE(bz >= 0.0, "indefinite preconditioner: <b, M^-1 b> < 0 (or not a number)");
  if (bz == 0.0) return hipeig_vec_fill(c, x, n, 0.0);            // beta1 == 0: SciPy returns x = 0

  MinresState* h = c->h_mr_state;
  minres_init_state(h, bz);
  MinresState* V = c->d_mr_state;
  HIPEIG_CHECK(hipMemcpyAsync(V, h, sizeof(MinresState), hipMemcpyHostToDevice, c->stream));
  // the pinned record is rewritten by the first chunk's copy-back; the upload above must have read it
  if (hipeig_sync_checked(c)) return 4;

  int variant = hipeig_csr_pick_variant(c, A);
  if (variant < 0) return 1;
  const bool fixed = (variant == 5);                    // TCOO-W with fixed-point accumulators: same structure as 4
  if (fixed) variant = 4;
  HIPEIG_REQUIRE(variant >= 1 && variant <= 4, "unknown sweep layout");
  // column splits serve the slabs of row-partitioned runs, which this path does not take
  HIPEIG_REQUIRE(!(variant == 4 && A->w.csplit > 1), "the preconditioned solve does not take a column-split TCOO-W layout");
  if (variant == 4 && hipeig_tcoow_reserve(c, A)) return 1;
  const CsrView view = hipeig_csr_view(A);
  const BlockedLayout& L = (variant == 4) ? A->w : A->t;
  const TcooView tview = hipeig_tcoo_view(A, L);
  const size_t ldsA = (variant == 4) ? blocked_lds_bytes(A->w, 1) : (variant == 3) ? hipeig_tcoo_lds_bytes(A) : 0;
  if (variant == 4) {
    HIPEIG_CHECK(hipFuncSetAttribute((const void*)pmr_ka_kernel<4, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HIPEIG_TCOOW_LDS_MAX));
    HIPEIG_CHECK(hipFuncSetAttribute((const void*)pmr_ka_kernel<4, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HIPEIG_TCOOW_LDS_MAX));
  }
  if (variant == 3)
    HIPEIG_CHECK(hipFuncSetAttribute((const void*)pmr_ka_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)HIPEIG_TCOO_LDS_MAX));
  const SweepGrid sgA = hipeig_sweep_grid(A, variant);
  const int gA = sgA.wgs, nsweepA = sgA.launches;
  const int nPA = gA * nsweepA;                               // partial <v,y> sums one iteration leaves in pA
  HIPEIG_REQUIRE(nPA <= HIPEIG_WIDE_PARTIALS, "too many sweeps for the partial-sum buffer");
  MinresArgs a;
  a.sigma = sigma; a.sign = sign; a.rtol = rtol; a.maxiter = maxiter;
  a.pA = tot + 0; a.nA = 1;
  a.pD = tot + 1; a.nD = 1;
  a.pC = tot + 2; a.nC = 1; a.sC = 0;

  const char* fk_env = getenv("HIPEIG_MINRES_FUSE_KD");
  const bool fuse_kd = !(fk_env && atoi(fk_env) == 0);

  // The operator sweep of iteration k gathering zk.  `kd`: the pending KD of the previous iteration (do_kd = 0: none),
  // `Sin`: the record the sweep starts from.
  auto enqueue_ka = [&](const double* zk, const double* r1, double* yb, const MinresState* Sin, PmrKdArgs kd) -> int {
    const double* xg = zk;
    TcooView tv = tview;
#define KA_LAUNCH(VAR, FIX, GRID, THREADS, LDS, TV, OFF)                                                            \
    do {                                                                                                            \
      PmrKdArgs kl = kd;                                                                                            \
      kl.red = MinresRed{pD + (OFF), pD, nPA, (unsigned)nPA, cntD, tot + 1, nullptr};                               \
      const MinresRed ra{pA + (OFF), pA, nPA, (unsigned)nPA, cntA, tot + 0, nullptr};                               \
      hipLaunchKernelGGL((pmr_ka_kernel<VAR, FIX>), dim3(GRID), dim3(THREADS), LDS, c->stream, view, TV, xg, a, Sin, V + 1, zk, r1, yb, ra, kl); \
    } while (0)
    if (variant == 4) {
      bool has_last = true;
      int ncombine = 0;
      if (hipeig_tcoow_run_plan(c, A, zk, fixed ? 1 : 0, &tv, &has_last, &xg, &ncombine)) return 4;
      HIPEIG_REQUIRE(has_last && ncombine == 0, "unexpected split sweep");
      for (int sw = 0; sw < nsweepA; ++sw) {
        tv.unit_begin = sw * gA;
        if (fixed) KA_LAUNCH(4, 1, gA, TCOOW_THREADS, ldsA, tv, sw * gA);
        else KA_LAUNCH(4, 0, gA, TCOOW_THREADS, ldsA, tv, sw * gA);
      }
    } else if (variant == 3) {
      for (int sw = 0; sw < nsweepA; ++sw) {       // one launch per sweep; partials side by side
        tv.unit_begin = sw * gA * 4;
        KA_LAUNCH(3, 0, gA, HIPEIG_BLOCK, ldsA, tv, sw * gA);
      }
    } else if (variant == 1) {
      KA_LAUNCH(1, 0, gA, HIPEIG_BLOCK, 0, tview, 0);
    } else {
      KA_LAUNCH(2, 0, gA, HIPEIG_BLOCK, 0, tview, 0);
    }
#undef KA_LAUNCH
    return 0;
  };

  const PmrKdArgs no_kd{0, nullptr, nullptr, nullptr, nullptr, nullptr, MinresRed{nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr}};
  // One iteration's launches (R and W rotate with period 3, Z with period 2).  `first`: nothing is pending from the
  // iteration before (the chunk before ended with a stand-alone KD).
  auto enqueue_iteration = [&](int k, bool first) -> int {
    double* r2 = R[k % 3];
    double* yb = R[(k + 1) % 3];
    double* r1 = R[(k + 2) % 3];
    double* wn = W[k % 3];
    double* w1 = W[(k + 1) % 3];
    double* w2 = W[(k + 2) % 3];
    double* zk = Z[k % 2];
    double* zn = Z[(k + 1) % 2];                 // z_{k-1} until KC'(k) writes z_{k+1} there
    if (fuse_kd) {
      // KD(k-1): w = W[(k-1)%3] from w1 = W[k%3], w2 = W[(k+1)%3] and z_{k-1}
      const bool pending = !first;
      PmrKdArgs kd = no_kd;
      kd.do_kd = pending ? 1 : 0; kd.zold = zn; kd.w1 = wn; kd.w2 = w1; kd.w = w2; kd.x = xw;
      if (enqueue_ka(zk, r1, yb, pending ? V + 2 : V + 0, kd)) return 4;
      hipLaunchKernelGGL(pmr_kc_kernel, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, a, V + 1, V + 2, r2, minv, yb, zn, redC, pending ? 1 : 0);
      return 0;
    }
    if (enqueue_ka(zk, r1, yb, V + 0, no_kd)) return 4;
    hipLaunchKernelGGL(pmr_kc_kernel, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, a, V + 1, V + 2, r2, minv, yb, zn, redC, 0);
    hipLaunchKernelGGL(pmr_kd_kernel, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, a, V + 2, V + 0, zk, w1, w2, wn, xw, redD);
    return 0;
  };
  // The KD of iteration k as its own kernel: the end of a chunk of the two-kernel form.
  auto enqueue_last_kd = [&](int k) {
    if (!fuse_kd) return;
    hipLaunchKernelGGL(pmr_kd_kernel, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, a, V + 2, V + 0, Z[k % 2], W[(k + 1) % 3], W[(k + 2) % 3], W[k % 3], xw, redD);
  };

  // iterations between two looks at the state record (stand-alone KD + check kernel + copy-back + host sync).  Kernels
  // launched past the stopping iteration return at once, so a longer chunk wastes only their launches; a shorter one
  // pays the look more often.  A preconditioned solve of the benchmark class takes 15-40 iterations.
  // Measured (tools/precond_bench.py, profiles/r13_jacobi_minres.jsonl): chunks of 8 / 16 / 32 -> 0.2101 / 0.2106 / 0.2098 ms per
  // iteration at N = 1e6 (19 iterations), 2.174 / 2.166 / 2.169 at N = 1e7 (18): no difference outside the 0.5 % spread of the
  // repetitions, so the middle value stays.
  int chunk = 16;
  if (const char* e = getenv("HIPEIG_PMR_CHUNK")) chunk = atoi(e) > 0 ? atoi(e) : 16;      // tuning knob
  int k = 0;
  while (k < maxiter) {
    const int kend = (k + chunk < maxiter) ? k + chunk : maxiter;
    const int kfirst = k;
    for (; k < kend; ++k) {
      const int rc = enqueue_iteration(k, k == kfirst);
      if (rc) return rc;
    }
    HIPEIG_CHECK(hipGetLastError());
    enqueue_last_kd(kend - 1);
    hipLaunchKernelGGL(pmr_check_kernel, dim3(1), dim3(64), 0, c->stream, a, V + 0);
    HIPEIG_CHECK(hipGetLastError());
    HIPEIG_CHECK(hipMemcpyAsync(h, V, sizeof(MinresState), hipMemcpyDeviceToHost, c->stream));
    if (hipeig_sync_checked(c)) return 4;
    if (h->done) break;
  }
  HIPEIG_REQUIRE(h->done, "MINRES left the iteration loop without a stop code");
  HIPEIG_CHECK(hipMemcpyAsync(x, xw, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  *info = (h->istop == 6) ? maxiter : 0;
  if (out_stats) {
    out_stats[0] = h->itn; out_stats[1] = h->istop; out_stats[2] = h->rnorm; out_stats[3] = h->Anorm;
    out_stats[4] = h->ynorm; out_stats[5] = h->test1; out_stats[6] = h->test2; out_stats[7] = h->Acond;
  }
  return 0;
}
