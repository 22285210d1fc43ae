// Device side of the lock-step block MINRES: the kernels of one block iteration, shared by the plain driver
// (minres_block.hip) and the Jacobi-preconditioned one (minres_block_precond.hip), which runs KA, KD and the
// end-of-chunk check as they stand on other operands.  Recurrences and the order of the kernels: minres_block.hip.
#pragma once
#include "minres_device.h"
#include "block_sweep_launch.h"

// Per-operand sum of `count` partial records for the operand threadIdx.x % K (count == 1: the record
// has already been reduced, e.g. by an all-reduce).
template <int K>
__device__ __forceinline__ double sum_or_value_cols(const double* p, int count, double* lds) {
  if (count == 1) return p[threadIdx.x % K];
  return block_sum_partials_cols<K>(p, count, lds);
}

template <int K>
struct MinresBlockEpilogue {
  double sigma, sign, s, c1;         // s, c1: the scalars of THIS thread's operand (threadIdx.x % 8)
  int use_r1;
  const double* __restrict__ r2l;    // local rows of R2 (v = s*r2)
  const double* __restrict__ r1;
  double* __restrict__ y;
  __device__ __forceinline__ void elem(int64_t r, int j, double sum, double& acc) const {
    const int64_t i = r * K + j;
    const double v = s * r2l[i];
    double yv = sign * (mul_rn(sigma, v) - s * sum);
    if (use_r1) yv -= c1 * r1[i];
    y[i] = yv;
    acc = fma(v, yv, acc);
  }
};

// VARIANT 2: window-blocked (TCOO-B) sweep, 1024 threads; VARIANT 1: row-owner CSR sweep, 256 threads; VARIANT 3: dense
// block sweep over D (dense_device.h), 256 threads.
// LATE_TESTS = 1: the form of a row-partitioned run - the stopping tests of the previous iteration are not evaluated
// here but in KC's prologue, where its <x,x> arrives with the all-reduce that also carries this sweep's <v,y>.
template <int VARIANT, int K, int LATE_TESTS = 0>
__global__ void __launch_bounds__(VARIANT == 2 ? BCOO_THREADS : HIPEIG_BLOCK)
minres_block_ka_kernel(BcooView T, DenseView D, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                       const double* __restrict__ val, int64_t nrows, const double* __restrict__ xg, MinresArgs a,
                       const MinresState* __restrict__ Sin, MinresState* __restrict__ Sout,
                       const double* __restrict__ r2l, const double* __restrict__ r1, double* __restrict__ y,
                       double* __restrict__ partials) {
  __shared__ double red[(VARIANT == 2 ? BCOO_THREADS : HIPEIG_BLOCK) / 64 * K];
  __shared__ double sh_s[K], sh_c1[K];
  __shared__ int sh_use[K], sh_live;
  extern __shared__ double bcoo_lds[];
  const double xx = LATE_TESTS ? 0.0 : sum_or_value_cols<K>(a.pD, a.nD, red);
  if (threadIdx.x == 0) sh_live = 0;
  __syncthreads();
  if (threadIdx.x < K) {
    MinresState S = Sin[threadIdx.x];
    if (!LATE_TESTS) minres_tests(S, (S.itn > 0 && !S.done) ? xx : 0.0, a);
    if (blockIdx.x == 0) Sout[threadIdx.x] = S;
    const int use = (!S.done && S.itn >= 1);
    sh_s[threadIdx.x] = S.done ? 0.0 : S.s;
    sh_c1[threadIdx.x] = use ? S.beta / S.oldb : 0.0;
    sh_use[threadIdx.x] = use;
    if (!S.done) atomicOr(&sh_live, 1);
  }
  __syncthreads();
  if (!sh_live) return;                                   // every column has stopped
  MinresBlockEpilogue<K> epi;
  const int j = threadIdx.x % K;
  epi.sigma = a.sigma; epi.sign = a.sign; epi.s = sh_s[j]; epi.c1 = sh_c1[j]; epi.use_r1 = sh_use[j];
  epi.r2l = r2l; epi.r1 = r1; epi.y = y;
  double acc = 0.0;
  if (VARIANT == 3) dense_block_sweep<K>(D, xg, epi, acc);
  else if (VARIANT == 2) bcoo_wg_sweep<K>(T, xg, epi, acc, bcoo_lds);
  else csr_rowowner_block_sweep<K>(rowptr, col, val, nrows, xg, epi, acc);
  const double tot = block_reduce_cols<K>(acc, red);
  if (threadIdx.x < K) partials[(size_t)blockIdx.x * K + threadIdx.x] = tot;
}

template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
minres_block_kc_kernel(int64_t n, MinresArgs a, const MinresState* __restrict__ Sin, MinresState* __restrict__ Sout,
                       const double* __restrict__ r2, double* __restrict__ y, double* __restrict__ partials, int test_prev) {
  __shared__ double red[HIPEIG_BLOCK / 64 * K];
  __shared__ double sh_c[K];
  const double alfa = sum_or_value_cols<K>(a.pA, a.nA, red);
  const double xx = test_prev ? sum_or_value_cols<K>(a.pD, a.nD, red) : 0.0;
  if (threadIdx.x < K) {
    MinresState S = Sin[threadIdx.x];
    if (test_prev) minres_tests(S, (S.itn > 0 && !S.done) ? xx : 0.0, a);      // row-partitioned run: the tests of the iteration before
    if (!S.done) S.alfa = alfa;
    if (blockIdx.x == 0) Sout[threadIdx.x] = S;
    sh_c[threadIdx.x] = S.done ? 0.0 : S.alfa / S.beta;
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;           // multiple of K/2: operand pair fixed per thread
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j0 = (int)(t0 % (K / 2)) * 2;
  const double c0 = sh_c[j0], c1 = sh_c[j0 + 1];
  const double2* r22 = reinterpret_cast<const double2*>(r2);
  double2* y2 = reinterpret_cast<double2*>(y);
  double a0 = 0.0, a1 = 0.0;
  for (int64_t t = t0; t < n * (K / 2); t += stride) {
    const double2 rv = r22[t];
    double2 yv = y2[t];
    yv.x -= c0 * rv.x; yv.y -= c1 * rv.y;
    y2[t] = yv;
    a0 = fma(yv.x, yv.x, a0); a1 = fma(yv.y, yv.y, a1);
  }
  block_reduce_pairs<K>(a0, a1, red, partials + (size_t)blockIdx.x * K);
}

template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
minres_block_kd_kernel(int64_t n, MinresArgs a, const MinresState* __restrict__ Sin, MinresState* __restrict__ Sout,
                       const double* __restrict__ r2old, const double* __restrict__ w1, const double* __restrict__ w2,
                       double* __restrict__ w, double* __restrict__ x, double* __restrict__ partials) {
  __shared__ double red[HIPEIG_BLOCK / 64 * K];
  __shared__ double sh_sold[K], sh_oldeps[K], sh_delta[K], sh_denom[K], sh_phi[K];
  __shared__ int sh_done[K];
  double bb;
  if (a.sC > 0) {                                       // one share of <y_j,y_j> per rank, in the slots of the operand exchange
    bb = 0.0;
    if (threadIdx.x < K)
      for (int r = 0; r < a.nC; ++r) bb += a.pC[(int64_t)r * a.sC + threadIdx.x];
  } else {
    bb = sum_or_value_cols<K>(a.pC, a.nC, red);
  }
  if (threadIdx.x < K) {
    MinresState S = Sin[threadIdx.x];
    sh_sold[threadIdx.x] = S.s;
    if (!S.done) minres_advance(S, bb);
    if (blockIdx.x == 0) Sout[threadIdx.x] = S;
    sh_oldeps[threadIdx.x] = S.oldeps; sh_delta[threadIdx.x] = S.delta;
    sh_denom[threadIdx.x] = S.denom; sh_phi[threadIdx.x] = S.phi;
    sh_done[threadIdx.x] = S.done;
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j0 = (int)(t0 % (K / 2)) * 2, j1 = j0 + 1;
  const double s0 = sh_sold[j0], e0 = sh_oldeps[j0], d0 = sh_delta[j0], q0 = sh_denom[j0], p0 = sh_phi[j0];
  const double s1 = sh_sold[j1], e1 = sh_oldeps[j1], d1 = sh_delta[j1], q1 = sh_denom[j1], p1 = sh_phi[j1];
  const bool live0 = !sh_done[j0], live1 = !sh_done[j1];
  const double2* r2 = reinterpret_cast<const double2*>(r2old);
  const double2* w12 = reinterpret_cast<const double2*>(w1);
  const double2* w22 = reinterpret_cast<const double2*>(w2);
  double2* wn2 = reinterpret_cast<double2*>(w);
  double2* x2 = reinterpret_cast<double2*>(x);
  double a0 = 0.0, a1 = 0.0;
  if (live0 || live1) {
    for (int64_t t = t0; t < n * (K / 2); t += stride) {
      const double2 rv = r2[t], b1 = w12[t], b2 = w22[t];
      double2 xv = x2[t], wn;
      // a stopped column keeps its iterate; its w is never read again, so what is stored there is irrelevant
      wn.x = (s0 * rv.x - e0 * b1.x - d0 * b2.x) * q0;
      wn.y = (s1 * rv.y - e1 * b1.y - d1 * b2.y) * q1;
      if (live0) xv.x += p0 * wn.x;
      if (live1) xv.y += p1 * wn.y;
      wn2[t] = wn;
      x2[t] = xv;
      a0 = fma(xv.x, xv.x, a0); a1 = fma(xv.y, xv.y, a1);
    }
  }
  block_reduce_pairs<K>(a0, a1, red, partials + (size_t)blockIdx.x * K);
}

// Row-partitioned run: this rank's two records (<v,y> of the sweep, <x,x> of the KD before it) of K sums each, at
// out + 0 / 8, from the partial areas - ONE all-reduce of 16 doubles follows.  One workgroup per record.
template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
sum_two_records_kernel(const double* __restrict__ pA, int nA, const double* __restrict__ pD, int nD, double* __restrict__ out) {
  __shared__ double red[HIPEIG_BLOCK / 64 * K];
  const double* p = blockIdx.x == 0 ? pA : pD;
  const int cnt = blockIdx.x == 0 ? nA : nD;
  const double v = block_sum_partials_cols<K>(p, cnt, red);
  if (threadIdx.x < K) out[blockIdx.x * 8 + threadIdx.x] = v;
}

// End-of-chunk evaluation of the stopping tests (what KA's prologue would do next).
template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
minres_block_check_kernel(MinresArgs a, MinresState* __restrict__ S0) {
  __shared__ double red[HIPEIG_BLOCK / 64 * K];
  const double xx = sum_or_value_cols<K>(a.pD, a.nD, red);
  if (threadIdx.x < K) {
    MinresState S = S0[threadIdx.x];
    minres_tests(S, (S.itn > 0 && !S.done) ? xx : 0.0, a);
    S0[threadIdx.x] = S;
  }
}

// one record of 8 per-operand sums from `count` partial records (distributed path, before the all-reduce)
template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
sum_partials_cols_kernel(const double* __restrict__ p, int count, double* __restrict__ out) {
  __shared__ double red[HIPEIG_BLOCK / 64 * K];
  const double v = block_sum_partials_cols<K>(p, count, red);
  if (threadIdx.x < K) out[threadIdx.x] = v;
}
// ---- the context's workspace of a block solve -------------------------------------------------------------------------
// The recurrence records: a device ring of 3 x 8 and a pinned copy of 8.
static inline int minres_block_reserve_states(hipeig_ctx* c) {
  if (!c->d_mrb_state) {
    HIPEIG_CHECK(hipMalloc((void**)&c->d_mrb_state, 3 * BCOO_KMAX * sizeof(MinresState)));
    HIPEIG_CHECK(hipHostMalloc((void**)&c->h_mrb_state, BCOO_KMAX * sizeof(MinresState), hipHostMallocDefault));
  }
  return 0;
}

// The seven interleaved blocks (r1 r2 y, w1 w2 w, x) of nb doubles each; mrb_ws_n is their stride.
static inline int minres_block_reserve_blocks(hipeig_ctx* c, int64_t nb) {
  if (c->mrb_ws_n < nb) {
    if (c->mrb_ws) HIPEIG_CHECK(hipFree(c->mrb_ws));
    c->mrb_ws = nullptr; c->mrb_ws_n = 0;
    HIPEIG_CHECK(hipMalloc((void**)&c->mrb_ws, (size_t)nb * 7 * sizeof(double)));
    c->mrb_ws_n = nb;
  }
  return 0;
}
