// The orthogonalisation step of the GMRES-type solvers (GCROT): the sequential MGS projection and the Arnoldi step in
// its four forms - one workgroup, fused column kernels, blocked four columns per pass, partitioned with an all-reduce
// per column - with the side streams, the pinned result slots and the batch launch of the split form.
#include "common.h"
#include <math.h>

// ---- sequential MGS projection with the coefficients kept on the device -------------------
// w <- w - sum_j c_j V_j with c_j = <V_j, w_current> taken one column after the other (the
// Arnoldi orthogonalisation of GMRES-type solvers: scipy _fgmres, the loop the reference's
// gcrotmk runs).  Two launches per column and no host round trip: the update kernel sums the
// dot kernel's partials in its prologue (identical value in every workgroup), workgroup 0 stores
// the coefficient, and all m coefficients are copied back once at the end.
// `npart` = 1 means p[0..nval) already holds reduced (all-reduced) values.
// Complex vectors are (re, im) pairs: c = conj(v).w = (vr.wr + vi.wi) + i (vr.wi - vi.wr); partials [re | im], stride g.
template <bool PAIR>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
mgsp_dot_kernel(int64_t n, const double* __restrict__ vr, const double* __restrict__ vi,
                const double* __restrict__ wr, const double* __restrict__ wi, double* __restrict__ partials) {
  __shared__ double lds[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double re = 0.0, im = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (PAIR) {
      const double a = vr[i], b = vi[i], x = wr[i], y = wi[i];
      re = fma(a, x, re); re = fma(b, y, re);
      im = fma(a, y, im); im = fma(-b, x, im);
    } else {
      re = fma(vr[i], wr[i], re);
    }
  }
  re = block_reduce_sum(re, lds);
  if (PAIR) im = block_reduce_sum(im, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = re;
    if (PAIR) partials[gridDim.x + blockIdx.x] = im;
  }
}

template <bool PAIR>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
mgsp_update_kernel(int64_t n, const double* __restrict__ p, int npart, int pstride,
                   const double* __restrict__ vr, const double* __restrict__ vi,
                   double* __restrict__ wr, double* __restrict__ wi, double* __restrict__ coef_out) {
  __shared__ double lds[4];
  const double cr = (npart == 1) ? p[0] : block_sum_partials(p, npart, lds);
  const double ci = !PAIR ? 0.0 : (npart == 1) ? p[1] : block_sum_partials(p + pstride, npart, lds);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    coef_out[0] = cr;
    if (PAIR) coef_out[1] = ci;
  }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (PAIR) {
      const double a = vr[i], b = vi[i];
      wr[i] = wr[i] - (cr * a - ci * b);           // w -= c * v
      wi[i] = wi[i] - (cr * b + ci * a);
    } else {
      wr[i] = fma(-cr, vr[i], wr[i]);
    }
  }
}

__global__ void mgsp_reduce_kernel(const double* __restrict__ p, int npart, int nval, int pstride, double* __restrict__ out) {
  __shared__ double lds[4];
  for (int k = 0; k < nval; ++k) {
    const double v = block_sum_partials(p + (size_t)k * pstride, npart, lds);
    if (threadIdx.x == 0) out[k] = v;
  }
}

// ---- one Arnoldi step of a GMRES-type solver with a single host round trip ---------------------
// scipy _fgmres per inner iteration (the loop behind the reference's gcrotmk, numpyVector.py:161):
//   w_norm = ||w||;  for v in [C..., V...]: h = <v, w>, w -= h v;  h_last = ||w||;  w *= 1/h_last (if finite)
// Everything stays on the device; out = [ ||w||^2 before, h_0 .. h_{m-1}, ||w||^2 after ] comes back in one
// copy (for pairs: complex h as (re, im), so 2m + 2 doubles).  The host takes the square roots, checks the
// breakdown condition and updates its small QR factorisation.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
sumsq_kernel(int64_t n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ partials) {
  __shared__ double lds[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    s = fma(a[i], a[i], s);
    if (b) s = fma(b[i], b[i], s);
  }
  s = block_reduce_sum(s, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// w *= 1/sqrt(ss[0]) when that factor is finite (scipy: alpha = 1/h; if isfinite(alpha): w = scal(alpha, w))
__global__ void __launch_bounds__(HIPEIG_BLOCK)
scale_by_inv_norm_kernel(int64_t n, const double* __restrict__ ss, double* __restrict__ a, double* __restrict__ b) {
  const double alpha = 1.0 / sqrt(ss[0]);
  if (!isfinite(alpha)) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    a[i] *= alpha;
    if (b) b[i] *= alpha;
  }
}

// Single-GPU form of the step: the update with column j and the dot product with column j+1 share one
// pass (and one launch), the two norms ride on the first and the last pass: m + 2 launches and three vector
// passes per column instead of 2m + 5 launches and five passes.  (A partitioned run keeps the unfused path: it
// needs an all-reduce between a dot and its update.  The two paths assign elements to threads differently, so their
// coefficients agree to rounding, not bit for bit.)
// Workspace (doubles, g = grid): two phase buffers of 3g - [re | im | ||w||^2 after] - used alternately, and
// g for ||w||^2 before at offset 6g.
template <bool PAIR>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
arnoldi_first_kernel(int64_t n, const double* __restrict__ a, const double* __restrict__ b,
                     const double* __restrict__ wre, const double* __restrict__ wim, double* __restrict__ partials) {
  __shared__ double lds[4];
  const int g = gridDim.x;
  const int64_t stride = (int64_t)g * blockDim.x;
  double ss = 0.0, re = 0.0, im = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double x = wre[i], y = PAIR ? wim[i] : 0.0;
    ss = fma(x, x, ss);
    if (PAIR) ss = fma(y, y, ss);
    if (a) {
      const double p = a[i], q = PAIR ? b[i] : 0.0;
      re = fma(p, x, re);
      if (PAIR) { re = fma(q, y, re); im = fma(p, y, im); im = fma(-q, x, im); }
    }
  }
  ss = block_reduce_sum(ss, lds);
  re = block_reduce_sum(re, lds);
  if (PAIR) im = block_reduce_sum(im, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = re;
    if (PAIR) partials[g + blockIdx.x] = im;
    partials[6 * g + blockIdx.x] = ss;
  }
}

// The kernel GCROT's orthogonalisation lives in (63 % of the device time of a complex contour solve at N = 1e6,
// rocprofv3 of tools/experiments/gcrot_complex_solve.py).  16-byte accesses, two of them per stream in flight per
// thread and every load of a trip issued before its first store; the column being subtracted is read for the last
// time here (non-temporal), the next column stays cached for the next launch.
typedef double arn_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 arn_ld(const double* p, int64_t i2, bool nt) {
  if (nt) { const arn_d2 v = __builtin_nontemporal_load(reinterpret_cast<const arn_d2*>(p) + i2); return make_double2(v.x, v.y); }
  return reinterpret_cast<const double2*>(p)[i2];
}

template <bool PAIR>
struct ArnoldiLane {                  // one 16-byte slot (two consecutive elements) of every stream
  double2 p, q, a2p, a2q, x, y;
  __device__ __forceinline__ void load(int64_t i2, const double* a, const double* b, const double* a2, const double* b2,
                                       const double* wre, const double* wim, int last) {
    p = arn_ld(a, i2, true);
    if (PAIR) q = arn_ld(b, i2, true);
    if (!last) { a2p = arn_ld(a2, i2, false); if (PAIR) a2q = arn_ld(b2, i2, false); }
    x = arn_ld(wre, i2, false);
    if (PAIR) y = arn_ld(wim, i2, false);
  }
  __device__ __forceinline__ void update(double cr, double ci) {
    if (PAIR) {
      x.x = x.x - (cr * p.x - ci * q.x); y.x = y.x - (cr * q.x + ci * p.x);       // w -= c * v
      x.y = x.y - (cr * p.y - ci * q.y); y.y = y.y - (cr * q.y + ci * p.y);
    } else {
      x.x = fma(-cr, p.x, x.x); x.y = fma(-cr, p.y, x.y);
    }
  }
  __device__ __forceinline__ void store(int64_t i2, double* wre, double* wim) const {
    reinterpret_cast<double2*>(wre)[i2] = x;
    if (PAIR) reinterpret_cast<double2*>(wim)[i2] = y;
  }
  __device__ __forceinline__ void accumulate(int last, double& re, double& im, double& ss) const {
    if (last) {
      ss = fma(x.x, x.x, ss); ss = fma(x.y, x.y, ss);
      if (PAIR) { ss = fma(y.x, y.x, ss); ss = fma(y.y, y.y, ss); }
    } else {
      re = fma(a2p.x, x.x, re); re = fma(a2p.y, x.y, re);
      if (PAIR) {
        re = fma(a2q.x, y.x, re); re = fma(a2q.y, y.y, re);
        im = fma(a2p.x, y.x, im); im = fma(-a2q.x, x.x, im);
        im = fma(a2p.y, y.y, im); im = fma(-a2q.y, x.y, im);
      }
    }
  }
};

template <bool PAIR>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
arnoldi_column_kernel(int64_t n, const double* __restrict__ pin, double* __restrict__ pout,
                      const double* __restrict__ a, const double* __restrict__ b,
                      const double* __restrict__ a2, const double* __restrict__ b2, int last,
                      double* __restrict__ wre, double* __restrict__ wim, double* __restrict__ coef_out) {
  __shared__ double lds[4];
  const int g = gridDim.x;
  const int64_t n2 = n >> 1;
  const int64_t stride = (int64_t)g * blockDim.x;
  // the first trip's loads do not depend on the coefficient: issue them BEFORE the prologue reduces the previous
  // launch's partial sums, so that the reduction (L2 reads + two barriers) hides behind their HBM latency
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  ArnoldiLane<PAIR> L0, L1;
  bool has0 = i < n2, has1 = i + stride < n2;
  if (has0) L0.load(i, a, b, a2, b2, wre, wim, last);
  if (has1) L1.load(i + stride, a, b, a2, b2, wre, wim, last);
  const double cr = block_sum_partials(pin, g, lds);
  const double ci = PAIR ? block_sum_partials(pin + g, g, lds) : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    coef_out[0] = cr;
    if (PAIR) coef_out[1] = ci;
  }
  double re = 0.0, im = 0.0, ss = 0.0;
  while (has0) {
    L0.update(cr, ci);
    L0.store(i, wre, wim);
    L0.accumulate(last, re, im, ss);
    if (has1) {
      L1.update(cr, ci);
      L1.store(i + stride, wre, wim);
      L1.accumulate(last, re, im, ss);
    }
    i += 2 * stride;
    has0 = i < n2; has1 = i + stride < n2;
    if (has0) L0.load(i, a, b, a2, b2, wre, wim, last);
    if (has1) L1.load(i + stride, a, b, a2, b2, wre, wim, last);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {           // odd length: the last element
    const int64_t i = n - 1;
    double x, y = 0.0;
    if (PAIR) {
      const double p = a[i], q = b[i];
      x = wre[i] - (cr * p - ci * q);
      y = wim[i] - (cr * q + ci * p);
      wre[i] = x; wim[i] = y;
    } else {
      x = fma(-cr, a[i], wre[i]);
      wre[i] = x;
    }
    if (last) {
      ss = fma(x, x, ss);
      if (PAIR) ss = fma(y, y, ss);
    } else {
      const double p = a2[i], q = PAIR ? b2[i] : 0.0;
      re = fma(p, x, re);
      if (PAIR) { re = fma(q, y, re); im = fma(p, y, im); im = fma(-q, x, im); }
    }
  }
  if (last) {
    ss = block_reduce_sum(ss, lds);
    if (threadIdx.x == 0) pout[2 * g + blockIdx.x] = ss;
  } else {
    re = block_reduce_sum(re, lds);
    if (PAIR) im = block_reduce_sum(im, lds);
    if (threadIdx.x == 0) {
      pout[blockIdx.x] = re;
      if (PAIR) pout[g + blockIdx.x] = im;
    }
  }
}

// ||w||^2 before / after to dres, then w *= 1/||w|| when that factor is finite
__global__ void __launch_bounds__(HIPEIG_BLOCK)
arnoldi_last_kernel(int64_t n, const double* __restrict__ p_before, const double* __restrict__ p_after,
                    double* __restrict__ wre, double* __restrict__ wim, double* __restrict__ d_before,
                    double* __restrict__ d_after) {
  __shared__ double lds[4];
  const int g = gridDim.x;
  const double sb = block_sum_partials(p_before, g, lds);
  const double sa = block_sum_partials(p_after, g, lds);
  if (blockIdx.x == 0 && threadIdx.x == 0) { *d_before = sb; *d_after = sa; }
  const double alpha = 1.0 / sqrt(sa);
  if (!isfinite(alpha)) return;
  const int64_t stride = (int64_t)g * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    wre[i] *= alpha;
    if (wim) wim[i] *= alpha;
  }
}

// Short vectors (the reference's own problem sizes: n = 100 ... 4000): the whole step - norm, the sequential sweep over
// all m columns, norm, scaling - in ONE workgroup and ONE launch, the vector being orthogonalised held in registers.
// At these lengths a launch per column is pure dispatch latency (~5 us each, 20-60 columns per step); a workgroup-wide
// reduction costs two barriers.  Same order of operations as the column kernels (sequential MGS, SciPy's _fgmres).
#define ARN_SMALL_THREADS 1024
#define ARN_SMALL_E 8                       // elements per thread: n <= 8192 (16 would spill the pair form)
#define ARN_SMALL_MAXCOLS 64
struct ArnSmallCols { const double* re[ARN_SMALL_MAXCOLS]; const double* im[ARN_SMALL_MAXCOLS]; };

// sums of (a, b) over the workgroup, returned to every thread; fixed tree.  lds: 2 x 16 doubles
__device__ __forceinline__ void arn_small_reduce2(double& a, double& b, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();                                   // the previous reduction's readers are done with lds
  if (lane == 0) { lds[wid] = a; lds[16 + wid] = b; }
  __syncthreads();
  a = lds[0]; b = lds[16];
  for (int w = 1; w < ARN_SMALL_THREADS / 64; ++w) { a += lds[w]; b += lds[16 + w]; }
}

// column tables of the step: in the kernel arguments (one step per launch) or in LDS (one step per WORKGROUP, below)
struct ArnColsArg {
  const ArnSmallCols& V;
  __device__ __forceinline__ const double* re(int j) const { return V.re[j]; }
  __device__ __forceinline__ const double* im(int j) const { return V.im[j]; }
};
struct ArnColsLds {
  const double* const* tab;                          // [2][ARN_SMALL_MAXCOLS]
  __device__ __forceinline__ const double* re(int j) const { return tab[j]; }
  __device__ __forceinline__ const double* im(int j) const { return tab[ARN_SMALL_MAXCOLS + j]; }
};

template <bool PAIR, class Cols>
__device__ __forceinline__ void arnoldi_small_body(int n, int m, const Cols& V, double* __restrict__ wre, double* __restrict__ wim,
                                                   double* __restrict__ dres, double* lds) {
  const int W = PAIR ? 2 : 1;
  double x[ARN_SMALL_E], y[ARN_SMALL_E];
  double ss = 0.0, zero = 0.0;
#pragma unroll
  for (int e = 0; e < ARN_SMALL_E; ++e) {
    const int i = threadIdx.x + e * ARN_SMALL_THREADS;
    x[e] = i < n ? wre[i] : 0.0;
    y[e] = (PAIR && i < n) ? wim[i] : 0.0;
    ss = fma(x[e], x[e], ss);
    if (PAIR) ss = fma(y[e], y[e], ss);
  }
  arn_small_reduce2(ss, zero, lds);
  if (threadIdx.x == 0) dres[0] = ss;
  for (int j = 0; j < m; ++j) {
    const double* __restrict__ vr = V.re(j);
    const double* __restrict__ vi = PAIR ? V.im(j) : nullptr;
    double re = 0.0, im = 0.0;
#pragma unroll
    for (int e = 0; e < ARN_SMALL_E; ++e) {
      const int i = threadIdx.x + e * ARN_SMALL_THREADS;
      const double p = i < n ? vr[i] : 0.0;
      const double q = (PAIR && i < n) ? vi[i] : 0.0;
      re = fma(p, x[e], re);
      if (PAIR) { re = fma(q, y[e], re); im = fma(p, y[e], im); im = fma(-q, x[e], im); }
    }
    arn_small_reduce2(re, im, lds);                  // c = conj(v) . w, the same value in every thread
    if (threadIdx.x == 0) { dres[1 + W * j] = re; if (PAIR) dres[2 + W * j] = im; }
#pragma unroll
    for (int e = 0; e < ARN_SMALL_E; ++e) {          // the column again (L1 / L2 at these lengths): registers hold only w
      const int i = threadIdx.x + e * ARN_SMALL_THREADS;
      const double p = i < n ? vr[i] : 0.0;
      const double q = (PAIR && i < n) ? vi[i] : 0.0;
      if (PAIR) {
        const double nx = x[e] - (re * p - im * q);              // w -= c * v
        y[e] = y[e] - (re * q + im * p);
        x[e] = nx;
      } else {
        x[e] = fma(-re, p, x[e]);
      }
    }
  }
  double sa = 0.0;
  zero = 0.0;
#pragma unroll
  for (int e = 0; e < ARN_SMALL_E; ++e) { sa = fma(x[e], x[e], sa); if (PAIR) sa = fma(y[e], y[e], sa); }
  arn_small_reduce2(sa, zero, lds);
  if (threadIdx.x == 0) dres[1 + W * m] = sa;
  const double alpha = 1.0 / sqrt(sa);
  const bool scale = isfinite(alpha);
#pragma unroll
  for (int e = 0; e < ARN_SMALL_E; ++e) {
    const int i = threadIdx.x + e * ARN_SMALL_THREADS;
    if (i < n) {
      wre[i] = scale ? x[e] * alpha : x[e];
      if (PAIR) wim[i] = scale ? y[e] * alpha : y[e];
    }
  }
}

template <bool PAIR>
__global__ void __launch_bounds__(ARN_SMALL_THREADS)
arnoldi_small_kernel(int n, int m, ArnSmallCols V, double* __restrict__ wre, double* __restrict__ wim, double* __restrict__ dres) {
  __shared__ double lds[32];
  arnoldi_small_body<PAIR>(n, m, ArnColsArg{V}, wre, wim, dres, lds);
}

// Several independent steps in ONE launch, a workgroup each (the right-hand sides of a lock-step block solve at lengths
// where a step is a single workgroup: launched one after the other they would use one CU of 256 in turn).  The items sit
// in pinned host memory the device reads directly; each workgroup copies its column table to LDS and writes its scalars
// straight into its pinned result slot - no copy in either direction is enqueued.
struct ArnBatchItem {
  int m, pad;
  double* wre; double* wim;
  const double* re[ARN_SMALL_MAXCOLS];
  const double* im[ARN_SMALL_MAXCOLS];
};
#define ARN_SLOT_DOUBLES SH_SLOT_LEN
static_assert(SH_NSLOTS == 16, "ctx->ev_slot[16] and the slot checks of the split form");

template <bool PAIR>
__global__ void __launch_bounds__(ARN_SMALL_THREADS)
arnoldi_small_batch_kernel(int n, const ArnBatchItem* __restrict__ items, double* __restrict__ slots) {
  __shared__ double lds[32];
  __shared__ const double* tab[2 * ARN_SMALL_MAXCOLS];
  const ArnBatchItem* it = items + blockIdx.x;
  const int m = it->m;
  for (int j = threadIdx.x; j < m; j += ARN_SMALL_THREADS) { tab[j] = it->re[j]; tab[ARN_SMALL_MAXCOLS + j] = it->im[j]; }
  double* wre = it->wre;
  double* wim = it->wim;
  __syncthreads();
  arnoldi_small_body<PAIR>(n, m, ArnColsLds{tab}, wre, wim, slots + (size_t)blockIdx.x * ARN_SLOT_DOUBLES, lds);
}

// the step as ONE workgroup (arnoldi_small_kernel): it only WRITES its scalars, so they can go straight to mapped host memory
template <bool PAIR>
static int arnoldi_small(hipeig_ctx* c, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                         double* wre, double* wim, double* dres) {
  ArnSmallCols V;
  for (int j = 0; j < ARN_SMALL_MAXCOLS; ++j) {
    V.re[j] = j < m ? Vre[j] : nullptr;
    V.im[j] = (PAIR && j < m) ? Vim[j] : nullptr;
  }
  hipLaunchKernelGGL((arnoldi_small_kernel<PAIR>), dim3(1), dim3(ARN_SMALL_THREADS), 0, c->stream, (int)n, m, V, wre, wim, dres);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

template <bool PAIR>
static int arnoldi_columns(hipeig_ctx* c, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                           double* wre, double* wim, double* dres) {
  const int g = grid_for(n, 4);
  const int W = PAIR ? 2 : 1;
  double* P = c->d_partials;
  hipLaunchKernelGGL((arnoldi_first_kernel<PAIR>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n,
                     m > 0 ? Vre[0] : nullptr, (PAIR && m > 0) ? Vim[0] : nullptr, wre, wim, P);
  for (int j = 0; j < m; ++j) {
    const int last = (j + 1 == m);
    hipLaunchKernelGGL((arnoldi_column_kernel<PAIR>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n,
                       P + (size_t)(j & 1) * 3 * g, P + (size_t)((j + 1) & 1) * 3 * g, Vre[j], PAIR ? Vim[j] : nullptr,
                       last ? nullptr : Vre[j + 1], (PAIR && !last) ? Vim[j + 1] : nullptr, last, wre, wim, dres + 1 + W * j);
  }
  const double* p_after = (m == 0) ? P + 6 * g : P + (size_t)(m & 1) * 3 * g + 2 * g;
  hipLaunchKernelGGL(arnoldi_last_kernel, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, P + 6 * g, p_after, wre, wim,
                     dres, dres + 1 + W * m);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// ---- several columns per pass (option; hipeig_arnoldi_step_p) ------------------------------------------------------
// The sweep above reads w once per column.  Here a pass applies the updates of a whole BLOCK of P = 4 columns and, in
// the same pass, forms everything the next block needs: its dot products with the updated w AND the Gram entries
// G_kl = <V_k, V_l> (l < k) of its own columns, from which the coefficients of the sequential sweep follow exactly,
//   h_0 = <V_0, w>,   h_k = <V_k, w - sum_{l<k} h_l V_l> = <V_k, w> - sum_{l<k} h_l G_kl .
// Algebraically this IS the modified Gram-Schmidt sweep of scipy's _fgmres, column after column; it differs in
// rounding (the G terms are accumulated sums instead of being folded into w element by element), which is why it is an
// option and the one-column form stays the default (iteration-count parity with scipy.sparse.linalg.gcrotmk).
// Traffic per column: (2P + 2) / P = 2.5 vector streams instead of 4, and a launch per FOUR columns.
// All sums finish in the kernel's last workgroup (common.h), so the next launch's prologue reads ~20 doubles.
#ifndef ARN_P
#define ARN_P 4
#endif
#ifndef ARN_BLOCK_THREADS
#define ARN_BLOCK_THREADS 256          // threads per workgroup of the blocked sweep (build-time knob)
#endif
struct ArnBlockCols { const double* re[ARN_P]; const double* im[ARN_P]; };
template <bool PAIR> struct ArnBlockShape {
  static constexpr int W = PAIR ? 2 : 1;
  static constexpr int NG = W * ARN_P;                         // dot products of a block with w
  static constexpr int NGRAM = W * ARN_P * (ARN_P - 1) / 2;    // lower triangle of the block's Gram matrix
  static constexpr int NV = NG + NGRAM + 1;                    // + one sum of squares
};

template <bool PAIR>
__global__ void __launch_bounds__(ARN_BLOCK_THREADS)
arnoldi_block_kernel(int64_t n, const double* __restrict__ tin, int nb_in, ArnBlockCols cur, int nb_next, ArnBlockCols nxt,
                     int want_ss, double* __restrict__ wre, double* __restrict__ wim, double* __restrict__ coef_out,
                     double* __restrict__ partials, unsigned* counters, double* __restrict__ tout, double* __restrict__ ss_out) {
  using Sh = ArnBlockShape<PAIR>;
  constexpr int W = Sh::W, P = ARN_P;
  __shared__ double lds[4];
  // coefficients of the block being applied, from the sums the previous launch left (identical in every thread)
  double hr[P], hi[P];
#pragma unroll
  for (int k = 0; k < P; ++k) { hr[k] = 0.0; hi[k] = 0.0; }
  if (nb_in > 0) {
    int gi = Sh::NG;                                           // Gram entries follow the dots: (k, l) for k = 1.., l < k
#pragma unroll
    for (int k = 0; k < P; ++k) {
      if (k < nb_in) {
        double cr = tin[W * k], ci = PAIR ? tin[W * k + 1] : 0.0;
#pragma unroll
        for (int l = 0; l < k; ++l) {
          const double gr = tin[gi + W * l], gim = PAIR ? tin[gi + W * l + 1] : 0.0;
          cr -= hr[l] * gr - hi[l] * gim;                      // h_l * G_kl
          if (PAIR) ci -= hr[l] * gim + hi[l] * gr;
        }
        hr[k] = cr; hi[k] = ci;
      }
      gi += W * k;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
      for (int k = 0; k < nb_in; ++k) { coef_out[W * k] = hr[k]; if (PAIR) coef_out[W * k + 1] = hi[k]; }
  }
  double acc[Sh::NV];
#pragma unroll
  for (int v = 0; v < Sh::NV; ++v) acc[v] = 0.0;
  const int64_t n2 = n >> 1;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    double2 cp[P], cq[P], np_[P], nq[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      if (k < nb_in) { cp[k] = arn_ld(cur.re[k], i, true); if (PAIR) cq[k] = arn_ld(cur.im[k], i, true); }
      if (k < nb_next) { np_[k] = arn_ld(nxt.re[k], i, false); if (PAIR) nq[k] = arn_ld(nxt.im[k], i, false); }
    }
    double2 x = arn_ld(wre, i, false), y = PAIR ? arn_ld(wim, i, false) : make_double2(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < P; ++k) {
      if (k < nb_in) {
        if (PAIR) {
          x.x -= hr[k] * cp[k].x - hi[k] * cq[k].x; y.x -= hr[k] * cq[k].x + hi[k] * cp[k].x;      // w -= h * v
          x.y -= hr[k] * cp[k].y - hi[k] * cq[k].y; y.y -= hr[k] * cq[k].y + hi[k] * cp[k].y;
        } else {
          x.x = fma(-hr[k], cp[k].x, x.x); x.y = fma(-hr[k], cp[k].y, x.y);
        }
      }
    }
    if (nb_in > 0) {
      reinterpret_cast<double2*>(wre)[i] = x;
      if (PAIR) reinterpret_cast<double2*>(wim)[i] = y;
    }
    int gi = Sh::NG;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      if (k < nb_next) {
        // conj(v_k) . w
        acc[W * k] = fma(np_[k].x, x.x, acc[W * k]); acc[W * k] = fma(np_[k].y, x.y, acc[W * k]);
        if (PAIR) {
          acc[W * k] = fma(nq[k].x, y.x, acc[W * k]); acc[W * k] = fma(nq[k].y, y.y, acc[W * k]);
          acc[W * k + 1] = fma(np_[k].x, y.x, acc[W * k + 1]); acc[W * k + 1] = fma(-nq[k].x, x.x, acc[W * k + 1]);
          acc[W * k + 1] = fma(np_[k].y, y.y, acc[W * k + 1]); acc[W * k + 1] = fma(-nq[k].y, x.y, acc[W * k + 1]);
        }
#pragma unroll
        for (int l = 0; l < k; ++l) {                          // conj(v_k) . v_l
          double& gr = acc[gi + W * l];
          gr = fma(np_[k].x, np_[l].x, gr); gr = fma(np_[k].y, np_[l].y, gr);
          if (PAIR) {
            gr = fma(nq[k].x, nq[l].x, gr); gr = fma(nq[k].y, nq[l].y, gr);
            double& gm = acc[gi + W * l + 1];
            gm = fma(np_[k].x, nq[l].x, gm); gm = fma(-nq[k].x, np_[l].x, gm);
            gm = fma(np_[k].y, nq[l].y, gm); gm = fma(-nq[k].y, np_[l].y, gm);
          }
        }
      }
      gi += W * k;
    }
    if (want_ss) {
      double& ss = acc[Sh::NV - 1];
      ss = fma(x.x, x.x, ss); ss = fma(x.y, x.y, ss);
      if (PAIR) { ss = fma(y.x, y.x, ss); ss = fma(y.y, y.y, ss); }
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {         // odd length: the last element (loops unrolled: acc stays in registers)
    const int64_t i = n - 1;
    double x = wre[i], y = PAIR ? wim[i] : 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      if (k < nb_in) {
        const double p = cur.re[k][i], q = PAIR ? cur.im[k][i] : 0.0;
        const double nx = x - (hr[k] * p - hi[k] * q);
        y = y - (hr[k] * q + hi[k] * p);
        x = nx;
      }
    }
    if (nb_in > 0) { wre[i] = x; if (PAIR) wim[i] = y; }
    double pn[P], qn[P];
#pragma unroll
    for (int k = 0; k < P; ++k) { pn[k] = k < nb_next ? nxt.re[k][i] : 0.0; qn[k] = (PAIR && k < nb_next) ? nxt.im[k][i] : 0.0; }
    int gi = Sh::NG;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      if (k < nb_next) {
        acc[W * k] = fma(pn[k], x, acc[W * k]);
        if (PAIR) { acc[W * k] = fma(qn[k], y, acc[W * k]); acc[W * k + 1] = fma(pn[k], y, acc[W * k + 1]); acc[W * k + 1] = fma(-qn[k], x, acc[W * k + 1]); }
#pragma unroll
        for (int l = 0; l < k; ++l) {
          acc[gi + W * l] = fma(pn[k], pn[l], acc[gi + W * l]);
          if (PAIR) {
            acc[gi + W * l] = fma(qn[k], qn[l], acc[gi + W * l]);
            acc[gi + W * l + 1] = fma(pn[k], qn[l], acc[gi + W * l + 1]); acc[gi + W * l + 1] = fma(-qn[k], pn[l], acc[gi + W * l + 1]);
          }
        }
      }
      gi += W * k;
    }
    if (want_ss) { acc[Sh::NV - 1] = fma(x, x, acc[Sh::NV - 1]); if (PAIR) acc[Sh::NV - 1] = fma(y, y, acc[Sh::NV - 1]); }
  }
  // all NV sums of the workgroup through ONE LDS stage (wave shuffles, one barrier, thread v adds the four wave sums)
  const int G = gridDim.x;
  __shared__ double red[Sh::NV][ARN_BLOCK_THREADS / 64];
  {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < Sh::NV; ++v) {
      const double r = wave_reduce_sum(acc[v]);
      if (lane == 0) red[v][wid] = r;
    }
    __syncthreads();
    if ((int)threadIdx.x < Sh::NV) {
      double t = red[threadIdx.x][0];
      for (int w = 1; w < ARN_BLOCK_THREADS / 64; ++w) t += red[threadIdx.x][w];
      store_partial(partials + (size_t)threadIdx.x * G + blockIdx.x, t);
    }
  }
  if (last_block_ticket(counters, (unsigned)G, blockIdx.x)) {
    // the NV totals side by side: 8 lanes per value (8 x 21 = 168 <= 256 threads), lane k adds the partials k, k + 8, ...
    // in ascending order and the 8 lane sums are folded in a fixed tree
    const int v = threadIdx.x >> 3, k = threadIdx.x & 7;
    double a = 0.0;
    if (v < Sh::NV)
      for (int i = k; i < G; i += 8) a += __hip_atomic_load(partials + (size_t)v * G + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a += __shfl_xor(a, 4, 64); a += __shfl_xor(a, 2, 64); a += __shfl_xor(a, 1, 64);
    if (v < Sh::NV && k == 0) {
      tout[v] = a;
      if (v == Sh::NV - 1 && ss_out) *ss_out = a;
    }
    release_ticket_counter(counters);
  }
}

// Workspace of one blocked Arnoldi step: a stream and what the step keeps per stream (so that the steps of different
// right-hand sides can run on different streams at once).
struct ArnSpace {
  hipStream_t stream;
  double* partials;          // Sh::NV areas of <= 8192 doubles
  double* tot;               // two total records of 32 doubles, used alternately
  unsigned* cnt;             // ticket counters (zero between kernels)
};

static ArnSpace arnoldi_main_space(hipeig_ctx* c) {
  return ArnSpace{c->stream, c->d_partials, c->d_scalars + SC_ARN_TOTALS, c->d_counters + 3 * HIPEIG_TICKET_WORDS};
}

#define ARN_SIDE_PARTIALS (32 * 8192)      // doubles per side stream: >= Sh::NV (21) areas of 8192
#define ARN_SIDE_DOUBLES (ARN_SIDE_PARTIALS + 64 + 128)      // + two total records + the step's result record

// Everything the split form holds beyond the context's own buffers: side streams, their events and workspaces, the batch
// items.  Afterwards arn_nstreams == 0 means "nothing held" again.  (Context destruction, and a failure halfway through
// arnoldi_side_streams.)
void arnoldi_release(hipeig_ctx* c) {
  for (int k = 0; k < 16; ++k) {
    if (c->arn_stream[k]) { (void)hipStreamSynchronize(c->arn_stream[k]); (void)hipStreamDestroy(c->arn_stream[k]); }
    if (c->ev_arn_in[k]) (void)hipEventDestroy(c->ev_arn_in[k]);
    c->arn_stream[k] = nullptr;
    c->ev_arn_in[k] = nullptr;
  }
  if (c->d_arn_ws) (void)hipFree(c->d_arn_ws);
  if (c->d_arn_cnt) (void)hipFree(c->d_arn_cnt);
  if (c->h_arn_items) (void)hipHostFree(c->h_arn_items);
  c->d_arn_ws = nullptr;
  c->d_arn_cnt = nullptr;
  c->h_arn_items = c->d_arn_items = nullptr;
  c->arn_nstreams = 0;
}

// The side streams are created on first use: HIPEIG_ARNOLDI_STREAMS of them (1..16; 1 = none, everything on the compute stream).
// Measured (tools/experiments/gcrot_block_solve.py, the 16 solves of one contour point, 4-column sweeps): 1 / 2 / 4 / 8 / 16
// streams at N = 1e6 8.78 / 8.70 / 7.13 / 6.70 / 6.64 s (6: 7.26; with GPU_MAX_HW_QUEUES=8 instead of the runtime's 4: 7.1-7.3),
// at N = 4e6 22.8 / - / 21.9 s, at N = 1e7 37.9 / - / 36.3 / 36.2 s - a sweep of 160 MB does not fill the chip at N = 1e6 (4.3 TB/s:
// launch ramp, the ticket tail), several of them from different right-hand sides do; identical coefficients and iteration counts.
static int arnoldi_side_streams(hipeig_ctx* c) {
  if (c->arn_nstreams) return 0;
  int ns = 8;
  if (const char* e = getenv("HIPEIG_ARNOLDI_STREAMS")) ns = atoi(e);
  if (ns < 1) ns = 1;
  if (ns > 16) ns = 16;
  if (ns > 1) {
    // all or nothing: a failure halfway releases what was created, so that arn_nstreams == 0 again means "nothing held"
    // and the next call starts from scratch instead of allocating over live workspaces
    hipError_t e = hipMalloc((void**)&c->d_arn_ws, (size_t)ns * ARN_SIDE_DOUBLES * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_arn_cnt, (size_t)ns * HIPEIG_TICKET_WORDS * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(c->d_arn_cnt, 0, (size_t)ns * HIPEIG_TICKET_WORDS * sizeof(unsigned));
    for (int k = 0; k < ns && e == hipSuccess; ++k) e = hipStreamCreateWithFlags(&c->arn_stream[k], hipStreamNonBlocking);
    for (int k = 0; k < 16 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&c->ev_arn_in[k], hipEventDisableTiming);
    if (e != hipSuccess) {
      hipeig_set_error("%s:%d: creating %d Arnoldi side streams -> %s", __FILE__, __LINE__, ns, hipGetErrorString(e));
      arnoldi_release(c);
      return 1;
    }
  }
  c->arn_nstreams = ns;
  return 0;
}

template <bool PAIR>
static int arnoldi_blocked(hipeig_ctx* c, const ArnSpace& sp, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                           double* wre, double* wim, double* dres) {
  using Sh = ArnBlockShape<PAIR>;
  constexpr int W = Sh::W;
  // One workgroup per CU, whatever the length (measured, tools/experiments/arnoldi_bench.py, 28 complex columns: N = 1e7
  // 145 / 113 / 98 / 89 / 82 us per column at 4883 / 2441 / 1220 / 610 / 244 workgroups, N = 1e6 15.6 / 12.8 at 488 / 244; the
  // sequential sweep: 116 / 13.9).  A pass reads 18 streams at once; with one workgroup per CU the whole chip walks through
  // each of them as one narrow front.
  int g = c->num_cu;
  if (const char* e = getenv("HIPEIG_ARNOLDI_PER_THREAD")) g = grid_wide(n, atoi(e) > 0 ? atoi(e) : 16);      // tuning knob (elements per thread)
  if (const char* e = getenv("HIPEIG_ARNOLDI_WGS")) g = atoi(e) > 0 ? atoi(e) : g;                              // tuning knob (workgroups)
  if ((int64_t)g * ARN_BLOCK_THREADS * 2 > n) g = (int)((n / 2 + ARN_BLOCK_THREADS - 1) / ARN_BLOCK_THREADS);
  if (g < 1) g = 1;
  if (g > 8192) g = 8192;                                      // Sh::NV partial areas of g doubles each
  double* P0 = sp.partials;
  double* tot = sp.tot;                                        // two total records of <= 32 doubles, used alternately
  unsigned* cnt = sp.cnt;
  auto cols = [&](int b0, ArnBlockCols* out) -> int {
    int nb = m - b0;
    if (nb > ARN_P) nb = ARN_P;
    if (nb < 0) nb = 0;
    for (int k = 0; k < ARN_P; ++k) {
      out->re[k] = k < nb ? Vre[b0 + k] : nullptr;
      out->im[k] = (PAIR && k < nb) ? Vim[b0 + k] : nullptr;
    }
    return nb;
  };
  ArnBlockCols none, cur, nxt;
  cols(m, &none);
  int nb_next = cols(0, &nxt);
  // first pass: ||w||^2 before and everything block 0 needs (no update); with m == 0 it is also ||w||^2 after
  hipLaunchKernelGGL((arnoldi_block_kernel<PAIR>), dim3(g), dim3(ARN_BLOCK_THREADS), 0, sp.stream, n, (const double*)nullptr, 0, none,
                     nb_next, nxt, 1, wre, wim, (double*)nullptr, P0, cnt, tot, dres);
  int flip = 0;
  for (int b0 = 0; b0 < m; b0 += ARN_P) {
    cur = nxt;
    const int nb_in = nb_next;
    nb_next = cols(b0 + ARN_P, &nxt);
    const int last = (nb_next == 0);
    hipLaunchKernelGGL((arnoldi_block_kernel<PAIR>), dim3(g), dim3(ARN_BLOCK_THREADS), 0, sp.stream, n, tot + 32 * flip, nb_in, cur,
                       nb_next, nxt, last, wre, wim, dres + 1 + W * b0, P0, cnt, tot + 32 * (flip ^ 1),
                       last ? dres + 1 + W * m : (double*)nullptr);
    flip ^= 1;
  }
  if (m == 0)
    HIPEIG_CHECK(hipMemcpyAsync(dres + 1, dres, sizeof(double), hipMemcpyDeviceToDevice, sp.stream));
  hipLaunchKernelGGL(scale_by_inv_norm_kernel, dim3(grid_stream(n)), dim3(HIPEIG_BLOCK), 0, sp.stream, n, dres + 1 + W * m, wre, wim);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

static int arnoldi_sumsq(hipeig_ctx* c, int64_t n, const double* a, const double* b, int g, double* dst) {
  hipLaunchKernelGGL(sumsq_kernel, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, a, b, c->d_partials);
  hipLaunchKernelGGL(mgsp_reduce_kernel, dim3(1), dim3(HIPEIG_BLOCK), 0, c->stream, c->d_partials, g, 1, g, dst);
  return hipeig_allreduce_sum(c, dst, 1);
}

// ---- the partitioned sweep --------------------------------------------------------------------------------------------
// Rows dealt to several ranks: a dot and its update cannot share a pass, an all-reduce sits between them.  Per column:
// dot kernel, one-workgroup reduce, all-reduce, update kernel; the coefficients go to coef[W * j].  With `with_norms`
// (the step) dres = [||w||^2 before, coefficients, ||w||^2 after] and w is scaled; without (the projection) dres holds
// the coefficients alone.  Without a communicator - a projection on one GPU - the update kernel sums the dot kernel's g
// partials itself: no reduce kernel, no all-reduce.
template <bool PAIR>
static int arnoldi_partitioned(hipeig_ctx* c, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                               double* wre, double* wim, double* dres, bool with_norms) {
  constexpr int W = PAIR ? 2 : 1;
  const int g = grid_for(n, 4);
  double* red = c->d_scalars + SC_ARN_RED;
  double* coef = dres + (with_norms ? 1 : 0);
  if (with_norms && arnoldi_sumsq(c, n, wre, wim, g, dres)) return 4;
  for (int j = 0; j < m; ++j) {
    const double* vim = PAIR ? Vim[j] : nullptr;
    hipLaunchKernelGGL((mgsp_dot_kernel<PAIR>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, Vre[j], vim, wre, wim, c->d_partials);
    const double* p = c->d_partials;
    int npart = g;
    if (c->collectives) {
      hipLaunchKernelGGL(mgsp_reduce_kernel, dim3(1), dim3(HIPEIG_BLOCK), 0, c->stream, c->d_partials, g, W, g, red);
      if (hipeig_allreduce_sum(c, red, W)) return 4;
      p = red; npart = 1;
    }
    hipLaunchKernelGGL((mgsp_update_kernel<PAIR>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, p, npart, g, Vre[j], vim,
                       wre, wim, coef + W * j);
  }
  if (with_norms) {
    if (arnoldi_sumsq(c, n, wre, wim, g, coef + W * m)) return 4;
    hipLaunchKernelGGL(scale_by_inv_norm_kernel, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, coef + W * m, wre, wim);
  }
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// The result record to the host.  `src`: the device record, or null when the kernels wrote straight into the mapped
// mirror; it is copied to `mirror` (pinned) on `stream`.  Then either `ev` is recorded for whoever collects the record
// later, or - no event - the compute stream is waited for and the record handed out.
static int arnoldi_result_to_host(hipeig_ctx* c, const double* src, double* mirror, int count, hipStream_t stream,
                                  hipEvent_t ev, double* out) {
  if (src) HIPEIG_CHECK(hipMemcpyAsync(mirror, src, sizeof(double) * count, hipMemcpyDeviceToHost, stream));
  if (ev) {
    HIPEIG_CHECK(hipEventRecord(ev, stream));
    return 0;
  }
  if (hipeig_sync_checked(c)) return 4;
  memcpy(out, mirror, sizeof(double) * count);
  return 0;
}

template <bool PAIR>
static int mgs_project_impl(hipeig_ctx* c, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                            double* wre, double* wim, double* coeffs) {
  constexpr int W = PAIR ? 2 : 1;
  HIPEIG_REQUIRE(m >= 0 && m <= ARN_PROJECT_MAX_SCALARS / W && coeffs, "bad arguments");
  if (m == 0) return 0;
  double* dcoef = c->d_scalars + SC_ARN_RESULT;
  if (const int rc = arnoldi_partitioned<PAIR>(c, n, m, Vre, Vim, wre, wim, dcoef, false)) return rc;
  return arnoldi_result_to_host(c, dcoef, c->h_scalars, W * m, c->stream, nullptr, coeffs);
}

extern "C" int hipeig_mgs_project(hipeig_ctx* c, int64_t n, int m, const double* const* V, double* w, double* coeffs) {
  return mgs_project_impl<false>(c, n, m, V, nullptr, w, nullptr, coeffs);
}

extern "C" int hipeig_pair_mgs_project(hipeig_ctx* c, int64_t n, int m, const double* const* Vre,
                                       const double* const* Vim, double* wre, double* wim, double* coeffs) {
  return mgs_project_impl<true>(c, n, m, Vre, Vim, wre, wim, coeffs);
}

// ---- one step, four plans -----------------------------------------------------------------------------------------------
// `cols_per_pass` columns per pass over w: 1 = the sequential sweep (scipy's order of rounding, the default everywhere),
// 4 = the blocked form (same algebra, 2.5 instead of 4 vector streams per column and a launch per four columns;
// coefficients agree with the sequential sweep to rounding).  The blocked form is for one GPU and vectors beyond the
// one-workgroup length; anything else takes a sequential form.  This is the only place that chooses:
//   PARTITIONED  a communicator is attached (whatever cols_per_pass says);
//   BLOCKED      cols_per_pass 4 and n beyond the one-workgroup length;
//   SMALL        n within the one-workgroup length, at most ARN_SMALL_MAXCOLS columns, HIPEIG_ARNOLDI_SMALL not 0;
//   COLUMNS      the rest - also n <= 8192 with more columns, or with HIPEIG_ARNOLDI_SMALL=0, even at cols_per_pass 4.
enum class ArnPlan { SMALL, COLUMNS, BLOCKED, PARTITIONED };

static bool arnoldi_one_workgroup(int64_t n) { return n <= (int64_t)ARN_SMALL_THREADS * ARN_SMALL_E; }

static ArnPlan arnoldi_plan(const hipeig_ctx* c, int64_t n, int m, int cols_per_pass) {
  static const bool small_on = !(getenv("HIPEIG_ARNOLDI_SMALL") && atoi(getenv("HIPEIG_ARNOLDI_SMALL")) == 0);
  if (c->collectives) return ArnPlan::PARTITIONED;
  if (cols_per_pass != 1 && !arnoldi_one_workgroup(n)) return ArnPlan::BLOCKED;
  return (small_on && arnoldi_one_workgroup(n) && m <= ARN_SMALL_MAXCOLS) ? ArnPlan::SMALL : ArnPlan::COLUMNS;
}

// most columns a plan's result record [nb^2, h.., na^2] takes (common.h: the regions of the scalar area)
template <bool PAIR>
static constexpr int arnoldi_max_cols(ArnPlan plan) {
  return plan == ArnPlan::BLOCKED ? (PAIR ? ARN_BLOCKED_MAX_COLS_PAIR : ARN_BLOCKED_MAX_COLS_REAL)
                                  : (ARN_STEP_MAX_SCALARS - 2) / (PAIR ? 2 : 1);
}

template <bool PAIR>
static int arnoldi_run(hipeig_ctx* c, ArnPlan plan, const ArnSpace& sp, int64_t n, int m, const double* const* Vre,
                       const double* const* Vim, double* wre, double* wim, double* dres) {
  switch (plan) {
    case ArnPlan::SMALL: return arnoldi_small<PAIR>(c, n, m, Vre, Vim, wre, wim, dres);
    case ArnPlan::COLUMNS: return arnoldi_columns<PAIR>(c, n, m, Vre, Vim, wre, wim, dres);
    case ArnPlan::BLOCKED: return arnoldi_blocked<PAIR>(c, sp, n, m, Vre, Vim, wre, wim, dres);
    default: return arnoldi_partitioned<PAIR>(c, n, m, Vre, Vim, wre, wim, dres, true);
  }
}

template <bool PAIR>
static int arnoldi_step_impl(hipeig_ctx* c, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                             double* wre, double* wim, double* out, int cols_per_pass) {
  constexpr int W = PAIR ? 2 : 1;
  HIPEIG_REQUIRE(cols_per_pass == 1 || cols_per_pass == 4, "cols_per_pass must be 1 or 4");
  const ArnPlan plan = arnoldi_plan(c, n, m, cols_per_pass);
  HIPEIG_REQUIRE(m >= 0 && m <= arnoldi_max_cols<PAIR>(plan) && out, "bad arguments");
  const bool direct = plan == ArnPlan::SMALL && c->h_scalars_dev;      // no copy to wait for: 28 -> 17 us per step
  double* dres = direct ? c->h_scalars_dev : c->d_scalars + SC_ARN_RESULT;
  if (const int rc = arnoldi_run<PAIR>(c, plan, arnoldi_main_space(c), n, m, Vre, Vim, wre, wim, dres)) return rc;
  return arnoldi_result_to_host(c, direct ? nullptr : dres, c->h_scalars, W * m + 2, c->stream, nullptr, out);
}

extern "C" int hipeig_arnoldi_step(hipeig_ctx* c, int64_t n, int m, const double* const* V, double* w, double* out) {
  return arnoldi_step_impl<false>(c, n, m, V, nullptr, w, nullptr, out, 1);
}

extern "C" int hipeig_pair_arnoldi_step(hipeig_ctx* c, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                                        double* wre, double* wim, double* out) {
  return arnoldi_step_impl<true>(c, n, m, Vre, Vim, wre, wim, out, 1);
}

extern "C" int hipeig_arnoldi_step_p(hipeig_ctx* c, int64_t n, int m, const double* const* V, double* w, double* out, int cols_per_pass) {
  return arnoldi_step_impl<false>(c, n, m, V, nullptr, w, nullptr, out, cols_per_pass);
}

extern "C" int hipeig_pair_arnoldi_step_p(hipeig_ctx* c, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                                          double* wre, double* wim, double* out, int cols_per_pass) {
  return arnoldi_step_impl<true>(c, n, m, Vre, Vim, wre, wim, out, cols_per_pass);
}

// Split form for several independent steps in a row (the right-hand sides of a lock-step block solve each orthogonalise
// against their OWN basis): `begin` enqueues the step and an asynchronous copy of its scalars into pinned slot `slot`
// (0..15, up to 126 doubles each), `end` waits for the stream and hands them over - the host work of one right-hand side
// then overlaps the kernels of the next instead of the GPU idling at every step's round trip.  Real steps (PAIR = false,
// m + 2 scalars) and complex pairs (2m + 2) share the slots, the side streams and their workspaces.
template <bool PAIR>
static int arnoldi_step_begin_impl(hipeig_ctx* c, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                                   double* wre, double* wim, int cols_per_pass, int slot) {
  constexpr int W = PAIR ? 2 : 1;
  HIPEIG_REQUIRE(slot >= 0 && slot < 16 && m >= 0 && W * m + 2 <= ARN_SLOT_DOUBLES - 2, "bad slot / too many columns for the split form");
  HIPEIG_REQUIRE(!c->collectives, "the split form is for one GPU");
  HIPEIG_REQUIRE(cols_per_pass == 1 || cols_per_pass == 4, "cols_per_pass must be 1 or 4");
  const ArnPlan plan = arnoldi_plan(c, n, m, cols_per_pass);          // one GPU: never PARTITIONED
  const size_t slot_at = SH_SLOTS + (size_t)slot * ARN_SLOT_DOUBLES;
  const bool direct = plan == ArnPlan::SMALL && c->h_scalars_dev;
  ArnSpace sp = arnoldi_main_space(c);
  double* dres = direct ? c->h_scalars_dev + slot_at : c->d_scalars + SC_ARN_RESULT;
  if (plan == ArnPlan::BLOCKED) {
    if (arnoldi_side_streams(c)) return 4;
    if (c->arn_nstreams > 1) {
      // The steps of the right-hand sides are independent: slot s runs on side stream s % ns with that stream's own partial
      // areas, total records, ticket counters and result record, behind an event that says "the compute stream has produced
      // this slot's operands".  The caller collects the slot (hipeig_arnoldi_step_end waits for the slot's event) before it
      // enqueues anything that reads what the step wrote, so nothing on the compute stream has to wait for the side stream.
      const int k = slot % c->arn_nstreams;
      double* base = c->d_arn_ws + (size_t)k * ARN_SIDE_DOUBLES;
      sp = ArnSpace{c->arn_stream[k], base, base + ARN_SIDE_PARTIALS, c->d_arn_cnt + (size_t)k * HIPEIG_TICKET_WORDS};
      dres = base + ARN_SIDE_PARTIALS + 64;
      HIPEIG_CHECK(hipEventRecord(c->ev_arn_in[slot], c->stream));
      HIPEIG_CHECK(hipStreamWaitEvent(sp.stream, c->ev_arn_in[slot], 0));
    }
  }
  if (const int rc = arnoldi_run<PAIR>(c, plan, sp, n, m, Vre, Vim, wre, wim, dres)) return rc;
  return arnoldi_result_to_host(c, direct ? nullptr : dres, c->h_scalars + slot_at, W * m + 2, sp.stream, c->ev_slot[slot], nullptr);
}

extern "C" int hipeig_pair_arnoldi_step_begin(hipeig_ctx* c, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                                              double* wre, double* wim, int cols_per_pass, int slot) {
  return arnoldi_step_begin_impl<true>(c, n, m, Vre, Vim, wre, wim, cols_per_pass, slot);
}

extern "C" int hipeig_arnoldi_step_begin(hipeig_ctx* c, int64_t n, int m, const double* const* V, double* w, int cols_per_pass, int slot) {
  return arnoldi_step_begin_impl<false>(c, n, m, V, nullptr, w, nullptr, cols_per_pass, slot);
}

// `count` (<= 16) such steps of length n <= 8192 in one launch (arnoldi_small_batch_kernel): step i has m[i] columns
// Vre[i * 64 + j] (and Vim[i * 64 + j] for pairs; tables of 64 entries per step), works on wre[i] (and wim[i]) and reports
// into pinned slot i; collect with hipeig_arnoldi_step_end(slot i).  Needs the mapped scalar area (returns 5 without it or
// for longer vectors: the caller then takes the step-by-step form).
template <bool PAIR>
static int arnoldi_step_batch_begin_impl(hipeig_ctx* c, int64_t n, int count, const int* m, const double* const* Vre,
                                         const double* const* Vim, double* const* wre, double* const* wim) {
  constexpr int W = PAIR ? 2 : 1;
  HIPEIG_REQUIRE(count >= 1 && count <= 16 && m && Vre && wre && (!PAIR || (Vim && wim)), "bad arguments");
  HIPEIG_REQUIRE(!c->collectives, "the split form is for one GPU");
  if (!arnoldi_one_workgroup(n) || !c->h_scalars_dev) return 5;
  if (!c->h_arn_items) {
    HIPEIG_CHECK(hipHostMalloc(&c->h_arn_items, 16 * sizeof(ArnBatchItem), hipHostMallocMapped));
    if (hipHostGetDevicePointer(&c->d_arn_items, c->h_arn_items, 0) != hipSuccess) {
      (void)hipGetLastError();
      hipHostFree(c->h_arn_items);
      c->h_arn_items = nullptr;
      return 5;
    }
  }
  // the previous batch has been collected (every `end` waits for the batch's event) before its items are overwritten
  HIPEIG_CHECK(hipEventSynchronize(c->ev_slot[0]));
  ArnBatchItem* items = (ArnBatchItem*)c->h_arn_items;
  for (int i = 0; i < count; ++i) {
    HIPEIG_REQUIRE(m[i] >= 0 && m[i] <= ARN_SMALL_MAXCOLS && W * m[i] + 2 <= ARN_SLOT_DOUBLES - 2, "too many columns for the split form");
    items[i].m = m[i]; items[i].pad = 0;
    items[i].wre = wre[i]; items[i].wim = PAIR ? wim[i] : nullptr;
    for (int j = 0; j < m[i]; ++j) {
      items[i].re[j] = Vre[(size_t)i * ARN_SMALL_MAXCOLS + j];
      items[i].im[j] = PAIR ? Vim[(size_t)i * ARN_SMALL_MAXCOLS + j] : nullptr;
    }
  }
  hipLaunchKernelGGL((arnoldi_small_batch_kernel<PAIR>), dim3(count), dim3(ARN_SMALL_THREADS), 0, c->stream, (int)n,
                     (const ArnBatchItem*)c->d_arn_items, c->h_scalars_dev + SH_SLOTS);
  HIPEIG_CHECK(hipGetLastError());
  for (int i = 0; i < count; ++i) HIPEIG_CHECK(hipEventRecord(c->ev_slot[i], c->stream));
  return 0;
}

extern "C" int hipeig_pair_arnoldi_step_batch_begin(hipeig_ctx* c, int64_t n, int count, const int* m, const double* const* Vre,
                                                    const double* const* Vim, double* const* wre, double* const* wim) {
  return arnoldi_step_batch_begin_impl<true>(c, n, count, m, Vre, Vim, wre, wim);
}

extern "C" int hipeig_arnoldi_step_batch_begin(hipeig_ctx* c, int64_t n, int count, const int* m, const double* const* V,
                                               double* const* w) {
  return arnoldi_step_batch_begin_impl<false>(c, n, count, m, V, nullptr, w, nullptr);
}

extern "C" int hipeig_arnoldi_step_end(hipeig_ctx* c, int slot, int count, double* out) {
  HIPEIG_REQUIRE(slot >= 0 && slot < 16 && count >= 0 && count <= ARN_SLOT_DOUBLES && out, "bad arguments");
  HIPEIG_CHECK(hipEventSynchronize(c->ev_slot[slot]));        // this step only: the steps enqueued behind it keep running
  memcpy(out, c->h_scalars + SH_SLOTS + (size_t)slot * ARN_SLOT_DOUBLES, sizeof(double) * count);
  return 0;
}

