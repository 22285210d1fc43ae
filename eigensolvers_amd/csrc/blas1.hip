// BLAS-1 class and tall-skinny kernels of the Krylov loop (all HBM-bound, fp64).
//
// Every kernel is a grid-stride sweep with 16-byte (double2) accesses, at most
// HIPEIG_MAX_PARTIALS workgroups of 256 threads.  Reductions are two-stage with a fixed
// tree (wave shuffle -> LDS -> per-workgroup partial -> fixed-order final sum), never
// atomics, so the results of THESE kernels are bitwise reproducible.  (The operator sweeps are a
// separate matter: kernel variants 1-3 of spmv_device.h fix the order of the adds inside a row, the
// default variant 4 for large operators and the block kernel of spmm_device.h accumulate with LDS
// atomics and reproduce a row's sum only to rounding.)
#include "common.h"
#include <math.h>
#include <vector>

struct PtrTable {
  const double* p[HIPEIG_MAX_COLS];
};
struct CoefTable {
  double c[HIPEIG_MAX_COLS];
};

// ---- reductions of RECORDS that finish inside the kernel that produces them ------------------------------------------
// multi_dot (one value per column), the MGS pair of dots, a Gram block (up to 1024 elements): every workgroup leaves a
// record of nv values, and the totals are formed without a second launch (round 3 did this for single scalars, common.h):
//   * workgroup b stores its record at partials[b * nv ..] (agent-scope stores, waited for) and takes a ticket of its
//     GROUP of 64 workgroups;
//   * the workgroup that completes a group adds the group's <= 64 records in ascending order into a group record and takes
//     a ticket of the master counter; the one that completes the master adds the <= 32 group records in order and stores
//     the totals (to mapped host memory on one GPU: a stream wait, no copy).
// Two levels because one workgroup adding 2048 records of 1 KiB would take longer than the launch it replaces; the group
// sums run on as many CUs as there are groups.  Order and tree are fixed by (gridDim.x, nv): bitwise reproducible.
#define REC_GROUP 64
#define REC_GROUP_DOUBLES 32768            // size of ctx->d_group_partials: (groups) x (values per record) must fit

__device__ __forceinline__ double agent_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void agent_store_nowait(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// sum_{i = first, first + step, ... < count} p[i * nv]: loads in batches of 8 (all in flight), adds in index order
__device__ __forceinline__ double agent_sum_strided(const double* p, int first, int count, int step, size_t nv) {
  double a = 0.0;
  int i = first;
  for (; i + 7 * step < count; i += 8 * step) {
    double t[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) t[q] = agent_load(p + (size_t)(i + q * step) * nv);
#pragma unroll
    for (int q = 0; q < 8; ++q) a += t[q];
  }
  for (; i < count; i += step) a += agent_load(p + (size_t)i * nv);
  return a;
}

// Totals of `count` records of nv values (record-major) by ONE 256-thread workgroup; store(e, total_e) is called once per
// value.  nv <= 128: 256 / nvp lanes share a value (nvp = nv rounded up to a power of two), their sums are added in lane
// order through LDS; larger records: one thread per value, 256 values at a time.  lds: 256 doubles.
template <class Store>
__device__ __forceinline__ void sum_records(const double* p, int count, int nv, double* lds, Store store) {
  const int t = threadIdx.x;
  if (nv <= 128) {
    int nvp = 1;
    while (nvp < nv) nvp <<= 1;
    const int kl = HIPEIG_BLOCK / nvp, v = t & (nvp - 1), k = t / nvp;
    lds[k * nvp + v] = (v < nv) ? agent_sum_strided(p + v, k, count, kl, (size_t)nv) : 0.0;
    __syncthreads();
    if (t < nv) {
      double s = lds[t];
      for (int q = 1; q < kl; ++q) s += lds[q * nvp + t];
      store(t, s);
    }
    __syncthreads();
  } else {
    for (int e = t; e < nv; e += HIPEIG_BLOCK) store(e, agent_sum_strided(p + e, 0, count, 1, (size_t)nv));
  }
}

// Call after every thread of the workgroup has issued the agent_store_nowait's of its share of the record
// partials[blockIdx.x * nv ..].  counters: 1 + ceil(gridDim.x / 64) words, zero before the kernel and after it.
__device__ __forceinline__ void finish_records(double* partials, double* group_partials, int nv, unsigned* counters,
                                               double* lds /* 256 doubles */, double* out) {
  __shared__ int sh_flag;
  const unsigned G = gridDim.x, ng = (G + REC_GROUP - 1) / REC_GROUP, g = blockIdx.x / REC_GROUP;
  const unsigned gsize = (g == ng - 1) ? G - g * REC_GROUP : REC_GROUP;
  wait_for_my_stores();
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool last = __hip_atomic_fetch_add(counters + 1 + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gsize - 1u;
    if (last) __hip_atomic_store(counters + 1 + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_flag = last;
  }
  __syncthreads();
  if (!sh_flag) return;                               // uniform
  __syncthreads();
  if (ng == 1) {
    sum_records(partials, (int)G, nv, lds, [&](int e, double s) { out[e] = s; });
    return;
  }
  double* mine = group_partials + (size_t)g * nv;
  sum_records(partials + (size_t)g * REC_GROUP * nv, (int)gsize, nv, lds, [&](int e, double s) { agent_store_nowait(mine + e, s); });
  wait_for_my_stores();
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool last = __hip_atomic_fetch_add(counters, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ng - 1u;
    if (last) __hip_atomic_store(counters, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_flag = last;
  }
  __syncthreads();
  if (!sh_flag) return;
  __syncthreads();
  sum_records(group_partials, (int)ng, nv, lds, [&](int e, double s) { out[e] = s; });
}

// Where a record kernel stores its totals: the pinned, mapped host buffer when the caller wants them on the host of a
// single-GPU context (the result then needs a stream wait but no copy command), else the device scalar area.
static double* record_target(hipeig_ctx* c, bool to_host) {
  return (to_host && !c->collectives && c->h_scalars_dev) ? c->h_scalars_dev : c->d_scalars;
}

// The totals are where record_target() said: sum them over the ranks if the context is partitioned and hand them over.
static int records_to_host(hipeig_ctx* c, int ncols, double* host_out) {
  HIPEIG_CHECK(hipGetLastError());
  if (host_out && !c->collectives && c->h_scalars_dev) {
    if (hipeig_sync_checked(c)) return 4;
    memcpy(host_out, c->h_scalars, sizeof(double) * ncols);
    return 0;
  }
  if (hipeig_allreduce_sum(c, c->d_scalars, ncols)) return 4;
  if (host_out) {
    HIPEIG_CHECK(hipMemcpyAsync(c->h_scalars, c->d_scalars, sizeof(double) * ncols,
                                hipMemcpyDeviceToHost, c->stream));
    if (hipeig_sync_checked(c)) return 4;
    memcpy(host_out, c->h_scalars, sizeof(double) * ncols);
  }
  return 0;
}

// Grid of a streaming kernel that ends in finish_records: every workgroup pays a fixed price for its record (store, wait,
// ticket), so FEWER, fatter workgroups win as long as the chip stays busy.  Measured (tools/experiments/mgs_grid.sh,
// multidot_grid.sh; profiles/r04_mgs_fused_sweep_grid.txt, r04_multidot_grid.txt): MGS m = 16 at N = 1e7 with 2 / 8 / 32 /
// 64 / 128 elements per thread 1.71 / 1.16 / 0.93 / 0.97 / 1.44 ms, at N = 1e6 with 2 / 8 / 16 / 32: 0.42 / 0.277 / 0.275 /
// 0.35 ms; multi_dot m = 16 at N = 1e7 with 2 / 32 / 48: 0.273 / 0.245 / 0.267 ms, at N = 1e6 with 2 / 4 / 8 / 16: 0.063 /
// 0.053 / 0.054 / 0.072 ms.  Hence n / 8192 workgroups, but at least two per CU (as far as n / 1024 goes).
static int grid_records(const hipeig_ctx* c, int64_t n, const char* knob) {
  int64_t g = n / 8192;
  const int64_t floor2 = n / 1024 < 2 * (int64_t)c->num_cu ? n / 1024 : 2 * (int64_t)c->num_cu;
  if (g < floor2) g = floor2;
  if (const char* e = knob ? getenv(knob) : nullptr) g = atoi(e) > 0 ? n / (256 * (int64_t)atoi(e)) : g;      // tuning knob: elements per thread
  if (g < 1) g = 1;
  if (g > HIPEIG_MAX_PARTIALS) g = HIPEIG_MAX_PARTIALS;
  return (int)g;
}

// ---- dot / nrm2 ------------------------------------------------------------------------
// The total is formed by the kernel's last workgroup (common.h) and stored to `out` - on one GPU the pinned, mapped host
// word, so that a dot product is ONE launch and a stream wait (round 2: two launches).
__global__ void __launch_bounds__(HIPEIG_BLOCK)
dot_kernel(int64_t n, const double* __restrict__ x, const double* __restrict__ y,
           double* __restrict__ partials, unsigned* counters, double* __restrict__ out) {
  __shared__ double lds[4];
  const int64_t n2 = n >> 1;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  const double2* y2 = reinterpret_cast<const double2*>(y);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double a0 = 0.0, a1 = 0.0;
  for (; i + stride < n2; i += 2 * stride) {        // two independent 16-byte loads in flight
    const double2 xa = x2[i], ya = y2[i];
    const double2 xb = x2[i + stride], yb = y2[i + stride];
    a0 = fma(xa.x, ya.x, a0); a0 = fma(xa.y, ya.y, a0);
    a1 = fma(xb.x, yb.x, a1); a1 = fma(xb.y, yb.y, a1);
  }
  for (; i < n2; i += stride) {
    const double2 xa = x2[i], ya = y2[i];
    a0 = fma(xa.x, ya.x, a0); a0 = fma(xa.y, ya.y, a0);
  }
  double a = a0 + a1;
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) a = fma(x[n - 1], y[n - 1], a);
  a = block_reduce_sum(a, lds);
  if (threadIdx.x == 0) store_partial(partials + blockIdx.x, a);
  if (last_block_ticket(counters, gridDim.x, blockIdx.x)) {
    const double t = sum_partials_agent(partials, gridDim.x, lds);
    if (threadIdx.x == 0) *out = t;
    release_ticket_counter(counters);
  }
}

extern "C" int hipeig_dot(hipeig_ctx* c, int64_t n, const double* x, const double* y, double* out) {
  HIPEIG_REQUIRE(out != nullptr, "null output");
  const int g = grid_records(c, n, "HIPEIG_DOT_PER_THREAD");
  unsigned* cnt = c->d_counters + 3 * HIPEIG_TICKET_WORDS;
  const bool direct = !c->collectives && c->h_scalars_dev;
  hipLaunchKernelGGL(dot_kernel, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, x, y, c->d_partials, cnt,
                     direct ? c->h_scalars_dev : c->d_scalars);
  HIPEIG_CHECK(hipGetLastError());
  if (direct) {
    if (hipeig_sync_checked(c)) return 4;
    *out = c->h_scalars[0];
    return 0;
  }
  if (hipeig_allreduce_sum(c, c->d_scalars, 1)) return 4;
  HIPEIG_CHECK(hipMemcpyAsync(c->h_scalars, c->d_scalars, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (hipeig_sync_checked(c)) return 4;
  *out = c->h_scalars[0];
  return 0;
}

extern "C" int hipeig_nrm2(hipeig_ctx* c, int64_t n, const double* x, double* out) {
  double ss = 0.0;
  int rc = hipeig_dot(c, n, x, x, &ss);
  if (rc) return rc;
  *out = sqrt(ss);
  return 0;
}

// ---- scale / axpby ---------------------------------------------------------------------
// y = x * alpha (divide == 0) or y = x / alpha (divide == 1; the reference divides, e.g.
// array /= norm at numpyVector.py:77 and x/np.sqrt(innerprod) at :142)
__global__ void __launch_bounds__(HIPEIG_BLOCK)
scale_kernel(int64_t n, double alpha, int divide, const double* __restrict__ x, double* __restrict__ y) {
  const int64_t n2 = n >> 1;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  double2* y2 = reinterpret_cast<double2*>(y);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (divide) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      double2 v = x2[i];
      v.x /= alpha; v.y /= alpha;
      y2[i] = v;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) y[n - 1] = x[n - 1] / alpha;
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
      double2 v = x2[i];
      v.x *= alpha; v.y *= alpha;
      y2[i] = v;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) y[n - 1] = x[n - 1] * alpha;
  }
}

extern "C" int hipeig_scale(hipeig_ctx* c, int64_t n, double alpha, const double* x, double* y) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(scale_kernel, dim3(grid_stream(n)), dim3(HIPEIG_BLOCK), 0, c->stream, n, alpha, 0, x, y);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

extern "C" int hipeig_divide(hipeig_ctx* c, int64_t n, double alpha, const double* x, double* y) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(scale_kernel, dim3(grid_stream(n)), dim3(HIPEIG_BLOCK), 0, c->stream, n, alpha, 1, x, y);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

extern "C" int hipeig_normalize(hipeig_ctx* c, int64_t n, double* x, double* norm_out) {
  double nrm = 0.0;
  int rc = hipeig_nrm2(c, n, x, &nrm);
  if (rc) return rc;
  if (norm_out) *norm_out = nrm;
  // la.norm then array /= norm (numpyVector.py:76-78): a true division, not a
  // multiplication by the reciprocal, to stay on the reference's rounding.
  if (n == 0) return 0;
  hipLaunchKernelGGL(scale_kernel, dim3(grid_stream(n)), dim3(HIPEIG_BLOCK), 0, c->stream, n, nrm, 1, x, x);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

__global__ void __launch_bounds__(HIPEIG_BLOCK)
axpby_kernel(int64_t n, double a, const double* __restrict__ x, double b, double* __restrict__ y) {
  const int64_t n2 = n >> 1;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  double2* y2 = reinterpret_cast<double2*>(y);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    const double2 xv = x2[i];
    double2 yv = y2[i];
    yv.x = a * xv.x + b * yv.x;
    yv.y = a * xv.y + b * yv.y;
    y2[i] = yv;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) y[n - 1] = a * x[n - 1] + b * y[n - 1];
}

extern "C" int hipeig_axpby(hipeig_ctx* c, int64_t n, double a, const double* x, double b, double* y) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(axpby_kernel, dim3(grid_stream(n)), dim3(HIPEIG_BLOCK), 0, c->stream, n, a, x, b, y);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// ---- linear combination: out = (accumulate ? out : 0) + sum_j c[j]*v_j -----------------
template <int MB>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
lincomb_kernel(int64_t n, int m, PtrTable tab, CoefTable cf, const double* __restrict__ dcoef,
               double dscale, int accumulate, double* __restrict__ out) {
  double cj[MB];
#pragma unroll
  for (int j = 0; j < MB; ++j) cj[j] = (j < m) ? (dcoef ? dscale * dcoef[j] : cf.c[j]) : 0.0;
  const int64_t n2 = n >> 1;
  double2* o2 = reinterpret_cast<double2*>(out);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    double2 acc = accumulate ? o2[i] : make_double2(0.0, 0.0);
#pragma unroll
    for (int j = 0; j < MB; ++j) {
      if (j < m) {
        const double2 v = reinterpret_cast<const double2*>(tab.p[j])[i];
        acc.x = fma(cj[j], v.x, acc.x);
        acc.y = fma(cj[j], v.y, acc.y);
      }
    }
    o2[i] = acc;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    double acc = accumulate ? out[n - 1] : 0.0;
    for (int j = 0; j < m; ++j) acc = fma(cj[j], tab.p[j][n - 1], acc);
    out[n - 1] = acc;
  }
}

// dcoef (device, scaled by dscale) overrides coeffs (host) when non-null; it holds k doubles.
static int lincomb_impl(hipeig_ctx* c, int64_t n, int k, const double* coeffs, const double* dcoef,
                        double dscale, const double* const* vecs, double* out, int accumulate_first) {
  if (n == 0) return 0;
  const int g = grid_stream(n);
  for (int j0 = 0; j0 < k; j0 += HIPEIG_MAX_COLS) {
    const int m = (k - j0 < HIPEIG_MAX_COLS) ? (k - j0) : HIPEIG_MAX_COLS;
    PtrTable tab;
    CoefTable cf;
    for (int j = 0; j < HIPEIG_MAX_COLS; ++j) {
      tab.p[j] = (j < m) ? vecs[j0 + j] : nullptr;
      cf.c[j] = (j < m && coeffs) ? coeffs[j0 + j] : 0.0;
    }
    const int acc = (j0 > 0) || accumulate_first;
    const double* dc = dcoef ? dcoef + j0 : nullptr;
    if (m <= 4)
      hipLaunchKernelGGL((lincomb_kernel<4>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, m, tab, cf, dc, dscale, acc, out);
    else if (m <= 8)
      hipLaunchKernelGGL((lincomb_kernel<8>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, m, tab, cf, dc, dscale, acc, out);
    else
      hipLaunchKernelGGL((lincomb_kernel<HIPEIG_MAX_COLS>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, m, tab, cf, dc, dscale, acc, out);
    HIPEIG_CHECK(hipGetLastError());
  }
  return 0;
}

extern "C" int hipeig_lincomb(hipeig_ctx* c, int64_t n, int k, const double* coeffs,
                              const double* const* vecs, double* out) {
  HIPEIG_REQUIRE(k >= 1, "need at least one vector");
  for (int j = 0; j < k; ++j) HIPEIG_REQUIRE(vecs[j] != out, "out must not alias an input");
  return lincomb_impl(c, n, k, coeffs, nullptr, 1.0, vecs, out, 0);
}

// ---- block linear combination: outs[c] = sum_j C[j][c] * v_j, all k outputs in ONE pass ----
// (basisTransformation with a coefficient matrix, util_funcs.py:229-230: the tall-skinny product
// Y*C.)  Every thread keeps the KB output accumulators of its two rows in registers and streams the m
// inputs past them, so the inputs are read once instead of k times: (m + k) * 8N bytes.  Pointer
// table and coefficients are read from device memory with wave-uniform (scalar) loads.
struct OutTable {
  double* p[HIPEIG_MAX_COLS];
};

template <int KB>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
lincomb_block_kernel(int64_t n, int m, int k, const double* const* __restrict__ vecs,
                     const double* __restrict__ coef /* m x KB, row-major, zero-padded */, OutTable outs) {
  const int64_t n2 = n >> 1;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    double2 acc[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) acc[c] = make_double2(0.0, 0.0);
#pragma unroll 4
    for (int j = 0; j < m; ++j) {
      const double2 v = reinterpret_cast<const double2*>(vecs[j])[i];
#pragma unroll
      for (int c = 0; c < KB; ++c) {
        const double w = coef[j * KB + c];
        acc[c].x = fma(w, v.x, acc[c].x);
        acc[c].y = fma(w, v.y, acc[c].y);
      }
    }
#pragma unroll
    for (int c = 0; c < KB; ++c)
      if (c < k) reinterpret_cast<double2*>(outs.p[c])[i] = acc[c];
  }
  if ((n & 1) && blockIdx.x == 0 && (int)threadIdx.x < k) {
    const int c = threadIdx.x;
    double a = 0.0;
    for (int j = 0; j < m; ++j) a = fma(coef[j * KB + c], vecs[j][n - 1], a);
    outs.p[c][n - 1] = a;
  }
}

extern "C" int hipeig_lincomb_block(hipeig_ctx* c, int64_t n, int m, int k, const double* C, int ldc,
                                    const double* const* vecs, double* const* outs) {
  HIPEIG_REQUIRE(m >= 1 && k >= 1 && ldc >= k, "bad shape");
  HIPEIG_REQUIRE((size_t)m <= c->ptrs_count, "too many input vectors for one call");
  for (int j = 0; j < m; ++j)
    for (int q = 0; q < k; ++q) HIPEIG_REQUIRE(vecs[j] != outs[q], "an output must not alias an input");
  if (n == 0) return 0;
  // Sources of asynchronous copies are the context's PINNED staging buffers (h_ptrs, h_scalars), never
  // pageable memory that goes out of scope or is refilled while a copy may still be reading it.  Only this
  // function and hipeig_comm_setup_rows (which drains the stream) rewrite them from the host, so it is enough
  // to wait for the event recorded behind the previous call's last copy - not for the whole stream.
  HIPEIG_CHECK(hipEventSynchronize(c->ev_stage));
  for (int j = 0; j < m; ++j) c->h_ptrs[j] = vecs[j];
  HIPEIG_CHECK(hipMemcpyAsync((void*)c->d_ptrs, c->h_ptrs, sizeof(double*) * m, hipMemcpyHostToDevice, c->stream));
  const int g = grid_for(n, 2);                       // the per-workgroup coefficient prologue wants long-lived workgroups (measured: n/512 workgroups 8 % slower)
  double* dcoef = c->d_partials;                      // free here: this call has no reduction
  double* cf = c->h_scalars;
  size_t cf_used = 0;
  for (int c0 = 0; c0 < k; c0 += HIPEIG_MAX_COLS) {
    const int kk = (k - c0 < HIPEIG_MAX_COLS) ? (k - c0) : HIPEIG_MAX_COLS;
    const int KB = kk <= 4 ? 4 : kk <= 8 ? 8 : HIPEIG_MAX_COLS;
    if (cf_used + (size_t)m * KB > c->scalars_doubles) {            // staging area full: wait for the copies issued so far
      if (hipeig_sync_checked(c)) return 4;
      cf_used = 0;
    }
    HIPEIG_REQUIRE((size_t)m * KB <= c->scalars_doubles, "too many input vectors for the coefficient staging buffer");
    double* slot = cf + cf_used;
    for (int j = 0; j < m; ++j)
      for (int q = 0; q < KB; ++q) slot[(size_t)j * KB + q] = (q < kk) ? C[(size_t)j * ldc + c0 + q] : 0.0;
    HIPEIG_CHECK(hipMemcpyAsync(dcoef, slot, sizeof(double) * m * KB, hipMemcpyHostToDevice, c->stream));
    cf_used += (size_t)m * KB;
    OutTable ot;
    for (int q = 0; q < HIPEIG_MAX_COLS; ++q) ot.p[q] = (q < kk) ? outs[c0 + q] : nullptr;
    if (KB == 4)
      hipLaunchKernelGGL((lincomb_block_kernel<4>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, m, kk, c->d_ptrs, dcoef, ot);
    else if (KB == 8)
      hipLaunchKernelGGL((lincomb_block_kernel<8>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, m, kk, c->d_ptrs, dcoef, ot);
    else
      hipLaunchKernelGGL((lincomb_block_kernel<HIPEIG_MAX_COLS>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, m, kk, c->d_ptrs, dcoef, ot);
    HIPEIG_CHECK(hipGetLastError());
    dcoef += (size_t)m * KB;
  }
  HIPEIG_CHECK(hipEventRecord(c->ev_stage, c->stream));  // behind the last copy out of the staging buffers
  return 0;
}

extern "C" int hipeig_multi_axpy(hipeig_ctx* c, int64_t n, int m, const double* const* Y,
                                 const double* coef, double* x) {
  if (m == 0) return 0;
  return lincomb_impl(c, n, m, coef, nullptr, 1.0, Y, x, 1);
}

// ---- multi_dot: out[j] = <Y_j, x> -------------------------------------------------------
template <int MB>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
multi_dot_kernel(int64_t n, int m, PtrTable tab, const double* __restrict__ x,
                 double* __restrict__ partials, double* __restrict__ group_partials, unsigned* counters, double* __restrict__ out) {
  __shared__ double lds[HIPEIG_BLOCK];
  double acc[MB];
#pragma unroll
  for (int j = 0; j < MB; ++j) acc[j] = 0.0;
  const int64_t n2 = n >> 1;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    const double2 xv = x2[i];
#pragma unroll
    for (int j = 0; j < MB; ++j) {
      if (j < m) {
        const double2 v = reinterpret_cast<const double2*>(tab.p[j])[i];
        acc[j] = fma(v.x, xv.x, acc[j]);
        acc[j] = fma(v.y, xv.y, acc[j]);
      }
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < MB; ++j)
      if (j < m) acc[j] = fma(tab.p[j][n - 1], x[n - 1], acc[j]);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < MB; ++j) {
    const double r = wave_reduce_sum(acc[j]);
    if (lane == 0) lds[wid * MB + j] = r;
  }
  __syncthreads();
  if ((int)threadIdx.x < m) {
    const int j = threadIdx.x;
    agent_store_nowait(partials + (size_t)blockIdx.x * m + j, lds[j] + lds[MB + j] + lds[2 * MB + j] + lds[3 * MB + j]);
  }
  __syncthreads();                                   // lds is reused by the record sums
  finish_records(partials, group_partials, m, counters, lds, out);
}

// One launch for <= 16 columns: records [block][m] in the partial workspace (reused by the next launch: same stream),
// totals to out[0..m).
static int multi_dot_launch(hipeig_ctx* c, int64_t n, int m, const double* const* Y, const double* x, int g, double* out) {
  PtrTable tab;
  for (int j = 0; j < HIPEIG_MAX_COLS; ++j) tab.p[j] = (j < m) ? Y[j] : nullptr;
  unsigned* cnt = c->d_counters + 3 * HIPEIG_TICKET_WORDS;
  if (m <= 4)
    hipLaunchKernelGGL((multi_dot_kernel<4>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, m, tab, x, c->d_partials, c->d_group_partials, cnt, out);
  else if (m <= 8)
    hipLaunchKernelGGL((multi_dot_kernel<8>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, m, tab, x, c->d_partials, c->d_group_partials, cnt, out);
  else
    hipLaunchKernelGGL((multi_dot_kernel<HIPEIG_MAX_COLS>), dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, m, tab, x, c->d_partials, c->d_group_partials, cnt, out);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// Device-side result in ctx->d_scalars[0..m); optionally copied to the host.
static int multi_dot_impl(hipeig_ctx* c, int64_t n, int m, const double* const* Y, const double* x,
                          double* host_out) {
  HIPEIG_REQUIRE(m >= 1 && m <= HIPEIG_MAX_COLS * HIPEIG_MAX_COLS, "too many columns for one call");
  const int g = grid_records(c, n, "HIPEIG_MULTIDOT_PER_THREAD");
  double* target = record_target(c, host_out != nullptr);
  for (int j0 = 0; j0 < m; j0 += HIPEIG_MAX_COLS) {
    const int mm = (m - j0 < HIPEIG_MAX_COLS) ? (m - j0) : HIPEIG_MAX_COLS;
    if (multi_dot_launch(c, n, mm, Y + j0, x, g, target + j0)) return 1;
  }
  return records_to_host(c, m, host_out);
}

extern "C" int hipeig_multi_dot(hipeig_ctx* c, int64_t n, int m, const double* const* Y,
                                const double* x, double* out) {
  int done = 0;
  const int cap = HIPEIG_MAX_COLS * HIPEIG_MAX_COLS;
  while (done < m) {
    const int mm = (m - done < cap) ? (m - done) : cap;
    int rc = multi_dot_impl(c, n, mm, Y + done, x, out + done);
    if (rc) return rc;
    done += mm;
  }
  return 0;
}

// ---- Gram blocks on the matrix cores -------------------------------------------------------
// C[i][j] = sum_r A_i[r] * B_j[r]: v_mfma_f64_16x16x4_f64 with the ROW index r as the K dimension.
// One pass handles up to 32 columns of A and 32 of B (2 x 2 accumulator blocks of 16 x 16; the
// symmetric case A == B reads only its 32 columns and skips the lower block).  A workgroup stages a
// tile of 128 rows x all columns in LDS - every wave instruction is a coalesced 1 KiB read of ONE
// column (lane = row pair, 16 bytes) - then its four waves each take a quarter of the tile's rows
// as K-steps of 4.  LDS column stride 130 doubles (= 2 mod 32): the 32 lanes of an operand read
// (16 columns x 2 rows) hit 32 distinct 8-byte banks.  Two workgroups per CU overlap one's loads with
// the other's MFMAs.  Traffic: every column is read once per pass, (ma + mb) * 8N bytes against
// 8N * ma * (mb + 1) for mb multi_dot sweeps.  Per-workgroup partial blocks are summed in fixed order
// by the kernel's own last workgroups (finish_records above).
typedef double d4_t __attribute__((ext_vector_type(4)));
#define GRAM_ROWS 128
#define GRAM_LD 130
#define GRAM_MAX_WG 2048

struct PtrTable32 {
  const double* p[32];
};

template <int NA, int NB, bool SAME>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
gram_tile_kernel(int64_t n, int ma, int mb, PtrTable32 A, PtrTable32 B, double* __restrict__ partials,
                 double* __restrict__ group_partials, unsigned* counters, double* __restrict__ out) {
  extern __shared__ double gram_lds[];
  constexpr int CA = NA * 16, CB = SAME ? 0 : NB * 16;
  double* tA = gram_lds;
  double* tB = SAME ? gram_lds : gram_lds + CA * GRAM_LD;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // tell the compiler it is wave-uniform
  d4_t acc[NA][NB];
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
  const int64_t ntiles = (n + GRAM_ROWS - 1) / GRAM_ROWS;
  // The next tile is loaded into registers while the MFMAs of the current one run out of LDS.
  constexpr int NQ = (CA + CB) / 4;
  double2 pre[NQ];
  const double* srcs[NQ];                            // this wave's columns (wave-uniform: scalar registers)
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int col = wid + 4 * q;
    srcs[q] = (col < CA) ? (col < ma ? A.p[col] : nullptr) : (col - CA < mb ? B.p[col - CA] : nullptr);
  }
#define GRAM_FETCH(T)                                                                                   \
  {                                                                                                     \
    const int64_t r = (T) * GRAM_ROWS + 2 * lane;                                                       \
    _Pragma("unroll") for (int q = 0; q < NQ; ++q) {                                                    \
      const double* src = srcs[q];                                                                      \
      double2 v = make_double2(0.0, 0.0);                                                               \
      if (src && (T) < ntiles) {                                                                        \
        if (r + 1 < n) {                                                                                \
          typedef double gram_v2 __attribute__((ext_vector_type(2)));                                   \
          const gram_v2 w = __builtin_nontemporal_load(reinterpret_cast<const gram_v2*>(src + r));      \
          v = make_double2(w.x, w.y);                                                                   \
        } else if (r < n) v.x = src[r];                                                                 \
      }                                                                                                 \
      pre[q] = v;                                                                                       \
    }                                                                                                   \
  }
  GRAM_FETCH((int64_t)blockIdx.x)
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {           // uniform trip count per workgroup
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      *reinterpret_cast<double2*>(gram_lds + (wid + 4 * q) * GRAM_LD + 2 * lane) = pre[q];
    __syncthreads();
    GRAM_FETCH(t + gridDim.x)
#pragma unroll
    for (int s = 0; s < GRAM_ROWS / 16; ++s) {
      const int row = 4 * (wid * (GRAM_ROWS / 16) + s) + (lane >> 4);
      double a[NA], b[NB];
#pragma unroll
      for (int i = 0; i < NA; ++i) a[i] = tA[(i * 16 + (lane & 15)) * GRAM_LD + row];
#pragma unroll
      for (int j = 0; j < NB; ++j) b[j] = SAME ? a[j] : tB[(j * 16 + (lane & 15)) * GRAM_LD + row];
#pragma unroll
      for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
          if (!SAME || j >= i) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
#undef GRAM_FETCH
  // C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg.  Sum the four waves'
  // blocks through LDS (the tile area is free now): red[wave][block][256].
  double* red = gram_lds;
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        red[(wid * NA * NB + i * NB + j) * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[i][j][reg];
  __syncthreads();
  const int e = threadIdx.x;                       // 256 threads <-> 256 elements of a block
#pragma unroll
  for (int blk = 0; blk < NA * NB; ++blk) {
    const double v = red[(0 * NA * NB + blk) * 256 + e] + red[(1 * NA * NB + blk) * 256 + e] +
                     red[(2 * NA * NB + blk) * 256 + e] + red[(3 * NA * NB + blk) * 256 + e];
    agent_store_nowait(partials + (size_t)blockIdx.x * (NA * NB * 256) + blk * 256 + e, v);
  }
  __syncthreads();                                   // the LDS block area is reused by the record sums
  finish_records(partials, group_partials, NA * NB * 256, counters, gram_lds, out);
}

template <int NA, int NB, bool SAME>
static int gram_tile_launch(hipeig_ctx* c, int64_t n, int na, int nb, const PtrTable32& ta, const PtrTable32& tb, int& g) {
  constexpr size_t tile = (size_t)(NA * 16 + (SAME ? 0 : NB * 16)) * GRAM_LD * sizeof(double);
  constexpr size_t red = (size_t)4 * NA * NB * 256 * sizeof(double);
  constexpr size_t lds = tile > red ? tile : red;
  static bool configured = false;
  {
    // workgroups per CU that fit the LDS (at most 8), capped by the partial-block workspace
    int per_cu = (int)((size_t)160 * 1024 / (lds + 512));
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;
    int64_t cap = (int64_t)c->num_cu * per_cu;
    const int64_t room = (int64_t)(c->partials_doubles / ((size_t)NA * NB * 256));
    if (cap > room) cap = room;
    if (g > cap) g = (int)cap;
  }
  if (!configured) {
    HIPEIG_CHECK(hipFuncSetAttribute((const void*)gram_tile_kernel<NA, NB, SAME>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    configured = true;
  }
  hipLaunchKernelGGL((gram_tile_kernel<NA, NB, SAME>), dim3(g), dim3(HIPEIG_BLOCK), lds, c->stream, n, na, nb, ta, tb, c->d_partials,
                     c->d_group_partials, c->d_counters + 3 * HIPEIG_TICKET_WORDS, record_target(c, true));
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

extern "C" int hipeig_gram(hipeig_ctx* c, int64_t n, int ma, const double* const* A, int mb,
                           const double* const* B, double* out) {
  HIPEIG_REQUIRE(ma >= 1 && mb >= 1, "empty set");
  if (ma < 3 || mb < 3 || n < 64) {
    // tiny blocks: one multi_dot sweep per column of B
    double* col = (double*)malloc(sizeof(double) * ma);
    HIPEIG_REQUIRE(col != nullptr, "out of host memory");
    int rc = 0;
    for (int j = 0; j < mb && !rc; ++j) {
      rc = hipeig_multi_dot(c, n, ma, A, B[j], col);
      for (int i = 0; i < ma; ++i) out[(size_t)i * mb + j] = col[i];
    }
    free(col);
    return rc;
  }
  bool symmetric = (ma == mb);
  for (int i = 0; i < ma && symmetric; ++i) symmetric = (A[i] == B[i]);
  int64_t g64 = (n + GRAM_ROWS - 1) / GRAM_ROWS;
  if (g64 > GRAM_MAX_WG) g64 = GRAM_MAX_WG;         // upper bound; each launch lowers it to what fits a CU
  const int g = (int)g64;
  std::vector<double> blk(4 * 256);
  for (int ia = 0; ia < ma; ia += 32) {
    for (int ib = 0; ib < mb; ib += 32) {
      if (symmetric && ib < ia) continue;           // mirrored from the upper block below
      const int na = (ma - ia < 32) ? ma - ia : 32, nb = (mb - ib < 32) ? mb - ib : 32;
      const int NA = (na + 15) / 16, NB = (nb + 15) / 16;
      PtrTable32 ta, tb;
      bool same = (na == nb);
      for (int q = 0; q < 32; ++q) {
        ta.p[q] = (q < na) ? A[ia + q] : nullptr;
        tb.p[q] = (q < nb) ? B[ib + q] : nullptr;
        if (ta.p[q] != tb.p[q]) same = false;
      }
      int rc, gl = g;                              // the launch lowers gl to the grid it used
      if (same && NA == 1) rc = gram_tile_launch<1, 1, true>(c, n, na, nb, ta, tb, gl);
      else if (same) rc = gram_tile_launch<2, 2, true>(c, n, na, nb, ta, tb, gl);
      else if (NA == 1 && NB == 1) rc = gram_tile_launch<1, 1, false>(c, n, na, nb, ta, tb, gl);
      else if (NA == 1) rc = gram_tile_launch<1, 2, false>(c, n, na, nb, ta, tb, gl);
      else if (NB == 1) rc = gram_tile_launch<2, 1, false>(c, n, na, nb, ta, tb, gl);
      else rc = gram_tile_launch<2, 2, false>(c, n, na, nb, ta, tb, gl);
      if (rc) return rc;
      if (records_to_host(c, NA * NB * 256, blk.data())) return 4;
      for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) {
          const int bi = i >> 4, bj = j >> 4;
          double v;
          if (same && bj < bi) v = blk[(bj * NB + bi) * 256 + (j & 15) * 16 + (i & 15)];   // lower block of a symmetric pass
          else v = blk[(bi * NB + bj) * 256 + (i & 15) * 16 + (j & 15)];
          out[(size_t)(ia + i) * mb + (ib + j)] = v;
          if (symmetric && ib > ia) out[(size_t)(ib + j) * mb + (ia + i)] = v;
        }
    }
  }
  return 0;
}

// ---- Gram-Schmidt ------------------------------------------------------------------------
// The reference's sequential MGS (numpyVector.py:132-139: per q  t1 = x.q, t2 = q.q, x = x - q*(t1/t2)) as ONE kernel per
// basis vector plus one: kernel j applies the update of q_{j-1} with the totals kernel j-1 left and, on the updated x in
// the same pass, forms the two dots with q_j; the kernel behind the last vector applies the last update and forms x.x,
// the inner product the lindep test needs (:140).  Round 3 ran dots, a 2-workgroup sum and the update as three launches
// per vector and read x twice: 40N bytes per vector against 32N now.  Same element-wise roundings as the reference:
// x + (-(q * coef)), two roundings.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
mgs_sweep_kernel(int64_t n, double* __restrict__ x, const double* __restrict__ q_prev, const double* __restrict__ t_prev,
                 const double* __restrict__ q_next, double* __restrict__ partials, double* __restrict__ group_partials,
                 unsigned* counters, double* __restrict__ out) {
  __shared__ double lds[HIPEIG_BLOCK];
  const double coef = q_prev ? t_prev[0] / t_prev[1] : 0.0;
  const int64_t n2 = n >> 1;
  double2* x2 = reinterpret_cast<double2*>(x);
  const double2* p2 = reinterpret_cast<const double2*>(q_prev);
  const double2* q2 = reinterpret_cast<const double2*>(q_next);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double a = 0.0, b = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    double2 xv = x2[i];
    if (q_prev) {
      const double2 pv = p2[i];
      xv.x = add_rn(xv.x, -mul_rn(pv.x, coef));
      xv.y = add_rn(xv.y, -mul_rn(pv.y, coef));
      x2[i] = xv;
    }
    if (q_next) {
      const double2 qv = q2[i];
      a = fma(xv.x, qv.x, a); a = fma(xv.y, qv.y, a);
      b = fma(qv.x, qv.x, b); b = fma(qv.y, qv.y, b);
    } else {
      a = fma(xv.x, xv.x, a); a = fma(xv.y, xv.y, a);
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    double xv = x[n - 1];
    if (q_prev) { xv = add_rn(xv, -mul_rn(q_prev[n - 1], coef)); x[n - 1] = xv; }
    if (q_next) { a = fma(xv, q_next[n - 1], a); b = fma(q_next[n - 1], q_next[n - 1], b); }
    else a = fma(xv, xv, a);
  }
  a = block_reduce_sum(a, lds);
  b = block_reduce_sum(b, lds);
  if (threadIdx.x == 0) {
    agent_store_nowait(partials + 2 * blockIdx.x, a);
    agent_store_nowait(partials + 2 * blockIdx.x + 1, b);
  }
  finish_records(partials, group_partials, 2, counters, lds, out);
}

extern "C" int hipeig_orthonormalize(hipeig_ctx* c, int64_t n, int m, const double* const* Y,
                                     double* x, double lindep, int method, double* innerprod,
                                     int* is_lindep) {
  HIPEIG_REQUIRE(innerprod && is_lindep, "null outputs");
  HIPEIG_REQUIRE(method == 0 || method == 1, "method must be 0 (MGS) or 1 (CGS2)");
  double ip = 0.0;
  if (method == 0) {
    // kernel j: update with q_{j-1}, dots with q_j; totals alternate between two slots of the scalar area (kernel j reads
    // slot j-1 while its last workgroup writes slot j); the last kernel's x.x goes to the host
    const int g = grid_records(c, n, "HIPEIG_MGS_PER_THREAD");
    unsigned* cnt = c->d_counters + 3 * HIPEIG_TICKET_WORDS;
    for (int j = 0; j <= m; ++j) {
      double* slot = (j == m) ? record_target(c, true) : c->d_scalars + SC_RECORDS + 2 * (j & 1);
      const double* prev = c->d_scalars + SC_RECORDS + 2 * ((j + 1) & 1);
      hipLaunchKernelGGL(mgs_sweep_kernel, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, x, j > 0 ? Y[j - 1] : nullptr, prev,
                         j < m ? Y[j] : nullptr, c->d_partials, c->d_group_partials, cnt, slot);
      HIPEIG_CHECK(hipGetLastError());
      if (j < m && c->collectives && hipeig_allreduce_sum(c, slot, 2)) return 4;
    }
    if (records_to_host(c, 1, &ip)) return 4;
  } else {
    const int cap = HIPEIG_MAX_COLS * HIPEIG_MAX_COLS;
    for (int pass = 0; pass < 2; ++pass) {
      for (int j0 = 0; j0 < m; j0 += cap) {
        const int mm = (m - j0 < cap) ? (m - j0) : cap;
        if (multi_dot_impl(c, n, mm, Y + j0, x, nullptr)) return 4;       // coefficients stay on the device
        if (lincomb_impl(c, n, mm, nullptr, c->d_scalars, -1.0, Y + j0, x, 1)) return 4;
      }
    }
  }
  if (method != 0) {
    int rc = hipeig_dot(c, n, x, x, &ip);
    if (rc) return rc;
  }
  *innerprod = ip;
  if (ip > lindep) {
    *is_lindep = 0;
    hipLaunchKernelGGL(scale_kernel, dim3(grid_stream(n)), dim3(HIPEIG_BLOCK), 0, c->stream, n, sqrt(ip), 1, x, x);
    HIPEIG_CHECK(hipGetLastError());
  } else {
    *is_lindep = 1;
  }
  return 0;
}
