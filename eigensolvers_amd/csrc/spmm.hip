// Block operands: interleaved [row][K] storage (K = 4 or 8), the TCOO-B layout build and the block
// product Y = H X (hipeig_spmm).  Kernel bodies live in spmm_device.h; the lock-step block MINRES
// (minres_block.hip) fuses its vector updates into the same sweeps.
#include <vector>
#include "block_sweep_launch.h"
#include "gcrot_precond_device.h"

struct PtrTable8 { const double* p[BCOO_KPACK]; };
struct OutTable8 { double* p[BCOO_KPACK]; };

// ---- interleave / de-interleave ---------------------------------------------------------
// Thread t owns the 16-byte pair (2t, 2t+1) of the block: row t / (K/2), operands 2(t % (K/2)) and the next,
// so the block side is one fully coalesced 16-byte access per lane and every column is touched in
// runs of 64 / (K/2) consecutive rows per wave instruction.  Missing operands (k < K) read as zero.
__device__ __forceinline__ const double* pick8(const PtrTable8& t, int j) {
  const double* p = t.p[0];
#pragma unroll
  for (int q = 1; q < BCOO_KPACK; ++q) p = (j == q) ? t.p[q] : p;
  return p;
}
__device__ __forceinline__ double* pick8(const OutTable8& t, int j) {
  double* p = t.p[0];
#pragma unroll
  for (int q = 1; q < BCOO_KPACK; ++q) p = (j == q) ? t.p[q] : p;
  return p;
}

template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
block_pack_kernel(int64_t n, int k, PtrTable8 cols, double* __restrict__ blk) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;           // multiple of K/2: the operand pair is fixed
  const int j0 = (int)((((int64_t)blockIdx.x * blockDim.x + threadIdx.x) % (K / 2)) * 2);
  const double* c0 = j0 < k ? pick8(cols, j0) : nullptr;
  const double* c1 = j0 + 1 < k ? pick8(cols, j0 + 1) : nullptr;
  double2* out = reinterpret_cast<double2*>(blk);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * (K / 2); t += stride) {
    const int64_t row = t / (K / 2);
    double2 v;
    v.x = c0 ? c0[row] : 0.0;
    v.y = c1 ? c1[row] : 0.0;
    out[t] = v;
  }
}

// The packs of the diagonally right-preconditioned GCROT products (hipeig_spmm_shift_m, hipeig_spmm_shift_pairs_zm): the
// block receives minv (.) x instead of x, scaled with DiagMul's element as the operands stream through, so the scaling costs
// the reads of minv and no pass of its own.  Same thread-to-element map as block_pack_kernel.
// Real operands, one real minv for all of them.
template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
block_pack_scaled_kernel(int64_t n, int k, PtrTable8 cols, const double* __restrict__ minv, double* __restrict__ blk) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int j0 = (int)((((int64_t)blockIdx.x * blockDim.x + threadIdx.x) % (K / 2)) * 2);
  const double* c0 = j0 < k ? pick8(cols, j0) : nullptr;
  const double* c1 = j0 + 1 < k ? pick8(cols, j0 + 1) : nullptr;
  double2* out = reinterpret_cast<double2*>(blk);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * (K / 2); t += stride) {
    const int64_t row = t / (K / 2);
    const double m = minv[row];
    double2 v;
    v.x = c0 ? DiagMul::real(m, c0[row]) : 0.0;
    v.y = c1 ? DiagMul::real(m, c1[row]) : 0.0;
    out[t] = v;
  }
}

// Complex operands as (re, im) columns 2p, 2p + 1 - a thread's 16-byte pair is one complex element - each with a minv of
// its own: M.p[2p] its real half, M.p[2p + 1] its imaginary half or null for a real minv.
template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
block_pack_pairs_scaled_kernel(int64_t n, int k, PtrTable8 cols, PtrTable8 M, double* __restrict__ blk) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int j0 = (int)((((int64_t)blockIdx.x * blockDim.x + threadIdx.x) % (K / 2)) * 2);
  const bool live = j0 + 1 < k;                                      // k is even: a complex operand is there or is not
  const double* c0 = live ? pick8(cols, j0) : nullptr;
  const double* c1 = live ? pick8(cols, j0 + 1) : nullptr;
  const double* m0 = live ? pick8(M, j0) : nullptr;
  const double* m1 = live ? pick8(M, j0 + 1) : nullptr;
  double2* out = reinterpret_cast<double2*>(blk);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * (K / 2); t += stride) {
    const int64_t row = t / (K / 2);
    double2 v{0.0, 0.0};
    if (live) DiagMul::pair(m0[row], m1 ? m1[row] : 0.0, m1 != nullptr, c0[row], c1[row], v.x, v.y);
    out[t] = v;
  }
}

template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
block_unpack_kernel(int64_t n, int k, const double* __restrict__ blk, OutTable8 cols) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int j0 = (int)((((int64_t)blockIdx.x * blockDim.x + threadIdx.x) % (K / 2)) * 2);
  double* c0 = j0 < k ? pick8(cols, j0) : nullptr;
  double* c1 = j0 + 1 < k ? pick8(cols, j0 + 1) : nullptr;
  const double2* in = reinterpret_cast<const double2*>(blk);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * (K / 2); t += stride) {
    const int64_t row = t / (K / 2);
    const double2 v = in[t];
    if (c0) c0[row] = v.x;
    if (c1) c1[row] = v.y;
  }
}

int hipeig_block_pack(hipeig_ctx* c, int K, int64_t n, int k, const double* const* cols, double* blk) {
  HIPEIG_REQUIRE((K == 4 || K == 8 || K == 16) && k >= 1 && k <= K, "a block holds 1..K operands, K = 4, 8 or 16");
  if (n == 0) return 0;
  PtrTable8 t;
  for (int j = 0; j < BCOO_KPACK; ++j) t.p[j] = j < k ? cols[j] : nullptr;
  const int g = grid_stream(n * (K / 2) * 2);
  if (K == 4) hipLaunchKernelGGL(block_pack_kernel<4>, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, k, t, blk);
  else if (K == 8) hipLaunchKernelGGL(block_pack_kernel<8>, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, k, t, blk);
  else hipLaunchKernelGGL(block_pack_kernel<16>, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, k, t, blk);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// Mre == nullptr: real operands scaled by the one vector `minv`; else k = 2 * (complex operands), columns (re, im), and
// Mre[p], Mim[p] (may be null) the minv of complex operand p.
static int block_pack_scaled(hipeig_ctx* c, int K, int64_t n, int k, const double* const* cols, const double* minv,
                             const double* const* Mre, const double* const* Mim, double* blk) {
  HIPEIG_REQUIRE((K == 4 || K == 8 || K == 16) && k >= 1 && k <= K, "a block holds 1..K operands, K = 4, 8 or 16");
  if (n == 0) return 0;
  PtrTable8 t, m;
  for (int j = 0; j < BCOO_KPACK; ++j) {
    t.p[j] = j < k ? cols[j] : nullptr;
    m.p[j] = (Mre && j < k) ? ((j & 1) ? Mim[j / 2] : Mre[j / 2]) : nullptr;
  }
  const int g = grid_stream(n * (K / 2) * 2);
  const dim3 grid(g), block(HIPEIG_BLOCK);
  if (Mre) {
    HIPEIG_REQUIRE(k % 2 == 0, "complex operands come as (re, im) columns");
    if (K == 4) hipLaunchKernelGGL(block_pack_pairs_scaled_kernel<4>, grid, block, 0, c->stream, n, k, t, m, blk);
    else if (K == 8) hipLaunchKernelGGL(block_pack_pairs_scaled_kernel<8>, grid, block, 0, c->stream, n, k, t, m, blk);
    else hipLaunchKernelGGL(block_pack_pairs_scaled_kernel<16>, grid, block, 0, c->stream, n, k, t, m, blk);
  } else {
    if (K == 4) hipLaunchKernelGGL(block_pack_scaled_kernel<4>, grid, block, 0, c->stream, n, k, t, minv, blk);
    else if (K == 8) hipLaunchKernelGGL(block_pack_scaled_kernel<8>, grid, block, 0, c->stream, n, k, t, minv, blk);
    else hipLaunchKernelGGL(block_pack_scaled_kernel<16>, grid, block, 0, c->stream, n, k, t, minv, blk);
  }
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

int hipeig_block_unpack(hipeig_ctx* c, int K, int64_t n, int k, const double* blk, double* const* cols) {
  HIPEIG_REQUIRE((K == 4 || K == 8 || K == 16) && k >= 1 && k <= K, "a block holds 1..K operands, K = 4, 8 or 16");
  if (n == 0) return 0;
  OutTable8 t;
  for (int j = 0; j < BCOO_KPACK; ++j) t.p[j] = j < k ? cols[j] : nullptr;
  const int g = grid_stream(n * (K / 2) * 2);
  if (K == 4) hipLaunchKernelGGL(block_unpack_kernel<4>, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, k, blk, t);
  else if (K == 8) hipLaunchKernelGGL(block_unpack_kernel<8>, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, k, blk, t);
  else hipLaunchKernelGGL(block_unpack_kernel<16>, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, k, blk, t);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// ---- TCOO-B ---------------------------------------------------------------------------------
BcooView hipeig_bcoo_view(const hipeig_csr* A, const BlockedLayout& L) {
  BcooView t;
  t.idx = L.idx; t.val = L.val; t.off = L.off;
  t.nunits = L.nunits; t.nwin = L.nwin; t.wbits = L.wbits; t.rw = L.rw;
  t.unit_begin = 0;
  t.nrows = A->nrows;
  return t;
}

// Decide between the window-blocked and the row-owner block kernel for interleave width K and build the
// former's layout (idempotent).  Returns 2 (TCOO-B) or 1 (row-owner), -1 on failure.  The dense block sweep (3) is taken
// only when pinned, after reserving the dense copy; an operator or context it does not suit is refused (-1), not replaced.
// for_solve: the caller is the block MINRES, whose sweeps leave per-workgroup partials - it cannot take a layout that needs
// more than HIPEIG_MAX_PARTIALS workgroups per product and keeps the row-owner kernel there (N = 1e7: 16 sweeps of 256).
int hipeig_block_pick_variant(hipeig_ctx* c, hipeig_csr* A, int K, int for_solve) {
  BlockedLayout& L = A->b[layout_slot(K)];
  A->last_block_k = K;
  if (A->block_variant == 3) return hipeig_dense_reserve(c, A) ? -1 : (A->last_block_variant = 3);
  if (A->block_variant == 1 || A->nnz == 0 || A->nrows == 0) return A->last_block_variant = 1;
  // an operator pinned to a reproducible kernel (variants 1-3, 5) keeps that promise for block products and block
  // solves too: the row-owner kernel adds a row's terms in a fixed order, the window-blocked one uses fp64 atomics
  if (A->block_variant == 0 && (A->reproducible || (A->variant != 0 && A->variant != 4))) return A->last_block_variant = 1;
  auto fits_solve = [](const BlockedLayout& l) {
    const SweepGrid g = blocked_grid(l);
    return (int64_t)g.launches * g.wgs <= HIPEIG_MAX_PARTIALS;
  };
  if (L.state == 1) return A->last_block_variant = (for_solve && A->block_variant == 0 && !fits_solve(L)) ? 1 : 2;
  if (L.state == 2 && A->block_variant == 0) return A->last_block_variant = 1;
  int wbits = K == 16 ? 10 : K == 8 ? 11 : 12;           // 128 KiB of the operand block per window (measured best of 2^8..2^15 rows at N = 1e6,
                                                         // K = 8: 32 windows fit one L2, so workgroups that drift apart still hit)
  if (const char* e = getenv("HIPEIG_BCOO_WBITS")) wbits = atoi(e);          // tuning knob
  if (wbits < 8 || wbits > 20) { hipeig_set_error("HIPEIG_BCOO_WBITS out of range"); return -1; }
  while (wbits > 8 && ((int64_t)1 << (wbits - 1)) >= A->gather_len) --wbits;
  int64_t nwin = (A->gather_len + ((int64_t)1 << wbits) - 1) >> wbits;
  while (nwin > BCOO_MAX_WIN && wbits < 20) { ++wbits; nwin = (A->gather_len + ((int64_t)1 << wbits) - 1) >> wbits; }
  int64_t rw_max = ((int64_t)HIPEIG_BCOO_LDS_MAX - (nwin + 2) * 4) / (K * 8);
  if (rw_max > ((int64_t)1 << (32 - wbits)) - 1) rw_max = ((int64_t)1 << (32 - wbits)) - 1;    // 0xFFFFFFFF stays the padding mark
  int64_t sweeps = (A->nrows + (int64_t)c->num_cu * rw_max - 1) / ((int64_t)c->num_cu * rw_max);
  if (sweeps < 1) sweeps = 1;
  int64_t rw = (A->nrows + sweeps * c->num_cu - 1) / (sweeps * c->num_cu);
  if (rw < 8) rw = 8;
  if (rw > rw_max) rw = rw_max;
  if (const char* e = getenv("HIPEIG_BCOO_RW")) { rw = atoi(e); if (rw < 1 || rw > rw_max) { hipeig_set_error("HIPEIG_BCOO_RW out of range"); return -1; } }
  // L2 reuse of the operand lines inside one XCD (32 workgroups share a window): round 2 kept the windows only above ~2
  // touches per line (spmm_device.h).  Round 4 measured the other end (tools/experiments/pair_block_width.py, block_bench.py):
  // once the operand block has outgrown the 256 MiB Infinity Cache the row-owner kernel's gathers go to HBM one line each
  // and the windows win although hardly a line is touched twice - N = 1e7: K = 8 15.2 -> 11.8 ms per product, 8 complex
  // operands (K = 16) 2.90 -> 1.85 ms per operand - and the 16-wide block wins with them at N = 1e6 too (0.134 -> 0.109).
  // A block that fits one L2 needs no windows.
  const double rows_per_line = 128.0 / (K * 8);
  const double touches = 32.0 * (double)rw * ((double)A->nnz / (double)A->nrows) * rows_per_line / (double)A->gather_len;
  const bool fits_l2 = A->gather_len * (int64_t)(K * 8) <= ((int64_t)3 << 20);
  const bool beyond_mall = A->gather_len * (int64_t)(K * 8) > ((int64_t)256 << 20);
  if (A->block_variant == 0 && (fits_l2 || (touches < 2.0 && !beyond_mall && K != 16))) {
    L.state = 2;
    return A->last_block_variant = 1;
  }
  BlockedLayout G{};
  G.nunits = (int)((A->nrows + rw - 1) / rw); G.nwin = (int)nwin; G.wbits = wbits; G.rw = (int)rw;
  G.binbits = wbits;                                     // one bin per window
  G.wgs_per_sweep = c->num_cu;                           // one 1024-thread workgroup (all of the LDS) per CU
  G.csplit = 1;
  // would the layout fit the solve?  state stays undecided: a product may still build it
  if (for_solve && A->block_variant == 0 && !fits_solve(G)) return A->last_block_variant = 1;
  const int rc = hipeig_build_binned(c, A, G, 0, &L);
  if (rc == 2) { L.state = 2; return A->last_block_variant = 1; }
  if (rc) return -1;
  L.state = 1;
  return A->last_block_variant = 2;
}

// All-gather of an interleaved block of width K into the layout the remapped column indices address (the chunk-major
// layout of the single-vector exchange, K doubles per position; comm.hip).  Single rank: the local block is the operand.
int hipeig_block_allgather(hipeig_ctx* c, hipeig_csr* A, int K, const double* xb_local, const double** xb_full) {
  if (!c->collectives) { *xb_full = xb_local; return 0; }
  HIPEIG_REQUIRE(A->col_stride > 0 && A->gl.h * A->gl.nchunks >= A->nrows, "operator was not prepared for this communicator");
  return hipeig_allgather_block(c, A->gl, K, xb_local, A->nrows, xb_full);
}

// ---- plain block product -------------------------------------------------------------------
template <int K>
struct StoreBlockEpilogue {
  double* __restrict__ Y;
  __device__ __forceinline__ void elem(int64_t r, int j, double sum, double& acc) const { Y[r * K + j] = sum; }
};

// Columns (2p, 2p + 1) of the block are the real and imaginary halves of complex operand p; the epilogue applies the
// complex shift of a contour solve, y_p = sign*(z*x_p - H x_p) (feast.py:83-90 -> numpyVector.py:152-161), with the
// roundings of PairEpilogue (spmv.hip): the real part of the shift and the operator sum separately, then the zi term.
// xl: the packed operand block restricted to this operator's rows.
template <int K>
struct ShiftPairBlockEpilogue {
  double ar, ai, as;                                   // sign*zr, sign*zi, -sign
  const double* __restrict__ xl;
  double* __restrict__ Y;
  __device__ __forceinline__ void elem(int64_t r, int j, double sum, double& acc) const {
    const int64_t base = r * K + (j & ~1);
    const double vr = xl[base], vi = xl[base + 1];
    const double own = (j & 1) ? vi : vr;
    const double t = add_rn(mul_rn(ar, own), mul_rn(as, sum));
    Y[r * K + j] = (j & 1) ? fma(ai, vr, t) : fma(-ai, vi, t);
  }
};

// The same product with a shift PER OPERAND: the solves of different contour points are independent (feast.py:189-200),
// so one block may carry operands of several points.  ar[p], ai[p] = sign*zr_p, sign*zi_p of complex operand p (columns
// 2p, 2p + 1); the operator sum of a column does not depend on the shift, and per element the arithmetic and its roundings
// are those of ShiftPairBlockEpilogue.  The operand index is a per-thread value: the shift is picked by an unrolled
// compare chain over the kernel arguments (selects between scalar registers, no indexed copy of the array in scratch).
template <int K>
struct ShiftPairsZBlockEpilogue {
  double ar[K / 2], ai[K / 2];                         // sign*zr_p, sign*zi_p; unused operands: 0
  double as;                                           // -sign
  const double* __restrict__ xl;
  double* __restrict__ Y;
  __device__ __forceinline__ void elem(int64_t r, int j, double sum, double& acc) const {
    const int p = j >> 1;
    double a_r = ar[0], a_i = ai[0];
#pragma unroll
    for (int q = 1; q < K / 2; ++q) {
      a_r = (p == q) ? ar[q] : a_r;
      a_i = (p == q) ? ai[q] : a_i;
    }
    const int64_t base = r * K + (j & ~1);
    const double vr = xl[base], vi = xl[base + 1];
    const double own = (j & 1) ? vi : vr;
    const double t = add_rn(mul_rn(a_r, own), mul_rn(as, sum));
    Y[r * K + j] = (j & 1) ? fma(a_i, vr, t) : fma(-a_i, vi, t);
  }
};

// The real shift of a lock-step GCROT solve, y_j = sign*(sigma*x_j - (H X)_j) (numpyVector.py:152/161 for the nBlock
// right-hand sides of inexact_Lanczos.py:319-320), with the roundings of AxpyEpilogue (spmv.hip): the shift term and the
// operator sum separately, then their sum - a column differs from hipeig_spmv_shift only through the operator sum.
// a_self = sign*sigma, a_sum = -sign; xl: the packed operand block restricted to this operator's rows.
template <int K>
struct ShiftBlockEpilogue {
  double a_self, a_sum;
  const double* __restrict__ xl;
  double* __restrict__ Y;
  __device__ __forceinline__ void elem(int64_t r, int j, double sum, double& acc) const {
    const int64_t i = r * K + j;
    const double t = (a_self == 0.0) ? 0.0 : mul_rn(a_self, xl[i]);
    Y[i] = add_rn(t, mul_rn(a_sum, sum));
  }
};

template <int K, class Epi>
__global__ void __launch_bounds__(BCOO_THREADS)
spmm_bcoo_kernel(BcooView T, const double* __restrict__ X, Epi epi) {
  extern __shared__ double bcoo_lds[];
  double acc = 0.0;
  bcoo_wg_sweep<K>(T, X, epi, acc, bcoo_lds);
}

template <int K, class Epi>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
spmm_dense_kernel(DenseView D, const double* __restrict__ X, Epi epi) {
  double acc = 0.0;
  dense_block_sweep<K>(D, X, epi, acc);
}

template <int K, class Epi>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
spmm_rowowner_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const double* __restrict__ val,
                     int64_t nrows, const double* __restrict__ X, Epi epi) {
  double acc = 0.0;
  csr_rowowner_block_sweep<K>(rowptr, col, val, nrows, X, epi, acc);
}

int hipeig_rowowner_grid(const hipeig_ctx* c, const hipeig_csr* A) {
  int64_t g = (A->nrows + 3) / 4;
  if (g > 8 * (int64_t)c->num_cu) g = 8 * (int64_t)c->num_cu;
  if (g > HIPEIG_MAX_PARTIALS) g = HIPEIG_MAX_PARTIALS;
  return g < 1 ? 1 : (int)g;
}

// Block product on interleaved blocks of width K (local rows) with the epilogue `epi`; Xb is this rank's slice.
template <int K, class Epi>
static int spmm_block_run(hipeig_ctx* c, hipeig_csr* A, const double* Xb, const Epi& epi) {
  if (A->nrows == 0) return 0;
  BlockSweepPlan plan;
  if (const int rc = block_sweep_plan_build<K>(c, A, 0, &plan)) return rc;
  const double* xg = nullptr;
  if (hipeig_block_allgather(c, A, K, Xb, &xg)) return 4;
  if (const int rc = block_sweep_set_lds_limit(plan, spmm_bcoo_kernel<K, Epi>)) return rc;
  block_sweep_launch(c, plan, [&](auto v, int grid, int threads, size_t lds, const BcooView& tv, int) {
    if constexpr (decltype(v)::value == 2)
      hipLaunchKernelGGL((spmm_bcoo_kernel<K, Epi>), dim3(grid), dim3(threads), lds, c->stream, tv, xg, epi);
    else if constexpr (decltype(v)::value == 3)
      hipLaunchKernelGGL((spmm_dense_kernel<K, Epi>), dim3(grid), dim3(threads), lds, c->stream, plan.dview, xg, epi);
    else
      hipLaunchKernelGGL((spmm_rowowner_kernel<K, Epi>), dim3(grid), dim3(threads), lds, c->stream,
                         A->d_rowptr, A->d_col, A->d_val, A->nrows, xg, epi);
  });
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// Yb = H Xb
template <int K>
static int spmm_block_impl(hipeig_ctx* c, hipeig_csr* A, const double* Xb, double* Yb) {
  return spmm_block_run<K>(c, A, Xb, StoreBlockEpilogue<K>{Yb});
}

static int ensure_blk_ws(hipeig_ctx* c, size_t doubles) {
  if (c->blk_ws_doubles >= doubles) return 0;
  if (c->blk_ws) HIPEIG_CHECK(hipFree(c->blk_ws));
  c->blk_ws = nullptr; c->blk_ws_doubles = 0;
  HIPEIG_CHECK(hipMalloc((void**)&c->blk_ws, doubles * sizeof(double)));
  c->blk_ws_doubles = doubles;
  return 0;
}

extern "C" int hipeig_spmm(hipeig_ctx* c, hipeig_csr* A, int k, const double* const* X, double* const* Y) {
  HIPEIG_REQUIRE(k >= 1 && X && Y, "bad arguments");
  if (A->nrows == 0) return 0;
  if (c->collectives && !c->comm && !c->loop) {
    // a communicator without RCCL has no exchange for block operands: k products through the direct exchange instead
    for (int j = 0; j < k; ++j)
      if (hipeig_spmv(c, A, X[j], Y[j])) return 1;
    return 0;
  }
  // operand slice: a partitioned run hands over local slices; a row slab applied to full-length
  // operands (single process) gathers from the whole operand, so the block has ncols rows
  const int64_t nx = c->collectives ? A->nrows : A->ncols;
  const int64_t ny = A->nrows;
  if (ensure_blk_ws(c, (size_t)(nx + ny) * BCOO_KMAX)) return 1;
  double* Xi = c->blk_ws;
  double* Yi = c->blk_ws + (size_t)nx * BCOO_KMAX;
  for (int j0 = 0; j0 < k;) {
    const int K = (k - j0 <= 4) ? 4 : 8;                     // blocks of <= 4 take the narrow interleave (twice the rows per workgroup)
    const int kk = (k - j0 < K) ? k - j0 : K;
    if (hipeig_block_pack(c, K, nx, kk, X + j0, Xi)) return 1;
    if (K == 4 ? spmm_block_impl<4>(c, A, Xi, Yi) : spmm_block_impl<8>(c, A, Xi, Yi)) return 1;
    if (hipeig_block_unpack(c, K, ny, kk, Yi, Y + j0)) return 1;
    j0 += kk;
  }
  return 0;
}

// The real shifted operator of the lock-step GCROT solves (the nBlock solves of one block Lanczos iteration share operator
// and shift, inexact_Lanczos.py:319-320): Y_j = sign*(sigma*X_j - H X_j), j < k, the shift applied in the block product's
// epilogue.  Kernel choice, chunking (8 operands per pass, 4 for a remainder of <= 4) and the contexts taken are those of
// hipeig_spmm; a context without a block exchange runs hipeig_spmv_shift per operand.
extern "C" int hipeig_spmm_shift(hipeig_ctx* c, hipeig_csr* A, int k, double sigma, double sign,
                                 const double* const* X, double* const* Y) {
  HIPEIG_REQUIRE(k >= 1 && X && Y, "bad arguments");
  HIPEIG_REQUIRE(sign == 1.0 || sign == -1.0, "sign must be +1 or -1");
  if (A->nrows == 0) return 0;
  if (c->collectives && !c->comm && !c->loop) {
    for (int j = 0; j < k; ++j)
      if (hipeig_spmv_shift(c, A, sigma, sign, X[j], Y[j])) return 1;
    return 0;
  }
  const int64_t nx = c->collectives ? A->nrows : A->ncols;
  const int64_t ny = A->nrows;
  const int64_t xoff = c->collectives ? 0 : A->row_offset;      // the shift term reads this operator's rows of the block
  if (ensure_blk_ws(c, (size_t)(nx + ny) * BCOO_KMAX)) return 1;
  double* Xi = c->blk_ws;
  double* Yi = c->blk_ws + (size_t)nx * BCOO_KMAX;
  const double a_self = sign * sigma, a_sum = -sign;
  for (int j0 = 0; j0 < k;) {
    const int K = (k - j0 <= 4) ? 4 : 8;
    const int kk = (k - j0 < K) ? k - j0 : K;
    if (hipeig_block_pack(c, K, nx, kk, X + j0, Xi)) return 1;
    if (K == 4 ? spmm_block_run<4>(c, A, Xi, ShiftBlockEpilogue<4>{a_self, a_sum, Xi + xoff * 4, Yi})
               : spmm_block_run<8>(c, A, Xi, ShiftBlockEpilogue<8>{a_self, a_sum, Xi + xoff * 8, Yi})) return 1;
    if (hipeig_block_unpack(c, K, ny, kk, Yi, Y + j0)) return 1;
    j0 += kk;
  }
  return 0;
}

template <int K>
static ShiftPairsZBlockEpilogue<K> shift_pairs_z_epilogue(const double* zr, const double* zi, int np, double sign,
                                                          const double* xl, double* Y) {
  ShiftPairsZBlockEpilogue<K> e{};
  for (int p = 0; p < np && p < K / 2; ++p) { e.ar[p] = sign * zr[p]; e.ai[p] = sign * zi[p]; }
  e.as = -sign; e.xl = xl; e.Y = Y;
  return e;
}

// The complex matvec of the contour solves for SEVERAL right-hand sides at once (feast.py:198-200: the m0 solves of one
// contour point share operator and shift): y_p = sign*(z*x_p - H x_p), p < npairs, complex operands as (re, im) buffers.
// Four complex operands fill an 8-wide block (two a 4-wide one), so the (index, value) stream of the operator is read
// once per four operands instead of once each; the shift is applied in the block product's epilogue.  A row-partitioned
// or direct-only context and npairs = 1 take hipeig_spmv_shift_pair per operand.
// zr, zi: one shift for all operands (zstride = 0) or npairs of them (zstride = 1; hipeig_spmm_shift_pairs_z below).
// Mre, Mim (hipeig_spmm_shift_pairs_zm only): operand p is scaled by its minv (Mre[p], Mim[p] or null) on its way into the
// block; without them the pack, and everything else, is what it was.
static int spmm_shift_pairs_impl(hipeig_ctx* c, hipeig_csr* A, int npairs, const double* zr, const double* zi, int zstride, double sign,
                                 const double* const* Xre, const double* const* Xim, double* const* Yre, double* const* Yim,
                                 const double* const* Mre = nullptr, const double* const* Mim = nullptr) {
  HIPEIG_REQUIRE(npairs >= 1 && zr && zi && Xre && Xim && Yre && Yim, "bad arguments");
  HIPEIG_REQUIRE(sign == 1.0 || sign == -1.0, "sign must be +1 or -1");
  if (A->nrows == 0) return 0;
  if (Mre && npairs == 1) {                           // scale into the workspace, then the single pair product
    const int64_t n = A->ncols;
    const size_t half = ((size_t)n + 1) & ~(size_t)1;  // keeps the second half 16-byte aligned
    if (ensure_blk_ws(c, 2 * half)) return 1;
    if (hipeig_pair_diag_mul(c, n, Mre[0], Mim[0], Xre[0], Xim[0], c->blk_ws, c->blk_ws + half)) return 1;
    return hipeig_spmv_shift_pair(c, A, zr[0], zi[0], sign, c->blk_ws, c->blk_ws + half, Yre[0], Yim[0]);
  }
  if (npairs == 1 || c->collectives) {
    for (int p = 0; p < npairs; ++p)
      if (hipeig_spmv_shift_pair(c, A, zr[p * zstride], zi[p * zstride], sign, Xre[p], Xim[p], Yre[p], Yim[p])) return 1;
    return 0;
  }
  const int64_t nx = A->ncols, ny = A->nrows;
  // complex operands per pass over the operator: 4 (an 8-wide block, 64 B per operand row: a gather uses half a line) or 8
  // (16 wide, 128 B = one whole line per gather; HIPEIG_PAIR_BLOCK_WIDTH, see EXPERIMENTS.md R4-block16)
  // Measured per complex operand, 4 / 8 per pass (tools/experiments/pair_block_width.py): N = 1e6 0.107 / 0.109, 2e6 0.387 /
  // 0.365, 4e6 0.933 / 0.973, 1e7 2.98 / 1.85 ms (single pair products: 0.177 / 0.51 / 1.46 / 3.94).  Within +-6 % while the
  // 8-wide block (64 B per row) still sits in the 256 MiB Infinity Cache; once it does not, its gathers pay a whole line from
  // HBM for half a line of data and the 16-wide block wins by 38 %.
  int wide = (nx * (int64_t)64 > ((int64_t)288 << 20)) ? 8 : 4;
  if (const char* e = getenv("HIPEIG_PAIR_BLOCK_WIDTH")) wide = atoi(e) >= 8 ? 8 : 4;
  if (ensure_blk_ws(c, (size_t)(nx + ny) * BCOO_KPACK)) return 1;
  double* Xi = c->blk_ws;
  double* Yi = c->blk_ws + (size_t)nx * BCOO_KPACK;
  const double as = -sign;
  for (int p0 = 0; p0 < npairs;) {
    const int left = npairs - p0;
    const int np = (wide == 8 && left > 4) ? (left < 8 ? left : 8) : (left < 4 ? left : 4);
    const int K = (np <= 2) ? 4 : (np <= 4) ? 8 : 16;
    const double* cols[BCOO_KPACK];
    double* outs[BCOO_KPACK];
    for (int p = 0; p < np; ++p) {
      cols[2 * p] = Xre[p0 + p]; cols[2 * p + 1] = Xim[p0 + p];
      outs[2 * p] = Yre[p0 + p]; outs[2 * p + 1] = Yim[p0 + p];
    }
    if (Mre ? block_pack_scaled(c, K, nx, 2 * np, cols, nullptr, Mre + p0, Mim + p0, Xi)
            : hipeig_block_pack(c, K, nx, 2 * np, cols, Xi)) return 1;
    int rc;
    if (zstride == 0) {
      const double ar = sign * zr[0], ai = sign * zi[0];
      if (K == 4) rc = spmm_block_run<4>(c, A, Xi, ShiftPairBlockEpilogue<4>{ar, ai, as, Xi + A->row_offset * 4, Yi});
      else if (K == 8) rc = spmm_block_run<8>(c, A, Xi, ShiftPairBlockEpilogue<8>{ar, ai, as, Xi + A->row_offset * 8, Yi});
      else rc = spmm_block_run<16>(c, A, Xi, ShiftPairBlockEpilogue<16>{ar, ai, as, Xi + A->row_offset * 16, Yi});
    } else if (K == 4) rc = spmm_block_run<4>(c, A, Xi, shift_pairs_z_epilogue<4>(zr + p0, zi + p0, np, sign, Xi + A->row_offset * 4, Yi));
    else if (K == 8) rc = spmm_block_run<8>(c, A, Xi, shift_pairs_z_epilogue<8>(zr + p0, zi + p0, np, sign, Xi + A->row_offset * 8, Yi));
    else rc = spmm_block_run<16>(c, A, Xi, shift_pairs_z_epilogue<16>(zr + p0, zi + p0, np, sign, Xi + A->row_offset * 16, Yi));
    if (rc) return rc;
    if (hipeig_block_unpack(c, K, ny, 2 * np, Yi, outs)) return 1;
    p0 += np;
  }
  return 0;
}

extern "C" int hipeig_spmm_shift_pairs(hipeig_ctx* c, hipeig_csr* A, int npairs, double zr, double zi, double sign,
                                       const double* const* Xre, const double* const* Xim, double* const* Yre, double* const* Yim) {
  return spmm_shift_pairs_impl(c, A, npairs, &zr, &zi, 0, sign, Xre, Xim, Yre, Yim);
}

// The same with a shift per operand, y_p = sign*(z_p*x_p - H x_p): the solves of ALL contour points of a FEAST iteration
// are independent (feast.py:189-200), so operands of different points may share a pass over the operator.  zr, zi: host
// arrays of npairs shifts.  Chunking, the width rule and the per-operand fallbacks are those of hipeig_spmm_shift_pairs.
extern "C" int hipeig_spmm_shift_pairs_z(hipeig_ctx* c, hipeig_csr* A, int npairs, const double* zr, const double* zi, double sign,
                                         const double* const* Xre, const double* const* Xim, double* const* Yre, double* const* Yim) {
  return spmm_shift_pairs_impl(c, A, npairs, zr, zi, 1, sign, Xre, Xim, Yre, Yim);
}

// ---- the products of the diagonally right-preconditioned GCROT solves (gcrot_precond.hip) -----------------
static int whole_operator_without_collectives(const hipeig_ctx* c, const hipeig_csr* A) {
  HIPEIG_REQUIRE(!c->collectives, "the preconditioned GCROT products run on one GPU: a context with collectives is not implemented");
  HIPEIG_REQUIRE(A->nrows == A->ncols && A->row_offset == 0, "the preconditioned GCROT products need a whole square operator");
  return 0;
}

// hipeig_spmm_shift on T_j = minv (.) X_j: Y_j = sign*(sigma*T_j - H T_j), T_j formed while the operands are packed.  The
// chunking, the sweep and ShiftBlockEpilogue are hipeig_spmm_shift's.
extern "C" int hipeig_spmm_shift_m(hipeig_ctx* c, hipeig_csr* A, int k, double sigma, double sign, const double* minv,
                                   const double* const* X, double* const* Y) {
  HIPEIG_REQUIRE(k >= 1 && minv && X && Y, "bad arguments");
  HIPEIG_REQUIRE(sign == 1.0 || sign == -1.0, "sign must be +1 or -1");
  if (whole_operator_without_collectives(c, A)) return 1;
  if (A->nrows == 0) return 0;
  const int64_t n = A->nrows;
  if (ensure_blk_ws(c, (size_t)(2 * n) * BCOO_KMAX)) return 1;
  double* Xi = c->blk_ws;
  double* Yi = c->blk_ws + (size_t)n * BCOO_KMAX;
  const double a_self = sign * sigma, a_sum = -sign;
  for (int j0 = 0; j0 < k;) {
    const int K = (k - j0 <= 4) ? 4 : 8;
    const int kk = (k - j0 < K) ? k - j0 : K;
    if (block_pack_scaled(c, K, n, kk, X + j0, minv, nullptr, nullptr, Xi)) return 1;
    if (K == 4 ? spmm_block_run<4>(c, A, Xi, ShiftBlockEpilogue<4>{a_self, a_sum, Xi, Yi})
               : spmm_block_run<8>(c, A, Xi, ShiftBlockEpilogue<8>{a_self, a_sum, Xi, Yi})) return 1;
    if (hipeig_block_unpack(c, K, n, kk, Yi, Y + j0)) return 1;
    j0 += kk;
  }
  return 0;
}

// hipeig_spmm_shift_pairs_z on t_p = Minv_p (.) x_p, a minv per operand: y_p = sign*(z_p*t_p - H t_p).
extern "C" int hipeig_spmm_shift_pairs_zm(hipeig_ctx* c, hipeig_csr* A, int npairs, const double* zr, const double* zi, double sign,
                                          const double* const* Mre, const double* const* Mim,
                                          const double* const* Xre, const double* const* Xim, double* const* Yre, double* const* Yim) {
  HIPEIG_REQUIRE(Mre && Mim, "bad arguments");
  for (int p = 0; p < npairs; ++p) HIPEIG_REQUIRE(Mre[p] != nullptr, "every operand needs the real half of its minv");
  if (whole_operator_without_collectives(c, A)) return 1;
  return spmm_shift_pairs_impl(c, A, npairs, zr, zi, 1, sign, Xre, Xim, Yre, Yim, Mre, Mim);
}

extern "C" int hipeig_csr_block_info(hipeig_csr* A, int64_t info[4]) {
  const BlockedLayout& L = A->b[layout_slot(A->last_block_k == 4 ? 4 : A->last_block_k == 16 ? 16 : 8)];
  info[0] = A->last_block_variant; info[1] = L.nunits; info[2] = L.nwin; info[3] = L.rw;
  return 0;
}

extern "C" int hipeig_csr_set_block_variant(hipeig_csr* A, int variant) {
  HIPEIG_REQUIRE(variant >= 0 && variant <= 3, "unknown block variant (0 auto, 1 row-owner, 2 window-blocked, 3 dense)");
  if (variant == 3 && hipeig_dense_refusal(nullptr, A)) return 2;   // what the operator alone shows; the context at first use
  A->block_variant = variant;
  return 0;
}
