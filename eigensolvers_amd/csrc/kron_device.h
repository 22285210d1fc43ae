// Kronecker-sum operator for gfx950:  H = sum_d  I (x) T_d (x) I  +  diag(V)  on a direct-product grid n_1 x ... x n_D
// (C order, last mode fastest), applied factor by factor.  For mode d the vector is the tensor [o_d, n_d, s_d],
// o_d = prod_{e<d} n_e, s_d = prod_{e>d} n_e, and the mode adds  Y[o, i, j] += sum_k T_d[i, k] X[o, k, j].
//
// One launch per mode, modes in ascending order; the first launch starts every row from V[r] * x[r] (one rounded product;
// 0 without V), the later ones from the running sum of the launches before, kept as fp64 in the operator's raw buffer.
// The epilogue of the caller (product, shifted product, a MINRES sweep) is carried over that buffer by the combine launch
// of sweep_launch.h.  Three kernel forms (kron.hip picks per mode; hipeig_kron_info says which):
//
//  * kron_inner_mfma_kernel (s_d >= 16): v_mfma_f64_16x16x4_f64 with A = a 16 x 4 tile of the padded T_d (32 rows of it are
//    staged in LDS per workgroup, all k, row stride kpad + 2: the 32 lanes of an operand read hit 32 distinct 8-byte banks)
//    and B = 4 rows k x 16 columns of X_o.  A wave owns 64 consecutive columns as four INTERLEAVED 16-column tiles - tile t
//    holds the columns j0 + 4 c + t, c = 0..15 - so that a lane loads and stores 4 consecutive doubles and the 16 lanes of a
//    row k read 512 contiguous bytes.  Rows k >= n_d and columns j >= s_d are masked to zero and never read or written.
//  * kron_last_mfma_kernel (s_d = 1):  Y[o, :] += X[o, :] T_d^T, the row index o is the M dimension.  A workgroup stages
//    the contiguous 64 x n_D slab of X (coalesced, zero padded) and 32 rows of T_d in LDS; A = 16 rows o x 4 k of the slab,
//    B[k][i] = T_d[i][k] - the same LDS read pattern as A.
//  * kron_plain_kernel (1 < s_d < 16, and n_d = 1): one thread per element, an ascending fma chain over k.
//
// f64 operand / result lane maps (as gram_tile_kernel, blas1.hip): A [lane & 15][lane >> 4], B [lane >> 4][lane & 15],
// C/D column lane & 15, row (lane >> 4) + 4 * reg.
//
// Order of the adds of one row, fixed by the dims alone: V x first, then mode 1, 2, ..., D; inside an MFMA mode the k-steps
// 0-3, 4-7, ... in ascending order, each one matrix-core instruction that adds its four products to the running sum in the
// hardware's fixed order (padded k add exact zeros); inside a plain mode k ascending.  No atomics, no dependence on the
// grid or on which wave owns a tile: bitwise reproducible.  Every term enters the sum once, so with m = sum_d n_d + 1
// roundings at most  |y_r - (H x)_r| <= gamma_m * (|V_r x_r| + sum_d sum_k |T_d[i_d, k]| |x_..k..|),  gamma_m = m u / (1 - m u).
#pragma once
#include "common.h"

#define KRON_MAX_MODES 8
#define KRON_MAX_N 208                   // (64 + 32) rows of kpad + 2 doubles fit the 160 KiB of LDS
#define KRON_IT 2                        // 16-row tiles of T_d staged per workgroup
#define KRON_JT 4                        // interleaved 16-column tiles per wave (inner form)
#define KRON_SLAB 64                     // rows o of X per workgroup (last-mode form)

typedef double kron_d4 __attribute__((ext_vector_type(4)));
typedef double kron_d2 __attribute__((ext_vector_type(2)));

struct KronMode {
  const double* __restrict__ t;          // padded factor: npad x kpad row-major, zero outside n x n
  int32_t n, npad, kpad;                 // npad: n rounded up to 16, kpad: to 4
  int64_t no, s;                         // o_d and s_d
};

// The value a row starts from in this launch.
__device__ __forceinline__ double kron_start(int first, const double* __restrict__ v, const double* __restrict__ x, const double* y,
                                             int64_t r) {
  if (!first) return y[r];
  return v ? mul_rn(v[r], x[r]) : 0.0;
}

// 32 (or the last 16) rows of the padded factor, all k, into LDS with row stride ld.
__device__ __forceinline__ void kron_stage_factor(const KronMode& m, int row0, int rows, int ld, double* ts) {
  for (int e = threadIdx.x; e < rows * m.kpad; e += HIPEIG_BLOCK) {
    const int r = e / m.kpad, k = e - r * m.kpad;
    ts[r * ld + k] = m.t[(size_t)(row0 + r) * m.kpad + k];
  }
}

// grid: x = ceil(no * ceil(s / 64) / 4) (a wave per (o, 64-column block)), y = ceil(npad / 32); LDS 32 * (kpad + 2) doubles.
// vec2: s is even and x, y are 16-byte aligned, so a lane's columns can move as two 16-byte accesses.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
kron_inner_mfma_kernel(KronMode m, const double* __restrict__ x, const double* __restrict__ v, double* y, int first, int vec2) {
  extern __shared__ double kron_lds[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ld = m.kpad + 2;
  const int row0 = blockIdx.y * (16 * KRON_IT);
  const int rows = m.npad - row0 < 16 * KRON_IT ? m.npad - row0 : 16 * KRON_IT;
  kron_stage_factor(m, row0, rows, ld, kron_lds);
  __syncthreads();                                               // the only barrier: a wave without an item leaves below
  const int64_t njb = (m.s + 63) >> 6;
  const int64_t item = (int64_t)blockIdx.x * 4 + wid;
  if (item >= m.no * njb) return;
  const int64_t o = item / njb;
  const int c = lane & 15, q = lane >> 4;
  const int64_t j = (item - o * njb) * 64 + 4 * c;               // this lane's columns j .. j + 3 (tile t: column j + t)
  const int64_t slab = o * m.n * m.s;
  const int ntile = rows >> 4;
  kron_d4 acc[KRON_IT][KRON_JT];
#pragma unroll
  for (int it = 0; it < KRON_IT; ++it)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = row0 + 16 * it + q + 4 * reg;
#pragma unroll
      for (int t = 0; t < KRON_JT; ++t)
        acc[it][t][reg] = (it < ntile && i < m.n && j + t < m.s) ? kron_start(first, v, x, y, slab + (int64_t)i * m.s + j + t) : 0.0;
    }
  for (int k0 = 0; k0 < m.kpad; k0 += 4) {
    const int k = k0 + q;
    double b[KRON_JT] = {0.0, 0.0, 0.0, 0.0};
    if (k < m.n) {
      const double* p = x + slab + (int64_t)k * m.s + j;
      if (vec2) {
        if (j < m.s) { const kron_d2 w = *reinterpret_cast<const kron_d2*>(p); b[0] = w.x; b[1] = w.y; }
        if (j + 2 < m.s) { const kron_d2 w = *reinterpret_cast<const kron_d2*>(p + 2); b[2] = w.x; b[3] = w.y; }
      } else {
#pragma unroll
        for (int t = 0; t < KRON_JT; ++t)
          if (j + t < m.s) b[t] = p[t];
      }
    }
#pragma unroll
    for (int it = 0; it < KRON_IT; ++it) {
      if (it < ntile) {
        const double a = kron_lds[(16 * it + c) * ld + k];
#pragma unroll
        for (int t = 0; t < KRON_JT; ++t) acc[it][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[t], acc[it][t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int it = 0; it < KRON_IT; ++it)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = row0 + 16 * it + q + 4 * reg;
      if (it >= ntile || i >= m.n) continue;
      double* p = y + slab + (int64_t)i * m.s + j;
      if (vec2) {
        if (j < m.s) *reinterpret_cast<kron_d2*>(p) = kron_d2{acc[it][0][reg], acc[it][1][reg]};
        if (j + 2 < m.s) *reinterpret_cast<kron_d2*>(p + 2) = kron_d2{acc[it][2][reg], acc[it][3][reg]};
      } else {
#pragma unroll
        for (int t = 0; t < KRON_JT; ++t)
          if (j + t < m.s) p[t] = acc[it][t][reg];
      }
    }
}

// grid: x = ceil(no / 64), y = ceil(npad / 32); LDS (64 + 32) * (kpad + 2) doubles: the slab of X, then the rows of T_d.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
kron_last_mfma_kernel(KronMode m, const double* __restrict__ x, const double* __restrict__ v, double* y, int first) {
  extern __shared__ double kron_lds[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ld = m.kpad + 2;
  double* xs = kron_lds;
  double* ts = kron_lds + KRON_SLAB * ld;
  const int64_t o0 = (int64_t)blockIdx.x * KRON_SLAB;
  const int nrow = m.no - o0 < KRON_SLAB ? (int)(m.no - o0) : KRON_SLAB;
  const int row0 = blockIdx.y * (16 * KRON_IT);
  const int rows = m.npad - row0 < 16 * KRON_IT ? m.npad - row0 : 16 * KRON_IT;
  for (int e = threadIdx.x; e < KRON_SLAB * m.kpad; e += HIPEIG_BLOCK) {      // rows past the end and k >= n: zeros, never read from x
    const int r = e / m.kpad, k = e - r * m.kpad;
    xs[r * ld + k] = (r < nrow && k < m.n) ? x[(o0 + r) * m.n + k] : 0.0;
  }
  kron_stage_factor(m, row0, rows, ld, ts);
  __syncthreads();                                               // the only barrier
  if (16 * wid >= nrow) return;
  const int c = lane & 15, q = lane >> 4;
  const int ntile = rows >> 4;
  kron_d4 acc[KRON_IT];
#pragma unroll
  for (int it = 0; it < KRON_IT; ++it)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = row0 + 16 * it + c;
      const int64_t o = o0 + 16 * wid + q + 4 * reg;
      acc[it][reg] = (it < ntile && i < m.n && o < m.no) ? kron_start(first, v, x, y, o * m.n + i) : 0.0;
    }
  for (int k0 = 0; k0 < m.kpad; k0 += 4) {
    const double a = xs[(16 * wid + c) * ld + k0 + q];
#pragma unroll
    for (int it = 0; it < KRON_IT; ++it) {
      if (it < ntile) {
        const double b = ts[(16 * it + c) * ld + k0 + q];
        acc[it] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[it], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int it = 0; it < KRON_IT; ++it)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = row0 + 16 * it + c;
      const int64_t o = o0 + 16 * wid + q + 4 * reg;
      if (it < ntile && i < m.n && o < m.no) y[o * m.n + i] = acc[it][reg];
    }
}

// One thread per element: short inner strides and singleton modes.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
kron_plain_kernel(KronMode m, int64_t total, const double* __restrict__ x, const double* __restrict__ v, double* y, int first) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < total; r += step) {
    const int64_t j = r % m.s, oi = r / m.s;
    const int64_t i = oi % m.n, o = oi / m.n;
    const double* xp = x + o * m.n * m.s + j;
    const double* tp = m.t + i * m.kpad;
    double acc = kron_start(first, v, x, y, r);
    for (int k = 0; k < m.n; ++k) acc = fma(tp[k], xp[(int64_t)k * m.s], acc);
    y[r] = acc;
  }
}

// d[r] = ((T_1[i_1, i_1] + T_2[i_2, i_2]) + ...) + V[r]: the order in which the explicit matrix is summed.
struct KronDiagArgs {
  int32_t D;
  int32_t n[KRON_MAX_MODES], off[KRON_MAX_MODES];                // size of mode d and where its diagonal starts in td
  const double* __restrict__ td;
  const double* __restrict__ v;                                  // may be null
};

__global__ void __launch_bounds__(HIPEIG_BLOCK)
kron_diagonal_kernel(KronDiagArgs a, int64_t total, double* __restrict__ d) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < total; r += step) {
    int32_t idx[KRON_MAX_MODES];
    int64_t rest = r;
#pragma unroll
    for (int e = KRON_MAX_MODES - 1; e >= 0; --e) {
      idx[e] = 0;
      if (e < a.D) { idx[e] = (int32_t)(rest % a.n[e]); rest /= a.n[e]; }
    }
    double acc = a.td[a.off[0] + idx[0]];
#pragma unroll
    for (int e = 1; e < KRON_MAX_MODES; ++e)
      if (e < a.D) acc = add_rn(acc, a.td[a.off[e] + idx[e]]);
    if (a.v) acc = add_rn(acc, a.v[r]);
    d[r] = acc;
  }
}
