// Mode transforms of the separable (fast-diagonalisation) preconditioner of the Kronecker-sum operator for gfx950:
//   M^-1 = Q S Q^T,  Q = Q_1 (x) ... (x) Q_D,  S = diag(sinv)      
// One launch per mode,  Z[o, i, j] = sum_k Q[i, k] X[o, k, j],  OUT of place (kron_device.h adds into a running sum; here
// every launch starts its rows from zero and writes another vector).  The three forms of kron_device.h, picked by the
// same rule (kron_precond.hip), with its staging helper, its constants, its tile and lane maps and its masks:
//   kp_inner_mfma_kernel (s_d >= 16), kp_last_mfma_kernel (s_d = 1), kp_plain_kernel (1 < s_d < 16 and n_d = 1).
// Epilogue (template SCALE): 0 stores the sum, 1 stores mul_rn(sinv[r], sum) - the last forward mode of an apply, so that
// S costs no launch of its own.
//
// Order of the adds of one element, fixed by the dims alone: from zero, the k-steps 0-3, 4-7, ... in ascending order, each
// one v_mfma_f64_16x16x4_f64 (padded k add exact zeros); in the plain form k ascending.  No atomics, no scratch, no
// dependence on the grid: bitwise reproducible, and with n_d products and n_d adds per element
//   |z - Q x|_i <= gamma_{n_d + 2} sum_k |Q[i, k]| |x_k|.
//
// `st`: inside a MINRES iteration the state record KC left; a launch past the stop returns at once (null: always runs).
#pragma once
#include "common.h"

// kron_device.h defines its kernels with external linkage for kron.hip.  This is a second translation unit that needs its
// helpers and kron_diagonal_kernel, so it takes the header into an unnamed namespace: the same source, internal linkage.
namespace {
#include "kron_device.h"

// grid and LDS as kron_inner_mfma_kernel
template <int SCALE>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
kp_inner_mfma_kernel(KronMode m, const double* __restrict__ x, double* __restrict__ z, const double* __restrict__ sinv,
                     const MinresState* __restrict__ st, int vec2) {
  extern __shared__ double kron_lds[];
  if (st && st->done) return;                                    // uniform: before the barrier
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
    for (int t = 0; t < KRON_JT; ++t) acc[it][t] = kron_d4{0.0, 0.0, 0.0, 0.0};
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
      const int64_t r = slab + (int64_t)i * m.s + j;
      double v[KRON_JT];
#pragma unroll
      for (int t = 0; t < KRON_JT; ++t) {
        v[t] = acc[it][t][reg];
        if (SCALE && j + t < m.s) v[t] = mul_rn(sinv[r + t], v[t]);
      }
      double* p = z + r;
      if (vec2) {
        if (j < m.s) *reinterpret_cast<kron_d2*>(p) = kron_d2{v[0], v[1]};
        if (j + 2 < m.s) *reinterpret_cast<kron_d2*>(p + 2) = kron_d2{v[2], v[3]};
      } else {
#pragma unroll
        for (int t = 0; t < KRON_JT; ++t)
          if (j + t < m.s) p[t] = v[t];
      }
    }
}

// grid and LDS as kron_last_mfma_kernel
template <int SCALE>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
kp_last_mfma_kernel(KronMode m, const double* __restrict__ x, double* __restrict__ z, const double* __restrict__ sinv,
                    const MinresState* __restrict__ st) {
  extern __shared__ double kron_lds[];
  if (st && st->done) return;                                    // uniform: before the barrier
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
  for (int it = 0; it < KRON_IT; ++it) acc[it] = kron_d4{0.0, 0.0, 0.0, 0.0};
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
      if (it < ntile && i < m.n && o < m.no) {
        const int64_t r = o * m.n + i;
        z[r] = SCALE ? mul_rn(sinv[r], acc[it][reg]) : acc[it][reg];
      }
    }
}

// One thread per element: short inner strides and singleton modes.
template <int SCALE>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
kp_plain_kernel(KronMode m, int64_t total, const double* __restrict__ x, double* __restrict__ z,
                const double* __restrict__ sinv, const MinresState* __restrict__ st) {
  if (st && st->done) return;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < total; r += step) {
    const int64_t j = r % m.s, oi = r / m.s;
    const int64_t i = oi % m.n, o = oi / m.n;
    const double* xp = x + o * m.n * m.s + j;
    const double* tp = m.t + i * m.kpad;
    double acc = 0.0;
    for (int k = 0; k < m.n; ++k) acc = fma(tp[k], xp[(int64_t)k * m.s], acc);
    z[r] = SCALE ? mul_rn(sinv[r], acc) : acc;
  }
}

}  // namespace
