// Dense row sweeps for gfx950: the operator's local rows as one row-major fp64 copy (dense.hip builds it from the CSR
// arrays on first use).  A dense row has no column indices and no gathers: a wave reads 1 KiB of consecutive matrix bytes
// per instruction (16 B per lane, non-temporal: the matrix is read once and must not push the operand out of L2) and
// takes the operand with plain loads, shared by the rows of its group.  No LDS accumulators, no atomics.
//
//  * dense_row_sweep       - one operand; the contract of csr_vector_sweep: epi.row(r, sum, acc) once per row, from one lane.
//  * dense_block_sweep<K>  - an interleaved block [row][K] of operands; the contract of csr_rowowner_block_sweep:
//    epi.elem(r, j, sum, acc) once per (row, operand), from a lane with lane % K == j.
//
// Order of the adds of one row (and operand): lane l adds the terms of columns 128 q + 2 l, 128 q + 2 l + 1, q = 0, 1, ...,
// as one fma chain in ascending order; the 64 lane sums are then folded by a fixed shuffle tree.  It depends on the
// number of columns only - not on the grid, not on which wave gets the row: bitwise reproducible.  Worst case per row
// (2 ceil(ncols / 128) chained roundings per lane + 6 tree levels): (2 ceil(ncols / 128) + 6) * 2^-53 * sum_j |a_ij x_j|.
//
// Workgroups are persistent (grid <= HIPEIG_MAX_PARTIALS, dense.hip: hipeig_dense_grid) and walk the row groups
// blockIdx.x, blockIdx.x + gridDim.x, ..., so a fused reduction leaves at most 2048 partials.
#pragma once
#include "common.h"

#define DENSE_ROWS_PER_WAVE 4            // single operand: rows a wave carries through one pass over the columns
#define DENSE_LD_ALIGN 16                // doubles: every row starts on a 128-byte line
#define DENSE_BLOCK_ACC 32               // block form: accumulators per lane (rows per wave x K)

struct DenseView {
  const double* __restrict__ a;          // nrows x ld, row-major; columns [ncols, ld) are zero
  int64_t nrows, ncols, ld;
};

typedef double dense_f64x2 __attribute__((ext_vector_type(2)));

// rows a wave owns in the block form: 8 / 4 / 2 for K = 4 / 8 / 16
template <int K> struct DenseBlockShape {
  static_assert(K == 4 || K == 8 || K == 16, "interleave width is 4, 8 or 16");
  static constexpr int ROWS = DENSE_BLOCK_ACC / K;
};

template <class Epi>
__device__ __forceinline__ void dense_row_sweep(const DenseView& D, const double* __restrict__ x, const Epi& epi, double& acc) {
  constexpr int R = DENSE_ROWS_PER_WAVE, WPB = HIPEIG_BLOCK / HIPEIG_WAVE;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t ngroups = (D.nrows + R * WPB - 1) / (R * WPB);
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t r0 = (g * WPB + wid) * R;
    if (r0 >= D.nrows) continue;                                 // uniform for the wave; the sweep has no barrier
    const double* row[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {                                // rows past the end re-read the last one, never stored
      const int64_t r = r0 + i < D.nrows ? r0 + i : D.nrows - 1;
      row[i] = D.a + r * D.ld;
    }
    double s[R];
#pragma unroll
    for (int i = 0; i < R; ++i) s[i] = 0.0;
#pragma unroll 2
    for (int64_t c = 2 * lane; c < D.ld; c += 2 * HIPEIG_WAVE) {  // ld is even: c + 1 < ld
      dense_f64x2 av[R];
#pragma unroll
      for (int i = 0; i < R; ++i) av[i] = __builtin_nontemporal_load(reinterpret_cast<const dense_f64x2*>(row[i] + c));
      const double x0 = c < D.ncols ? x[c] : 0.0;                // the operand is ncols long and need not be 16-byte aligned
      const double x1 = c + 1 < D.ncols ? x[c + 1] : 0.0;
#pragma unroll
      for (int i = 0; i < R; ++i) s[i] = fma(av[i].y, x1, fma(av[i].x, x0, s[i]));
    }
#pragma unroll
    for (int i = 0; i < R; ++i) s[i] = wave_reduce_sum(s[i]);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < R; ++i)
        if (r0 + i < D.nrows) epi.row(r0 + i, s[i], acc);
    }
  }
}

// Sum over the 64 lanes, the same bits in every lane (a + b and b + a round alike).
__device__ __forceinline__ double dense_wave_allsum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Register form: a wave keeps ROWS x K accumulators per lane and reads, per step of 128 columns, 16 B of every row and
// the 2 K operand values of its two columns (16-byte loads: the blocks are 16-byte aligned like every interleaved block).
template <int K, class Epi>
__device__ __forceinline__ void dense_block_sweep(const DenseView& D, const double* __restrict__ X, const Epi& epi, double& acc) {
  constexpr int R = DenseBlockShape<K>::ROWS, WPB = HIPEIG_BLOCK / HIPEIG_WAVE;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t ngroups = (D.nrows + R * WPB - 1) / (R * WPB);
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t r0 = (g * WPB + wid) * R;
    if (r0 >= D.nrows) continue;
    const double* row[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + i < D.nrows ? r0 + i : D.nrows - 1;
      row[i] = D.a + r * D.ld;
    }
    double s[R][K];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < K; ++j) s[i][j] = 0.0;
    for (int64_t c = 2 * lane; c < D.ld; c += 2 * HIPEIG_WAVE) {
      dense_f64x2 av[R];
#pragma unroll
      for (int i = 0; i < R; ++i) av[i] = __builtin_nontemporal_load(reinterpret_cast<const dense_f64x2*>(row[i] + c));
      // operand rows c and c + 1: 2 K consecutive doubles; past ncols the matrix holds zeros but the block ends, so clamp
      // the row read and zero the value
      const bool ok0 = c < D.ncols, ok1 = c + 1 < D.ncols;
      const dense_f64x2* x0p = reinterpret_cast<const dense_f64x2*>(X + (ok0 ? c : 0) * K);
      const dense_f64x2* x1p = reinterpret_cast<const dense_f64x2*>(X + (ok1 ? c + 1 : 0) * K);
      double x0[K], x1[K];
#pragma unroll
      for (int j = 0; j < K / 2; ++j) {
        const dense_f64x2 u = x0p[j], w = x1p[j];
        x0[2 * j] = ok0 ? u.x : 0.0; x0[2 * j + 1] = ok0 ? u.y : 0.0;
        x1[2 * j] = ok1 ? w.x : 0.0; x1[2 * j + 1] = ok1 ? w.y : 0.0;
      }
#pragma unroll
      for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) s[i][j] = fma(av[i].y, x1[j], fma(av[i].x, x0[j], s[i][j]));
    }
    // every lane obtains every sum; lane j < K keeps operand j's and runs the epilogue of its column
#pragma unroll
    for (int i = 0; i < R; ++i) {
      double mine = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double t = dense_wave_allsum(s[i][j]);
        mine = (lane == j) ? t : mine;
      }
      if (lane < K && r0 + i < D.nrows) epi.elem(r0 + i, lane, mine, acc);
    }
  }
}
