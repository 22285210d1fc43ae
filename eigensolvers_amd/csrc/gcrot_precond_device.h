// The element of GCROT's diagonal right preconditioner: y = m * x for one entry of M^-1 = diag(m) and one entry of the
// operand, real or complex.  One definition for the stand-alone kernels (gcrot_precond.hip) and for the
// scaled operand packs of the block products (spmm.hip), so that all of them evaluate the same expression: a product that
// scales while it packs then sees, bit for bit, the operand hipeig_diag_mul / hipeig_pair_diag_mul would have written.
#pragma once
#include "common.h"

struct DiagMul {
  // real m, real x: one rounding
  static __device__ __forceinline__ double real(double m, double x) { return mul_rn(m, x); }
  // complex x = xr + i xi times m = mr + i mi; `has_mi` false: m is real (mi is not read) and each half takes one rounding.
  // Spelled out with explicit fused operations (and contraction off), as MinresKd::apply is, so that every instantiation
  // rounds identically: yr = fma(-mi, xi, rn(mr xr)), yi = fma(mi, xr, rn(mr xi)).
  static __device__ __forceinline__ void pair(double mr, double mi, bool has_mi, double xr, double xi, double& yr, double& yi) {
#pragma clang fp contract(off)
    const double pr = mr * xr, pi = mr * xi;
    yr = has_mi ? fma(-mi, xi, pr) : pr;
    yi = has_mi ? fma(mi, xr, pi) : pi;
  }
};
