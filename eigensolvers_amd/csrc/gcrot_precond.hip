// The diagonal right preconditioner of the GCROT(m,k) solves (opt-in: linearSystemArgs["gcrotPreconditioner"]): the solver
// is handed the composed operator v -> sign (z I - H) (minv (.) v) and its result u is turned into x = minv (.) u, which is
// what scipy.sparse.linalg.gcrotmk(A, b, M=diags(minv)) computes.  Here: minv for a real shift or a complex
// contour point z, and the scalings y = minv (.) x.  The block products that scale while they pack are in spmm.hip.
#include <math.h>
#include "gcrot_precond_device.h"
#include "minres_device.h"

// The fixed operations of minv (mirrored by precond_gcrotmk.jacobi_inverse_z_host): m = (rn(zr - d_i), zi),
// real z:    t = |mr|
// complex z: s = rn(rn(mr mr) + rn(zi zi)), t = sqrt(s)
// t >= g:     real 1 / mr                      complex (mr / s, -zi / s)
// 0 < t < g:  real copysign(1 / g, mr)         complex ((mr / t) / g, (-zi / t) / g)
// t == 0:     1 / g
template <int CPLX>
struct JacobiZ {
  double zr, zi;
  __device__ __forceinline__ double m_re(double d) const { return zr - d; }
  __device__ __forceinline__ double norm2(double mr) const {
#pragma clang fp contract(off)
    return mr * mr + zi * zi;
  }
  __device__ __forceinline__ double modulus(double mr) const { return CPLX ? __dsqrt_rn(norm2(mr)) : fabs(mr); }
  __device__ __forceinline__ void inverse(double mr, double g, double& re, double& im) const {
    const double t = modulus(mr);
    if (t >= g) {
      if (CPLX) { const double s = norm2(mr); re = mr / s; im = -zi / s; }
      else { re = 1.0 / mr; im = 0.0; }
    } else if (t > 0.0) {
      if (CPLX) { re = (mr / t) / g; im = (-zi / t) / g; }
      else { re = copysign(1.0 / g, mr); im = 0.0; }
    } else {
      re = 1.0 / g; im = 0.0;
    }
  }
};

// max_i and min_i of t_i, finished in the last workgroup (common.h), as jacobi_range_kernel of minres_precond.hip does it.
// A NaN counts as +inf in the maximum, which is how the host sees it (fmax would drop it).
template <int CPLX>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
jacobi_z_range_kernel(int64_t n, const double* __restrict__ d, JacobiZ<CPLX> jz, double* __restrict__ part, unsigned* counter,
                      double* __restrict__ out) {
  __shared__ double lds[8];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double mx = 0.0, mn = INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double t = jz.modulus(jz.m_re(d[i]));
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

template <int CPLX>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
jacobi_z_inverse_kernel(int64_t n, const double* __restrict__ d, JacobiZ<CPLX> jz, double g, double* __restrict__ minv_re,
                        double* __restrict__ minv_im) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double re, im;
    jz.inverse(jz.m_re(d[i]), g, re, im);
    minv_re[i] = re;
    if (minv_im) minv_im[i] = im;
  }
}

extern "C" int hipeig_jacobi_inverse_z(hipeig_ctx* c, int64_t n, const double* d, double zr, double zi, double floor_rel,
                                       double* minv_re, double* minv_im) {
  HIPEIG_REQUIRE(d != nullptr && minv_re != nullptr, "null vector");
  HIPEIG_REQUIRE(minv_im != nullptr || zi == 0.0, "a complex z needs the imaginary half of the output");
  HIPEIG_REQUIRE(zr == zr && zi == zi && fabs(zr) < INFINITY && fabs(zi) < INFINITY, "z must be finite");
  HIPEIG_REQUIRE(floor_rel >= 0.0 && floor_rel < INFINITY, "the relative floor must be finite and >= 0");
  if (n <= 0) return 0;
  const int cplx = zi != 0.0;
  const int gr = grid_for(n, 8);
  double* tot = c->d_scalars + SC_MINRES_TOT;
  if (cplx)
    hipLaunchKernelGGL(jacobi_z_range_kernel<1>, dim3(gr), dim3(HIPEIG_BLOCK), 0, c->stream, n, d, JacobiZ<1>{zr, zi},
                       c->d_partials, c->d_counters, tot);
  else
    hipLaunchKernelGGL(jacobi_z_range_kernel<0>, dim3(gr), dim3(HIPEIG_BLOCK), 0, c->stream, n, d, JacobiZ<0>{zr, zi},
                       c->d_partials, c->d_counters, tot);
  HIPEIG_CHECK(hipGetLastError());
  HIPEIG_CHECK(hipMemcpyAsync(c->h_scalars, tot, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (hipeig_sync_checked(c)) return 4;
  const double tmax = c->h_scalars[0], tmin = c->h_scalars[1];
  const double g = floor_rel * tmax;
  const double mmin = fmax(tmin, g);                    // the smallest modulus 1 / |minv_i| that will be inverted
  if (!(tmax < INFINITY) || !(g < INFINITY) || !(mmin > 0.0) || !(1.0 / mmin < INFINITY)) {
    hipeig_set_error("Jacobi preconditioner is not finite: max |z - d_i| = %g, min = %g, relative floor %g (a diagonal "
                     "entry equal to z needs a floor > 0)", tmax, tmin, floor_rel);
    return 3;
  }
  if (cplx)
    hipLaunchKernelGGL(jacobi_z_inverse_kernel<1>, dim3(grid_stream(n)), dim3(HIPEIG_BLOCK), 0, c->stream, n, d,
                       JacobiZ<1>{zr, zi}, g, minv_re, minv_im);
  else
    hipLaunchKernelGGL(jacobi_z_inverse_kernel<0>, dim3(grid_stream(n)), dim3(HIPEIG_BLOCK), 0, c->stream, n, d,
                       JacobiZ<0>{zr, zi}, g, minv_re, minv_im);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// ---- y = m (.) x ----------------------------------------------------------------------------------------------------------
// Two elements (16 bytes) per lane and stream, the odd last element by one thread.  An element is read before it is written
// and no thread reads another thread's, so y may be x.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
diag_mul_kernel(int64_t n, const double* __restrict__ m, const double* x, double* y) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double2* m2 = reinterpret_cast<const double2*>(m);
  const double2* x2 = reinterpret_cast<const double2*>(x);
  double2* y2 = reinterpret_cast<double2*>(y);
  for (int64_t t = first; t < n / 2; t += stride) {
    const double2 mv = m2[t], xv = x2[t];
    double2 o;
    o.x = DiagMul::real(mv.x, xv.x);
    o.y = DiagMul::real(mv.y, xv.y);
    y2[t] = o;
  }
  if ((n & 1) && first == 0) y[n - 1] = DiagMul::real(m[n - 1], x[n - 1]);
}

template <int HAS_MI>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
pair_diag_mul_kernel(int64_t n, const double* __restrict__ mr, const double* __restrict__ mi, const double* xr, const double* xi,
                     double* yr, double* yi) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double2* mr2 = reinterpret_cast<const double2*>(mr);
  const double2* mi2 = reinterpret_cast<const double2*>(mi);
  const double2* xr2 = reinterpret_cast<const double2*>(xr);
  const double2* xi2 = reinterpret_cast<const double2*>(xi);
  double2* yr2 = reinterpret_cast<double2*>(yr);
  double2* yi2 = reinterpret_cast<double2*>(yi);
  for (int64_t t = first; t < n / 2; t += stride) {
    const double2 a = mr2[t], b = HAS_MI ? mi2[t] : double2{0.0, 0.0}, vr = xr2[t], vi = xi2[t];
    double2 orr, oi;
    DiagMul::pair(a.x, b.x, HAS_MI, vr.x, vi.x, orr.x, oi.x);
    DiagMul::pair(a.y, b.y, HAS_MI, vr.y, vi.y, orr.y, oi.y);
    yr2[t] = orr; yi2[t] = oi;
  }
  if ((n & 1) && first == 0) {
    double orr, oi;
    DiagMul::pair(mr[n - 1], HAS_MI ? mi[n - 1] : 0.0, HAS_MI, xr[n - 1], xi[n - 1], orr, oi);
    yr[n - 1] = orr; yi[n - 1] = oi;
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int hipeig_diag_mul(hipeig_ctx* c, int64_t n, const double* m, const double* x, double* y) {
  HIPEIG_REQUIRE(m != nullptr && x != nullptr && y != nullptr, "null vector");
  HIPEIG_REQUIRE(aligned16(m) && aligned16(x) && aligned16(y), "vectors must be 16-byte aligned");
  if (n <= 0) return 0;
  hipLaunchKernelGGL(diag_mul_kernel, dim3(grid_stream(n)), dim3(HIPEIG_BLOCK), 0, c->stream, n, m, x, y);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

extern "C" int hipeig_pair_diag_mul(hipeig_ctx* c, int64_t n, const double* mr, const double* mi, const double* xr,
                                    const double* xi, double* yr, double* yi) {
  HIPEIG_REQUIRE(mr != nullptr && xr != nullptr && xi != nullptr && yr != nullptr && yi != nullptr, "null vector");
  HIPEIG_REQUIRE(yr != yi && yr != xi && yi != xr, "the halves of the result may alias the same halves of the operand only");
  HIPEIG_REQUIRE(aligned16(mr) && aligned16(mi) && aligned16(xr) && aligned16(xi) && aligned16(yr) && aligned16(yi),
                 "vectors must be 16-byte aligned");
  if (n <= 0) return 0;
  const int g = grid_stream(n);
  if (mi)
    hipLaunchKernelGGL(pair_diag_mul_kernel<1>, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, mr, mi, xr, xi, yr, yi);
  else
    hipLaunchKernelGGL(pair_diag_mul_kernel<0>, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, n, mr, mi, xr, xi, yr, yi);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}
