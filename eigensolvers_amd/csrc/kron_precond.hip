// Host side of the separable preconditioner of the Kronecker-sum operator (kernels in kron_precond_device.h; recurrence,
// bound and byte model: DESIGN.md 3.2c).  M^-1 = Q S Q^T with Q = Q_1 (x) ... (x) Q_D from the host decompositions
// T_d + diag(v_d) = Q_d diag(lam_d) Q_d^T and S = diag(sinv), sinv_r = 1 / max(|sigma - Lam_r|, f max |sigma - Lam|),
// Lam_r = sum_d lam_d[i_d].  The record holds the padded device copies of Q_d and Q_d^T (16 rows, 4 columns, as the
// operator's factors) and the lam_d tables; sinv is the caller's vector (one per shift and floor).
//
// An apply is 2 D launches: forward modes 1..D with Q_d^T (the last one stores sinv (.) sum), backward modes 1..D with Q_d.
// It keeps no vector of its own: the launches alternate between the operator's raw-sum buffer, which is free between two
// products, and the output, which is written for good only by the last launch (2 D - 1 is odd).  The input is only read.
#include <vector>
#include "kron_precond_device.h"
#include "minres_device.h"

struct hipeig_kron_precond {
  int D;
  int64_t N;
  KronMode mode[2][KRON_MAX_MODES];      // [0]: t = Q_d (backward), [1]: t = Q_d^T (forward)
  int form[KRON_MAX_MODES];              // 1 inner MFMA, 2 last-mode MFMA, 3 plain FMA: the rule of kron.hip
  double* d_q[2][KRON_MAX_MODES];
  double* d_lam;                         // the lam_d tables, mode after mode
  int32_t lam_off[KRON_MAX_MODES];
  double* scratch;                       // the operator's raw-sum buffer (not owned)
  int64_t bytes;
};

static size_t kp_last_lds(const KronMode& m) { return (size_t)(KRON_SLAB + 16 * KRON_IT) * (m.kpad + 2) * sizeof(double); }
static size_t kp_inner_lds(const KronMode& m) { return (size_t)(16 * KRON_IT) * (m.kpad + 2) * sizeof(double); }

// One mode launch on the compute stream: z = (I (x) Q_d or Q_d^T (x) I) x, scaled by sinv where it is given.
template <int SCALE>
static void kp_launch_mode(hipeig_ctx* c, const hipeig_kron_precond* P, int d, int transpose, const double* x, double* z,
                           const double* sinv, const MinresState* st) {
  const KronMode& m = P->mode[transpose ? 1 : 0][d];
  const int groups = (m.npad + 16 * KRON_IT - 1) / (16 * KRON_IT);
  if (P->form[d] == 1) {
    const int64_t items = m.no * ((m.s + 63) >> 6);
    const int vec2 = (m.s % 2 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)z % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL(kp_inner_mfma_kernel<SCALE>, dim3((unsigned)((items + 3) / 4), groups), dim3(HIPEIG_BLOCK), kp_inner_lds(m),
                       c->stream, m, x, z, sinv, st, vec2);
  } else if (P->form[d] == 2) {
    hipLaunchKernelGGL(kp_last_mfma_kernel<SCALE>, dim3((unsigned)((m.no + KRON_SLAB - 1) / KRON_SLAB), groups), dim3(HIPEIG_BLOCK),
                       kp_last_lds(m), c->stream, m, x, z, sinv, st);
  } else {
    hipLaunchKernelGGL(kp_plain_kernel<SCALE>, dim3(grid_stream(2 * P->N)), dim3(HIPEIG_BLOCK), 0, c->stream, m, P->N, x, z, sinv, st);
  }
}

// z = Q (sinv (.) (Q^T x)): 2 D launches through the operator's raw-sum buffer and z (see the header of this file).
int hipeig_kp_apply(hipeig_ctx* c, const hipeig_kron_precond* P, const double* sinv, const double* x, double* z,
                    const MinresState* st) {
  HIPEIG_REQUIRE(x != z && x != P->scratch && z != P->scratch, "the apply is out of place and works in the operator's raw-sum buffer");
  const int L = 2 * P->D;
  const double* src = x;
  for (int l = 0; l < L; ++l) {
    double* dst = (l & 1) ? z : P->scratch;
    if (l < P->D - 1) kp_launch_mode<0>(c, P, l, 1, src, dst, nullptr, st);
    else if (l == P->D - 1) kp_launch_mode<1>(c, P, l, 1, src, dst, sinv, st);
    else kp_launch_mode<0>(c, P, l - P->D, 0, src, dst, nullptr, st);
    src = dst;
  }
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// <y, z>, finished in the last workgroup (common.h); the reduction of pmr_start_kernel on its own.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
kp_dot_kernel(int64_t n, const double* __restrict__ y, const double* __restrict__ z, MinresRed rc,
              const MinresState* __restrict__ st) {
  __shared__ double red[4];
  if (st && st->done) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) acc = fma(y[i], z[i], acc);
  acc = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) store_partial(rc.part + blockIdx.x, acc);
  if (last_block_ticket(rc.counter, rc.tickets, blockIdx.x)) {
    const double yz = sum_partials_agent(rc.base, rc.count, red);
    if (threadIdx.x == 0) *rc.tot = yz;
    release_ticket_counter(rc.counter);
  }
}

// KC's tail in a separable solve (minres.hip): z = M^-1 y and <y, z> into the slot of <y, y>.
int hipeig_kp_apply_dot(hipeig_ctx* c, const hipeig_kron_precond* P, const double* sinv, const double* y, double* z, int grid,
                        const MinresRed& rc, const MinresState* st) {
  if (const int e = hipeig_kp_apply(c, P, sinv, y, z, st)) return e;
  hipLaunchKernelGGL(kp_dot_kernel, dim3(grid), dim3(HIPEIG_BLOCK), 0, c->stream, P->N, y, (const double*)z, rc, st);
  return 0;
}

// Start of a separable solve: r2_0 = b, z_0 = M^-1 b and beta1^2 = <b, z_0> on the host (refuses < 0, as hipeig_pmr_start).
int hipeig_kp_start(hipeig_ctx* c, const hipeig_kron_precond* P, const double* sinv, const double* b, double* r2, double* z,
                    int grid, const MinresRed& rc, double* bz_out) {
  HIPEIG_CHECK(hipMemcpyAsync(r2, b, (size_t)P->N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  if (const int e = hipeig_kp_apply_dot(c, P, sinv, r2, z, grid, rc, nullptr)) return e;
  HIPEIG_CHECK(hipGetLastError());
  HIPEIG_CHECK(hipMemcpyAsync(c->h_scalars, rc.tot, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (hipeig_sync_checked(c)) return 4;
  const double bz = c->h_scalars[0];
  HIPEIG_REQUIRE(bz >= 0.0, "indefinite preconditioner: <b, M^-1 b> < 0 (or not a number)");
  *bz_out = bz;
  return 0;
}

int64_t hipeig_kp_n(const hipeig_kron_precond* P) { return P->N; }

extern "C" int hipeig_kron_precond_destroy(hipeig_ctx* c, hipeig_kron_precond* P) {
  if (!P) return 0;
  if (c) hipStreamSynchronize(c->stream);
  for (int t = 0; t < 2; ++t)
    for (int d = 0; d < KRON_MAX_MODES; ++d)
      if (P->d_q[t][d]) hipFree(P->d_q[t][d]);
  if (P->d_lam) hipFree(P->d_lam);
  free(P);
  return 0;
}

extern "C" int hipeig_kron_precond_create(hipeig_ctx* c, hipeig_csr* A, int D, const int64_t* dims, const double* const* bases,
                                          const double* const* eigenvalues, hipeig_kron_precond** out) {
  HIPEIG_REQUIRE(c && A && dims && bases && eigenvalues && out, "null argument");
  HIPEIG_REQUIRE(hipeig_kron_raw(A) != nullptr, "the separable preconditioner belongs to a Kronecker-sum operator");
  HIPEIG_REQUIRE(!c->collectives, "the separable preconditioner runs on one GPU");
  HIPEIG_REQUIRE(D >= 1 && D <= KRON_MAX_MODES, "1 to 8 modes");
  int64_t N = 1;
  for (int d = 0; d < D; ++d) {
    HIPEIG_REQUIRE(bases[d] && eigenvalues[d], "null table");
    HIPEIG_REQUIRE(dims[d] >= 1 && dims[d] <= KRON_MAX_N, "a mode the Kronecker kernels do not take");
    N *= dims[d];
    HIPEIG_REQUIRE(N < ((int64_t)1 << 31), "the product of the dims must stay below 2^31");
  }
  HIPEIG_REQUIRE(N == A->nrows, "the dims are not the operator's");
  hipeig_kron_precond* P = (hipeig_kron_precond*)calloc(1, sizeof(hipeig_kron_precond));
  if (!P) { hipeig_set_error("out of host memory"); return 1; }
  auto build = [&]() -> int {
    P->D = D; P->N = N; P->scratch = hipeig_kron_raw(A);
    std::vector<double> lam;
    std::vector<std::vector<double>> padded((size_t)2 * D);     // outlive the asynchronous uploads
    int64_t o = 1, bytes = 0;
    for (int d = 0; d < D; ++d) {
      const int n = (int)dims[d];
      const int npad = (n + 15) / 16 * 16, kpad = (n + 3) / 4 * 4;
      const int64_t s = N / (o * n);
      P->form[d] = (n == 1) ? 3 : (s == 1) ? 2 : (s >= 16) ? 1 : 3;
      for (int t = 0; t < 2; ++t) {
        std::vector<double>& p = padded[(size_t)2 * d + t];
        p.assign((size_t)npad * kpad, 0.0);
        for (int i = 0; i < n; ++i)
          for (int q = 0; q < n; ++q) p[(size_t)i * kpad + q] = t ? bases[d][(size_t)q * n + i] : bases[d][(size_t)i * n + q];
        HIPEIG_CHECK(hipMalloc((void**)&P->d_q[t][d], p.size() * sizeof(double)));
        HIPEIG_CHECK(hipMemcpyAsync(P->d_q[t][d], p.data(), p.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        KronMode& m = P->mode[t][d];
        m.t = P->d_q[t][d]; m.n = n; m.npad = npad; m.kpad = kpad; m.no = o; m.s = s;
        bytes += (int64_t)p.size() * 8;
      }
      o *= n;
      P->lam_off[d] = (int32_t)lam.size();
      for (int i = 0; i < n; ++i) lam.push_back(eigenvalues[d][i]);
    }
    HIPEIG_CHECK(hipMalloc((void**)&P->d_lam, lam.size() * sizeof(double)));
    HIPEIG_CHECK(hipMemcpyAsync(P->d_lam, lam.data(), lam.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    bytes += (int64_t)lam.size() * 8;
    HIPEIG_CHECK(hipFuncSetAttribute((const void*)kp_last_mfma_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPEIG_CHECK(hipFuncSetAttribute((const void*)kp_last_mfma_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPEIG_CHECK(hipStreamSynchronize(c->stream));
    P->bytes = bytes;
    return 0;
  };
  if (const int rc = build()) {
    hipeig_kron_precond_destroy(c, P);
    return rc;
  }
  *out = P;
  return 0;
}

// out[0] = modes, [1] = N, [2] = launches per apply (2 D), [3] = device bytes of the record (the tables; an apply works in
// the operator's raw-sum buffer and its output), [4] = launches a preconditioned iteration adds to the plain one
// (2 D + 1); per mode d (0-based) out[8 + 4 d] = kernel form (as hipeig_kron_info), [9 + 4 d] = n_d, [10 + 4 d] /
// [11 + 4 d] = padded rows / columns.
extern "C" int hipeig_kron_precond_info(hipeig_kron_precond* P, int64_t out[40]) {
  HIPEIG_REQUIRE(P && out, "null argument");
  memset(out, 0, 40 * sizeof(int64_t));
  out[0] = P->D; out[1] = P->N; out[2] = 2 * P->D; out[3] = P->bytes; out[4] = 2 * P->D + 1;
  for (int d = 0; d < P->D; ++d) {
    const KronMode& m = P->mode[0][d];
    out[8 + 4 * d] = P->form[d]; out[9 + 4 * d] = m.n; out[10 + 4 * d] = m.npad; out[11 + 4 * d] = m.kpad;
  }
  return 0;
}

// sinv[r] = 1 / max(|sigma - Lam_r|, floor_rel max |sigma - Lam|): kron_diagonal_kernel on the lam_d tables without V (Lam
// summed in mode order, into the operator's raw-sum buffer), then hipeig_jacobi_inverse with its refusals.
extern "C" int hipeig_kron_precond_scale(hipeig_ctx* c, hipeig_kron_precond* P, double sigma, double floor_rel, double* sinv) {
  HIPEIG_REQUIRE(c && P && sinv, "null argument");
  HIPEIG_REQUIRE(sinv != P->scratch, "sinv must not be the operator's raw-sum buffer");
  KronDiagArgs a;
  memset(&a, 0, sizeof(a));
  a.D = P->D;
  for (int e = 0; e < P->D; ++e) { a.n[e] = P->mode[0][e].n; a.off[e] = P->lam_off[e]; }
  a.td = P->d_lam; a.v = nullptr;
  hipLaunchKernelGGL(kron_diagonal_kernel, dim3(grid_stream(2 * P->N)), dim3(HIPEIG_BLOCK), 0, c->stream, a, P->N, P->scratch);
  HIPEIG_CHECK(hipGetLastError());
  return hipeig_jacobi_inverse(c, P->N, P->scratch, sigma, floor_rel, sinv);
}

extern "C" int hipeig_kron_precond_transform(hipeig_ctx* c, hipeig_kron_precond* P, int d, int transpose, const double* x,
                                             double* z) {
  HIPEIG_REQUIRE(c && P && x && z, "null argument");
  HIPEIG_REQUIRE(d >= 0 && d < P->D, "no such mode");
  HIPEIG_REQUIRE(x != z, "the transform is out of place");
  kp_launch_mode<0>(c, P, d, transpose ? 1 : 0, x, z, nullptr, nullptr);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

extern "C" int hipeig_kron_precond_apply(hipeig_ctx* c, hipeig_kron_precond* P, const double* sinv, const double* x, double* z) {
  HIPEIG_REQUIRE(c && P && sinv && x && z, "null argument");
  return hipeig_kp_apply(c, P, sinv, x, z, nullptr);
}
