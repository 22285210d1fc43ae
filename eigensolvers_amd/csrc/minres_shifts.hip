// Shifted MINRES: sign*(z_j I - H) x_j = b for up to 8 shifts z_j (real or complex) of one real symmetric H and one real
// right-hand side from ONE Lanczos run (FEAST's contour solves of a subspace vector, feast.py:189-200: the Krylov space
// K(H, b) does not depend on the shift).  DESIGN.md section 3.5.
//
// One step = three kernels, no host round trip:
//   KA  w = H v_k - beta_k v_{k-1}                 (the operator's sweep, fused)     + <v_k, w>  = alpha_k
//   KC  w -= alpha_k v_k                                                            + <w, w>    = beta_{k+1}^2
//   KU  per live shift: rotation (complex 2x2, recomputed by every workgroup from the state record),
//       d_k = (v_k - r1 d_{k-1} - r2 d_{k-2}) / nu  over d_{k-2};  x_j += (conj(c_k) tau_j) d_k
// The Lanczos vectors are kept un-normalised (r_k = beta_k v_k, as minres.hip keeps r2): v_k = r_k / beta_k is formed
// where r_k is read - the sweep's epilogue scales the row sum, KU scales its one read of r_k - so the normalisation is
// no pass of its own.  KU reads r_k once and, per live shift, d_{k-1}, d_{k-2}, x (split re / im) and writes d_k, x:
// 8 n + 80 n bytes per live shift; a stopped shift is skipped, its x is never touched again.  KU carries no reduction:
// |tau_j| IS the residual norm of shift j.
//
// The state (Lanczos scalars, the two last rotations and tau of every shift, live flags) lives in two device records:
// KA, KC and KU of a step read one, KU's workgroup 0 writes the other.  Once `done` is set every later kernel of a chunk
// returns at once (KU after copying the final record on), so the result does not depend on how many steps the host enqueues between two looks at the record.
#include <math.h>
#include "sweep_launch.h"
#include "minres_device.h"

#define MS_MAX_SHIFTS 8

struct MsState {
  double beta1, beta, oldb, s;       // ||b||, beta_k, beta_{k-1}, 1 / beta_k
  double target;                     // max(atol, rtol * ||b||)
  double c1r[MS_MAX_SHIFTS], c1i[MS_MAX_SHIFTS], s1[MS_MAX_SHIFTS];   // rotation k-1 (s = t_lo / nu is real)
  double c2r[MS_MAX_SHIFTS], c2i[MS_MAX_SHIFTS], s2[MS_MAX_SHIFTS];   // rotation k-2
  double taur[MS_MAX_SHIFTS], taui[MS_MAX_SHIFTS];
  int its[MS_MAX_SHIFTS];            // steps shift j has taken
  int live[MS_MAX_SHIFTS];
  int itn;                           // completed steps (operator products)
  int done;
  int nshift, maxiter;
};
static_assert(sizeof(MsState) % 4 == 0, "the record is copied word by word");

// Coefficients of one shift's element update at step k.
struct MsUpd {
  double r1r, r1i, r2, inv, gr, gi;  // r1 (complex), r2 (real), 1/nu, g = conj(c_k) tau
  // d = (v - r1 d1 - r2 d2) / nu ; x += g d.  Explicit fused operations with contraction off, as MinresKd::apply, so that
  // the vector loop and the odd tail element round alike.
  __device__ __forceinline__ void apply(double v, double d1r, double d1i, double d2r, double d2i, double& dr, double& di,
                                        double& xr, double& xi) const {
#pragma clang fp contract(off)
    dr = fma(-r2, d2r, fma(r1i, d1i, fma(-r1r, d1r, v))) * inv;
    di = fma(-r2, d2i, fma(-r1i, d1r, -(r1r * d1i))) * inv;
    xr = fma(-gi, di, fma(gr, dr, xr));
    xi = fma(gi, dr, fma(gr, di, xi));
  }
};

// Row epilogue of the Lanczos sweep: w = s * (H r_k) - (beta_k / beta_{k-1}) r_{k-1} and the partial of <v_k, w>.
struct LanczosRowEpilogue {
  double s, c1;
  int use_r1;
  const double* __restrict__ rk;     // r_k, local rows (v_k = s * r_k)
  const double* __restrict__ rkm1;
  double* __restrict__ w;
  __device__ __forceinline__ void row(int64_t r, double sum, double& acc) const {
    const double v = mul_rn(s, rk[r]);
    double wv = mul_rn(s, sum);
    if (use_r1) wv = fma(-c1, rkm1[r], wv);
    w[r] = wv;
    acc = fma(v, wv, acc);
  }
};

// VARIANT 1-4: the operator sweep of that layout; 5: the combine step of a column-split TCOO-W sweep; FIXED: fixed-point
// accumulators (public variant 5); 6: the dense row sweep over D - the instantiations of minres_ka_kernel.
template <int VARIANT, int FIXED = 0>
__global__ void __launch_bounds__(VARIANT == 4 ? TCOOW_THREADS : HIPEIG_BLOCK)
ms_sweep_kernel(CsrView A, TcooView T, DenseView D, const double* __restrict__ xg, const MsState* __restrict__ Sin,
                const double* __restrict__ rk, const double* __restrict__ rkm1, double* __restrict__ w, MinresRed ra) {
  __shared__ double prod[VARIANT == 2 ? SPMV_NNZ_PER_BLOCK : 8];
  __shared__ double red[16];
  extern __shared__ double tcoo_lds[];
  if (Sin->done) return;
  LanczosRowEpilogue epi;
  epi.s = Sin->s;
  epi.use_r1 = Sin->itn >= 1;
  epi.c1 = epi.use_r1 ? Sin->beta / Sin->oldb : 0.0;
  epi.rk = rk; epi.rkm1 = rkm1; epi.w = w;
  double acc = 0.0;
  if (VARIANT == 6) dense_row_sweep(D, xg, epi, acc);
  else if (VARIANT == 5) tcoow_combine_sweep(T.raw_out, T.part_base, T.part_stride, T.nrows, epi, acc);
  else if (VARIANT == 4) tcoo_wg_sweep<LanczosRowEpilogue, FIXED>(T, xg, epi, acc, tcoo_lds, red);
  else if (VARIANT == 3) tcoo_sweep(T, xg, epi, acc, tcoo_lds);
  else if (VARIANT == 2) csr_stream_sweep(A, xg, epi, acc, prod);
  else csr_vector_sweep(A, xg, epi, acc);
  acc = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) store_partial(ra.part + blockIdx.x, acc);
  if (last_block_ticket(ra.counter, ra.tickets, (unsigned)(ra.part - ra.base) + blockIdx.x)) {
    const double vw = sum_partials_agent(ra.base, ra.count, red);
    if (threadIdx.x == 0) *ra.tot = vw;
    release_ticket_counter(ra.counter);
  }
}

// w -= alpha v_k = w - (alpha / beta_k) r_k, and <w, w>.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
ms_kc_kernel(int64_t n, const MsState* __restrict__ Sin, const double* __restrict__ pA, const double* __restrict__ rk,
             double* __restrict__ w, MinresRed rc) {
  __shared__ double red[4];
  if (Sin->done) return;
  const double c = pA[0] / Sin->beta;
  const int64_t n2 = n >> 1;
  const double2* r2 = reinterpret_cast<const double2*>(rk);
  double2* w2 = reinterpret_cast<double2*>(w);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    const double2 rv = r2[i];
    double2 wv = w2[i];
    wv.x = fma(-c, rv.x, wv.x); wv.y = fma(-c, rv.y, wv.y);
    w2[i] = wv;
    acc = fma(wv.x, wv.x, acc); acc = fma(wv.y, wv.y, acc);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double wv = fma(-c, rk[n - 1], w[n - 1]);
    w[n - 1] = wv;
    acc = fma(wv, wv, acc);
  }
  acc = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) store_partial(rc.part + blockIdx.x, acc);
  if (last_block_ticket(rc.counter, rc.tickets, blockIdx.x)) {
    const double ww = sum_partials_agent(rc.base, rc.count, red);
    if (threadIdx.x == 0) *rc.tot = ww;
    release_ticket_counter(rc.counter);
  }
}

struct MsUpdArgs {
  int64_t n, npad;
  double sign;
  double zr[MS_MAX_SHIFTS], zi[MS_MAX_SHIFTS];
  double* xr[MS_MAX_SHIFTS];
  double* xi[MS_MAX_SHIFTS];
  double* d;                         // shift j, ring slot q, half p (re, im): d + ((j * 2 + q) * 2 + p) * npad
  const double* pA;                  // alpha_k
  const double* pC;                  // beta_{k+1}^2
  int slot;                          // ring slot of d_{k-2}, which d_k overwrites; d_{k-1} is the other one
  int probe;                         // timing aid: the record is not advanced
};

// Rotation of shift j at the step the record S is in (alpha, beta_{k+1} just reduced); advances the shift's part of Sn.
__device__ __forceinline__ MsUpd ms_rotate(const MsState& S, MsState& Sn, int j, double sign, double zr, double zi,
                                           double alpha, double betan) {
  const double t_up = (S.itn == 0) ? 0.0 : -sign * S.beta;
  const double tdr = sign * (zr - alpha), tdi = sign * zi;
  const double t_lo = -sign * betan;
  const double c1r = S.c1r[j], c1i = S.c1i[j], s1 = S.s1[j];
  const double tmpr = S.c2r[j] * t_up, tmpi = S.c2i[j] * t_up;
  MsUpd u;
  u.r2 = S.s2[j] * t_up;
  u.r1r = (c1r * tmpr + c1i * tmpi) + s1 * tdr;           // conj(c1) tmp + conj(s1) t_d
  u.r1i = (c1r * tmpi - c1i * tmpr) + s1 * tdi;
  const double ddr = -s1 * tmpr + (c1r * tdr - c1i * tdi);  // -s1 tmp + c1 t_d
  const double ddi = -s1 * tmpi + (c1r * tdi + c1i * tdr);
  const double nu = hypot(hypot(ddr, ddi), t_lo);
  const double cr = ddr / nu, ci = ddi / nu, sn = t_lo / nu;
  u.inv = 1.0 / nu;
  const double tr = S.taur[j], ti = S.taui[j];
  u.gr = cr * tr + ci * ti;                                 // conj(c) tau
  u.gi = cr * ti - ci * tr;
  Sn.c2r[j] = c1r; Sn.c2i[j] = c1i; Sn.s2[j] = s1;
  Sn.c1r[j] = cr; Sn.c1i[j] = ci; Sn.s1[j] = sn;
  Sn.taur[j] = -sn * tr; Sn.taui[j] = -sn * ti;
  Sn.its[j] = S.itn + 1;
  Sn.live[j] = hypot(Sn.taur[j], Sn.taui[j]) > S.target;
  return u;
}

__global__ void __launch_bounds__(HIPEIG_BLOCK)
ms_update_kernel(MsUpdArgs a, const MsState* __restrict__ Sin, MsState* __restrict__ Sout, const double* __restrict__ rk) {
  __shared__ MsState Sn;
  __shared__ MsUpd upd[MS_MAX_SHIFTS];
  if (Sin->done) {
    // hand the final record on: the next step reads the OTHER record, which still holds the state before the stop
    if (blockIdx.x == 0 && !a.probe)
      for (int k = threadIdx.x; k < (int)(sizeof(MsState) / 4); k += blockDim.x)
        reinterpret_cast<uint32_t*>(Sout)[k] = reinterpret_cast<const uint32_t*>(Sin)[k];
    return;
  }
  // thread j advances shift j (uniform over the grid: every workgroup computes the same record)
  for (int k = threadIdx.x; k < (int)(sizeof(MsState) / 4); k += blockDim.x)
    reinterpret_cast<uint32_t*>(&Sn)[k] = reinterpret_cast<const uint32_t*>(Sin)[k];
  __syncthreads();
  const double alpha = a.pA[0];
  const double betan = sqrt(a.pC[0]);
  const double s = Sin->s;
  const int nshift = Sin->nshift;
  if ((int)threadIdx.x < nshift && Sin->live[threadIdx.x])
    upd[threadIdx.x] = ms_rotate(*Sin, Sn, threadIdx.x, a.sign, a.zr[threadIdx.x], a.zi[threadIdx.x], alpha, betan);
  __syncthreads();
  if (blockIdx.x == 0 && !a.probe) {
    if (threadIdx.x == 0) {
      int any = 0;
      for (int j = 0; j < nshift; ++j) any |= Sn.live[j];
      Sn.oldb = Sn.beta; Sn.beta = betan; Sn.s = 1.0 / betan;
      Sn.itn += 1;
      Sn.done = (!any || Sn.itn >= Sn.maxiter || !(betan > 0.0)) ? 1 : 0;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < (int)(sizeof(MsState) / 4); k += blockDim.x)
      reinterpret_cast<uint32_t*>(Sout)[k] = reinterpret_cast<const uint32_t*>(&Sn)[k];
  }
  const int64_t n2 = a.n >> 1;
  const double2* r2 = reinterpret_cast<const double2*>(rk);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
    const double2 rv = r2[i];
    const double vx = mul_rn(s, rv.x), vy = mul_rn(s, rv.y);
    for (int j = 0; j < nshift; ++j) {
      if (!Sin->live[j]) continue;                         // uniform
      const MsUpd u = upd[j];
      double* dj = a.d + (int64_t)j * 4 * a.npad;
      const double2* d1r = reinterpret_cast<const double2*>(dj + (int64_t)((1 - a.slot) * 2) * a.npad);
      const double2* d1i = reinterpret_cast<const double2*>(dj + (int64_t)((1 - a.slot) * 2 + 1) * a.npad);
      double2* d2r = reinterpret_cast<double2*>(dj + (int64_t)(a.slot * 2) * a.npad);
      double2* d2i = reinterpret_cast<double2*>(dj + (int64_t)(a.slot * 2 + 1) * a.npad);
      double2* xr = reinterpret_cast<double2*>(a.xr[j]);
      double2* xi = reinterpret_cast<double2*>(a.xi[j]);
      const double2 p1r = d1r[i], p1i = d1i[i], p2r = d2r[i], p2i = d2i[i];
      double2 qr = xr[i], qi = xi[i], nr, ni;
      u.apply(vx, p1r.x, p1i.x, p2r.x, p2i.x, nr.x, ni.x, qr.x, qi.x);
      u.apply(vy, p1r.y, p1i.y, p2r.y, p2i.y, nr.y, ni.y, qr.y, qi.y);
      d2r[i] = nr; d2i[i] = ni;
      xr[i] = qr; xi[i] = qi;
    }
  }
  if ((a.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t i = a.n - 1;
    const double v = mul_rn(s, rk[i]);
    for (int j = 0; j < nshift; ++j) {
      if (!Sin->live[j]) continue;
      const MsUpd u = upd[j];
      double* dj = a.d + (int64_t)j * 4 * a.npad;
      const double* d1r = dj + (int64_t)((1 - a.slot) * 2) * a.npad;
      const double* d1i = dj + (int64_t)((1 - a.slot) * 2 + 1) * a.npad;
      double* d2r = dj + (int64_t)(a.slot * 2) * a.npad;
      double* d2i = dj + (int64_t)(a.slot * 2 + 1) * a.npad;
      double nr, ni, qr = a.xr[j][i], qi = a.xi[j][i];
      u.apply(v, d1r[i], d1i[i], d2r[i], d2i[i], nr, ni, qr, qi);
      d2r[i] = nr; d2i[i] = ni;
      a.xr[j][i] = qr; a.xi[j][i] = qi;
    }
  }
}

static int env_int(const char* name, int fallback) {
  const char* e = getenv(name);
  return (e && atoi(e) > 0) ? atoi(e) : fallback;
}

extern "C" int hipeig_minres_shifts(hipeig_ctx* c, hipeig_csr* A, double sign, int nshift, const double* zr, const double* zi,
                                    const double* b, double* const* x_re, double* const* x_im, double rtol, double atol,
                                    int maxiter, int* info, double* out_stats) {
  HIPEIG_REQUIRE(info != nullptr && zr != nullptr && zi != nullptr && x_re != nullptr && x_im != nullptr, "null argument");
  HIPEIG_REQUIRE(nshift >= 1 && nshift <= MS_MAX_SHIFTS, "1 to 8 shifts per call");
  HIPEIG_REQUIRE(sign == 1.0 || sign == -1.0, "sign must be +1 or -1");
  HIPEIG_REQUIRE(maxiter >= 1, "maxiter must be positive");
  HIPEIG_REQUIRE(!c->collectives, "shifted MINRES runs on whole vectors (no row partition)");
  HIPEIG_REQUIRE(A->nrows == A->ncols, "the inner solve needs a square operator");
  const int64_t n = A->nrows;
  for (int j = 0; j < nshift; ++j) {
    HIPEIG_REQUIRE(x_re[j] != nullptr && x_im[j] != nullptr && x_re[j] != b && x_im[j] != b, "x must not be null or alias b");
    info[j] = 0;
    HIPEIG_CHECK(hipMemsetAsync(x_re[j], 0, (size_t)n * sizeof(double), c->stream));
    HIPEIG_CHECK(hipMemsetAsync(x_im[j], 0, (size_t)n * sizeof(double), c->stream));
  }
  if (out_stats) memset(out_stats, 0, (size_t)nshift * 4 * sizeof(double));
  double bb = 0.0;
  if (hipeig_dot(c, n, b, b, &bb)) return 1;
  if (bb == 0.0) return hipeig_sync_checked(c) ? 4 : 0;       // b == 0: every x_j = 0

  // workspace: two state records, R[3] (r_{k-1}, r_k, w rotate) and per shift two ring slots of a split complex d
  const int64_t npad = (n + 31) & ~(int64_t)31;
  const int64_t head = 256;                                    // doubles kept for the two records
  static_assert(2 * sizeof(MsState) <= 256 * sizeof(double), "the state records outgrew their area");
  const int64_t need = head + npad * (3 + 4 * MS_MAX_SHIFTS);
  if (c->ms_ws_doubles < need) {
    if (c->ms_ws) HIPEIG_CHECK(hipFree(c->ms_ws));
    c->ms_ws = nullptr; c->ms_ws_doubles = 0;
    HIPEIG_CHECK(hipMalloc((void**)&c->ms_ws, (size_t)need * sizeof(double)));
    c->ms_ws_doubles = need;
  }
  if (!c->h_ms_state) HIPEIG_CHECK(hipHostMalloc((void**)&c->h_ms_state, sizeof(MsState), hipHostMallocDefault));
  MsState* V = reinterpret_cast<MsState*>(c->ms_ws);
  double* R[3] = {c->ms_ws + head, c->ms_ws + head + npad, c->ms_ws + head + 2 * npad};
  double* D = c->ms_ws + head + 3 * npad;
  HIPEIG_CHECK(hipMemsetAsync(R[1], 0, (size_t)npad * (2 + 4 * nshift) * sizeof(double), c->stream));
  HIPEIG_CHECK(hipMemcpyAsync(R[0], b, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));

  MsState* h = reinterpret_cast<MsState*>(c->h_ms_state);
  memset(h, 0, sizeof(MsState));
  h->beta1 = sqrt(bb); h->beta = h->beta1; h->oldb = 0.0; h->s = 1.0 / h->beta1;
  h->target = fmax(atol, rtol * h->beta1);
  h->nshift = nshift; h->maxiter = maxiter;
  for (int j = 0; j < nshift; ++j) {
    h->c1r[j] = 1.0; h->c2r[j] = 1.0; h->taur[j] = h->beta1; h->live[j] = 1;
  }
  HIPEIG_CHECK(hipMemcpyAsync(V, h, sizeof(MsState), hipMemcpyHostToDevice, c->stream));
  if (hipeig_sync_checked(c)) return 4;                        // the pinned record is rewritten by the first chunk's copy-back

  SweepPlan plan;
  if (const int rc = sweep_plan_build(c, A, grid_wide(n, 8), &plan)) return rc;   // combine launch of a column-split sweep: minres.hip's grid
  HIPEIG_REQUIRE(plan.nPA <= HIPEIG_WIDE_PARTIALS, "too many sweeps for the partial-sum buffer");
  if (const int rc = sweep_set_lds_limits(plan, (const void*)ms_sweep_kernel<3>, (const void*)ms_sweep_kernel<4, 0>,
                                          (const void*)ms_sweep_kernel<4, 1>)) return rc;
  const int gE = grid_wide(n, env_int("HIPEIG_MS_PER_THREAD", 8));         // KC: its reduction finishes in the last workgroup
  // KU: no reduction, so no cap on the grid; every workgroup pays the rotations of its prologue once
  const int64_t upt = env_int("HIPEIG_MS_UPDATE_PER_THREAD", 4);
  int64_t gU64 = (n + HIPEIG_BLOCK * upt - 1) / (HIPEIG_BLOCK * upt);
  if (gU64 < 1) gU64 = 1;
  if (gU64 > ((int64_t)1 << 22)) gU64 = (int64_t)1 << 22;
  const int gU = (int)gU64;
  const int nPA = plan.nPA;
  double* pA = c->d_partials;
  double* pC = c->d_partials + HIPEIG_WIDE_PARTIALS;
  double* tot = c->d_scalars + SC_MINRES_TOT;                           // [0] <v,w>, [1] <w,w>
  unsigned* cntA = c->d_counters + 0;
  unsigned* cntC = c->d_counters + HIPEIG_TICKET_WORDS;
  HIPEIG_CHECK(hipMemsetAsync(tot, 0, 8 * sizeof(double), c->stream));
  const MinresRed redC{pC, pC, gE, (unsigned)gE, cntC, tot + 1, nullptr};

  MsUpdArgs ua;
  memset(&ua, 0, sizeof(ua));
  ua.n = n; ua.npad = npad; ua.sign = sign; ua.d = D; ua.pA = tot + 0; ua.pC = tot + 1;
  for (int j = 0; j < nshift; ++j) { ua.zr[j] = zr[j]; ua.zi[j] = zi[j]; ua.xr[j] = x_re[j]; ua.xi[j] = x_im[j]; }
  // measurement aid (tools/shifted_feast_bench.py): 1 / 2 / 3 launch ONLY the sweep / KC / KU of every step, `maxiter` times
  // on a record that does not advance - the time of that phase alone; the solutions are meaningless
  const int probe = env_int("HIPEIG_MS_PROBE", 0);
  ua.probe = probe ? 1 : 0;

  auto enqueue_sweep = [&](const MsState* Sin, double* rk, double* rkm1, double* w) -> int {
    SweepOperand op;
    if (sweep_prepare(c, A, plan, rk, &op)) return 4;         // no communicator: the operand itself
    sweep_launch(c, plan, op, [&](auto v, auto f, int grid, int threads, size_t lds, const TcooView& tv, const double* xg, int off) {
      const MinresRed ra{pA + off, pA, nPA, (unsigned)nPA, cntA, tot + 0, nullptr};
      hipLaunchKernelGGL((ms_sweep_kernel<decltype(v)::value, decltype(f)::value>), dim3(grid), dim3(threads), lds, c->stream, plan.view, tv, plan.dview, xg, Sin, rk, rkm1, w, ra);
    });
    return 0;
  };

  // steps between two looks at the state record; kernels launched past the stopping step return at once
  const int chunk = env_int("HIPEIG_MS_CHUNK", 32);
  int k = 0;
  while (k < maxiter) {
    const int kend = (k + chunk < maxiter) ? k + chunk : maxiter;
    for (; k < kend; ++k) {
      const int kk = probe ? 0 : k;                            // probe: the same buffers and record every time
      const MsState* Sin = V + (kk & 1);
      double* rk = R[kk % 3];
      double* w = R[(kk + 1) % 3];
      double* rkm1 = R[(kk + 2) % 3];
      if (!probe || probe == 1)
        if (enqueue_sweep(Sin, rk, rkm1, w)) return 4;
      if (!probe || probe == 2)
        hipLaunchKernelGGL(ms_kc_kernel, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, Sin, (const double*)(tot + 0), (const double*)rk, w, redC);
      if (!probe || probe == 3) {
        ua.slot = kk & 1;
        hipLaunchKernelGGL(ms_update_kernel, dim3(gU), dim3(HIPEIG_BLOCK), 0, c->stream, ua, Sin, V + ((kk + 1) & 1), (const double*)rk);
      }
    }
    HIPEIG_CHECK(hipGetLastError());
    HIPEIG_CHECK(hipMemcpyAsync(h, V + (probe ? 0 : (kend & 1)), sizeof(MsState), hipMemcpyDeviceToHost, c->stream));
    if (hipeig_sync_checked(c)) return 4;
    if (h->done) break;
  }
  HIPEIG_REQUIRE(probe || h->done, "shifted MINRES left the step loop without a stop");
  for (int j = 0; j < nshift; ++j) {
    info[j] = (probe || h->live[j]) ? maxiter : 0;
    if (out_stats) {
      out_stats[4 * j + 0] = h->its[j];
      out_stats[4 * j + 1] = hypot(h->taur[j], h->taui[j]);
      out_stats[4 * j + 2] = probe ? maxiter : h->itn;
      out_stats[4 * j + 3] = 0.0;
    }
  }
  return 0;
}
