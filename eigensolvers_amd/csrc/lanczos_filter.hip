// FEAST's filtered vectors from two Lanczos passes, k <= 8 right-hand sides in lock step on interleaved block products
// (feast.py:189-200 only ever forms q = sum_k Re(c_k x_k) of the contour solves sign*(z_k I - H) x_k = b; every MINRES
// iterate x_k lies in the Krylov space of the same real Lanczos basis, so q = sum_i g_i v_i with real g_i that follow
// from the Lanczos tridiagonal alone).  DESIGN.md section 3.6; the NumPy statement is eigensolvers_amd/lanczos_filter.py.
//
// Pass 1 (hipeig_lanczos_block_scalars), three kernels per step, no host round trip, no per-shift vector:
//   sweep  W = s (H R_k) - (beta_k / beta_{k-1}) R_{k-1}     (block product, fused)  + per-column partials <v_k, w>
//   KC     W -= (alpha / beta_k) R_k                                                 + per-column partials <w, w>
//   scalar one workgroup, thread = (column, shift): the rotation recurrence of minres_shifts.hip for up to 32 shifts per
//          column, live flags, the column's stop, and alpha_k, beta_{k+1} appended to the column's device arrays
// The Lanczos vectors are kept un-normalised (r_k = beta_k v_k) as in minres_shifts.hip; the per-column sums follow
// minres_block.hip: every workgroup leaves K partials, the consumer's prologue adds them in a fixed order.  A column that
// has stopped is masked: its scalars are no longer recorded and its vectors are zeroed (s = 0), never read.
//
// Pass 2 (hipeig_lanczos_combine), one kernel per step, no reduction: the block sweep's element epilogue does
//   q[c] += G[r][i][c] v_i ;  r_{i+1} = (H r_i)/beta_i - (beta_i/beta_{i-1}) r_{i-1} - (alpha_i/beta_i) r_i   written over r_{i-1}
// (v_{i+1} = (H v_i - alpha_i v_i - beta_i v_{i-1}) / beta_{i+1} on pass 1's un-normalised vectors, v_i = r_i / beta_i)
// from the scalar tables uploaded once; column r stops after its own m_r terms; the last term needs no product.
//
// Keep mode (basis_mode 1): pass 1 leaves every r_k in a slot of a basis in device memory instead of a ring of three, and
// pass 2 is one stream over the slots - see "kept basis" below.  Prefix mode (basis_mode 2): a basis that outgrows its
// byte budget keeps the first p vectors, and pass 2 is the stream for the terms i < p - 1 plus the recurrence from step
// p - 1.  The three are one host path with a plan - see "pass 2, host side".  basis_mode 3 / 4: modes 1 / 2 with the basis
// stored in fp32 - the recurrence stays in the fp64 ring and KC leaves a rounded copy of every vector in its slot - see
// "fp32 basis" below.
#include <limits.h>
#include <math.h>
#include "block_sweep_launch.h"

#define LF_MAX_SHIFTS 32
#define LF_HEAD_DOUBLES 4096                                  // doubles kept for the state record

struct LfCol {
  double beta1, beta, oldb, s, target;                       // ||b||, beta_k, beta_{k-1}, 1 / beta_k, max(atol, rtol ||b||)
  int itn, done;                                              // completed steps; the column has stopped
};

struct LfState {
  int done, nshift, maxiter, pad;                             // done: every column has stopped
  LfCol col[BCOO_KMAX];
  double c1r[BCOO_KMAX][LF_MAX_SHIFTS], c1i[BCOO_KMAX][LF_MAX_SHIFTS], s1[BCOO_KMAX][LF_MAX_SHIFTS];   // rotation k-1
  double c2r[BCOO_KMAX][LF_MAX_SHIFTS], c2i[BCOO_KMAX][LF_MAX_SHIFTS];                                 // rotation k-2 (its s is not needed here)
  double taur[BCOO_KMAX][LF_MAX_SHIFTS], taui[BCOO_KMAX][LF_MAX_SHIFTS];
  int its[BCOO_KMAX][LF_MAX_SHIFTS];
  int live[BCOO_KMAX][LF_MAX_SHIFTS];
};
static_assert(sizeof(LfState) <= LF_HEAD_DOUBLES * sizeof(double), "the state record outgrew its area");

struct LfShifts {
  double sign;
  double zr[LF_MAX_SHIFTS], zi[LF_MAX_SHIFTS];
};

// Block counterpart of LanczosRowEpilogue (minres_shifts.hip): s, c1, use_r1 are those of THIS thread's column.
template <int K>
struct LfScalarsEpilogue {
  double s, c1;
  int use_r1;
  const double* __restrict__ rk;
  const double* __restrict__ rkm1;
  double* __restrict__ w;
  __device__ __forceinline__ void elem(int64_t r, int j, double sum, double& acc) const {
    const int64_t i = r * K + j;
    const double v = mul_rn(s, rk[i]);
    double wv = mul_rn(s, sum);
    if (use_r1) wv = fma(-c1, rkm1[i], wv);
    w[i] = wv;
    acc = fma(v, wv, acc);
  }
};

// VARIANT 2: window-blocked (TCOO-B) sweep, 1024 threads; VARIANT 1: row-owner CSR sweep, 256 threads; VARIANT 3: dense
// block sweep over D (dense_device.h), 256 threads.
template <int VARIANT, int K>
__global__ void __launch_bounds__(VARIANT == 2 ? BCOO_THREADS : HIPEIG_BLOCK)
lf_sweep_kernel(BcooView T, DenseView D, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                const double* __restrict__ val, int64_t nrows, const LfState* __restrict__ S,
                const double* __restrict__ rk, const double* __restrict__ rkm1, double* __restrict__ w,
                double* __restrict__ partials) {
  __shared__ double red[(VARIANT == 2 ? BCOO_THREADS : HIPEIG_BLOCK) / 64 * K];
  __shared__ double sh_s[K], sh_c1[K];
  __shared__ int sh_use[K];
  extern __shared__ double bcoo_lds[];
  if (S->done) return;
  if (threadIdx.x < K) {
    const LfCol c = S->col[threadIdx.x];
    const int use = (!c.done && c.itn >= 1);
    sh_s[threadIdx.x] = c.done ? 0.0 : c.s;
    sh_c1[threadIdx.x] = use ? c.beta / c.oldb : 0.0;
    sh_use[threadIdx.x] = use;
  }
  __syncthreads();
  LfScalarsEpilogue<K> epi;
  const int j = threadIdx.x % K;
  epi.s = sh_s[j]; epi.c1 = sh_c1[j]; epi.use_r1 = sh_use[j];
  epi.rk = rk; epi.rkm1 = rkm1; epi.w = w;
  double acc = 0.0;
  if (VARIANT == 3) dense_block_sweep<K>(D, rk, epi, acc);
  else if (VARIANT == 2) bcoo_wg_sweep<K>(T, rk, epi, acc, bcoo_lds);
  else csr_rowowner_block_sweep<K>(rowptr, col, val, nrows, rk, epi, acc);
  const double tot = block_reduce_cols<K>(acc, red);
  if (threadIdx.x < K) partials[(size_t)blockIdx.x * K + threadIdx.x] = tot;
}

// W -= (alpha / beta_k) R_k per column, and the partials of <w, w>.  S32: the finished w also goes, rounded to fp32
// (round to nearest even), to w32 - a slot of an fp32 basis - in one 8-byte store of the thread's column pair.
template <int K, bool S32 = false>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
lf_kc_kernel(int64_t n, const LfState* __restrict__ S, const double* __restrict__ pA, int nA,
             const double* __restrict__ rk, double* __restrict__ w, double* __restrict__ partials,
             float* __restrict__ w32 = nullptr) {
  __shared__ double red[HIPEIG_BLOCK / 64 * K];
  __shared__ double sh_c[K];
  if (S->done) return;
  const double alpha = block_sum_partials_cols<K>(pA, nA, red);
  if (threadIdx.x < K) {
    const LfCol c = S->col[threadIdx.x];
    sh_c[threadIdx.x] = c.done ? 0.0 : alpha / c.beta;
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;           // multiple of K/2: the column pair is fixed per thread
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j0 = (int)(t0 % (K / 2)) * 2;
  const double c0 = sh_c[j0], c1 = sh_c[j0 + 1];
  const double2* r2 = reinterpret_cast<const double2*>(rk);
  double2* w2 = reinterpret_cast<double2*>(w);
  double a0 = 0.0, a1 = 0.0;
  for (int64_t t = t0; t < n * (K / 2); t += stride) {
    const double2 rv = r2[t];
    double2 wv = w2[t];
    wv.x = fma(-c0, rv.x, wv.x); wv.y = fma(-c1, rv.y, wv.y);
    w2[t] = wv;
    if (S32) reinterpret_cast<float2*>(w32)[t] = make_float2((float)wv.x, (float)wv.y);
    a0 = fma(wv.x, wv.x, a0); a1 = fma(wv.y, wv.y, a1);
  }
  block_reduce_pairs<K>(a0, a1, red, partials + (size_t)blockIdx.x * K);
}

// The packed b, slot 0 of an fp32 basis, rounded once: a column pair per thread, as above.
__global__ void __launch_bounds__(HIPEIG_BLOCK)
lf_round_kernel(int64_t n2, const double2* __restrict__ r, float2* __restrict__ r32) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n2; t += stride) {
    const double2 v = r[t];
    r32[t] = make_float2((float)v.x, (float)v.y);
  }
}

// One workgroup of 256: thread (column = t / 32, shift = t % 32) advances that shift's rotation with the expressions of
// ms_rotate (minres_shifts.hip) - only c, s and tau are needed, no update coefficients - then threads 0..K-1 close their
// column's step.  probe: timing aid, nothing is stored.
template <int K>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
lf_scalar_kernel(LfState* __restrict__ S, LfShifts a, const double* __restrict__ pA, int nA, const double* __restrict__ pC,
                 int nC, double* __restrict__ alphas, double* __restrict__ betas, int ld, int probe) {
  __shared__ double red[HIPEIG_BLOCK / 64 * K];
  __shared__ double sh_alpha[K], sh_betan[K];
  __shared__ int sh_any[K], sh_done[K];
  if (S->done) return;
  const double alpha_t = block_sum_partials_cols<K>(pA, nA, red);
  const double ww_t = block_sum_partials_cols<K>(pC, nC, red);
  if (threadIdx.x < K) {
    sh_alpha[threadIdx.x] = alpha_t;
    sh_betan[threadIdx.x] = sqrt(ww_t);
    sh_any[threadIdx.x] = 0;
  }
  __syncthreads();
  const int cj = threadIdx.x / LF_MAX_SHIFTS, j = threadIdx.x % LF_MAX_SHIFTS;
  if (cj < K && j < S->nshift && !S->col[cj].done && S->live[cj][j]) {
    const LfCol c = S->col[cj];
    const double sign = a.sign, alpha = sh_alpha[cj], betan = sh_betan[cj];
    const double t_up = (c.itn == 0) ? 0.0 : -sign * c.beta;
    const double tdr = sign * (a.zr[j] - alpha), tdi = sign * a.zi[j];
    const double t_lo = -sign * betan;
    const double c1r = S->c1r[cj][j], c1i = S->c1i[cj][j], s1 = S->s1[cj][j];
    const double tmpr = S->c2r[cj][j] * t_up, tmpi = S->c2i[cj][j] * t_up;
    const double ddr = -s1 * tmpr + (c1r * tdr - c1i * tdi);  // -s1 tmp + c1 t_d
    const double ddi = -s1 * tmpi + (c1r * tdi + c1i * tdr);
    const double nu = hypot(hypot(ddr, ddi), t_lo);
    const double cr = ddr / nu, ci = ddi / nu, sn = t_lo / nu;
    const double tr = -sn * S->taur[cj][j], ti = -sn * S->taui[cj][j];
    const int live = hypot(tr, ti) > c.target;
    if (!probe) {
      S->c2r[cj][j] = c1r; S->c2i[cj][j] = c1i;
      S->c1r[cj][j] = cr; S->c1i[cj][j] = ci; S->s1[cj][j] = sn;
      S->taur[cj][j] = tr; S->taui[cj][j] = ti;
      S->its[cj][j] = c.itn + 1;
      S->live[cj][j] = live;
    }
    if (live) atomicOr(&sh_any[cj], 1);
  }
  __syncthreads();
  if (threadIdx.x < K) {
    LfCol c = S->col[threadIdx.x];
    if (!c.done && !probe) {
      const double betan = sh_betan[threadIdx.x];
      alphas[(size_t)threadIdx.x * ld + c.itn] = sh_alpha[threadIdx.x];
      betas[(size_t)threadIdx.x * (ld + 1) + c.itn + 1] = betan;
      c.oldb = c.beta; c.beta = betan; c.s = 1.0 / betan;
      c.itn += 1;
      c.done = (!sh_any[threadIdx.x] || c.itn >= S->maxiter || !(betan > 0.0)) ? 1 : 0;
      S->col[threadIdx.x] = c;
    }
    sh_done[threadIdx.x] = c.done;
  }
  __syncthreads();
  if (threadIdx.x == 0 && !probe) {
    int all = 1;
    for (int q = 0; q < K; ++q) all &= sh_done[q];
    S->done = all;
  }
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------------
// Pass 2 repeats pass 1's arithmetic, not only its mathematics: the coefficients G were computed from the alpha, beta of
// pass 1's vectors, and a Lanczos recurrence amplifies a rounding difference between the two passes' vectors into the
// rebuilt sums (measured: a single solution rebuilt through a pass 2 on normalised vectors missed its residual bound at
// rtol 1e-10 by 2.5 %).  So the vectors stay un-normalised here too, and an element goes through the same operations in
// the same order as in pass 1's sweep epilogue and KC: with the row-owner sweep the vectors are pass 1's bit for bit.
// Scalars of one step, per column: LF_TAB(K, NC) doubles - s_i = 1 / beta_i [K], beta_i / beta_{i-1} [K] (0 at i = 0),
// alpha_i / beta_i [K], G[i][K][NC] - formed on the host with the divisions pass 1's kernels make.
#define LF_TAB(K, NC) ((K) * (3 + (NC)))

// Doubles of workspace pass 2 takes at most (lf_pass2_impl; a prefix basis comes closest): the state record's area, the
// stream's and the product steps' tables for `steps` steps in all, two work vectors and NC packed combinations.
static int64_t lf_tail_doubles(int K, int NC, int64_t steps, int64_t nb) {
  const int64_t tab_d = (steps * (LF_TAB(K, NC) + K * (1 + NC) + 1) + 3 * K + 31) & ~(int64_t)31;
  return LF_HEAD_DOUBLES + tab_d + (2 + NC) * nb;
}

template <int K, int NC>
struct LfCombineEpilogue {
  double s, c1, c, g[NC];                                    // g[cc]: this thread's column, combination cc
  int acc_on, upd_on;                                        // i < m_r ; i + 1 < m_r
  const double* __restrict__ rk;
  double* __restrict__ rkm1;                                 // r_{i-1}, overwritten by r_{i+1} (same element, same thread)
  double* __restrict__ Q;                                    // NC packed blocks, nb doubles apart
  int64_t nb;
  // explicit fused operations with contraction off, as MsUpd::apply: every element rounds alike wherever it is computed
  __device__ __forceinline__ void elem(int64_t r, int j, double sum, double& acc) const {
#pragma clang fp contract(off)
    const int64_t i = r * K + j;
    const double rv = rk[i];
    if (acc_on) {
      const double v = mul_rn(s, rv);
#pragma unroll
      for (int cc = 0; cc < NC; ++cc) Q[i + cc * nb] = fma(g[cc], v, Q[i + cc * nb]);
    }
    if (upd_on) rkm1[i] = fma(-c, rv, fma(-c1, rkm1[i], mul_rn(s, sum)));
  }
};

// NC <= 2 serves a pass 2 without a basis; the product steps behind a prefix basis take NC up to 8 - the
// epilogue then holds NC coefficients per thread and makes NC read-modify-writes of Q per element, nothing else changes.
template <int VARIANT, int K, int NC>
__global__ void __launch_bounds__(VARIANT == 2 ? BCOO_THREADS : HIPEIG_BLOCK)
lf_combine_kernel(BcooView T, DenseView D, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                  const double* __restrict__ val, int64_t nrows, const double* __restrict__ tab, const int* __restrict__ m,
                  int step, const double* __restrict__ rk, double* __restrict__ rkm1, double* __restrict__ Q, int64_t nb) {
  __shared__ double sh_tab[LF_TAB(K, NC)];
  __shared__ int sh_m[K];
  extern __shared__ double bcoo_lds[];
  if (threadIdx.x < LF_TAB(K, NC)) sh_tab[threadIdx.x] = tab[threadIdx.x];
  if (threadIdx.x < K) sh_m[threadIdx.x] = m[threadIdx.x];
  __syncthreads();
  LfCombineEpilogue<K, NC> epi;
  const int j = threadIdx.x % K;
  epi.s = sh_tab[j]; epi.c1 = sh_tab[K + j]; epi.c = sh_tab[2 * K + j];
#pragma unroll
  for (int cc = 0; cc < NC; ++cc) epi.g[cc] = sh_tab[3 * K + j * NC + cc];
  epi.acc_on = step < sh_m[j]; epi.upd_on = step + 1 < sh_m[j];
  epi.rk = rk; epi.rkm1 = rkm1; epi.Q = Q; epi.nb = nb;
  double acc = 0.0;
  if (VARIANT == 3) dense_block_sweep<K>(D, rk, epi, acc);
  else if (VARIANT == 2) bcoo_wg_sweep<K>(T, rk, epi, acc, bcoo_lds);
  else csr_rowowner_block_sweep<K>(rowptr, col, val, nrows, rk, epi, acc);
}

// The last term of the columns that run to the call's last step: q[c] += G[r][i][c] v_i, no product.
template <int K, int NC>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
lf_last_term_kernel(int64_t n, const double* __restrict__ tab, const int* __restrict__ m, int step,
                    const double* __restrict__ rk, double* __restrict__ Q, int64_t nb) {
#pragma clang fp contract(off)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * K; i += stride) {
    const int j = (int)(i % K);
    if (step >= m[j]) continue;
    const double v = mul_rn(tab[j], rk[i]);
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) Q[i + cc * nb] = fma(tab[3 * K + j * NC + cc], v, Q[i + cc * nb]);
  }
}

static int lf_env_int(const char* name, int fallback) {
  const char* e = getenv(name);
  return (e && atoi(e) > 0) ? atoi(e) : fallback;
}

static int lf_reserve(hipeig_ctx* c, int64_t need) {
  if (c->lf_ws_doubles >= need) return 0;
  if (c->lf_ws) HIPEIG_CHECK(hipFree(c->lf_ws));
  c->lf_ws = nullptr; c->lf_ws_doubles = 0;
  HIPEIG_CHECK(hipMalloc((void**)&c->lf_ws, (size_t)need * sizeof(double)));
  c->lf_ws_doubles = need;
  return 0;
}

// interleave width of a block of k columns: as hipeig_spmm (<= 4 take the narrow interleave); HIPEIG_LF_WIDTH = 8 forces the
// wide one (the order in which a row's terms are added depends on the width, so runs are comparable bit for bit only at
// the same one)
static int lf_width(int k) {
  if (lf_env_int("HIPEIG_LF_WIDTH", 0) == 8) return 8;
  return k <= 4 ? 4 : 8;
}

// ---- kept basis --------------------------------------------------------------------------------------------------------
// Pass 1 writes every r_k = beta_k v_k once anyway.  In keep mode step k's w goes to slot k + 1 of the basis instead of the
// oldest ring buffer (the sweep reads slots k and k - 1, KC updates slot k + 1 in place), so the vectors of the run stay
// in HBM at no extra byte of traffic, and pass 2 becomes one stream over them (lf_basis_combine_kernel) - pass 1's vectors
// themselves, whichever sweep produced them.  Slots are carved from segments of seg_slots slots, allocated while the run
// advances; a fresh slot is fully written by the sweep (every row, padding columns as 0) before anything reads it.
//
// fp32 basis (basis_mode 3 / 4, elem_bytes = 4): pass 2 only forms q = sum_i g_i v_i, so the copy it streams over may be
// narrower than the vectors of the recurrence.  Pass 1 runs in the ring of three exactly as mode 0 - the same kernels on
// the same operands, so the same scalars - and KC's S32 variant leaves step k's finished w, rounded, in slot k + 1 (slot 0:
// the packed b, lf_round_kernel): 4 n K more bytes written per step.  A slot is nb floats; KC writes the n K elements the
// stream reads (padding and finished columns as 0).  A prefix of such a basis cannot restart pass 2's recurrence from
// its slots - rounded start vectors would no longer repeat pass 1's arithmetic - so the basis owns two fp64 hand-over
// vectors: r_{p-1} and r_{p-2}, copied out of the ring in stream order before step p - 1 is enqueued.  They are
// allocations of their own, outside the byte budget (which is the segments') and outside the pool, and count as held.
struct hipeig_lanczos_basis {
  int K, k, seg_slots, nseg, seg_cap;
  int elem_bytes;                                             // 8, or 4: slots of nb floats
  int64_t n, nb, nrows;                                       // nb: elements per slot; nrows: the operator's
  size_t seg_bytes;
  int steps[BCOO_KMAX];                                       // vectors kept per column: v_0 .. v_{steps - 1}
  int ran[BCOO_KMAX];                                         // steps the column ran: more than `steps` behind a prefix
  double** seg;
  double* hand[2];                                            // fp32 prefix: r_{p-1}, r_{p-2} in fp64 (nb doubles each), else null
};

void hipeig_lf_pool_clear(hipeig_ctx* c) {
  for (int i = 0; i < c->lf_pool_n; ++i) (void)hipFree(c->lf_pool[i].p);
  c->lf_pool_n = 0; c->lf_pool_bytes = 0;
}

// A segment of `bytes`: a pooled one of that size, else a fresh allocation.  nullptr when the device has no room even
// after the pool was emptied - an expected outcome (the caller falls back to the ring), so the error state is cleared.
static double* lf_pool_take(hipeig_ctx* c, size_t bytes) {
  for (int i = 0; i < c->lf_pool_n; ++i)
    if (c->lf_pool[i].bytes == bytes) {
      double* p = c->lf_pool[i].p;
      c->lf_pool[i] = c->lf_pool[--c->lf_pool_n];
      c->lf_pool_bytes -= (int64_t)bytes;
      return p;
    }
  double* p = nullptr;
  if (hipMalloc((void**)&p, bytes) == hipSuccess) return p;
  (void)hipGetLastError();
  if (c->lf_pool_n == 0) return nullptr;
  hipeig_lf_pool_clear(c);
  if (hipMalloc((void**)&p, bytes) == hipSuccess) return p;
  (void)hipGetLastError();
  return nullptr;
}

static void lf_pool_give(hipeig_ctx* c, double* p, size_t bytes) {
  if (c->lf_pool_n == c->lf_pool_cap) {
    const int cap = c->lf_pool_cap ? 2 * c->lf_pool_cap : 64;
    LfPoolEntry* grown = (LfPoolEntry*)realloc(c->lf_pool, (size_t)cap * sizeof(LfPoolEntry));
    if (!grown) { (void)hipFree(p); return; }
    c->lf_pool = grown; c->lf_pool_cap = cap;
  }
  c->lf_pool[c->lf_pool_n].p = p; c->lf_pool[c->lf_pool_n].bytes = bytes;
  ++c->lf_pool_n;
  c->lf_pool_bytes += (int64_t)bytes;
}

static inline double* lf_slot(const hipeig_lanczos_basis* B, int i) {
  char* s = reinterpret_cast<char*>(B->seg[i / B->seg_slots]) + (int64_t)(i % B->seg_slots) * B->nb * B->elem_bytes;
  return reinterpret_cast<double*>(s);
}

static inline float* lf_slot32(const hipeig_lanczos_basis* B, int i) { return reinterpret_cast<float*>(lf_slot(B, i)); }

// One more segment, unless it would exceed the byte budget or the device has no room: 0 = added.
static int lf_basis_grow(hipeig_ctx* c, hipeig_lanczos_basis* B, int64_t budget) {
  if ((int64_t)(B->nseg + 1) * (int64_t)B->seg_bytes > budget) return 1;
  if (B->nseg == B->seg_cap) {
    const int cap = B->seg_cap ? 2 * B->seg_cap : 16;
    double** grown = (double**)realloc(B->seg, (size_t)cap * sizeof(double*));
    if (!grown) return 1;
    B->seg = grown; B->seg_cap = cap;
  }
  double* p = lf_pool_take(c, B->seg_bytes);
  if (!p) return 1;
  B->seg[B->nseg++] = p;
  return 0;
}

// Hand the segments from index `from` on back to the context (work enqueued on them is ordered before their next use:
// one stream).
static void lf_basis_trim(hipeig_ctx* c, hipeig_lanczos_basis* B, int from) {
  while (B->nseg > from) lf_pool_give(c, B->seg[--B->nseg], B->seg_bytes);
}

static void lf_basis_drop_hand(hipeig_ctx* c, hipeig_lanczos_basis* B) {
  for (int q = 0; q < 2; ++q) {
    if (B->hand[q]) (void)hipFree(B->hand[q]);               // not pooled: a vector can never serve as a segment
    B->hand[q] = nullptr;
  }
}

static void lf_basis_free(hipeig_ctx* c, hipeig_lanczos_basis* B) {
  if (!B) return;
  lf_basis_trim(c, B, 0);
  lf_basis_drop_hand(c, B);
  free(B->seg);
  free(B);
}

// keep != nullptr: keep mode with `budget` bytes for the segments; *keep receives the basis, or nullptr when it was not kept
// (budget or device memory ran out: the run went on in the ring of three, same kernels, same operands, same scalars).
// prefix: when the next segment is refused the ones held stay and are written to their last slot, p = nseg * seg_slots
// vectors; vector i >= p lives in ring buffer i % 3, so the hand-over is a choice of pointers at enqueue time - steps
// p - 1 and p read their operands from the slots - and may fall inside a chunk.
// elem 4: an fp32 basis.  Every vector of the recurrence lives in the ring; a slot only receives KC's rounded copy, so a
// refused segment costs no copy (keep: the basis is freed; prefix: the slots held stay, and r_{p-1}, r_{p-2} are copied
// from the ring to the hand-over vectors before step p - 1 - which overwrites neither - is enqueued).
template <int K>
static int lf_scalars_impl(hipeig_ctx* c, hipeig_csr* A, double sign, int k, const double* const* b, int nshift,
                           const double* zr, const double* zi, double rtol, double atol, int maxiter, double* alphas,
                           double* betas, int* iterations, double* estimates, int* info, double* out_stats,
                           int64_t budget, hipeig_lanczos_basis** keep, int prefix, int elem) {
  const int64_t n = A->nrows;
  const int64_t nb = ((n * K + 31) & ~(int64_t)31);
  const int64_t ld = maxiter;
  const int64_t tabs = ((int64_t)K * (2 * ld + 1) + 31) & ~(int64_t)31;
  int64_t need = LF_HEAD_DOUBLES + tabs + 3 * nb;
  // a prefix is followed by a pass 2 with product steps: its workspace (NC <= 2) is taken before the first segment, so
  // that the basis cannot eat the room of the pass it serves
  if (keep && prefix && lf_tail_doubles(K, 2, maxiter, nb) > need) need = lf_tail_doubles(K, 2, maxiter, nb);
  if (lf_reserve(c, need)) return 1;
  if (!c->h_lf_state) HIPEIG_CHECK(hipHostMalloc((void**)&c->h_lf_state, sizeof(LfState), hipHostMallocDefault));
  LfState* V = reinterpret_cast<LfState*>(c->lf_ws);
  double* d_alphas = c->lf_ws + LF_HEAD_DOUBLES;
  double* d_betas = d_alphas + (int64_t)K * ld;
  double* R[3] = {c->lf_ws + LF_HEAD_DOUBLES + tabs, c->lf_ws + LF_HEAD_DOUBLES + tabs + nb,
                  c->lf_ws + LF_HEAD_DOUBLES + tabs + 2 * nb};

  LfState* h = reinterpret_cast<LfState*>(c->h_lf_state);
  memset(h, 0, sizeof(LfState));
  h->nshift = nshift; h->maxiter = maxiter;
  int live = 0;
  for (int j = 0; j < K; ++j) {
    double bb = 0.0;
    if (j < k && hipeig_dot(c, n, b[j], b[j], &bb)) return 1;
    LfCol& cj = h->col[j];
    if (bb > 0.0) {
      cj.beta1 = sqrt(bb); cj.beta = cj.beta1; cj.oldb = 0.0; cj.s = 1.0 / cj.beta1;
      cj.target = fmax(atol, rtol * cj.beta1);
      for (int q = 0; q < nshift; ++q) {
        h->c1r[j][q] = 1.0; h->c2r[j][q] = 1.0; h->taur[j][q] = cj.beta1; h->live[j][q] = 1;
      }
      ++live;
    } else {
      cj.done = 1;                                            // padding column, or b == 0: q = 0 with no product
    }
    if (j < k) betas[(size_t)j * (ld + 1)] = cj.beta1;
  }
  h->done = live == 0;
  if (live == 0) return 0;
  // measurement aid (tools/shifted_feast_bench.py): 1 / 2 / 3 launch ONLY the sweep / KC / scalar kernel, `maxiter` times on a
  // record that does not advance - the time of that phase alone; the results are meaningless
  const int probe = lf_env_int("HIPEIG_LF_PROBE", 0);
  // steps between two looks at the state record; kernels launched past the last column's stop return at once
  const int chunk = lf_env_int("HIPEIG_LF_CHUNK", 32);
  const bool narrow = elem == 4;
  struct Guard {
    hipeig_ctx* c; hipeig_lanczos_basis* B;
    ~Guard() { lf_basis_free(c, B); }
  } kept{c, nullptr};
  if (keep && !probe) {
    hipeig_lanczos_basis* B = (hipeig_lanczos_basis*)calloc(1, sizeof(hipeig_lanczos_basis));
    HIPEIG_REQUIRE(B != nullptr, "out of host memory");
    B->K = K; B->k = k; B->n = n; B->nb = nb; B->nrows = A->nrows; B->elem_bytes = elem;
    B->seg_slots = lf_env_int("HIPEIG_LF_SEGMENT", 32);       // slots per segment
    B->seg_bytes = (size_t)B->seg_slots * (size_t)nb * (size_t)elem;
    kept.B = B;
    bool ok = true;
    if (narrow && prefix)                                     // the hand-over vectors, before the segments can eat their room
      for (int q = 0; q < 2 && ok; ++q)
        if (hipMalloc((void**)&B->hand[q], (size_t)nb * sizeof(double)) != hipSuccess) {
          (void)hipGetLastError();
          B->hand[q] = nullptr; ok = false;
        }
    if (!ok || lf_basis_grow(c, B, budget)) { lf_basis_free(c, B); kept.B = nullptr; }
  }
  if (kept.B && !narrow) {
    if (hipeig_block_pack(c, K, n, k, b, lf_slot(kept.B, 0))) return 1;
  } else {
    if (hipeig_block_pack(c, K, n, k, b, R[0])) return 1;
    HIPEIG_CHECK(hipMemsetAsync(R[1], 0, (size_t)nb * 2 * sizeof(double), c->stream));
    if (kept.B)
      hipLaunchKernelGGL(lf_round_kernel, dim3(grid_stream(n * K)), dim3(HIPEIG_BLOCK), 0, c->stream, n * (K / 2),
                         reinterpret_cast<const double2*>(R[0]), reinterpret_cast<float2*>(lf_slot32(kept.B, 0)));
  }
  HIPEIG_CHECK(hipMemcpyAsync(V, h, sizeof(LfState), hipMemcpyHostToDevice, c->stream));
  if (hipeig_sync_checked(c)) return 4;                       // the pinned record is rewritten by the first copy-back

  BlockSweepPlan plan;
  if (const int rc = block_sweep_plan_build<K>(c, A, 1, &plan)) return rc;
  if (const int rc = block_sweep_set_lds_limit(plan, lf_sweep_kernel<2, K>)) return rc;
  const int nPA = plan.nPA;
  const int gE = grid_for(n * (K / 2), lf_env_int("HIPEIG_LF_PER_THREAD", 32));
  double* pA = c->d_partials;
  double* pC = c->d_partials + BLOCK_PART_STRIDE;
  HIPEIG_REQUIRE(c->partials_doubles >= (size_t)2 * BLOCK_PART_STRIDE, "partial-sum workspace too small");

  LfShifts sh;
  memset(&sh, 0, sizeof(sh));
  sh.sign = sign;
  for (int q = 0; q < nshift; ++q) { sh.zr[q] = zr[q]; sh.zi[q] = zi[q]; }

  auto enqueue_sweep = [&](const double* rk, const double* rkm1, double* w) {
    block_sweep_launch(c, plan, [&](auto v, int grid, int threads, size_t lds, const BcooView& tv, int off) {
      hipLaunchKernelGGL((lf_sweep_kernel<decltype(v)::value, K>), dim3(grid), dim3(threads), lds, c->stream, tv, plan.dview, A->d_rowptr,
                         A->d_col, A->d_val, n, (const LfState*)V, rk, rkm1, w, pA + (size_t)off * K);
    });
  };

  int steps = 0;
  int cap = INT_MAX;                                          // prefix mode, once a segment was refused: the slots held
  auto vec = [&](int i) { return (kept.B && !narrow && i < cap) ? lf_slot(kept.B, i) : R[i % 3]; };
  while (steps < maxiter) {
    const int kend = (steps + chunk < maxiter) ? steps + chunk : maxiter;
    // the segments this chunk writes (slots up to kend) before it is enqueued; when the budget or the device says no, the
    // two live vectors move to the ring and the run goes on as plain pass 1 - or, in prefix mode, the slots held are all
    // there will be (slot `steps` exists: cap > steps)
    while (kept.B && cap == INT_MAX && kept.B->nseg * kept.B->seg_slots <= kend)
      if (lf_basis_grow(c, kept.B, budget)) {
        if (prefix) { cap = kept.B->nseg * kept.B->seg_slots; break; }
        if (!narrow) {
          HIPEIG_CHECK(hipMemcpyAsync(R[steps % 3], lf_slot(kept.B, steps), (size_t)nb * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
          if (steps)
            HIPEIG_CHECK(hipMemcpyAsync(R[(steps + 2) % 3], lf_slot(kept.B, steps - 1), (size_t)nb * sizeof(double),
                                        hipMemcpyDeviceToDevice, c->stream));
        }
        lf_basis_free(c, kept.B);
        kept.B = nullptr;
      }
    for (; steps < kend; ++steps) {
      const int kk = probe ? 0 : steps;
      double* rk = vec(kk);
      double* w = vec(kk + 1);
      double* rkm1 = kk ? vec(kk - 1) : (kept.B && !narrow) ? lf_slot(kept.B, 0) : R[2];   // step 0 reads no r_{-1}
      if (kept.B && narrow && steps == cap - 1) {             // r_{p-1} is complete; step p - 1 writes R[p % 3]
        HIPEIG_CHECK(hipMemcpyAsync(kept.B->hand[0], R[steps % 3], (size_t)nb * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        if (steps)
          HIPEIG_CHECK(hipMemcpyAsync(kept.B->hand[1], R[(steps + 2) % 3], (size_t)nb * sizeof(double),
                                      hipMemcpyDeviceToDevice, c->stream));
      }
      if (!probe || probe == 1) enqueue_sweep(rk, rkm1, w);
      if (kept.B && narrow && kk + 1 < cap)
        hipLaunchKernelGGL((lf_kc_kernel<K, true>), dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, (const LfState*)V,
                           (const double*)pA, nPA, (const double*)rk, w, pC, lf_slot32(kept.B, kk + 1));
      else if (!probe || probe == 2)
        hipLaunchKernelGGL(lf_kc_kernel<K>, dim3(gE), dim3(HIPEIG_BLOCK), 0, c->stream, n, (const LfState*)V,
                           (const double*)pA, nPA, (const double*)rk, w, pC, (float*)nullptr);
      if (!probe || probe == 3)
        hipLaunchKernelGGL(lf_scalar_kernel<K>, dim3(1), dim3(HIPEIG_BLOCK), 0, c->stream, V, sh, (const double*)pA, nPA,
                           (const double*)pC, gE, d_alphas, d_betas, (int)ld, probe ? 1 : 0);
    }
    HIPEIG_CHECK(hipGetLastError());
    HIPEIG_CHECK(hipMemcpyAsync(h, V, sizeof(LfState), hipMemcpyDeviceToHost, c->stream));
    if (hipeig_sync_checked(c)) return 4;
    if (h->done) break;
  }
  HIPEIG_REQUIRE(probe || h->done, "the Lanczos pass left the step loop without a stop in every column");
  int products = 0;
  for (int j = 0; j < k; ++j) {
    const int m = h->col[j].itn;
    if (m > products) products = m;
    if (m > 0 && !probe) {
      HIPEIG_CHECK(hipMemcpyAsync(alphas + (size_t)j * ld, d_alphas + (size_t)j * ld, (size_t)m * sizeof(double),
                                  hipMemcpyDeviceToHost, c->stream));
      HIPEIG_CHECK(hipMemcpyAsync(betas + (size_t)j * (ld + 1) + 1, d_betas + (size_t)j * (ld + 1) + 1,
                                  (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    int any = 0;
    for (int q = 0; q < nshift; ++q) {
      iterations[(size_t)j * nshift + q] = h->its[j][q];
      estimates[(size_t)j * nshift + q] = hypot(h->taur[j][q], h->taui[j][q]);
      any |= h->live[j][q];
    }
    info[j] = (probe || any) ? maxiter : 0;
    if (out_stats) out_stats[1 + j] = m;
    if (kept.B) { kept.B->steps[j] = m < cap ? m : cap; kept.B->ran[j] = m; }
  }
  if (out_stats) out_stats[0] = probe ? maxiter : products;
  if (hipeig_sync_checked(c)) return 4;
  if (kept.B) {                                               // memory follows the steps taken: slots 0 .. products - 1
    const int held = products < cap ? products : cap;        // a run that stopped before the cap holds a whole basis
    lf_basis_trim(c, kept.B, (held + kept.B->seg_slots - 1) / kept.B->seg_slots);
    if (products <= cap) lf_basis_drop_hand(c, kept.B);      // a whole basis: no recurrence will restart behind it
    *keep = kept.B;
    kept.B = nullptr;
  }
  return 0;
}

extern "C" int hipeig_lanczos_block_scalars(hipeig_ctx* c, hipeig_csr* A, double sign, int k, const double* const* b,
                                            int nshift, const double* zr, const double* zi, double rtol, double atol,
                                            int maxiter, double* alphas, double* betas, int* iterations, double* estimates,
                                            int* info, double* out_stats, int basis_mode, int64_t basis_bytes,
                                            hipeig_lanczos_basis** basis) {
  HIPEIG_REQUIRE(basis_mode >= 0 && basis_mode <= 4, "basis mode: 0 none, 1 keep, 2 keep a prefix, 3 / 4 the same in fp32");
  HIPEIG_REQUIRE(basis_mode == 0 || basis != nullptr, "null argument");
  if (basis) *basis = nullptr;
  HIPEIG_REQUIRE(basis_mode == 0 || basis_bytes >= 0, "negative byte budget");
  HIPEIG_REQUIRE(b && zr && zi && alphas && betas && iterations && estimates && info, "null argument");
  HIPEIG_REQUIRE(k >= 1 && k <= BCOO_KMAX, "1 to 8 right-hand sides per call");
  HIPEIG_REQUIRE(nshift >= 1 && nshift <= LF_MAX_SHIFTS, "1 to 32 shifts per run");
  HIPEIG_REQUIRE(sign == 1.0 || sign == -1.0, "sign must be +1 or -1");
  HIPEIG_REQUIRE(maxiter >= 1, "maxiter must be positive");
  HIPEIG_REQUIRE(!c->collectives, "the Lanczos filter runs on whole vectors (no row partition)");
  HIPEIG_REQUIRE(A->nrows == A->ncols, "the Lanczos run needs a square operator");
  for (int j = 0; j < k; ++j) {
    HIPEIG_REQUIRE(b[j] != nullptr, "null right-hand side");
    info[j] = 0;
    betas[(size_t)j * (maxiter + 1)] = 0.0;
    for (int q = 0; q < nshift; ++q) { iterations[(size_t)j * nshift + q] = 0; estimates[(size_t)j * nshift + q] = 0.0; }
  }
  if (out_stats) memset(out_stats, 0, (size_t)(1 + k) * sizeof(double));
  if (A->nrows == 0) return 0;
  hipeig_lanczos_basis** keep = basis_mode ? basis : nullptr;
  const int prefix = basis_mode == 2 || basis_mode == 4;
  const int elem = basis_mode >= 3 ? 4 : 8;
  if (lf_width(k) == 4)
    return lf_scalars_impl<4>(c, A, sign, k, b, nshift, zr, zi, rtol, atol, maxiter, alphas, betas, iterations, estimates, info,
                              out_stats, basis_bytes, keep, prefix, elem);
  return lf_scalars_impl<8>(c, A, sign, k, b, nshift, zr, zi, rtol, atol, maxiter, alphas, betas, iterations, estimates, info,
                            out_stats, basis_bytes, keep, prefix, elem);
}

// Table records of the product steps `first` .. m[j] - 1 of every column, record i at t0 + (i - first) * LF_TAB.
template <int K, int NC>
static void lf_fill_product_tab(double* t0, int first, int k, const int* m, const double* const* alphas,
                                const double* const* betas, const double* const* G) {
  for (int j = 0; j < k; ++j)
    for (int i = first; i < m[j]; ++i) {
      double* t = t0 + (int64_t)(i - first) * LF_TAB(K, NC);
      t[j] = 1.0 / betas[j][i];                                // the divisions of pass 1: LfCol::s, the sweep's c1, KC's c
      t[K + j] = i ? betas[j][i] / betas[j][i - 1] : 0.0;
      t[2 * K + j] = alphas[j][i] / betas[j][i];
      for (int cc = 0; cc < NC; ++cc) t[3 * K + j * NC + cc] = G[j][(size_t)i * NC + cc];
    }
}

// Steps first .. mmax - 2 with a product each, then the last term: vector i lives in Vb[i & 1] (Vb[first & 1] = r_first,
// the other r_{first-1}, zeros at first = 0); d_tab holds the records from `first` on, Q the NC packed sums so far.
template <int K, int NC>
static int lf_enqueue_products(hipeig_ctx* c, hipeig_csr* A, const double* d_tab, const int* d_m, int first, int mmax,
                               double* const* Vb, double* Q, int64_t nb) {
  const int64_t n = A->nrows;
  BlockSweepPlan plan;
  if (const int rc = block_sweep_plan_build<K>(c, A, 1, &plan)) return rc;
  if (const int rc = block_sweep_set_lds_limit(plan, lf_combine_kernel<2, K, NC>)) return rc;
  for (int i = first; i + 1 < mmax; ++i) {
    const double* tab = d_tab + (int64_t)(i - first) * LF_TAB(K, NC);
    const double* rk = Vb[i & 1];
    double* rkm1 = Vb[(i + 1) & 1];
    block_sweep_launch(c, plan, [&](auto v, int grid, int threads, size_t lds, const BcooView& tv, int) {      // no partials
      hipLaunchKernelGGL((lf_combine_kernel<decltype(v)::value, K, NC>), dim3(grid), dim3(threads), lds, c->stream, tv, plan.dview,
                         A->d_rowptr, A->d_col, A->d_val, n, tab, d_m, i, rk, rkm1, Q, nb);
    });
  }
  hipLaunchKernelGGL((lf_last_term_kernel<K, NC>), dim3(grid_stream(n * K)), dim3(HIPEIG_BLOCK), 0, c->stream, n,
                     d_tab + (int64_t)(mmax - 1 - first) * LF_TAB(K, NC), d_m, mmax - 1, (const double*)Vb[(mmax - 1) & 1], Q,
                     nb);
  HIPEIG_CHECK(hipGetLastError());
  return 0;
}

// q[j * NC + cc] <- column j of packed block cc of Q
template <int K, int NC>
static int lf_unpack_combinations(hipeig_ctx* c, int64_t n, int k, const double* Q, int64_t nb, double* const* q) {
  for (int cc = 0; cc < NC; ++cc) {
    double* part[BCOO_KMAX];
    for (int j = 0; j < k; ++j) part[j] = q[j * NC + cc];
    if (hipeig_block_unpack(c, K, n, k, Q + (int64_t)cc * nb, part)) return 1;
  }
  return 0;
}

// ---- pass 2 from a kept basis ------------------------------------------------------------------------------------------
// q[c] = sum_{i < m_j} G[j][i][c] v_i, v_i = r_i / beta_i, over the stored vectors: one stream, no product.  A thread owns
// one double2 of the interleaved [row][K] layout - a fixed pair of columns, as lf_kc_kernel - keeps its 2 NC accumulators
// in registers and takes the slots in ascending order, LF_BC_UNROLL independent 16-byte loads in flight; q is written
// once.  Every element goes through the operations of LfCombineEpilogue::elem / lf_last_term_kernel - v = mul_rn(1/beta_i,
// r_i), q = fma(G, v, q), contraction off - so with the row-owner sweep the result equals the product pass bit for bit.
// The coefficients differ per column (not wave-uniform): they and the slot pointers are staged through LDS, LF_BC_STEPS
// steps at a time.  Table of one step: 1 / beta_i [K], G[i][K][NC], zero from a column's m_j on (those terms are skipped).
#define LF_BC_STEPS 32
#define LF_BC_UNROLL 4
#define LF_BC_TAB(K, NC) ((K) * (1 + (NC)))

// a slot pointer comes out of LDS, so the compiler no longer knows that it points to global memory: say so, or the
// loads become flat ones
typedef double lf_double2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) lf_double2* lf_global_double2;

template <int K, int NC>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
lf_basis_combine_kernel(int64_t n2, int mmax, const double* __restrict__ tab, const double* const* __restrict__ slots,
                        const int* __restrict__ m, double* __restrict__ Q, int64_t nb) {
#pragma clang fp contract(off)
  constexpr int TW = LF_BC_TAB(K, NC);
  __shared__ double sh_tab[LF_BC_STEPS * TW];
  __shared__ const double* sh_slot[LF_BC_STEPS];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;           // multiple of K/2: the column pair is fixed per thread
  const int j0 = (int)(threadIdx.x % (K / 2)) * 2;                  // blockDim.x is one too
  const int m0 = m[j0], m1 = m[j0 + 1];
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n2; base += stride) {   // uniform per workgroup (barriers inside)
    const int64_t t = base + threadIdx.x;
    const bool on = t < n2;
    double a0[NC], a1[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) { a0[cc] = 0.0; a1[cc] = 0.0; }
    for (int i0 = 0; i0 < mmax; i0 += LF_BC_STEPS) {
      const int ns = (mmax - i0 < LF_BC_STEPS) ? mmax - i0 : LF_BC_STEPS;
      __syncthreads();
      for (int x = threadIdx.x; x < ns * TW; x += blockDim.x) sh_tab[x] = tab[(int64_t)i0 * TW + x];
      if ((int)threadIdx.x < ns) sh_slot[threadIdx.x] = slots[i0 + threadIdx.x];
      __syncthreads();
      if (!on) continue;
      auto term = [&](int ii, const lf_double2 rv) {
        const double* tb = sh_tab + ii * TW;
        const double v0 = mul_rn(tb[j0], rv.x), v1 = mul_rn(tb[j0 + 1], rv.y);
        if (i0 + ii < m0) {
#pragma unroll
          for (int cc = 0; cc < NC; ++cc) a0[cc] = fma(tb[K + j0 * NC + cc], v0, a0[cc]);
        }
        if (i0 + ii < m1) {
#pragma unroll
          for (int cc = 0; cc < NC; ++cc) a1[cc] = fma(tb[K + (j0 + 1) * NC + cc], v1, a1[cc]);
        }
      };
      int ii = 0;
      for (; ii + LF_BC_UNROLL <= ns; ii += LF_BC_UNROLL) {
        lf_double2 rv[LF_BC_UNROLL];
#pragma unroll
        for (int u = 0; u < LF_BC_UNROLL; ++u) rv[u] = ((lf_global_double2)sh_slot[ii + u])[t];
#pragma unroll
        for (int u = 0; u < LF_BC_UNROLL; ++u) term(ii + u, rv[u]);
      }
      for (; ii < ns; ++ii) term(ii, ((lf_global_double2)sh_slot[ii])[t]);
    }
    if (on) {
#pragma unroll
      for (int cc = 0; cc < NC; ++cc) reinterpret_cast<double2*>(Q + (int64_t)cc * nb)[t] = make_double2(a0[cc], a1[cc]);
    }
  }
}

// The same stream over fp32 slots.  An element goes through the operations above in the same ascending order -
// v = mul_rn(1/beta_i, (double)r32), q = fma(G, v, q), fp64 accumulators, contraction off - so the result differs from the
// fp64 basis's only by the rounding of the stored elements: ||q32 - q64|| <= 2^-24 sum_i |g_i| ||v_i||.  A thread owns
// CW = 4 adjacent columns of a row, which keeps the loads at 16 bytes per lane (a whole row at K = 4, half a row at
// K = 8), with 4 NC accumulators.  (The pair mapping above with 8-byte loads was measured beside it and dropped:
// DESIGN.md 3.6.)
typedef float lf_floatv4 __attribute__((ext_vector_type(4)));

template <int K, int NC>
__global__ void __launch_bounds__(HIPEIG_BLOCK)
lf_basis_combine32_kernel(int64_t nt, int mmax, const double* __restrict__ tab, const double* const* __restrict__ slots,
                          const int* __restrict__ m, double* __restrict__ Q, int64_t nb) {
#pragma clang fp contract(off)
  constexpr int CW = 4;
  typedef lf_floatv4 vec_t;
  typedef const __attribute__((address_space(1))) vec_t* global_vec;
  constexpr int TW = LF_BC_TAB(K, NC);
  __shared__ double sh_tab[LF_BC_STEPS * TW];
  __shared__ const double* sh_slot[LF_BC_STEPS];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;           // multiple of K/CW: the columns are fixed per thread
  const int j0 = (int)(threadIdx.x % (K / CW)) * CW;                // blockDim.x is one too
  int mj[CW];
#pragma unroll
  for (int x = 0; x < CW; ++x) mj[x] = m[j0 + x];
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < nt; base += stride) {   // uniform per workgroup (barriers inside)
    const int64_t t = base + threadIdx.x;
    const bool on = t < nt;
    double a[CW][NC];
#pragma unroll
    for (int x = 0; x < CW; ++x)
#pragma unroll
      for (int cc = 0; cc < NC; ++cc) a[x][cc] = 0.0;
    for (int i0 = 0; i0 < mmax; i0 += LF_BC_STEPS) {
      const int ns = (mmax - i0 < LF_BC_STEPS) ? mmax - i0 : LF_BC_STEPS;
      __syncthreads();
      for (int x = threadIdx.x; x < ns * TW; x += blockDim.x) sh_tab[x] = tab[(int64_t)i0 * TW + x];
      if ((int)threadIdx.x < ns) sh_slot[threadIdx.x] = slots[i0 + threadIdx.x];
      __syncthreads();
      if (!on) continue;
      auto term = [&](int ii, const vec_t rv) {
        const double* tb = sh_tab + ii * TW;
#pragma unroll
        for (int x = 0; x < CW; ++x) {
          const double v = mul_rn(tb[j0 + x], (double)rv[x]);
          if (i0 + ii < mj[x]) {
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) a[x][cc] = fma(tb[K + (j0 + x) * NC + cc], v, a[x][cc]);
          }
        }
      };
      int ii = 0;
      for (; ii + LF_BC_UNROLL <= ns; ii += LF_BC_UNROLL) {
        vec_t rv[LF_BC_UNROLL];
#pragma unroll
        for (int u = 0; u < LF_BC_UNROLL; ++u) rv[u] = ((global_vec)sh_slot[ii + u])[t];
#pragma unroll
        for (int u = 0; u < LF_BC_UNROLL; ++u) term(ii + u, rv[u]);
      }
      for (; ii < ns; ++ii) term(ii, ((global_vec)sh_slot[ii])[t]);
    }
    if (on) {
#pragma unroll
      for (int cc = 0; cc < NC; ++cc)
#pragma unroll
        for (int x = 0; x < CW; x += 2)
          reinterpret_cast<double2*>(Q + (int64_t)cc * nb)[t * (CW / 2) + x / 2] = make_double2(a[x][cc], a[x + 1][cc]);
    }
  }
}

// ---- pass 2, host side -------------------------------------------------------------------------------------------------
// One path with a plan (prefix_split in lanczos_filter.py states it): the terms i < stream come from the basis's slots in
// one stream (columns masked by min(m_j, stream)) that leaves Q packed in the workspace; the recurrence takes over at step
// first = stream on two work vectors and makes a product per step up to mmax - 2 (columns masked by m_j), then the last term.
//   no basis                stream = 0        r_0 = packed b, r_{-1} = zeros                          mmax - 1 products
//   basis holds p >= mmax   stream = mmax     -                                                       none
//   basis holds p <  mmax   stream = p - 1    r_{p-1}, r_{p-2} copied from their slots (zeros, p = 1)  mmax - p products
//                                             (an fp32 basis: from its fp64 hand-over vectors)
// The basis is never written: it serves any number of calls.  Every element meets the mul_rn / fma sequence of the
// product steps in ascending i (the stream's accumulators start from 0, as Q does without a stream), so with the
// row-owner sweep the three situations agree bit for bit.
struct LfPlan {
  int mmax, stream;
  int64_t o_slots, o_prod, o_m, tab_d;                         // the table's parts, in doubles: see lf_fill_pass2_tab
  bool recurs() const { return stream < mmax; }
  int products() const { return recurs() ? mmax - 1 - stream : 0; }
};

template <int K, int NC>
static LfPlan lf_plan(const hipeig_lanczos_basis* B, int k, const int* m) {
  LfPlan P{};
  int p = 0;                                                  // vectors the basis holds for its longest column
  for (int j = 0; j < k; ++j) {
    P.mmax = m[j] > P.mmax ? m[j] : P.mmax;
    if (B) p = B->steps[j] > p ? B->steps[j] : p;
  }
  P.stream = !B ? 0 : p >= P.mmax ? P.mmax : p - 1;
  P.o_slots = (int64_t)P.stream * LF_BC_TAB(K, NC);
  P.o_prod = P.o_slots + P.stream;
  P.o_m = P.o_prod + (P.recurs() ? (int64_t)(P.mmax - P.stream) * LF_TAB(K, NC) : 0);
  P.tab_d = (P.o_m + K + 31) & ~(int64_t)31;
  return P;
}

// Pass 2's table: `stream` records of LF_BC_TAB doubles, `stream` slot pointers, the records of the steps stream ..
// mmax - 1 (lf_fill_product_tab), then min(m_j, stream) [K] and m_j [K] as ints.  h_tab comes zeroed.
template <int K, int NC>
static void lf_fill_pass2_tab(double* h_tab, const LfPlan& P, const hipeig_lanczos_basis* B, int k, const int* m,
                              const double* const* alphas, const double* const* betas, const double* const* G) {
  static_assert(sizeof(double*) == sizeof(double), "slot pointers are stored in the table's doubles");
  const double** h_slots = reinterpret_cast<const double**>(h_tab + P.o_slots);
  int* h_ms = reinterpret_cast<int*>(h_tab + P.o_m);
  int* h_m = h_ms + K;
  for (int i = 0; i < P.stream; ++i) h_slots[i] = lf_slot(B, i);
  for (int j = 0; j < K; ++j) {
    h_m[j] = j < k ? m[j] : 0;
    h_ms[j] = h_m[j] < P.stream ? h_m[j] : P.stream;
    for (int i = 0; i < h_ms[j]; ++i) {
      double* t = h_tab + (int64_t)i * LF_BC_TAB(K, NC);
      t[j] = 1.0 / betas[j][i];                              // LfCol::s, as lf_fill_product_tab
      for (int cc = 0; cc < NC; ++cc) t[K + j * NC + cc] = G[j][(size_t)i * NC + cc];
    }
  }
  if (P.recurs()) lf_fill_product_tab<K, NC>(h_tab + P.o_prod, P.stream, k, m, alphas, betas, G);
}

template <int K, int NC>
static int lf_pass2_impl(hipeig_ctx* c, hipeig_csr* A, const hipeig_lanczos_basis* B, int k, const double* const* b,
                         const int* m, const double* const* alphas, const double* const* betas, const double* const* G,
                         double* const* q, double* out_stats) {
  const int64_t n = A->nrows;
  const int64_t nb = ((n * K + 31) & ~(int64_t)31);
  const LfPlan P = lf_plan<K, NC>(B, k, m);
  if (P.mmax == 0) {
    for (int j = 0; j < k * NC; ++j) if (hipeig_vec_fill(c, q[j], n, 0.0)) return 1;
    return 0;
  }
  // the state record's area, the table, the recurrence's two work vectors - none from a whole basis, which may have left
  // no room for them - and the NC packed combinations
  const int64_t need = LF_HEAD_DOUBLES + P.tab_d + ((P.recurs() ? 2 : 0) + NC) * nb;
  HIPEIG_REQUIRE(need <= lf_tail_doubles(K, NC, P.mmax, nb), "tail workspace bound");
  if (lf_reserve(c, need)) return 1;
  double* d_tab = c->lf_ws + LF_HEAD_DOUBLES;
  double* Vb[2] = {d_tab + P.tab_d, d_tab + P.tab_d + nb};
  double* Q = d_tab + P.tab_d + (P.recurs() ? 2 * nb : 0);
  double* h_tab = (double*)calloc((size_t)P.tab_d, sizeof(double));
  HIPEIG_REQUIRE(h_tab != nullptr, "out of host memory");
  lf_fill_pass2_tab<K, NC>(h_tab, P, B, k, m, alphas, betas, G);
  hipError_t e = hipMemcpyAsync(d_tab, h_tab, (size_t)P.tab_d * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  free(h_tab);
  HIPEIG_CHECK(e);
  const int* d_ms = reinterpret_cast<const int*>(d_tab + P.o_m);
  const bool narrow = B && B->elem_bytes == 4;
  const double* const* d_slots = reinterpret_cast<const double* const*>(d_tab + P.o_slots);
  if (P.stream > 0 && !narrow)
    hipLaunchKernelGGL((lf_basis_combine_kernel<K, NC>), dim3(grid_stream(n * K)), dim3(HIPEIG_BLOCK), 0, c->stream,
                       n * (K / 2), P.stream, (const double*)d_tab, d_slots, d_ms, Q, nb);
  else if (P.stream > 0)
    hipLaunchKernelGGL((lf_basis_combine32_kernel<K, NC>), dim3(grid_stream(n * K / 2)), dim3(HIPEIG_BLOCK), 0, c->stream,
                       n * (K / 4), P.stream, (const double*)d_tab, d_slots, d_ms, Q, nb);
  else                                                        // no stream: the recurrence starts at step 0, r_{-1} = Q = 0
    HIPEIG_CHECK(hipMemsetAsync(Vb[1], 0, (size_t)nb * (1 + NC) * sizeof(double), c->stream));
  HIPEIG_CHECK(hipGetLastError());
  if (P.recurs()) {
    const int first = P.stream;
    if (narrow) {
      HIPEIG_REQUIRE(B->hand[0] && B->hand[1], "an fp32 prefix without its hand-over vectors");
    }
    if (B)
      HIPEIG_CHECK(hipMemcpyAsync(Vb[first & 1], narrow ? B->hand[0] : lf_slot(B, first), (size_t)nb * sizeof(double),
                                  hipMemcpyDeviceToDevice, c->stream));
    else if (hipeig_block_pack(c, K, n, k, b, Vb[0]))
      return 1;
    if (first)
      HIPEIG_CHECK(hipMemcpyAsync(Vb[(first + 1) & 1], narrow ? B->hand[1] : lf_slot(B, first - 1), (size_t)nb * sizeof(double),
                                  hipMemcpyDeviceToDevice, c->stream));
    if (lf_enqueue_products<K, NC>(c, A, d_tab + P.o_prod, d_ms + K, first, P.mmax, Vb, Q, nb)) return 1;
  }
  if (lf_unpack_combinations<K, NC>(c, n, k, Q, nb, q)) return 1;
  if (hipeig_sync_checked(c)) return 4;
  if (out_stats) out_stats[0] = P.products();
  return 0;
}

extern "C" int hipeig_lanczos_combine(hipeig_ctx* c, hipeig_csr* A, const hipeig_lanczos_basis* B, int k,
                                      const double* const* b, const int* m, const double* const* alphas,
                                      const double* const* betas, int nc, const double* const* G, double* const* q,
                                      double* out_stats) {
  HIPEIG_REQUIRE(A && (B || b) && m && alphas && betas && G && q, "null argument");
  HIPEIG_REQUIRE(!c->collectives, "the Lanczos filter runs on whole vectors (no row partition)");
  if (B) {
    HIPEIG_REQUIRE(k == B->k, "the basis was kept for another number of columns");
    HIPEIG_REQUIRE(nc == 1 || nc == 2 || nc == 4 || nc == 8, "1, 2, 4 or 8 combinations per column");
    HIPEIG_REQUIRE(A->nrows == A->ncols && A->nrows == B->nrows, "the operator is not the one the basis was kept for");
  } else {
    HIPEIG_REQUIRE(k >= 1 && k <= BCOO_KMAX, "1 to 8 right-hand sides per call");
    HIPEIG_REQUIRE(nc == 1 || nc == 2, "one or two combinations per column");
    HIPEIG_REQUIRE(A->nrows == A->ncols, "the Lanczos run needs a square operator");
  }
  for (int j = 0; j < k; ++j) {
    HIPEIG_REQUIRE(m[j] >= 0, "negative number of terms");
    HIPEIG_REQUIRE(!B || m[j] <= B->ran[j], "more terms than the steps the column ran");
    HIPEIG_REQUIRE((B || b[j] != nullptr) && (m[j] == 0 || (alphas[j] && betas[j] && G[j])), "null column argument");
    for (int cc = 0; cc < nc; ++cc)
      HIPEIG_REQUIRE(q[j * nc + cc] != nullptr && (B || q[j * nc + cc] != b[j]), B ? "q must not be null" : "q must not be null or alias b");
    HIPEIG_REQUIRE(m[j] == 0 || betas[j][0] > 0.0, B ? "a Lanczos vector past a breakdown was asked for" : "terms asked for a zero right-hand side");
    for (int i = 1; i < m[j]; ++i) HIPEIG_REQUIRE(betas[j][i] > 0.0, "a Lanczos vector past a breakdown was asked for");
  }
  if (out_stats) out_stats[0] = 0.0;
  if (A->nrows == 0) return 0;
  const int K = B ? B->K : lf_width(k);
#define LF_PASS2_CASE(KK, NN) \
  if (K == KK && nc == NN) return lf_pass2_impl<KK, NN>(c, A, B, k, b, m, alphas, betas, G, q, out_stats);
  LF_PASS2_CASE(4, 1) LF_PASS2_CASE(4, 2) LF_PASS2_CASE(4, 4) LF_PASS2_CASE(4, 8)
  LF_PASS2_CASE(8, 1) LF_PASS2_CASE(8, 2) LF_PASS2_CASE(8, 4) LF_PASS2_CASE(8, 8)
#undef LF_PASS2_CASE
  HIPEIG_REQUIRE(false, "unknown interleave width");
}

extern "C" int hipeig_lanczos_basis_info(hipeig_ctx* c, const hipeig_lanczos_basis* B, int64_t info[8]) {
  HIPEIG_REQUIRE(info != nullptr, "null argument");
  memset(info, 0, 8 * sizeof(int64_t));
  info[5] = c->lf_pool_bytes;
  if (!B) return 0;
  int top = 0;
  for (int j = 0; j < B->k; ++j) top = B->steps[j] > top ? B->steps[j] : top;
  info[0] = top;
  info[1] = (int64_t)B->nseg * (int64_t)B->seg_bytes + (B->hand[0] ? 2 * B->nb * (int64_t)sizeof(double) : 0);
  info[2] = B->K;
  info[3] = B->n;
  info[4] = B->k;
  info[6] = B->nseg;
  info[7] = B->seg_slots;
  return 0;
}

extern "C" int hipeig_lanczos_basis_element_bytes(hipeig_ctx* c, const hipeig_lanczos_basis* B, int* out) {
  HIPEIG_REQUIRE(out != nullptr, "null argument");
  *out = B ? B->elem_bytes : 0;
  return 0;
}

extern "C" int hipeig_lanczos_basis_release(hipeig_ctx* c, hipeig_lanczos_basis* B) {
  lf_basis_free(c, B);
  return 0;
}
