// Sparse operator: creation, layout preparation and the y = Hx / y = sign*(sigma*x - Hx)
// entry points.  Kernel bodies live in spmv_device.h.
#include <vector>
#include "sweep_launch.h"

static int build_tcoow_layout(hipeig_ctx* c, hipeig_csr* A, int pair);

// y[r] = a_self*xl[r] + a_sum*sum  (a_self = 0, a_sum = 1: plain product;
// a_self = sign*sigma, a_sum = -sign: the shifted operator of numpyVector.py:152/154).
// Two roundings like the reference's sigma*x - H@x (no contraction into an FMA).
struct AxpyEpilogue {
  double a_self, a_sum;
  const double* __restrict__ xl;
  double* __restrict__ y;
  __device__ __forceinline__ void row(int64_t r, double sum, double& acc) const {
    const double t = (a_self == 0.0) ? 0.0 : mul_rn(a_self, xl[r]);
    y[r] = add_rn(t, mul_rn(a_sum, sum));
  }
};

__global__ void __launch_bounds__(HIPEIG_BLOCK)
spmv_stream_kernel(CsrView A, const double* __restrict__ x, AxpyEpilogue epi) {
  __shared__ double prod[SPMV_NNZ_PER_BLOCK];
  double acc = 0.0;
  csr_stream_sweep(A, x, epi, acc, prod);
}

__global__ void __launch_bounds__(HIPEIG_BLOCK)
spmv_vector_kernel(CsrView A, const double* __restrict__ x, AxpyEpilogue epi) {
  double acc = 0.0;
  csr_vector_sweep(A, x, epi, acc);
}

__global__ void __launch_bounds__(HIPEIG_BLOCK)
spmv_tcoo_kernel(TcooView T, const double* __restrict__ x, AxpyEpilogue epi) {
  extern __shared__ double tcoo_lds[];
  double acc = 0.0;
  tcoo_sweep(T, x, epi, acc, tcoo_lds);
}

template <int FIXED>
__global__ void __launch_bounds__(TCOOW_THREADS)
spmv_tcoow_kernel(TcooView T, const double* __restrict__ x, AxpyEpilogue epi) {
  extern __shared__ double tcoo_lds[];
  __shared__ double red16[16];
  double acc = 0.0;
  tcoo_wg_sweep<AxpyEpilogue, FIXED>(T, x, epi, acc, tcoo_lds, red16);
}

__global__ void __launch_bounds__(HIPEIG_BLOCK)
spmv_dense_kernel(DenseView D, const double* __restrict__ x, AxpyEpilogue epi) {
  double acc = 0.0;
  dense_row_sweep(D, x, epi, acc);
}

// Complex operand, real operator, complex shift (the contour solves of feast.py:83-90 through GCROT): with
// x = xr + i xi and z = zr + i zi,  y = sign*(z*x - H x):
//   yr = sign*(zr*xr - H xr) - sign*zi*xi,   yi = sign*(zr*xi - H xi) + sign*zi*xr.
// ar = sign*zr, ai = sign*zi, as = -sign (ar = ai = 0, as = 1: the plain product).  The real part of the
// shift and the operator sum are rounded separately, like the reference's sigma*x - H@x.
struct PairEpilogue {
  double ar, ai, as;
  const double* __restrict__ xr;
  const double* __restrict__ xi;
  double* __restrict__ yr;
  double* __restrict__ yi;
  __device__ __forceinline__ void row2(int64_t r, double sr, double si, double& acc) const {
    const double vr = xr[r], vi = xi[r];
    const double tr = add_rn(mul_rn(ar, vr), mul_rn(as, sr));
    const double ti = add_rn(mul_rn(ar, vi), mul_rn(as, si));
    yr[r] = fma(-ai, vi, tr);
    yi[r] = fma(ai, vr, ti);
  }
};

__global__ void __launch_bounds__(TCOOW_THREADS)
spmv_tcoow_pair_kernel(TcooView T, const double* __restrict__ xpair, PairEpilogue epi) {
  extern __shared__ double tcoo_lds[];
  double acc = 0.0;
  tcoo_wg_sweep<PairEpilogue, 0, 1>(T, xpair, epi, acc, tcoo_lds, nullptr);
}

// xp[i] = (xr[i], xi[i]): the interleaved operand of the pair sweep
__global__ void __launch_bounds__(HIPEIG_BLOCK)
pair_pack_kernel(int64_t n, const double* __restrict__ xr, const double* __restrict__ xi, double2* __restrict__ xp) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) xp[i] = make_double2(xr[i], xi[i]);
}

__global__ void __launch_bounds__(HIPEIG_BLOCK) absmax_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ partials) {
  __shared__ double lds[16];
  double m = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double v = fabs(x[i]);
    m = (v > m || v != v) ? v : m;                     // NaN sticks
  }
  m = block_max_all(m, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

// max_i sum_j |a_ij| over the local rows (one wavefront per row), as per-workgroup maxima
__global__ void __launch_bounds__(HIPEIG_BLOCK)
rowabs_max_kernel(const int32_t* __restrict__ rowptr, const double* __restrict__ val, int64_t nrows, double* __restrict__ partials) {
  __shared__ double lds[16];
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  double m = 0.0;
  for (int64_t r = wave; r < nrows; r += nwaves) {
    double a = 0.0;
    for (int p = rowptr[r] + lane; p < rowptr[r + 1]; p += 64) a += fabs(val[p]);
    a = wave_reduce_sum(a);
    a = __shfl(a, 0, 64);
    m = fmax(m, a);
  }
  m = block_max_all(m, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

// The same over the gathered operand of a row-partitioned operator: only positions that hold an operand entry count.
// The scalar slots behind the last chunk do not (MINRES leaves its share of <y,y> there before every exchange), nor do
// the tails of a (rank, chunk) piece beyond the rank's rows: no exchange of this operator writes them, and the buffer is
// the context's, so an earlier operator's operand may still lie there.  A maximum is exact: the same bits on every rank.
__global__ void __launch_bounds__(HIPEIG_BLOCK) absmax_gathered_kernel(const double* __restrict__ x, GatherLayout gl, RankRows rows,
                                                                       double* __restrict__ partials) {
  __shared__ double lds[16];
  double m = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = gl.total();
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
    int k = 0;
    while (k + 1 < gl.nchunks && p >= gl.cbase[k + 1]) ++k;
    const int64_t q = p - gl.cbase[k], cs = gl.cstride(k);
    const int r = (int)(q / cs);
    const int64_t i = q - (int64_t)r * cs;                // offset inside the piece of (rank r, chunk k)
    if (i >= gl.h || (int64_t)k * gl.h + i >= rows.n[r]) continue;
    const double v = fabs(x[p]);
    m = (v > m || v != v) ? v : m;                     // NaN sticks
  }
  m = block_max_all(m, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

// Operand maximum for the fixed-point sweep: per-workgroup maxima into the context's fx area.
#define HIPEIG_FX_AREA (4 * HIPEIG_WIDE_PARTIALS)      // behind the three partial-sum areas of the MINRES kernels
int hipeig_fixed_prepare(hipeig_ctx* c, const hipeig_csr* A, const double* xg, TcooView* t) {
  const int g = grid_for(A->gather_len, 8);
  double* area = c->d_partials + HIPEIG_FX_AREA;
  if (A->col_stride > 0)
    hipLaunchKernelGGL(absmax_gathered_kernel, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, xg, A->gl, A->rank_rows, area);
  else
    hipLaunchKernelGGL(absmax_kernel, dim3(g), dim3(HIPEIG_BLOCK), 0, c->stream, xg, A->gather_len, area);
  t->fx_xmax = area; t->fx_count = g; t->fx_bound = A->absrow_max;
  return 0;
}

__global__ void __launch_bounds__(HIPEIG_BLOCK)
spmv_tcoow_combine_kernel(const double* __restrict__ parts, int nparts, int64_t stride, int64_t nrows, AxpyEpilogue epi) {
  double acc = 0.0;
  tcoow_combine_sweep(parts, nparts, stride, nrows, epi, acc);
}

// sweep_launch's callback for the product kernels: the one place that names them, for hipeig_spmv, hipeig_spmv_shift and the
// raw launches of a TCOO-W plan.  They keep a name per layout (bench.py and the committed counter pass look them up by it).
static auto spmv_launcher(hipeig_ctx* c, const SweepPlan& p, const AxpyEpilogue& epi) {
  const CsrView view = p.view;
  const DenseView dview = p.dview;
  return [=](auto v, auto f, int grid, int threads, size_t lds, const TcooView& tv, const double* xg, int) {
    constexpr int V = decltype(v)::value;
    const dim3 g(grid), t(threads);
    if constexpr (V == 6) hipLaunchKernelGGL(spmv_dense_kernel, g, t, lds, c->stream, dview, xg, epi);
    else if constexpr (V == 5) hipLaunchKernelGGL(spmv_tcoow_combine_kernel, g, t, lds, c->stream, tv.raw_out, tv.part_base, tv.part_stride, tv.nrows, epi);
    else if constexpr (V == 4) hipLaunchKernelGGL(spmv_tcoow_kernel<decltype(f)::value>, g, t, lds, c->stream, tv, xg, epi);
    else if constexpr (V == 3) hipLaunchKernelGGL(spmv_tcoo_kernel, g, t, lds, c->stream, tv, xg, epi);
    else if constexpr (V == 2) hipLaunchKernelGGL(spmv_stream_kernel, g, t, lds, c->stream, view, xg, epi);
    else hipLaunchKernelGGL(spmv_vector_kernel, g, t, lds, c->stream, view, xg, epi);
  };
}

// Device view of a TCOO-family copy: TCOO (A->t), TCOO-W (A->w) or the pair copy of TCOO-W (A->p)
TcooView hipeig_tcoo_view(const hipeig_csr* A, const BlockedLayout& L) {
  TcooView t;
  t.idx = L.idx; t.val = L.val; t.off = L.off;
  t.nunits = L.nunits; t.nwin = L.nwin; t.wbits = L.wbits; t.rw = L.rw;
  t.unit_begin = 0;
  t.prefetch = (&L == &A->t) ? A->t_prefetch : 0;
  t.ablate = 0;
  if (const char* e = getenv("HIPEIG_TCOO_ABLATE")) t.ablate = atoi(e);   // timing experiments (wrong results)
  t.nrows = A->nrows;
  t.gather_len = A->gather_len;
  t.nrun = 0; t.yinit = nullptr; t.raw_out = nullptr;
  t.csplit = 1; t.part_base = 0; t.part_stride = 0;
  t.fx_xmax = nullptr; t.fx_count = 0; t.fx_bound = 0.0;
  return t;
}

CsrView hipeig_csr_view(const hipeig_csr* A) {
  CsrView v;
  v.rowptr = A->d_rowptr;
  v.col = A->d_col;
  v.val = A->d_val;
  v.row_blocks = A->d_row_blocks;
  v.n_row_blocks = A->n_row_blocks;
  v.nrows = A->nrows;
  v.group = A->lanes_per_row;
  return v;
}

// Workgroups per launch and sweep launches of one product with `variant` (4 stands for 5 too)
SweepGrid hipeig_sweep_grid(const hipeig_csr* A, int variant) {
  if (variant == 6) return SweepGrid{hipeig_dense_grid(A, DENSE_ROWS_PER_WAVE * (HIPEIG_BLOCK / HIPEIG_WAVE)), 1};
  if (variant == 4 || variant == 5) return blocked_grid(A->w);
  if (variant == 3) return blocked_grid(A->t, 4);
  int64_t g = A->n_row_blocks;
  if (variant == 1) {
    const int64_t groups_per_block = HIPEIG_BLOCK / A->lanes_per_row;
    g = (A->nrows + groups_per_block - 1) / groups_per_block;
  }
  if (g < 1) g = 1;
  if (g > HIPEIG_MAX_PARTIALS) g = HIPEIG_MAX_PARTIALS;
  return SweepGrid{(int)g, 1};
}

// Partial-sum slabs of the split / overlapped sweeps (context buffer, grown on demand).
static int tcoow_ensure_parts(hipeig_ctx* c, int64_t doubles) {
  if (c->ytmp_n >= doubles) return 0;
  if (c->ytmp) { if (hipFree(c->ytmp) != hipSuccess) return -1; }
  c->ytmp = nullptr; c->ytmp_n = 0;
  if (hipMalloc((void**)&c->ytmp, (size_t)doubles * sizeof(double)) != hipSuccess) {
    hipeig_set_error("out of device memory for the partial-sum slabs");
    return -1;
  }
  c->ytmp_n = doubles;
  return 0;
}

int64_t hipeig_tcoow_part_stride(const hipeig_csr* A) { return (A->nrows + 63) & ~(int64_t)63; }

// The column windows of a partitioned TCOO-W operator by what they need:
// set 0 - windows that lie entirely inside this rank's own column ranges (one range per chunk of the gathered layout):
//         they can be swept as soon as the slice has been copied into the gathered buffer, while the exchange runs;
// set 1 + k - the other windows whose last column belongs to chunk k: complete once chunk k has arrived.
// Every set is at most two runs of consecutive windows (a chunk's windows minus the local run inside them).
struct WindowSets {
  int nset;                        // 1 + nchunks
  int nrun[1 + HIPEIG_GATHER_MAX_CHUNKS];
  int lo[1 + HIPEIG_GATHER_MAX_CHUNKS][4], hi[1 + HIPEIG_GATHER_MAX_CHUNKS][4];
};

static void tcoow_window_sets(const hipeig_ctx* c, const hipeig_csr* A, WindowSets* ws) {
  const GatherLayout& gl = A->gl;
  const int wb = A->w.wbits, nwin = A->w.nwin;
  const int64_t W = (int64_t)1 << wb;
  memset(ws, 0, sizeof(*ws));
  ws->nset = 1 + gl.nchunks;
  int prev_end = 0;                                   // first window not yet given to a chunk
  for (int k = 0; k < gl.nchunks; ++k) {
    // windows whose last position lies in chunk k: [prev_end, wend)
    int wend = (k == gl.nchunks - 1) ? nwin : (int)(gl.cbase[k + 1] >> wb);      // window holding cbase[k+1] straddles: it waits for k+1
    if (wend > nwin) wend = nwin;
    if (wend < prev_end) wend = prev_end;
    // own range inside chunk k, and the windows entirely inside it
    const int64_t rows_lo = (int64_t)k * gl.h;
    int64_t rows = A->nrows - rows_lo;
    if (rows > gl.h) rows = gl.h;
    int l0 = 0, l1 = 0;
    if (rows > 0) {
      const int64_t p0 = gl.cbase[k] + (int64_t)c->rank * gl.cstride(k), p1 = p0 + rows;
      l0 = (int)((p0 + W - 1) >> wb); l1 = (int)(p1 >> wb);
      if (l0 < prev_end) l0 = prev_end;
      if (l1 > wend) l1 = wend;
      if (l1 < l0) l1 = l0;
    }
    if (l1 > l0) {
      const int q = ws->nrun[0]++;
      ws->lo[0][q] = l0; ws->hi[0][q] = l1;
      if (l0 > prev_end) { const int r = ws->nrun[1 + k]++; ws->lo[1 + k][r] = prev_end; ws->hi[1 + k][r] = l0; }
      if (wend > l1) { const int r = ws->nrun[1 + k]++; ws->lo[1 + k][r] = l1; ws->hi[1 + k][r] = wend; }
    } else if (wend > prev_end) {
      const int r = ws->nrun[1 + k]++; ws->lo[1 + k][r] = prev_end; ws->hi[1 + k][r] = wend;
    }
    prev_end = wend;
  }
}

// Allocate the slabs one product of A can need, so that no allocation happens later (a hipGraph
// capture must not allocate).
int hipeig_tcoow_reserve(hipeig_ctx* c, const hipeig_csr* A) {
  if (!A->w.idx) return 0;
  const int64_t stride = hipeig_tcoow_part_stride(A);
  const int nl = c->collectives ? 1 + A->gl.nchunks : 1;
  const int64_t need = (A->w.csplit > 1) ? (int64_t)nl * A->w.csplit * stride : (c->collectives ? A->nrows : 0);
  return need > 0 ? tcoow_ensure_parts(c, need) : 0;
}

// Everything one TCOO-W product does before its epilogue-bearing launch, as a list of sweep launches:
//   launch i covers the windows of tv[i]; wait[i] >= 0: the compute stream must first wait for that chunk of the
//   operand exchange (hipeig_allgather_x_wait_chunk).
// Without a communicator (or without the overlap) that is ONE launch over all windows after a plain exchange.  With it,
// the exchange is started first and the launches are: this rank's own windows (under the exchange), then per chunk the
// windows that chunk completes.  Accumulators: with column splits every launch stores its own raw
// slabs (part_base = launch * csplit) and *ncombine > 0 tells the caller to add that many slabs in a combine kernel
// that carries the epilogue; without, the launches hand their sums on through ctx->ytmp (raw_out -> yinit) and the
// LAST launch carries the epilogue.
struct TcoowPlan {
  int nlaunch;
  TcooView tv[2 + HIPEIG_GATHER_MAX_CHUNKS];
  int wait[2 + HIPEIG_GATHER_MAX_CHUNKS];
  int ncombine;
  const double* xg;
  bool overlapped;
};

int hipeig_tcoow_plan(hipeig_ctx* c, hipeig_csr* A, const double* x_local, TcoowPlan* P) {
  const int cs = A->w.csplit;
  const int64_t stride = hipeig_tcoow_part_stride(A);
  P->nlaunch = 0; P->ncombine = 0; P->xg = nullptr; P->overlapped = false;
  WindowSets ws;
  bool split_sets = c->collectives && c->overlap && A->w.idx && A->col_stride > 0 && A->last_variant != 5;   // the fixed-point form needs max|x| of the whole operand first
  if (split_sets) {
    tcoow_window_sets(c, A, &ws);
    int nonempty = 0;
    for (int q = 0; q < ws.nset; ++q) nonempty += ws.nrun[q] > 0;
    if (ws.nrun[0] == 0 && A->gl.nchunks == 1) split_sets = false;        // nothing to hide the exchange behind
    if (nonempty <= 1 && ws.nrun[0] == 0) split_sets = false;
  }
  if (!split_sets) {
    if (hipeig_allgather_x(c, A->gl, x_local, A->nrows, &P->xg)) return 4;
    TcooView t = hipeig_tcoo_view(A, A->w);
    if (cs > 1) {
      if (tcoow_ensure_parts(c, cs * stride)) return 4;
      t.csplit = cs; t.part_base = 0; t.part_stride = stride; t.raw_out = c->ytmp;
      P->ncombine = cs;
    }
    P->tv[0] = t; P->wait[0] = -1; P->nlaunch = 1;
    return 0;
  }
  int nl = 0;
  for (int q = 0; q < ws.nset; ++q) nl += ws.nrun[q] > 0;
  if (tcoow_ensure_parts(c, cs > 1 ? (int64_t)nl * cs * stride : A->nrows)) return 4;
  if (hipeig_allgather_x_begin(c, A->gl, x_local, A->nrows)) return 4;
  P->overlapped = true;
  int li = 0;
  for (int q = 0; q < ws.nset; ++q) {
    if (ws.nrun[q] == 0) continue;
    TcooView t = hipeig_tcoo_view(A, A->w);
    t.nrun = ws.nrun[q];
    for (int r = 0; r < ws.nrun[q]; ++r) { t.run_lo[r] = ws.lo[q][r]; t.run_hi[r] = ws.hi[q][r]; }
    t.csplit = cs; t.part_stride = stride;
    if (cs > 1) { t.yinit = nullptr; t.raw_out = c->ytmp; t.part_base = li * cs; }
    else {
      t.part_base = 0;
      t.yinit = (li > 0) ? c->ytmp : nullptr;
      t.raw_out = (li + 1 < nl) ? c->ytmp : nullptr;
    }
    P->tv[li] = t;
    P->wait[li] = (q == 0) ? -1 : q - 1;
    ++li;
  }
  P->nlaunch = nl;
  P->ncombine = (cs > 1) ? nl * cs : 0;
  // a set without windows still has to be waited for by the launch that follows it; the last launch waits for the
  // last chunk in any case (it - or the combine kernel behind it - may read the scalar slots riding on that chunk)
  P->wait[nl - 1] = A->gl.nchunks - 1;
  P->xg = nullptr;                                           // set by the caller after the first wait: hipeig_gathered()
  return 0;
}

// Runs every launch of the plan that carries no epilogue (the product kernel with the empty one) and leaves in *o what
// the caller's own kernel still has to do: the last view's launches when o->has_last, else the combine launch over
// o->ncombine slabs in ctx->ytmp; o->xg is the operand.
int hipeig_tcoow_run_plan(hipeig_ctx* c, hipeig_csr* A, const SweepPlan& p, const double* x_local, SweepOperand* o) {
  TcoowPlan P;
  if (hipeig_tcoow_plan(c, A, x_local, &P)) return 4;
  o->xg = P.overlapped ? hipeig_gathered(c) : P.xg;
  const int nraw = P.ncombine ? P.nlaunch : P.nlaunch - 1;
  if (p.fixed) {                                            // never overlapped (hipeig_tcoow_plan): max|x| of the whole operand first
    HIPEIG_REQUIRE(!P.overlapped && P.nlaunch == 1, "the fixed-point sweep takes the plain exchange");
    if (hipeig_fixed_prepare(c, A, o->xg, &P.tv[0])) return 4;
  }
  const auto raw = spmv_launcher(c, p, AxpyEpilogue{0.0, 0.0, nullptr, nullptr});
  bool marked = false;
  for (int i = 0; i < P.nlaunch; ++i) {
    if (P.wait[i] >= 0) {
      if (hipeig_allgather_x_wait_chunk(c, A->gl, P.wait[i])) return 4;
      if (P.overlapped && !marked) { hipeig_phase_mark(c, 2); marked = true; }
    }
    if (i < nraw) {
      sweep_launch(c, p, SweepOperand{o->xg, P.tv[i], true, 0}, raw);
      if (P.overlapped && i == 0) hipeig_phase_mark(c, 1);
    }
  }
  if (hipGetLastError() != hipSuccess) { hipeig_set_error("sweep launch failed"); return 4; }
  o->has_last = (P.ncombine == 0);
  o->tv = P.tv[P.nlaunch - 1];
  o->ncombine = P.ncombine;
  return 0;
}

static int launch_spmv(hipeig_ctx* c, hipeig_csr* A, double a_self, double a_sum,
                       const double* x, double* y) {
  if (A->nrows == 0) return 0;
  SweepPlan plan;
  // combine launch of a column-split sweep: here a two-stream update, two rows per thread (the solvers' carries their epilogue)
  if (const int rc = sweep_plan_build(c, A, grid_for(A->nrows, 2), &plan)) return rc;
  SweepOperand op;
  if (sweep_prepare(c, A, plan, x, &op)) return 4;
  // shift term: x restricted to this operator's rows.  Partitioned run: x IS that slice; a row
  // slab applied to a full-length operand (single process): the slice starts at row_offset.
  const AxpyEpilogue epi{a_self, a_sum, c->collectives ? x : x + A->row_offset, y};
  sweep_launch(c, plan, op, spmv_launcher(c, plan, epi));
  HIPEIG_CHECK(hipGetLastError());
  hipeig_phase_mark(c, 3);
  return 0;
}

// One sweep for both halves of a complex operand (see PairEpilogue).  Taken for operators the automatic choice
// gives the TCOO-W kernel to (variant 4) on an unpartitioned context; everything else - small operators, pinned or
// reproducible variants, row-partitioned runs - runs the two real sweeps and the two updates the pair replaces.
static int launch_spmv_pair(hipeig_ctx* c, hipeig_csr* A, double zr, double zi, double sign,
                            const double* xr, const double* xi, double* yr, double* yi) {
  if (A->nrows == 0) return 0;
  const double ar = sign * zr, ai = sign * zi, as = (sign == 0.0) ? 1.0 : -sign;
  int variant = hipeig_csr_pick_variant(c, A);
  if (variant < 0) return 1;
  A->last_pair_fused = 0;
  // Measured (tools/pair_bench.py, 64 non-zeros per row): N = 1e6 (32 per row) 0.227 -> 0.187 ms, 2e6 0.68 -> 0.50 ms,
  // 4e6 1.38 -> 1.49 ms, 6e6 2.46 -> 2.45 ms, 8e6 3.29 -> 3.55 ms, 1e7 4.2 -> 4.7 ms (window / bin sizes change
  // nothing): with two accumulators per row a unit holds half the rows, and once the rows no longer fit ONE launch
  // the 16-byte gathers of the sparser tiles cost more line fills than the second pass over the stream saves.
  const char* env = getenv("HIPEIG_PAIR_SWEEP");                     // 0 = always two sweeps, 1 = always the pair sweep
  const bool one_launch = A->nrows <= (int64_t)c->num_cu * (TCOOW_MAX_RW / 2);
  const bool want = variant == 4 && !c->collectives && (env ? atoi(env) != 0 : one_launch);
  if (want) {
    const int rc = build_tcoow_layout(c, A, 1);
    if (rc == 1) return 1;
    if (rc == 0 && !tcoow_ensure_parts(c, 2 * A->gather_len)) {
      double* xp = c->ytmp;
      hipLaunchKernelGGL(pair_pack_kernel, dim3(grid_stream(2 * A->gather_len)), dim3(HIPEIG_BLOCK), 0, c->stream,
                         A->gather_len, xr, xi, reinterpret_cast<double2*>(xp));
      TcooView t = hipeig_tcoo_view(A, A->p);
      PairEpilogue epi{ar, ai, as, xr + A->row_offset, xi + A->row_offset, yr, yi};
      const SweepGrid g = blocked_grid(A->p);
      for (int i = 0; i < g.launches; ++i) {                            // one launch per sweep
        t.unit_begin = i * g.wgs;
        hipLaunchKernelGGL(spmv_tcoow_pair_kernel, dim3(g.wgs), dim3(TCOOW_THREADS), blocked_lds_bytes(A->p, 2), c->stream, t, xp, epi);
      }
      HIPEIG_CHECK(hipGetLastError());
      A->last_pair_fused = 1;
      return 0;
    }
  }
  const double a_self = (sign == 0.0) ? 0.0 : ar;
  if (launch_spmv(c, A, a_self, as, xr, yr)) return 1;
  if (launch_spmv(c, A, a_self, as, xi, yi)) return 1;
  if (ai != 0.0) {
    const int64_t o = c->collectives ? 0 : A->row_offset;
    if (hipeig_axpby(c, A->nrows, -ai, xi + o, 1.0, yr)) return 1;
    if (hipeig_axpby(c, A->nrows, ai, xr + o, 1.0, yi)) return 1;
  }
  return 0;
}

extern "C" int hipeig_spmv_shift_pair(hipeig_ctx* c, hipeig_csr* A, double zr, double zi, double sign,
                                      const double* xr, const double* xi, double* yr, double* yi) {
  HIPEIG_REQUIRE(xr != yr && xr != yi && xi != yr && xi != yi && yr != yi, "in-place product is not supported");
  HIPEIG_REQUIRE(sign == 1.0 || sign == -1.0 || sign == 0.0, "sign must be +1, -1 or 0 (plain product)");
  return launch_spmv_pair(c, A, zr, zi, sign, xr, xi, yr, yi);
}

extern "C" int hipeig_csr_pair_info(hipeig_csr* A, int64_t out[2]) {
  out[0] = A->last_pair_fused;
  out[1] = 0;
  if (A->last_pair_fused && A->p.nunits > 0) out[1] = blocked_grid(A->p).launches;
  return 0;
}

extern "C" int hipeig_spmv(hipeig_ctx* c, hipeig_csr* A, const double* x, double* y) {
  HIPEIG_REQUIRE(x != y, "in-place product is not supported");
  return launch_spmv(c, A, 0.0, 1.0, x, y);
}

extern "C" int hipeig_spmv_shift(hipeig_ctx* c, hipeig_csr* A, double sigma, double sign,
                                 const double* x, double* y) {
  HIPEIG_REQUIRE(x != y, "in-place product is not supported");
  HIPEIG_REQUIRE(sign == 1.0 || sign == -1.0, "sign must be +1 or -1");
  return launch_spmv(c, A, sign * sigma, -sign, x, y);
}

// ---- TCOO construction -------------------------------------------------------------------
// One workgroup per unit (RW consecutive rows), rows handled in chunks of 256 (one row per
// thread).  count pass: non-zeros per (unit, window).  fill pass: a non-zero of row r and
// window c goes to  off[unit][c] + (#nnz of window c in earlier rows of the unit) + (#earlier
// nnz of window c in row r): row-major order inside every tile, independent of scheduling.

__global__ void __launch_bounds__(256)
tcoo_build_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                  const double* __restrict__ val, int64_t nrows, int rw, int nwin, int wbits,
                  uint32_t* __restrict__ counts /* [nunits][nwin], count pass */,
                  const uint32_t* __restrict__ off /* fill pass */, uint32_t* __restrict__ idx_out,
                  double* __restrict__ val_out, int fill) {
  extern __shared__ uint32_t tb_lds[];               // cnt[256][nwin] then base[nwin]
  uint32_t* cnt = tb_lds;
  uint32_t* base = tb_lds + 256 * nwin;
  const int u = blockIdx.x, t = threadIdx.x;
  for (int c = t; c < nwin; c += 256) base[c] = fill ? off[(size_t)u * nwin + c] : 0u;
  const int64_t row0 = (int64_t)u * rw;
  for (int chunk = 0; chunk < rw; chunk += 256) {
    const int64_t r = row0 + chunk + t;
    const bool live = (chunk + t < rw) && (r < nrows);
    for (int c = 0; c < nwin; ++c) cnt[t * nwin + c] = 0;
    int s = 0, e = 0;
    if (live) {
      s = rowptr[r]; e = rowptr[r + 1];
      for (int p = s; p < e; ++p) cnt[t * nwin + (col[p] >> wbits)] += 1;
    }
    __syncthreads();
    // column-wise exclusive scan over the 256 rows of the chunk (thread c scans window c)
    for (int c = t; c < nwin; c += 256) {
      uint32_t run = base[c];
      for (int k = 0; k < 256; ++k) {
        const uint32_t v = cnt[k * nwin + c];
        cnt[k * nwin + c] = run;
        run += v;
      }
      base[c] = run;
    }
    __syncthreads();
    if (fill && live) {
      const uint32_t rl = (uint32_t)(chunk + t);
      for (int p = s; p < e; ++p) {
        const int cc = col[p];
        const int c = cc >> wbits;
        const uint32_t dst = cnt[t * nwin + c]++;
        idx_out[dst] = (rl << wbits) | ((uint32_t)cc & ((1u << wbits) - 1u));
        val_out[dst] = val[p];
      }
    }
    __syncthreads();
  }
  if (!fill)
    for (int c = t; c < nwin; c += 256) counts[(size_t)u * nwin + c] = base[c];
}

size_t hipeig_tcoo_lds_bytes(const hipeig_csr* A) { return (size_t)4 * A->t.rw * sizeof(double); }

// Build the column-window blocked copy (idempotent).  Returns 0 on success, 1 on failure,
// 2 if the operator does not suit the layout (caller falls back to the CSR-stream kernel).
int hipeig_csr_build_tcoo(hipeig_ctx* c, hipeig_csr* A) {
  if (A->t.idx) return 0;
  if (A->nnz == 0 || A->nrows == 0) return 2;
  int wbits = TCOO_MAX_WBITS;
  if (const char* e = getenv("HIPEIG_TCOO_WBITS")) wbits = atoi(e);          // tuning knob
  HIPEIG_REQUIRE(wbits >= 10 && wbits <= 22, "HIPEIG_TCOO_WBITS out of range");
  while (wbits > 10 && ((int64_t)1 << (wbits - 1)) >= A->gather_len) --wbits;   // one window if x is short
  const int nwin = (int)((A->gather_len + ((int64_t)1 << wbits) - 1) >> wbits);
  if (nwin > TCOO_MAX_WIN) return 2;
  // rows per wave: fill 2 workgroups x 4 waves per CU, at most TCOO_MAX_RW (20 KiB LDS per wave)
  int64_t rw = (A->nrows + (int64_t)c->num_cu * 8 - 1) / ((int64_t)c->num_cu * 8);
  rw = (rw + 63) / 64 * 64;
  if (rw < 64) rw = 64;
  if (rw > TCOO_MAX_RW) rw = TCOO_MAX_RW;
  if (const char* e = getenv("HIPEIG_TCOO_RW")) rw = (atoi(e) + 63) / 64 * 64;   // tuning knob
  HIPEIG_REQUIRE(rw >= 64 && rw * 32 <= 163840, "HIPEIG_TCOO_RW out of range");
  // (row_in_unit << wbits | col_in_window) must stay below 0xFFFFFFFF, the sweep's mark for "no entry": rw < 2^(32 - wbits),
  // as spmm.hip keeps it for the block layout.  One step of 64 below, not 1: rw stays a multiple of 64, as the automatic
  // choice and the knob round it (neither tcoo_build_kernel nor tcoo_sweep needs that; every wave's accumulators then
  // start on a 512-byte boundary of the LDS).
  if (rw >= ((int64_t)1 << (32 - wbits))) rw = ((int64_t)1 << (32 - wbits)) - 64;
  int per_cu = (int)(163840 / ((size_t)4 * rw * sizeof(double)));             // LDS-limited residency
  if (per_cu > 8) per_cu = 8;
  if (per_cu < 1) per_cu = 1;
  if (const char* e = getenv("HIPEIG_TCOO_WG_PER_CU")) per_cu = atoi(e);      // tuning knob
  HIPEIG_REQUIRE(per_cu >= 1 && per_cu <= 8, "HIPEIG_TCOO_WG_PER_CU out of range");
  BlockedLayout L{};
  L.nunits = (int)((A->nrows + rw - 1) / rw); L.nwin = nwin; L.wbits = wbits; L.rw = (int)rw;
  L.wgs_per_sweep = per_cu * c->num_cu; L.csplit = 1; L.slots = A->nnz;
  const size_t ntile = (size_t)L.nunits * nwin;
  const size_t lds = ((size_t)256 * nwin + nwin) * sizeof(uint32_t);
  uint32_t* d_counts = nullptr;
  auto build = [&]() -> int {
    HIPEIG_CHECK(hipMalloc((void**)&d_counts, ntile * sizeof(uint32_t)));
    HIPEIG_CHECK(hipFuncSetAttribute((const void*)tcoo_build_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(((size_t)256 * TCOO_MAX_WIN + TCOO_MAX_WIN) * sizeof(uint32_t))));
    hipLaunchKernelGGL(tcoo_build_kernel, dim3(L.nunits), dim3(256), lds, c->stream, A->d_rowptr, A->d_col, A->d_val,
                       A->nrows, L.rw, nwin, wbits, d_counts, (const uint32_t*)nullptr, (uint32_t*)nullptr, (double*)nullptr, 0);
    HIPEIG_CHECK(hipGetLastError());
    std::vector<uint32_t> off(ntile + 1);
    HIPEIG_CHECK(hipMemcpyAsync(off.data() + 1, d_counts, ntile * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPEIG_CHECK(hipStreamSynchronize(c->stream));
    off[0] = 0;
    uint64_t run = 0;
    for (size_t i = 1; i <= ntile; ++i) { run += off[i]; off[i] = (uint32_t)run; }
    HIPEIG_REQUIRE(run == (uint64_t)A->nnz, "TCOO count pass lost non-zeros");
    HIPEIG_CHECK(hipMalloc((void**)&L.off, (ntile + 1) * sizeof(uint32_t)));
    HIPEIG_CHECK(hipMalloc((void**)&L.idx, (size_t)A->nnz * sizeof(uint32_t)));
    HIPEIG_CHECK(hipMalloc((void**)&L.val, (size_t)A->nnz * sizeof(double)));
    HIPEIG_CHECK(hipMemcpyAsync(L.off, off.data(), (ntile + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(tcoo_build_kernel, dim3(L.nunits), dim3(256), lds, c->stream, A->d_rowptr, A->d_col, A->d_val,
                       A->nrows, L.rw, nwin, wbits, (uint32_t*)nullptr, (const uint32_t*)L.off, L.idx, L.val, 1);
    HIPEIG_CHECK(hipGetLastError());
    HIPEIG_CHECK(hipStreamSynchronize(c->stream));
    HIPEIG_CHECK(hipFuncSetAttribute((const void*)spmv_tcoo_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)HIPEIG_TCOO_LDS_MAX));   // the largest any operator may ask for
    return 0;
  };
  const int rc = build();
  if (d_counts) hipFree(d_counts);
  if (rc) { hipeig_free_layout(&L); return rc; }
  A->t = L;
  A->t_prefetch = 0;
  if (const char* e = getenv("HIPEIG_TCOO_PREFETCH")) A->t_prefetch = atoi(e) != 0;   // tuning knob
  A->bytes += (int64_t)A->nnz * 12 + (int64_t)(ntile + 1) * 4;
  return 0;
}

// ---- binned copies: TCOO-W, its pair copy, TCOO-B ----------------------------------------------
// Bucketing by (unit, column bin) with global counters: count, scan on the host, scatter.
// Which slot of its bin a non-zero lands in depends on scheduling; the SET of non-zeros of
// every bin does not, and the sweeps' accumulation order is unordered anyway.
// LANE_MAJOR: slots are stored lane-major inside their 256-slot batch (TCOO-W, tcoow_islot / tcoow_vslot).
template <int LANE_MAJOR>
__global__ void __launch_bounds__(256)
bin_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
           const double* __restrict__ val, int64_t nrows, int rw, int binbits, int nbins, int wbits,
           uint32_t* __restrict__ cursor, uint32_t* __restrict__ idx_out, double* __restrict__ val_out, int fill) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const uint32_t wmask = (1u << wbits) - 1u;
  for (int64_t r = wave; r < nrows; r += nwaves) {
    const int64_t unit = r / rw;
    const uint32_t rl = (uint32_t)(r - unit * rw);
    uint32_t* cur = cursor + unit * nbins;
    const int s = rowptr[r], e = rowptr[r + 1];
    for (int p = s + lane; p < e; p += 64) {
      const uint32_t cc = (uint32_t)col[p];
      const uint32_t slot = atomicAdd(cur + (cc >> binbits), 1u);
      if (fill) {
        idx_out[LANE_MAJOR ? tcoow_islot(slot) : slot] = (rl << wbits) | (cc & wmask);
        val_out[LANE_MAJOR ? tcoow_vslot(slot) : slot] = val[p];
      }
    }
  }
}

void hipeig_free_layout(BlockedLayout* L) {
  if (L->idx) hipFree(L->idx);
  if (L->val) hipFree(L->val);
  if (L->off) hipFree(L->off);
  L->idx = nullptr; L->val = nullptr; L->off = nullptr;
}

int hipeig_build_binned(hipeig_ctx* c, hipeig_csr* A, const BlockedLayout& geom, unsigned policy, BlockedLayout* out) {
  const int bpw = 1 << (geom.wbits - geom.binbits);    // bins per window
  const int64_t nbins = (int64_t)geom.nwin * bpw;
  const size_t ntile = (size_t)geom.nunits * geom.nwin, ncnt = (size_t)geom.nunits * nbins;
  HIPEIG_REQUIRE(ncnt < ((size_t)1 << 30), "too many (unit, bin) counters");
  BlockedLayout L = geom;
  L.idx = nullptr; L.val = nullptr; L.off = nullptr;
  L.align = (policy & BIN_GROUP_ALIGN) ? 1 : 0;
  uint32_t* d_cur = nullptr;
  auto scatter = [&](uint32_t* idx, double* val, int fill) {
    const int grid = 8 * c->num_cu;
    if (policy & BIN_LANE_MAJOR)
      hipLaunchKernelGGL(bin_kernel<1>, dim3(grid), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, A->nrows,
                         L.rw, L.binbits, (int)nbins, L.wbits, d_cur, idx, val, fill);
    else
      hipLaunchKernelGGL(bin_kernel<0>, dim3(grid), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, A->nrows,
                         L.rw, L.binbits, (int)nbins, L.wbits, d_cur, idx, val, fill);
  };
  auto build = [&]() -> int {
    HIPEIG_CHECK(hipMalloc((void**)&d_cur, ncnt * sizeof(uint32_t)));
    HIPEIG_CHECK(hipMemsetAsync(d_cur, 0, ncnt * sizeof(uint32_t), c->stream));
    scatter(nullptr, nullptr, 0);
    HIPEIG_CHECK(hipGetLastError());
    std::vector<uint32_t> cnt(ncnt);
    HIPEIG_CHECK(hipMemcpyAsync(cnt.data(), d_cur, ncnt * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPEIG_CHECK(hipStreamSynchronize(c->stream));
    // Exclusive scan in place (-> scatter cursors) with the padding of `policy`: padding slots (index 0xFFFFFFFF,
    // value 0) are skipped by the sweeps.
    const bool unit_batch = policy & BIN_UNIT_BATCH, win_batch = policy & BIN_WIN_BATCH, align = L.align;
    std::vector<uint32_t> off(ntile + 1);
    uint64_t run = 0, counted = 0;
    for (size_t i = 0; i < ncnt; ++i) {
      if (i % bpw == 0) {
        const size_t tile = i / bpw;
        if ((unit_batch && tile % L.nwin == 0) || win_batch) run = (run + TCOOW_BATCH - 1) & ~(uint64_t)(TCOOW_BATCH - 1);
        else if (align) run = (run + 63) & ~(uint64_t)63;
        off[tile] = (uint32_t)run;
      }
      const uint32_t n = cnt[i];
      if (align && n > 0 && n <= 64 && (run & 63) + n > 64) run = (run + 63) & ~(uint64_t)63;
      cnt[i] = (uint32_t)run;
      run += n;
      counted += n;
    }
    off[ntile] = (uint32_t)run;
    HIPEIG_REQUIRE(counted == (uint64_t)A->nnz, "count pass lost non-zeros");
    if (unit_batch) run = (run + TCOOW_BATCH - 1) & ~(uint64_t)(TCOOW_BATCH - 1);     // the last batch is loaded whole
    HIPEIG_REQUIRE(run < ((uint64_t)1 << 32), "blocked stream too long for 32-bit offsets");
    L.slots = (int64_t)run;
    const size_t nslots = (size_t)run;
    HIPEIG_CHECK(hipMemcpyAsync(d_cur, cnt.data(), ncnt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPEIG_CHECK(hipMalloc((void**)&L.off, (ntile + 1) * sizeof(uint32_t)));
    if (policy & BIN_UNCACHED) {
      HIPEIG_CHECK(hipExtMallocWithFlags((void**)&L.idx, nslots * sizeof(uint32_t), hipDeviceMallocUncached));
      HIPEIG_CHECK(hipExtMallocWithFlags((void**)&L.val, nslots * sizeof(double), hipDeviceMallocUncached));
    } else {
      HIPEIG_CHECK(hipMalloc((void**)&L.idx, nslots * sizeof(uint32_t)));
      HIPEIG_CHECK(hipMalloc((void**)&L.val, nslots * sizeof(double)));
    }
    if (nslots != (size_t)A->nnz) {
      HIPEIG_CHECK(hipMemsetAsync(L.idx, 0xFF, nslots * sizeof(uint32_t), c->stream));
      HIPEIG_CHECK(hipMemsetAsync(L.val, 0, nslots * sizeof(double), c->stream));
    }
    HIPEIG_CHECK(hipMemcpyAsync(L.off, off.data(), (ntile + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    scatter(L.idx, L.val, 1);
    HIPEIG_CHECK(hipGetLastError());
    HIPEIG_CHECK(hipStreamSynchronize(c->stream));     // `cnt` and `off` must outlive the copies
    return 0;
  };
  const int rc = build();
  if (d_cur) hipFree(d_cur);
  if (rc) { hipeig_free_layout(&L); return rc; }
  *out = L;
  A->bytes += L.slots * 12 + (int64_t)(ntile + 1) * 4;
  return 0;
}

// TCOO-W (pair = 0, into A->w) or the copy of the pair sweep (pair = 1, into A->p: two accumulators per row, so half
// the rows per unit; no column splits).  Returns 0 on success, 1 on failure, 2 if the operator does not suit the layout.
static int build_tcoow_layout(hipeig_ctx* c, hipeig_csr* A, int pair) {
  BlockedLayout& out = pair ? A->p : A->w;
  if (out.idx) return 0;
  if (A->nnz == 0 || A->nrows == 0) return 2;
  const int acc = pair ? 2 : 1;                        // accumulators per row
  const int64_t max_rw = TCOOW_MAX_RW / acc;
  int wbits = 17;                                      // 15 bits are left for the row inside the unit
  if (const char* e = getenv(pair ? "HIPEIG_TCOOW_PAIR_WBITS" : "HIPEIG_TCOOW_WBITS")) wbits = atoi(e);         // tuning knob
  HIPEIG_REQUIRE(wbits >= 10 && wbits <= 17, "HIPEIG_TCOOW_WBITS out of range");
  while (wbits > 10 && ((int64_t)1 << (wbits - 1)) >= A->gather_len) --wbits;
  const int nwin = (int)((A->gather_len + ((int64_t)1 << wbits) - 1) >> wbits);
  if (nwin > TCOOW_MAX_WIN) return 2;
  int binbits = 4;                                     // 16 columns = ONE line of x per bin (with aligned bins: 4 / 5 / 6 / 7 -> 1.90 / 1.93 / 1.95 / 2.01 ms per product)
  if (const char* e = getenv(pair ? "HIPEIG_TCOOW_PAIR_BINBITS" : "HIPEIG_TCOOW_BINBITS")) binbits = atoi(e);     // tuning knob
  if (binbits > wbits) binbits = wbits;
  HIPEIG_REQUIRE(binbits >= 3, "HIPEIG_TCOOW_BINBITS out of range");
  // one unit per CU if it fits; otherwise the fewest sweeps that fit the LDS, with the rows spread
  // evenly over sweeps * CUs units so that the last sweep is as full as the first
  int64_t sweeps = (A->nrows + (int64_t)c->num_cu * max_rw - 1) / ((int64_t)c->num_cu * max_rw);
  if (sweeps < 1) sweeps = 1;
  int64_t rw = (A->nrows + sweeps * c->num_cu - 1) / (sweeps * c->num_cu);
  rw = (rw + 63) / 64 * 64;
  if (rw < 64) rw = 64;
  if (rw > max_rw) rw = max_rw;
  // Fewer full-size row blocks than half the CUs (a small operator, or the slab of a many-GPU run):
  // keep the row blocks as tall as the LDS allows and let `csplit` workgroups share each of them by
  // column ranges, so that the traffic of x through the L1s is (row blocks) x |x| instead of CUs x |x|.
  int csplit = 1;
  if (!pair) {
    const int64_t rb_min = (A->nrows + TCOOW_MAX_RW - 1) / TCOOW_MAX_RW;
    // Worth it only when x is much larger than the L2s (measured: slab of N = 1e7 on 1/8 of the rows
    // 0.53 -> 0.34 ms, on 1/4 0.90 -> 0.62 ms; at N = 1e6, x = 8 MB, the combine launch costs more than
    // the sweep gains: MINRES iteration 0.141 -> 0.163 ms).
    // Half of what the splits buy on these slabs is column locality per XCD (round 4, EXPERIMENTS.md R4-fold / R4-multigpu):
    // share = blockIdx % csplit, XCD = blockIdx % 8, so with 2 / 4 splits (the slabs of a 4- / 8-GPU run) an XCD's L2 sees
    // a half / a quarter of x, while 3 splits (6 ranks) leave every XCD all of x: 0.46 ms against 0.32 ideal.
    int want = (rb_min * 2 <= c->num_cu && A->gather_len >= 4000000) ? (int)(c->num_cu / rb_min) : 1;
    if (const char* e = getenv("HIPEIG_TCOOW_CSPLIT")) want = atoi(e);          // tuning knob (1 = off)
    if (want > 64) want = 64;
    if (want > 1 && rb_min * want <= HIPEIG_MAX_PARTIALS) {
      csplit = want;
      rw = ((A->nrows + rb_min - 1) / rb_min + 63) / 64 * 64;
      if (rw > TCOOW_MAX_RW) rw = TCOOW_MAX_RW;
    }
  }
  if (const char* e = getenv(pair ? "HIPEIG_TCOOW_PAIR_RW" : "HIPEIG_TCOOW_RW")) rw = (atoi(e) + 63) / 64 * 64;   // tuning knob
  // rw < 2^(32 - wbits): 0xFFFFFFFF stays the padding mark (never binding here: rw <= 20224 < 2^15 <= 2^(32 - wbits))
  HIPEIG_REQUIRE(rw >= 64 && rw <= max_rw && rw < ((int64_t)1 << (32 - wbits)), "HIPEIG_TCOOW_RW out of range");
  BlockedLayout G{};
  G.nunits = (int)((A->nrows + rw - 1) / rw); G.nwin = nwin; G.wbits = wbits; G.rw = (int)rw;
  G.binbits = binbits; G.csplit = csplit;
  int per_cu = (int)(163840 / (blocked_lds_bytes(G, acc) + 256));
  if (per_cu > 2) per_cu = 2;                          // 1024-thread workgroups: at most 32 waves per CU
  if (per_cu < 1) per_cu = 1;
  if (const char* e = getenv("HIPEIG_TCOOW_WG_PER_LAUNCH_CU")) per_cu = atoi(e);   // tuning knob: workgroups per CU in ONE launch (2 with full-height units: both sweeps in one launch, the second workgroup of a CU starts when its first ends)
  HIPEIG_REQUIRE(per_cu >= 1 && per_cu <= 8, "HIPEIG_TCOOW_WG_PER_LAUNCH_CU out of range");
  G.wgs_per_sweep = per_cu * c->num_cu;
  // Bins never straddle a 64-element instruction group and tiles start on group boundaries (round 3; the gaps are
  // padding slots that the sweep skips; ~2 % of the stream).  A line of x is then fetched by exactly ONE gather
  // instruction of one wave: L1 -> L2 read requests per launch 1.829e8 -> 1.704e8, i.e. gather fills per non-zero
  // 0.468 -> 0.431 against the ideal (1 - exp(-k))/k = 0.426, and 2.083 -> 1.90 ms per product at N = 1e7
  // (profiles/r03_spmv_aligned_bins.txt).  HIPEIG_TCOOW_ALIGN=0 restores the unaligned stream.
  // Whatever the knob, every stream range a wave can start on begins on a 256-slot batch (the sweep loads batches
  // lane-major, tcoow_islot / tcoow_vslot): unit starts, and on a row-partitioned operator every window start, since any window can
  // begin a run of the overlapped plan (hipeig_tcoow_plan).  Column-split shares are cut at batch multiples.
  const char* al_env = getenv(pair ? "HIPEIG_TCOOW_PAIR_ALIGN" : "HIPEIG_TCOOW_ALIGN");
  // experiment knob: place the once-read stream in uncached (MTYPE_UC) memory so that it does not
  // occupy L2 lines / tag bandwidth next to the x window
  const char* uc = getenv("HIPEIG_TCOOW_UNCACHED");
  const unsigned policy = BIN_LANE_MAJOR | BIN_UNIT_BATCH | (al_env && atoi(al_env) == 0 ? 0u : BIN_GROUP_ALIGN) |
                          (A->col_stride > 0 ? BIN_WIN_BATCH : 0u) | (uc && atoi(uc) != 0 ? BIN_UNCACHED : 0u);
  const int rc = hipeig_build_binned(c, A, G, policy, &out);
  if (rc) return rc;
  if (pair) {
    HIPEIG_CHECK(hipFuncSetAttribute((const void*)spmv_tcoow_pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)HIPEIG_TCOOW_LDS_MAX));
    return 0;
  }
  HIPEIG_CHECK(hipFuncSetAttribute((const void*)spmv_tcoow_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)HIPEIG_TCOOW_LDS_MAX));
  HIPEIG_CHECK(hipFuncSetAttribute((const void*)spmv_tcoow_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)HIPEIG_TCOOW_LDS_MAX));
  {
    // bound of the fixed-point form (variant 5): max_i sum_j |a_ij| over the local rows
    const int gr = 8 * c->num_cu < HIPEIG_MAX_PARTIALS ? 8 * c->num_cu : HIPEIG_MAX_PARTIALS;
    double* area = c->d_partials + HIPEIG_FX_AREA;
    hipLaunchKernelGGL(rowabs_max_kernel, dim3(gr), dim3(HIPEIG_BLOCK), 0, c->stream, A->d_rowptr, A->d_val, A->nrows, area);
    std::vector<double> part((size_t)gr);
    HIPEIG_CHECK(hipMemcpyAsync(part.data(), area, sizeof(double) * gr, hipMemcpyDeviceToHost, c->stream));
    HIPEIG_CHECK(hipStreamSynchronize(c->stream));
    double m = 0.0;
    for (double v : part) m = (v > m || v != v) ? v : m;
    A->absrow_max = m;
  }
  return 0;
}

int hipeig_csr_build_tcoow(hipeig_ctx* c, hipeig_csr* A) { return build_tcoow_layout(c, A, 0); }

// The variant a launch will use (building the TCOO copy on demand); -1 on failure.
int hipeig_csr_pick_variant(hipeig_ctx* c, hipeig_csr* A) {
  int variant = A->variant;
  if (variant == 6 && hipeig_dense_reserve(c, A)) return -1;    // opt-in only; refused, never replaced by another layout
  if (variant == 0) {
    // the gathered operand does not fit one XCD's L2 -> window it; small problems stream
    variant = (A->gather_len * 8 > (int64_t)3 << 20 && A->nnz > (int64_t)1 << 20) ? (A->reproducible ? 5 : 4) : 2;
  }
  if (variant == 4 || variant == 5) {
    const int rc = hipeig_csr_build_tcoow(c, A);
    if (rc == 1) return -1;
    if (rc == 2) variant = 3;
  }
  if (variant == 3) {
    const int rc = hipeig_csr_build_tcoo(c, A);
    if (rc == 1) return -1;
    if (rc == 2) variant = 2;
  }
  A->last_variant = variant;
  A->last_launches = hipeig_sweep_grid(A, variant).launches;   // sweep launches (split mode adds a combine launch)
  return variant;
}

// ---- layout preparation ------------------------------------------------------------------
__global__ void remap_cols_kernel(int32_t* __restrict__ col, int64_t nnz, const int64_t* __restrict__ offs,
                                  GatherLayout gl) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += step) {
    const int64_t j = col[p];
    int lo = 0, hi = gl.nranks - 1;                    // owner rank: offs[r] <= j < offs[r + 1] (empty slabs have equal offsets)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (j >= offs[mid]) lo = mid; else hi = mid - 1;
    }
    col[p] = (int32_t)gl.pos(lo, j - offs[lo]);
  }
}

// Partition the rows into blocks of <= SPMV_NNZ_PER_BLOCK non-zeros (a longer single row
// gets a block of its own) and pick the sub-wave width from the mean row length.
// rowptr32: host copy of the (int32) row pointer.
int hipeig_csr_finalize(hipeig_ctx* c, hipeig_csr* A, const int32_t* rowptr32) {
  std::vector<int32_t> rb;
  rb.reserve((size_t)(A->nnz / (SPMV_NNZ_PER_BLOCK / 2) + 16));
  rb.push_back(0);
  int64_t r = 0;
  while (r < A->nrows) {
    const int32_t base = rowptr32[r];
    int64_t e = r + 1;
    while (e < A->nrows && rowptr32[e + 1] - base <= SPMV_NNZ_PER_BLOCK && e - r < 1024) ++e;
    rb.push_back((int32_t)e);
    r = e;
  }
  A->n_row_blocks = (int32_t)rb.size() - 1;
  HIPEIG_CHECK(hipMalloc((void**)&A->d_row_blocks, rb.size() * sizeof(int32_t)));
  HIPEIG_CHECK(hipMemcpyAsync(A->d_row_blocks, rb.data(), rb.size() * sizeof(int32_t),
                              hipMemcpyHostToDevice, c->stream));
  HIPEIG_CHECK(hipStreamSynchronize(c->stream));
  const double mean = A->nrows ? (double)A->nnz / (double)A->nrows : 0.0;
  A->lanes_per_row = mean < 6 ? 4 : mean < 24 ? 8 : mean < 96 ? 16 : mean < 384 ? 32 : 64;
  A->bytes = (A->nrows + 1) * 4 + A->nnz * 12 + (int64_t)rb.size() * 4;

  A->gather_len = A->ncols;
  // distributed: gather row counts, size x_full and remap global columns to its layout
  if (hipeig_comm_setup_rows(c, A->nrows, &A->gl)) return 4;
  if (c->collectives) {
    HIPEIG_REQUIRE(c->nranks <= HIPEIG_MAX_RANKS, "too many ranks");
    std::vector<int64_t> offs(c->nranks + 1, 0);
    for (int k = 0; k < c->nranks; ++k) offs[k + 1] = offs[k] + c->row_counts[k];
    HIPEIG_REQUIRE(offs[c->nranks] == A->ncols, "row counts over ranks must add up to ncols");
    HIPEIG_REQUIRE(offs[c->rank] == A->row_offset, "row_offset does not match the rank order");
    HIPEIG_REQUIRE(A->gl.total() < (int64_t)1 << 31, "gathered operand too long for int32 columns");
    for (int k = 0; k < c->nranks; ++k) A->rank_rows.n[k] = (int32_t)c->row_counts[k];     // each below ncols < 2^31
    int64_t* d_offs = (int64_t*)(c->d_scalars + 1024);
    HIPEIG_CHECK(hipMemcpyAsync(d_offs, offs.data(), sizeof(int64_t) * (c->nranks + 1),
                                hipMemcpyHostToDevice, c->stream));
    if (A->nnz > 0) {
      hipLaunchKernelGGL(remap_cols_kernel, dim3(2048), dim3(HIPEIG_BLOCK), 0, c->stream,
                         A->d_col, A->nnz, d_offs, A->gl);
      HIPEIG_CHECK(hipGetLastError());
    }
    HIPEIG_CHECK(hipStreamSynchronize(c->stream));
    A->col_stride = A->gl.h;
    A->gather_len = A->gl.total();
  }
  return 0;
}

static int csr_upload(hipeig_ctx* c, hipeig_csr* A, const int32_t* rp32, const int32_t* col, const double* val) {
  const int64_t nrows = A->nrows, nnz = A->nnz;
  HIPEIG_CHECK(hipMalloc((void**)&A->d_rowptr, (size_t)(nrows + 1) * sizeof(int32_t)));
  HIPEIG_CHECK(hipMalloc((void**)&A->d_col, (size_t)(nnz > 0 ? nnz : 1) * sizeof(int32_t)));
  HIPEIG_CHECK(hipMalloc((void**)&A->d_val, (size_t)(nnz > 0 ? nnz : 1) * sizeof(double)));
  HIPEIG_CHECK(hipMemcpyAsync(A->d_rowptr, rp32, (size_t)(nrows + 1) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  if (nnz > 0) {
    HIPEIG_CHECK(hipMemcpyAsync(A->d_col, col, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPEIG_CHECK(hipMemcpyAsync(A->d_val, val, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  HIPEIG_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int hipeig_csr_create(hipeig_ctx* c, int64_t nrows, int64_t ncols, int64_t row_offset,
                                 const int64_t* rowptr, const int32_t* col, const double* val,
                                 hipeig_csr** out) {
  HIPEIG_REQUIRE(out && rowptr, "null argument");
  HIPEIG_REQUIRE(nrows >= 0 && ncols >= 0 && ncols < ((int64_t)1 << 31), "bad shape");
  HIPEIG_REQUIRE(rowptr[0] == 0, "rowptr[0] must be 0");
  const int64_t nnz = rowptr[nrows];
  HIPEIG_REQUIRE(nnz >= 0 && nnz < ((int64_t)1 << 31), "local nnz must fit int32");
  std::vector<int32_t> rp32((size_t)nrows + 1);
  for (int64_t i = 0; i <= nrows; ++i) {
    if (i > 0) HIPEIG_REQUIRE(rowptr[i] >= rowptr[i - 1], "rowptr must be non-decreasing");
    rp32[i] = (int32_t)rowptr[i];
  }
  for (int64_t p = 0; p < nnz; ++p)
    HIPEIG_REQUIRE(col[p] >= 0 && col[p] < ncols, "column index out of range");
  hipeig_csr* A = (hipeig_csr*)calloc(1, sizeof(hipeig_csr));
  HIPEIG_REQUIRE(A != nullptr, "out of host memory");
  A->nrows = nrows; A->ncols = ncols; A->nnz = nnz; A->row_offset = row_offset;
  int rc = csr_upload(c, A, rp32.data(), col, val);
  if (rc == 0) rc = hipeig_csr_finalize(c, A, rp32.data());
  if (rc) { hipeig_csr_destroy(c, A); return rc; }        // nothing allocated so far outlives a failure
  *out = A;
  return 0;
}

extern "C" int hipeig_csr_destroy(hipeig_ctx* c, hipeig_csr* A) {
  if (!A) return 0;
  hipStreamSynchronize(c->stream);
  if (c->mr_graph && c->mr_graph_key && *(const void**)c->mr_graph_key == (const void*)A) {
    hipGraphExecDestroy(c->mr_graph);      // the captured MINRES chunk points into this operator
    c->mr_graph = nullptr;
  }
  if (A->d_rowptr) hipFree(A->d_rowptr);
  if (A->d_col) hipFree(A->d_col);
  if (A->d_val) hipFree(A->d_val);
  if (A->d_row_blocks) hipFree(A->d_row_blocks);
  for (BlockedLayout* L : {&A->t, &A->w, &A->p, &A->b[0], &A->b[1], &A->b[2]}) hipeig_free_layout(L);
  hipeig_dense_free(A);
  free(A);
  return 0;
}

// Layout constants of the blocked copy the product runs on (what a committed counter profile is only valid for):
// out[0] = kernel variant of the last launch, [1] rows per row block, [2] window bits, [3] row blocks, [4] windows,
// [5] column splits, [6] workgroups per sweep launch, [7] threads per workgroup, [8] batch unroll, [9] chunks of the
// operand exchange, [10] rows per (rank, chunk) of the gathered layout (0: not partitioned), [11] bins, [12] stream
// slots incl. padding (TCOO-W)
extern "C" int hipeig_csr_layout_info(hipeig_csr* A, int64_t out[13]) {
  memset(out, 0, 13 * sizeof(int64_t));
  out[0] = A->last_variant;
  const bool wg = A->last_variant == 4 || A->last_variant == 5;
  if (wg || A->last_variant == 3) {
    const BlockedLayout& L = wg ? A->w : A->t;
    out[1] = L.rw; out[2] = L.wbits; out[3] = L.nunits; out[4] = L.nwin; out[6] = L.wgs_per_sweep;
    out[7] = wg ? TCOOW_THREADS : HIPEIG_BLOCK; out[8] = TCOO_UNROLL;
  }
  if (wg) { out[5] = A->w.csplit; out[11] = A->w.binbits + 100 * A->w.align; out[12] = A->w.slots; }
  if (A->col_stride > 0) { out[9] = A->gl.nchunks; out[10] = A->gl.h; }
  return 0;
}

extern "C" int hipeig_csr_info(hipeig_csr* A, int64_t info[8]) {
  info[0] = A->nrows; info[1] = A->ncols; info[2] = A->nnz; info[3] = A->row_offset;
  info[4] = A->last_variant; info[5] = A->bytes; info[6] = A->n_row_blocks; info[7] = A->last_launches;
  return 0;
}

// Error-bound ingredients of the fixed-point variant: out[0] = max_i sum_j |a_ij| (local rows, set when the
// blocked layout is built; 0 before), out[1] = max |x| of the operand of the most recent variant-5 product.
extern "C" int hipeig_csr_fixed_info(hipeig_ctx* c, hipeig_csr* A, double out[2]) {
  out[0] = A->absrow_max;
  out[1] = 0.0;
  const int g = grid_for(A->gather_len, 8);
  std::vector<double> part((size_t)g);
  HIPEIG_CHECK(hipMemcpyAsync(part.data(), c->d_partials + HIPEIG_FX_AREA, sizeof(double) * g, hipMemcpyDeviceToHost, c->stream));
  HIPEIG_CHECK(hipStreamSynchronize(c->stream));
  for (double v : part) out[1] = (v > out[1] || v != v) ? v : out[1];
  return 0;
}

extern "C" int hipeig_csr_set_variant(hipeig_csr* A, int variant) {
  HIPEIG_REQUIRE(variant >= 0 && variant <= 6, "unknown variant");
  if (variant == 6 && hipeig_dense_refusal(nullptr, A)) return 2;   // what the operator alone shows; the context at first use
  A->variant = variant;
  return 0;
}

extern "C" int hipeig_csr_set_reproducible(hipeig_csr* A, int on) {
  A->reproducible = on ? 1 : 0;
  return 0;
}

extern "C" int hipeig_csr_download(hipeig_ctx* c, hipeig_csr* A, int64_t* rowptr, int32_t* col, double* val) {
  HIPEIG_REQUIRE(A->col_stride == 0 || col == nullptr, "columns of a partitioned operator are remapped");
  HIPEIG_CHECK(hipStreamSynchronize(c->stream));
  if (rowptr) {
    std::vector<int32_t> rp((size_t)A->nrows + 1);
    HIPEIG_CHECK(hipMemcpy(rp.data(), A->d_rowptr, rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < rp.size(); ++i) rowptr[i] = rp[i];
  }
  if (col && A->nnz) HIPEIG_CHECK(hipMemcpy(col, A->d_col, (size_t)A->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (val && A->nnz) HIPEIG_CHECK(hipMemcpy(val, A->d_val, (size_t)A->nnz * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
