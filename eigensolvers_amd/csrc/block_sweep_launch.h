// Host side of "one operator sweep of an interleaved block of K operands with an element epilogue": the block products
// (spmm.hip), the iteration sweep of the block MINRES (minres_block.hip) and both passes of the Lanczos filter
// (lanczos_filter.hip).  The caller owns the kernel - a template whose first parameter is VARIANT, as
// minres_block_ka_kernel - and its arguments; the kernel choice, the view, the grid and the order of the launches live here, once.
//   BlockSweepPlan plan;  block_sweep_plan_build<K>(c, A, for_solve, &plan);  block_sweep_set_lds_limit(plan, k<2, K>, ...);
//   per sweep:  hipeig_block_allgather(...)  (the caller's: a solver's exchange carries sums of its own)
//               block_sweep_launch(...)      (one launch of the row-owner kernel, or one per sweep of the windows)
#pragma once
#include <type_traits>
#include "spmm_device.h"
#include "dense_device.h"

// spmm.hip
int hipeig_block_pick_variant(hipeig_ctx* c, hipeig_csr* A, int K, int for_solve);
BcooView hipeig_bcoo_view(const hipeig_csr* A, const BlockedLayout& L);
int hipeig_block_allgather(hipeig_ctx* c, hipeig_csr* A, int K, const double* xb_local, const double** xb_full);
int hipeig_block_pack(hipeig_ctx* c, int K, int64_t n, int k, const double* const* cols, double* blk);
int hipeig_block_unpack(hipeig_ctx* c, int K, int64_t n, int k, const double* blk, double* const* cols);
int hipeig_rowowner_grid(const hipeig_ctx* c, const hipeig_csr* A);
// dense.hip
DenseView hipeig_dense_view(const hipeig_csr* A);
// comm.hip
double* hipeig_gather_block_slot(hipeig_ctx* c, const GatherLayout& gl, int K);
int hipeig_block_reserve(hipeig_ctx* c, const GatherLayout& gl, int K);

// Doubles between the partial areas of a block solve in hipeig_ctx::d_partials: one record of K <= BCOO_KMAX per workgroup.
#define BLOCK_PART_STRIDE ((size_t)HIPEIG_MAX_PARTIALS * BCOO_KMAX)

struct BlockSweepPlan {
  int variant;               // 1 row-owner CSR sweep, 2 window-blocked (TCOO-B), 3 dense block sweep
  BcooView tview;            // the blocked copy (variants 1 and 3: passed along, never read)
  DenseView dview;           // the dense copy of variant 3 (the caller's kernel takes it from the plan)
  size_t lds;                // dynamic LDS of a sweep launch
  int threads;               // per workgroup
  int gA, nsweep;            // workgroups per sweep launch, sweep launches
  int nPA;                   // records of K partials one sweep leaves (side by side, one per workgroup)
};

// Picks the kernel for interleave width K (building the blocked copy on demand) and sizes one sweep of A.  for_solve: the
// sweep leaves per-workgroup partials (hipeig_block_pick_variant), which have to fit their area.
template <int K>
static inline int block_sweep_plan_build(hipeig_ctx* c, hipeig_csr* A, int for_solve, BlockSweepPlan* p) {
  // its CSR arrays are empty: a block sweep over them would be a silent zero product
  HIPEIG_REQUIRE(!hipeig_kron_raw(A), "block sweeps are not built for the Kronecker-sum operator: apply it vector by vector");
  p->variant = hipeig_block_pick_variant(c, A, K, for_solve);
  if (p->variant < 0) return 1;
  const BlockedLayout& L = A->b[layout_slot(K)];
  p->tview = hipeig_bcoo_view(A, L);
  p->dview = hipeig_dense_view(A);                             // variant 3: hipeig_block_pick_variant has reserved the copy
  // dense: a persistent grid over groups of 4 waves x DenseBlockShape<K>::ROWS rows, one launch, no LDS
  const SweepGrid sg = (p->variant == 2) ? blocked_grid(L)
                     : (p->variant == 3) ? SweepGrid{hipeig_dense_grid(A, DenseBlockShape<K>::ROWS * (HIPEIG_BLOCK / HIPEIG_WAVE)), 1}
                                         : SweepGrid{hipeig_rowowner_grid(c, A), 1};
  if (p->variant == 3) A->dense_grid_blk = sg.wgs;
  p->gA = sg.wgs; p->nsweep = sg.launches;
  p->lds = (p->variant == 2) ? blocked_lds_bytes(L, K) : 0;
  p->threads = (p->variant == 2) ? BCOO_THREADS : HIPEIG_BLOCK;
  p->nPA = p->gA * p->nsweep;
  if (for_solve) HIPEIG_REQUIRE((int64_t)p->nsweep * p->gA <= HIPEIG_MAX_PARTIALS, "too many sweeps for the partial-sum buffer");
  return 0;
}

// The window-blocked layout takes more dynamic LDS than the default limit: the caller's <2, ...> instantiation(s).
template <class... Kernel>
static inline int block_sweep_set_lds_limit(const BlockSweepPlan& p, Kernel... k2) {
  if (p.variant != 2) return 0;
  for (const void* k : {(const void*)k2...})
    HIPEIG_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HIPEIG_BCOO_LDS_MAX));
  return 0;
}

// The launches of one sweep.  `launch(variant, grid, threads, lds_bytes, tview, partial_offset)` is called once per kernel
// launch with the first as std::integral_constant, so that the caller's generic lambda names its kernel as
// kernel<decltype(variant)::value, K, ...>; workgroup b of that launch owns record partial_offset + b of the plan's nPA.
template <class Launch>
static inline void block_sweep_launch(hipeig_ctx* c, const BlockSweepPlan& p, Launch&& launch) {
  using std::integral_constant;
  if (p.variant == 2) {
    BcooView tv = p.tview;
    for (int sw = 0; sw < p.nsweep; ++sw) {                       // one launch per sweep of the windows; partials side by side
      tv.unit_begin = sw * p.gA;
      launch(integral_constant<int, 2>{}, p.gA, p.threads, p.lds, tv, sw * p.gA);
    }
  } else if (p.variant == 3) {
    launch(integral_constant<int, 3>{}, p.gA, p.threads, p.lds, p.tview, 0);
  } else {
    launch(integral_constant<int, 1>{}, p.gA, p.threads, p.lds, p.tview, 0);
  }
}
