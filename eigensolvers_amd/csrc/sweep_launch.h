// Host side of "one operator sweep of a single vector with a row epilogue": the product and shifted product of spmv.hip
// (no reduction) and the iteration sweeps of the MINRES drivers (minres.hip, minres_shifts.hip: one reduced scalar).  The
// caller owns the kernel - a template over (VARIANT, FIXED) as minres_ka_kernel, or named kernels picked with `if constexpr` as
// spmv_launcher - and its arguments; the layout, the grids,
// the exchange and the order of the launches live here, once.
//   SweepPlan plan;  sweep_plan_build(c, A, combine_grid, &plan);  sweep_set_lds_limits(plan, k<3>, k<4,0>, k<4,1>);
//   per sweep:  sweep_prepare(...)  (exchange, waits, raw launches; hands back the gathered operand)
//               sweep_launch(...)   (the epilogue launches, then the combine launch of a column-split sweep)
// The product raises the LDS limits of its kernels where the layouts are built, not per product.  The sweeps of interleaved
// blocks have their own launcher, block_sweep_launch.h; the pair sweep (two accumulators per row, no split, no exchange)
// keeps its loop in spmv.hip.
#pragma once
#include <type_traits>
#include "spmv_device.h"
#include "dense_device.h"

CsrView hipeig_csr_view(const hipeig_csr* A);
TcooView hipeig_tcoo_view(const hipeig_csr* A, const BlockedLayout& L);
int hipeig_tcoow_reserve(hipeig_ctx* c, const hipeig_csr* A);
SweepGrid hipeig_sweep_grid(const hipeig_csr* A, int variant);
int hipeig_csr_pick_variant(hipeig_ctx* c, hipeig_csr* A);
size_t hipeig_tcoo_lds_bytes(const hipeig_csr* A);
DenseView hipeig_dense_view(const hipeig_csr* A);
void hipeig_phase_mark(hipeig_ctx* c, int k);
const double* hipeig_gathered(hipeig_ctx* c);

struct SweepPlan {
  int variant;               // 1-4 (the public variant 5 is 4 with `fixed`), 6 the dense row sweep, 7 the Kronecker-sum operator
  int fixed;                 // TCOO-W with fixed-point accumulators: same structure as 4
  CsrView view;
  TcooView tview;            // the blocked copy of variants 3 / 4
  DenseView dview;           // the dense copy of variant 6 (the caller's kernel takes it from the plan)
  size_t lds;                // dynamic LDS of a sweep launch
  int gA, nsweep;            // workgroups per sweep launch, sweep launches
  bool split;                // column-split TCOO-W: raw slabs + a combine launch that carries the epilogue
  int gC;                    // grid of that combine launch
  int nPA;                   // workgroups whose epilogue runs in one sweep: the partials a reducing kernel leaves, side by side
  const double* kron_raw;    // variant 7: the operator's raw sums, which the combine launch carries the epilogue over
};

// Picks the layout (building the blocked copy on demand) and sizes one sweep of A.  `combine_grid`: the grid of the combine
// launch of a column-split sweep, the caller's because it depends on what the epilogue carries.  A caller whose kernel leaves
// a partial per workgroup requires nPA <= HIPEIG_WIDE_PARTIALS itself.
static inline int sweep_plan_build(hipeig_ctx* c, hipeig_csr* A, int combine_grid, SweepPlan* p) {
  p->variant = hipeig_csr_pick_variant(c, A);
  if (p->variant < 0) return 1;
  p->fixed = (p->variant == 5) ? 1 : 0;
  if (p->fixed) p->variant = 4;
  HIPEIG_REQUIRE((p->variant >= 1 && p->variant <= 4) || p->variant == 6 || p->variant == 7, "unknown sweep layout");
  p->kron_raw = hipeig_kron_raw(A);
  HIPEIG_REQUIRE((p->variant == 7) == (p->kron_raw != nullptr), "variant 7 belongs to the operators of hipeig_kron_create, and they take no other");
  if (p->variant == 4 && hipeig_tcoow_reserve(c, A)) return 1;
  p->view = hipeig_csr_view(A);
  p->tview = hipeig_tcoo_view(A, (p->variant == 4) ? A->w : A->t);
  p->dview = hipeig_dense_view(A);                             // variant 6: hipeig_csr_pick_variant has reserved the copy
  p->lds = (p->variant == 4) ? blocked_lds_bytes(A->w, 1) : (p->variant == 3) ? hipeig_tcoo_lds_bytes(A) : 0;
  const SweepGrid sg = hipeig_sweep_grid(A, p->variant);
  p->gA = sg.wgs; p->nsweep = sg.launches;
  p->split = (p->variant == 4) && A->w.csplit > 1;
  p->gC = combine_grid;
  p->nPA = p->split ? p->gC : p->gA * p->nsweep;
  if (p->variant == 6) A->dense_grid_vec = p->gA;              // lds = 0, one launch, no split: a persistent grid
  if (p->variant == 7) { p->gA = p->gC; p->nsweep = 1; p->nPA = p->gC; }   // the one epilogue launch is the combine launch: no LDS, no blocked copy
  return 0;
}

// The blocked layouts take more dynamic LDS than the default limit: the caller's <3>, <4, 0> and <4, 1> instantiations.
static inline int sweep_set_lds_limits(const SweepPlan& p, const void* k3, const void* k40, const void* k41) {
  if (p.variant == 3) HIPEIG_CHECK(hipFuncSetAttribute(k3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HIPEIG_TCOO_LDS_MAX));
  if (p.variant == 4) {
    HIPEIG_CHECK(hipFuncSetAttribute(k40, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HIPEIG_TCOOW_LDS_MAX));
    HIPEIG_CHECK(hipFuncSetAttribute(k41, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HIPEIG_TCOOW_LDS_MAX));
  }
  return 0;
}

// What sweep_prepare leaves for sweep_launch.
struct SweepOperand {
  const double* xg;          // the gathered operand (one GPU: the operand itself)
  TcooView tv;               // view of the epilogue launches
  bool has_last;             // false: the raw launches covered every window and only the combine launch follows
  int ncombine;              // slabs the combine launch adds (0: none)
};

// spmv.hip: the exchange and every launch of a TCOO-W sweep that carries no epilogue (product kernels with the empty one)
int hipeig_tcoow_run_plan(hipeig_ctx* c, hipeig_csr* A, const SweepPlan& p, const double* x_local, SweepOperand* o);

// Everything of one sweep that comes before its epilogue launches: the operand exchange with its waits and, for TCOO-W,
// the raw launches of the plan (own windows under the exchange, chunk by chunk behind it).
static inline int sweep_prepare(hipeig_ctx* c, hipeig_csr* A, const SweepPlan& p, const double* x_local, SweepOperand* o) {
  o->xg = nullptr; o->tv = p.tview; o->has_last = true; o->ncombine = 0;
  if (p.variant == 4) return hipeig_tcoow_run_plan(c, A, p, x_local, o) ? 4 : 0;
  if (p.variant == 6) { o->xg = x_local; return 0; }           // whole operator, no communicator: no exchange
  if (p.variant == 7) {                                        // the same, and the product itself: raw sums into the operator's buffer
    o->xg = x_local;
    return hipeig_kron_product(c, A, x_local) ? 4 : 0;
  }
  return hipeig_allgather_x(c, A->gl, x_local, A->nrows, &o->xg) ? 4 : 0;
}

// The epilogue launches of one sweep.  `launch(variant, fixed, grid, threads, lds_bytes, tview, xg, partial_offset)` is
// called once per kernel launch with the first two as std::integral_constant, so that the caller's generic lambda names
// its kernel as kernel<decltype(variant)::value, decltype(fixed)::value> (variant 5: the combine step, tcoow_combine_sweep on
// tview.raw_out / part_base / part_stride; variant 6: dense_row_sweep on the plan's dview; a Kronecker-sum operator: that
// combine step alone, over the one slab sweep_prepare left in the operator's raw buffer); workgroup b of that launch owns
// partial partial_offset + b of the plan's nPA.
template <class Launch>
static inline void sweep_launch(hipeig_ctx* c, const SweepPlan& p, const SweepOperand& o, Launch&& launch) {
  using std::integral_constant;
  TcooView tv = o.tv;
  if (p.variant == 4) {
    if (o.has_last) {
      for (int sw = 0; sw < p.nsweep; ++sw) {
        tv.unit_begin = sw * p.gA;
        if (p.fixed) launch(integral_constant<int, 4>{}, integral_constant<int, 1>{}, p.gA, TCOOW_THREADS, p.lds, tv, o.xg, sw * p.gA);
        else launch(integral_constant<int, 4>{}, integral_constant<int, 0>{}, p.gA, TCOOW_THREADS, p.lds, tv, o.xg, sw * p.gA);
      }
    }
    if (o.ncombine) {
      tv.raw_out = c->ytmp;
      tv.part_base = o.ncombine;                                  // number of slabs to add
      launch(integral_constant<int, 5>{}, integral_constant<int, 0>{}, p.gC, HIPEIG_BLOCK, (size_t)0, tv, o.xg, 0);
    }
  } else if (p.variant == 3) {
    for (int sw = 0; sw < p.nsweep; ++sw) {                       // one launch per sweep, 4 units per workgroup; partials side by side
      tv.unit_begin = sw * p.gA * 4;
      launch(integral_constant<int, 3>{}, integral_constant<int, 0>{}, p.gA, HIPEIG_BLOCK, p.lds, tv, o.xg, sw * p.gA);
    }
  } else if (p.variant == 7) {
    tv.raw_out = const_cast<double*>(p.kron_raw);
    tv.part_base = 1; tv.part_stride = 0;                         // one slab of tv.nrows raw sums
    launch(integral_constant<int, 5>{}, integral_constant<int, 0>{}, p.gC, HIPEIG_BLOCK, (size_t)0, tv, o.xg, 0);
  } else if (p.variant == 6) {
    launch(integral_constant<int, 6>{}, integral_constant<int, 0>{}, p.gA, HIPEIG_BLOCK, (size_t)0, tv, o.xg, 0);
  } else if (p.variant == 1) {
    launch(integral_constant<int, 1>{}, integral_constant<int, 0>{}, p.gA, HIPEIG_BLOCK, (size_t)0, tv, o.xg, 0);
  } else {
    launch(integral_constant<int, 2>{}, integral_constant<int, 0>{}, p.gA, HIPEIG_BLOCK, (size_t)0, tv, o.xg, 0);
  }
}
