/*
 * hipeig.h - C ABI of libhipeig.so: the MI355X (gfx950) backend of the inexact-Lanczos
 * shift-and-invert hot path.
 *
 * This is the drop-in boundary.  The upstream reference has no FFI of its own: its
 * plugin surface is the Python ABC ``AbstractVector`` (abstractVector.py:15-169) and the
 * ndarray backend ``NumpyVector`` (numpyVector.py:23-238).  Every entry point below is
 * what a ``HipVector`` sitting beside ``NumpyVector`` binds through ``ctypes``; each one
 * cites the reference call site it replaces.  Signatures use plain pointers and sizes
 * only (no torch / numpy types).  All device pointers are raw ``double*`` obtained from
 * ``hipeig_vec_alloc``; a "vector" is the LOCAL row slice of the (possibly
 * row-partitioned) global vector, ``n`` always being the local length.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; ``hipeig_last_error()``
 *     returns a thread-local human-readable message for the last failure.
 *   - functions that return scalars to the host (dot, nrm2, gram, minres info ...) are
 *     synchronous on return; all others are asynchronous on the context's compute
 *     stream and ordered with respect to each other.
 *   - reductions use a fixed grid and a fixed summation tree: results are bitwise
 *     reproducible run to run for the same inputs, device and rank count.
 *   - with a communicator attached (hipeig_comm_init) every reduction is followed by an
 *     RCCL all-reduce and every operator application by an all-gather of x.
 */
#ifndef HIPEIG_H
#define HIPEIG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hipeig_ctx hipeig_ctx;   /* device, streams, workspaces, communicator      */
typedef struct hipeig_csr hipeig_csr;   /* device-resident sparse operator (local rows)    */

/* ---- context ---------------------------------------------------------------------- */
int hipeig_ctx_create(int device, hipeig_ctx** out);
int hipeig_ctx_destroy(hipeig_ctx* ctx);
int hipeig_ctx_sync(hipeig_ctx* ctx);                       /* wait for the compute stream */
const char* hipeig_last_error(void);
/* info[0]=CU count, [1]=wave size, [2]=total HBM bytes, [3]=free HBM bytes, [4]=L2 bytes  */
int hipeig_device_info(hipeig_ctx* ctx, int64_t info[8], char* name, int name_len);

/* ---- communicator (one process per GPU; RCCL over xGMI) --------------------------- */
/* The host side exchanges the 128-byte id out of band (eigensolvers_amd.distributed: a TCP exchange). */
int hipeig_comm_unique_id(void* id128);
/* path of the RCCL library in use (ROCm's /opt/rocm/lib/librccl.so unless HIPEIG_RCCL_LIB says otherwise) */
int hipeig_comm_library(char* path, int path_len);
int hipeig_comm_init(hipeig_ctx* ctx, int nranks, int rank, const void* id128);
int hipeig_comm_destroy(hipeig_ctx* ctx);
int hipeig_comm_info(hipeig_ctx* ctx, int* nranks, int* rank);
/* stats[0] = collectives (operand exchanges + all-reduces) issued by the most recent hipeig_minres / hipeig_minres_block call of
 * this rank: a row-partitioned MINRES iteration costs two - the exchange of the operand, which also carries every rank's
 * share of <y,y>, and ONE all-reduce carrying <v,y> and the previous iteration's <x,x>. */
int hipeig_comm_stats(hipeig_ctx* ctx, int64_t stats[4]);
/* Replica mode for work that is spread over ranks without partitioning the rows (FEAST: one contour
 * point per GPU, feast.py:186-201): partitioned = 0 keeps the communicator but switches the implicit
 * all-gather / all-reduce of every product / reduction off; the only exchange is then
 * hipeig_vec_allreduce (SUM of a whole vector over the ranks, in place), which replaces the serial
 * accumulation of the quadrature terms in updateQ (feast.py:105-121). */
int hipeig_comm_set_partitioned(hipeig_ctx* ctx, int partitioned);
int hipeig_vec_allreduce(hipeig_ctx* ctx, double* v, int64_t n);
/* Rehearsal backend: the same collectives between several contexts of ONE process (one host thread
 * per rank; host barrier + device-to-device copies, sums in rank order).  Lets the multi-rank path
 * be run on a single GPU, where RCCL refuses two ranks on one device.  Every rank's thread must
 * make the same sequence of calls; a rank waiting 120 s for its peers fails instead of hanging. */
/* ---- the operand exchange of a row-partitioned product (numpyVector.py:152: one H@x per MINRES iteration) ------------
 * Two backends behind the same calls: 0 = RCCL's ncclAllGather (default), 1 = direct peer writes - every rank stores its
 * slice into the gathered buffers of its peers over all xGMI links at once (csrc/comm_direct.hip).  The direct backend
 * needs the peers' buffers mapped: hipeig_direct_alloc returns this rank's 192-byte record (two hipIpc handles - gathered
 * buffers, arrival flags - and the PCI bus id of its device; capacity in doubles per buffer, at least the gathered length
 * of the largest operator; attach refuses when a peer's device is not visible or not addressable from here), the host
 * side all-gathers the records of all ranks in rank order (eigensolvers_amd.distributed) and hands them to
 * hipeig_direct_attach; hipeig_comm_set_gather_backend then switches (every rank at the same point, nothing in flight).
 * hipeig_comm_gather_info: info[0] backend, [1] attached, [2] capacity, [3] exchanges begun, [4] error word of the
 * bounded waits (0 = none), [5] HIPEIG_GATHER_CHUNKS override (0 = automatic).  A wait that gave up (HIPEIG_DIRECT_WAIT_S,
 * default 120 s: the skew between ranks it tolerates) makes the NEXT call that returns anything to the host - dot, nrm2,
 * the solvers, downloads, hipeig_ctx_sync - fail with rc 4; the error sticks to the context.                           */
int hipeig_comm_init_direct(hipeig_ctx* ctx, int nranks, int rank);   /* rank / size without RCCL: every exchange direct */
int hipeig_comm_set_allreduce_backend(hipeig_ctx* ctx, int backend);  /* small all-reduces: 0 RCCL, 1 the peers' mailboxes */
int hipeig_direct_alloc(hipeig_ctx* ctx, int64_t capacity_doubles, void* record192_out);
int hipeig_direct_attach(hipeig_ctx* ctx, const void* all_records /* nranks x 192 bytes */);
int hipeig_direct_release(hipeig_ctx* ctx);    /* frees the direct buffers again (after a collective fall-back to RCCL) */
int hipeig_comm_set_wait_limit(hipeig_ctx* ctx, double seconds);   /* limit of the bounded waits from now on; <= 0: default */
int hipeig_comm_set_gather_backend(hipeig_ctx* ctx, int backend);
int hipeig_comm_gather_info(hipeig_ctx* ctx, int64_t info[8]);
/* chunks of the operand exchange (1-4; 0 = automatic) for operators created from now on; the same on every rank */
int hipeig_comm_set_gather_chunks(hipeig_ctx* ctx, int nchunks);
/* measurement hooks: per-phase event times of the most recent partitioned product (ms; negative = phase absent):
 * out[0] operand exchange, [1] sweep of the rank's own column windows (under the exchange), [2] sweep of the other
 * windows incl. waits for later chunks, [3] whole product, [4] compute stream idle before the first chunk arrived;
 * and the average time of `reps` back-to-back all-reduces of `count` doubles.                                          */
int hipeig_phase_timing(hipeig_ctx* ctx, int on);
/* on = 0: products of this context place their own slice and SKIP the exchange (results meaningless) - times one rank's
 * sweeps alone on a shared GPU; not collective, switch back on before the next collective product                     */
int hipeig_comm_set_exchange(hipeig_ctx* ctx, int on);
int hipeig_phase_get(hipeig_ctx* ctx, double out[8]);
int hipeig_comm_bench_allreduce(hipeig_ctx* ctx, int count, int reps, double* ms_each);
int hipeig_loopback_group_create(int nranks, void** group_out);
int hipeig_loopback_group_destroy(void* group);
int hipeig_comm_init_loopback(hipeig_ctx* ctx, void* group, int rank);

/* ---- vectors: replaces the ndarray held by NumpyVector (numpyVector.py:25-28) ----- */
int hipeig_vec_alloc(hipeig_ctx* ctx, int64_t n, double** out);
int hipeig_vec_free(hipeig_ctx* ctx, double* v);
int hipeig_vec_upload(hipeig_ctx* ctx, double* dst, const double* host_src, int64_t n);
int hipeig_vec_download(hipeig_ctx* ctx, double* host_dst, const double* src, int64_t n);
int hipeig_vec_copy(hipeig_ctx* ctx, double* dst, const double* src, int64_t n);  /* copy(), :95 */
int hipeig_vec_fill(hipeig_ctx* ctx, double* v, int64_t n, double value);

/* ---- BLAS-1 class ----------------------------------------------------------------- */
/* vdot / np.dot, numpyVector.py:89-93 (real vectors: conjugated == bilinear)            */
int hipeig_dot(hipeig_ctx* ctx, int64_t n, const double* x, const double* y, double* out);
/* la.norm, numpyVector.py:80-81                                                          */
int hipeig_nrm2(hipeig_ctx* ctx, int64_t n, const double* x, double* out);
/* normalize(): x /= ||x||, numpyVector.py:76-78; returns the norm it divided by          */
int hipeig_normalize(hipeig_ctx* ctx, int64_t n, double* x, double* norm_out);
/* __mul__/__rmul__/__truediv__ (out of place), numpyVector.py:57-64: y = alpha*x         */
int hipeig_scale(hipeig_ctx* ctx, int64_t n, double alpha, const double* x, double* y);
/* y = x / alpha (a true division, as ndarray/alpha rounds)                               */
int hipeig_divide(hipeig_ctx* ctx, int64_t n, double alpha, const double* x, double* y);
/* y = a*x + b*y                                                                          */
int hipeig_axpby(hipeig_ctx* ctx, int64_t n, double a, const double* x, double b, double* y);
/* linearCombination, numpyVector.py:105-119: out = sum_j coeffs[j]*vecs[j]  (k >= 1)     */
int hipeig_lincomb(hipeig_ctx* ctx, int64_t n, int k, const double* coeffs,
                   const double* const* vecs, double* out);
/* basisTransformation, util_funcs.py:208-231: outs[c] = sum_j C[j*ldc + c]*vecs[j]       */
int hipeig_lincomb_block(hipeig_ctx* ctx, int64_t n, int m, int k, const double* C, int ldc,
                         const double* const* vecs, double* const* outs);

/* ---- tall-skinny products --------------------------------------------------------- */
/* out[j] = <Y_j, x>, j < m : one pass over x and the m basis columns.  Replaces the m
 * python-level vdots of extendOverlapMatrix / extendMatrixRepresentation
 * (numpyVector.py:205-238) and the projections of the Gram-Schmidt sweep (:132-139).     */
int hipeig_multi_dot(hipeig_ctx* ctx, int64_t n, int m, const double* const* Y,
                     const double* x, double* out);
/* x += sum_j c[j]*Y_j                                                                    */
int hipeig_multi_axpy(hipeig_ctx* ctx, int64_t n, int m, const double* const* Y,
                      const double* c, double* x);
/* out[i*mb + j] = <A_i, B_j> (row-major ma x mb). overlapMatrix (numpyVector.py:192-203)
 * with A == B; matrixRepresentation (:180-190) with B = H*A.                             */
int hipeig_gram(hipeig_ctx* ctx, int64_t n, int ma, const double* const* A, int mb,
                const double* const* B, double* out);
/* orthogonalize_against_set, numpyVector.py:121-145.  x is orthogonalised against the m
 * columns of Y in place and normalised by sqrt(x.x).  method 0 = the reference's single
 * modified-Gram-Schmidt sweep (division by q.q included), 1 = classical GS applied twice
 * (two batched passes, one reduction each).  *innerprod receives x.x BEFORE
 * normalisation; if it is <= lindep x is left un-normalised and *is_lindep = 1 (the
 * caller returns None, numpyVector.py:141-144).                                          */
int hipeig_orthonormalize(hipeig_ctx* ctx, int64_t n, int m, const double* const* Y,
                          double* x, double lindep, int method, double* innerprod,
                          int* is_lindep);

/* Sequential modified Gram-Schmidt projection, coefficients returned: for j = 0..m-1:
 * coeffs[j] = <V_j, w>; w -= coeffs[j]*V_j.  This is the Arnoldi orthogonalisation inside
 * scipy's gcrotmk/_fgmres, i.e. the inner loop of NumpyVector.solve with linearSolver="gcrotmk"
 * (numpyVector.py:161); no host round trip between columns.  The pair form treats (re, im)
 * buffer pairs as complex vectors with the conjugated product (complex contour solves of
 * feast.py:90); coeffs then holds m (re, im) pairs.                                       */
int hipeig_mgs_project(hipeig_ctx* ctx, int64_t n, int m, const double* const* V, double* w,
                       double* coeffs);
int hipeig_pair_mgs_project(hipeig_ctx* ctx, int64_t n, int m, const double* const* Vre,
                            const double* const* Vim, double* wre, double* wim, double* coeffs);
/* One whole Arnoldi step of scipy's _fgmres (the inner loop of gcrotmk, numpyVector.py:161) with a single
 * host round trip: out = [ ||w||^2 before, h_0..h_{m-1}, ||w||^2 after ]; w is orthogonalised against
 * V_0..V_{m-1} one column after the other and then scaled by 1/||w|| when that is finite.  The pair form
 * works on complex vectors held as (re, im) buffers: h_j = conj(V_j).w as (re, im), out has 2m + 2 doubles. */
int hipeig_arnoldi_step(hipeig_ctx* ctx, int64_t n, int m, const double* const* V, double* w, double* out);
int hipeig_pair_arnoldi_step(hipeig_ctx* ctx, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                             double* wre, double* wim, double* out);

/* The same step with `cols_per_pass` columns per pass over w: 1 = the sequential sweep (scipy's order of rounding); 4 = a
 * pass applies four columns and forms the next four's products with the updated w together with their 4 x 4 Gram block,
 * from which the sequential coefficients follow exactly (h_k = <V_k,w> - sum_{l<k} h_l <V_k,V_l>): 2.5 instead of 4 vector
 * streams per column, a launch per four columns, coefficients equal to the sequential ones to rounding.            */
int hipeig_arnoldi_step_p(hipeig_ctx* ctx, int64_t n, int m, const double* const* V, double* w, double* out, int cols_per_pass);
int hipeig_pair_arnoldi_step_p(hipeig_ctx* ctx, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                               double* wre, double* wim, double* out, int cols_per_pass);

/* Split form of the pair step for several independent steps in a row (the right-hand sides of a lock-step block solve):
 * begin enqueues the step and an asynchronous copy of its 2m + 2 scalars into pinned slot `slot` (0..15, 2m + 2 <= 126),
 * end waits for the stream and copies `count` of them out.  One GPU only.                                         */
int hipeig_pair_arnoldi_step_begin(hipeig_ctx* ctx, int64_t n, int m, const double* const* Vre, const double* const* Vim,
                                   double* wre, double* wim, int cols_per_pass, int slot);
/* `count` (<= 16) such steps in ONE launch, a workgroup per step, for lengths at which a step is a single workgroup
 * (n <= 8192): step i has m[i] columns Vre[64 i + j], Vim[64 i + j], works on (wre[i], wim[i]) and reports into slot i
 * (collect with hipeig_arnoldi_step_end).  Returns 5, having done nothing, for longer vectors (take the step-by-step form). */
int hipeig_pair_arnoldi_step_batch_begin(hipeig_ctx* ctx, int64_t n, int count, const int* m, const double* const* Vre,
                                         const double* const* Vim, double* const* wre, double* const* wim);
int hipeig_arnoldi_step_end(hipeig_ctx* ctx, int slot, int count, double* out);
/* The real counterparts for the lock-step GCROT solves of a real shift (the nBlock solves of inexact_Lanczos.py:319-320,
 * each numpyVector.py:161's gcrotmk): begin reports m + 2 doubles [ ||w||^2 before, h_0..h_{m-1}, ||w||^2 after ] into
 * pinned slot `slot` (m + 2 <= 126), on the side streams and workspaces of the pair form; the batch runs up to 16 steps
 * of length n <= 8192 in one launch (step i: m[i] <= 64 columns V[64 i + j], vector w[i], slot i) and returns 5, having
 * done nothing, for longer vectors.  Collect either with hipeig_arnoldi_step_end.  One GPU only.                    */
int hipeig_arnoldi_step_begin(hipeig_ctx* ctx, int64_t n, int m, const double* const* V, double* w, int cols_per_pass, int slot);
int hipeig_arnoldi_step_batch_begin(hipeig_ctx* ctx, int64_t n, int count, const int* m, const double* const* V,
                                    double* const* w);

/* ---- sparse operator: replaces the scipy.sparse / ndarray H handed to the loop ----- */
/* Host CSR -> device.  rowptr has nrows+1 entries (local rows), col holds GLOBAL column
 * indices in [0, ncols).  Rows may be empty or unsorted; duplicates are summed by the
 * product.  row_offset = global index of local row 0 (row partition), used for the fused
 * shift term sigma*x[row].                                                               */
int hipeig_csr_create(hipeig_ctx* ctx, int64_t nrows, int64_t ncols, int64_t row_offset,
                      const int64_t* rowptr, const int32_t* col, const double* val,
                      hipeig_csr** out);
/* Seeded synthetic "gapped random-sparse Hermitian" operator generated on the device
 * (rows [row_begin,row_end) of the N x N matrix); bit-identical to
 * eigensolvers_amd.generators.gapped_csr_host.  params: see generators.py.               */
int hipeig_csr_generate(hipeig_ctx* ctx, int64_t N, int64_t row_begin, int64_t row_end,
                        int K, uint64_t seed, double eps, uint32_t keep_thresh24,
                        const double* targets, int ntargets, hipeig_csr** out);
int hipeig_csr_destroy(hipeig_ctx* ctx, hipeig_csr* A);
/* info[0]=nrows [1]=ncols [2]=nnz [3]=row_offset [4]=kernel variant of the last launch
 * (1 CSR-vector, 2 CSR-stream, 3/4 column-window blocked with wave / workgroup units)
 * [5]=device bytes [6]=row blocks [7]=kernel launches (sweeps) per product of that variant */
int hipeig_csr_info(hipeig_csr* A, int64_t info[8]);
/* layout constants of the blocked copy the last product ran on: out[0] variant, [1] rows per row block, [2] window bits,
 * [3] row blocks, [4] windows, [5] column splits, [6] workgroups per sweep launch, [7] threads per workgroup, [8] batch
 * unroll, [9] chunks of the operand exchange, [10] rows per (rank, chunk) of the gathered layout (0: not partitioned),
 * [11] log2 of the columns per bin + 100 when bins are aligned to 64-element instruction groups, [12] slots of the
 * workgroup-unit stream including padding (0 for the other variants)                                              */
int hipeig_csr_layout_info(hipeig_csr* A, int64_t out[13]);
/* copy the device CSR (local rows) back to the host; pass NULL to skip an array          */
int hipeig_csr_download(hipeig_ctx* ctx, hipeig_csr* A, int64_t* rowptr, int32_t* col,
                        double* val);
/* force a kernel variant (0 = automatic choice, 1..4 as above, 5 = variant 4 with fixed-point (int64) LDS
 * accumulators: bitwise reproducible whatever the order in which waves reach a row, same speed; absolute error per
 * row ~ nnz_row * 2^-61 * max_i sum_j|a_ij| * max|x|; 6 = dense row sweep on a row-major fp64 copy built on first
 * use - opt-in only, never the automatic choice; refused, not replaced, on an operator that is not whole and square, on a
 * context with a communicator and where the copy does not fit the free device memory).  7 is the Kronecker-sum operator's
 * and cannot be set: hipeig_kron_create pins it. */
int hipeig_csr_set_variant(hipeig_csr* A, int variant);
/* The dense H of the reference's own drivers and unit tests (numpyVector.py:100 `self.array = H @ self.array`, :152
 * `sigma*x - H@x` with H an ndarray): out[0] = rows, [1] = columns, [2] = doubles per row of the dense copy (columns
 * rounded up to a 128-byte line), [3] = bytes of the copy (0 until variant 6 / block variant 3 built it), [4] = rows a
 * wave carries per pass of the single-vector sweep, [5] / [6] = workgroups of the last dense single-vector / block
 * launch, [7] = 0 (reserved).                                                                                  */
int hipeig_csr_dense_info(hipeig_csr* A, int64_t out[8]);

/* ---- Kronecker-sum operator on a direct-product grid ---------------------------------------------------------
 * H = sum_d I (x) T_d (x) I + diag(V), N = n_1 * ... * n_D, vector index in C order (last mode fastest).  The reference
 * asks of an operator only H@x, H.shape and H.dtype (numpyVector.py:98-100 applyOp, :147-163 the linear operator of
 * solve, :180-189 matrixRepresentation), so its users hand over whatever applies fastest; for the vibrational
 * Hamiltonians in a product / DVR basis the method was written for (examples/stateFollowingHO.py) that is the factored
 * form.  The handle is an hipeig_csr (kernel variant 7, nnz = 0, an empty CSR behind it) and goes wherever a single
 * vector meets the operator: hipeig_spmv, hipeig_spmv_shift, hipeig_spmv_shift_pair, hipeig_minres, hipeig_minres_x0,
 * hipeig_minres_jacobi, hipeig_minres_shifts.  The block entry points (hipeig_spmm*, hipeig_minres_block*,
 * hipeig_lanczos_block_scalars, hipeig_lanczos_combine), hipeig_csr_diagonal and hipeig_dense_solve_small refuse it.
 * The adds of a row are in an order fixed by the dims alone (csrc/kron_device.h): bitwise reproducible.
 *
 * hipeig_kron_create (numpyVector.py:100 `H @ self.array`, :152/:154 `sigma*x - H@x`): 1 <= D <= 8 modes, dims[d] = n_d
 * with 1 <= n_d <= 208 and N < 2^31; factors[d] = T_d on the host, n_d x n_d row-major, applied as given (T_d[i][k], not
 * transposed, symmetric or not); diag = V on the host, N doubles, or NULL.  Refused with a message: a context with a
 * communicator, a factor the kernels do not take.  Device copies: the factors zero-padded to a multiple of 16 rows and 4
 * columns, V, and an N-double raw-sum buffer.                                                                      */
int hipeig_kron_create(hipeig_ctx* ctx, int D, const int64_t* dims, const double* const* factors, const double* diag,
                       hipeig_csr** out);
/* frees the Kronecker record and the handle (in place of hipeig_csr_destroy)                                       */
int hipeig_kron_destroy(hipeig_ctx* ctx, hipeig_csr* A);
/* What one `H @ x` (numpyVector.py:100) costs: out[0] = modes, [1] = N, [2] = kernel launches per product (one per mode
 * + the launch that carries the caller's row epilogue over the raw sums), [3] = device bytes, [4] = bytes of the raw-sum
 * buffer, [5] = largest n_d the kernels take; per mode d (0-based) out[8 + 4 d] = kernel form (1 = matrix cores, inner
 * stride >= 16; 2 = matrix cores, last mode; 3 = plain FMA: inner stride 2..15 or n_d = 1), [9 + 4 d] = n_d,
 * [10 + 4 d] / [11 + 4 d] = padded rows / columns of the device copy of T_d.                                       */
int hipeig_kron_info(hipeig_csr* A, int64_t out[40]);
/* d[r] = ((T_1[i_1][i_1] + T_2[i_2][i_2]) + ...) + V[r] (device pointer, N doubles): the diagonal of the Jacobi
 * preconditioner (scipy.sparse.linalg.minres(..., M=), the solve of numpyVector.py:163 with a preconditioner), in
 * the order in which the explicit matrix sums its terms.                                                          */
int hipeig_kron_diagonal(hipeig_ctx* ctx, hipeig_csr* A, double* d);
/* options["reduction"] = "deterministic" of the vectors: on != 0 restricts the AUTOMATIC choice
 * (variant 0) to bitwise reproducible kernels - CSR-stream where it would be picked anyway, variant 5 in place of 4,
 * the row-owner kernel for block products.  A pinned variant is not touched.                                      */
int hipeig_csr_set_reproducible(hipeig_csr* A, int on);
/* variant 5's error-bound ingredients: out[0] = max_i sum_j |a_ij| over the local rows, out[1] = max |x| of the
 * operand of the most recent variant-5 product; absolute error per row <= (nnz_row/2 + 1) * 2^-60 * out[0] * out[1] */
int hipeig_csr_fixed_info(hipeig_ctx* ctx, hipeig_csr* A, double out[2]);

/* applyOp, numpyVector.py:98-100: y = H x.  x,y are local slices.                        */
int hipeig_spmv(hipeig_ctx* ctx, hipeig_csr* A, const double* x, double* y);
/* the LinearOperator lambda of solve(), numpyVector.py:152/154:
 * y = sign*(sigma*x - H x), sign = +1 (Green's function) or -1 (reverseGF)               */
int hipeig_spmv_shift(hipeig_ctx* ctx, hipeig_csr* A, double sigma, double sign,
                      const double* x, double* y);
/* The same lambda for a COMPLEX shift and operand (feast.py:83-90 -> numpyVector.py:152-161 with sigma = z_k on the
 * contour; H real): y = sign*(z*x - H x) with x = xr + i xi, z = zr + i zi, y = yr + i yi, the halves in separate
 * buffers.  sign = 0: the plain product y = H x (applyOp on a complex vector, numpyVector.py:98-100).  On a large
 * unpartitioned operator both halves share ONE sweep of the (index, value) stream; otherwise two sweeps.
 * hipeig_csr_pair_info: out[0] = 1 when the most recent call took the one-sweep form, out[1] = its launches.       */
int hipeig_spmv_shift_pair(hipeig_ctx* ctx, hipeig_csr* A, double zr, double zi, double sign,
                           const double* xr, const double* xi, double* yr, double* yi);
int hipeig_csr_pair_info(hipeig_csr* A, int64_t out[2]);

/* The k applications of matrixRepresentation (numpyVector.py:184-185) as ONE block product:
 * Y[j] = H X[j], j < k.  Internally the operands are interleaved so that each non-zero costs
 * one index fetch and one contiguous gather for all k (tall-skinny SpMM).                   */
int hipeig_spmm(hipeig_ctx* ctx, hipeig_csr* A, int k, const double* const* X, double* const* Y);
/* The LinearOperator lambda of solve() (numpyVector.py:152,161) for the nBlock right-hand sides of one block Lanczos
 * iteration, which share operator and real shift (inexact_Lanczos.py:319-320): Y[j] = sign*(sigma*X[j] - H X[j]), j < k,
 * as block products whose epilogue applies the shift with hipeig_spmv_shift's roundings.  Kernel choice, chunking and
 * the contexts taken are those of hipeig_spmm.                                                                        */
int hipeig_spmm_shift(hipeig_ctx* ctx, hipeig_csr* A, int k, double sigma, double sign,
                      const double* const* X, double* const* Y);
/* The complex matvec of the contour solves for SEVERAL right-hand sides (feast.py:198-200: the m0 solves of a contour point
 * share operator and shift): Y_p = sign*(z*X_p - H X_p), p < npairs, the complex operands as (re, im) buffers.  Four operands
 * share one pass over the operator (an 8-wide block product whose epilogue applies the shift).                        */
int hipeig_spmm_shift_pairs(hipeig_ctx* ctx, hipeig_csr* A, int npairs, double zr, double zi, double sign,
                            const double* const* Xre, const double* const* Xim, double* const* Yre, double* const* Yim);
/* The same with one shift PER OPERAND: Y_p = sign*(z_p*X_p - H X_p), zr / zi host arrays of npairs shifts.  The solves of
 * all contour points of a FEAST iteration are independent (feast.py:189-200), so operands that belong to different points
 * may share a pass over the operator - the operator sum of a column does not depend on the shift, only the epilogue does.
 * Chunking (4 or 8 complex operands per pass), kernel choice and the fallbacks (npairs = 1, contexts with collectives:
 * hipeig_spmv_shift_pair per operand with that operand's shift) are those of hipeig_spmm_shift_pairs; so are the
 * roundings per element.                                                                                              */
int hipeig_spmm_shift_pairs_z(hipeig_ctx* ctx, hipeig_csr* A, int npairs, const double* zr, const double* zi, double sign,
                              const double* const* Xre, const double* const* Xim, double* const* Yre, double* const* Yim);

/* ---- diagonal right preconditioner of GCROT(m,k) (opt-in: linearSystemArgs["gcrotPreconditioner"] = "jacobi") ---- */
/* The reference calls scipy.sparse.linalg.gcrotmk without M (numpyVector.py:161; feast.py:83-90 for the contour points), so
 * these restate SciPy 1.15.3, not the reference: gcrotmk(A, b, M=diags(minv)) applies M on the right (_fgmres: z = M v,
 * w = A z), i.e. it is gcrotmk on the composed operator v -> A (minv (.) v) followed by x = minv (.) u.
 *
 * minv = 1 / (z - d[i]) for z = zr + i zi, kept away from a diagonal entry that meets z: with m_i = z - d[i], t_i = |m_i|
 * and g = floor_rel * max_j t_j it is 1 / m_i where t_i >= g, the phase of 1 / m_i at modulus 1 / g where 0 < t_i < g and
 * 1 / g where t_i == 0.  Unlike hipeig_jacobi_inverse it keeps sign and phase: GCROT needs no positive definite M.
 * zi == 0: a real minv, minv_im may be NULL (zeros are written when it is not); else minv_im is required.  Fails
 * (hipeig_last_error, "not finite") before anything is written when an element would not be finite (a d[i] equal to z
 * with floor_rel = 0), when d holds a non-finite value or when every t_i is 0.                                          */
int hipeig_jacobi_inverse_z(hipeig_ctx* ctx, int64_t n, const double* d, double zr, double zi, double floor_rel,
                            double* minv_re, double* minv_im);
/* y = m (.) x, element by element: SciPy's `M v` for M = diags(m) (and the closing x = M u).  y may be x.  Asynchronous. */
int hipeig_diag_mul(hipeig_ctx* ctx, int64_t n, const double* m, const double* x, double* y);
/* The same for complex x = xr + i xi and m = mr + i mi; mi == NULL: a real m.  (yr, yi) may be (xr, xi).               */
int hipeig_pair_diag_mul(hipeig_ctx* ctx, int64_t n, const double* mr, const double* mi, const double* xr, const double* xi,
                         double* yr, double* yi);
/* hipeig_spmm_shift (above) applied to T[j] = minv (.) X[j] - SciPy's w = A (M v) for the lock-step real-shift solves:
 * Y[j] = sign*(sigma*T[j] - H T[j]), T[j] formed with hipeig_diag_mul's element while the operands are packed, so the
 * result is hipeig_spmm_shift's on hipeig_diag_mul's output.  A whole square operator on a context without collectives. */
int hipeig_spmm_shift_m(hipeig_ctx* ctx, hipeig_csr* A, int k, double sigma, double sign, const double* minv,
                        const double* const* X, double* const* Y);
/* hipeig_spmm_shift_pairs_z (above) applied to t_p = Minv_p (.) x_p with a minv PER OPERAND (Mre[p], Mim[p]; Mim[p] may
 * be NULL), so that operands of different contour points still share a pass over the operator: Y_p = sign*(z_p*t_p - H t_p),
 * t_p formed with hipeig_pair_diag_mul's element while the operands are packed.  Chunking, width rule and sweeps are those
 * of hipeig_spmm_shift_pairs_z; npairs == 1 is hipeig_pair_diag_mul, then hipeig_spmv_shift_pair.  A whole square
 * operator on a context without collectives.                                                                          */
int hipeig_spmm_shift_pairs_zm(hipeig_ctx* ctx, hipeig_csr* A, int npairs, const double* zr, const double* zi, double sign,
                               const double* const* Mre, const double* const* Mim,
                               const double* const* Xre, const double* const* Xim, double* const* Yre, double* const* Yim);

/* Kernel choice of the block product / block solve: 0 = automatic, 1 = row-owner CSR (a wavefront per row,
 * 64-byte gathers from wherever the operand block lives), 2 = column-window blocked (operand windows
 * L2-resident, 8 accumulators per row in LDS), 3 = dense block sweep on the dense copy of variant 6 (opt-in only,
 * refused under the same conditions).  info[0] = variant of the last block launch, [1] = row
 * blocks, [2] = column windows, [3] = rows per row block of the window-blocked layout.              */
int hipeig_csr_set_block_variant(hipeig_csr* A, int variant);
int hipeig_csr_block_info(hipeig_csr* A, int64_t info[4]);

/* ---- inner linear solve: NumpyVector.solve with linearSolver="minres" (:147-178) ---- */
/* Solves sign*(sigma*I - H) x = b from a zero initial guess with the Paige-Saunders
 * MINRES recurrences in the evaluation order of scipy.sparse.linalg.minres (the call at
 * numpyVector.py:163), all vectors and recurrence scalars device-resident.
 * out_stats: [0]=iterations [1]=istop (SciPy's code) [2]=rnorm estimate [3]=Anorm
 *            [4]=ynorm [5]=test1 [6]=test2 [7]=Acond.
 * *info follows SciPy: maxiter if the iteration limit was hit (istop==6) else 0.         */
int hipeig_minres(hipeig_ctx* ctx, hipeig_csr* A, double sigma, double sign, const double* b,
                  double* x, double rtol, int maxiter, int* info, double out_stats[8]);
/* The same with SciPy's initial guess (numpyVector.py:163 hands x0 on to scipy.sparse.linalg.minres): r1 = b - A x0,
 * the iterate starts at x0.  x0 == NULL is hipeig_minres.  The reference's solvers never pass one
 * (inexact_Lanczos.py:99, feast.py:90-97); the parameter is part of NumpyVector.solve's signature.            */
int hipeig_minres_x0(hipeig_ctx* ctx, hipeig_csr* A, double sigma, double sign, const double* b,
                     const double* x0, double* x, double rtol, int maxiter, int* info,
                     double out_stats[8]);

/* ---- Jacobi-preconditioned MINRES (opt-in: linearSystemArgs["preconditioner"] = "jacobi") ---- */
/* The reference passes no preconditioner (numpyVector.py:163 calls scipy.sparse.linalg.minres without M), so these three
 * restate SciPy, not the reference: scipy.sparse.linalg.minres(A, b, M=diags(minv)) of SciPy 1.15.3.
 *
 * d[i] = sum of the stored (i, i) entries of local row i in stored order (duplicate (row, col) entries are separate stored
 * elements), 0 when the row stores none: what scipy.sparse's A.diagonal() returns.  On a row slice the diagonal column of
 * local row i is row_offset + i.  Asynchronous.                                                                    */
int hipeig_csr_diagonal(hipeig_ctx* ctx, hipeig_csr* A, double* d);
/* minv[i] = 1 / max(t_i, floor_rel * max_j t_j) with t_i = |sigma - d[i]|: the inverse of the diagonal of |sigma*I - H|
 * (Davidson's correction), the M^-1 that SciPy's minres takes as `M`.  Fails (hipeig_last_error) instead of writing when
 * an element would not be finite: a d[i] equal to sigma with floor_rel = 0, a non-finite d[i].                        */
int hipeig_jacobi_inverse(hipeig_ctx* ctx, int64_t n, const double* d, double sigma, double floor_rel,
                          double* minv);
/* hipeig_minres with SciPy's M: the Lanczos vectors are built from z = minv (.) r2 and beta^2 = <r2, z>, so rtol is tested
 * in SciPy's preconditioned quantities (beta1 = sqrt(<b, M^-1 b>), rnorm = phibar in the M^-1 norm).  info and out_stats
 * as in hipeig_minres.  One GPU, whole vectors, a square operator: a context with collectives is refused.          */
int hipeig_minres_jacobi(hipeig_ctx* ctx, hipeig_csr* A, double sigma, double sign, const double* b,
                         const double* minv, double* x, double rtol, int maxiter, int* info,
                         double out_stats[8]);

/* ---- separable preconditioner of the Kronecker-sum operator (opt-in: linearSystemArgs["preconditioner"] = "separable") ----
 * SciPy's minres(A, b, M=...) again, with the fast-diagonalisation M^-1 = Q S Q^T: H = H0 + W with the separable part
 * H0 = sum_d I (x) (T_d + diag(v_d)) (x) I, T_d + diag(v_d) = Q_d diag(lam_d) Q_d^T decomposed on the host, Q = Q_1 (x)
 * ... (x) Q_D, S = diag(sinv), sinv_r = 1 / max(|sigma - Lam_r|, floor_rel * max |sigma - Lam|), Lam_r = sum_d lam_d[i_d].
 * Symmetric positive definite for any orthogonal Q_d.  The reference passes no M (numpyVector.py:163).
 *
 * hipeig_kron_precond_create: A is the operator of hipeig_kron_create and D, dims are its own; bases[d] = Q_d on the host,
 * n_d x n_d row-major, eigenvalues[d] = lam_d, n_d doubles.  Device copies: Q_d and Q_d^T zero-padded to a multiple of 16
 * rows and 4 columns, as the operator's factors, and the lam_d tables.  An apply keeps no vector of its own: it works in
 * the operator's raw-sum buffer, which is free between two products, and in its output.                            */
typedef struct hipeig_kron_precond hipeig_kron_precond;
int hipeig_kron_precond_create(hipeig_ctx* ctx, hipeig_csr* A, int D, const int64_t* dims, const double* const* bases,
                               const double* const* eigenvalues, hipeig_kron_precond** out);
int hipeig_kron_precond_destroy(hipeig_ctx* ctx, hipeig_kron_precond* P);
/* out[0] = modes, [1] = N, [2] = launches per apply (2 D), [3] = device bytes of the tables, [4] = launches a
 * preconditioned iteration adds to the plain one (2 D + 1); per mode d (0-based) out[8 + 4 d] = kernel form (as
 * hipeig_kron_info), [9 + 4 d] = n_d, [10 + 4 d] / [11 + 4 d] = padded rows / columns of the device copies.       */
int hipeig_kron_precond_info(hipeig_kron_precond* P, int64_t out[40]);
/* sinv (device pointer, N doubles, not the operator's raw-sum buffer): Lam_r = ((lam_1[i_1] + lam_2[i_2]) + ...) in mode
 * order, then hipeig_jacobi_inverse on it, with its refusal of an element that would not be finite.               */
int hipeig_kron_precond_scale(hipeig_ctx* ctx, hipeig_kron_precond* P, double sigma, double floor_rel, double* sinv);
/* one mode alone, out of place: z[o][i][j] = sum_k Q_d[i][k] x[o][k][j] (transpose != 0: Q_d[k][i]), d 0-based.   */
int hipeig_kron_precond_transform(hipeig_ctx* ctx, hipeig_kron_precond* P, int d, int transpose, const double* x,
                                  double* z);
/* z = Q (sinv (.) (Q^T x)): the modes 1..D with Q_d^T, the last of them storing sinv (.) sum, then the modes 1..D with
 * Q_d; 2 D launches.  x, z and the operator's raw-sum buffer are three different vectors; x is only read.         */
int hipeig_kron_precond_apply(hipeig_ctx* ctx, hipeig_kron_precond* P, const double* sinv, const double* x, double* z);
/* hipeig_minres_jacobi with this M^-1: z = M^-1 r2 from an apply per iteration, beta^2 = <r2, z>; rtol, info and
 * out_stats as there.  One GPU, no x0, no captured graph; 3 D + 3 launches per iteration.                         */
int hipeig_minres_kron_separable(hipeig_ctx* ctx, hipeig_csr* A, hipeig_kron_precond* P, const double* sinv,
                                 double sigma, double sign, const double* b, double* x, double rtol, int maxiter,
                                 int* info, double out_stats[8]);

/* linearSolver = "pardiso" (numpyVector.py:166-170: spsolve of sigma*I - H, kept by the reference "only for comparing
 * with fortran" - the 4 x 4 known-answer system of unittests/test_feast_fortran.py): x = (sign*(z I - H))^-1 b by
 * Gaussian elimination with partial pivoting in the LDS of one workgroup, n <= 96, z = zr + i zi.  b_im and x_im may be
 * NULL for a real system (zi == 0).  *singular != 0: a zero pivot column, x is not written.                    */
int hipeig_dense_solve_small(hipeig_ctx* ctx, hipeig_csr* A, double zr, double zi, double sign,
                             const double* b_re, const double* b_im, double* x_re, double* x_im,
                             int* singular);

/* The nBlock solves of one block-Lanczos iteration (inexact_Lanczos.py:319-320: one NumpyVector.solve
 * per block vector, same operator, same shift) advanced in lock step: k <= 8 right-hand sides, ONE block
 * product per iteration.  Column j runs exactly the recurrences and stopping tests of hipeig_minres on
 * b[j]; a column that has stopped is masked, so x[j] is the iterate SciPy would return for it.
 * info[j] as in hipeig_minres; out_stats (may be NULL) receives k records of 8 doubles.             */
int hipeig_minres_block(hipeig_ctx* ctx, hipeig_csr* A, double sigma, double sign, int k,
                        const double* const* b, double* const* x, double rtol, int maxiter,
                        int* info, double* out_stats);

/* hipeig_minres_block with SciPy's M = diag(1 / minv) (opt-in: linearSystemArgs["preconditionerLockStep"]): column j runs
 * the recurrences and stopping tests of hipeig_minres_jacobi on b[j] - z = minv (.) r2, beta^2 = <r2, z>, rtol tested in
 * the preconditioned quantities - on interleaved blocks, one block product per iteration; a column with <b, minv (.) b>
 * == 0 returns x = 0 after 0 iterations, a negative or not-a-number one fails.  minv: hipeig_jacobi_inverse's vector
 * (n doubles), shared by the columns.  info and out_stats as in hipeig_minres_block.  One GPU, whole vectors, a square
 * operator: a context with collectives is refused.                                                                */
int hipeig_minres_block_jacobi(hipeig_ctx* ctx, hipeig_csr* A, double sigma, double sign, int k,
                               const double* const* b, const double* minv, double* const* x,
                               double rtol, int maxiter, int* info, double* out_stats);

/* Shifted MINRES: sign*(z_j I - H) x_j = b for nshift (1..8) shifts z_j = zr[j] + i zi[j] - real (zi = 0) or complex -
 * of one real symmetric operator and one real right-hand side, all from ONE Lanczos run on H: one operator product per
 * step whatever nshift is.  Each shift keeps a complex rotation recurrence and a three-term direction update, its
 * residual norm |tau_j| is minimal over the Krylov space, and it stops after the step at which
 * |tau_j| <= max(atol, rtol*||b||) (SciPy gcrotmk's criterion); its x_j is then left alone.  x_re[j] / x_im[j]: the
 * halves of x_j (n doubles each, overwritten).  info[j] = 0, or maxiter when shift j was still live there.
 * out_stats (may be NULL): nshift records of 4 doubles - steps of shift j, |tau_j|, operator products of the run, 0.
 * One GPU, whole vectors: a context with collectives is refused.                                                  */
int hipeig_minres_shifts(hipeig_ctx* ctx, hipeig_csr* A, double sign, int nshift, const double* zr,
                         const double* zi, const double* b, double* const* x_re, double* const* x_im,
                         double rtol, double atol, int maxiter, int* info, double* out_stats);

/* FEAST's filtered vectors without any per-shift vector (feast.py:189-200 only forms q = sum_k Re(c_k x_k) of its contour
 * solves; every x_k lies in the Krylov space of one real Lanczos basis, so q = sum_i g_i v_i with real g_i that follow from
 * the Lanczos tridiagonal).  PASS 1: the Lanczos recurrence of k (1..8) real right-hand sides in lock step on interleaved
 * block products, and per (column, shift) the rotation recurrence and stop rule of hipeig_minres_shifts for nshift (1..32)
 * shifts of sign*(z I - H) - scalars only.  alphas: k rows of maxiter doubles, betas: k rows of maxiter + 1 (betas[0] =
 * ||b||; step i, 0-based, yields alphas[i] and betas[i + 1]); iterations / estimates: k rows of nshift (stop step, |tau|);
 * info[j] = 0, or maxiter when a shift of column j was still live there.  out_stats (may be NULL): 1 + k doubles - block
 * products of the run, then the steps each column ran.  One GPU, whole vectors: a context with collectives is refused.
 *
 * basis_mode 0: the vectors live in a ring of three; basis_bytes is not read and basis may be NULL.
 * basis_mode 1 (lanczos_filter.py, lanczos_run(keepBasis=True)): the vectors are KEPT in device memory - step k's new
 * vector goes to slot k + 1 of a basis carved from segments allocated while the run advances (HIPEIG_LF_SEGMENT slots each,
 * default 32) instead of over the oldest ring buffer: the same kernels on the same operands, so every result equals mode
 * 0's (bit for bit with the row-owner sweep).  basis_bytes: byte budget of the segments.  When the next segment would
 * exceed it, or the device has no room, the run goes on in the ring and *basis is NULL (not an error); otherwise *basis
 * owns the vectors until hipeig_lanczos_basis_release.
 * basis_mode 2 (keepPrefix=True): as mode 1 while segments can be had.  When the next segment is refused the segments held
 * stay and are written to their last slot - p = segments * slots vectors - and from step p - 1 on the new vector goes to
 * the ring; steps p - 1 and p read their operands from the slots, so kernels, operands and scalars are still mode 0's.
 * The basis then holds min(steps of column j, p) vectors per column.  A run that stops before p ends as a whole basis;
 * *basis is NULL only when not even the first segment fits.  The workspace of the pass 2 that follows (nc <= 2) is reserved
 * before the first segment.
 * basis_mode 3 / 4 (basisPrecision="fp32"): modes 1 / 2 with the basis stored in fp32, twice the vectors per byte.  The
 * recurrence runs in the fp64 ring of three exactly as mode 0 (the same scalars), and the kernel that finishes step k's
 * vector also leaves it, rounded to nearest even, in slot k + 1 (slot 0: b): 4 n K more bytes written per step.  A slot is
 * n K floats (padded to 32), so a segment is half the bytes.  Mode 3: a refused segment frees the basis, *basis is NULL.
 * Mode 4: the slots held stay, and r_{p-1}, r_{p-2} are copied in fp64 to two hand-over vectors the basis owns, from which
 * pass 2's recurrence restarts (rounded start vectors would not repeat pass 1's arithmetic).  basis_bytes is the budget of
 * the segments; the hand-over vectors (16 bytes per padded element of a slot) come on top and are freed, not pooled.   */
typedef struct hipeig_lanczos_basis hipeig_lanczos_basis;
int hipeig_lanczos_block_scalars(hipeig_ctx* ctx, hipeig_csr* A, double sign, int k, const double* const* b,
                                 int nshift, const double* zr, const double* zi, double rtol, double atol,
                                 int maxiter, double* alphas, double* betas, int* iterations, double* estimates,
                                 int* info, double* out_stats, int basis_mode, int64_t basis_bytes,
                                 hipeig_lanczos_basis** basis);
/* PASS 2 of the same (lanczos_filter.py, LanczosRun.combine): q[j*nc + c] = sum_{i < m[j]} G[j][i*nc + c] v_i for c < nc, with
 * pass 1's scalars (alphas[j], betas[j]: host arrays of at least m[j] and m[j] + 1 doubles); q: k*nc vectors of n doubles,
 * overwritten.  Column j stops after its own m[j] terms, at most the steps it ran.  With mmax = max_j m[j]:
 *   basis NULL: the Lanczos vectors are rebuilt from b (k columns, read only here; q must not alias them) by the
 *     recurrence - no dot products - and the sums accumulated in the block product's epilogue, nc = 1 or 2; the last term
 *     needs no product: mmax - 1 block products;
 *   a basis that holds p >= mmax vectors: one stream over the stored vectors v_i = r_i / betas[j][i], nc = 1, 2, 4 or 8,
 *     no product, any number of calls per basis; k must be the basis's column count and A the operator it was kept for;
 *   a basis that holds p < mmax: the stream takes the terms i < p - 1, r_{p-2} and r_{p-1} are copied out of their slots
 *     (the basis is never written) and the recurrence runs from step p - 1: mmax - p block products.
 * An fp32 basis (basis_mode 3 / 4) is taken the same way: the stream widens every stored element to fp64 and then makes
 * the same operations in the same order, so each q differs from the fp64 basis's by at most 2^-24 sum_i |G[j][i]| ||v_i||
 * over the stream's terms; the recurrence behind a prefix starts from the fp64 hand-over vectors.
 * out_stats[0] (may be NULL) = block products made.  Every element meets the same operations in the same order in the
 * three situations: with the row-owner sweep the results are equal bit for bit.                                        */
int hipeig_lanczos_combine(hipeig_ctx* ctx, hipeig_csr* A, const hipeig_lanczos_basis* basis, int k,
                           const double* const* b, const int* m, const double* const* alphas,
                           const double* const* betas, int nc, const double* const* G, double* const* q,
                           double* out_stats);
/* What a kept basis holds (lanczos_filter.py, LanczosRun.basis_bytes and default_basis_budget): info[0] vectors kept (the
 * largest column's; behind a prefix at most its p), [1] bytes held: its segments, and the two fp64 hand-over vectors of an fp32 prefix, [2] interleave width K, [3] rows, [4] columns, [5] bytes of released
 * segments the context would hand out again, [6] segments, [7] slots per segment.  basis may be NULL: only [5] is set. */
int hipeig_lanczos_basis_info(hipeig_ctx* ctx, const hipeig_lanczos_basis* basis, int64_t info[8]);
/* Bytes of one stored element of a kept basis: *out = 8, or 4 for basis_mode 3 / 4; 0 when basis is NULL. */
int hipeig_lanczos_basis_element_bytes(hipeig_ctx* ctx, const hipeig_lanczos_basis* basis, int* out);
/* Give a kept basis's segments back to the context for reuse (lanczos_filter.py, LanczosRun.release); basis may be NULL.
 * The context frees them when an allocation fails and when it is destroyed.                                           */
int hipeig_lanczos_basis_release(hipeig_ctx* ctx, hipeig_lanczos_basis* basis);

/* ---- timing on the library's compute stream (HIP events) --------------------------- */
int hipeig_timer_start(hipeig_ctx* ctx);
int hipeig_timer_stop(hipeig_ctx* ctx, float* elapsed_ms);   /* synchronous */

#ifdef __cplusplus
}
#endif
#endif /* HIPEIG_H */
