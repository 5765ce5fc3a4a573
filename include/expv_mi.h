/* expv_mi.h -- C ABI of libexpv_mi.so: MI355X-native Krylov exp(tA)v engine.
 *
 * Drop-in boundary for the Krylov path of SciML/ExponentialUtilities.jl (v1.35.0).
 * The reference has no FFI for this path (it is pure Julia; its extension points are
 * multiple dispatch on the operator / array types, docs/src/interfaces.md:7-36).  Each entry
 * point below names the reference method a Julia shim forwards to it with `ccall`
 * (INTEGRATION.md shows the binding).  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - every function returns an expv_mi_status (0 = OK) and never throws / longjmps;
 *     expv_mi_last_error(ctx) returns the message of the last failure on that context;
 *   - all matrices are COLUMN-MAJOR with an explicit leading dimension (Julia layout);
 *   - dtype: EXPV_MI_F64 = double, EXPV_MI_C64 = interleaved (re,im) double pairs;
 *   - *_loc says where a caller buffer lives: EXPV_MI_HOST (library stages it through
 *     HBM) or EXPV_MI_DEVICE (a HIP device pointer on the context's device);
 *   - the caller owns every buffer it passes; the library owns what is behind handles;
 *   - a handle is not thread-safe; distinct contexts are independent; calls are
 *     synchronous on return (host-visible outputs are valid).
 */
#ifndef EXPV_MI_H
#define EXPV_MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct expv_mi_ctx_s *expv_mi_ctx_t;
typedef struct expv_mi_op_s *expv_mi_op_t;
typedef struct expv_mi_ks_s *expv_mi_ks_t;
typedef struct expv_mi_comm_s *expv_mi_comm_t;      /* an RCCL communicator bound to a context (final gather of a sharded batch) */
typedef struct expv_mi_tscache_s *expv_mi_tscache_t;

typedef enum {
  EXPV_MI_OK = 0,
  EXPV_MI_DIMENSION_MISMATCH = 1, /* DimensionMismatch, arnoldi.jl:217-218                  */
  EXPV_MI_ARGUMENT_ERROR = 2,     /* ArgumentError, krylov_phiv.jl:132,221                   */
  EXPV_MI_ASSERTION = 3,          /* @assert "Dimension mismatch", krylov_phiv.jl:205,625    */
  EXPV_MI_SINGULAR = 4,           /* SingularException, exp_baseexp.jl:54-56                 */
  EXPV_MI_UNSUPPORTED = 5,        /* error(...), krylov_phiv_error_estimate.jl:97,164        */
  EXPV_MI_OUT_OF_MEMORY = 6,
  EXPV_MI_HIP_ERROR = 7,
  EXPV_MI_BOUNDS = 8              /* BoundsError (kiops.jl:303 with several output times)    */
} expv_mi_status;

/* Element types = the reference's BlasFloat (ExponentialUtilities.jl:19).  F64 / C64: every entry point, every step form.
 * F32 / C32: operators, KrylovSubspace (T and U of one precision), arnoldi! / lanczos!, expv! / phiv! / combine, expv,
 * the error-estimate mode, phiv_timestep!, mul!, and the host small-dense functions -- computed natively on 32-bit storage
 * (4 / 2 rows per 16-byte pack: half the HBM traffic), with the projection sums accumulated in fp64 and the host's small
 * exponentials in fp64; they run the two-kernel step and the modular launches (the single-pass step is 64-bit only).
 * expv_mi_kiops (reference method Float64-only, kiops.jl:89) and expv_mi_expv_batch answer EXPV_MI_UNSUPPORTED for F32 / C32. */
typedef enum { EXPV_MI_F64 = 0, EXPV_MI_C64 = 1, EXPV_MI_F32 = 2, EXPV_MI_C32 = 3 } expv_mi_dtype;
typedef enum { EXPV_MI_HOST = 0, EXPV_MI_DEVICE = 1 } expv_mi_loc;

/* Orthogonalisation arithmetic of arnoldi_step! (arnoldi.jl:301-304).
 *   MGS    : the reference's literal sequence (dot -> axpy, one column at a time).
 *   LOWSYNC: the same projection written as  h = (I + L)^-1 V^H y  (L = strict lower triangle
 *            of V^H V), which is algebraically identical to MGS on the computed basis but needs
 *            one grid-wide reduction per Krylov step instead of one per column.
 *   AUTO   : LOWSYNC whenever the window holds at least 2 columns (a 1-column window is MGS). */
typedef enum { EXPV_MI_ORTHO_AUTO = 0, EXPV_MI_ORTHO_MGS = 1, EXPV_MI_ORTHO_LOWSYNC = 2,
               /* OPT-IN, not the reference's arithmetic: lanczos! for a Hermitian banded Float64 operator as a PIPELINED recurrence (csrc/lanczos_pl.hip)
                * -- alpha_j, beta_j from inner products "by expansion", reduced one pass behind the pass that needs nothing of them, the whole
                * factorisation one resident kernel.  Stated bars (tests/test_gpu_parity.py::test_pipelined_lanczos_*): expv!(w, t, Ks) within 1e-11 of
                * the reference recurrence's, H within 1e-11 of its largest entry while the reference's own basis keeps its orthogonality; happy
                * breakdown detected down to ~1e-7 |A| only.  Where it does not apply (not Hermitian, not banded fp64, augmented, a continuation,
                * m > 128) the call runs the default path; expv_mi_expv_stats.path_flags says which ran (EXPV_MI_PATH_PIPELINED_LANCZOS). */
               EXPV_MI_ORTHO_PIPELINED = 3 } expv_mi_ortho;

/* ------------------------------------------------------------------ context ---------- */
/* One context = one GPU + one HIP stream.  `stream` may be NULL (library creates its own) or an
 * existing hipStream_t (e.g. torch.cuda.Stream().cuda_stream) that the library launches on and never destroys: calls stay behind
 * what the caller queued on it before, device outputs are valid for what the caller queues on it afterwards.  NULL always means
 * "a private stream", so the null / legacy stream (handle 0, e.g. torch.cuda.default_stream().cuda_stream) cannot be adopted --
 * a host that wants the library on torch's stream creates one (torch.cuda.Stream()) and passes that; the Python front end raises
 * ValueError for a handle of 0 instead of creating a private stream behind the caller's back. */
int expv_mi_ctx_create(int device_id, void *stream, expv_mi_ctx_t *ctx);
int expv_mi_ctx_destroy(expv_mi_ctx_t ctx);
int expv_mi_ctx_sync(expv_mi_ctx_t ctx);
/* Device-resident outputs (w of expv!/phiv!, ...) are complete when a call returns (default), or -- on != 0 --
 * stream-ordered like any HIP library: valid for later work on the context's stream, or after
 * expv_mi_ctx_sync.  Host outputs are always complete on return.  Lets consecutive calls overlap the host part
 * of one with the last kernel of the previous one. */
int expv_mi_ctx_set_async_outputs(expv_mi_ctx_t ctx, int on);
/* Banded pipeline: run consecutive Krylov steps on two streams so that a step's kernel starts while the previous
 * one finishes (default on).  Off: one launch after the other on the context's stream -- same results; per-kernel
 * durations are then meaningful to a profiler. */
int expv_mi_ctx_set_pipeline_overlap(expv_mi_ctx_t ctx, int on);
/* Engine options of a context, by name (A/B switches and limits; every one has a default that is right for production):
 *   "pipeline" 1        single-pass Krylov step for banded / structured-grid operators (0: two-kernel step instead)
 *   "wave" 1            its wave form for operators too wide for a halo recompute
 *   "fused" 1           single-reduction two-kernel step for regular-row sparse operators (0: modular launches)
 *   "fused_two_reductions" 0   the older two-reduction form of that step
 *   "dia" 1             diagonal storage forms instead of SELL slots where the pattern allows
 *   "mailbox" 1         Hessenberg / state to the host through host-mapped memory instead of a copy + stream sync
 *   "pipeline_serial" 0 single-pass step one launch after the other (like expv_mi_ctx_set_pipeline_overlap(ctx, 0))
 *   "spin_limit" 400000 polls before a waiting kernel gives up and the host redoes the factorisation without waits
 *   "batch_rounds" 2    batched single-pass step: resident rounds of fat workgroups
 *   "nontemporal" -1    single-pass step: non-temporal loads of the streamed operands: -1 when a step's footprint is far
 *                       beyond the 256 MiB Infinity Cache (> 480 MB), 0 never, 1 always; results do not depend on it
 *   "stencil" 0         banded fp64 operators whose stored diagonals are constant (constant-coefficient finite differences): apply
 *                       them from scalars instead of streaming the diagonals (bitwise the same result, 40 % less operator-side
 *                       traffic on a 5-diagonal operator); off by default so that a general sparse operator is timed as one
 *   "elide" 1           banded fp64 operators, halo form of the single-pass step: a stored diagonal that holds ONE value on a whole tile of
 *                       512 rows (found per tile and diagonal at creation and at every values update, expv_mi_op_elide_info) is read
 *                       there as one entry instead of being streamed; bitwise the same result.  0: stream everything (EXPV_MI_ELIDE=0).
 *                       "stencil" 1 on a wholly constant operator takes precedence
 *   "recycle" 1         expv_mi_ks_destroy keeps the storage of the subspace (one per context) and the next expv_mi_ks_create of
 *                       the same shape takes it over, reset to the freshly built state: the create-use-destroy pattern of the
 *                       convenience methods costs no hipMalloc / hipFree.  0: destroy frees at once
 *   "ee_blocked" 1      error-estimate mode: blocks of Lanczos steps through the ordinary factorisation, every step of a block
 *                       tested on the host when the block is there; 0: one step at a time (same stopping step, same result)
 *   "reorder" 1         sparse operators with no single-pass form in their natural ordering: 1 = try a bandwidth-reducing
 *                       ordering (reverse Cuthill-McKee) at creation and keep P A P' when it gives one; 0 = never; 2 = always keep it
 *                       (expv_mi_op_reorder_info says what happened; read when an operator is created)
 *   "patch" 1           2-D grid stencils (every offset within 2 of 0 or of +-k): 1 = stored in a grid-patch ordering at creation, the
 *                       single-pass step runs in its patch form (a tile = a 16 x 32 patch of the grid, the ring of rows around it
 *                       recomputed: no per-tile flags); 0 = natural ordering, wave form (expv_mi_op_patch_info; read when an
 *                       operator is created)
 *   "matfree_fused" 0   matrix-free operators (expv_mi_op_create_callback): 0 (default since round 6) = the modular path -- mul!(y, A, v_j) on
 *                       the NORMALISED column like the reference (arnoldi.jl:185), then projection, update, scale as separate launches;
 *                       1 = the two-kernel step: the callback is applied to the un-normalised u_j = beta_{j-1} v_j and its y~ goes straight
 *                       into the step's first kernel (one reduction, two launches + the callback per step).  1 is for LINEAR callbacks
 *                       only: a finite-difference Jacobian-vector product (f(u + eps v) - f(u)) / eps with eps tuned for |v| = 1 loses
 *                       accuracy on a scaled argument
 *   "fa2_pipelined" 1   two-kernel step on SELL slots: every independent request of a slice (operator slots, this row pack of u_j, the first
 *                       window columns) is issued up front: three dependent round trips per slice instead of seven (real element types;
 *                       random columns at n = 1e6: 3.40 -> 3.15 ms per expv); 0 = the earlier loop.  Results agree to rounding
 *   "kiops_skip_redo" 1 kiops after a rejected sub-step continues behind the closing pass of the factorisation it rejected (init = j + 1)
 *                       instead of recomputing step j as the reference's loop `for j in init:m` does (arnoldi.jl:368 -- the same H[:, j]
 *                       and v_{j+1} again); the statistics tuple is the reference's; 0 = recompute
 *   "resident" 0        whole factorisation as ONE cooperative kernel with part of the operand kept in LDS (experimental:
 *                       correct, slower than the default on every shape measured; kept for A/B)
 * A new context takes its defaults from the environment variables EXPV_MI_NO_PIPE, _NO_WAVE, _NO_FUSED, _FUSED_V1, _NO_DIA,
 * _NO_MAILBOX, _PIPE_SERIAL, _PIPE_SPIN_LIMIT, _BATCH_ROUNDS, _NONTEMPORAL, _RESIDENT, _STENCIL, _NO_RECYCLE, _EE_STEPWISE, _REORDER, _PATCH (read once, at creation) -- nothing reads the environment later.
 * Unknown names return EXPV_MI_ARGUMENT_ERROR. */
int expv_mi_ctx_set_option(expv_mi_ctx_t ctx, const char *name, int64_t value);
int expv_mi_ctx_get_option(expv_mi_ctx_t ctx, const char *name, int64_t *value);
/* Cumulative counters of a context: out[0] Krylov steps (operator applications inside arnoldi!/lanczos!), [1] factorisations,
 * [2] of those on the single-pass pipeline, [3] of those with overlapped steps, [4] factorisations redone one launch after
 * the other because a bounded device wait expired (device shared with other work), [5] redone on the two-kernel step because
 * the wave form's tile wait expired, [6] operator applications outside a factorisation (phiv_timestep!'s recurrence, mul!),
 * [7] factorisations whose H and state came home by copy + stream synchronisation instead of through the host mailbox (option
 * mailbox = 0, or a step form without one).  A non-zero [4] / [5] means the overlapped / wave form was switched off for the following 64 calls. */
int expv_mi_ctx_counters(expv_mi_ctx_t ctx, int64_t out[8]);
/* EXPV_MI_PATH_* flags of the most recent factorisation on the context -- what expv_mi_expv_stats.path_flags reports for a whole-call
 * expv, for expv_mi_arnoldi / expv_mi_lanczos / the drivers too (0: none yet). */
int expv_mi_ctx_last_path(expv_mi_ctx_t ctx, int32_t *path_flags);
/* Device self-test: the cross-lane sums of the kernels run on v_permlane32/16_swap + DPP (no LDS round trip); this runs them
 * against the LDS-permute (shuffle) forms on random values and returns the number of lanes whose result differs in ANY bit:
 * out[0] single exchanges (distances 32 .. 1), [1] 64-lane butterfly total, [2] 32-lane butterfly total, [3] lane 0 of the
 * wave total against the shift-down tree, [4] multi-value recursive halving (2, 4, 8, 16 values), [5] the same for 32
 * values, [6..7] reserved.  All zero on a device the library is built for. */
int expv_mi_ctx_selftest(expv_mi_ctx_t ctx, int64_t out[8]);
/* path flags of the most recent factorisation (also returned in expv_mi_expv_stats.path_flags) */
enum {
  EXPV_MI_PATH_MODULAR = 1, EXPV_MI_PATH_TWO_KERNEL = 2, EXPV_MI_PATH_PIPELINE = 4, EXPV_MI_PATH_WAVE = 8,
  EXPV_MI_PATH_OVERLAPPED = 16, EXPV_MI_PATH_REDO_SERIAL = 32, EXPV_MI_PATH_REDO_WAVE_OFF = 64,
  EXPV_MI_PATH_RESIDENT = 128,  /* the whole factorisation ran as one resident (cooperative) kernel */
  EXPV_MI_PATH_PATCH = 256,     /* single-pass step, patch form: operator stored in a grid-patch ordering, ring recomputed */
  EXPV_MI_PATH_PIPELINED_LANCZOS = 512,     /* the opt-in pipelined Lanczos recurrence ran (EXPV_MI_ORTHO_PIPELINED) */
  EXPV_MI_PATH_FA2_PIPELINED = 1024,        /* two-kernel step: its first kernel ran in the requests-up-front instantiation (option fa2_pipelined; real types, SELL slots) */
  EXPV_MI_PATH_REAL_OPERATOR = 2048         /* a mixed call: a real operator read in its own type under a complex subspace (see expv_mi_arnoldi); beside
                                             * EXPV_MI_PATH_TWO_KERNEL or EXPV_MI_PATH_MODULAR, the only two forms such a call runs */
};
const char *expv_mi_last_error(expv_mi_ctx_t ctx);
const char *expv_mi_version(void);

/* raw device memory for host languages without a GPU array type (the Julia shim's MIVector) */
int expv_mi_malloc(expv_mi_ctx_t ctx, size_t bytes, void **dptr);
/* expv_mi_free never dereferences `ctx` (it may already be destroyed -- finalizers run in any order -- or NULL); errors go to
 * expv_mi_last_error(NULL) */
int expv_mi_free(expv_mi_ctx_t ctx, void *dptr);
int expv_mi_memcpy_h2d(expv_mi_ctx_t ctx, void *dst, const void *src, size_t bytes);
int expv_mi_memcpy_d2h(expv_mi_ctx_t ctx, void *dst, const void *src, size_t bytes);

/* per-kernel timing (HIP events on the context's stream) for bench.py's roofline leg */
enum {
  EXPV_MI_K_FIRSTSTEP = 0, EXPV_MI_K_MATVEC = 1, EXPV_MI_K_DOTS = 2, EXPV_MI_K_UPDATE = 3,
  EXPV_MI_K_SCALE = 4, EXPV_MI_K_COMBINE = 5, EXPV_MI_K_FUSED_A = 6, EXPV_MI_K_FUSED_B = 7,
  EXPV_MI_K_LINCOMB = 8, EXPV_MI_K_AUG = 9, EXPV_MI_K_BATCH = 10, EXPV_MI_K_COUNT = 11
};
int expv_mi_prof_enable(expv_mi_ctx_t ctx, int on);
int expv_mi_prof_reset(expv_mi_ctx_t ctx);
int expv_mi_prof_get(expv_mi_ctx_t ctx, int kernel_id, int64_t *launches, double *total_ms);
const char *expv_mi_prof_name(int kernel_id);

/* ------------------------------------------------------------------ operators -------- */
/* The operator contract of docs/src/interfaces.md:7-36 (eltype, size, mul!, ishermitian).
 * Matrices are copied to HBM at create time (CSC is converted to CSR32 once; setup cost). */

/* SparseArrays.SparseMatrixCSC{T,Int64} as Julia holds it: colptr[n+1], rowval[nnz], nzval[nnz];
 * index_base = 1 for Julia arrays, 0 for scipy. */
int expv_mi_op_create_csc(expv_mi_ctx_t ctx, int dtype, int64_t n, const int64_t *colptr,
                          const int64_t *rowval, const void *nzval, int index_base, expv_mi_op_t *op);
/* CSR from HOST arrays: rowptr[n+1], colind[nnz], vals[nnz]; idx_bytes = 4 or 8 (nnz is read from rowptr[n]). */
int expv_mi_op_create_csr(expv_mi_ctx_t ctx, int dtype, int64_t n, const void *rowptr, const void *colind,
                          const void *vals, int idx_bytes, int index_base, expv_mi_op_t *op);
/* CSR / CSC from arrays that live where `loc` says.  loc = EXPV_MI_DEVICE is what test/gpu/gputests.jl:41-58 hands over
 * (CuSparseMatrixCSR(A): a matrix already on the device; a torch.sparse_csr tensor, a ROCSparseMatrixCSR): all three arrays are
 * device pointers on the context's device, the indices idx_bytes = 4 or 8 wide with index base 0 or 1, the values of `dtype`.
 * `nnz` is the length of the index / value arrays AS THE CALLER KNOWS IT; rowptr[n] - index_base must equal it (the library does
 * not take a buffer length from device memory it has not checked).  The arrays are read during the call only.
 *   - The index arrays are checked on the device before anything indexes by them: rowptr[0] == index_base, rowptr non-decreasing,
 *     rowptr[n] - index_base == nnz, every index in [0, n).  A violation returns EXPV_MI_ARGUMENT_ERROR with the host creators'
 *     message (+ the first offending position) and nothing else has run.
 *   - Only the normalised pattern, 4 (n + 1 + nnz) bytes, comes to the host, where the orderings and storage layouts are planned
 *     (plan cache included).  The values go from the caller's buffer to their stored places on the device; opnorm(A, Inf),
 *     ishermitian and the constant-diagonal test are evaluated there, as by expv_mi_op_update_values.  One exception: rows that are
 *     not sorted and free of duplicates have their Hermitian test on the host, on a downloaded copy (expv_mi_op_ingest_info tells).
 *   - expv_mi_op_update_values takes new values in the caller's entry order (CSR or CSC), as for host-created operators.
 * loc = EXPV_MI_HOST: exactly expv_mi_op_create_csr / _csc on host arrays (4-byte CSC indices are widened). */
int expv_mi_op_create_csr_loc(expv_mi_ctx_t ctx, int dtype, int64_t n, int64_t nnz, const void *rowptr, const void *colind,
                              const void *vals, int idx_bytes, int index_base, int loc, expv_mi_op_t *op);
int expv_mi_op_create_csc_loc(expv_mi_ctx_t ctx, int dtype, int64_t n, int64_t nnz, const void *colptr, const void *rowval,
                              const void *nzval, int idx_bytes, int index_base, int loc, expv_mi_op_t *op);
/* A sparse operator from coordinate triplets (row[k], col[k], vals[k]), k < nnz -- torch.sparse_coo, sparse(I, J, V, n, n), a
 * ROCSparseMatrixCOO, the output of a finite-element assembly: indices idx_bytes = 4 or 8 wide with index base 0 or 1, values of
 * `dtype`, each array 8-byte aligned at least.  The entries may come in ANY ORDER and may REPEAT a coordinate.  The operator is
 * that of the matrix with a_ij = the sum of the entries whose coordinates are (i, j); the sum is taken in the operator's element
 * type IN ASCENDING ORDER OF THE ENTRY'S POSITION k in the caller's arrays (complex types: real and imaginary parts separately).
 * That order is part of the contract: the same triplets give the same bits, whatever the device did in between.  A sum that comes
 * out as zero stays a stored entry (as in sparse(I, J, V) and scipy); expv_mi_op_info reports the number of DISTINCT coordinates
 * as nnz.  nnz = 0 with n > 0 is the zero operator.
 *   - loc = EXPV_MI_DEVICE: device pointers on the context's device, read during the call only.  loc = EXPV_MI_HOST: the three
 *     arrays are staged into device memory and take the same path -- one implementation, the same bits.
 *   - Both index arrays are range-checked on the device before anything indexes by them; an index outside [0, n) (after the base is
 *     taken off) returns EXPV_MI_ARGUMENT_ERROR, "row index out of range" / "column index out of range" + the smallest offending
 *     position, and *op is untouched.
 *   - Sorting (stable radix sort by (row, col)), coalescing and compression to CSR run on the device; from the checked CSR arrays
 *     on the operator is the one expv_mi_op_create_csr_loc makes of them (the pattern visits the host once, the values never do).
 *     Entries that arrive strictly ascending by (row, col) skip the sort and the summation; entries that arrive non-descending
 *     (adjacent repeats only) skip the sort.
 *   - expv_mi_op_update_values on such an operator takes the values of ALL the triplets handed over at creation (out[6] of
 *     expv_mi_op_ingest_info), in the caller's triplet order; they are summed exactly as at creation: the result is bit-equal to
 *     creating the operator anew.  For this the operator keeps 4 (triplets + distinct coordinates + 1) bytes of device memory
 *     (nothing when the triplets arrived strictly ascending). */
int expv_mi_op_create_coo_loc(expv_mi_ctx_t ctx, int dtype, int64_t n, int64_t nnz, const void *row, const void *col, const void *vals,
                              int idx_bytes, int index_base, int loc, expv_mi_op_t *op);
/* A sparse operator from block-compressed arrays with SQUARE blocks -- torch.sparse_bsr / sparse_bsc, scipy's bsr_matrix, a
 * ROCSparseMatrixBSR (rowPtr, colVal, nzVal, blockDim, dir): the Jacobian of a multi-component problem.  n is the SCALAR size, a
 * multiple of block_dim; nb = n / block_dim block rows (BSR) or block columns (BSC, layout bit EXPV_MI_BSR_COMPRESSED_COLS).
 * ptr[nb + 1] and idx[nnzb] are idx_bytes = 4 or 8 wide with index base 0 or 1, vals[nnzb * block_dim^2] of `dtype`, every array
 * aligned to its own element size at least (for 16-byte complex values 8 bytes suffice).  The block
 * holding element (r, c) at vals[k][r][c] is ROW-MAJOR (torch, scipy, rocSPARSE dir = row), at vals[k][c][r] COLUMN-MAJOR.
 *   - The operator is the scalar matrix scipy's bsr_matrix((vals, idx, ptr)).tocsr() gives: EVERY element of every stored block is
 *     a stored entry, zeros included, and expv_mi_op_info reports nnz = nnzb * block_dim^2.  A value-dependent pattern would break
 *     the fixed map expv_mi_op_update_values relies on; a caller who wants stored zeros gone hands over CSR.  Block `k = ptr[bi] + kk`
 *     of block row bi, cnt = ptr[bi + 1] - ptr[bi], puts its element (r, c) at scalar CSR position
 *         block_dim^2 ptr[bi] + r block_dim cnt + kk block_dim + c,   column idx[k] block_dim + c,
 *     rowptr[bi block_dim + r] = block_dim^2 ptr[bi] + r block_dim cnt (positions are formed in 64-bit arithmetic).  BSC is the same
 *     with rows and columns exchanged and yields scalar CSC arrays.  Block indices inside a block row may be unsorted and may repeat:
 *     the scalar rows are then unsorted / hold duplicates exactly as a CSR caller's would and take the same path (Hermitian test on
 *     the host, expv_mi_op_ingest_info out[2]).  nnzb = 0 with n > 0 is the zero operator.
 *   - Host-side checks, before any device work, EXPV_MI_ARGUMENT_ERROR "op_create_bsr: ...", in this order: null output; idx_bytes;
 *     unknown layout bits; block_dim < 1; n out of range for CSR32; n not a multiple of block_dim; negative nnzb; nnzb * block_dim^2
 *     exceeds CSR32; null ptr / idx / vals; bad loc.
 *   - loc = EXPV_MI_DEVICE: device pointers on the context's device, read during the call only.  loc = EXPV_MI_HOST: the three
 *     arrays are staged into device memory and take the same path -- one implementation, the same bits.
 *   - The block arrays are checked on the device before anything indexes by them, as the pattern of an nb x nb CSR matrix:
 *     ptr[0] == index_base, ptr non-decreasing, ptr[nb] - index_base == nnzb, every block index in [0, nb) -- nb, not n.  A
 *     violation returns EXPV_MI_ARGUMENT_ERROR in the host creators' words (+ the first offending position), *op is untouched and
 *     nothing else has run.  The expansion of the pattern and the permutation of the values into scalar order then run on the
 *     device (op_bsr.hip); from the checked scalar arrays on the operator is the one expv_mi_op_create_csr_loc / _csc_loc makes of
 *     them, and expv_mi_op_ingest_info reports like theirs (out[6] = out[7] = 0).
 *   - expv_mi_op_update_values on such an operator takes nnzb * block_dim^2 values in the caller's block order and layout; the
 *     result is bit-equal to creating the operator anew.  For this the operator keeps the normalised block pointer array,
 *     4 (nb + 1) bytes of device memory, and from the first refresh on a buffer of nnz values that the permuted values go to. */
enum { EXPV_MI_BSR_BLOCK_ROW_MAJOR = 0,   /* values inside a block: vals[k][r][c] (torch, scipy, rocSPARSE dir = row) */
       EXPV_MI_BSR_BLOCK_COL_MAJOR = 1,   /* vals[k][c][r] (rocSPARSE / CUSPARSE dir = column) */
       EXPV_MI_BSR_COMPRESSED_COLS = 2 }; /* BSC: ptr runs over block COLUMNS, idx holds block rows; OR-ed with the block order */
int expv_mi_op_create_bsr_loc(expv_mi_ctx_t ctx, int dtype, int64_t n, int64_t nnzb, int block_dim,
                              const void *ptr, const void *idx, const void *vals,
                              int idx_bytes, int index_base, int layout, int loc, expv_mi_op_t *op);
/* A sparse operator from STORED DIAGONALS (DIA / banded storage) -- scipy's dia_matrix, LAPACK band rows, the DIA format of GPU
 * sparse libraries, the vectors of a Tridiagonal: the operator of a method-of-lines discretisation.  offsets_host is ALWAYS a host
 * array of ndiag offsets k = column - row, in any order.  data is ndiag rows of ld elements of `dtype`, lives where `loc` says, is
 * aligned to its element size at least (8 bytes suffice for 16-byte complex) and is read during the call only; `align` says where
 * in its row a diagonal's elements lie (the enum below).  All four element types.
 *   - THE PATTERN IS DECIDED BY THE OFFSETS ALONE.  Every position of a stored diagonal that lies inside the matrix is a stored
 *     entry, zeros included: a value-dependent pattern would break the fixed map expv_mi_op_update_values relies on (the same
 *     decision as for block arrays).  As a matrix it equals scipy's dia_matrix((data, offsets)).tocsr(); scipy additionally drops
 *     stored zeros, this library does not.  expv_mi_op_info reports nnz = sum over k of max(0, n - |k|).
 *   - The position contract.  Offsets with |k| >= n contribute nothing, as in scipy.  Let s_0 < ... < s_{q-1} be the remaining
 *     offsets in ascending order and d(r) the caller's row of `data` for s_r.  Scalar CSR row i lists, in ascending r, the entries
 *     with 0 <= i + s_r < n, at column i + s_r, and
 *         rowptr[i] = sum over r of clamp(min(i, n - s_r) - max(0, -s_r), 0, n - |s_r|)
 *     (positions are formed in 64-bit arithmetic).  Rows are therefore always sorted and free of duplicates, whatever order the
 *     caller's offsets come in.  expv_mi_op_ingest_info reports out[0] = 1, out[1] = 4 (n + 1 + nnz), out[2] = 0 (Hermitian test on
 *     the device) and out[6] = out[7] = 0.
 *   - PADDING IS NEVER READ.  The slots of `data` that correspond to no matrix position are not read and may hold anything, NaN
 *     included: the first k (COL) or last k (ROW) slots of a diagonal, everything beyond a diagonal's extent up to ld, and the
 *     whole row of an out-of-range offset.
 *   - Host-side checks, before any device work, EXPV_MI_ARGUMENT_ERROR "op_create_dia: ...", *op untouched, in this order: null
 *     output; unknown align; n out of range for CSR32; ndiag < 0; null offsets_host with ndiag > 0; duplicate offsets ("offset array
 *     contains duplicate values", scipy's words); nnz exceeds CSR32; ld smaller than the longest extent an in-range diagonal needs
 *     under `align` (COL: n for k > 0, n + k for k <= 0; ROW: n - k for k >= 0, n for k < 0; START: n - |k|); null data with
 *     nnz > 0; bad loc.  Nothing else about the input can be wrong: no value is checked on the device.
 *   - ndiag = 0, or every offset out of range, with n > 0 is the zero operator.
 *   - loc = EXPV_MI_DEVICE: a device pointer on the context's device.  loc = EXPV_MI_HOST: the in-matrix segments of `data` are
 *     staged into device memory and take the same path -- one implementation, the same bits.
 *   - The pattern and the values are expanded on the device (op_dia.hip); from the scalar arrays on the operator is the one
 *     expv_mi_op_create_csr_loc makes of them.
 *   - expv_mi_op_update_values on such an operator takes a `data` array of the same ndiag x ld shape, alignment and offsets order,
 *     never reads padding, and gives a result bit-equal to creating the operator anew.  For this the operator keeps the offsets
 *     table (12 bytes per in-range diagonal, on the device and on the host) and from the first refresh on a buffer of nnz values. */
enum { EXPV_MI_DIA_ALIGN_COL = 0,    /* element (i, i+k) of diagonal k at data[d*ld + (i+k)]: scipy dia_matrix, LAPACK band rows */
       EXPV_MI_DIA_ALIGN_ROW = 1,    /* ... at data[d*ld + i]: the DIA of GPU sparse libraries */
       EXPV_MI_DIA_ALIGN_START = 2 };/* ... at data[d*ld + min(i, i+k)]: compact vectors, Julia's Tridiagonal(dl, d, du) / k => v pairs */
int expv_mi_op_create_dia_loc(expv_mi_ctx_t ctx, int dtype, int64_t n, int ndiag, const int64_t *offsets_host,
                              const void *data, int64_t ld, int align, int loc, expv_mi_op_t *op);
/* The operator of A' = conj(transpose(A)) (EXPV_MI_OP_ADJOINT) or of transpose(A) (EXPV_MI_OP_TRANSPOSE) of an operator that
 * exists -- expv(t, A', b) of the reference, where A' is a lazy wrapper and mul! does the rest (arnoldi.jl:185): the call of an
 * adjoint sensitivity and of a left eigenvector.  Here the result is an INDEPENDENT operator on the parent's context with its own
 * storage, built on the device: the parent may be updated or destroyed afterwards, and neither the parent's values nor their
 * transposed copies visit the host.  All four element types; for the real ones the two values of `how` give the same bits.
 *   - Sparse parents, however they were created (host or device CSR / CSC, triplets, block arrays, stored diagonals; reordered,
 *     patch form, irregular rows).  BY DEFINITION the result is the operator expv_mi_op_create_csr_loc would make, on the same
 *     context, of the zero-based CSR32 arrays of A' (or transpose(A)) in the caller's natural ordering with every row in ascending
 *     column order: the same planners, the plan cache keyed by the ADJOINT's pattern, its own reordering decision.  nnz equals the
 *     parent's, stored zeros stay stored.  A parent stored as P A P' has its stored indices relabelled through P on the device
 *     first.  Where the parent's rows repeat a coordinate the repeats stay separate entries, adjacent in the adjoint's row, in the
 *     parent's stored order -- deterministic, but bit-equality with an operator made of arrays transposed elsewhere is not claimed
 *     for such a parent.  Only the adjoint's PATTERN comes to the host (the planners live there), as for every device-born
 *     operator: expv_mi_op_ingest_info reports out[0] = 1, out[1] = 4 (n + 1 + nnz), out[2] = 0 (rows sorted and free of
 *     repeats), out[3 .. 5] as usual, out[6] = out[7] = 0.
 *   - Dense parents: the result owns a packed (leading dimension n) column-major copy of A' / transpose(A), n^2 elements, and goes
 *     through the property pass of expv_mi_op_create_dense(..., EXPV_MI_DEVICE).  Rows n .. lda - 1 of the parent are never read.
 *   - Matrix-free parents: EXPV_MI_UNSUPPORTED -- there is no adjoint callback to call.
 *   - Checks before any device work, EXPV_MI_ARGUMENT_ERROR "op_create_adjoint: ...", in this order: null output; null parent, or
 *     a parent whose context is gone; `how` not one of the two.  *op is untouched on every failure.
 *   - expv_mi_op_update_values on a sparse adjoint-born operator takes nnz values in the ADJOINT's own sorted-row order, which is
 *     the column-major order of A (A's entries column after column, rows ascending inside a column).
 * expv_mi_op_adjoint_refresh(adj, parent) re-reads the parent's CURRENT stored values on the device -- sparse: one gather through
 * the map adj keeps (4 nnz bytes: adjoint entry e <- parent stored entry src[e]), conjugated for EXPV_MI_OP_ADJOINT; dense: the
 * transposition again -- and refills adj through the path of expv_mi_op_update_values, so ishermitian and opnorm(A', Inf) =
 * opnorm(A, 1) are re-evaluated.  The result is bit for bit what expv_mi_op_create_adjoint(parent) would make anew.
 * EXPV_MI_ARGUMENT_ERROR "op_adjoint_refresh: ...": a null handle, adj not adjoint-born, another context, another kind, dtype, n
 * or nnz.  A parent with the same counts but ANOTHER PATTERN than the one adj was made from is the caller's error and is not
 * detected, as for expv_mi_op_update_values. */
#define EXPV_MI_OP_TRANSPOSE 1   /* transpose(A): no conjugation */
#define EXPV_MI_OP_ADJOINT   2   /* A' = conj(transpose(A)); real types: same bits as TRANSPOSE */
int expv_mi_op_create_adjoint(expv_mi_op_t parent, int how, expv_mi_op_t *op);
int expv_mi_op_adjoint_refresh(expv_mi_op_t adj, expv_mi_op_t parent);
/* The operator C = c_1 A_1 + ... + c_K A_K (+ c_I I) of operators that exist, 1 <= K <= EXPV_MI_LINCOMB_MAX_TERMS -- the reference's
 * expv(t, H0 + f(tk)*H1, b) and expv(t, A - sigma*I, b), where + and * on a sparse matrix make the sum: a driven Hamiltonian, the
 * Jacobian J0 + c(u) J1 of an exponential integrator, a shifted operator.  The result is an INDEPENDENT operator on the terms'
 * context with its own storage, built on the device from what the terms STORE: they may be updated or destroyed afterwards, and
 * neither their values nor the combined ones visit the host.  `coef` holds (re, im) pairs, one per term, plus one more for the
 * identity when EXPV_MI_LINCOMB_IDENTITY is set in `flags`; each is rounded once to the real type of the operator's elements.
 *   - Pattern.  Decided by the terms' patterns and the flag alone, never by a value or a coefficient: the union of the terms'
 *     coordinates, plus the whole diagonal with EXPV_MI_LINCOMB_IDENTITY, in the caller's natural ordering, every row sorted and
 *     free of repeats.  An entry that cancels to zero stays stored; a term with coefficient 0 still contributes its pattern and
 *     its products (0 * NaN is NaN); nnz is the number of distinct coordinates.
 *   - Which operator.  BY DEFINITION the one expv_mi_op_create_csr_loc makes, on the same context, of those zero-based CSR32
 *     arrays: the same planners, its own reordering decision, the plan cache keyed by the COMBINED pattern.  Only that pattern
 *     comes to the host; expv_mi_op_ingest_info reports as for the adjoint: out[0] = 1, out[1] = 4 (n + 1 + nnz), out[2] = 0,
 *     out[3 .. 5] as usual, out[6] = out[7] = 0.
 *   - Values, bit for bit.  The contributions to one coordinate are added left to right in term order; inside a term that repeats
 *     a coordinate, in that term's stored order; the identity comes last.  The accumulator STARTS as the first contribution, not
 *     as 0, so -0 survives.  A coefficient with im == 0 multiplies each real component once; a complex one gives
 *     (cr ar - ci ai, cr ai + ci ar), each product rounded, then the sum or difference rounded; the identity contributes its
 *     coefficient (cr, ci) as it is.  Nothing is fused and no floating-point atomic is used: two creations give the same bits.
 *   - Terms.  All sparse or all dense, on one context, of one dtype and n.  A sparse term may be of any birth, reordered (its
 *     stored indices are relabelled through its permutation on the device first) or in patch form; the same handle may appear
 *     twice; A + A' takes the operator expv_mi_op_create_adjoint made as a term.  All four element types.  Dense terms: the
 *     result owns a packed (leading dimension n) column-major matrix written by one element-wise kernel -- 16-byte packs where the
 *     address and the term's lda allow, rows n .. lda - 1 of a term are never read -- and goes through the property pass of
 *     expv_mi_op_create_dense(..., EXPV_MI_DEVICE); the identity touches the diagonal only.
 *   - Checks before any device work, EXPV_MI_ARGUMENT_ERROR "op_create_lincomb: ...", in this order: null output; unknown flag
 *     bits; nterms outside [1, 8] (the identity without a term is refused too: this call has nothing to take a context, an element
 *     type and n from); null coef; null terms; a null term, or one whose context is gone; terms on different contexts, or of
 *     different dtype or n; a matrix-free term (EXPV_MI_UNSUPPORTED); sparse and dense terms mixed; a nonzero imaginary
 *     coefficient for a real dtype; a coefficient that is not finite; for sparse terms, sum of nnz_k (+ n) > 2^31 - 1.  *op is
 *     untouched on every failure.
 *   - expv_mi_op_update_values on a sparse result takes nnz values in ITS OWN sorted-row order.
 * expv_mi_op_lincomb_refresh(op, nterms, terms, coef) takes new coefficients and the terms' CURRENT values -- the terms it was made
 * from, or others of the same patterns.  Sparse: one gather-scale-sum launch through the map the operator keeps, into a buffer it
 * keeps, then the path of expv_mi_op_update_values, so ishermitian and opnorm(C, Inf) are re-evaluated; dense: the element-wise
 * kernel again.  The result is bit for bit what expv_mi_op_create_lincomb would make anew.  EXPV_MI_ARGUMENT_ERROR
 * "op_lincomb_refresh: ...": a null handle, op not lincomb-born, another nterms, a term on another context or of another kind,
 * dtype, n or (sparse) nnz than the term in its place had, a bad coefficient.  Terms with the same counts but ANOTHER PATTERN are
 * the caller's error and are not detected, as for expv_mi_op_update_values.  Kept on a sparse result for this: 4 (sum of nnz_k
 * [+ n] + nnz + 1) bytes of map and segment table and, from the first refresh on, a buffer of nnz values. */
#define EXPV_MI_LINCOMB_MAX_TERMS 8
#define EXPV_MI_LINCOMB_IDENTITY  1   /* flags: coef carries one more pair, the identity's */
int expv_mi_op_create_lincomb(int nterms, const expv_mi_op_t *terms, const double *coef, int flags, expv_mi_op_t *op);
int expv_mi_op_lincomb_refresh(expv_mi_op_t op, int nterms, const expv_mi_op_t *terms, const double *coef);
/* How a sparse operator came to be: out[0] 1 = created from device arrays (or triplets); out[1] bytes of pattern brought to the
 * host; out[2] bytes of VALUES brought to the host (0 when every row is sorted and free of duplicates); out[3] the whole creation
 * and out[4] the ingest kernels + status read-back (triplets: check, sort, compress and sums, by device events), in microseconds;
 * out[5] 1 = ordering plan taken from the plan cache; out[6] the triplets handed to expv_mi_op_create_coo_loc (0 for CSR / CSC
 * born operators); out[7] the sort passes that ran for them.  An operator created from host CSR / CSC arrays reports zeros.  One
 * created from stored diagonals (expv_mi_op_create_dia_loc) reports out[0] = 1, out[1] = 4 (n + 1 + nnz), out[2] = 0 always (its
 * rows are sorted by construction), out[4] the table upload, the expansion kernels and the wait for them, out[6] = out[7] = 0. */
int expv_mi_op_ingest_info(expv_mi_op_t op, int64_t out[8]);
/* Dense column-major n x n (Matrix{T}); `loc` = where A lives now. */
int expv_mi_op_create_dense(expv_mi_ctx_t ctx, int dtype, int64_t n, const void *A, int64_t lda, int loc,
                            expv_mi_op_t *op);
/* Matrix-free operator: `matvec(user, x_dev, y_dev, hip_stream)` must enqueue y = A*x on the stream
 * (basictests.jl:786-816 interface contract).  What the callback may rely on: x and y are device vectors of n elements, 16-byte
 * aligned, valid for the duration of the call, y does not alias x.  By default (context option "matfree_fused" = 0) x is the
 * NORMALISED basis column v_j, |v_j| = 1, exactly what the reference hands to mul! (arnoldi.jl:185) -- a callback that is only
 * approximately linear (a finite-difference Jacobian-vector product) sees the arguments it was tuned for.  With "matfree_fused" = 1
 * (LINEAR callbacks: one reduction and two launches less per step) the library applies it to the un-normalised u_j = beta_j v_j and
 * rescales the result.  Either way it is called once per step up to m even when the device finds a happy breakdown earlier (the
 * host does not synchronise inside the loop; the later results are discarded -- the reference stops calling mul! there, arnoldi.jl:370). */
typedef int (*expv_mi_matvec_fn)(void *user, const void *x_dev, void *y_dev, void *hip_stream);
int expv_mi_op_create_callback(expv_mi_ctx_t ctx, int dtype, int64_t n, expv_mi_matvec_fn fn, void *user,
                               int ishermitian, int64_t nnz_hint, expv_mi_op_t *op);
/* New values on the SAME sparsity pattern (a Jacobian refreshed every time step): `vals` holds nnz values of the operator's
 * dtype in the order of the arrays the operator was created from (nzval order for op_create_csc, vals order for
 * op_create_csr); loc = EXPV_MI_HOST or EXPV_MI_DEVICE.  The stored forms are refilled on the device and ishermitian /
 * opnorm(A, Inf) re-evaluated -- ~20x cheaper than destroy + create (n = 1e6, nnz = 5e6: 2.6 ms against 36-42 ms).  The reference
 * has no counterpart because it reads A at call time (mul!(y, A, x)); a caller that mutates A in place calls this instead.
 * An operator created from triplets takes one value per TRIPLET, in triplet order (see expv_mi_op_create_coo_loc); one created
 * from block arrays takes nnzb * block_dim^2 values in block order and layout (see expv_mi_op_create_bsr_loc); one created from
 * stored diagonals takes a `data` array of the creation's ndiag x ld shape, alignment and offsets order, whose padding is not read
 * (see expv_mi_op_create_dia_loc). */
int expv_mi_op_update_values(expv_mi_op_t op, const void *vals, int loc);
int expv_mi_op_destroy(expv_mi_op_t op);
/* size(A,1), nnz (NA of krylov_phiv_adaptive.jl:335-342), LinearAlgebra.ishermitian(A), opnorm(A,Inf) */
int expv_mi_op_info(expv_mi_op_t op, int64_t *n, int64_t *nnz, int *ishermitian, double *opnorm_inf,
                    int *dtype);
/* Row ordering of a sparse operator (context option "reorder", default 1): an operator that would take the two-kernel step in its
 * natural ordering is stored as P A P' (P = reverse Cuthill-McKee on the pattern of A + A') when that puts it on the single-pass
 * step; every entry point permutes vectors on their way in and out, H / beta / the results are those of the natural ordering
 * (rounding apart).  out[0] = 1 when reordered, out[1] / out[2] = max |col - row| before / after, out[3] = the reordering's share
 * of the creation time in microseconds.  No reference counterpart (the reference applies A in the caller's ordering). */
int expv_mi_op_reorder_info(expv_mi_op_t op, int64_t out[4]);
/* Patch form (context option "patch", default 1; read when an operator is created).  Besides the grid-patch ordering described here the
 * same option gives (i) meshes in an arbitrary numbering an ordering cut from breadth-first bands (expv_mi_host_mesh_patch_order) and
 * (ii) banded operators without a diagonal form the patch form in their OWN ordering (nothing permuted; the halo is the ring): out[0]
 * = 1 and out[1] = 0 for both.
 * Grid-patch ordering: a 5- / 9-point stencil on a 2-D grid
 * with rows of k cells (every offset within 2 of 0 or of +-k) is stored in an ordering in which a tile of the single-pass step is a
 * 16 x 32 patch of the grid, and the step recomputes u_j on the ring of rows around each tile (patch form) instead of waiting for
 * per-tile flags (wave form).  A special case of the reordering above: expv_mi_op_reorder_info reports it too, vectors are permuted
 * the same way.  out[0] = 1 when the operator is stored that way, out[1] = k, out[2] = tiles, out[3] = longest ring, out[4] = sum
 * of the ring lengths, out[5] = tiles whose ring is longer than 128 rows, out[6] = column indices kept after sharing the equal
 * column blocks of slices, out[7] = ring entries stored per tile. */
int expv_mi_op_patch_info(expv_mi_op_t op, int64_t out[8]);
/* Constant tiles of a banded fp64 operator (context option "elide"): out[0] tiles of 512 stored rows, out[1] stored diagonals,
 * out[2] (tile, diagonal) pairs on which the diagonal holds one bit pattern (zero fill included) and is therefore not streamed by
 * the single-pass step, out[3] 1 = every diagonal is constant on all its rows (what option "stencil" needs).  mask (may be null):
 * receives min(mask_len, out[0]) bytes, bit d of byte t = diagonal d on tile t.  All zero for operators without that form. */
int expv_mi_op_elide_info(expv_mi_op_t op, int64_t out[4], unsigned char *mask, int64_t mask_len);
/* Ordering plans by pattern (no reference counterpart: the reference applies A as stored, arnoldi.jl:185).  What creation derives from
 * the PATTERN of a sparse operator -- the row ordering, P A P' with the map back to the caller's entries, the rings and tile-local
 * columns of the patch form -- is kept for the last few patterns (process-wide; default 2, environment EXPV_MI_PLAN_CACHE at load
 * time, ~100 MB of host memory per entry at n = 1e6): creating an operator with a pattern seen before costs one hash and one comparison
 * of the pattern plus the value scatter and the uploads (0.4 .. 1.1 s -> a few tens of ms at n = 1e6).  Patterns are compared entry by
 * entry, never by hash alone.  what = 0: statistics only; 1: drop every stored plan; 2: set the capacity to `value` (0 .. 64; 0 = off).
 * out (may be null) = {plans stored, hits, misses, capacity} after the call. */
int expv_mi_plan_cache(int what, int64_t value, int64_t out[4]);
/* The same analysis on the host, no device needed (tests; what expv_mi_op_create_csr would do with option patch = 1): CSR pattern with
 * 0-based int32 indices; perm (n entries, may be null): row i of the stored operator is row perm[i] of A; ring_count (one entry per
 * tile of 4096 / sizeof(element) rows, may be null); out as in expv_mi_op_patch_info (all zero when no 2-D grid is recognised). */
int expv_mi_host_patch_order(int64_t n, const int32_t *rowptr, const int32_t *colind, int dtype, int32_t *perm, int32_t *ring_count,
                             int64_t out[8]);
/* The same for a mesh in ANY numbering (what creation tries, under option patch, before reverse Cuthill-McKee for an operator without a
 * single-pass form in its natural ordering): patches cut from two breadth-first distance fields of the graph of A + A'; kept when
 * every tile's ring fits (<= 256 rows) and the rings average <= 176 rows (Float32: 352).  out[1] = 0 (no grid row length). */
int expv_mi_host_mesh_patch_order(int64_t n, const int32_t *rowptr, const int32_t *colind, int dtype, int32_t *perm, int32_t *ring_count,
                                  int64_t out[8]);
/* mul!(y, A, x)  (arnoldi.jl:185) */
int expv_mi_op_apply(expv_mi_op_t op, const void *x, int x_loc, void *y, int y_loc);
/* mul!(y, A, x) for a REAL operator (F64 / F32) and vectors of its complex type (C64 / C32): the operator is read as it is stored, no
 * promoted copy.  Host and device locations and reordered operators as in expv_mi_op_apply; complete on return.  An operator with a
 * fused form (SELL slots without overflow entries, or the general diagonal form under option dia) is walked once against the
 * interleaved x: one operator value and one complex gather per entry, one fma per component in ascending stored order -- the values
 * of the promoted operator's mul!.  Every other operator (overflow rows, column-blocked storage, dense, matrix-free) applies its own
 * real mul! to the real and to the imaginary plane of x: a matrix-free callback sees real n-vectors, twice.  Counter [6] of
 * expv_mi_ctx_counters counts one application on the first path and two on the second.
 * A complex operator is EXPV_MI_ARGUMENT_ERROR "op_apply_complex: ...". */
int expv_mi_op_apply_complex(expv_mi_op_t op, const void *x, int x_loc, void *y, int y_loc);

/* y[0:nrows] = A x for a DEVICE-RESIDENT column-major nrows x ncols block A (leading dimension lda >= nrows), x (ncols) and
 * y (nrows) device vectors, enqueued on the context's stream (stream-ordered: nothing is synchronised).  The same kernel as the
 * dense operator's mul! (arnoldi.jl:185).  This is the local half of an operator whose ROWS are spread over several GPUs
 * (BASELINE configs[2] at n = 2e5 does not fit one device: exponentialutilities.jl_amd/dist.py RowShardedDense calls it from
 * inside its matrix-free callback, then all-gathers the pieces); no reference counterpart (the reference is single-process).
 * `scratch` (device, nsplit * nrows elements, or NULL with nsplit <= 1) holds the partial sums of a column-split launch. */
int expv_mi_gemv_block(expv_mi_ctx_t ctx, int dtype, int64_t nrows, int64_t ncols, const void *A, int64_t lda,
                       const void *x, void *y, void *scratch, int nsplit);

/* exponential!(A) for a dense matrix on the device -- exp.jl:56-58 -> exponential!(A, ExpMethodHigham2005(false)),
 * exp_noalloc.jl:114-168; test/gpu/gputests.jl:22-39.  A: column-major n x n, leading dimension lda >= n, overwritten with exp(A);
 * rows n..lda-1 of every column are neither read nor written.  loc = EXPV_MI_DEVICE: a device pointer on the context's device;
 * EXPV_MI_HOST: staged through HBM, result copied back.  All four element types.  Always computed on the device (no host fallback
 * at any n): opnorm(A, 1) with fp64 column sums, Pade order 3 / 5 / 7 / 9 / 13 by the thresholds 0.015 / 0.25 / 0.95 / 2.1, above
 * 2.1 s = max(0, ceil(log2(nA / 5.4))) exact scalings by 1/2, Horner in A^2 (products on the matrix cores), (V - U) X = (V + U) by a
 * blocked LU with partial pivoting, s squarings.  No balancing, like the reference's GPU dispatch.  ONE deliberate difference: the
 * reference's generated evaluation graphs stop at 2^-8 (exp_generated/exp_13.jl:19) and under-scale for nA >= 1382.4; here s is
 * unbounded, like exp_baseexp.jl and expv_mi_host_expm.
 * A non-finite opnorm(A, 1) answers EXPV_MI_ARGUMENT_ERROR ("ArgumentError: matrix contains Infs or NaNs"), an exactly zero pivot
 * column of the LU EXPV_MI_SINGULAR; A is untouched in both cases.  n = 0 does nothing.  Complete on return unless the context's
 * outputs are stream-ordered (expv_mi_ctx_set_async_outputs).
 * info (may be NULL): [0] Pade order used (3,5,7,9,13), [1] squarings s, [2] row exchanges of the solve's LU, [3] whole call in
 * microseconds, [4..7] 0. */
int expv_mi_expm(expv_mi_ctx_t ctx, int dtype, int64_t n, void *A, int64_t lda, int loc, int64_t info[8]);

/* exponential!(A, ExpMethodHigham2005Base()) for a dense matrix on the device -- exp_baseexp.jl:112-161, the algorithm of
 * expv_mi_host_expm: the finite check (on opnorm(A, 1) of the caller's matrix: errors and the untouched A as expv_mi_expm), then
 * gebal job 'B' (permute, then scale by powers of two; see expv_mi_gebal), opnorm(A_bal, 1) with fp64 column sums, then exactly
 * expv_mi_expm's order / s selection, Pade, LU and squarings on the balanced matrix, and unbalance folded into the copy into A.
 * ONE deliberate difference to expv_mi_expm and exp_noalloc.jl:117: the norm that selects order and s is taken AFTER balancing, as
 * in exp_baseexp.jl:127-129.  For A = D B D^-1 with a badly scaled D it sees |B|, not |A|: dozens of squarings fewer, and none of
 * their rounding.  The reference has no such method for a GPU array (its balancing routines index scalars).  On a matrix that
 * balancing leaves alone the result is expv_mi_expm's bit for bit.  Arguments, loc, errors, n = 0, n > 65535 and completion as
 * expv_mi_expm; a scaling loop that has not settled after 128 sweeps answers EXPV_MI_UNSUPPORTED with A untouched.
 * info (may be NULL): [0..3] as expv_mi_expm, [4] ilo, [5] ihi (1-based), [6] sweeps of the scaling loop (the last one changes
 * nothing), [7] microseconds spent balancing and undoing it (with stream-ordered outputs: without the last pass). */
int expv_mi_expm_balanced(expv_mi_ctx_t ctx, int dtype, int64_t n, void *A, int64_t lda, int loc, int64_t info[8]);

/* LAPACK.gebal!('B', A) for a dense matrix on the device (or a staged host matrix, loc = EXPV_MI_HOST): A, column-major n x n with
 * leading dimension lda >= n, is balanced in place (rows n..lda-1 untouched).  xGEBAL job 'B', 2-norm variant, radix 2, factor
 * 0.95, the decisions and their order those of the host routine (expv_mi_host_gebal); the row and column norms are summed in fp64
 * for every element type, the guards sfmin / sfmax are those of the element type's real type, -0.0 counts as zero.  *ilo, *ihi:
 * 1-based; scale_host (HOST memory, n doubles) in LAPACK's convention: the factors inside ilo..ihi, outside them 1 + the position
 * each one was exchanged with.  Any of the three may be NULL.  n = 0: *ilo = 1, *ihi = 0.  A non-finite entry answers
 * EXPV_MI_ARGUMENT_ERROR as LAPACK.gebal!'s chkfinite does, n > 65535 EXPV_MI_UNSUPPORTED; A is untouched then. */
int expv_mi_gebal(expv_mi_ctx_t ctx, int dtype, int64_t n, void *A, int64_t lda, int loc, int64_t *ilo, int64_t *ihi,
                  double *scale_host);

/* phi!(out, A, k) for a dense matrix on the device -- phi.jl:159-257: out[j] <- phi_j(A), j = 0 .. k (phi_0 = exp).  A: column-major
 * n x n, leading dimension lda >= n, NOT modified; out: a HOST array of k + 1 pointers to column-major n x n matrices with leading
 * dimension ldo >= n.  loc applies to A and to every out[j] (EXPV_MI_DEVICE: device pointers; EXPV_MI_HOST: staged through HBM).  Rows
 * n..ld-1 of every column are neither read nor written.  All four element types, always on the device.
 * Scaling and recovering: opnorm(A, 1) with fp64 column sums, s = the smallest integer with opnorm 2^-s <= 1 (not capped),
 * phi_k(A 2^-s) by its Taylor series to degree 18 (64-bit types) / 10 (32-bit types) in Paterson-Stockmeyer form,
 * phi_j = A 2^-s phi_{j+1} + I / j! downwards, then s times phi_0(2X) = phi_0(X)^2,
 * phi_j(2X) = 2^-j (phi_0(X) phi_j(X) + sum_{i=1..j} phi_i(X) / (j - i)!), every product on the matrix cores.
 * The deliberate difference: ONE Taylor core with the fixed threshold 1 for all four element types, where the reference takes a
 * tabulated Pade approximant for Float64 / ComplexF64 (phi_almohy.jl) and the basis-vector route (k + 1 augmented exponentials) for
 * the others.  k = 0 computes exp(A) by this path, not by expv_mi_expm's Pade.
 * There is no NaN-fill convention: a non-finite opnorm(A, 1) answers EXPV_MI_ARGUMENT_ERROR ("ArgumentError: matrix contains Infs or
 * NaNs").  k < 0, k > 16, an out[j] that overlaps A or another out[i]: EXPV_MI_ARGUMENT_ERROR; n > 65535: EXPV_MI_UNSUPPORTED.  The
 * results are built in the context's workspace and copied out last: every failure leaves `out` untouched.  Overflow inside the
 * recovery gives Inf / NaN entries, returned as computed.  n = 0 does nothing.  Complete on return unless the context's outputs are
 * stream-ordered (expv_mi_ctx_set_async_outputs).
 * info (may be NULL): [0] Taylor degree, [1] scalings s, [2] matrix products launched (a recovery step's wide product counts once),
 * [3] whole call in microseconds, [4..7] 0. */
int expv_mi_phi(expv_mi_ctx_t ctx, int dtype, int64_t n, int k, const void *A, int64_t lda, void *const *out, int64_t ldo, int loc,
                int64_t info[8]);

/* mul!(C, A, B, alpha, beta): C = alpha A B + beta C for DEVICE-resident column-major blocks (A m x k, B k x n, C m x n), enqueued on
 * the context's stream, stream-ordered like expv_mi_gemv_block.  The product kernel of expv_mi_expm (gfx950 matrix cores); C must not
 * alias A or B.  beta == 0 does not read C.  alpha_im / beta_im must be 0 for the real types.  The tile (64 x 64 or 128 x 128) is
 * chosen by size; a context created under EXPV_MI_DENSE_TILE=1 / 2 always takes the small / big one (A/B runs, tests). */
int expv_mi_gemm(expv_mi_ctx_t ctx, int dtype, int64_t m, int64_t n, int64_t k, double alpha_re, double alpha_im,
                 const void *A, int64_t lda, const void *B, int64_t ldb, double beta_re, double beta_im, void *C, int64_t ldc);

/* ------------------------------------------------------------------ KrylovSubspace --- */
/* KrylovSubspace{T,U}(n, maxiter, augmented)  (arnoldi.jl:63-76).  V lives in HBM,
 * (n+augmented) x (maxiter+1); H is host-resident, (maxiter+1) x (maxiter + (augmented != 0)),
 * element type U = dtype_U (EXPV_MI_F64 for a Hermitian problem). */
int expv_mi_ks_create(expv_mi_ctx_t ctx, int dtype_T, int dtype_U, int64_t n, int maxiter, int augmented,
                      expv_mi_ks_t *ks);
int expv_mi_ks_destroy(expv_mi_ks_t ks);
/* Base.resize!(Ks, maxiter)  (arnoldi.jl:80-93): contents survive only when augmented != 0 */
int expv_mi_ks_resize(expv_mi_ks_t ks, int maxiter);
/* fields m, maxiter, augmented, beta, wasbreakdown (arnoldi.jl:54-58) */
int expv_mi_ks_get(expv_mi_ks_t ks, int *m, int *maxiter, int *augmented, double *beta, int *wasbreakdown);
int expv_mi_ks_set_m(expv_mi_ks_t ks, int m);
/* Ks.H: pointer to the host matrix (valid until resize/destroy), its leading dimension and shape */
int expv_mi_ks_H(expv_mi_ks_t ks, void **H, int *ldh, int *nrows, int *ncols);
/* copy columns [col0, col0+ncols) of Ks.V to / from the host (ld of the host array = ldh_host).
 * Rows are ALWAYS in the caller's (natural) ordering: a basis produced by a reordered operator (expv_mi_op_reorder_info) is kept in
 * the operator's stored ordering until one of these three accessors is called, which converts it back in place first (and a later
 * continuation with that operator converts it forth again); expv_mi_expv_ks / _phiv_ks / _combine un-permute their results. */
int expv_mi_ks_V_download(expv_mi_ks_t ks, int col0, int ncols, void *dst, int64_t ld_dst);
int expv_mi_ks_V_upload(expv_mi_ks_t ks, int col0, int ncols, const void *src, int64_t ld_src);
int expv_mi_ks_V_devptr(expv_mi_ks_t ks, void **V, int64_t *ldv);   /* ldv: rows padded to whole waves of 16-byte packs (128; 256 for F32), padding = 0 */

/* arnoldi!(Ks, A, b; tol, m, ishermitian, iop, init)  (arnoldi.jl:345-377);
 * ishermitian != 0 runs lanczos! (arnoldi.jl:456-490).  ishermitian < 0 = ask the operator. */
typedef struct {
  int32_t m;            /* requested Krylov dimension; <= 0 means min(maxiter, n)                  */
  int32_t iop;          /* incomplete-orthogonalisation window; 0 = full Arnoldi                   */
  int32_t init;         /* continue at step `init` (0 = fresh first step)                          */
  int32_t ishermitian;  /* 1 Lanczos, 0 Arnoldi, -1 LinearAlgebra.ishermitian(A)                   */
  int32_t ortho;        /* expv_mi_ortho                                                           */
  int32_t flags;        /* EXPV_MI_ARNOLDI_* bits, 0 by default                                     */
  double tol;           /* happy-breakdown threshold (absolute), default 1e-7                      */
} expv_mi_arnoldi_opts;
/* flags bit 0 (expv_mi_arnoldi / expv_mi_lanczos): return as soon as H[1:m, 1:m], beta and the first m basis columns are final; the
 * closing pass of the single-pass step (v_{m+1}, H[m+1, m], the breakdown test of step m) finishes on the device and is collected by
 * the NEXT library call that touches the subspace (expv_mi_ks_get / _H / _V_* / _set_m / _resize, expv_mi_expv_ks, expv_mi_phiv_ks,
 * expv_mi_combine, another factorisation, destroy).  expv!(w, t, Ks) then runs its host exponential -- which needs H[1:m, 1:m] only --
 * UNDER that pass instead of behind it (krylov_phiv.jl:200-247; round 6).  A host that caches the pointer of expv_mi_ks_H across a
 * factorisation must not set it; the Julia shim and the Python mirror fetch H through the call every time and do. */
#define EXPV_MI_ARNOLDI_DEFER_TAIL 1
void expv_mi_arnoldi_opts_default(expv_mi_arnoldi_opts *o);
/* The operator's dtype equals the subspace's dtype_T, or -- a MIXED call, T = promote_type(eltype(A), eltype(b)) with a real A and a
 * complex b -- the operator is F64 / F32 and dtype_T its complex counterpart C64 / C32; b has dtype_T.  Mathematically a mixed call
 * is the call on the promoted operator; the operator is never promoted, copied or re-created.  It runs one of two forms
 * (path_flags carries EXPV_MI_PATH_REAL_OPERATOR): the two-kernel step with the operator walked in its real type, on an operator with
 * a fused form (see expv_mi_op_apply_complex) when options fused = 1, fused_two_reductions = 0, ortho != MGS and the window is
 * <= 64 columns (or Lanczos); the modular launches with expv_mi_op_apply_complex's mul! otherwise.  The single-pass, wave, patch,
 * resident and pipelined-Lanczos forms are off; a reordering of the stored operator stays in force.  ishermitian < 0 asks the
 * operator: a real symmetric one runs lanczos! with a real tridiagonal H (dtype_U = the real type).  Happy breakdown, a zero b,
 * init > 0, expv_mi_ks_resize, EXPV_MI_ARNOLDI_DEFER_TAIL and every evaluation of the resulting subspace are those of any call.
 * Every other mismatch (a complex operator with a real subspace, F64 with C32, F32 with C64) is EXPV_MI_ARGUMENT_ERROR "operator
 * dtype must equal the subspace dtype T". */
int expv_mi_arnoldi(expv_mi_ks_t ks, expv_mi_op_t op, const void *b, int b_loc,
                    const expv_mi_arnoldi_opts *opts);
/* lanczos!(Ks, A, b; ...) called directly (basictests.jl:746) */
int expv_mi_lanczos(expv_mi_ks_t ks, expv_mi_op_t op, const void *b, int b_loc,
                    const expv_mi_arnoldi_opts *opts);
/* augmented form used by kiops: arnoldi!(Ks, (A, B), (w, w_aug); init, t, mu, l, ...)
 * (arnoldi.jl:191-205, :257-279).  B is n x p (dtype T), w is the n-vector column l of kiops' w,
 * w_aug (host, p doubles) receives the t^i/i!*mu fill of firststep!. */
int expv_mi_arnoldi_aug(expv_mi_ks_t ks, expv_mi_op_t op, const void *B, int64_t ldb, int p, int b_loc,
                        const void *w, int w_loc, double *w_aug_host, double t, double mu,
                        const expv_mi_arnoldi_opts *opts);
/* (a mixed pair -- real operator, subspace of its complex type -- is EXPV_MI_ARGUMENT_ERROR "arnoldi_aug: real operator with complex
 *  vectors is not supported here"; so is expv_mi_expv_error_estimate, "expv_error_estimate: ...".  expv_mi_kiops and
 *  expv_mi_expv_batch take the vectors' type from the operator / the values and cannot be handed such a pair: they have no
 *  refusal, and complex data passed as u / B beside a real operator is read as real data of the same byte length, as it always was.
 *  Promote the operator for those two.) */

/* ------------------------------------------------------------------ evaluation ------- */
/* expv!(w, t, Ks)  (krylov_phiv.jl:200-280): w = beta * V[:,1:m] * exp(t*H[1:m,1:m]) e1.
 * t = t_re + i t_im; w_dtype must be C64 when t or T is complex. */
int expv_mi_expv_ks(expv_mi_ks_t ks, double t_re, double t_im, void *w, int w_loc, int w_dtype);
/* phiv!(w, t, Ks, k; correct, errest)  (krylov_phiv.jl:607-653); W is n x (k+1); *errest always set */
int expv_mi_phiv_ks(expv_mi_ks_t ks, double t_re, double t_im, int k, int correct, void *W, int64_t ldw,
                    int w_loc, int w_dtype, double *errest);
/* lmul!(beta_scale, mul!(w, V[:,1:m], coef))  (K10/K11 of SURVEY.md): coef is host, m x ncols */
int expv_mi_combine(expv_mi_ks_t ks, int mcols, int ncols, const void *coef_host, int ldc, int coef_dtype,
                    double beta_scale, void *W, int64_t ldw, int w_loc, int w_dtype);

/* expv(t, A, b; m, tol, iop, ishermitian, mode)  (krylov_phiv.jl:125-160) in one call */
typedef struct {
  int32_t m_used;        /* Ks.m after the factorisation      */
  int32_t wasbreakdown;
  int32_t matvecs;       /* operator applications performed   */
  int32_t path_flags;    /* EXPV_MI_PATH_* of the factorisation: which step form ran, whether a wait expired */
  double beta;
} expv_mi_expv_stats;
int expv_mi_expv(expv_mi_ctx_t ctx, expv_mi_op_t op, double t_re, double t_im, const void *b, int b_loc,
                 void *w, int w_loc, int w_dtype, const expv_mi_arnoldi_opts *opts,
                 expv_mi_expv_stats *stats);
/* expv_mi_expv for a REAL operator with b and w of its complex type (a mixed call, see expv_mi_arnoldi): exp(-i t H) b with a real
 * sparse H and a complex b, t = t_re + i t_im.  The private subspace (kept in the context, keyed on the vectors' type) is complex,
 * its H real when the operator is symmetric; v_{m+1} and H[m+1, m] are skipped as there; b and w may alias as there.  A complex
 * operator is EXPV_MI_ARGUMENT_ERROR "expv_realop: ...". */
int expv_mi_expv_realop(expv_mi_ctx_t ctx, expv_mi_op_t op, double t_re, double t_im, const void *b, int b_loc,
                        void *w, int w_loc, const expv_mi_arnoldi_opts *opts, expv_mi_expv_stats *stats);
/* expv!(w, t, A, b, Ks, cache; atol, rtol, m)  error-estimate mode, Hermitian only
 * (krylov_phiv_error_estimate.jl:149-207) */
int expv_mi_expv_error_estimate(expv_mi_ks_t ks, expv_mi_op_t op, double t_re, double t_im, const void *b,
                                int b_loc, void *w, int w_loc, double atol, double rtol, int m,
                                int ishermitian);

/* w = exp(t A) b WITHOUT a Krylov basis: the truncated Taylor series of Al-Mohy & Higham (SIAM J. Sci. Comput. 33, 2011) -- the
 * reference's second expv algorithm, ext/ExponentialUtilitiesStaticArraysExt.jl:124-163 (parameters :76-103, theta tables :10-73),
 * which stops at N <= 50 for want of a norm estimator.  Three work vectors, no inner product, no host exponential.  All four element
 * types; w has the operator's element type; b and w live where b_loc / w_loc say and may alias; a reordered operator gets its
 * vectors permuted on entry and exit.  t_im != 0 needs a complex operator (EXPV_MI_ARGUMENT_ERROR otherwise).  Complete on return.
 *   mu = tr(A) / n,  alpha = |t| opnorm(A - mu I, Inf),  (m*, s) as expv_mi_host_taylor_params gives them;  F = v = b, then s stages:
 *       c1 = |v|_inf;  for j = 1 .. m*:  v <- (t / s) (A - mu I) v / j,  F += v,  c2 = |v|_inf,  stop the stage when
 *       c1 + c2 <= tol |F|_inf, else c1 = c2;   F *= exp(mu t / s),  v = F;  the loop ends early when F is not finite.
 *   - THE NORM IS THE INFINITY NORM, not the reference's 1-norm: the exact maximum absolute row sum, one pass over the rows a stored
 *     operator already keeps on the device (a row without a stored diagonal entry contributes |mu|).  A row maximum does not depend
 *     on summation order, and the truncation analysis holds in any subordinate norm.  Trace and norm are invariant under the
 *     symmetric permutation of a reordered operator.  Matrix-free operators: mu = 0 and the caller passes opnorm > 0, a bound on
 *     opnorm(A, Inf) (EXPV_MI_ARGUMENT_ERROR without one); for stored operators opnorm is ignored.
 *   - precision 0: tol and table of the operator's real type (2^-53 for F64 / C64, 2^-24 for F32 / C32); 1: the 2^-24 table also for
 *     F64 / C64 (the arithmetic stays double: the cheap mode for integrator tolerances); anything else EXPV_MI_ARGUMENT_ERROR.
 *     In SINGLE arithmetic the series loses accuracy through its hump: the rounding error is about eps32 e^(alpha / s), and the
 *     2^-24 table allows alpha / s up to 13.4 (-i Laplacian, ComplexF32, alpha / s = 10: 3e-4; typical cases 2e-7 .. 6e-7).  That is
 *     the reference's behaviour for Float32 and is kept: no cap on alpha / s.
 *   - This entry takes the first branch of the reference's parameter search (alpha for every p: valid, conservative); the power-norm
 *     refinement, which needs products with A', is expv_mi_expv_taylor_power.  max_matvecs > 0 and m* s > max_matvecs: EXPV_MI_ARGUMENT_ERROR naming alpha, m*, s;
 *     nothing is computed, w is untouched.  A non-finite alpha is an EXPV_MI_ARGUMENT_ERROR too.
 *   - The stopping rule is decided on the device: the host enqueues s (m* + 1) launches and reads nothing in between; the launches
 *     of a stopped stage return at once.  The maxima are order-independent: the same inputs give the same bits.
 *   - Non-finite data is not an error: status OK, the non-finite w is returned.  t = 0 or alpha = 0 returns exp(mu t) b (b bit for
 *     bit when that factor is 1); b = 0 returns 0 after no application; n = 0 does nothing.
 * info (may be NULL): [0] m*, [1] s, [2] operator applications whose term entered F, [3] stages stopped before m*, [4] term launches
 * enqueued, [5] stream synchronisations that waited for device-to-host data (<= 2: mu / alpha, and the final state together with a
 * host w), [6] 1 = fused term kernel (SELL slots without overflow entries, or the general diagonal form), 2 = mul! + update kernel,
 * [7] 0, or 1 + the stage (from 0) at which a non-finite F ended the loop.  dinfo (may be NULL): [0] alpha, [1] Re mu, [2] Im mu,
 * [3] |F|_inf when the last stage closed. */
int expv_mi_expv_taylor(expv_mi_ctx_t ctx, expv_mi_op_t op, double t_re, double t_im, const void *b, int b_loc, void *w, int w_loc,
                        int precision, int64_t max_matvecs, double opnorm, int64_t info[8], double dinfo[4]);
/* w = exp(t A) b for a REAL stored or matrix-free operator (EXPV_MI_F64 / EXPV_MI_F32), t = t_re + i t_im, complex vectors: the
 * Schroedinger / wave propagation exp(-i t H) b with a real sparse H, a real Jacobian along a complex ray.  The operator is read in
 * its own real type -- no promoted complex copy is made -- and the series is that of expv_mi_expv_taylor.
 *   - w always has the operator's complex counterpart (C64 for an F64 operator, C32 for F32).  b_dtype is that complex type or the
 *     operator's own real type; a real b is widened on the device with im = +0.  b and w may be the same vector only when b is
 *     complex.  t_im = 0 is allowed: a real time applied to a complex vector.
 *   - The plan is expv_mi_expv_taylor's, from the same kernels: mu = tr(A) / n (real), alpha = |t| opnorm(A - mu I, Inf), the theta
 *     table and tol of the operator's real type and `precision`, (m*, s) of expv_mi_host_taylor_params; the max_matvecs refusal, the
 *     matrix-free opnorm rule and the early returns are the same, with the same messages ("expv_taylor: ..."): t = 0 or alpha = 0
 *     gives exp(mu t) b, b = 0 gives 0 after no application, n = 0 does nothing.
 *   - THE ROUNDINGS.  R = the operator's real type, C its complex type.  (A x)_i is accumulated per component in ascending stored
 *     order: acc.re = fma(a, x.re, acc.re), acc.im = fma(a, x.im, acc.im).  Everything after (A x)_i is the element step of
 *     expv_mi_expv_taylor in C with mu = (mu, 0) and the complex c = (t / s) / j rounded to C; the stage close is the same kernel.
 *     CONSEQUENCE: on finite data, a call that takes the fused path ([6] = 1) returns the same values -- == element by element -- as
 *     expv_mi_expv_taylor on the same operator promoted to C, whenever that call takes the fused path too and keeps the rows in the
 *     same stored ordering (the grid-patch ordering sizes its tiles by the element type: there the two differ by rounding); only the
 *     sign of a zero may differ (the complex multiply-add adds -0 x.im, the real one does not).  mu, alpha, m*, s and the
 *     application count are then identical as well.
 *   - An operator without a fused form ([6] = 2: SELL with overflow entries, column-blocked storage, dense, matrix-free)
 *     is applied with its own real mul! to the real plane and to the imaginary plane of v, then one update kernel does the element
 *     step: a matrix-free callback sees real vectors of n elements, twice per term.  Workspace: three complex vectors, plus four
 *     real planes on this path.  A reordered operator gets b permuted on entry and w on exit.
 *   - Refused before any device work, w untouched, EXPV_MI_ARGUMENT_ERROR "expv_taylor_realop: ...": a complex operator (use
 *     expv_mi_expv_taylor), a b_dtype that is neither of the two types, a real b that overlaps w, an unknown loc.
 * info / dinfo (may be NULL): as expv_mi_expv_taylor; dinfo[2] = 0.  [2] counts terms; the context's operator-application counter
 * counts mul! calls and rises by two per term when [6] = 2.  Block, grid, power and phiv forms of this call do not exist. */
int expv_mi_expv_taylor_realop(expv_mi_ctx_t ctx, expv_mi_op_t op, double t_re, double t_im, const void *b, int b_loc, int b_dtype, void *w,
                               int w_loc, int precision, int64_t max_matvecs, double opnorm, int64_t info[8], double dinfo[4]);
/* Host only: theta_m (m = 1 .. 55) of the table of `precision` (0: tol = 2^-53, 1: tol = 2^-24) -- the positive root of
 * h~_m(x) = tol x, h~_m(x) = (-1)^m log(e^x T_m(-x)), below the first real zero of T_m(-x) (tools/expv_taylor_theta.py). */
int expv_mi_host_taylor_theta(int precision, int m, double *theta);
/* Host only: m* = argmin over 1 <= m <= 55 of m ceil(alpha / theta_m) (the first minimum on ties), s = ceil(alpha / theta_m*);
 * alpha = 0 gives (0, 1); a negative, NaN or infinite alpha EXPV_MI_ARGUMENT_ERROR (message: expv_mi_last_error(NULL)). */
int expv_mi_host_taylor_params(int precision, double alpha, int *m, int64_t *s);
/* Host only: the reference's WHOLE parameter search (ext/ExponentialUtilitiesStaticArraysExt.jl:99-121).  alpha1 = |t| opnorm(B, Inf),
 * d[i] = |t| ||B^(i+2)||^(1/(i+2)), i = 0 .. 7 (d_2 .. d_9), B = A - mu I.  alpha1 = 0 gives (0, 1).  alpha1 <= 4 theta_55 * 8 * 11 / 55
 * (the cheap condition): the result of expv_mi_host_taylor_params, p_used = 0, d is not read.  Otherwise, for p = 2 .. 8,
 * alpha_p = max(d_p, d_{p+1}) and the first minimum of m ceil(alpha_p / theta_m) over p (p - 1) - 1 <= m <= 55; the overall minimum
 * is taken by (cost, m), p_used is the first p that reaches it, s = max(cost / m, 1) -- d all zero gives (1, 1).  Argument errors are
 * those of expv_mi_host_taylor_params, and a d_p that is negative or not finite. */
int expv_mi_host_taylor_params_power(int precision, double alpha1, const double d[8], int *m, int64_t *s, int *p_used);

/* A lower bound of ||(A - sigma I)^p||_inf (which = 0) or ||(A - sigma I)^p||_1 (which = 1), 1 <= p <= 16, of a STORED operator,
 * sparse or dense, all four element types, without forming a power: the block 1-norm estimator of Higham & Tisseur (SIAM J. Matrix
 * Anal. Appl. 21, 2000, Algorithm 2.4) with t = 2 columns and itmax = 5 -- the "1-norm estimation algorithm" for want of which
 * the reference's Taylor expv stops at N <= 50 (ext/ExponentialUtilitiesStaticArraysExt.jl:92-97).  An estimate never exceeds the
 * norm (rounding apart) and is usually exact or within a few per cent.  sigma = shift_re + i shift_im (shift_im != 0 needs a
 * complex operator).
 *   - adj: an operator of A' on the same context with the same dtype and n (expv_mi_op_create_adjoint makes one).  NULL: A itself
 *     when expv_mi_op_info reports it Hermitian; otherwise an adjoint is created for the call and destroyed (info[6], info[7]).
 *     The infinity norm of B^p is the 1-norm of (B')^p: `which` only swaps the roles of op and adj and conjugates the shift.
 *   - p = 1 with which = 0 is the EXACT row-sum norm, from the norm pass of expv_mi_expv_taylor; n <= 2 is exact too.
 *   - Nothing is random and two calls give the same bits.  The start block is (1/n, +-1/n); every "random" sign is
 *     expv_mi_host_normest_signs(natural row, column, draw), draws counted from 0 through the call; every tie (the larger column
 *     sum, the 12 largest h_i, "h_max is h[ind_best]" -- an index comparison) goes to the smaller natural index; a column is
 *     parallel to another when ALL n signs agree (integer counts); column sums are accumulated in fp64, per-workgroup partials
 *     finished in index order.  Complex types take sign = y / |y| (0 -> 1) and no parallel tests.  Vectors cross between the two
 *     operators in the natural ordering, so a reordered operator and its unreordered twin differ by rounding only.
 *   - No overflow, no underflow: every application multiplies its result by the exact power of two that brings its INPUT column
 *     to [1, 2) (complex: max(|re|, |im|)), the exponents are summed in integers and est is a double: est of 2^k A is 2^(kp) est of A,
 *     the same mantissa.  The scale is applied to the result of an application, so inside one the accumulator holds two
 *     applications' growth: this holds for ||A - sigma I|| between about 1e-19 and 1e19 in the 32-bit types (2^-511 .. 2^511 in the
 *     64-bit ones).
 *   - sigma is rounded to the operator's element type, for every p.
 *   - Checks before any device work, EXPV_MI_ARGUMENT_ERROR "op_norm_power: ...": null op / est, p outside 1 .. 16, unknown which, a
 *     matrix-free operator (EXPV_MI_UNSUPPORTED), a complex shift on a real operator, adj of another context, dtype or n.
 * info (may be NULL): [0] iterations, [1] panel applications (one = the operator applied to both columns), [2] blocking reads (two
 * per iteration, plus one per resampled column), [3] natural index of the column that gave est (-1: none), [4] resampled columns,
 * [5] the exit: 1 est did not grow, 2 itmax, 3 every new sign column parallel to an old one, 4 h_max is the best index, 5 the most
 * promising indices were visited already, 6 non-finite, 7 exact, [6] 1 = a temporary adjoint was made, [7] its cost in microseconds. */
int expv_mi_op_norm_power(expv_mi_op_t op, expv_mi_op_t adj, int p, double shift_re, double shift_im, int which, int64_t info[8],
                          double *est);
/* Host only: out[i] = +1 or -1, i < n: the estimator's sign for natural row i of column `col` at draw `attempt` -- the low bit of
 * the mixer behind expv_mi_host_wrapsum applied to ((i + 1) g) ^ (col << 32 | attempt). */
int expv_mi_host_normest_signs(int64_t n, int col, int64_t attempt, int8_t *out);

/* expv_mi_expv_taylor with the reference's whole parameter search.  mu and alpha1 as there.  alpha1 = 0 or the cheap condition of
 * expv_mi_host_taylor_params_power: nothing is estimated and the call IS expv_mi_expv_taylor, bit for bit.  Otherwise d_2 .. d_9 =
 * |t| est_p^(1/p), est_p = expv_mi_op_norm_power(op, adj, p, mu, which = 0), and (m*, s) = expv_mi_host_taylor_params_power(alpha1,
 * d); the series, its stopping rule and every rounding are those of expv_mi_expv_taylor.  An estimate is a lower bound, so the
 * search may choose fewer terms than exact norms would: the published algorithm's behaviour, kept.  For a non-normal operator
 * (block-triangular couplings, the augmented matrix of a forced problem) m* s drops by orders of magnitude.  Stored operators only
 * (matrix-free: EXPV_MI_UNSUPPORTED); adj as for expv_mi_op_norm_power, a temporary one is made only when the estimator runs;
 * max_matvecs is compared with the refined m* s.  info (may be NULL): [0..7] as expv_mi_expv_taylor, [8] p_used, [9] the estimator's
 * panel applications, [10] its blocking reads, [11] 1 = a temporary adjoint was made.  dinfo (may be NULL): [0..3] as
 * expv_mi_expv_taylor, [4..11] d_2 .. d_9 (zeros when nothing was estimated). */
int expv_mi_expv_taylor_power(expv_mi_ctx_t ctx, expv_mi_op_t op, expv_mi_op_t adj, double t_re, double t_im, const void *b, int b_loc,
                              void *w, int w_loc, int precision, int64_t max_matvecs, int64_t info[12], double dinfo[12]);

/* W = exp(t A) B for an n x ncols block B: ncols independent problems of expv_mi_expv_taylor that share every pass over the operator.
 * (mu, alpha, m*, s) depend on A and t alone and are computed once; every column keeps its own stopping state, and COLUMN k OF W IS BIT
 * FOR BIT what expv_mi_expv_taylor returns for column k of B with the same operator, t and precision.
 *   - B and W have the operator's element type and live where b_loc / w_loc say.  Layouts: */
enum { EXPV_MI_BLOCK_COL_MAJOR = 0,   /* element (i,k) at [i + k*ld]: Julia, Fortran-order numpy */
       EXPV_MI_BLOCK_ROW_MAJOR = 1 }; /* element (i,k) at [i*ld + k]: a contiguous torch (n,p) tensor */
/*     Elements between the columns (rows) of a padded leading dimension are neither read nor written.  W may be B itself (same
 *     pointer, ld and layout); any other overlap is EXPV_MI_ARGUMENT_ERROR.
 *   - Operators with a fused term kernel (SELL slots without overflow entries, or the general diagonal form) run in panels of 8
 *     columns (the remainder in the smallest panel of 2, 4 or 8 that holds it, padded with zero columns) on work vectors that keep a
 *     row's values adjacent: the operator is read once per term for the whole panel, and a gathered column index is one contiguous
 *     access.  A column that has stopped or ended is masked in the later term launches of its stage (its F is written back
 *     unchanged) but keeps being streamed until the last column of its panel stops; a launch whose columns have all stopped returns
 *     at once.  Every other operator (SELL with overflow entries, dense, matrix-free) runs the single-vector loop column by column.
 *     ncols = 1 runs the single-vector loop as well.
 *   - precision, max_matvecs (compared with m* s, the cost of ONE column), opnorm and the refusal of a complex t on a real operator
 *     are those of expv_mi_expv_taylor, with its messages; a refused call leaves W untouched.  ncols = 0 or n = 0 does nothing;
 *     ncols < 0, an unknown layout or loc and a leading dimension too small are EXPV_MI_ARGUMENT_ERROR "expv_taylor_block: ...",
 *     found before any device work.  Complete on return.
 * info (may be NULL): [0] m*, [1] s, [2] applications summed over the columns, [3] term launches that did work (did not return at
 * once), [4] term launches enqueued, [5] stream synchronisations that waited for device-to-host data (<= 2), [6] 1 = block kernel
 * (ncols = 1: the fused single-vector kernel), 2 = column by column through the mul! + update loop, [7] columns whose F went
 * non-finite.  dinfo (may be NULL): as expv_mi_expv_taylor, [3] = the largest |F|_inf of a column (NaN when one is).  col_info (NULL
 * or 3 ncols words): info[2], info[3], info[7] of the single call for column k at [3k .. 3k+2]; col_normF (NULL or ncols): its
 * dinfo[3]. */
int expv_mi_expv_taylor_block(expv_mi_ctx_t ctx, expv_mi_op_t op, double t_re, double t_im, const void *B, int64_t ldb, int ncols,
                              int b_layout, int b_loc, void *W, int64_t ldw, int w_layout, int w_loc, int precision,
                              int64_t max_matvecs, double opnorm, int64_t info[8], double dinfo[4], int64_t *col_info,
                              double *col_normF);

/* W(:, k) = exp(r_k t A) b for nt real multipliers r_k >= 0 (any order, duplicates allowed) in ONE sweep of the series of
 * expv_mi_expv_taylor: the time grid of the basis-free family (saveat, dense output, a propagator sampled along a ray).
 *   - R = max r_k, T = R t;  mu, alpha = |T| opnorm(A - mu I, Inf) and (m*, s) are those of expv_mi_expv_taylor for T;  h = T / s.
 *     Output k is classified in double, with exactly these expressions (expv_mi_host_taylor_grid_plan):
 *         x_k = s (r_k / R),  i_k = max(ceil(x_k) - 1, 0),  rho_k = x_k - i_k
 *     r_k = 0: the output is b, bit for bit (kind 0).  rho_k = 1: a copy of F after stage i_k has closed (kind 2).  Otherwise an
 *     interior output of stage i_k (kind 1): within a stage the terms v_j = (hA)^j F / j! are all there, and
 *     exp(rho h A) F = sum_j rho^j v_j, so no output costs a pass over the operator.
 *   - F and v run exactly as in expv_mi_expv_taylor, operation for operation: EVERY OUTPUT WITH r_k = R IS BIT FOR BIT what
 *     expv_mi_expv_taylor returns for (R t_re, R t_im).  An interior output starts as G_k = F with d_k0 = 1; at term j
 *     d_kj = d_k,j-1 rho_k in double, rounded to the operator's real type and passed by value, and G_k += d_kj v_j (one fused
 *     multiply-add per real component).  Its stopping test, on the device: c2 = d_kj |v_j|_inf, c1 starts as the stage's c1, stop
 *     when c1 + c2 <= tol |G_k|_inf, else c1 = c2.  A stopped output is masked (written back unchanged, no maxima); so is F once
 *     its own test has passed; v_j keeps being computed while F or any output of the stage is live, and a term launch returns at
 *     once when all of them have stopped or the call has ended.  The output closes with G_k <- exp(mu rho_k h) G_k (skipped when
 *     that factor is exactly 1).  The interior outputs of a stage live in panels of 8 interleaved columns (the remainder in the
 *     smallest panel of 2, 4 or 8): the first panel is updated in the epilogue of the term kernel, each further one by an
 *     accumulate-only launch per term that reads v_j once.  Workspace: the three vectors of the single call and
 *     n x 8 ceil(q_max / 8) elements, q_max the most interior outputs of one stage.
 *   - A non-finite F at the close of stage i ends the loop as in expv_mi_expv_taylor; every output of a later stage is the
 *     non-finite F as it stands; the status is OK.  alpha = 0 or t = 0: output k is exp(mu r_k t) b (b bit for bit when the factor
 *     is 1).  b = 0: zeros, no application.  nt = 0 or n = 0 does nothing.
 *   - W is n x nt in the operator's element type, layout and leading dimension as in expv_mi_expv_taylor_block, and lives where
 *     w_loc says; b lives where b_loc says; W may not overlap b.  A reordered operator answers in the caller's ordering.
 *   - nt < 0, a negative, NaN or infinite r_k, an unknown layout or loc, ldw too small and W overlapping b are
 *     EXPV_MI_ARGUMENT_ERROR "expv_taylor_grid: ...", found before any device work; precision, a complex t on a real operator, a
 *     matrix-free operator without opnorm and max_matvecs (against m* s) are refused as by expv_mi_expv_taylor, with its messages.
 *     A refused call leaves W untouched.  Complete on return.
 * info (may be NULL): [0..7] as expv_mi_expv_taylor: [2] = term launches that did work (operator applications, shared by all
 * outputs), [3] = stages whose F stopped before m*, [4] = term launches enqueued (m* s), [5] <= 2; [8] = accumulate-only launches
 * enqueued, [9] = q_max.  dinfo (may be NULL): as expv_mi_expv_taylor.  col_info (NULL or 3 nt words), for output k: [3k] its stage
 * (-1 for r_k = 0), [3k+1] the terms that entered it (stage end: the terms F took in that stage), [3k+2] its kind: 0 = b,
 * 1 = interior, 2 = stage end. */
int expv_mi_expv_taylor_grid(expv_mi_ctx_t ctx, expv_mi_op_t op, double t_re, double t_im, const double *r, int nt, const void *b, int b_loc,
                             void *W, int64_t ldw, int w_layout, int w_loc, int precision, int64_t max_matvecs, double opnorm, int64_t info[10],
                             double dinfo[4], int64_t *col_info);
/* Host only: the classification above for s stages: stage[k] = i_k (-1 for r_k = 0), rho[k] (0 for r_k = 0), kind[k]; each output
 * pointer may be NULL.  nt < 0, s < 1 and a negative, NaN or infinite r_k are EXPV_MI_ARGUMENT_ERROR. */
int expv_mi_host_taylor_grid_plan(int64_t s, const double *r, int nt, int64_t *stage, double *rho, int *kind);

/* w = phi_0(tA) u_0 + t phi_1(tA) u_1 + ... + t^p phi_p(tA) u_p for B = [u_0 ... u_p] (what phiv_timestep(t, A, B) returns) WITHOUT a
 * Krylov basis: the series of expv_mi_expv_taylor on the augmented matrix of Al-Mohy & Higham (2011, Theorem 2.1 and section 5),
 *       A~ = [A W; 0 J],  W = [u_p ... u_1],  J the p x p upward shift:  the first n rows of exp(t A~) [u_0; e_p] are w.
 * A~ is never formed: the p tail components of every term do not depend on the data and are computed on the host in (complex)
 * double, exactly as the recurrence defines them (the paper truncates them with the rest); the device keeps three work vectors of n
 * elements and adds a combination of the columns of B to each term.
 *   - B is n x ncols, ncols = p + 1, 1 <= ncols <= 9, in the operator's element type; layouts and locations as in
 *     expv_mi_expv_taylor_block.  A column-major device block of an operator in its natural ordering is read where it lies; A ROW-MAJOR
 *     DEVICE BLOCK IS TRANSPOSED ONCE into a column-major staging copy of n x ncols elements (so are a host block, copied, and the block
 *     of a reordered operator, permuted).  w holds n elements and may be column 0 of B; overlap with any other column is
 *     EXPV_MI_ARGUMENT_ERROR.  A reordered operator gets every column of B permuted on entry and w on exit.
 *   - mu = tr(A) / (n + p);  U = max |u_k[i]| and Wmax = max_i sum_k |u_k[i]| over k >= 1;  nu = 2^-ceil(log2 Wmax) (1 for Wmax = 0): the
 *     similarity diag(I, 1 / nu) changes nothing but the norm (the paper's guard against over-scaling);
 *     alpha = |t| max( max_i (|a_ii - mu| + sum_{j != i} |a_ij| + nu sum_{k>=1} |u_k[i]|), 1 + |mu| ), the infinity norm of the scaled
 *     A~ - mu I;  (m*, s) as expv_mi_host_taylor_params gives them.  Matrix-free operators: mu = 0 and opnorm stands for the A part
 *     of every row sum.  A non-finite entry among u_1 .. u_p makes alpha non-finite: EXPV_MI_ARGUMENT_ERROR.
 *   - Stage `stage` (tau = stage t / s, h = t / s) starts from zeta_0[i] = tau^(p-i) / (p-i)!, i = 1 .. p; term j:
 *       v_j = (h / j) (A - mu I) v_{j-1} + sum_{k=1..p} g_j[p+1-k] u_k,  g_j = (h / j) zeta_{j-1},  zeta_j = (h / j)(J - mu I) zeta_{j-1},  F += v_j;
 *     the g, rounded to the element type, travel by value.  The stopping test is that of expv_mi_expv_taylor with the tail as a
 *     floor: c2 = max(|v_j|_inf, |zeta_j|_inf U), c1 at stage start max(|F|_inf, |zeta_0|_inf U), against |F|_inf of the n rows --
 *     without the floor a call with u_0 = 0 would stop before the forcing has entered.  A launch whose g are all zero does not read
 *     B (mu = 0: every term j > p).  A stage closes with F *= exp(mu h), v = F.
 *   - ncols = 1 IS expv_mi_expv_taylor, bit for bit (mu = tr(A) / n, its alpha, no add).
 *   - precision, max_matvecs, opnorm, the refusal of a complex t on a real operator, non-finite data in A or u_0, n = 0 and
 *     "complete on return" are those of expv_mi_expv_taylor, with its messages.  ncols outside 1 .. 9, an unknown layout or loc and a
 *     leading dimension too small are EXPV_MI_ARGUMENT_ERROR "phiv_taylor: ...", found before any device work.  A refused call
 *     leaves w untouched.
 * info (may be NULL): as expv_mi_expv_taylor; [5] <= 3.  dinfo (may be NULL): [0] alpha, [1] Re mu, [2] Im mu, [3] |F|_inf when the
 * last stage closed, [4] nu, [5] U, [6], [7] 0. */
int expv_mi_phiv_taylor(expv_mi_ctx_t ctx, expv_mi_op_t op, double t_re, double t_im, const void *B, int64_t ldb, int ncols, int b_layout,
                        int b_loc, void *w, int w_loc, int precision, int64_t max_matvecs, double opnorm, int64_t info[8], double dinfo[8]);

/* ------------------------------------------------------------------ time stepping ---- */
typedef void (*expv_mi_print_fn)(const char *line, void *user);
typedef struct {
  double tau;          /* 0 = choose (krylov_phiv_adaptive.jl:284-292 / :374-383)   */
  double tol;          /* 1e-7                                                      */
  double delta;        /* 1.2                                                       */
  double gamma;        /* 0.8                                                       */
  double opnorm;       /* used iff has_opnorm                                       */
  int32_t has_opnorm;  /* 0: estimate from the Arnoldi Hessenberg (default)         */
  int32_t m;           /* <= 0: min(10, n)                                          */
  int32_t iop;
  int32_t correct;
  int32_t adaptive;
  int32_t ishermitian; /* -1 ask operator; only steers the flop model (see :332-334) */
  int32_t verbose;
  int32_t ortho;
  int32_t no_basis_reuse; /* 1: rebuild the Krylov basis on every adaptation retry like krylov_phiv_adaptive.jl:417 does
                             even when only tau changed (the basis does not depend on tau); 0 (default): reuse it --
                             bit-identical results, the saved factorisations are counted in stats.arnoldi_reused */
  int32_t reserved;
  int64_t NA;          /* 0: nnz of the operator                                    */
  expv_mi_print_fn print; /* verbose lines go here (stdout when NULL); the slow-progress notice (stats.stalled_steps) goes
                             here whenever it is set, verbose or not                                                          */
  void *print_user;
} expv_mi_timestep_opts;
typedef struct {
  int32_t num_timesteps;
  int32_t matvecs;
  int32_t m_final;
  int32_t arnoldi_calls;  /* factorisations the reference performs for this call (control-flow parity)             */
  int32_t arnoldi_reused; /* ... of which this many were NOT recomputed (tau-only retries reuse the basis);
                             `matvecs` keeps counting what the reference performs                                   */
  int32_t stalled_steps;  /* 0, or -- when it reached 10^4 -- the longest run of accepted sub-steps over which the step never
                             grew: the reference's controller keeps a tiny seed step for the whole interval
                             (krylov_phiv_adaptive.jl:391-417); the same is reported once per decade through `print`          */
} expv_mi_timestep_stats;
void expv_mi_timestep_opts_default(expv_mi_timestep_opts *o);
/* _phiv_timestep_caches(u_prototype, maxiter, p)  (krylov_phiv_adaptive.jl:502-511) */
int expv_mi_timestep_caches_create(expv_mi_ctx_t ctx, int dtype, int64_t n, int maxiter, int p,
                                   expv_mi_tscache_t *cache);
int expv_mi_timestep_caches_destroy(expv_mi_tscache_t cache);
/* phiv_timestep!(U, ts, A, B; ...)  (krylov_phiv_adaptive.jl:260-453).  B is n x (p+1); U is n x nts;
 * ts (host) is sorted in place like the reference (:297).  expv_timestep! is the p = 0 case.
 * Errors of the adaptive controller: EXPV_MI_ARGUMENT_ERROR "InexactError" where Julia's ceil(Int, ...) of :470 throws (the
 * error estimate did not move with m, e.g. an exhausted Krylov space), and -- where the reference would loop for ever --
 * after 1000 rejected proposals for one sub-step (kiops: 1000 rejected steps in a row). */
int expv_mi_phiv_timestep(expv_mi_ctx_t ctx, expv_mi_op_t op, int nts, double *ts, const void *B,
                          int64_t ldb, int ncoef, int b_loc, void *U, int64_t ldu, int u_loc,
                          const expv_mi_timestep_opts *opts, expv_mi_tscache_t caches,
                          expv_mi_timestep_stats *stats);
/* expv_mi_phiv_timestep for a REAL operator with B, U and the caches of its complex type (mixed calls, see expv_mi_arnoldi).  The W
 * recurrence applies the operator with expv_mi_op_apply_complex's mul! and adds the columns of B in a second pass; ncoef = 1 is
 * expv_timestep!.  A complex operator is EXPV_MI_ARGUMENT_ERROR "phiv_timestep_realop: ...". */
int expv_mi_phiv_timestep_realop(expv_mi_ctx_t ctx, expv_mi_op_t op, int nts, double *ts, const void *B,
                                 int64_t ldb, int ncoef, int b_loc, void *U, int64_t ldu, int u_loc,
                                 const expv_mi_timestep_opts *opts, expv_mi_tscache_t caches,
                                 expv_mi_timestep_stats *stats);

/* kiops(tau_out, A, u; mmin, mmax, m, tol, iop, ishermitian, task1)  (kiops.jl:57-281).
 * u is n x ncols_u; w is n x 1 (numSteps = size(tau_out,2) = 1 is the only reachable case, see
 * DESIGN.md); stats = (step, reject, krystep, exps, m_ret).  For dtype C64 (no reference method)
 * the mathematical extension is computed and w is complex.
 * Round 6: a device-resident w is complete on return unless the context's outputs are stream-ordered (expv_mi_ctx_set_async_outputs): then it is
 * valid for later work on the context's stream / after expv_mi_ctx_sync, like every other result, and back-to-back calls overlap one call's solution
 * update with the next call's first launches.  After a rejected sub-step the basis is continued behind the closing pass of the rejected factorisation
 * instead of recomputing its last step (context option "kiops_skip_redo"); the statistics tuple is the reference's either way. */
typedef struct {
  int32_t mmin, mmax, m, iop, ishermitian, task1, ortho, reserved;
  double tol;
} expv_mi_kiops_opts;
void expv_mi_kiops_opts_default(expv_mi_kiops_opts *o);
int expv_mi_kiops(expv_mi_ctx_t ctx, expv_mi_op_t op, const double *tau_out, int ntau, int tau_ncols,
                  const void *u, int64_t ldu, int ncols_u, int u_loc, void *w, int64_t ldw, int w_loc,
                  const expv_mi_kiops_opts *opts, int64_t stats[5]);

/* ------------------------------------------------------------------ batch ------------ */
/* nprob independent problems expv(t[p], A_p, b[:, p]; m, tol, iop, ishermitian) of equal size n whose
 * operators share ONE sparsity pattern (BASELINE config 5): rowptr[n+1] / colind[nnz_per_prob] (CSR32,
 * 0-based) once, vals = nnz_per_prob values per problem, problem-major; b and w are n x nprob.
 * The problems advance in lock step (problem index in blockIdx.y of every launch); each keeps its own
 * Hessenberg matrix and happy-breakdown state, m_used[p] = Ks.m of problem p.  ishermitian applies to all.
 * rowptr / colind are host arrays; mat_loc says where `vals` lives. */
int expv_mi_expv_batch(expv_mi_ctx_t ctx, int dtype, int64_t n, int nprob, const int32_t *rowptr,
                       const int32_t *colind, const void *vals, int64_t nnz_per_prob, int mat_loc,
                       const double *t, const void *b, int64_t ldb, int b_loc, void *w, int64_t ldw,
                       int w_loc, const expv_mi_arnoldi_opts *opts, int32_t *m_used);

/* The same batch over SEVERAL GPUs of one node from ONE host process (the Julia shim's way to run BASELINE config 5: a Julia
 * host has no torch.distributed).  ctxs[0..nctx) are contexts on the participating devices; problem p goes to context
 * floor(p * nctx / nprob)-style contiguous blocks (first nprob % nctx contexts get one more), every shard runs in its own
 * host thread, nothing is exchanged between the shards while they run, and the FINAL GATHER of the
 * result columns happens here: w_loc = EXPV_MI_HOST -> each shard writes its columns of the caller's host matrix;
 * w_loc = EXPV_MI_DEVICE -> w lives on ctxs[0]'s device and the other shards' blocks arrive by peer copies over xGMI
 * (hipMemcpyPeerAsync; within one process peer copies ARE the xGMI collective -- RCCL is what the one-process-per-GPU
 * form uses, exponentialutilities.jl_amd/dist.py).  vals, t, b are host arrays (mat_loc / b_loc must be EXPV_MI_HOST).
 * Returns the first failing shard's status; expv_mi_last_error(ctxs[k]) has the message. */
int expv_mi_expv_batch_multi(expv_mi_ctx_t *ctxs, int nctx, int dtype, int64_t n, int nprob, const int32_t *rowptr,
                             const int32_t *colind, const void *vals, int64_t nnz_per_prob, const double *t,
                             const void *b, int64_t ldb, void *w, int64_t ldw, int w_loc,
                             const expv_mi_arnoldi_opts *opts, int32_t *m_used);

/* ------------------------------------------------------------------ final gather over RCCL ---------- */
/* BASELINE configs[4] in the one-process-per-GPU form: every rank solves its block of the independent problems with
 * expv_mi_expv_batch on its own context (nothing is exchanged while they run) and the result blocks meet in
 * ONE all-gather over xGMI.  The reference has no counterpart ("Distributed: none"); the Python harness does
 * the same gather through torch.distributed (exponentialutilities.jl_amd/dist.py), a Julia host -- which has no torch.distributed --
 * through these four calls.  librccl.so is opened at first use (dlopen): the library links nothing of RCCL.
 *   expv_mi_rccl_available()        1 when librccl.so and its four entry points were found
 *   expv_mi_rccl_unique_id(id128)   rank 0 fills 128 bytes (ncclGetUniqueId); the host hands them to the other ranks by its own means
 *                                   (MPI.jl, Distributed.jl, a file)
 *   expv_mi_comm_create(ctx, id128, nranks, rank, &comm)   collective over the nranks processes (ncclCommInitRank on ctx's device)
 *   expv_mi_gather_rccl(comm, send, recv, count, dtype)    ncclAllGather of `count` elements per rank on the CONTEXT's stream, behind
 *                                   whatever the context has queued: recv (device, nranks * count elements) holds rank r's block at
 *                                   r * count.  Complete on return unless the context's outputs are stream-ordered.  With contiguous
 *                                   shards of n-row columns, count = n * columns_per_rank gives the n x nprob result matrix on every rank
 *   expv_mi_comm_destroy(comm)
 * Status EXPV_MI_UNSUPPORTED when librccl.so is missing, EXPV_MI_HIP_ERROR with the RCCL message in expv_mi_last_error otherwise. */
int expv_mi_rccl_available(void);
int expv_mi_rccl_unique_id(void *id128);
int expv_mi_comm_create(expv_mi_ctx_t ctx, const void *id128, int nranks, int rank, expv_mi_comm_t *comm);
int expv_mi_gather_rccl(expv_mi_comm_t comm, const void *send_dev, void *recv_dev, int64_t count, int dtype);
int expv_mi_comm_destroy(expv_mi_comm_t comm);

/* ------------------------------------------------------------------ ABI self-description -- */
/* sizeof and field layout of the option / result structs as THIS library was compiled, so a host language that restates
 * them (Julia `struct`, ctypes.Structure) can verify its layout at load time instead of trusting the header by eye.
 * layout string: "name:type@offset,..." with type in {i32, i64, f64, ptr}. */
enum {
  EXPV_MI_ABI_ARNOLDI_OPTS = 0, EXPV_MI_ABI_EXPV_STATS = 1, EXPV_MI_ABI_TIMESTEP_OPTS = 2,
  EXPV_MI_ABI_TIMESTEP_STATS = 3, EXPV_MI_ABI_KIOPS_OPTS = 4, EXPV_MI_ABI_COUNT = 5
};
size_t expv_mi_abi_sizeof(int kind);
const char *expv_mi_abi_layout(int kind);

/* ------------------------------------------------------------------ host small-dense ---- */
/* The m x m pieces that stay on the host (north_star); exported so a host language can reuse them
 * and so they can be tested without a GPU.
 * exponential!(A, ExpMethodHigham2005Base()), in place  (exp_baseexp.jl:112-161) */
/* Host only (no GPU needed): which storage forms expv_mi_op_create_csr/_csc would build for a 0-based CSR32 pattern and
 * therefore which factorisation path the operator takes.  out[0] SELL slices built,
 * out[1] max |col - row|, out[2] diagonals of the DIA form of the banded pipeline (0: none), out[3] diagonals of the
 * general DIA form (0: none), out[4] its largest |offset|, out[5] reach in rows of the SELL wave form (-1: n/a),
 * out[6] rows sorted and free of duplicates, out[7] slot cut-off of the SELL form (0: regular rows, every slice keeps its longest
 * row; > 0: irregular rows -- the entries of a row beyond the cut are applied from the CSR arrays by the overflow pass).  No reference counterpart (the reference stores CSC only). */
int expv_mi_host_pattern_info(int64_t n, const int32_t *rowptr, const int32_t *colind, int dtype, int64_t out[8]);
/* Host only: the scalar CSR pattern expv_mi_op_create_dia_loc makes of stored diagonals (its position contract), and its host-side
 * checks -- the SAME validation function, with the same status and messages (read them with expv_mi_last_error(NULL)); the checks
 * on `data` and `loc` have no counterpart here.  rowptr[n + 1], colind[nnz] and src[nnz] may each be NULL; src[p] is the element
 * index into `data` that position p reads.  out = {nnz, in-range diagonals q, smallest in-range offset, largest in-range offset}
 * (the offsets are 0 when q = 0); out is written before the arrays, so a first call with NULL arrays sizes them. */
int expv_mi_host_dia_pattern(int64_t n, int ndiag, const int64_t *offsets, int64_t ld, int align,
                             int32_t *rowptr, int32_t *colind, int64_t *src, int64_t out[4]);
/* The ordering expv_mi_op_create_* would compute for this pattern (host only: reverse Cuthill-McKee on A + A'): perm[i] = the row
 * that becomes row i; out[0] / out[1] = max |col - row| before / after, out[2] / out[3] = step form before / after (3 single-pass
 * halo form, 2 wave form, 1 two-kernel step, 0 two-kernel step + overflow pass); out[2] has bit 8 (256) set when operator
 * creation would keep the ordering (option "reorder" = 1).  perm may be NULL. */
int expv_mi_host_rcm(int64_t n, const int32_t *rowptr, const int32_t *colind, int dtype, int32_t *perm, int64_t out[4]);
/* Content hash of a host buffer: out = {whole 8-byte words, sum_i mix64(x_i ^ (i + 1) g) mod 2^64 (+ the tail bytes as one more
 * word)}, mix64 = the two-round multiply / xor-shift finaliser, g = 0x9e3779b97f4a7c15; threaded.  Position-salted AND non-linear:
 * a permutation of the contents changes it (the linear index-weighted sum of round 3 did not, for mantissa-free values at
 * distances of 2048 k words).  For host mirrors that keep an uploaded copy of a caller's matrix and must notice in-place
 * changes (the reference reads A at call time, krylov_phiv.jl / arnoldi.jl mul!); no counterpart in the reference. */
int expv_mi_host_wrapsum(const void *buf, uint64_t nbytes, uint64_t out[2]);
int expv_mi_host_expm(int dtype, int n, void *A, int lda);
/* The balancing step of expv_mi_host_expm on its own (xGEBAL job 'B'; needs no GPU): A (column-major, leading dimension lda) is
 * balanced in place in its own element type; *ilo, *ihi 1-based, scale (n doubles) in LAPACK's convention.  Any of the three may
 * be NULL.  Unlike expv_mi_gebal the norms are summed in the element type's real type. */
int expv_mi_host_gebal(int dtype, int n, void *A, int lda, int64_t *ilo, int64_t *ihi, double *scale);
/* Z*(exp.(t*lambda).*Z[1,:]) of SymTridiagonal(d, e)  (krylov_phiv.jl:227-228); out: n complex */
int expv_mi_host_symtridiag_expcol(int n, const double *d, const double *e, double t_re, double t_im,
                                   double *out_c64);
/* Its last entry alone, e_n' exp(t T) e_1 -- what the per-step stopping test of the error-estimate mode reads
 * (krylov_phiv_error_estimate.jl:197) -- from the first and last rows of the eigenvector matrix only: O(n^2) instead of O(n^3),
 * bit for bit the entry the full product gives; out: one complex */
int expv_mi_host_symtridiag_exp_last(int n, const double *d, const double *e, double t_re, double t_im,
                                     double *out_c64);
/* phiv_dense!(w, A, v, k)  (phi.jl:84-115); w is m x (k+1) packed */
int expv_mi_host_phiv_dense(int dtype, int m, int k, const void *A, int lda, const void *v, void *w);

#ifdef __cplusplus
}
#endif
#endif /* EXPV_MI_H */
