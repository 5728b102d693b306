/*
 * spblas_gfx950.h -- C ABI of the MI355X (gfx950 / CDNA4) Sparse BLAS backend for
 * the spblas-reference view/operator API.
 *
 * This is the drop-in boundary.  The reference has no runtime
 * plugin ABI of its own: a backend is a set of C++ overloads compiled in with
 * -DSPBLAS_ENABLE_<NAME> whose bodies call a vendor C library.  The entry points
 * below are exactly what our overload set (the headers under
 * include/spblas/vendor/gfx950/) binds, one for each vendor-library call the existing AMD slot makes
 * (paths relative to /root/reference/include/spblas/):
 *
 *   rocsparse_create_handle / rocsparse_set_stream / rocsparse_destroy_handle
 *       vendor/rocsparse/detail/abstract_operation_state.hpp:20-28,
 *       vendor/rocsparse/multiply_spgemm.hpp:34-43      -> spblas_gfx950_create/destroy/set_stream
 *   rocsparse_spmv(..., stage_buffer_size) + allocate_workspace
 *       vendor/rocsparse/detail/spmv_impl.hpp:60-69     -> spblas_gfx950_spmv_plan_create  (multiply_inspect)
 *   rocsparse_spmv(..., stage_compute)
 *       vendor/rocsparse/detail/spmv_impl.hpp:72-77     -> spblas_gfx950_spmv
 *   oneapi::mkl::sparse::gemm (the only device SpMM in the reference)
 *       vendor/onemkl_sycl/spmm_impl.hpp:116-120        -> spblas_gfx950_spmm
 *   rocsparse_spgemm stage_buffer_size + stage_nnz + rocsparse_spmat_get_size
 *       vendor/rocsparse/multiply_spgemm.hpp:94-115     -> spblas_gfx950_spgemm_symbolic (multiply_compute)
 *   rocsparse_spgemm stage_compute / stage_symbolic / stage_numeric
 *       vendor/rocsparse/multiply_spgemm.hpp:137-213    -> spblas_gfx950_spgemm_numeric  (multiply_fill / multiply_numeric)
 *
 * Conventions
 *   - Plain C: pointers, sizes, enums.  No C++/torch types cross this boundary.
 *   - Every array pointer is a DEVICE pointer owned by the caller (csr_view is
 *     non-owning, views/csr_view.hpp:12-77).  alpha/beta are HOST pointers to one
 *     scalar of the value type.  The library never frees caller memory.
 *   - Work is enqueued on the handle's hipStream_t and is asynchronous with respect
 *     to the host, like the rocSPARSE slot; the only host synchronisations are in
 *     plan creation and in spgemm_symbolic (it must return nnz(C), as
 *     rocsparse_spmat_get_size does at multiply_spgemm.hpp:114-115).
 *   - Every function returns a spblas_gfx950_status; the C++ header layer maps
 *     them to the reference's exception types (std::invalid_argument for shape
 *     errors, std::runtime_error otherwise, std::bad_alloc for allocation).
 *   - Zero-based indices; column indices within a row may be unsorted and may
 *     repeat (backend/generate.hpp:112-117 shuffles them).
 *   - One handle / plan per host thread; no internal locking (the reference makes
 *     no thread-safety statement either).
 */
#ifndef SPBLAS_GFX950_H
#define SPBLAS_GFX950_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spblas_gfx950_handle_s* spblas_gfx950_handle_t;
typedef struct spblas_gfx950_plan_s* spblas_gfx950_plan_t;
typedef struct spblas_gfx950_spgemm_s* spblas_gfx950_spgemm_t;
typedef struct spblas_gfx950_trsv_s* spblas_gfx950_trsv_t;
typedef struct spblas_gfx950_ilu0_s* spblas_gfx950_ilu0_t;
typedef struct spblas_gfx950_multicolor_s* spblas_gfx950_multicolor_t;
typedef struct spblas_gfx950_permute_s* spblas_gfx950_permute_t;
typedef struct spblas_gfx950_aggregate_s* spblas_gfx950_aggregate_t;
typedef struct spblas_gfx950_coarsen_s* spblas_gfx950_coarsen_t;
typedef struct spblas_gfx950_smooth_s* spblas_gfx950_smooth_t;
typedef struct spblas_gfx950_gs_s* spblas_gfx950_gs_t;

typedef enum spblas_gfx950_status {
  SPBLAS_GFX950_STATUS_SUCCESS = 0,
  SPBLAS_GFX950_STATUS_INVALID_HANDLE = 1,
  SPBLAS_GFX950_STATUS_INVALID_POINTER = 2,
  SPBLAS_GFX950_STATUS_INVALID_SIZE = 3,  /* shape mismatch -> std::invalid_argument */
  SPBLAS_GFX950_STATUS_INVALID_VALUE = 4, /* bad enum / flag */
  SPBLAS_GFX950_STATUS_NOT_SUPPORTED = 5,
  SPBLAS_GFX950_STATUS_ALLOC_FAILED = 6,       /* -> std::bad_alloc */
  SPBLAS_GFX950_STATUS_HIP_ERROR = 7,          /* see spblas_gfx950_last_hip_error */
  SPBLAS_GFX950_STATUS_INSUFFICIENT_SPACE = 8, /* "SpGEMM ran out of memory" */
  SPBLAS_GFX950_STATUS_PLAN_MISMATCH = 9       /* plan built for a different matrix */
} spblas_gfx950_status;

typedef enum spblas_gfx950_datatype {
  SPBLAS_GFX950_F32 = 0, /* float  : vendor/rocsparse/types.hpp:42-44 */
  SPBLAS_GFX950_F64 = 1, /* double : vendor/rocsparse/types.hpp:47-49 */
  /* complex, interleaved (re, im) like std::complex<float / double>; alpha / beta point at ONE complex host scalar.
   * SpMV (op N) and SpMM on CSR with int32 columns only: spmv_plan_create (AUTO / VECTOR / ROWBLOCK; SLICED returns
   * STATUS_NOT_SUPPORTED), spblas_gfx950_spmv[_conj], spblas_gfx950_spmm[_strided[_conj]].  The other entry points that take a
   * value type (spgemm_numeric[_addend], csr_add_numeric, csr_transpose, scale, sptrsv_solve, sptrsm_solve, sptrsv_sweeps,
   * ilu0_factor, ilu0_sweeps, csr_permute_values, permute_vector, gs_sweep) return STATUS_NOT_SUPPORTED for them, before any other check; so do plan_update_values / plan_detach and the
   * two-stage / multi-GPU calls on a complex plan. */
  SPBLAS_GFX950_C32 = 2, /* std::complex<float>  */
  SPBLAS_GFX950_C64 = 3, /* std::complex<double> */
  /* 16-bit values; alpha / beta point at ONE float each.  Products and sums are formed in fp32 and every output element is
   * rounded to the 16-bit type once (round-to-nearest-even; beta * y is added in fp32 before that rounding).  SpMV (op N)
   * and SpMM on CSR with int32 columns only: spmv_plan_create (AUTO / VECTOR / ROWBLOCK; AUTO never picks SLICED, SLICED
   * returns STATUS_NOT_SUPPORTED), spblas_gfx950_spmv, spblas_gfx950_spmm[_strided], spmm_inspect.  op = T, the _conj entry
   * points and every other entry point that takes a value type (spgemm_numeric[_addend], csr_add_numeric, csr_transpose,
   * scale, sptrsv_solve, sptrsm_solve, sptrsv_sweeps, ilu0_factor, ilu0_sweeps, csr_permute_values, permute_vector, gs_sweep) return
   * STATUS_NOT_SUPPORTED for them,
   * before any other check; so do plan_update_values / plan_detach / spmv_expand / spmv_reduce_rows on a 16-bit plan. */
  SPBLAS_GFX950_F16 = 4, /* IEEE binary16 (torch.float16) */
  SPBLAS_GFX950_BF16 = 5 /* bfloat16 (torch.bfloat16)     */
} spblas_gfx950_datatype;

typedef enum spblas_gfx950_indextype {
  SPBLAS_GFX950_I32 = 0, /* vendor/rocsparse/types.hpp:11-12 (index_t = offset_t = int32_t) */
  SPBLAS_GFX950_I64 = 1  /* row offsets only; column indices are always int32 */
} spblas_gfx950_indextype;

typedef enum spblas_gfx950_operation {
  SPBLAS_GFX950_OP_N = 0, /* csr_view                      (vendor/rocsparse/detail/get_transpose.hpp:25-26) */
  SPBLAS_GFX950_OP_T = 1  /* csc_view / transposed(csr)    (vendor/rocsparse/detail/get_transpose.hpp:27-28) */
} spblas_gfx950_operation;

/* SpMV algorithm selector (plan creation).  AUTO picks from the row statistics. */
typedef enum spblas_gfx950_spmv_alg {
  SPBLAS_GFX950_SPMV_AUTO = 0,
  SPBLAS_GFX950_SPMV_VECTOR = 1,   /* sub-wavefront group per row, no plan data */
  SPBLAS_GFX950_SPMV_ROWBLOCK = 2, /* nnz-window row blocks staged through LDS   */
  SPBLAS_GFX950_SPMV_SLICED = 3    /* column-sliced reorder (x slice L2-resident) */
} spblas_gfx950_spmv_alg;

/* ---- library / handle ---------------------------------------------------- */
int spblas_gfx950_version(void);
const char* spblas_gfx950_status_string(int status);
/* hipError_t of the most recent STATUS_HIP_ERROR on this thread (0 if none). */
int spblas_gfx950_last_hip_error(void);

/* stream: a hipStream_t (NULL = the null stream), cf. hip_allocator(hipStream_t),
 * vendor/rocsparse/hip_allocator.hpp:22.
 * Graph capture: the execute calls that take a plan or a state whose structure is known (spblas_gfx950_spmv,
 * spblas_gfx950_spmm, spblas_gfx950_sptrsv_solve / _sptrsm_solve, spblas_gfx950_ilu0_factor / _ilu0_sweeps, spblas_gfx950_spgemm_numeric after the first fill) only launch kernels
 * and memsets on this stream and may be recorded with hipStreamBeginCapture and replayed.  Nothing is allocated on a
 * capturing stream: a call that would have to (plan creation, inspect, symbolic passes, the first execute of a plan that
 * sizes a workspace) returns SPBLAS_GFX950_STATUS_NOT_SUPPORTED there -- run it once outside the capture.
 * The FIRST handle a process creates loads the library's code objects on the current device (about 16 ms on MI355X, once):
 * the runtime would otherwise load each one at the first launch of one of its kernels -- 5.5 of the 9 ms of a first
 * multiply_inspect, 2.2 of the 3.2 ms of a first multiply_compute.  SPBLAS_GFX950_PRELOAD=0 in the environment leaves it to
 * the first use. */
int spblas_gfx950_create(spblas_gfx950_handle_t* handle, void* stream);
int spblas_gfx950_destroy(spblas_gfx950_handle_t handle);
int spblas_gfx950_set_stream(spblas_gfx950_handle_t handle, void* stream);
int spblas_gfx950_get_stream(spblas_gfx950_handle_t handle, void** stream);

/* Handle options consulted by later plan creations. */
typedef enum spblas_gfx950_option {
  /* Row-sharded multi-GPU runs gather y stripe by stripe (spblas-reference_amd/sharded.py).
   * value > 0 asks the SLICED inspect to put its row-bin boundaries on divisors of `value`
   * (the stripe length), so that spblas_gfx950_spmv_reduce_rows can finish whole stripes. */
  SPBLAS_GFX950_OPT_BIN_ROW_ALIGN = 1,
  /* value > 0 caps the slice split K of spblas_gfx950_spmv_reduce_rows (0 = heuristic only).  Callers
   * that run the reduces of several stripes side by side on different streams keep K small so the
   * partial-sum traffic does not grow with the number of stripes. */
  SPBLAS_GFX950_OPT_MAX_KSPLIT = 2,
  /* value = 1 lets plan creation with alg = AUTO choose the SLICED plan, which re-tiles A and keeps a COPY
   * of its values.  Default 0: AUTO only picks plans that read the caller's value array on every multiply,
   * which is what the reference's CPU path and the rocSPARSE slot do (algorithms/multiply_impl.hpp:48-52,
   * vendor/rocsparse/detail/spmv_impl.hpp:72-77).  The host layers set it for operands wrapped in
   * matrix_opt (views/matrix_opt_impl.hpp: the view that owns a vendor-optimised form of the matrix), the
   * same opt-in oneMKL's optimize_* stage gets in vendor/onemkl_sycl/spmm_impl.hpp:48-61.  Asking for
   * alg = SLICED explicitly needs no option.
   * value = 2: as 1, and the caller announces that the values WILL change (a time-stepping solver): SLICED snapshot
   * plans -- chosen by AUTO or requested explicitly -- keep the source position of every entry from the start (+4 B per
   * entry), so that the first spblas_gfx950_spmv_plan_update_values is a gather like every later one instead of a second
   * inspect (see the value snapshot contract below). */
  SPBLAS_GFX950_OPT_VALUE_SNAPSHOT = 3,
  /* value = 1: the caller GUARANTEES that a c_colind array it passes to spblas_gfx950_spgemm_numeric[_addend] still
   * holds what the previous numeric call on the same state wrote there whenever it is the same address; repeated
   * fills of one result then leave the column indices alone (cfg5: 1.40 -> 0.94 ms per fill).  Default 0: every
   * numeric call writes c_colind -- an equal address proves nothing (allocators hand freed addresses out again:
   * the reference's SpGEMMReuseAndChangePointer test does exactly that, test/gtest/device/spgemm_reuse_test.cpp:325). */
  SPBLAS_GFX950_OPT_SPGEMM_KEEP_COLIND = 4,
  /* SLICED plans store their products with plain stores (value 0, the default) or with the non-temporal hint
   * (value 1).  value 2 = decide by a timed trial: the first plan of this HANDLE with >= 32 M placed entries per
   * value size runs eight SpMVs on a zero vector at inspect and the handle keeps the faster flavour for its later
   * plans.  Which flavour wins is a property of the machine (-1...-4 % where the reduce pays for the expand's
   * write-backs, +3 % where it does not); the trial roughly doubles the first inspect, so it is for callers who
   * will run hundreds of multiplies.  Results are identical either way.  The environment variable
   * SPBLAS_GFX950_PB_NT = 0 / 1 / -2 (trial) overrides the option for reproducible runs. */
  SPBLAS_GFX950_OPT_STORE_TRIAL = 5
} spblas_gfx950_option;
int spblas_gfx950_set_option(spblas_gfx950_handle_t handle, int option, int64_t value);

/* ---- SpMV:  y = alpha * op(A) * x + beta * y ------------------------------ */
/* multiply_inspect(A, x, y): device-side analysis of the sparsity pattern.
 * Builds the nnz-window row partition, the long-row list and (SLICED) the
 * column-sliced reorder; the result lives in device memory owned by the plan.
 * `values` may be NULL unless alg == SLICED.
 * Value snapshot contract: ROWBLOCK / VECTOR plans hold structure only and every multiply reads the
 * caller's values.  The SLICED plan holds a re-tiled COPY of the values.  On request (alg = SLICED) or by AUTO under
 * SPBLAS_GFX950_OPT_VALUE_SNAPSHOT the copy is a SNAPSHOT: after changing the values IN PLACE call
 * spblas_gfx950_spmv_plan_update_values; a multiply that passes a DIFFERENT values pointer than the one
 * the copy was taken from refreshes the copy by itself first (one extra pass over A).  A snapshot plan keeps no source
 * positions until then: the FIRST refresh builds the plan again from the caller's arrays (inspect-class work: not inside a
 * stream capture: STATUS_NOT_SUPPORTED there, also from a spblas_gfx950_spmv that meets a new values pointer) and keeps
 * them, every later refresh is a gather (option value 2 above: kept from the start).  If that second build runs out of memory
 * or declines, the plan falls back to its structure-only form (row-block windows on the caller's arrays, plan_info[0]
 * changes) and the call succeeds: a plan is never left half built.  AUTO WITHOUT the option may choose the SLICED plan
 * too (>= 16 M entries, not skewed): such a plan reads the caller's values on EVERY multiply (plan_info_sliced[9] bit 6),
 * so the caller sees the same semantics as with a structure-only plan.  Its default form is VALUE-FREE (bit 7, round 5):
 * the plan holds no values at all -- the first kernel gathers x, the second multiplies by the caller's array, staged bin by
 * bin through LDS; where that form does not apply, the copying form of round 4 (a value refresh per multiply, kept only
 * if it beats the row-block kernel by rule -- x of 32 MB or more -- or, with SPBLAS_GFX950_AUTO_TRIAL=1, in a timed trial).
 * The calls that are not given the values -- the two-stage calls (spmv_expand / spmv_reduce_rows) and the multi-GPU steps
 * (spmv_reduce_rows_bcast, spmv_step_bcast[_chunked]) -- refuse the COPYING form.  Since round 6 the value-free form is
 * accepted by spmv_reduce_rows_bcast and spmv_step_bcast: it reads the value array registered with the plan (plan_create,
 * the last spblas_gfx950_spmv, plan_update_values) as it is when the step runs -- no copy that could go stale.
 * The plan is tied to (m, n, nnz, rowptr, colind). */
int spblas_gfx950_spmv_plan_create(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t* plan,
                                   int64_t m, int64_t n, int64_t nnz, const void* rowptr,
                                   const int32_t* colind, const void* values, int offset_type,
                                   int value_type, int alg);
int spblas_gfx950_spmv_plan_update_values(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan,
                                          const void* values);
/* The owner of a plan declares that it is about to RELEASE the arrays the plan was built from -- what a host layer does
 * for an inspected csc_view / transposed(csr) operand, whose row-major form it materialised for the plan alone
 * (vendor/rocsparse/detail/get_transpose.hpp:19-29 has rocSPARSE do the transposition inside the call; here it is done
 * once, at inspect).  Succeeds only for a self-contained plan: SLICED with its own copy of the values, no hub rows, no
 * hot-column split (STATUS_NOT_SUPPORTED otherwise: keep the arrays).  Afterwards spblas_gfx950_spmv with this plan takes
 * rowptr = colind = values = NULL (op = N, same m / n / nnz / types), plan_update_values returns STATUS_NOT_SUPPORTED (the
 * values changed: inspect again), spblas_gfx950_spmm does not accept the plan.  cfg2-sized transposed operand: the inspected
 * form holds 1.43 x the matrix instead of 2.43 x. */
int spblas_gfx950_spmv_plan_detach(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan);
/* A plan carries workspaces (products, partial sums): it must not run on two streams at once.  plan_destroy frees on
 * the handle's current stream, ordered behind the last launch that used the plan on whichever stream that was.  The same
 * holds for EVERY destroy of this header -- spblas_gfx950_sptrsv_destroy, _ilu0_destroy, _gs_destroy, _multicolor_destroy,
 * _csr_permute_destroy, _aggregate_destroy, _coarsen_destroy, _smooth_destroy, _spgemm_destroy -- and for a symbolic pass that replaces the
 * result a SpGEMM state holds: each owner remembers the stream of its last use, and its arrays are freed (stream-ordered, on the handle's current stream) behind an
 * event recorded there; the host is not blocked, except that sptrsv_destroy waits for the stream of the last solve before
 * it releases the plan's pinned status word.  Nothing is inserted while the handle's stream is being captured.  Two USES of
 * one owner on different streams are not ordered against each other: that stays the caller's business. */
int spblas_gfx950_plan_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan);
/* Introspection for tests/bench: info[0]=alg, [1]=window nnz, [2]=#windows,
 * [3]=#long rows, [4]=max row length, [5]=device bytes held, [6]=#column slices,
 * [7]=#empty rows, [8]=rows per row-bin (SLICED), [9]=1 if the bins honour BIN_ROW_ALIGN,
 * [10]=#expand work items, [11]=#reduce work items (SLICED plans of skewed matrices; else 0). */
int spblas_gfx950_plan_info(spblas_gfx950_plan_t plan, int64_t info[12]);
/* More of a SLICED plan (zeros for other plans): info[0]=#row-bins, [1]=1 if the bins have variable heights (row-skewed
 * matrix: a new bin every [8] rows and every ~nnz/2048 entries), [2]=blocks of 32 entries in expand order,
 * [3]=blocks in reduce order (bins padded to groups of 8 blocks), [4]=entries placed in tiles, [5]=#rows kept out of
 * the tiles (hub rows), [6]=hub threshold (row length), [7]=reduce K split, [8]=rows the tiles are built over (fewer
 * than m when the empty rows were taken out).  For ANY plan: [9] bit 0 = AUTO decided by a timed trial, bit 1 = the
 * reduce streams one-byte row codes (runs sorted by row) instead of 16-bit rows, bit 2 = the expand stores its products
 * with the non-temporal hint, bit 3 = this plan ran the store trial that decides bit 2 (plans with >= 32 M placed
 * entries, once per process, device and value size; SPBLAS_GFX950_PB_NT=0/1 forces the flavour), bit 4 = hot-column
 * split (plan_info_hot), bit 6 = the plan reads the caller's values on every multiply (made without the snapshot opt-in),
 * bit 7 = ... and holds no copy of them (value-free tiles); [10]/[11]=time of the
 * row-block / the sliced plan in AUTO's trial, nanoseconds -- or, when only the store trial ran, of one SpMV with plain /
 * non-temporal product stores. */
int spblas_gfx950_plan_info_sliced(spblas_gfx950_plan_t plan, int64_t info[12]);
/* Hot-column split of a SLICED plan (column-skewed matrices, csrc/spmv_hot.hip): [0] hot columns, [1] entries multiplied
 * in row order with those x values in LDS, [2] rows that have such entries, [3] of them longer than a window, [4] entries
 * left to the tiles, [5] device bytes of the tiled part, [6] windows of 256 entries the hot part is cut into, [7] = 0.
 * All 0 for a plan without the split. */
int spblas_gfx950_plan_info_hot(spblas_gfx950_plan_t plan, int64_t info[8]);
/* What the inspect laid out for the hot part of such a plan (a diagnostic for tests, like spmm_plan_blocks; no kernel
 * runs).  counts: [0] sampled references from which a column was taken, [1] hot columns K, [2] entries of A_hot, [3] rows
 * that have such entries, [4] windows of 256 entries, [5] rows that lie in more than one window, [6] workgroups the
 * multiply will launch (SPBLAS_GFX950_PB_HOT_GRID at inspect sets it: a test hook), [7] splits below this plan (2: the
 * remainder was split again, SPBLAS_GFX950_PB_HOT_DEPTH).  hot_cols ([1] ascending column numbers), hot_rows ([3] rows of
 * y), hot_rowptr ([3] + 1 offsets into A_hot, always 64 bits), win_row ([4] + 1: first row of A_hot that starts at or
 * behind each window's first entry) and cross_rows ([5] rows of A_hot, in no particular order) are HOST arrays, each may
 * be NULL; they are copied on the handle's stream, which is synchronised once.  A plan without the split reports eight
 * zeros and copies nothing.  NOT_SUPPORTED while the stream is capturing. */
int spblas_gfx950_plan_hot_layout(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int64_t counts[8],
                                  int32_t* hot_cols, int32_t* hot_rows, int64_t* hot_rowptr, int32_t* win_row,
                                  int32_t* cross_rows);

/* Two-stage execution of a SLICED plan (other plans: STATUS_NOT_SUPPORTED), used to overlap the
 * multi-GPU all-gather of finished y rows with the rest of the SpMV:
 *   expand       products of every stored entry with x (x read once, LDS-resident slices)
 *   reduce_rows  y[r] = alpha * (A x)[r] + beta * y[r] for the row-bins that START in
 *                [row_begin, row_end), from the products of the last expand.  `y` is the base of
 *                the full local y (entry r at y[r]).  spblas_gfx950_spmv == expand + reduce_rows(0, m).
 *                A plan of a row-skewed matrix that cuts its long rows into pieces (plan_info_sliced[8] > m or the
 *                plan was made without SPBLAS_GFX950_OPT_BIN_ROW_ALIGN on such a matrix) reduces all rows in ONE call:
 *                a proper sub-range returns STATUS_NOT_SUPPORTED there.  Plans created under OPT_BIN_ROW_ALIGN > 1 (what
 *                the striped multi-GPU step sets) never cut rows.
 * expand is not handed A's values: a plan that copies them on every multiply (a plain inspected csr_view below the size of
 * value-free tiles) returns STATUS_NOT_SUPPORTED from it.  A VALUE-FREE plan is taken -- its expand gathers x only, and its
 * reduce (spblas_gfx950_spmv_reduce_rows_bcast) reads the value array registered with the plan. */
int spblas_gfx950_spmv_expand(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, const void* x);
int spblas_gfx950_spmv_reduce_rows(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, const void* alpha,
                                   const void* beta, void* y, int64_t row_begin, int64_t row_end);

/* multiply(info, A, x, y) / multiply(A, x, y).  plan may be NULL (no inspect):
 * a plan-free kernel is chosen from nnz/m.  op == OP_T computes y = alpha*A^T*x
 * for an m x n CSR A (y has n entries, x has m): the CSC / transposed case.
 * op == OP_T without a plan, from 4 M entries and 65 536 columns on: the products go through a workspace in the handle's
 * scratch (6 B per fp32 entry, 10 B per fp64 entry + 4 B per (8 192-entry tile, column slice) pair; kept by the handle until
 * spblas_gfx950_destroy), 0.66 ms at 1e8 entries against 4.8 ms for one float atomic per entry -- which is what a call
 * recorded in a stream capture, or one the scratch cannot be allocated for, still does.  Either way the additions into one
 * element of y can come in another order on the next call (reproducibility); an inspected operand
 * (multiply_inspect on the csc_view) runs the CSR kernels, whose order is fixed. */
int spblas_gfx950_spmv(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int op, int64_t m,
                       int64_t n, int64_t nnz, const void* alpha, const void* rowptr,
                       const int32_t* colind, const void* values, const void* x, const void* beta,
                       void* y, int offset_type, int value_type);

/* Diagnostic, like plan_info: what the last spblas_gfx950_spmv with op == OP_T and no plan (real value types) did on this
 * handle.  Writes min(n_out, 8) entries: out[0] = path (SPMV_T_NONE before the first such call, SPMV_T_SCATTER: one atomic per
 * entry, SPMV_T_TWO_PASS: through the workspace); [1] = why the scatter kernel ran (SPMV_T_NOT_WANTED: below the size rule or
 * SPBLAS_GFX950_SPMV_T2=0, SPMV_T_DOES_NOT_FIT: more than 1 024 slices, no entries, or a count beyond 32 bits,
 * SPMV_T_CAPTURING: the stream is recording a graph, SPMV_T_NO_SCRATCH: the handle's scratch could not be sized; 0 for the
 * two-pass form); [2] = slice width W in columns, [3] = slices S, [4] = tiles of 8 192 entries -- the geometry the decision
 * was made on, reported for both paths --; [5] = segment length in entries (0 unless the two-pass form was wanted and fits);
 * [6] = 1 if a SPBLAS_GFX950_SPMV_T2_W test hook was set but ignored (below 64 or wider than the LDS holds); [7] = work items
 * of the accumulate pass, or -1 (scatter path, another call has taken the handle's scratch since, or the stream is
 * capturing).  [0] .. [6] are host integers; asking for [7] (n_out > 7) after a two-pass call copies one word back and
 * SYNCHRONISES the stream of that call.  Changes nothing about the multiply. */
#define SPBLAS_GFX950_SPMV_T_NONE 0
#define SPBLAS_GFX950_SPMV_T_SCATTER 1
#define SPBLAS_GFX950_SPMV_T_TWO_PASS 2
#define SPBLAS_GFX950_SPMV_T_NOT_WANTED 1
#define SPBLAS_GFX950_SPMV_T_DOES_NOT_FIT 2
#define SPBLAS_GFX950_SPMV_T_CAPTURING 3
#define SPBLAS_GFX950_SPMV_T_NO_SCRATCH 4
int spblas_gfx950_spmv_t_last(spblas_gfx950_handle_t handle, int64_t* out, int n_out);

/* Conjugated operands (complex types only): y = alpha * op'(A) * x' + beta * y with bit 0 of conj_flags = conj(A) (every stored
 * value conjugated) and bit 1 = conj(x).  conj_flags = 0 is spblas_gfx950_spmv itself; non-zero flags with a real value type
 * or bits above 1 return STATUS_INVALID_VALUE.  Complex values take op = N only (STATUS_NOT_SUPPORTED for op = T).  Products
 * are the componentwise formula (ac - bd, ad + bc) with the conjugations folded in as sign flips, accumulated in the value
 * type; no C Annex G inf / NaN recovery. */
int spblas_gfx950_spmv_conj(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int op, int64_t m, int64_t n,
                            int64_t nnz, const void* alpha, const void* rowptr, const int32_t* colind, const void* values,
                            const void* x, const void* beta, void* y, int offset_type, int value_type, int conj_flags);

/* ---- multi-GPU: fused all-gather of y (second stage) -------------------- */
/* One process per GPU; the reference has no multi-device path, so nothing is mirrored here.
 * ipc_alloc/export/open: every rank allocates its copy of the full y (and, with uncached = 1 because
 * it is polled while peers write it, a small flag array) with ipc_alloc, exports a 64-byte handle (hipIpcGetMemHandle) that it sends to the other ranks by any
 * host channel, and maps their buffers with ipc_open (hipIpcOpenMemHandle, peer access enabled).
 * spmv_reduce_rows_bcast: like spmv_reduce_rows with beta = 0, but local row r is stored as row
 * y_row_offset + r into ALL n_peers buffers of the DEVICE array y_peers (the local copy and the mapped
 * copies of the other ranks) -- on xGMI the traffic of a direct all-gather, issued by the reduce /
 * combine kernels themselves.  step_signal / step_wait: device-side barrier that ends a step:
 * signal stores `step` into slot `rank` of every rank's flag array (after the producing kernels on
 * the same stream), wait spins until all n_peers slots of the local array reached `step`
 * (status_dev[0] = 1 after timeout_ms without progress). */
int spblas_gfx950_ipc_alloc(size_t bytes, int uncached, void** ptr);
int spblas_gfx950_ipc_free(void* ptr);
int spblas_gfx950_ipc_export(void* ptr, unsigned char handle[64]);
int spblas_gfx950_ipc_open(const unsigned char handle[64], void** ptr);
int spblas_gfx950_ipc_close(void* ptr);
int spblas_gfx950_spmv_reduce_rows_bcast(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, const void* alpha,
                                         void* const* y_peers, int n_peers, int64_t y_row_offset,
                                         int64_t row_begin, int64_t row_end);
/* expand + reduce_rows_bcast of the whole local matrix in one call.  stripes > 1 cuts the row bins into
 * that many contiguous groups whose reduces alternate between the handle's stream and an auxiliary
 * stream owned by the handle, so that the link-bound peer stores of one stripe overlap the reduce of
 * the next; the handle's stream is joined with the auxiliary one before the call returns. */
int spblas_gfx950_spmv_step_bcast(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, const void* alpha,
                                  const void* x, void* const* y_peers, int n_peers, int64_t y_row_offset,
                                  int stripes);
/* Dependent iteration (x of step k + 1 is y of step k) with the peers' rows arriving BEHIND the next expand instead of in
 * front of it (round 4).  The reduce runs in `chunks` stripes as in spmv_step_bcast; after each stripe's peer stores a
 * small kernel on the same stream publishes slot rank * chunks + c = step in every rank's flag array (flag_peers: device
 * array of the n_peers flag arrays, int64[n_peers * chunks] each, uncached memory).  With `wait` the expand of THIS step --
 * whose x must be this rank's copy of the previous step's y -- waits, x slice by x slice, for the chunks that slice is made
 * of (own rows: stream order; bounded spin with s_sleep; a time-out sets status_dev[0] and lets the kernel finish) and reads
 * the slice with system-scope loads; status_dev[1] receives the longest wait of a workgroup in wall-clock ticks.  There is
 * no step barrier: a rank's step k + 2 overwrites copy k & 1 only after its expand has seen every rank's chunks of step
 * k + 1, which they publish after their expand of step k + 1 has read that copy.  spmv_chunk_rows: the local row
 * boundaries (chunks + 1, host) of the stripes -- every rank needs every rank's (chunk_rows of the wait descriptor: global
 * rows, device, int64[n_ranks * (chunks + 1)]).  Plans cut on the arithmetic bin grid only (row shards of a matrix with
 * uniform rows); STATUS_NOT_SUPPORTED otherwise.  Nothing here has been run across
 * devices yet: n ranks sharing one device exercise the code path (tests/mp_fused_worker.py), max_expand_workgroups
 * keeps their waiting expands from filling that one device. */
typedef struct spblas_gfx950_chunk_wait {
  const void* flags;          /* this rank's flag array */
  const int64_t* chunk_rows;  /* device */
  int n_ranks, chunks;
  int64_t step;               /* wait until the slots have reached this step */
  int64_t timeout_ms;
  int* status_dev;            /* device int[2] */
  int max_expand_workgroups;  /* 0 = one workgroup per x slice */
} spblas_gfx950_chunk_wait;
int spblas_gfx950_spmv_chunk_rows(spblas_gfx950_plan_t plan, int chunks, int64_t* rows);
int spblas_gfx950_spmv_step_bcast_chunked(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, const void* alpha,
                                          const void* x, void* const* y_peers, int n_peers, int64_t y_row_offset,
                                          int chunks, void* const* flag_peers, int rank, int64_t step,
                                          const spblas_gfx950_chunk_wait* wait);
int spblas_gfx950_step_signal(spblas_gfx950_handle_t handle, void* const* flag_peers, int n_peers, int rank,
                              int64_t step);
int spblas_gfx950_step_wait(spblas_gfx950_handle_t handle, const void* flags, int n_peers, int64_t step,
                            int64_t timeout_ms, int* status_dev);
/* Tick rate (kHz) of the device clock the waits above are bounded by and the wait statistics (status_dev[1] of a
 * chunk wait) are counted in: hipDeviceAttributeWallClockRate of the handle's device (100 MHz on gfx9).  No vendor call
 * replaced: rocSPARSE has no device-side waits. */
int spblas_gfx950_wall_clock_khz(spblas_gfx950_handle_t handle, int* khz);
/* One-shot: the NEXT spmv_reduce_rows_bcast on this handle issues step_wait(flags, n_peers, step, ...) right before the
 * kernel that stores into the peers' copies of y (the combine kernel when the reduce is K-split, else the reduce
 * itself).  Throughput form of the fused step for independent right-hand sides: expand and reduce of step k overlap
 * the peers' stores of step k-1. */
int spblas_gfx950_bcast_wait_before(spblas_gfx950_handle_t handle, const void* flags, int n_peers, int64_t step,
                                    int64_t timeout_ms, int* status_dev);

/* ---- SpMM:  C = alpha * A * B + beta * C,  B (k x n), C (m x n) row-major --- */
/* ldb/ldc are row strides in elements (mdspan layout_right, test/gtest/spmm_test.cpp).
 * multiply_inspect(A, B, C) = spmv_plan_create (alg ROWBLOCK: row statistics, long-row list) followed by
 * spmm_inspect, the counterpart of oneMKL's optimize_gemm (vendor/onemkl_sycl/spmm_impl.hpp:40-67): it probes every
 * block of 32 rows for column locality and hands the blocks whose entries fall into <= 8 aligned tiles of 128
 * columns (>= 1/5 dense: the measured crossover) to the LDS-staged matrix-core kernel (fp32; exact f32 MFMA).  spmm with such a plan
 * also cuts rows longer than the plan's nnz window into parts (hub rows of power-law matrices).  plan = NULL:
 * one lane group per row, no analysis.  spmm_plan_info: [0] inspected, [1] row blocks on the matrix cores,
 * [2] entries inside them, [3] long rows. */
int spblas_gfx950_spmm_inspect(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan);
int spblas_gfx950_spmm_plan_info(spblas_gfx950_plan_t plan, int64_t info[4]);
/* What spmm_inspect decided, block by block (a diagnostic for tests, like spmv_t_last; no kernel runs).  counts: [0]
 * inspected, [1] row blocks of 32 rows, [2] qualifying blocks, [3] those on the band path's matrix-core kernel, [4] entries in
 * the qualifying blocks, [5] band kernels (0: the tile kernel), [6] B rows staged per chunk, [7] wavefronts per workgroup
 * of the entry-loop kernel, [8] the per-mille window density of the matrix-core rule, [9] entries per tile a block had to
 * hold.  kind (counts[1] bytes: 0 row-group kernel, 1 entry loop / tile kernel, 2 matrix cores), win (2 per block:
 * smallest and largest column) and tiles (17 per block: count, then ascending tile ids) are HOST arrays, each may be NULL;
 * they are copied on the handle's stream, which is synchronised once.  A plan the probe did not run on (not fp32, fewer
 * than 256 entries, SPBLAS_GFX950_SPMM_NO_PANEL) reports ten zeros and copies nothing.  NOT_SUPPORTED while the stream is
 * capturing. */
int spblas_gfx950_spmm_plan_blocks(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int64_t counts[10],
                                   unsigned char* kind, int32_t* win, int32_t* tiles);
int spblas_gfx950_spmm(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int64_t m, int64_t k,
                       int64_t n, int64_t nnz, const void* alpha, const void* rowptr,
                       const int32_t* colind, const void* values, const void* B, int64_t ldb,
                       const void* beta, void* C, int64_t ldc, int offset_type, int value_type);
/* The same product for dense operands of either mdspan layout: element (i, j) of B lives at B[i*b_row_stride +
 * j*b_col_stride], likewise C.  The reference's CPU path takes any layout through mdspan's operator()
 * (backend/view_customizations.hpp:230-240; mdspan_col_major is a public alias, detail/mdspan.hpp:31-36).  Both
 * column strides 1 (layout_right): identical to spblas_gfx950_spmm with ldb / ldc = the row strides, plan included.
 * Any other combination of layout_right / layout_left operands (row stride 1 and column stride >= rows, or column
 * stride 1 and row stride >= n) runs a lane-group-per-row kernel whose gathers follow the strides; the plan is only
 * checked.  Overlapping layouts return STATUS_INVALID_SIZE. */
int spblas_gfx950_spmm_strided(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int64_t m, int64_t k,
                               int64_t n, int64_t nnz, const void* alpha, const void* rowptr,
                               const int32_t* colind, const void* values, const void* B, int64_t b_row_stride,
                               int64_t b_col_stride, const void* beta, void* C, int64_t c_row_stride,
                               int64_t c_col_stride, int offset_type, int value_type);

/* spblas_gfx950_spmm_strided with conjugated operands: bit 0 of conj_flags = conj(A), bit 1 = conj(B); the same rules as
 * spblas_gfx950_spmv_conj.  Complex plans use the plan's long-row list (rows longer than its window are cut into parts);
 * the matrix-core kernels are fp32 only. */
int spblas_gfx950_spmm_strided_conj(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int64_t m, int64_t k,
                                    int64_t n, int64_t nnz, const void* alpha, const void* rowptr,
                                    const int32_t* colind, const void* values, const void* B, int64_t b_row_stride,
                                    int64_t b_col_stride, const void* beta, void* C, int64_t c_row_stride,
                                    int64_t c_col_stride, int offset_type, int value_type, int conj_flags);

/* ---- SpGEMM:  C = alpha * A * B   (CSR x CSR -> CSR, int32 indices) -------- */
/* State object = spgemm_state_t (vendor/rocsparse/multiply_spgemm.hpp:28-230). */
int spblas_gfx950_spgemm_create(spblas_gfx950_handle_t handle, spblas_gfx950_spgemm_t* state);
int spblas_gfx950_spgemm_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_spgemm_t state);
/* multiply_compute / multiply_symbolic_compute: structural product.  Writes
 * c_rowptr[0..m] (device, caller-allocated: test/gtest/device/spgemm_test.cpp:37-40)
 * and returns nnz(C) = sum_i |union_{k in A_i} cols(B_k)| in *c_nnz (host).
 * Synchronises the stream once. */
int spblas_gfx950_spgemm_symbolic(spblas_gfx950_handle_t handle, spblas_gfx950_spgemm_t state, int64_t m,
                                  int64_t k, int64_t n, int64_t a_nnz, const int32_t* a_rowptr,
                                  const int32_t* a_colind, int64_t b_nnz, const int32_t* b_rowptr,
                                  const int32_t* b_colind, int32_t* c_rowptr, int64_t* c_nnz);
/* multiply_fill / multiply_symbolic_fill + multiply_numeric: fills c_colind
 * (ascending within each row, as spgemm_gustavsons.hpp:42 sorts them) and c_values.
 * c_capacity = entries available in c_colind / c_values; fewer than nnz(C) ->
 * STATUS_INSUFFICIENT_SPACE (csr_builder.hpp:18-22).  c_rowptr is rewritten from
 * the state's copy, so a different buffer than the one passed to symbolic is fine
 * (test/gtest/device/spgemm_reuse_test.cpp).  a_values/b_values may change between
 * calls; the pattern may not.
 * Memory held by the state: 8 bytes per entry of A from the symbolic pass on (the bounds of the B row
 * every A entry selects) and 16 bytes per row of 65..256 products that a wavefront can sort in one round
 * (spblas_gfx950_spgemm_info: "direct" rows); fp32 fills with many such rows keep an interleaved
 * (column, value) copy of B, 8 bytes per entry, rewritten by every fill; from the SECOND numeric pass on -- a one-shot fill pays nothing -- also one
 * byte per product of the rows with at most 256 products, two per product of the rows with 257..1024,
 * and 4 bytes per entry of C: later passes accumulate by recorded rank (SPBLAS_GFX950_SPGEMM_REUSE=0
 * in the environment keeps every pass on the hash kernels).  All of it is optional: an allocation
 * failure leaves the hash path in place. */
int spblas_gfx950_spgemm_numeric(spblas_gfx950_handle_t handle, spblas_gfx950_spgemm_t state, const void* alpha,
                                 const int32_t* a_rowptr, const int32_t* a_colind, const void* a_values,
                                 const int32_t* b_rowptr, const int32_t* b_colind, const void* b_values,
                                 int32_t* c_rowptr, int32_t* c_colind, void* c_values, int64_t c_capacity,
                                 int value_type);
/* Introspection of a state after spgemm_symbolic (no reference counterpart; the tests and bench.py use it):
 * info[0] = nnz(C), info[1] = rows with 65..256 products (the wave-per-row bin), info[2] = those of them that are
 * "direct" -- product count == structural length and an A row of one round of loads: sorted in registers by the
 * persistent kernel, no hash --, info[3] = 1 when later fills accumulate by recorded rank, info[4] = lanes that walk
 * one row of B together (4, 8 or 16, from B's mean row length; 0 before a symbolic pass), info[5] = rows with 1..64
 * products, info[6] = rows with 257..1024, info[7] = rows with more than 4096 (the dense accumulator).  The product
 * counts include the addend's row; a row the persistent kernel takes counts under info[1] whatever its count.  Rows
 * with 1025..4096 products are the rows of C minus info[1], info[5..7] and the rows without a product. */
int spblas_gfx950_spgemm_info(spblas_gfx950_spgemm_t state, int64_t info[8]);

/* Four-argument SpGEMM  C = alpha*A*B + beta*D  (the reference
 * surface is multiply_compute, multiply_fill, multiply_symbolic_compute, multiply_symbolic_fill and
 * multiply_numeric taking (state, a, b, c, d),
 * vendor/rocsparse/multiply_spgemm.hpp:118-214,237-274, with alpha = scale(a)*scale(b) and
 * beta = scale(d); expected values test/gtest/device/rocsparse/spgemm_4args_test.cpp:78-95).
 * set_addend registers D's pattern (m x n, int32) BEFORE spgemm_symbolic, which then counts
 * pattern(A*B) U pattern(D); passing d_rowptr = NULL removes it again.  After such a symbolic
 * pass the numeric step must be spgemm_numeric_addend (plain spgemm_numeric returns
 * STATUS_PLAN_MISMATCH, and vice versa).  beta is a HOST pointer like alpha. */
int spblas_gfx950_spgemm_set_addend(spblas_gfx950_handle_t handle, spblas_gfx950_spgemm_t state, int64_t d_nnz,
                                    const int32_t* d_rowptr, const int32_t* d_colind);
int spblas_gfx950_spgemm_numeric_addend(spblas_gfx950_handle_t handle, spblas_gfx950_spgemm_t state, const void* alpha,
                                        const int32_t* a_rowptr, const int32_t* a_colind, const void* a_values,
                                        const int32_t* b_rowptr, const int32_t* b_colind, const void* b_values,
                                        const void* beta, const int32_t* d_rowptr, const int32_t* d_colind,
                                        const void* d_values, int32_t* c_rowptr, int32_t* c_colind, void* c_values,
                                        int64_t c_capacity, int value_type);

/* ---- add:  C = alpha*A + beta*B  (CSR + CSR -> CSR, int32 indices) ------------------------ */
/* Device counterpart of add(a, b, c) / add_inspect / add_compute (algorithms/add_impl.hpp:40-115;
 * SURVEY.md section 8f rank 2).  Uses a spgemm state object (spblas_gfx950_spgemm_create): the
 * symbolic call is add_inspect -- it writes c_rowptr (m+1) and returns nnz(C) = structural size of
 * the union, add_impl.hpp:79-108 -- the numeric call is add_compute and may be repeated with new
 * values.  Columns of every output row are ascending (SPA + sort, add_impl.hpp:57-65).  alpha/beta
 * carry the scaled_view factors of a and b (HOST pointers); capacity < nnz(C) gives
 * STATUS_INSUFFICIENT_SPACE ("add: ran out of memory", add_impl.hpp:67-72). */
int spblas_gfx950_csr_add_symbolic(spblas_gfx950_handle_t handle, spblas_gfx950_spgemm_t state, int64_t m, int64_t n,
                                   int64_t a_nnz, const int32_t* a_rowptr, const int32_t* a_colind, int64_t b_nnz,
                                   const int32_t* b_rowptr, const int32_t* b_colind, int32_t* c_rowptr,
                                   int64_t* c_nnz);
int spblas_gfx950_csr_add_numeric(spblas_gfx950_handle_t handle, spblas_gfx950_spgemm_t state, const void* alpha,
                                  const int32_t* a_rowptr, const int32_t* a_colind, const void* a_values,
                                  const void* beta, const int32_t* b_rowptr, const int32_t* b_colind,
                                  const void* b_values, int32_t* c_rowptr, int32_t* c_colind, void* c_values,
                                  int64_t c_capacity, int value_type);

/* ---- sparse triangular solve  x = inv(A) b  (CSR, int32 indices) --------------------------- */
/* Device counterpart of triangular_solve_inspect / triangular_solve
 * (algorithms/triangular_solve_impl.hpp:13-107).  As in the reference
 * loop (:57-93) only the strict triangle named by uplo and the diagonal entries are read, so a
 * general square matrix may be passed; with DIAG_UNIT stored diagonal entries are ignored.
 *   sptrsv_create  = triangular_solve_inspect: level sets of the dependency graph, built on the
 *                    device from rowptr/colind only (values may change between solves).
 *   sptrsv_solve   = triangular_solve: one launch per wide level, one single-workgroup launch per
 *                    run of narrow levels.  alpha (HOST pointer) is the scaled_view factor of A
 *                    (x = inv(alpha*A) b); b and x are device vectors of m entries (b == x is fine).
 *   sptrsv_info    : info[0] levels, [1] widest level, [2] kernel launches per solve, [3] lanes/row.
 *   sptrsv_status  : synchronises the handle's stream and reports how the LAST solve of the plan ended: 0 = complete,
 *                    1 = a device-side wait of the cooperative kernel (its grid barrier: bounded polls,
 *                    SPBLAS_GFX950_TRSV_SPIN_LIMIT) gave up -- x is not valid.  Nothing in a correct program makes
 *                    that happen; a caller that wants certainty asks once after the solves it cares about.  A caller that
 *                    never asks still hears of it: the kernel raises a pinned host word on that path and the NEXT
 *                    sptrsv_solve on the plan returns STATUS_HIP_ERROR (last_hip_error = hipErrorLaunchTimeOut) once,
 *                    before it launches anything, without synchronising the stream.  The x of a solve that no later
 *                    call follows is unverified unless sptrsv_status is asked. */
enum spblas_gfx950_uplo {
  SPBLAS_GFX950_LOWER = 0, /* lower_triangle_t  (detail/triangular_types.hpp:10-13) */
  SPBLAS_GFX950_UPPER = 1  /* upper_triangle_t  (detail/triangular_types.hpp:5-8)   */
};
enum spblas_gfx950_diag {
  SPBLAS_GFX950_DIAG_EXPLICIT = 0, /* explicit_diagonal_t       (detail/triangular_types.hpp:20-23) */
  SPBLAS_GFX950_DIAG_UNIT = 1      /* implicit_unit_diagonal_t  (detail/triangular_types.hpp:15-18) */
};
int spblas_gfx950_sptrsv_create(spblas_gfx950_handle_t handle, spblas_gfx950_trsv_t* plan, int64_t m, int64_t nnz,
                                const int32_t* rowptr, const int32_t* colind, int uplo, int diag);
int spblas_gfx950_sptrsv_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_trsv_t plan);
int spblas_gfx950_sptrsv_info(spblas_gfx950_trsv_t plan, int64_t info[4]);
int spblas_gfx950_sptrsv_status(spblas_gfx950_handle_t handle, spblas_gfx950_trsv_t plan, int* status);
int spblas_gfx950_sptrsv_solve(spblas_gfx950_handle_t handle, spblas_gfx950_trsv_t plan, int64_t m, int64_t nnz,
                               const void* alpha, const int32_t* rowptr, const int32_t* colind, const void* values,
                               const void* b, void* x, int value_type);
/* The same solve for n right-hand sides in one call:  X(:, j) = inv(alpha*A) B(:, j),  j = 0 .. n-1  (no reference
 * counterpart: the reference solves one vector).  The triangle read is the one sptrsv_solve reads; `plan` is a plan of
 * sptrsv_create, unchanged -- one plan serves both calls, in any order.  Every level of the plan is handed over once for
 * all n columns.
 *   value types   F32 / F64; C32 / C64 / F16 / BF16 return STATUS_NOT_SUPPORTED before any other check.  The checks that
 *                 follow are those of sptrsv_solve, in its order: handle, pointers, plan against m / nnz.
 *   layouts       element (i, j) of B lives at B[i*b_row_stride + j*b_col_stride], likewise X.  Each operand is
 *                 layout_right (column stride 1, row stride >= n) or layout_left (row stride 1, column stride >= m): the
 *                 rule of spblas_gfx950_spmm_strided; B and X may differ.  Anything else, or n < 0: STATUS_INVALID_SIZE.
 *                 n == 0: success, nothing is launched, X is not touched.  An X that is layout_right with rows a multiple of
 *                 16 bytes apart is read and written in 16-byte pieces (any base alignment: the columns before the first
 *                 and after the last aligned piece go one by one); every other X element by element through its strides.
 *   n == 1        with B and X contiguous vectors of m elements the call IS sptrsv_solve: the same kernels, the same bits.
 *   aliasing      B == X with equal strides is allowed (in place).  Any other overlap of B and X is a caller error and is
 *                 not checked.
 *   results       the same plan, device and arguments give the same bits; the bits of a column do not depend on the values
 *                 of the other columns (they do depend on n, the layouts and the alignment of X, which choose how many
 *                 lanes share a row's entries).
 *   capture       recordable on the terms of sptrsv_solve: the first solve of a plan, by either call, sizes the plan's
 *                 control words and returns STATUS_NOT_SUPPORTED on a capturing stream; later solves only launch kernels.
 *   status        always one launch per wide level and one per run of narrow levels -- there is no cooperative form, so no
 *                 device-side wait that could give up: sptrsv_status reports 0 after it, and a give-up of an earlier
 *                 sptrsv_solve on the plan is reported by this call as by the next sptrsv_solve. */
int spblas_gfx950_sptrsm_solve(spblas_gfx950_handle_t handle, spblas_gfx950_trsv_t plan, int64_t m, int64_t nnz,
                               int64_t n, const void* alpha, const int32_t* rowptr, const int32_t* colind,
                               const void* values, const void* B, int64_t b_row_stride, int64_t b_col_stride,
                               void* X, int64_t x_row_stride, int64_t x_col_stride, int value_type);
/* What the last sptrsm_solve on this handle decided (a diagnostic for tests, like spmv_t_last; host integers only: no kernel
 * runs, nothing is synchronised).  Writes min(n_out, 8) entries: out[0] = path (SPTRSM_NONE before the first such call,
 * SPTRSM_FORWARDED: n == 1 with two contiguous vectors, the call went to sptrsv_solve and [1] .. [7] are 0, SPTRSM_ELEMENTS:
 * every element of X through its strides, SPTRSM_PIECES: whole units of X as 16-byte pieces); [1] = elements of X's base past
 * a 16-byte boundary (0 on the element path); [2] = units of 16 bytes a row of X is cut into, the partial ones in front and
 * behind included; [3] = log2 of the unit lanes C of a team; [4] = its entry lanes E = min(lanes per row of the plan, 64 / C);
 * [5] = 1 if whole units of B are read as 16-byte pieces too; [6] = bytes the buffer descriptor of X spans (0 on the element
 * path); [7] = passes of a team over the units of a row, ceil(units / C).  A call refused before it launched (a status other
 * than success from the argument checks or the plan's entry protocol) leaves the previous report.  Changes nothing about
 * the solve. */
#define SPBLAS_GFX950_SPTRSM_NONE 0
#define SPBLAS_GFX950_SPTRSM_FORWARDED 1
#define SPBLAS_GFX950_SPTRSM_ELEMENTS 2
#define SPBLAS_GFX950_SPTRSM_PIECES 3
int spblas_gfx950_sptrsm_last(spblas_gfx950_handle_t handle, int64_t* out, int n_out);
/* An APPROXIMATE solve by Jacobi sweeps on the triangular system (the iterative sparse triangular solve of Anzt, Chow and
 * Dongarra; no reference counterpart): what a preconditioner apply needs, at the price of `sweeps + 1` SpMV-shaped launches
 * instead of one hand-off per level.  The triangle read is the one sptrsv_solve reads (strict part named by uplo, the LAST
 * stored diagonal entry of a row, none stored: 0; stored diagonals ignored with DIAG_UNIT; columns outside [0, m) ignored).  With
 *     row(r, v) = (b_r - alpha * sum_{c strictly inside the triangle} a_rc * v_c) / (alpha * d_r)      (no division: DIAG_UNIT)
 * the iterates are   x0_r = row(r, 0)  -- the sum is taken as 0, nothing is gathered --   and   xk_r = row(r, x(k-1)),
 * k = 1 .. sweeps: every row reads the PREVIOUS iterate only (Jacobi, not Gauss-Seidel).  x receives x(sweeps).
 *   fixed point   a row of level l (0-based, as sptrsv_create counts levels) reads rows of lower levels only, so from sweep l
 *                 on it holds the value of the exact solve and keeps its bits: sweeps >= levels - 1 gives the solution of
 *                 the triangular system.  Whatever the early iterates of deep rows hold, Inf / NaN included, is overwritten.
 *   results       the entries of a row are summed in a fixed order given by the lanes per row, which are chosen from nnz / m
 *                 by the rule of sptrsv_create: the bits of x depend on (m, nnz, the arguments, sweeps) only -- not on
 *                 whether a plan was passed, nor on what x and work held before.
 *   buffers       x and work are device vectors of m elements.  Sweep k writes x when sweeps - k is even and work otherwise,
 *                 so the last sweep lands in x without a copy; sweeps == 0 writes x from b alone.  work holds x(sweeps - 1)
 *                 afterwards (unspecified with a plan).  The library allocates nothing, synchronises nothing and keeps no
 *                 pointer between calls: the call may be recorded in a graph from its first use.
 *   plan          NULL, or a plan of sptrsv_create for the same m / nnz / uplo / diag and the same structure (the structure
 *                 is the caller's promise, as for sptrsv_solve).  With a plan `sweeps` is clamped to levels - 1 and sweep
 *                 k >= 2 runs over the rows of level >= k - 1 only (the rows below are final in both buffers) where those
 *                 are at most a third of the rows; the set is walked in level order, which costs more per row.  The plan is
 *                 read only: no control words, no status word -- sptrsv_status and a later sptrsv_solve are not affected.
 *                 Without a plan every sweep covers all m rows and `sweeps` is taken as given.
 *   checks        in this order: C32 / C64 / F16 / BF16 return STATUS_NOT_SUPPORTED before anything else; handle; pointers
 *                 (alpha, rowptr, colind / values when nnz > 0, b / x when m > 0; work may be NULL only when sweeps == 0 or
 *                 m == 0); m, nnz (the limits of sptrsv_create) and sweeps < 0: STATUS_INVALID_SIZE; uplo / diag:
 *                 STATUS_INVALID_VALUE; a plan whose m / nnz / uplo / diag differ: STATUS_PLAN_MISMATCH; b == x, work == x or
 *                 work == b (m > 0): STATUS_INVALID_VALUE -- every sweep reads b, and the iterates alternate between x and
 *                 work; partial overlaps are the caller's error and are not checked; value type (F32 / F64, else
 *                 STATUS_INVALID_VALUE).  m == 0: success, nothing is launched.
 *   not offered   a block of right-hand sides, complex and 16-bit values, csc_view operands, several sweeps in one launch. */
int spblas_gfx950_sptrsv_sweeps(spblas_gfx950_handle_t handle, spblas_gfx950_trsv_t plan /* may be NULL */, int64_t m,
                                int64_t nnz, int sweeps, int uplo, int diag, const void* alpha, const int32_t* rowptr,
                                const int32_t* colind, const void* values, const void* b, void* x, void* work,
                                int value_type);

/* ---- incomplete LU on the pattern of A, ILU(0)  (CSR, int32 indices; no reference counterpart) ---------------- */
/* A is square, m x m.  Preconditions: the columns of every row are strictly ascending and every row stores its diagonal
 * entry (ilu0_create checks both).  The result LU has A's pattern in ONE array of nnz values: the entries left of the diagonal
 * are L, whose unit diagonal is implied; the diagonal and the entries right of it are U.  Row by row (IKJ):
 *     w = row i of A
 *     for k in the columns of row i with k < i, ascending:    w[k] = w[k] / LU[k][k]
 *         for j in the columns of row k with j > k, if j is also a column of row i:    w[j] = fma(-w[k], LU[k][j], w[j])
 *     row i of LU = w
 * Every entry receives its updates in ascending k, one fma each: the same plan, device and arguments give the same bits on
 * every call.  No pivoting, no fill, no shift of small pivots.  The storage is what the triangular solves read -- ONE array
 * serves both, without a copy or a split:
 *     sptrsv_solve / sptrsm_solve (LOWER, DIAG_UNIT,     LU, b, y)   then   (UPPER, DIAG_EXPLICIT, LU, y, x).
 *   ilu0_create   the inspect: checks the structure on the device (a row whose columns are not strictly ascending, a column
 *                 outside [0, m), a row without a stored diagonal or offsets that do not describe nnz entries:
 *                 STATUS_INVALID_VALUE), records the position of every diagonal entry, and builds the LOWER level plan by
 *                 calling spblas_gfx950_sptrsv_create -- row i needs exactly the rows k < i with (i, k) in the pattern.  It
 *                 synchronises the handle's stream more than once -- once for the structure check, which runs before the
 *                 level builder sees the arrays, then as sptrsv_create does -- (STATUS_NOT_SUPPORTED inside a capture) and
 *                 allocates everything a factor call needs, the status word included.
 *   ilu0_factor   a_values == lu_values: in place.  Otherwise A's values are copied to lu_values on the stream first and are
 *                 never written.  It allocates nothing and synchronises nothing: it enqueues the optional copy, one single-wavefront
 *                 launch that resets the status word, one launch per wide level and one single-workgroup launch per run of narrow levels, so it
 *                 may be recorded in a graph from its first call.  rowptr / colind must be the arrays (the same addresses)
 *                 the plan was made from: anything else is STATUS_PLAN_MISMATCH.
 *                 Order of checks: C32 / C64 / F16 / BF16 return STATUS_NOT_SUPPORTED before anything else; then handle,
 *                 pointers, plan against m / nnz / rowptr / colind (STATUS_PLAN_MISMATCH), value type (F32 / F64, else STATUS_INVALID_VALUE).
 *   pivots        a zero or non-finite pivot does not stop the factorisation: IEEE arithmetic carries on.  ilu0_status
 *                 synchronises the stream and sets *row to the smallest row index whose final LU[i][i] is zero or not finite
 *                 in the plan's last factor call, -1 if there is none (or no factor call yet).
 *   ilu0_info     info[0] levels, [1] widest level, [2] level launches per factor = the plan's launch groups (the reset of the
 *                 status word and the optional copy come on top), [3] lanes per row. */
int spblas_gfx950_ilu0_create(spblas_gfx950_handle_t handle, spblas_gfx950_ilu0_t* plan, int64_t m, int64_t nnz,
                              const int32_t* rowptr, const int32_t* colind);
int spblas_gfx950_ilu0_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_ilu0_t plan);
int spblas_gfx950_ilu0_info(spblas_gfx950_ilu0_t plan, int64_t info[4]);
int spblas_gfx950_ilu0_status(spblas_gfx950_handle_t handle, spblas_gfx950_ilu0_t plan, int64_t* row);
int spblas_gfx950_ilu0_factor(spblas_gfx950_handle_t handle, spblas_gfx950_ilu0_t plan, int64_t m, int64_t nnz,
                              const int32_t* rowptr, const int32_t* colind, const void* a_values, void* lu_values,
                              int value_type);
/* ILU(0) by fixed-point sweeps: an APPROXIMATE factor without one hand-off per level (the fine-grained parallel ILU of Chow and
 * Patel, SIAM J. Sci. Comput. 37(2), 2015, in row form; no reference counterpart).  With LU(0) = A, for k = 1 .. sweeps every
 * row i independently runs the sequence of ilu0_factor on a copy of A's row, reading the PREVIOUS iterate only:
 *     w = row i of A
 *     for c in the columns of row i with c < i, ascending:    w[c] = w[c] / LU(k-1)[c][c]
 *         for j in the columns of row c with j > c, if j is also a column of row i:    w[j] = fma(-w[c], LU(k-1)[c][j], w[j])
 *     row i of LU(k) = w
 * Inside a row the elimination is exact; across rows it is Jacobi.  One launch per sweep, all m rows in index order.
 *   fixed point   a row of level l (0-based, in the LOWER level plan of ilu0_create; ilu0_info's info[0] counts the levels) reads
 *                 rows of lower levels only, so from sweep l on it holds the bits of ilu0_factor, whatever Inf / NaN the earlier
 *                 iterates carried: sweeps >= levels - 1 IS ilu0_factor, bit for bit.  `sweeps` is clamped to
 *                 max(1, levels - 1).
 *   results       the bits of LU depend on (A, the pattern, sweeps) alone -- not on the lanes per row, the grid or on what
 *                 lu_values and work held before.
 *   buffers       lu_values and work are device arrays of nnz values.  Sweep 1 reads A as the previous iterate (no copy);
 *                 with s = the clamped count, sweep k writes lu_values when s - k is even and work otherwise, so the last
 *                 sweep lands in lu_values.  a_values is never written; work is unspecified afterwards.  Nothing is
 *                 allocated and nothing synchronised: the call enqueues the single-wavefront reset of the status word and
 *                 one launch per sweep, and may be recorded in a graph from its first use.
 *   pivots        only the LAST sweep checks its final diagonal and raises the plan's status word: ilu0_status afterwards
 *                 reports on LU(s) as it does on the factor of ilu0_factor.  ilu0_info is unchanged.
 *   checks        in this order: C32 / C64 / F16 / BF16 return STATUS_NOT_SUPPORTED before anything else; handle; pointers
 *                 (plan, rowptr, colind / a_values / lu_values when nnz > 0, work when nnz > 0 and the REQUESTED sweeps >= 2);
 *                 plan against m / nnz / rowptr / colind (the same addresses): STATUS_PLAN_MISMATCH; value type (F32 / F64,
 *                 else STATUS_INVALID_VALUE); sweeps < 1: STATUS_INVALID_VALUE; a_values == lu_values, a_values == work or
 *                 lu_values == work: STATUS_INVALID_VALUE -- every sweep re-reads A, so there is no in-place form; partial
 *                 overlaps are the caller's error and are not checked.  m == 0: success, nothing is launched.
 *   not offered   an active-row set per sweep, a block of matrices, complex and 16-bit values, csc_view operands, several
 *                 sweeps in one launch, scaling A to a unit diagonal first (the caller's, with spblas_gfx950_scale). */
int spblas_gfx950_ilu0_sweeps(spblas_gfx950_handle_t handle, spblas_gfx950_ilu0_t plan, int64_t m, int64_t nnz, int sweeps,
                              const int32_t* rowptr, const int32_t* colind, const void* a_values, void* lu_values, void* work,
                              int value_type);

/* ---- multicolour ordering and symmetric permutation  (CSR, int32 indices; no reference counterpart) -------------- */
/* The exact ilu0_factor and the exact triangular solves pay one hand-off per level of the dependency graph.  Ordering the rows
 * by the colours of a distance-1 colouring of the graph of A + A^T makes that graph shallow: rows of one colour share no stored
 * off-diagonal entry, so in B = P A P^T row i depends only on rows of lower colours and BOTH triangles of B have at most
 * `colours` levels.  The ordering changes the incomplete factor: a Krylov iteration preconditioned with ILU(0) of B usually needs
 * more iterations than with ILU(0) of A in its natural order -- depth is traded for convergence.
 *   colouring     Jones-Plassmann with fixed priorities.  key(v) = (uint64(h(v)) << 32) | v, compared unsigned, with
 *                 h(v) = mix(uint32(v + 1) * 0x9E3779B1u) and mix(x): x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13;
 *                 x *= 0xC2B2AE35u; x ^= x >> 16 (32-bit wraparound).  The neighbours of v are the columns of row v of A and of
 *                 row v of A^T without v itself (the pattern need not be symmetric; self loops and duplicate entries are legal
 *                 and ignored).  One launch per round: an uncoloured vertex with an uncoloured neighbour of larger key waits,
 *                 every other one takes the smallest colour no neighbour holds.
 *   determinism   the result equals sequential greedy colouring in descending key order whatever the schedule: the colours
 *                 depend on the pattern alone.  Only the number of rounds may vary from call to call.
 *   multicolor_create   the inspect: checks the structure on the device (a column outside [0, m) or offsets that do not describe
 *                 nnz entries: STATUS_INVALID_VALUE), forms the pattern of A^T with spblas_gfx950_csr_transpose, runs the
 *                 rounds -- the host reads the count of coloured vertices after each, at most m of them -- and sorts the
 *                 vertices by (colour, index).  It synchronises the handle's stream (STATUS_NOT_SUPPORTED inside a capture)
 *                 and keeps 3 m + colours + 1 int32 on the device until multicolor_destroy.  A is square, m x m.
 *   multicolor_info     info[0] colours, [1] rounds, [2] vertices of the largest colour class, [3] lanes per row.
 *   multicolor_copy     copies the results into caller-allocated int32 device arrays on the stream; any of them may be NULL.
 *                 perm[m]: new -> old, sorted by (colour, old index); inv_perm[m]: old -> new; color[m];
 *                 color_ptr[colours + 1]: rows color_ptr[c] .. color_ptr[c + 1] - 1 of the new order have colour c. */
int spblas_gfx950_multicolor_create(spblas_gfx950_handle_t handle, spblas_gfx950_multicolor_t* plan, int64_t m, int64_t nnz,
                                    const int32_t* rowptr, const int32_t* colind);
int spblas_gfx950_multicolor_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_multicolor_t plan);
int spblas_gfx950_multicolor_info(spblas_gfx950_multicolor_t plan, int64_t info[4]);
int spblas_gfx950_multicolor_copy(spblas_gfx950_handle_t handle, spblas_gfx950_multicolor_t plan, int32_t* perm,
                                  int32_t* inv_perm, int32_t* color, int32_t* color_ptr);
/* B = P A P^T for a square CSR matrix: row i of B is row perm[i] of A with column c renamed inv_perm[c]; the columns of every
 * row of B are ASCENDING and equal columns keep their source order -- the form ilu0_create / sptrsv_create take.
 *   csr_permute_create   the inspect: checks on the device that perm is a permutation of 0 .. m - 1 and that rowptr / colind
 *                 describe an m x m matrix of nnz entries (else STATUS_INVALID_VALUE, with nothing written to B), writes
 *                 b_rowptr[m + 1] and b_colind[nnz] (caller-allocated, not A's own arrays) and keeps map[nnz], the position in
 *                 A's arrays of every entry of B.  The rows are sorted by two passes of spblas_gfx950_csr_transpose that carry
 *                 the source position as payload.  It allocates and synchronises (STATUS_NOT_SUPPORTED inside a capture).
 *   csr_permute_values   b_values[p] = a_values[map[p]]: one gather launch, nothing allocated, nothing synchronised, so it may
 *                 be recorded in a graph from its first use -- what a refactorisation on a fixed pattern calls.  Order of
 *                 checks: C32 / C64 / F16 / BF16 return STATUS_NOT_SUPPORTED before anything else; then handle, pointers,
 *                 plan against nnz (STATUS_PLAN_MISMATCH), value type (F32 / F64, else STATUS_INVALID_VALUE),
 *                 a_values == b_values (STATUS_INVALID_VALUE: no in-place form).
 *   permute_vector       inverse == 0: dst[i] = src[perm[i]] (b into the new order); otherwise dst[perm[i]] = src[i] (x back).
 *                 n elements, src != dst, F32 / F64; perm is NOT checked (csr_permute_create did).  One launch, capturable. */
int spblas_gfx950_csr_permute_create(spblas_gfx950_handle_t handle, spblas_gfx950_permute_t* plan, int64_t m, int64_t nnz,
                                     const int32_t* rowptr, const int32_t* colind, const int32_t* perm, int32_t* b_rowptr,
                                     int32_t* b_colind);
int spblas_gfx950_csr_permute_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_permute_t plan);
int spblas_gfx950_csr_permute_values(spblas_gfx950_handle_t handle, spblas_gfx950_permute_t plan, int64_t nnz,
                                     const void* a_values, void* b_values, int value_type);
int spblas_gfx950_permute_vector(spblas_gfx950_handle_t handle, int64_t n, const int32_t* perm, const void* src, void* dst,
                                 int value_type, int inverse);

/* ---- multicolour Gauss-Seidel / SOR / SSOR sweeps  (CSR, int32 indices; no reference counterpart) ----------------- */
/* The smoother the colouring above is made for, and a preconditioner without a factorisation: one symmetric sweep from x = 0
 * is SSOR -- no ilu0, no level plans, no pivots that can break down, nothing to refresh when the values change.
 *   order         sigma(i) = perm[i] when gs_create was given a perm, else sigma(i) = i.  Colour c is the positions
 *                 color_ptr[c] .. color_ptr[c + 1] - 1 of that order (multicolor_copy's color_ptr: with its perm on A itself,
 *                 without a perm on B = P A P^T).
 *   row update    dot = sum of a_rc * x_c over the stored entries of row r with c != r, as stored (repeated off-diagonal
 *                 entries are summed);  g = (b_r - dot) / d_r, d_r the row's one stored diagonal entry;
 *                 x_r = g when omega == 1 (the old x_r is NOT read), else x_r = fma(omega, g - x_r, x_r).
 *   sweep         forward: the colours 0 .. C - 1 one after the other, every row of a colour independently; backward:
 *                 C - 1 .. 0; symmetric: forward, then backward.  `sweeps` repeats that; sweeps == 0 leaves x untouched and
 *                 launches nothing.  x is updated in place, b is only read, A's values are read as they are at the call and
 *                 never written.
 *   determinism   rows of one colour share no stored off-diagonal entry (gs_create checks it), so a launch that updates a
 *                 colour in place is race free and the sweep equals sequential Gauss-Seidel in colour order bit for bit.  The
 *                 bits of x depend on the matrix, color_ptr, perm, b, the incoming x, omega, sweeps and the direction -- not on
 *                 the grid, on earlier calls or on whether the launches were recorded in a graph.  The lanes per row follow
 *                 sptrsv_create's rule from nnz / m (> 96: 64, > 24: 16, > 6: 8, else 4); a row's entries are reduced in the
 *                 order of the triangular solve's row kernel, so the bits depend on that lane count alone.
 *   gs_create     the inspect.  color_ptr[colours + 1] and perm[m] (may be NULL) are int32 device arrays.  It refuses with
 *                 STATUS_INVALID_VALUE, writing nothing, unless: color_ptr starts at 0, is non-decreasing and ends at m (empty
 *                 colours are allowed); perm is a permutation of 0 .. m - 1 (the check of csr_permute_create); the row offsets
 *                 describe nnz entries and every column lies in [0, m); every row has EXACTLY ONE stored diagonal entry; no
 *                 stored off-diagonal entry (r, c) has r and c in one colour.  color_ptr is checked on the host, where the plan
 *                 keeps it, everything else on the device.  It allocates and synchronises (STATUS_NOT_SUPPORTED inside a
 *                 capture).  The plan holds structure only, no values: the colour offsets on the host, the position of every
 *                 row's diagonal entry (m int32), its own copy of perm (m int32, when one was given) and the lane count.
 *   gs_info       info[0] colours, [1] rows of the largest colour, [2] lanes per row, [3] launches per forward sweep (the
 *                 non-empty colours).
 *   gs_sweep      one launch per non-empty colour and half-sweep on the handle's stream; nothing allocated, nothing
 *                 synchronised, no pointer kept, so it records into a graph from its first call.  omega points at one host
 *                 scalar of the value type and is taken as given: convergence is the caller's business.  Order of checks:
 *                 C32 / C64 / F16 / BF16 return STATUS_NOT_SUPPORTED before anything else; then handle, pointers (the plan
 *                 included), sizes, values (direction, sweeps < 0, b == x, a value type other than F32 / F64:
 *                 STATUS_INVALID_VALUE), plan against m and nnz (STATUS_PLAN_MISMATCH).  m == 0 succeeds and launches nothing.
 * Not offered: a block of right-hand sides, weighted Jacobi, an implied zero initial guess that skips the gathers, several
 * colours per launch, scaled operands, complex / 16-bit values, int64 indices, CSC operands, distance-2 colourings. */
typedef enum spblas_gfx950_gs_direction {
  SPBLAS_GFX950_GS_FORWARD = 0,
  SPBLAS_GFX950_GS_BACKWARD = 1,
  SPBLAS_GFX950_GS_SYMMETRIC = 2
} spblas_gfx950_gs_direction;
int spblas_gfx950_gs_create(spblas_gfx950_handle_t handle, spblas_gfx950_gs_t* plan, int64_t m, int64_t nnz,
                            const int32_t* rowptr, const int32_t* colind, int64_t colours, const int32_t* color_ptr,
                            const int32_t* perm /* may be NULL */);
int spblas_gfx950_gs_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_gs_t plan);
int spblas_gfx950_gs_info(spblas_gfx950_gs_t plan, int64_t info[4]);
int spblas_gfx950_gs_sweep(spblas_gfx950_handle_t handle, spblas_gfx950_gs_t plan, int64_t m, int64_t nnz, int sweeps,
                           int direction, const void* omega, const int32_t* rowptr, const int32_t* colind, const void* values,
                           const void* b, void* x, int value_type);

/* ---- MIS-2 aggregation and the Galerkin coarse matrix  (CSR, int32 indices; no reference counterpart) ------------- */
/* The two pieces an aggregation-based algebraic multigrid needs next to transpose, SpGEMM and gs_sweep: a rule that groups the
 * rows into coarse unknowns, and A_c = P^T A P for the piecewise-constant P of that grouping.
 *   strength      in the value type T: d_i = the FIRST stored diagonal entry of row i, 0 without one; t2 = T(theta * theta),
 *                 the product taken in double.  A stored (i, j), j != i, is strong iff a_ij * a_ij >= (t2 * |d_i|) * |d_j|,
 *                 evaluated exactly so (products only).  A NaN on either side makes the entry weak.  theta == 0 makes every
 *                 stored off-diagonal entry with finite operands strong, explicit zeros included.
 *   graph         u ~ v iff (u, v) or (v, u) is a strong entry (the pattern need not be symmetric; self loops and repeats
 *                 count once).
 *   roots         a maximal independent set at distance 2 (MIS-2; Bell, Dalton, Olson 2012) with the FIXED keys of the
 *                 colouring above.  One round is four launches on ping-pong arrays, none of which reads what it writes:
 *                 T1[v] = the largest key of an undecided vertex in {v} + N(v) (0 if none), at every vertex; an undecided v
 *                 whose key equals the largest T1 in {v} + N(v) becomes a root; every undecided vertex within distance 2 of a
 *                 root becomes covered (two launches).  The host reads the count of decided vertices after every round.
 *   determinism   the roots are greedy MIS on the square of the graph in descending key order.  Roots, aggregates and the number
 *                 of rounds depend on the pattern, the values and theta alone.
 *   aggregates    the roots are numbered in ascending vertex index.  A root takes its number, a neighbour of a root that root's
 *                 number; in a second launch every other vertex takes the aggregate of the neighbour of the largest key among
 *                 those the first launch assigned.  A vertex without a strong neighbour is an aggregate of its own.
 *   aggregate_create   the inspect: structure check as multicolor_create (STATUS_INVALID_VALUE), transpose, strength, rounds,
 *                 numbering.  Order of checks: C32 / C64 / F16 / BF16 return STATUS_NOT_SUPPORTED before anything else; then
 *                 handle, capture (STATUS_NOT_SUPPORTED), pointers, sizes, then STATUS_INVALID_VALUE for m == 0 with nnz != 0, a
 *                 value type other than F32 / F64, a theta that is negative or not finite.  It synchronises the stream and
 *                 keeps m + aggregates int32 on the device until aggregate_destroy.
 *   aggregate_info     info[0] aggregates, [1] rounds, [2] rows of the largest aggregate, [3] of the smallest, [4] aggregates
 *                 of one row, [5] strong stored entries of A, [6] lanes per row, [7] m.
 *   aggregate_copy     agg[m] and root[aggregates] (the root row of every aggregate, ascending) into caller-allocated int32
 *                 device arrays on the stream; either may be NULL.
 *   aggregate_prolongator   the tentative prolongator P (m x aggregates) as CSR: p_rowptr[m + 1] = 0 .. m, p_colind[m] = agg,
 *                 p_values[m] = 1 (F32 / F64).  One launch, nothing allocated or synchronised: capturable.  m must be the
 *                 plan's (STATUS_PLAN_MISMATCH).
 *   coarsen_create     the inspect of A_c = P^T A P for ANY int32 map agg[m] with entries in [0, n_agg) (a value outside:
 *                 STATUS_INVALID_VALUE, as for a bad structure; an aggregate without rows gives an empty row of A_c).  Entry p
 *                 of A is renamed (agg[row], agg[col]); two passes of spblas_gfx950_csr_transpose that carry the source
 *                 position bring the entries into (I, J, position) order; runs of equal (I, J) collapse to one entry.  The
 *                 plan keeps c_rowptr[n_agg + 1], c_colind[c_nnz] (ascending, duplicate free), seg_ptr[c_nnz + 1] and
 *                 map[nnz].  It allocates and synchronises (STATUS_NOT_SUPPORTED inside a capture).  A is m x m.
 *   coarsen_info       info[0] n_agg, [1] c_nnz -- what to allocate for A_c --, [2] m, [3] nnz.
 *   coarsen_structure  copies c_rowptr and c_colind into caller-allocated arrays on the stream; capturable.
 *   coarsen_values     VALUES only: c_values[e] = the sum of a_values[map[q]] for q = seg_ptr[e] .. seg_ptr[e + 1] - 1 in
 *                 ascending q, which is ascending source position, by plain additions in T that start from the first term: the
 *                 bits depend on A and agg alone.  One launch, nothing allocated or synchronised, recordable from its first
 *                 use.  Order of checks: C32 / C64 / F16 / BF16 return STATUS_NOT_SUPPORTED before anything else; then handle,
 *                 pointers, plan against nnz and c_nnz (STATUS_PLAN_MISMATCH), value type (F32 / F64, else
 *                 STATUS_INVALID_VALUE), a_values == c_values (STATUS_INVALID_VALUE: no in-place form).
 *   smooth_*           the smoothed prolongator P = (I - omega D_F^-1 A_F) T of smoothed aggregation (Vanek, Mandel, Brezina
 *                 1996): T is the piecewise-constant prolongator of ANY int32 map agg[m] into [0, n_agg), A_F is A with its weak
 *                 off-diagonal entries (the strength rule above) removed and added to the diagonal, D_F its diagonal.
 *   smooth_create      the inspect, value-free.  Row i of P holds one entry for every distinct aggregate among {agg[i]} and
 *                 {agg[j] : (i, j) stored in A}, columns ascending; a weak or cancelling contribution leaves an explicit zero.
 *                 An extended list of nnz + m entries -- row i gives (agg[i], payload -1) first, then (agg[col], payload p) for
 *                 its entries -- goes through one pair of spblas_gfx950_csr_transpose over the m x n_agg matrix, there and back:
 *                 (row, J, position) order with the own-aggregate marker first in its run; head flags and one scan give the
 *                 tables.  Checks as coarsen_create, in its order (agg and the structure before anything indexes with them);
 *                 STATUS_INVALID_SIZE when nnz + m does not fit int32.  It allocates and synchronises (STATUS_NOT_SUPPORTED
 *                 inside a capture).  The plan keeps p_rowptr[m + 1], p_colind[p_nnz], seg_ptr[p_nnz + 1], map[nnz + m] and
 *                 one work array of m 8-byte slots (d) the value pass rewrites: ONE PLAN SERVES ONE STREAM AT A TIME.
 *   smooth_info        info[0] n_agg, [1] p_nnz -- what to allocate for P (m x n_agg) --, [2] m, [3] nnz.
 *   smooth_structure   copies p_rowptr and p_colind into caller-allocated arrays on the stream; capturable.
 *   smooth_values      VALUES only, fixed to the bit in the value type T (F32 / F64):
 *                   d_i      the first stored diagonal entry of row i, 0 without one; t2 = T(theta * theta)
 *                   strong   a stored (i, j), j != i, with a * a >= (t2 * |d_i|) * |d_j|, exactly as for aggregate_create
 *                   dF_i     T(0) plus, in ascending stored position, every entry of row i that has j == i (repeats
 *                            included) or is a weak off-diagonal entry; plain additions
 *                   row i    is smoothed iff dF_i is finite and non-zero: s_i = T(omega) / dF_i (the IEEE quotient) and
 *                            base_i = T(1) - T(omega); otherwise s_i = 0 and base_i = 1 (the row of T; an empty row is a
 *                            single 1)
 *                   P(i, J)  fma(-s_i, acc, b) -- one fused multiply-add --, acc = T(0) plus the strong entries of row i with
 *                            agg[j] == J in ascending position by plain additions, b = base_i if J == agg[i], else 0
 *                 theta == 0 makes every finite off-diagonal entry strong; omega == 0 gives T on P's pattern.  What overflows
 *                 past s_i is the caller's.  The bits depend on A, agg, omega and theta alone.  Two launches (d, then one team
 *                 of lanes per fine row that stages the row in LDS), nothing allocated or synchronised, recordable from its
 *                 first use.  omega points at one host scalar of the value type, read during the call.  rowptr / colind are
 *                 the arrays smooth_create saw.  Order of checks: C32 / C64 / F16 / BF16 return STATUS_NOT_SUPPORTED before
 *                 anything else; then handle, pointers, plan against m, nnz and p_nnz (STATUS_PLAN_MISMATCH), value type
 *                 (F32 / F64, else STATUS_INVALID_VALUE), omega not finite or theta negative or not finite
 *                 (STATUS_INVALID_VALUE), a_values == p_values (STATUS_INVALID_VALUE: no in-place form).
 * Not offered: an estimate of the spectral radius of D^-1 A (the caller supplies omega), a fused P^T A P for a general P (two
 * SpGEMMs do it), classical (Ruge-Stueben) coarsening, a restriction other than
 * P^T, rectangular or block matrices, weights in P, scaled / conjugated / CSC operands, complex / 16-bit values, int64 indices,
 * a hierarchy or cycle driver (examples/device_aggregate.cpp and examples/device_smoothed_aggregation.cpp show a two-grid
 * correction). */
int spblas_gfx950_aggregate_create(spblas_gfx950_handle_t handle, spblas_gfx950_aggregate_t* plan, int64_t m, int64_t nnz,
                                   const int32_t* rowptr, const int32_t* colind, const void* values, double theta,
                                   int value_type);
int spblas_gfx950_aggregate_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_aggregate_t plan);
int spblas_gfx950_aggregate_info(spblas_gfx950_aggregate_t plan, int64_t info[8]);
int spblas_gfx950_aggregate_copy(spblas_gfx950_handle_t handle, spblas_gfx950_aggregate_t plan, int32_t* agg, int32_t* root);
int spblas_gfx950_aggregate_prolongator(spblas_gfx950_handle_t handle, spblas_gfx950_aggregate_t plan, int64_t m,
                                        int32_t* p_rowptr, int32_t* p_colind, void* p_values, int value_type);
int spblas_gfx950_coarsen_create(spblas_gfx950_handle_t handle, spblas_gfx950_coarsen_t* plan, int64_t m, int64_t nnz,
                                 const int32_t* rowptr, const int32_t* colind, const int32_t* agg, int64_t n_agg);
int spblas_gfx950_coarsen_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_coarsen_t plan);
int spblas_gfx950_coarsen_info(spblas_gfx950_coarsen_t plan, int64_t info[4]);
int spblas_gfx950_coarsen_structure(spblas_gfx950_handle_t handle, spblas_gfx950_coarsen_t plan, int32_t* c_rowptr,
                                    int32_t* c_colind);
int spblas_gfx950_coarsen_values(spblas_gfx950_handle_t handle, spblas_gfx950_coarsen_t plan, int64_t nnz, const void* a_values,
                                 int64_t c_nnz, void* c_values, int value_type);
int spblas_gfx950_smooth_create(spblas_gfx950_handle_t handle, spblas_gfx950_smooth_t* plan, int64_t m, int64_t nnz,
                                const int32_t* rowptr, const int32_t* colind, const int32_t* agg, int64_t n_agg);
int spblas_gfx950_smooth_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_smooth_t plan);
int spblas_gfx950_smooth_info(spblas_gfx950_smooth_t plan, int64_t info[4]);
int spblas_gfx950_smooth_structure(spblas_gfx950_handle_t handle, spblas_gfx950_smooth_t plan, int32_t* p_rowptr,
                                   int32_t* p_colind);
int spblas_gfx950_smooth_values(spblas_gfx950_handle_t handle, spblas_gfx950_smooth_t plan, int64_t m, int64_t nnz,
                                const int32_t* rowptr, const int32_t* colind, const void* a_values, const void* omega,
                                double theta, int64_t p_nnz, void* p_values, int value_type);

/* ---- scale:  values[i] *= alpha  (algorithms/scale_impl.hpp:13-19) --------------------------- */
/* In-place scaling of a matrix's value array or of a dense vector (n elements, device memory).  A SLICED
 * SpMV plan holds a snapshot of the values: refresh it with spblas_gfx950_spmv_plan_update_values. */
int spblas_gfx950_scale(spblas_gfx950_handle_t handle, int64_t n, const void* alpha, void* values, int value_type);

/* ---- 64-bit indices ---------------------------------------------------------------------- */
/* The kernels of this library take int32 column (row) indices; the slot it replaces also admits int64 ones
 * (vendor/rocsparse/types.hpp:16-24: rocsparse_indextype_i64).  dst[i] = (int32) src[i] for count device elements;
 * STATUS_INVALID_VALUE when an index lies outside [0, bound) (bound <= 2^31 - 1: the number of columns), in which case
 * dst is not to be used.  Inspect-class: it synchronises the handle's stream (STATUS_NOT_SUPPORTED inside a capture).
 * The host layers call it once per index array (multiply_inspect, or the first multiply) and keep the narrowed copy. */
int spblas_gfx950_narrow_indices(spblas_gfx950_handle_t handle, int64_t count, const int64_t* src, int32_t* dst,
                                 int64_t bound);

/* ---- transpose:  B = A^T  (CSR -> CSR, int32 indices) ------------------------------------ */
/* Device counterpart of transpose(a, b) (algorithms/transpose_impl.hpp:14-53): stable counting
 * sort by column, so every output row lists its entries in source order.  t_rowptr has n+1
 * entries, t_colind / t_values nnz entries, all caller-allocated device memory.  Also what
 * multiply_inspect uses to serve csc_view / transposed(csr) operands with the regular kernels
 * (vendor/rocsparse/detail/get_transpose.hpp:19-29 maps CSC to a transposed CSR operation). */
int spblas_gfx950_csr_transpose(spblas_gfx950_handle_t handle, int64_t m, int64_t n, int64_t nnz,
                                const int32_t* rowptr, const int32_t* colind, const void* values,
                                int32_t* t_rowptr, int32_t* t_colind, void* t_values, int value_type);

#ifdef __cplusplus
}
#endif
#endif /* SPBLAS_GFX950_H */
