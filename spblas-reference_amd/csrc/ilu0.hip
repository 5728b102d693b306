// Incomplete LU factorisation on the pattern of A, ILU(0), for CSR operands on gfx950 (no reference counterpart).
//
// A is square with int32 row offsets and columns; the columns of a row are strictly ascending and every row stores its
// diagonal.  LU has A's pattern in ONE value array: left of the diagonal L (unit diagonal implied), the diagonal and what is
// right of it U -- what triangular_solve reads with (lower, implicit_unit_diagonal) and (upper, explicit_diagonal).  Row by row,
// in IKJ order:
//   w = row i of A
//   for k in the columns of row i with k < i, ascending:   w[k] = w[k] / LU[k][k]
//       for j in the columns of row k with j > k, if j is also a column of row i:   w[j] = fma(-w[k], LU[k][j], w[j])
//   row i of LU = w
// Every entry receives its updates in ascending k, one fma each, whatever the lane count: the bits depend on A alone.  No
// pivoting, no fill, no shift of a small pivot; a zero or non-finite pivot does not stop anything, the smallest row whose
// final diagonal is one is recorded in the plan's status word (spblas_gfx950_ilu0_status).
//
// Schedule: row i needs exactly the rows k < i with (i, k) in the pattern -- the LOWER level sets of
// spblas_gfx950_sptrsv_create, which ilu0_create builds by calling it; the plan's launch groups are taken as they are and
// run in the shape of sptrsm.hip: one launch per wide level, one single-workgroup launch per run of narrow levels with
// __threadfence(); __syncthreads(); between its levels, behind one single-wavefront launch that resets the status word.  There is
// no device-side wait of any kind.
//
// Row work: a TEAM of G lanes of one wavefront (G = the plan's lanes per row) owns a row.
//   fast path   rows of at most G x ILU0_LDS_PER_LANE entries: the team's slice of LDS holds the row's columns and working
//               values.  For every strict-lower entry (in-row position q, column k) every lane forms w[k] / LU[k][k], lane 0
//               stores it to LU (a lower entry is final once divided), the lanes stride over the upper part of pivot row k,
//               each looks its column up in the row's sorted columns right of q (binary search in LDS) and applies one fma on
//               a hit -- the pivot row's columns are distinct, so no two lanes touch one entry within a k.  LDS operations of
//               one wavefront complete in order; a wavefront-scope fence keeps the compiler from moving them across a step.
//   long path   longer rows (any length): the same steps with the working values in LU itself, read and written at agent
//               scope (past the L1) and drained (vmcnt(0)) between steps, the row's columns searched in colind.
// Hand-off of LU inside a launch (the single-workgroup kernel walks many levels): every LU value is stored write-through at
// agent scope and every load of LU is an agent-scope load, as sptrsm.hip does for X; rowptr, colind and the plan's arrays are
// never written and are read with plain loads.
//
// The same factor by fixed-point sweeps (spblas_gfx950_ilu0_sweeps, further down): one launch per sweep over all rows, every row
// from the previous iterate, no hand-off between levels; levels - 1 sweeps give the bits of the schedule above.
#include "common.hpp"
#include "complex_api.hpp"
#include "csr_inspect.hpp"
#include "lowp_api.hpp"
#include "trsv_plan.hpp"

#include <algorithm>
#include <cstdint>
#include <new>

#define ILU0_LEVEL_THREADS 256
#define ILU0_CHAIN_THREADS 512
#define ILU0_LDS_PER_LANE 8  // entries of a row per lane of its team that the fast path holds in LDS

struct spblas_gfx950_ilu0_s {
  int64_t m = 0, nnz = 0;
  const int32_t *rowptr = nullptr, *colind = nullptr;  // the arrays the plan was made from: a factor call must pass the same pair
  spblas_gfx950_trsv_t levels = nullptr;  // the LOWER level plan (spblas_gfx950_sptrsv_create), read only
  int32_t* diag = nullptr;                // [m] position of each row's diagonal entry in colind / values
  unsigned* status = nullptr;             // [4] word 0: 0 = every pivot fine, else 0xFFFFFFFF - the smallest row whose pivot is not
  spb::use_record use;                    // the stream of the last factor / sweeps / status call: destroy frees behind it

  void note(hipStream_t s) {  // ... which also read the level plan this one owns
    spb::note_use(use, s);
    if (levels)
      spb::note_use(levels->use, s);
  }
};

namespace spb {

template <typename T>
struct ilu0_args {
  const int32_t* order;
  const int32_t* rowptr;
  const int32_t* colind;
  const int32_t* diag;
  T* lu;
  unsigned* status;
  int G;
};

template <typename T>
__device__ __forceinline__ T ilu0_ld(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void ilu0_st(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ilu0_fma(float a, float b, float c) {
  return __builtin_fmaf(a, b, c);
}
__device__ __forceinline__ double ilu0_fma(double a, double b, double c) {
  return __builtin_fma(a, b, c);
}
// between two steps of a row: the team's LDS accesses stay on their side (no instruction: LDS is in order per wavefront)
__device__ __forceinline__ void ilu0_step_lds() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
// ... and the long path's: this wavefront's write-through stores to LU are acknowledged before its next loads of LU
__device__ __forceinline__ void ilu0_step_global() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  __builtin_amdgcn_wave_barrier();
}

template <typename T>
__device__ __forceinline__ void ilu0_pivot_check(const ilu0_args<T>& a, int r, T d) {
  if (!(d != T(0)) || !(d - d == T(0)))  // zero, NaN or infinite
    atomicMax(a.status, 0xFFFFFFFFu - (unsigned) r);
}

// One row, factored by its team.  `t` = lane index inside the team; wc / wv = the team's G x ILU0_LDS_PER_LANE LDS slots.
template <typename T>
__device__ __forceinline__ void ilu0_row(const ilu0_args<T>& a, int r, int t, int* wc, T* wv) {
  const int G = a.G;
  const int p0 = a.rowptr[r], len = a.rowptr[r + 1] - p0;
  const int dq = a.diag[r] - p0;  // in-row position of the diagonal = number of strict-lower entries
  if (len <= G * ILU0_LDS_PER_LANE) {
    for (int e = t; e < len; e += G) {
      wc[e] = a.colind[p0 + e];
      wv[e] = ilu0_ld(a.lu + p0 + e);
    }
    ilu0_step_lds();
    for (int q = 0; q < dq; ++q) {
      const int k = wc[q];
      const int kd = a.diag[k], k1 = a.rowptr[k + 1];
      const T mult = wv[q] / ilu0_ld(a.lu + kd);
      if (t == 0)
        ilu0_st(a.lu + p0 + q, mult);  // final: later steps touch positions right of q only
      for (int p = kd + 1 + t; p < k1; p += G) {
        const int c = a.colind[p];
        const T u = ilu0_ld(a.lu + p);
        int lo = q + 1, hi = len;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (wc[mid] < c)
            lo = mid + 1;
          else
            hi = mid;
        }
        if (lo < len && wc[lo] == c)
          wv[lo] = ilu0_fma(-mult, u, wv[lo]);
      }
      ilu0_step_lds();
    }
    for (int e = dq + t; e < len; e += G)
      ilu0_st(a.lu + p0 + e, wv[e]);
    if (t == 0)
      ilu0_pivot_check(a, r, wv[dq]);
  } else {
    const int32_t* rc = a.colind + p0;
    T* rv = a.lu + p0;
    for (int q = 0; q < dq; ++q) {
      const int k = rc[q];
      const int kd = a.diag[k], k1 = a.rowptr[k + 1];
      const T mult = ilu0_ld(rv + q) / ilu0_ld(a.lu + kd);
      if (t == 0)
        ilu0_st(rv + q, mult);
      for (int p = kd + 1 + t; p < k1; p += G) {
        const int c = a.colind[p];
        const T u = ilu0_ld(a.lu + p);
        int lo = q + 1, hi = len;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (rc[mid] < c)
            lo = mid + 1;
          else
            hi = mid;
        }
        if (lo < len && rc[lo] == c)
          ilu0_st(rv + lo, ilu0_fma(-mult, u, ilu0_ld(rv + lo)));
      }
      ilu0_step_global();
    }
    if (t == 0)
      ilu0_pivot_check(a, r, ilu0_ld(rv + dq));
  }
}

// one wide level: rows order[f0..f1), one team per row
template <typename T>
__global__ __launch_bounds__(ILU0_LEVEL_THREADS) void ilu0_level_kernel(int f0, int f1, ilu0_args<T> a) {
  __shared__ int s_cols[ILU0_LEVEL_THREADS * ILU0_LDS_PER_LANE];
  __shared__ T s_vals[ILU0_LEVEL_THREADS * ILU0_LDS_PER_LANE];
  const int team = (int) threadIdx.x / a.G;
  const int idx = f0 + (int) blockIdx.x * (ILU0_LEVEL_THREADS / a.G) + team;
  if (idx >= f1)
    return;
  const int slot = team * a.G * ILU0_LDS_PER_LANE;
  ilu0_row<T>(a, a.order[idx], (int) threadIdx.x % a.G, s_cols + slot, s_vals + slot);
}

// levels [l0, l1), all narrow: one workgroup, a barrier between levels
template <typename T>
__global__ __launch_bounds__(ILU0_CHAIN_THREADS) void ilu0_chain_kernel(int l0, int l1, const int32_t* __restrict__ level_ptr,
                                                                       ilu0_args<T> a) {
  __shared__ int s_cols[ILU0_CHAIN_THREADS * ILU0_LDS_PER_LANE];
  __shared__ T s_vals[ILU0_CHAIN_THREADS * ILU0_LDS_PER_LANE];
  const int team = (int) threadIdx.x / a.G;
  const int slot = team * a.G * ILU0_LDS_PER_LANE;
  for (int l = l0; l < l1; ++l) {
    const int f0 = level_ptr[l], f1 = level_ptr[l + 1];
    for (int idx = f0 + team; idx < f1; idx += ILU0_CHAIN_THREADS / a.G)
      ilu0_row<T>(a, a.order[idx], (int) threadIdx.x % a.G, s_cols + slot, s_vals + slot);
    __threadfence();  // LU of this level must be visible to the whole workgroup before the next one
    __syncthreads();
  }
}

// ---- ILU(0) by fixed-point sweeps (spblas_gfx950_ilu0_sweeps; the row form of Chow and Patel, SIAM J. Sci. Comput. 37(2)) ----
// LU(0) = A; sweep k: every row runs ilu0_row's sequence on a copy of A's row, with the pivot values and pivot rows taken from
// the PREVIOUS iterate -- exact elimination inside a row, Jacobi across rows.  A row of level l reads rows of lower levels only, so
// it has ilu0's bits from sweep l on.  prev, next and A are different buffers (sweep 1: prev IS A) and a sweep ends at a kernel
// boundary: every load of A and prev is a plain load, every store of the fast path a plain store.
template <typename T>
struct ilu0_sweep_args {
  const int32_t* rowptr;
  const int32_t* colind;
  const int32_t* diag;
  const T* a;     // A's values: the start of every row in every sweep
  const T* prev;  // the previous iterate: pivots and pivot rows
  T* next;        // this sweep's iterate
  unsigned* status;
  int m, G;
  int last;  // the last sweep checks the final pivots
};

// One row of one sweep, by its team.  The fast path keeps columns and working values in the team's LDS slice and stores the whole
// row, lower part included, at the end; the long path works in the row's own slice of `next`, seeded with A's row, with the
// agent-scope accesses and the drain of ilu0_row's long path (only this team touches that slice).
template <typename T>
__device__ __forceinline__ void ilu0_sweep_row(const ilu0_sweep_args<T>& a, int r, int t, int* wc, T* wv) {
  const int G = a.G;
  const int p0 = a.rowptr[r], len = a.rowptr[r + 1] - p0;
  const int dq = a.diag[r] - p0;
  if (len <= G * ILU0_LDS_PER_LANE) {
    for (int e = t; e < len; e += G) {
      wc[e] = a.colind[p0 + e];
      wv[e] = a.a[p0 + e];
    }
    ilu0_step_lds();
    for (int q = 0; q < dq; ++q) {
      const int k = wc[q];
      const int kd = a.diag[k], k1 = a.rowptr[k + 1];
      const T mult = wv[q] / a.prev[kd];
      for (int p = kd + 1 + t; p < k1; p += G) {
        const int c = a.colind[p];
        const T u = a.prev[p];
        int lo = q + 1, hi = len;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (wc[mid] < c)
            lo = mid + 1;
          else
            hi = mid;
        }
        if (lo < len && wc[lo] == c)
          wv[lo] = ilu0_fma(-mult, u, wv[lo]);
      }
      // every lane of the team read wv[q] above in ONE instruction of the wavefront, issued before this store (LDS operations of
      // a wavefront complete in order), so the store cannot reach a lane's read of the dividend; the next step reads it divided
      if (t == 0)
        wv[q] = mult;  // final: later steps touch positions right of q only
      ilu0_step_lds();
    }
    for (int e = t; e < len; e += G)
      a.next[p0 + e] = wv[e];
    if (a.last && t == 0) {
      const T d = wv[dq];
      if (!(d != T(0)) || !(d - d == T(0)))
        atomicMax(a.status, 0xFFFFFFFFu - (unsigned) r);
    }
  } else {
    const int32_t* rc = a.colind + p0;
    T* rv = a.next + p0;
    for (int e = t; e < len; e += G)
      ilu0_st(rv + e, a.a[p0 + e]);
    ilu0_step_global();
    for (int q = 0; q < dq; ++q) {
      const int k = rc[q];
      const int kd = a.diag[k], k1 = a.rowptr[k + 1];
      const T mult = ilu0_ld(rv + q) / a.prev[kd];
      for (int p = kd + 1 + t; p < k1; p += G) {
        const int c = a.colind[p];
        const T u = a.prev[p];
        int lo = q + 1, hi = len;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (rc[mid] < c)
            lo = mid + 1;
          else
            hi = mid;
        }
        if (lo < len && rc[lo] == c)
          ilu0_st(rv + lo, ilu0_fma(-mult, u, ilu0_ld(rv + lo)));
      }
      // as in the fast path: the team's loads of rv[q] above were one instruction, issued (and, feeding the division, returned)
      // before lane 0 reaches this store
      if (t == 0)
        ilu0_st(rv + q, mult);
      ilu0_step_global();
    }
    if (a.last && t == 0) {
      const T d = ilu0_ld(rv + dq);
      if (!(d != T(0)) || !(d - d == T(0)))
        atomicMax(a.status, 0xFFFFFFFFu - (unsigned) r);
    }
  }
}

// one sweep: all m rows in index order, one team per row
template <typename T>
__global__ __launch_bounds__(ILU0_LEVEL_THREADS) void ilu0_sweep_kernel(ilu0_sweep_args<T> a) {
  __shared__ int s_cols[ILU0_LEVEL_THREADS * ILU0_LDS_PER_LANE];
  __shared__ T s_vals[ILU0_LEVEL_THREADS * ILU0_LDS_PER_LANE];
  const int team = (int) threadIdx.x / a.G;
  const int64_t r = (int64_t) blockIdx.x * (ILU0_LEVEL_THREADS / a.G) + team;
  if (r >= a.m)
    return;
  const int slot = team * a.G * ILU0_LDS_PER_LANE;
  ilu0_sweep_row<T>(a, (int) r, (int) threadIdx.x % a.G, s_cols + slot, s_vals + slot);
}

// Resets the status word in front of a factor's launches.  A kernel, not hipMemsetAsync.  Observed, cause not established: with
// a 16-byte hipMemsetAsync here, a graph that recorded the factor and both solves read back arbitrary bits from the word after
// replay (factors and x exact; the same calls outside a capture were fine).  With this kernel the word replays correctly.
__global__ __launch_bounds__(64) void ilu0_reset_kernel(unsigned* __restrict__ status) {
  if (threadIdx.x < 4)
    status[threadIdx.x] = 0u;
}

// Structure check of the inspect and the diagonal positions: one lane per row.  flag[0] = 1 when a row's offsets leave
// [0, nnz], its columns are not strictly ascending inside [0, m), or it stores no diagonal entry.
__global__ __launch_bounds__(256) void ilu0_check_kernel(int64_t m, int64_t nnz, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ colind, int32_t* __restrict__ diag,
                                                         int32_t* __restrict__ flag) {
  const int64_t r = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (r >= m)
    return;
  const int64_t p0 = rowptr[r], p1 = rowptr[r + 1];
  int d = -1;
  bool ok = row_offsets_ok(r, m, nnz, p0, p1);
  if (ok) {
    int64_t prev = -1;
    for (int64_t p = p0; p < p1; ++p) {
      const int64_t c = colind[p];
      ok = ok && c > prev && c < m;
      prev = c;
      if (c == r)
        d = (int) p;
    }
  }
  diag[r] = d;
  if (!ok || d < 0)
    flag[0] = 1;
}

template <typename T>
static int ilu0_factor_typed(spblas_gfx950_handle_t h, spblas_gfx950_ilu0_s* pl, const int32_t* rowptr, const int32_t* colind,
                             const T* a_values, T* lu_values) {
  hipStream_t s = h->stream;
  pl->note(s);
  const spblas_gfx950_trsv_s* lv = pl->levels;
  if (a_values != lu_values && pl->nnz > 0)
    SPB_HIP(hipMemcpyAsync(lu_values, a_values, (size_t) pl->nnz * sizeof(T), hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(ilu0_reset_kernel, dim3(1), dim3(64), 0, s, pl->status);
  ilu0_args<T> a;
  a.order = lv->order;
  a.rowptr = rowptr;
  a.colind = colind;
  a.diag = pl->diag;
  a.lu = lu_values;
  a.status = pl->status;
  a.G = lv->lanes;
  for (const auto& g : lv->groups) {
    if (g.wide) {
      const int f0 = lv->h_level_ptr[g.l0], f1 = lv->h_level_ptr[g.l0 + 1];
      hipLaunchKernelGGL((ilu0_level_kernel<T>), dim3((unsigned) cdiv(f1 - f0, ILU0_LEVEL_THREADS / a.G)),
                         dim3(ILU0_LEVEL_THREADS), 0, s, f0, f1, a);
    } else {
      hipLaunchKernelGGL((ilu0_chain_kernel<T>), dim3(1), dim3(ILU0_CHAIN_THREADS), 0, s, g.l0, g.l1, lv->level_ptr, a);
    }
  }
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

template <typename T>
static int ilu0_sweeps_typed(spblas_gfx950_handle_t h, spblas_gfx950_ilu0_s* pl, int sweeps, const int32_t* rowptr,
                             const int32_t* colind, const T* a_values, T* lu_values, T* work) {
  hipStream_t s = h->stream;
  pl->note(s);
  const spblas_gfx950_trsv_s* lv = pl->levels;
  // a row of level l is final from sweep l on: more than levels - 1 sweeps change nothing
  const int levels = lv->h_level_ptr.empty() ? 0 : (int) lv->h_level_ptr.size() - 1;
  const int s_eff = std::min(sweeps, std::max(1, levels - 1));
  hipLaunchKernelGGL(ilu0_reset_kernel, dim3(1), dim3(64), 0, s, pl->status);
  ilu0_sweep_args<T> a;
  a.rowptr = rowptr;
  a.colind = colind;
  a.diag = pl->diag;
  a.a = a_values;
  a.status = pl->status;
  a.m = (int) pl->m;
  a.G = lv->lanes;
  const unsigned grid = (unsigned) cdiv(pl->m, ILU0_LEVEL_THREADS / a.G);
  for (int k = 1; k <= s_eff; ++k) {
    const bool to_work = ((s_eff - k) & 1) != 0;  // the last sweep lands in lu_values
    a.next = to_work ? work : lu_values;
    a.prev = k == 1 ? a_values : (to_work ? lu_values : work);  // LU(0) is A itself: no copy
    a.last = k == s_eff;
    hipLaunchKernelGGL((ilu0_sweep_kernel<T>), dim3(grid), dim3(ILU0_LEVEL_THREADS), 0, s, a);
  }
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

} // namespace spb

using namespace spb;

extern "C" {

int spblas_gfx950_ilu0_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_ilu0_t plan) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  order_behind_last_use(plan->use, handle->stream);  // (the level plan's destroy does the same for itself)
  (void) spblas_gfx950_sptrsv_destroy(handle, plan->levels);
  dev_free(plan->diag, handle->stream);
  dev_free(plan->status, handle->stream);
  delete plan;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_ilu0_create(spblas_gfx950_handle_t handle, spblas_gfx950_ilu0_t* plan_out, int64_t m, int64_t nnz,
                              const int32_t* rowptr, const int32_t* colind) {
  if (const int st = inspect_args_status(handle, plan_out && rowptr && (nnz <= 0 || colind), m, nnz))
    return st;
  *plan_out = nullptr;
  auto* pl = new (std::nothrow) spblas_gfx950_ilu0_s();
  if (!pl)
    return SPBLAS_GFX950_STATUS_ALLOC_FAILED;
  pl->m = m;
  pl->nnz = nnz;
  pl->rowptr = rowptr;
  pl->colind = colind;
  hipStream_t s = handle->stream;
  dev_temps temps(s);
  int32_t* flag = nullptr;
  auto fail = [&](int code) {
    (void) hipStreamSynchronize(s);
    (void) spblas_gfx950_ilu0_destroy(handle, pl);
    return code;
  };
  int rc;
  if ((rc = dev_alloc((void**) &pl->status, 16, s)) || (rc = temps.alloc(&flag, 16)) ||
      (rc = dev_alloc((void**) &pl->diag, (size_t) m * 4, s)))
    return fail(rc);
  hipError_t e = hipMemsetAsync(pl->status, 0, 16, s);
  if (e == hipSuccess)
    e = hipMemsetAsync(flag, 0, 16, s);
  if (e != hipSuccess)
    return fail(hip_fail(e));
  if (m > 0) {
    // the structure is checked, with a synchronisation of its own, BEFORE the level inspect sees it
    hipLaunchKernelGGL(ilu0_check_kernel, dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, nnz, rowptr, colind, pl->diag,
                       flag);
    if ((e = hipGetLastError()) != hipSuccess)
      return fail(hip_fail(e));
  }
  if ((rc = read_flag(handle, flag)))
    return fail(rc);
  // the dependency graph of ILU(0) is the one of the lower solve: its level plan, built by the existing code
  if ((rc = spblas_gfx950_sptrsv_create(handle, &pl->levels, m, nnz, rowptr, colind, SPBLAS_GFX950_LOWER,
                                        SPBLAS_GFX950_DIAG_UNIT)))
    return fail(rc);
  *plan_out = pl;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_ilu0_info(spblas_gfx950_ilu0_t plan, int64_t info[4]) {
  if (!plan || !info || !plan->levels)
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  const spblas_gfx950_trsv_s* lv = plan->levels;
  info[0] = lv->h_level_ptr.empty() ? 0 : (int64_t) lv->h_level_ptr.size() - 1;  // levels
  info[1] = lv->max_width;                                                       // widest level
  info[2] = (int64_t) lv->groups.size();                                         // level launches per factor (one per plan group)
  info[3] = lv->lanes;                                                           // lanes per row
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_ilu0_status(spblas_gfx950_handle_t handle, spblas_gfx950_ilu0_t plan, int64_t* row) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan || !row)
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (stream_capturing(handle->stream))
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  plan->note(handle->stream);
  unsigned st = 0;
  SPB_HIP(hipMemcpyAsync(&st, plan->status, sizeof(unsigned), hipMemcpyDeviceToHost, handle->stream));
  SPB_HIP(hipStreamSynchronize(handle->stream));
  *row = st == 0 ? -1 : (int64_t) (0xFFFFFFFFu - st);
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_ilu0_factor(spblas_gfx950_handle_t handle, spblas_gfx950_ilu0_t plan, int64_t m, int64_t nnz,
                              const int32_t* rowptr, const int32_t* colind, const void* a_values, void* lu_values,
                              int value_type) {
  if (is_complex_type(value_type) || is_lowp_type(value_type))  // complex / 16-bit values: SpMV / SpMM only
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan || !rowptr || (nnz > 0 && (!colind || !a_values || !lu_values)))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (m != plan->m || nnz != plan->nnz || rowptr != plan->rowptr || (nnz > 0 && colind != plan->colind))
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  if (value_type != SPBLAS_GFX950_F32 && value_type != SPBLAS_GFX950_F64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (value_type == SPBLAS_GFX950_F32)
    return ilu0_factor_typed<float>(handle, plan, rowptr, colind, static_cast<const float*>(a_values),
                                    static_cast<float*>(lu_values));
  return ilu0_factor_typed<double>(handle, plan, rowptr, colind, static_cast<const double*>(a_values),
                                   static_cast<double*>(lu_values));
}

int spblas_gfx950_ilu0_sweeps(spblas_gfx950_handle_t handle, spblas_gfx950_ilu0_t plan, int64_t m, int64_t nnz, int sweeps,
                              const int32_t* rowptr, const int32_t* colind, const void* a_values, void* lu_values, void* work,
                              int value_type) {
  if (is_complex_type(value_type) || is_lowp_type(value_type))  // complex / 16-bit values: SpMV / SpMM only
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan || !rowptr || (nnz > 0 && (!colind || !a_values || !lu_values || (!work && sweeps >= 2))))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (m != plan->m || nnz != plan->nnz || rowptr != plan->rowptr || (nnz > 0 && colind != plan->colind))
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  if (value_type != SPBLAS_GFX950_F32 && value_type != SPBLAS_GFX950_F64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (sweeps < 1)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  // every sweep re-reads A while the iterates alternate between lu_values and work: no in-place form
  if (nnz > 0 && (a_values == lu_values || (work && (work == a_values || work == lu_values))))
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (m == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  if (value_type == SPBLAS_GFX950_F32)
    return ilu0_sweeps_typed<float>(handle, plan, sweeps, rowptr, colind, static_cast<const float*>(a_values),
                                    static_cast<float*>(lu_values), static_cast<float*>(work));
  return ilu0_sweeps_typed<double>(handle, plan, sweeps, rowptr, colind, static_cast<const double*>(a_values),
                                   static_cast<double*>(lu_values), static_cast<double*>(work));
}

} // extern "C"

// Loads this file's code object at handle creation (handle.hip), as the other files do.
namespace spb {
void preload_ilu0() {
  hipFuncAttributes attr;
  (void) hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&ilu0_level_kernel<float>));
  (void) hipGetLastError();
}
} // namespace spb
