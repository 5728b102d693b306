// The smoothed prolongator of an aggregation, P = (I - omega D_F^-1 A_F) T, on gfx950 (smoothed aggregation after Vanek, Mandel
// and Brezina 1996; no reference counterpart).  T is the piecewise-constant prolongator of an int32 map agg[m]; A_F is A with its
// WEAK off-diagonal entries removed and added to the diagonal (the strength rule of aggregate, aggregate.hip); D_F its diagonal.
//
// smooth_create  the pattern of P is structural: row i holds one entry for every distinct aggregate among {agg[i]} and
//   {agg[j] : (i, j) stored}, columns ascending.  An extended list of nnz + m entries -- row i gives (agg[i], payload -1) first,
//   then (agg[col], payload p) for its entries in stored order -- goes through ONE pair of stable transposes over the m x n_agg
//   matrix (there and back): the entries then stand in (row, J, position) order with the own-aggregate marker first in its run.
//   Head flags and one scan give p_rowptr, p_colind, seg_ptr and map, as in coarsen_create.
// smooth_values  fixed to the bit, in the value type T:
//     d_i     the first stored diagonal entry of row i (ag_diag_kernel, the kernel aggregate uses);  t2 = T(theta * theta)
//     strong  a stored (i, j) with j != i and  a * a >= (t2 * |d_i|) * |d_j|
//     dF_i    T(0) plus, in ascending stored position, every entry of row i with j == i (repeats included) or weak
//     s_i     T(omega) / dF_i (the IEEE quotient) and base_i = T(1) - T(omega) when dF_i is finite and non-zero; else 0 and 1
//     P(i, J) fma(-s_i, acc, b):  acc = T(0) plus the strong entries of row i with agg[j] == J in ascending position,
//             b = base_i when J == agg[i], else 0
//   Two launches.  The second gives a TEAM of G = lanes_per_row(m, nnz) lanes to every fine row: every term of row i of P comes
//   from row i of A, so the team reads the row's columns and values once, coalesced, gathers d_j once per entry and keeps value
//   and kind (strong / lumped) of every entry in LDS; dF_i is formed chunk by chunk in position order, every lane holding the
//   same sum (the chunk's terms come by shuffles); then lane t takes the entries t, t + G, ... of row i of P and adds its terms
//   from the staged row through map.  A row of more than SM_STAGE_PER_LANE * G entries is not staged: its lanes re-read the
//   entry and its d_j from global memory, with the same order of additions.
#include "aggregate_kernels.hpp"
#include "common.hpp"
#include "complex_api.hpp"
#include "csr_inspect.hpp"
#include "lowp_api.hpp"
#include "scan.hpp"

#include <cmath>
#include <cstdint>
#include <new>

// entries a team stages per lane: a row of up to SM_STAGE_PER_LANE * G entries lives in LDS (tests/smooth_util.py restates it)
#define SM_STAGE_PER_LANE 8

struct spblas_gfx950_smooth_s {
  int64_t m = 0, nnz = 0, n_agg = 0, p_nnz = 0;
  int lanes = 4;
  int32_t* p_rowptr = nullptr;  // [m + 1]
  int32_t* p_colind = nullptr;  // [p_nnz] ascending, duplicate free
  int32_t* seg_ptr = nullptr;   // [p_nnz + 1] first sorted position of every entry of P
  int32_t* map = nullptr;       // [nnz + m] position in A's arrays of every sorted position; -1: the own-aggregate marker
  void* d = nullptr;            // [m] 8-byte slots: the first stored diagonal entries, rewritten by every value pass
  spb::use_record use;          // the stream of the last structure copy / value pass: destroy frees behind it
};

namespace spb {

__device__ __forceinline__ float sm_fma(float a, float b, float c) {
  return fmaf(a, b, c);
}
__device__ __forceinline__ double sm_fma(double a, double b, double c) {
  return fma(a, b, c);
}
// the IEEE quotient.  For float it is taken in double and rounded once, which is exact for float operands (53 >= 2 * 24 + 2)
// whatever the build's float division is.
__device__ __forceinline__ float sm_quotient(float a, float b) {
  return (float) ((double) a / (double) b);
}
__device__ __forceinline__ double sm_quotient(double a, double b) {
  return a / b;
}
__device__ __forceinline__ bool sm_finite(float x) { return __builtin_isfinite(x); }
__device__ __forceinline__ bool sm_finite(double x) { return __builtin_isfinite(x); }

// the extended list: row i gives (agg[i], -1) first, then (agg[col], p) for its entries; x_rowptr[i] = rowptr[i] + i
template <int G>
__global__ __launch_bounds__(AG_THREADS) void sm_extend_kernel(int m, const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ colind,
                                                               const int32_t* __restrict__ agg, int32_t* __restrict__ x_rowptr,
                                                               int32_t* __restrict__ x_col, int32_t* __restrict__ x_pos) {
  const int t = (int) threadIdx.x % G, v = ag_vertex<G>(m);
  if (v < 0)
    return;
  const int p0 = rowptr[v], p1 = rowptr[v + 1];
  if (t == 0) {
    x_rowptr[v] = p0 + v;
    x_col[p0 + v] = agg[v];
    x_pos[p0 + v] = -1;
    if (v == m - 1)
      x_rowptr[m] = p1 + m;
  }
  for (int p = p0 + t; p < p1; p += G) {
    x_col[p + v + 1] = agg[colind[p]];
    x_pos[p + v + 1] = p;
  }
}

template <typename T, int G>
__global__ __launch_bounds__(AG_THREADS) void sm_values_kernel(int m, const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ colind, const T* __restrict__ values,
                                                               const T* __restrict__ d, T omega, T t2,
                                                               const int32_t* __restrict__ p_rowptr,
                                                               const int32_t* __restrict__ seg_ptr,
                                                               const int32_t* __restrict__ map, T* __restrict__ p_values) {
  constexpr int CAP = SM_STAGE_PER_LANE * G;
  __shared__ T s_val[AG_THREADS * SM_STAGE_PER_LANE];
  __shared__ uint8_t s_lump[AG_THREADS * SM_STAGE_PER_LANE];
  const int t = (int) threadIdx.x % G, v = ag_vertex<G>(m);
  T* const tv = s_val + ((int) threadIdx.x / G) * CAP;
  uint8_t* const tl = s_lump + ((int) threadIdx.x / G) * CAP;
  int r0 = 0, len = 0;
  bool staged = false;
  T dF = T(0), lhs_d = T(0);
  if (v >= 0) {
    r0 = rowptr[v];
    len = rowptr[v + 1] - r0;
    staged = len <= CAP;
    lhs_d = t2 * ag_abs(d[v]);
    for (int k0 = 0; k0 < len; k0 += G) {  // (uniform inside the team)
      const int k = k0 + t;
      T a = T(0);
      int lump = 0;
      if (k < len) {
        const int j = colind[r0 + k];
        a = values[r0 + k];
        lump = ag_is_strong(a, lhs_d, d[j], j, v) ? 0 : 1;
        if (staged) {
          tv[k] = a;
          tl[k] = (uint8_t) lump;
        }
      }
      // the chunk's lumped entries in position order, the same sum in every lane
      const int n = min(G, len - k0);
      for (int u = 0; u < n; ++u) {
        const T x = __shfl(a, u, G);
        if (__shfl(lump, u, G))
          dF = dF + x;
      }
    }
  }
  // A team lies inside one wavefront and reads only what its own lanes staged, so no ordering ACROSS waves is needed: the
  // barrier serves as a conservative fence between the team's LDS writes and reads (every thread arrives: no return above).
  __syncthreads();
  if (v < 0)
    return;
  const bool smoothed = sm_finite(dF) && dF != T(0);
  const T s = smoothed ? sm_quotient(omega, dF) : T(0);
  const T base = smoothed ? T(1) - omega : T(1);
  for (int e = p_rowptr[v] + t, e1 = p_rowptr[v + 1]; e < e1; e += G) {
    int q = seg_ptr[e];
    const int q1 = seg_ptr[e + 1];
    T b = T(0);
    if (map[q] < 0) {  // the own-aggregate marker stands first in its run
      b = base;
      ++q;
    }
    T acc = T(0);
    for (; q < q1; ++q) {
      const int p = map[q];
      if (staged) {
        if (!tl[p - r0])
          acc = acc + tv[p - r0];
      } else {
        const T a = values[p];
        const int j = colind[p];
        if (ag_is_strong(a, lhs_d, d[j], j, v))
          acc = acc + a;
      }
    }
    p_values[e] = sm_fma(-s, acc, b);
  }
}

template <typename T>
static int smooth_values_typed(spblas_gfx950_handle_s* handle, spblas_gfx950_smooth_s* pl, const int32_t* rowptr,
                               const int32_t* colind, const T* values, T omega, double theta, T* p_values) {
  hipStream_t s = handle->stream;
  const int m = (int) pl->m;
  T* d = static_cast<T*>(pl->d);
  const T t2 = (T) (theta * theta);
  with_lanes(pl->lanes, [&](auto gc) {
    constexpr int G = decltype(gc)::value;
    const dim3 grid((unsigned) cdiv(pl->m, AG_THREADS / G)), block(AG_THREADS);
    hipLaunchKernelGGL((ag_diag_kernel<T, G>), grid, block, 0, s, m, rowptr, colind, values, d);
    hipLaunchKernelGGL((sm_values_kernel<T, G>), grid, block, 0, s, m, rowptr, colind, values, (const T*) d, omega, t2,
                       (const int32_t*) pl->p_rowptr, (const int32_t*) pl->seg_ptr, (const int32_t*) pl->map, p_values);
  });
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

} // namespace spb

using namespace spb;

extern "C" {

int spblas_gfx950_smooth_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_smooth_t plan) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  order_behind_last_use(plan->use, handle->stream);
  dev_free(plan->p_rowptr, handle->stream);
  dev_free(plan->p_colind, handle->stream);
  dev_free(plan->seg_ptr, handle->stream);
  dev_free(plan->map, handle->stream);
  dev_free(plan->d, handle->stream);
  delete plan;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_smooth_create(spblas_gfx950_handle_t handle, spblas_gfx950_smooth_t* plan_out, int64_t m, int64_t nnz,
                                const int32_t* rowptr, const int32_t* colind, const int32_t* agg, int64_t n_agg) {
  if (const int st = inspect_args_status(handle, plan_out && rowptr && (nnz <= 0 || colind) && (m <= 0 || agg), m, nnz))
    return st;
  *plan_out = nullptr;
  if (n_agg < 0 || n_agg >= INT32_MAX || nnz + m > INT32_MAX)  // the extended list has nnz + m entries
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if ((m == 0 && nnz != 0) || (m > 0 && n_agg == 0))  // no aggregate could hold a row
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  auto* pl = new (std::nothrow) spblas_gfx950_smooth_s();
  if (!pl)
    return SPBLAS_GFX950_STATUS_ALLOC_FAILED;
  pl->m = m;
  pl->nnz = nnz;
  pl->n_agg = n_agg;
  pl->lanes = lanes_per_row(m, nnz);
  hipStream_t s = handle->stream;
  dev_temps temps(s);
  int32_t *flag = nullptr, *x_rowptr = nullptr, *x_col = nullptr, *x_pos = nullptr, *r_rowptr = nullptr, *r_col = nullptr,
          *r_pos = nullptr, *s_rowptr = nullptr, *s_col = nullptr, *head = nullptr;
  long long* partials = nullptr;
  auto fail = [&](int code) {
    (void) hipStreamSynchronize(s);
    (void) spblas_gfx950_smooth_destroy(handle, pl);
    return code;
  };
  int rc;
  hipError_t e;
  const int64_t ext = nnz + m;
  const size_t mb = (size_t) (m + 1) * 4, cb = (size_t) (n_agg + 1) * 4, xb = (size_t) ext * 4;
  if ((rc = dev_alloc((void**) &pl->p_rowptr, mb, s)))
    return fail(rc);
  if ((e = hipMemsetAsync(pl->p_rowptr, 0, mb, s)) != hipSuccess)
    return fail(hip_fail(e));
  if (m == 0) {
    if ((rc = dev_alloc((void**) &pl->seg_ptr, 4, s)))
      return fail(rc);
    if ((e = hipMemsetAsync(pl->seg_ptr, 0, 4, s)) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess)
      return fail(hip_fail(e));
    *plan_out = pl;
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  if ((rc = temps.alloc(&flag, 16)))
    return fail(rc);
  if ((e = hipMemsetAsync(flag, 0, 16, s)) != hipSuccess)
    return fail(hip_fail(e));
  // agg and the structure are checked, with a synchronisation, BEFORE anything indexes with them
  hipLaunchKernelGGL(cz_check_agg_kernel, dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, agg, n_agg, flag);
  if ((rc = check_csr_structure(handle, m, nnz, rowptr, colind, flag)))
    return fail(rc);
  if ((rc = dev_alloc((void**) &pl->map, xb, s)) || (rc = dev_alloc(&pl->d, (size_t) m * 8, s)) ||
      (rc = temps.alloc(&x_rowptr, mb)) || (rc = temps.alloc(&x_col, xb)) || (rc = temps.alloc(&x_pos, xb)) ||
      (rc = temps.alloc(&r_rowptr, cb)) || (rc = temps.alloc(&r_col, xb)) || (rc = temps.alloc(&r_pos, xb)) ||
      (rc = temps.alloc(&s_rowptr, mb)) || (rc = temps.alloc(&s_col, xb)) || (rc = temps.alloc(&head, xb + 4)) ||
      (rc = temps.alloc(&partials, (size_t) (cdiv(ext, 2048) + 2) * sizeof(long long))))
    return fail(rc);
  const dim3 xgrid(stride_grid(handle, ext)), block(256);
  with_lanes(pl->lanes, [&](auto gc) {
    constexpr int G = decltype(gc)::value;
    hipLaunchKernelGGL(sm_extend_kernel<G>, dim3((unsigned) cdiv(m, AG_THREADS / G)), dim3(AG_THREADS), 0, s, (int) m, rowptr,
                       colind, agg, x_rowptr, x_col, x_pos);
  });
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(hip_fail(e));
  // there: by aggregate, (row, position) order kept inside; and back: by row, (aggregate, position) order kept inside
  if ((rc = spblas_gfx950_csr_transpose(handle, m, n_agg, ext, x_rowptr, x_col, x_pos, r_rowptr, r_col, r_pos,
                                        SPBLAS_GFX950_F32)) ||
      (rc = spblas_gfx950_csr_transpose(handle, n_agg, m, ext, r_rowptr, r_col, r_pos, s_rowptr, s_col, pl->map,
                                        SPBLAS_GFX950_F32)))
    return fail(rc);
  // runs of equal (row, J) collapse: head flags, their exclusive scan, the entry tables
  if ((e = hipMemsetAsync(head, 0, xb + 4, s)) != hipSuccess)
    return fail(hip_fail(e));
  hipLaunchKernelGGL(cz_row_start_kernel, dim3((unsigned) cdiv(m, 256)), block, 0, s, m, (const int32_t*) s_rowptr, head);
  hipLaunchKernelGGL(cz_heads_kernel, xgrid, block, 0, s, ext, (const int32_t*) s_col, head);
  scan_counts_i32(s, ext, head, partials);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(hip_fail(e));
  int32_t h_pnnz = 0;
  {
    readback_scope rb(handle);
    if ((rc = readback_add(handle, &h_pnnz, head + ext, 4)) || (rc = readback_flush(handle)))
      return fail(rc);
  }
  pl->p_nnz = h_pnnz;
  if (pl->p_nnz < m || pl->p_nnz > ext)  // cannot happen: every row heads at least the run of its marker
    return fail(SPBLAS_GFX950_STATUS_HIP_ERROR);
  if ((rc = dev_alloc((void**) &pl->p_colind, (size_t) pl->p_nnz * 4, s)) ||
      (rc = dev_alloc((void**) &pl->seg_ptr, (size_t) (pl->p_nnz + 1) * 4, s)))
    return fail(rc);
  hipLaunchKernelGGL(cz_emit_kernel, xgrid, block, 0, s, ext, (const int32_t*) head, (const int32_t*) s_col, pl->seg_ptr,
                     pl->p_colind);
  hipLaunchKernelGGL(cz_rowptr_kernel, dim3((unsigned) cdiv(m + 1, 256)), block, 0, s, m, (const int32_t*) s_rowptr,
                     (const int32_t*) head, pl->p_rowptr);
  if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess)
    return fail(hip_fail(e));
  *plan_out = pl;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_smooth_info(spblas_gfx950_smooth_t plan, int64_t info[4]) {
  if (!plan || !info)
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  info[0] = plan->n_agg;  // columns of P
  info[1] = plan->p_nnz;  // entries of P
  info[2] = plan->m;      // rows of P
  info[3] = plan->nnz;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_smooth_structure(spblas_gfx950_handle_t handle, spblas_gfx950_smooth_t plan, int32_t* p_rowptr,
                                   int32_t* p_colind) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan || !p_rowptr || (plan->p_nnz > 0 && !p_colind))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  hipStream_t s = handle->stream;
  note_use(plan->use, s);
  SPB_HIP(hipMemcpyAsync(p_rowptr, plan->p_rowptr, (size_t) (plan->m + 1) * 4, hipMemcpyDeviceToDevice, s));
  if (plan->p_nnz > 0)
    SPB_HIP(hipMemcpyAsync(p_colind, plan->p_colind, (size_t) plan->p_nnz * 4, hipMemcpyDeviceToDevice, s));
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_smooth_values(spblas_gfx950_handle_t handle, spblas_gfx950_smooth_t plan, int64_t m, int64_t nnz,
                                const int32_t* rowptr, const int32_t* colind, const void* a_values, const void* omega,
                                double theta, int64_t p_nnz, void* p_values, int value_type) {
  if (is_complex_type(value_type) || is_lowp_type(value_type))  // complex / 16-bit values: SpMV / SpMM only
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan || !omega || !rowptr || (nnz > 0 && (!colind || !a_values)) || (p_nnz > 0 && !p_values))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (m != plan->m || nnz != plan->nnz || p_nnz != plan->p_nnz)
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  if (value_type != SPBLAS_GFX950_F32 && value_type != SPBLAS_GFX950_F64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  const double w = value_type == SPBLAS_GFX950_F32 ? (double) *static_cast<const float*>(omega) : *static_cast<const double*>(omega);
  if (!std::isfinite(w) || !std::isfinite(theta) || theta < 0.0)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (p_nnz > 0 && a_values == p_values)  // every entry of P re-reads A: no in-place form
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (m == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  note_use(plan->use, handle->stream);
  if (value_type == SPBLAS_GFX950_F32)
    return smooth_values_typed<float>(handle, plan, rowptr, colind, static_cast<const float*>(a_values), (float) w, theta,
                                      static_cast<float*>(p_values));
  return smooth_values_typed<double>(handle, plan, rowptr, colind, static_cast<const double*>(a_values), w, theta,
                                     static_cast<double*>(p_values));
}

} // extern "C"

// Loads this file's code object at handle creation (handle.hip), as the other files do: a first values call recorded in a graph
// finds its kernels loaded.
namespace spb {
void preload_smooth() {
  hipFuncAttributes attr;
  (void) hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&sm_values_kernel<float, 8>));
  (void) hipGetLastError();
}
} // namespace spb
