// Approximate sparse triangular solve by Jacobi sweeps  (the "iterative sparse triangular solve" of Anzt, Chow and
// Dongarra, Euro-Par 2015; no reference counterpart).
//
// T = the triangle of A that sptrsv_solve reads (sptrsv.hip: the strict part named by uplo plus the diagonal).  With
//   row(r, v) = (b_r - alpha * sum_{c strictly inside the triangle} a_rc v_c) / (alpha * d_r)        (no division: unit diagonal)
// the iterates are  x0_r = row(r, 0)  (the sum taken as 0: nothing is gathered)  and  xk_r = row(r, x(k-1)),  k = 1 .. s.
// Every row reads the PREVIOUS iterate only, so a sweep is one SpMV-shaped launch without any hand-off between levels: where
// the exact solve pays one store -> load hand-off per level, a sweep pays one pass over the triangle.  A row of level l reads
// rows of lower levels only, so it holds the exact solve's value from sweep l on: s >= levels - 1 IS the solve.
//
// Kernel: a group of G lanes owns a row (G = lanes_per_row(m, nnz), as in sptrsv_create), strides its entries, masks them with
// trsv_strict and the column range, carries the diagonal VALUE with its position through the reduction (trsv_row's
// arithmetic, in trsv_row's order: the bits depend on G alone, not on the grid or on a plan) and lane 0 stores.  The two
// iterates live in different buffers and a sweep ends at a kernel boundary: plain loads, plain stores, no agent-scope
// atomics.  Two entries per lane are in flight before the first gather (rows average a dozen entries; the x gather is the
// cost).  The lane groups of a capped grid stride over the rows and load the next row's index, entry range and b while the
// current row is computed: of the four dependent loads order -> rowptr -> colind -> x two are left on a row's path.  Measured
// at 4 M rows: 4 - 8 % faster than one workgroup per 256 / G rows on a 7-point Laplacian, equal on random columns.
//
// Buffers: the caller's x and a caller-provided work vector.  Sweep k writes x when s - k is even, so sweep s lands in x.
// With a plan, sweep k >= 1 may run over order[level_ptr[k - 1] .. m) only: the rows of level >= k - 1 (it does where that
// set is at most a third of the rows, see trsv_sweeps_typed).  A row of level l is still written in sweep l + 1 -- only then do
// BOTH buffers hold its final value; leaving it out from sweep l + 1 on would let sweep l + 2 read the stale value of sweep
// l - 1 from the other buffer.
#include "common.hpp"
#include "complex_api.hpp"
#include "csr_inspect.hpp"
#include "lowp_api.hpp"
#include "trsv_plan.hpp"

#include <algorithm>

#define TRSV_SWEEP_THREADS 256
#define TRSV_SWEEP_BLOCKS_PER_CU 16  // grid cap: twice the 8 workgroups of 256 lanes a CU holds at 8 waves per SIMD
#define TRSV_SWEEP_ACTIVE_DIV 3  // a plan's active set is used when it holds at most m / 3 rows

namespace spb {

// rows order[first .. first + count) (order == nullptr: the rows first .. first + count themselves), one lane group per row,
// the groups of the (capped) grid striding over the rows; the next row's index, entry range and b are loaded while the current
// row is computed.  gather == 0: sweep 0, the sum is 0 by definition and xin is not read.
template <typename T, int G>
__global__ __launch_bounds__(TRSV_SWEEP_THREADS) void trsv_sweep_kernel(int first, int count,
                                                                         const int32_t* __restrict__ order,
                                                                         const int32_t* __restrict__ rowptr,
                                                                         const int32_t* __restrict__ colind,
                                                                         const T* __restrict__ values, T alpha,
                                                                         const T* __restrict__ b, const T* __restrict__ xin,
                                                                         T* __restrict__ xout, int upper, int unit, int m,
                                                                         int gather) {
  constexpr int RPB = TRSV_SWEEP_THREADS / G;
  const int lane = threadIdx.x % G;
  const int64_t stride = (int64_t) gridDim.x * RPB;
  int64_t slot = (int64_t) blockIdx.x * RPB + threadIdx.x / G;
  // (whole lane groups leave the loop together: G divides the wavefront, the shuffles below stay inside a group)
  int r = -1, p = 0, p1 = 0;
  T br = T(0);
  if (slot < count) {
    r = order ? order[first + slot] : first + (int) slot;
    p = rowptr[r] + lane;
    p1 = rowptr[r + 1];
    br = b[r];
  }
  while (r >= 0) {
    slot += stride;
    int nr = -1, np = 0, np1 = 0;
    T nbr = T(0);
    if (slot < count) {
      nr = order ? order[first + slot] : first + (int) slot;
      np = rowptr[nr] + lane;
      np1 = rowptr[nr + 1];
      nbr = b[nr];
    }
    T dot = T(0), dval = T(0);
    int dpos = -1;
    if (gather || !unit) {  // (sweep 0 of a unit solve is x = b)
      // two entries per lane in flight; the additions keep the order of the one-entry loop
      for (; p + G < p1; p += 2 * G) {
        const int c0 = colind[p], c1 = colind[p + G];
        const T a0 = values[p], a1 = values[p + G];
        const bool s0 = c0 >= 0 && c0 < m && trsv_strict(c0, r, upper);
        const bool s1 = c1 >= 0 && c1 < m && trsv_strict(c1, r, upper);
        T x0 = T(0), x1 = T(0);
        if (gather) {
          if (s0)
            x0 = xin[c0];
          if (s1)
            x1 = xin[c1];
        }
        if (s0) {
          if (gather)
            dot += a0 * x0;
        } else if (c0 == r) {
          dpos = p, dval = a0;  // the last stored diagonal entry wins
        }
        if (s1) {
          if (gather)
            dot += a1 * x1;
        } else if (c1 == r) {
          dpos = p + G, dval = a1;
        }
      }
      if (p < p1) {
        const int c = colind[p];
        const T a = values[p];
        if (c >= 0 && c < m && trsv_strict(c, r, upper)) {
          if (gather)
            dot += a * xin[c];
        } else if (c == r) {
          dpos = p, dval = a;
        }
      }
    }
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) {
      dot += __shfl_xor(dot, o, SPB_WAVE);
      const int other = __shfl_xor(dpos, o, SPB_WAVE);
      const T oval = __shfl_xor(dval, o, SPB_WAVE);
      if (other > dpos)
        dpos = other, dval = oval;
    }
    if (lane == 0) {
      T v = br - alpha * dot;
      if (!unit)
        v = v / (alpha * (dpos >= 0 ? dval : T(0)));
      xout[r] = v;
    }
    r = nr, p = np, p1 = np1, br = nbr;
  }
}

template <typename T, int G>
static int trsv_sweeps_typed(spblas_gfx950_handle_t h, const spblas_gfx950_trsv_s* pl, int m, int sweeps, int upper, int unit,
                             const int32_t* rowptr, const int32_t* colind, const T* values, T alpha, const T* b, T* x,
                             T* work) {
  constexpr int rows_per_block = TRSV_SWEEP_THREADS / G;
  const int64_t grid_cap = (int64_t) cu_count(h) * TRSV_SWEEP_BLOCKS_PER_CU;
  if (pl) {  // rows of level <= s are final after s sweeps: more sweeps than levels - 1 change nothing
    const int last = (int) pl->h_level_ptr.size() - 2;
    if (sweeps > last)
      sweeps = last < 0 ? 0 : last;
  }
  for (int k = 0; k <= sweeps; ++k) {
    T* out = ((sweeps - k) & 1) ? work : x;
    const T* in = ((sweeps - k) & 1) ? x : work;
    // the active set: rows of level >= k - 1 (sweeps 0 and 1, and every sweep without a plan: all rows, in index order).
    // It is walked in the plan's level order, which scatters the row reads: measured at 4 M rows a row costs 1.5 x (random
    // columns) to 2.5 x (7-point Laplacian, whose levels are hyperplanes) what it costs in index order, so the set is used
    // only where it holds at most a third of the rows; otherwise the sweep covers all rows -- the rows below the set are
    // at their fixed point and are rewritten with the same bits.
    int first = (pl && k >= 1) ? pl->h_level_ptr[(size_t) k - 1] : 0;
    if ((int64_t) (m - first) * TRSV_SWEEP_ACTIVE_DIV > m)
      first = 0;
    const int count = m - first;
    if (count <= 0)
      continue;
    const int64_t grid = std::min<int64_t>(cdiv(count, rows_per_block), grid_cap);
    hipLaunchKernelGGL((trsv_sweep_kernel<T, G>), dim3((unsigned) grid), dim3(TRSV_SWEEP_THREADS), 0,
                       h->stream, first, count, first > 0 ? pl->order : nullptr, rowptr, colind, values, alpha, b, in, out,
                       upper, unit, m, k > 0 ? 1 : 0);
  }
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

template <typename T>
static int trsv_sweeps_lanes(spblas_gfx950_handle_t h, const spblas_gfx950_trsv_s* pl, int lanes, int m, int sweeps, int upper,
                             int unit, const int32_t* rowptr, const int32_t* colind, const void* values, const void* alpha,
                             const void* b, void* x, void* work) {
  const T* v = static_cast<const T*>(values);
  const T a = *static_cast<const T*>(alpha);
  const T* bb = static_cast<const T*>(b);
  T* xx = static_cast<T*>(x);
  T* ww = static_cast<T*>(work);
  return with_lanes(lanes, [&](auto g) {
    return trsv_sweeps_typed<T, decltype(g)::value>(h, pl, m, sweeps, upper, unit, rowptr, colind, v, a, bb, xx, ww);
  });
}

} // namespace spb

using namespace spb;

extern "C" {

int spblas_gfx950_sptrsv_sweeps(spblas_gfx950_handle_t handle, spblas_gfx950_trsv_t plan, int64_t m, int64_t nnz, int sweeps,
                                int uplo, int diag, const void* alpha, const int32_t* rowptr, const int32_t* colind,
                                const void* values, const void* b, void* x, void* work, int value_type) {
  if (is_complex_type(value_type) || is_lowp_type(value_type))  // complex / 16-bit values: SpMV / SpMM only
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!alpha || !rowptr || (nnz > 0 && (!colind || !values)) || (m > 0 && (!b || !x)) || (!work && sweeps != 0 && m != 0))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (m < 0 || nnz < 0 || m >= INT32_MAX || nnz > INT32_MAX || sweeps < 0)  // the limits of sptrsv_create
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if ((uplo != SPBLAS_GFX950_LOWER && uplo != SPBLAS_GFX950_UPPER) ||
      (diag != SPBLAS_GFX950_DIAG_EXPLICIT && diag != SPBLAS_GFX950_DIAG_UNIT))
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (plan && (plan->m != m || plan->nnz != nnz || plan->uplo != uplo || plan->diag != diag))
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  if (m > 0 && (b == x || (work && (work == x || work == b))))  // every sweep reads b; the iterates alternate between x and work
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (value_type != SPBLAS_GFX950_F32 && value_type != SPBLAS_GFX950_F64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (m == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  if (plan)
    note_use(plan->use, handle->stream);  // (the sweeps walk the plan's row order)
  const int lanes = lanes_per_row(m, nnz);  // sptrsv_create's call: with and without a plan the same lanes, hence the same bits
  const int upper = uplo == SPBLAS_GFX950_UPPER, unit = diag == SPBLAS_GFX950_DIAG_UNIT;
  if (value_type == SPBLAS_GFX950_F32)
    return trsv_sweeps_lanes<float>(handle, plan, lanes, (int) m, sweeps, upper, unit, rowptr, colind, values, alpha, b, x, work);
  return trsv_sweeps_lanes<double>(handle, plan, lanes, (int) m, sweeps, upper, unit, rowptr, colind, values, alpha, b, x, work);
}

} // extern "C"

// Loads this file's code object with the library's others (handle.hip: spblas_gfx950_create), so that a first call
// recorded in a graph finds its kernels loaded.
namespace spb {
void preload_sptrsv_sweeps() {
  hipFuncAttributes attr;
  (void) hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&trsv_sweep_kernel<float, 8>));
  (void) hipGetLastError();
}
} // namespace spb
