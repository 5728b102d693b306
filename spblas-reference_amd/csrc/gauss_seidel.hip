// Multicolour Gauss-Seidel / SOR / SSOR sweeps on a square CSR matrix (no reference counterpart).
//
// sigma = the row order: sigma(i) = perm[i] when the inspect was given a perm, else i.  Colour c is the positions
// color_ptr[c] .. color_ptr[c + 1] - 1 of that order.  One row update is
//   dot = sum of a_rc * x_c over the stored entries of row r with c != r, as stored (repeated off-diagonal entries are summed)
//   g   = (b_r - dot) / d_r                         d_r = the row's ONE stored diagonal entry
//   x_r = g                      if omega == 1  (the old x_r is not read)
//   x_r = fma(omega, g - x_r, x_r)   otherwise
// A forward sweep updates the colours 0 .. C - 1 one after the other, a backward sweep C - 1 .. 0, a symmetric sweep is a
// forward one followed by a backward one.  gs_create checks that no stored off-diagonal entry joins two rows of one colour (the
// colouring multicolor_create gives): the rows of a colour neither read nor write each other's x, so one launch that updates
// a colour IN PLACE is race free, and the whole sweep equals sequential Gauss-Seidel in colour order bit for bit, whatever the
// schedule.  The bits of x depend on the matrix, the colouring, b, the incoming x, omega, the number of sweeps and the
// direction -- not on the grid, on earlier calls or on whether the launches were recorded in a graph.
//
// Kernel: a relative of trsv_sweep_kernel (sptrsv_sweeps.hip) that reads and writes the SAME vector, covers both triangles,
// carries omega and walks one colour's range of the row order.  A group of G lanes owns a row (G = lanes_per_row of
// csr_inspect.hpp), strides its entries two per lane in flight and reduces in trsv_row's order (the bits depend on G alone);
// lane 0 applies the update.  The groups of a capped grid stride over the colour's rows and load the NEXT row's index, entry
// range, b and diagonal (through the plan's diagonal positions) while the current row is computed -- none of those loads
// touches x.  x is one pointer, read and written, hence not __restrict__; a colour ends at a kernel boundary: plain loads and
// stores, no atomics, no cooperative launch, nothing that can wait.
//
// Not offered: a block of right-hand sides, weighted Jacobi, an implied zero initial guess that skips the gathers, several
// colours per launch, scaled operands, complex / 16-bit values, int64 indices, CSC operands, distance-2 colourings.
#include "common.hpp"
#include "complex_api.hpp"
#include "csr_inspect.hpp"
#include "lowp_api.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#define GS_THREADS 256
#define GS_BLOCKS_PER_CU 16  // the grid cap of sptrsv_sweeps.hip: twice the 8 workgroups of 256 lanes a CU holds at 8 waves per SIMD

struct spblas_gfx950_gs_s {
  int64_t m = 0, nnz = 0;
  int64_t colours = 0, largest = 0, launches = 0;
  int lanes = 4;
  std::vector<int32_t> h_color_ptr;  // [colours + 1]
  int32_t* diag = nullptr;           // [m] position of row r's diagonal entry in colind / values
  int32_t* perm = nullptr;           // [m] the plan's own copy of the row order; nullptr: the rows themselves
  spb::use_record use;               // the stream of the last sweep: destroy frees behind it
};

namespace spb {

__device__ __forceinline__ float gs_fma(float a, float b, float c) {
  return fmaf(a, b, c);
}
__device__ __forceinline__ double gs_fma(double a, double b, double c) {
  return fma(a, b, c);
}

// positions first .. first + count of the row order (order == nullptr: the rows first .. first + count themselves)
template <typename T, int G>
__global__ __launch_bounds__(GS_THREADS) void gs_color_kernel(int first, int count, const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ colind,
                                                               const T* __restrict__ values,
                                                               const int32_t* __restrict__ diag, const T* __restrict__ b,
                                                               T* x, T omega, int relax) {
  constexpr int RPB = GS_THREADS / G;
  const int lane = threadIdx.x % G;
  const int64_t stride = (int64_t) gridDim.x * RPB;
  int64_t slot = (int64_t) blockIdx.x * RPB + threadIdx.x / G;
  // (whole lane groups leave the loop together: G divides the wavefront, the shuffles below stay inside a group)
  int r = -1, p = 0, p1 = 0;
  T br = T(0), dr = T(0);
  if (slot < count) {
    r = order ? order[first + slot] : first + (int) slot;
    p = rowptr[r] + lane;
    p1 = rowptr[r + 1];
    br = b[r];
    dr = values[diag[r]];
  }
  while (r >= 0) {
    slot += stride;
    int nr = -1, np = 0, np1 = 0;
    T nbr = T(0), ndr = T(0);
    if (slot < count) {
      nr = order ? order[first + slot] : first + (int) slot;
      np = rowptr[nr] + lane;
      np1 = rowptr[nr + 1];
      nbr = b[nr];
      ndr = values[diag[nr]];
    }
    T dot = T(0);
    // two entries per lane in flight; the additions keep the order of the one-entry loop
    for (; p + G < p1; p += 2 * G) {
      const int c0 = colind[p], c1 = colind[p + G];
      const T a0 = values[p], a1 = values[p + G];
      T x0 = T(0), x1 = T(0);
      if (c0 != r)
        x0 = x[c0];
      if (c1 != r)
        x1 = x[c1];
      if (c0 != r)
        dot += a0 * x0;
      if (c1 != r)
        dot += a1 * x1;
    }
    if (p < p1) {
      const int c = colind[p];
      const T a = values[p];
      if (c != r)
        dot += a * x[c];
    }
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1)
      dot += __shfl_xor(dot, o, SPB_WAVE);
    if (lane == 0) {
      const T g = (br - dot) / dr;
      if (relax) {
        const T old = x[r];
        x[r] = gs_fma(omega, g - old, old);
      } else {
        x[r] = g;
      }
    }
    r = nr, p = np, p1 = np1, br = nbr, dr = ndr;
  }
}

// ---- the inspect's checks (structure and perm: csr_inspect.hpp).  flag[0] = 1 on a violation.
// color[sigma(i)] = the colour of position i: the last c with color_ptr[c] <= i (color_ptr checked on the host before)
__global__ __launch_bounds__(256) void gs_row_color_kernel(int64_t m, int colours, const int32_t* __restrict__ color_ptr,
                                                           const int32_t* __restrict__ perm, int32_t* __restrict__ color) {
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= m)
    return;
  int lo = 0, hi = colours;  // color_ptr[lo] <= i < color_ptr[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (color_ptr[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  color[perm ? perm[i] : (int) i] = lo;
}
// exactly one stored diagonal entry per row (its position goes to diag[]), no off-diagonal entry inside a colour.  Eight lanes
// per row; structure and perm were checked before, so every index below is in range.
__global__ __launch_bounds__(256) void gs_check_entries_kernel(int64_t m, const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ colind,
                                                               const int32_t* __restrict__ color, int32_t* __restrict__ diag,
                                                               int32_t* __restrict__ flag) {
  const int64_t r64 = (int64_t) blockIdx.x * 32 + threadIdx.x / 8;
  const int r = r64 < m ? (int) r64 : -1;  // (every lane takes part in the shuffles)
  int ndiag = 0, dpos = -1, clash = 0;
  if (r >= 0) {
    const int mine = color[r];
    const int p1 = rowptr[r + 1];
    for (int p = rowptr[r] + (int) threadIdx.x % 8; p < p1; p += 8) {
      const int c = colind[p];
      if (c == r)
        ++ndiag, dpos = p;
      else if (color[c] == mine)
        clash = 1;
    }
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) {
    ndiag += __shfl_xor(ndiag, o, SPB_WAVE);
    dpos = max(dpos, __shfl_xor(dpos, o, SPB_WAVE));
    clash |= __shfl_xor(clash, o, SPB_WAVE);
  }
  if (r >= 0 && threadIdx.x % 8 == 0) {
    if (ndiag != 1 || clash)
      flag[0] = 1;
    diag[r] = dpos;
  }
}

template <typename T, int G>
static int gs_sweep_typed(spblas_gfx950_handle_t h, const spblas_gfx950_gs_s* pl, int sweeps, int direction,
                          const int32_t* rowptr, const int32_t* colind, const T* values, T omega, const T* b, T* x) {
  constexpr int rows_per_block = GS_THREADS / G;
  const int64_t grid_cap = (int64_t) cu_count(h) * GS_BLOCKS_PER_CU;
  const int relax = omega == T(1) ? 0 : 1;
  const int colours = (int) pl->colours;
  auto half = [&](bool forward) {
    for (int k = 0; k < colours; ++k) {
      const int c = forward ? k : colours - 1 - k;
      const int first = pl->h_color_ptr[(size_t) c], count = pl->h_color_ptr[(size_t) c + 1] - first;
      if (count <= 0)
        continue;
      const int64_t grid = std::min<int64_t>(cdiv(count, rows_per_block), grid_cap);
      hipLaunchKernelGGL((gs_color_kernel<T, G>), dim3((unsigned) grid), dim3(GS_THREADS), 0, h->stream, first, count,
                         pl->perm, rowptr, colind, values, pl->diag, b, x, omega, relax);
    }
  };
  for (int s = 0; s < sweeps; ++s) {
    if (direction != SPBLAS_GFX950_GS_BACKWARD)
      half(true);
    if (direction != SPBLAS_GFX950_GS_FORWARD)
      half(false);
  }
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

template <typename T>
static int gs_sweep_lanes(spblas_gfx950_handle_t h, const spblas_gfx950_gs_s* pl, int sweeps, int direction,
                          const int32_t* rowptr, const int32_t* colind, const void* values, const void* omega, const void* b,
                          void* x) {
  const T* v = static_cast<const T*>(values);
  const T w = *static_cast<const T*>(omega);
  const T* bb = static_cast<const T*>(b);
  T* xx = static_cast<T*>(x);
  return with_lanes(pl->lanes, [&](auto g) {
    return gs_sweep_typed<T, decltype(g)::value>(h, pl, sweeps, direction, rowptr, colind, v, w, bb, xx);
  });
}

} // namespace spb

using namespace spb;

extern "C" {

int spblas_gfx950_gs_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_gs_t plan) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  order_behind_last_use(plan->use, handle->stream);  // the last sweep may have run elsewhere and still read these
  dev_free(plan->diag, handle->stream);
  dev_free(plan->perm, handle->stream);
  delete plan;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_gs_create(spblas_gfx950_handle_t handle, spblas_gfx950_gs_t* plan_out, int64_t m, int64_t nnz,
                            const int32_t* rowptr, const int32_t* colind, int64_t colours, const int32_t* color_ptr,
                            const int32_t* perm) {
  if (const int st = inspect_args_status(handle, plan_out && rowptr && color_ptr && (nnz <= 0 || colind), m, nnz))
    return st;
  if (colours < 0 || colours >= INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  *plan_out = nullptr;
  if (m == 0 && nnz != 0)  // no offsets of an empty matrix describe entries
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  auto* pl = new (std::nothrow) spblas_gfx950_gs_s();
  if (!pl)
    return SPBLAS_GFX950_STATUS_ALLOC_FAILED;
  pl->m = m;
  pl->nnz = nnz;
  pl->colours = colours;
  pl->lanes = lanes_per_row(m, nnz);
  hipStream_t s = handle->stream;
  dev_temps temps(s);
  int32_t *flag = nullptr, *seen = nullptr, *color = nullptr;
  auto fail = [&](int code) {
    (void) hipStreamSynchronize(s);
    (void) spblas_gfx950_gs_destroy(handle, pl);
    return code;
  };
  hipError_t e;
  // the colour offsets: checked on the host, where the plan keeps them
  try {
    pl->h_color_ptr.resize((size_t) colours + 1);
  } catch (const std::bad_alloc&) {
    return fail(SPBLAS_GFX950_STATUS_ALLOC_FAILED);
  }
  if ((e = hipMemcpyAsync(pl->h_color_ptr.data(), color_ptr, pl->h_color_ptr.size() * 4, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = hipStreamSynchronize(s)) != hipSuccess)
    return fail(hip_fail(e));
  if (pl->h_color_ptr.front() != 0 || pl->h_color_ptr.back() != m)
    return fail(SPBLAS_GFX950_STATUS_INVALID_VALUE);
  for (int64_t c = 0; c < colours; ++c) {
    const int64_t n = (int64_t) pl->h_color_ptr[(size_t) c + 1] - pl->h_color_ptr[(size_t) c];
    if (n < 0)
      return fail(SPBLAS_GFX950_STATUS_INVALID_VALUE);
    pl->largest = std::max(pl->largest, n);
    pl->launches += n > 0 ? 1 : 0;
  }
  if (m == 0) {
    *plan_out = pl;
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  int rc;
  if ((rc = temps.alloc(&flag, 16)) || (rc = temps.alloc(&color, (size_t) m * 4)) ||
      (rc = dev_alloc((void**) &pl->diag, (size_t) m * 4, s)) || (perm && (rc = temps.alloc(&seen, (size_t) m * 4))) ||
      (perm && (rc = dev_alloc((void**) &pl->perm, (size_t) m * 4, s))))
    return fail(rc);
  if ((e = hipMemsetAsync(flag, 0, 16, s)) != hipSuccess ||
      (perm && (e = hipMemsetAsync(seen, 0xFF, (size_t) m * 4, s)) != hipSuccess))
    return fail(hip_fail(e));
  // perm and the structure are checked, with a synchronisation, BEFORE anything indexes with them
  const dim3 rows_grid((unsigned) cdiv(m, 256)), block(256);
  if (perm)
    hipLaunchKernelGGL(check_perm_kernel, rows_grid, block, 0, s, m, perm, seen, flag);
  if ((rc = check_csr_structure(handle, m, nnz, rowptr, colind, flag)))
    return fail(rc);
  // one diagonal entry per row, no entry inside a colour
  hipLaunchKernelGGL(gs_row_color_kernel, rows_grid, block, 0, s, m, (int) colours, color_ptr, perm, color);
  hipLaunchKernelGGL(gs_check_entries_kernel, dim3((unsigned) cdiv(m, 32)), block, 0, s, m, rowptr, colind, color, pl->diag, flag);
  if ((e = hipGetLastError()) != hipSuccess ||
      (perm && (e = hipMemcpyAsync(pl->perm, perm, (size_t) m * 4, hipMemcpyDeviceToDevice, s)) != hipSuccess))
    return fail(hip_fail(e));
  if ((rc = read_flag(handle, flag)))
    return fail(rc);
  *plan_out = pl;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_gs_info(spblas_gfx950_gs_t plan, int64_t info[4]) {
  if (!plan || !info)
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  info[0] = plan->colours;
  info[1] = plan->largest;   // rows of the largest colour
  info[2] = plan->lanes;     // lanes per row
  info[3] = plan->launches;  // launches per forward sweep: the non-empty colours
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_gs_sweep(spblas_gfx950_handle_t handle, spblas_gfx950_gs_t plan, int64_t m, int64_t nnz, int sweeps,
                           int direction, const void* omega, const int32_t* rowptr, const int32_t* colind, const void* values,
                           const void* b, void* x, int value_type) {
  if (is_complex_type(value_type) || is_lowp_type(value_type))  // complex / 16-bit values: SpMV / SpMM only
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan || !omega || !rowptr || (nnz > 0 && (!colind || !values)) || (m > 0 && (!b || !x)))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (m < 0 || nnz < 0 || m >= INT32_MAX || nnz > INT32_MAX)  // the limits of gs_create
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if ((direction != SPBLAS_GFX950_GS_FORWARD && direction != SPBLAS_GFX950_GS_BACKWARD &&
       direction != SPBLAS_GFX950_GS_SYMMETRIC) ||
      sweeps < 0 || (m > 0 && b == x) || (value_type != SPBLAS_GFX950_F32 && value_type != SPBLAS_GFX950_F64))
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (plan->m != m || plan->nnz != nnz)
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  if (m == 0 || sweeps == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  note_use(plan->use, handle->stream);
  if (value_type == SPBLAS_GFX950_F32)
    return gs_sweep_lanes<float>(handle, plan, sweeps, direction, rowptr, colind, values, omega, b, x);
  return gs_sweep_lanes<double>(handle, plan, sweeps, direction, rowptr, colind, values, omega, b, x);
}

} // extern "C"

// Loads this file's code object with the library's others (handle.hip: spblas_gfx950_create), so that a first call
// recorded in a graph finds its kernels loaded.
namespace spb {
void preload_gauss_seidel() {
  hipFuncAttributes attr;
  (void) hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&gs_color_kernel<float, 8>));
  (void) hipGetLastError();
}
} // namespace spb
