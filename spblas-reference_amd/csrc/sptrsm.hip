// Sparse triangular solve with several right-hand sides  X(:, j) = inv(T) B(:, j),  j = 0 .. n-1,  on gfx950.
//
// T is the triangle the vector solve reads (head comment of sptrsv.hip): the strict triangle named by `uplo`, the last
// stored diagonal entry of a row or the implicit unit diagonal, entries whose column lies outside [0, m) ignored, alpha from
// scaled(alpha, A).  The plan is the one of spblas_gfx950_sptrsv_create, unchanged (rows sorted by level, launch groups,
// lanes per row, narrow threshold): one launch per wide level, one single-workgroup launch per run of narrow levels.  A
// level costs one hand-off whatever n is (sptrsv.hip: the vector solve is bound by that latency, not by bytes), so the n
// columns share it.
//
// Work split: a TEAM of E x C lanes of one wavefront owns a row.  The n columns are cut into UNITS of V = 16 bytes / sizeof(T)
// consecutive columns (4 fp32, 2 fp64); lane (e, c) of the team takes the row's entries e, e + E, ... and the units c, c + C,
// ...; the E partial sums of a unit are added by __shfl_xor over the entry lanes (a fixed tree: the bits of a (row, column)
// depend on E and on that column's operands only, never on the values of another column), lane e = 0 subtracts from B and
// divides.  Neighbouring lanes hold neighbouring units of the SAME gathered row of X, so a team reads C x 16 contiguous
// bytes per entry.
//   X layout_right with a row stride that is a multiple of 16 bytes (TRSM_VEC): a unit that lies inside [0, n) and on a
//   16-byte boundary is ONE buffer_load / buffer_store_dwordx4 with the sc1 bit (raw_buffer_*_b128, aux 16).  Which columns
//   start a unit follows the pointer's misalignment (`mis` elements past a 16-byte boundary), the same for every row; the
//   columns before the first and after the last whole unit are partial units and go element by element.  A buffer
//   descriptor addresses 4 GiB: a wider X takes the element path.
//   Anything else (layout_left X, odd leading dimension): the same split, every element through its strides.
// Hand-off of X inside a launch (the single-workgroup kernel walks many levels): every X value is stored write-through at
// agent scope and every load of X is an agent-scope load -- 16-byte pieces through the buffer forms above, elements through
// __hip_atomic_load / _store(RELAXED, AGENT) -- exactly as the vector kernels do; B is read with plain loads (a B that IS X
// is read by the lane that later stores the same bytes, and nobody else writes them).
// All element offsets into B / X are 64-bit.
//
// A cooperative one-launch form (trsv_coop_kernel's scheme: a grid barrier per wide level) was built and measured against
// these launches at 4 M rows / 246 levels and lost at every n (fp32: n = 4 2.07 vs 1.98 ms, n = 8 2.25 vs 2.05, n = 16 3.02
// vs 2.39, n = 64 5.93 vs 4.14; fp64 the same picture): with n columns a level is no longer one dependent load but real
// work, and 256 resident workgroups hold fewer rows in flight than a launch sized to the level.  It is not part of this
// file.
#include "common.hpp"
#include "complex_api.hpp"
#include "lowp_api.hpp"
#include "trsv_plan.hpp"

#include <cstdint>

#define TRSM_CHAIN_THREADS 1024
#define TRSM_MAX_C 16  // unit lanes per team at most (16 x 16 bytes = 256 contiguous bytes per gathered row and pass)

namespace spb {

typedef unsigned trsm_u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
struct trsm_piece;  // the 16-byte piece of T
template <>
struct trsm_piece<float> {
  typedef float type __attribute__((ext_vector_type(4)));
};
template <>
struct trsm_piece<double> {
  typedef double type __attribute__((ext_vector_type(2)));
};

template <typename T>
struct trsm_args {
  const int32_t* order;
  const int32_t* rowptr;
  const int32_t* colind;
  const T* values;
  T alpha;
  const T* B;
  int64_t brs, bcs;
  T* X;
  int64_t xrs, xcs;
  unsigned x_bytes;  // TRSM_VEC: bytes the buffer descriptor of X spans
  int n, mis, units;  // columns; elements of X's misalignment; units per row = ceil((n + mis) / V)
  int b_piece;        // TRSM_VEC: whole units of B are aligned 16-byte pieces as well
  int E, logC;        // entry lanes and log2(unit lanes) of a team
  int upper, unit, m;
};

// One row, solved by its team.  `t` = lane index inside the team.
template <typename T, bool VEC>
__device__ __forceinline__ void trsm_row(const trsm_args<T>& a, int r, int t) {
  constexpr int V = 16 / (int) sizeof(T);
  typedef typename trsm_piece<T>::type piece_t;
  const int C = 1 << a.logC, cl = t & (C - 1), e = t >> a.logC, E = a.E;
  const int p0 = a.rowptr[r], p1 = a.rowptr[r + 1];
  __amdgpu_buffer_rsrc_t xrsrc;
  if constexpr (VEC)
    xrsrc = __builtin_amdgcn_make_buffer_rsrc(a.X, 0, (int) a.x_bytes, 0x00020000);
  for (int u0 = 0; u0 < a.units; u0 += C) {  // (team-uniform trip count: every lane takes part in the shuffles)
    const int u = u0 + cl;
    const int lo = u * V - a.mis;  // first column of the unit (negative inside the partial unit in front)
    const int j0 = lo > 0 ? lo : 0, j1 = u < a.units ? (lo + V < a.n ? lo + V : a.n) : j0;
    const bool whole = VEC && j1 - j0 == V;
    // the right-hand side of the unit, issued with the row's other loads (entry lane 0 alone needs it)
    T bv[V];
#pragma unroll
    for (int k = 0; k < V; ++k)
      bv[k] = T(0);
    if (e == 0) {
      if (whole && a.b_piece) {
        const piece_t pb = *reinterpret_cast<const piece_t*>(a.B + (int64_t) r * a.brs + lo);
#pragma unroll
        for (int k = 0; k < V; ++k)
          bv[k] = pb[k];
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (lo + k >= j0 && lo + k < j1)
            bv[k] = a.B[(int64_t) r * a.brs + (int64_t) (lo + k) * a.bcs];
      }
    }
    T acc[V], dval = T(0);
    int dpos = -1;
#pragma unroll
    for (int k = 0; k < V; ++k)
      acc[k] = T(0);
    for (int p = p0 + e; p < p1; p += E) {
      const int c = a.colind[p];
      const T av = a.values[p];
      if (c >= 0 && c < a.m && trsv_strict(c, r, a.upper)) {
        if (whole) {
          if constexpr (VEC) {
            const unsigned off = (unsigned) (((int64_t) c * a.xrs + lo) * (int64_t) sizeof(T));
            const piece_t px = __builtin_bit_cast(piece_t, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, (int) off, 0, 16));
#pragma unroll
            for (int k = 0; k < V; ++k)
              acc[k] += av * px[k];
          }
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k)
            if (lo + k >= j0 && lo + k < j1)
              acc[k] += av * __hip_atomic_load(a.X + (int64_t) c * a.xrs + (int64_t) (lo + k) * a.xcs, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
        }
      } else if (c == r) {
        dpos = p, dval = av;  // the last stored diagonal entry wins
      }
    }
    for (int o = E >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < V; ++k)
        acc[k] += __shfl_xor(acc[k], o << a.logC, SPB_WAVE);
      const int other = __shfl_xor(dpos, o << a.logC, SPB_WAVE);
      const T oval = __shfl_xor(dval, o << a.logC, SPB_WAVE);
      if (other > dpos)
        dpos = other, dval = oval;
    }
    if (e == 0 && j1 > j0) {
      T xv[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        xv[k] = bv[k] - a.alpha * acc[k];
        if (!a.unit)
          xv[k] = xv[k] / (a.alpha * (dpos >= 0 ? dval : T(0)));
      }
      if (whole) {
        if constexpr (VEC) {
          piece_t px;
#pragma unroll
          for (int k = 0; k < V; ++k)
            px[k] = xv[k];
          const unsigned off = (unsigned) (((int64_t) r * a.xrs + lo) * (int64_t) sizeof(T));
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(trsm_u32x4, px), xrsrc, (int) off, 0, 16);
        }
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (lo + k >= j0 && lo + k < j1)
            __hip_atomic_store(a.X + (int64_t) r * a.xrs + (int64_t) (lo + k) * a.xcs, xv[k], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// one wide level: rows order[f0..f1), one team per row
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void trsm_level_kernel(int f0, int f1, trsm_args<T> a) {
  const int team = a.E << a.logC;
  const int idx = f0 + (int) blockIdx.x * (256 / team) + (int) threadIdx.x / team;
  if (idx >= f1)
    return;
  trsm_row<T, VEC>(a, a.order[idx], (int) threadIdx.x % team);
}

// levels [l0, l1), all narrow: one workgroup, a barrier between levels
template <typename T, bool VEC>
__global__ __launch_bounds__(TRSM_CHAIN_THREADS) void trsm_chain_kernel(int l0, int l1,
                                                                       const int32_t* __restrict__ level_ptr,
                                                                       trsm_args<T> a) {
  const int team = a.E << a.logC;
  for (int l = l0; l < l1; ++l) {
    const int f0 = level_ptr[l], f1 = level_ptr[l + 1];
    for (int idx = f0 + (int) threadIdx.x / team; idx < f1; idx += TRSM_CHAIN_THREADS / team)
      trsm_row<T, VEC>(a, a.order[idx], (int) threadIdx.x % team);
    __threadfence();  // X of this level must be visible to the whole workgroup before the next one
    __syncthreads();
  }
}

template <typename T, bool VEC>
static int trsm_launch(spblas_gfx950_handle_t h, spblas_gfx950_trsv_s* pl, const trsm_args<T>& a) {
  hipStream_t s = h->stream;
  const int team = a.E << a.logC;
  for (const auto& g : pl->groups) {
    if (g.wide) {
      const int f0 = pl->h_level_ptr[g.l0], f1 = pl->h_level_ptr[g.l0 + 1];
      hipLaunchKernelGGL((trsm_level_kernel<T, VEC>), dim3((unsigned) cdiv(f1 - f0, 256 / team)), dim3(256), 0, s, f0, f1, a);
    } else {
      hipLaunchKernelGGL((trsm_chain_kernel<T, VEC>), dim3(1), dim3(TRSM_CHAIN_THREADS), 0, s, g.l0, g.l1, pl->level_ptr, a);
    }
  }
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

template <typename T>
static int trsm_solve_typed(spblas_gfx950_handle_t h, spblas_gfx950_trsv_s* pl, int64_t n, const int32_t* rowptr,
                            const int32_t* colind, const T* values, T alpha, const T* B, int64_t brs, int64_t bcs, T* X,
                            int64_t xrs, int64_t xcs) {
  constexpr int V = 16 / (int) sizeof(T);
  bool capturing = false;
  size_t bar_off = 0;
  // the same entry protocol as the vector solve: control words sized by the plan's first solve (refused under capture), a
  // pending give-up of an earlier solve reported once, the status word zeroed -- spblas_gfx950_sptrsv_status stays truthful
  if (const int rc = trsv_begin_solve(h, pl, &capturing, &bar_off))
    return rc;
  trsm_args<T> a;
  a.order = pl->order;
  a.rowptr = rowptr;
  a.colind = colind;
  a.values = values;
  a.alpha = alpha;
  a.B = B;
  a.brs = brs;
  a.bcs = bcs;
  a.X = X;
  a.xrs = xrs;
  a.xcs = xcs;
  a.n = (int) n;
  a.upper = pl->uplo == SPBLAS_GFX950_UPPER;
  a.unit = pl->diag == SPBLAS_GFX950_DIAG_UNIT;
  a.m = (int) pl->m;
  // 16-byte pieces of X: layout_right, rows a multiple of 16 bytes apart, element-aligned base, at least one whole unit,
  // and all of X within reach of one buffer descriptor (32-bit byte offsets)
  const uintptr_t xaddr = reinterpret_cast<uintptr_t>(X), baddr = reinterpret_cast<uintptr_t>(B);
  const int64_t x_span = ((pl->m - 1) * xrs + n) * (int64_t) sizeof(T);
  const bool vec = xcs == 1 && (xrs * (int64_t) sizeof(T)) % 16 == 0 && xaddr % sizeof(T) == 0 && n >= V &&
                   x_span <= (int64_t) 0xFFFFFFF0u;
  a.mis = vec ? (int) ((xaddr % 16) / sizeof(T)) : 0;
  a.units = (int) cdiv(n + a.mis, V);
  a.x_bytes = vec ? (unsigned) x_span : 0u;
  a.b_piece = vec && bcs == 1 && (brs * (int64_t) sizeof(T)) % 16 == 0 && baddr % 16 == xaddr % 16;
  int logC = 0;
  while ((1 << logC) < a.units && (1 << logC) < TRSM_MAX_C)
    ++logC;
  a.logC = logC;
  a.E = pl->lanes < (SPB_WAVE >> logC) ? pl->lanes : (SPB_WAVE >> logC);
  auto& last = h->sptrsm_last;  // the decision, for spblas_gfx950_sptrsm_last
  last.path = vec ? SPBLAS_GFX950_SPTRSM_PIECES : SPBLAS_GFX950_SPTRSM_ELEMENTS;
  last.mis = a.mis;
  last.units = a.units;
  last.logC = a.logC;
  last.E = a.E;
  last.b_piece = a.b_piece;
  last.x_bytes = a.x_bytes;
  last.passes = cdiv(a.units, (int64_t) 1 << logC);
  return vec ? trsm_launch<T, true>(h, pl, a) : trsm_launch<T, false>(h, pl, a);
}

} // namespace spb

using namespace spb;

extern "C" int spblas_gfx950_sptrsm_solve(spblas_gfx950_handle_t handle, spblas_gfx950_trsv_t plan, int64_t m, int64_t nnz,
                                          int64_t n, const void* alpha, const int32_t* rowptr, const int32_t* colind,
                                          const void* values, const void* B, int64_t brs, int64_t bcs, void* X, int64_t xrs,
                                          int64_t xcs, int value_type) {
  if (is_complex_type(value_type) || is_lowp_type(value_type))  // complex / 16-bit values: SpMV / SpMM only
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan || !alpha || !rowptr || (nnz > 0 && (!colind || !values)) || (m > 0 && n > 0 && (!B || !X)))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (m != plan->m || nnz != plan->nnz)
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  if (value_type != SPBLAS_GFX950_F32 && value_type != SPBLAS_GFX950_F64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  // each operand is layout_right (column stride 1, rows >= n apart) or layout_left (row stride 1, columns >= m apart): the rule
  // of spblas_gfx950_spmm_strided
  const auto layout_ok = [m, n](int64_t rs, int64_t cs) {
    return (cs == 1 && rs >= n) || (rs == 1 && cs >= m) || m <= 1 || n <= 1;
  };
  if (n < 0 || n > INT32_MAX - 16 || brs < 0 || bcs < 0 || xrs < 0 || xcs < 0 || !layout_ok(brs, bcs) || !layout_ok(xrs, xcs))
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if (m == 0 || n == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  if (n == 1 && (m == 1 || (brs == 1 && xrs == 1))) {  // two contiguous vectors: the vector solve itself, bit for bit
    const int rc = spblas_gfx950_sptrsv_solve(handle, plan, m, nnz, alpha, rowptr, colind, values, B, X, value_type);
    if (rc == SPBLAS_GFX950_STATUS_SUCCESS) {
      handle->sptrsm_last = {};
      handle->sptrsm_last.path = SPBLAS_GFX950_SPTRSM_FORWARDED;
    }
    return rc;
  }
  if (value_type == SPBLAS_GFX950_F32)
    return trsm_solve_typed<float>(handle, plan, n, rowptr, colind, static_cast<const float*>(values),
                                   *static_cast<const float*>(alpha), static_cast<const float*>(B), brs, bcs,
                                   static_cast<float*>(X), xrs, xcs);
  return trsm_solve_typed<double>(handle, plan, n, rowptr, colind, static_cast<const double*>(values),
                                  *static_cast<const double*>(alpha), static_cast<const double*>(B), brs, bcs,
                                  static_cast<double*>(X), xrs, xcs);
}

// What the last block solve on this handle decided (a diagnostic for tests: the counterpart of spblas_gfx950_spmv_t_last).
extern "C" int spblas_gfx950_sptrsm_last(spblas_gfx950_handle_t handle, int64_t* out, int n_out) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!out)
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (n_out < 1)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  const auto& last = handle->sptrsm_last;
  const int64_t v[8] = {last.path, last.mis, last.units, last.logC, last.E, last.b_piece, last.x_bytes, last.passes};
  for (int i = 0; i < n_out && i < 8; ++i)
    out[i] = v[i];
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

// Loads this file's code object at handle creation (handle.hip), as the other files do.
namespace spb {
void preload_sptrsm() {
  hipFuncAttributes attr;
  (void) hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&trsm_level_kernel<float, true>));
  (void) hipGetLastError();
}
} // namespace spb
