// Multicolour ordering and symmetric permutation of a square CSR matrix on gfx950 (no reference counterpart).
//
// multicolor_create colours the graph of A + A^T at distance 1 and sorts the rows by colour; csr_permute_create forms
// B = P A P^T with ascending columns.  Rows of one colour share no stored off-diagonal entry, so row i of B depends only on rows
// of lower colours: both triangles of B have at most `colours` levels for ilu0_create / sptrsv_create.
//
// Colouring: Jones-Plassmann with FIXED priorities.
//   key(v) = (uint64(h(v)) << 32) | v, compared unsigned;  h(v) = mix(uint32(v + 1) * 0x9E3779B1u);
//   mix(x): x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16  (32-bit wraparound).
//   The neighbours of v are the columns of row v of A and of row v of A^T (whose pattern the inspect forms once with
//   spblas_gfx950_csr_transpose), without v itself; a neighbour met twice counts once (the forbidden set is a set).
//   One launch per round: every uncoloured v looks at its neighbours; if one of them is uncoloured and has a larger key, v waits
//   for a later round; otherwise v takes the smallest colour no neighbour holds.
// Determinism: v takes its colour only after every neighbour with a larger key was SEEN coloured, and a neighbour with a smaller
// key cannot take one before v has (it waits for v).  So v's colour is the smallest one that no larger-key neighbour holds -- the
// colour sequential greedy colouring gives v when the vertices are visited in descending key order.  The colours depend on the
// pattern alone, not on the schedule, the lanes per row or the launch; only the number of rounds may vary.
// colour[] is one array, -1 = uncoloured; every element is written once (agent-scope store) and read with agent-scope loads, so a
// colour written earlier in the same launch may be seen (fewer rounds); a stale -1 only delays a vertex.  The uncoloured vertex of
// the largest key never waits, so every round colours at least one vertex: at most m rounds.
//
// Row work: a TEAM of G lanes of one wavefront owns a vertex (G = lanes_per_row(m, nnz), csr_inspect.hpp).  Every
// lane keeps a 64-bit mask of the colours base .. base + 63 it met; the masks are OR-reduced over the team by shuffles.  A full
// window moves base on by 64 and the neighbours are scanned again: nothing is sized by the degree.
//
// Every round runs over ALL vertices (a coloured one costs one load); the host reads the count of coloured vertices after
// every round.  perm / color_ptr are the stable counting sort of the vertices by colour -- the transpose of the m x colours
// matrix with one entry per row, by the existing transpose (whose offsets come from the scans in scan.hpp).
//
// Permutation: row i of B is row perm[i] of A with column c renamed inv_perm[c].  The rows are brought into ascending column
// order by two passes of the existing stable transpose over the renamed matrix, carrying the SOURCE POSITION of every entry as the
// 4-byte payload: the first pass orders by column, the second by row and keeps the column order inside a row; equal columns keep
// their source order.  The payload of the second pass is the plan's entry map; csr_permute_values is one gather through it.
#include "common.hpp"
#include "complex_api.hpp"
#include "csr_inspect.hpp"
#include "lowp_api.hpp"
#include "mc_key.hpp"
#include "scan.hpp"

#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#define MC_THREADS 256

struct spblas_gfx950_multicolor_s {
  int64_t m = 0, nnz = 0;
  int64_t colours = 0, rounds = 0, largest = 0;
  int lanes = 4;
  int32_t* color = nullptr;      // [m]
  int32_t* perm = nullptr;       // [m] new -> old, sorted by (colour, old index)
  int32_t* inv_perm = nullptr;   // [m] old -> new
  int32_t* color_ptr = nullptr;  // [colours + 1] first new index of every colour
  spb::use_record use;           // the stream of the last copy out of the plan: destroy frees behind it
};

struct spblas_gfx950_permute_s {
  int64_t m = 0, nnz = 0;
  int32_t* map = nullptr;  // [nnz] position in A's arrays of B's entry p
  spb::use_record use;     // the stream of the last gather through the map: destroy frees behind it
};

namespace spb {

// (mc_key: mc_key.hpp, shared with aggregate.hip)
struct mc_args {
  const int32_t *rowptr, *colind;      // A
  const int32_t *t_rowptr, *t_colind;  // the pattern of A^T
  int32_t* color;
  unsigned* counters;  // [0] vertices coloured so far, [1] colours in use (largest colour + 1)
  int m;
};

// one neighbour list of v: what the team's lane t learns from its share of it
__device__ __forceinline__ void mc_scan(const int32_t* __restrict__ colind, int p0, int p1, int t, int G, int v, uint64_t kv,
                                        int base, const int32_t* color, uint64_t& mask, int& wait) {
  for (int p = p0 + t; p < p1; p += G) {
    const int u = colind[p];
    if (u == v)
      continue;
    const int c = __hip_atomic_load(color + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c < 0) {
      if (mc_key(u) > kv)
        wait = 1;
    } else if (c >= base && c < base + 64) {
      mask |= 1ull << (c - base);
    }
  }
}

// One round over all vertices, one team of G lanes per vertex.  All control flow below is uniform inside a team (v, colour[v] --
// written by this team alone -- and the reduced mask / wait are), so the shuffles only read lanes that are active.
template <int G>
__global__ __launch_bounds__(MC_THREADS) void mc_round_kernel(mc_args a) {
  const int t = (int) threadIdx.x % G;
  const int64_t v64 = (int64_t) blockIdx.x * (MC_THREADS / G) + (int) threadIdx.x / G;
  int mine = -1;  // lane 0 of a team that coloured its vertex in this round: the colour
  if (v64 < a.m && __hip_atomic_load(a.color + v64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) {
    const int v = (int) v64;
    const uint64_t kv = mc_key(v);
    const int p0 = a.rowptr[v], p1 = a.rowptr[v + 1], q0 = a.t_rowptr[v], q1 = a.t_rowptr[v + 1];
    // a neighbour with a smaller key stays uncoloured until v is coloured, one with a larger key is coloured for good once it was
    // seen so: the forbidden set does not change between the scans of two windows
    for (int base = 0;; base += 64) {
      uint64_t mask = 0;
      int wait = 0;
      mc_scan(a.colind, p0, p1, t, G, v, kv, base, a.color, mask, wait);
      mc_scan(a.t_colind, q0, q1, t, G, v, kv, base, a.color, mask, wait);
#pragma unroll
      for (int o = G >> 1; o > 0; o >>= 1) {
        mask |= __shfl_xor(mask, o, SPB_WAVE);
        wait |= __shfl_xor(wait, o, SPB_WAVE);
      }
      if (wait)
        break;
      if (~mask != 0ull) {
        const int c = base + __builtin_ctzll(~mask);
        if (t == 0) {
          __hip_atomic_store(a.color + v, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          mine = c;
        }
        break;
      }
    }
  }
  // one pair of atomics per wavefront
  const unsigned long long done = __ballot(mine >= 0);
  int top = mine;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    top = max(top, __shfl_xor(top, o, SPB_WAVE));
  if ((threadIdx.x & 63) == 0 && done != 0ull) {
    atomicAdd(a.counters, (unsigned) __popcll(done));
    atomicMax(a.counters + 1, (unsigned) top + 1u);
  }
}

// (the structure and perm checks of the two inspects: csr_inspect.hpp)
__global__ __launch_bounds__(256) void mc_iota_kernel(int64_t n, int32_t* __restrict__ out) {
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i < n)
    out[i] = (int32_t) i;
}

__global__ __launch_bounds__(256) void mc_invert_kernel(int64_t m, const int32_t* __restrict__ perm,
                                                        int32_t* __restrict__ inv) {
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i < m)
    inv[perm[i]] = (int32_t) i;
}

__global__ __launch_bounds__(256) void pm_row_len_kernel(int64_t m, const int32_t* __restrict__ perm,
                                                         const int32_t* __restrict__ rowptr, int32_t* __restrict__ len) {
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i < m) {
    const int r = perm[i];
    len[i] = rowptr[r + 1] - rowptr[r];
  }
}

// rows of A in the new order, columns renamed, not yet sorted: eight lanes per row; pos[] = the entry's place in A's arrays
__global__ __launch_bounds__(256) void pm_fill_kernel(int64_t m, const int32_t* __restrict__ perm, const int32_t* __restrict__ inv,
                                                      const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                      const int32_t* __restrict__ b_rowptr, int32_t* __restrict__ col,
                                                      int32_t* __restrict__ pos) {
  const int64_t i = (int64_t) blockIdx.x * 32 + threadIdx.x / 8;
  if (i >= m)
    return;
  const int r = perm[i];
  const int s0 = rowptr[r], len = rowptr[r + 1] - s0, d0 = b_rowptr[i];
  for (int e = (int) threadIdx.x % 8; e < len; e += 8) {
    col[d0 + e] = inv[colind[s0 + e]];
    pos[d0 + e] = s0 + e;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void pm_gather_kernel(int64_t n, const int32_t* __restrict__ map, const T* __restrict__ src,
                                                        T* __restrict__ dst) {
  for (int64_t p = (int64_t) blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t) gridDim.x * 256)
    dst[p] = src[map[p]];
}
template <typename T>
__global__ __launch_bounds__(256) void pm_scatter_kernel(int64_t n, const int32_t* __restrict__ map, const T* __restrict__ src,
                                                         T* __restrict__ dst) {
  for (int64_t p = (int64_t) blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t) gridDim.x * 256)
    dst[map[p]] = src[p];
}

static void launch_round(hipStream_t s, int lanes, const mc_args& a) {
  with_lanes(lanes, [&](auto g) {
    constexpr int G = decltype(g)::value;
    hipLaunchKernelGGL(mc_round_kernel<G>, dim3((unsigned) cdiv(a.m, MC_THREADS / G)), dim3(MC_THREADS), 0, s, a);
  });
}

} // namespace spb

using namespace spb;

extern "C" {

int spblas_gfx950_multicolor_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_multicolor_t plan) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  order_behind_last_use(plan->use, handle->stream);
  dev_free(plan->color, handle->stream);
  dev_free(plan->perm, handle->stream);
  dev_free(plan->inv_perm, handle->stream);
  dev_free(plan->color_ptr, handle->stream);
  delete plan;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_multicolor_create(spblas_gfx950_handle_t handle, spblas_gfx950_multicolor_t* plan_out, int64_t m, int64_t nnz,
                                    const int32_t* rowptr, const int32_t* colind) {
  if (const int st = inspect_args_status(handle, plan_out && rowptr && (nnz <= 0 || colind), m, nnz))
    return st;
  *plan_out = nullptr;
  if (m == 0 && nnz != 0)  // no offsets of an empty matrix describe entries
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  auto* pl = new (std::nothrow) spblas_gfx950_multicolor_s();
  if (!pl)
    return SPBLAS_GFX950_STATUS_ALLOC_FAILED;
  pl->m = m;
  pl->nnz = nnz;
  pl->lanes = lanes_per_row(m, nnz);
  hipStream_t s = handle->stream;
  dev_temps temps(s);
  int32_t *flag = nullptr, *t_rowptr = nullptr, *t_colind = nullptr, *junk = nullptr, *iota = nullptr;
  unsigned* counters = nullptr;
  auto fail = [&](int code) {
    (void) hipStreamSynchronize(s);
    (void) spblas_gfx950_multicolor_destroy(handle, pl);
    return code;
  };
  int rc;
  hipError_t e;
  if ((rc = dev_alloc((void**) &pl->color_ptr, 4, s)))
    return fail(rc);
  if (m == 0) {
    if ((e = hipMemsetAsync(pl->color_ptr, 0, 4, s)) != hipSuccess)
      return fail(hip_fail(e));
    *plan_out = pl;
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  dev_free(pl->color_ptr, s);  // sized once the colours are counted
  pl->color_ptr = nullptr;
  if ((rc = temps.alloc(&flag, 16)) || (rc = temps.alloc(&counters, 16)) ||
      (rc = dev_alloc((void**) &pl->color, (size_t) m * 4, s)) || (rc = dev_alloc((void**) &pl->perm, (size_t) m * 4, s)) ||
      (rc = dev_alloc((void**) &pl->inv_perm, (size_t) m * 4, s)))
    return fail(rc);
  if ((e = hipMemsetAsync(flag, 0, 16, s)) != hipSuccess || (e = hipMemsetAsync(counters, 0, 16, s)) != hipSuccess ||
      (e = hipMemsetAsync(pl->color, 0xFF, (size_t) m * 4, s)) != hipSuccess)
    return fail(hip_fail(e));
  // the structure is checked, with a synchronisation of its own, BEFORE the transpose sees it
  if ((rc = check_csr_structure(handle, m, nnz, rowptr, colind, flag)))
    return fail(rc);
  // the pattern of A^T; the transpose moves 4-byte values along, here the columns themselves, into a buffer nobody reads
  const size_t junk_n = (size_t) std::max(m, nnz);
  if ((rc = temps.alloc(&t_rowptr, (size_t) (m + 1) * 4)) || (rc = temps.alloc(&t_colind, (size_t) nnz * 4)) ||
      (rc = temps.alloc(&junk, junk_n * 4)) || (rc = temps.alloc(&iota, (size_t) (m + 1) * 4)))
    return fail(rc);
  if ((rc = spblas_gfx950_csr_transpose(handle, m, m, nnz, rowptr, colind, colind, t_rowptr, t_colind, junk,
                                        SPBLAS_GFX950_F32)))
    return fail(rc);
  mc_args a;
  a.rowptr = rowptr;
  a.colind = colind;
  a.t_rowptr = t_rowptr;
  a.t_colind = t_colind;
  a.color = pl->color;
  a.counters = counters;
  a.m = (int) m;
  unsigned h_cnt[2] = {0u, 0u};
  {
    readback_scope rb(handle);
    while ((int64_t) h_cnt[0] < m) {
      const unsigned before = h_cnt[0];
      launch_round(s, pl->lanes, a);
      if ((e = hipGetLastError()) != hipSuccess)
        return fail(hip_fail(e));
      if ((rc = readback_add(handle, h_cnt, counters, 8)) || (rc = readback_flush(handle)))
        return fail(rc);
      ++pl->rounds;
      if (h_cnt[0] == before || pl->rounds > m)  // cannot happen: the uncoloured vertex of the largest key never waits
        return fail(SPBLAS_GFX950_STATUS_HIP_ERROR);
    }
  }
  pl->colours = (int64_t) h_cnt[1];
  // perm and color_ptr: the vertices sorted by (colour, index) = the transpose of the m x colours matrix whose row v holds the
  // one entry (v, colour[v]); its row offsets are the class offsets, its columns the permutation
  if ((rc = dev_alloc((void**) &pl->color_ptr, (size_t) (pl->colours + 1) * 4, s)))
    return fail(rc);
  hipLaunchKernelGGL(mc_iota_kernel, dim3((unsigned) cdiv(m + 1, 256)), dim3(256), 0, s, m + 1, iota);
  if ((rc = spblas_gfx950_csr_transpose(handle, m, pl->colours, m, iota, pl->color, pl->color, pl->color_ptr, pl->perm, junk,
                                        SPBLAS_GFX950_F32)))
    return fail(rc);
  hipLaunchKernelGGL(mc_invert_kernel, dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, pl->perm, pl->inv_perm);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(hip_fail(e));
  std::vector<int32_t> h_ptr((size_t) pl->colours + 1);
  if ((e = hipMemcpyAsync(h_ptr.data(), pl->color_ptr, h_ptr.size() * 4, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = hipStreamSynchronize(s)) != hipSuccess)
    return fail(hip_fail(e));
  for (int64_t c = 0; c < pl->colours; ++c)
    pl->largest = std::max<int64_t>(pl->largest, h_ptr[c + 1] - h_ptr[c]);
  *plan_out = pl;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_multicolor_info(spblas_gfx950_multicolor_t plan, int64_t info[4]) {
  if (!plan || !info)
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  info[0] = plan->colours;
  info[1] = plan->rounds;
  info[2] = plan->largest;  // vertices of the largest colour class
  info[3] = plan->lanes;    // lanes per row
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_multicolor_copy(spblas_gfx950_handle_t handle, spblas_gfx950_multicolor_t plan, int32_t* perm,
                                  int32_t* inv_perm, int32_t* color, int32_t* color_ptr) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan)
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  hipStream_t s = handle->stream;
  note_use(plan->use, s);
  const size_t mb = (size_t) plan->m * 4;
  if (perm && mb)
    SPB_HIP(hipMemcpyAsync(perm, plan->perm, mb, hipMemcpyDeviceToDevice, s));
  if (inv_perm && mb)
    SPB_HIP(hipMemcpyAsync(inv_perm, plan->inv_perm, mb, hipMemcpyDeviceToDevice, s));
  if (color && mb)
    SPB_HIP(hipMemcpyAsync(color, plan->color, mb, hipMemcpyDeviceToDevice, s));
  if (color_ptr)
    SPB_HIP(hipMemcpyAsync(color_ptr, plan->color_ptr, (size_t) (plan->colours + 1) * 4, hipMemcpyDeviceToDevice, s));
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_csr_permute_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_permute_t plan) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  order_behind_last_use(plan->use, handle->stream);
  dev_free(plan->map, handle->stream);
  delete plan;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_csr_permute_create(spblas_gfx950_handle_t handle, spblas_gfx950_permute_t* plan_out, int64_t m, int64_t nnz,
                                     const int32_t* rowptr, const int32_t* colind, const int32_t* perm, int32_t* b_rowptr,
                                     int32_t* b_colind) {
  if (const int st = inspect_args_status(
          handle, plan_out && rowptr && b_rowptr && (m <= 0 || perm) && (nnz <= 0 || (colind && b_colind)), m, nnz))
    return st;
  *plan_out = nullptr;
  if (m == 0 && nnz != 0)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (b_rowptr == rowptr || (nnz > 0 && b_colind == colind))  // no in-place form
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  auto* pl = new (std::nothrow) spblas_gfx950_permute_s();
  if (!pl)
    return SPBLAS_GFX950_STATUS_ALLOC_FAILED;
  pl->m = m;
  pl->nnz = nnz;
  hipStream_t s = handle->stream;
  dev_temps temps(s);
  int32_t *flag = nullptr, *inv = nullptr, *c_col = nullptr, *c_pos = nullptr, *d_rowptr = nullptr, *d_col = nullptr,
          *d_pos = nullptr;
  long long* partials = nullptr;
  auto fail = [&](int code) {
    (void) hipStreamSynchronize(s);
    (void) spblas_gfx950_csr_permute_destroy(handle, pl);
    return code;
  };
  hipError_t e;
  if (m == 0) {
    if ((e = hipMemsetAsync(b_rowptr, 0, 4, s)) != hipSuccess)
      return fail(hip_fail(e));
    *plan_out = pl;
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  int rc;
  if ((rc = temps.alloc(&flag, 16)) || (rc = temps.alloc(&inv, (size_t) m * 4)))
    return fail(rc);
  if ((e = hipMemsetAsync(flag, 0, 16, s)) != hipSuccess || (e = hipMemsetAsync(inv, 0xFF, (size_t) m * 4, s)) != hipSuccess)
    return fail(hip_fail(e));
  // perm and the structure are checked, with a synchronisation, BEFORE anything indexes with them or B is written
  hipLaunchKernelGGL(check_perm_kernel, dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, perm, inv, flag);
  if ((rc = check_csr_structure(handle, m, nnz, rowptr, colind, flag)))
    return fail(rc);
  if ((rc = temps.alloc(&partials, (size_t) (cdiv(m, 2048) + 2) * sizeof(long long))))
    return fail(rc);
  hipLaunchKernelGGL(pm_row_len_kernel, dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, perm, rowptr, b_rowptr);
  scan_counts_i32(s, m, b_rowptr, partials);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(hip_fail(e));
  if (nnz > 0) {
    const size_t nb = (size_t) nnz * 4;
    if ((rc = dev_alloc((void**) &pl->map, nb, s)) || (rc = temps.alloc(&c_col, nb)) || (rc = temps.alloc(&c_pos, nb)) ||
        (rc = temps.alloc(&d_col, nb)) || (rc = temps.alloc(&d_pos, nb)) || (rc = temps.alloc(&d_rowptr, (size_t) (m + 1) * 4)))
      return fail(rc);
    hipLaunchKernelGGL(pm_fill_kernel, dim3((unsigned) cdiv(m, 32)), dim3(256), 0, s, m, perm, inv, rowptr, colind, b_rowptr,
                       c_col, c_pos);
    if ((e = hipGetLastError()) != hipSuccess)
      return fail(hip_fail(e));
    // by column, then by row again: ascending columns inside every row, equal columns in source order.  The positions ride as
    // the 4-byte values, which the transpose only moves.
    if ((rc = spblas_gfx950_csr_transpose(handle, m, m, nnz, b_rowptr, c_col, c_pos, d_rowptr, d_col, d_pos, SPBLAS_GFX950_F32)) ||
        (rc = spblas_gfx950_csr_transpose(handle, m, m, nnz, d_rowptr, d_col, d_pos, b_rowptr, b_colind, pl->map,
                                          SPBLAS_GFX950_F32)))
      return fail(rc);
  }
  if ((e = hipStreamSynchronize(s)) != hipSuccess)
    return fail(hip_fail(e));
  *plan_out = pl;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_csr_permute_values(spblas_gfx950_handle_t handle, spblas_gfx950_permute_t plan, int64_t nnz,
                                     const void* a_values, void* b_values, int value_type) {
  if (is_complex_type(value_type) || is_lowp_type(value_type))  // complex / 16-bit values: SpMV / SpMM only
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan || (nnz > 0 && (!a_values || !b_values)))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (nnz != plan->nnz)
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  if (value_type != SPBLAS_GFX950_F32 && value_type != SPBLAS_GFX950_F64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (nnz > 0 && a_values == b_values)  // a gather: no in-place form
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (nnz == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  note_use(plan->use, handle->stream);
  const dim3 grid(stride_grid(handle, nnz)), block(256);
  if (value_type == SPBLAS_GFX950_F32)
    hipLaunchKernelGGL(pm_gather_kernel<uint32_t>, grid, block, 0, handle->stream, nnz, plan->map,
                       static_cast<const uint32_t*>(a_values), static_cast<uint32_t*>(b_values));
  else
    hipLaunchKernelGGL(pm_gather_kernel<uint64_t>, grid, block, 0, handle->stream, nnz, plan->map,
                       static_cast<const uint64_t*>(a_values), static_cast<uint64_t*>(b_values));
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_permute_vector(spblas_gfx950_handle_t handle, int64_t n, const int32_t* perm, const void* src, void* dst,
                                 int value_type, int inverse) {
  if (is_complex_type(value_type) || is_lowp_type(value_type))  // complex / 16-bit values: SpMV / SpMM only
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (n < 0 || n >= INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if (n > 0 && (!perm || !src || !dst))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (value_type != SPBLAS_GFX950_F32 && value_type != SPBLAS_GFX950_F64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (n > 0 && src == dst)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (n == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  const dim3 grid(stride_grid(handle, n)), block(256);
  hipStream_t s = handle->stream;
  if (value_type == SPBLAS_GFX950_F32) {
    const uint32_t* x = static_cast<const uint32_t*>(src);
    uint32_t* y = static_cast<uint32_t*>(dst);
    if (inverse)
      hipLaunchKernelGGL(pm_scatter_kernel<uint32_t>, grid, block, 0, s, n, perm, x, y);
    else
      hipLaunchKernelGGL(pm_gather_kernel<uint32_t>, grid, block, 0, s, n, perm, x, y);
  } else {
    const uint64_t* x = static_cast<const uint64_t*>(src);
    uint64_t* y = static_cast<uint64_t*>(dst);
    if (inverse)
      hipLaunchKernelGGL(pm_scatter_kernel<uint64_t>, grid, block, 0, s, n, perm, x, y);
    else
      hipLaunchKernelGGL(pm_gather_kernel<uint64_t>, grid, block, 0, s, n, perm, x, y);
  }
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

} // extern "C"

// Loads this file's code object at handle creation (handle.hip), as the other files do.
namespace spb {
void preload_multicolor() {
  hipFuncAttributes attr;
  (void) hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&mc_round_kernel<4>));
  (void) hipGetLastError();
}
} // namespace spb
