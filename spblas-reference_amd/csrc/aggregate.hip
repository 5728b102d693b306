// MIS-2 aggregation of a square CSR matrix and the Galerkin coarse matrix A_c = P^T A P of an aggregation, on gfx950 (no
// reference counterpart).  Together with transpose / SpGEMM / gauss_seidel these are the pieces of an aggregation-based AMG.
//
// aggregate_create
//   strength   in the value type T:  d_i = the first stored diagonal entry of row i (0 if none);  t2 = T(theta * theta) (the
//              product in double);  a stored (i, j), j != i, is STRONG iff  a_ij * a_ij >= (t2 * |d_i|) * |d_j|  -- products only,
//              in this order, so a host model restates it bit for bit; a NaN on either side compares false: weak.
//   graph      u ~ v iff (u, v) or (v, u) is a strong entry.  The pattern of A^T comes from spblas_gfx950_csr_transpose with the
//              source position of every entry as its 4-byte payload: a transposed entry looks its strength flag up there.
//   roots      a maximal independent set at distance 2 (Bell, Dalton, Olson 2012), priorities key(v) = mc_key(v) (mc_key.hpp).
//              state[v]: 0 undecided, 1 root, 2 covered.  One round = four launches on ping-pong arrays; no launch reads what it
//              writes:
//                t1     T1[v] = max key of an UNDECIDED vertex in {v} + N(v), 0 if none -- at EVERY vertex
//                t2     T2[v] = max T1 over {v} + N(v); an undecided v with T2[v] == key(v) becomes a root   (state A -> B)
//                near   near[v] = a root in {v} + N(v)                                                        (reads B)
//                cover  an undecided v with near[] set in {v} + N(v) becomes covered                          (state B -> A)
//              (T2 is only needed where the root decision is taken, so t2 writes the decision instead of T2; near / cover look at
//              every root, old or new: whatever lies within distance 2 of an old root was covered when it became one.)
//              The undecided vertex of the largest key becomes a root in every round, so the rounds end.  The host reads the count
//              of decided vertices after every round.
//   determinism the roots are greedy MIS on G^2 in descending key order: v becomes a root exactly when it is undecided and holds
//              the largest key among the undecided vertices within distance 2, and it is covered exactly when a vertex within
//              distance 2 became a root.  Each launch reads only what earlier launches wrote, so the roots AND the number of rounds
//              depend on the pattern, the values and theta alone -- not on the schedule or the lanes per row.
//   aggregates roots numbered in ascending vertex index (scan.hpp).  Phase 1: a root takes its id, a neighbour of a root that
//              root's id (two roots are >= 3 apart: it is unique).  Phase 2, a launch of its own that reads phase 1 only: every
//              other vertex takes the aggregate of its phase-1 neighbour of the largest key (one exists, by maximality).
//   row work   a TEAM of G = lanes_per_row(m, nnz) lanes of one wavefront owns a vertex; the 64-bit maxima are reduced over the
//              team by shuffles.  Nothing is sized by the degree.
//
// coarsen_create  entry p of A is renamed (agg[row], agg[col]).  Two passes of the stable transpose bring the entries into
//   (I, J, p) order: the first, over the m x n_agg matrix (row, agg[col]), orders by J and keeps (row, p) order inside; then the
//   fine rows are renamed I = agg[row] and the second pass orders by I and keeps (J, p) order inside.  The source position rides
//   as the payload (as in csr_permute_create).  Runs of equal (I, J) collapse: head flags, one scan, seg_ptr / c_colind / c_rowptr.
// coarsen_values  c[e] = a[map[seg_ptr[e]]] + a[map[seg_ptr[e] + 1]] + ... in ascending sorted position = ascending source
//   position, plain additions in T from the first term: the bits depend on A and agg alone.  One launch.
#include "aggregate_kernels.hpp"
#include "common.hpp"
#include "complex_api.hpp"
#include "csr_inspect.hpp"
#include "lowp_api.hpp"
#include "mc_key.hpp"
#include "scan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>

struct spblas_gfx950_aggregate_s {
  int64_t m = 0, nnz = 0;
  int64_t n_agg = 0, rounds = 0, largest = 0, smallest = 0, singletons = 0, strong = 0;
  int lanes = 4;
  int32_t* agg = nullptr;   // [m] aggregate of every vertex
  int32_t* root = nullptr;  // [n_agg] root vertex of every aggregate, ascending
  spb::use_record use;      // the stream of the last copy / prolongator out of the plan: destroy frees behind it
};

struct spblas_gfx950_coarsen_s {
  int64_t m = 0, nnz = 0, n_agg = 0, c_nnz = 0;
  int32_t* c_rowptr = nullptr;  // [n_agg + 1]
  int32_t* c_colind = nullptr;  // [c_nnz] ascending, duplicate free
  int32_t* seg_ptr = nullptr;   // [c_nnz + 1] first sorted position of every coarse entry
  int32_t* map = nullptr;       // [nnz] position in A's arrays of every sorted position
  spb::use_record use;          // the stream of the last structure copy / value pass: destroy frees behind it
};

namespace spb {

struct ag_graph {
  const int32_t *rowptr, *colind;               // A
  const int32_t *t_rowptr, *t_colind, *t_pos;   // the pattern of A^T; t_pos[q] = position in A of transposed entry q
  const uint8_t* strong;                        // [nnz] 1 = strong entry of A (never set on a diagonal entry)
  int m;
};

// f(u) for lane t's share of the neighbours of v: the strong entries of row v of A and of row v of A^T (a neighbour may come
// twice; every use below is a maximum or an OR, so repeats count once)
template <int G, typename F>
__device__ __forceinline__ void ag_neighbours(const ag_graph& g, int v, int t, F&& f) {
  for (int p = g.rowptr[v] + t, p1 = g.rowptr[v + 1]; p < p1; p += G)
    if (g.strong[p])
      f(g.colind[p]);
  for (int q = g.t_rowptr[v] + t, q1 = g.t_rowptr[v + 1]; q < q1; q += G)
    if (g.strong[g.t_pos[q]])
      f(g.t_colind[q]);
}

// counter += the lanes of this wavefront with `one` set; every lane of the wavefront calls it
__device__ __forceinline__ void ag_count(unsigned* counter, bool one) {
  const unsigned long long b = __ballot(one);
  if ((threadIdx.x & 63) == 0 && b != 0ull)
    atomicAdd(counter, (unsigned) __popcll(b));
}

// strong[p] of every entry of A; counters[5] += the strong ones
template <typename T, int G>
__global__ __launch_bounds__(AG_THREADS) void ag_strength_kernel(int m, const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ colind,
                                                                 const T* __restrict__ values, const T* __restrict__ d, T t2,
                                                                 uint8_t* __restrict__ strong, unsigned* __restrict__ counters) {
  const int t = (int) threadIdx.x % G, v = ag_vertex<G>(m);
  unsigned n = 0;
  if (v >= 0) {
    const T lhs_d = t2 * ag_abs(d[v]);
    for (int p = rowptr[v] + t, p1 = rowptr[v + 1]; p < p1; p += G) {
      const int j = colind[p];
      const T a = values[p];
      const bool s = ag_is_strong(a, lhs_d, d[j], j, v);
      strong[p] = s ? 1 : 0;
      n += s ? 1u : 0u;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    n += __shfl_xor(n, o, SPB_WAVE);
  if ((threadIdx.x & 63) == 0 && n != 0u)
    atomicAdd(counters + 5, n);
}

template <int G>
__global__ __launch_bounds__(AG_THREADS) void ag_t1_kernel(ag_graph g, const int32_t* __restrict__ state,
                                                           uint64_t* __restrict__ T1) {
  const int t = (int) threadIdx.x % G, v = ag_vertex<G>(g.m);
  if (v < 0)
    return;
  uint64_t best = (t == 0 && state[v] == 0) ? mc_key(v) : 0ull;
  ag_neighbours<G>(g, v, t, [&](int u) {
    if (state[u] == 0) {
      const uint64_t k = mc_key(u);
      best = k > best ? k : best;
    }
  });
  best = ag_team_max<G>(best);
  if (t == 0)
    T1[v] = best;
}

// an undecided v whose key is the largest T1 in {v} + N(v) becomes a root; every other state is copied
template <int G>
__global__ __launch_bounds__(AG_THREADS) void ag_t2_kernel(ag_graph g, const int32_t* __restrict__ state_in,
                                                           const uint64_t* __restrict__ T1, int32_t* __restrict__ state_out,
                                                           unsigned* __restrict__ counters) {
  const int t = (int) threadIdx.x % G, v = ag_vertex<G>(g.m);
  bool fresh = false;
  if (v >= 0) {
    const int s = state_in[v];
    int out = s;
    if (s == 0) {
      uint64_t best = t == 0 ? T1[v] : 0ull;
      ag_neighbours<G>(g, v, t, [&](int u) {
        const uint64_t k = T1[u];
        best = k > best ? k : best;
      });
      best = ag_team_max<G>(best);
      if (best == mc_key(v))
        out = 1;
    }
    if (t == 0) {
      state_out[v] = out;
      fresh = out != s;
    }
  }
  ag_count(counters, fresh);
}

template <int G>
__global__ __launch_bounds__(AG_THREADS) void ag_near_kernel(ag_graph g, const int32_t* __restrict__ state,
                                                             int32_t* __restrict__ near) {
  const int t = (int) threadIdx.x % G, v = ag_vertex<G>(g.m);
  if (v < 0)
    return;
  int hit = (t == 0 && state[v] == 1) ? 1 : 0;
  ag_neighbours<G>(g, v, t, [&](int u) { hit |= state[u] == 1 ? 1 : 0; });
  hit = ag_team_max<G>(hit);
  if (t == 0)
    near[v] = hit;
}

template <int G>
__global__ __launch_bounds__(AG_THREADS) void ag_cover_kernel(ag_graph g, const int32_t* __restrict__ state_in,
                                                              const int32_t* __restrict__ near, int32_t* __restrict__ state_out,
                                                              unsigned* __restrict__ counters) {
  const int t = (int) threadIdx.x % G, v = ag_vertex<G>(g.m);
  bool fresh = false;
  if (v >= 0) {
    const int s = state_in[v];
    int out = s;
    if (s == 0) {
      int hit = t == 0 ? near[v] : 0;
      ag_neighbours<G>(g, v, t, [&](int u) { hit |= near[u]; });
      hit = ag_team_max<G>(hit);
      if (hit)
        out = 2;
    }
    if (t == 0) {
      state_out[v] = out;
      fresh = out != s;
    }
  }
  ag_count(counters, fresh);
}

// ids[v] = 1 on a root (the scan turns it into the root's rank); ids has m + 1 entries
__global__ __launch_bounds__(256) void ag_root_flag_kernel(int64_t m, const int32_t* __restrict__ state, int32_t* __restrict__ ids) {
  const int64_t v = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (v < m)
    ids[v] = state[v] == 1 ? 1 : 0;
}

__global__ __launch_bounds__(256) void ag_roots_kernel(int64_t m, const int32_t* __restrict__ state,
                                                       const int32_t* __restrict__ ids, int32_t* __restrict__ root) {
  const int64_t v = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (v < m && state[v] == 1)
    root[ids[v]] = (int32_t) v;
}

// phase 1: a root takes its id, a neighbour of a root that root's id, every other vertex -1
template <int G>
__global__ __launch_bounds__(AG_THREADS) void ag_phase1_kernel(ag_graph g, const int32_t* __restrict__ state,
                                                               const int32_t* __restrict__ ids, int32_t* __restrict__ agg1) {
  const int t = (int) threadIdx.x % G, v = ag_vertex<G>(g.m);
  if (v < 0)
    return;
  int id = -1;
  if (state[v] == 1) {
    id = ids[v];
  } else {
    ag_neighbours<G>(g, v, t, [&](int u) {
      if (state[u] == 1)
        id = max(id, ids[u]);
    });
    id = ag_team_max<G>(id);
  }
  if (t == 0)
    agg1[v] = id;
}

// phase 2 reads phase 1 only: the aggregate of the phase-1 neighbour of the largest key; counters[1] += vertices left without one
template <int G>
__global__ __launch_bounds__(AG_THREADS) void ag_phase2_kernel(ag_graph g, const int32_t* __restrict__ agg1,
                                                               int32_t* __restrict__ agg, unsigned* __restrict__ counters) {
  const int t = (int) threadIdx.x % G, v = ag_vertex<G>(g.m);
  bool lost = false;
  if (v >= 0) {
    int id = agg1[v];
    if (id < 0) {
      uint64_t best = 0ull;
      ag_neighbours<G>(g, v, t, [&](int u) {
        if (agg1[u] >= 0) {
          const uint64_t k = mc_key(u);
          best = k > best ? k : best;
        }
      });
      best = ag_team_max<G>(best);
      if (best != 0ull)
        id = agg1[(int) (uint32_t) best];  // the low word of a key is its vertex
    }
    if (t == 0) {
      agg[v] = id;
      lost = id < 0;
    }
  }
  ag_count(counters + 1, lost);
}

__global__ __launch_bounds__(256) void ag_hist_kernel(int64_t m, const int32_t* __restrict__ agg, int32_t* __restrict__ size) {
  const int64_t v = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (v < m && agg[v] >= 0)
    atomicAdd(size + agg[v], 1);
}

// counters[2] = largest aggregate, [3] = smallest (arrives as 0xFFFFFFFF), [4] = aggregates of one vertex
__global__ __launch_bounds__(256) void ag_stats_kernel(int64_t n, const int32_t* __restrict__ size, unsigned* __restrict__ counters) {
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  unsigned hi = 0u, lo = 0xFFFFFFFFu;
  if (i < n)
    hi = lo = (unsigned) size[i];
  ag_count(counters + 4, i < n && hi == 1u);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hi = max(hi, (unsigned) __shfl_xor(hi, o, SPB_WAVE));
    lo = min(lo, (unsigned) __shfl_xor(lo, o, SPB_WAVE));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(counters + 2, hi);
    atomicMin(counters + 3, lo);
  }
}

__global__ __launch_bounds__(256) void ag_iota_kernel(int64_t n, int32_t* __restrict__ out) {
  for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t) gridDim.x * 256)
    out[i] = (int32_t) i;
}

// the tentative prolongator: row offsets 0 .. m, columns agg, values 1
template <typename T>
__global__ __launch_bounds__(256) void ag_prolongator_kernel(int64_t m, const int32_t* __restrict__ agg,
                                                             int32_t* __restrict__ p_rowptr, int32_t* __restrict__ p_colind,
                                                             T* __restrict__ p_values) {
  for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i <= m; i += (int64_t) gridDim.x * 256) {
    p_rowptr[i] = (int32_t) i;
    if (i < m) {
      p_colind[i] = agg[i];
      p_values[i] = T(1);
    }
  }
}

// ---- coarsen
// out[p] = agg[in[p]]; pos[p] = p when given
__global__ __launch_bounds__(256) void cz_rename_kernel(int64_t nnz, const int32_t* __restrict__ agg, const int32_t* __restrict__ in,
                                                        int32_t* __restrict__ out, int32_t* __restrict__ pos) {
  for (int64_t p = (int64_t) blockIdx.x * 256 + threadIdx.x; p < nnz; p += (int64_t) gridDim.x * 256) {
    out[p] = agg[in[p]];
    if (pos)
      pos[p] = (int32_t) p;
  }
}

// c[e] = the terms of coarse entry e added one after the other in ascending sorted position, from the first term
template <typename T>
__global__ __launch_bounds__(256) void cz_values_kernel(int64_t c_nnz, const int32_t* __restrict__ seg_ptr,
                                                        const int32_t* __restrict__ map, const T* __restrict__ a,
                                                        T* __restrict__ c) {
  const int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (e >= c_nnz)
    return;
  const int q0 = seg_ptr[e], q1 = seg_ptr[e + 1];
  T s = a[map[q0]];
  for (int q = q0 + 1; q < q1; ++q)
    s = s + a[map[q]];
  c[e] = s;
}

template <typename T>
static int aggregate_run(spblas_gfx950_handle_s* handle, spblas_gfx950_aggregate_s* pl, dev_temps& temps, const int32_t* rowptr,
                         const int32_t* colind, const T* values, double theta) {
  const int64_t m = pl->m, nnz = pl->nnz;
  hipStream_t s = handle->stream;
  int32_t *flag = nullptr, *t_rowptr = nullptr, *t_colind = nullptr, *t_pos = nullptr, *pos = nullptr, *state_a = nullptr,
          *state_b = nullptr, *near = nullptr, *ids = nullptr, *agg1 = nullptr, *size = nullptr;
  uint8_t* strong = nullptr;
  uint64_t* T1 = nullptr;
  T* d = nullptr;
  unsigned* counters = nullptr;
  long long* partials = nullptr;
  int rc;
  hipError_t e;
  if ((rc = temps.alloc(&flag, 16)) || (rc = temps.alloc(&counters, 32)) ||
      (rc = dev_alloc((void**) &pl->agg, (size_t) m * 4, s)))
    return rc;
  if ((e = hipMemsetAsync(flag, 0, 16, s)) != hipSuccess || (e = hipMemsetAsync(counters, 0, 32, s)) != hipSuccess ||
      (e = hipMemsetAsync(counters + 3, 0xFF, 4, s)) != hipSuccess)
    return hip_fail(e);
  // the structure is checked, with a synchronisation of its own, BEFORE anything indexes with it
  if ((rc = check_csr_structure(handle, m, nnz, rowptr, colind, flag)))
    return rc;
  const size_t mb = (size_t) m * 4, nb = (size_t) nnz * 4;
  if ((rc = temps.alloc(&t_rowptr, mb + 4)) || (rc = temps.alloc(&t_colind, nb)) || (rc = temps.alloc(&t_pos, nb)) ||
      (rc = temps.alloc(&pos, nb)) || (rc = temps.alloc(&strong, (size_t) nnz)) || (rc = temps.alloc(&d, (size_t) m * sizeof(T))) ||
      (rc = temps.alloc(&state_a, mb)) || (rc = temps.alloc(&state_b, mb)) || (rc = temps.alloc(&near, mb)) ||
      (rc = temps.alloc(&T1, (size_t) m * 8)) || (rc = temps.alloc(&ids, mb + 4)) || (rc = temps.alloc(&agg1, mb)) ||
      (rc = temps.alloc(&partials, (size_t) (cdiv(m, 2048) + 2) * sizeof(long long))))
    return rc;
  // the pattern of A^T with the source positions as the 4-byte payload the transpose only moves
  if (nnz > 0)
    hipLaunchKernelGGL(ag_iota_kernel, dim3(stride_grid(handle, nnz)), dim3(256), 0, s, nnz, pos);
  if ((e = hipGetLastError()) != hipSuccess)
    return hip_fail(e);
  if ((rc = spblas_gfx950_csr_transpose(handle, m, m, nnz, rowptr, colind, pos, t_rowptr, t_colind, t_pos, SPBLAS_GFX950_F32)))
    return rc;
  if ((e = hipMemsetAsync(state_a, 0, mb, s)) != hipSuccess)
    return hip_fail(e);
  const T t2 = (T) (theta * theta);
  ag_graph g;
  g.rowptr = rowptr;
  g.colind = colind;
  g.t_rowptr = t_rowptr;
  g.t_colind = t_colind;
  g.t_pos = t_pos;
  g.strong = strong;
  g.m = (int) m;
  const int lanes = pl->lanes;
  auto grid_of = [&](int G) { return dim3((unsigned) cdiv(m, AG_THREADS / G)); };
  const dim3 block(AG_THREADS);
  with_lanes(lanes, [&](auto gc) {
    constexpr int G = decltype(gc)::value;
    hipLaunchKernelGGL((ag_diag_kernel<T, G>), grid_of(G), block, 0, s, (int) m, rowptr, colind, values, d);
    hipLaunchKernelGGL((ag_strength_kernel<T, G>), grid_of(G), block, 0, s, (int) m, rowptr, colind, values, (const T*) d, t2,
                       strong, counters);
  });
  if ((e = hipGetLastError()) != hipSuccess)
    return hip_fail(e);
  unsigned h_cnt[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  int32_t h_roots = 0;
  {
    readback_scope rb(handle);
    while ((int64_t) h_cnt[0] < m) {
      const unsigned before = h_cnt[0];
      with_lanes(lanes, [&](auto gc) {
        constexpr int G = decltype(gc)::value;
        hipLaunchKernelGGL(ag_t1_kernel<G>, grid_of(G), block, 0, s, g, (const int32_t*) state_a, T1);
        hipLaunchKernelGGL(ag_t2_kernel<G>, grid_of(G), block, 0, s, g, (const int32_t*) state_a, (const uint64_t*) T1, state_b,
                           counters);
        hipLaunchKernelGGL(ag_near_kernel<G>, grid_of(G), block, 0, s, g, (const int32_t*) state_b, near);
        hipLaunchKernelGGL(ag_cover_kernel<G>, grid_of(G), block, 0, s, g, (const int32_t*) state_b, (const int32_t*) near,
                           state_a, counters);
      });
      if ((e = hipGetLastError()) != hipSuccess)
        return hip_fail(e);
      if ((rc = readback_add(handle, h_cnt, counters, 4)) || (rc = readback_flush(handle)))
        return rc;
      ++pl->rounds;
      if (h_cnt[0] == before || pl->rounds > m)  // cannot happen: the undecided vertex of the largest key becomes a root
        return SPBLAS_GFX950_STATUS_HIP_ERROR;
    }
    // the roots numbered in ascending vertex index
    hipLaunchKernelGGL(ag_root_flag_kernel, dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, (const int32_t*) state_a, ids);
    scan_counts_i32(s, m, ids, partials);
    if ((e = hipGetLastError()) != hipSuccess)
      return hip_fail(e);
    if ((rc = readback_add(handle, &h_roots, ids + m, 4)) || (rc = readback_flush(handle)))
      return rc;
    pl->n_agg = h_roots;
    if (pl->n_agg <= 0 || pl->n_agg > m)
      return SPBLAS_GFX950_STATUS_HIP_ERROR;
    if ((rc = dev_alloc((void**) &pl->root, (size_t) pl->n_agg * 4, s)) || (rc = temps.alloc(&size, (size_t) pl->n_agg * 4)))
      return rc;
    if ((e = hipMemsetAsync(size, 0, (size_t) pl->n_agg * 4, s)) != hipSuccess)
      return hip_fail(e);
    hipLaunchKernelGGL(ag_roots_kernel, dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, (const int32_t*) state_a,
                       (const int32_t*) ids, pl->root);
    with_lanes(lanes, [&](auto gc) {
      constexpr int G = decltype(gc)::value;
      hipLaunchKernelGGL(ag_phase1_kernel<G>, grid_of(G), block, 0, s, g, (const int32_t*) state_a, (const int32_t*) ids, agg1);
      hipLaunchKernelGGL(ag_phase2_kernel<G>, grid_of(G), block, 0, s, g, (const int32_t*) agg1, pl->agg, counters);
    });
    hipLaunchKernelGGL(ag_hist_kernel, dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, (const int32_t*) pl->agg, size);
    hipLaunchKernelGGL(ag_stats_kernel, dim3((unsigned) cdiv(pl->n_agg, 256)), dim3(256), 0, s, pl->n_agg, (const int32_t*) size,
                       counters);
    if ((e = hipGetLastError()) != hipSuccess)
      return hip_fail(e);
    if ((rc = readback_add(handle, h_cnt, counters, 32)) || (rc = readback_flush(handle)))
      return rc;
  }
  if (h_cnt[1] != 0u)  // cannot happen: a covered vertex has a phase-1 neighbour
    return SPBLAS_GFX950_STATUS_HIP_ERROR;
  pl->largest = h_cnt[2];
  pl->smallest = h_cnt[3];
  pl->singletons = h_cnt[4];
  pl->strong = h_cnt[5];
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

} // namespace spb

using namespace spb;

extern "C" {

int spblas_gfx950_aggregate_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_aggregate_t plan) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  order_behind_last_use(plan->use, handle->stream);
  dev_free(plan->agg, handle->stream);
  dev_free(plan->root, handle->stream);
  delete plan;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_aggregate_create(spblas_gfx950_handle_t handle, spblas_gfx950_aggregate_t* plan_out, int64_t m, int64_t nnz,
                                   const int32_t* rowptr, const int32_t* colind, const void* values, double theta,
                                   int value_type) {
  if (is_complex_type(value_type) || is_lowp_type(value_type))  // complex / 16-bit values: SpMV / SpMM only
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (const int st = inspect_args_status(handle, plan_out && rowptr && (nnz <= 0 || (colind && values)), m, nnz))
    return st;
  *plan_out = nullptr;
  if (m == 0 && nnz != 0)  // no offsets of an empty matrix describe entries
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (value_type != SPBLAS_GFX950_F32 && value_type != SPBLAS_GFX950_F64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (!std::isfinite(theta) || theta < 0.0)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  auto* pl = new (std::nothrow) spblas_gfx950_aggregate_s();
  if (!pl)
    return SPBLAS_GFX950_STATUS_ALLOC_FAILED;
  pl->m = m;
  pl->nnz = nnz;
  pl->lanes = lanes_per_row(m, nnz);
  if (m == 0) {
    *plan_out = pl;
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  int rc;
  {
    dev_temps temps(handle->stream);
    rc = value_type == SPBLAS_GFX950_F32
             ? aggregate_run<float>(handle, pl, temps, rowptr, colind, static_cast<const float*>(values), theta)
             : aggregate_run<double>(handle, pl, temps, rowptr, colind, static_cast<const double*>(values), theta);
    if (rc != SPBLAS_GFX950_STATUS_SUCCESS)
      (void) hipStreamSynchronize(handle->stream);  // the kernels may still be using the temporaries
  }
  if (rc != SPBLAS_GFX950_STATUS_SUCCESS) {
    (void) spblas_gfx950_aggregate_destroy(handle, pl);
    return rc;
  }
  *plan_out = pl;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_aggregate_info(spblas_gfx950_aggregate_t plan, int64_t info[8]) {
  if (!plan || !info)
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  info[0] = plan->n_agg;
  info[1] = plan->rounds;
  info[2] = plan->largest;     // vertices of the largest aggregate
  info[3] = plan->smallest;    // ... of the smallest
  info[4] = plan->singletons;  // aggregates of one vertex
  info[5] = plan->strong;      // strong stored entries of A
  info[6] = plan->lanes;       // lanes per row
  info[7] = plan->m;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_aggregate_copy(spblas_gfx950_handle_t handle, spblas_gfx950_aggregate_t plan, int32_t* agg, int32_t* root) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan)
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  hipStream_t s = handle->stream;
  note_use(plan->use, s);
  if (agg && plan->m > 0)
    SPB_HIP(hipMemcpyAsync(agg, plan->agg, (size_t) plan->m * 4, hipMemcpyDeviceToDevice, s));
  if (root && plan->n_agg > 0)
    SPB_HIP(hipMemcpyAsync(root, plan->root, (size_t) plan->n_agg * 4, hipMemcpyDeviceToDevice, s));
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_aggregate_prolongator(spblas_gfx950_handle_t handle, spblas_gfx950_aggregate_t plan, int64_t m,
                                        int32_t* p_rowptr, int32_t* p_colind, void* p_values, int value_type) {
  if (is_complex_type(value_type) || is_lowp_type(value_type))  // complex / 16-bit values: SpMV / SpMM only
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan || !p_rowptr || (m > 0 && (!p_colind || !p_values)))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (m != plan->m)
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  if (value_type != SPBLAS_GFX950_F32 && value_type != SPBLAS_GFX950_F64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  hipStream_t s = handle->stream;
  note_use(plan->use, s);
  const dim3 grid(stride_grid(handle, m + 1)), block(256);
  if (value_type == SPBLAS_GFX950_F32)
    hipLaunchKernelGGL(ag_prolongator_kernel<float>, grid, block, 0, s, m, (const int32_t*) plan->agg, p_rowptr, p_colind,
                       static_cast<float*>(p_values));
  else
    hipLaunchKernelGGL(ag_prolongator_kernel<double>, grid, block, 0, s, m, (const int32_t*) plan->agg, p_rowptr, p_colind,
                       static_cast<double*>(p_values));
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_coarsen_destroy(spblas_gfx950_handle_t handle, spblas_gfx950_coarsen_t plan) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  order_behind_last_use(plan->use, handle->stream);
  dev_free(plan->c_rowptr, handle->stream);
  dev_free(plan->c_colind, handle->stream);
  dev_free(plan->seg_ptr, handle->stream);
  dev_free(plan->map, handle->stream);
  delete plan;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_coarsen_create(spblas_gfx950_handle_t handle, spblas_gfx950_coarsen_t* plan_out, int64_t m, int64_t nnz,
                                 const int32_t* rowptr, const int32_t* colind, const int32_t* agg, int64_t n_agg) {
  if (const int st = inspect_args_status(handle, plan_out && rowptr && (nnz <= 0 || colind) && (m <= 0 || agg), m, nnz))
    return st;
  *plan_out = nullptr;
  if (n_agg < 0 || n_agg >= INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if ((m == 0 && nnz != 0) || (m > 0 && n_agg == 0))  // no aggregate could hold a row
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  auto* pl = new (std::nothrow) spblas_gfx950_coarsen_s();
  if (!pl)
    return SPBLAS_GFX950_STATUS_ALLOC_FAILED;
  pl->m = m;
  pl->nnz = nnz;
  pl->n_agg = n_agg;
  hipStream_t s = handle->stream;
  dev_temps temps(s);
  int32_t *flag = nullptr, *c_col = nullptr, *c_pos = nullptr, *r_rowptr = nullptr, *r_col = nullptr, *r_pos = nullptr,
          *s_rowptr = nullptr, *s_col = nullptr, *head = nullptr;
  long long* partials = nullptr;
  auto fail = [&](int code) {
    (void) hipStreamSynchronize(s);
    (void) spblas_gfx950_coarsen_destroy(handle, pl);
    return code;
  };
  int rc;
  hipError_t e;
  const size_t cb = (size_t) (n_agg + 1) * 4, nb = (size_t) nnz * 4;
  if ((rc = dev_alloc((void**) &pl->c_rowptr, cb, s)))
    return fail(rc);
  if ((e = hipMemsetAsync(pl->c_rowptr, 0, cb, s)) != hipSuccess)
    return fail(hip_fail(e));
  if (m > 0) {
    if ((rc = temps.alloc(&flag, 16)))
      return fail(rc);
    if ((e = hipMemsetAsync(flag, 0, 16, s)) != hipSuccess)
      return fail(hip_fail(e));
    // agg and the structure are checked, with a synchronisation, BEFORE anything indexes with them
    hipLaunchKernelGGL(cz_check_agg_kernel, dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, agg, n_agg, flag);
    if ((rc = check_csr_structure(handle, m, nnz, rowptr, colind, flag)))
      return fail(rc);
  }
  if (nnz == 0) {
    if ((rc = dev_alloc((void**) &pl->seg_ptr, 4, s)))
      return fail(rc);
    if ((e = hipMemsetAsync(pl->seg_ptr, 0, 4, s)) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess)
      return fail(hip_fail(e));
    *plan_out = pl;
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  if ((rc = dev_alloc((void**) &pl->map, nb, s)) || (rc = temps.alloc(&c_col, nb)) || (rc = temps.alloc(&c_pos, nb)) ||
      (rc = temps.alloc(&r_rowptr, cb)) || (rc = temps.alloc(&r_col, nb)) || (rc = temps.alloc(&r_pos, nb)) ||
      (rc = temps.alloc(&s_rowptr, cb)) || (rc = temps.alloc(&s_col, nb)) || (rc = temps.alloc(&head, nb + 4)) ||
      (rc = temps.alloc(&partials, (size_t) (cdiv(nnz, 2048) + 2) * sizeof(long long))))
    return fail(rc);
  const dim3 ngrid(stride_grid(handle, nnz)), block(256);
  // pass 1 over the m x n_agg matrix (row, agg[col]): by coarse column, (row, position) order kept inside
  hipLaunchKernelGGL(cz_rename_kernel, ngrid, block, 0, s, nnz, agg, colind, c_col, c_pos);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(hip_fail(e));
  if ((rc = spblas_gfx950_csr_transpose(handle, m, n_agg, nnz, rowptr, c_col, c_pos, r_rowptr, r_col, r_pos, SPBLAS_GFX950_F32)))
    return fail(rc);
  // pass 2 over the n_agg x n_agg matrix (agg[col], agg[row]): by coarse row, (coarse column, position) order kept inside
  hipLaunchKernelGGL(cz_rename_kernel, ngrid, block, 0, s, nnz, agg, (const int32_t*) r_col, c_col, (int32_t*) nullptr);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(hip_fail(e));
  if ((rc = spblas_gfx950_csr_transpose(handle, n_agg, n_agg, nnz, r_rowptr, c_col, r_pos, s_rowptr, s_col, pl->map,
                                        SPBLAS_GFX950_F32)))
    return fail(rc);
  // runs of equal (I, J) collapse: head flags, their exclusive scan, the entry tables
  if ((e = hipMemsetAsync(head, 0, nb + 4, s)) != hipSuccess)
    return fail(hip_fail(e));
  hipLaunchKernelGGL(cz_row_start_kernel, dim3((unsigned) cdiv(n_agg, 256)), block, 0, s, n_agg, (const int32_t*) s_rowptr, head);
  hipLaunchKernelGGL(cz_heads_kernel, ngrid, block, 0, s, nnz, (const int32_t*) s_col, head);
  scan_counts_i32(s, nnz, head, partials);
  if ((e = hipGetLastError()) != hipSuccess)
    return fail(hip_fail(e));
  int32_t h_cnnz = 0;
  {
    readback_scope rb(handle);
    if ((rc = readback_add(handle, &h_cnnz, head + nnz, 4)) || (rc = readback_flush(handle)))
      return fail(rc);
  }
  pl->c_nnz = h_cnnz;
  if (pl->c_nnz <= 0 || pl->c_nnz > nnz)  // cannot happen: nnz > 0 entries head at least one run
    return fail(SPBLAS_GFX950_STATUS_HIP_ERROR);
  if ((rc = dev_alloc((void**) &pl->c_colind, (size_t) pl->c_nnz * 4, s)) ||
      (rc = dev_alloc((void**) &pl->seg_ptr, (size_t) (pl->c_nnz + 1) * 4, s)))
    return fail(rc);
  hipLaunchKernelGGL(cz_emit_kernel, ngrid, block, 0, s, nnz, (const int32_t*) head, (const int32_t*) s_col, pl->seg_ptr,
                     pl->c_colind);
  hipLaunchKernelGGL(cz_rowptr_kernel, dim3((unsigned) cdiv(n_agg + 1, 256)), block, 0, s, n_agg, (const int32_t*) s_rowptr,
                     (const int32_t*) head, pl->c_rowptr);
  if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess)
    return fail(hip_fail(e));
  *plan_out = pl;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_coarsen_info(spblas_gfx950_coarsen_t plan, int64_t info[4]) {
  if (!plan || !info)
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  info[0] = plan->n_agg;  // rows and columns of A_c
  info[1] = plan->c_nnz;  // entries of A_c
  info[2] = plan->m;
  info[3] = plan->nnz;    // terms summed by one value pass
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_coarsen_structure(spblas_gfx950_handle_t handle, spblas_gfx950_coarsen_t plan, int32_t* c_rowptr,
                                    int32_t* c_colind) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan || !c_rowptr || (plan->c_nnz > 0 && !c_colind))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  hipStream_t s = handle->stream;
  note_use(plan->use, s);
  SPB_HIP(hipMemcpyAsync(c_rowptr, plan->c_rowptr, (size_t) (plan->n_agg + 1) * 4, hipMemcpyDeviceToDevice, s));
  if (plan->c_nnz > 0)
    SPB_HIP(hipMemcpyAsync(c_colind, plan->c_colind, (size_t) plan->c_nnz * 4, hipMemcpyDeviceToDevice, s));
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int spblas_gfx950_coarsen_values(spblas_gfx950_handle_t handle, spblas_gfx950_coarsen_t plan, int64_t nnz, const void* a_values,
                                 int64_t c_nnz, void* c_values, int value_type) {
  if (is_complex_type(value_type) || is_lowp_type(value_type))  // complex / 16-bit values: SpMV / SpMM only
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (!plan || (nnz > 0 && !a_values) || (c_nnz > 0 && !c_values))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (nnz != plan->nnz || c_nnz != plan->c_nnz)
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  if (value_type != SPBLAS_GFX950_F32 && value_type != SPBLAS_GFX950_F64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (c_nnz > 0 && a_values == c_values)  // every coarse entry re-reads A: no in-place form
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (c_nnz == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  note_use(plan->use, handle->stream);
  const dim3 grid((unsigned) cdiv(c_nnz, 256)), block(256);
  if (value_type == SPBLAS_GFX950_F32)
    hipLaunchKernelGGL(cz_values_kernel<float>, grid, block, 0, handle->stream, c_nnz, (const int32_t*) plan->seg_ptr,
                       (const int32_t*) plan->map, static_cast<const float*>(a_values), static_cast<float*>(c_values));
  else
    hipLaunchKernelGGL(cz_values_kernel<double>, grid, block, 0, handle->stream, c_nnz, (const int32_t*) plan->seg_ptr,
                       (const int32_t*) plan->map, static_cast<const double*>(a_values), static_cast<double*>(c_values));
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

} // extern "C"

// Loads this file's code object at handle creation (handle.hip), as the other files do.
namespace spb {
void preload_aggregate() {
  hipFuncAttributes attr;
  (void) hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&ag_t1_kernel<4>));
  (void) hipGetLastError();
}
} // namespace spb
