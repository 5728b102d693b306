// What aggregate.hip and smooth.hip share (not part of the ABI): the team-per-row helpers, the strength rule -- the kernel for d
// (the first stored diagonal entry of a row) and the predicate ag_is_strong, each written once, so that the rule of aggregate
// and of the prolongator smoother cannot drift apart --, the check of an aggregate map and the kernels that collapse the runs
// of a sorted entry list into CSR tables.
#pragma once

#include "common.hpp"

#include <cstdint>

#define AG_THREADS 256

namespace spb {

template <int G, typename V>
__device__ __forceinline__ V ag_team_max(V x) {
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) {
    const V y = __shfl_xor(x, o, SPB_WAVE);
    x = y > x ? y : x;
  }
  return x;
}

// the vertex of a thread's team, or -1 past the end (uniform inside a team: the shuffles read active lanes only)
template <int G>
__device__ __forceinline__ int ag_vertex(int m) {
  const int64_t v = (int64_t) blockIdx.x * (AG_THREADS / G) + (int) threadIdx.x / G;
  return v < m ? (int) v : -1;
}

__device__ __forceinline__ float ag_abs(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double ag_abs(double x) { return __builtin_fabs(x); }

// The strength rule, written ONCE: entry a of row v in column j is strong iff j != v and a * a >= lhs_d * |d_j|, where
// lhs_d = t2 * |d_v| is formed by the caller once per row.  Products only, in this order; a NaN on either side compares false.
template <typename T>
__device__ __forceinline__ bool ag_is_strong(T a, T lhs_d, T dj, int j, int v) {
  return j != v && a * a >= lhs_d * ag_abs(dj);
}

// d[v] = the first stored diagonal entry of row v, 0 without one
template <typename T, int G>
__global__ __launch_bounds__(AG_THREADS) void ag_diag_kernel(int m, const int32_t* __restrict__ rowptr,
                                                             const int32_t* __restrict__ colind, const T* __restrict__ values,
                                                             T* __restrict__ d) {
  const int t = (int) threadIdx.x % G, v = ag_vertex<G>(m);
  if (v < 0)
    return;
  int first = INT32_MAX;
  for (int p = rowptr[v] + t, p1 = rowptr[v + 1]; p < p1; p += G)
    if (colind[p] == v) {
      first = p;
      break;
    }
  first = -ag_team_max<G>(-first);
  if (t == 0)
    d[v] = first != INT32_MAX ? values[first] : T(0);
}

// flag[0] = 1 when an entry of agg lies outside [0, n_agg)
static __global__ __launch_bounds__(256) void cz_check_agg_kernel(int64_t m, const int32_t* __restrict__ agg, int64_t n_agg,
                                                                  int32_t* __restrict__ flag) {
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i < m && (agg[i] < 0 || agg[i] >= n_agg))
    flag[0] = 1;
}

// head[] arrives zeroed: the first sorted position of every non-empty row of the sorted list
static __global__ __launch_bounds__(256) void cz_row_start_kernel(int64_t n_agg, const int32_t* __restrict__ s_rowptr,
                                                                  int32_t* __restrict__ head) {
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i < n_agg && s_rowptr[i] < s_rowptr[i + 1])
    head[s_rowptr[i]] = 1;
}

// ... and every position whose column differs from its predecessor's (head[q] is touched by thread q alone)
static __global__ __launch_bounds__(256) void cz_heads_kernel(int64_t nnz, const int32_t* __restrict__ s_col,
                                                              int32_t* __restrict__ head) {
  for (int64_t q = (int64_t) blockIdx.x * 256 + threadIdx.x; q < nnz; q += (int64_t) gridDim.x * 256)
    if (q > 0 && s_col[q] != s_col[q - 1])
      head[q] = 1;
}

// rank[] = the exclusive scan of the head flags (nnz + 1 entries): position q heads entry rank[q] iff rank[q + 1] != rank[q]
static __global__ __launch_bounds__(256) void cz_emit_kernel(int64_t nnz, const int32_t* __restrict__ rank,
                                                             const int32_t* __restrict__ s_col, int32_t* __restrict__ seg_ptr,
                                                             int32_t* __restrict__ c_colind) {
  for (int64_t q = (int64_t) blockIdx.x * 256 + threadIdx.x; q < nnz; q += (int64_t) gridDim.x * 256) {
    const int e = rank[q];
    if (rank[q + 1] != e) {
      seg_ptr[e] = (int32_t) q;
      c_colind[e] = s_col[q];
    }
    if (q == nnz - 1)
      seg_ptr[rank[nnz]] = (int32_t) nnz;
  }
}

static __global__ __launch_bounds__(256) void cz_rowptr_kernel(int64_t n_agg, const int32_t* __restrict__ s_rowptr,
                                                               const int32_t* __restrict__ rank, int32_t* __restrict__ c_rowptr) {
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i <= n_agg)
    c_rowptr[i] = rank[s_rowptr[i]];
}

} // namespace spb
