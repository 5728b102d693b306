// The SpMV / SpMM kernels and launchers of the value types whose arithmetic is not the storage type's own: 16-bit values
// with fp32 sums (lowp.hip) and complex values with conjugated views (complex.hip).  Modelled on the real kernels of
// spmv.hip / spmm.hip; index arithmetic, window ownership and summation orders are written here once, everything that touches
// a value goes through the policy VT of the including file:
//   mem, acc          a value in memory / in a register (sums are formed and kept in acc: fp32, or (re, im) of the value's
//                     precision); raw: what the row-block kernel holds between its loads and its products; out: a finished
//                     element on its way to memory
//   scalar            alpha / beta as the kernels take them; host_scalar(const void*) reads one from the caller's memory
//   zero, load, stream (read-once load), add, mac<CA, CB> (acc += op(a) * op(b); CA / CB conjugate, 16-bit ignores them)
//   stream_raw, load_raw, raw_zero, stage<CA, CB>   phase 1 of the row-block kernel: the product of two raw values
//   shfl, group_sum, group_sum_c<W>                 lane-group exchange and sums
//   update(y, i, alpha, s, beta), scale(beta, p)    y[i] = alpha * s + beta * y[i], *p = beta * *p; the element is read only
//                     when beta != 0 (NaN in y / C does not propagate at beta == 0).  nonzero(beta), finish(alpha, s, beta,
//                     old): the same for the row-group kernel, which loads and stores V elements at once
//   wide, load_vec<V>, store_vec<V>                 V = wide or 1 elements of a B / C row per lane access (16 bytes or one)
//   window                                          entries per row-block window: 2 * window acc fill 16 KiB of LDS
//   acc_words, word                                 an acc as words of the plan's long-row buffer (mm_long_cap counts words)
// Kernels (HBM-bound):
//   vk_spmv_vector_kernel     plan-free / VECTOR plan: a power-of-two group of lanes per row, group sums in acc.
//   vk_spmv_rowblock_kernel   ROWBLOCK plan: one 256-thread workgroup per nnz window of the plan; rows longer than the window
//                             leave their slices in the plan's part_head / part_tail (acc) and vk_spmv_long_fixup_kernel adds
//                             them up in window order, the tail last.
//   vk_spmm_rowgroup_kernel   layout_right B and C: a group of G lanes per row, each lane V elements of a B row per gather.
//   vk_spmm_strided_kernel    any other layout (layout_left, padded leading dimensions): element-wise gathers along the strides.
//   vk_spmm_long_rows_kernel  with a plan: rows longer than its window, cut into parts of ~4 K entries over many workgroups
//   vk_spmm_long_finish_kernel  (partial rows in acc), then added in part order (the row kernels skip those rows).
//   vk_scale_kernel           A without entries: y = beta * y, C = beta * C.
#pragma once

#include "common.hpp"
#include "multiply_args.hpp"
#include "plan.hpp"

namespace spb {

// ---------------------------------------------------------------------------------------------------------------------
// SpMV
// ---------------------------------------------------------------------------------------------------------------------
template <typename VT, typename O, int LPR, bool CA, bool CX>
__global__ __launch_bounds__(256) void vk_spmv_vector_kernel(int64_t m, const O* __restrict__ rowptr,
                                                             const int32_t* __restrict__ colind,
                                                             const typename VT::mem* __restrict__ values,
                                                             const typename VT::mem* __restrict__ x,
                                                             typename VT::mem* __restrict__ y, typename VT::scalar alpha,
                                                             typename VT::scalar beta) {
  constexpr int ROWS = 256 / LPR;
  const int64_t row = (int64_t) blockIdx.x * ROWS + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  typename VT::acc s = VT::zero();
  if (row < m) {
    const O p0 = rowptr[row], p1 = rowptr[row + 1];
    for (O p = p0 + lane; p < p1; p += LPR)
      VT::template mac<CA, CX>(s, VT::stream(values + p), VT::load(x + stream_load(colind + p)));
  }
  s = VT::template group_sum_c<LPR>(s);
  if (row < m && lane == 0)
    VT::update(y, row, alpha, s, beta);
}

// Sum of op(values[p]) * op(x[colind[p]]) for p in [lo, hi) over the whole workgroup (valid in every thread).
template <typename VT, typename O, bool CA, bool CX>
__device__ typename VT::acc block_segment_dot(O lo, O hi, const int32_t* __restrict__ colind,
                                              const typename VT::mem* __restrict__ values,
                                              const typename VT::mem* __restrict__ x, typename VT::acc* red) {
  typename VT::acc s = VT::zero();
  for (O p = lo + (O) threadIdx.x; p < hi; p += 256)
    VT::template mac<CA, CX>(s, VT::stream(values + p), VT::load(x + stream_load(colind + p)));
  s = VT::template group_sum_c<64>(s);
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
    red[threadIdx.x >> 6] = s;
  __syncthreads();
  typename VT::acc t = red[0];
  for (int i = 1; i < 4; ++i)
    t = VT::add(t, red[i]);
  return t;
}

// Window w owns the rows whose first entry lies in [w*WIN, (w+1)*WIN) (spmv.hip, spmv_rowblock_kernel): a row no longer
// than WIN ends before (w+2)*WIN, hence 2*WIN LDS slots; a longer row leaves its slice of this window in part_tail[w] (the
// window it starts in) or part_head[w] (later windows).
template <typename VT, typename O, bool HAS_LONG, bool CA, bool CX>
__global__ __launch_bounds__(256) void vk_spmv_rowblock_kernel(int64_t nnz, const O* __restrict__ rowptr,
                                                               const int32_t* __restrict__ colind,
                                                               const typename VT::mem* __restrict__ values,
                                                               const typename VT::mem* __restrict__ x,
                                                               typename VT::mem* __restrict__ y, typename VT::scalar alpha,
                                                               typename VT::scalar beta, const int32_t* __restrict__ win_row,
                                                               typename VT::acc* __restrict__ part_head,
                                                               typename VT::acc* __restrict__ part_tail) {
  typedef typename VT::acc acc_t;
  constexpr int WIN = VT::window;
  constexpr int CAP = 2 * WIN;
  constexpr int ITERS = CAP / 256;
  static_assert(CAP % 256 == 0, "window must be a multiple of 128");
  static_assert(CAP * sizeof(acc_t) <= 16384, "products must fit 16 KiB of LDS");
  __shared__ acc_t prod[CAP];
  __shared__ acc_t red[4];

  const int tid = threadIdx.x;
  const int64_t w = blockIdx.x;
  const int r_begin = win_row[w];
  int r_end = win_row[w + 1];
  const O wlo = (O) (w * WIN);
  const O whi = (O) ((w + 1) * WIN < nnz ? (w + 1) * WIN : nnz);

  const O a = rowptr[r_begin];  // first entry of the first owned row (>= wlo)
  O e = rowptr[r_end];          // one past the last entry of the last owned row

  if (HAS_LONG) {
    if (r_begin > 0 && a > wlo) {  // long row entering this window from an earlier one
      const O hs = rowptr[r_begin - 1];
      if (a - hs > (O) WIN) {
        const acc_t s = block_segment_dot<VT, O, CA, CX>(wlo, a < whi ? a : whi, colind, values, x, red);
        if (tid == 0)
          part_head[w] = s;
        __syncthreads();
      }
    }
    if (r_end > r_begin) {  // long row starting in this window (necessarily the last owned row)
      const O ls = rowptr[r_end - 1];
      if (e - ls > (O) WIN) {
        const acc_t s = block_segment_dot<VT, O, CA, CX>(ls, whi, colind, values, x, red);
        if (tid == 0)
          part_tail[w] = s;
        __syncthreads();
        r_end -= 1;
        e = ls;
      }
    }
  }
  const int total = (int) (e - a);  // <= CAP

  // ---- phase 1: stream colind / values (all loads of the thread in flight together), gather x, stage the products
  int32_t c[ITERS];
  typename VT::raw v[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int q = it * 256 + tid;
    c[it] = 0;
    v[it] = VT::raw_zero();
    if (q < total) {
      c[it] = stream_load(colind + a + q);
      v[it] = VT::stream_raw(values + a + q);
    }
  }
  typename VT::raw xv[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it)
    xv[it] = VT::load_raw(x + c[it]);
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int q = it * 256 + tid;
    if (q < total)
      prod[q] = VT::template stage<CA, CX>(v[it], xv[it]);
  }
  __syncthreads();

  // ---- phase 2: a group of `lpr` lanes reduces each owned row out of LDS
  const int nrows = r_end - r_begin;
  int lpr = 1;
  while (lpr < 64 && nrows * lpr * 2 <= 256)
    lpr <<= 1;
  const int grp = tid / lpr, lig = tid % lpr, ngrp = 256 / lpr;
  for (int r = r_begin + grp; r < r_end; r += ngrp) {
    const int s0 = (int) (rowptr[r] - a), s1 = (int) (rowptr[r + 1] - a);
    acc_t s = VT::zero();
    for (int q = s0 + lig; q < s1; q += lpr)
      s = VT::add(s, prod[q]);
    s = VT::group_sum(s, lpr);
    if (lig == 0)
      VT::update(y, r, alpha, s, beta);
  }
}

// One wavefront per long row: y[r] = alpha * (heads + tail) + beta * y[r].
template <typename VT, typename O>
__global__ __launch_bounds__(64) void vk_spmv_long_fixup_kernel(int64_t n_long, int win, const int32_t* __restrict__ long_rows,
                                                                const O* __restrict__ rowptr,
                                                                const typename VT::acc* __restrict__ part_head,
                                                                const typename VT::acc* __restrict__ part_tail,
                                                                typename VT::mem* __restrict__ y, typename VT::scalar alpha,
                                                                typename VT::scalar beta) {
  const int64_t i = blockIdx.x;
  if (i >= n_long)
    return;
  const int r = long_rows[i];
  const int64_t p0 = (int64_t) rowptr[r], p1 = (int64_t) rowptr[r + 1];
  const int64_t w0 = p0 / win, w1 = (p1 - 1) / win;
  typename VT::acc s = VT::zero();
  for (int64_t w = w0 + 1 + threadIdx.x; w <= w1; w += 64)
    s = VT::add(s, part_head[w]);
  s = VT::template group_sum_c<64>(s);
  if (threadIdx.x == 0)
    VT::update(y, r, alpha, VT::add(s, part_tail[w0]), beta);
}

// y = beta * y (A without entries); strided so that the same kernel serves C of SpMM
template <typename VT>
__global__ __launch_bounds__(256) void vk_scale_kernel(int64_t rows, int64_t cols, typename VT::mem* __restrict__ y, int64_t rs,
                                                       int64_t cs, typename VT::scalar beta) {
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i < rows * cols) {
    const int64_t r = i / cols, c = i % cols;
    typename VT::mem* p = y + r * rs + c * cs;
    VT::scale(beta, p);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// SpMM
// ---------------------------------------------------------------------------------------------------------------------
// Modelled on spmm_rowgroup_kernel (spmm.hip): G lanes per row walk its entries G at a time, the (column, value) pairs are
// handed round by shuffles, every lane accumulates V consecutive columns of C; panels of G*V columns.  long_len > 0: rows
// longer than that belong to the long-row kernels.
template <typename VT, typename O, int V, bool CA, bool CB>
__global__ __launch_bounds__(256) void vk_spmm_rowgroup_kernel(int64_t m, int64_t n, const O* __restrict__ rowptr,
                                                               const int32_t* __restrict__ colind,
                                                               const typename VT::mem* __restrict__ values,
                                                               const typename VT::mem* __restrict__ B, int64_t ldb,
                                                               typename VT::mem* __restrict__ C, int64_t ldc,
                                                               typename VT::scalar alpha, typename VT::scalar beta, int G,
                                                               int long_len) {
  typedef typename VT::acc acc_t;
  const int rows_per_block = 256 / G;
  const int64_t row = (int64_t) blockIdx.x * rows_per_block + threadIdx.x / G;
  const int lig = threadIdx.x % G;
  const int64_t panel_cols = (int64_t) G * V;
  O p0 = 0, p1 = 0;
  bool mine = row < m;
  if (mine) {
    p0 = rowptr[row];
    p1 = rowptr[row + 1];
    if (long_len > 0 && p1 - p0 > (O) long_len)
      mine = false;
  }
  if (!mine)
    p0 = p1 = 0;
  const bool scaled = VT::nonzero(beta);
  for (int64_t col0 = (int64_t) lig * V; col0 - (int64_t) lig * V < n; col0 += panel_cols) {
    const bool active = mine && col0 < n;
    acc_t acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i)
      acc[i] = VT::zero();
    const typename VT::mem* __restrict__ Bc = B + col0;
    for (O base = p0; base < p1; base += G) {
      int32_t c = 0;
      acc_t v = VT::zero();
      if (base + lig < p1) {
        c = stream_load(colind + base + lig);
        v = VT::stream(values + base + lig);
      }
      const int cnt = (int) ((p1 - base) < (O) G ? (p1 - base) : (O) G);
      int j = 0;
      for (; j + 4 <= cnt; j += 4) {
        const int64_t k0 = __shfl(c, j, G), k1 = __shfl(c, j + 1, G), k2 = __shfl(c, j + 2, G), k3 = __shfl(c, j + 3, G);
        const acc_t a0 = VT::shfl(v, j, G), a1 = VT::shfl(v, j + 1, G), a2 = VT::shfl(v, j + 2, G), a3 = VT::shfl(v, j + 3, G);
        if (active) {
          acc_t b0[V], b1[V], b2[V], b3[V];
          VT::template load_vec<V>(Bc + k0 * ldb, b0);
          VT::template load_vec<V>(Bc + k1 * ldb, b1);
          VT::template load_vec<V>(Bc + k2 * ldb, b2);
          VT::template load_vec<V>(Bc + k3 * ldb, b3);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            VT::template mac<CA, CB>(acc[i], a0, b0[i]);
            VT::template mac<CA, CB>(acc[i], a1, b1[i]);
            VT::template mac<CA, CB>(acc[i], a2, b2[i]);
            VT::template mac<CA, CB>(acc[i], a3, b3[i]);
          }
        }
      }
      for (; j < cnt; ++j) {
        const int64_t k0 = __shfl(c, j, G);
        const acc_t a0 = VT::shfl(v, j, G);
        if (active) {
          acc_t b0[V];
          VT::template load_vec<V>(Bc + k0 * ldb, b0);
#pragma unroll
          for (int i = 0; i < V; ++i)
            VT::template mac<CA, CB>(acc[i], a0, b0[i]);
        }
      }
    }
    if (active) {
      typename VT::mem* cp = C + row * ldc + col0;
      acc_t old[V];
      if (scaled) {
        VT::template load_vec<V>(cp, old);
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i)
          old[i] = VT::zero();
      }
      typename VT::out out[V];
#pragma unroll
      for (int i = 0; i < V; ++i)
        out[i] = VT::finish(alpha, acc[i], beta, old[i]);
      VT::template store_vec<V>(cp, out);
    }
  }
}

// Dense operands of any layout: element (i, j) at i*rs + j*cs (spmm_strided_kernel of spmm.hip).  G lanes per row, JT output
// columns per tile in registers, group reduction by shuffles, lane j % G writes column j of the tile.
template <typename VT, typename O, int JT, bool CA, bool CB>
__global__ __launch_bounds__(256) void vk_spmm_strided_kernel(int64_t m, int64_t n, const O* __restrict__ rowptr,
                                                              const int32_t* __restrict__ colind,
                                                              const typename VT::mem* __restrict__ values,
                                                              const typename VT::mem* __restrict__ B, int64_t brs, int64_t bcs,
                                                              typename VT::mem* __restrict__ C, int64_t crs, int64_t ccs,
                                                              typename VT::scalar alpha, typename VT::scalar beta, int G,
                                                              int long_len) {
  typedef typename VT::acc acc_t;
  const int64_t row = (int64_t) blockIdx.x * (256 / G) + threadIdx.x / G;
  const int lig = threadIdx.x % G;
  O p0 = 0, p1 = 0;
  bool mine = row < m;
  if (mine) {
    p0 = rowptr[row];
    p1 = rowptr[row + 1];
    if (long_len > 0 && p1 - p0 > (O) long_len)
      mine = false;
  }
  if (!mine)
    p0 = p1 = 0;
  for (int64_t j0 = (int64_t) blockIdx.y * JT; j0 < n; j0 += (int64_t) gridDim.y * JT) {
    acc_t acc[JT];
#pragma unroll
    for (int j = 0; j < JT; ++j)
      acc[j] = VT::zero();
    for (O p = p0 + lig; p < p1; p += G) {
      const int64_t c = colind[p];
      const acc_t v = VT::load(values + p);
      const typename VT::mem* __restrict__ bp = B + c * brs + j0 * bcs;
#pragma unroll
      for (int j = 0; j < JT; ++j)
        if (j0 + j < n)
          VT::template mac<CA, CB>(acc[j], v, VT::load(bp + j * bcs));
    }
#pragma unroll
    for (int j = 0; j < JT; ++j)
      acc[j] = VT::group_sum(acc[j], G);
    if (mine) {
#pragma unroll
      for (int j = 0; j < JT; ++j)
        if (lig == (j % G) && j0 + j < n) {
          typename VT::mem* cp = C + row * crs + (j0 + j) * ccs;
          VT::update(cp, 0, alpha, acc[j], beta);
        }
    }
  }
}

// Workgroup (i, part) sums entries [lo, hi) of long row i for all n columns into part_buf[(i*parts + part)*n ..]
// (spmm_long_rows_kernel of spmm.hip, B along its strides).
template <typename VT, typename O, bool CA, bool CB>
__global__ __launch_bounds__(256) void vk_spmm_long_rows_kernel(const int32_t* __restrict__ long_rows, int parts, int64_t n,
                                                                const O* __restrict__ rowptr,
                                                                const int32_t* __restrict__ colind,
                                                                const typename VT::mem* __restrict__ values,
                                                                const typename VT::mem* __restrict__ B, int64_t brs,
                                                                int64_t bcs, typename VT::acc* __restrict__ part_buf) {
  typedef typename VT::acc acc_t;
  __shared__ acc_t red[256];
  const int64_t i = blockIdx.x;
  const int part = blockIdx.y;
  const int64_t r = long_rows[i];
  const O p0 = rowptr[r], p1 = rowptr[r + 1];
  const O per = ((p1 - p0) + (O) parts - 1) / (O) parts;
  const O lo = p0 + (O) part * per < p1 ? p0 + (O) part * per : p1;
  const O hi = (lo + per) < p1 ? (lo + per) : p1;
  const int cpp = n < 256 ? (int) n : 256;  // columns per pass
  const int eg = 256 / cpp;                  // entry groups
  const int j = threadIdx.x % cpp, e = threadIdx.x / cpp;
  acc_t* out = part_buf + ((int64_t) i * parts + part) * n;
  for (int64_t c0 = 0; c0 < n; c0 += cpp) {
    const bool col_ok = e < eg && c0 + j < n;
    acc_t acc = VT::zero();
    if (col_ok) {
      const typename VT::mem* Bc = B + (c0 + j) * bcs;
      O p = lo + (O) e;
      for (; p + (O) (3 * eg) < hi; p += (O) (4 * eg)) {  // four gathers in flight
        const int64_t k0 = colind[p], k1 = colind[p + eg], k2 = colind[p + 2 * eg], k3 = colind[p + 3 * eg];
        const acc_t b0 = VT::load(Bc + k0 * brs), b1 = VT::load(Bc + k1 * brs), b2 = VT::load(Bc + k2 * brs),
                    b3 = VT::load(Bc + k3 * brs);
        VT::template mac<CA, CB>(acc, VT::load(values + p), b0);
        VT::template mac<CA, CB>(acc, VT::load(values + (p + eg)), b1);
        VT::template mac<CA, CB>(acc, VT::load(values + (p + 2 * eg)), b2);
        VT::template mac<CA, CB>(acc, VT::load(values + (p + 3 * eg)), b3);
      }
      for (; p < hi; p += (O) eg)
        VT::template mac<CA, CB>(acc, VT::load(values + p), VT::load(Bc + (int64_t) colind[p] * brs));
    }
    __syncthreads();
    red[threadIdx.x] = acc;
    __syncthreads();
    if (e == 0 && c0 + j < n) {
      acc_t sum = red[j];
      for (int g = 1; g < eg; ++g)
        sum = VT::add(sum, red[g * cpp + j]);
      out[c0 + j] = sum;
    }
  }
}

// C[row] = alpha * (parts in order) + beta * C[row] for every long row
template <typename VT>
__global__ __launch_bounds__(256) void vk_spmm_long_finish_kernel(const int32_t* __restrict__ long_rows, int parts, int64_t n,
                                                                  const typename VT::acc* __restrict__ part_buf,
                                                                  typename VT::mem* __restrict__ C, int64_t crs, int64_t ccs,
                                                                  typename VT::scalar alpha, typename VT::scalar beta) {
  const int64_t i = blockIdx.x;
  const int64_t r = long_rows[i];
  for (int64_t j = threadIdx.x; j < n; j += 256) {
    typename VT::acc sum = VT::zero();
    for (int q = 0; q < parts; ++q)
      sum = VT::add(sum, part_buf[((int64_t) i * parts + q) * n + j]);
    typename VT::mem* cp = C + r * crs + j * ccs;
    VT::update(cp, 0, alpha, sum, beta);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side: the arguments are checked (the entry points of lowp.hip / complex.hip), the types resolved
// ---------------------------------------------------------------------------------------------------------------------
template <typename VT, typename O, bool CA, bool CX>
static int vk_spmv(spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int64_t m, int64_t nnz, const void* alpha_p,
                   const void* rowptr_p, const int32_t* colind, const void* values_p, const void* x_p, const void* beta_p,
                   void* y_p) {
  typedef typename VT::acc acc_t;
  typedef typename VT::mem mem_t;
  const typename VT::scalar alpha = VT::host_scalar(alpha_p), beta = VT::host_scalar(beta_p);
  const O* rowptr = static_cast<const O*>(rowptr_p);
  const mem_t* values = static_cast<const mem_t*>(values_p);
  const mem_t* x = static_cast<const mem_t*>(x_p);
  mem_t* y = static_cast<mem_t*>(y_p);
  hipStream_t s = h->stream;
  if (m == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  if (nnz == 0) {
    hipLaunchKernelGGL((vk_scale_kernel<VT>), dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, (int64_t) 1, y, (int64_t) 1,
                       (int64_t) 1, beta);
    SPB_HIP(hipGetLastError());
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  if (pl && pl->alg == SPBLAS_GFX950_SPMV_ROWBLOCK && pl->win == VT::window) {
    note_use(pl->use, s);  // part_head / part_tail are the plan's
    acc_t* ph = static_cast<acc_t*>(pl->part_head);
    acc_t* pt = static_cast<acc_t*>(pl->part_tail);
    if (pl->n_long > 0) {
      hipLaunchKernelGGL((vk_spmv_rowblock_kernel<VT, O, true, CA, CX>), dim3((unsigned) pl->nwin), dim3(256), 0, s, nnz,
                         rowptr, colind, values, x, y, alpha, beta, pl->win_row, ph, pt);
      hipLaunchKernelGGL((vk_spmv_long_fixup_kernel<VT, O>), dim3((unsigned) pl->n_long), dim3(64), 0, s, pl->n_long, pl->win,
                         pl->long_rows, rowptr, ph, pt, y, alpha, beta);
    } else {
      hipLaunchKernelGGL((vk_spmv_rowblock_kernel<VT, O, false, CA, CX>), dim3((unsigned) pl->nwin), dim3(256), 0, s, nnz,
                         rowptr, colind, values, x, y, alpha, beta, pl->win_row, ph, pt);
    }
    SPB_HIP(hipGetLastError());
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  const int lpr = pl ? pl->vector_lpr : pick_lpr(m, nnz);
#define SPB_VKVEC(L)                                                                                                           \
  hipLaunchKernelGGL((vk_spmv_vector_kernel<VT, O, L, CA, CX>), dim3((unsigned) cdiv(m, 256 / L)), dim3(256), 0, s, m, rowptr, \
                     colind, values, x, y, alpha, beta)
  switch (lpr) {
  case 2: SPB_VKVEC(2); break;
  case 4: SPB_VKVEC(4); break;
  case 8: SPB_VKVEC(8); break;
  case 16: SPB_VKVEC(16); break;
  case 32: SPB_VKVEC(32); break;
  default: SPB_VKVEC(64); break;
  }
#undef SPB_VKVEC
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

template <typename VT, typename O, bool CA, bool CB>
static int vk_spmm(spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int64_t m, int64_t n, int64_t nnz, const void* alpha_p,
                   const void* rowptr_p, const int32_t* colind, const void* values_p, const void* B_p, int64_t brs, int64_t bcs,
                   const void* beta_p, void* C_p, int64_t crs, int64_t ccs) {
  typedef typename VT::acc acc_t;
  typedef typename VT::mem mem_t;
  const typename VT::scalar alpha = VT::host_scalar(alpha_p), beta = VT::host_scalar(beta_p);
  const O* rowptr = static_cast<const O*>(rowptr_p);
  const mem_t* values = static_cast<const mem_t*>(values_p);
  const mem_t* B = static_cast<const mem_t*>(B_p);
  mem_t* C = static_cast<mem_t*>(C_p);
  hipStream_t s = h->stream;
  if (m == 0 || n == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  if (nnz == 0) {
    hipLaunchKernelGGL((vk_scale_kernel<VT>), dim3((unsigned) cdiv(m * n, 256)), dim3(256), 0, s, m, n, C, crs, ccs, beta);
    SPB_HIP(hipGetLastError());
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  // a plan's long-row list: rows longer than its window are cut into parts of ~4 K entries (at most 64 per row) over
  // many workgroups instead of serialising on one lane group; the partial rows (acc) live in the plan (grown on demand)
  const int long_len = pl && pl->n_long > 0 ? pl->win : 0;
  if (long_len > 0) {
    int64_t parts = cdiv(pl->max_row_len, 4096);
    parts = parts < 1 ? 1 : (parts > 64 ? 64 : parts);
    const int64_t need = pl->n_long * parts * n * VT::acc_words;  // (in words of the value type's plans)
    if (pl->mm_long_cap < need || pl->mm_long_parts != (int) parts) {
      if (stream_capturing(s))  // the first call with this many columns has to run outside the capture
        return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
      dev_free(pl->mm_long_part, s);
      pl->mm_long_part = nullptr;
      pl->mm_long_cap = 0;
      int rc = dev_alloc(&pl->mm_long_part, (size_t) need * sizeof(typename VT::word), s);
      if (rc)
        return rc;
      pl->mm_long_cap = need;
      pl->mm_long_parts = (int) parts;
    }
    note_use(pl->use, s);
  }
  if (ccs == 1 && bcs == 1) {
    // layout_right: 16-byte gathers (VT::wide elements) when B and C allow them
    constexpr int W = VT::wide;
    const uintptr_t bits = (uintptr_t) B | (uintptr_t) C;
    const bool wide = W > 1 && n % W == 0 && brs % W == 0 && crs % W == 0 && (bits % 16) == 0;
    int G = 1;
    while (G < 64 && (int64_t) G * (wide ? W : 1) < n)
      G <<= 1;
    const unsigned grid = (unsigned) cdiv(m, 256 / G);
    if constexpr (W > 1) {
      if (wide)
        hipLaunchKernelGGL((vk_spmm_rowgroup_kernel<VT, O, W, CA, CB>), dim3(grid), dim3(256), 0, s, m, n, rowptr, colind,
                           values, B, brs, C, crs, alpha, beta, G, long_len);
    }
    if (!wide)
      hipLaunchKernelGGL((vk_spmm_rowgroup_kernel<VT, O, 1, CA, CB>), dim3(grid), dim3(256), 0, s, m, n, rowptr, colind, values,
                         B, brs, C, crs, alpha, beta, G, long_len);
  } else {
    int G = 2;
    const int64_t avg = nnz / m;
    while (G < 64 && G < avg)
      G <<= 1;
    constexpr int JT = 8;
    const int64_t tiles = cdiv(n, JT);
    hipLaunchKernelGGL((vk_spmm_strided_kernel<VT, O, JT, CA, CB>),
                       dim3((unsigned) cdiv(m, 256 / G), (unsigned) (tiles < 64 ? tiles : 64)), dim3(256), 0, s, m, n, rowptr,
                       colind, values, B, brs, bcs, C, crs, ccs, alpha, beta, G, long_len);
  }
  if (long_len > 0) {
    acc_t* part = static_cast<acc_t*>(pl->mm_long_part);
    hipLaunchKernelGGL((vk_spmm_long_rows_kernel<VT, O, CA, CB>), dim3((unsigned) pl->n_long, (unsigned) pl->mm_long_parts),
                       dim3(256), 0, s, pl->long_rows, pl->mm_long_parts, n, rowptr, colind, values, B, brs, bcs, part);
    hipLaunchKernelGGL((vk_spmm_long_finish_kernel<VT>), dim3((unsigned) pl->n_long), dim3(256), 0, s, pl->long_rows,
                       pl->mm_long_parts, n, part, C, crs, ccs, alpha, beta);
  }
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

} // namespace spb
