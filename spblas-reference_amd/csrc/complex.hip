// Complex SpMV / SpMM for gfx950 (std::complex<float> = c32, std::complex<double> = c64, interleaved re / im):
//   y = alpha * op'(A) * x' + beta * y,   C = alpha * op'(A) * B' + beta * C
// where op' / ' conjugate A's values and / or x / B (conj_flags bit 0 / bit 1: conjugated_view in the reference,
// views/conjugated_view_impl.hpp).  The maths is the reference CPU path (algorithms/multiply_impl.hpp:33-92) on complex
// scalars, accumulated in the value type.  A product is the plain componentwise formula (ac - bd, ad + bc) as four FMAs, the
// conjugations folded in as sign flips at compile time; no C Annex G inf / NaN recovery.
//
// Kernels (HBM-bound; algorithmic bytes per entry = 4 + s, s = 8 (c32) or 16 (c64), per row sizeof(O) + s, per column s):
//   cspmv_vector_kernel     plan-free / VECTOR plan: a power-of-two group of lanes per row, one 8- or 16-byte value load
//                           per entry, per-component group sums.
//   cspmv_rowblock_kernel   ROWBLOCK plan: one 256-thread workgroup per nnz window of the plan (the window is chosen for
//                           the complex value size at plan creation, so the 2 * WIN complex products fit 16 KiB of LDS);
//                           rows longer than the window reduce their slices into the plan's part_head / part_tail and
//                           cspmv_long_fixup_kernel adds them up, as spmv.hip does for real values.
//   cspmm_rowgroup_kernel   layout_right B and C: a group of G lanes per row, each lane 16 bytes of B per gather (two c32
//                           or one c64 element).
//   cspmm_strided_kernel    any other layout (layout_left, padded leading dimensions): element-wise gathers along the strides.
//   cspmm_long_rows_kernel  with a plan: rows longer than its window, cut into parts of ~4 K entries over many workgroups,
//   cspmm_long_finish_kernel  then added in part order (the row kernels skip those rows).
// The real kernels (spmv.hip, spmm.hip) are untouched; this file only adds code.
#include "common.hpp"
#include "complex_api.hpp"
#include "lowp_api.hpp"
#include "plan.hpp"

namespace spb {

// Complex value types: in registers an (re, im) vector; in memory the alignment of std::complex (4 / 8 bytes), which the
// caller's arrays are only guaranteed to have.
template <typename R>
struct cplx;
template <>
struct cplx<float> {
  typedef float reg __attribute__((ext_vector_type(2)));
  typedef float mem __attribute__((ext_vector_type(2), aligned(4)));
};
template <>
struct cplx<double> {
  typedef double reg __attribute__((ext_vector_type(2)));
  typedef double mem __attribute__((ext_vector_type(2), aligned(8)));
};

// streaming (read-once) load of one value of A at the alignment of std::complex (common.hpp: stream_load)
__device__ __forceinline__ cplx<float>::reg cstream_load(const cplx<float>::mem* p) {
  return __builtin_nontemporal_load(p);
}
__device__ __forceinline__ cplx<double>::reg cstream_load(const cplx<double>::mem* p) {
  return __builtin_nontemporal_load(p);
}

template <typename C2>
__device__ __forceinline__ C2 czero() {
  C2 z;
  z.x = 0;
  z.y = 0;
  return z;
}

// acc += op(a) * op(b): (ar, ai') * (br, bi') with ai' = -ai under CA, bi' = -bi under CB
template <bool CA, bool CB, typename C2>
__device__ __forceinline__ void cmac(C2& acc, const C2 a, const C2 b) {
  const auto ai = CA ? -a.y : a.y;
  const auto bi = CB ? -b.y : b.y;
  acc.x = __builtin_fma(a.x, b.x, acc.x);
  acc.x = __builtin_fma(-ai, bi, acc.x);
  acc.y = __builtin_fma(a.x, bi, acc.y);
  acc.y = __builtin_fma(ai, b.x, acc.y);
}

template <typename C2>
__device__ __forceinline__ C2 cmul(const C2 a, const C2 b) {
  C2 r;
  r.x = a.x * b.x - a.y * b.y;
  r.y = a.x * b.y + a.y * b.x;
  return r;
}

// alpha * s, or alpha * s + beta * old when beta != 0 (beta == 0: old is not read, NaN in y does not propagate)
template <typename C2>
__device__ __forceinline__ C2 cfinish(const C2 alpha, const C2 s, const C2 beta, const C2* old) {
  C2 r = cmul(alpha, s);
  if (beta.x != 0 || beta.y != 0) {
    const C2 b = cmul(beta, *old);
    r.x += b.x;
    r.y += b.y;
  }
  return r;
}

template <int WIDTH, typename C2>
__device__ __forceinline__ C2 cgroup_sum_c(C2 v) {
  v.x = group_sum_c<WIDTH>(v.x);
  v.y = group_sum_c<WIDTH>(v.y);
  return v;
}

template <typename C2>
__device__ __forceinline__ C2 cgroup_sum(C2 v, int width) {
  v.x = group_sum(v.x, width);
  v.y = group_sum(v.y, width);
  return v;
}

template <typename C2>
__device__ __forceinline__ C2 cshfl(const C2 v, int src, int width) {
  C2 r;
  r.x = __shfl(v.x, src, width);
  r.y = __shfl(v.y, src, width);
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// SpMV
// ---------------------------------------------------------------------------------------------------------------------
template <typename R, typename O, int LPR, bool CA, bool CX>
__global__ __launch_bounds__(256) void cspmv_vector_kernel(int64_t m, const O* __restrict__ rowptr,
                                                           const int32_t* __restrict__ colind,
                                                           const typename cplx<R>::mem* __restrict__ values,
                                                           const typename cplx<R>::mem* __restrict__ x,
                                                           typename cplx<R>::mem* __restrict__ y,
                                                           typename cplx<R>::reg alpha, typename cplx<R>::reg beta) {
  typedef typename cplx<R>::reg C2;
  constexpr int ROWS = 256 / LPR;
  const int64_t row = (int64_t) blockIdx.x * ROWS + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  C2 s = czero<C2>();
  if (row < m) {
    const O p0 = rowptr[row], p1 = rowptr[row + 1];
    for (O p = p0 + lane; p < p1; p += LPR)
      cmac<CA, CX>(s, cstream_load(values + p), (C2) x[stream_load(colind + p)]);
  }
  s = cgroup_sum_c<LPR>(s);
  if (row < m && lane == 0) {
    const C2 old = beta.x != 0 || beta.y != 0 ? (C2) y[row] : czero<C2>();
    y[row] = cfinish(alpha, s, beta, &old);
  }
}

// Sum of op(values[p]) * op(x[colind[p]]) for p in [lo, hi) over the whole workgroup (valid in every thread).
template <typename R, typename O, bool CA, bool CX>
__device__ typename cplx<R>::reg block_segment_cdot(O lo, O hi, const int32_t* __restrict__ colind,
                                                    const typename cplx<R>::mem* __restrict__ values,
                                                    const typename cplx<R>::mem* __restrict__ x,
                                                    typename cplx<R>::reg* red) {
  typedef typename cplx<R>::reg C2;
  C2 s = czero<C2>();
  for (O p = lo + (O) threadIdx.x; p < hi; p += 256)
    cmac<CA, CX>(s, cstream_load(values + p), (C2) x[stream_load(colind + p)]);
  s = cgroup_sum_c<64>(s);
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
    red[threadIdx.x >> 6] = s;
  __syncthreads();
  C2 t = red[0];
  for (int i = 1; i < 4; ++i) {
    t.x += red[i].x;
    t.y += red[i].y;
  }
  return t;
}

// Window w owns the rows whose first entry lies in [w*WIN, (w+1)*WIN) (spmv.hip, spmv_rowblock_kernel): a row no longer
// than WIN ends before (w+2)*WIN, hence 2*WIN complex LDS slots; a longer row leaves its slice of this window in
// part_tail[w] (the window it starts in) or part_head[w] (later windows).
template <typename R, typename O, int WIN, bool HAS_LONG, bool CA, bool CX>
__global__ __launch_bounds__(256) void cspmv_rowblock_kernel(
    int64_t nnz, const O* __restrict__ rowptr, const int32_t* __restrict__ colind,
    const typename cplx<R>::mem* __restrict__ values, const typename cplx<R>::mem* __restrict__ x,
    typename cplx<R>::mem* __restrict__ y, typename cplx<R>::reg alpha, typename cplx<R>::reg beta,
    const int32_t* __restrict__ win_row, typename cplx<R>::reg* __restrict__ part_head,
    typename cplx<R>::reg* __restrict__ part_tail) {
  typedef typename cplx<R>::reg C2;
  constexpr int CAP = 2 * WIN;
  constexpr int ITERS = CAP / 256;
  static_assert(CAP % 256 == 0, "window must be a multiple of 128");
  static_assert(CAP * sizeof(C2) <= 16384, "products must fit 16 KiB of LDS");
  __shared__ C2 prod[CAP];
  __shared__ C2 red[4];

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
        const C2 s = block_segment_cdot<R, O, CA, CX>(wlo, a < whi ? a : whi, colind, values, x, red);
        if (tid == 0)
          part_head[w] = s;
        __syncthreads();
      }
    }
    if (r_end > r_begin) {  // long row starting in this window (necessarily the last owned row)
      const O ls = rowptr[r_end - 1];
      if (e - ls > (O) WIN) {
        const C2 s = block_segment_cdot<R, O, CA, CX>(ls, whi, colind, values, x, red);
        if (tid == 0)
          part_tail[w] = s;
        __syncthreads();
        r_end -= 1;
        e = ls;
      }
    }
  }
  const int total = (int) (e - a);  // <= CAP

  // ---- phase 1: stream colind / values (all loads of the thread in flight together), gather x, stage products
  int32_t c[ITERS];
  C2 v[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int q = it * 256 + tid;
    c[it] = 0;
    v[it] = czero<C2>();
    if (q < total) {
      c[it] = stream_load(colind + a + q);
      v[it] = cstream_load(values + a + q);
    }
  }
  C2 xv[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it)
    xv[it] = (C2) x[c[it]];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int q = it * 256 + tid;
    if (q < total) {
      C2 p = czero<C2>();
      cmac<CA, CX>(p, v[it], xv[it]);
      prod[q] = p;
    }
  }
  __syncthreads();

  // ---- phase 2: a group of `lpr` lanes reduces each owned row out of LDS, per component
  const int nrows = r_end - r_begin;
  int lpr = 1;
  while (lpr < 64 && nrows * lpr * 2 <= 256)
    lpr <<= 1;
  const int grp = tid / lpr, lig = tid % lpr, ngrp = 256 / lpr;
  for (int r = r_begin + grp; r < r_end; r += ngrp) {
    const int s0 = (int) (rowptr[r] - a), s1 = (int) (rowptr[r + 1] - a);
    C2 s = czero<C2>();
    for (int q = s0 + lig; q < s1; q += lpr) {
      s.x += prod[q].x;
      s.y += prod[q].y;
    }
    s = cgroup_sum(s, lpr);
    if (lig == 0) {
      const C2 old = beta.x != 0 || beta.y != 0 ? (C2) y[r] : czero<C2>();
      y[r] = cfinish(alpha, s, beta, &old);
    }
  }
}

// One wavefront per long row: y[r] = alpha * (tail + heads) + beta * y[r].
template <typename R, typename O>
__global__ __launch_bounds__(64) void cspmv_long_fixup_kernel(int64_t n_long, int win, const int32_t* __restrict__ long_rows,
                                                              const O* __restrict__ rowptr,
                                                              const typename cplx<R>::reg* __restrict__ part_head,
                                                              const typename cplx<R>::reg* __restrict__ part_tail,
                                                              typename cplx<R>::mem* __restrict__ y,
                                                              typename cplx<R>::reg alpha, typename cplx<R>::reg beta) {
  typedef typename cplx<R>::reg C2;
  const int64_t i = blockIdx.x;
  if (i >= n_long)
    return;
  const int r = long_rows[i];
  const int64_t p0 = (int64_t) rowptr[r], p1 = (int64_t) rowptr[r + 1];
  const int64_t w0 = p0 / win, w1 = (p1 - 1) / win;
  C2 s = czero<C2>();
  for (int64_t w = w0 + 1 + threadIdx.x; w <= w1; w += 64) {
    s.x += part_head[w].x;
    s.y += part_head[w].y;
  }
  s = cgroup_sum_c<64>(s);
  if (threadIdx.x == 0) {
    s.x += part_tail[w0].x;
    s.y += part_tail[w0].y;
    const C2 old = beta.x != 0 || beta.y != 0 ? (C2) y[r] : czero<C2>();
    y[r] = cfinish(alpha, s, beta, &old);
  }
}

// y = beta * y (A without entries); strided so that the same kernel serves C of SpMM
template <typename R>
__global__ __launch_bounds__(256) void cscale_kernel(int64_t rows, int64_t cols, typename cplx<R>::mem* __restrict__ y,
                                                     int64_t rs, int64_t cs, typename cplx<R>::reg beta) {
  typedef typename cplx<R>::reg C2;
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i < rows * cols) {
    const int64_t r = i / cols, c = i % cols;
    typename cplx<R>::mem* p = y + r * rs + c * cs;
    *p = beta.x != 0 || beta.y != 0 ? cmul(beta, (C2) *p) : czero<C2>();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// SpMM
// ---------------------------------------------------------------------------------------------------------------------
// V complex elements of B per lane and gather: c32 V = 2 (16 B), c64 V = 1 (16 B); c32 with a B / C that is not 16-byte
// aligned (odd n or leading dimension) V = 1.
template <typename R, int V>
struct cvec;
template <>
struct cvec<float, 2> {
  typedef float mem __attribute__((ext_vector_type(4), aligned(16)));
};
template <typename R>
struct cvec<R, 1> {
  typedef typename cplx<R>::mem mem;
};

template <typename R, int V>
__device__ __forceinline__ void cload_vec(const typename cplx<R>::mem* p, typename cplx<R>::reg (&out)[V]) {
  if constexpr (V == 1) {
    out[0] = (typename cplx<R>::reg) * p;
  } else {
    const typename cvec<R, 2>::mem q = *reinterpret_cast<const typename cvec<R, 2>::mem*>(p);
    out[0].x = q.x;
    out[0].y = q.y;
    out[1].x = q.z;
    out[1].y = q.w;
  }
}

template <typename R, int V>
__device__ __forceinline__ void cstore_vec(typename cplx<R>::mem* p, const typename cplx<R>::reg (&in)[V]) {
  if constexpr (V == 1) {
    *p = in[0];
  } else {
    typename cvec<R, 2>::mem q;
    q.x = in[0].x;
    q.y = in[0].y;
    q.z = in[1].x;
    q.w = in[1].y;
    *reinterpret_cast<typename cvec<R, 2>::mem*>(p) = q;
  }
}

// Modelled on spmm_rowgroup_kernel (spmm.hip): G lanes per row walk its entries G at a time, the (column, value) pairs are
// handed round by shuffles, every lane accumulates V consecutive columns of C; panels of G*V columns.  long_len > 0: rows
// longer than that belong to the long-row kernels.
template <typename R, typename O, int V, bool CA, bool CB>
__global__ __launch_bounds__(256) void cspmm_rowgroup_kernel(int64_t m, int64_t n, const O* __restrict__ rowptr,
                                                             const int32_t* __restrict__ colind,
                                                             const typename cplx<R>::mem* __restrict__ values,
                                                             const typename cplx<R>::mem* __restrict__ B, int64_t ldb,
                                                             typename cplx<R>::mem* __restrict__ C, int64_t ldc,
                                                             typename cplx<R>::reg alpha, typename cplx<R>::reg beta, int G,
                                                             int long_len) {
  typedef typename cplx<R>::reg C2;
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
  const bool beta0 = beta.x == 0 && beta.y == 0;
  for (int64_t col0 = (int64_t) lig * V; col0 - (int64_t) lig * V < n; col0 += panel_cols) {
    const bool active = mine && col0 < n;
    C2 acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i)
      acc[i] = czero<C2>();
    const typename cplx<R>::mem* __restrict__ Bc = B + col0;
    for (O base = p0; base < p1; base += G) {
      int32_t c = 0;
      C2 v = czero<C2>();
      if (base + lig < p1) {
        c = stream_load(colind + base + lig);
        v = cstream_load(values + base + lig);
      }
      const int cnt = (int) ((p1 - base) < (O) G ? (p1 - base) : (O) G);
      int j = 0;
      for (; j + 4 <= cnt; j += 4) {
        const int64_t k0 = __shfl(c, j, G), k1 = __shfl(c, j + 1, G), k2 = __shfl(c, j + 2, G), k3 = __shfl(c, j + 3, G);
        const C2 a0 = cshfl(v, j, G), a1 = cshfl(v, j + 1, G), a2 = cshfl(v, j + 2, G), a3 = cshfl(v, j + 3, G);
        if (active) {
          C2 b0[V], b1[V], b2[V], b3[V];
          cload_vec<R, V>(Bc + k0 * ldb, b0);
          cload_vec<R, V>(Bc + k1 * ldb, b1);
          cload_vec<R, V>(Bc + k2 * ldb, b2);
          cload_vec<R, V>(Bc + k3 * ldb, b3);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            cmac<CA, CB>(acc[i], a0, b0[i]);
            cmac<CA, CB>(acc[i], a1, b1[i]);
            cmac<CA, CB>(acc[i], a2, b2[i]);
            cmac<CA, CB>(acc[i], a3, b3[i]);
          }
        }
      }
      for (; j < cnt; ++j) {
        const int64_t k0 = __shfl(c, j, G);
        const C2 a0 = cshfl(v, j, G);
        if (active) {
          C2 b0[V];
          cload_vec<R, V>(Bc + k0 * ldb, b0);
#pragma unroll
          for (int i = 0; i < V; ++i)
            cmac<CA, CB>(acc[i], a0, b0[i]);
        }
      }
    }
    if (active) {
      typename cplx<R>::mem* cp = C + row * ldc + col0;
      C2 old[V];
      if (beta0) {
#pragma unroll
        for (int i = 0; i < V; ++i)
          old[i] = czero<C2>();
      } else {
        cload_vec<R, V>(cp, old);
      }
      C2 out[V];
#pragma unroll
      for (int i = 0; i < V; ++i)
        out[i] = cfinish(alpha, acc[i], beta, &old[i]);
      cstore_vec<R, V>(cp, out);
    }
  }
}

// Dense operands of any layout: element (i, j) at i*rs + j*cs (spmm_strided_kernel of spmm.hip, complex).  G lanes per
// row, JT output columns per tile in registers, group reduction by shuffles, lane j % G writes column j of the tile.
template <typename R, typename O, int JT, bool CA, bool CB>
__global__ __launch_bounds__(256) void cspmm_strided_kernel(int64_t m, int64_t n, const O* __restrict__ rowptr,
                                                            const int32_t* __restrict__ colind,
                                                            const typename cplx<R>::mem* __restrict__ values,
                                                            const typename cplx<R>::mem* __restrict__ B, int64_t brs,
                                                            int64_t bcs, typename cplx<R>::mem* __restrict__ C, int64_t crs,
                                                            int64_t ccs, typename cplx<R>::reg alpha,
                                                            typename cplx<R>::reg beta, int G, int long_len) {
  typedef typename cplx<R>::reg C2;
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
    C2 acc[JT];
#pragma unroll
    for (int j = 0; j < JT; ++j)
      acc[j] = czero<C2>();
    for (O p = p0 + lig; p < p1; p += G) {
      const int64_t c = colind[p];
      const C2 v = (C2) values[p];
      const typename cplx<R>::mem* __restrict__ bp = B + c * brs + j0 * bcs;
#pragma unroll
      for (int j = 0; j < JT; ++j)
        if (j0 + j < n)
          cmac<CA, CB>(acc[j], v, (C2) bp[j * bcs]);
    }
#pragma unroll
    for (int j = 0; j < JT; ++j)
      acc[j] = cgroup_sum(acc[j], G);
    if (mine) {
#pragma unroll
      for (int j = 0; j < JT; ++j)
        if (lig == (j % G) && j0 + j < n) {
          typename cplx<R>::mem* cp = C + row * crs + (j0 + j) * ccs;
          const C2 old = beta.x != 0 || beta.y != 0 ? (C2) *cp : czero<C2>();
          *cp = cfinish(alpha, acc[j], beta, &old);
        }
    }
  }
}

// Workgroup (i, part) sums entries [lo, hi) of long row i for all n columns into part_buf[(i*parts + part)*n ..]
// (spmm_long_rows_kernel of spmm.hip, complex, B along its strides).
template <typename R, typename O, bool CA, bool CB>
__global__ __launch_bounds__(256) void cspmm_long_rows_kernel(const int32_t* __restrict__ long_rows, int parts, int64_t n,
                                                              const O* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                              const typename cplx<R>::mem* __restrict__ values,
                                                              const typename cplx<R>::mem* __restrict__ B, int64_t brs,
                                                              int64_t bcs, typename cplx<R>::reg* __restrict__ part_buf) {
  typedef typename cplx<R>::reg C2;
  __shared__ C2 red[256];
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
  C2* out = part_buf + ((int64_t) i * parts + part) * n;
  for (int64_t c0 = 0; c0 < n; c0 += cpp) {
    const bool col_ok = e < eg && c0 + j < n;
    C2 acc = czero<C2>();
    if (col_ok) {
      const typename cplx<R>::mem* Bc = B + (c0 + j) * bcs;
      O p = lo + (O) e;
      for (; p + (O) (3 * eg) < hi; p += (O) (4 * eg)) {  // four gathers in flight
        const int64_t k0 = colind[p], k1 = colind[p + eg], k2 = colind[p + 2 * eg], k3 = colind[p + 3 * eg];
        const C2 b0 = (C2) Bc[k0 * brs], b1 = (C2) Bc[k1 * brs], b2 = (C2) Bc[k2 * brs], b3 = (C2) Bc[k3 * brs];
        cmac<CA, CB>(acc, (C2) values[p], b0);
        cmac<CA, CB>(acc, (C2) values[p + eg], b1);
        cmac<CA, CB>(acc, (C2) values[p + 2 * eg], b2);
        cmac<CA, CB>(acc, (C2) values[p + 3 * eg], b3);
      }
      for (; p < hi; p += (O) eg)
        cmac<CA, CB>(acc, (C2) values[p], (C2) Bc[(int64_t) colind[p] * brs]);
    }
    __syncthreads();
    red[threadIdx.x] = acc;
    __syncthreads();
    if (e == 0 && c0 + j < n) {
      C2 sum = red[j];
      for (int g = 1; g < eg; ++g) {
        sum.x += red[g * cpp + j].x;
        sum.y += red[g * cpp + j].y;
      }
      out[c0 + j] = sum;
    }
  }
}

// C[row] = alpha * (parts in order) + beta * C[row] for every long row
template <typename R>
__global__ __launch_bounds__(256) void cspmm_long_finish_kernel(const int32_t* __restrict__ long_rows, int parts, int64_t n,
                                                                const typename cplx<R>::reg* __restrict__ part_buf,
                                                                typename cplx<R>::mem* __restrict__ C, int64_t crs,
                                                                int64_t ccs, typename cplx<R>::reg alpha,
                                                                typename cplx<R>::reg beta) {
  typedef typename cplx<R>::reg C2;
  const int64_t i = blockIdx.x;
  const int64_t r = long_rows[i];
  for (int64_t j = threadIdx.x; j < n; j += 256) {
    C2 sum = czero<C2>();
    for (int q = 0; q < parts; ++q) {
      sum.x += part_buf[((int64_t) i * parts + q) * n + j].x;
      sum.y += part_buf[((int64_t) i * parts + q) * n + j].y;
    }
    typename cplx<R>::mem* cp = C + r * crs + j * ccs;
    const C2 old = beta.x != 0 || beta.y != 0 ? (C2) *cp : czero<C2>();
    *cp = cfinish(alpha, sum, beta, &old);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// ROWBLOCK window of a complex plan (spmv.hip: plan_build picks it by value_type through complex_window): 2 * WIN products
// of 8 / 16 bytes = 16 KiB of LDS, the budget of the real kernels.
template <typename R>
struct cwindow_of {
  static constexpr int value = sizeof(R) == 4 ? 1024 : 512;
};

int complex_window(int value_type) {
  return value_type == SPBLAS_GFX950_C32 ? cwindow_of<float>::value : cwindow_of<double>::value;
}

static int cpick_lpr(int64_t m, int64_t nnz) {  // spmv.hip: pick_lpr
  const double avg = m > 0 ? (double) nnz / (double) m : 0.0;
  int lpr = 2;
  while (lpr < 64 && (double) lpr * 1.5 < avg)
    lpr <<= 1;
  return lpr;
}

template <typename R>
static typename cplx<R>::reg host_scalar(const void* p) {
  const R* s = static_cast<const R*>(p);
  typename cplx<R>::reg c;
  c.x = s[0];
  c.y = s[1];
  return c;
}

template <typename R, typename O, bool CA, bool CX>
static int cspmv_typed(spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int64_t m, int64_t nnz, const void* alpha_p,
                       const void* rowptr_p, const int32_t* colind, const void* values_p, const void* x_p, const void* beta_p,
                       void* y_p) {
  typedef typename cplx<R>::reg C2;
  typedef typename cplx<R>::mem CM;
  const C2 alpha = host_scalar<R>(alpha_p), beta = host_scalar<R>(beta_p);
  const O* rowptr = static_cast<const O*>(rowptr_p);
  const CM* values = static_cast<const CM*>(values_p);
  const CM* x = static_cast<const CM*>(x_p);
  CM* y = static_cast<CM*>(y_p);
  hipStream_t s = h->stream;
  if (m == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  if (nnz == 0) {
    hipLaunchKernelGGL((cscale_kernel<R>), dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, (int64_t) 1, y, (int64_t) 1,
                       (int64_t) 1, beta);
    SPB_HIP(hipGetLastError());
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  constexpr int WIN = cwindow_of<R>::value;
  if (pl && pl->alg == SPBLAS_GFX950_SPMV_ROWBLOCK && pl->win == WIN) {
    pl->last_stream = s;  // part_head / part_tail are the plan's
    pl->used = true;
    C2* ph = static_cast<C2*>(pl->part_head);
    C2* pt = static_cast<C2*>(pl->part_tail);
    if (pl->n_long > 0) {
      hipLaunchKernelGGL((cspmv_rowblock_kernel<R, O, WIN, true, CA, CX>), dim3((unsigned) pl->nwin), dim3(256), 0, s, nnz,
                         rowptr, colind, values, x, y, alpha, beta, pl->win_row, ph, pt);
      hipLaunchKernelGGL((cspmv_long_fixup_kernel<R, O>), dim3((unsigned) pl->n_long), dim3(64), 0, s, pl->n_long, pl->win,
                         pl->long_rows, rowptr, ph, pt, y, alpha, beta);
    } else {
      hipLaunchKernelGGL((cspmv_rowblock_kernel<R, O, WIN, false, CA, CX>), dim3((unsigned) pl->nwin), dim3(256), 0, s, nnz,
                         rowptr, colind, values, x, y, alpha, beta, pl->win_row, ph, pt);
    }
    SPB_HIP(hipGetLastError());
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  const int lpr = pl ? pl->vector_lpr : cpick_lpr(m, nnz);
#define SPB_CVEC(L)                                                                                                            \
  hipLaunchKernelGGL((cspmv_vector_kernel<R, O, L, CA, CX>), dim3((unsigned) cdiv(m, 256 / L)), dim3(256), 0, s, m, rowptr,   \
                     colind, values, x, y, alpha, beta)
  switch (lpr) {
  case 2: SPB_CVEC(2); break;
  case 4: SPB_CVEC(4); break;
  case 8: SPB_CVEC(8); break;
  case 16: SPB_CVEC(16); break;
  case 32: SPB_CVEC(32); break;
  default: SPB_CVEC(64); break;
  }
#undef SPB_CVEC
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

template <typename R, typename O, bool CA, bool CB>
static int cspmm_typed(spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int64_t m, int64_t n, int64_t nnz,
                       const void* alpha_p, const void* rowptr_p, const int32_t* colind, const void* values_p, const void* B_p,
                       int64_t brs, int64_t bcs, const void* beta_p, void* C_p, int64_t crs, int64_t ccs) {
  typedef typename cplx<R>::reg C2;
  typedef typename cplx<R>::mem CM;
  const C2 alpha = host_scalar<R>(alpha_p), beta = host_scalar<R>(beta_p);
  const O* rowptr = static_cast<const O*>(rowptr_p);
  const CM* values = static_cast<const CM*>(values_p);
  const CM* B = static_cast<const CM*>(B_p);
  CM* C = static_cast<CM*>(C_p);
  hipStream_t s = h->stream;
  if (m == 0 || n == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  if (nnz == 0) {
    hipLaunchKernelGGL((cscale_kernel<R>), dim3((unsigned) cdiv(m * n, 256)), dim3(256), 0, s, m, n, C, crs, ccs, beta);
    SPB_HIP(hipGetLastError());
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  // a plan's long-row list: rows longer than its window are cut into parts of ~4 K entries (at most 64 per row) over
  // many workgroups instead of serialising on one lane group; the partial rows live in the plan (grown on demand)
  const int long_len = pl && pl->n_long > 0 ? pl->win : 0;
  if (long_len > 0) {
    int64_t parts = cdiv(pl->max_row_len, 4096);
    parts = parts < 1 ? 1 : (parts > 64 ? 64 : parts);
    const int64_t need = pl->n_long * parts * n * 2;  // (in units of R: a complex partial is two)
    if (pl->mm_long_cap < need || pl->mm_long_parts != (int) parts) {
      if (stream_capturing(s))  // the first call with this many columns has to run outside the capture
        return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
      dev_free(pl->mm_long_part, s);
      pl->mm_long_part = nullptr;
      pl->mm_long_cap = 0;
      int rc = dev_alloc(&pl->mm_long_part, (size_t) need * sizeof(R), s);
      if (rc)
        return rc;
      pl->mm_long_cap = need;
      pl->mm_long_parts = (int) parts;
    }
    pl->last_stream = s;
    pl->used = true;
  }
  if (ccs == 1 && bcs == 1) {
    // layout_right: 16-byte gathers when B and C allow them
    int V = 1;
    if constexpr (sizeof(R) == 4) {
      const uintptr_t bits = (uintptr_t) B | (uintptr_t) C;
      if (n % 2 == 0 && brs % 2 == 0 && crs % 2 == 0 && (bits % 16) == 0)
        V = 2;
    }
    int G = 1;
    while (G < 64 && (int64_t) G * V < n)
      G <<= 1;
    const unsigned grid = (unsigned) cdiv(m, 256 / G);
    if constexpr (sizeof(R) == 4) {
      if (V == 2)
        hipLaunchKernelGGL((cspmm_rowgroup_kernel<R, O, 2, CA, CB>), dim3(grid), dim3(256), 0, s, m, n, rowptr, colind, values,
                           B, brs, C, crs, alpha, beta, G, long_len);
      else
        hipLaunchKernelGGL((cspmm_rowgroup_kernel<R, O, 1, CA, CB>), dim3(grid), dim3(256), 0, s, m, n, rowptr, colind, values,
                           B, brs, C, crs, alpha, beta, G, long_len);
    } else {
      hipLaunchKernelGGL((cspmm_rowgroup_kernel<R, O, 1, CA, CB>), dim3(grid), dim3(256), 0, s, m, n, rowptr, colind, values, B,
                         brs, C, crs, alpha, beta, G, long_len);
    }
  } else {
    int G = 2;
    const int64_t avg = nnz / m;
    while (G < 64 && G < avg)
      G <<= 1;
    constexpr int JT = 8;
    const int64_t tiles = cdiv(n, JT);
    hipLaunchKernelGGL((cspmm_strided_kernel<R, O, JT, CA, CB>), dim3((unsigned) cdiv(m, 256 / G), (unsigned) (tiles < 64 ? tiles : 64)),
                       dim3(256), 0, s, m, n, rowptr, colind, values, B, brs, bcs, C, crs, ccs, alpha, beta, G, long_len);
  }
  if (long_len > 0) {
    C2* part = static_cast<C2*>(pl->mm_long_part);
    hipLaunchKernelGGL((cspmm_long_rows_kernel<R, O, CA, CB>), dim3((unsigned) pl->n_long, (unsigned) pl->mm_long_parts),
                       dim3(256), 0, s, pl->long_rows, pl->mm_long_parts, n, rowptr, colind, values, B, brs, bcs, part);
    hipLaunchKernelGGL((cspmm_long_finish_kernel<R>), dim3((unsigned) pl->n_long), dim3(256), 0, s, pl->long_rows,
                       pl->mm_long_parts, n, part, C, crs, ccs, alpha, beta);
  }
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

// conj_flags (0..3) and the offset type resolved to template arguments
template <typename R, typename O>
static int cspmv_conj(spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int flags, int64_t m, int64_t nnz, const void* alpha,
                      const void* rowptr, const int32_t* colind, const void* values, const void* x, const void* beta, void* y) {
  switch (flags) {
  case 0: return cspmv_typed<R, O, false, false>(h, pl, m, nnz, alpha, rowptr, colind, values, x, beta, y);
  case 1: return cspmv_typed<R, O, true, false>(h, pl, m, nnz, alpha, rowptr, colind, values, x, beta, y);
  case 2: return cspmv_typed<R, O, false, true>(h, pl, m, nnz, alpha, rowptr, colind, values, x, beta, y);
  default: return cspmv_typed<R, O, true, true>(h, pl, m, nnz, alpha, rowptr, colind, values, x, beta, y);
  }
}

template <typename R, typename O>
static int cspmm_conj(spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int flags, int64_t m, int64_t n, int64_t nnz,
                      const void* alpha, const void* rowptr, const int32_t* colind, const void* values, const void* B,
                      int64_t brs, int64_t bcs, const void* beta, void* C, int64_t crs, int64_t ccs) {
  switch (flags) {
  case 0: return cspmm_typed<R, O, false, false>(h, pl, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C, crs, ccs);
  case 1: return cspmm_typed<R, O, true, false>(h, pl, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C, crs, ccs);
  case 2: return cspmm_typed<R, O, false, true>(h, pl, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C, crs, ccs);
  default: return cspmm_typed<R, O, true, true>(h, pl, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C, crs, ccs);
  }
}

} // namespace spb

using namespace spb;

extern "C" int spblas_gfx950_spmv_conj(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int op, int64_t m, int64_t n,
                                       int64_t nnz, const void* alpha, const void* rowptr, const int32_t* colind,
                                       const void* values, const void* x, const void* beta, void* y, int offset_type,
                                       int value_type, int conj_flags) {
  if (is_lowp_type(value_type))  // (16-bit values: spblas_gfx950_spmv)
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (conj_flags < 0 || conj_flags > 3)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (!is_complex_type(value_type)) {
    if (conj_flags != 0)
      return SPBLAS_GFX950_STATUS_INVALID_VALUE;
    return spblas_gfx950_spmv(handle, plan, op, m, n, nnz, alpha, rowptr, colind, values, x, beta, y, offset_type, value_type);
  }
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (m < 0 || n < 0 || nnz < 0 || m > INT32_MAX || n > INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if (offset_type == SPBLAS_GFX950_I32 && nnz > INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if ((op != SPBLAS_GFX950_OP_N && op != SPBLAS_GFX950_OP_T) ||
      (offset_type != SPBLAS_GFX950_I32 && offset_type != SPBLAS_GFX950_I64))
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (op != SPBLAS_GFX950_OP_N)  // (csc_view / transposed() complex operands: not implemented)
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!alpha || !beta || !rowptr || (nnz > 0 && (!colind || !values)) || (m > 0 && !y) || (n > 0 && nnz > 0 && !x))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (plan && (plan->m != m || plan->n != n || plan->nnz != nnz || plan->rowptr != rowptr || plan->colind != colind ||
               plan->offset_type != offset_type || plan->value_type != value_type))
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  if (value_type == SPBLAS_GFX950_C32)
    return offset_type == SPBLAS_GFX950_I32
               ? cspmv_conj<float, int32_t>(handle, plan, conj_flags, m, nnz, alpha, rowptr, colind, values, x, beta, y)
               : cspmv_conj<float, int64_t>(handle, plan, conj_flags, m, nnz, alpha, rowptr, colind, values, x, beta, y);
  return offset_type == SPBLAS_GFX950_I32
             ? cspmv_conj<double, int32_t>(handle, plan, conj_flags, m, nnz, alpha, rowptr, colind, values, x, beta, y)
             : cspmv_conj<double, int64_t>(handle, plan, conj_flags, m, nnz, alpha, rowptr, colind, values, x, beta, y);
}

extern "C" int spblas_gfx950_spmm_strided_conj(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int64_t m, int64_t k,
                                               int64_t n, int64_t nnz, const void* alpha, const void* rowptr,
                                               const int32_t* colind, const void* values, const void* B, int64_t brs,
                                               int64_t bcs, const void* beta, void* C, int64_t crs, int64_t ccs,
                                               int offset_type, int value_type, int conj_flags) {
  if (is_lowp_type(value_type))  // (16-bit values: spblas_gfx950_spmm_strided)
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (conj_flags < 0 || conj_flags > 3)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (!is_complex_type(value_type)) {
    if (conj_flags != 0)
      return SPBLAS_GFX950_STATUS_INVALID_VALUE;
    return spblas_gfx950_spmm_strided(handle, plan, m, k, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C, crs,
                                      ccs, offset_type, value_type);
  }
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (m < 0 || k < 0 || n < 0 || nnz < 0 || m > INT32_MAX || k > INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if (bcs == 1 && ccs == 1) {
    // both layout_right (spblas_gfx950_spmm_strided: an operand of at most one row gets the leading dimension n)
    if (k <= 1)
      brs = n > 1 ? n : 1;
    if (m <= 1)
      crs = n > 1 ? n : 1;
    if (brs < n || crs < n)
      return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  } else {
    const auto layout_ok = [n](int64_t rows, int64_t rs, int64_t cs) {
      return (cs == 1 && rs >= n) || (rs == 1 && cs >= rows) || rows <= 1 || n <= 1;
    };
    if (brs < 0 || bcs < 0 || crs < 0 || ccs < 0 || !layout_ok(k, brs, bcs) || !layout_ok(m, crs, ccs))
      return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  }
  if (offset_type == SPBLAS_GFX950_I32 && nnz > INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if (offset_type != SPBLAS_GFX950_I32 && offset_type != SPBLAS_GFX950_I64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (!alpha || !beta || !rowptr || (nnz > 0 && (!colind || !values || !B)) || (m > 0 && n > 0 && !C))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (plan && (plan->m != m || plan->n != k || plan->nnz != nnz || plan->rowptr != rowptr || plan->colind != colind ||
               plan->offset_type != offset_type || plan->value_type != value_type))
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  if (value_type == SPBLAS_GFX950_C32)
    return offset_type == SPBLAS_GFX950_I32
               ? cspmm_conj<float, int32_t>(handle, plan, conj_flags, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs,
                                            beta, C, crs, ccs)
               : cspmm_conj<float, int64_t>(handle, plan, conj_flags, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs,
                                            beta, C, crs, ccs);
  return offset_type == SPBLAS_GFX950_I32
             ? cspmm_conj<double, int32_t>(handle, plan, conj_flags, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs,
                                           beta, C, crs, ccs)
             : cspmm_conj<double, int64_t>(handle, plan, conj_flags, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs,
                                           beta, C, crs, ccs);
}
