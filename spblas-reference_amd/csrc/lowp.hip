// 16-bit SpMV / SpMM for gfx950 (IEEE binary16 = f16, bfloat16 = bf16; A's values, x / B and y / C share one type):
//   y = alpha * A * x + beta * y,   C = alpha * A * B + beta * C
// with float alpha / beta.  Every product and sum is formed in fp32 (a product of two 16-bit values is exact in fp32);
// beta * y is added in fp32 too, and each output element is rounded to the 16-bit type ONCE, round-to-nearest-even
// (v_cvt_pk_bf16_f32 / v_cvt_f16_f32): NaN stays NaN, an f16 result beyond the format's range becomes +-inf.  beta == 0:
// y is not read.  Nothing is accumulated in 16 bits and no 16-bit atomics are used (global_atomic_pk_add_bf16 rounds on
// every add); partial sums of long rows are fp32 and are added in a fixed order, so a plan gives the same bits every time.
//
// Kernels (HBM-bound; algorithmic bytes per entry = 4 + 2, per row sizeof(O) + 2, per column 2):
//   lspmv_vector_kernel     plan-free / VECTOR plan: a power-of-two group of lanes per row, fp32 group sums.
//   lspmv_rowblock_kernel   ROWBLOCK plan: one 256-thread workgroup per nnz window of the plan (lowp_window: the 2 * WIN
//                           fp32 products fit 16 KiB of LDS); rows longer than the window leave their slices in the plan's
//                           part_head / part_tail (fp32) and lspmv_long_fixup_kernel adds them up in window order.
//   lspmm_rowgroup_kernel   layout_right B and C: a group of G lanes per row, each lane one 16-byte load = 8 values of a B
//                           row per gather (2-byte loads when B / C are not 16-byte aligned or n is not a multiple of 8).
//   lspmm_strided_kernel    any other layout (layout_left, padded leading dimensions): element-wise gathers along the strides.
//   lspmm_long_rows_kernel  with a plan: rows longer than its window, cut into parts of ~4 K entries over many workgroups
//   lspmm_long_finish_kernel  (fp32 partial rows), then added in part order (the row kernels skip those rows).
// The real and complex kernels (spmv.hip, spmm.hip, complex.hip) are untouched; this file only adds code.
#include "common.hpp"
#include "lowp_api.hpp"
#include "plan.hpp"

namespace spb {

// The two formats, stored as raw 16-bit words (the caller's torch.float16 / torch.bfloat16 arrays).
struct f16_tag {};
struct bf16_tag {};

template <typename T>
struct lp;
template <>
struct lp<f16_tag> {
  __device__ __forceinline__ static float to(uint16_t h) { return (float) __builtin_bit_cast(_Float16, h); }
  __device__ __forceinline__ static uint16_t from(float f) { return __builtin_bit_cast(uint16_t, (_Float16) f); }
  // the two values of one 32-bit word (element 2i in the low half)
  __device__ __forceinline__ static float lo(uint32_t u) { return to((uint16_t) (u & 0xffffu)); }
  __device__ __forceinline__ static float hi(uint32_t u) { return to((uint16_t) (u >> 16)); }
};
template <>
struct lp<bf16_tag> {
  // bf16 -> fp32 is a 16-bit shift; fp32 -> bf16 rounds to nearest even (v_cvt_pk_bf16_f32)
  __device__ __forceinline__ static float to(uint16_t h) { return __uint_as_float((uint32_t) h << 16); }
  __device__ __forceinline__ static uint16_t from(float f) { return __builtin_bit_cast(uint16_t, (__bf16) f); }
  __device__ __forceinline__ static float lo(uint32_t u) { return __uint_as_float(u << 16); }
  __device__ __forceinline__ static float hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
};

// alpha * s (+ beta * old when beta != 0; beta == 0: old is not read, NaN in y does not propagate), rounded once
template <typename T>
__device__ __forceinline__ uint16_t lfinish(float alpha, float s, float beta, const uint16_t* old) {
  float r = alpha * s;
  if (beta != 0.0f)
    r = __builtin_fmaf(beta, lp<T>::to(*old), r);
  return lp<T>::from(r);
}

// ---------------------------------------------------------------------------------------------------------------------
// SpMV
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, typename O, int LPR>
__global__ __launch_bounds__(256) void lspmv_vector_kernel(int64_t m, const O* __restrict__ rowptr,
                                                           const int32_t* __restrict__ colind,
                                                           const uint16_t* __restrict__ values,
                                                           const uint16_t* __restrict__ x, uint16_t* __restrict__ y,
                                                           float alpha, float beta) {
  constexpr int ROWS = 256 / LPR;
  const int64_t row = (int64_t) blockIdx.x * ROWS + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  float s = 0.0f;
  if (row < m) {
    const O p0 = rowptr[row], p1 = rowptr[row + 1];
    for (O p = p0 + lane; p < p1; p += LPR)
      s = __builtin_fmaf(lp<T>::to(stream_load(values + p)), lp<T>::to(x[stream_load(colind + p)]), s);
  }
  s = group_sum_c<LPR>(s);
  if (row < m && lane == 0)
    y[row] = lfinish<T>(alpha, s, beta, y + row);
}

// Sum of values[p] * x[colind[p]] for p in [lo, hi) over the whole workgroup (valid in every thread).
template <typename T, typename O>
__device__ float block_segment_ldot(O lo, O hi, const int32_t* __restrict__ colind, const uint16_t* __restrict__ values,
                                    const uint16_t* __restrict__ x, float* red) {
  float s = 0.0f;
  for (O p = lo + (O) threadIdx.x; p < hi; p += 256)
    s = __builtin_fmaf(lp<T>::to(stream_load(values + p)), lp<T>::to(x[stream_load(colind + p)]), s);
  s = group_sum_c<64>(s);
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
    red[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// Window w owns the rows whose first entry lies in [w*WIN, (w+1)*WIN) (spmv.hip, spmv_rowblock_kernel): a row no longer
// than WIN ends before (w+2)*WIN, hence 2*WIN fp32 LDS slots; a longer row leaves its slice of this window in
// part_tail[w] (the window it starts in) or part_head[w] (later windows).
template <typename T, typename O, int WIN, bool HAS_LONG>
__global__ __launch_bounds__(256) void lspmv_rowblock_kernel(int64_t nnz, const O* __restrict__ rowptr,
                                                             const int32_t* __restrict__ colind,
                                                             const uint16_t* __restrict__ values,
                                                             const uint16_t* __restrict__ x, uint16_t* __restrict__ y,
                                                             float alpha, float beta, const int32_t* __restrict__ win_row,
                                                             float* __restrict__ part_head, float* __restrict__ part_tail) {
  constexpr int CAP = 2 * WIN;
  constexpr int ITERS = CAP / 256;
  static_assert(CAP % 256 == 0, "window must be a multiple of 128");
  static_assert(CAP * sizeof(float) <= 16384, "products must fit 16 KiB of LDS");
  __shared__ float prod[CAP];
  __shared__ float red[4];

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
        const float s = block_segment_ldot<T, O>(wlo, a < whi ? a : whi, colind, values, x, red);
        if (tid == 0)
          part_head[w] = s;
        __syncthreads();
      }
    }
    if (r_end > r_begin) {  // long row starting in this window (necessarily the last owned row)
      const O ls = rowptr[r_end - 1];
      if (e - ls > (O) WIN) {
        const float s = block_segment_ldot<T, O>(ls, whi, colind, values, x, red);
        if (tid == 0)
          part_tail[w] = s;
        __syncthreads();
        r_end -= 1;
        e = ls;
      }
    }
  }
  const int total = (int) (e - a);  // <= CAP

  // ---- phase 1: stream colind / values (all loads of the thread in flight together), gather x, stage fp32 products
  int32_t c[ITERS];
  uint16_t v[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int q = it * 256 + tid;
    c[it] = 0;
    v[it] = 0;
    if (q < total) {
      c[it] = stream_load(colind + a + q);
      v[it] = stream_load(values + a + q);
    }
  }
  uint16_t xv[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it)
    xv[it] = x[c[it]];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int q = it * 256 + tid;
    if (q < total)
      prod[q] = lp<T>::to(v[it]) * lp<T>::to(xv[it]);
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
    float s = 0.0f;
    for (int q = s0 + lig; q < s1; q += lpr)
      s += prod[q];
    s = group_sum(s, lpr);
    if (lig == 0)
      y[r] = lfinish<T>(alpha, s, beta, y + r);
  }
}

// One wavefront per long row: y[r] = alpha * (tail + heads) + beta * y[r].
template <typename T, typename O>
__global__ __launch_bounds__(64) void lspmv_long_fixup_kernel(int64_t n_long, int win, const int32_t* __restrict__ long_rows,
                                                              const O* __restrict__ rowptr, const float* __restrict__ part_head,
                                                              const float* __restrict__ part_tail, uint16_t* __restrict__ y,
                                                              float alpha, float beta) {
  const int64_t i = blockIdx.x;
  if (i >= n_long)
    return;
  const int r = long_rows[i];
  const int64_t p0 = (int64_t) rowptr[r], p1 = (int64_t) rowptr[r + 1];
  const int64_t w0 = p0 / win, w1 = (p1 - 1) / win;
  float s = 0.0f;
  for (int64_t w = w0 + 1 + threadIdx.x; w <= w1; w += 64)
    s += part_head[w];
  s = group_sum_c<64>(s);
  if (threadIdx.x == 0)
    y[r] = lfinish<T>(alpha, part_tail[w0] + s, beta, y + r);
}

// y = beta * y (A without entries); strided so that the same kernel serves C of SpMM
template <typename T>
__global__ __launch_bounds__(256) void lscale_kernel(int64_t rows, int64_t cols, uint16_t* __restrict__ y, int64_t rs,
                                                     int64_t cs, float beta) {
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i < rows * cols) {
    const int64_t r = i / cols, c = i % cols;
    uint16_t* p = y + r * rs + c * cs;
    *p = lfinish<T>(0.0f, 0.0f, beta, p);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// SpMM
// ---------------------------------------------------------------------------------------------------------------------
// V values of a B / C row per lane access: 8 (one 16-byte load) or 1
template <typename T, int V>
__device__ __forceinline__ void lload_vec(const uint16_t* p, float (&out)[V]) {
  if constexpr (V == 1) {
    out[0] = lp<T>::to(*p);
  } else {
    static_assert(V == 8, "8 values per 16-byte access");
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    out[0] = lp<T>::lo(q.x);
    out[1] = lp<T>::hi(q.x);
    out[2] = lp<T>::lo(q.y);
    out[3] = lp<T>::hi(q.y);
    out[4] = lp<T>::lo(q.z);
    out[5] = lp<T>::hi(q.z);
    out[6] = lp<T>::lo(q.w);
    out[7] = lp<T>::hi(q.w);
  }
}

template <int V>
__device__ __forceinline__ void lstore_vec(uint16_t* p, const uint16_t (&in)[V]) {
  if constexpr (V == 1) {
    *p = in[0];
  } else {
    uint4 q;
    q.x = (uint32_t) in[0] | ((uint32_t) in[1] << 16);
    q.y = (uint32_t) in[2] | ((uint32_t) in[3] << 16);
    q.z = (uint32_t) in[4] | ((uint32_t) in[5] << 16);
    q.w = (uint32_t) in[6] | ((uint32_t) in[7] << 16);
    *reinterpret_cast<uint4*>(p) = q;
  }
}

// Modelled on spmm_rowgroup_kernel (spmm.hip): G lanes per row walk its entries G at a time, the (column, value) pairs are
// handed round by shuffles, every lane accumulates V consecutive columns of C in fp32; panels of G*V columns.
// long_len > 0: rows longer than that belong to the long-row kernels.
template <typename T, typename O, int V>
__global__ __launch_bounds__(256) void lspmm_rowgroup_kernel(int64_t m, int64_t n, const O* __restrict__ rowptr,
                                                             const int32_t* __restrict__ colind,
                                                             const uint16_t* __restrict__ values,
                                                             const uint16_t* __restrict__ B, int64_t ldb,
                                                             uint16_t* __restrict__ C, int64_t ldc, float alpha, float beta,
                                                             int G, int long_len) {
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
  for (int64_t col0 = (int64_t) lig * V; col0 - (int64_t) lig * V < n; col0 += panel_cols) {
    const bool active = mine && col0 < n;
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i)
      acc[i] = 0.0f;
    const uint16_t* __restrict__ Bc = B + col0;
    for (O base = p0; base < p1; base += G) {
      int32_t c = 0;
      float v = 0.0f;
      if (base + lig < p1) {
        c = stream_load(colind + base + lig);
        v = lp<T>::to(stream_load(values + base + lig));
      }
      const int cnt = (int) ((p1 - base) < (O) G ? (p1 - base) : (O) G);
      int j = 0;
      for (; j + 4 <= cnt; j += 4) {
        const int64_t k0 = __shfl(c, j, G), k1 = __shfl(c, j + 1, G), k2 = __shfl(c, j + 2, G), k3 = __shfl(c, j + 3, G);
        const float a0 = __shfl(v, j, G), a1 = __shfl(v, j + 1, G), a2 = __shfl(v, j + 2, G), a3 = __shfl(v, j + 3, G);
        if (active) {
          float b0[V], b1[V], b2[V], b3[V];
          lload_vec<T, V>(Bc + k0 * ldb, b0);
          lload_vec<T, V>(Bc + k1 * ldb, b1);
          lload_vec<T, V>(Bc + k2 * ldb, b2);
          lload_vec<T, V>(Bc + k3 * ldb, b3);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            acc[i] = __builtin_fmaf(a0, b0[i], acc[i]);
            acc[i] = __builtin_fmaf(a1, b1[i], acc[i]);
            acc[i] = __builtin_fmaf(a2, b2[i], acc[i]);
            acc[i] = __builtin_fmaf(a3, b3[i], acc[i]);
          }
        }
      }
      for (; j < cnt; ++j) {
        const int64_t k0 = __shfl(c, j, G);
        const float a0 = __shfl(v, j, G);
        if (active) {
          float b0[V];
          lload_vec<T, V>(Bc + k0 * ldb, b0);
#pragma unroll
          for (int i = 0; i < V; ++i)
            acc[i] = __builtin_fmaf(a0, b0[i], acc[i]);
        }
      }
    }
    if (active) {
      uint16_t* cp = C + row * ldc + col0;
      float old[V];
      if (beta != 0.0f) {
        lload_vec<T, V>(cp, old);
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i)
          old[i] = 0.0f;
      }
      uint16_t out[V];
#pragma unroll
      for (int i = 0; i < V; ++i)
        out[i] = lp<T>::from(beta != 0.0f ? __builtin_fmaf(beta, old[i], alpha * acc[i]) : alpha * acc[i]);
      lstore_vec<V>(cp, out);
    }
  }
}

// Dense operands of any layout: element (i, j) at i*rs + j*cs (spmm_strided_kernel of spmm.hip, 16-bit).  G lanes per
// row, JT output columns per tile in fp32 registers, group reduction by shuffles, lane j % G writes column j of the tile.
template <typename T, typename O, int JT>
__global__ __launch_bounds__(256) void lspmm_strided_kernel(int64_t m, int64_t n, const O* __restrict__ rowptr,
                                                            const int32_t* __restrict__ colind,
                                                            const uint16_t* __restrict__ values,
                                                            const uint16_t* __restrict__ B, int64_t brs, int64_t bcs,
                                                            uint16_t* __restrict__ C, int64_t crs, int64_t ccs, float alpha,
                                                            float beta, int G, int long_len) {
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
    float acc[JT];
#pragma unroll
    for (int j = 0; j < JT; ++j)
      acc[j] = 0.0f;
    for (O p = p0 + lig; p < p1; p += G) {
      const int64_t c = colind[p];
      const float v = lp<T>::to(values[p]);
      const uint16_t* __restrict__ bp = B + c * brs + j0 * bcs;
#pragma unroll
      for (int j = 0; j < JT; ++j)
        if (j0 + j < n)
          acc[j] = __builtin_fmaf(v, lp<T>::to(bp[j * bcs]), acc[j]);
    }
#pragma unroll
    for (int j = 0; j < JT; ++j)
      acc[j] = group_sum(acc[j], G);
    if (mine) {
#pragma unroll
      for (int j = 0; j < JT; ++j)
        if (lig == (j % G) && j0 + j < n) {
          uint16_t* cp = C + row * crs + (j0 + j) * ccs;
          *cp = lfinish<T>(alpha, acc[j], beta, cp);
        }
    }
  }
}

// Workgroup (i, part) sums entries [lo, hi) of long row i for all n columns into part_buf[(i*parts + part)*n ..] in fp32
// (spmm_long_rows_kernel of spmm.hip, 16-bit, B along its strides).
template <typename T, typename O>
__global__ __launch_bounds__(256) void lspmm_long_rows_kernel(const int32_t* __restrict__ long_rows, int parts, int64_t n,
                                                              const O* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                              const uint16_t* __restrict__ values,
                                                              const uint16_t* __restrict__ B, int64_t brs, int64_t bcs,
                                                              float* __restrict__ part_buf) {
  __shared__ float red[256];
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
  float* out = part_buf + ((int64_t) i * parts + part) * n;
  for (int64_t c0 = 0; c0 < n; c0 += cpp) {
    const bool col_ok = e < eg && c0 + j < n;
    float acc = 0.0f;
    if (col_ok) {
      const uint16_t* Bc = B + (c0 + j) * bcs;
      O p = lo + (O) e;
      for (; p + (O) (3 * eg) < hi; p += (O) (4 * eg)) {  // four gathers in flight
        const int64_t k0 = colind[p], k1 = colind[p + eg], k2 = colind[p + 2 * eg], k3 = colind[p + 3 * eg];
        const float b0 = lp<T>::to(Bc[k0 * brs]), b1 = lp<T>::to(Bc[k1 * brs]), b2 = lp<T>::to(Bc[k2 * brs]),
                    b3 = lp<T>::to(Bc[k3 * brs]);
        acc = __builtin_fmaf(lp<T>::to(values[p]), b0, acc);
        acc = __builtin_fmaf(lp<T>::to(values[p + eg]), b1, acc);
        acc = __builtin_fmaf(lp<T>::to(values[p + 2 * eg]), b2, acc);
        acc = __builtin_fmaf(lp<T>::to(values[p + 3 * eg]), b3, acc);
      }
      for (; p < hi; p += (O) eg)
        acc = __builtin_fmaf(lp<T>::to(values[p]), lp<T>::to(Bc[(int64_t) colind[p] * brs]), acc);
    }
    __syncthreads();
    red[threadIdx.x] = acc;
    __syncthreads();
    if (e == 0 && c0 + j < n) {
      float sum = red[j];
      for (int g = 1; g < eg; ++g)
        sum += red[g * cpp + j];
      out[c0 + j] = sum;
    }
  }
}

// C[row] = alpha * (parts in order) + beta * C[row] for every long row
template <typename T>
__global__ __launch_bounds__(256) void lspmm_long_finish_kernel(const int32_t* __restrict__ long_rows, int parts, int64_t n,
                                                                const float* __restrict__ part_buf, uint16_t* __restrict__ C,
                                                                int64_t crs, int64_t ccs, float alpha, float beta) {
  const int64_t i = blockIdx.x;
  const int64_t r = long_rows[i];
  for (int64_t j = threadIdx.x; j < n; j += 256) {
    float sum = 0.0f;
    for (int q = 0; q < parts; ++q)
      sum += part_buf[((int64_t) i * parts + q) * n + j];
    uint16_t* cp = C + r * crs + j * ccs;
    *cp = lfinish<T>(alpha, sum, beta, cp);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// ROWBLOCK window of a 16-bit plan (spmv.hip: plan_build picks it through lowp_window): 2 * WIN fp32 products = 16 KiB
// of LDS, the budget of the real kernels.
constexpr int LOWP_WIN = 2048;

int lowp_window() {
  return LOWP_WIN;
}

static int lpick_lpr(int64_t m, int64_t nnz) {  // spmv.hip: pick_lpr
  const double avg = m > 0 ? (double) nnz / (double) m : 0.0;
  int lpr = 2;
  while (lpr < 64 && (double) lpr * 1.5 < avg)
    lpr <<= 1;
  return lpr;
}

template <typename T, typename O>
static int lspmv_typed(spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int64_t m, int64_t nnz, float alpha,
                       const void* rowptr_p, const int32_t* colind, const void* values_p, const void* x_p, float beta,
                       void* y_p) {
  const O* rowptr = static_cast<const O*>(rowptr_p);
  const uint16_t* values = static_cast<const uint16_t*>(values_p);
  const uint16_t* x = static_cast<const uint16_t*>(x_p);
  uint16_t* y = static_cast<uint16_t*>(y_p);
  hipStream_t s = h->stream;
  if (m == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  if (nnz == 0) {
    hipLaunchKernelGGL((lscale_kernel<T>), dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, (int64_t) 1, y, (int64_t) 1,
                       (int64_t) 1, beta);
    SPB_HIP(hipGetLastError());
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  if (pl && pl->alg == SPBLAS_GFX950_SPMV_ROWBLOCK && pl->win == LOWP_WIN) {
    pl->last_stream = s;  // part_head / part_tail are the plan's
    pl->used = true;
    float* ph = static_cast<float*>(pl->part_head);
    float* pt = static_cast<float*>(pl->part_tail);
    if (pl->n_long > 0) {
      hipLaunchKernelGGL((lspmv_rowblock_kernel<T, O, LOWP_WIN, true>), dim3((unsigned) pl->nwin), dim3(256), 0, s, nnz, rowptr,
                         colind, values, x, y, alpha, beta, pl->win_row, ph, pt);
      hipLaunchKernelGGL((lspmv_long_fixup_kernel<T, O>), dim3((unsigned) pl->n_long), dim3(64), 0, s, pl->n_long, pl->win,
                         pl->long_rows, rowptr, ph, pt, y, alpha, beta);
    } else {
      hipLaunchKernelGGL((lspmv_rowblock_kernel<T, O, LOWP_WIN, false>), dim3((unsigned) pl->nwin), dim3(256), 0, s, nnz,
                         rowptr, colind, values, x, y, alpha, beta, pl->win_row, ph, pt);
    }
    SPB_HIP(hipGetLastError());
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  const int lpr = pl ? pl->vector_lpr : lpick_lpr(m, nnz);
#define SPB_LVEC(L)                                                                                                            \
  hipLaunchKernelGGL((lspmv_vector_kernel<T, O, L>), dim3((unsigned) cdiv(m, 256 / L)), dim3(256), 0, s, m, rowptr, colind,    \
                     values, x, y, alpha, beta)
  switch (lpr) {
  case 2: SPB_LVEC(2); break;
  case 4: SPB_LVEC(4); break;
  case 8: SPB_LVEC(8); break;
  case 16: SPB_LVEC(16); break;
  case 32: SPB_LVEC(32); break;
  default: SPB_LVEC(64); break;
  }
#undef SPB_LVEC
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

template <typename T, typename O>
static int lspmm_typed(spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int64_t m, int64_t n, int64_t nnz, float alpha,
                       const void* rowptr_p, const int32_t* colind, const void* values_p, const void* B_p, int64_t brs,
                       int64_t bcs, float beta, void* C_p, int64_t crs, int64_t ccs) {
  const O* rowptr = static_cast<const O*>(rowptr_p);
  const uint16_t* values = static_cast<const uint16_t*>(values_p);
  const uint16_t* B = static_cast<const uint16_t*>(B_p);
  uint16_t* C = static_cast<uint16_t*>(C_p);
  hipStream_t s = h->stream;
  if (m == 0 || n == 0)
    return SPBLAS_GFX950_STATUS_SUCCESS;
  if (nnz == 0) {
    hipLaunchKernelGGL((lscale_kernel<T>), dim3((unsigned) cdiv(m * n, 256)), dim3(256), 0, s, m, n, C, crs, ccs, beta);
    SPB_HIP(hipGetLastError());
    return SPBLAS_GFX950_STATUS_SUCCESS;
  }
  // a plan's long-row list: rows longer than its window are cut into parts of ~4 K entries (at most 64 per row) over
  // many workgroups instead of serialising on one lane group; the fp32 partial rows live in the plan (grown on demand)
  const int long_len = pl && pl->n_long > 0 ? pl->win : 0;
  if (long_len > 0) {
    int64_t parts = cdiv(pl->max_row_len, 4096);
    parts = parts < 1 ? 1 : (parts > 64 ? 64 : parts);
    const int64_t need = pl->n_long * parts * n;  // (floats)
    if (pl->mm_long_cap < need || pl->mm_long_parts != (int) parts) {
      if (stream_capturing(s))  // the first call with this many columns has to run outside the capture
        return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
      dev_free(pl->mm_long_part, s);
      pl->mm_long_part = nullptr;
      pl->mm_long_cap = 0;
      int rc = dev_alloc(&pl->mm_long_part, (size_t) need * sizeof(float), s);
      if (rc)
        return rc;
      pl->mm_long_cap = need;
      pl->mm_long_parts = (int) parts;
    }
    pl->last_stream = s;
    pl->used = true;
  }
  if (ccs == 1 && bcs == 1) {
    // layout_right: 16-byte gathers (8 values) when B and C allow them
    const uintptr_t bits = (uintptr_t) B | (uintptr_t) C;
    const int V = (n % 8 == 0 && brs % 8 == 0 && crs % 8 == 0 && (bits % 16) == 0) ? 8 : 1;
    int G = 1;
    while (G < 64 && (int64_t) G * V < n)
      G <<= 1;
    const unsigned grid = (unsigned) cdiv(m, 256 / G);
    if (V == 8)
      hipLaunchKernelGGL((lspmm_rowgroup_kernel<T, O, 8>), dim3(grid), dim3(256), 0, s, m, n, rowptr, colind, values, B, brs, C,
                         crs, alpha, beta, G, long_len);
    else
      hipLaunchKernelGGL((lspmm_rowgroup_kernel<T, O, 1>), dim3(grid), dim3(256), 0, s, m, n, rowptr, colind, values, B, brs, C,
                         crs, alpha, beta, G, long_len);
  } else {
    int G = 2;
    const int64_t avg = nnz / m;
    while (G < 64 && G < avg)
      G <<= 1;
    constexpr int JT = 8;
    const int64_t tiles = cdiv(n, JT);
    hipLaunchKernelGGL((lspmm_strided_kernel<T, O, JT>), dim3((unsigned) cdiv(m, 256 / G), (unsigned) (tiles < 64 ? tiles : 64)),
                       dim3(256), 0, s, m, n, rowptr, colind, values, B, brs, bcs, C, crs, ccs, alpha, beta, G, long_len);
  }
  if (long_len > 0) {
    float* part = static_cast<float*>(pl->mm_long_part);
    hipLaunchKernelGGL((lspmm_long_rows_kernel<T, O>), dim3((unsigned) pl->n_long, (unsigned) pl->mm_long_parts), dim3(256), 0,
                       s, pl->long_rows, pl->mm_long_parts, n, rowptr, colind, values, B, brs, bcs, part);
    hipLaunchKernelGGL((lspmm_long_finish_kernel<T>), dim3((unsigned) pl->n_long), dim3(256), 0, s, pl->long_rows,
                       pl->mm_long_parts, n, part, C, crs, ccs, alpha, beta);
  }
  SPB_HIP(hipGetLastError());
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

int lowp_spmv(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int op, int64_t m, int64_t n, int64_t nnz,
              const void* alpha_p, const void* rowptr, const int32_t* colind, const void* values, const void* x,
              const void* beta_p, void* y, int offset_type, int value_type) {
  if (op == SPBLAS_GFX950_OP_T)  // (csc_view / transposed() 16-bit operands: not implemented)
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (m < 0 || n < 0 || nnz < 0 || m > INT32_MAX || n > INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if (offset_type == SPBLAS_GFX950_I32 && nnz > INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if (op != SPBLAS_GFX950_OP_N || (offset_type != SPBLAS_GFX950_I32 && offset_type != SPBLAS_GFX950_I64))
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (!alpha_p || !beta_p || !rowptr || (nnz > 0 && (!colind || !values)) || (m > 0 && !y) || (n > 0 && nnz > 0 && !x))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (plan && (plan->m != m || plan->n != n || plan->nnz != nnz || plan->rowptr != rowptr || plan->colind != colind ||
               plan->offset_type != offset_type || plan->value_type != value_type))
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  const float alpha = *static_cast<const float*>(alpha_p), beta = *static_cast<const float*>(beta_p);
  if (value_type == SPBLAS_GFX950_BF16)
    return offset_type == SPBLAS_GFX950_I32
               ? lspmv_typed<bf16_tag, int32_t>(handle, plan, m, nnz, alpha, rowptr, colind, values, x, beta, y)
               : lspmv_typed<bf16_tag, int64_t>(handle, plan, m, nnz, alpha, rowptr, colind, values, x, beta, y);
  return offset_type == SPBLAS_GFX950_I32
             ? lspmv_typed<f16_tag, int32_t>(handle, plan, m, nnz, alpha, rowptr, colind, values, x, beta, y)
             : lspmv_typed<f16_tag, int64_t>(handle, plan, m, nnz, alpha, rowptr, colind, values, x, beta, y);
}

int lowp_spmm_strided(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int64_t m, int64_t k, int64_t n, int64_t nnz,
                      const void* alpha_p, const void* rowptr, const int32_t* colind, const void* values, const void* B,
                      int64_t brs, int64_t bcs, const void* beta_p, void* C, int64_t crs, int64_t ccs, int offset_type,
                      int value_type) {
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
  if (!alpha_p || !beta_p || !rowptr || (nnz > 0 && (!colind || !values || !B)) || (m > 0 && n > 0 && !C))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (plan && (plan->m != m || plan->n != k || plan->nnz != nnz || plan->rowptr != rowptr || plan->colind != colind ||
               plan->offset_type != offset_type || plan->value_type != value_type))
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  const float alpha = *static_cast<const float*>(alpha_p), beta = *static_cast<const float*>(beta_p);
  if (value_type == SPBLAS_GFX950_BF16)
    return offset_type == SPBLAS_GFX950_I32
               ? lspmm_typed<bf16_tag, int32_t>(handle, plan, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C,
                                                crs, ccs)
               : lspmm_typed<bf16_tag, int64_t>(handle, plan, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C,
                                                crs, ccs);
  return offset_type == SPBLAS_GFX950_I32
             ? lspmm_typed<f16_tag, int32_t>(handle, plan, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C, crs,
                                             ccs)
             : lspmm_typed<f16_tag, int64_t>(handle, plan, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C, crs,
                                             ccs);
}

} // namespace spb
