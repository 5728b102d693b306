// 16-bit SpMV / SpMM for gfx950 (IEEE binary16 = f16, bfloat16 = bf16; A's values, x / B and y / C share one type):
//   y = alpha * A * x + beta * y,   C = alpha * A * B + beta * C
// with float alpha / beta.  Every product and sum is formed in fp32 (a product of two 16-bit values is exact in fp32);
// beta * y is added in fp32 too, and each output element is rounded to the 16-bit type ONCE, round-to-nearest-even
// (v_cvt_pk_bf16_f32 / v_cvt_f16_f32): NaN stays NaN, an f16 result beyond the format's range becomes +-inf.  beta == 0:
// y is not read.  Nothing is accumulated in 16 bits and no 16-bit atomics are used (global_atomic_pk_add_bf16 rounds on
// every add); partial sums of long rows are fp32 and are added in a fixed order, so a plan gives the same bits every time.
//
// The kernels and their launchers are those of value_kernels.hpp, shared with complex.hip (HBM-bound; algorithmic bytes per
// entry = 4 + 2, per row sizeof(O) + 2, per column 2).  This file holds what is particular to 16-bit values: the two
// conversions, the row-block window, the value policy lp_values<T> the kernels are instantiated with, and the entry points
// with their own order of checks.
#include "value_kernels.hpp"

#include "lowp_api.hpp"

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

// ROWBLOCK window of a 16-bit plan (spmv.hip: plan_build picks it through lowp_window): 2 * WIN fp32 products = 16 KiB
// of LDS, the budget of the real kernels.
constexpr int LOWP_WIN = 2048;

int lowp_window() {
  return LOWP_WIN;
}

// The value policy of value_kernels.hpp: raw 16-bit words in memory, fp32 in registers (CA / CB: nothing to conjugate).
template <typename T>
struct lp_values {
  typedef uint16_t mem;
  typedef uint16_t out;
  typedef uint16_t raw;  // the row-block kernel keeps the words as loaded through its gather and converts at the product
  typedef float acc;
  typedef float scalar;
  typedef float word;  // a plan counts its long-row partials in floats
  static constexpr int acc_words = 1;
  static constexpr int window = LOWP_WIN;
  static constexpr int wide = 8;  // 8 values per 16-byte access

  static float host_scalar(const void* p) { return *static_cast<const float*>(p); }

  __device__ __forceinline__ static float zero() { return 0.0f; }
  __device__ __forceinline__ static float load(const uint16_t* p) { return lp<T>::to(*p); }
  __device__ __forceinline__ static float stream(const uint16_t* p) { return lp<T>::to(stream_load(p)); }
  __device__ __forceinline__ static float add(float a, float b) { return a + b; }
  template <bool CA, bool CB>
  __device__ __forceinline__ static void mac(float& s, float a, float b) {
    s = __builtin_fmaf(a, b, s);
  }

  __device__ __forceinline__ static uint16_t raw_zero() { return 0; }
  __device__ __forceinline__ static uint16_t stream_raw(const uint16_t* p) { return stream_load(p); }
  __device__ __forceinline__ static uint16_t load_raw(const uint16_t* p) { return *p; }
  // a plain multiply, no FMA onto +0: a product can be -0
  template <bool CA, bool CB>
  __device__ __forceinline__ static float stage(uint16_t a, uint16_t b) {
    return lp<T>::to(a) * lp<T>::to(b);
  }

  __device__ __forceinline__ static float shfl(float v, int src, int width) { return __shfl(v, src, width); }
  __device__ __forceinline__ static float group_sum(float v, int width) { return spb::group_sum(v, width); }
  template <int WIDTH>
  __device__ __forceinline__ static float group_sum_c(float v) {
    return spb::group_sum_c<WIDTH>(v);
  }

  __device__ __forceinline__ static bool nonzero(float beta) { return beta != 0.0f; }
  // alpha * s (+ beta * old when beta != 0), rounded once
  __device__ __forceinline__ static uint16_t finish(float alpha, float s, float beta, float old) {
    return lp<T>::from(beta != 0.0f ? __builtin_fmaf(beta, old, alpha * s) : alpha * s);
  }
  // ... on y[i] in place (beta == 0: y[i] is not read, NaN in y does not propagate)
  __device__ __forceinline__ static void update(uint16_t* y, int64_t i, float alpha, float s, float beta) {
    uint16_t* p = y + i;
    float r = alpha * s;
    if (beta != 0.0f)
      r = __builtin_fmaf(beta, lp<T>::to(*p), r);
    *p = lp<T>::from(r);
  }
  // *p = beta * *p as an FMA onto 0 * 0: beta * (-0) comes out +0
  __device__ __forceinline__ static void scale(float beta, uint16_t* p) { update(p, 0, 0.0f, 0.0f, beta); }

  template <int V>
  __device__ __forceinline__ static void load_vec(const uint16_t* p, float (&out)[V]) {
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
  __device__ __forceinline__ static void store_vec(uint16_t* p, const uint16_t (&in)[V]) {
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
};

// the value and offset types resolved to template arguments
template <typename O>
static int lspmv_values(int value_type, spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int64_t m, int64_t nnz,
                        const void* alpha, const void* rowptr, const int32_t* colind, const void* values, const void* x,
                        const void* beta, void* y) {
  return value_type == SPBLAS_GFX950_BF16
             ? vk_spmv<lp_values<bf16_tag>, O, false, false>(h, pl, m, nnz, alpha, rowptr, colind, values, x, beta, y)
             : vk_spmv<lp_values<f16_tag>, O, false, false>(h, pl, m, nnz, alpha, rowptr, colind, values, x, beta, y);
}

template <typename O>
static int lspmm_values(int value_type, spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int64_t m, int64_t n, int64_t nnz,
                        const void* alpha, const void* rowptr, const int32_t* colind, const void* values, const void* B,
                        int64_t brs, int64_t bcs, const void* beta, void* C, int64_t crs, int64_t ccs) {
  return value_type == SPBLAS_GFX950_BF16
             ? vk_spmm<lp_values<bf16_tag>, O, false, false>(h, pl, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta,
                                                             C, crs, ccs)
             : vk_spmm<lp_values<f16_tag>, O, false, false>(h, pl, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta,
                                                            C, crs, ccs);
}

int lowp_spmv(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int op, int64_t m, int64_t n, int64_t nnz,
              const void* alpha, const void* rowptr, const int32_t* colind, const void* values, const void* x,
              const void* beta, void* y, int offset_type, int value_type) {
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
  if (!alpha || !beta || !csr_arrays_ok(nnz, rowptr, colind, values) || (m > 0 && !y) || (n > 0 && nnz > 0 && !x))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (plan && !plan_matches(*plan, m, n, nnz, rowptr, colind, offset_type, value_type))
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  return offset_type == SPBLAS_GFX950_I32
             ? lspmv_values<int32_t>(value_type, handle, plan, m, nnz, alpha, rowptr, colind, values, x, beta, y)
             : lspmv_values<int64_t>(value_type, handle, plan, m, nnz, alpha, rowptr, colind, values, x, beta, y);
}

int lowp_spmm_strided(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int64_t m, int64_t k, int64_t n, int64_t nnz,
                      const void* alpha, const void* rowptr, const int32_t* colind, const void* values, const void* B,
                      int64_t brs, int64_t bcs, const void* beta, void* C, int64_t crs, int64_t ccs, int offset_type,
                      int value_type) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (m < 0 || k < 0 || n < 0 || nnz < 0 || m > INT32_MAX || k > INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if (!spmm_strides_ok(m, k, n, brs, bcs, crs, ccs))
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if (offset_type == SPBLAS_GFX950_I32 && nnz > INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  if (offset_type != SPBLAS_GFX950_I32 && offset_type != SPBLAS_GFX950_I64)
    return SPBLAS_GFX950_STATUS_INVALID_VALUE;
  if (!alpha || !beta || !csr_arrays_ok(nnz, rowptr, colind, values) || (nnz > 0 && !B) || (m > 0 && n > 0 && !C))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (plan && !plan_matches(*plan, m, k, nnz, rowptr, colind, offset_type, value_type))
    return SPBLAS_GFX950_STATUS_PLAN_MISMATCH;
  return offset_type == SPBLAS_GFX950_I32
             ? lspmm_values<int32_t>(value_type, handle, plan, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C,
                                     crs, ccs)
             : lspmm_values<int64_t>(value_type, handle, plan, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C,
                                     crs, ccs);
}

} // namespace spb
