// Complex SpMV / SpMM for gfx950 (std::complex<float> = c32, std::complex<double> = c64, interleaved re / im):
//   y = alpha * op'(A) * x' + beta * y,   C = alpha * op'(A) * B' + beta * C
// where op' / ' conjugate A's values and / or x / B (conj_flags bit 0 / bit 1: conjugated_view in the reference,
// views/conjugated_view_impl.hpp).  The maths is the reference CPU path (algorithms/multiply_impl.hpp:33-92) on complex
// scalars, accumulated in the value type.  A product is the plain componentwise formula (ac - bd, ad + bc) as four FMAs, the
// conjugations folded in as sign flips at compile time; no C Annex G inf / NaN recovery.
//
// The kernels and their launchers are those of value_kernels.hpp, shared with lowp.hip (HBM-bound; algorithmic bytes per
// entry = 4 + s, s = 8 (c32) or 16 (c64), per row sizeof(O) + s, per column s; one 8- or 16-byte value load per entry, sums
// per component).  This file holds what is particular to complex values: the (re, im) arithmetic, the row-block windows, the
// value policy cplx_values<R> the kernels are instantiated with, and the entry points with their own order of checks.
#include "value_kernels.hpp"

#include "complex_api.hpp"
#include "lowp_api.hpp"

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

// V complex elements of B per lane and gather: c32 V = 2 (16 B), c64 V = 1 (16 B); c32 with a B / C that is not 16-byte
// aligned (odd n or leading dimension) V = 1.
template <typename R, int V>
struct cvec;
template <>
struct cvec<float, 2> {
  typedef float mem __attribute__((ext_vector_type(4), aligned(16)));
};

// ROWBLOCK window of a complex plan (spmv.hip: plan_build picks it by value_type through complex_window): 2 * WIN products
// of 8 / 16 bytes = 16 KiB of LDS, the budget of the real kernels.
template <typename R>
struct cwindow_of {
  static constexpr int value = sizeof(R) == 4 ? 1024 : 512;
};

int complex_window(int value_type) {
  return value_type == SPBLAS_GFX950_C32 ? cwindow_of<float>::value : cwindow_of<double>::value;
}

// The value policy of value_kernels.hpp: (re, im) of precision R, sums per component in R.
template <typename R>
struct cplx_values {
  typedef typename cplx<R>::mem mem;
  typedef typename cplx<R>::reg acc;
  typedef acc out;
  typedef acc raw;
  typedef acc scalar;
  typedef R word;  // a plan counts its long-row partials in units of R: a complex partial is two
  static constexpr int acc_words = 2;
  static constexpr int window = cwindow_of<R>::value;
  static constexpr int wide = sizeof(R) == 4 ? 2 : 1;

  static acc host_scalar(const void* p) {
    const R* s = static_cast<const R*>(p);
    acc c;
    c.x = s[0];
    c.y = s[1];
    return c;
  }

  __device__ __forceinline__ static acc zero() {
    acc z;
    z.x = 0;
    z.y = 0;
    return z;
  }
  __device__ __forceinline__ static acc load(const mem* p) { return (acc) *p; }
  // streaming (read-once) load of one value of A at the alignment of std::complex (common.hpp: stream_load)
  __device__ __forceinline__ static acc stream(const mem* p) { return __builtin_nontemporal_load(p); }
  __device__ __forceinline__ static acc add(acc a, const acc& b) {
    a.x += b.x;
    a.y += b.y;
    return a;
  }
  template <bool CA, bool CB>
  __device__ __forceinline__ static void mac(acc& s, const acc a, const acc b) {
    cmac<CA, CB>(s, a, b);
  }

  __device__ __forceinline__ static acc raw_zero() { return zero(); }
  __device__ __forceinline__ static acc stream_raw(const mem* p) { return stream(p); }
  __device__ __forceinline__ static acc load_raw(const mem* p) { return load(p); }
  // FMAs onto +0: no component of a product is -0 unless both of its terms are
  template <bool CA, bool CB>
  __device__ __forceinline__ static acc stage(const acc a, const acc b) {
    acc p = zero();
    cmac<CA, CB>(p, a, b);
    return p;
  }

  __device__ __forceinline__ static acc shfl(const acc v, int src, int width) {
    acc r;
    r.x = __shfl(v.x, src, width);
    r.y = __shfl(v.y, src, width);
    return r;
  }
  __device__ __forceinline__ static acc group_sum(acc v, int width) {
    v.x = spb::group_sum(v.x, width);
    v.y = spb::group_sum(v.y, width);
    return v;
  }
  template <int WIDTH>
  __device__ __forceinline__ static acc group_sum_c(acc v) {
    v.x = spb::group_sum_c<WIDTH>(v.x);
    v.y = spb::group_sum_c<WIDTH>(v.y);
    return v;
  }

  __device__ __forceinline__ static bool nonzero(const acc beta) { return beta.x != 0 || beta.y != 0; }
  // alpha * s, or alpha * s + beta * old when beta != 0
  __device__ __forceinline__ static acc finish(const acc alpha, const acc s, const acc beta, const acc old) {
    acc r = cmul(alpha, s);
    if (beta.x != 0 || beta.y != 0) {
      const acc b = cmul(beta, old);
      r.x += b.x;
      r.y += b.y;
    }
    return r;
  }
  // ... on y[i] in place (beta == 0: y[i] is not read, NaN in y does not propagate)
  __device__ __forceinline__ static void update(mem* y, int64_t i, const acc alpha, const acc s, const acc beta) {
    const acc old = beta.x != 0 || beta.y != 0 ? (acc) y[i] : zero();
    y[i] = finish(alpha, s, beta, old);
  }
  // *p = beta * *p, exact zero when beta is zero
  __device__ __forceinline__ static void scale(const acc beta, mem* p) {
    *p = beta.x != 0 || beta.y != 0 ? cmul(beta, (acc) *p) : zero();
  }

  template <int V>
  __device__ __forceinline__ static void load_vec(const mem* p, acc (&out)[V]) {
    if constexpr (V == 1) {
      out[0] = (acc) *p;
    } else {
      const typename cvec<R, 2>::mem q = *reinterpret_cast<const typename cvec<R, 2>::mem*>(p);
      out[0].x = q.x;
      out[0].y = q.y;
      out[1].x = q.z;
      out[1].y = q.w;
    }
  }
  template <int V>
  __device__ __forceinline__ static void store_vec(mem* p, const acc (&in)[V]) {
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
};

// conj_flags (0..3) and the offset type resolved to template arguments
template <typename R, typename O>
static int cspmv_conj(spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int flags, int64_t m, int64_t nnz, const void* alpha,
                      const void* rowptr, const int32_t* colind, const void* values, const void* x, const void* beta, void* y) {
  typedef cplx_values<R> VT;
  switch (flags) {
  case 0: return vk_spmv<VT, O, false, false>(h, pl, m, nnz, alpha, rowptr, colind, values, x, beta, y);
  case 1: return vk_spmv<VT, O, true, false>(h, pl, m, nnz, alpha, rowptr, colind, values, x, beta, y);
  case 2: return vk_spmv<VT, O, false, true>(h, pl, m, nnz, alpha, rowptr, colind, values, x, beta, y);
  default: return vk_spmv<VT, O, true, true>(h, pl, m, nnz, alpha, rowptr, colind, values, x, beta, y);
  }
}

template <typename R, typename O>
static int cspmm_conj(spblas_gfx950_handle_t h, spblas_gfx950_plan_s* pl, int flags, int64_t m, int64_t n, int64_t nnz,
                      const void* alpha, const void* rowptr, const int32_t* colind, const void* values, const void* B,
                      int64_t brs, int64_t bcs, const void* beta, void* C, int64_t crs, int64_t ccs) {
  typedef cplx_values<R> VT;
  switch (flags) {
  case 0: return vk_spmm<VT, O, false, false>(h, pl, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C, crs, ccs);
  case 1: return vk_spmm<VT, O, true, false>(h, pl, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C, crs, ccs);
  case 2: return vk_spmm<VT, O, false, true>(h, pl, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C, crs, ccs);
  default: return vk_spmm<VT, O, true, true>(h, pl, m, n, nnz, alpha, rowptr, colind, values, B, brs, bcs, beta, C, crs, ccs);
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
  if (!alpha || !beta || !csr_arrays_ok(nnz, rowptr, colind, values) || (m > 0 && !y) || (n > 0 && nnz > 0 && !x))
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (plan && !plan_matches(*plan, m, n, nnz, rowptr, colind, offset_type, value_type))
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
