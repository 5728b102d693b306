// What the solver-side inspects share (sptrsv, sptrsv_sweeps, ilu0, multicolor, gauss_seidel; not part of the ABI): the
// lanes-per-row rule and its dispatch, the grid of a grid-stride launch, the structure checks of a square CSR operand, the
// first argument checks of a create call and the owner of an inspect's temporary device buffers.
#pragma once

#include "common.hpp"

#include <algorithm>
#include <type_traits>

namespace spb {

// Lanes of one wavefront that own a row, from the mean row length.  Written once, in sptrsv.hip next to the plan it was made for
// (where tests/ladder_tt.py reads its steps): the plans and the plan-free sweeps call it with the same (m, nnz), which is what
// makes their bits agree.
int lanes_per_row(int64_t m, int64_t nnz);

// f(std::integral_constant<int, G>{}) for G = lanes: a generic lambda reads decltype(g)::value and launches kernel<T, G>.
template <typename F>
auto with_lanes(int lanes, F&& f) {
  switch (lanes) {
    case 4: return f(std::integral_constant<int, 4>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 64: return f(std::integral_constant<int, 64>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

inline int cu_count(const spblas_gfx950_handle_s* h) {
  return h->num_cus > 0 ? h->num_cus : 256;
}

// workgroups of 256 lanes of a grid-stride kernel over n items: at most 16 per CU, at least one
inline unsigned stride_grid(const spblas_gfx950_handle_s* h, int64_t n) {
  const int64_t cap = (int64_t) cu_count(h) * 16;
  return (unsigned) std::max<int64_t>(1, std::min(cap, cdiv(n, 256)));
}

// ---- structure checks of an m x m CSR operand.  flag[0] = 1 on a violation.
// row r's offsets p0 .. p1 lie in [0, nnz], ascend, start at 0 and end at nnz
__device__ __forceinline__ bool row_offsets_ok(int64_t r, int64_t m, int64_t nnz, int64_t p0, int64_t p1) {
  return p0 >= 0 && p0 <= p1 && p1 <= nnz && (r > 0 || p0 == 0) && (r + 1 < m || p1 == nnz);
}
static __global__ __launch_bounds__(256) void csr_check_rows_kernel(int64_t m, int64_t nnz, const int32_t* __restrict__ rowptr,
                                                                    int32_t* __restrict__ flag) {
  const int64_t r = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (r >= m)
    return;
  const int64_t p0 = rowptr[r], p1 = rowptr[r + 1];
  if (!row_offsets_ok(r, m, nnz, p0, p1))
    flag[0] = 1;
}
// ... every column lies in [0, m)
static __global__ __launch_bounds__(256) void csr_check_cols_kernel(int64_t m, int64_t nnz, const int32_t* __restrict__ colind,
                                                                    int32_t* __restrict__ flag) {
  bool bad = false;
  for (int64_t p = (int64_t) blockIdx.x * 256 + threadIdx.x; p < nnz; p += (int64_t) gridDim.x * 256) {
    const int c = colind[p];
    bad |= c < 0 || c >= m;
  }
  if (bad)
    flag[0] = 1;
}
// inv[] arrives filled with -1.  flag[0] = 1 when perm holds an index outside [0, m) or one index twice; else inv = perm^-1.
static __global__ __launch_bounds__(256) void check_perm_kernel(int64_t m, const int32_t* __restrict__ perm,
                                                                int32_t* __restrict__ inv, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= m)
    return;
  const int p = perm[i];
  if (p < 0 || p >= m || atomicCAS(inv + p, -1, (int) i) != -1)
    flag[0] = 1;
}

// flag[0] of the checks queued on the handle's stream: synchronises it; STATUS_INVALID_VALUE when one of them set the flag
inline int read_flag(spblas_gfx950_handle_s* h, const int32_t* flag) {
  int32_t bad = 0;
  SPB_HIP(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, h->stream));
  SPB_HIP(hipStreamSynchronize(h->stream));
  return bad != 0 ? SPBLAS_GFX950_STATUS_INVALID_VALUE : SPBLAS_GFX950_STATUS_SUCCESS;
}

// STATUS_INVALID_VALUE unless rowptr / colind describe an m x m matrix of nnz entries (or a check queued before on the same
// flag failed).  Synchronises the stream; flag = 16 zeroed device bytes of the caller's.
inline int check_csr_structure(spblas_gfx950_handle_s* h, int64_t m, int64_t nnz, const int32_t* rowptr, const int32_t* colind,
                               int32_t* flag) {
  hipStream_t s = h->stream;
  if (m > 0)
    hipLaunchKernelGGL(csr_check_rows_kernel, dim3((unsigned) cdiv(m, 256)), dim3(256), 0, s, m, nnz, rowptr, flag);
  if (nnz > 0)
    hipLaunchKernelGGL(csr_check_cols_kernel, dim3(stride_grid(h, nnz)), dim3(256), 0, s, m, nnz, colind, flag);
  SPB_HIP(hipGetLastError());
  return read_flag(h, flag);
}

// The first checks of every create call, in their documented order.  pointers_ok: the call's own pointer condition.
inline int inspect_args_status(const spblas_gfx950_handle_s* handle, bool pointers_ok, int64_t m, int64_t nnz) {
  if (!handle)
    return SPBLAS_GFX950_STATUS_INVALID_HANDLE;
  if (stream_capturing(handle->stream))  // inspect-class call: sizes its output on the host, never part of a graph
    return SPBLAS_GFX950_STATUS_NOT_SUPPORTED;
  if (!pointers_ok)
    return SPBLAS_GFX950_STATUS_INVALID_POINTER;
  if (m < 0 || nnz < 0 || m >= INT32_MAX || nnz > INT32_MAX)
    return SPBLAS_GFX950_STATUS_INVALID_SIZE;
  return SPBLAS_GFX950_STATUS_SUCCESS;
}

// The temporary device buffers of one inspect: whatever path the inspect leaves by, they are freed (in stream order) exactly
// once.  A failure path synchronises the stream before it returns, as the kernels may still be using them.
class dev_temps {
 public:
  explicit dev_temps(hipStream_t s) : s_(s) {}
  dev_temps(const dev_temps&) = delete;
  dev_temps& operator=(const dev_temps&) = delete;
  ~dev_temps() {
    for (int i = 0; i < n_; ++i)
      dev_free(p_[i], s_);
  }
  template <typename T>
  int alloc(T** p, size_t bytes) {
    *p = nullptr;
    if (n_ == kMax)  // (an inspect with more temporaries raises kMax)
      return SPBLAS_GFX950_STATUS_ALLOC_FAILED;
    void* q = nullptr;
    const int rc = dev_alloc(&q, bytes, s_);
    if (rc == SPBLAS_GFX950_STATUS_SUCCESS && q) {
      p_[n_++] = q;
      *p = static_cast<T*>(q);
    }
    return rc;
  }
  // the buffer moves into a plan: the caller owns it from here on
  template <typename T>
  T* release(T* p) {
    for (int i = 0; i < n_; ++i)
      if (p_[i] == p) {
        p_[i] = p_[--n_];
        break;
      }
    return p;
  }

 private:
  static constexpr int kMax = 20;
  hipStream_t s_;
  void* p_[kMax];
  int n_ = 0;
};

} // namespace spb
