// 16-bit value types (SPBLAS_GFX950_F16 / BF16): what the real entry points of spmv.hip / spmm.hip need from lowp.hip.
#pragma once

#include "spblas_gfx950.h"

namespace spb {

inline bool is_lowp_type(int value_type) {
  return value_type == SPBLAS_GFX950_F16 || value_type == SPBLAS_GFX950_BF16;
}

// ROWBLOCK window (entries) of a 16-bit plan: the row-block kernel stages fp32 products, so 2 * window of them fill the
// same 16 KiB of LDS as the real kernels'
int lowp_window();

// spblas_gfx950_spmv / spblas_gfx950_spmm_strided for F16 / BF16 (alpha / beta point at one float each)
int lowp_spmv(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int op, int64_t m, int64_t n, int64_t nnz,
              const void* alpha, const void* rowptr, const int32_t* colind, const void* values, const void* x,
              const void* beta, void* y, int offset_type, int value_type);
int lowp_spmm_strided(spblas_gfx950_handle_t handle, spblas_gfx950_plan_t plan, int64_t m, int64_t k, int64_t n, int64_t nnz,
                      const void* alpha, const void* rowptr, const int32_t* colind, const void* values, const void* B,
                      int64_t brs, int64_t bcs, const void* beta, void* C, int64_t crs, int64_t ccs, int offset_type,
                      int value_type);

} // namespace spb
