// Complex value types (SPBLAS_GFX950_C32 / C64): what the real entry points of spmv.hip / spmm.hip need from complex.hip.
#pragma once

#include "spblas_gfx950.h"

namespace spb {

inline bool is_complex_type(int value_type) {
  return value_type == SPBLAS_GFX950_C32 || value_type == SPBLAS_GFX950_C64;
}

// ROWBLOCK window (entries) of a complex plan: 2 * window complex products fill the same 16 KiB of LDS as the real kernels'
int complex_window(int value_type);

} // namespace spb
