// What the SpMV / SpMM entry points of spmv.hip, spmm.hip, lowp.hip and complex.hip share on the host (not part of the ABI):
// the lanes-per-row rule of the plan-free kernels and the predicates of the argument checks.  Only the PREDICATES are shared:
// the order in which an entry point reports its statuses is part of its behaviour (tests/test_gpu_value_family.py), so every
// entry keeps its own sequence of calls.
#pragma once

#include "common.hpp"
#include "plan.hpp"

namespace spb {

// Lanes of one wavefront that own a row in the vector kernels, from the mean row length.  Written once, in spmv.hip (where
// tests/ladder.py describes its steps): a plan records it (vector_lpr) and the plan-free paths of every value type call it
// with the same (m, nnz).
int pick_lpr(int64_t m, int64_t nnz);

// The plan was made for this matrix: same shape and entry count, same offset and column arrays, same index and value types.
inline bool plan_matches(const spblas_gfx950_plan_s& pl, int64_t m, int64_t n, int64_t nnz, const void* rowptr,
                         const int32_t* colind, int offset_type, int value_type) {
  return pl.m == m && pl.n == n && pl.nnz == nnz && pl.rowptr == rowptr && pl.colind == colind &&
         pl.offset_type == offset_type && pl.value_type == value_type;
}

// The CSR arrays a multiply reads are there: the offsets always, columns and values when the matrix has entries.
inline bool csr_arrays_ok(int64_t nnz, const void* rowptr, const int32_t* colind, const void* values) {
  return rowptr && (nnz == 0 || (colind && values));
}

// Leading dimension of a layout_right operand of `rows` rows and n columns.  A layout_left mdspan with ONE row also has
// strides (1, 1): its row stride says nothing -- an operand of at most one row gets the leading dimension n.
inline int64_t one_row_ld(int64_t rows, int64_t n, int64_t rs) {
  return rows <= 1 ? (n > 1 ? n : 1) : rs;
}

// A rows x n operand with element (i, j) at i*rs + j*cs is layout_right (column stride 1, rows >= n apart) or layout_left
// (row stride 1, columns >= rows apart); with one row or one column any strides do.
inline bool dense_layout_ok(int64_t rows, int64_t n, int64_t rs, int64_t cs) {
  return (cs == 1 && rs >= n) || (rs == 1 && cs >= rows) || rows <= 1 || n <= 1;
}

// The dense operands of spmm_strided, B (k x n) and C (m x n).  Both layout_right: the row strides are leading dimensions
// (one_row_ld applied to both, in place) and must reach n; otherwise no stride is negative and each operand is one of the
// two layouts.  false: STATUS_INVALID_SIZE.
inline bool spmm_strides_ok(int64_t m, int64_t k, int64_t n, int64_t& brs, int64_t bcs, int64_t& crs, int64_t ccs) {
  if (bcs == 1 && ccs == 1) {
    brs = one_row_ld(k, n, brs);
    crs = one_row_ld(m, n, crs);
    return brs >= n && crs >= n;
  }
  return brs >= 0 && bcs >= 0 && crs >= 0 && ccs >= 0 && dense_layout_ok(k, n, brs, bcs) && dense_layout_ok(m, n, crs, ccs);
}

} // namespace spb
