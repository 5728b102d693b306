// Compile check of the triangular_solve / triangular_solve_inspect overloads for a block of right-hand sides
// (include/spblas/vendor/gfx950/triangular_solve_impl.hpp: matrix B, matrix X) INSIDE the reference tree, like
// dropin_check.cpp: row- and column-major mdspans in every combination, float and double, with and without info, a scaled
// A and a scaled B; the vector overloads next to them must stay unambiguous.
// g++ -fsyntax-only: nothing is linked or run.  -DSPBLAS_TRSM_COMPLEX / -DSPBLAS_TRSM_MIXED instead instantiate a complex
// block solve and a float matrix with a double right-hand side; each has to fail with "no matching function"
// (tests/test_sptrsm_cpu.py).
#include <complex>
#include <cstdint>
#include <span>

#include <spblas/spblas.hpp>

using I = spblas::index_t;
using O = spblas::offset_t;

#if !defined(SPBLAS_TRSM_COMPLEX) && !defined(SPBLAS_TRSM_MIXED)
template <typename T>
void trsm_instantiations(spblas::csr_view<T, I, O> a, T* b_data, T* x_data, std::span<T> b, std::span<T> x, I m, I n) {
  using namespace spblas;
  mdspan_row_major<T, I> Br(b_data, m, n), Xr(x_data, m, n);
  mdspan_col_major<T, I> Bl(b_data, m, n), Xl(x_data, m, n);
  operation_info_t info = triangular_solve_inspect(a, lower_triangle_t{}, explicit_diagonal_t{}, Br, Xr);
  triangular_solve_inspect(info, a, lower_triangle_t{}, explicit_diagonal_t{}, Bl, Xl);
  triangular_solve(info, a, lower_triangle_t{}, explicit_diagonal_t{}, Br, Xr);
  triangular_solve(info, a, lower_triangle_t{}, explicit_diagonal_t{}, Bl, Xl);
  triangular_solve(info, a, lower_triangle_t{}, explicit_diagonal_t{}, Br, Xl);
  triangular_solve(info, a, lower_triangle_t{}, explicit_diagonal_t{}, Bl, Xr);
  triangular_solve(a, upper_triangle_t{}, implicit_unit_diagonal_t{}, Br, Xr);
  triangular_solve(a, upper_triangle_t{}, implicit_unit_diagonal_t{}, Bl, Xl);
  triangular_solve(scaled(T(2), a), lower_triangle_t{}, explicit_diagonal_t{}, scaled(T(3), Br), Xr);
  triangular_solve(info, a, lower_triangle_t{}, explicit_diagonal_t{}, scaled(T(3), Bl), Xl);
  // one info serves the vector form as well, and the vector overloads still bind
  triangular_solve(info, a, lower_triangle_t{}, explicit_diagonal_t{}, b, x);
  triangular_solve(a, lower_triangle_t{}, explicit_diagonal_t{}, scaled(T(3), b), x);
}

template void trsm_instantiations<float>(spblas::csr_view<float, I, O>, float*, float*, std::span<float>, std::span<float>, I,
                                         I);
template void trsm_instantiations<double>(spblas::csr_view<double, I, O>, double*, double*, std::span<double>,
                                          std::span<double>, I, I);
#elif defined(SPBLAS_TRSM_COMPLEX)
// complex values are out of scope: the overload must not match (no error inside the backend headers)
void trsm_complex(spblas::csr_view<std::complex<float>, I, O> a, std::complex<float>* b_data, std::complex<float>* x_data, I m) {
  spblas::mdspan_row_major<std::complex<float>, I> B(b_data, m, 4), X(x_data, m, 4);
  spblas::triangular_solve(a, spblas::lower_triangle_t{}, spblas::explicit_diagonal_t{}, B, X);
}
#else
// a float matrix with a double right-hand side: no overload matches
void trsm_mixed(spblas::csr_view<float, I, O> a, double* b_data, float* x_data, I m) {
  spblas::mdspan_row_major<double, I> B(b_data, m, 4);
  spblas::mdspan_row_major<float, I> X(x_data, m, 4);
  spblas::triangular_solve(a, spblas::lower_triangle_t{}, spblas::explicit_diagonal_t{}, B, X);
}
#endif
