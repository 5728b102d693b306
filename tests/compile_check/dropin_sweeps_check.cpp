// Compile check of spblas::gfx950::triangular_solve_sweeps (include/spblas/vendor/gfx950/triangular_solve_impl.hpp) INSIDE the
// reference tree, like dropin_ilu0_check.cpp: float and double, with and without info, both triangles and diagonal kinds, a
// scaled matrix and a scaled right-hand side, and an info that comes from triangular_solve_inspect.  g++ -fsyntax-only: nothing
// is linked or run.  -DSPBLAS_SWEEPS_COMPLEX / -DSPBLAS_SWEEPS_CSC instead pass a complex matrix and a csc_view; each has to
// fail with "no matching function" (tests/test_sweeps_cpu.py).
#include <complex>
#include <cstdint>
#include <span>

#include <spblas/spblas.hpp>

using I = spblas::index_t;
using O = spblas::offset_t;

#if !defined(SPBLAS_SWEEPS_COMPLEX) && !defined(SPBLAS_SWEEPS_CSC)
template <typename T>
void sweeps_instantiations(spblas::csr_view<T, I, O> a, std::span<T> b, std::span<T> y, std::span<T> x) {
  using namespace spblas;
  gfx950::triangular_solve_sweeps(a, lower_triangle_t{}, implicit_unit_diagonal_t{}, b, y, 3);
  gfx950::triangular_solve_sweeps(a, upper_triangle_t{}, explicit_diagonal_t{}, y, x, 3);
  operation_info_t info = triangular_solve_inspect(a, lower_triangle_t{}, explicit_diagonal_t{}, b, x);
  gfx950::triangular_solve_sweeps(info, a, lower_triangle_t{}, explicit_diagonal_t{}, b, x, 0);
  gfx950::triangular_solve_sweeps(info, scaled(T(2), a), upper_triangle_t{}, implicit_unit_diagonal_t{}, scaled(T(0.5), b), x, 5);
  operation_info_t fresh;
  gfx950::triangular_solve_sweeps(fresh, a, lower_triangle_t{}, explicit_diagonal_t{}, b, x, 2);
}

template void sweeps_instantiations<float>(spblas::csr_view<float, I, O>, std::span<float>, std::span<float>, std::span<float>);
template void sweeps_instantiations<double>(spblas::csr_view<double, I, O>, std::span<double>, std::span<double>,
                                            std::span<double>);
#elif defined(SPBLAS_SWEEPS_COMPLEX)
void sweeps_complex(spblas::csr_view<std::complex<float>, I, O> a, std::span<std::complex<float>> b,
                    std::span<std::complex<float>> x) {
  spblas::gfx950::triangular_solve_sweeps(a, spblas::lower_triangle_t{}, spblas::explicit_diagonal_t{}, b, x, 2);
}
#else
void sweeps_csc(spblas::csc_view<float, I, O> a, std::span<float> b, std::span<float> x) {
  spblas::gfx950::triangular_solve_sweeps(a, spblas::lower_triangle_t{}, spblas::explicit_diagonal_t{}, b, x, 2);
}
#endif
