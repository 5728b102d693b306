// Compile check of spblas::gfx950::ilu0_inspect / ilu0 / ilu0_status (include/spblas/vendor/gfx950/ilu0_impl.hpp) INSIDE the
// reference tree, like dropin_check.cpp: float and double, with and without info, in place and out of place, and the two
// triangular solves on the one LU view.  g++ -fsyntax-only: nothing is linked or run.  -DSPBLAS_ILU0_COMPLEX /
// -DSPBLAS_ILU0_SCALED / -DSPBLAS_ILU0_WIDE instead pass a complex matrix, a scaled view and 64-bit row offsets; each has to
// fail with "no matching function" (tests/test_ilu0_cpu.py).
#include <complex>
#include <cstdint>
#include <span>

#include <spblas/spblas.hpp>

using I = spblas::index_t;
using O = spblas::offset_t;

#if !defined(SPBLAS_ILU0_COMPLEX) && !defined(SPBLAS_ILU0_SCALED) && !defined(SPBLAS_ILU0_WIDE)
template <typename T>
std::int64_t ilu0_instantiations(spblas::csr_view<T, I, O> a, spblas::csr_view<T, I, O> lu, std::span<T> b, std::span<T> y,
                                 std::span<T> x) {
  using namespace spblas;
  operation_info_t info = gfx950::ilu0_inspect(a);
  gfx950::ilu0_inspect(info, a);
  gfx950::ilu0(info, a, lu);
  gfx950::ilu0(a, lu);
  gfx950::ilu0(info, a, a);  // in place
  triangular_solve(lu, lower_triangle_t{}, implicit_unit_diagonal_t{}, b, y);
  triangular_solve(lu, upper_triangle_t{}, explicit_diagonal_t{}, y, x);
  return gfx950::ilu0_status(info);
}

template std::int64_t ilu0_instantiations<float>(spblas::csr_view<float, I, O>, spblas::csr_view<float, I, O>,
                                                 std::span<float>, std::span<float>, std::span<float>);
template std::int64_t ilu0_instantiations<double>(spblas::csr_view<double, I, O>, spblas::csr_view<double, I, O>,
                                                  std::span<double>, std::span<double>, std::span<double>);
#elif defined(SPBLAS_ILU0_COMPLEX)
void ilu0_complex(spblas::csr_view<std::complex<float>, I, O> a) {
  spblas::gfx950::ilu0(a, a);
}
#elif defined(SPBLAS_ILU0_SCALED)
void ilu0_scaled(spblas::csr_view<float, I, O> a) {
  spblas::gfx950::ilu0(spblas::scaled(2.0f, a), a);
}
#else
void ilu0_wide(spblas::csr_view<float, I, std::int64_t> a) {
  spblas::gfx950::ilu0(a, a);
}
#endif
