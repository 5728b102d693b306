// Compile check of spblas::gfx950::ilu0_sweeps (include/spblas/vendor/gfx950/ilu0_impl.hpp) INSIDE the reference tree, like
// dropin_ilu0_check.cpp: float and double, with and without info, followed by the two approximate applies on the one LU view.
// g++ -fsyntax-only: nothing is linked or run.  -DSPBLAS_ILU0_SWEEPS_COMPLEX / -DSPBLAS_ILU0_SWEEPS_CSC instead pass a complex
// matrix and a csc_view; each has to fail with "no matching function" (tests/test_ilu0_sweeps_cpu.py).
#include <complex>
#include <cstdint>
#include <span>

#include <spblas/spblas.hpp>

using I = spblas::index_t;
using O = spblas::offset_t;

#if !defined(SPBLAS_ILU0_SWEEPS_COMPLEX) && !defined(SPBLAS_ILU0_SWEEPS_CSC)
template <typename T>
std::int64_t ilu0_sweeps_instantiations(spblas::csr_view<T, I, O> a, spblas::csr_view<T, I, O> lu, std::span<T> work,
                                        std::span<T> b, std::span<T> y, std::span<T> x) {
  using namespace spblas;
  operation_info_t info = gfx950::ilu0_inspect(a);
  gfx950::ilu0_sweeps(info, a, lu, work, 3);
  gfx950::ilu0_sweeps(a, lu, work, 2);
  gfx950::ilu0_sweeps(info, a, lu, std::span<T>{}, 1);  // one sweep needs no work array
  gfx950::triangular_solve_sweeps(lu, lower_triangle_t{}, implicit_unit_diagonal_t{}, b, y, 3);
  gfx950::triangular_solve_sweeps(lu, upper_triangle_t{}, explicit_diagonal_t{}, y, x, 3);
  return gfx950::ilu0_status(info);
}

template std::int64_t ilu0_sweeps_instantiations<float>(spblas::csr_view<float, I, O>, spblas::csr_view<float, I, O>,
                                                        std::span<float>, std::span<float>, std::span<float>,
                                                        std::span<float>);
template std::int64_t ilu0_sweeps_instantiations<double>(spblas::csr_view<double, I, O>, spblas::csr_view<double, I, O>,
                                                         std::span<double>, std::span<double>, std::span<double>,
                                                         std::span<double>);
#elif defined(SPBLAS_ILU0_SWEEPS_COMPLEX)
void ilu0_sweeps_complex(spblas::csr_view<std::complex<float>, I, O> a, spblas::csr_view<std::complex<float>, I, O> lu,
                         std::span<std::complex<float>> work) {
  spblas::gfx950::ilu0_sweeps(a, lu, work, 2);
}
#else
void ilu0_sweeps_csc(spblas::csc_view<float, I, O> a, spblas::csc_view<float, I, O> lu, std::span<float> work) {
  spblas::gfx950::ilu0_sweeps(a, lu, work, 2);
}
#endif
