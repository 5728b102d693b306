// Compile check of the complex SpMV / SpMM overloads of the drop-in headers (include/spblas/vendor/gfx950/complex_impl.hpp)
// INSIDE the reference tree, like dropin_check.cpp: the call shapes of the reference's test/gtest/conjugate_test.cpp
// (SpMV with conjugated(a) / conjugated(b), SpMM with conjugated(a) / conjugated(B)) on std::complex<float>, and the
// multiply_inspect / matrix_opt / scaled / layout_left / int64-offset / std::complex<double> variants.
// g++ -fsyntax-only: nothing is linked or run.  -DSPBLAS_COMPLEX_SPGEMM / -DSPBLAS_COMPLEX_MIXED instead
// instantiate a complex multiply_compute and a complex A times a real B; each has to fail with "no matching function"
// (tests/test_complex_cpu.py).
#include <complex>
#include <cstdint>
#include <span>
#include <vector>

#include <spblas/spblas.hpp>

using I = spblas::index_t;
using O = spblas::offset_t;

#if !defined(SPBLAS_COMPLEX_SPGEMM) && !defined(SPBLAS_COMPLEX_MIXED)
template <typename T, typename Off>
void complex_instantiations(spblas::csr_view<T, I, Off> a, std::vector<T>& b, std::vector<T>& c, T* b_data, T* c_data,
                            I m, I k, I n) {
  using namespace spblas;
  // conjugate_test.cpp:52 / :77 -- SpMV, matrix or vector conjugated
  multiply(conjugated(a), b, c);
  multiply(a, conjugated(b), c);
  multiply(conjugated(a), conjugated(b), c);
  // conjugate_test.cpp:106 / :139 -- SpMM, matrix or dense operand conjugated
  mdspan_row_major<T, I> B(b_data, k, n);
  mdspan_row_major<T, I> C(c_data, m, n);
  multiply(conjugated(a), B, C);
  multiply(a, conjugated(B), C);
  // scaled factors on either side of a conjugated view
  const T s(0.5, 2.0);
  multiply(scaled(s, conjugated(a)), b, c);
  multiply(conjugated(scaled(s, a)), scaled(s, b), c);
  multiply(scaled(s, a), conjugated(scaled(s, B)), C);
  // inspected and matrix_opt operands
  operation_info_t info = multiply_inspect(conjugated(a), b, c);
  multiply(info, conjugated(a), b, c);
  matrix_opt a_opt(a);
  operation_info_t info_opt = multiply_inspect(a_opt, b, c);
  multiply(info_opt, conjugated(a_opt), b, c);
  operation_info_t info_mm = multiply_inspect(a, B, C);
  multiply(info_mm, conjugated(a), B, C);
  // layout_left dense operands
  mdspan_col_major<T, I> Bl(b_data, k, n);
  mdspan_col_major<T, I> Cl(c_data, m, n);
  multiply(a, conjugated(Bl), Cl);
  multiply(conjugated(a), B, Cl);
}

template void complex_instantiations<std::complex<float>, O>(spblas::csr_view<std::complex<float>, I, O>,
                                                            std::vector<std::complex<float>>&, std::vector<std::complex<float>>&,
                                                            std::complex<float>*, std::complex<float>*, I, I, I);
template void complex_instantiations<std::complex<double>, O>(spblas::csr_view<std::complex<double>, I, O>,
                                                             std::vector<std::complex<double>>&,
                                                             std::vector<std::complex<double>>&, std::complex<double>*,
                                                             std::complex<double>*, I, I, I);
template void complex_instantiations<std::complex<float>, std::int64_t>(
    spblas::csr_view<std::complex<float>, I, std::int64_t>, std::vector<std::complex<float>>&,
    std::vector<std::complex<float>>&, std::complex<float>*, std::complex<float>*, I, I, I);
template void complex_instantiations<std::complex<double>, std::int64_t>(
    spblas::csr_view<std::complex<double>, I, std::int64_t>, std::vector<std::complex<double>>&,
    std::vector<std::complex<double>>&, std::complex<double>*, std::complex<double>*, I, I, I);
#elif defined(SPBLAS_COMPLEX_SPGEMM)
// complex SpGEMM is out of scope: the overload must not match (no error inside the backend headers)
void complex_spgemm(spblas::csr_view<std::complex<float>, I, O> a, spblas::csr_view<std::complex<float>, I, O> b,
                    spblas::csr_view<std::complex<float>, I, O> c) {
  spblas::operation_info_t info = spblas::multiply_compute(a, b, c);
  (void) info;
}
#else
// a complex matrix with a real dense operand: no overload matches
void complex_mixed(spblas::csr_view<std::complex<float>, I, O> a, double* b_data, std::complex<float>* c_data, I m, I k) {
  spblas::mdspan_row_major<double, I> B(b_data, k, 4);
  spblas::mdspan_row_major<std::complex<float>, I> C(c_data, m, 4);
  spblas::multiply(a, B, C);
}
#endif
