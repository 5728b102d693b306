// Compile check of spblas::gfx950::gauss_seidel_inspect / gauss_seidel (include/spblas/vendor/gfx950/gauss_seidel_impl.hpp)
// INSIDE the reference tree, like dropin_permute_check.cpp: float and double, with and without perm, every direction, after
// multicolor_order on A itself and on the permuted B.  g++ -fsyntax-only: nothing is linked or run.  -DSPBLAS_GS_COMPLEX /
// -DSPBLAS_GS_SCALED / -DSPBLAS_GS_WIDE instead pass a complex matrix, a scaled view and 64-bit row offsets; each has to fail
// with "no matching function" (tests/test_gs_cpu.py).
#include <complex>
#include <cstdint>
#include <span>

#include <spblas/spblas.hpp>

using I = spblas::index_t;
using O = spblas::offset_t;

#if !defined(SPBLAS_GS_COMPLEX) && !defined(SPBLAS_GS_SCALED) && !defined(SPBLAS_GS_WIDE)
template <typename T>
std::int64_t gs_instantiations(spblas::csr_view<T, I, O> a, spblas::csr_view<T, I, O> pa, std::span<std::int32_t> perm,
                               std::span<std::int32_t> color_ptr, std::span<T> b, std::span<T> pb, std::span<T> x,
                               std::span<T> px) {
  using namespace spblas;
  operation_info_t order, on_a, on_b;
  gfx950::multicolor_order(order, a);
  gfx950::multicolor_copy(order, perm, {}, {}, color_ptr);
  gfx950::gauss_seidel_info_t gi = gfx950::gauss_seidel_inspect(on_a, a, color_ptr, perm);
  gfx950::gauss_seidel(on_a, a, b, x);
  gfx950::gauss_seidel(on_a, a, b, x, 2);
  gfx950::gauss_seidel(on_a, a, b, x, 2, T(1.5));
  gfx950::gauss_seidel(on_a, a, b, x, 1, T(1), gfx950::gs_direction::backward);
  gfx950::permute(a, perm, pa);
  gfx950::permute_vector<T>(perm, b, pb);
  gfx950::gauss_seidel_inspect(on_b, pa, color_ptr);
  gfx950::gauss_seidel(on_b, pa, pb, px, 1, T(1), gfx950::gs_direction::symmetric);
  gfx950::permute_vector<T>(perm, px, x, true);
  return gi.colors + gi.max_color_size + gi.lanes_per_row + gi.launches_per_forward_sweep;
}

template std::int64_t gs_instantiations<float>(spblas::csr_view<float, I, O>, spblas::csr_view<float, I, O>,
                                               std::span<std::int32_t>, std::span<std::int32_t>, std::span<float>,
                                               std::span<float>, std::span<float>, std::span<float>);
template std::int64_t gs_instantiations<double>(spblas::csr_view<double, I, O>, spblas::csr_view<double, I, O>,
                                                std::span<std::int32_t>, std::span<std::int32_t>, std::span<double>,
                                                std::span<double>, std::span<double>, std::span<double>);
#elif defined(SPBLAS_GS_COMPLEX)
void gs_complex(spblas::operation_info_t& info, spblas::csr_view<std::complex<float>, I, O> a,
                std::span<std::int32_t> color_ptr) {
  spblas::gfx950::gauss_seidel_inspect(info, a, color_ptr);
}
#elif defined(SPBLAS_GS_SCALED)
void gs_scaled(spblas::operation_info_t& info, spblas::csr_view<float, I, O> a, std::span<std::int32_t> color_ptr) {
  spblas::gfx950::gauss_seidel_inspect(info, spblas::scaled(2.0f, a), color_ptr);
}
#else
void gs_wide(spblas::operation_info_t& info, spblas::csr_view<float, I, std::int64_t> a, std::span<std::int32_t> color_ptr) {
  spblas::gfx950::gauss_seidel_inspect(info, a, color_ptr);
}
#endif
