// Compile check of spblas::gfx950::multicolor_order / multicolor_copy / permute_inspect / permute / permute_vector
// (include/spblas/vendor/gfx950/permute_impl.hpp) INSIDE the reference tree, like dropin_ilu0_check.cpp: float and double, with
// and without info, and the pairing with ilu0 and the two triangular solves on the permuted matrix.  g++ -fsyntax-only: nothing
// is linked or run.  -DSPBLAS_PERMUTE_COMPLEX / -DSPBLAS_PERMUTE_SCALED / -DSPBLAS_PERMUTE_WIDE instead pass a complex matrix, a
// scaled view and 64-bit row offsets; each has to fail with "no matching function" (tests/test_multicolor_cpu.py).
#include <complex>
#include <cstdint>
#include <span>

#include <spblas/spblas.hpp>

using I = spblas::index_t;
using O = spblas::offset_t;

#if !defined(SPBLAS_PERMUTE_COMPLEX) && !defined(SPBLAS_PERMUTE_SCALED) && !defined(SPBLAS_PERMUTE_WIDE)
template <typename T>
std::int64_t permute_instantiations(spblas::csr_view<T, I, O> a, spblas::csr_view<T, I, O> b, std::span<std::int32_t> perm,
                                    std::span<std::int32_t> inverse, std::span<std::int32_t> color,
                                    std::span<std::int32_t> color_ptr, std::span<T> rhs, std::span<T> pb, std::span<T> y,
                                    std::span<T> px, std::span<T> x) {
  using namespace spblas;
  operation_info_t order;
  gfx950::multicolor_info_t mc = gfx950::multicolor_order(order, a);
  gfx950::multicolor_copy(order, perm, inverse, color, color_ptr);
  gfx950::multicolor_copy(order, perm, {}, {}, {});
  operation_info_t info = gfx950::permute_inspect(a, perm, b);
  gfx950::permute_inspect(info, a, perm, b);
  gfx950::permute(info, a, perm, b);
  gfx950::permute(a, perm, b);
  gfx950::permute_vector<T>(perm, rhs, pb);
  gfx950::ilu0(b, b);
  triangular_solve(b, lower_triangle_t{}, implicit_unit_diagonal_t{}, pb, y);
  triangular_solve(b, upper_triangle_t{}, explicit_diagonal_t{}, y, px);
  gfx950::permute_vector<T>(perm, px, x, true);
  return mc.colors + mc.rounds + mc.max_color_size + mc.lanes_per_row;
}

template std::int64_t permute_instantiations<float>(spblas::csr_view<float, I, O>, spblas::csr_view<float, I, O>,
                                                    std::span<std::int32_t>, std::span<std::int32_t>, std::span<std::int32_t>,
                                                    std::span<std::int32_t>, std::span<float>, std::span<float>,
                                                    std::span<float>, std::span<float>, std::span<float>);
template std::int64_t permute_instantiations<double>(spblas::csr_view<double, I, O>, spblas::csr_view<double, I, O>,
                                                     std::span<std::int32_t>, std::span<std::int32_t>, std::span<std::int32_t>,
                                                     std::span<std::int32_t>, std::span<double>, std::span<double>,
                                                     std::span<double>, std::span<double>, std::span<double>);
#elif defined(SPBLAS_PERMUTE_COMPLEX)
void permute_complex(spblas::csr_view<std::complex<float>, I, O> a, spblas::csr_view<std::complex<float>, I, O> b,
                     std::span<std::int32_t> perm) {
  spblas::gfx950::permute(a, perm, b);
}
#elif defined(SPBLAS_PERMUTE_SCALED)
void permute_scaled(spblas::csr_view<float, I, O> a, spblas::csr_view<float, I, O> b, std::span<std::int32_t> perm) {
  spblas::gfx950::permute(spblas::scaled(2.0f, a), perm, b);
}
#else
void permute_wide(spblas::csr_view<float, I, std::int64_t> a, spblas::csr_view<float, I, std::int64_t> b,
                  std::span<std::int32_t> perm) {
  spblas::gfx950::permute(a, perm, b);
}
#endif
