// Compile check of spblas::gfx950::aggregate / aggregate_copy / prolongator / coarsen_inspect / coarsen_structure / coarsen
// (include/spblas/vendor/gfx950/aggregate_impl.hpp) INSIDE the reference tree, like dropin_permute_check.cpp: float and double,
// with and without theta, and the pairing with multicolor_order / gauss_seidel on the coarse matrix and with the transposed
// SpMV that restricts a residual.  g++ -fsyntax-only: nothing is linked or run.  -DSPBLAS_AGGREGATE_COMPLEX /
// -DSPBLAS_AGGREGATE_SCALED / -DSPBLAS_AGGREGATE_WIDE instead pass a complex matrix, a scaled view and 64-bit row offsets; each
// has to fail with "no matching function" (tests/test_aggregate_dropin_cpu.py).
#include <complex>
#include <cstdint>
#include <span>

#include <spblas/spblas.hpp>
#include <spblas/algorithms/transposed.hpp>  // not pulled in by spblas.hpp when a vendor backend is selected

using I = spblas::index_t;
using O = spblas::offset_t;

#if !defined(SPBLAS_AGGREGATE_COMPLEX) && !defined(SPBLAS_AGGREGATE_SCALED) && !defined(SPBLAS_AGGREGATE_WIDE)
template <typename T>
std::int64_t aggregate_instantiations(spblas::csr_view<T, I, O> a, spblas::csr_view<T, I, O> p, spblas::csr_view<T, I, O> a_c,
                                      std::span<std::int32_t> agg, std::span<std::int32_t> root, std::span<std::int32_t> perm,
                                      std::span<std::int32_t> color_ptr, std::span<T> r, std::span<T> r_c, std::span<T> e_c) {
  using namespace spblas;
  operation_info_t ag, cz, order, gs;
  gfx950::aggregate_info_t ai = gfx950::aggregate(ag, a);
  ai = gfx950::aggregate(ag, a, 0.25);
  gfx950::aggregate_copy(ag, agg, root);
  gfx950::aggregate_copy(ag, agg, {});
  gfx950::prolongator(ag, p);
  gfx950::coarsen_info_t ci = gfx950::coarsen_inspect(cz, a, agg, ai.aggregates);
  gfx950::coarsen_structure(cz, a_c);
  gfx950::coarsen(cz, a, a_c);
  gfx950::multicolor_order(order, a_c);
  gfx950::multicolor_copy(order, perm, {}, {}, color_ptr);
  gfx950::gauss_seidel_inspect(gs, a_c, color_ptr, perm);
  multiply(transposed(p), r, r_c);
  gfx950::gauss_seidel(gs, a_c, r_c, e_c, 4, T(1), gfx950::gs_direction::symmetric);
  multiply(p, e_c, r);
  return ai.aggregates + ai.rounds + ai.largest + ai.smallest + ai.singletons + ai.strong_entries + ai.lanes_per_row + ci.rows +
         ci.nnz;
}

template std::int64_t aggregate_instantiations<float>(spblas::csr_view<float, I, O>, spblas::csr_view<float, I, O>,
                                                      spblas::csr_view<float, I, O>, std::span<std::int32_t>,
                                                      std::span<std::int32_t>, std::span<std::int32_t>, std::span<std::int32_t>,
                                                      std::span<float>, std::span<float>, std::span<float>);
template std::int64_t aggregate_instantiations<double>(spblas::csr_view<double, I, O>, spblas::csr_view<double, I, O>,
                                                       spblas::csr_view<double, I, O>, std::span<std::int32_t>,
                                                       std::span<std::int32_t>, std::span<std::int32_t>, std::span<std::int32_t>,
                                                       std::span<double>, std::span<double>, std::span<double>);
#elif defined(SPBLAS_AGGREGATE_COMPLEX)
void aggregate_complex(spblas::csr_view<std::complex<float>, I, O> a) {
  spblas::operation_info_t info;
  spblas::gfx950::aggregate(info, a);
}
#elif defined(SPBLAS_AGGREGATE_SCALED)
void aggregate_scaled(spblas::csr_view<float, I, O> a, std::span<std::int32_t> agg) {
  spblas::operation_info_t info;
  spblas::gfx950::coarsen_inspect(info, spblas::scaled(2.0f, a), agg, 4);
}
#else
void aggregate_wide(spblas::csr_view<float, I, std::int64_t> a, spblas::csr_view<float, I, std::int64_t> a_c) {
  spblas::operation_info_t info;
  spblas::gfx950::coarsen(info, a, a_c);
}
#endif
