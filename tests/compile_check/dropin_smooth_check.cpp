// Compile check of spblas::gfx950::smooth_prolongator_inspect / smooth_prolongator_structure / smooth_prolongator
// (include/spblas/vendor/gfx950/smooth_impl.hpp) INSIDE the reference tree, like dropin_aggregate_check.cpp: float and double,
// with and without theta, after aggregate / aggregate_copy and before the transposed SpMV that restricts a residual.
// g++ -fsyntax-only: nothing is linked or run.  -DSPBLAS_SMOOTH_COMPLEX / -DSPBLAS_SMOOTH_SCALED / -DSPBLAS_SMOOTH_WIDE instead
// pass a complex matrix, a scaled view and 64-bit row offsets; each has to fail with "no matching function"
// (tests/test_smooth_dropin_cpu.py).
#include <complex>
#include <cstdint>
#include <span>

#include <spblas/spblas.hpp>
#include <spblas/algorithms/transposed.hpp>  // not pulled in by spblas.hpp when a vendor backend is selected

using I = spblas::index_t;
using O = spblas::offset_t;

#if !defined(SPBLAS_SMOOTH_COMPLEX) && !defined(SPBLAS_SMOOTH_SCALED) && !defined(SPBLAS_SMOOTH_WIDE)
template <typename T>
std::int64_t smooth_instantiations(spblas::csr_view<T, I, O> a, spblas::csr_view<T, I, O> p, std::span<std::int32_t> agg,
                                   std::span<T> r, std::span<T> r_c) {
  using namespace spblas;
  operation_info_t ag, sm;
  gfx950::aggregate_info_t ai = gfx950::aggregate(ag, a, 0.25);
  gfx950::aggregate_copy(ag, agg, {});
  gfx950::smooth_prolongator_info_t pi = gfx950::smooth_prolongator_inspect(sm, a, agg, ai.aggregates);
  gfx950::smooth_prolongator_structure(sm, p);
  gfx950::smooth_prolongator(sm, a, p, T(2) / T(3));
  gfx950::smooth_prolongator(sm, a, p, 0.5, 0.25);
  multiply(transposed(p), r, r_c);
  multiply(p, r_c, r);
  return pi.rows + pi.columns + pi.nnz;
}

template std::int64_t smooth_instantiations<float>(spblas::csr_view<float, I, O>, spblas::csr_view<float, I, O>,
                                                   std::span<std::int32_t>, std::span<float>, std::span<float>);
template std::int64_t smooth_instantiations<double>(spblas::csr_view<double, I, O>, spblas::csr_view<double, I, O>,
                                                    std::span<std::int32_t>, std::span<double>, std::span<double>);
#elif defined(SPBLAS_SMOOTH_COMPLEX)
void smooth_complex(spblas::csr_view<std::complex<float>, I, O> a, std::span<std::int32_t> agg) {
  spblas::operation_info_t info;
  spblas::gfx950::smooth_prolongator_inspect(info, a, agg, 4);
}
#elif defined(SPBLAS_SMOOTH_SCALED)
void smooth_scaled(spblas::csr_view<float, I, O> a, std::span<std::int32_t> agg) {
  spblas::operation_info_t info;
  spblas::gfx950::smooth_prolongator_inspect(info, spblas::scaled(2.0f, a), agg, 4);
}
#else
void smooth_wide(spblas::csr_view<float, I, std::int64_t> a, spblas::csr_view<float, I, std::int64_t> p) {
  spblas::operation_info_t info;
  spblas::gfx950::smooth_prolongator(info, a, p, 0.5f);
}
#endif
