// Host-only check of the complex operand rules of include/spblas/vendor/gfx950/complex_impl.hpp, compiled inside the
// reference tree like dropin_check.cpp and RUN on the CPU (nothing here touches a device or the library):
//   __gfx950::complex_scaling_factor  a scaled() factor is conjugated iff an odd number of conjugated views wrap it
//                                     (views/conjugated_view_impl.hpp), factors of A and x / B multiplied
//   __gfx950::conj_flags              bit 0 = A conjugated, bit 1 = x / B conjugated (parity rule of is_conjugated)
// Exit status 0 = every check held; otherwise the number of failed checks (each printed).
#include <complex>
#include <cstdio>
#include <vector>

#include <spblas/spblas.hpp>

using I = spblas::index_t;
using O = spblas::offset_t;

static int failures = 0;

template <typename T>
static void expect(const char* what, T got, T want) {
  if (got != want) {
    std::printf("FAIL %s: got (%g, %g), want (%g, %g)\n", what, (double) got.real(), (double) got.imag(), (double) want.real(),
                (double) want.imag());
    ++failures;
  }
}

static void expect_int(const char* what, int got, int want) {
  if (got != want) {
    std::printf("FAIL %s: got %d, want %d\n", what, got, want);
    ++failures;
  }
}

template <typename T>
static void run() {
  using namespace spblas;
  namespace g = spblas::__gfx950;
  spblas::csr_view<T, I, O> a(static_cast<T*>(nullptr), static_cast<O*>(nullptr), static_cast<I*>(nullptr), {0, 0}, 0);
  std::vector<T> x(4, T(1));
  const T s(0.5, 2.0), t(-1.0, 3.0), one(1, 0);
  std::vector<T> b_data(8, T(1));
  mdspan_row_major<T, I> B(b_data.data(), 2, 4);

  expect("no factors", g::complex_scaling_factor<T>(a, x), one);
  expect("scaled(s, A)", g::complex_scaling_factor<T>(scaled(s, a), x), s);
  expect("scaled(s, conjugated(A))", g::complex_scaling_factor<T>(scaled(s, conjugated(a)), x), s);
  expect("conjugated(scaled(s, A))", g::complex_scaling_factor<T>(conjugated(scaled(s, a)), x), std::conj(s));
  {  // (whatever chain conjugated(conjugated(...)) builds, the factor follows its parity)
    auto cc = conjugated(conjugated(scaled(s, a)));
    expect("conjugated(conjugated(scaled(s, A)))", g::complex_scaling_factor<T>(cc, x),
           __detail::is_conjugated(cc) ? std::conj(s) : s);
  }
  expect("conjugated(scaled(s, conjugated(scaled(t, A))))",
         g::complex_scaling_factor<T>(conjugated(scaled(s, conjugated(scaled(t, a)))), x), std::conj(s) * t);
  expect("scaled(s, A) x conjugated(scaled(t, B))", g::complex_scaling_factor<T>(scaled(s, a), conjugated(scaled(t, B))),
         s * std::conj(t));
  expect("conjugated(scaled(s, A)) x scaled(t, x)", g::complex_scaling_factor<T>(conjugated(scaled(s, a)), scaled(t, x)),
         std::conj(s) * t);
  expect("conjugated(A) x conjugated(scaled(t, B))", g::complex_scaling_factor<T>(conjugated(a), conjugated(scaled(t, B))),
         std::conj(t));

  expect_int("flags A, x", g::conj_flags(a, x), 0);
  expect_int("flags conj(A), x", g::conj_flags(conjugated(a), x), 1);
  expect_int("flags A, conj(x)", g::conj_flags(a, conjugated(x)), 2);
  expect_int("flags conj(scaled(s, conj(A))), conj(x)", g::conj_flags(conjugated(scaled(s, conjugated(a))), conjugated(x)), 2);
  expect_int("flags scaled(s, conj(A)), conj(B)", g::conj_flags(scaled(s, conjugated(a)), conjugated(B)), 3);
}

int main() {
  run<std::complex<float>>();
  run<std::complex<double>>();
  if (failures == 0)
    std::printf("complex factor checks: all passed\n");
  return failures;
}
