// X = inv(L) B for a block of right-hand sides with triangular_solve_inspect / triangular_solve on rank-2 operands:
// the sparse lower-triangular system of device_sptrsv.cpp, eight load cases solved together -- every level of the
// dependency graph is handed over once for all of them instead of once per vector.  The program checks itself on the host.
#include <cmath>

#include "common.hpp"

int main() {
  using T = double;
  using I = spblas::index_t;
  using O = spblas::offset_t;
  const int n = 100000, below = 5, nrhs = 8;
  std::mt19937 g(4);
  ex::host_csr<T> h;
  h.shape = spblas::index<I>(n, n);
  h.rowptr.push_back(0);
  for (int i = 0; i < n; ++i) {
    for (int t = 0; t < below && i > 0; ++t) {
      h.colind.push_back((I) (g() % i));
      h.values.push_back(T(0.1) * T((g() % 100) + 1) / T(100));
    }
    h.colind.push_back(i);
    h.values.push_back(T(2) + T(i % 3));
    h.rowptr.push_back((O) h.colind.size());
  }
  h.nnz = (O) h.colind.size();
  ex::device_csr<T> a(h);
  std::vector<T> b(static_cast<std::size_t>(n) * nrhs);  // row-major: the right-hand sides of a row lie together
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < nrhs; ++j)
      b[static_cast<std::size_t>(i) * nrhs + j] = T(1) + T((i + 3 * j) % 11);
  ex::device_array<T> d_b(b), d_x(b.size());
  spblas::mdspan_row_major<T, I> B(d_b.data(), n, nrhs), X(d_x.data(), n, nrhs);

  auto info = spblas::triangular_solve_inspect(a.view, spblas::lower_triangle, spblas::explicit_diagonal, B, X);
  spblas::triangular_solve(info, a.view, spblas::lower_triangle, spblas::explicit_diagonal, B, X);
  const auto x = d_x.to_host();

  // checked on the host, one right-hand side after the other: (1) the residual of every row, on the scale of its terms, as
  // device_sptrsv.cpp does; (2) every x against forward substitution in the same loop -- rounding differences are amplified
  // by the conditioning of the solve, so this bound is 100 x looser, as in the test suite (1e-12 and 1e-10 for double)
  double worst_resid = 0, worst_diff = 0;
  std::vector<double> ref(n);
  for (int j = 0; j < nrhs; ++j) {
    for (int i = 0; i < n; ++i) {
      const double bi = b[static_cast<std::size_t>(i) * nrhs + j];
      double s = 0, mag = std::abs(bi), acc = bi, d = 0;
      for (auto p = h.rowptr[i]; p < h.rowptr[i + 1]; ++p) {
        const double xc = x[static_cast<std::size_t>(h.colind[p]) * nrhs + j];
        s += h.values[p] * xc;
        mag += std::abs(h.values[p] * xc);
        if (h.colind[p] < i)
          acc -= h.values[p] * ref[h.colind[p]];
        else if (h.colind[p] == i)
          d = h.values[p];
      }
      ref[i] = acc / d;
      worst_resid = std::max(worst_resid, std::abs(s - bi) / mag);
      worst_diff = std::max(worst_diff, std::abs(x[static_cast<std::size_t>(i) * nrhs + j] - ref[i]) / std::abs(ref[i]));
    }
  }
  std::printf("device_sptrsm: n %d, nnz %d, %d right-hand sides, max row residual %.3g, max relative difference from the host "
              "loop %.3g\n", n, (int) h.nnz, nrhs, worst_resid, worst_diff);
  return worst_resid < 1e-12 && worst_diff < 1e-10 ? 0 : 1;
}
