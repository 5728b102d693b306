// ILU(0) as a preconditioner building block: spblas::gfx950::ilu0_inspect / ilu0 factor a sparse matrix on its own pattern,
// and the ONE result view feeds both triangular solves -- lower with the implied unit diagonal, then upper with the stored
// one.  The matrix is tridiagonal, so the factorisation has no fill: L U = A, and the two solves return the solution of
// A x = b.  All values are small dyadic numbers, so the program checks x for equality.
#include <cmath>

#include "common.hpp"

int main() {
  using T = double;
  using I = spblas::index_t;
  using O = spblas::offset_t;
  const int n = 50000;
  // L = unit lower bidiagonal, U = upper bidiagonal with a power-of-two diagonal; A = L U, stored row by row, columns sorted
  std::vector<T> l(n, T(0)), d(n), u(n, T(0)), x_true(n);
  for (int i = 0; i < n; ++i) {
    l[i] = i > 0 ? T((i % 3) - 1 == 0 ? 2 : (i % 3) - 1) : T(0);  // -1, 2, 1, ...
    d[i] = T(i % 4 == 0 ? 0.5 : (i % 4 == 1 ? 2 : (i % 4 == 2 ? -1 : 4)));
    u[i] = i + 1 < n ? T(i % 2 ? -2 : 1) : T(0);
    x_true[i] = T((i % 7) - 3 == 0 ? 2 : (i % 7) - 3);
  }
  ex::host_csr<T> h;
  h.shape = spblas::index<I>(n, n);
  h.rowptr.push_back(0);
  for (int i = 0; i < n; ++i) {
    if (i > 0) {
      h.colind.push_back(i - 1);
      h.values.push_back(l[i] * d[i - 1]);
    }
    h.colind.push_back(i);
    h.values.push_back(d[i] + (i > 0 ? l[i] * u[i - 1] : T(0)));
    if (i + 1 < n) {
      h.colind.push_back(i + 1);
      h.values.push_back(u[i]);
    }
    h.rowptr.push_back((O) h.colind.size());
  }
  h.nnz = (O) h.colind.size();
  std::vector<T> b(n);
  for (int i = 0; i < n; ++i) {
    T s = 0;
    for (auto p = h.rowptr[i]; p < h.rowptr[i + 1]; ++p)
      s += h.values[p] * x_true[h.colind[p]];
    b[i] = s;
  }

  ex::device_csr<T> a(h);
  ex::device_array<T> lu_values(h.values.size()), d_b(b), d_y(b.size()), d_x(b.size());
  spblas::csr_view<T, I, O> lu(lu_values.data(), a.rowptr.data(), a.colind.data(), h.shape, h.nnz);

  auto info = spblas::gfx950::ilu0_inspect(a.view);
  spblas::gfx950::ilu0(info, a.view, lu);
  const auto bad_row = spblas::gfx950::ilu0_status(info);
  spblas::triangular_solve(lu, spblas::lower_triangle, spblas::implicit_unit_diagonal, d_b.span(), d_y.span());
  spblas::triangular_solve(lu, spblas::upper_triangle, spblas::explicit_diagonal, d_y.span(), d_x.span());
  ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");

  const auto x = d_x.to_host();
  const auto f = lu_values.to_host();
  int wrong_x = 0, wrong_f = 0;
  for (int i = 0; i < n; ++i) {
    wrong_x += x[i] != x_true[i];
    auto p = h.rowptr[i];
    if (i > 0)
      wrong_f += f[p++] != l[i];
    wrong_f += f[p++] != d[i];
    if (i + 1 < n)
      wrong_f += f[p] != u[i];
  }
  std::printf("device_ilu0: n %d, nnz %d, first bad pivot %lld, %d factor entries and %d solution entries differ\n", n,
              (int) h.nnz, (long long) bad_row, wrong_f, wrong_x);
  return bad_row == -1 && wrong_f == 0 && wrong_x == 0 ? 0 : 1;
}
