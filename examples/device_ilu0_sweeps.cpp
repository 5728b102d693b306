// An ILU(0) preconditioner built AND applied without a single hand-off between levels: spblas::gfx950::ilu0_sweeps runs three
// fixed-point sweeps on the factorisation's equations (one launch each) where ilu0 follows the dependency graph level by
// level, and spblas::gfx950::triangular_solve_sweeps applies L and U by three Jacobi sweeps each.  The matrix is the 5-point
// Laplacian of a 64 x 64 grid.  The program prints the relative residual  |b - L U x| / |b|,  L and U the EXACT factor of
// ilu0, of the approximate chain beside that of the exact factor with the exact pair of solves (which is rounding only), and
// how far the swept factor is from the exact one.
#include <cmath>

#include "common.hpp"

int main() {
  using T = double;
  using I = spblas::index_t;
  using O = spblas::offset_t;
  const int g = 64, n = g * g, sweeps = 3;
  ex::host_csr<T> h;
  h.shape = spblas::index<I>(n, n);
  h.rowptr.push_back(0);
  for (int i = 0; i < n; ++i) {  // columns ascending, the diagonal stored: what ilu0 asks for
    const int r = i / g, c = i % g;
    auto put = [&](int col, T v) {
      h.colind.push_back(col);
      h.values.push_back(v);
    };
    if (r > 0) put(i - g, T(-1));
    if (c > 0) put(i - 1, T(-1));
    put(i, T(4));
    if (c + 1 < g) put(i + 1, T(-1));
    if (r + 1 < g) put(i + g, T(-1));
    h.rowptr.push_back((O) h.colind.size());
  }
  h.nnz = (O) h.colind.size();
  std::vector<T> b(n);
  for (int i = 0; i < n; ++i)
    b[i] = T(1 + (i % 5));

  ex::device_csr<T> a(h);
  ex::device_array<T> lu_values(h.values.size()), lus_values(h.values.size()), work(h.values.size()), d_b(b), d_y(b.size()),
      d_x(b.size()), d_xs(b.size());
  spblas::csr_view<T, I, O> lu(lu_values.data(), a.rowptr.data(), a.colind.data(), h.shape, h.nnz);
  spblas::csr_view<T, I, O> lus(lus_values.data(), a.rowptr.data(), a.colind.data(), h.shape, h.nnz);

  auto info = spblas::gfx950::ilu0_inspect(a.view);
  // the exact factor and the exact pair of solves ...
  spblas::gfx950::ilu0(info, a.view, lu);
  spblas::triangular_solve(lu, spblas::lower_triangle, spblas::implicit_unit_diagonal, d_b.span(), d_y.span());
  spblas::triangular_solve(lu, spblas::upper_triangle, spblas::explicit_diagonal, d_y.span(), d_x.span());
  // ... and the factor by sweeps (A is read, never written; the iterates alternate between lus and work), applied by sweeps
  spblas::gfx950::ilu0_sweeps(info, a.view, lus, work.span(), sweeps);
  const auto bad_row = spblas::gfx950::ilu0_status(info);
  spblas::gfx950::triangular_solve_sweeps(lus, spblas::lower_triangle, spblas::implicit_unit_diagonal, d_b.span(), d_y.span(),
                                          sweeps);
  spblas::gfx950::triangular_solve_sweeps(lus, spblas::upper_triangle, spblas::explicit_diagonal, d_y.span(), d_xs.span(),
                                          sweeps);
  ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");

  const auto f = lu_values.to_host(), fs = lus_values.to_host();
  T dd = 0, ff = 0;
  for (std::size_t p = 0; p < f.size(); ++p) {
    dd += (fs[p] - f[p]) * (fs[p] - f[p]);
    ff += f[p] * f[p];
  }
  auto residual = [&](const std::vector<T>& x) {  // |b - L (U x)| / |b| on the host, L and U the exact factor
    std::vector<T> ux(n);
    for (int i = 0; i < n; ++i) {
      T s = 0;
      for (auto p = h.rowptr[i]; p < h.rowptr[i + 1]; ++p)
        if (h.colind[p] >= i)
          s += f[p] * x[h.colind[p]];
      ux[i] = s;
    }
    T rr = 0, bb = 0;
    for (int i = 0; i < n; ++i) {
      T s = ux[i];
      for (auto p = h.rowptr[i]; p < h.rowptr[i + 1]; ++p)
        if (h.colind[p] < i)
          s += f[p] * ux[h.colind[p]];
      rr += (b[i] - s) * (b[i] - s);
      bb += b[i] * b[i];
    }
    return std::sqrt(rr / bb);
  };
  const T r_exact = residual(d_x.to_host()), r_sweeps = residual(d_xs.to_host()), f_diff = std::sqrt(dd / ff);
  std::printf("device_ilu0_sweeps: n %d, nnz %d, relative residual |b - LUx| / |b|: exact factor and exact pair %.3e, "
              "%d factor sweeps and %d sweeps per apply %.3e; |LU(%d) - LU| / |LU| %.3e, first bad pivot %lld\n",
              n, (int) h.nnz, (double) r_exact, sweeps, sweeps, (double) r_sweeps, sweeps, (double) f_diff, (long long) bad_row);
  return r_exact < 1e-12 && std::isfinite(r_sweeps) && r_sweeps < 1.0 && f_diff < 0.1 && bad_row == -1 ? 0 : 1;
}
