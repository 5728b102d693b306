// An ILU(0) preconditioner applied APPROXIMATELY: spblas::gfx950::triangular_solve_sweeps replaces each of the two
// triangular solves by three Jacobi sweeps on the triangular system -- four SpMV-shaped launches instead of one hand-off per
// level of the dependency graph.  The matrix is the 5-point Laplacian of a 64 x 64 grid; the program prints the relative
// residual  |b - L U x| / |b|  of the sweeps beside that of the exact pair of solves (which is rounding only: L U x = b is
// what the pair solves).  A preconditioner need not be exact: the sweeps leave a residual well below |b|.
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
  ex::device_array<T> lu_values(h.values.size()), d_b(b), d_y(b.size()), d_x(b.size()), d_xs(b.size());
  spblas::csr_view<T, I, O> lu(lu_values.data(), a.rowptr.data(), a.colind.data(), h.shape, h.nnz);

  spblas::gfx950::ilu0(a.view, lu);
  // the exact pair ...
  spblas::triangular_solve(lu, spblas::lower_triangle, spblas::implicit_unit_diagonal, d_b.span(), d_y.span());
  spblas::triangular_solve(lu, spblas::upper_triangle, spblas::explicit_diagonal, d_y.span(), d_x.span());
  // ... and the same two applications by sweeps (plan-free: no inspect at all)
  spblas::gfx950::triangular_solve_sweeps(lu, spblas::lower_triangle, spblas::implicit_unit_diagonal, d_b.span(), d_y.span(),
                                          sweeps);
  spblas::gfx950::triangular_solve_sweeps(lu, spblas::upper_triangle, spblas::explicit_diagonal, d_y.span(), d_xs.span(),
                                          sweeps);
  ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");

  const auto f = lu_values.to_host();
  auto residual = [&](const std::vector<T>& x) {  // |b - L (U x)| / |b| on the host
    std::vector<T> ux(n), lux(n);
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
  const T r_exact = residual(d_x.to_host()), r_sweeps = residual(d_xs.to_host());
  std::printf("device_sptrsv_sweeps: n %d, nnz %d, relative residual |b - LUx| / |b|: exact pair %.3e, %d sweeps each %.3e\n", n,
              (int) h.nnz, (double) r_exact, sweeps, (double) r_sweeps);
  return r_exact < 1e-12 && std::isfinite(r_sweeps) && r_sweeps < 1.0 ? 0 : 1;
}
