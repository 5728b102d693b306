// Multicolour Gauss-Seidel as a smoother: spblas::gfx950::multicolor_order colours a 7-point Laplacian (diagonal 6.5, the matrix
// of device_multicolor.cpp), gauss_seidel_inspect
// takes the colouring and gauss_seidel runs symmetric sweeps (forward through the colours, then backward) on A x = b, x updated
// in place.  The sweeps run twice: on A itself with the row order `perm`, and on B = P A P^T with the permuted b and no perm.
// Both are sequential Gauss-Seidel in colour order, so after permute_vector takes the second solution back the two agree to
// rounding (B's rows hold their entries in another order).  The program prints the relative residual || b - A x || / || b ||
// after every sweep and checks that it falls monotonically from the 1 of x = 0 and that the two solutions agree.
#include <cmath>

#include "common.hpp"

int main() {
  using T = double;
  using I = spblas::index_t;
  using O = spblas::offset_t;
  const int g = 16, n = g * g * g, sweeps = 6;
  ex::host_csr<T> h;
  h.shape = spblas::index<I>(n, n);
  h.rowptr.push_back(0);
  for (int z = 0; z < g; ++z)
    for (int y = 0; y < g; ++y)
      for (int x = 0; x < g; ++x) {
        const int i = (z * g + y) * g + x;
        auto put = [&](bool ok, int j, T v) {
          if (ok) {
            h.colind.push_back(j);
            h.values.push_back(v);
          }
        };
        put(z > 0, i - g * g, T(-1));
        put(y > 0, i - g, T(-1));
        put(x > 0, i - 1, T(-1));
        put(true, i, T(6.5));
        put(x + 1 < g, i + 1, T(-1));
        put(y + 1 < g, i + g, T(-1));
        put(z + 1 < g, i + g * g, T(-1));
        h.rowptr.push_back((O) h.colind.size());
      }
  h.nnz = (O) h.colind.size();
  std::vector<T> b(n);
  for (int i = 0; i < n; ++i)
    b[i] = T(1) + T(i % 5) / 4;
  auto residual = [&](const std::vector<T>& x) {
    double num = 0, den = 0;
    for (int i = 0; i < n; ++i) {
      T s = b[i];
      for (int p = h.rowptr[i]; p < h.rowptr[i + 1]; ++p)
        s -= h.values[p] * x[h.colind[p]];
      num += (double) s * (double) s;
      den += (double) b[i] * (double) b[i];
    }
    return std::sqrt(num / den);
  };

  ex::device_csr<T> a(h);
  ex::device_array<T> b_values(h.values.size()), d_b(b), d_pb(b.size()), d_x(std::vector<T>(n, T(0))),
      d_px(std::vector<T>(n, T(0))), d_back(b.size());
  ex::device_array<O> b_rowptr(n + 1);
  ex::device_array<I> b_colind(h.colind.size()), perm(n);
  spblas::csr_view<T, I, O> pa(b_values.data(), b_rowptr.data(), b_colind.data(), h.shape, h.nnz);

  spblas::operation_info_t order, on_a, on_b;
  const auto mc = spblas::gfx950::multicolor_order(order, a.view);
  ex::device_array<I> color_ptr((std::size_t) mc.colors + 1);
  spblas::gfx950::multicolor_copy(order, perm.span(), {}, {}, color_ptr.span());
  spblas::gfx950::permute(a.view, perm.span(), pa);
  spblas::gfx950::permute_vector<T>(perm.span(), d_b.span(), d_pb.span());
  const auto gi = spblas::gfx950::gauss_seidel_inspect(on_a, a.view, color_ptr.span(), perm.span());
  spblas::gfx950::gauss_seidel_inspect(on_b, pa, color_ptr.span());

  bool falling = true;
  double last = 1.0, res = 1.0;
  std::printf("device_gauss_seidel: n %d, nnz %d, colours %lld, %lld launches per forward sweep, residual", n, (int) h.nnz,
              (long long) gi.colors, (long long) gi.launches_per_forward_sweep);
  for (int s = 0; s < sweeps; ++s) {
    spblas::gfx950::gauss_seidel(on_a, a.view, d_b.span(), d_x.span(), 1, T(1), spblas::gfx950::gs_direction::symmetric);
    spblas::gfx950::gauss_seidel(on_b, pa, d_pb.span(), d_px.span(), 1, T(1), spblas::gfx950::gs_direction::symmetric);
    ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    res = residual(d_x.to_host());
    std::printf(" %.3e", res);
    falling = falling && res < last;
    last = res;
  }
  spblas::gfx950::permute_vector<T>(perm.span(), d_px.span(), d_back.span(), true);
  ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
  const auto x = d_x.to_host();
  const auto xb = d_back.to_host();
  double diff = 0, top = 0;
  for (int i = 0; i < n; ++i) {
    diff = std::max(diff, std::fabs((double) x[i] - (double) xb[i]));
    top = std::max(top, std::fabs((double) x[i]));
  }
  std::printf(", A with perm against permuted B: %.3e of %.3e\n", diff, top);
  return falling && diff <= 1e-12 * top && gi.colors == mc.colors ? 0 : 1;
}
