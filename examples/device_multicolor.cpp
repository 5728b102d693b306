// Multicolour ordering in front of ILU(0): spblas::gfx950::multicolor_order colours the matrix graph, permute forms
// B = P A P^T and permute_vector takes b along; ilu0 and the two triangular solves then run on B, whose level plans are as
// shallow as the colouring (6 colours on the 7-point Laplacian against 3 g - 2 levels in the natural order), and permute_vector
// takes x back.  ILU(0) is incomplete, so x = inv(L U) b is a preconditioner apply, not the solution of A x = b: the program
// prints the level counts and the relative residual of the two solves, || P b - L U (P x) || / || b || with the device's factor
// multiplied out on the host, and checks that both triangles of B are no deeper than the colouring, that the natural order is
// deeper, and that the residual is at rounding level.
#include <cmath>

#include "common.hpp"

namespace {
std::int64_t lower_levels(const std::vector<int>& rowptr, const std::vector<int>& colind) {
  const int m = (int) rowptr.size() - 1;
  std::vector<int> lev(m, 0);
  int top = 0;
  for (int i = 0; i < m; ++i) {
    for (int p = rowptr[i]; p < rowptr[i + 1]; ++p)
      if (colind[p] < i)
        lev[i] = std::max(lev[i], lev[colind[p]] + 1);
    top = std::max(top, lev[i] + 1);
  }
  return m ? top : 0;
}
} // namespace

int main() {
  using T = double;
  using I = spblas::index_t;
  using O = spblas::offset_t;
  const int g = 24, n = g * g * g;
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

  ex::device_csr<T> a(h);
  ex::device_array<T> b_values(h.values.size()), d_b(b), d_pb(b.size()), d_y(b.size()), d_px(b.size()), d_x(b.size());
  ex::device_array<O> b_rowptr(n + 1);
  ex::device_array<I> b_colind(h.colind.size()), perm(n);
  spblas::csr_view<T, I, O> pa(b_values.data(), b_rowptr.data(), b_colind.data(), h.shape, h.nnz);

  // 1. colour   2. permute A and b   3. ilu0 on B   4. both solves   5. un-permute x
  spblas::operation_info_t order;
  const auto mc = spblas::gfx950::multicolor_order(order, a.view);
  spblas::gfx950::multicolor_copy(order, perm.span(), {}, {}, {});
  spblas::gfx950::permute(a.view, perm.span(), pa);
  spblas::gfx950::permute_vector<T>(perm.span(), d_b.span(), d_pb.span());
  auto info = spblas::gfx950::ilu0_inspect(pa);
  spblas::gfx950::ilu0(info, pa, pa);
  const auto bad_row = spblas::gfx950::ilu0_status(info);
  spblas::triangular_solve(pa, spblas::lower_triangle, spblas::implicit_unit_diagonal, d_pb.span(), d_y.span());
  spblas::triangular_solve(pa, spblas::upper_triangle, spblas::explicit_diagonal, d_y.span(), d_px.span());
  spblas::gfx950::permute_vector<T>(perm.span(), d_px.span(), d_x.span(), true);
  ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");

  const auto rp = b_rowptr.to_host();
  const auto ci = b_colind.to_host();
  const auto lu = b_values.to_host();
  const auto p = perm.to_host();
  const auto x = d_x.to_host();
  // levels of A and of B on the host, both triangles (the upper one: the lower one of the reversed order)
  const auto nat = lower_levels(h.rowptr, h.colind);
  const auto low = lower_levels(rp, ci);
  std::vector<int> rrp(1, 0), rci;
  for (int i = n - 1; i >= 0; --i) {
    for (int q = rp[i]; q < rp[i + 1]; ++q)
      rci.push_back(n - 1 - ci[q]);
    rrp.push_back((int) rci.size());
  }
  const auto upp = lower_levels(rrp, rci);
  // || P b - L U (P x) || / || b ||: w = U px, then L w, row by row
  std::vector<T> px(n), w(n);
  for (int i = 0; i < n; ++i)
    px[i] = x[p[i]];
  for (int i = 0; i < n; ++i) {
    T s = 0;
    for (int q = rp[i]; q < rp[i + 1]; ++q)
      if (ci[q] >= i)
        s += lu[q] * px[ci[q]];
    w[i] = s;
  }
  double num = 0, den = 0;
  for (int i = 0; i < n; ++i) {
    T s = w[i];
    for (int q = rp[i]; q < rp[i + 1]; ++q)
      if (ci[q] < i)
        s += lu[q] * w[ci[q]];
    num += (double) (b[p[i]] - s) * (double) (b[p[i]] - s);
    den += (double) b[p[i]] * (double) b[p[i]];
  }
  const double res = std::sqrt(num / den);
  std::printf("device_multicolor: n %d, nnz %d, colours %lld in %lld rounds, levels natural %lld, after ordering lower %lld "
              "upper %lld, first bad pivot %lld, residual of L U (P x) = P b %.3e\n",
              n, (int) h.nnz, (long long) mc.colors, (long long) mc.rounds, (long long) nat, (long long) low, (long long) upp,
              (long long) bad_row, res);
  return bad_row == -1 && low <= mc.colors && upp <= mc.colors && mc.colors < nat && res < 1e-12 ? 0 : 1;
}
