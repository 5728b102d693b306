// Aggregation multigrid in two levels: spblas::gfx950::aggregate groups the rows of a 7-point Laplacian (16^3, diagonal 6) into
// MIS-2 aggregates, prolongator writes the piecewise-constant P, coarsen_inspect / coarsen_structure / coarsen form the
// Galerkin matrix A_c = P^T A P.  Both levels are smoothed by multicolour Gauss-Seidel (multicolor_order +
// gauss_seidel_inspect + gauss_seidel).  One two-grid correction on A x = b from x = 0:
//   x <- one symmetric sweep;  r = b - A x;  r_c = P^T r;  e_c <- 20 symmetric sweeps on A_c e_c = r_c from 0;
//   x <- x + P e_c;  x <- one symmetric sweep.
// The program prints the fine and coarse sizes and the relative residual after two plain sweeps and through the correction
// (which spends the same two fine sweeps), and checks that the cycle lowers the residual below what smoothing alone reaches.
// (The correction of a piecewise-constant P lowers the error in the energy norm; the 2-norm of the residual may rise right
// after it -- the rough part it adds is what the post-smoothing sweep removes.)
#include <cmath>
#include <memory>

#include "common.hpp"

using T = double;
using I = spblas::index_t;
using O = spblas::offset_t;

// the smoother of one level: the colouring of A and the Gauss-Seidel plan on A with its row order
struct smoother {
  spblas::operation_info_t order, gs;
  ex::device_array<I> perm;
  std::unique_ptr<ex::device_array<I>> color_ptr;
  smoother(spblas::csr_view<T, I, O> a, std::size_t n) : perm(n) {
    const auto mc = spblas::gfx950::multicolor_order(order, a);
    color_ptr = std::make_unique<ex::device_array<I>>((std::size_t) mc.colors + 1);
    spblas::gfx950::multicolor_copy(order, perm.span(), {}, {}, color_ptr->span());
    spblas::gfx950::gauss_seidel_inspect(gs, a, color_ptr->span(), perm.span());
  }
  void sweep(spblas::csr_view<T, I, O> a, std::span<T> b, std::span<T> x, int sweeps) {
    spblas::gfx950::gauss_seidel(gs, a, b, x, sweeps, T(1), spblas::gfx950::gs_direction::symmetric);
  }
};

int main() {
  const int g = 16, n = g * g * g;
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
        put(true, i, T(6));
        put(x + 1 < g, i + 1, T(-1));
        put(y + 1 < g, i + g, T(-1));
        put(z + 1 < g, i + g * g, T(-1));
        h.rowptr.push_back((O) h.colind.size());
      }
  h.nnz = (O) h.colind.size();
  std::vector<T> b(n);
  for (int i = 0; i < n; ++i)
    b[i] = T(1) + T(i % 5) / 4;
  auto residual = [&](const std::vector<T>& x, std::vector<T>* r) {
    double num = 0, den = 0;
    for (int i = 0; i < n; ++i) {
      T s = b[i];
      for (int p = h.rowptr[i]; p < h.rowptr[i + 1]; ++p)
        s -= h.values[p] * x[h.colind[p]];
      if (r)
        (*r)[i] = s;
      num += (double) s * (double) s;
      den += (double) b[i] * (double) b[i];
    }
    return std::sqrt(num / den);
  };

  ex::device_csr<T> a(h);
  // aggregates and the prolongator
  spblas::operation_info_t ag;
  const auto ai = spblas::gfx950::aggregate(ag, a.view, 0.08);
  const int nc = (int) ai.aggregates;
  ex::device_array<I> agg(n);
  spblas::gfx950::aggregate_copy(ag, agg.span(), {});
  ex::device_array<T> p_values(n);
  ex::device_array<O> p_rowptr(n + 1);
  ex::device_array<I> p_colind(n);
  spblas::csr_view<T, I, O> p(p_values.data(), p_rowptr.data(), p_colind.data(), spblas::index<I>(n, nc), (O) n);
  spblas::gfx950::prolongator(ag, p);
  // the coarse matrix
  spblas::operation_info_t cz;
  const auto ci = spblas::gfx950::coarsen_inspect(cz, a.view, agg.span(), nc);
  ex::device_array<T> c_values((std::size_t) ci.nnz);
  ex::device_array<O> c_rowptr((std::size_t) nc + 1);
  ex::device_array<I> c_colind((std::size_t) ci.nnz);
  spblas::csr_view<T, I, O> ac(c_values.data(), c_rowptr.data(), c_colind.data(), spblas::index<I>(nc, nc), (O) ci.nnz);
  spblas::gfx950::coarsen_structure(cz, ac);
  spblas::gfx950::coarsen(cz, a.view, ac);
  ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
  std::printf("device_aggregate: fine %d rows / %d entries, coarse %d rows / %lld entries (%lld rounds, aggregates of %lld to "
              "%lld rows)", n, (int) h.nnz, nc, (long long) ci.nnz, (long long) ai.rounds, (long long) ai.smallest,
              (long long) ai.largest);
  // the entry sum is preserved: P has one 1 per row
  double sum_a = 0, sum_c = 0;
  for (T v : h.values)
    sum_a += v;
  for (T v : c_values.to_host())
    sum_c += v;

  smoother fine(a.view, n), coarse(ac, (std::size_t) nc);
  ex::device_array<T> d_b(b), d_x(std::vector<T>(n, T(0))), d_r(n), d_rc((std::size_t) nc), d_e(n);

  // smoothing alone: two symmetric sweeps
  fine.sweep(a.view, d_b.span(), d_x.span(), 2);
  ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
  const double plain = residual(d_x.to_host(), nullptr);

  // the two-grid correction with the same two fine sweeps
  std::vector<T> x(n, T(0)), r(n);
  ex::hip_ok(hipMemcpy(d_x.data(), x.data(), n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
  fine.sweep(a.view, d_b.span(), d_x.span(), 1);
  ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
  x = d_x.to_host();
  const double pre = residual(x, &r);
  ex::hip_ok(hipMemcpy(d_r.data(), r.data(), n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
  spblas::multiply(spblas::transposed(p), d_r.span(), d_rc.span());                 // r_c = P^T r
  ex::device_array<T> d_ec(std::vector<T>((std::size_t) nc, T(0)));
  coarse.sweep(ac, d_rc.span(), d_ec.span(), 20);
  spblas::multiply(p, d_ec.span(), d_e.span());                                     // e = P e_c
  ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
  const auto e = d_e.to_host();
  for (int i = 0; i < n; ++i)
    x[i] += e[i];
  const double corrected = residual(x, nullptr);
  ex::hip_ok(hipMemcpy(d_x.data(), x.data(), n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
  fine.sweep(a.view, d_b.span(), d_x.span(), 1);
  ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
  const double cycle = residual(d_x.to_host(), nullptr);
  std::printf(", residual: 2 sweeps %.3e; two-grid: pre-smoothed %.3e, corrected %.3e, post-smoothed %.3e\n", plain, pre,
              corrected, cycle);
  const bool ok = nc > 0 && nc < n && std::fabs(sum_a - sum_c) <= 1e-9 * std::fabs(sum_a) && cycle < 1.0 && cycle < plain;
  return ok ? 0 : 1;
}
