// Smoothed aggregation in two levels: spblas::gfx950::aggregate groups the rows of a 7-point Laplacian (16^3, diagonal 6) into
// MIS-2 aggregates; smooth_prolongator_inspect / smooth_prolongator_structure / smooth_prolongator form the smoothed prolongator
// P = (I - omega D^-1 A) T with omega = 2/3 (Vanek, Mandel, Brezina 1996); transpose gives P^T and two SpGEMMs give the
// Galerkin matrix A_c = P^T (A P).  The same is done for the tentative prolongator T (prolongator()).  Both levels are smoothed
// by multicolour Gauss-Seidel.  One two-grid correction on A x = b from x = 0, once with each prolongator:
//   x <- one symmetric sweep;  r = b - A x;  r_c = P^T r;  e_c <- 30 symmetric sweeps on A_c e_c = r_c from 0;
//   x <- x + P e_c;  x <- one symmetric sweep.
// The program prints the sizes of both coarse matrices and the relative residual after the cycle with T and with P, and exits
// non-zero unless the smoothed prolongator leaves the smaller residual.
#include <cmath>
#include <memory>

#include "common.hpp"

using T = double;
using I = spblas::index_t;
using O = spblas::offset_t;
using csr = spblas::csr_view<T, I, O>;

// the smoother of one level: the colouring of A and the Gauss-Seidel plan on A with its row order
struct smoother {
  spblas::operation_info_t order, gs;
  ex::device_array<I> perm;
  std::unique_ptr<ex::device_array<I>> color_ptr;
  smoother(csr a, std::size_t n) : perm(n) {
    const auto mc = spblas::gfx950::multicolor_order(order, a);
    color_ptr = std::make_unique<ex::device_array<I>>((std::size_t) mc.colors + 1);
    spblas::gfx950::multicolor_copy(order, perm.span(), {}, {}, color_ptr->span());
    spblas::gfx950::gauss_seidel_inspect(gs, a, color_ptr->span(), perm.span());
  }
  void sweep(csr a, std::span<T> b, std::span<T> x, int sweeps) {
    spblas::gfx950::gauss_seidel(gs, a, b, x, sweeps, T(1), spblas::gfx950::gs_direction::symmetric);
  }
};

// a device CSR matrix that owns its arrays
struct owned_csr {
  std::unique_ptr<ex::device_array<T>> values;
  std::unique_ptr<ex::device_array<O>> rowptr;
  std::unique_ptr<ex::device_array<I>> colind;
  csr view{nullptr, nullptr, nullptr, {0, 0}, 0};
  owned_csr(int m, int n, std::size_t nnz) {
    values = std::make_unique<ex::device_array<T>>(nnz);
    rowptr = std::make_unique<ex::device_array<O>>((std::size_t) m + 1);
    colind = std::make_unique<ex::device_array<I>>(nnz);
    view = csr(values->data(), rowptr->data(), colind->data(), spblas::index<I>(m, n), (O) nnz);
  }
};

// C = A * B with the two-phase SpGEMM
static std::unique_ptr<owned_csr> product(csr a, csr b) {
  const int m = (int) a.shape()[0], n = (int) b.shape()[1];
  ex::device_array<O> rowptr((std::size_t) m + 1);
  csr c(nullptr, rowptr.data(), nullptr, {m, n}, 0);
  auto info = spblas::multiply_compute(a, b, c);
  const auto nnz = (std::size_t) info.result_nnz();
  auto out = std::make_unique<owned_csr>(m, n, nnz);
  ex::hip_ok(hipMemcpy(out->rowptr->data(), rowptr.data(), ((std::size_t) m + 1) * sizeof(O), hipMemcpyDeviceToDevice),
             "hipMemcpy");
  spblas::multiply_fill(info, a, b, out->view);
  return out;
}

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
  // the aggregates
  spblas::operation_info_t ag;
  const auto ai = spblas::gfx950::aggregate(ag, a.view, 0.08);
  const int nc = (int) ai.aggregates;
  ex::device_array<I> agg(n);
  spblas::gfx950::aggregate_copy(ag, agg.span(), {});
  // the tentative prolongator T ...
  owned_csr tent(n, nc, (std::size_t) n);
  spblas::gfx950::prolongator(ag, tent.view);
  // ... and the smoothed one, P = (I - 2/3 D^-1 A) T
  spblas::operation_info_t sm;
  const auto pi = spblas::gfx950::smooth_prolongator_inspect(sm, a.view, agg.span(), nc);
  owned_csr smoothed(n, nc, (std::size_t) pi.nnz);
  spblas::gfx950::smooth_prolongator_structure(sm, smoothed.view);
  spblas::gfx950::smooth_prolongator(sm, a.view, smoothed.view, T(2) / T(3));
  smoother fine(a.view, n);
  ex::device_array<T> d_b(b);

  // one two-grid correction with the prolongator p; returns the relative residual after it
  long long coarse_nnz[2] = {0, 0};
  int which = 0;
  auto two_grid = [&](csr p) {
    owned_csr pt(nc, n, (std::size_t) p.size());
    spblas::transpose(p, pt.view);                                                    // P^T
    auto ap = product(a.view, p);                                                     // A P
    auto ac = product(pt.view, ap->view);                                             // A_c = P^T (A P)
    coarse_nnz[which++] = (long long) ac->view.size();
    smoother coarse(ac->view, (std::size_t) nc);
    ex::device_array<T> d_x(std::vector<T>(n, T(0))), d_r(n), d_rc((std::size_t) nc), d_e(n);
    ex::device_array<T> d_ec(std::vector<T>((std::size_t) nc, T(0)));
    fine.sweep(a.view, d_b.span(), d_x.span(), 1);
    ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    std::vector<T> x = d_x.to_host(), r(n);
    residual(x, &r);
    ex::hip_ok(hipMemcpy(d_r.data(), r.data(), n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
    spblas::multiply(pt.view, d_r.span(), d_rc.span());                               // r_c = P^T r
    coarse.sweep(ac->view, d_rc.span(), d_ec.span(), 30);
    spblas::multiply(p, d_ec.span(), d_e.span());                                     // e = P e_c
    ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    const auto e = d_e.to_host();
    for (int i = 0; i < n; ++i)
      x[i] += e[i];
    ex::hip_ok(hipMemcpy(d_x.data(), x.data(), n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
    fine.sweep(a.view, d_b.span(), d_x.span(), 1);
    ex::hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    return residual(d_x.to_host(), nullptr);
  };
  const double plain = two_grid(tent.view);
  const double smooth = two_grid(smoothed.view);

  // every row of the smoothed P sums to 1 where the row of A sums to 0 (the interior rows), and P holds T's pattern and more
  const auto pv = smoothed.values->to_host();
  const auto prp = smoothed.rowptr->to_host();
  const int centre = (8 * g + 8) * g + 8;
  double row_sum = 0;
  for (O e = prp[centre]; e < prp[centre + 1]; ++e)
    row_sum += pv[e];
  std::printf("device_smoothed_aggregation: fine %d rows / %d entries, %d aggregates; tentative P %d entries -> A_c %lld entries, "
              "smoothed P %lld entries -> A_c %lld entries; residual after one two-grid cycle: tentative %.3e, smoothed %.3e\n",
              n, (int) h.nnz, nc, n, coarse_nnz[0], (long long) pi.nnz, coarse_nnz[1], plain, smooth);
  const bool ok = nc > 0 && nc < n && pi.nnz > n && std::fabs(row_sum - 1.0) <= 1e-12 && smooth < plain && smooth < 1.0;
  return ok ? 0 : 1;
}
