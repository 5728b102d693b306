#pragma once
// Standalone C++20 mirror of the spblas-reference operator interface for the multiply() path,
// bound to the gfx950 backend.  WHY IT EXISTS: the reference's own headers need range-v3 and
// kokkos-mdspan (fetched by CMake, absent from this image), so the drop-in backend headers in
// include/spblas/vendor/gfx950/ cannot be compiled here.  This header offers the same names,
// argument meaning and error behaviour with nothing but the standard library, so that C++
// programs and tests written like the reference's device tests
// (/root/reference/test/gtest/device/spmv_test.cpp, spgemm_test.cpp) build with g++ and run on
// the GPU through the same C ABI and the same __gfx950 call layer.  It is not a copy of the
// reference: only the public surface of the hot path is restated.
//
//   csr_view / csc_view            views/csr_view.hpp:12-77, views/csc_view.hpp
//   scaled(alpha, t)               algorithms/scaled.hpp, views/scaled_view_impl.hpp
//   scale(alpha, t)                algorithms/scale_impl.hpp:13-31 (in place, on the device)
//   transposed(a)                  algorithms/transposed.hpp:7-21
//   matrix_opt                     views/matrix_opt_impl.hpp:14-93
//   mdspan_row_major<T, I>         detail/mdspan.hpp:38-41 (minimal 2-D row-major view)
//   operation_info_t               detail/operation_info_t.hpp:28-104
//   spgemm_state_t + multiply_*    vendor/rocsparse/multiply_spgemm.hpp:28-317 (3- and 4-argument forms)
//   add / add_inspect / add_compute algorithms/add_impl.hpp:40-115
//   multiply / multiply_inspect    vendor/rocsparse/detail/spmv_impl.hpp:18-90,
//                                  vendor/onemkl_sycl/spmm_impl.hpp:133-198
#include <algorithm>
#include <concepts>
#include <cstdint>
#include <memory>
#include <optional>
#include <span>
#include <stdexcept>
#include <type_traits>
#include <utility>

#include <spblas/vendor/gfx950/detail/backend_calls.hpp>

namespace spblas {

using index_t = std::int32_t;
using offset_t = index_t;

template <std::integral I = index_t>
class index {
public:
  constexpr index() = default;
  constexpr index(I r, I c) : v_{r, c} {}
  constexpr I operator[](int i) const {
    return v_[i];
  }
  constexpr bool operator==(const index&) const = default;

private:
  I v_[2] = {0, 0};
};

class view_base {};

template <typename T, std::integral I = index_t, std::integral O = I>
class csr_view : public view_base {
public:
  using scalar_type = T;
  using index_type = I;
  using offset_type = O;
  csr_view(T* values, O* rowptr, I* colind, index<I> shape, O nnz)
      : values_(values, values ? nnz : 0), rowptr_(rowptr, rowptr ? shape[0] + 1 : 0),
        colind_(colind, colind ? nnz : 0), shape_(shape), nnz_(nnz) {}
  void update(std::span<T> values, std::span<O> rowptr, std::span<I> colind) {
    values_ = values;
    rowptr_ = rowptr;
    colind_ = colind;
  }
  void update(std::span<T> values, std::span<O> rowptr, std::span<I> colind, index<I> shape, O nnz) {
    update(values, rowptr, colind);
    shape_ = shape;
    nnz_ = nnz;
  }
  std::span<T> values() const noexcept {
    return values_;
  }
  std::span<O> rowptr() const noexcept {
    return rowptr_;
  }
  std::span<I> colind() const noexcept {
    return colind_;
  }
  index<I> shape() const noexcept {
    return shape_;
  }
  O size() const noexcept {
    return nnz_;
  }

private:
  std::span<T> values_;
  std::span<O> rowptr_;
  std::span<I> colind_;
  index<I> shape_;
  O nnz_;
};

template <typename T, std::integral I = index_t, std::integral O = I>
class csc_view : public view_base {
public:
  using scalar_type = T;
  using index_type = I;
  using offset_type = O;
  csc_view(T* values, O* colptr, I* rowind, index<I> shape, O nnz)
      : values_(values, nnz), colptr_(colptr, shape[1] + 1), rowind_(rowind, nnz), shape_(shape), nnz_(nnz) {}
  std::span<T> values() const noexcept {
    return values_;
  }
  std::span<O> colptr() const noexcept {
    return colptr_;
  }
  std::span<I> rowind() const noexcept {
    return rowind_;
  }
  index<I> shape() const noexcept {
    return shape_;
  }
  O size() const noexcept {
    return nnz_;
  }

private:
  std::span<T> values_;
  std::span<O> colptr_;
  std::span<I> rowind_;
  index<I> shape_;
  O nnz_;
};

// Minimal row-major 2-D view: data_handle(), extent(r), stride(0) -- what the backend reads from
// an mdspan<T, dextents<I,2>, layout_right> (detail/mdspan.hpp:38-41).
template <typename T, std::integral I = index_t>
class mdspan_row_major {
public:
  using value_type = T;
  mdspan_row_major(T* data, I rows, I cols) : data_(data), rows_(rows), cols_(cols), ld_(cols) {}
  mdspan_row_major(T* data, I rows, I cols, I row_stride) : data_(data), rows_(rows), cols_(cols), ld_(row_stride) {}
  T* data_handle() const {
    return data_;
  }
  I extent(int r) const {
    return r == 0 ? rows_ : cols_;
  }
  I stride(int r) const {
    return r == 0 ? ld_ : 1;
  }

private:
  T* data_;
  I rows_, cols_, ld_;
};

template <typename S, typename V>
class scaled_view : public view_base {
public:
  scaled_view(S alpha, V base) : alpha_(alpha), base_(base) {}
  S alpha() const {
    return alpha_;
  }
  V base() const {
    return base_;
  }

private:
  S alpha_;
  V base_;
};

template <typename S, typename V>
auto scaled(S alpha, V&& v) {
  return scaled_view<S, std::remove_cvref_t<V>>(alpha, std::forward<V>(v));
}

template <typename V>
class conjugated_view : public view_base {
public:
  explicit conjugated_view(V base) : base_(base) {}
  V base() const {
    return base_;
  }

private:
  V base_;
};

template <typename V>
auto conjugated(V&& v) {
  return conjugated_view<std::remove_cvref_t<V>>(std::forward<V>(v));
}

template <typename T, typename I, typename O>
auto transposed(csr_view<T, I, O> a) {
  return csc_view<T, I, O>(a.values().data(), a.rowptr().data(), a.colind().data(),
                           index<I>(a.shape()[1], a.shape()[0]), a.size());
}
template <typename T, typename I, typename O>
auto transposed(csc_view<T, I, O> a) {
  return csr_view<T, I, O>(a.values().data(), a.colptr().data(), a.rowind().data(),
                           index<I>(a.shape()[1], a.shape()[0]), a.size());
}

// matrix_opt: owns the cached inspect result (views/matrix_opt_impl.hpp:90-92 holds the vendor
// handle the same way).
template <typename M>
class matrix_opt : public view_base {
public:
  explicit matrix_opt(M matrix) : matrix_(matrix), state_(std::make_shared<holder>()) {}
  M base() const {
    return matrix_;
  }
  struct holder {
    std::unique_ptr<__gfx950::spmv_state_t> spmv;
  };
  holder& cache() const {
    return *state_;
  }

private:
  M matrix_;
  std::shared_ptr<holder> state_;
};

// ---- view inspection (detail/view_inspectors.hpp:22-138) ------------------------------------
namespace __detail {

template <typename T>
struct is_csr : std::false_type {};
template <typename T, typename I, typename O>
struct is_csr<csr_view<T, I, O>> : std::true_type {};
template <typename T>
struct is_csc : std::false_type {};
template <typename T, typename I, typename O>
struct is_csc<csc_view<T, I, O>> : std::true_type {};
template <typename T>
struct is_dense : std::false_type {};
template <typename T, typename I>
struct is_dense<mdspan_row_major<T, I>> : std::true_type {};
template <typename T>
struct is_span : std::false_type {};
template <typename T, std::size_t E>
struct is_span<std::span<T, E>> : std::true_type {};
template <typename T>
struct is_scaled : std::false_type {};
template <typename S, typename V>
struct is_scaled<scaled_view<S, V>> : std::true_type {};
template <typename T>
struct is_conj : std::false_type {};
template <typename V>
struct is_conj<conjugated_view<V>> : std::true_type {};
template <typename T>
struct is_opt : std::false_type {};
template <typename M>
struct is_opt<matrix_opt<M>> : std::true_type {};

template <typename T>
concept has_base = requires(const std::remove_cvref_t<T>& t) { t.base(); };

template <typename T>
auto get_ultimate_base(T&& t) {
  if constexpr (has_base<T>) {
    return get_ultimate_base(t.base());
  } else {
    return t;
  }
}
template <typename T>
using ultimate_base_type_t = decltype(get_ultimate_base(std::declval<T>()));

// product of all scaling factors as double, or nullopt (view_inspectors.hpp:22-77)
template <typename T>
std::optional<double> get_scaling_factor(T&& t) {
  if constexpr (has_base<T>) {
    auto inner = get_scaling_factor(t.base());
    if constexpr (is_scaled<std::remove_cvref_t<T>>::value) {
      return inner ? std::optional<double>(double(t.alpha()) * *inner) : std::optional<double>(double(t.alpha()));
    } else {
      return inner;
    }
  } else {
    return std::nullopt;
  }
}
template <typename T, typename U>
std::optional<double> get_scaling_factor(T&& t, U&& u) {
  auto a = get_scaling_factor(t), b = get_scaling_factor(u);
  if (a && b) {
    return *a * *b;
  }
  return a ? a : b;
}

template <typename T>
bool is_conjugated(T&& t) {  // odd number of conjugated views (view_inspectors.hpp:81-97)
  if constexpr (has_base<T>) {
    if constexpr (is_conj<std::remove_cvref_t<T>>::value) {
      return !is_conjugated(t.base());
    } else {
      return is_conjugated(t.base());
    }
  } else {
    return false;
  }
}

template <typename T>
concept has_csr_base = is_csr<ultimate_base_type_t<T>>::value;
template <typename T>
concept has_csc_base = is_csc<ultimate_base_type_t<T>>::value;
template <typename T>
concept has_dense_base = is_dense<ultimate_base_type_t<T>>::value;
template <typename T>
concept has_span_base = is_span<ultimate_base_type_t<T>>::value;

} // namespace __detail

// ---- operation_info_t (detail/operation_info_t.hpp:28-104) -----------------------------------
class spgemm_state_t;

class operation_info_t {
public:
  operation_info_t() = default;
  operation_info_t(index<index_t> shape, std::int64_t nnz) : result_shape_(shape), result_nnz_(nnz) {}
  operation_info_t(operation_info_t&&) = default;
  operation_info_t& operator=(operation_info_t&&) = default;
  auto result_shape() {
    return result_shape_;
  }
  auto result_nnz() {
    return result_nnz_;
  }
  void update_impl_(index<index_t> shape, std::int64_t nnz) {
    result_shape_ = shape;
    result_nnz_ = nnz;
  }

  std::unique_ptr<__gfx950::abstract_operation_state_t> state_;
  std::shared_ptr<spgemm_state_t> spgemm_;

  __gfx950::spmv_state_t& spmv_state() {
    auto* s = dynamic_cast<__gfx950::spmv_state_t*>(state_.get());
    if (!s) {
      state_ = std::make_unique<__gfx950::spmv_state_t>();
      s = static_cast<__gfx950::spmv_state_t*>(state_.get());
    }
    return *s;
  }

private:
  index<index_t> result_shape_{0, 0};
  std::int64_t result_nnz_ = 0;
};

// ---- SpMV ------------------------------------------------------------------------------------
namespace __gfx950 {

template <typename A>
using scalar_of_t = typename __detail::ultimate_base_type_t<A>::scalar_type;

inline void reject_conjugated(bool c) {
  if (c) {
    throw std::runtime_error("gfx950 backend does not support conjugated views.");  // spmv_impl.hpp:29-33
  }
}

template <typename A>
__gfx950::spmv_state_t* cached_state(A&& a) {
  if constexpr (__detail::is_opt<std::remove_cvref_t<A>>::value) {
    return a.cache().spmv.get();
  } else if constexpr (__detail::is_scaled<std::remove_cvref_t<A>>::value) {
    auto b = a.base();
    return cached_state(b);
  } else {
    return nullptr;
  }
}

} // namespace __gfx950

template <typename A, typename B, typename C>
  requires((__detail::has_csr_base<A> || __detail::has_csc_base<A>) && __detail::has_span_base<B> &&
           __detail::is_span<std::remove_cvref_t<C>>::value)
void multiply_inspect(operation_info_t& info, A&& a, B&& b, C&& c) {
  if constexpr (__detail::has_csr_base<A>) {
    auto ab = __detail::get_ultimate_base(a);
    using T = typename decltype(ab)::scalar_type;
    using O = typename decltype(ab)::offset_type;
    // a matrix_opt operand may get the plan that keeps a re-tiled copy of the values (value snapshot contract,
    // spblas_gfx950.h); a plain view gets a plan that reads the caller's values on every multiply
    constexpr bool opt = __detail::is_opt<std::remove_cvref_t<A>>::value;
    info.spmv_state().template inspect<T, O>(ab.shape()[0], ab.shape()[1], ab.size(), ab.rowptr().data(),
                                             ab.colind().data(), ab.values().data(), SPBLAS_GFX950_SPMV_AUTO, opt);
    if constexpr (opt) {  // cache in the matrix_opt as well
      a.cache().spmv = std::make_unique<__gfx950::spmv_state_t>();
      a.cache().spmv->template inspect<T, O>(ab.shape()[0], ab.shape()[1], ab.size(), ab.rowptr().data(),
                                             ab.colind().data(), ab.values().data(), SPBLAS_GFX950_SPMV_AUTO, true);
    }
  }
}

template <typename A, typename B, typename C>
  requires((__detail::has_csr_base<A> || __detail::has_csc_base<A>) && __detail::has_span_base<B> &&
           __detail::is_span<std::remove_cvref_t<C>>::value)
operation_info_t multiply_inspect(A&& a, B&& b, C&& c) {
  operation_info_t info;
  multiply_inspect(info, a, b, c);
  return info;
}

template <typename A, typename B, typename C>
  requires((__detail::has_csr_base<A> || __detail::has_csc_base<A>) && __detail::has_span_base<B> &&
           __detail::is_span<std::remove_cvref_t<C>>::value)
void multiply(operation_info_t& info, A&& a, B&& b, C&& c) {
  auto ab = __detail::get_ultimate_base(a);
  auto bb = __detail::get_ultimate_base(b);
  using T = typename decltype(ab)::scalar_type;
  using O = typename decltype(ab)::offset_type;
  __gfx950::reject_conjugated(__detail::is_conjugated(a) || __detail::is_conjugated(b));
  if (static_cast<std::size_t>(ab.shape()[0]) != c.size() || static_cast<std::size_t>(ab.shape()[1]) != bb.size()) {
    throw std::invalid_argument("multiply: matrix and vector dimensions are incompatible.");  // multiply_impl.hpp:37-41
  }
  const T alpha = static_cast<T>(__detail::get_scaling_factor(a, b).value_or(1.0));  // spmv_impl.hpp:35-37
  auto& state = info.spmv_state();
  if constexpr (__detail::has_csr_base<A>) {
    auto plan = state.plan_for(ab.shape()[0], ab.shape()[1], ab.size(), ab.rowptr().data(), ab.colind().data(),
                               ab.values().data());
    if (!plan) {
      if (auto* cached = __gfx950::cached_state(a)) {
        plan = cached->plan_for(ab.shape()[0], ab.shape()[1], ab.size(), ab.rowptr().data(), ab.colind().data(),
                                ab.values().data());
      }
    }
    __gfx950::spmv<T, O>(state.handle(), plan, SPBLAS_GFX950_OP_N, ab.shape()[0], ab.shape()[1], ab.size(), alpha,
                         ab.rowptr().data(), ab.colind().data(), ab.values().data(), bb.data(), T(0), c.data());
  } else {
    __gfx950::spmv<T, O>(state.handle(), nullptr, SPBLAS_GFX950_OP_T, ab.shape()[1], ab.shape()[0], ab.size(), alpha,
                         ab.colptr().data(), ab.rowind().data(), ab.values().data(), bb.data(), T(0), c.data());
  }
}

template <typename A, typename B, typename C>
  requires((__detail::has_csr_base<A> || __detail::has_csc_base<A>) && __detail::has_span_base<B> &&
           __detail::is_span<std::remove_cvref_t<C>>::value)
void multiply(A&& a, B&& b, C&& c) {
  operation_info_t info;
  multiply(info, a, b, c);
}

// ---- SpMM ------------------------------------------------------------------------------------
template <typename A, typename X, typename Y>
  requires(__detail::has_csr_base<A> && __detail::has_dense_base<X> && __detail::is_dense<std::remove_cvref_t<Y>>::value)
operation_info_t multiply_inspect(A&& a, X&& x, Y&& y) {
  operation_info_t info;
  auto ab = __detail::get_ultimate_base(a);
  using T = typename decltype(ab)::scalar_type;
  using O = typename decltype(ab)::offset_type;
  info.spmv_state().template inspect<T, O>(ab.shape()[0], ab.shape()[1], ab.size(), ab.rowptr().data(),
                                           ab.colind().data(), ab.values().data(), SPBLAS_GFX950_SPMV_ROWBLOCK);
  info.spmv_state().inspect_spmm();  // column-locality probe + long-row list (vendor/onemkl_sycl/spmm_impl.hpp:40-67)
  return info;
}

template <typename A, typename X, typename Y>
  requires(__detail::has_csr_base<A> && __detail::has_dense_base<X> && __detail::is_dense<std::remove_cvref_t<Y>>::value)
void multiply(operation_info_t& info, A&& a, X&& x, Y&& y) {
  auto ab = __detail::get_ultimate_base(a);
  auto xb = __detail::get_ultimate_base(x);
  using T = typename decltype(ab)::scalar_type;
  using O = typename decltype(ab)::offset_type;
  __gfx950::reject_conjugated(__detail::is_conjugated(a) || __detail::is_conjugated(x));
  if (ab.shape()[0] != y.extent(0) || xb.extent(1) != y.extent(1) || ab.shape()[1] != xb.extent(0)) {
    throw std::invalid_argument("multiply: matrix dimensions are incompatible.");  // multiply_impl.hpp:70-76
  }
  const T alpha = static_cast<T>(__detail::get_scaling_factor(a, x).value_or(1.0));
  auto plan = info.spmv_state().plan_for(ab.shape()[0], ab.shape()[1], ab.size(), ab.rowptr().data(), ab.colind().data(),
                                         ab.values().data());
  __gfx950::spmm<T, O>(info.spmv_state().handle(), plan, ab.shape()[0], ab.shape()[1], y.extent(1), ab.size(), alpha,
                       ab.rowptr().data(), ab.colind().data(), ab.values().data(), xb.data_handle(), xb.stride(0), T(0),
                       y.data_handle(), y.stride(0));
}

template <typename A, typename X, typename Y>
  requires(__detail::has_csr_base<A> && __detail::has_dense_base<X> && __detail::is_dense<std::remove_cvref_t<Y>>::value)
void multiply(A&& a, X&& x, Y&& y) {
  operation_info_t info;
  multiply(info, a, x, y);
}

// ---- scale (algorithms/scale_impl.hpp:13-31) ---------------------------------------------------
template <typename Scalar, typename T, typename I, typename O>
void scale(Scalar alpha, csr_view<T, I, O> a) {
  __gfx950::handle_t h;
  __gfx950::scale_values<T>(h, static_cast<std::int64_t>(a.size()), static_cast<T>(alpha), a.values().data());
}

template <typename Scalar, typename T, typename I, typename O>
void scale(Scalar alpha, csc_view<T, I, O> a) {
  __gfx950::handle_t h;
  __gfx950::scale_values<T>(h, static_cast<std::int64_t>(a.size()), static_cast<T>(alpha), a.values().data());
}

template <typename Scalar, typename T>
void scale(Scalar alpha, std::span<T> v) {
  __gfx950::handle_t h;
  __gfx950::scale_values<T>(h, static_cast<std::int64_t>(v.size()), static_cast<T>(alpha), v.data());
}

// ---- transpose (algorithms/transpose_impl.hpp:9-61) -------------------------------------------
template <typename A, typename B>
operation_info_t transpose_inspect(A&&, B&&) {
  return {};
}

template <typename T, typename I, typename O>
void transpose(csr_view<T, I, O> a, csr_view<T, I, O>& b) {
  if (a.shape()[0] != b.shape()[1] || a.shape()[1] != b.shape()[0]) {
    throw std::invalid_argument("transpose: matrix dimensions are incompatible.");
  }
  if (b.values().size() < static_cast<std::size_t>(a.size()) ||
      b.colind().size() < static_cast<std::size_t>(a.size())) {
    throw std::runtime_error("transpose: Transpose ran out of memory.");
  }
  __gfx950::handle_t h;
  __gfx950::csr_transpose<T>(h, a.shape()[0], a.shape()[1], a.size(), a.rowptr().data(), a.colind().data(),
                             a.values().data(), b.rowptr().data(), b.colind().data(), b.values().data());
  b.update(b.values(), b.rowptr(), b.colind(), b.shape(), a.size());
}

template <typename T, typename I, typename O>
void transpose(operation_info_t&, csr_view<T, I, O> a, csr_view<T, I, O>& b) {
  transpose(a, b);
}

// ---- SpGEMM ----------------------------------------------------------------------------------
class spgemm_state_t {
public:
  spgemm_state_t() : impl_(std::make_unique<__gfx950::spgemm_handle_t>()) {}
  explicit spgemm_state_t(void* hip_stream) : impl_(std::make_unique<__gfx950::spgemm_handle_t>(hip_stream)) {}
  auto result_shape() {
    return result_shape_;
  }
  auto result_nnz() {
    return result_nnz_;
  }

  template <typename A, typename B, typename C>
  void compute(A&& a, B&& b, C&& c) {
    impl_->set_addend(0, nullptr, nullptr);
    has_addend_ = false;
    compute_products(a, b, c);
  }

  template <typename A, typename B, typename C>
  void compute_products(A&& a, B&& b, C&& c) {
    auto ab = __detail::get_ultimate_base(a);
    auto bb = __detail::get_ultimate_base(b);
    __gfx950::reject_conjugated(__detail::is_conjugated(a) || __detail::is_conjugated(b));
    if (ab.shape()[0] != c.shape()[0] || bb.shape()[1] != c.shape()[1] || ab.shape()[1] != bb.shape()[0]) {
      throw std::invalid_argument("multiply: matrix dimensions are incompatible.");  // spgemm_gustavsons.hpp:22-27
    }
    result_nnz_ = impl_->symbolic(ab.shape()[0], ab.shape()[1], bb.shape()[1], ab.size(), ab.rowptr().data(),
                                  ab.colind().data(), bb.size(), bb.rowptr().data(), bb.colind().data(),
                                  c.rowptr().data());
    result_shape_ = index<index_t>(ab.shape()[0], bb.shape()[1]);
  }

  template <typename A, typename B, typename C>
  void numeric(A&& a, B&& b, C&& c) {
    auto ab = __detail::get_ultimate_base(a);
    auto bb = __detail::get_ultimate_base(b);
    using T = typename decltype(ab)::scalar_type;
    const T alpha = static_cast<T>(__detail::get_scaling_factor(a, b).value_or(1.0));
    const auto capacity = static_cast<std::int64_t>(std::min(c.values().size(), c.colind().size()));
    impl_->numeric<T>(alpha, ab.rowptr().data(), ab.colind().data(), ab.values().data(), bb.rowptr().data(),
                      bb.colind().data(), bb.values().data(), c.rowptr().data(), c.colind().data(), c.values().data(),
                      capacity);
    c.update(c.values(), c.rowptr(), c.colind(), c.shape(), static_cast<typename std::remove_cvref_t<C>::offset_type>(result_nnz_));
  }

  // C = alpha*A*B + beta*D (multiply_spgemm.hpp:118-214): alpha = scale(a)*scale(b), beta = scale(d)
  template <typename A, typename B, typename C, typename D>
  void compute(A&& a, B&& b, C&& c, D&& d) {
    auto db = __detail::get_ultimate_base(d);
    __gfx950::reject_conjugated(__detail::is_conjugated(d));
    if (db.shape()[0] != c.shape()[0] || db.shape()[1] != c.shape()[1]) {
      throw std::invalid_argument("multiply: matrix dimensions are incompatible.");
    }
    impl_->set_addend(db.size(), db.rowptr().data(), db.colind().data());
    has_addend_ = true;
    compute_products(a, b, c);
  }
  template <typename A, typename B, typename C, typename D>
  void numeric(A&& a, B&& b, C&& c, D&& d) {
    if (!has_addend_) {
      throw std::runtime_error("multiply_fill: the addend must be passed to multiply_compute as well");
    }
    auto ab = __detail::get_ultimate_base(a);
    auto bb = __detail::get_ultimate_base(b);
    auto db = __detail::get_ultimate_base(d);
    using T = typename decltype(ab)::scalar_type;
    const T alpha = static_cast<T>(__detail::get_scaling_factor(a, b).value_or(1.0));
    const T beta = static_cast<T>(__detail::get_scaling_factor(d).value_or(1.0));
    const auto capacity = static_cast<std::int64_t>(std::min(c.values().size(), c.colind().size()));
    impl_->numeric_addend<T>(alpha, ab.rowptr().data(), ab.colind().data(), ab.values().data(), bb.rowptr().data(),
                             bb.colind().data(), bb.values().data(), beta, db.rowptr().data(), db.colind().data(),
                             db.values().data(), c.rowptr().data(), c.colind().data(), c.values().data(), capacity);
    c.update(c.values(), c.rowptr(), c.colind(), c.shape(), static_cast<typename std::remove_cvref_t<C>::offset_type>(result_nnz_));
  }

  // add(a, b, c) (algorithms/add_impl.hpp:40-115)
  template <typename A, typename B, typename C>
  void add_symbolic(A&& a, B&& b, C&& c) {
    auto ab = __detail::get_ultimate_base(a);
    auto bb = __detail::get_ultimate_base(b);
    __gfx950::reject_conjugated(__detail::is_conjugated(a) || __detail::is_conjugated(b));
    if (ab.shape()[0] != bb.shape()[0] || ab.shape()[1] != bb.shape()[1] || bb.shape()[0] != c.shape()[0] ||
        bb.shape()[1] != c.shape()[1]) {
      throw std::invalid_argument("add: matrix dimensions are incompatible.");  // add_impl.hpp:44-47
    }
    result_nnz_ = impl_->add_symbolic(ab.shape()[0], ab.shape()[1], ab.size(), ab.rowptr().data(), ab.colind().data(),
                                      bb.size(), bb.rowptr().data(), bb.colind().data(), c.rowptr().data());
    result_shape_ = index<index_t>(ab.shape()[0], ab.shape()[1]);
    has_addend_ = true;
  }
  template <typename A, typename B, typename C>
  void add_numeric(A&& a, B&& b, C&& c) {
    auto ab = __detail::get_ultimate_base(a);
    auto bb = __detail::get_ultimate_base(b);
    using T = typename decltype(ab)::scalar_type;
    const T alpha = static_cast<T>(__detail::get_scaling_factor(a).value_or(1.0));
    const T beta = static_cast<T>(__detail::get_scaling_factor(b).value_or(1.0));
    const auto capacity = static_cast<std::int64_t>(std::min(c.values().size(), c.colind().size()));
    if (capacity < result_nnz_) {  // add_impl.hpp:67-72
      throw std::runtime_error("add: ran out of memory.  CSR output view has insufficient memory.");
    }
    impl_->add_numeric<T>(alpha, ab.rowptr().data(), ab.colind().data(), ab.values().data(), beta, bb.rowptr().data(),
                          bb.colind().data(), bb.values().data(), c.rowptr().data(), c.colind().data(),
                          c.values().data(), capacity);
    c.update(c.values(), c.rowptr(), c.colind(), c.shape(), static_cast<typename std::remove_cvref_t<C>::offset_type>(result_nnz_));
  }

private:
  std::unique_ptr<__gfx950::spgemm_handle_t> impl_;
  index<index_t> result_shape_{0, 0};
  std::int64_t result_nnz_ = 0;
  bool has_addend_ = false;
};

template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
void multiply_inspect(spgemm_state_t&, A&&, B&&, C&&) {}  // multiply_spgemm.hpp:232-235

template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
void multiply_compute(spgemm_state_t& s, A&& a, B&& b, C&& c) {
  s.compute(a, b, c);
}
template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
void multiply_fill(spgemm_state_t& s, A&& a, B&& b, C&& c) {
  s.numeric(a, b, c);
}
template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
void multiply_symbolic_compute(spgemm_state_t& s, A&& a, B&& b, C&& c) {
  s.compute(a, b, c);
}
template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
void multiply_symbolic_fill(spgemm_state_t& s, A&& a, B&& b, C&& c) {
  s.numeric(a, b, c);  // leaves C's structure (rowptr + colind) in the caller's arrays, multiply_spgemm.hpp:147-176
}
template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
void multiply_numeric(spgemm_state_t& s, A&& a, B&& b, C&& c) {
  s.numeric(a, b, c);
}

// four-argument family (multiply_spgemm.hpp:237-274)
template <typename A, typename B, typename C, typename D>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value &&
           __detail::has_csr_base<D>)
void multiply_compute(spgemm_state_t& s, A&& a, B&& b, C&& c, D&& d) {
  s.compute(a, b, c, d);
}
template <typename A, typename B, typename C, typename D>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value &&
           __detail::has_csr_base<D>)
void multiply_fill(spgemm_state_t& s, A&& a, B&& b, C&& c, D&& d) {
  s.numeric(a, b, c, d);
}
template <typename A, typename B, typename C, typename D>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value &&
           __detail::has_csr_base<D>)
void multiply_symbolic_compute(spgemm_state_t& s, A&& a, B&& b, C&& c, D&& d) {
  s.compute(a, b, c, d);
}
template <typename A, typename B, typename C, typename D>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value &&
           __detail::has_csr_base<D>)
void multiply_symbolic_fill(spgemm_state_t& s, A&& a, B&& b, C&& c, D&& d) {
  s.numeric(a, b, c, d);
}
template <typename A, typename B, typename C, typename D>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value &&
           __detail::has_csr_base<D>)
void multiply_numeric(spgemm_state_t& s, A&& a, B&& b, C&& c, D&& d) {
  s.numeric(a, b, c, d);
}

template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
void multiply_compute(operation_info_t& info, A&& a, B&& b, C&& c) {
  if (!info.spgemm_) {
    info.spgemm_ = std::make_shared<spgemm_state_t>();
  }
  info.spgemm_->compute(a, b, c);
  info.update_impl_(info.spgemm_->result_shape(), info.spgemm_->result_nnz());
}
template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
operation_info_t multiply_compute(A&& a, B&& b, C&& c) {
  operation_info_t info;
  multiply_compute(info, a, b, c);
  return info;
}
template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
void multiply_fill(operation_info_t& info, A&& a, B&& b, C&& c) {
  if (!info.spgemm_) {
    throw std::runtime_error("multiply_fill: info does not come from multiply_compute");
  }
  info.spgemm_->numeric(a, b, c);
}

// ---- add (algorithms/add.hpp:8-19, add_impl.hpp:40-115) ----------------------------------------
template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
void add_inspect(operation_info_t& info, A&& a, B&& b, C&& c) {
  if (!info.spgemm_) {
    info.spgemm_ = std::make_shared<spgemm_state_t>();
  }
  info.spgemm_->add_symbolic(a, b, c);
  info.update_impl_(info.spgemm_->result_shape(), info.spgemm_->result_nnz());
}
template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
operation_info_t add_inspect(A&& a, B&& b, C&& c) {
  operation_info_t info;
  add_inspect(info, a, b, c);
  return info;
}
template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
void add_compute(operation_info_t& info, A&& a, B&& b, C&& c) {
  if (!info.spgemm_) {
    throw std::runtime_error("add_compute: info does not come from add_inspect");
  }
  info.spgemm_->add_numeric(a, b, c);
}
template <typename A, typename B, typename C>
  requires(__detail::has_csr_base<A> && __detail::has_csr_base<B> && __detail::is_csr<std::remove_cvref_t<C>>::value)
void add(A&& a, B&& b, C&& c) {
  spgemm_state_t s;
  s.add_symbolic(a, b, c);
  s.add_numeric(a, b, c);
}

// ---- triangular_solve (algorithms/triangular_solve.hpp:8-19, triangular_solve_impl.hpp:13-107) ---
struct upper_triangle_t {  // detail/triangular_types.hpp:5-8
  explicit upper_triangle_t() = default;
};
inline constexpr upper_triangle_t upper_triangle{};
struct lower_triangle_t {  // :10-13
  explicit lower_triangle_t() = default;
};
inline constexpr lower_triangle_t lower_triangle{};
struct implicit_unit_diagonal_t {  // :15-18
  explicit implicit_unit_diagonal_t() = default;
};
inline constexpr implicit_unit_diagonal_t implicit_unit_diagonal{};
struct explicit_diagonal_t {  // :20-23
  explicit explicit_diagonal_t() = default;
};
inline constexpr explicit_diagonal_t explicit_diagonal{};

namespace __gfx950 {
template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
void trsv_prepare(trsv_state_t& st, A&& a, Triangle, DiagonalStorage, B&& b, X&& x) {
  static_assert(std::is_same_v<Triangle, upper_triangle_t> || std::is_same_v<Triangle, lower_triangle_t>);
  static_assert(std::is_same_v<DiagonalStorage, implicit_unit_diagonal_t> ||
                std::is_same_v<DiagonalStorage, explicit_diagonal_t>);
  auto ab = __detail::get_ultimate_base(a);
  reject_conjugated(__detail::is_conjugated(a));
  // the reference asserts these (triangular_solve_impl.hpp:50-53); a device backend has to refuse
  auto bb = __detail::get_ultimate_base(b);  // b may be scaled(beta, b) (examples/simple_sptrsv.cpp:49-53)
  if (ab.shape()[0] != ab.shape()[1] || static_cast<std::int64_t>(std::ranges::size(x)) != ab.shape()[1] ||
      static_cast<std::int64_t>(std::ranges::size(bb)) != ab.shape()[0]) {
    throw std::invalid_argument("triangular_solve: matrix and vector dimensions are incompatible.");
  }
  const int uplo = std::is_same_v<Triangle, upper_triangle_t> ? SPBLAS_GFX950_UPPER : SPBLAS_GFX950_LOWER;
  const int diag =
      std::is_same_v<DiagonalStorage, implicit_unit_diagonal_t> ? SPBLAS_GFX950_DIAG_UNIT : SPBLAS_GFX950_DIAG_EXPLICIT;
  if (!st.matches(ab.rowptr().data(), ab.colind().data(), ab.shape()[0], ab.size(), uplo, diag)) {
    st.inspect(ab.shape()[0], ab.size(), ab.rowptr().data(), ab.colind().data(), uplo, diag);
  }
}
inline trsv_state_t& trsv_state_of(operation_info_t& info) {
  auto* s = dynamic_cast<trsv_state_t*>(info.state_.get());
  if (!s) {
    info.state_ = std::make_unique<trsv_state_t>();
    s = static_cast<trsv_state_t*>(info.state_.get());
  }
  return *s;
}
} // namespace __gfx950

template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
  requires(__detail::has_csr_base<A>)
void triangular_solve_inspect(operation_info_t& info, A&& a, Triangle t, DiagonalStorage d, B&& b, X&& x) {
  __gfx950::trsv_prepare(__gfx950::trsv_state_of(info), a, t, d, b, x);
}
template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
  requires(__detail::has_csr_base<A>)
operation_info_t triangular_solve_inspect(A&& a, Triangle t, DiagonalStorage d, B&& b, X&& x) {
  operation_info_t info;
  triangular_solve_inspect(info, a, t, d, b, x);
  return info;
}
template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
  requires(__detail::has_csr_base<A>)
void triangular_solve(operation_info_t& info, A&& a, Triangle t, DiagonalStorage d, B&& b, X&& x) {
  auto& st = __gfx950::trsv_state_of(info);
  __gfx950::trsv_prepare(st, a, t, d, b, x);  // re-analyses only if the matrix / triangle changed
  auto ab = __detail::get_ultimate_base(a);
  using T = typename decltype(ab)::scalar_type;
  const T alpha = static_cast<T>(__detail::get_scaling_factor(a).value_or(1.0));
  // a scaled right-hand side: the solve is linear in b, so the factor is applied to x afterwards
  auto bb = __detail::get_ultimate_base(b);
  const auto beta = __detail::get_scaling_factor(b);
  st.template solve<T>(alpha, ab.rowptr().data(), ab.colind().data(), ab.values().data(), std::ranges::data(bb),
                       std::ranges::data(x));
  if (beta.has_value()) {
    __gfx950::handle_t h;
    __gfx950::scale_values<T>(h, static_cast<std::int64_t>(std::ranges::size(x)), static_cast<T>(*beta),
                              std::ranges::data(x));
  }
}
template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
  requires(__detail::has_csr_base<A>)
void triangular_solve(A&& a, Triangle t, DiagonalStorage d, B&& b, X&& x) {
  operation_info_t info;
  triangular_solve(info, a, t, d, b, x);
}

// ---- a block of right-hand sides: X(:, j) = inv(A) B(:, j) for every column in one solve (spblas_gfx950_sptrsm_solve).
// B (possibly scaled) and X are mdspan_row_major; the state is the vector solve's, so one info serves both forms. ----------
namespace __gfx950 {
template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
void trsm_prepare(trsv_state_t& st, A&& a, Triangle, DiagonalStorage, B&& b, X&& x) {
  static_assert(std::is_same_v<Triangle, upper_triangle_t> || std::is_same_v<Triangle, lower_triangle_t>);
  static_assert(std::is_same_v<DiagonalStorage, implicit_unit_diagonal_t> ||
                std::is_same_v<DiagonalStorage, explicit_diagonal_t>);
  auto ab = __detail::get_ultimate_base(a);
  auto bb = __detail::get_ultimate_base(b);
  static_assert(std::is_same_v<typename decltype(ab)::scalar_type, std::remove_cv_t<typename decltype(bb)::value_type>> &&
                    std::is_same_v<typename decltype(ab)::scalar_type, typename std::remove_cvref_t<X>::value_type>,
                "triangular_solve: B and X must have A's value type");
  reject_conjugated(__detail::is_conjugated(a) || __detail::is_conjugated(b));
  if (ab.shape()[0] != ab.shape()[1] || static_cast<std::int64_t>(x.extent(0)) != static_cast<std::int64_t>(ab.shape()[1]) ||
      static_cast<std::int64_t>(bb.extent(0)) != static_cast<std::int64_t>(ab.shape()[0]) || bb.extent(1) != x.extent(1)) {
    throw std::invalid_argument("triangular_solve: matrix and vector dimensions are incompatible.");
  }
  const int uplo = std::is_same_v<Triangle, upper_triangle_t> ? SPBLAS_GFX950_UPPER : SPBLAS_GFX950_LOWER;
  const int diag =
      std::is_same_v<DiagonalStorage, implicit_unit_diagonal_t> ? SPBLAS_GFX950_DIAG_UNIT : SPBLAS_GFX950_DIAG_EXPLICIT;
  if (!st.matches(ab.rowptr().data(), ab.colind().data(), ab.shape()[0], ab.size(), uplo, diag)) {
    st.inspect(ab.shape()[0], ab.size(), ab.rowptr().data(), ab.colind().data(), uplo, diag);
  }
}
} // namespace __gfx950

template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
  requires(__detail::has_csr_base<A> && __detail::has_dense_base<B> && __detail::is_dense<std::remove_cvref_t<X>>::value)
void triangular_solve_inspect(operation_info_t& info, A&& a, Triangle t, DiagonalStorage d, B&& b, X&& x) {
  __gfx950::trsm_prepare(__gfx950::trsv_state_of(info), a, t, d, b, x);
}
template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
  requires(__detail::has_csr_base<A> && __detail::has_dense_base<B> && __detail::is_dense<std::remove_cvref_t<X>>::value)
operation_info_t triangular_solve_inspect(A&& a, Triangle t, DiagonalStorage d, B&& b, X&& x) {
  operation_info_t info;
  triangular_solve_inspect(info, a, t, d, b, x);
  return info;
}
template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
  requires(__detail::has_csr_base<A> && __detail::has_dense_base<B> && __detail::is_dense<std::remove_cvref_t<X>>::value)
void triangular_solve(operation_info_t& info, A&& a, Triangle t, DiagonalStorage d, B&& b, X&& x) {
  auto& st = __gfx950::trsv_state_of(info);
  __gfx950::trsm_prepare(st, a, t, d, b, x);
  auto ab = __detail::get_ultimate_base(a);
  auto bb = __detail::get_ultimate_base(b);
  using T = typename decltype(ab)::scalar_type;
  const T alpha = static_cast<T>(__detail::get_scaling_factor(a).value_or(1.0));
  const auto beta = __detail::get_scaling_factor(b);
  st.template solve_matrix<T>(alpha, ab.rowptr().data(), ab.colind().data(), ab.values().data(), x.extent(1),
                              bb.data_handle(), bb.stride(0), bb.stride(1), x.data_handle(), x.stride(0), x.stride(1));
  if (beta.has_value()) {  // the solve is linear in B: the factor is applied to X afterwards
    __gfx950::handle_t h;
    __gfx950::scale_dense<T>(h, static_cast<T>(*beta), x.data_handle(), x.extent(0), x.extent(1), x.stride(0), x.stride(1));
  }
}
template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
  requires(__detail::has_csr_base<A> && __detail::has_dense_base<B> && __detail::is_dense<std::remove_cvref_t<X>>::value)
void triangular_solve(A&& a, Triangle t, DiagonalStorage d, B&& b, X&& x) {
  operation_info_t info;
  triangular_solve(info, a, t, d, b, x);
}

// ---- an APPROXIMATE triangular solve by Jacobi sweeps (spblas_gfx950_sptrsv_sweeps; no reference counterpart, hence
// spblas::gfx950).  x0_r = b_r / d_r, then `sweeps` times x_r = (b_r - the row's strict entries times the PREVIOUS x) / d_r; a
// row of level l is exact from sweep l on.  Vectors only; b must not be x.  An info that holds the result of
// triangular_solve_inspect for this matrix, triangle and diagonal narrows the later sweeps to the rows that can still change;
// any other info, and the overload without one, runs plan-free -- the call never inspects.  The second iterate lives in the
// info's state (allocated at the first call); the overload without info allocates and frees it around the call. ----------
namespace gfx950 {
template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
  requires(__detail::has_csr_base<A>)
void triangular_solve_sweeps(operation_info_t& info, A&& a, Triangle, DiagonalStorage, B&& b, X&& x, int sweeps) {
  static_assert(std::is_same_v<Triangle, upper_triangle_t> || std::is_same_v<Triangle, lower_triangle_t>);
  static_assert(std::is_same_v<DiagonalStorage, implicit_unit_diagonal_t> ||
                std::is_same_v<DiagonalStorage, explicit_diagonal_t>);
  auto ab = __detail::get_ultimate_base(a);
  auto bb = __detail::get_ultimate_base(b);
  __gfx950::reject_conjugated(__detail::is_conjugated(a));
  if (ab.shape()[0] != ab.shape()[1] || static_cast<std::int64_t>(std::ranges::size(x)) != ab.shape()[1] ||
      static_cast<std::int64_t>(std::ranges::size(bb)) != ab.shape()[0] || sweeps < 0) {
    throw std::invalid_argument("triangular_solve_sweeps: matrix and vector dimensions are incompatible.");
  }
  const int uplo = std::is_same_v<Triangle, upper_triangle_t> ? SPBLAS_GFX950_UPPER : SPBLAS_GFX950_LOWER;
  const int diag =
      std::is_same_v<DiagonalStorage, implicit_unit_diagonal_t> ? SPBLAS_GFX950_DIAG_UNIT : SPBLAS_GFX950_DIAG_EXPLICIT;
  using T = typename decltype(ab)::scalar_type;
  const T alpha = static_cast<T>(__detail::get_scaling_factor(a).value_or(1.0));
  const auto beta = __detail::get_scaling_factor(b);
  auto& st = __gfx950::trsv_state_of(info);
  st.template sweeps<T>(sweeps, uplo, diag, ab.shape()[0], ab.size(), alpha, ab.rowptr().data(), ab.colind().data(),
                        ab.values().data(), std::ranges::data(bb), std::ranges::data(x));
  if (beta.has_value()) {  // the iteration is linear in b: the factor is applied to x afterwards
    __gfx950::scale_values<T>(st.handle(), static_cast<std::int64_t>(std::ranges::size(x)), static_cast<T>(*beta),
                              std::ranges::data(x));
  }
}
template <typename A, typename Triangle, typename DiagonalStorage, typename B, typename X>
  requires(__detail::has_csr_base<A>)
void triangular_solve_sweeps(A&& a, Triangle t, DiagonalStorage d, B&& b, X&& x, int sweeps) {
  operation_info_t info;
  triangular_solve_sweeps(info, a, t, d, b, x, sweeps);
}
} // namespace gfx950

// ---- ILU(0): incomplete LU on A's own pattern (spblas_gfx950_ilu0_*; no reference counterpart, hence spblas::gfx950) --------
// A is a plain csr_view (float / double, int32 indices and offsets) with sorted rows and a stored diagonal in every row; LU is
// a csr_view over A's row offsets and columns with its own value array, or A itself (in place).  LU holds L left of the
// diagonal (unit diagonal implied) and U on and right of it: the ONE view serves
//   triangular_solve(lu, lower_triangle, implicit_unit_diagonal, b, y)  and  triangular_solve(lu, upper_triangle, explicit_diagonal, y, x).
namespace __gfx950 {
inline ilu0_state_t& ilu0_state_of(operation_info_t& info) {
  auto* s = dynamic_cast<ilu0_state_t*>(info.state_.get());
  if (!s) {
    info.state_ = std::make_unique<ilu0_state_t>();
    s = static_cast<ilu0_state_t*>(info.state_.get());
  }
  return *s;
}
template <typename T>
ilu0_state_t& ilu0_prepare(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "ilu0: float / double values only");
  if (a.shape()[0] != a.shape()[1]) {
    throw std::invalid_argument("ilu0: matrix dimensions are incompatible.");
  }
  auto& st = ilu0_state_of(info);
  if (!st.matches(a.rowptr().data(), a.colind().data(), a.shape()[0], a.size())) {
    st.inspect(a.shape()[0], a.size(), a.rowptr().data(), a.colind().data());
  }
  return st;
}
} // namespace __gfx950

namespace gfx950 {
template <typename T>
void ilu0_inspect(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a) {
  __gfx950::ilu0_prepare(info, a);
}
template <typename T>
operation_info_t ilu0_inspect(const csr_view<T, std::int32_t, std::int32_t>& a) {
  operation_info_t info;
  ilu0_inspect(info, a);
  return info;
}
template <typename T>
void ilu0(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a,
          const csr_view<T, std::int32_t, std::int32_t>& lu) {
  auto& st = __gfx950::ilu0_prepare(info, a);  // re-analyses only if the pattern changed
  if (lu.rowptr().data() != a.rowptr().data() || lu.colind().data() != a.colind().data() || lu.size() != a.size() ||
      lu.shape()[0] != a.shape()[0] || lu.shape()[1] != a.shape()[1]) {
    throw std::invalid_argument("ilu0: lu must be a view over A's own row offsets and columns.");
  }
  st.template factor<T>(a.rowptr().data(), a.colind().data(), a.values().data(), lu.values().data());
}
template <typename T>
void ilu0(const csr_view<T, std::int32_t, std::int32_t>& a, const csr_view<T, std::int32_t, std::int32_t>& lu) {
  operation_info_t info;
  ilu0(info, a, lu);
}
// An APPROXIMATE ilu0 by fixed-point sweeps (spblas_gfx950_ilu0_sweeps): LU(0) = A, then `sweeps` times every row runs ilu0's
// elimination on A's row with the pivots and pivot rows of the PREVIOUS iterate.  A row of level l has ilu0's bits from sweep l
// on: sweeps >= levels - 1 IS ilu0.  a, lu and work (at least a.size() elements; may be empty when sweeps == 1) are three
// different value arrays -- there is no in-place form.
template <typename T>
void ilu0_sweeps(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a,
                 const csr_view<T, std::int32_t, std::int32_t>& lu, std::type_identity_t<std::span<T>> work, int sweeps) {
  if (lu.rowptr().data() != a.rowptr().data() || lu.colind().data() != a.colind().data() || lu.size() != a.size() ||
      lu.shape()[0] != a.shape()[0] || lu.shape()[1] != a.shape()[1]) {
    throw std::invalid_argument("ilu0_sweeps: lu must be a view over A's own row offsets and columns.");
  }
  if (sweeps < 1) {
    throw std::invalid_argument("ilu0_sweeps: sweeps must be at least 1.");
  }
  if (sweeps >= 2 && work.size() < static_cast<std::size_t>(a.size())) {
    throw std::invalid_argument("ilu0_sweeps: work must hold at least A's number of entries.");
  }
  if (a.size() > 0 && (lu.values().data() == a.values().data() ||
                       (!work.empty() && (work.data() == a.values().data() || work.data() == lu.values().data())))) {
    throw std::invalid_argument("ilu0_sweeps: a, lu and work must be three different value arrays (no in-place form).");
  }
  auto& st = __gfx950::ilu0_prepare(info, a);  // after the argument checks; re-analyses only if the pattern changed
  st.template sweeps<T>(sweeps, a.rowptr().data(), a.colind().data(), a.values().data(), lu.values().data(),
                        work.empty() ? nullptr : work.data());
}
template <typename T>
void ilu0_sweeps(const csr_view<T, std::int32_t, std::int32_t>& a, const csr_view<T, std::int32_t, std::int32_t>& lu,
                 std::type_identity_t<std::span<T>> work, int sweeps) {
  operation_info_t info;
  ilu0_sweeps(info, a, lu, work, sweeps);
}
// synchronises the stream: the smallest row whose pivot was zero or not finite in the last ilu0 call with this info, else -1
inline std::int64_t ilu0_status(operation_info_t& info) {
  return __gfx950::ilu0_state_of(info).status();
}
} // namespace gfx950

// ---- multicolour ordering and symmetric permutation (spblas_gfx950_multicolor_* / csr_permute_* / permute_vector; no reference
// counterpart, hence spblas::gfx950) -----------------------------------------------------------------------------------------
// multicolor_order colours the graph of A + A^T at distance 1 (Jones-Plassmann with fixed priorities: the colours equal
// sequential greedy colouring in descending key order and depend on the pattern alone) and sorts the rows by colour.
// permute forms B = P A P^T with ascending columns: both triangles of B have at most `colors` levels for ilu0 / triangular_solve,
// at the price of a weaker ILU(0) preconditioner than in the natural order.  A is a square plain csr_view (float / double,
// int32 indices and offsets); perm, the result arrays and B's arrays are caller-allocated device memory.
namespace gfx950 {
struct multicolor_info_t {
  std::int64_t colors = 0, rounds = 0, max_color_size = 0, lanes_per_row = 0;
};
} // namespace gfx950

namespace __gfx950 {
template <typename State>
State& state_of(operation_info_t& info) {
  auto* s = dynamic_cast<State*>(info.state_.get());
  if (!s) {
    info.state_ = std::make_unique<State>();
    s = static_cast<State*>(info.state_.get());
  }
  return *s;
}
template <typename T>
permute_state_t& permute_prepare(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a,
                                 std::span<const std::int32_t> perm, const csr_view<T, std::int32_t, std::int32_t>& b) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "permute: float / double values only");
  if (a.shape()[0] != a.shape()[1] || b.shape()[0] != a.shape()[0] || b.shape()[1] != a.shape()[1] ||
      perm.size() != static_cast<std::size_t>(a.shape()[0])) {
    throw std::invalid_argument("permute: matrix dimensions are incompatible.");
  }
  if (b.rowptr().size() < static_cast<std::size_t>(a.shape()[0]) + 1 ||
      (a.size() > 0 && (b.colind().data() == nullptr || b.values().data() == nullptr))) {
    throw std::invalid_argument("permute: b must hold m + 1 row offsets and A's number of columns and values.");
  }
  auto& st = state_of<permute_state_t>(info);
  if (!st.matches(a.rowptr().data(), a.colind().data(), perm.data(), b.rowptr().data(), b.colind().data(), a.shape()[0],
                  a.size())) {
    st.inspect(a.shape()[0], a.size(), a.rowptr().data(), a.colind().data(), perm.data(), b.rowptr().data(),
               b.colind().data());
  }
  return st;
}
} // namespace __gfx950

namespace gfx950 {
// the inspect: synchronises the stream; the results stay in `info` until multicolor_copy fetches them
template <typename T>
multicolor_info_t multicolor_order(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "multicolor_order: float / double values only");
  if (a.shape()[0] != a.shape()[1]) {
    throw std::invalid_argument("multicolor_order: matrix dimensions are incompatible.");
  }
  auto& st = __gfx950::state_of<__gfx950::multicolor_state_t>(info);
  st.inspect(a.shape()[0], a.size(), a.rowptr().data(), a.colind().data());
  std::int64_t v[4];
  st.info(v);
  return multicolor_info_t{v[0], v[1], v[2], v[3]};
}
// perm (new -> old, sorted by (colour, old index)), inverse (old -> new), color: m elements; color_ptr: colors + 1.  An empty
// span is skipped.
inline void multicolor_copy(operation_info_t& info, std::span<std::int32_t> perm, std::span<std::int32_t> inverse,
                            std::span<std::int32_t> color, std::span<std::int32_t> color_ptr) {
  auto& st = __gfx950::state_of<__gfx950::multicolor_state_t>(info);
  std::int64_t v[4];
  st.info(v);
  const auto m = static_cast<std::size_t>(st.rows());
  if ((!perm.empty() && perm.size() < m) || (!inverse.empty() && inverse.size() < m) || (!color.empty() && color.size() < m) ||
      (!color_ptr.empty() && color_ptr.size() < static_cast<std::size_t>(v[0]) + 1)) {
    throw std::invalid_argument("multicolor_copy: an output is shorter than the result.");
  }
  st.copy(perm.empty() ? nullptr : perm.data(), inverse.empty() ? nullptr : inverse.data(),
          color.empty() ? nullptr : color.data(), color_ptr.empty() ? nullptr : color_ptr.data());
}
// writes B's row offsets and columns and keeps the source position of every entry (inspect-class: synchronises)
template <typename T>
void permute_inspect(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a,
                     std::type_identity_t<std::span<const std::int32_t>> perm,
                     const csr_view<T, std::int32_t, std::int32_t>& b) {
  __gfx950::permute_prepare(info, a, perm, b);
  info.update_impl_(a.shape(), a.size());
}
template <typename T>
operation_info_t permute_inspect(const csr_view<T, std::int32_t, std::int32_t>& a,
                                 std::type_identity_t<std::span<const std::int32_t>> perm,
                                 const csr_view<T, std::int32_t, std::int32_t>& b) {
  operation_info_t info;
  permute_inspect(info, a, perm, b);
  return info;
}
// with the info of permute_inspect for these arrays: only the value gather (one launch, capturable); otherwise inspects first
template <typename T>
void permute(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a,
             std::type_identity_t<std::span<const std::int32_t>> perm, const csr_view<T, std::int32_t, std::int32_t>& b) {
  auto& st = __gfx950::permute_prepare(info, a, perm, b);
  st.template values<T>(a.values().data(), b.values().data());
}
template <typename T>
void permute(const csr_view<T, std::int32_t, std::int32_t>& a, std::type_identity_t<std::span<const std::int32_t>> perm,
             const csr_view<T, std::int32_t, std::int32_t>& b) {
  operation_info_t info;
  permute(info, a, perm, b);
}
// inverse == false: dst[i] = src[perm[i]] (b into the new order); true: dst[perm[i]] = src[i] (x back).  src != dst.
template <typename T>
void permute_vector(std::span<const std::int32_t> perm, std::type_identity_t<std::span<const T>> src, std::span<T> dst,
                    bool inverse = false) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "permute_vector: float / double values only");
  if (src.size() != perm.size() || dst.size() != perm.size()) {
    throw std::invalid_argument("permute_vector: perm, src and dst must have one length.");
  }
  __gfx950::handle_t h;
  __gfx950::permute_vector_values<T>(h, static_cast<std::int64_t>(perm.size()), perm.data(), src.data(), dst.data(), inverse);
}
} // namespace gfx950

// ---- multicolour Gauss-Seidel / SOR / SSOR sweeps (spblas_gfx950_gs_*; no reference counterpart, hence spblas::gfx950) ---------
// sigma(i) = perm[i] when a perm was given, else i; colour c is the positions color_ptr[c] .. color_ptr[c + 1] - 1.  One row update:
//   dot = sum of a_rc x_c over the stored entries of row r with c != r (repeated off-diagonal entries are summed)
//   g = (b_r - dot) / d_r, d_r the row's one stored diagonal entry;  x_r = g when omega == 1 (the old x_r is not read), else
//   x_r = fma(omega, g - x_r, x_r).
// forward: colours 0 .. C - 1 one after the other, backward: C - 1 .. 0, symmetric: forward then backward; `sweeps` repeats that
// (0: x untouched, nothing launched).  x is updated in place, b only read, A's values read as they are at the call.  The result
// equals sequential Gauss-Seidel in colour order bit for bit and does not depend on the grid, earlier calls or graph capture.
// gauss_seidel_inspect checks (std::invalid_argument otherwise): color_ptr runs from 0 to m without descending (empty colours
// allowed); perm is a permutation; the offsets describe the entries, columns in [0, m); exactly one stored diagonal entry per
// row; no stored off-diagonal entry joins two rows of one colour.  gauss_seidel never inspects by itself: an info that is not a
// gauss_seidel_inspect of these row offsets and columns throws std::invalid_argument.  One symmetric sweep from x = 0 is SSOR.
// Not offered: a block of right-hand sides, weighted Jacobi, an implied zero initial guess, several colours per launch, scaled
// / complex / 16-bit / int64 / csc_view operands, distance-2 colourings.
namespace gfx950 {
// color_ptr (colours + 1) and perm (m, or empty) are int32 device arrays.  Inspect-class: allocates and synchronises.
template <typename T>
gauss_seidel_info_t gauss_seidel_inspect(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a,
                                         std::type_identity_t<std::span<const std::int32_t>> color_ptr,
                                         std::type_identity_t<std::span<const std::int32_t>> perm = {}) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "gauss_seidel: float / double values only");
  if (a.shape()[0] != a.shape()[1] || color_ptr.empty() ||
      (!perm.empty() && perm.size() != static_cast<std::size_t>(a.shape()[0]))) {
    throw std::invalid_argument("gauss_seidel_inspect: matrix dimensions are incompatible.");
  }
  auto& st = __gfx950::state_of<__gfx950::gs_state_t>(info);
  st.inspect(a.shape()[0], a.size(), a.rowptr().data(), a.colind().data(), static_cast<std::int64_t>(color_ptr.size()) - 1,
             color_ptr.data(), perm.empty() ? nullptr : perm.data());
  info.update_impl_(a.shape(), a.size());
  std::int64_t v[4];
  st.info(v);
  return gauss_seidel_info_t{v[0], v[1], v[2], v[3]};
}
// b and x: m elements of A's type in device memory, different buffers.  Capturable from the first call.
template <typename T>
void gauss_seidel(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a,
                  std::type_identity_t<std::span<const T>> b, std::type_identity_t<std::span<T>> x, int sweeps = 1,
                  std::type_identity_t<T> omega = T(1), gs_direction direction = gs_direction::forward) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "gauss_seidel: float / double values only");
  const auto m = static_cast<std::size_t>(a.shape()[0]);
  if (a.shape()[0] != a.shape()[1] || b.size() != m || x.size() != m) {
    throw std::invalid_argument("gauss_seidel: matrix dimensions are incompatible.");
  }
  auto* st = dynamic_cast<__gfx950::gs_state_t*>(info.state_.get());
  if (!st || !st->matches(a.rowptr().data(), a.colind().data(), a.shape()[0], a.size())) {
    throw std::invalid_argument("gauss_seidel: info must be the result of gauss_seidel_inspect for these row offsets and columns");
  }
  if (sweeps < 0 || (m > 0 && b.data() == x.data())) {
    throw std::invalid_argument("gauss_seidel: sweeps must not be negative and b and x must be different buffers");
  }
  st->template sweep<T>(sweeps, static_cast<int>(direction), omega, a.values().data(), b.data(), x.data());
}
} // namespace gfx950

// ---- MIS-2 aggregation and the Galerkin coarse matrix (spblas_gfx950_aggregate_* / coarsen_*; no reference counterpart, hence
// spblas::gfx950) ---------------------------------------------------------------------------------------------------------------
// aggregate groups the rows of A around the roots of a maximal independent set at distance 2 of the strength graph: in the value
// type T, d_i the first stored diagonal entry of row i (0 without one), t2 = T(theta * theta), a stored off-diagonal a_ij is
// strong iff a_ij * a_ij >= (t2 * |d_i|) * |d_j| (NaN: weak); i ~ j iff a_ij or a_ji is strong.  The roots are greedy MIS on the
// square of that graph in descending order of multicolor_order's fixed keys: roots, aggregates and rounds depend on the pattern,
// the values and theta alone.  coarsen forms A_c = P^T A P for the piecewise-constant P of ANY int32 map agg with entries in
// [0, n_agg): coarsen_inspect sizes A_c, coarsen_structure writes its row offsets and ascending columns, coarsen writes VALUES
// only -- every coarse entry is the sum of its terms in ascending source position, plain additions from the first term: one
// launch, capturable, the same bits on every call.  All operands are plain csr_views (float / double, int32 indices and offsets)
// over caller-allocated device memory.
namespace gfx950 {
struct aggregate_info_t {
  std::int64_t aggregates = 0, rounds = 0, largest = 0, smallest = 0, singletons = 0, strong_entries = 0, lanes_per_row = 0;
};
struct coarsen_info_t {
  std::int64_t rows = 0, nnz = 0;  // A_c is rows x rows with nnz entries
};
// the inspect: synchronises the stream; the results stay in `info` until aggregate_copy / prolongator fetch them
template <typename T>
aggregate_info_t aggregate(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a, double theta = 0.0) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "aggregate: float / double values only");
  if (a.shape()[0] != a.shape()[1]) {
    throw std::invalid_argument("aggregate: matrix dimensions are incompatible.");
  }
  auto& st = __gfx950::state_of<__gfx950::aggregate_state_t>(info);
  st.inspect(a.shape()[0], a.size(), a.rowptr().data(), a.colind().data(), a.values().data(), theta);
  std::int64_t v[8];
  st.info(v);
  return aggregate_info_t{v[0], v[1], v[2], v[3], v[4], v[5], v[6]};
}
// agg: m elements; root (the root row of every aggregate, ascending): aggregates elements.  An empty span is skipped.
inline void aggregate_copy(operation_info_t& info, std::span<std::int32_t> agg, std::span<std::int32_t> root) {
  auto& st = __gfx950::state_of<__gfx950::aggregate_state_t>(info);
  std::int64_t v[8];
  st.info(v);
  if ((!agg.empty() && agg.size() < static_cast<std::size_t>(st.rows())) ||
      (!root.empty() && root.size() < static_cast<std::size_t>(v[0]))) {
    throw std::invalid_argument("aggregate_copy: an output is shorter than the result.");
  }
  st.copy(agg.empty() ? nullptr : agg.data(), root.empty() ? nullptr : root.data());
}
// the tentative prolongator P (m x aggregates): row offsets 0 .. m, columns agg, values 1.  One launch, capturable.
template <typename T>
void prolongator(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& p) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "prolongator: float / double values only");
  auto& st = __gfx950::state_of<__gfx950::aggregate_state_t>(info);
  const auto m = static_cast<std::size_t>(st.rows());
  if (p.rowptr().size() < m + 1 || p.colind().size() < m || p.values().size() < m) {
    throw std::invalid_argument("prolongator: p must hold m + 1 row offsets and m columns and values.");
  }
  st.template prolongator<T>(p.rowptr().data(), p.colind().data(), p.values().data());
}
// the structure of A_c for any map agg with entries in [0, n_agg) (inspect-class: synchronises)
template <typename T>
coarsen_info_t coarsen_inspect(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a,
                               std::type_identity_t<std::span<const std::int32_t>> agg, std::int64_t n_agg) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "coarsen_inspect: float / double values only");
  if (a.shape()[0] != a.shape()[1] || agg.size() != static_cast<std::size_t>(a.shape()[0])) {
    throw std::invalid_argument("coarsen_inspect: matrix dimensions are incompatible.");
  }
  auto& st = __gfx950::state_of<__gfx950::coarsen_state_t>(info);
  st.inspect(a.shape()[0], a.size(), a.rowptr().data(), a.colind().data(), agg.data(), n_agg);
  info.update_impl_({static_cast<index_t>(n_agg), static_cast<index_t>(n_agg)}, st.coarse_nnz());
  return coarsen_info_t{st.coarse_rows(), st.coarse_nnz()};
}
// A_c's row offsets and its ascending, duplicate-free columns into caller-allocated arrays; copies on the stream, capturable
template <typename T>
void coarsen_structure(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a_c) {
  auto& st = __gfx950::state_of<__gfx950::coarsen_state_t>(info);
  if (!st.ready()) {
    throw std::invalid_argument("coarsen_structure: info must come from coarsen_inspect.");
  }
  if (a_c.rowptr().size() < static_cast<std::size_t>(st.coarse_rows()) + 1 ||
      a_c.colind().size() < static_cast<std::size_t>(st.coarse_nnz())) {
    throw std::invalid_argument("coarsen_structure: a_c must hold n_agg + 1 row offsets and nnz(A_c) columns.");
  }
  st.structure(a_c.rowptr().data(), a_c.colind().data());
}
// VALUES only.  With an info made for other row offset / column arrays the same aggregation is inspected again first
// (inspect-class); otherwise one launch, capturable.
template <typename T>
void coarsen(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a,
             const csr_view<T, std::int32_t, std::int32_t>& a_c) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "coarsen: float / double values only");
  auto& st = __gfx950::state_of<__gfx950::coarsen_state_t>(info);
  if (!st.ready()) {
    throw std::invalid_argument("coarsen: info must come from coarsen_inspect.");
  }
  if (a.shape()[0] != a.shape()[1] || a.shape()[0] != st.fine_rows() || static_cast<std::int64_t>(a.size()) != st.fine_nnz()) {
    throw std::invalid_argument("coarsen: matrix dimensions are incompatible.");
  }
  if (!st.matches(a.rowptr().data(), a.colind().data(), st.agg(), st.fine_rows(), st.fine_nnz(), st.coarse_rows())) {
    st.reinspect(a.rowptr().data(), a.colind().data());
  }
  if (a_c.values().size() < static_cast<std::size_t>(st.coarse_nnz())) {
    throw std::invalid_argument("coarsen: a_c must hold nnz(A_c) values.");
  }
  st.template values<T>(a.values().data(), a_c.values().data());
}

// ---- the smoothed prolongator of smoothed aggregation (spblas_gfx950_smooth_*; no reference counterpart) ----------------------
// P = (I - omega D_F^-1 A_F) T for the piecewise-constant T of ANY int32 map agg into [0, n_agg): A_F is A with its weak
// off-diagonal entries (the strength rule above) removed and added to the diagonal, D_F its diagonal.  smooth_prolongator_inspect
// sizes P (value-free), smooth_prolongator_structure writes its row offsets and ascending columns, smooth_prolongator writes
// VALUES only, fixed to the bit (include/spblas_gfx950.h, smooth_values): two launches, capturable.  One info serves one stream
// at a time.
// (smooth_prolongator_info_t {rows, columns, nnz} comes with the backend calls.)
template <typename T>
smooth_prolongator_info_t smooth_prolongator_inspect(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a,
                                                     std::type_identity_t<std::span<const std::int32_t>> agg,
                                                     std::int64_t n_agg) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "smooth_prolongator_inspect: float / double values only");
  if (a.shape()[0] != a.shape()[1] || agg.size() != static_cast<std::size_t>(a.shape()[0])) {
    throw std::invalid_argument("smooth_prolongator_inspect: matrix dimensions are incompatible.");
  }
  auto& st = __gfx950::state_of<__gfx950::smooth_state_t>(info);
  st.inspect(a.shape()[0], a.size(), a.rowptr().data(), a.colind().data(), agg.data(), n_agg);
  info.update_impl_({static_cast<index_t>(a.shape()[0]), static_cast<index_t>(n_agg)}, st.p_nnz());
  return smooth_prolongator_info_t{st.fine_rows(), st.columns(), st.p_nnz()};
}
template <typename T>
void smooth_prolongator_structure(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& p) {
  auto& st = __gfx950::state_of<__gfx950::smooth_state_t>(info);
  if (!st.ready()) {
    throw std::invalid_argument("smooth_prolongator_structure: info must come from smooth_prolongator_inspect.");
  }
  if (p.rowptr().size() < static_cast<std::size_t>(st.fine_rows()) + 1 ||
      p.colind().size() < static_cast<std::size_t>(st.p_nnz())) {
    throw std::invalid_argument("smooth_prolongator_structure: p must hold m + 1 row offsets and nnz(P) columns.");
  }
  st.structure(p.rowptr().data(), p.colind().data());
}
// With an info made for other row offset / column arrays the same aggregation is inspected again first (inspect-class).
template <typename T>
void smooth_prolongator(operation_info_t& info, const csr_view<T, std::int32_t, std::int32_t>& a,
                        const csr_view<T, std::int32_t, std::int32_t>& p, std::type_identity_t<T> omega, double theta = 0.0) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "smooth_prolongator: float / double values only");
  auto& st = __gfx950::state_of<__gfx950::smooth_state_t>(info);
  if (!st.ready()) {
    throw std::invalid_argument("smooth_prolongator: info must come from smooth_prolongator_inspect.");
  }
  if (a.shape()[0] != a.shape()[1] || a.shape()[0] != st.fine_rows() || static_cast<std::int64_t>(a.size()) != st.fine_nnz()) {
    throw std::invalid_argument("smooth_prolongator: matrix dimensions are incompatible.");
  }
  if (!st.matches(a.rowptr().data(), a.colind().data())) {
    st.reinspect(a.rowptr().data(), a.colind().data());
  }
  if (p.values().size() < static_cast<std::size_t>(st.p_nnz())) {
    throw std::invalid_argument("smooth_prolongator: p must hold nnz(P) values.");
  }
  st.template values<T>(a.rowptr().data(), a.colind().data(), a.values().data(), omega, theta, p.values().data());
}
} // namespace gfx950

} // namespace spblas
