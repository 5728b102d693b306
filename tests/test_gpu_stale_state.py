"""-m gpu: state the library keeps between calls must not go stale.

1. The int32 copy of an int64 index array (api._int32_columns).  A plan-free multiply(a, x, y) reads the caller's arrays as
   they are at the time of the call, so indices edited in place between two multiplies -- copy_ into a reused buffer, one
   element assigned -- must show in the second result, an edit to a value outside the matrix must raise like a fresh tensor
   does, and neither the int64 tensor nor its copy may outlive the operand.  A plan binds the structure (the reference's
   inspect does too): int64 indices edited in place after multiply_inspect are a user error, which this layer sees and
   reports (ValueError) instead of multiplying with the old structure; a new multiply_inspect takes the new structure.
   Every comparison is against the float64 product of the NEW structure, bound of util.assert_parity.

   The C++ layer keeps its narrowed copy in the operation_info state (wide_spmv_state_t::columns, keyed by the array's
   address).  A plan-free C++ multiply(a, x, y) creates that state for the one call and drops it on return, so it cannot
   reuse a copy across calls: no C++ case is needed for the plan-free form.  With an info the structure is bound at the
   first call that sees the array (with or without an inspect), and the C++ layer has no way to see a later edit.

2. The step wait armed by spblas_gfx950_bcast_wait_before belongs to the next spblas_gfx950_spmv_reduce_rows_bcast and
   must be launched before the kernel that stores into the peers' copies of y, whatever form the plan has.  Checked
   through the C ABI in one process: the wait is armed on a flag word nobody advances, with a timeout of 50 ms of the
   library's own bounded wait and a status word; after the call the status word must report the timeout (the same
   bounded, reported wait test_a_solve_that_gave_up_waiting_is_reported relies on: nothing hangs).  On a value-free plan
   and on a plan that owns its values.
"""
import ctypes
import gc
import os

import numpy as np
import pytest
import torch

import gpu_util as G
import spblas_reference_amd as sp
import util
from oracle import oracle
from spblas_reference_amd import _capi, generate

pytestmark = pytest.mark.gpu

M, N, PER, NB = 3000, 5000, 12, 24


def _matrix(dtype, seed=5):
    values, rowptr, colind, shape, nnz = generate.generate_csr(M, N, M * PER, seed=seed)
    values = ((values / 100.0) - 0.5).astype(dtype)
    return values, rowptr, colind, shape, nnz


def _edited(colind, weight, x_h, edit, rng, bound):
    """The index array after the edit: `copy_` -> every index drawn again; `element` -> the index of the entry with the
    largest `weight` moved to a column whose x differs by more than 0.25 (so that the old structure's result is far
    outside the bound)."""
    new = colind.astype(np.int64).copy()
    if edit == "copy_":
        new[:] = rng.integers(0, bound, new.size)
        return new, None
    k = int(np.argmax(weight))
    far = np.flatnonzero(np.abs(x_h - x_h[new[k]]) > 0.25)
    new[k] = far[0]
    return new, k


def _apply(idx_t, new, k, edit):
    if edit == "copy_":
        idx_t.copy_(G.dev(new))
    else:
        idx_t[k] = int(new[k])


def _spmv_check(a, x, x_h, shape, rowptr, colind, values, dtype, what):
    y = torch.full((shape[0],), float("nan"), dtype=x.dtype, device="cuda")
    sp.multiply(a, x, y)
    ref = oracle.spmv(shape, rowptr, colind.astype(np.int32), values, x_h)
    absrow = oracle.spmv_absrow(rowptr, colind.astype(np.int32), values, x_h)
    util.assert_parity(G.host(y), ref, absrow, dtype, row_len=np.diff(rowptr), what=what)


def _spmm_check(a, B, B_h, shape, rowptr, colind, values, dtype, what):
    C = torch.full((shape[0], NB), float("nan"), dtype=B.dtype, device="cuda")
    sp.multiply(a, B, C)
    ci = colind.astype(np.int32)
    ref = oracle.spmm(shape, rowptr, ci, values, B_h)
    absr = oracle.spmm(shape, rowptr, ci, np.abs(values), np.abs(B_h))
    util.assert_parity(G.host(C), ref, absr, dtype, row_len=np.diff(rowptr), what=what)


def _csc_check(a_csc, xt, xt_h, shape, rowptr, colind, values, dtype, what):
    """The CSR arrays read as a csc_view of the (n, m) transpose: y = A^T x (atomic scatter; bound with the longest column)."""
    m, n = shape
    yt = torch.full((n,), float("nan"), dtype=xt.dtype, device="cuda")
    sp.multiply(a_csc, xt, yt)
    ci = colind.astype(np.int32)
    ref = oracle.spmv_csc((n, m), rowptr, ci, values, xt_h)
    absr = oracle.spmv_csc((n, m), rowptr, ci, np.abs(values), np.abs(xt_h))
    col_len = np.bincount(colind, minlength=n)
    util.assert_parity(G.host(yt), ref, absr, dtype, row_len=col_len, what=what)


@pytest.mark.parametrize("edit", ["copy_", "element"])
@pytest.mark.parametrize("offsets", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_plan_free_multiplies_read_int64_indices_as_they_are_now(gpu, dtype, offsets, edit):
    rng = np.random.default_rng(11)
    values, rowptr, colind, shape, nnz = _matrix(dtype)
    x_h = (rng.random(N) - 0.5).astype(dtype)
    xt_h = (rng.random(M) - 0.5).astype(dtype)
    B_h = (rng.random((N, NB)) - 0.5).astype(dtype)
    x, xt, B = G.dev(x_h), G.dev(xt_h), G.dev(B_h)
    vals_d, rp_d = G.dev(values), G.dev(rowptr.astype(offsets))
    for form in ("spmv", "spmm", "csc"):
        ci64 = G.dev(colind.astype(np.int64))          # a fresh index tensor per form: each sees a first multiply, then the edit
        if form == "csc":
            a = sp.csc_view(vals_d, rp_d, ci64, (N, M), nnz)
            run = lambda ci, what: _csc_check(a, xt, xt_h, shape, rowptr, ci, values, dtype, what)
            # (here the index names the row of y an entry adds values * xt[its row] to: the entry with the largest such term)
            new, k = _edited(colind, np.abs(values * np.repeat(xt_h, np.diff(rowptr))), x_h, edit, rng, N)
        else:
            a = sp.csr_view(vals_d, rp_d, ci64, shape, nnz)
            if form == "spmv":
                run = lambda ci, what: _spmv_check(a, x, x_h, shape, rowptr, ci, values, dtype, what)
            else:
                run = lambda ci, what: _spmm_check(a, B, B_h, shape, rowptr, ci, values, dtype, what)
            new, k = _edited(colind, np.abs(values), B_h[:, 0] if form == "spmm" else x_h, edit, rng, N)
        run(colind, f"{form}: first multiply")
        _apply(ci64, new, k, edit)
        run(new, f"{form}: multiply after {edit} into the same int64 index tensor")
        _apply(ci64, colind.astype(np.int64), k, edit)  # ... and back again: a third version of the same tensor
        run(colind, f"{form}: multiply after the edit was undone")


@pytest.mark.parametrize("bad", ["n", "2**32+7"])
@pytest.mark.parametrize("offsets", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_an_index_edited_to_outside_the_matrix_raises_on_the_next_multiply(gpu, dtype, offsets, bad):
    values, rowptr, colind, shape, nnz = _matrix(dtype)
    bad_value = N if bad == "n" else (1 << 32) + 7     # the second would wrap to column 7
    rng = np.random.default_rng(3)
    x, B = G.dev((rng.random(N) - 0.5).astype(dtype)), G.dev((rng.random((N, NB)) - 0.5).astype(dtype))
    xt = G.dev((rng.random(M) - 0.5).astype(dtype))
    y = torch.empty(M, dtype=x.dtype, device="cuda")
    yt = torch.empty(N, dtype=x.dtype, device="cuda")
    C = torch.empty((M, NB), dtype=x.dtype, device="cuda")
    ci64 = G.dev(colind.astype(np.int64))
    a = sp.csr_view(G.dev(values), G.dev(rowptr.astype(offsets)), ci64, shape, nnz)
    a_csc = sp.csc_view(a.values(), a.rowptr(), ci64, (N, M), nnz)
    for run in (lambda: sp.multiply(a, x, y), lambda: sp.multiply(a, B, C), lambda: sp.multiply(a_csc, xt, yt)):
        run()                                           # valid indices: the copy is made and kept
        ci64[4321] = bad_value
        with pytest.raises(ValueError, match="outside the matrix"):
            run()
        with pytest.raises(ValueError, match="outside the matrix"):
            run()                                       # ... and again: the refused copy was not kept either
        ci64[4321] = int(colind[4321])
        run()
    torch.cuda.synchronize()


def test_the_same_index_tensor_in_a_narrower_view_is_range_checked_again(gpu):
    """The copy is tied to the bound it was checked against: after a multiply on an (M, N) view, the same int64 tensor in an
    (M, N - 1000) view -- where some of its indices lie outside the matrix -- raises, and the wide view still works."""
    values, rowptr, colind, shape, nnz = _matrix(np.float32)
    assert colind.max() >= N - 1000
    ci64 = G.dev(colind.astype(np.int64))
    vals_d, rp_d = G.dev(values), G.dev(rowptr)
    x = torch.rand(N, device="cuda")
    y = torch.empty(M, device="cuda")
    sp.multiply(sp.csr_view(vals_d, rp_d, ci64, (M, N), nnz), x, y)
    with pytest.raises(ValueError, match="outside the matrix"):
        sp.multiply(sp.csr_view(vals_d, rp_d, ci64, (M, N - 1000), nnz), x[:N - 1000].contiguous(), y)
    x_h = G.host(x)
    _spmv_check(sp.csr_view(vals_d, rp_d, ci64, (M, N), nnz), x, x_h, shape, rowptr, colind, values, np.float32, "wide view again")


def test_the_narrowed_copy_does_not_outlive_the_operand(gpu):
    """2^22 x 2^22, 4 entries per row: the int64 indices are 128 MiB, their int32 copy 64 MiB, x and y 16 MiB each.  After the
    operand and its tensors are dropped, torch's allocated bytes must be back within the size of x and y of the reading
    taken before the operand existed -- so neither the int64 tensor nor the copy is still held."""
    m = 1 << 22
    torch.cuda.synchronize()
    gc.collect()
    before = torch.cuda.memory_allocated()
    x = torch.rand(m, device="cuda")
    y = torch.empty(m, device="cuda")
    values, rowptr, colind, shape, nnz = generate.uniform_csr_device(m, m, 4, device="cuda", seed=2)
    ci64 = colind.long()
    del colind
    a = sp.csr_view(values, rowptr, ci64, shape, nnz)
    sp.multiply(a, x, y)
    torch.cuda.synchronize()
    key = id(ci64)
    assert key in sp.api._NARROWED
    held = torch.cuda.memory_allocated() - before
    assert held >= nnz * 12, held                       # the copy exists while the operand does (12 B per entry with the int64s)
    # spot check of the product itself: the rows of the first 1000 and last 1000
    rows = torch.cat([torch.arange(1000), torch.arange(m - 1000, m)]).cuda()
    pos = (rowptr[rows].long()[:, None] + torch.arange(4, device="cuda")[None, :])
    ref = (values[pos].double() * x[ci64[pos]].double()).sum(1)
    absr = (values[pos].double() * x[ci64[pos]].double()).abs().sum(1)
    util.assert_parity(G.host(y[rows]), G.host(ref), G.host(absr), np.float32, what="2^22 rows, int64 columns")
    del a, values, rowptr, ci64, rows, pos, ref, absr
    gc.collect()
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    print(f"allocated: before {before}, with the operand +{held}, after {after} (x and y: {x.nbytes + y.nbytes})")
    assert after - before <= x.nbytes + y.nbytes, (before, after, after - before)
    assert key not in sp.api._NARROWED, "the entry of the narrowing cache outlived its index tensor"


@pytest.mark.parametrize("offsets", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_int64_indices_edited_after_inspect_raise_and_a_new_inspect_follows_them(gpu, dtype, offsets):
    """The plan binds the structure.  multiply(info, a, ...) after an in-place edit of the int64 indices raises (never the old
    structure's result); multiply_inspect again and the new structure is used, through THE plan.  A csr_view (forced
    row-block and SLICED plans, matrix_opt), SpMM, and a csc_view."""
    rng = np.random.default_rng(17)
    values, rowptr, colind, shape, nnz = _matrix(dtype)
    x_h = (rng.random(N) - 0.5).astype(dtype)
    xt_h = (rng.random(M) - 0.5).astype(dtype)
    B_h = (rng.random((N, NB)) - 0.5).astype(dtype)
    x, xt, B = G.dev(x_h), G.dev(xt_h), G.dev(B_h)
    new = rng.integers(0, N, nnz).astype(np.int64)
    lens = np.diff(rowptr)

    def spmv_ref(ci):
        ci = ci.astype(np.int32)
        return oracle.spmv(shape, rowptr, ci, values, x_h), oracle.spmv_absrow(rowptr, ci, values, x_h)

    for name, alg in (("rowblock", _capi.SPMV_ROWBLOCK), ("sliced", _capi.SPMV_SLICED), ("matrix_opt", None)):
        ci64 = G.dev(colind.astype(np.int64))
        a = sp.csr_view(G.dev(values), G.dev(rowptr.astype(offsets)), ci64, shape, nnz)
        op = sp.matrix_opt(a) if alg is None else a
        y = torch.full((M,), float("nan"), dtype=x.dtype, device="cuda")
        info = sp.multiply_inspect(op, x, y) if alg is None else sp.multiply_inspect(op, x, y, alg=alg)
        if alg is not None:
            assert info.state_.info()["alg"] == alg
        sp.multiply(info, op, x, y)
        util.assert_parity(G.host(y), *spmv_ref(colind), dtype, row_len=lens, what=f"{name}: inspected, before the edit")
        ci64.copy_(G.dev(new))
        with pytest.raises(ValueError, match="modified in place after multiply_inspect"):
            sp.multiply(info, op, x, y)
        if alg is None:                                  # the plan a matrix_opt carries is bound in the same way
            with pytest.raises(ValueError, match="modified in place after multiply_inspect"):
                sp.multiply(op, x, y)
        info = sp.multiply_inspect(op, x, y) if alg is None else sp.multiply_inspect(op, x, y, alg=alg)
        y.fill_(float("nan"))
        sp.multiply(info, op, x, y)
        util.assert_parity(G.host(y), *spmv_ref(new), dtype, row_len=lens, what=f"{name}: inspected again after the edit")
        assert sp.api._find_plan(info, op, sp.api._int32_columns(a, "t")) is info.state_   # the multiply used THE plan
    # SpMM
    ci64 = G.dev(colind.astype(np.int64))
    a = sp.csr_view(G.dev(values), G.dev(rowptr.astype(offsets)), ci64, shape, nnz)
    C = torch.full((M, NB), float("nan"), dtype=x.dtype, device="cuda")
    info = sp.multiply_inspect(a, B, C)
    sp.multiply(info, a, B, C)
    ci64.copy_(G.dev(new))
    with pytest.raises(ValueError, match="modified in place after multiply_inspect"):
        sp.multiply(info, a, B, C)
    info = sp.multiply_inspect(a, B, C)
    C.fill_(float("nan"))
    sp.multiply(info, a, B, C)
    ci = new.astype(np.int32)
    util.assert_parity(G.host(C), oracle.spmm(shape, rowptr, ci, values, B_h),
                       oracle.spmm(shape, rowptr, ci, np.abs(values), np.abs(B_h)), dtype, row_len=lens,
                       what="SpMM: inspected again after the edit")
    # csc_view (the inspect materialises the row-major form from the narrowed copy)
    ci64 = G.dev(colind.astype(np.int64))
    a_csc = sp.csc_view(G.dev(values), G.dev(rowptr.astype(offsets)), ci64, (N, M), nnz)
    yt = torch.full((N,), float("nan"), dtype=x.dtype, device="cuda")
    info = sp.multiply_inspect(a_csc, xt, yt)
    sp.multiply(info, a_csc, xt, yt)
    ci64.copy_(G.dev(new))
    with pytest.raises(ValueError, match="modified in place after multiply_inspect"):
        sp.multiply(info, a_csc, xt, yt)
    info = sp.multiply_inspect(a_csc, xt, yt)
    yt.fill_(float("nan"))
    sp.multiply(info, a_csc, xt, yt)
    util.assert_parity(G.host(yt), oracle.spmv_csc((N, M), rowptr, ci, values, xt_h),
                       oracle.spmv_csc((N, M), rowptr, ci, np.abs(values), np.abs(xt_h)), dtype,
                       row_len=np.bincount(new, minlength=N), what="csc_view: inspected again after the edit")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("form", ["value_free", "owns_values"])
def test_an_armed_step_wait_runs_before_the_peer_storing_reduce(gpu, form, dt):
    m, n = 30000, 50000
    values, rowptr, colind, shape, nnz = generate.uniform_csr_device(m, n, 20, dtype=dt, seed=3, device="cuda")
    a = sp.csr_view(values, rowptr, colind, shape, nnz)
    x = torch.rand(n, dtype=dt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    y = torch.full((m,), float("nan"), dtype=dt, device="cuda")
    if form == "value_free":
        os.environ["SPBLAS_GFX950_PB_VFREE"] = "2"
        os.environ["SPBLAS_GFX950_PB_VF_ROWS"] = "500"
        try:
            info = sp.multiply_inspect(a, x, y, alg=_capi.SPMV_SLICED)
        finally:
            del os.environ["SPBLAS_GFX950_PB_VFREE"], os.environ["SPBLAS_GFX950_PB_VF_ROWS"]
        op = a
    else:
        op = sp.matrix_opt(a)
        info = sp.multiply_inspect(op, x, y, alg=_capi.SPMV_SLICED)
    si = info.state_.sliced_info()
    assert info.state_.info()["alg"] == _capi.SPMV_SLICED and si["value_free"] == (1 if form == "value_free" else 0), si
    sp.multiply(info, op, x, y)                        # expand + reduce: the products of x are in place for the reduce below
    torch.cuda.synchronize()
    lib, hd = _capi.lib(), sp.api._Handle.current(y.device)
    y_peer = torch.full((m,), float("nan"), dtype=dt, device="cuda")
    peers = torch.tensor([y_peer.data_ptr()], dtype=torch.int64, device="cuda")   # the rank's own buffer is the only "peer"
    flag = torch.zeros(1, dtype=torch.int64, device="cuda")                        # never advanced
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    alpha = (ctypes.c_float if dt == torch.float32 else ctypes.c_double)(1.0)
    torch.cuda.synchronize()
    sp.api.check(lib.spblas_gfx950_bcast_wait_before(hd.h, ctypes.c_void_p(flag.data_ptr()), 1, 1, 50,
                                                     ctypes.c_void_p(status.data_ptr())), "bcast_wait_before")
    sp.api.check(lib.spblas_gfx950_spmv_reduce_rows_bcast(hd.h, info.state_.plan, ctypes.byref(alpha),
                                                          ctypes.c_void_p(peers.data_ptr()), 1, 0, 0, m),
                 "spmv_reduce_rows_bcast")
    torch.cuda.synchronize()
    assert int(status.item()) == 1, (f"{form}: the wait armed by bcast_wait_before was not launched with the reduce that "
                                     f"stores into the peers' y (status word {int(status.item())}, 1 = timed out as it must)")
    assert torch.equal(y_peer, y), "the rows stored into the peer buffer differ from the plan's own multiply"
    # the wait belonged to that one call: a second reduce runs without it
    status.zero_()
    y_peer.fill_(float("nan"))
    sp.api.check(lib.spblas_gfx950_spmv_reduce_rows_bcast(hd.h, info.state_.plan, ctypes.byref(alpha),
                                                          ctypes.c_void_p(peers.data_ptr()), 1, 0, 0, m),
                 "spmv_reduce_rows_bcast")
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and torch.equal(y_peer, y)
    vh, rh, ch, xh = G.host(values), G.host(rowptr), G.host(colind), G.host(x)
    util.assert_parity(G.host(y_peer), oracle.spmv(shape, rh, ch, vh, xh), oracle.spmv_absrow(rh, ch, vh, xh),
                       np.float32 if dt == torch.float32 else np.float64, row_len=np.diff(rh), what=f"{form}: peer rows")
