"""-m gpu tests for complex SpMV / SpMM (complex64 = std::complex<float>, complex128 = std::complex<double>) with conjugated
operands: the cases of the reference's test/gtest/conjugate_test.cpp (SpMV / SpMM with the matrix or the vector / dense
operand conjugated, util::dims, n in {1, 8, 32}) and the plan / layout / offset / shape combinations of the backend.
Expected values are computed in complex128 on the host from the CSR arrays (scipy.sparse), never through the library."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import spblas_reference_amd as sp
import util
from ladder import check_complex
from spblas_reference_amd import _capi
from spblas_reference_amd.api import _Handle

pytestmark = pytest.mark.gpu

CDT = {np.complex64: torch.complex64, np.complex128: torch.complex128}
CONJ = [(False, False), (True, False), (False, True), (True, True)]


# --------------------------------------------------------------------------------------------------------- helpers
def rand_complex(rng, size, dtype):
    return (rng.uniform(-1, 1, size) + 1j * rng.uniform(-1, 1, size)).astype(dtype)


def make_csr(rng, m, n, per_row, dtype, empty_every=0, long_rows=None, shuffle=False, dups=False):
    """CSR arrays with `per_row` entries per row (random columns), every `empty_every`-th row empty, long_rows = {row:
    length}; shuffle: entries of a row in random order; dups: repeated columns inside rows."""
    lens = np.full(m, per_row, dtype=np.int64)
    if empty_every:
        lens[::empty_every] = 0
    for r, length in (long_rows or {}).items():
        if r < m:
            lens[r] = length
    if n == 0:
        lens[:] = 0
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    nnz = int(rowptr[-1])
    colind = rng.integers(0, max(n, 1), nnz).astype(np.int32)
    if not shuffle:
        for r in range(m):
            if lens[r] > 1 and lens[r] < 5000:
                colind[rowptr[r]:rowptr[r + 1]].sort()
    if dups and nnz > 4:
        colind[1::7] = colind[0:-1:7][:len(colind[1::7])]
    values = rand_complex(rng, nnz, dtype)
    return values, rowptr, colind, (m, n), nnz


def host_csr(values, rowptr, colind, shape, conj_a=False):
    v = values.astype(np.complex128)
    return sps.csr_matrix((np.conj(v) if conj_a else v, colind, rowptr), shape=shape)


def abs_csr(values, rowptr, colind, shape):
    return sps.csr_matrix((np.abs(values.astype(np.complex128)), colind, rowptr), shape=shape)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def view(values, rowptr, colind, shape, nnz, dev, offset64=False):
    rp = rowptr.astype(np.int64 if offset64 else np.int32)
    return sp.csr_view(to_dev(values, dev), to_dev(rp, dev), to_dev(colind, dev), shape, nnz)


check = check_complex   # (the bound lives in tests/ladder.py, shared with the ladder tests)


def row_lengths(rowptr):
    return np.diff(rowptr.astype(np.int64))


def wrap(a, conj_a, mode):
    """A as the multiply sees it: matrix_opt when mode == 'opt', conjugated when asked"""
    if mode == "opt":
        a = sp.matrix_opt(a)
    return sp.conjugated(a) if conj_a else a


MODES = {"plan_free": None, "vector": _capi.SPMV_VECTOR, "rowblock": _capi.SPMV_ROWBLOCK, "auto": _capi.SPMV_AUTO,
         "opt": "opt"}


def spmv_run(a, x, y, mode, conj_a=False, conj_x=False, alpha=None):
    aa = wrap(a, conj_a, mode)
    xx = sp.conjugated(x) if conj_x else x
    if alpha is not None:
        aa = sp.scaled(alpha, aa)
    if mode == "plan_free":
        sp.multiply(aa, xx, y)
        return None
    if mode == "opt":
        sp.multiply_inspect(aa, xx, y)
        sp.multiply(aa, xx, y)
        return None
    info = sp.multiply_inspect(aa, xx, y, alg=MODES[mode])
    sp.multiply(info, aa, xx, y)
    return info


# --------------------------------------------------------------------------------------------- conjugate_test.cpp
def expect_complex_eq(expected, actual):
    """conjugate_test.cpp:17-36 (CPU backends): per component max(1e-2, 256 eps (|t| + |u|))."""
    eps = float(np.finfo(np.float32).eps)
    for t, u in ((expected.real, actual.real), (expected.imag, actual.imag)):
        diff = np.abs(t - u)
        tol = np.maximum(1e-2, 256.0 * eps * (np.abs(t) + np.abs(u)))
        assert (diff <= tol).all(), f"{(diff > tol).sum()} components off, worst {np.max(diff - tol):.3g}"


@pytest.mark.parametrize("dim", util.dims)
@pytest.mark.parametrize("which", ["matrix", "vector"])
def test_conjugate_spmv_reference_cases(gpu, dim, which):
    m, n, nnz = dim
    rng = np.random.default_rng(m * 7 + n)
    rows = np.sort(rng.integers(0, m, nnz))
    rowptr = np.searchsorted(rows, np.arange(m + 1)).astype(np.int32)
    colind = rng.integers(0, n, nnz).astype(np.int32)
    values = (rng.random(nnz) + 1j * rng.random(nnz)).astype(np.complex64)
    b = np.full(n, 1.0 - 2.0j, dtype=np.complex64)
    a = view(values, rowptr, colind, (m, n), nnz, gpu)
    x = to_dev(b, gpu)
    y = torch.zeros(m, dtype=torch.complex64, device=gpu)
    if which == "matrix":
        sp.multiply(sp.conjugated(a), x, y)
    else:
        sp.multiply(a, sp.conjugated(x), y)
    ref = host_csr(values, rowptr, colind, (m, n), which == "matrix") @ (np.conj(b) if which == "vector" else b).astype(np.complex128)
    got = y.cpu().numpy()
    expect_complex_eq(ref, got)
    check(got, ref, abs_csr(values, rowptr, colind, (m, n)) @ np.abs(b), np.complex64, row_lengths(rowptr), which)


@pytest.mark.parametrize("dim", util.dims)
@pytest.mark.parametrize("n", [1, 8, 32])
@pytest.mark.parametrize("which", ["matrix", "dense"])
def test_conjugate_spmm_reference_cases(gpu, dim, n, which):
    m, k, nnz = dim
    rng = np.random.default_rng(m + 3 * k + n)
    rows = np.sort(rng.integers(0, m, nnz))
    rowptr = np.searchsorted(rows, np.arange(m + 1)).astype(np.int32)
    colind = rng.integers(0, k, nnz).astype(np.int32)
    values = (rng.random(nnz) + 1j * rng.random(nnz)).astype(np.complex64)
    B = (rng.random((k, n)) + 1j * rng.random((k, n))).astype(np.complex64)
    a = view(values, rowptr, colind, (m, k), nnz, gpu)
    Bd = to_dev(B, gpu)
    C = torch.zeros((m, n), dtype=torch.complex64, device=gpu)
    if which == "matrix":
        sp.multiply(sp.conjugated(a), Bd, C)
    else:
        sp.multiply(a, sp.conjugated(Bd), C)
    ref = host_csr(values, rowptr, colind, (m, k), which == "matrix") @ (np.conj(B) if which == "dense" else B).astype(np.complex128)
    got = C.cpu().numpy()
    expect_complex_eq(ref, got)
    check(got, ref, abs_csr(values, rowptr, colind, (m, k)) @ np.abs(B), np.complex64, row_lengths(rowptr), which)


# ------------------------------------------------------------------------------------------------------ SpMV product
@pytest.fixture(scope="module")
def nasty():
    """Unsorted rows with duplicate columns, every 5th row empty, two rows far longer than any window (3000 / 9000 entries)."""
    out = {}
    for dt in (np.complex64, np.complex128):
        rng = np.random.default_rng(11)
        out[dt] = make_csr(rng, 3000, 2500, 9, dt, empty_every=5, long_rows={7: 3000, 1234: 9000}, shuffle=True, dups=True)
    return out


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("conj", CONJ)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("offset64", [False, True])
def test_spmv_conj_plans_offsets(gpu, nasty, dtype, conj, mode, offset64):
    values, rowptr, colind, shape, nnz = nasty[dtype]
    ca, cx = conj
    a = view(values, rowptr, colind, shape, nnz, gpu, offset64)
    xh = rand_complex(np.random.default_rng(2), shape[1], dtype)
    x = to_dev(xh, gpu)
    y = torch.full((shape[0],), complex("nan"), dtype=CDT[dtype], device=gpu)
    info = spmv_run(a, x, y, mode, ca, cx)
    if info is not None:
        want = {"vector": _capi.SPMV_VECTOR, "rowblock": _capi.SPMV_ROWBLOCK}.get(mode)
        got_alg = info.state_.info()["alg"]
        assert got_alg != _capi.SPMV_SLICED and (want is None or got_alg == want)
        if mode == "rowblock":
            assert info.state_.info()["n_long_rows"] == 2
    ref = host_csr(values, rowptr, colind, shape, ca) @ (np.conj(xh) if cx else xh).astype(np.complex128)
    absrow = abs_csr(values, rowptr, colind, shape) @ np.abs(xh)
    check(y.cpu().numpy(), ref, absrow, dtype, row_lengths(rowptr), f"{mode} conj={conj}")


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("mode", ["plan_free", "rowblock"])
def test_spmv_row_of_a_million_entries(gpu, dtype, mode):
    rng = np.random.default_rng(3)
    values, rowptr, colind, shape, nnz = make_csr(rng, 5000, 40000, 4, dtype, long_rows={2500: 1 << 20})
    a = view(values, rowptr, colind, shape, nnz, gpu)
    xh = rand_complex(rng, shape[1], dtype)
    y = torch.full((shape[0],), complex("nan"), dtype=CDT[dtype], device=gpu)
    spmv_run(a, to_dev(xh, gpu), y, mode, conj_a=True)
    ref = host_csr(values, rowptr, colind, shape, True) @ xh.astype(np.complex128)
    check(y.cpu().numpy(), ref, abs_csr(values, rowptr, colind, shape) @ np.abs(xh), dtype, row_lengths(rowptr))


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("mode", ["plan_free", "rowblock"])
@pytest.mark.parametrize("conj", CONJ)
def test_spmv_row_of_a_million_entries_exact(gpu, dtype, mode, conj):
    """Small-integer components: every partial sum of the 2^20-entry row is an integer below 2^24, so every summation order
    gives the exact result in c32 too -- a row that is missing, half summed or conjugated wrongly cannot pass."""
    rng = np.random.default_rng(16)
    m, n, long_len = 3000, 50000, 1 << 20
    lens = np.full(m, 3, dtype=np.int64)
    lens[1500] = long_len
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    nnz = int(rowptr[-1])
    colind = rng.integers(0, n, nnz).astype(np.int32)
    values = (rng.integers(-2, 3, nnz) + 1j * rng.integers(-2, 3, nnz)).astype(dtype)
    xh = (rng.integers(-2, 3, n) + 1j * rng.integers(-2, 3, n)).astype(dtype)
    ca, cx = conj
    a = view(values, rowptr, colind, (m, n), nnz, gpu)
    y = torch.full((m,), complex("nan"), dtype=CDT[dtype], device=gpu)
    spmv_run(a, to_dev(xh, gpu), y, mode, ca, cx)
    ref = host_csr(values, rowptr, colind, (m, n), ca) @ (np.conj(xh) if cx else xh).astype(np.complex128)
    got = y.cpu().numpy().astype(np.complex128)
    assert np.abs(ref[1500]) > 100  # (not a trivially small row sum)
    assert np.array_equal(got, ref), f"{np.sum(got != ref)} rows differ; long row {got[1500]} vs {ref[1500]}"


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_prepared_multiply_complex(gpu, dtype):
    """prepared_multiply binds the conjugating entry point for complex operands; contents may change between calls."""
    rng = np.random.default_rng(17)
    values, rowptr, colind, shape, nnz = make_csr(rng, 2000, 1800, 9, dtype, long_rows={5: 3000})
    a = view(values, rowptr, colind, shape, nnz, gpu)
    x = torch.zeros(shape[1], dtype=CDT[dtype], device=gpu)
    y = torch.empty(shape[0], dtype=CDT[dtype], device=gpu)
    aa = sp.scaled(1.0 - 1.0j, sp.conjugated(a))
    info = sp.multiply_inspect(aa, x, y, alg=_capi.SPMV_ROWBLOCK)
    call = sp.prepared_multiply(info, aa, sp.conjugated(x), y)
    A = host_csr(values, rowptr, colind, shape, True)
    for seed in (1, 2):
        xh = rand_complex(np.random.default_rng(seed), shape[1], dtype)
        x.copy_(to_dev(xh, gpu))
        call()
        check(y.cpu().numpy(), (1.0 - 1.0j) * (A @ np.conj(xh).astype(np.complex128)),
              abs(1.0 - 1.0j) * (abs_csr(values, rowptr, colind, shape) @ np.abs(xh)), dtype, row_lengths(rowptr), "prepared")


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("m,n", [(0, 5), (5, 0), (1, 1), (1, 300), (300, 1), (0, 0)])
@pytest.mark.parametrize("mode", ["plan_free", "rowblock"])
def test_spmv_degenerate_shapes(gpu, dtype, m, n, mode):
    rng = np.random.default_rng(m + n)
    values, rowptr, colind, shape, nnz = make_csr(rng, m, n, 3 if n else 0, dtype)
    a = view(values, rowptr, colind, shape, nnz, gpu)
    xh = rand_complex(rng, n, dtype)
    y = torch.full((m,), complex("nan"), dtype=CDT[dtype], device=gpu)
    spmv_run(a, to_dev(xh, gpu), y, mode, conj_x=True)
    ref = host_csr(values, rowptr, colind, shape) @ np.conj(xh).astype(np.complex128) if m and n else np.zeros(m)
    check(y.cpu().numpy(), ref, abs_csr(values, rowptr, colind, shape) @ np.abs(xh) if m and n else np.zeros(m), dtype,
          np.ones(m))


# ------------------------------------------------------------------------------------------------ scaling factors
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("mode", ["plan_free", "rowblock"])
def test_scaled_and_conjugated_order(gpu, dtype, mode):
    """scaled(s, conjugated(A)) = s conj(A); conjugated(scaled(s, A)) = conj(s) conj(A) (views/conjugated_view_impl.hpp)."""
    rng = np.random.default_rng(8)
    values, rowptr, colind, shape, nnz = make_csr(rng, 2000, 1500, 12, dtype)
    a = view(values, rowptr, colind, shape, nnz, gpu)
    xh = rand_complex(rng, shape[1], dtype)
    x = to_dev(xh, gpu)
    s = 0.5 + 2.0j
    absrow = abs(s) * (abs_csr(values, rowptr, colind, shape) @ np.abs(xh))
    conjA = host_csr(values, rowptr, colind, shape, True)
    results = {}
    for name, aa, factor in (("scaled(conj)", sp.scaled(s, sp.conjugated(a)), s),
                             ("conj(scaled)", sp.conjugated(sp.scaled(s, a)), np.conj(s))):
        y = torch.empty(shape[0], dtype=CDT[dtype], device=gpu)
        if mode == "plan_free":
            sp.multiply(aa, x, y)
        else:
            info = sp.multiply_inspect(aa, x, y, alg=_capi.SPMV_ROWBLOCK)
            sp.multiply(info, aa, x, y)
        got = y.cpu().numpy()
        check(got, factor * (conjA @ xh.astype(np.complex128)), absrow, dtype, row_lengths(rowptr), name)
        results[name] = got
    assert np.abs(results["scaled(conj)"] - results["conj(scaled)"]).max() > 0.1
    # the factor on x: conjugated(scaled(s, x)) = conj(s) conj(x), together with a factor on A
    y = torch.empty(shape[0], dtype=CDT[dtype], device=gpu)
    sp.multiply(sp.scaled(2.0 - 1.0j, a), sp.conjugated(sp.scaled(s, x)), y)
    ref = (2.0 - 1.0j) * np.conj(s) * (host_csr(values, rowptr, colind, shape) @ np.conj(xh).astype(np.complex128))
    check(y.cpu().numpy(), ref, abs(2.0 - 1.0j) * absrow, dtype, row_lengths(rowptr), "alpha on x")


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("plan", [False, True])
def test_beta_through_the_c_abi(gpu, dtype, plan):
    """y = alpha conj(A) x + beta y with beta != 0 (spblas_gfx950_spmv_conj), and C = alpha A conj(B) + beta C (spmm)."""
    rng = np.random.default_rng(9)
    values, rowptr, colind, shape, nnz = make_csr(rng, 1500, 1200, 10, dtype, empty_every=4, long_rows={3: 5000})
    a = view(values, rowptr, colind, shape, nnz, gpu)
    xh, yh = rand_complex(rng, shape[1], dtype), rand_complex(rng, shape[0], dtype)
    x, y = to_dev(xh, gpu), to_dev(yh, gpu)
    vt, ct = sp.api._VT[CDT[dtype]]
    alpha, beta = ct(1.5 - 0.5j), ct(-0.25 + 2.0j)
    hd = _Handle.current(gpu)
    lib = _capi.lib()
    info = sp.multiply_inspect(a, x, y, alg=_capi.SPMV_ROWBLOCK) if plan else None
    pl = info.state_.plan if plan else None
    rc = lib.spblas_gfx950_spmv_conj(hd.h, pl, _capi.OP_N, shape[0], shape[1], nnz, ctypes.byref(alpha),
                                     sp.api._ptr(a.rowptr()), sp.api._ptr(a.colind()), sp.api._ptr(a.values()),
                                     sp.api._ptr(x), ctypes.byref(beta), sp.api._ptr(y), _capi.I32, vt, _capi.CONJ_A)
    assert rc == _capi.SUCCESS
    al, be = complex(1.5 - 0.5j), complex(-0.25 + 2.0j)
    ref = al * (host_csr(values, rowptr, colind, shape, True) @ xh.astype(np.complex128)) + be * yh
    absrow = abs(al) * (abs_csr(values, rowptr, colind, shape) @ np.abs(xh)) + abs(be) * np.abs(yh)
    check(y.cpu().numpy(), ref, absrow, dtype, row_lengths(rowptr), "spmv beta")
    n = 5
    Bh, Ch = rand_complex(rng, (shape[1], n), dtype), rand_complex(rng, (shape[0], n), dtype)
    B, C = to_dev(Bh, gpu), to_dev(Ch, gpu)
    if plan:
        info = sp.multiply_inspect(a, B, C)
        pl = info.state_.plan
    rc = lib.spblas_gfx950_spmm_strided_conj(hd.h, pl, shape[0], shape[1], n, nnz, ctypes.byref(alpha),
                                             sp.api._ptr(a.rowptr()), sp.api._ptr(a.colind()), sp.api._ptr(a.values()),
                                             sp.api._ptr(B), n, 1, ctypes.byref(beta), sp.api._ptr(C), n, 1, _capi.I32, vt,
                                             _capi.CONJ_X)
    assert rc == _capi.SUCCESS
    ref = al * (host_csr(values, rowptr, colind, shape) @ np.conj(Bh).astype(np.complex128)) + be * Ch
    absm = abs(al) * (abs_csr(values, rowptr, colind, shape) @ np.abs(Bh)) + abs(be) * np.abs(Ch)
    check(C.cpu().numpy(), ref, absm, dtype, row_lengths(rowptr), "spmm beta")


# ------------------------------------------------------------------------------------------------------------ SpMM
@pytest.fixture(scope="module")
def spmm_mat():
    out = {}
    for dt in (np.complex64, np.complex128):
        rng = np.random.default_rng(21)
        out[dt] = make_csr(rng, 1200, 900, 7, dt, empty_every=6, long_rows={10: 2600, 600: 2600}, shuffle=True,
                           dups=True)
    return out


def dense(h, layout, dev):
    """h (k x n) on the device as layout_right, layout_left or a padded layout_right / layout_left window"""
    t = to_dev(h, dev)
    if layout == "right":
        return t
    if layout == "left":
        return t.t().contiguous().t()
    if layout == "right_pad":
        big = torch.zeros((h.shape[0], h.shape[1] + 3), dtype=t.dtype, device=dev)
        big[:, :h.shape[1]] = t
        return big[:, :h.shape[1]]
    big = torch.zeros((h.shape[1], h.shape[0] + 5), dtype=t.dtype, device=dev)  # left_pad
    big[:, :h.shape[0]] = t.t()
    return big[:, :h.shape[0]].t()


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("n", [1, 2, 3, 8, 32, 37, 128])
@pytest.mark.parametrize("layout", ["right", "left", "right_pad", "left_pad"])
@pytest.mark.parametrize("conj", CONJ)
@pytest.mark.parametrize("inspected", [False, True])
def test_spmm_layouts_conj(gpu, spmm_mat, dtype, n, layout, conj, inspected):
    values, rowptr, colind, shape, nnz = spmm_mat[dtype]
    ca, cb = conj
    rng = np.random.default_rng(n)
    Bh = rand_complex(rng, (shape[1], n), dtype)
    a = view(values, rowptr, colind, shape, nnz, gpu)
    B = dense(Bh, layout, gpu)
    C = dense(np.full((shape[0], n), np.nan, dtype=dtype), layout, gpu)
    aa = sp.conjugated(a) if ca else a
    bb = sp.conjugated(B) if cb else B
    if inspected:
        info = sp.multiply_inspect(aa, bb, C)
        assert info.state_.spmm_info()["long_rows"] == 2
        sp.multiply(info, aa, bb, C)
    else:
        sp.multiply(aa, bb, C)
    ref = host_csr(values, rowptr, colind, shape, ca) @ (np.conj(Bh) if cb else Bh).astype(np.complex128)
    absm = abs_csr(values, rowptr, colind, shape) @ np.abs(Bh)
    check(C.cpu().numpy(), ref, absm, dtype, row_lengths(rowptr), f"n={n} {layout} conj={conj}")


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("offset64", [False, True])
def test_spmm_matrix_opt_scaled_offsets(gpu, dtype, offset64):
    rng = np.random.default_rng(4)
    values, rowptr, colind, shape, nnz = make_csr(rng, 800, 700, 9, dtype, long_rows={1: 3000})
    a = sp.matrix_opt(view(values, rowptr, colind, shape, nnz, gpu, offset64))
    Bh = rand_complex(rng, (shape[1], 16), dtype)
    B = to_dev(Bh, gpu)
    C = torch.empty((shape[0], 16), dtype=CDT[dtype], device=gpu)
    s = -1.0 + 0.5j
    aa = sp.scaled(s, sp.conjugated(a))
    sp.multiply_inspect(aa, B, C)
    sp.multiply(aa, sp.scaled(2.0j, B), C)
    ref = s * 2.0j * (host_csr(values, rowptr, colind, shape, True) @ Bh.astype(np.complex128))
    check(C.cpu().numpy(), ref, 2 * abs(s) * (abs_csr(values, rowptr, colind, shape) @ np.abs(Bh)), dtype,
          row_lengths(rowptr))


# ------------------------------------------------------------------------------------------------------ torch bits
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_torch_conj_bit(gpu, dtype):
    rng = np.random.default_rng(12)
    values, rowptr, colind, shape, nnz = make_csr(rng, 1000, 800, 8, dtype)
    a = view(values, rowptr, colind, shape, nnz, gpu)
    xh = rand_complex(rng, shape[1], dtype)
    x = to_dev(xh, gpu)
    xc = x.conj()
    assert xc.is_conj()
    y = torch.empty(shape[0], dtype=CDT[dtype], device=gpu)
    sp.multiply(a, xc, y)
    A = host_csr(values, rowptr, colind, shape)
    absrow = abs_csr(values, rowptr, colind, shape) @ np.abs(xh)
    check(y.cpu().numpy(), A @ np.conj(xh).astype(np.complex128), absrow, dtype, row_lengths(rowptr), "x.conj()")
    # conjugated view of a lazily conjugated tensor: the two cancel
    sp.multiply(a, sp.conjugated(xc), y)
    check(y.cpu().numpy(), A @ xh.astype(np.complex128), absrow, dtype, row_lengths(rowptr), "conjugated(x.conj())")
    # A's values with the conj bit
    ac = sp.csr_view(a.values().conj(), a.rowptr(), a.colind(), shape, nnz)
    sp.multiply(ac, x, y)
    check(y.cpu().numpy(), host_csr(values, rowptr, colind, shape, True) @ xh.astype(np.complex128), absrow, dtype,
          row_lengths(rowptr), "values.conj()")
    # a negative view of x is resolved
    sp.multiply(a, torch._neg_view(x), y)
    check(y.cpu().numpy(), -(A @ xh.astype(np.complex128)), absrow, dtype, row_lengths(rowptr), "neg view")
    # ... and an output with the conj bit is refused
    with pytest.raises(ValueError):
        sp.multiply(a, x, torch.empty(shape[0], dtype=CDT[dtype], device=gpu).conj())
    # SpMM: B.conj()
    Bh = rand_complex(rng, (shape[1], 4), dtype)
    C = torch.empty((shape[0], 4), dtype=CDT[dtype], device=gpu)
    sp.multiply(a, to_dev(Bh, gpu).conj(), C)
    check(C.cpu().numpy(), A @ np.conj(Bh).astype(np.complex128), abs_csr(values, rowptr, colind, shape) @ np.abs(Bh),
          dtype, row_lengths(rowptr), "B.conj()")


def test_real_conjugated_still_rejected(gpu):
    a = sp.csr_view(torch.ones(2, device=gpu), torch.tensor([0, 1, 2], dtype=torch.int32, device=gpu),
                    torch.tensor([0, 1], dtype=torch.int32, device=gpu), (2, 2), 2)
    with pytest.raises(RuntimeError):
        sp.multiply(sp.conjugated(a), torch.ones(2, device=gpu), torch.empty(2, device=gpu))


# ------------------------------------------------------------------------------------------------------ graphs
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_graph_capture_and_replay(gpu, dtype):
    rng = np.random.default_rng(13)
    values, rowptr, colind, shape, nnz = make_csr(rng, 4000, 3000, 11, dtype, long_rows={100: 4000})
    a = view(values, rowptr, colind, shape, nnz, gpu)
    x = torch.zeros(shape[1], dtype=CDT[dtype], device=gpu)
    y = torch.empty(shape[0], dtype=CDT[dtype], device=gpu)
    aa = sp.conjugated(a)
    info = sp.multiply_inspect(aa, x, y, alg=_capi.SPMV_ROWBLOCK)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sp.multiply(info, aa, x, y)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.multiply(info, aa, x, y)
    xh = rand_complex(rng, shape[1], dtype)
    x.copy_(to_dev(xh, gpu))
    g.replay()
    torch.cuda.synchronize()
    ref = host_csr(values, rowptr, colind, shape, True) @ xh.astype(np.complex128)
    check(y.cpu().numpy(), ref, abs_csr(values, rowptr, colind, shape) @ np.abs(xh), dtype, row_lengths(rowptr), "graph")


# ------------------------------------------------------------------------------------------------------ plan checks
def test_plan_rules_and_rejections(gpu):
    rng = np.random.default_rng(14)
    values, rowptr, colind, shape, nnz = make_csr(rng, 500, 400, 6, np.complex64)
    a = view(values, rowptr, colind, shape, nnz, gpu)
    x = to_dev(rand_complex(rng, shape[1], np.complex64), gpu)
    y = torch.empty(shape[0], dtype=torch.complex64, device=gpu)
    with pytest.raises(sp.BackendError) as e:
        sp.multiply_inspect(a, x, y, alg=_capi.SPMV_SLICED)
    assert e.value.status == _capi.NOT_SUPPORTED
    hd = _Handle.current(gpu)
    lib = _capi.lib()
    al, be = sp.api.c_complex64(1), sp.api.c_complex64(0)
    P = sp.api._ptr
    args = (shape[0], shape[1], nnz, ctypes.byref(al), P(a.rowptr()), P(a.colind()), P(a.values()), P(x), ctypes.byref(be),
            P(y), _capi.I32, _capi.C32)
    assert lib.spblas_gfx950_spmv(hd.h, None, _capi.OP_T, *args) == _capi.NOT_SUPPORTED
    assert lib.spblas_gfx950_spmv_conj(hd.h, None, _capi.OP_N, *args, 4) == _capi.INVALID_VALUE
    # non-zero flags with a real type
    ar, br = ctypes.c_float(1), ctypes.c_float(0)
    xr, yr = torch.ones(shape[1], device=gpu), torch.empty(shape[0], device=gpu)
    vr = torch.ones(nnz, device=gpu)
    assert lib.spblas_gfx950_spmv_conj(hd.h, None, _capi.OP_N, shape[0], shape[1], nnz, ctypes.byref(ar), P(a.rowptr()),
                                       P(a.colind()), P(vr), P(xr), ctypes.byref(br), P(yr), _capi.I32, _capi.F32,
                                       _capi.CONJ_A) == _capi.INVALID_VALUE
    # a complex plan: no value refresh, no two-stage calls
    info = sp.multiply_inspect(a, x, y, alg=_capi.SPMV_ROWBLOCK)
    assert lib.spblas_gfx950_spmv_plan_update_values(hd.h, info.state_.plan, P(a.values())) == _capi.NOT_SUPPORTED
    assert lib.spblas_gfx950_spmv_plan_detach(hd.h, info.state_.plan) == _capi.NOT_SUPPORTED
    assert lib.spblas_gfx950_spmv_expand(hd.h, info.state_.plan, P(x)) == _capi.NOT_SUPPORTED
    # out of scope in Python: TypeError
    c = sp.csr_view(None, torch.zeros(shape[0] + 1, dtype=torch.int32, device=gpu), None, (shape[0], shape[0]), 0)
    at = sp.csr_view(a.values(), a.rowptr(), a.colind(), shape, nnz)
    with pytest.raises(TypeError):
        sp.multiply_compute(a, sp.transposed(at), c)
    with pytest.raises(TypeError):
        sp.add(a, a, sp.csr_view(None, torch.zeros(shape[0] + 1, dtype=torch.int32, device=gpu), None, shape, 0))
    with pytest.raises(TypeError):
        sp.multiply(sp.transposed(a), y, x)
    with pytest.raises(TypeError):
        sp.multiply(sp.csr_view(a.values(), a.rowptr(), a.colind().long(), shape, nnz), x, y)


def test_auto_never_sliced_for_complex(gpu):
    """AUTO on a complex matrix of >= 16 M entries: the size at which real matrices may get the SLICED plan."""
    m = n = 1 << 21
    per = 8
    rowptr = torch.arange(0, m * per + 1, per, dtype=torch.int32, device=gpu)
    colind = torch.randint(0, n, (m * per,), dtype=torch.int32, device=gpu)
    values = torch.ones(m * per, dtype=torch.complex64, device=gpu)
    a = sp.csr_view(values, rowptr, colind, (m, n), m * per)
    x = torch.ones(n, dtype=torch.complex64, device=gpu)
    y = torch.empty(m, dtype=torch.complex64, device=gpu)
    info = sp.multiply_inspect(sp.matrix_opt(a), x, y)
    assert info.state_.info()["alg"] != _capi.SPMV_SLICED
    info = sp.multiply_inspect(a, x, y)
    assert info.state_.info()["alg"] != _capi.SPMV_SLICED
    sp.multiply(info, a, x, y)
    assert torch.equal(y, torch.full_like(y, per))


def test_large_c64_spmv_every_element(gpu):
    """2 M x 2 M, 10 entries per row, complex128, conj(A): every element against complex128 on the host."""
    m = n = 2_000_000
    per = 10
    g = torch.Generator(device=gpu).manual_seed(15)
    rowptr = torch.arange(0, m * per + 1, per, dtype=torch.int32, device=gpu)
    colind = torch.randint(0, n, (m * per,), dtype=torch.int32, device=gpu, generator=g)
    values = torch.complex(torch.rand(m * per, dtype=torch.float64, device=gpu, generator=g) - 0.5,
                           torch.rand(m * per, dtype=torch.float64, device=gpu, generator=g) - 0.5)
    x = torch.complex(torch.rand(n, dtype=torch.float64, device=gpu, generator=g),
                      torch.rand(n, dtype=torch.float64, device=gpu, generator=g) - 0.5)
    y = torch.full((m,), complex("nan"), dtype=torch.complex128, device=gpu)
    a = sp.csr_view(values, rowptr, colind, (m, n), m * per)
    info = sp.multiply_inspect(sp.conjugated(a), x, y)
    sp.multiply(info, sp.conjugated(a), x, y)
    rp, ci, v, xh = rowptr.cpu().numpy(), colind.cpu().numpy(), values.cpu().numpy(), x.cpu().numpy()
    ref = host_csr(v, rp, ci, (m, n), True) @ xh
    check(y.cpu().numpy(), ref, abs_csr(v, rp, ci, (m, n)) @ np.abs(xh), np.complex128, np.full(m, per), "2M c64")
