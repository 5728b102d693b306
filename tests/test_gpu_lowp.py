"""-m gpu tests for 16-bit SpMV / SpMM (torch.float16 = IEEE binary16, torch.bfloat16): plan-free and inspected
(VECTOR / ROWBLOCK / AUTO, matrix_opt), alpha / beta, int64 offsets, dense layouts and leading-dimension windows, empty rows
and zero sizes, NaN / inf inputs, an f16 overflow, integer data that must match bit for bit (a million-entry row
included), the full cfg2 / cfg3 shapes in bf16, and the plan rules.

Expected values come from the same 16-bit inputs upcast to float64 (scipy on the host, or tests/fullcheck.py in torch on the
device), never through the library.  Bound per element: half an ulp of the 16-bit type (the one rounding of the result)
plus (len(row) + 2) * 2^-24 * (|alpha| sum |a x| + |beta y|) for the fp32 sums, the alpha product and the beta add."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import fullcheck as F
from ladder import bits_equal, check_lowp
import spblas_reference_amd as sp
from spblas_reference_amd import _capi, generate
from spblas_reference_amd.api import _Handle

pytestmark = pytest.mark.gpu

LOWP = [torch.float16, torch.bfloat16]
VT = {torch.float16: _capi.F16, torch.bfloat16: _capi.BF16}


def _name(dt):
    return str(dt).replace("torch.", "")


# --------------------------------------------------------------------------------------------------------- helpers
def make_csr(rng, m, n, per_row, dt, dev, empty_every=0, long_rows=None, ints=False, offset64=False):
    """(a, host) with a = csr_view on the device and host = (rowptr, colind, float64 values of the 16-bit entries)."""
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
    raw = rng.integers(-2, 3, nnz).astype(np.float32) if ints else rng.uniform(-1, 1, nnz).astype(np.float32)
    vals = torch.from_numpy(raw).to(dt)
    a = sp.csr_view(vals.to(dev), torch.from_numpy(rowptr if offset64 else rowptr.astype(np.int32)).to(dev),
                    torch.from_numpy(colind).to(dev), (m, n), nnz)
    return a, (rowptr, colind, vals.double().numpy())


def rand16(rng, shape, dt, dev, ints=False):
    raw = rng.integers(-2, 3, shape).astype(np.float32) if ints else rng.uniform(-1, 1, shape).astype(np.float32)
    return torch.from_numpy(raw).to(dt).to(dev)


def host_mat(host, shape, absolute=False):
    rowptr, colind, v = host
    return sps.csr_matrix((np.abs(v) if absolute else v, colind, rowptr), shape=shape)


check = check_lowp   # (the bound lives in tests/ladder.py, shared with the ladder tests)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() > 0 else 0)


def capi_spmv(a, x, y, alpha, beta, plan=None):
    hd = _Handle.current(y.device)
    al, be = ctypes.c_float(alpha), ctypes.c_float(beta)
    m, n = a.shape()
    ot = _capi.I64 if a.rowptr().dtype == torch.int64 else _capi.I32
    return _capi.lib().spblas_gfx950_spmv(hd.h, plan, _capi.OP_N, m, n, a.size(), ctypes.byref(al), ptr(a.rowptr()),
                                          ptr(a.colind()), ptr(a.values()), ptr(x), ctypes.byref(be), ptr(y), ot,
                                          VT[a.values().dtype])


def capi_spmm(a, B, C, alpha, beta, plan=None):
    hd = _Handle.current(C.device)
    al, be = ctypes.c_float(alpha), ctypes.c_float(beta)
    m, k = a.shape()
    ot = _capi.I64 if a.rowptr().dtype == torch.int64 else _capi.I32
    return _capi.lib().spblas_gfx950_spmm_strided(hd.h, plan, m, k, C.shape[1], a.size(), ctypes.byref(al), ptr(a.rowptr()),
                                                  ptr(a.colind()), ptr(a.values()), ptr(B), B.stride(0), B.stride(1),
                                                  ctypes.byref(be), ptr(C), C.stride(0), C.stride(1), ot,
                                                  VT[a.values().dtype])


ALGS = {"VECTOR": _capi.SPMV_VECTOR, "ROWBLOCK": _capi.SPMV_ROWBLOCK, "AUTO": _capi.SPMV_AUTO}


def run_spmv(kind, a, x, y, scale=None):
    """kind: 'free' (no inspect), VECTOR / ROWBLOCK / AUTO plans, or 'opt' (AUTO on a matrix_opt operand)."""
    op = a if scale is None else sp.scaled(scale, a)
    if kind == "free":
        sp.multiply(op, x, y)
        return None
    if kind == "opt":
        mo = sp.matrix_opt(a)
        op = mo if scale is None else sp.scaled(scale, mo)
        info = sp.multiply_inspect(op, x, y)
    else:
        info = sp.multiply_inspect(op, x, y, alg=ALGS[kind])
    sp.multiply(info, op, x, y)
    return info


# ------------------------------------------------------------------------------------------------------ SpMV
@pytest.mark.parametrize("offset64", [False, True], ids=["o32", "o64"])
@pytest.mark.parametrize("kind", ["free", "VECTOR", "ROWBLOCK", "AUTO", "opt"])
@pytest.mark.parametrize("dt", LOWP, ids=_name)
def test_spmv_plans(gpu, dt, kind, offset64):
    rng = np.random.default_rng(1)
    shape = (3000, 2500)
    a, host = make_csr(rng, *shape, 9, dt, gpu, empty_every=7, long_rows={10: 5000, 2000: 2100}, offset64=offset64)
    x = rand16(rng, shape[1], dt, gpu)
    y = torch.full((shape[0],), float("nan"), dtype=dt, device=gpu)
    info = run_spmv(kind, a, x, y, scale=0.5)
    if info is not None:
        pi = info.state_.info()
        assert pi["alg"] != _capi.SPMV_SLICED
        if kind == "ROWBLOCK":
            assert pi["n_long_rows"] == 2
    xh = x.double().cpu().numpy()
    ref = 0.5 * (host_mat(host, shape) @ xh)
    absrow = 0.5 * (host_mat(host, shape, True) @ np.abs(xh))
    check(y, ref, absrow, np.diff(host[0]), dt, f"spmv {kind}")


@pytest.mark.parametrize("kind", ["free", "VECTOR", "ROWBLOCK"])
@pytest.mark.parametrize("dt", LOWP, ids=_name)
def test_spmv_alpha_beta(gpu, dt, kind):
    """y = alpha A x + beta y through the C ABI (float scalars); beta == 0 does not read y (NaN there stays out)."""
    rng = np.random.default_rng(2)
    shape = (2000, 1800)
    a, host = make_csr(rng, *shape, 13, dt, gpu, empty_every=5, long_rows={7: 4500})
    x = rand16(rng, shape[1], dt, gpu)
    y0 = rand16(rng, shape[0], dt, gpu)
    plan = None
    if kind != "free":
        info = sp.multiply_inspect(a, x, y0.clone(), alg=ALGS[kind])
        plan = info.state_.plan
    y = y0.clone()
    assert capi_spmv(a, x, y, 1.5, -0.75, plan) == _capi.SUCCESS
    xh, yh = x.double().cpu().numpy(), y0.double().cpu().numpy()
    ref = 1.5 * (host_mat(host, shape) @ xh) - 0.75 * yh
    absrow = 1.5 * (host_mat(host, shape, True) @ np.abs(xh)) + 0.75 * np.abs(yh)
    check(y, ref, absrow, np.diff(host[0]), dt, f"alpha/beta {kind}")
    y = torch.full_like(y0, float("nan"))
    assert capi_spmv(a, x, y, -2.0, 0.0, plan) == _capi.SUCCESS
    check(y, -2.0 * (host_mat(host, shape) @ xh), 2.0 * (host_mat(host, shape, True) @ np.abs(xh)), np.diff(host[0]), dt,
          f"beta = 0 {kind}")


# ------------------------------------------------------------------------------------------------------ SpMM
def dense(rows, cols, layout, dt, dev, rng):
    """A rows x cols operand: 'right' (row-major), 'right_ld' (row stride cols + 5), 'left' (column-major), 'left_ld'
    (column stride rows + 3); its values."""
    vals = rand16(rng, (rows, cols), dt, dev)
    if layout == "right":
        return vals.clone()
    if layout == "right_ld":
        t = torch.zeros((rows, cols + 5), dtype=dt, device=dev)[:, :cols]
    elif layout == "left":
        t = torch.zeros((cols, rows), dtype=dt, device=dev).t()
    else:
        t = torch.zeros((cols, rows + 3), dtype=dt, device=dev)[:, :rows].t()
    t.copy_(vals)
    return t


@pytest.mark.parametrize("layout", ["right", "right_ld", "left", "left_ld"])
@pytest.mark.parametrize("n", [1, 8, 13, 128])
@pytest.mark.parametrize("dt", LOWP, ids=_name)
def test_spmm(gpu, dt, n, layout):
    rng = np.random.default_rng(3)
    m, k = 1500, 1200
    for offset64 in (False, True):
        a, host = make_csr(rng, m, k, 7, dt, gpu, empty_every=5, long_rows={3: 4500}, offset64=offset64)
        B = dense(k, n, layout, dt, gpu, rng)
        Bh = B.double().cpu().numpy()
        ref = 2.0 * (host_mat(host, (m, k)) @ Bh)
        absrow = 2.0 * (host_mat(host, (m, k), True) @ np.abs(Bh))
        for inspect in (False, True):
            C = dense(m, n, layout, dt, gpu, rng)
            C.fill_(float("nan"))
            if inspect:
                info = sp.multiply_inspect(a, B, C)
                sp.multiply(info, sp.scaled(2.0, a), B, C)
            else:
                sp.multiply(sp.scaled(2.0, a), B, C)
            check(C, ref, absrow, np.diff(host[0]), dt, f"spmm n={n} {layout} inspect={inspect} o64={offset64}")


@pytest.mark.parametrize("dt", LOWP, ids=_name)
def test_spmm_alpha_beta(gpu, dt):
    rng = np.random.default_rng(4)
    m, k, n = 900, 700, 24
    a, host = make_csr(rng, m, k, 10, dt, gpu, empty_every=9, long_rows={5: 3000})
    info = sp.multiply_inspect(a, torch.empty((k, n), dtype=dt, device=gpu), torch.empty((m, n), dtype=dt, device=gpu))
    for layout in ("right", "left_ld"):
        B, C0 = dense(k, n, layout, dt, gpu, rng), dense(m, n, layout, dt, gpu, rng)
        Bh, Ch = B.double().cpu().numpy(), C0.double().cpu().numpy()
        for plan in (None, info.state_.plan):
            C = C0.clone() if layout == "right" else dense(m, n, layout, dt, gpu, rng).copy_(C0)
            assert capi_spmm(a, B, C, 0.5, 2.0, plan) == _capi.SUCCESS
            ref = 0.5 * (host_mat(host, (m, k)) @ Bh) + 2.0 * Ch
            absrow = 0.5 * (host_mat(host, (m, k), True) @ np.abs(Bh)) + 2.0 * np.abs(Ch)
            check(C, ref, absrow, np.diff(host[0]), dt, f"spmm alpha/beta {layout} plan={plan is not None}")


# ------------------------------------------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("dt", LOWP, ids=_name)
def test_empty_rows_and_zero_sizes(gpu, dt):
    rng = np.random.default_rng(5)
    # no entries at all: y = beta * y
    a, _ = make_csr(rng, 40, 30, 0, dt, gpu)
    y0 = rand16(rng, 40, dt, gpu)
    y = y0.clone()
    assert capi_spmv(a, rand16(rng, 30, dt, gpu), y, 1.0, 3.0) == _capi.SUCCESS
    assert torch.equal(y, (3.0 * y0.float()).to(dt))
    y = torch.full((40,), float("nan"), dtype=dt, device=gpu)
    sp.multiply(a, rand16(rng, 30, dt, gpu), y)
    assert bool((y == 0).all())
    C0 = rand16(rng, (40, 6), dt, gpu)
    C = C0.clone()
    assert capi_spmm(a, rand16(rng, (30, 6), dt, gpu), C, 1.0, -1.0) == _capi.SUCCESS
    assert torch.equal(C, (-C0.float()).to(dt))
    # zero-size shapes
    for m, n in ((0, 5), (5, 0), (0, 0)):
        a, _ = make_csr(rng, m, n, 3, dt, gpu)
        y = torch.full((m,), float("nan"), dtype=dt, device=gpu)
        sp.multiply(a, torch.ones(n, dtype=dt, device=gpu), y)
        assert bool((y == 0).all())
        C = torch.full((m, 4), float("nan"), dtype=dt, device=gpu)
        sp.multiply(a, torch.ones((n, 4), dtype=dt, device=gpu), C)
        assert bool((C == 0).all())
        C = torch.empty((m, 0), dtype=dt, device=gpu)
        sp.multiply(a, torch.ones((n, 0), dtype=dt, device=gpu), C)
        if m:
            info = sp.multiply_inspect(a, torch.ones(n, dtype=dt, device=gpu), y)
            sp.multiply(info, a, torch.ones(n, dtype=dt, device=gpu), y)
            assert bool((y == 0).all())
    # mostly empty rows, every plan
    a, host = make_csr(rng, 5000, 400, 4, dt, gpu, empty_every=2)
    x = rand16(rng, 400, dt, gpu)
    xh = x.double().cpu().numpy()
    for kind in ("free", "VECTOR", "ROWBLOCK", "AUTO"):
        y = torch.full((5000,), float("nan"), dtype=dt, device=gpu)
        run_spmv(kind, a, x, y)
        check(y, host_mat(host, (5000, 400)) @ xh, host_mat(host, (5000, 400), True) @ np.abs(xh), np.diff(host[0]), dt,
              f"empty rows {kind}")


@pytest.mark.parametrize("dt", LOWP, ids=_name)
def test_nan_and_inf_inputs(gpu, dt):
    rng = np.random.default_rng(6)
    m, n = 300, 200
    a, host = make_csr(rng, m, n, 6, dt, gpu, long_rows={50: 4200})
    vals = a.values()
    vals[host[0][3]] = float("nan")            # a NaN in row 3
    vals[host[0][9]] = float("inf")            # +inf in row 9
    vals[host[0][50] + 4000] = float("-inf")   # -inf in the long row
    host = (host[0], host[1], vals.double().cpu().numpy())
    x = rand16(rng, n, dt, gpu)
    x[int(host[1][host[0][20]])] = float("inf")  # an inf x that row 20 (among others) reads
    x[int(host[1][host[0][21]])] = 0.0
    xh = x.double().cpu().numpy()
    with np.errstate(invalid="ignore"):
        ref = host_mat(host, (m, n)) @ xh
    for kind in ("free", "ROWBLOCK"):
        y = torch.empty(m, dtype=dt, device=gpu)
        run_spmv(kind, a, x, y)
        yd = y.double().cpu().numpy()
        assert np.array_equal(np.isnan(yd), np.isnan(ref)), kind
        assert np.array_equal(yd[np.isinf(ref)], ref[np.isinf(ref)]), kind
    Bh = np.repeat(xh[:, None], 8, axis=1)
    with np.errstate(invalid="ignore"):
        ref_mm = host_mat(host, (m, n)) @ Bh
    C = torch.empty((m, 8), dtype=dt, device=gpu)
    info = sp.multiply_inspect(a, x[:, None].repeat(1, 8), C)
    sp.multiply(info, a, x[:, None].repeat(1, 8).contiguous(), C)
    Cd = C.double().cpu().numpy()
    assert np.array_equal(np.isnan(Cd), np.isnan(ref_mm))
    assert np.array_equal(Cd[np.isinf(ref_mm)], ref_mm[np.isinf(ref_mm)])


def test_f16_overflow_becomes_inf(gpu):
    dt = torch.float16
    # rows: 60000 + 60000 (-> +inf), -(60000 + 60000) (-> -inf), 32752 + 32752 = 65504 (the largest finite value)
    rowptr = torch.tensor([0, 2, 4, 6], dtype=torch.int32, device=gpu)
    colind = torch.tensor([0, 1, 0, 1, 0, 1], dtype=torch.int32, device=gpu)
    vals = torch.tensor([60000, 60000, -60000, -60000, 32752, 32752], dtype=dt, device=gpu)
    a = sp.csr_view(vals, rowptr, colind, (3, 2), 6)
    x = torch.ones(2, dtype=dt, device=gpu)
    for kind in ("free", "VECTOR", "ROWBLOCK"):
        y = torch.empty(3, dtype=dt, device=gpu)
        run_spmv(kind, a, x, y)
        assert y.tolist() == [float("inf"), float("-inf"), 65504.0], kind
    C = torch.empty((3, 8), dtype=dt, device=gpu)
    sp.multiply(a, torch.ones((2, 8), dtype=dt, device=gpu), C)
    assert (C[0] == float("inf")).all() and (C[1] == float("-inf")).all() and (C[2] == 65504.0).all()


# ------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("dt", LOWP, ids=_name)
def test_exact_integer_data_bit_for_bit(gpu, dt):
    """Integer data whose fp32 sums are exact: every path must round the exact sum once, bit for bit.  Row 2 holds a
    million entries: the row-block plan splits it over its windows, the SpMM plan over its long-row parts."""
    rng = np.random.default_rng(7)
    m, n = 4000, 8192
    a, host = make_csr(rng, m, n, 5, dt, gpu, empty_every=11, long_rows={2: 1_000_000, 3000: 3000}, ints=True)
    x = rand16(rng, n, dt, gpu, ints=True)
    ref = host_mat(host, (m, n)) @ x.double().cpu().numpy()
    assert np.abs(ref).max() < 65504
    for kind in ("free", "VECTOR", "ROWBLOCK", "AUTO", "opt"):
        y = torch.full((m,), float("nan"), dtype=dt, device=gpu)
        info = run_spmv(kind, a, x, y)
        if kind == "ROWBLOCK":
            assert info.state_.info()["n_long_rows"] == 2
        assert bits_equal(y, ref, dt), kind
    B = rand16(rng, (n, 16), dt, gpu, ints=True)
    ref_mm = host_mat(host, (m, n)) @ B.double().cpu().numpy()
    for inspect in (False, True):
        C = torch.full((m, 16), float("nan"), dtype=dt, device=gpu)
        if inspect:
            info = sp.multiply_inspect(a, B, C)
            assert info.state_.info()["n_long_rows"] == 2
            sp.multiply(info, a, B, C)
        else:
            sp.multiply(a, B, C)
        assert bits_equal(C, ref_mm, dt), f"spmm inspect={inspect}"
        Cl = torch.empty((16, m), dtype=dt, device=gpu).t()
        if inspect:
            sp.multiply(info, a, B, Cl)
        else:
            sp.multiply(a, B, Cl)
        assert bits_equal(Cl, ref_mm, dt), f"spmm layout_left inspect={inspect}"


# ------------------------------------------------------------------------------------------------------ full size
def test_full_size_cfg2_bf16_spmv(gpu):
    """cfg2's shape in bf16 (10M x 10M, 10 per row): plan-free, ROWBLOCK and AUTO (plain and matrix_opt: 100 M entries,
    never SLICED), every element against float64."""
    dt = torch.bfloat16
    m = n = 10_000_000
    values, rowptr, colind, shape, nnz = generate.uniform_csr_device(m, n, 10, seed=0)
    values = values.to(dt)
    a = sp.csr_view(values, rowptr, colind, shape, nnz)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.rand(n, device="cuda", generator=g) * 2 - 1).to(dt)
    ref, absrow = F.spmv_ref_f64(rowptr, colind, values, x)
    lens = (rowptr[1:].long() - rowptr[:-1].long()).cpu().numpy()
    for kind in ("free", "ROWBLOCK", "AUTO", "opt"):
        y = torch.full((m,), float("nan"), dtype=dt, device="cuda")
        info = run_spmv(kind, a, x, y)
        if info is not None:
            assert info.state_.info()["alg"] != _capi.SPMV_SLICED
        check(y, ref, absrow, lens, dt, f"cfg2 bf16 {kind}")


def test_full_size_cfg3_bf16_spmm(gpu):
    """cfg3's shape in bf16 (A 2M x 2M, 32 per row, B 2M x 128): plan-free and inspected, every element against float64."""
    dt = torch.bfloat16
    m = k = 2_000_000
    values, rowptr, colind, shape, nnz = generate.uniform_csr_device(m, k, 32, seed=0)
    values = values.to(dt)
    a = sp.csr_view(values, rowptr, colind, shape, nnz)
    g = torch.Generator(device="cuda").manual_seed(2)
    B = torch.rand((k, 128), device="cuda", generator=g).to(dt)
    C_ref, C_abs = F.spmm_ref_f64(rowptr, colind, values, B)
    lens = (rowptr[1:].long() - rowptr[:-1].long()).cpu().numpy()
    for inspect in (False, True):
        C = torch.full((m, 128), float("nan"), dtype=dt, device="cuda")
        if inspect:
            info = sp.multiply_inspect(sp.matrix_opt(a), B, C)
            sp.multiply(info, a, B, C)
        else:
            sp.multiply(a, B, C)
        check(C, C_ref, C_abs, lens, dt, f"cfg3 bf16 inspect={inspect}")
    del C_ref, C_abs
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------ plans
@pytest.mark.parametrize("dt", LOWP, ids=_name)
def test_plan_rules(gpu, dt):
    rng = np.random.default_rng(8)
    a, host = make_csr(rng, 3000, 2000, 8, dt, gpu, long_rows={1: 6000})
    x = rand16(rng, 2000, dt, gpu)
    y = torch.empty(3000, dtype=dt, device=gpu)
    hd = _Handle.current(gpu)
    lib = _capi.lib()
    plan = ctypes.c_void_p()
    # SLICED on request: NOT_SUPPORTED
    assert lib.spblas_gfx950_spmv_plan_create(hd.h, ctypes.byref(plan), 3000, 2000, a.size(), ptr(a.rowptr()),
                                              ptr(a.colind()), ptr(a.values()), _capi.I32, VT[dt],
                                              _capi.SPMV_SLICED) == _capi.NOT_SUPPORTED
    # value refresh, detach and the two-stage calls refuse a 16-bit plan
    info = sp.multiply_inspect(sp.matrix_opt(a), x, y)
    p = info.state_.plan
    assert info.state_.info()["alg"] == _capi.SPMV_ROWBLOCK
    assert lib.spblas_gfx950_spmv_plan_update_values(hd.h, p, ptr(a.values())) == _capi.NOT_SUPPORTED
    assert lib.spblas_gfx950_spmv_plan_detach(hd.h, p) == _capi.NOT_SUPPORTED
    assert lib.spblas_gfx950_spmv_expand(hd.h, p, ptr(x)) == _capi.NOT_SUPPORTED
    one = ctypes.c_float(1)
    assert lib.spblas_gfx950_spmv_reduce_rows(hd.h, p, ctypes.byref(one), ctypes.byref(one), ptr(y), 0,
                                              3000) == _capi.NOT_SUPPORTED
    # a 16-bit plan does not serve another value type
    yf = torch.empty(3000, dtype=torch.float32, device=gpu)
    al, be = ctypes.c_float(1), ctypes.c_float(0)
    other = torch.float16 if dt == torch.bfloat16 else torch.bfloat16
    assert lib.spblas_gfx950_spmv(hd.h, p, _capi.OP_N, 3000, 2000, a.size(), ctypes.byref(al), ptr(a.rowptr()),
                                  ptr(a.colind()), ptr(a.values()), ptr(x), ctypes.byref(be), ptr(yf), _capi.I32,
                                  VT[other]) == _capi.PLAN_MISMATCH
    # two multiplies with one plan: the same bits (SpMV with the long-row split, SpMM with the long-row parts)
    sp.multiply(info, a, x, y)
    y2 = torch.empty_like(y)
    sp.multiply(info, a, x, y2)
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))
    B = rand16(rng, (2000, 64), dt, gpu)
    C1, C2 = (torch.empty((3000, 64), dtype=dt, device=gpu) for _ in range(2))
    info_mm = sp.multiply_inspect(a, B, C1)
    sp.multiply(info_mm, a, B, C1)
    sp.multiply(info_mm, a, B, C2)
    assert torch.equal(C1.view(torch.int16), C2.view(torch.int16))


@pytest.mark.parametrize("dt", LOWP, ids=_name)
def test_auto_never_sliced_at_16m_entries(gpu, dt):
    """AUTO on a plain and on a matrix_opt 16-bit operand of 16.8 M entries (the size from which real values may get the
    sliced plan): a row-block plan, and its multiply is right."""
    m = n = 1 << 22
    values, rowptr, colind, shape, nnz = generate.uniform_csr_device(m, n, 4, seed=3)
    assert nnz >= 16 << 20
    a = sp.csr_view(values.to(dt), rowptr, colind, shape, nnz)
    x = torch.rand(n, device="cuda").to(dt)
    ref, absrow = F.spmv_ref_f64(rowptr, colind, a.values(), x)
    for op in (a, sp.matrix_opt(a)):
        y = torch.full((m,), float("nan"), dtype=dt, device="cuda")
        info = sp.multiply_inspect(op, x, y)
        assert info.state_.info()["alg"] == _capi.SPMV_ROWBLOCK
        sp.multiply(info, op, x, y)
        check(y, ref, absrow, np.full(m, 4), dt, "AUTO at 16.8 M entries")


@pytest.mark.parametrize("dt", LOWP, ids=_name)
def test_graph_capture_and_replay(gpu, dt):
    rng = np.random.default_rng(9)
    a, host = make_csr(rng, 4000, 3000, 11, dt, gpu, long_rows={100: 5000})
    x = rand16(rng, 3000, dt, gpu)
    y = torch.empty(4000, dtype=dt, device=gpu)
    B = rand16(rng, (3000, 32), dt, gpu)
    C = torch.empty((4000, 32), dtype=dt, device=gpu)
    info = sp.multiply_inspect(a, x, y, alg=_capi.SPMV_ROWBLOCK)
    info_mm = sp.multiply_inspect(a, B, C)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture (the SpMM long-row workspace is sized here)
        sp.multiply(info, sp.scaled(0.25, a), x, y)
        sp.multiply(info_mm, a, B, C)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    y_eager, C_eager = y.clone(), C.clone()
    y.zero_()
    C.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.multiply(info, sp.scaled(0.25, a), x, y)
        sp.multiply(info_mm, a, B, C)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), y_eager.view(torch.int16))
    assert torch.equal(C.view(torch.int16), C_eager.view(torch.int16))
    xh = x.double().cpu().numpy()
    check(y, 0.25 * (host_mat(host, (4000, 3000)) @ xh), 0.25 * (host_mat(host, (4000, 3000), True) @ np.abs(xh)),
          np.diff(host[0]), dt, "graph")
