"""CPU tests of 16-bit SpMV / SpMM support (float16 / bfloat16, no GPU): the C ABI declares the two value types, the entry
points without a 16-bit form refuse them before any other check, and the Python layer maps the dtypes and raises TypeError,
naming the dtype, for every out-of-scope call."""
import ctypes
import os
import re

import pytest
import torch

import spblas_reference_amd as sp
from spblas_reference_amd import _capi
from spblas_reference_amd.api import _VT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOWP = [torch.float16, torch.bfloat16]


def _names(dt):
    return str(dt).replace("torch.", "")


def test_header_declares_16bit_types():
    text = open(os.path.join(ROOT, "include", "spblas_gfx950.h")).read()
    assert re.search(r"SPBLAS_GFX950_F16\s*=\s*4", text) and re.search(r"SPBLAS_GFX950_BF16\s*=\s*5", text)
    assert (_capi.F16, _capi.BF16) == (4, 5)


def test_dtype_mapping_uses_float_scalars():
    assert _VT[torch.float16] == (_capi.F16, ctypes.c_float)
    assert _VT[torch.bfloat16] == (_capi.BF16, ctypes.c_float)
    # (the existing types are unchanged)
    assert _VT[torch.float32] == (_capi.F32, ctypes.c_float) and _VT[torch.float64] == (_capi.F64, ctypes.c_double)


def test_real_only_entry_points_return_not_supported_for_16bit():
    """Every entry point that takes a value type and has no 16-bit form says NOT_SUPPORTED for F16 / BF16, before any
    other check (here: a null handle and null pointers)."""
    lib = _capi.lib()
    N = None
    one = ctypes.c_float(1)
    for vt in (_capi.F16, _capi.BF16):
        assert lib.spblas_gfx950_spgemm_numeric(N, N, N, N, N, N, N, N, N, N, N, N, 0, vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_spgemm_numeric_addend(N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, 0,
                                                       vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_csr_add_numeric(N, N, N, N, N, N, N, N, N, N, N, N, N, 0, vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_csr_transpose(N, 1, 1, 0, N, N, N, N, N, N, vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_scale(N, 1, N, N, vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_sptrsv_solve(N, N, 1, 0, N, N, N, N, N, N, vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_spmv_conj(N, N, 0, 1, 1, 0, ctypes.byref(one), N, N, N, N, ctypes.byref(one), N, 0, vt,
                                           0) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_spmm_strided_conj(N, N, 1, 1, 1, 0, ctypes.byref(one), N, N, N, N, 1, 1,
                                                   ctypes.byref(one), N, 1, 1, 0, vt, 0) == _capi.NOT_SUPPORTED
        # op = T (csc_view / transposed()): NOT_SUPPORTED; op = N goes on to the handle check
        assert lib.spblas_gfx950_spmv(N, N, _capi.OP_T, 1, 1, 0, ctypes.byref(one), N, N, N, N, ctypes.byref(one), N, 0,
                                      vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_spmv(N, N, _capi.OP_N, 1, 1, 0, ctypes.byref(one), N, N, N, N, ctypes.byref(one), N, 0,
                                      vt) == _capi.INVALID_HANDLE
        assert lib.spblas_gfx950_spmm_strided(N, N, 1, 1, 1, 0, ctypes.byref(one), N, N, N, N, 1, 1, ctypes.byref(one), N,
                                              1, 1, 0, vt) == _capi.INVALID_HANDLE
    # (real types keep their order of checks: a null handle first)
    assert lib.spblas_gfx950_scale(N, 1, N, N, _capi.F32) == _capi.INVALID_HANDLE
    # value types beyond the enum are still invalid
    assert lib.spblas_gfx950_spmv_plan_create(N, N, 1, 1, 0, N, N, N, 0, 6, 0) == _capi.INVALID_HANDLE


def _csr(dt, colind_dtype=torch.int32):
    return sp.csr_view(torch.ones(2, dtype=dt), torch.tensor([0, 1, 2], dtype=torch.int32),
                       torch.tensor([0, 1], dtype=colind_dtype), (2, 2), 2)


@pytest.mark.parametrize("dt", LOWP, ids=_names)
def test_out_of_scope_16bit_operations_raise_type_error(dt):
    a = _csr(dt)
    name = _names(dt)
    c = sp.csr_view(None, torch.zeros(3, dtype=torch.int32), None, (2, 2), 0)
    x, y = torch.ones(2, dtype=dt), torch.ones(2, dtype=dt)
    with pytest.raises(TypeError, match=name):
        sp.multiply_compute(a, a, c)
    with pytest.raises(TypeError, match=name):
        sp.add(a, a, c)
    with pytest.raises(TypeError, match=name):
        sp.transpose(a, _csr(dt))
    with pytest.raises(TypeError, match=name):
        sp.triangular_solve(a, sp.lower_triangle, sp.explicit_diagonal, x, y)
    with pytest.raises(TypeError, match=name):
        sp.scale(2.0, a)
    with pytest.raises(TypeError, match=name):  # csc_view / transposed()
        sp.multiply(sp.transposed(a), x, y)
    with pytest.raises(TypeError, match=name):
        sp.multiply(sp.csc_view(a.values(), a.rowptr(), a.colind(), (2, 2), 2), x, y)
    with pytest.raises(TypeError, match=name):
        sp.multiply_inspect(sp.transposed(a), x, y)
    with pytest.raises(TypeError, match="int32 column"):  # int64 column indices
        sp.multiply(_csr(dt, torch.int64), x, y)
    with pytest.raises(TypeError, match="int32 column"):
        sp.multiply_inspect(_csr(dt, torch.int64), x, y)
    with pytest.raises(TypeError, match="int32 column"):
        sp.multiply(_csr(dt, torch.int64), torch.ones(2, 3, dtype=dt), torch.ones(2, 3, dtype=dt))
    with pytest.raises(TypeError, match="complex"):  # a complex scaled() factor
        sp.multiply(sp.scaled(1 + 2j, a), x, y)
    with pytest.raises(TypeError, match="complex"):
        sp.multiply(a, sp.scaled(1j, torch.ones(2, 3, dtype=dt)), torch.ones(2, 3, dtype=dt))


@pytest.mark.parametrize("dt", LOWP, ids=_names)
def test_mixed_value_types_raise_type_error(dt):
    a = _csr(dt)
    other = torch.bfloat16 if dt == torch.float16 else torch.float16
    for x, y in ((torch.ones(2), torch.ones(2, dtype=dt)), (torch.ones(2, dtype=dt), torch.ones(2)),
                 (torch.ones(2, dtype=other), torch.ones(2, dtype=dt))):
        with pytest.raises(TypeError, match="one value type"):
            sp.multiply(a, x, y)
    with pytest.raises(TypeError, match="value type"):  # a real A with 16-bit x
        sp.multiply(_csr(torch.float32), torch.ones(2, dtype=dt), torch.ones(2, dtype=dt))
    with pytest.raises(TypeError, match="one value type"):
        sp.multiply(a, torch.ones(2, 3, dtype=dt), torch.ones(2, 3, dtype=torch.float32))


@pytest.mark.parametrize("dt", LOWP, ids=_names)
def test_multi_gpu_paths_reject_16bit_values(dt):
    from spblas_reference_amd import sharded
    a = _csr(dt)
    for make in (lambda: sharded.ShardedSpMV(a, [0, 2]), lambda: sharded.PipelinedShardedSpMV([a], [(0, 2)]),
                 lambda: sharded.OverlappedShardedSpMV(a, [(0, 2)]), lambda: sharded.FusedShardedSpMV(a, [0, 2]),
                 lambda: sharded.ShardedSpMM(a, [0, 2], 4)):
        with pytest.raises(TypeError, match=_names(dt)):
            make()
