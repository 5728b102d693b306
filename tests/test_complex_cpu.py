"""CPU tests of complex SpMV / SpMM support (no GPU): the C ABI declares and exports the complex value types and the two
conjugating entry points, the argument checks that need no device, the scaling-factor rule for conjugated complex
operands, the Python rejections of the out-of-scope operations, and compiler evidence for the drop-in headers
(tests/compile_check/dropin_complex_check.cpp: the call shapes of the reference's test/gtest/conjugate_test.cpp compile;
a complex SpGEMM does not match any overload)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import spblas_reference_amd as sp
from oracle.reference_build import REF
from spblas_reference_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "compile_check", "dropin_complex_check.cpp")
VENDOR = os.path.join("include", "spblas", "vendor", "gfx950")


def _header():
    return open(os.path.join(ROOT, "include", "spblas_gfx950.h")).read()


def test_header_declares_complex_types_and_entry_points():
    text = _header()
    assert re.search(r"SPBLAS_GFX950_C32\s*=\s*2", text) and re.search(r"SPBLAS_GFX950_C64\s*=\s*3", text)
    for name in ("spblas_gfx950_spmv_conj", "spblas_gfx950_spmm_strided_conj"):
        assert re.search(name + r"\s*\(", text), name
    assert (_capi.C32, _capi.C64, _capi.CONJ_A, _capi.CONJ_X) == (2, 3, 1, 2)
    bound = {n: args for n, _, args in _capi.PROTOTYPES}
    assert len(bound["spblas_gfx950_spmv_conj"]) == len(bound["spblas_gfx950_spmv"]) + 1
    assert len(bound["spblas_gfx950_spmm_strided_conj"]) == len(bound["spblas_gfx950_spmm_strided"]) + 1


def test_conj_entry_points_check_arguments_without_a_gpu():
    lib = _capi.lib()
    one = ctypes.c_float(1)
    # bits above 1: INVALID_VALUE before anything else
    assert lib.spblas_gfx950_spmv_conj(None, None, 0, 1, 1, 0, ctypes.byref(one), None, None, None, None, ctypes.byref(one),
                                       None, 0, _capi.C32, 4) == _capi.INVALID_VALUE
    # non-zero flags with a real value type
    assert lib.spblas_gfx950_spmv_conj(None, None, 0, 1, 1, 0, ctypes.byref(one), None, None, None, None, ctypes.byref(one),
                                       None, 0, _capi.F32, _capi.CONJ_A) == _capi.INVALID_VALUE
    assert lib.spblas_gfx950_spmm_strided_conj(None, None, 1, 1, 1, 0, ctypes.byref(one), None, None, None, None, 1, 1,
                                               ctypes.byref(one), None, 1, 1, 0, _capi.F64, _capi.CONJ_X) == _capi.INVALID_VALUE
    # complex with a null handle
    for vt in (_capi.C32, _capi.C64):
        assert lib.spblas_gfx950_spmv(None, None, 0, 1, 1, 0, ctypes.byref(one), None, None, None, None, ctypes.byref(one),
                                      None, 0, vt) == _capi.INVALID_HANDLE
        assert lib.spblas_gfx950_spmm_strided_conj(None, None, 1, 1, 1, 0, ctypes.byref(one), None, None, None, None, 1, 1,
                                                   ctypes.byref(one), None, 1, 1, 0, vt, 3) == _capi.INVALID_HANDLE


def test_real_only_entry_points_return_not_supported_for_complex():
    """Every entry point that takes a value type and has no complex form says NOT_SUPPORTED for C32 / C64, before any
    other check (here: a null handle and null pointers)."""
    lib = _capi.lib()
    N = None
    for vt in (_capi.C32, _capi.C64):
        assert lib.spblas_gfx950_spgemm_numeric(N, N, N, N, N, N, N, N, N, N, N, N, 0, vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_spgemm_numeric_addend(N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, 0,
                                                       vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_csr_add_numeric(N, N, N, N, N, N, N, N, N, N, N, N, N, 0, vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_csr_transpose(N, 1, 1, 0, N, N, N, N, N, N, vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_scale(N, 1, N, N, vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_sptrsv_solve(N, N, 1, 0, N, N, N, N, N, N, vt) == _capi.NOT_SUPPORTED
    # (real types keep their order of checks: a null handle first)
    assert lib.spblas_gfx950_scale(N, 1, N, N, _capi.F32) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_csr_transpose(N, 1, 1, 0, N, N, N, N, N, N, _capi.F64) == _capi.INVALID_HANDLE


def test_multi_gpu_paths_reject_complex_values():
    from spblas_reference_amd import sharded
    a = sp.csr_view(torch.ones(2, dtype=torch.complex64), torch.tensor([0, 1, 2], dtype=torch.int32),
                    torch.tensor([0, 1], dtype=torch.int32), (2, 2), 2)
    for make in (lambda: sharded.ShardedSpMV(a, [0, 2]), lambda: sharded.PipelinedShardedSpMV([a], [(0, 2)]),
                 lambda: sharded.OverlappedShardedSpMV(a, [(0, 2)]), lambda: sharded.FusedShardedSpMV(a, [0, 2]),
                 lambda: sharded.ShardedSpMM(a, [0, 2], 4)):
        with pytest.raises(TypeError, match="complex"):
            make()


def test_complex_scaling_factor_rule():
    """A factor is conjugated iff an odd number of conjugated views wrap it (views/conjugated_view_impl.hpp)."""
    a = object()
    f = sp.api.complex_scaling_factor
    assert f(sp.scaled(1 + 2j, sp.conjugated(a))) == 1 + 2j
    assert f(sp.conjugated(sp.scaled(1 + 2j, a))) == 1 - 2j
    assert f(sp.conjugated(sp.conjugated(sp.scaled(1 + 2j, a)))) == 1 + 2j
    assert f(sp.conjugated(sp.scaled(1 + 2j, sp.conjugated(sp.scaled(3j, a))))) == (1 - 2j) * 3j
    assert f(sp.scaled(2j, a), sp.conjugated(sp.scaled(1j, a))) == 2j * -1j
    assert f(a) is None
    assert f(sp.scaled(2.0, a), sp.scaled(3.0, a)) == 6.0


def test_out_of_scope_complex_operations_raise_type_error():
    c64 = torch.complex64
    a = sp.csr_view(torch.ones(2, dtype=c64), torch.tensor([0, 1, 2], dtype=torch.int32),
                    torch.tensor([0, 1], dtype=torch.int32), (2, 2), 2)
    c = sp.csr_view(None, torch.zeros(3, dtype=torch.int32), None, (2, 2), 0)
    with pytest.raises(TypeError, match="complex"):
        sp.multiply_compute(a, a, c)
    with pytest.raises(TypeError, match="complex"):
        sp.add(a, a, c)
    with pytest.raises(TypeError, match="complex"):
        sp.triangular_solve(a, sp.lower_triangle, sp.explicit_diagonal, torch.ones(2, dtype=c64), torch.ones(2, dtype=c64))
    with pytest.raises(TypeError, match="csr_view"):
        sp.multiply(sp.transposed(a), torch.ones(2, dtype=c64), torch.ones(2, dtype=c64))
    with pytest.raises(TypeError, match="int32 column"):
        sp.multiply(sp.csr_view(a.values(), a.rowptr(), a.colind().long(), (2, 2), 2), torch.ones(2, dtype=c64),
                    torch.ones(2, dtype=c64))
    with pytest.raises(ValueError):
        sp.multiply(a, torch.ones(2, dtype=c64), torch.ones(2, dtype=c64).conj())


def _compile(tmp_path, extra):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    from oracle.reference_build import compile_flags, patched_reference_headers
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    return subprocess.run([gxx, "-fsyntax-only"] + extra + compile_flags(scratch) + [CHECK], capture_output=True, text=True)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
def test_dropin_complex_call_shapes_compile(tmp_path):
    r = _compile(tmp_path, [])
    assert r.returncode == 0, "complex call shapes do not compile inside the reference tree:\n" + r.stderr[-6000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
@pytest.mark.parametrize("case", ["SPBLAS_COMPLEX_SPGEMM", "SPBLAS_COMPLEX_MIXED"])
def test_dropin_complex_out_of_scope_is_no_matching_function(tmp_path, case):
    """a complex SpGEMM, and a complex A with a real dense B: no overload matches, no error inside the backend headers"""
    r = _compile(tmp_path, ["-D" + case])
    assert r.returncode != 0
    assert "no matching function" in r.stderr
    errors = [ln for ln in r.stderr.splitlines() if " error: " in ln or ln.startswith("error:")]
    assert errors
    inside = [ln for ln in errors if VENDOR in ln]
    assert not inside, "errors inside the backend headers:\n" + "\n".join(inside)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
def test_cpp_complex_scaling_factor_and_conj_flags_run_on_the_host(tmp_path):
    """tests/compile_check/complex_factor_check.cpp: the C++ rule (__gfx950::complex_scaling_factor, conj_flags) on
    nested scaled / conjugated views, compiled inside the reference tree and run on the CPU (no device, no library)."""
    from oracle.reference_build import compile_flags, patched_reference_headers
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    exe = str(tmp_path / "complex_factor_check")
    src = os.path.join(ROOT, "tests", "compile_check", "complex_factor_check.cpp")
    r = subprocess.run([shutil.which("g++"), "-O1", "-w"] + compile_flags(scratch) + [src, "-o", exe], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "all passed" in r.stdout, r.stdout + r.stderr
