"""CPU tests of triangular_solve with a block of right-hand sides (no GPU): the checker of tests/trsm_util.py is proved on
a numpy emulation of the device's lane-wide sums -- it accepts the emulation on every generator and refuses swapped columns
and a single element that is off --, the C ABI declares, exports and binds spblas_gfx950_sptrsm_solve and orders its first
checks like the other real-only entry points, the Python layer raises its argument errors on CPU tensors, and the drop-in
headers' new overloads compile inside the reference tree (a complex or mixed-type call matches nothing)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import spblas_reference_amd as sp
import trsm_util as TU
from oracle.reference_build import REF
from spblas_reference_amd import _build, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "compile_check", "dropin_trsm_check.cpp")
VENDOR = os.path.join("include", "spblas", "vendor", "gfx950")


# ---- the checker -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", TU.GENERATORS)
def test_checker_accepts_a_lane_wide_solve_and_refuses_wrong_ones(name, dtype):
    """An X computed in the value type with each row summed 8 lanes wide and then by a tree passes both bounds on every
    generator, both triangles and both diagonal modes alternating over the generators; the same X with two columns swapped
    fails; the same X with ONE element off by a relative 1e-3 (fp32) / 1e-9 (fp64) fails."""
    gi = TU.GENERATORS.index(name)
    upper, unit = bool(gi & 1), bool((gi >> 1) & 1) ^ (dtype is np.float64)
    M = TU.system(name, upper, unit)
    m = M.shape[0]
    B = TU.rhs(m, 5, seed=gi)
    ref = TU.oracle_block(M, B, upper, unit, dtype)
    X = TU.emulate(M, B, upper, unit, dtype)
    assert TU.violations(M, B, X, upper, unit, dtype, ref=ref) == []
    swapped = X.copy()
    swapped[:, [1, 3]] = swapped[:, [3, 1]]
    assert TU.violations(M, B, swapped, upper, unit, dtype, ref=ref) != []
    off = X.copy()
    r, c = m // 2, 2
    off[r, c] *= dtype(1 + (1e-3 if dtype is np.float32 else 1e-9))
    assert off[r, c] != X[r, c]
    assert TU.violations(M, B, off, upper, unit, dtype, ref=ref) != []


def test_checker_looks_at_the_last_row_and_the_last_column():
    M = TU.system("tri500", False, False)
    B = TU.rhs(500, 9)
    X = TU.emulate(M, B, False, False, np.float64)
    for r, c in ((499, 8), (0, 0), (499, 0), (0, 8)):
        off = X.copy()
        off[r, c] *= 1 + 1e-9
        assert TU.violations(M, B, off, False, False, np.float64) != [], (r, c)
    assert TU.violations(M, B, X[:, :8], False, False, np.float64) != []   # a missing column is not a pass


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_sptrsm_solve_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spblas_gfx950.h")).read(), flags=re.S)
    assert re.search(r"\bspblas_gfx950_sptrsm_solve\s*\(", text)
    bound = {n: args for n, _, args in _capi.PROTOTYPES}
    # the vector solve's arguments plus n and two strides per operand
    assert len(bound["spblas_gfx950_sptrsm_solve"]) == len(bound["spblas_gfx950_sptrsv_solve"]) + 5
    _build.build()
    assert hasattr(ctypes.CDLL(_capi.library_path()), "spblas_gfx950_sptrsm_solve")
    assert "sptrsm.hip" in _build.SOURCES and "device_sptrsm" in _build.EXAMPLES


def test_sptrsm_solve_orders_its_first_checks_like_the_other_real_only_entry_points():
    lib = _capi.lib()
    N = None
    for vt in (_capi.C32, _capi.C64, _capi.F16, _capi.BF16):   # before any other check: a null handle, null pointers
        assert lib.spblas_gfx950_sptrsm_solve(N, N, 1, 0, 1, N, N, N, N, N, 1, 1, N, 1, 1, vt) == _capi.NOT_SUPPORTED
    for vt in (_capi.F32, _capi.F64):
        assert lib.spblas_gfx950_sptrsm_solve(N, N, 1, 0, 1, N, N, N, N, N, 1, 1, N, 1, 1, vt) == _capi.INVALID_HANDLE


# ---- Python argument errors (CPU tensors: raised before anything touches a device) ----------------------------------
def _cpu_matrix(dtype=torch.float32, m=4):
    return sp.csr_view(torch.ones(m, dtype=dtype), torch.arange(m + 1, dtype=torch.int32), torch.arange(m, dtype=torch.int32),
                       (m, m), m)


@pytest.mark.parametrize("call", [sp.triangular_solve, sp.triangular_solve_inspect])
def test_python_argument_errors_for_matrix_operands(call):
    a = _cpu_matrix()
    lo, ex = sp.lower_triangle, sp.explicit_diagonal
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    msg = "matrix and vector dimensions are incompatible"
    with pytest.raises(ValueError, match=msg):   # a 1-D / 2-D mix, either way round
        call(a, lo, ex, z(4, 3), z(4))
    with pytest.raises(ValueError, match=msg):
        call(a, lo, ex, z(4), z(4, 1))
    with pytest.raises(ValueError, match=msg):   # unequal n
        call(a, lo, ex, z(4, 3), z(4, 2))
    with pytest.raises(ValueError, match=msg):   # wrong m, in B and in X
        call(a, lo, ex, z(5, 3), z(4, 3))
    with pytest.raises(ValueError, match=msg):
        call(a, lo, ex, z(4, 3), z(3, 3))
    with pytest.raises(ValueError, match=msg):   # rank 3
        call(a, lo, ex, z(4, 3, 1), z(4, 3, 1))
    with pytest.raises(TypeError, match="value type"):
        call(a, lo, ex, z(4, 3, dtype=torch.float64), z(4, 3))
    with pytest.raises(TypeError, match="value type"):
        call(a, lo, ex, z(4, 3), z(4, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="row-major"):   # neither layout: every second column of a wider tensor
        call(a, lo, ex, z(4, 6)[:, ::2], z(4, 3))
    with pytest.raises(ValueError, match="row-major"):
        call(a, lo, ex, z(4, 3), z(8, 6)[::2, ::2])
    with pytest.raises(TypeError):
        call(a, "lower", ex, z(4, 3), z(4, 3))
    with pytest.raises(NotImplementedError):     # X is a plain tensor, as for the vector
        call(a, lo, ex, z(4, 3), sp.scaled(2.0, z(4, 3)))


def test_complex_and_16_bit_matrix_operands_keep_their_type_error():
    lo, ex = sp.lower_triangle, sp.explicit_diagonal
    for dtype, word in ((torch.complex64, "complex"), (torch.float16, "16-bit|half|bf16|fp16|float16"),
                        (torch.bfloat16, "16-bit|half|bf16|fp16|bfloat16")):
        a = _cpu_matrix(dtype)
        with pytest.raises(TypeError, match=word):
            sp.triangular_solve(a, lo, ex, torch.ones((4, 3), dtype=dtype), torch.ones((4, 3), dtype=dtype))
        with pytest.raises(TypeError):
            sp.triangular_solve(_cpu_matrix(), lo, ex, torch.ones((4, 3), dtype=dtype), torch.ones((4, 3)))


# ---- the drop-in overloads, compiled inside the reference tree -------------------------------------------------------
def _compile(tmp_path, extra):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    from oracle.reference_build import compile_flags, patched_reference_headers
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    return subprocess.run([gxx, "-fsyntax-only"] + extra + compile_flags(scratch) + [CHECK], capture_output=True, text=True)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
def test_dropin_matrix_overloads_compile_on_both_layouts(tmp_path):
    r = _compile(tmp_path, [])
    assert r.returncode == 0, "the block overloads do not compile inside the reference tree:\n" + r.stderr[-6000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
@pytest.mark.parametrize("case", ["SPBLAS_TRSM_COMPLEX", "SPBLAS_TRSM_MIXED"])
def test_dropin_complex_or_mixed_block_solve_is_no_matching_function(tmp_path, case):
    r = _compile(tmp_path, ["-D" + case])
    assert r.returncode != 0
    assert "no matching function" in r.stderr
    errors = [ln for ln in r.stderr.splitlines() if " error: " in ln or ln.startswith("error:")]
    assert errors
    inside = [ln for ln in errors if VENDOR in ln]
    assert not inside, "errors inside the backend headers:\n" + "\n".join(inside)


def test_standalone_layer_and_example_build_with_gxx():
    """include/spblas_gfx950/spblas.hpp with the mdspan_row_major overloads, through examples/device_sptrsm.cpp."""
    out = _build.build_examples()
    assert any(p.endswith("device_sptrsm") and os.path.exists(p) for p in out)
