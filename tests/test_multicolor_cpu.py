"""CPU tests of the multicolour ordering and the permutation: the host model and the checkers of tests/multicolor_util.py on
every fixture the GPU tests use, the figures the ordering promises on the 7-point Laplacian, the build lists, the C ABI surface
and every refusal that needs no device.  Fails on a backend without the feature: the names do not exist there."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import multicolor_util as M
import spblas_reference_amd as sp
from spblas_reference_amd import _build, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/include"
CHECK = os.path.join(ROOT, "tests", "compile_check", "dropin_permute_check.cpp")
NAMES = ["multicolor_create", "multicolor_destroy", "multicolor_info", "multicolor_copy", "csr_permute_create",
         "csr_permute_destroy", "csr_permute_values", "permute_vector"]
FIXTURES = M.fixtures()


def test_key_function_matches_a_scalar_evaluation():
    def key(v):
        x = ((v + 1) * 0x9E3779B1) & 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        x ^= x >> 16
        return (x << 32) | v
    k = M.keys(5000)
    assert [int(t) for t in k[:50]] == [key(v) for v in range(50)] and int(k[4999]) == key(4999)
    assert np.unique(k).size == k.size


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_model_is_a_proper_colouring_on_every_fixture(name):
    rowptr, colind = FIXTURES[name]
    color = M.model_colors(rowptr, colind)
    perm, inverse, color_ptr = M.order_from_colors(color)
    assert M.check_order(rowptr, colind, color, perm, inverse, color_ptr) == []
    m = rowptr.size - 1
    if name.startswith("complete_"):
        assert color_ptr.size - 1 == m                       # 17, 65, 130 colours: the last two cross the 64-colour windows
    if name.startswith("diagonal") or name == "one_row":
        assert color_ptr.size - 1 == 1
    if m:
        # B's triangles are no deeper than the colouring
        lo, up = M.level_counts(*M.host_permute(rowptr, colind, perm)[:2])
        assert lo <= color_ptr.size - 1 and up <= color_ptr.size - 1


def test_checker_refuses_wrong_results():
    rowptr, colind = FIXTURES["grid5_9x7"]
    color = M.model_colors(rowptr, colind)
    perm, inverse, color_ptr = M.order_from_colors(color)
    bad = color.copy()
    bad[1] = bad[0]                                                # neighbours 0 and 1 alike
    assert M.check_order(rowptr, colind, bad, *M.order_from_colors(bad)) != []
    swapped = perm.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert any("sorted" in t for t in M.check_order(rowptr, colind, color, swapped, inverse, color_ptr))
    assert M.check_order(rowptr, colind, color, perm, inverse, color_ptr[:-1]) != []
    # the one-sided fixtures: a colouring from the rows alone puts both ends of a one-sided entry into one class
    rp, ci = FIXTURES["one_sided"]
    own_rows = np.zeros(rp.size - 1, np.int32)                     # what a vertex sees that only reads its own row, at its worst
    assert M.check_order(rp, ci, own_rows, *M.order_from_colors(own_rows)) != []


def test_laplacian_12_takes_6_colours_and_6_levels_against_34():
    rowptr, colind = FIXTURES["lap7_12"]
    assert M.level_counts(rowptr, colind) == (34, 34)
    color = M.model_colors(rowptr, colind)
    perm, _, color_ptr = M.order_from_colors(color)
    assert color_ptr.size - 1 == 6
    b_rowptr, b_colind, _ = M.host_permute(rowptr, colind, perm)
    assert M.level_counts(b_rowptr, b_colind) == (6, 6)


def test_slow_path_frees_one_vertex_per_round_without_in_launch_visibility():
    rowptr, colind = FIXTURES["slow_path_300"]
    k = M.keys(300)
    S = M.neighbours(rowptr, colind)
    waits = sum(1 for v in range(300) if (k[S.indices[S.indptr[v]:S.indptr[v + 1]]] > k[v]).any())
    assert waits == 299


def test_host_permute_is_p_a_pt_with_stable_columns():
    import scipy.sparse as sps
    rng = np.random.default_rng(0)
    for name, (rowptr, colind) in M.permutation_matrices().items():
        m = rowptr.size - 1
        perm = rng.permutation(m).astype(np.int32)
        b_rowptr, b_colind, pos = M.host_permute(rowptr, colind, perm)
        vals = rng.integers(1, 9, colind.size).astype(np.float64)
        for i in range(m):
            c = b_colind[b_rowptr[i]:b_rowptr[i + 1]]
            assert (np.diff(c) >= 0).all()
            same = np.flatnonzero(np.diff(c) == 0)
            assert (np.diff(pos[b_rowptr[i]:b_rowptr[i + 1]])[same] > 0).all()    # equal columns keep the source order
        if m:
            A = sps.csr_matrix((vals, colind, rowptr), shape=(m, m))
            B = sps.csr_matrix((vals[pos], b_colind, b_rowptr), shape=(m, m))
            P = sps.csr_matrix((np.ones(m), (np.arange(m), perm)), shape=(m, m))
            assert abs(P @ A @ P.T - B).sum() == 0
        ident = M.host_permute(rowptr, colind, np.arange(m))
        if name in ("lap7_5x4x3",):                                               # sorted rows: the identity gives A's own arrays
            assert np.array_equal(ident[0], rowptr) and np.array_equal(ident[1], colind)
            assert np.array_equal(ident[2], np.arange(colind.size))


def test_build_lists_name_the_new_source_and_example():
    assert "multicolor.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "multicolor.hip"))
    assert "device_multicolor" in _build.EXAMPLES
    assert os.path.exists(os.path.join(ROOT, "examples", "device_multicolor.cpp"))
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "examples/device_multicolor" in ignored
    out = _build.build_examples()
    assert any(p.endswith("device_multicolor") and os.path.exists(p) for p in out)


def test_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spblas_gfx950.h")).read(), flags=re.S)
    bound = {n for n, _, _ in _capi.PROTOTYPES}
    _build.build()
    dll = ctypes.CDLL(_capi.library_path())
    for n in NAMES:
        full = "spblas_gfx950_" + n
        assert re.search(r"\b" + full + r"\s*\(", text), full
        assert full in bound and hasattr(dll, full), full
    for layer in (os.path.join("include", "spblas_gfx950", "spblas.hpp"),
                  os.path.join("include", "spblas", "vendor", "gfx950", "permute_impl.hpp")):
        src = open(os.path.join(ROOT, layer)).read()
        for name in ("multicolor_order", "permute_inspect", "permute(", "permute_vector"):
            assert name in src, (layer, name)
    assert "permute_impl.hpp" in open(os.path.join(ROOT, "include", "spblas", "vendor", "gfx950", "gfx950.hpp")).read()


def test_value_calls_order_their_first_checks_like_the_other_real_only_entry_points():
    lib = _capi.lib()
    N = None
    for vt in (_capi.C32, _capi.C64, _capi.F16, _capi.BF16):   # before any other check: a null handle, null pointers
        assert lib.spblas_gfx950_csr_permute_values(N, N, 1, N, N, vt) == _capi.NOT_SUPPORTED
        assert lib.spblas_gfx950_permute_vector(N, 1, N, N, N, vt, 0) == _capi.NOT_SUPPORTED
    assert lib.spblas_gfx950_csr_permute_values(N, N, 1, N, N, _capi.F32) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_permute_vector(N, 1, N, N, N, _capi.F64, 1) == _capi.INVALID_HANDLE


def test_entry_points_refuse_a_null_handle_and_null_plans():
    lib = _capi.lib()
    plan = ctypes.c_void_p()
    arr = (ctypes.c_int64 * 4)()
    assert lib.spblas_gfx950_multicolor_create(None, ctypes.byref(plan), 1, 1, None, None) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_multicolor_destroy(None, None) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_multicolor_copy(None, None, None, None, None, None) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_multicolor_info(None, arr) == _capi.INVALID_POINTER
    assert lib.spblas_gfx950_csr_permute_create(None, ctypes.byref(plan), 1, 1, None, None, None, None, None) == \
        _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_csr_permute_destroy(None, None) == _capi.INVALID_HANDLE


def _cpu_matrix(dtype=torch.float32, m=4, itype=torch.int32):
    return sp.csr_view(torch.ones(m, dtype=dtype), torch.arange(m + 1, dtype=itype), torch.arange(m, dtype=itype), (m, m), m)


def test_python_surface_and_argument_errors():
    for name in ("multicolor_order", "multicolor_order_t", "permute_inspect", "permute", "permute_vector"):
        assert hasattr(sp, name)
    a, b = _cpu_matrix(), _cpu_matrix()
    perm = torch.arange(4, dtype=torch.int32)
    for dt in (torch.complex64, torch.complex128, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError):
            sp.multicolor_order(_cpu_matrix(dt))
        with pytest.raises(TypeError):
            sp.permute(_cpu_matrix(dt), perm, _cpu_matrix(dt))
        with pytest.raises(TypeError):
            sp.permute_inspect(_cpu_matrix(dt), perm, _cpu_matrix(dt))
        with pytest.raises(TypeError):
            sp.permute_vector(perm, torch.ones(4, dtype=dt), torch.ones(4, dtype=dt))
    for fn in (sp.multicolor_order, lambda x: sp.permute(x, perm, b), lambda x: sp.permute_inspect(x, perm, b)):
        with pytest.raises(TypeError):
            fn(_cpu_matrix(itype=torch.int64))
        with pytest.raises(TypeError):
            fn(sp.scaled(2.0, a))
        with pytest.raises(TypeError):
            fn(sp.transposed(a))
        with pytest.raises(TypeError):
            fn(sp.csc_view(a.values(), a.rowptr(), a.colind(), (4, 4), 4))
        with pytest.raises(ValueError):
            fn(sp.csr_view(torch.ones(4), torch.arange(5, dtype=torch.int32), torch.arange(4, dtype=torch.int32), (4, 5), 4))
    with pytest.raises(TypeError):
        sp.permute(a, perm.to(torch.int64), b)
    with pytest.raises(ValueError):
        sp.permute(a, perm[:3], b)
    with pytest.raises(TypeError):
        sp.permute(a, perm, _cpu_matrix(torch.float64))                       # another value type
    with pytest.raises(TypeError):
        sp.permute(a, perm, sp.scaled(2.0, b))
    with pytest.raises(ValueError):
        sp.permute(a, perm, _cpu_matrix(m=5))                                 # another shape
    with pytest.raises(ValueError):
        sp.permute(a, perm, sp.csr_view(torch.ones(3), b.rowptr(), b.colind(), (4, 4), 4))   # too short
    with pytest.raises(ValueError):
        sp.permute(a, perm, a)                                                # no in-place form
    with pytest.raises(TypeError):
        sp.permute(a, perm)
    with pytest.raises(TypeError):
        sp.permute_inspect(a)
    x = torch.ones(4)
    with pytest.raises(ValueError):
        sp.permute_vector(perm, x, x)
    with pytest.raises(ValueError):
        sp.permute_vector(perm, x, torch.ones(5))
    with pytest.raises(TypeError):
        sp.permute_vector(perm, x, torch.ones(4, dtype=torch.float64))
    with pytest.raises(TypeError):
        sp.permute_vector(perm.to(torch.int64), x, torch.ones(4))
    # well-formed host operands reach the device check: there is no CPU path
    with pytest.raises(RuntimeError):
        sp.multicolor_order(a)
    with pytest.raises(RuntimeError):
        sp.permute(a, perm, b)
    with pytest.raises(RuntimeError):
        sp.permute_vector(perm, x, torch.ones(4))


def _compile(tmp_path, extra):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    from oracle.reference_build import compile_flags, patched_reference_headers
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    return subprocess.run([gxx, "-fsyntax-only"] + extra + compile_flags(scratch) + [CHECK], capture_output=True, text=True)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
def test_dropin_permute_compiles_inside_the_reference_tree(tmp_path):
    r = _compile(tmp_path, [])
    assert r.returncode == 0, "permute_impl.hpp does not compile inside the reference tree:\n" + r.stderr[-6000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
@pytest.mark.parametrize("case", ["SPBLAS_PERMUTE_COMPLEX", "SPBLAS_PERMUTE_SCALED", "SPBLAS_PERMUTE_WIDE"])
def test_dropin_permute_out_of_scope_operands_are_no_matching_function(tmp_path, case):
    r = _compile(tmp_path, ["-D" + case])
    assert r.returncode != 0
    assert "no matching function" in r.stderr
