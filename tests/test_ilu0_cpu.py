"""CPU tests of ILU(0) (no GPU): the generators and checkers of tests/ilu_util.py are proved on a host IKJ loop -- it recovers
every exact family bit for bit in fp32 and fp64, the residual checker accepts the host factor of a random diagonally dominant
matrix and refuses an entry that is off by a step of its bound, a swapped pair and a skipped update --, the C ABI declares,
exports and binds the spblas_gfx950_ilu0_* entry points and orders their first checks like the other real-only entry points,
the Python layer raises its argument errors on CPU tensors, and the drop-in header compiles inside the reference tree."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ilu_util as U
import ladder_tt as TT
import spblas_reference_amd as sp
from oracle.reference_build import REF
from spblas_reference_amd import _build, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "compile_check", "dropin_ilu0_check.cpp")
VENDOR = os.path.join("include", "spblas", "vendor", "gfx950")
NAMES = ["create", "destroy", "info", "status", "factor"]


# ---- the exact families --------------------------------------------------------------------------------------------------
def _families():
    out = {}
    for limit, extra, lanes in U.lane_cases()[:4]:
        out[f"shapes_{limit}_{extra}"] = U.shape_system(limit, extra)[:2]
    out["levels"] = U.level_pattern([60, 130, 3, 2, 140], seed=1, upper=(0, 6), long_rows=2, long_len=40)[:2]
    out["interleaved"] = U.interleave(*U.level_pattern([8, 5, 3], seed=2)[:2], 7)
    out["dense40"] = U.pattern_from_rows([list(range(40))] * 40)
    out["bidiagonal"] = U.pattern_from_rows([[i - 1] if i else [] for i in range(300)])
    out["diagonal"] = U.pattern_from_rows([[] for _ in range(20)])
    out["random"] = U.random_pattern(400, 30, seed=3, band=100)
    out["laplacian"] = U.laplacian7(7, 6, 5)
    return out


FAMILIES = _families()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_host_loop_recovers_every_exact_family(name, dtype):
    rowptr, colind = FAMILIES[name]
    U.check_pattern(rowptr, colind)
    a, want = U.exact_system(rowptr, colind, seed=len(name))
    assert not np.array_equal(a, want) or colind.size == rowptr.size - 1     # (a diagonal matrix is its own factor)
    got = U.host_ilu0(rowptr, colind, a, dtype)
    assert got.dtype == np.dtype(dtype)
    assert U.exact_violations(got, want, rowptr, colind) == []
    off = got.copy()
    off[colind.size // 2] *= dtype(-1)
    assert U.exact_violations(off, want, rowptr, colind) != []


def test_zero_pivot_family_keeps_the_independent_rows_exact():
    rowptr, colind, _ = U.level_pattern([200, 130, 40, 30], seed=9)
    for zeros in ((150,), (230, 90)):
        a, want = U.exact_system(rowptr, colind, seed=9, zero_pivots=zeros)
        got = U.host_ilu0(rowptr, colind, a, np.float32)
        clean = U.independent_rows(rowptr, colind, zeros)
        assert 0 < clean.sum() < clean.size
        assert U.exact_violations(got, want, rowptr, colind, rows_mask=clean) == []
        d = got[U.diag_positions(rowptr, colind)]
        bad = np.flatnonzero((d == 0) | ~np.isfinite(d))
        assert bad.min() == min(zeros) and set(zeros) <= set(bad.tolist())


def test_generators_hold_the_rungs_they_claim():
    for limit, extra, lanes in U.lane_cases():
        rowptr, colind, G, specs, front, _ = U.shape_system(limit, extra)
        m = rowptr.size - 1
        assert G == lanes and int(rowptr[-1]) == limit * m + extra
        rows = np.arange(front, front + len(specs))
        d = U.diag_positions(rowptr, colind)
        lows = d[rows] - rowptr[rows]
        ups = rowptr[rows + 1] - d[rows] - 1
        assert [tuple(x) for x in zip(lows.tolist(), ups.tolist())] == [tuple(s) for s in specs]
        assert set(U.lower_counts(G)) <= set(lows.tolist()) and set(U.upper_counts(G)) <= set(ups.tolist())
        cap = U.lds_cap(G)
        assert {cap - 1, cap, cap + 1} <= set((lows + ups + 1).tolist())
        # pivot rows run the same ladder: the shaped rows are read by the shaped rows behind them
        read = np.unique(np.concatenate([colind[rowptr[r]:d[r]] for r in rows]))
        assert np.isin(rows[:-8], read).mean() > 0.9
    widths = [200, 3, 130, 2]
    rowptr, colind, lev = U.level_pattern(widths, seed=4)
    assert np.bincount(lev).tolist() == widths and (np.diff(lev) < 0).any()   # rows not sorted by level
    assert U.predicted_info(rowptr, colind) == {"levels": 4, "max_level_width": 200, "launches_per_factor": 4, "lanes_per_row": 4}


# ---- the residual checker ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_residual_checker_accepts_the_host_factor_and_refuses_wrong_ones(dtype):
    rowptr, colind = U.random_pattern(500, 24, seed=5, band=120)
    a = U.dominant_values(rowptr, colind, seed=6).astype(dtype)
    lu = U.host_ilu0(rowptr, colind, a, dtype)
    assert U.residual_violations(rowptr, colind, a, lu, dtype) == []
    rows = np.repeat(np.arange(500), np.diff(rowptr))
    # (1) ONE entry of U off by three times its own bound (its l is the implied 1, so the residual moves by exactly that)
    L, Up = U.split_lu(rowptr, colind, lu)
    p = int(np.flatnonzero((rows == 250) & (colind > 250))[0])
    terms = int((L[250].toarray().ravel() != 0) @ (Up[:, colind[p]].toarray().ravel() != 0))
    mag = float(np.abs(L[250].toarray().ravel()) @ np.abs(Up[:, colind[p]].toarray().ravel()))
    step = 3 * (terms + 2) * U.EPS[np.dtype(dtype)] * (abs(float(a[p])) + mag)
    off = lu.astype(np.float64)
    off[p] += step
    assert off[p] != lu[p]
    assert U.residual_violations(rowptr, colind, a, off, dtype) != []
    # (2) one swapped pair of neighbouring entries
    swapped = lu.copy()
    q = int(rowptr[100]) + 3
    swapped[q], swapped[q + 1] = lu[q + 1], lu[q]
    assert U.residual_violations(rowptr, colind, a, swapped, dtype) != []
    # (3) one skipped update: row 300 leaves out the pivot step of its first lower column
    k = int(colind[rowptr[300]])
    assert k < 300
    skipped = U.host_ilu0(rowptr, colind, a, dtype, skip_update=(300, k))
    assert not np.array_equal(skipped, lu)
    assert U.residual_violations(rowptr, colind, a, skipped, dtype) != []
    # ... and A itself is no factor of A
    assert U.residual_violations(rowptr, colind, a, a, dtype) != []


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_ilu0_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spblas_gfx950.h")).read(), flags=re.S)
    bound = {n for n, _, _ in _capi.PROTOTYPES}
    _build.build()
    dll = ctypes.CDLL(_capi.library_path())
    for n in NAMES:
        name = f"spblas_gfx950_ilu0_{n}"
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in bound and hasattr(dll, name), name
    assert "ilu0.hip" in _build.SOURCES and "device_ilu0" in _build.EXAMPLES


def test_ilu0_factor_orders_its_first_checks_like_the_other_real_only_entry_points():
    lib = _capi.lib()
    N = None
    for vt in (_capi.C32, _capi.C64, _capi.F16, _capi.BF16):   # before any other check: a null handle, null pointers
        assert lib.spblas_gfx950_ilu0_factor(N, N, 1, 1, N, N, N, N, vt) == _capi.NOT_SUPPORTED
    for vt in (_capi.F32, _capi.F64):
        assert lib.spblas_gfx950_ilu0_factor(N, N, 1, 1, N, N, N, N, vt) == _capi.INVALID_HANDLE


def test_ilu0_entry_points_refuse_a_null_handle():
    lib = _capi.lib()
    plan, row = ctypes.c_void_p(), ctypes.c_int64(0)
    assert lib.spblas_gfx950_ilu0_create(None, ctypes.byref(plan), 1, 1, None, None) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_ilu0_status(None, None, ctypes.byref(row)) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_ilu0_destroy(None, None) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_ilu0_info(None, None) == _capi.INVALID_POINTER


def test_limits_are_read_from_the_source():
    t = U.ilu0_limits()
    assert t["lds_per_lane"] >= 1 and t["level_threads"] % 64 == 0 and t["chain_threads"] % 64 == 0
    assert [c[2] for c in U.lane_cases()] == [4, 8, 8, 16, 16, 64]
    assert U.lds_cap(4) == 4 * t["lds_per_lane"]


# ---- Python argument errors (CPU tensors: raised before anything touches a device) -----------------------------------------
def _cpu_matrix(dtype=torch.float32, m=4, itype=torch.int32):
    return sp.csr_view(torch.ones(m, dtype=dtype), torch.arange(m + 1, dtype=itype), torch.arange(m, dtype=itype), (m, m), m)


def test_python_surface_and_argument_errors():
    for name in ("ilu0_inspect", "ilu0", "ilu0_status"):
        assert hasattr(sp, name)
    a = _cpu_matrix()
    for wrapped in (sp.scaled(2.0, a), sp.conjugated(a), sp.transposed(a),
                    sp.csc_view(a.values(), a.rowptr(), a.colind(), (4, 4), 4)):
        with pytest.raises(TypeError):
            sp.ilu0_inspect(wrapped)
        with pytest.raises(TypeError):
            sp.ilu0(wrapped, a)
    for dtype in (torch.complex64, torch.complex128, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match=str(dtype).replace("torch.", "")):
            sp.ilu0_inspect(_cpu_matrix(dtype))
        with pytest.raises(TypeError, match=str(dtype).replace("torch.", "")):
            sp.ilu0(_cpu_matrix(dtype), _cpu_matrix(dtype))
    with pytest.raises(TypeError, match="int32"):
        sp.ilu0_inspect(_cpu_matrix(itype=torch.int64))
    with pytest.raises(TypeError, match="int32"):
        sp.ilu0_inspect(sp.csr_view(a.values(), a.rowptr().to(torch.int64), a.colind(), (4, 4), 4))
    with pytest.raises(ValueError):    # not square
        sp.ilu0_inspect(sp.csr_view(a.values(), a.rowptr(), a.colind(), (4, 5), 4))
    lu = lambda v: sp.csr_view(v, a.rowptr(), a.colind(), (4, 4), 4)
    with pytest.raises(ValueError):    # too short
        sp.ilu0(a, lu(torch.ones(3)))
    with pytest.raises(ValueError):    # another value type
        sp.ilu0(a, lu(torch.ones(4, dtype=torch.float64)))
    with pytest.raises(ValueError):    # another device
        sp.ilu0(a, lu(torch.ones(4, device="meta")))
    with pytest.raises(ValueError):    # not A's structure arrays
        sp.ilu0(a, sp.csr_view(torch.ones(4), a.rowptr().clone(), a.colind(), (4, 4), 4))
    with pytest.raises(TypeError):
        sp.ilu0(a, torch.ones(4))
    with pytest.raises(TypeError):
        sp.ilu0_status(sp.operation_info_t())
    with pytest.raises(RuntimeError, match="device"):   # well-formed CPU operands: there is no CPU fallback
        sp.ilu0(a, lu(torch.ones(4)))


# ---- the drop-in header, compiled inside the reference tree ---------------------------------------------------------------
def _compile(tmp_path, extra):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    from oracle.reference_build import compile_flags, patched_reference_headers
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    return subprocess.run([gxx, "-fsyntax-only"] + extra + compile_flags(scratch) + [CHECK], capture_output=True, text=True)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
def test_dropin_ilu0_compiles_inside_the_reference_tree(tmp_path):
    r = _compile(tmp_path, [])
    assert r.returncode == 0, "ilu0_impl.hpp does not compile inside the reference tree:\n" + r.stderr[-6000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
@pytest.mark.parametrize("case", ["SPBLAS_ILU0_COMPLEX", "SPBLAS_ILU0_SCALED", "SPBLAS_ILU0_WIDE"])
def test_dropin_ilu0_out_of_scope_operands_are_no_matching_function(tmp_path, case):
    r = _compile(tmp_path, ["-D" + case])
    assert r.returncode != 0
    assert "no matching function" in r.stderr
    errors = [ln for ln in r.stderr.splitlines() if " error: " in ln or ln.startswith("error:")]
    inside = [ln for ln in errors if VENDOR in ln]
    assert errors and not inside, "errors inside the backend headers:\n" + "\n".join(inside)


def test_standalone_layer_and_example_build_with_gxx():
    """include/spblas_gfx950/spblas.hpp with spblas::gfx950::ilu0*, through examples/device_ilu0.cpp."""
    out = _build.build_examples()
    assert any(p.endswith("device_ilu0") and os.path.exists(p) for p in out)
