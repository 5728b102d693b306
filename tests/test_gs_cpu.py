"""CPU tests of the multicolour Gauss-Seidel sweeps: the host model, the structure check and the generators of tests/gs_util.py
on every system the GPU tests use, the build lists, the C ABI surface, the drop-in header inside the reference tree and every
refusal that needs no device.  Fails on a backend without the feature: the names do not exist there."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gs_util as GS
import spblas_reference_amd as sp
from spblas_reference_amd import _build, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/include"
CHECK = os.path.join(ROOT, "tests", "compile_check", "dropin_gs_check.cpp")
NAMES = ["gs_create", "gs_destroy", "gs_info", "gs_sweep"]
LANES = (4, 8, 16, 64)


# ---- the dyadic systems are exact: float32 in stored order = float32 in a permuted order = float64 ---------------------------
@pytest.mark.parametrize("lanes", LANES)
def test_dyadic_systems_are_exact_for_two_sweeps(lanes):
    y = GS.dyadic_system(lanes)
    assert y.lanes == lanes
    assert GS.structure_violations(y.rowptr, y.colind, y.color_ptr, y.perm) == []
    assert GS.structure_violations(y.b_rowptr, y.b_colind, y.color_ptr) == []
    assert (np.diff(y.color_ptr) == 0).any(), "no empty colour"
    for omega in GS.OMEGAS:
        for direction in GS.DIRECTIONS:
            for sweeps in (1, 2):
                stored, _ = GS.reference(y, sweeps, omega, direction, np.float32)
                shuffled, _ = GS.reference(y, sweeps, omega, direction, np.float32, perm_seed=3)
                wide, _ = GS.reference(y, sweeps, omega, direction, np.float64)
                on_b, _ = GS.reference(y, sweeps, omega, direction, np.float32, on_b=True)
                what = (omega, direction, sweeps)
                assert stored.dtype == np.float32 and np.isfinite(wide).all()
                assert np.array_equal(stored.astype(np.float64), wide), what
                assert np.array_equal(shuffled.astype(np.float64), wide), what
                assert np.array_equal(on_b.astype(np.float64), wide[y.perm]), what      # B = P A P^T: the same iterates, moved


@pytest.mark.parametrize("lanes", LANES)
def test_dyadic_systems_hold_the_shapes_they_claim(lanes):
    y = GS.dyadic_system(lanes)
    rows = np.repeat(np.arange(y.m), np.diff(y.rowptr))
    off = np.bincount(rows[y.colind != rows], minlength=y.m)
    assert set(GS.shape_counts(lanes)) <= set(off.tolist())
    # the diagonal first, in the middle and last, for every count
    place = {}
    for r in range(y.m):
        c = y.colind[y.rowptr[r]:y.rowptr[r + 1]]
        at = int(np.flatnonzero(c == r)[0])
        place.setdefault(int(off[r]), set()).add("first" if at == 0 else "last" if at == c.size - 1 else "middle")
    for k in GS.shape_counts(lanes):
        assert place[k] >= ({"first", "middle", "last"} if k >= 2 else {"first"}), (k, place[k])
    # values, b and x0 as promised; quiet rows hold the diagonal alone; some off-diagonal entry is stored twice
    d = y.colind == rows
    assert set(np.abs(y.values[d]).tolist()) <= {1.0, 2.0} and set(np.abs(y.values[~d]).tolist()) == {1.0}
    assert np.abs(y.b).max() <= 4 and np.abs(y.x0).max() <= 4 and (y.b == np.round(y.b)).all() and (y.x0 == np.round(y.x0)).all()
    assert (off[y.quiet] == 0).all() and y.quiet.size == y.color_ptr[1]
    assert any(np.unique(y.colind[y.rowptr[r]:y.rowptr[r + 1]]).size < y.rowptr[r + 1] - y.rowptr[r] for r in range(y.m))
    # at omega = 1 a quiet row is b / d from the first sweep on, whatever it held
    x, _ = GS.reference(y, 1, 1.0, "forward")
    dq = np.zeros(y.m)
    dq[rows[d]] = y.values[d]
    assert np.array_equal(x[y.quiet], y.b[y.quiet] / dq[y.quiet])


def test_forward_backward_and_jacobi_differ_on_the_coloured_chain():
    y = GS.colored_chain()
    assert GS.structure_violations(y.rowptr, y.colind, y.color_ptr, y.perm) == []
    f, _ = GS.reference(y, 1, 1.0, "forward")
    b, _ = GS.reference(y, 1, 1.0, "backward")
    s, _ = GS.reference(y, 1, 1.0, "symmetric")
    j = GS.host_jacobi(y.rowptr, y.colind, y.values, y.b, y.x0)
    for p, q in ((f, b), (f, j), (b, j), (s, f), (s, b)):
        assert not np.array_equal(p, q)
    for direction in GS.DIRECTIONS:                       # exact as well: float32 = float64
        for omega in GS.OMEGAS:
            lo, _ = GS.reference(y, 2, omega, direction, np.float32)
            hi, _ = GS.reference(y, 2, omega, direction, np.float64)
            assert np.array_equal(lo.astype(np.float64), hi)


def test_sweeps_zero_returns_x0_and_directions_compose():
    y = GS.dominant_system(40, seed=1)
    x, _ = GS.reference(y, 0, 1.0, "symmetric")
    assert np.array_equal(x, y.x0)
    f, _ = GS.reference(y, 1, 0.75, "forward")
    fb, _ = GS.host_gauss_seidel(y.rowptr, y.colind, y.values, y.b, f, y.color_ptr, y.perm, 1, 0.75, "backward", np.float64)
    s, _ = GS.reference(y, 1, 0.75, "symmetric")
    assert np.array_equal(s, fb)                           # a symmetric sweep IS forward followed by backward


def test_forward_sweep_is_the_dense_lower_solve_in_sigmas_order():
    y = GS.dominant_system(40, seed=1)
    m = y.m
    A = np.zeros((m, m))
    rows = np.repeat(np.arange(m), np.diff(y.rowptr))
    np.add.at(A, (rows, y.colind), y.values)
    P = A[np.ix_(y.perm, y.perm)]                          # sigma's order: position i is row perm[i]
    DL, Up = np.tril(P), np.triu(P, 1)
    want = np.linalg.solve(DL, y.b[y.perm] - Up @ y.x0[y.perm])
    got, S = GS.reference(y, 1, 1.0, "forward")
    assert np.abs(got[y.perm] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert S.shape == (m,) and (S > 0).all()
    back = np.linalg.solve(np.triu(P), y.b[y.perm] - np.tril(P, -1) @ want)
    sym, _ = GS.reference(y, 1, 1.0, "symmetric")
    assert np.abs(sym[y.perm] - back).max() <= 1e-12 * max(1.0, np.abs(back).max())


@pytest.mark.parametrize("omega", [1.0, 0.75])
def test_dominant_systems_contract(omega):
    """By 1/2 in the maximum norm at omega = 1; at omega < 1 by 1 - omega / 2 (module docstring of gs_util)."""
    y = GS.dominant_system(2000, seed=3)
    assert GS.structure_violations(y.rowptr, y.colind, y.color_ptr, y.perm) == []
    assert int(np.diff(y.rowptr).max()) <= 9
    m = y.m
    import scipy.sparse as sps
    A = sps.csr_matrix((y.values, y.colind, y.rowptr), shape=(m, m))
    import scipy.sparse.linalg as spl
    exact = spl.spsolve(A.tocsc(), y.b)
    rate = 0.5 if omega == 1.0 else 1.0 - omega / 2.0
    x = y.x0.copy()
    err = np.abs(x - exact).max()
    for direction in ("forward", "backward", "symmetric"):
        x, _ = GS.host_gauss_seidel(y.rowptr, y.colind, y.values, y.b, x, y.color_ptr, y.perm, 1, omega, direction, np.float64)
        new = np.abs(x - exact).max()
        assert new <= rate * err + 1e-13, (direction, new, err)
        err = new


# ---- the structure check -----------------------------------------------------------------------------------------------------
def _all_systems():
    out = {f"dyadic_{g}": GS.dyadic_system(g) for g in LANES}
    out["chain"] = GS.colored_chain()
    out["dominant"] = GS.dominant_system(2000, seed=3)
    for name in GS.multicolor_fixtures():
        out[name] = GS.multicolor_system(name)
    return out


def test_structure_check_accepts_every_fixture():
    for name, y in _all_systems().items():
        assert GS.structure_violations(y.rowptr, y.colind, y.color_ptr, y.perm) == [], name
        assert GS.structure_violations(y.b_rowptr, y.b_colind, y.color_ptr) == [], name


def test_structure_check_rejects_each_of_the_five_violations():
    y = GS.dyadic_system(8)
    ok = lambda **kw: GS.structure_violations(kw.get("rowptr", y.rowptr), kw.get("colind", y.colind),
                                              kw.get("color_ptr", y.color_ptr), kw.get("perm", y.perm))
    assert ok() == []
    for cp in GS.bad_color_ptrs(y.color_ptr):
        assert ok(color_ptr=cp) != [], cp
    for pm in GS.bad_perms(y.perm):
        assert ok(perm=pm) != []
    for rp, ci in GS.bad_structures(y.rowptr, y.colind):
        assert ok(rowptr=rp, colind=ci) != []
    for rp, ci in GS.bad_diagonals(y.rowptr, y.colind):
        assert any("diagonal" in t for t in ok(rowptr=rp, colind=ci))
    planted = GS.same_colour_pairs(y)
    assert [w for w, _, _ in planted] == ["first", "middle", "last"]
    for where, rp, ci in planted:
        assert any("joins two rows" in t for t in ok(rowptr=rp, colind=ci)), where


# ---- build lists, the C ABI surface, the layers -------------------------------------------------------------------------------
def test_build_lists_name_the_new_source_and_example():
    assert "gauss_seidel.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "gauss_seidel.hip"))
    assert "device_gauss_seidel" in _build.EXAMPLES
    assert os.path.exists(os.path.join(ROOT, "examples", "device_gauss_seidel.cpp"))
    assert "examples/device_gauss_seidel" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "gauss_seidel.hip" in open(os.path.join(ROOT, "cmake", "SpblasGfx950.cmake")).read()
    assert "preload_gauss_seidel();" in open(os.path.join(_build.CSRC, "handle.hip")).read()
    out = _build.build_examples()
    assert any(p.endswith("device_gauss_seidel") and os.path.exists(p) for p in out)


def test_kernel_source_keeps_x_unrestricted_and_free_of_atomics():
    src = open(os.path.join(_build.CSRC, "gauss_seidel.hip")).read()
    kernel = src[src.index("void gs_color_kernel("):src.index("// ---- the inspect's checks")]
    assert re.search(r"\bT\* x,", kernel) and "__restrict__ x" not in kernel
    assert "atomic" not in kernel.lower() and "cooperative" not in kernel.lower()


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
                  os.path.join("include", "spblas", "vendor", "gfx950", "gauss_seidel_impl.hpp")):
        src = open(os.path.join(ROOT, layer)).read()
        for name in ("gauss_seidel_inspect(", "gauss_seidel(", "gs_direction"):
            assert name in src, (layer, name)
    assert "gauss_seidel_impl.hpp" in open(os.path.join(ROOT, "include", "spblas", "vendor", "gfx950", "gfx950.hpp")).read()


def test_sweep_orders_its_first_checks_like_the_other_solve_side_calls():
    lib = _capi.lib()
    N = None
    one = ctypes.c_float(1.0)
    for vt in (_capi.C32, _capi.C64, _capi.F16, _capi.BF16):   # before any other check: a null handle, null pointers
        assert lib.spblas_gfx950_gs_sweep(N, N, 1, 1, 1, 0, N, N, N, N, N, N, vt) == _capi.NOT_SUPPORTED
    assert lib.spblas_gfx950_gs_sweep(N, N, 1, 1, 1, 0, ctypes.byref(one), N, N, N, N, N, _capi.F32) == _capi.INVALID_HANDLE
    plan = ctypes.c_void_p()
    arr = (ctypes.c_int64 * 4)()
    assert lib.spblas_gfx950_gs_create(None, ctypes.byref(plan), 1, 1, None, None, 1, None, None) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_gs_destroy(None, None) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_gs_info(None, arr) == _capi.INVALID_POINTER


def _cpu_matrix(dtype=torch.float32, m=4, itype=torch.int32):
    return sp.csr_view(torch.ones(m, dtype=dtype), torch.arange(m + 1, dtype=itype), torch.arange(m, dtype=itype), (m, m), m)


def test_python_surface_and_argument_errors():
    for name in ("gauss_seidel", "gauss_seidel_inspect"):
        assert hasattr(sp, name)
    a = _cpu_matrix()
    cp = torch.tensor([0, 4], dtype=torch.int32)
    perm = torch.arange(4, dtype=torch.int32)
    b, x = torch.ones(4), torch.zeros(4)
    info = sp.operation_info_t()
    for dt in (torch.complex64, torch.complex128, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError):
            sp.gauss_seidel_inspect(_cpu_matrix(dt), cp)
        with pytest.raises(TypeError):
            sp.gauss_seidel(info, _cpu_matrix(dt), torch.ones(4, dtype=dt), torch.ones(4, dtype=dt))
    for fn in (lambda t: sp.gauss_seidel_inspect(t, cp), lambda t: sp.gauss_seidel_inspect(info, t, cp, perm),
               lambda t: sp.gauss_seidel(info, t, b, x)):
        with pytest.raises(TypeError):
            fn(_cpu_matrix(itype=torch.int64))
        with pytest.raises(TypeError):
            fn(sp.scaled(2.0, a))
        with pytest.raises(TypeError):
            fn(sp.conjugated(a))
        with pytest.raises(TypeError):
            fn(sp.transposed(a))
        with pytest.raises(TypeError):
            fn(sp.csc_view(a.values(), a.rowptr(), a.colind(), (4, 4), 4))
        with pytest.raises(ValueError):
            fn(sp.csr_view(torch.ones(4), torch.arange(5, dtype=torch.int32), torch.arange(4, dtype=torch.int32), (4, 5), 4))
    with pytest.raises(TypeError):
        sp.gauss_seidel_inspect(a, cp.to(torch.int64))
    with pytest.raises(TypeError):
        sp.gauss_seidel_inspect(a, [0, 4])
    with pytest.raises(TypeError):
        sp.gauss_seidel_inspect(a, cp, perm.to(torch.int64))
    with pytest.raises(ValueError):
        sp.gauss_seidel_inspect(a, cp, perm[:3])
    with pytest.raises(ValueError):
        sp.gauss_seidel_inspect(a, torch.zeros(8, dtype=torch.int32)[::2])      # not contiguous
    with pytest.raises(TypeError):
        sp.gauss_seidel_inspect(a)
    with pytest.raises(TypeError):
        sp.gauss_seidel_inspect(info, a)
    # the sweep's arguments, in front of the info check
    with pytest.raises(TypeError):
        sp.gauss_seidel(info, a, sp.scaled(2.0, b), x)
    with pytest.raises(TypeError):
        sp.gauss_seidel(info, a, b.double(), x)
    with pytest.raises(ValueError):
        sp.gauss_seidel(info, a, torch.ones(5), x)
    with pytest.raises(ValueError):
        sp.gauss_seidel(info, a, b, torch.zeros(8)[::2])
    with pytest.raises(ValueError):
        sp.gauss_seidel(info, a, x, x)
    with pytest.raises(NotImplementedError):
        sp.gauss_seidel(info, a, torch.ones(4, 2), torch.ones(4, 2))
    for bad in (True, 1.0, "1", None):
        with pytest.raises(TypeError):
            sp.gauss_seidel(info, a, b, x, sweeps=bad)
    with pytest.raises(ValueError):
        sp.gauss_seidel(info, a, b, x, sweeps=-1)
    with pytest.raises(TypeError):
        sp.gauss_seidel(info, a, b, x, omega="1")
    for bad in ("up", "Forward", 0, None):
        with pytest.raises(ValueError):
            sp.gauss_seidel(info, a, b, x, direction=bad)
    # an info that is no Gauss-Seidel inspect: ValueError, never a hidden inspect
    with pytest.raises(ValueError):
        sp.gauss_seidel(info, a, b, x)
    with pytest.raises(ValueError):
        sp.gauss_seidel(None, a, b, x)
    # well-formed host operands reach the device check: there is no CPU path
    with pytest.raises(RuntimeError):
        sp.gauss_seidel_inspect(a, cp)


def _compile(tmp_path, extra):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    from oracle.reference_build import compile_flags, patched_reference_headers
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    return subprocess.run([gxx, "-fsyntax-only"] + extra + compile_flags(scratch) + [CHECK], capture_output=True, text=True)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
def test_dropin_gauss_seidel_compiles_inside_the_reference_tree(tmp_path):
    r = _compile(tmp_path, [])
    assert r.returncode == 0, "gauss_seidel_impl.hpp does not compile inside the reference tree:\n" + r.stderr[-6000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
@pytest.mark.parametrize("case", ["SPBLAS_GS_COMPLEX", "SPBLAS_GS_SCALED", "SPBLAS_GS_WIDE"])
def test_dropin_gauss_seidel_out_of_scope_operands_are_no_matching_function(tmp_path, case):
    r = _compile(tmp_path, ["-D" + case])
    assert r.returncode != 0
    assert "no matching function" in r.stderr


def test_shape_systems_are_exact_and_take_four_lanes():
    for name, y in GS.shape_systems(256).items():
        assert y.lanes == 4, name
        assert GS.structure_violations(y.rowptr, y.colind, y.color_ptr, y.perm) == [], name
        for omega in GS.OMEGAS:
            for direction in GS.DIRECTIONS:
                for sweeps in ((1, 2) if omega == 1.0 else (1,)):      # omega != 1: the deep chains gain two bits per update
                    lo, _ = GS.reference(y, sweeps, omega, direction, np.float32, perm_seed=1)
                    hi, _ = GS.reference(y, sweeps, omega, direction, np.float64)
                    assert np.array_equal(lo.astype(np.float64), hi), (name, omega, direction, sweeps)
    assert GS.shape_systems(256)["grid_stride"].color_ptr[1] == 256 * 16 * 64 + 1
