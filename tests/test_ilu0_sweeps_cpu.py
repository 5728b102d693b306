"""CPU tests of ilu0_sweeps (no GPU): the host model of tests/ilu_sweeps_util.py -- the correctly rounded fma, the recurrence and
its fixed point, generators whose iterates really differ, mutations of the recurrence that must show --, the C ABI (declared,
exported, bound, first checks in the documented order), the Python layer's argument errors on CPU tensors, and the C++ layers
(the drop-in header inside the reference tree, the standalone layer through examples/device_ilu0_sweeps.cpp)."""
import ctypes
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import ilu_sweeps_util as S
import ilu_util as U
import spblas_reference_amd as sp
from oracle.reference_build import REF
from spblas_reference_amd import _build, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "compile_check", "dropin_ilu0_sweeps_check.cpp")
VENDOR = os.path.join("include", "spblas", "vendor", "gfx950")
NAME = "spblas_gfx950_ilu0_sweeps"
DTYPES = list(S.DTYPES)
ILU0_SWEEPS = sp.ilu0_sweeps     # the operation all of this file is about: without it nothing here is collected


# ---- the rounding --------------------------------------------------------------------------------------------------------
def test_round_once_on_double_rounding_cases():
    one, h = Fraction(1), Fraction(1, 2 ** 24)       # h = half a step of fp32 at 1
    f32 = lambda x: np.float32(x)
    # just above a tie: float() drops the 2^-60 and lands ON the tie, which then goes to even (down): two roundings are wrong
    fr = one + h + Fraction(1, 2 ** 60)
    assert np.float32(float(fr)) == f32(1.0)
    assert S.round_once(fr, np.float32) == f32(1.0 + 2.0 ** -23)
    assert S.round_once(-fr, np.float32) == f32(-(1.0 + 2.0 ** -23))
    # just below a tie whose even neighbour is above
    fr = one + 3 * h - Fraction(1, 2 ** 60)
    assert np.float32(float(fr)) == f32(1.0 + 2.0 ** -22)
    assert S.round_once(fr, np.float32) == f32(1.0 + 2.0 ** -23)
    # exact ties go to even, both ways
    assert S.round_once(one + h, np.float32) == f32(1.0)
    assert S.round_once(one + 3 * h, np.float32) == f32(1.0 + 2.0 ** -22)
    # representable numbers and fp64
    assert S.round_once(Fraction(3, 8), np.float32) == f32(0.375) and S.round_once(Fraction(1, 3), np.float64) == 1.0 / 3.0
    assert S.round_once(Fraction(1, 3), np.float32) == f32(1.0 / 3.0)
    assert S.round_once(fr, np.float32).dtype == np.float32 and S.round_once(fr, np.float64).dtype == np.float64


def test_fma_exact_is_one_rounding_where_the_float64_product_is_two():
    # fp32: w - mult u = 2^-60 + (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 + 2^-60, just above a tie
    w, mult, u = np.float32(2.0 ** -60), np.float32(-(1.0 + 2.0 ** -12)), np.float32(1.0 + 2.0 ** -12)
    naive = np.float32(np.float64(w) - np.float64(mult) * np.float64(u))
    want = np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert naive == np.float32(1.0 + 2.0 ** -11) and S.fma_exact(w, mult, u, np.float32) == want
    assert S.fma_many(np.array([w]), mult, np.array([u]), np.float32)[0] == want
    # fp64: the product (1 + 2^-30)^2 = 1 + 2^-29 + 2^-60 is rounded on its own by w - mult * u
    w, mult, u = np.float64(-1.0), np.float64(-(1.0 + 2.0 ** -30)), np.float64(1.0 + 2.0 ** -30)
    assert w - mult * u == 2.0 ** -29 and S.fma_exact(w, mult, u, np.float64) == 2.0 ** -29 + 2.0 ** -60
    assert S.fma_many(np.array([w]), mult, np.array([u]), np.float64)[0] == 2.0 ** -29 + 2.0 ** -60
    # exact cancellation is +0
    z = S.fma_many(np.array([6.0]), np.float64(2.0), np.array([3.0]), np.float64)
    assert z[0] == 0.0 and not np.signbit(z[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_fma_many_equals_fma_exact_on_random_and_cancelling_data(dtype):
    rng = np.random.default_rng(5)
    n = 3000
    u = rng.uniform(-2, 2, n).astype(dtype)
    mult = dtype(rng.uniform(-2, 2))
    w = (mult.astype(np.float64) * u.astype(np.float64) * (1 + rng.choice([0.0, 1e-7, 1e-15, 1.0, -3.0], n))).astype(dtype)
    got = S.fma_many(w, mult, u, dtype)
    want = np.array([S.fma_exact(a, mult, b, dtype) for a, b in zip(w, u)], dtype)
    assert np.array_equal(U.bits(got), U.bits(want))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", S.SMALL)
def test_fast_route_equals_rational_arithmetic_on_whole_families(name, dtype):
    f = S.family(name)
    want = S.host_sweeps(f.rowptr, f.colind, f.values, 3, dtype, all_iterates=True, fma="fraction")
    got = f.iterates(dtype)
    for s in (1, 2, 3):
        assert np.array_equal(U.bits(got[s]), U.bits(want[s])), s
    assert np.array_equal(U.bits(f.exact(dtype)), U.bits(S.host_ilu0_fma(f.rowptr, f.colind, f.values, dtype, fma="fraction")))


def test_host_ilu0_fma_recovers_an_exact_family_and_differs_from_the_float64_product_loop():
    f = S.family("levels-6m+0")
    a, want = U.exact_system(f.rowptr, f.colind, seed=4)
    for dtype in DTYPES:
        assert U.exact_violations(S.host_ilu0_fma(f.rowptr, f.colind, a, dtype), want, f.rowptr, f.colind) == []
    lap = S.family("laplacian12x12x12")      # in fp64 the loop that rounds the product on its own differs on random data
    assert S.differing(lap.exact(np.float64), U.host_ilu0(lap.rowptr, lap.colind, lap.values, np.float64)) > 0


# ---- the recurrence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", S.FAMILY_NAMES)
def test_generators_iterates_differ_and_rows_of_level_up_to_s_are_final(name, dtype):
    f = S.family(name)
    U.check_pattern(f.rowptr, f.colind)
    its = f.iterates(dtype)                 # asserts that the iterates 1 .. 4 differ pairwise in at least 5 % of the entries
    assert len(its) == 6 and all(x.dtype == np.dtype(dtype) for x in its)
    assert np.array_equal(U.bits(its[0]), U.bits(f.values.astype(dtype)))
    exact = f.exact(dtype)
    for s in range(1, 6):
        assert U.exact_violations(its[s], exact, f.rowptr, f.colind, rows_mask=f.levels <= s) == [], s


def test_families_cover_every_lane_count_both_paths_and_every_lower_count():
    seen = {}
    for f in S.families():
        seen.setdefault(f.name.split("-")[0], set()).add(f.lanes)
        if f.name.startswith("shapes"):
            cap = U.lds_cap(f.lanes)
            lens = np.diff(f.rowptr)
            lows = U.diag_positions(f.rowptr, f.colind) - f.rowptr[:-1]
            assert {cap, cap + 1} <= set(lens.tolist()) and lens.max() == cap + 1
            assert {0, 1, f.lanes - 1, f.lanes, f.lanes + 1} <= set(lows.tolist())
            assert lows[lens > cap].max() >= 2 * f.lanes
        if f.name.startswith("laplacian"):
            assert np.diff(f.rowptr).max() == 7 <= U.lds_cap(f.lanes)        # fast path only
        if f.name.startswith("levels"):
            assert np.bincount(f.levels).tolist() == S.LEVEL_WIDTHS
        assert f.m <= 600 or f.name == "laplacian12x12x12"
    assert seen["levels"] == {4, 8, 16, 64} and seen["shapes"] == {4, 8, 16, 64}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["laplacian6x5x4", "levels-6m+0", "levels-24m+1", "shapes-6m+0"])
def test_host_sweeps_at_levels_minus_one_is_the_exact_factor(name, dtype):
    f = S.family(name)
    its = S.host_sweeps(f.rowptr, f.colind, f.values, f.n_levels, dtype, all_iterates=True)
    exact = f.exact(dtype)
    assert np.array_equal(U.bits(its[f.n_levels - 1]), U.bits(exact))
    assert np.array_equal(U.bits(its[f.n_levels]), U.bits(exact))


def test_an_unsymmetric_random_pattern_tests_nothing():
    """Why the families are structurally symmetric or drawn next to the diagonal: updates need structural matches."""
    rp, ci = U.random_pattern(300, 6, seed=3)
    v = U.dominant_values(rp, ci, seed=4)
    its = S.host_sweeps(rp, ci, v, 4, np.float64, all_iterates=True)
    assert S.differing(its[3], its[4]) < S.MIN_DIFFERENT


@pytest.mark.parametrize("name", S.FAMILY_NAMES)
def test_mutations_of_the_recurrence_change_bits_on_every_family(name):
    f = S.family(name)
    dtype = np.float32
    its = f.iterates(dtype)
    gs = S.host_sweeps(f.rowptr, f.colind, f.values, 2, dtype, mutate="gauss_seidel")
    assert S.differing(gs, its[2]) > 0.01
    fp = S.host_sweeps(f.rowptr, f.colind, f.values, 2, dtype, mutate="from_prev")
    assert S.differing(fp, its[2]) > 0.01
    _, steps = S.steps_of(f.rowptr, f.colind)
    rng = np.random.default_rng(len(name))
    cands = [(i, q) for i, row in enumerate(steps) for q, st in enumerate(row) if st[1].size]
    i, q = cands[int(rng.integers(len(cands)))]
    dropped = S.host_sweeps(f.rowptr, f.colind, f.values, 1, dtype, mutate=("drop", i, q, int(rng.integers(1000))))
    diff = U.bits(dropped) != U.bits(its[1])
    assert diff.any() and not diff[:f.rowptr[i]].any() and not diff[f.rowptr[i + 1]:].any()     # one row, nothing else


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spblas_gfx950.h")).read(), flags=re.S)
    assert re.search(rf"\b{NAME}\s*\(", text)
    _build.build()
    dll = ctypes.CDLL(_capi.library_path())
    proto = {n: a for n, _, a in _capi.PROTOTYPES}
    assert NAME in proto and hasattr(dll, NAME) and len(proto[NAME]) == 11
    decl = re.search(rf"{NAME}\s*\((.*?)\);", text, flags=re.S).group(1)
    assert len(decl.split(",")) == 11
    assert "device_ilu0_sweeps" in _build.EXAMPLES
    assert hasattr(sp, "ilu0_sweeps")
    for header in (os.path.join(VENDOR, "ilu0_impl.hpp"), os.path.join("include", "spblas_gfx950", "spblas.hpp")):
        assert "ilu0_sweeps" in open(os.path.join(ROOT, header)).read()
    src = open(os.path.join(ROOT, "spblas-reference_amd", "csrc", "ilu0.hip")).read()
    assert "ilu0_sweep_kernel" in src and NAME in src


def test_first_checks_come_in_the_documented_order():
    lib = getattr(_capi.lib(), NAME)
    N = None
    call = lambda vt, sweeps=1: lib(N, N, 1, 1, sweeps, N, N, N, N, N, vt)
    for vt in (_capi.C32, _capi.C64, _capi.F16, _capi.BF16):    # before any other check: a null handle, null pointers
        assert call(vt) == _capi.NOT_SUPPORTED
        assert call(vt, 0) == _capi.NOT_SUPPORTED
    for vt in (_capi.F32, _capi.F64, 17):                       # the handle comes before pointers, value type and sweeps
        assert call(vt) == _capi.INVALID_HANDLE
        assert call(vt, 0) == _capi.INVALID_HANDLE


# ---- Python argument errors (CPU tensors: raised before anything touches a device) -----------------------------------------
def _cpu_matrix(dtype=torch.float32, m=4, itype=torch.int32):
    return sp.csr_view(torch.ones(m, dtype=dtype), torch.arange(m + 1, dtype=itype), torch.arange(m, dtype=itype), (m, m), m)


def test_python_surface_and_argument_errors():
    a = _cpu_matrix()
    lu = lambda v: sp.csr_view(v, a.rowptr(), a.colind(), (4, 4), 4)
    good, work = lu(torch.zeros(4)), torch.zeros(4)
    for wrapped in (sp.scaled(2.0, a), sp.conjugated(a), sp.transposed(a),
                    sp.csc_view(a.values(), a.rowptr(), a.colind(), (4, 4), 4)):
        with pytest.raises(TypeError):
            sp.ilu0_sweeps(wrapped, good, work, 2)
    for dtype in (torch.complex64, torch.complex128, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match=str(dtype).replace("torch.", "")):
            sp.ilu0_sweeps(_cpu_matrix(dtype), _cpu_matrix(dtype), torch.zeros(4, dtype=dtype), 2)
    with pytest.raises(TypeError, match="int32"):
        sp.ilu0_sweeps(_cpu_matrix(itype=torch.int64), good, work, 2)
    with pytest.raises(ValueError):    # not square
        sp.ilu0_sweeps(sp.csr_view(a.values(), a.rowptr(), a.colind(), (4, 5), 4), good, work, 2)
    with pytest.raises(ValueError):    # lu too short
        sp.ilu0_sweeps(a, lu(torch.ones(3)), work, 2)
    with pytest.raises(ValueError):    # another value type
        sp.ilu0_sweeps(a, lu(torch.ones(4, dtype=torch.float64)), work, 2)
    with pytest.raises(ValueError):    # not A's structure arrays
        sp.ilu0_sweeps(a, sp.csr_view(torch.ones(4), a.rowptr().clone(), a.colind(), (4, 4), 4), work, 2)
    with pytest.raises(TypeError):
        sp.ilu0_sweeps(a, torch.ones(4), work, 2)
    with pytest.raises(ValueError, match="own"):      # lu shares A's values: no in-place form
        sp.ilu0_sweeps(a, a, work, 2)
    with pytest.raises(ValueError, match="own"):
        sp.ilu0_sweeps(a, lu(a.values()), work, 1)
    for bad in (a.values(), good.values()):           # work is A's values, or lu's
        with pytest.raises(ValueError, match="work"):
            sp.ilu0_sweeps(a, good, bad, 2)
    with pytest.raises(ValueError, match="work"):     # None needs sweeps <= 1
        sp.ilu0_sweeps(a, good, None, 2)
    with pytest.raises(ValueError, match="work"):     # too short, another type, not contiguous
        sp.ilu0_sweeps(a, good, torch.zeros(3), 2)
    with pytest.raises(ValueError, match="work"):
        sp.ilu0_sweeps(a, good, torch.zeros(4, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="work"):
        sp.ilu0_sweeps(a, good, torch.zeros(8)[::2], 2)
    with pytest.raises(TypeError, match="work"):
        sp.ilu0_sweeps(a, good, [0.0] * 4, 2)
    for bad in (2.0, "2", None, True):
        with pytest.raises(TypeError, match="sweeps"):
            sp.ilu0_sweeps(a, good, work, bad)
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match="sweeps"):
            sp.ilu0_sweeps(a, good, work, bad)
    with pytest.raises(TypeError):                    # wrong argument count
        sp.ilu0_sweeps(a, good, work)
    with pytest.raises(RuntimeError, match="device"):   # well-formed CPU operands: there is no CPU fallback
        sp.ilu0_sweeps(a, good, work, 2)
    with pytest.raises(RuntimeError, match="device"):
        sp.ilu0_sweeps(sp.operation_info_t(), a, good, None, 1)


# ---- the drop-in header, compiled inside the reference tree ---------------------------------------------------------------
def _compile(tmp_path, extra):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    from oracle.reference_build import compile_flags, patched_reference_headers
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    return subprocess.run([gxx, "-fsyntax-only"] + extra + compile_flags(scratch) + [CHECK], capture_output=True, text=True)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
def test_dropin_ilu0_sweeps_compiles_inside_the_reference_tree(tmp_path):
    r = _compile(tmp_path, [])
    assert r.returncode == 0, "ilu0_sweeps does not compile inside the reference tree:\n" + r.stderr[-6000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
@pytest.mark.parametrize("case", ["SPBLAS_ILU0_SWEEPS_COMPLEX", "SPBLAS_ILU0_SWEEPS_CSC"])
def test_dropin_ilu0_sweeps_out_of_scope_operands_are_no_matching_function(tmp_path, case):
    r = _compile(tmp_path, ["-D" + case])
    assert r.returncode != 0
    assert "no matching function" in r.stderr
    errors = [ln for ln in r.stderr.splitlines() if " error: " in ln or ln.startswith("error:")]
    inside = [ln for ln in errors if VENDOR in ln]
    assert errors and not inside, "errors inside the backend headers:\n" + "\n".join(inside)


def test_standalone_layer_and_example_build_with_gxx():
    """include/spblas_gfx950/spblas.hpp with spblas::gfx950::ilu0_sweeps, through examples/device_ilu0_sweeps.cpp."""
    out = _build.build_examples()
    assert any(p.endswith("device_ilu0_sweeps") and os.path.exists(p) for p in out)
