"""CPU tests of triangular_solve_sweeps (no GPU): the generators of tests/sweeps_util.py hold what they claim -- the dyadic
systems give IDENTICAL iterates in float64 and in float32 under two summation orders (so a different order is no excuse on
the device), the dominant systems keep a permuted float32 restatement within 2 tol S_r of the float64 one --, the host
recurrence at s = levels - 1 is scipy's exact triangular solve, the C ABI declares, exports and binds the new entry point and
orders its first checks as documented, the Python layer raises its argument errors on CPU tensors, and the C++ overloads compile
inside the reference tree and in the standalone layer."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla
import torch

import ladder_tt as TT
import spblas_reference_amd as sp
import sweeps_util as SU
from oracle.reference_build import REF
from spblas_reference_amd import _build, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "compile_check", "dropin_sweeps_check.cpp")
VENDOR = os.path.join("include", "spblas", "vendor", "gfx950")
LANES = (4, 8, 16, 64)


def _dyadic_cases():
    out = []
    for k, lanes in enumerate(LANES):
        for upper in (False, True):
            for unit in (False, True):
                alpha = SU.ALPHAS[(k + upper + 2 * unit) % 3]
                out.append((f"dyadic_l{lanes}_{'u' if upper else 'l'}_{'unit' if unit else 'expl'}",
                            lambda lanes=lanes, upper=upper, unit=unit, alpha=alpha: SU.cached(
                                ("dyadic", lanes, upper, unit),
                                lambda: SU.dyadic_system(600, lanes, upper, unit, alpha, seed=lanes + 2 * upper + unit))))
                out.append((f"shapes_l{lanes}_{'u' if upper else 'l'}_{'unit' if unit else 'expl'}",
                            lambda lanes=lanes, upper=upper, unit=unit: SU.shape_sweep_system(lanes, upper, unit)))
    return out


DYADIC = _dyadic_cases()


def _strict_mask(y):
    rows = np.repeat(np.arange(y.m), np.diff(y.rowptr))
    return rows, (y.colind > rows) if y.uplo == "upper" else (y.colind < rows)


@pytest.mark.parametrize("name,make", DYADIC, ids=[n for n, _ in DYADIC])
def test_dyadic_systems_hold_their_claims_and_are_exact_in_any_order(name, make):
    y = make()
    rows, strict = _strict_mask(y)
    assert set(np.unique(y.values[strict])) <= {-1.0, 1.0}
    assert np.isnan(y.values[~strict & (y.colind != rows)]).all(), "the other triangle holds NaN"
    per_row = np.bincount(rows[strict], minlength=y.m)
    if name.startswith("dyadic"):
        assert per_row.max() <= 4 and per_row.min() == 0
        assert y.levels.max() + 1 >= 8, "deep enough for an active set that shrinks"
    else:
        G = y.lanes
        assert set(range(0, 2 * G + 3)) <= set(per_row.tolist()), "every strict count 0 ... 2 G + 2"
        # the diagonal read sits in every lane slot: first, G - 1, G, 2 G - 1, 2 G
        if y.diag == "explicit":
            dpos = np.flatnonzero(y.colind == rows)
            last = {}
            for p in dpos:
                last[int(rows[p])] = int(p - y.rowptr[rows[p]])
            assert {0, G - 1, G, 2 * G - 1, 2 * G} <= set(last.values())
    d = np.zeros(y.m)
    dp = np.flatnonzero(y.colind == rows)
    d[rows[dp]] = y.values[dp]
    if y.diag == "explicit":
        assert set(np.unique(d)) <= {-2.0, -1.0, 1.0, 2.0}
    else:
        assert np.isnan(y.values[dp]).all(), "stored diagonals of a unit system hold NaN"
    assert np.array_equal(y.b, np.round(y.b)) and np.abs(y.b).max() <= 4 and y.alpha in SU.ALPHAS
    assert TT.lanes_of(y.nnz, y.m) == y.lanes and 590 <= y.m <= 700
    its64, _ = SU.reference(y, 4, np.float64, all_iterates=True)
    for perm_seed in (None, 11):
        its32, _ = SU.reference(y, 4, np.float32, all_iterates=True, perm_seed=perm_seed)
        its64p, _ = SU.reference(y, 4, np.float64, all_iterates=True, perm_seed=perm_seed)
        for k in range(5):
            assert np.isfinite(its64[k]).all()
            assert np.array_equal(its64[k], its32[k].astype(np.float64)), (name, k, perm_seed)
            assert np.array_equal(its64[k], its64p[k]), (name, k, perm_seed)
    assert np.abs(its64[4]).max() < 2 ** 12


def test_lane_classes_cover_every_step_of_the_plan_rule():
    assert sorted({make().lanes for _, make in DYADIC}) == list(LANES)
    assert [s[0] for s in TT.trsv_limits()["lane_steps"]] == [6, 24, 96]
    # the rule is written once under csrc/ -- lanes_per_row, defined in sptrsv.hip (where TT.trsv_limits reads it) and declared
    # in the shared header --, and the plans and the plan-free sweeps all call it
    rule = "avg > 96 ? 64 : (avg > 24 ? 16 : (avg > 6 ? 8 : 4))"
    srcs = {f: open(os.path.join(TT.CSRC, f)).read() for f in sorted(os.listdir(TT.CSRC)) if f.endswith((".hip", ".hpp"))}
    assert {f: s.count("avg > 96") for f, s in srcs.items() if "avg > 96" in s} == {"sptrsv.hip": 1}
    assert srcs["sptrsv.hip"].count(rule) == 1 and "int lanes_per_row(int64_t m, int64_t nnz);" in srcs["csr_inspect.hpp"]
    assert "pl->lanes = lanes_per_row(m, nnz);" in srcs["sptrsv.hip"]
    for f in ("sptrsv_sweeps.hip", "multicolor.hip", "gauss_seidel.hip"):
        assert "lanes_per_row(" in srcs[f] and "avg > 96" not in srcs[f], f


def _dominant(kind):
    return SU.cached(("dominant", kind), lambda: {
        "lower": lambda: SU.dominant_system(3000, 2, seed=31, alpha=1.0),
        "upper_unit": lambda: SU.dominant_system(1500, 5, upper=True, unit=True, seed=32, alpha=-2.0),
        "wide": lambda: SU.dominant_system(700, 30, seed=33, alpha=0.5),
    }[kind]())


@pytest.mark.parametrize("kind", ["lower", "upper_unit", "wide"])
def test_dominant_systems_contract_and_the_reference_stays_inside_its_own_bound(kind):
    y = _dominant(kind)
    rows, strict = _strict_mask(y)
    absrow = np.bincount(rows[strict], weights=np.abs(y.values[strict]), minlength=y.m)
    assert np.abs(y.values[strict]).max() < 1.0
    if y.diag == "explicit":
        d = np.zeros(y.m)
        dp = np.flatnonzero(y.colind == rows)
        d[rows[dp]] = y.values[dp]
        assert (np.abs(d) >= 2 * absrow + 0.5).all()
    else:
        assert (absrow <= 0.25 + 1e-15).all()
    if kind == "lower":
        assert 12 <= y.levels.max() + 1 <= 40, y.levels.max() + 1
    for s in (0, 1, 3, 8):
        ref, S = SU.reference(y, s, np.float64)
        assert np.isfinite(ref).all() and np.isfinite(S).all() and (S > 0).any()
        x32, _ = SU.reference(y, s, np.float32, perm_seed=7)
        assert SU.bound_violations(x32, ref, S, np.float32, f"{kind} s={s}") == []
        x64p, _ = SU.reference(y, s, np.float64, perm_seed=7)
        assert SU.bound_violations(x64p, ref, S, np.float64, f"{kind} s={s}") == []
    # the checker bites: one row off by three bounds
    ref, S = SU.reference(y, 3, np.float64)
    off = ref.copy()
    off[y.m // 2] += 6e-6 * S[y.m // 2]
    assert SU.bound_violations(off, ref, S, np.float32) != []
    assert SU.bit_violations(off.astype(np.float32), ref.astype(np.float32)) != []


def _triangle(y):
    """alpha (N + D) or alpha N + I as a scipy matrix, from the masked entries."""
    rows, strict = _strict_mask(y)
    T = sps.csr_matrix((y.alpha * y.values[strict], (rows[strict], y.colind[strict])), shape=(y.m, y.m))
    if y.diag == "unit":
        return (T + sps.identity(y.m)).tocsr()
    d = np.zeros(y.m)
    dp = np.flatnonzero(y.colind == rows)
    d[rows[dp]] = y.values[dp]
    return (T + sps.diags(y.alpha * d)).tocsr()


@pytest.mark.parametrize("name,make", DYADIC, ids=[n for n, _ in DYADIC])
def test_host_recurrence_reaches_the_exact_solve_at_levels_minus_one(name, make):
    y = make()
    levels = int(y.levels.max()) + 1
    want = spla.spsolve_triangular(_triangle(y), y.b, lower=y.uplo == "lower")
    got, _ = SU.reference(y, levels - 1, np.float64)
    assert SU.bit_violations(got, want, name) == []
    more, _ = SU.reference(y, levels + 3, np.float64)
    assert SU.bit_violations(more, want, name) == []


@pytest.mark.parametrize("upper", [False, True])
def test_chain_closed_form(upper):
    y = SU.chain_system(70, upper)
    assert y.levels.max() == 69 and np.bincount(y.levels).max() == 1
    for s in (0, 1, 2, 35, 68, 69, 70):
        got, _ = SU.reference(y, s, np.float32)
        assert np.array_equal(got, SU.chain_closed_form(70, s, upper).astype(np.float32))


def test_host_recurrence_details():
    # the last stored diagonal wins, no stored diagonal divides by zero, columns outside [0, m) are ignored, Jacobi not Gauss-Seidel
    rowptr = np.array([0, 2, 5, 7])
    colind = np.array([0, 0, 0, 1, 7, 0, 1])
    values = np.array([9.0, 2.0, 1.0, 4.0, np.nan, 1.0, 1.0])
    b = np.array([2.0, 4.0, 1.0])
    its, S = SU.host_sweeps(rowptr, colind, values, b, 2, "lower", "explicit", 1.0, np.float64, all_iterates=True)
    assert its[0][0] == 1.0 and its[0][1] == 1.0 and np.isinf(its[0][2])
    assert its[1][1] == (4.0 - 1.0) / 4.0 and not np.isfinite(its[1][2])
    assert its[2][1] == its[1][1]
    u, _ = SU.host_sweeps(rowptr, colind, values, b, 1, "lower", "unit", 1.0, np.float64)
    assert u.tolist() == [2.0, 4.0 - 2.0, 1.0 - (2.0 + 4.0)]
    assert S[0] == 1.0 and S[1] == (4.0 + 1.0) / 4.0


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spblas_gfx950.h")).read(), flags=re.S)
    name = "spblas_gfx950_sptrsv_sweeps"
    assert re.search(rf"\b{name}\s*\(", text)
    _build.build()
    dll = ctypes.CDLL(_capi.library_path())
    proto = {n: a for n, _, a in _capi.PROTOTYPES}
    assert name in proto and hasattr(dll, name) and len(proto[name]) == 15
    decl = re.search(rf"{name}\s*\((.*?)\);", text, flags=re.S).group(1)
    assert len(decl.split(",")) == 15
    assert "sptrsv_sweeps.hip" in _build.SOURCES and "device_sptrsv_sweeps" in _build.EXAMPLES
    for n in ("triangular_solve_sweeps",):
        assert hasattr(sp, n)
        assert n in open(os.path.join(ROOT, VENDOR, "triangular_solve_impl.hpp")).read()
        assert n in open(os.path.join(ROOT, "include", "spblas_gfx950", "spblas.hpp")).read()


def test_first_checks_come_in_the_documented_order():
    lib = _capi.lib()
    N = None
    call = lambda vt, sweeps=1: lib.spblas_gfx950_sptrsv_sweeps(N, N, 1, 1, sweeps, 0, 0, N, N, N, N, N, N, N, vt)
    for vt in (_capi.C32, _capi.C64, _capi.F16, _capi.BF16):    # before any other check: a null handle, null pointers
        assert call(vt) == _capi.NOT_SUPPORTED
        assert call(vt, -1) == _capi.NOT_SUPPORTED
    for vt in (_capi.F32, _capi.F64, 17):
        assert call(vt) == _capi.INVALID_HANDLE


# ---- Python argument errors (CPU tensors: raised before anything touches a device) -----------------------------------------
def _cpu_matrix(dtype=torch.float32, m=4, itype=torch.int32):
    return sp.csr_view(torch.ones(m, dtype=dtype), torch.arange(m + 1, dtype=itype), torch.arange(m, dtype=itype), (m, m), m)


def test_python_surface_and_argument_errors():
    a = _cpu_matrix()
    b, x = torch.ones(4), torch.zeros(4)
    lo, ex = sp.lower_triangle, sp.explicit_diagonal
    for dtype in (torch.complex64, torch.complex128, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError):
            sp.triangular_solve_sweeps(_cpu_matrix(dtype), lo, ex, b.to(dtype), x.to(dtype), 2)
    with pytest.raises(NotImplementedError):      # a block of right-hand sides
        sp.triangular_solve_sweeps(a, lo, ex, torch.ones(4, 2), torch.zeros(4, 2), 2)
    with pytest.raises(NotImplementedError):
        sp.triangular_solve_sweeps(a, lo, ex, sp.scaled(2.0, torch.ones(4, 2)), torch.zeros(4, 2), 2)
    with pytest.raises(NotImplementedError):      # csc_view / transposed
        sp.triangular_solve_sweeps(sp.csc_view(a.values(), a.rowptr(), a.colind(), (4, 4), 4), lo, ex, b, x, 2)
    with pytest.raises(NotImplementedError):
        sp.triangular_solve_sweeps(sp.transposed(a), lo, ex, b, x, 2)
    with pytest.raises(TypeError):                # uplo / diag are tag objects
        sp.triangular_solve_sweeps(a, "lower", ex, b, x, 2)
    with pytest.raises(TypeError):
        sp.triangular_solve_sweeps(a, lo, 0, b, x, 2)
    with pytest.raises(TypeError, match="int32"):
        sp.triangular_solve_sweeps(_cpu_matrix(itype=torch.int64), lo, ex, b, x, 2)
    with pytest.raises(ValueError):               # lengths
        sp.triangular_solve_sweeps(a, lo, ex, torch.ones(5), x, 2)
    with pytest.raises(TypeError):                # value types of b / x
        sp.triangular_solve_sweeps(a, lo, ex, b.double(), x, 2)
    with pytest.raises(RuntimeError):
        sp.triangular_solve_sweeps(sp.conjugated(a), lo, ex, b, x, 2)
    for bad in (2.0, "2", None, True):
        with pytest.raises(TypeError, match="sweeps"):
            sp.triangular_solve_sweeps(a, lo, ex, b, x, bad)
    with pytest.raises(ValueError, match="sweeps"):
        sp.triangular_solve_sweeps(a, lo, ex, b, x, -1)
    with pytest.raises(TypeError):                # wrong argument count
        sp.triangular_solve_sweeps(a, lo, ex, b, x)
    with pytest.raises(RuntimeError, match="device"):   # well-formed CPU operands: there is no CPU fallback
        sp.triangular_solve_sweeps(a, lo, ex, b, x, 2)


# ---- the drop-in header, compiled inside the reference tree ---------------------------------------------------------------
def _compile(tmp_path, extra):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    from oracle.reference_build import compile_flags, patched_reference_headers
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    return subprocess.run([gxx, "-fsyntax-only"] + extra + compile_flags(scratch) + [CHECK], capture_output=True, text=True)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
def test_dropin_sweeps_compile_inside_the_reference_tree(tmp_path):
    r = _compile(tmp_path, [])
    assert r.returncode == 0, "triangular_solve_sweeps does not compile inside the reference tree:\n" + r.stderr[-6000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
@pytest.mark.parametrize("case", ["SPBLAS_SWEEPS_COMPLEX", "SPBLAS_SWEEPS_CSC"])
def test_dropin_sweeps_out_of_scope_operands_are_no_matching_function(tmp_path, case):
    r = _compile(tmp_path, ["-D" + case])
    assert r.returncode != 0
    assert "no matching function" in r.stderr
    errors = [ln for ln in r.stderr.splitlines() if " error: " in ln or ln.startswith("error:")]
    inside = [ln for ln in errors if VENDOR in ln]
    assert errors and not inside, "errors inside the backend headers:\n" + "\n".join(inside)


def test_standalone_layer_and_example_build_with_gxx():
    """include/spblas_gfx950/spblas.hpp with spblas::gfx950::triangular_solve_sweeps, through examples/device_sptrsv_sweeps.cpp."""
    out = _build.build_examples()
    assert any(p.endswith("device_sptrsv_sweeps") and os.path.exists(p) for p in out)
