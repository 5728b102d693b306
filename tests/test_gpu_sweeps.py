"""-m gpu: triangular_solve_sweeps (csrc/sptrsv_sweeps.hip) against the host recurrence of tests/sweeps_util.py.

Dyadic systems must match host_sweeps BIT FOR BIT at every sweep count (tests/test_sweeps_cpu.py proves that no summation
order changes a bit of them), the integer systems of tests/ladder_tt.py must reach x_true at s = levels - 1, the chain must
follow its closed form for every s, plan and plan-free calls must give equal bits, dominant random systems must stay within
2 tol S_r of the float64 recurrence on EVERY row, poisoned and shifted buffers must not matter, every refusal must come in the
documented order, the first call on a fresh handle must be recordable in a graph, and the ILU(0) factors must pair with it."""
import ctypes
import gc
import os
import re
import subprocess
import threading

import numpy as np
import pytest
import torch

import gpu_util as G
import ilu_util as IU
import ladder_tt as TT
import spblas_reference_amd as sp
import sweeps_util as SU
from spblas_reference_amd import _capi, api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
LANES = (4, 8, 16, 64)
VT = {np.dtype(np.float32): _capi.F32, np.dtype(np.float64): _capi.F64}


class Dev:
    """A SweepSystem on the device."""

    def __init__(self, y, dtype):
        self.y, self.dtype = y, np.dtype(dtype)
        self.base = G.csr_on_device(np.asarray(y.values).astype(dtype), y.rowptr, y.colind, (y.m, y.m), y.nnz)
        self.a = self.base if y.alpha == 1.0 else sp.scaled(y.alpha, self.base)
        self.b = G.dev(np.asarray(y.b).astype(dtype))
        self.uplo = sp.upper_triangle if y.uplo == "upper" else sp.lower_triangle
        self.diag = sp.implicit_unit_diagonal if y.diag == "unit" else sp.explicit_diagonal
        self._info = None

    def info(self):
        if self._info is None:
            self._info = sp.triangular_solve_inspect(self.a, self.uplo, self.diag, self.b, torch.empty_like(self.b))
        return self._info

    def levels(self):
        return self.info().state_.info()["levels"]

    def sweeps(self, s, plan=False, x=None):
        x = torch.full_like(self.b, float("nan")) if x is None else x
        if plan:
            sp.triangular_solve_sweeps(self.info(), self.a, self.uplo, self.diag, self.b, x, s)
        else:
            sp.triangular_solve_sweeps(self.a, self.uplo, self.diag, self.b, x, s)
        return G.host(x)


def _iterates(key, y, s_max):
    """x0 ... x(s_max) of a dyadic system in float64 (exact: the same numbers in float32), computed once per system."""
    return SU.cached(("iterates", key, s_max), lambda: SU.reference(y, s_max, np.float64, all_iterates=True)[0])


# ---- 1. dyadic systems, bit for bit ------------------------------------------------------------------------------------------
def _dyadic(kind, lanes, upper, unit):
    if kind == "shapes":
        return SU.shape_sweep_system(lanes, upper, unit)
    alpha = SU.ALPHAS[(LANES.index(lanes) + upper + 2 * unit) % 3]
    return SU.cached(("dyadic", lanes, upper, unit),
                     lambda: SU.dyadic_system(600, lanes, upper, unit, alpha, seed=lanes + 2 * upper + unit))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("kind", ["dyadic", "shapes"])
def test_dyadic_systems_match_the_host_recurrence_bit_for_bit(gpu, kind, lanes, upper, unit, dtype):
    y = _dyadic(kind, lanes, upper, unit)
    d = Dev(y, dtype)
    assert d.info().state_.info()["lanes_per_row"] == lanes == y.lanes
    want = _iterates((kind, lanes, upper, unit), y, 4)
    bad = []
    for s in range(5):
        for plan in (False, True):
            bad += SU.bit_violations(d.sweeps(s, plan), want[s], f"s={s} plan={plan}")
    assert bad == []


def test_alphas_of_the_dyadic_systems_cover_all_three():
    assert {_dyadic(k, l, u, t).alpha for k in ("dyadic", "shapes") for l in LANES for u in (0, 1) for t in (0, 1)} == \
        set(SU.ALPHAS)


# ---- 2. the fixed point on the integer systems of the level-plan ladders --------------------------------------------------------
def _fixed_point(sysm, dtype):
    y = SU.of_tt(sysm)
    d = Dev(y, dtype)
    levels = d.levels()
    assert levels == int(sysm.level.max()) + 1
    bad = []
    for s in (levels - 1, levels + 3):
        for plan in (False, True):
            bad += [f"s={s} plan={plan}: {v}" for v in TT.exact_violations(d.sweeps(s, plan), sysm)]
    assert bad == []


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("upper,unit", [(False, False), (True, True), (False, True), (True, False)])
@pytest.mark.parametrize("lanes", LANES)
def test_fixed_point_on_the_row_shape_systems(gpu, lanes, upper, unit, dtype):
    _fixed_point(TT.shape_system(lanes, upper, unit), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lanes,grid", [(8, 1), (16, 2), (64, 2)])
def test_fixed_point_on_the_level_width_systems(gpu, lanes, grid, dtype):
    _fixed_point(TT.width_system(lanes, grid)[0], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(TT.SEQUENCES)))
def test_fixed_point_on_the_level_sequences(gpu, i, dtype):
    assert 1 <= len(TT.SEQUENCES[i]) <= 5
    _fixed_point(TT.sequence_system(i), dtype)


# ---- 3. the chain: one row per level ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("upper", [False, True])
def test_chain_follows_its_closed_form_for_every_sweep_count(gpu, upper, dtype):
    y = SU.chain_system(70, upper)
    d = Dev(y, dtype)
    assert d.levels() == 70
    bad = []
    for s in range(71):
        for plan in (False, True):      # with a plan s = 70 is clamped to 69: the same vector
            bad += SU.bit_violations(d.sweeps(s, plan), SU.chain_closed_form(70, s, upper), f"s={s} plan={plan}")
    assert bad == []


# ---- 4. / 5. dominant random systems ---------------------------------------------------------------------------------------------
def _dominant(kind):
    return SU.cached(("dominant", kind), lambda: {
        "lower": lambda: SU.dominant_system(3000, 2, seed=31, alpha=1.0),
        "upper_unit": lambda: SU.dominant_system(1500, 5, upper=True, unit=True, seed=32, alpha=-2.0),
        "wide": lambda: SU.dominant_system(700, 30, seed=33, alpha=0.5),
    }[kind]())


@pytest.mark.parametrize("dtype", DTYPES)
def test_plan_and_plan_free_calls_give_equal_bits(gpu, dtype):
    y = _dominant("lower")
    d = Dev(y, dtype)
    levels = d.levels()
    assert 12 <= levels <= 40 and levels == int(y.levels.max()) + 1
    bad = []
    for s in list(range(7)) + [levels + 2]:
        free, planned = d.sweeps(s, False), d.sweeps(s, True)
        assert np.isfinite(free).all()
        bad += SU.bit_violations(planned, free, f"s={s}")
    assert bad == []
    # levels + 2 sweeps are the solve: they and the exact solve stay within the bound of the recurrence's fixed point
    x = torch.full_like(d.b, float("nan"))
    sp.triangular_solve(d.info(), d.a, d.uplo, d.diag, d.b, x)
    ref, S = SU.reference(y, levels - 1, np.float64)
    assert SU.bound_violations(G.host(x), ref, S, dtype, "exact solve") == []
    assert SU.bound_violations(d.sweeps(levels + 2, True), ref, S, dtype, "levels + 2 sweeps") == []


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["lower", "upper_unit", "wide"])
def test_dominant_systems_stay_within_two_tol_S_of_the_float64_recurrence(gpu, kind, dtype):
    y = _dominant(kind)
    d = Dev(y, dtype)
    bad = []
    for s in (0, 1, 3, 8):
        ref, S = SU.cached(("dominant ref", kind, s), lambda: SU.reference(y, s, np.float64))
        for plan in (False, True):
            got = d.sweeps(s, plan)
            err = np.abs(got.astype(np.float64) - ref) / (SU.TOL[np.dtype(dtype)] * S)
            print(f"{kind} {np.dtype(dtype).name} s={s} plan={plan}: max error {np.nanmax(err):.3f} tol S_r (bound 2)")
            bad += SU.bound_violations(got, ref, S, dtype, f"s={s} plan={plan}")     # every row
    assert bad == []


# ---- 6. poison, over-long buffers, shifted base pointers (C ABI: the caller owns the work vector) ---------------------------------
def _abi(hd, plan, y, d, s, b, x, work, vt=None, m=None, nnz=None, uplo=None, diag=None, alpha=True, rowptr=True):
    ct = ctypes.c_float if d.dtype == np.float32 else ctypes.c_double
    al = ct(y.alpha)
    ptr = lambda t: ctypes.c_void_p(t if isinstance(t, int) else (t.data_ptr() if t is not None else 0))
    return _capi.lib().spblas_gfx950_sptrsv_sweeps(
        hd.h if hd is not None else None, plan, y.m if m is None else m, y.nnz if nnz is None else nnz, s,
        (_capi.UPPER if y.uplo == "upper" else _capi.LOWER) if uplo is None else uplo,
        (_capi.DIAG_UNIT if y.diag == "unit" else _capi.DIAG_EXPLICIT) if diag is None else diag,
        ctypes.byref(al) if alpha else None, ptr(d.base.rowptr()) if rowptr else None, ptr(d.base.colind()),
        ptr(d.base.values()), ptr(b), ptr(x), ptr(work), VT[d.dtype] if vt is None else vt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shift", [0, 1, 2])
def test_poisoned_over_long_and_shifted_buffers(gpu, shift, dtype):
    y = _dyadic("dyadic", 8, False, False)
    d = Dev(y, dtype)
    want = _iterates(("dyadic", 8, False, False), y, 4)
    hd = api._Handle.current(torch.device("cuda", 0))
    plan = d.info().state_.plan
    m = y.m
    bad = []
    for s in (0, 1, 2, 3):
        for pl in (None, plan):
            xbuf = torch.full((shift + m + 64,), float("nan"), dtype=d.b.dtype, device="cuda")
            wbuf = torch.full((shift + m + 64,), float("nan"), dtype=d.b.dtype, device="cuda")
            bbuf = torch.full((shift + m + 64,), float("nan"), dtype=d.b.dtype, device="cuda")
            bbuf[shift:shift + m].copy_(d.b)
            esz = xbuf.element_size()
            st = _abi(hd, pl, y, d, s, bbuf.data_ptr() + shift * esz, xbuf.data_ptr() + shift * esz,
                      wbuf.data_ptr() + shift * esz)
            assert st == _capi.SUCCESS
            x, w = G.host(xbuf), G.host(wbuf)
            bad += SU.bit_violations(x[shift:shift + m], want[s], f"s={s} plan={pl is not None}")
            assert np.isnan(x[:shift]).all() and np.isnan(x[shift + m:]).all(), "x written outside its m elements"
            assert np.isnan(w[:shift]).all() and np.isnan(w[shift + m:]).all(), "work written outside its m elements"
            if s == 0:
                assert np.isnan(w).all(), "s = 0 writes x directly: work is not touched"
            elif pl is None:
                bad += SU.bit_violations(w[shift:shift + m], want[s - 1], f"work after s={s}")
    assert bad == []


# ---- 7. every refusal, in the order of the check list ------------------------------------------------------------------------------
def test_refusals_come_in_the_documented_order(gpu):
    y = _dyadic("dyadic", 4, False, False)
    d = Dev(y, np.float32)
    hd = api._Handle.current(torch.device("cuda", 0))
    plan = d.info().state_.plan
    x, w = torch.zeros_like(d.b), torch.zeros_like(d.b)
    C = _capi
    # 1. value types that are not offered: before the handle
    for vt in (C.C32, C.C64, C.F16, C.BF16):
        assert _abi(None, None, y, d, 1, None, None, None, vt=vt, alpha=False, rowptr=False) == C.NOT_SUPPORTED
    # 2. the handle: before the pointers
    assert _abi(None, None, y, d, 1, None, None, None, alpha=False) == C.INVALID_HANDLE
    # 3. pointers: before the sizes
    assert _abi(hd, None, y, d, 1, d.b, x, w, alpha=False, m=-1) == C.INVALID_POINTER
    assert _abi(hd, None, y, d, 1, d.b, x, w, rowptr=False, nnz=-1) == C.INVALID_POINTER
    assert _abi(hd, None, y, d, -1, None, x, w) == C.INVALID_POINTER
    assert _abi(hd, None, y, d, -1, d.b, None, w) == C.INVALID_POINTER
    assert _abi(hd, None, y, d, 1, d.b, x, None) == C.INVALID_POINTER       # work is needed from one sweep on
    assert _abi(hd, None, y, d, -1, d.b, x, None, uplo=9) == C.INVALID_POINTER
    # 4. sizes: before uplo / diag
    for kw in ({"m": -1}, {"nnz": -1}, {"m": 2 ** 31 - 1}, {"nnz": 2 ** 31}):
        assert _abi(hd, None, y, d, 1, d.b, x, w, uplo=9, **kw) == C.INVALID_SIZE, kw
    assert _abi(hd, None, y, d, -1, d.b, x, w, diag=9) == C.INVALID_SIZE
    # 5. uplo / diag: before the plan
    assert _abi(hd, plan, y, d, 1, d.b, x, w, uplo=2, m=y.m + 1) == C.INVALID_VALUE
    assert _abi(hd, plan, y, d, 1, d.b, x, w, diag=-1) == C.INVALID_VALUE
    # 6. the plan: before the aliasing rules
    assert _abi(hd, plan, y, d, 1, d.b, d.b, w, uplo=C.UPPER) == C.PLAN_MISMATCH
    assert _abi(hd, plan, y, d, 1, d.b, x, x, diag=C.DIAG_UNIT) == C.PLAN_MISMATCH
    assert _abi(hd, plan, y, d, 1, d.b, x, w, nnz=y.nnz - 1) == C.PLAN_MISMATCH
    # 7. aliasing, 8. the value type
    assert _abi(hd, plan, y, d, 1, d.b, d.b, w) == C.INVALID_VALUE
    assert _abi(hd, None, y, d, 1, d.b, x, x) == C.INVALID_VALUE
    assert _abi(hd, None, y, d, 1, d.b, x, d.b) == C.INVALID_VALUE
    assert _abi(hd, None, y, d, 0, d.b, d.b, None) == C.INVALID_VALUE
    assert _abi(hd, None, y, d, 1, d.b, x, w, vt=17) == C.INVALID_VALUE
    torch.cuda.synchronize()
    assert not x.any() and not w.any(), "a refused call launched something"
    # m == 0: success, nothing launched; work may be missing
    assert _abi(hd, None, y, d, 3, None, None, None, m=0, nnz=0) == C.SUCCESS
    # sweeps == 0 needs no work vector
    assert _abi(hd, None, y, d, 0, d.b, x, None) == C.SUCCESS
    assert SU.bit_violations(G.host(x), _iterates(("dyadic", 4, False, False), y, 4)[0]) == []


def test_python_layer_on_the_device(gpu):
    y = _dyadic("dyadic", 4, False, False)
    d = Dev(y, np.float32)
    want = _iterates(("dyadic", 4, False, False), y, 4)
    # b sharing storage with x is cloned first
    x = d.b.clone()
    sp.triangular_solve_sweeps(d.a, d.uplo, d.diag, x, x, 3)
    assert SU.bit_violations(G.host(x), want[3]) == []
    # scaled(b): applied to x afterwards
    x = torch.full_like(d.b, float("nan"))
    sp.triangular_solve_sweeps(d.a, d.uplo, d.diag, sp.scaled(-4.0, d.b), x, 2)
    assert SU.bit_violations(G.host(x), -4.0 * want[2]) == []
    # an info made for the other triangle is not used and not replaced: the call never inspects
    other = sp.triangular_solve_inspect(d.a, sp.upper_triangle, d.diag, d.b, torch.empty_like(d.b))
    state = other.state_
    sp.triangular_solve_sweeps(other, d.a, d.uplo, d.diag, d.b, x, 4)
    assert other.state_ is state and SU.bit_violations(G.host(x), want[4]) == []
    empty = sp.operation_info_t()
    sp.triangular_solve_sweeps(empty, d.a, d.uplo, d.diag, d.b, x, 1)
    assert not isinstance(empty.state_, api._TrsvPlan) and SU.bit_violations(G.host(x), want[1]) == []
    # m == 0
    z = torch.zeros(0, device="cuda")
    a0 = sp.csr_view(z, torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), (0, 0), 0)
    sp.triangular_solve_sweeps(a0, d.uplo, d.diag, z, torch.zeros(0, device="cuda"), 3)


# ---- 8. graph capture --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_first_call_on_a_fresh_handle_is_recorded_in_a_graph(gpu, dtype):
    """A new host thread gets a handle of its own; the thread's FIRST sweeps calls (plan-free and with a plan) are recorded, never
    run eagerly.  After b and the values were edited in place the replay gives the recurrence of the new data."""
    y = _dyadic("dyadic", 8, True, False)
    rng = np.random.default_rng(5)
    rows = np.repeat(np.arange(y.m), np.diff(y.rowptr))
    flip = (y.colind > rows) & (rng.random(y.nnz) < 0.5)              # the second data set: other strict values, another b
    v2 = np.where(flip, -y.values, y.values)
    b2 = rng.integers(-4, 5, y.m).astype(np.float64)
    want1 = _iterates(("dyadic", 8, True, False), y, 4)[3]
    want2 = SU.host_sweeps(y.rowptr, y.colind, v2, b2, 3, y.uplo, y.diag, y.alpha, np.float64)[0]
    assert SU.bit_violations(want2.astype(np.float32), SU.host_sweeps(y.rowptr, y.colind, v2, b2, 3, y.uplo, y.diag, y.alpha,
                                                                      np.float32, perm_seed=3)[0]) == []
    out = {}

    def work():
        try:
            mine = api._Handle.current(torch.device("cuda", 0))
            d = Dev(y, dtype)
            info = d.info()
            x1, x2 = torch.full_like(d.b, float("nan")), torch.full_like(d.b, float("nan"))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                sp.triangular_solve_sweeps(d.a, d.uplo, d.diag, d.b, x1, 3)
                sp.triangular_solve_sweeps(info, d.a, d.uplo, d.diag, d.b, x2, 3)
            res = []
            for vals, b, want in ((y.values, y.b, want1), (v2, b2, want2), (y.values, y.b, want1)):
                d.base.values().copy_(G.dev(np.asarray(vals).astype(dtype)))
                d.b.copy_(G.dev(np.asarray(b).astype(dtype)))
                x1.fill_(float("nan"))
                x2.fill_(float("nan"))
                g.replay()
                res += SU.bit_violations(G.host(x1), want, "plan-free") + SU.bit_violations(G.host(x2), want, "plan")
            out["bad"], out["handle"] = res, mine.h.value
        except BaseException as e:   # noqa: BLE001 -- handed to the test's thread
            out["error"] = e

    here = api._Handle.current(torch.device("cuda", 0)).h.value
    t = threading.Thread(target=work)
    t.start()
    t.join()
    if "error" in out:
        raise out["error"]
    assert out["handle"] != here, "the thread did not get a handle of its own"
    assert out["bad"] == []


# ---- 9. ILU(0) pairing --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_ilu0_factors_applied_by_sweeps(gpu, dtype):
    rowptr, colind = IU.laplacian7(12, 12, 12)
    m, nnz = rowptr.size - 1, colind.size
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    vals = np.where(colind == rows, 6.0, -1.0).astype(dtype)
    a = G.csr_on_device(vals, rowptr, colind, (m, m), nnz)
    lu = sp.csr_view(torch.empty_like(a.values()), a.rowptr(), a.colind(), (m, m), nnz)
    sp.ilu0(a, lu)
    b_h = (1.0 + np.arange(m) % 5).astype(dtype)
    b = G.dev(b_h)
    new = lambda: torch.full_like(b, float("nan"))
    lo = (sp.lower_triangle, sp.implicit_unit_diagonal)
    up = (sp.upper_triangle, sp.explicit_diagonal)
    y_e, x_e, y_s, x_s, y_3, x_3 = new(), new(), new(), new(), new(), new()
    lo_info = sp.triangular_solve_inspect(lu, *lo, b, y_e)
    up_info = sp.triangular_solve_inspect(lu, *up, y_e, x_e)
    sp.triangular_solve(lo_info, lu, *lo, b, y_e)
    sp.triangular_solve(up_info, lu, *up, y_e, x_e)
    nl, nu = lo_info.state_.info()["levels"], up_info.state_.info()["levels"]
    assert nl == nu == 3 * 11 + 1
    # levels - 1 sweeps are the solves (plan-free: no clamp helps)
    sp.triangular_solve_sweeps(lu, *lo, b, y_s, nl - 1)
    sp.triangular_solve_sweeps(lu, *up, y_s, x_s, nu - 1)
    tol = SU.TOL[np.dtype(dtype)]
    lu_h = G.host(lu.values()).astype(np.float64)
    L, U = IU.split_lu(rowptr, colind, lu_h)
    ys, xs, ye, xe = (G.host(t).astype(np.float64) for t in (y_s, x_s, y_e, x_e))
    # the project's criterion for a triangular solve: |b - T x| <= tol (|b| + |T| |x|) on every row, for both factors ...
    assert (np.abs(b_h - L @ ys) <= tol * (np.abs(b_h) + abs(L) @ np.abs(ys))).all()
    assert (np.abs(ys - U @ xs) <= tol * (np.abs(ys) + abs(U) @ np.abs(xs))).all()
    # ... and the exact pair's result within the forward tolerance of the solve tests (100 tol, relative)
    assert np.abs(ys - ye).max() <= 100 * tol * np.abs(ye).max()
    assert np.abs(xs - xe).max() <= 100 * tol * np.abs(xe).max()
    # three sweeps each against the recurrence on the device's own factor: 2 tol S_r on every row
    sp.triangular_solve_sweeps(lo_info, lu, *lo, b, y_3, 3)
    sp.triangular_solve_sweeps(up_info, lu, *up, y_3, x_3, 3)
    y3 = G.host(y_3)
    ref, S = SU.host_sweeps(rowptr, colind, lu_h, b_h, 3, "lower", "unit", 1.0, np.float64)
    assert SU.bound_violations(y3, ref, S, dtype, "L by 3 sweeps") == []
    ref, S = SU.host_sweeps(rowptr, colind, lu_h, y3, 3, "upper", "explicit", 1.0, np.float64)
    assert SU.bound_violations(G.host(x_3), ref, S, dtype, "U by 3 sweeps") == []
    # a preconditioner apply: far closer to the exact pair than x = 0 is
    assert np.linalg.norm(G.host(x_3) - xe) < 0.5 * np.linalg.norm(xe)


# ---- 10. the example; memory ---------------------------------------------------------------------------------------------------------
def test_device_sptrsv_sweeps_example_reports_both_residuals(gpu):
    exe = os.path.join(ROOT, "examples", "device_sptrsv_sweeps")
    assert os.path.exists(exe), "examples/device_sptrsv_sweeps is not built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    mt = re.search(r"exact pair ([0-9.e+-]+), 3 sweeps each ([0-9.e+-]+)", r.stdout)
    assert mt, r.stdout
    exact, sweeps = float(mt.group(1)), float(mt.group(2))
    assert exact < 1e-12 and exact < sweeps < 1.0


def test_call_cycles_leave_device_memory_where_it_was(gpu):
    y = _dominant("lower")
    d = Dev(y, np.float32)
    x = torch.zeros_like(d.b)

    def cycle():
        info = sp.triangular_solve_inspect(d.a, d.uplo, d.diag, d.b, x)
        for s in (0, 1, 4):
            sp.triangular_solve_sweeps(info, d.a, d.uplo, d.diag, d.b, x, s)
            sp.triangular_solve_sweeps(d.a, d.uplo, d.diag, d.b, x, s)
        del info

    for _ in range(10):  # warm-up: the pools reach their size
        cycle()
    torch.cuda.synchronize()
    gc.collect()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(200):
        cycle()
    torch.cuda.synchronize()
    gc.collect()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 4 * 2 ** 20, f"free device memory fell by {(free0 - free1) / 2**20:.1f} MiB over 200 cycles"
