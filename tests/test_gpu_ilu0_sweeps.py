"""-m gpu tests of ilu0_sweeps (spblas_gfx950_ilu0_sweeps, csrc/ilu0.hip).  Every test calls ilu0_sweeps and so fails on a backend
without the feature.

Every check is BIT FOR BIT.  The reference is the host recurrence of tests/ilu_sweeps_util.py (one IEEE division per lower entry,
one correctly rounded fma per update; proved on the host by tests/test_ilu0_sweeps_cpu.py), computed once per family and type and
shared; where the statement is about the fixed point the reference is ilu0 on the same device.  In every call lu and work are
longer than nnz and prefilled, and what lies outside their nnz elements must come back untouched."""
import ctypes
import gc
import os
import re
import subprocess
import threading

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import gpu_util as G
import ilu_sweeps_util as S
import ilu_util as U
import spblas_reference_amd as sp
from spblas_reference_amd import _capi, api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
VT = {np.dtype(np.float32): _capi.F32, np.dtype(np.float64): _capi.F64}
PAD = 5


class Dev:
    """A pattern with values on the device.  Every value array is a window at element `offset` of a longer buffer."""

    def __init__(self, rowptr, colind, values, dtype, offset=0):
        self.rowptr, self.colind, self.dtype, self.offset = rowptr, colind, np.dtype(dtype), offset
        self.m, self.nnz = rowptr.size - 1, int(colind.size)
        self.d_rp = G.dev(rowptr.astype(np.int32))
        self.d_ci = G.dev(np.concatenate([colind.astype(np.int32), np.full(PAD, 2 ** 30, np.int32)]))
        self.a_host = np.concatenate([np.full(offset, np.nan), np.asarray(values, np.float64), np.full(PAD, np.nan)]).astype(dtype)
        self.a_buf = G.dev(self.a_host)
        self.a = self.view(self.a_buf)

    def view(self, buf):
        return sp.csr_view(buf[self.offset:], self.d_rp, self.d_ci, (self.m, self.m), self.nnz)

    def buffer(self, fill=float("nan")):
        return torch.full((self.offset + self.nnz + PAD,), fill, dtype=self.a_buf.dtype, device="cuda")

    def set_values(self, values):
        self.a_host[self.offset:self.offset + self.nnz] = np.asarray(values).astype(self.dtype)
        self.a_buf.copy_(G.dev(self.a_host))

    def run(self, s, info=None, fill=float("nan"), with_work=True):
        """One ilu0_sweeps call into fresh buffers; returns LU's nnz values on the host after checking what must stay untouched."""
        lu_buf, w_buf = self.buffer(fill), self.buffer(fill)
        args = (self.a, self.view(lu_buf), w_buf[self.offset:] if with_work else None, s)
        sp.ilu0_sweeps(*(args if info is None else (info,) + args))
        got, w = G.host(lu_buf), G.host(w_buf)
        o, n = self.offset, self.nnz
        guard = U.bits(np.full(1, fill, self.dtype))[0]
        for name, arr in (("lu", got), ("work", w)):
            assert (U.bits(arr[:o]) == guard).all() and (U.bits(arr[o + n:]) == guard).all(), f"{name} written outside its nnz values"
        if not with_work:
            assert (U.bits(w) == guard).all()
        assert np.array_equal(U.bits(G.host(self.a_buf)), U.bits(self.a_host)), "A's values changed"
        return got[o:o + n]

    def exact(self, info):
        lu_buf = self.buffer()
        sp.ilu0(info, self.a, self.view(lu_buf))
        return G.host(lu_buf)[self.offset:self.offset + self.nnz]


def family_dev(name, dtype, offset=0):
    f = S.family(name)
    return f, Dev(f.rowptr, f.colind, f.values, dtype, offset)


# ---- 1. against the host recurrence, every entry ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", S.FAMILY_NAMES)
def test_every_entry_has_the_bits_of_the_host_recurrence(gpu, name, dtype):
    """Both Laplacians, the mirrored level patterns either side of every lane step and the row shapes of every lane count (rows of
    G x 8 and G x 8 + 1 entries: the last of the fast path and the first of the long one, which has 4 G lower entries; lower
    counts 0, 1, G - 1, G, G + 1), s = 1 .. 4, with the lane count the family was made for."""
    f, d = family_dev(name, dtype)
    want = f.iterates(dtype)
    info = sp.ilu0_inspect(d.a)
    assert info.state_.info()["lanes_per_row"] == f.lanes and info.state_.info()["levels"] == f.n_levels
    if name.startswith("shapes"):
        lens = np.diff(f.rowptr)
        assert lens.max() == U.lds_cap(f.lanes) + 1 and U.lds_cap(f.lanes) in lens
    bad = []
    for s in S.SWEEPS:
        bad += [f"s={s}: {msg}" for msg in U.exact_violations(d.run(s, info), want[s], f.rowptr, f.colind)]
        assert sp.ilu0_status(info) == -1
    assert bad == []


# ---- 2. the fixed point ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["laplacian12x12x12", "levels-6m+0", "levels-24m+1"])
def test_fixed_point_is_ilu0_bit_for_bit(gpu, name, dtype):
    """levels - 1 sweeps, and more (clamped), ARE ilu0; a row of level <= s has ilu0's bits after s sweeps.  The level patterns
    hold a run of four narrow levels, which ilu0 walks in its single-workgroup kernel."""
    f, d = family_dev(name, dtype)
    info = sp.ilu0_inspect(d.a)
    levels = info.state_.info()["levels"]
    assert levels == f.n_levels
    exact = d.exact(info)
    assert sp.ilu0_status(info) == -1
    assert np.array_equal(U.bits(exact), U.bits(f.exact(dtype))), "ilu0 itself differs from the host's exact factor"
    for s in (levels - 1, levels + 5):
        assert U.exact_violations(d.run(s, info), exact, f.rowptr, f.colind) == [], s
        assert sp.ilu0_status(info) == -1
    assert U.exact_violations(d.run(levels - 2, info), exact, f.rowptr, f.colind, rows_mask=f.levels <= levels - 2) == []
    for s in range(1, 6):
        assert U.exact_violations(d.run(s, info), exact, f.rowptr, f.colind, rows_mask=f.levels <= s) == [], s


# ---- 3. the exact family with zero pivots ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("zeros", [(0,), (12, 11), (25,)])
def test_zero_pivots_status_and_clean_rows(gpu, zeros, dtype):
    """L and U known by construction, a zero on U's diagonal: early iterates hold inf / NaN wherever a row divides by it, yet at
    s >= levels - 1 the rows that do not depend on such a row are exact and the status is ilu0's."""
    f = S.family("levels-6m+0")
    assert (f.levels[list(zeros)] == 0).all()         # rows of level 0: many rows depend on them
    a_vals, want = U.exact_system(f.rowptr, f.colind, seed=9, zero_pivots=zeros)
    d = Dev(f.rowptr, f.colind, a_vals, dtype)
    info = sp.ilu0_inspect(d.a)
    d.exact(info)
    status = sp.ilu0_status(info)
    assert status == min(zeros)
    clean = U.independent_rows(f.rowptr, f.colind, zeros)
    assert 0 < clean.sum() < clean.size
    for s in (f.n_levels - 1, f.n_levels + 3):
        got = d.run(s, info)
        assert sp.ilu0_status(info) == status
        assert U.exact_violations(got, want, f.rowptr, f.colind, rows_mask=clean) == []
    early = d.run(2, info)
    assert not np.isfinite(early).all()          # (the early iterates really carried inf / NaN)
    # clean values on the same plan report -1 again
    a2, want2 = U.exact_system(f.rowptr, f.colind, seed=10)
    d.set_values(a2)
    assert U.exact_violations(d.run(f.n_levels - 1, info), want2, f.rowptr, f.colind) == []
    assert sp.ilu0_status(info) == -1


# ---- 4. buffers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_buffers_prefill_guards_offsets_and_repeated_calls(gpu, offset, dtype):
    f, d = family_dev("levels-6m+1", dtype, offset)
    want = f.iterates(dtype)
    info = sp.ilu0_inspect(d.a)
    for s in (1, 2, 3, 4):                        # odd and even: the last sweep lands in lu either way
        nan_fill = d.run(s, info)
        zero_fill = d.run(s, info, fill=0.0)
        again = d.run(s, info)
        plan_free = d.run(s)                      # analyses by itself
        for other in (zero_fill, again, plan_free):
            assert np.array_equal(U.bits(nan_fill), U.bits(other))
        assert U.exact_violations(nan_fill, want[s], f.rowptr, f.colind) == []
    assert U.exact_violations(d.run(1, info, with_work=False), want[1], f.rowptr, f.colind) == []     # one sweep needs no work
    # the same buffers twice in a row: the second call starts from the first one's leftovers
    lu_buf, w_buf = d.buffer(), d.buffer()
    lu = d.view(lu_buf)
    for s in (3, 2, 3):
        sp.ilu0_sweeps(info, d.a, lu, w_buf[offset:], s)
        assert U.exact_violations(G.host(lu_buf)[offset:offset + d.nnz], want[s], f.rowptr, f.colind) == []
    empty = sp.operation_info_t()                 # an empty info receives the plan
    sp.ilu0_sweeps(empty, d.a, lu, w_buf[offset:], 2)
    assert isinstance(empty.state_, api._Ilu0Plan) and empty.state_.info()["levels"] == f.n_levels


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def _abi(hd, plan, d, s, a, lu, work, vt=None, m=None, nnz=None, rowptr=None, colind=None):
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return _capi.lib().spblas_gfx950_ilu0_sweeps(
        None if hd is None else hd.h, plan, d.m if m is None else m, d.nnz if nnz is None else nnz, s,
        ptr(d.d_rp if rowptr is None else rowptr) if rowptr is not False else None,
        ptr(d.d_ci if colind is None else colind) if colind is not False else None, ptr(a), ptr(lu), ptr(work),
        VT[d.dtype] if vt is None else vt)


def test_refusals_come_in_the_documented_order(gpu):
    f, d = family_dev("laplacian6x5x4", np.float32)
    hd = api._Handle.current(torch.device("cuda", 0))
    info = sp.ilu0_inspect(d.a)
    plan = info.state_.plan
    a, lu, w = d.a.values(), torch.zeros_like(d.a.values()), torch.zeros_like(d.a.values())
    C = _capi
    # 1. value types that are not offered: before the handle
    for vt in (C.C32, C.C64, C.F16, C.BF16):
        assert _abi(None, None, d, 0, None, None, None, vt=vt, rowptr=False) == C.NOT_SUPPORTED
    # 2. the handle: before the pointers
    assert _abi(None, None, d, 0, None, None, None, rowptr=False) == C.INVALID_HANDLE
    # 3. pointers: before the plan's comparison, the value type, the sweep count and the aliasing rules
    assert _abi(hd, None, d, 0, a, a, a, vt=17, m=d.m + 1) == C.INVALID_POINTER
    assert _abi(hd, plan, d, 0, a, lu, w, rowptr=False, m=d.m + 1) == C.INVALID_POINTER
    assert _abi(hd, plan, d, 0, a, lu, w, colind=False, vt=17) == C.INVALID_POINTER
    assert _abi(hd, plan, d, 0, None, lu, w, nnz=d.nnz - 1) == C.INVALID_POINTER
    assert _abi(hd, plan, d, 0, a, None, a, vt=17) == C.INVALID_POINTER
    assert _abi(hd, plan, d, 2, a, a, None, m=d.m + 1) == C.INVALID_POINTER          # work is needed from two sweeps on ...
    assert _abi(hd, plan, d, 2 ** 30, a, lu, None) == C.INVALID_POINTER              # ... by the REQUESTED count
    # 4. the plan: m, nnz and the addresses of the structure arrays it was made from
    assert _abi(hd, plan, d, 0, a, a, w, vt=17, m=d.m + 1) == C.PLAN_MISMATCH
    assert _abi(hd, plan, d, 0, a, a, w, vt=17, nnz=d.nnz - 1) == C.PLAN_MISMATCH
    assert _abi(hd, plan, d, 0, a, a, w, vt=17, rowptr=d.d_rp.clone()) == C.PLAN_MISMATCH
    assert _abi(hd, plan, d, 0, a, a, w, vt=17, colind=d.d_ci.clone()) == C.PLAN_MISMATCH
    # 5. the value type, 6. the sweep count, 7. the three aliasings
    assert _abi(hd, plan, d, 2, a, lu, w, vt=17) == C.INVALID_VALUE
    assert _abi(hd, plan, d, 2, a, lu, w, vt=-1) == C.INVALID_VALUE
    assert _abi(hd, plan, d, 0, a, lu, w) == C.INVALID_VALUE
    assert _abi(hd, plan, d, -1, a, lu, w) == C.INVALID_VALUE
    assert _abi(hd, plan, d, 2, a, a, w) == C.INVALID_VALUE
    assert _abi(hd, plan, d, 2, a, lu, a) == C.INVALID_VALUE
    assert _abi(hd, plan, d, 2, a, lu, lu) == C.INVALID_VALUE
    assert _abi(hd, plan, d, 1, a, a, None) == C.INVALID_VALUE
    torch.cuda.synchronize()
    assert not lu.any() and not w.any(), "a refused call launched something"
    # one sweep needs no work array
    assert _abi(hd, plan, d, 1, a, lu, None) == C.SUCCESS
    assert U.exact_violations(G.host(lu)[:d.nnz], f.iterates(np.float32)[1], f.rowptr, f.colind) == []


def test_python_layer_refusals_on_the_device(gpu):
    f, d = family_dev("laplacian6x5x4", np.float32)
    info = sp.ilu0_inspect(d.a)
    lu, work = d.view(d.buffer()), d.buffer()
    for bad, exc in ((0, ValueError), (-1, ValueError), (True, TypeError), (2.0, TypeError)):
        with pytest.raises(exc, match="sweeps"):
            sp.ilu0_sweeps(info, d.a, lu, work, bad)
    with pytest.raises(ValueError, match="work"):
        sp.ilu0_sweeps(info, d.a, lu, None, 2)
    with pytest.raises(ValueError, match="own"):                # lu shares A's values
        sp.ilu0_sweeps(info, d.a, d.a, work, 2)
    with pytest.raises(ValueError, match="own"):
        sp.ilu0_sweeps(info, d.a, d.view(d.a_buf), work, 2)
    with pytest.raises(ValueError, match="work"):               # work is A's values, or lu's
        sp.ilu0_sweeps(info, d.a, lu, d.a.values(), 2)
    with pytest.raises(ValueError, match="work"):
        sp.ilu0_sweeps(info, d.a, lu, lu.values(), 2)
    with pytest.raises(ValueError, match="work"):               # on the host
        sp.ilu0_sweeps(info, d.a, lu, work.cpu(), 2)
    with pytest.raises(ValueError):                             # other structure arrays than A's
        sp.ilu0_sweeps(info, d.a, sp.csr_view(lu.values(), d.d_rp.clone(), d.d_ci, (d.m, d.m), d.nnz), work, 2)
    for td in (torch.complex64, torch.complex128, torch.float16, torch.bfloat16):
        vals = torch.ones(d.nnz, dtype=td, device="cuda")
        other = sp.csr_view(vals, d.d_rp, d.d_ci, (d.m, d.m), d.nnz)
        with pytest.raises(TypeError):
            sp.ilu0_sweeps(other, sp.csr_view(vals.clone(), d.d_rp, d.d_ci, (d.m, d.m), d.nnz), vals.clone(), 2)
    with pytest.raises(TypeError):
        sp.ilu0_sweeps(sp.csc_view(d.a.values(), d.d_rp, d.d_ci, (d.m, d.m), d.nnz), lu, work, 2)
    torch.cuda.synchronize()
    assert np.isnan(G.host(lu.values())).all() and np.isnan(G.host(work)).all(), "a refused call wrote something"
    # a view over other structure arrays with its own inspect result works, and replaces a stale plan in the info
    d2 = Dev(f.rowptr, f.colind, f.values, np.float32)
    sp.ilu0_sweeps(info, d2.a, d2.view(d2.buffer()), d2.buffer(), 2)
    assert info.state_.key == api._structure_key(d2.a)


# ---- 6. degenerate shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_shapes(gpu, dtype):
    empty = Dev(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), dtype)
    info = sp.ilu0_inspect(empty.a)
    for s in (1, 3):
        assert empty.run(s, info).size == 0 and sp.ilu0_status(info) == -1
    assert empty.run(1, info, with_work=False).size == 0
    one = Dev(*U.pattern_from_rows([[]]), np.array([3.0]), dtype)                  # m = 1
    info = sp.ilu0_inspect(one.a)
    assert one.run(4, info).tolist() == [3.0] and sp.ilu0_status(info) == -1
    rp, ci = U.pattern_from_rows([[] for _ in range(300)])                         # diagonal: one level, one sweep, LU = A
    vals = U.dominant_values(rp, ci, seed=1)
    diag = Dev(rp, ci, vals, dtype)
    info = sp.ilu0_inspect(diag.a)
    assert info.state_.info()["levels"] == 1
    for s in (1, 2, 7):
        assert np.array_equal(U.bits(diag.run(s, info)), U.bits(vals.astype(dtype)))
    zero = vals.copy()
    zero[17] = 0.0
    diag.set_values(zero)
    diag.run(5, info)
    assert sp.ilu0_status(info) == 17


@pytest.mark.parametrize("dtype", DTYPES)
def test_bidiagonal_chain_of_4097_rows_at_three_sweeps(gpu, dtype):
    m = 4097
    rp, ci = U.pattern_from_rows([[i - 1, i + 1] if 0 < i < m - 1 else ([1] if i == 0 else [m - 2]) for i in range(m)][:m])
    rp2, ci2 = U.pattern_from_rows([[i - 1] if i else [] for i in range(m)])
    for rowptr, colind in ((rp2, ci2), (rp, ci)):          # the bidiagonal chain, and the tridiagonal one whose pivots move
        vals = U.dominant_values(rowptr, colind, seed=m)
        d = Dev(rowptr, colind, vals, dtype)
        info = sp.ilu0_inspect(d.a)
        assert info.state_.info()["levels"] == m
        want = S.host_sweeps(rowptr, colind, vals, 3, dtype)
        assert U.exact_violations(d.run(3, info), want, rowptr, colind) == []
        assert sp.ilu0_status(info) == -1


# ---- 7. graph ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_first_call_on_a_fresh_handle_is_recorded_with_both_applies(gpu, dtype):
    """A new host thread gets a handle of its own.  After ilu0_inspect its FIRST ilu0_sweeps call is recorded, never run eagerly,
    together with the two applies by triangular_solve_sweeps; the graph is replayed after A's values were edited in place.  LU
    must have the bits of the host recurrence, and LU, x and the status those of eager calls on the same data."""
    f = S.family("levels-6m+0")
    rng = np.random.default_rng(7)
    v2 = f.values * rng.choice([1.0, 0.5, 2.0], f.nnz)
    v3 = f.values.copy()
    v3[U.diag_positions(f.rowptr, f.colind)[11]] = 0.0          # a zero pivot in a row of level 0: the status is the replay's own
    assert f.levels[11] == 0
    wants = [f.iterates(dtype)[3], S.host_sweeps(f.rowptr, f.colind, v2, 3, dtype), None]
    out = {}

    def work():
        try:
            mine = api._Handle.current(torch.device("cuda", 0))
            d = Dev(f.rowptr, f.colind, f.values, dtype)
            info = sp.ilu0_inspect(d.a)
            lu_buf, w_buf = d.buffer(), d.buffer()
            lu = d.view(lu_buf)
            b = G.dev((1.0 + np.arange(f.m) % 5).astype(dtype))
            y, x = torch.full_like(b, float("nan")), torch.full_like(b, float("nan"))
            lo, up = (sp.lower_triangle, sp.implicit_unit_diagonal), (sp.upper_triangle, sp.explicit_diagonal)

            def chain(lu, w, y, x):
                sp.ilu0_sweeps(info, d.a, lu, w, 3)
                sp.triangular_solve_sweeps(lu, *lo, b, y, 3)
                sp.triangular_solve_sweeps(lu, *up, y, x, 3)

            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                chain(lu, w_buf, y, x)
            bad = []
            for vals, want, status in ((f.values, wants[0], -1), (v2, wants[1], -1), (v3, None, 11), (f.values, wants[0], -1)):
                d.set_values(vals)
                for t in (lu_buf, w_buf, y, x):
                    t.fill_(float("nan"))
                g.replay()
                got_lu, got_x, got_status = G.host(lu_buf)[:d.nnz].copy(), G.host(x).copy(), sp.ilu0_status(info)
                lu_e, w_e = d.buffer(), d.buffer()
                y_e, x_e = torch.full_like(b, float("nan")), torch.full_like(b, float("nan"))
                chain(d.view(lu_e), w_e, y_e, x_e)
                assert got_status == status == sp.ilu0_status(info)
                bad += U.exact_violations(got_lu, G.host(lu_e)[:d.nnz], f.rowptr, f.colind)
                bad += [] if np.array_equal(U.bits(got_x), U.bits(G.host(x_e))) else ["x differs from the eager calls"]
                if want is not None:
                    bad += U.exact_violations(got_lu, want, f.rowptr, f.colind)
                    assert np.isfinite(got_x).all()
            out["bad"], out["handle"] = bad, mine.h.value
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


# ---- 8. one larger system -----------------------------------------------------------------------------------------------------------
def test_one_larger_mirrored_random_system(gpu):
    """2^18 rows, 9 entries per row inside a band of 4000, mirrored, fp32, s = 3: finite, rows of level <= 3 have ilu0's bits, and
    the clamped count is ilu0 bit for bit.  (ilu_util.residual_violations at s = levels - 1 is left out: on the mirrored pattern
    its host check alone takes longer than the rest of this file, and the factor it would check IS ilu0's, bit for bit, which
    tests/test_gpu_ilu0.py holds to that bound.)"""
    dtype = np.float32
    rp, ci = U.random_pattern(2 ** 18, 9, seed=9, band=4000)
    m = rp.size - 1
    P = sps.csr_matrix((np.ones(ci.size, np.int8), ci, rp), shape=(m, m))
    P = (P + P.T).tocsr()
    P.sort_indices()
    rowptr, colind = P.indptr.astype(np.int32), P.indices.astype(np.int32)
    vals = U.dominant_values(rowptr, colind, seed=10)
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    # the rows of level <= 3, by peeling: a row is of level <= k when all its strict-lower columns are of level <= k - 1
    lower = colind < rows
    has_lower = np.bincount(rows[lower], minlength=m) > 0
    level_le = ~has_lower
    for _ in range(3):
        blocked = np.bincount(rows[lower], weights=(~level_le[colind[lower]]).astype(np.float64), minlength=m) > 0
        level_le = ~blocked
    assert level_le.sum() > 0
    d = Dev(rowptr, colind, vals, dtype)
    info = sp.ilu0_inspect(d.a)
    assert info.state_.info()["lanes_per_row"] == 8
    exact = d.exact(info)
    got = d.run(3, info)
    assert np.isfinite(got).all() and sp.ilu0_status(info) == -1
    assert U.exact_violations(got, exact, rowptr, colind, rows_mask=level_le) == []
    assert S.differing(got, exact) > 0.05
    assert U.exact_violations(d.run(2 ** 30, info), exact, rowptr, colind) == []


# ---- 9. memory; 10. the example ----------------------------------------------------------------------------------------------------
def test_200_calls_leave_device_memory_where_it_was(gpu):
    f, d = family_dev("laplacian12x12x12", np.float32)
    lu, work = d.view(d.buffer()), d.buffer()

    def cycle():
        info = sp.ilu0_inspect(d.a)
        for s in (1, 2, 5):
            sp.ilu0_sweeps(info, d.a, lu, work, s)
        sp.ilu0_sweeps(d.a, lu, work, 3)
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


def test_device_ilu0_sweeps_example_reports_both_residuals(gpu):
    exe = os.path.join(ROOT, "examples", "device_ilu0_sweeps")
    assert os.path.exists(exe), "examples/device_ilu0_sweeps is not built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    mt = re.search(r"exact factor and exact pair ([0-9.e+-]+), 3 factor sweeps and 3 sweeps per apply ([0-9.e+-]+); "
                   r"\|LU\(3\) - LU\| / \|LU\| ([0-9.e+-]+), first bad pivot -1", r.stdout)
    assert mt, r.stdout
    exact, sweeps, diff = (float(mt.group(i)) for i in (1, 2, 3))
    assert exact < 1e-12 and exact < sweeps < 1.0 and 0 < diff < 0.1
