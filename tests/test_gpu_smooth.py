"""-m gpu tests of smooth_prolongator_inspect / smooth_prolongator_structure / smooth_prolongator (spblas_gfx950_smooth_*,
csrc/smooth.hip).  Every test fails on a backend without the feature: the names do not exist there.

The host model, the dense reference, the bound and the generators are tests/smooth_util.py, proved by tests/test_smooth_cpu.py.
Structure and values must equal the model's BIT FOR BIT, float32 and float64 (a NaN must stand where the model has one); random
values must also lie within the bound of the float64 reference.  Every output array is longer than its result and poisoned
behind it."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import aggregate_util as A
import gpu_util as G
import ilu_util as U
import smooth_util as S
import spblas_reference_amd as sp
from spblas_reference_amd import _capi

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TD = {np.float32: torch.float32, np.float64: torch.float64}
PAD = 5
WILD = 2 ** 30
OMEGA = 2.0 / 3.0


def on_device(g, dtype=np.float32):
    """csr_view over over-long arrays: a wild column and NaN behind nnz."""
    rowptr, colind, values = g[:3]
    m, nnz = rowptr.size - 1, int(colind.size)
    d_v = G.dev(np.concatenate([np.asarray(values, np.float64), np.full(PAD, np.nan)]).astype(dtype))
    d_ci = G.dev(np.concatenate([colind.astype(np.int32), np.full(PAD, WILD, np.int32)]))
    return sp.csr_view(d_v, G.dev(rowptr.astype(np.int32)), d_ci, (m, m), nnz)


def empty_p(m, n, nnz, dtype):
    """P's arrays, poisoned throughout: rowptr / colind with WILD, values with NaN."""
    return sp.csr_view(torch.full((nnz + PAD,), float("nan"), dtype=TD[dtype], device="cuda"),
                       torch.full((m + 1 + PAD,), WILD, dtype=torch.int32, device="cuda"),
                       torch.full((nnz + PAD,), WILD, dtype=torch.int32, device="cuda"), (m, n), nnz)


def host_p(p, m, nnz):
    rp, ci, v = G.host(p.rowptr()), G.host(p.colind()), G.host(p.values())
    assert (rp[m + 1:] == WILD).all() and (ci[nnz:] == WILD).all() and np.isnan(v[nnz:]).all(), "written behind the end"
    return rp[:m + 1], ci[:nnz], v[:nnz]


def same_bits(got, want):
    """Bit for bit, except that a NaN only has to be a NaN."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(U.bits(got)[~nan], U.bits(want)[~nan])


def smooth(a, agg, n, omega, theta, dtype):
    m = a.shape()[0]
    info = sp.smooth_prolongator_inspect(a, G.dev(np.asarray(agg, np.int32)), n)
    assert tuple(info.shape) == (m, n) and tuple(info.result_shape()) == (m, n) and info.result_nnz() == info.nnz
    p = empty_p(m, n, info.nnz, dtype)
    sp.smooth_prolongator_structure(info, p)
    sp.smooth_prolongator(info, a, p, omega, theta)
    return info, p


def check(g, agg, n, omega=OMEGA, theta=0.0, dtype=np.float32, reference=False):
    """Device against the model, bit for bit; returns (model, device values)."""
    m = g[0].size - 1
    a = on_device(g, dtype)
    info, p = smooth(a, agg, n, omega, theta, dtype)
    mod = S.model(g[0], g[1], g[2], agg, n, omega, theta, dtype)
    rp, ci, v = host_p(p, m, info.nnz)
    assert info.nnz == mod["p_colind"].size and np.array_equal(rp, mod["p_rowptr"]) and np.array_equal(ci, mod["p_colind"])
    assert S.check_structure(m, n, rp, ci) == []
    bad = np.flatnonzero(~((U.bits(v) == U.bits(mod["p_values"])) | (np.isnan(v) & np.isnan(mod["p_values"]))))
    assert bad.size == 0, f"{bad.size} of {v.size} values differ, first at entry {int(bad[0])} (row {int(mod['rows'][bad[0]])}): " \
                          f"{v[bad[0]]!r} against {mod['p_values'][bad[0]]!r}"
    assert np.array_equal(U.bits(G.host(a.values())[:g[1].size]), U.bits(np.asarray(g[2]).astype(dtype))), "A's values changed"
    if reference:
        ref = S.dense_reference(g[0], g[1], g[2], agg, n, omega, theta, dtype)
        got = dict(mod, p_values=v)
        assert S.against_reference(got, ref, dtype) == []
    return mod, v


def hashed_map(m, n):
    return (np.arange(m, dtype=np.int64) * 2654435761 % 1000003 % n).astype(np.int32)


def model_aggregates(g, theta=0.0, dtype=np.float32):
    got = A.model(g[0], g[1], g[2], theta, dtype)
    return got["agg"], got["n_agg"]


# ---- team widths, block edges, row lengths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rung", A.lane_rungs(), ids=lambda r: f"G{r[0]}_m{r[1]}")
def test_every_team_width_at_the_block_edges(gpu, rung):
    G_, m, g = rung
    n = max(1, m // 6)
    check(g, hashed_map(m, n), n, OMEGA, 0.25, np.float32)
    check(g, hashed_map(m, n), n, 0.5, 0.0, np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lanes", [4, 8, 16, 64])
def test_rows_of_0_1_2_entries_and_around_the_staging_capacity(gpu, lanes, dtype):
    g, lengths = S.capacity_rows(lanes)
    m = len(lengths)
    n = 23
    mod, _ = check(g, hashed_map(m, n), n, OMEGA, 0.25, dtype)
    cap = S.stage_capacity(lanes)
    assert np.diff(g[0])[:6].tolist() == [0, 1, 2, cap - 1, cap, cap + 1]
    assert mod["p_values"][0] == 1 and np.diff(mod["p_rowptr"])[0] == 1          # the empty row is a single 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_row_far_past_the_capacity(gpu, dtype):
    g, agg, n = S.hub_with_agg(5000)
    mod, _ = check(g, agg, n, OMEGA, 0.0, dtype)
    assert np.diff(mod["p_rowptr"])[0] == n and mod["terms"][:n].sum() == 5000
    # random values on the long row: the order of the additions shows
    v = np.random.default_rng(1).standard_normal(g[1].size)
    check((g[0], g[1], v), agg, n, OMEGA, 0.0, dtype)


def test_one_row_no_row_and_no_entry(gpu):
    for dtype in DTYPES:
        mod, v = check(A.diagonal(1), np.zeros(1, np.int32), 1, OMEGA, 0.0, dtype)
        assert v.tolist() == [np.dtype(dtype).type(1) - np.dtype(dtype).type(OMEGA)]         # no strong entry: base_i alone
    a = sp.csr_view(torch.zeros(0, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
                    torch.zeros(0, dtype=torch.int32, device="cuda"), (0, 0), 0)
    info = sp.smooth_prolongator_inspect(a, torch.zeros(0, dtype=torch.int32, device="cuda"), 0)
    assert tuple(info.shape) == (0, 0) and info.nnz == 0
    p = empty_p(0, 0, 0, np.float32)
    sp.smooth_prolongator_structure(info, p)
    sp.smooth_prolongator(info, a, p, OMEGA)
    assert G.host(p.rowptr())[0] == 0 and (G.host(p.rowptr())[1:] == WILD).all() and np.isnan(G.host(p.values())).all()
    # rows, but no entry at all: P is T
    import multicolor_util as MC
    rp, ci = MC.from_rows([[] for _ in range(7)])
    mod, v = check((rp, ci, np.zeros(0)), np.array([0, 1, 0, 2, 2, 1, 0], np.int32), 3, OMEGA, 0.0, np.float32)
    assert v.tolist() == [1.0] * 7 and mod["p_colind"].tolist() == [0, 1, 0, 2, 2, 1, 0]


# ---- the rule, case by case -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_diagonals_missing_doubled_and_unsorted_repeated_entries(gpu, dtype):
    nd = S.without_diagonal(A.grid5(5, 4))
    mod, v = check(nd, hashed_map(20, 4), 4, OMEGA, 0.0, dtype)
    assert not mod["smoothed"].any() and set(v.tolist()) <= {0.0, 1.0}             # dF = 0 everywhere: T on P's pattern
    g = S.two_diagonals()
    mod, _ = check(g, hashed_map(20, 4), 4, OMEGA, 0.0, dtype)
    assert (mod["dF"] == 7).all()                                                  # d uses the first (4), dF both (4 + 3)
    g = A.repeated_entries()
    agg, n = model_aggregates(g, 0.25, dtype)
    mod, _ = check(g, agg, n, OMEGA, 0.25, dtype, reference=True)
    assert (mod["dF"] >= 1004).all()
    assert any((np.diff(g[1][g[0][i]:g[0][i + 1]]) < 0).any() for i in range(g[0].size - 1))     # a row is not sorted


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_whose_own_aggregate_has_no_stored_entry(gpu, dtype):
    g, agg, n = S.foreign_rows()
    mod, v = check(g, agg, n, OMEGA, 0.0, dtype)
    assert mod["p_colind"].size == 79
    g = A.upper_bidiagonal(30)                          # with a diagonal, but the map sends row i elsewhere than its columns
    rows = A._rows(g[0])
    keep = g[1] != rows
    m = 30
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=m))]).astype(np.int32)
    check((rp2, g[1][keep], g[2][keep]), (np.arange(m) % 2).astype(np.int32), 2, OMEGA, 0.0, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_threshold_anisotropic_and_the_cancelling_row(gpu, dtype):
    g = A.threshold(dtype)
    T = np.dtype(dtype).type
    mod, _ = check(g, (np.arange(12) // 2).astype(np.int32), 6, 0.5, 0.25, dtype, reference=True)
    assert (mod["dF"][1:11] == T(4) + np.nextafter(T(1), T(0))).all() and mod["terms"].sum() == 12
    g = A.anisotropic(16, 16)
    agg, n = model_aggregates(g, 0.25, dtype)
    mod, _ = check(g, agg, n, OMEGA, 0.25, dtype, reference=True)
    assert mod["terms"].sum() == 2 * 15 * 16                                         # the x couplings only
    g = S.cancelling_row()
    mod, v = check(g, (np.arange(12) // 2).astype(np.int32), 6, OMEGA, 0.25, dtype)
    e0, e1 = mod["p_rowptr"][5], mod["p_rowptr"][6]
    assert not mod["smoothed"][5] and v[e0:e1].tolist() == [1.0 if c == 2 else 0.0 for c in mod["p_colind"][e0:e1]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_infinity_touch_the_rows_the_model_says(gpu, dtype):
    g = A.lap7(6)
    agg, n = model_aggregates(g, 0.0, dtype)
    clean, v0 = check(g, agg, n, OMEGA, 0.0, dtype)
    rows = A._rows(g[0])
    off = int(np.flatnonzero((rows == 40) & (g[1] != 40))[0])
    dia = int(np.flatnonzero((rows == 40) & (g[1] == 40))[0])
    for pos, bad in ((off, np.nan), (off, np.inf), (off, -np.inf), (dia, np.nan), (dia, np.inf)):
        vals = g[2].copy()
        vals[pos] = bad
        mod, v = check((g[0], g[1], vals), agg, n, OMEGA, 0.0, dtype)
        touched = set(mod["rows"][U.bits(v) != U.bits(v0)].tolist())
        assert 40 in touched and touched <= ({40} if pos == off else {40} | set(rows[g[1] == 40].tolist()))


def test_identity_one_aggregate_empty_aggregates_and_an_arbitrary_map(gpu):
    g = A.grid5(7, 9)
    m = 63
    vals = np.where(g[1] == A._rows(g[0]), 8.0, np.random.default_rng(4).integers(-3, 0, g[1].size).astype(np.float64))
    g = (g[0], g[1], vals)
    rng = np.random.default_rng(5)
    maps = {"one": (np.zeros(m, np.int32), 1), "identity": (np.arange(m, dtype=np.int32), m),
            "user": (rng.integers(0, 9, m).astype(np.int32), 9),
            "empty_aggregates": ((rng.integers(0, 5, m) * 3 + 1).astype(np.int32), 17)}       # 0, 2, 3, 5, ... hold no row
    for name, (agg, n) in maps.items():
        for dtype in DTYPES:
            mod, v = check(g, agg, n, OMEGA, 0.0, dtype, reference=True)
            if name == "one":
                assert mod["p_colind"].size == m and (mod["p_colind"] == 0).all()
            if name == "identity":                                # sorted rows with a diagonal: A's pattern
                assert np.array_equal(mod["p_rowptr"], g[0]) and np.array_equal(mod["p_colind"], g[1])
            if name == "empty_aggregates":
                assert not np.isin(mod["p_colind"], [0, 2, 3, 5]).any()
    a = on_device(g)
    for bad in (np.full(m, 9, np.int32), np.full(m, -1, np.int32)):
        with pytest.raises(ValueError):
            sp.smooth_prolongator_inspect(a, G.dev(bad), 9)


@pytest.mark.parametrize("dtype", DTYPES)
def test_omegas_and_the_tentative_prolongator_at_zero(gpu, dtype):
    g = A.random_graph(500, 8, 7)
    res = sp.aggregate(on_device(g, dtype), 0.25)
    agg, n = G.host(res.agg), res.n_agg
    for omega in (OMEGA, 0.5, 1.0, 1, -0.25):
        check(g, agg, n, omega, 0.25, dtype, reference=True)
    mod, v = check(g, agg, n, 0.0, 0.25, dtype)
    t = res.prolongator(TD[dtype])
    own = mod["p_colind"] == agg[mod["rows"]]
    assert own.sum() == 500 and np.array_equal(mod["p_colind"][own], G.host(t.colind()))
    assert np.array_equal(U.bits(v[own]), U.bits(G.host(t.values()))) and (U.bits(v[~own]) == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_values_bit_for_bit_and_within_the_bound(gpu, dtype):
    """Random float values: the quotient omega / dF_i is inexact in almost every row, so this is the case that shows whether the
    device quotient is the IEEE one.  theta = 0 keeps dF_i the stored diagonal (exact), which the bound assumes."""
    g = A.random_graph(2000, 10, 2)
    rows = A._rows(g[0])
    rng = np.random.default_rng(9)
    vals = np.where(g[1] == rows, 4.0 + rng.random(g[1].size), rng.standard_normal(g[1].size))
    res = sp.aggregate(on_device(g, dtype), 0.25)
    mod, _ = check((g[0], g[1], vals), G.host(res.agg), res.n_agg, OMEGA, 0.0, dtype, reference=True)
    assert mod["smoothed"].all()
    # graph Laplacian: the row sums of P are 1 within the summed bound
    g = S.graph_laplacian(300, 4, 1)
    agg, n = model_aggregates(g, 0.0, dtype)
    mod, v = check(g, agg, n, OMEGA, 0.0, dtype)
    sums = np.add.reduceat(v.astype(np.float64), mod["p_rowptr"][:-1])
    assert (np.abs(sums - 1) <= np.add.reduceat(S.bound(mod, dtype), mod["p_rowptr"][:-1])).all()


# ---- state between calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_edited_values_on_one_info_eagerly_and_in_a_graph(gpu, dtype):
    g = A.random_graph(2000, 10, 2)
    rp, ci = g[0], g[1]
    nnz = int(ci.size)
    rows = A._rows(rp)
    rng = np.random.default_rng(6)
    draw = lambda: np.where(ci == rows, 4.0 + rng.random(nnz), rng.standard_normal(nnz))
    a = on_device((rp, ci, draw()), dtype)
    agg, n = hashed_map(2000, 300), 300
    agg_dev = G.dev(agg)
    info = sp.smooth_prolongator_inspect(a, agg_dev, n)
    plan, pn = info.state_, info.nnz
    # the value array of P lies inside a longer NaN-patterned one whose pattern must keep its bits
    big = torch.full((pn + 2 * PAD,), float("nan"), dtype=TD[dtype], device="cuda")
    pattern = U.bits(G.host(big)).copy()
    p = sp.csr_view(big[PAD:PAD + pn], torch.full((2001,), WILD, dtype=torch.int32, device="cuda"),
                    torch.full((pn,), WILD, dtype=torch.int32, device="cuda"), (2000, n), pn)
    g0, g1 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0):                         # recorded from the FIRST call of each, on a fresh info
        sp.smooth_prolongator_structure(info, p)
    with torch.cuda.graph(g1):
        sp.smooth_prolongator(info, a, p, OMEGA, 0.25)
    assert (G.host(p.colind()) == WILD).all() and np.array_equal(U.bits(G.host(big)), pattern)    # recording ran nothing
    g0.replay()
    w = S.structure(rp, ci, agg, n)
    assert np.array_equal(G.host(p.rowptr()), w[0]) and np.array_equal(G.host(p.colind()), w[1])
    for replay in (True, True, True, False):
        new = draw().astype(dtype)
        a.values()[:nnz].copy_(G.dev(new))
        big.fill_(float("nan"))
        p.colind().fill_(WILD)                                # the value pass must not touch the structure
        g1.replay() if replay else sp.smooth_prolongator(info, a, p, OMEGA, 0.25)
        assert info.state_ is plan
        got = G.host(big)
        assert same_bits(got[PAD:PAD + pn], S.model(rp, ci, new, agg, n, OMEGA, 0.25, dtype)["p_values"])
        assert np.array_equal(U.bits(got[:PAD]), pattern[:PAD]) and np.array_equal(U.bits(got[PAD + pn:]), pattern[PAD + pn:])
        assert (G.host(p.colind()) == WILD).all()
    # the same values twice, and after a call with another omega: nothing is kept between calls
    first = G.host(big).copy()
    sp.smooth_prolongator(info, a, p, 0.25, 0.0)
    sp.smooth_prolongator(info, a, p, OMEGA, 0.25)
    assert np.array_equal(U.bits(G.host(big)), U.bits(first))
    # an info made for other arrays is replaced by a new inspect
    a2 = on_device((rp, ci, draw()), dtype)
    sp.smooth_prolongator(info, a2, p, OMEGA, 0.25)
    assert info.state_ is not plan and info.nnz == pn


def test_inspect_raises_inside_a_capture(gpu):
    g = A.grid5(7, 9)
    a = on_device(g)
    agg = G.dev(hashed_map(63, 9))
    first = sp.smooth_prolongator_inspect(a, agg, 9)        # the handle exists before the capture
    torch.cuda.synchronize()
    raised = []
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        try:
            sp.smooth_prolongator_inspect(a, agg, 9)
            raised.append(None)
        except Exception as e:  # noqa: BLE001
            raised.append(e)
    assert all(isinstance(e, sp.BackendError) and "not supported" in str(e).lower() for e in raised), raised
    assert sp.smooth_prolongator_inspect(a, agg, 9).nnz == first.nnz


def test_calls_check_their_plan_and_their_buffers(gpu):
    g = A.lap7(5)
    a = on_device(g)
    res = sp.aggregate(a)
    n = res.n_agg
    info = sp.smooth_prolongator_inspect(a, res.agg, n)
    plan, lib, nnz, pn = info.state_, _capi.lib(), a.size(), info.nnz
    p = empty_p(125, n, pn, np.float32)
    rp, ci, av, pv = a.rowptr().data_ptr(), a.colind().data_ptr(), a.values().data_ptr(), p.values().data_ptr()
    h = plan.hd.h
    w32 = lambda x: ctypes.byref(ctypes.c_float(x))
    val = lambda hh, pl, m, k, r, c, x, om, th, pk, y, vt: lib.spblas_gfx950_smooth_values(hh, pl, m, k, r, c, x, om,
                                                                                          ctypes.c_double(th), pk, y, vt)
    nan, inf = float("nan"), float("inf")
    # the statuses in their documented order
    assert val(None, None, 124, nnz, None, None, None, None, -1.0, pn, None, _capi.C32) == _capi.NOT_SUPPORTED
    assert val(None, None, 124, nnz, None, None, None, None, -1.0, pn, None, _capi.F16) == _capi.NOT_SUPPORTED
    assert val(None, None, 124, nnz, None, None, None, None, -1.0, pn, None, _capi.F32) == _capi.INVALID_HANDLE
    assert val(h, None, 125, nnz, rp, ci, av, w32(0.5), 0.0, pn, pv, _capi.F32) == _capi.INVALID_POINTER
    assert val(h, plan.plan, 124, nnz, rp, ci, av, None, -1.0, pn, pv, 99) == _capi.INVALID_POINTER
    assert val(h, plan.plan, 124, nnz, rp, ci, None, w32(nan), -1.0, pn, pv, 99) == _capi.INVALID_POINTER
    assert val(h, plan.plan, 124, nnz, rp, ci, av, w32(nan), -1.0, pn, av, 99) == _capi.PLAN_MISMATCH
    assert val(h, plan.plan, 125, nnz - 1, rp, ci, av, w32(nan), -1.0, pn, av, 99) == _capi.PLAN_MISMATCH
    assert val(h, plan.plan, 125, nnz, rp, ci, av, w32(nan), -1.0, pn - 1, av, 99) == _capi.PLAN_MISMATCH
    assert val(h, plan.plan, 125, nnz, rp, ci, av, w32(nan), -1.0, pn, av, 99) == _capi.INVALID_VALUE
    for om, th in ((nan, 0.0), (inf, 0.0), (0.5, -1.0), (0.5, nan), (0.5, inf)):
        assert val(h, plan.plan, 125, nnz, rp, ci, av, w32(om), th, pn, pv, _capi.F32) == _capi.INVALID_VALUE
    assert val(h, plan.plan, 125, nnz, rp, ci, av, w32(0.5), 0.0, pn, av, _capi.F32) == _capi.INVALID_VALUE   # no in-place form
    assert np.isnan(G.host(p.values())).all()
    assert val(h, plan.plan, 125, nnz, rp, ci, av, w32(0.5), 0.0, pn, pv, _capi.F32) == _capi.SUCCESS
    assert same_bits(G.host(p.values())[:pn], S.model(*g, G.host(res.agg), n, 0.5, 0.0, np.float32)["p_values"])
    st = lambda hh, pl, r, cc: lib.spblas_gfx950_smooth_structure(hh, pl, r, cc)
    assert st(None, plan.plan, p.rowptr().data_ptr(), p.colind().data_ptr()) == _capi.INVALID_HANDLE
    assert st(h, None, p.rowptr().data_ptr(), p.colind().data_ptr()) == _capi.INVALID_POINTER
    assert st(h, plan.plan, None, p.colind().data_ptr()) == _capi.INVALID_POINTER
    assert st(h, plan.plan, p.rowptr().data_ptr(), None) == _capi.INVALID_POINTER
    arr = (ctypes.c_int64 * 4)()
    assert lib.spblas_gfx950_smooth_info(None, arr) == _capi.INVALID_POINTER
    assert lib.spblas_gfx950_smooth_info(plan.plan, arr) == 0 and list(arr) == [n, pn, 125, nnz]
    create = lambda hh, out, m, k, r, c, ag, na: lib.spblas_gfx950_smooth_create(hh, out, m, k, r, c, ag, na)
    out = ctypes.c_void_p()
    ptrs = (rp, ci, res.agg.data_ptr())
    assert create(None, None, -1, nnz, None, None, None, -1) == _capi.INVALID_HANDLE
    assert create(h, None, -1, nnz, *ptrs, -1) == _capi.INVALID_POINTER
    assert create(h, ctypes.byref(out), -1, nnz, *ptrs, -1) == _capi.INVALID_SIZE
    assert create(h, ctypes.byref(out), 125, nnz, *ptrs, -1) == _capi.INVALID_SIZE
    assert create(h, ctypes.byref(out), 125, 2 ** 31 - 100, *ptrs, n) == _capi.INVALID_SIZE    # nnz + m does not fit int32
    assert create(h, ctypes.byref(out), 125, nnz, *ptrs, 0) == _capi.INVALID_VALUE
    assert create(h, ctypes.byref(out), 125, nnz, *ptrs, n - 1) == _capi.INVALID_VALUE          # an entry of agg is outside
    assert create(h, ctypes.byref(out), 125, nnz - 1, *ptrs, n) == _capi.INVALID_VALUE          # the offsets end past nnz
    assert out.value is None
    assert lib.spblas_gfx950_smooth_destroy(None, plan.plan) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_smooth_destroy(h, None) == 0
    # Python: the refusals of coarsen, in its TypeError / ValueError split
    alias = sp.csr_view(a.values()[:pn], p.rowptr(), p.colind(), (125, n), pn)
    with pytest.raises(ValueError):
        sp.smooth_prolongator(info, a, alias, 0.5)
    with pytest.raises(TypeError):
        sp.smooth_prolongator(sp.operation_info_t(), a, p, 0.5)
    with pytest.raises(TypeError):
        sp.smooth_prolongator(sp.coarsen_inspect(a, res.agg, n), a, p, 0.5)
    with pytest.raises(TypeError):
        sp.smooth_prolongator(info, a, empty_p(125, n, pn, np.float64), 0.5)
    with pytest.raises(ValueError):
        sp.smooth_prolongator(info, a, empty_p(125, n, pn - PAD - 1, np.float32), 0.5)
    for bad in (nan, inf, -inf, 1e300):
        with pytest.raises(ValueError):
            sp.smooth_prolongator(info, a, p, bad)
    for bad in (-0.5, nan, inf):
        with pytest.raises(ValueError):
            sp.smooth_prolongator(info, a, p, 0.5, bad)
    for bad in ("0.5", None, True):
        with pytest.raises(TypeError):
            sp.smooth_prolongator(info, a, p, bad)
    with pytest.raises(TypeError):
        sp.smooth_prolongator(info, a, p, 0.5, "0")
    with pytest.raises(TypeError):
        sp.smooth_prolongator_inspect(a, res.agg.long(), n)
    with pytest.raises(ValueError):
        sp.smooth_prolongator_inspect(a, res.agg[:124], n)
    with pytest.raises(TypeError):
        sp.smooth_prolongator_inspect(sp.transposed(a), res.agg, n)
    for td in (torch.complex64, torch.float16, torch.bfloat16):
        mk = sp.csr_view(torch.ones(nnz, dtype=td, device="cuda"), a.rowptr(), a.colind(), (125, 125), nnz)
        with pytest.raises(TypeError):
            sp.smooth_prolongator_inspect(mk, res.agg, n)
    bad_ci = g[1].copy()
    bad_ci[7] = 125
    with pytest.raises(ValueError):
        sp.smooth_prolongator_inspect(on_device((g[0], bad_ci, g[2])), res.agg, n)
    torch.cuda.synchronize()


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_galerkin_product_with_the_smoothed_prolongator(gpu, dtype):
    """A_c = multiply(transpose(P), multiply(A, P)) against the dense P^T A P of the MODEL's P in float64.  Both are sums of the
    same products in different orders: an entry of A P sums k1 products, an entry of P^T (A P) k2 of those; every product and
    every addition rounds once, so each side is within (terms + 1) u sum|p a p| of the exact sum and they differ by at most
    (terms + 1) eps sum|p| |a| |p| -- the bound of the SpGEMM tests, evaluated as |P|^T |A| |P| with terms bounded by the
    number of products of the entry."""
    import scipy.sparse as sps
    g = A.lap7(12)
    rp, ci = g[0], g[1]
    m, nnz = rp.size - 1, int(ci.size)
    res = sp.aggregate(on_device(g, dtype))
    n, agg = res.n_agg, G.host(res.agg)
    a = on_device(g, dtype)
    info, p = smooth(a, agg, n, OMEGA, 0.0, dtype)
    mod = S.model(rp, ci, g[2], agg, n, OMEGA, 0.0, dtype)
    assert same_bits(host_p(p, m, info.nnz)[2], mod["p_values"])
    pn = info.nnz
    a_exact = sp.csr_view(a.values()[:nnz], a.rowptr(), a.colind()[:nnz], (m, m), nnz)
    p_exact = sp.csr_view(p.values()[:pn], p.rowptr()[:m + 1], p.colind()[:pn], (m, n), pn)

    def product(x, y, shape):
        rp_ = torch.zeros(shape[0] + 1, dtype=torch.int32, device="cuda")
        z = sp.csr_view(None, rp_, None, shape, 0)
        st = sp.multiply_compute(x, y, z)
        k = st.result_nnz()
        z.update(torch.zeros(k, dtype=TD[dtype], device="cuda"), rp_, torch.zeros(k, dtype=torch.int32, device="cuda"), shape, k)
        sp.multiply_fill(st, x, y, z)
        return z

    ap = product(a_exact, p_exact, (m, n))
    pt = sp.csr_view(torch.zeros(pn, dtype=TD[dtype], device="cuda"), torch.zeros(n + 1, dtype=torch.int32, device="cuda"),
                     torch.zeros(pn, dtype=torch.int32, device="cuda"), (n, m), pn)
    sp.transpose(p_exact, pt)
    ac = product(pt, ap, (n, n))
    got = sps.csr_matrix((G.host(ac.values()).astype(np.float64), G.host(ac.colind()), G.host(ac.rowptr())), shape=(n, n)).toarray()
    P = S.as_csr(mod, m, n)
    Am = sps.csr_matrix((g[2].astype(dtype).astype(np.float64), ci.astype(np.int64), rp.astype(np.int64)), shape=(m, m))
    want = (P.T @ Am @ P).toarray()
    mag = (abs(P).T @ abs(Am) @ abs(P)).toarray()
    ones = lambda M_: sps.csr_matrix((np.ones(M_.nnz), M_.indices, M_.indptr), shape=M_.shape)
    terms = (ones(P).T @ ones(Am) @ ones(P)).toarray()
    assert (np.abs(got - want) <= (terms + 1) * np.finfo(dtype).eps * mag).all()
    assert (got != 0).sum() > n                                                         # a coarse matrix, not a diagonal


def test_create_destroy_cycles_do_not_leak_device_memory(gpu):
    g = A.lap7(24)
    a = on_device(g)
    res = sp.aggregate(a)
    info0 = sp.smooth_prolongator_inspect(a, res.agg, res.n_agg)
    p = empty_p(24 ** 3, res.n_agg, info0.nnz, np.float32)
    del info0

    def cycle():
        info = sp.smooth_prolongator_inspect(a, res.agg, res.n_agg)
        sp.smooth_prolongator_structure(info, p)
        sp.smooth_prolongator(info, a, p, OMEGA)
        del info

    for _ in range(5):      # warm-up: pools and the handle's scratch reach their size
        cycle()
    torch.cuda.synchronize()
    gc.collect()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(200):
        cycle()
    torch.cuda.synchronize()
    gc.collect()
    free1, _ = torch.cuda.mem_get_info()
    lost = free0 - free1
    # one cycle allocates ~1.5 MB of plan tables and work arrays: a leak of any of them shows over 200 cycles
    assert lost < 8 * 2 ** 20, f"free device memory fell by {lost / 2**20:.1f} MiB over 200 cycles"
