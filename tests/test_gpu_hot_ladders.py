"""-m gpu: the window ladder of the hot-column split of the SLICED SpMV (tests/ladder_hot.py has the families, the restated
inspect and the host model; tests/test_ladders_hot_cpu.py proves on the host that the families reach their rungs).

Every case first asserts that what the inspect laid out -- spblas_gfx950_plan_hot_layout: threshold, K, entries, rows,
windows, crossing rows, grid, depth, and the arrays hot_cols, hot_rows, hot_rowptr, win_row, cross_rows -- equals the
restatement, before y is looked at: a case cannot pass while missing its rung.  Then integer data whose result must equal
the float64 sum rounded once, bit for bit (ladder.check_exact), then random data under the existing bound of the value type
(ladder.check_random).  Arrays are over-long and poisoned as in test_gpu_sliced_ladders.Dev.  A family whose split the
inspect must refuse has to report the ordinary tiled plan (eight zeros, no hot_split) and be right all the same.
"""
import ctypes

import numpy as np
import pytest
import torch

import ladder as L
import ladder_hot as H
import spblas_reference_amd as sp
import test_gpu_sliced_ladders as TS
from spblas_reference_amd import _capi

pytestmark = pytest.mark.gpu

VTS = ["f32", "f64"]
OFFSETS = TS.OFFSETS
ARRAYS = ("hot_cols", "hot_rows", "hot_rowptr", "win_row", "cross_rows")
K_LABELS = ["1", "2", "63", "64", "65", "4095", "4096", "4097", "8193", "kmax-1", "kmax", "thr_rises_kept", "thr_rises_refused"]


def _family(name, vt):
    return H.family(name, vt, TS._cus())


def _assert_layout(info, fam):
    """hot_layout() of the plan against the restated inspect: every count, then every array."""
    n_splits, lays = H.layouts(fam, TS._cus())
    lay = lays[0]
    pi, si = info.state_.info(), info.state_.sliced_info()
    assert pi["alg"] == _capi.SPMV_SLICED, (fam.name, pi)
    got = info.state_.hot_layout()
    want = H.expected_counts(lay, n_splits)
    assert {k_: got[k_] for k_ in want} == want, (fam.name, {k_: (got[k_], want[k_]) for k_ in want if got[k_] != want[k_]})
    assert ("hot_split" in si) == (n_splits > 0), (fam.name, si)
    if n_splits == 0:
        assert all(got[a_].size == 0 for a_ in ARRAYS), fam.name
        return got
    for a_ in ARRAYS:
        assert np.array_equal(got[a_], getattr(lay, a_)), (fam.name, a_)
    hs = si["hot_split"]
    assert hs["hot_columns"] == lay.k and hs["hot_entries"] == lay.n_hot and hs["windows"] == lay.nwin
    assert hs["hot_rows"] == lay.m_hot and hs["hot_long_rows"] == lay.cross_rows.size
    return got


def _inspect(dev, monkeypatch, **kw):
    """multiply_inspect under the family's hooks (set around the inspect only); the layout is asserted before anything runs."""
    fam = dev.fam
    for k_, v_ in fam.env.items():
        monkeypatch.setenv(k_, v_)
    try:
        info = sp.multiply_inspect(dev.a, dev.x, dev.new_y(), alg=_capi.SPMV_SLICED, **kw)
    finally:
        for k_ in fam.env:
            monkeypatch.delenv(k_)
    _assert_layout(info, fam)
    return info


def _run(fam, offsets, monkeypatch):
    for exact in (True, False):
        dev = TS.Dev(fam, OFFSETS[offsets], exact)
        info = _inspect(dev, monkeypatch)
        y = dev.new_y()
        sp.multiply(info, dev.a, dev.x, y)
        dev.check(y, "window ladder")


# ============================================================================================ row starts, windows, ends
@pytest.mark.parametrize("name", H.SMALL + H.SHARES)
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_hot_ladder(gpu, vt, offsets, name, monkeypatch):
    """Row starts on every position of a window, every nibble, 1 ... 256 starts per window, rows over up to 33 windows, the ends
    of A_hot, the hot list's edges, the coverage tests and the second split (ladder_hot's docstring has the families)."""
    _run(_family(name, vt), offsets, monkeypatch)


@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_hot_ladder_walk(gpu, vt, offsets, monkeypatch):
    """SPBLAS_GFX950_PB_HOT_GRID=1: one workgroup, 16 k + r windows -- every wavefront walks k or k + 1 windows through the
    four rotating register sets, the prefetches clamped to the last window at every distance from the end."""
    for k, r in H.WALK_CASES:
        fam = _family(f"walk_{k}_{r}", vt)
        assert H.layouts(fam, TS._cus())[1][0].grid == 1
        _run(fam, offsets, monkeypatch)


@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_hot_ladder_walk_default_grid(gpu, vt, offsets, monkeypatch):
    """2 * 16 * CUs + 3 windows, built for this device: under the default grid every wavefront walks a second window and three
    walk a third."""
    fam = _family("walk_default", vt)
    lay = H.layouts(fam, TS._cus())[1][0]
    assert lay.grid == TS._cus() and lay.nwin == 32 * TS._cus() + 3
    _run(fam, offsets, monkeypatch)


@pytest.mark.parametrize("label", K_LABELS)
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_hot_ladder_hot_list(gpu, vt, offsets, label, monkeypatch):
    """K = 1 ... hot_max_cols (the LDS fill's trips of 4 096, the cap), and one column more than fits: the threshold rises to
    3 -- kept while the columns left carry the share, else refused and the tiled plan reported."""
    name = dict(zip(K_LABELS, H.hot_list_names(vt)))[label]
    _run(_family(name, vt), offsets, monkeypatch)


# ============================================================================================================ alpha / beta
@pytest.mark.parametrize("name", ["long_rows", "starts_per_window"])
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_hot_ladder_alpha_beta(gpu, vt, offsets, name, monkeypatch):
    """y = alpha A x + beta y through the C ABI with (1, 0), (-2, 0.5), (0.5, 1) and (0, 0.5) over a y of small even integers
    (still exact); with beta = 0, y starts as NaN and must not be read."""
    fam = _family(name, vt)
    for exact in (True, False):
        dev = TS.Dev(fam, OFFSETS[offsets], exact)
        info = _inspect(dev, monkeypatch)
        y0 = 2.0 * np.random.default_rng(8).integers(-3, 4, dev.m).astype(np.float64)
        for alpha, beta in ((1.0, 0.0), (-2.0, 0.5), (0.5, 1.0), (0.0, 0.5)):
            y = dev.new_y()
            if beta != 0.0:
                y.copy_(L.cast(vt, y0))
            TS._capi_spmv(dev, info, alpha, beta, y)
            ref = alpha * dev.ref + (beta * y0 if beta != 0.0 else 0.0)
            absrow = abs(alpha) * dev.absrow + abs(beta) * np.abs(y0) * (beta != 0.0)
            if exact:
                assert float(np.abs(absrow).max()) < 2 ** 23 and np.array_equal(ref * 2, np.round(ref * 2))
            dev.check(y, f"alpha={alpha} beta={beta}", ref=ref, absrow=absrow)


# ================================================================================================= state between calls
@pytest.mark.parametrize("name", ["long_rows", "starts_per_window"])
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_hot_ladder_state_between_calls(gpu, vt, offsets, name, monkeypatch):
    """One plan that keeps its source positions: three multiplies with identical bits; another x (the window partials of the
    first call must not show); new values through update_values (no second inspect: the layout is the same object); the
    two-stage calls, all rows in one reduce and a proper row range refused."""
    fam = _family(name, vt)
    for exact in (True, False):
        dev = TS.Dev(fam, OFFSETS[offsets], exact)
        info = _inspect(dev, monkeypatch, values_will_change=True)
        outs = []
        for rep in range(3):
            y = dev.new_y()
            sp.multiply(info, dev.a, dev.x, y)
            dev.check(y, f"repeat {rep}")
            outs.append(y.clone())
        assert torch.equal(L.bits(outs[0]), L.bits(outs[1])) and torch.equal(L.bits(outs[0]), L.bits(outs[2]))
        x2 = dev.x_host[::-1].copy() * (1.0 if exact else 0.75)
        ref2, abs2 = L.spmv_reference(fam.rowptr, fam.colind, dev.values, L.wide(L.cast(vt, x2)), fam.shape)
        xb2 = dev.xb.clone()
        xb2[:dev.n] = L.cast(vt, x2).cuda()
        y = dev.new_y()
        sp.multiply(info, dev.a, xb2[:dev.n], y)
        dev.check(y, "another x", ref=ref2, absrow=abs2)
        dev.set_values(dev.values[::-1] * (2.0 if exact else 0.5))
        info.state_.update_values(dev.a.values())
        _assert_layout(info, fam)
        y = dev.new_y()
        sp.multiply(info, dev.a, dev.x, y)
        dev.check(y, "new values")
        y = dev.new_y()
        expand, reduce_rows = info.state_.bind_stages(dev.x, y.data_ptr(), dev.dt)
        expand()
        reduce_rows(0, dev.m)
        dev.check(y, "two stages")
        with pytest.raises(sp.BackendError):
            reduce_rows(0, dev.m // 2)


# ==================================================================================================================== pads
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_hot_ladder_non_finite_x_on_the_first_hot_column(gpu, vt, offsets, monkeypatch):
    """x = inf on hot_cols[0], which is what every pad multiplies (0 * xs[0]).  long_rows ends in a partial window without a row
    start, a plain reduction: exactly the rows that reference the column are non-finite, every other row keeps its exact
    value."""
    fam = _family("long_rows", vt)
    lay = H.layouts(fam, TS._cus())[1][0]
    assert lay.n_hot % H.constants()["HOT_WIN"] and H.window_stats(lay)["plain"][-1]
    dev = TS.Dev(fam, OFFSETS[offsets], True)
    info = _inspect(dev, monkeypatch)
    col = int(lay.hot_cols[0])
    rows = np.repeat(np.arange(dev.m), np.diff(fam.rowptr))
    touched = np.zeros(dev.m, bool)
    touched[rows[fam.colind == col]] = True
    assert touched.any() and not touched[-1] and (~touched).sum() > 8
    xb = dev.xb.clone()
    xb[col] = float("inf")
    y = dev.new_y()
    sp.multiply(info, dev.a, xb[:dev.n], y)
    torch.cuda.synchronize()
    got = y.cpu()
    bad = ~torch.isfinite(got).numpy()
    assert np.array_equal(bad, touched), (f"non-finite rows {np.flatnonzero(bad & ~touched)[:8]} do not reference column {col}; "
                                          f"finite rows {np.flatnonzero(~bad & touched)[:8]} do")
    L.check_exact(vt, got[torch.from_numpy(~touched)], dev.ref[~touched], "rows that do not reference the column")


# ================================================================================================================= capture
@pytest.mark.parametrize("vt", VTS)
def test_hot_ladder_in_a_stream_capture(gpu, vt, monkeypatch):
    """One captured multiply of a split plan, replayed on the data it was captured with and on another x; the layout
    diagnostic is refused while the stream is capturing."""
    fam = _family("long_rows", vt)
    dev = TS.Dev(fam, np.int32, True)
    info = _inspect(dev, monkeypatch)
    y = dev.new_y()
    x = dev.x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sp.multiply(info, dev.a, x, y)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    status = []
    with torch.cuda.graph(g):
        sp.multiply(info, dev.a, x, y)
        hd = sp.api._Handle.current(y.device)
        counts = (ctypes.c_int64 * 8)()
        status.append(_capi.lib().spblas_gfx950_plan_hot_layout(hd.h, info.state_.plan, counts, None, None, None, None, None))
    assert status == [_capi.NOT_SUPPORTED]
    y.fill_(float("nan"))
    g.replay()
    dev.check(y, "replay")
    x2 = dev.x_host[::-1].copy()
    x.copy_(L.cast(vt, x2).cuda())
    y.fill_(float("nan"))
    g.replay()
    dev.check(y, "replay, another x", ref=L.spmv_reference(fam.rowptr, fam.colind, dev.values, x2, fam.shape)[0])


# ============================================================================================================== diagnostic
def test_hot_layout_checks_its_arguments(gpu, monkeypatch):
    """INVALID_HANDLE / INVALID_POINTER, counts only, and eight zeros for a SLICED plan that was never split."""
    lib = _capi.lib()
    fam = _family("pairs", "f32")
    dev = TS.Dev(fam, np.int32, True)
    info = _inspect(dev, monkeypatch)
    hd = sp.api._Handle.current(dev.x.device)
    counts = (ctypes.c_int64 * 8)()
    assert lib.spblas_gfx950_plan_hot_layout(None, info.state_.plan, counts, None, None, None, None, None) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_plan_hot_layout(hd.h, None, counts, None, None, None, None, None) == _capi.INVALID_POINTER
    assert lib.spblas_gfx950_plan_hot_layout(hd.h, info.state_.plan, None, None, None, None, None, None) == _capi.INVALID_POINTER
    assert lib.spblas_gfx950_plan_hot_layout(hd.h, info.state_.plan, counts, None, None, None, None, None) == 0
    assert counts[1] == 8 and counts[7] == 1
    monkeypatch.setenv(H.PRE + "PB_HOT", "0")
    plain = sp.multiply_inspect(dev.a, dev.x, dev.new_y(), alg=_capi.SPMV_SLICED)
    monkeypatch.delenv(H.PRE + "PB_HOT")
    got = plain.state_.hot_layout()
    assert all(got[k_] == 0 for k_ in ("thr", "k", "n_hot", "m_hot", "nwin", "n_cross", "grid", "depth"))
    assert all(got[a_].size == 0 for a_ in ARRAYS)
