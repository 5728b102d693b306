"""-m gpu: the column ladders of tests/ladder_trsm.py on the device -- the block triangular solve of csrc/sptrsm.hip on integer
systems whose solution must come out EXACTLY: X must equal x_true f_j (f_j = (-1)^j (j + 1), pairwise different) bit for bit, in
fp32 and fp64.  B and X are windows of wider tensors filled with a NaN bit pattern: outside the windows every bit must be
unchanged, and B must be unchanged unless B is X.  After every solve spblas_gfx950_sptrsm_last must report the geometry
restated in ladder_trsm.geometry -- path, mis, units, logC, E, b_piece, x_bytes, passes -- and is compared BEFORE X is looked
at.  Each test ends by comparing the set of rungs it ran with the set it intended.

  (a) every n = 1 ... 133 x every shift of X x B shifted alike / differently; odd leading dimension, layout_left X, layout_left B
      and B = X in place on a subset; n = 1 with two contiguous vectors (forwarded to the vector solve)
  (b) every (logC, E) of the rule E = min(lanes, 64 >> logC) for 4 / 8 / 16 / 64 lanes per row on ladder_tt's row-shape systems
  (c) wide levels of k (256 / team) - 1, + 0, + 1 rows and a narrow level of 1024 / team + 1 rows, for teams of 4 / 16 / 64 lanes
  (d) X spanning 2^31 - 16, 2^31 + 16, 0xFFFFFFF0 and 0xFFFFFFF0 + 16 bytes
  (e) random data on the rungs of (a) at the highest shift, under the bound of trsm_util.violations
  (f) one solve per path recorded into a graph and replayed on a new B
"""
import numpy as np
import pytest
import torch

import gpu_util as G
import ladder_trsm as M
import ladder_tt as T
import spblas_reference_amd as sp
import trsm_util as TU
import tt_ladder_run as R

pytestmark = pytest.mark.gpu
VTS = ["f32", "f64"]
SIZE_OF = {"f32": 4, "f64": 8}
DEVICE = "cuda"


def _bits(t):
    return t.view(R.INT_OF[t.element_size()])


class Dev:
    """A ladder system on the device with its exact values, its plan (checked against ladder_tt.predicted_info), and the
    first nmax columns of B = b f_j and of the X the solve must return, in the value type."""

    def __init__(self, sysm, vt, nmax, narrow=None, coop=True):
        self.sysm, self.vt, self.size = sysm, vt, SIZE_OF[vt]
        self.nd, self.td = R.NUMPY_OF[vt], R.TORCH_OF[vt]
        self.a = G.csr_on_device(sysm.exact_values.astype(self.nd), sysm.rowptr, sysm.colind, (sysm.m, sysm.m), sysm.nnz)
        self.A = sp.scaled(sysm.alpha, self.a) if sysm.alpha != 1.0 else self.a
        self.uplo, self.diag = R.tags(sysm.upper, sysm.unit)
        z = torch.zeros(sysm.m, dtype=self.td, device=DEVICE)
        self.info = sp.triangular_solve_inspect(self.A, self.uplo, self.diag, z, z.clone())
        want = T.predicted_info(sysm.rowptr, sysm.colind, sysm.m, sysm.upper, narrow=narrow,
                                coop=coop and not R.hsa_tool_loaded())
        got = self.info.state_.info()
        assert got == want and want["lanes_per_row"] == sysm.lanes, f"the plan reports {got}, restated on the host: {want}"
        self.B = G.dev(M.block_rhs(sysm, nmax).astype(self.nd))
        self.want = G.dev(M.block_x(sysm, nmax).astype(self.nd))
        self.hd = sp.api._Handle.current(self.B.device)

    def solve(self, wb, wx):
        sp.triangular_solve(self.info, self.A, self.uplo, self.diag, wb, wx)

    def restated(self, n, wx, xop, wb, bop):
        return M.geometry(self.sysm.m, n, self.size, self.sysm.lanes, wx.data_ptr(), *M.abi_strides(*xop, n), wb.data_ptr(),
                          *M.abi_strides(*bop, n))


def solve_window(d, n, xs, bs, xop, bop, inplace=False, B=None, exact=True):
    """One solve of n columns: X a window (layout, leading dimension) = xop, xs elements into a poisoned tensor, B likewise
    (bop, bs) or X itself.  Returns (what sptrsm_last reported, the window of X).  exact: X must equal d.want[:, :n]."""
    m = d.sysm.m
    what = f"{d.vt} n {n}, X {xop} shift {xs}, B {'is X' if inplace else (bop, 'shift', bs)}"
    fx = M.poisoned(M.window_numel(xs, m, n, xop[1], xop[0]), d.td, DEVICE)
    assert fx.data_ptr() % 16 == 0
    wx = M.window(fx, xs, m, n, xop[1], xop[0])
    if inplace:
        fb, wb = fx, wx
    else:
        fb = M.poisoned(M.window_numel(bs, m, n, bop[1], bop[0]), d.td, DEVICE)
        assert fb.data_ptr() % 16 == 0
        wb = M.window(fb, bs, m, n, bop[1], bop[0])
    wb.copy_((d.B if B is None else B)[:, :n])
    fb0 = None if inplace else fb.clone()
    d.solve(wb, wx)
    got, want = d.hd.sptrsm_last(), d.restated(n, wx, xop, wb, bop)
    assert got == want, f"{what}: sptrsm_last reports {got}, restated on the host: {want}"
    expect = M.poisoned(fx.numel(), d.td, DEVICE)
    M.window(expect, xs, m, n, xop[1], xop[0]).copy_(d.want[:, :n] if exact else wx)
    if not torch.equal(_bits(fx), _bits(expect)):
        bad = M.exact_violations(G.host(wx), d.sysm) if exact else []
        raise AssertionError(f"{what} ({got}): {bad or 'written outside the window of X'}")
    assert inplace or torch.equal(_bits(fb), _bits(fb0)), f"{what}: B changed"
    return got, wx


# ---- (a) columns x misalignment ----------------------------------------------------------------------------------------
def _column_paths(rungs, V):
    return {r: 1 if r[3] == "contig" else 3 if r[0] >= V and r[3] in ("R", "bL", "inplace") else 2 for r in rungs}


@pytest.mark.parametrize("vt", VTS)
def test_column_and_misalignment_ladder(gpu, vt):
    """(a): level 0, a run of narrow levels (the chain kernel) and a wide level; every n up to 2 TRSM_MAX_C V + V + 1 of fp32, X
    shifted by every 0 ... V - 1 elements, B shifted alike (its units are pieces too) and differently (they are not)."""
    sysm = M.column_system()
    size = SIZE_OF[vt]
    V = M.V_of(size)
    d = Dev(sysm, vt, M.column_ns()[-1])
    rungs = M.column_rungs(size)
    ran = {}
    for n, xs, bs, variant in rungs:
        xop, bop = M.rung_operands(sysm.m, n, xs, bs, variant, size)
        got, _ = solve_window(d, n, xs, bs, xop, bop, inplace=variant == "inplace")
        assert got["path"] != 3 or (got["mis"], got["b_piece"]) == (xs, int(bs == xs and variant != "bL"))
        ran[(n, xs, bs, variant)] = got["path"]
    assert ran == _column_paths(rungs, V) and len(ran) == len(rungs) and set(ran.values()) == {1, 2, 3}


# ---- (b) the (E, C) table ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", [False, True], ids=["explicit", "unit"])
@pytest.mark.parametrize("upper", [False, True], ids=["lower", "upper"])
@pytest.mark.parametrize("lanes", M.EC_LANES)
def test_entry_and_unit_lane_table(gpu, lanes, upper, unit):
    """(b): the row shapes of ladder_tt.row_shapes -- every strict count 0 ... 2 G + 2, the diagonal first, last, at G - 1, G,
    2 G - 1, 2 G, stored twice -- under every (logC, E) the lane class yields, one of them in two passes, at mis 0 and 1."""
    sysm = T.shape_system(lanes, upper, unit)
    table = M.ec_table(lanes)
    M.assert_shapes_around_every_E(sysm, lanes, set(table.values()))
    ran = set()
    for vt in VTS:
        size = SIZE_OF[vt]
        d = Dev(sysm, vt, max(M.ec_ns(size, 0)))
        for mis in (0, 1):
            for n in M.ec_ns(size, mis):
                op = ("R", M.ld_for(n, size))
                got, _ = solve_window(d, n, mis, mis, op, op)
                assert got["path"] == 2 or got["mis"] == mis
                ran.add((vt, mis, got["logC"], got["E"], got["passes"]))
    assert ran == {(vt, mis, lc, e, 1) for vt in VTS for mis in (0, 1) for lc, e in table.items()} | \
        {(vt, mis, max(table), table[max(table)], 2) for vt in VTS for mis in (0, 1)}


# ---- (c) level widths around the teams ---------------------------------------------------------------------------------
@pytest.mark.parametrize("team", M.TEAMS)
def test_level_widths_around_the_teams(gpu, monkeypatch, team):
    """(c): a workgroup of the level kernel holds 256 / team teams, one pass of the chain kernel 1024 / team: levels of one row
    fewer, as many and one more (the plan is made under a `narrow` limit that makes the levels wide, or all of them narrow)."""
    monkeypatch.setenv("SPBLAS_GFX950_TRSV_COOP", "0")          # (the plan then reports its launch groups one by one)
    wide, wlimit, narrow, nlimit = M.team_widths(team)
    ran = set()
    for which, limit in (("wide", wlimit), ("narrow", nlimit)):
        monkeypatch.setenv("SPBLAS_GFX950_TRSV_NARROW", str(limit))
        sysm = M.team_system(team, which)
        groups = T.groups_of(sysm.widths, limit)
        for vt in VTS:
            size = SIZE_OF[vt]
            n = M.team_n(team, size)
            d = Dev(sysm, vt, n, narrow=limit, coop=False)
            assert d.info.state_.info()["launches_per_solve"] == len(groups) == (len(wide) if which == "wide" else 1)
            op = ("R", M.ld_for(n, size))
            got, _ = solve_window(d, n, 0, 0, op, op)
            assert got["E"] << got["logC"] == team
            ran.add((which, vt, got["path"]))
    assert ran == {(w, vt, 3) for w in ("wide", "narrow") for vt in VTS}


# ---- (d) the reach of the buffer descriptor ----------------------------------------------------------------------------
def test_reach_of_the_buffer_descriptor(gpu):
    """(d): X is a window with a very large row stride inside ONE allocation that is never filled: spans of 2^31 - 16 bytes, of
    2^31 + 16 (the first byte offsets with the sign bit set), of exactly 0xFFFFFFF0 (the last span the pieces path admits) and of
    16 bytes more (the element path).  Lower: the last row is stored furthest; upper: row 0 gathers it.  Only the V elements in
    front of and behind every row of the window are poisoned and checked."""
    spans = M.reach_spans()
    slack = 4096
    total = max(spans.values()) + slack
    need = total + 256 * 2 ** 20
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB are free")
    store = torch.empty(total, dtype=torch.uint8, device=DEVICE)
    assert store.data_ptr() % 16 == 0
    ran = {}
    for vt in VTS:
        size = SIZE_OF[vt]
        V = M.V_of(size)
        flat = store.view(R.TORCH_OF[vt])
        lead = 4 * V
        for name, span in spans.items():
            m, n, xrs = M.reach_shape(span, size)
            for upper in (False, True):
                sysm = M.dense_system(m, upper, seed=m)
                d = Dev(sysm, vt, n)
                for shift in (0, 1):
                    what = f"{vt} {name}: m {m}, n {n}, row stride {xrs}, {'upper' if upper else 'lower'}, shift {shift}"
                    assert (lead + shift + (m - 1) * xrs + n + V) * size <= total
                    wx = torch.as_strided(flat, (m, n), (xrs, 1), lead + shift)
                    rows = torch.as_strided(flat, (m, n + 2 * V), (xrs, 1), lead + shift - V)   # every row with its guards
                    rows.copy_(M.poisoned(m * (n + 2 * V), d.td, DEVICE).view(m, n + 2 * V))
                    wb = d.B[:, :n].contiguous()
                    b0 = wb.clone()
                    d.solve(wb, wx)
                    got = d.hd.sptrsm_last()
                    want = M.geometry(m, n, size, sysm.lanes, wx.data_ptr(), xrs, 1, wb.data_ptr(), n, 1)
                    assert got == want, f"{what}: sptrsm_last reports {got}, restated on the host: {want}"
                    assert got["path"] == (2 if name == "first_refused" else 3) and got["x_bytes"] == (span if got["path"] == 3 else 0)
                    assert got["path"] == 2 or got["mis"] == shift
                    expect = M.poisoned(m * (n + 2 * V), d.td, DEVICE).view(m, n + 2 * V).clone()
                    expect[:, V:V + n] = d.want[:, :n]
                    if not torch.equal(_bits(rows.contiguous()), _bits(expect)):
                        bad = M.exact_violations(G.host(wx.contiguous()), sysm)
                        raise AssertionError(f"{what} ({got}): {bad or 'written in front of or behind a row of X'}")
                    assert torch.equal(_bits(wb), _bits(b0)), f"{what}: B changed"
                    ran[(vt, name, upper, shift)] = got["path"]
    del store, flat, wx, rows
    torch.cuda.empty_cache()
    assert ran == {(vt, name, up, s): 2 if name == "first_refused" else 3
                   for vt in VTS for name in ("below_2^31", "above_2^31", "last_admitted", "first_refused")
                   for up in (False, True) for s in (0, 1)}


# ---- (e) random data ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vt", VTS)
def test_random_data_on_the_column_ladder(gpu, vt):
    """(e): the rungs of (a) at shift V - 1 with the system's random values (a dominant diagonal) and trsm_util.rhs data, under
    the bound of trsm_util.violations against the oracle's columns."""
    sysm = M.column_system()
    size, nd = SIZE_OF[vt], R.NUMPY_OF[vt]
    V = M.V_of(size)
    nmax = M.column_ns()[-1]
    d = Dev(sysm, vt, nmax)
    Ms = T.as_scipy(sysm, sysm.random_values)
    # the same row offsets and columns with the random values: the plan made for the exact ones serves them
    d.A = sp.csr_view(G.dev(sysm.random_values.astype(nd)), d.a.rowptr(), d.a.colind(), (sysm.m, sysm.m), sysm.nnz)
    Bh = TU.rhs(sysm.m, nmax, seed=size)
    ref = TU.oracle_block(Ms, Bh, sysm.upper, sysm.unit, nd)
    Bd = G.dev(Bh.astype(nd))
    rungs = [r for r in M.column_rungs(size) if r[1] == V - 1]
    ran = {}
    for n, xs, bs, variant in rungs:
        xop, bop = M.rung_operands(sysm.m, n, xs, bs, variant, size)
        got, wx = solve_window(d, n, xs, bs, xop, bop, inplace=variant == "inplace", B=Bd, exact=False)
        if variant == "contig":
            d.info.state_.check_status()
        bad = TU.violations(Ms, Bh[:, :n], G.host(wx), sysm.upper, sysm.unit, nd, ref=ref[:, :n])
        assert not bad, f"{vt} n {n}, X shift {xs}, B shift {bs}, {variant}: {bad}"
        ran[(n, xs, bs, variant)] = got["path"]
    assert ran == _column_paths(rungs, V) and {r[0] for r in ran} == set(M.column_ns())


# ---- (f) capture -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [2, 3])
def test_block_solve_in_a_graph(gpu, path):
    """(f): after an eager first solve the block solve is recorded into a graph and replayed with new right-hand sides (the
    columns of B in reversed order: X must hold the columns of x_true f_j in reversed order)."""
    sysm = M.column_system()
    vt = "f32" if path == 3 else "f64"
    size = SIZE_OF[vt]
    V = M.V_of(size)
    n, shift = 4 * V + 1, 1
    d = Dev(sysm, vt, n)
    xop = ("R", M.ld_for(n, size)) if path == 3 else ("L", M.ld_for(sysm.m, size))
    bop = ("R", M.ld_for(n, size))
    got, _ = solve_window(d, n, shift, shift, xop, bop)          # the eager first solve of the plan
    assert got["path"] == path
    fx = M.poisoned(M.window_numel(shift, sysm.m, n, xop[1], xop[0]), d.td, DEVICE)
    fb = M.poisoned(M.window_numel(shift, sysm.m, n, bop[1], bop[0]), d.td, DEVICE)
    wx, wb = M.window(fx, shift, sysm.m, n, *xop[::-1]), M.window(fb, shift, sysm.m, n, *bop[::-1])
    wb.copy_(d.B[:, :n])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        d.solve(wb, wx)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d.solve(wb, wx)
    want = d.restated(n, wx, xop, wb, bop)
    assert d.hd.sptrsm_last() == want and want["path"] == path   # (host integers: recorded while the stream was capturing)
    ran = []
    for order in (list(range(n)), list(range(n))[::-1], [0] + list(range(n))[:0:-1]):
        idx = torch.tensor(order, device=DEVICE)
        fx.copy_(M.poisoned(fx.numel(), d.td, DEVICE))
        wb.copy_(d.B[:, :n][:, idx])
        fb0 = fb.clone()
        g.replay()
        torch.cuda.synchronize()
        expect = M.poisoned(fx.numel(), d.td, DEVICE)
        M.window(expect, shift, sysm.m, n, *xop[::-1]).copy_(d.want[:, :n][:, idx])
        assert torch.equal(_bits(fx), _bits(expect)), f"replay with columns {order[:3]} ...: X differs from x_true f_j"
        assert torch.equal(_bits(fb), _bits(fb0))
        ran.append(order[-1])
    assert ran == [n - 1, 0, 1]
