"""The ladders of tests/ladder_trsm.py checked without a GPU: the limits are read from csrc/sptrsm.hip, geometry() agrees with a
second restatement on the whole (n, mis, lanes) grid, the host model of trsm_row returns x_true f_j EXACTLY on every rung
family (at reduced sizes where the full ones would take the model minutes), every rung list holds what it claims -- each
(logC, E) pair, 1 / 2 / 3 passes, every misalignment, every width of the partial units in front and behind --, and the rungs bite:

  mutation of the model                              fails rung
  the tree strides by o instead of o << logC         (b) four lanes, two units (logC 1, E 4); invisible at logC 0
  a unit starts at u V + mis                         (a) n = 2 V + 1 at shift 1; invisible at shift 0
  the last partial unit is dropped                   (a) n = 2 V + 1 at shift 0; invisible at n = 2 V
"""
import numpy as np
import pytest

import ladder_trsm as M
import ladder_tt as T
import trsm_util as TU

DTYPES = {4: np.float32, 8: np.float64}
BASE = 1 << 20            # a 16-byte-aligned stand-in for an allocation's address


def _geo(sysm, n, itemsize, xs, bs, variant="R"):
    """geometry() of a rung of ladder (a) / (b) on stand-in addresses."""
    (lx, ldx), (lb, ldb) = M.rung_operands(sysm.m, n, xs, bs, variant, itemsize)
    xaddr = BASE + xs * itemsize
    baddr = xaddr if variant == "inplace" else 2 * BASE + bs * itemsize
    return M.geometry(sysm.m, n, itemsize, sysm.lanes, xaddr, *M.abi_strides(lx, ldx, n), baddr, *M.abi_strides(lb, ldb, n))


def _model(sysm, n, itemsize, geo, mutation=None, stats=None):
    return M.model_solve(sysm, M.block_rhs(sysm, n), DTYPES[itemsize], geo, mutation, stats)


# =============================================================================================================== limits
def test_limits_are_read_from_the_source():
    t = M.limits()
    assert t == {"max_c": 16, "chain_threads": 1024, "wave": 64, "piece": 16, "reach": 0xFFFFFFF0, "level_threads": 256}
    assert (M.V_of(4), M.V_of(8)) == (4, 2)
    assert M.column_ns()[0] == 1 and M.column_ns()[-1] == 2 * t["max_c"] * 4 + 4 + 1 == 133


# ============================================================================================================= geometry
def test_geometry_agrees_with_a_second_restatement_on_the_whole_grid():
    seen = set()
    for itemsize in (4, 8):
        V = M.V_of(itemsize)
        for lanes in (4, 8, 16, 64):
            for n in range(1, 141):
                for mis in range(V):
                    for xrs, xcs in ((M.ld_for(n, itemsize), 1), (M.ld_for(n, itemsize, odd=True), 1), (1, 48), (n, 1)):
                        if n == 1 and xcs != 1:
                            xrs, xcs = 1, 1
                        for bsh, brs, bcs in ((mis, M.ld_for(n, itemsize), 1), ((mis + 1) % V, M.ld_for(n, itemsize), 1),
                                              (mis, M.ld_for(n, itemsize, odd=True), 1), (mis, 1, 48)):
                            if n == 1 and bcs != 1:
                                brs, bcs = 1, 1
                            args = (37, n, itemsize, lanes, BASE + mis * itemsize, xrs, xcs, 2 * BASE + bsh * itemsize, brs, bcs)
                            a, b = M.geometry(*args), M.independent_geometry(*args)
                            assert a == b, (args, a, b)
                            seen.add((a["path"], a["logC"], a["E"], a["b_piece"], min(a["passes"], 3)))
    assert {s[0] for s in seen} == {1, 2, 3}
    assert {(s[1], s[2]) for s in seen if s[0] > 1} == {(lc, min(g, 64 >> lc)) for lc in range(5) for g in (4, 8, 16, 64)}
    assert {s[3] for s in seen if s[0] == 3} == {0, 1} and {s[3] for s in seen if s[0] == 2} == {0}
    # X one byte off the element grid, X within and beyond the reach
    for itemsize in (4, 8):
        for name, span in M.reach_spans().items():
            m, n, xrs = M.reach_shape(span, itemsize)
            args = (m, n, itemsize, 4, BASE, xrs, 1, 2 * BASE, n, 1)
            a, b = M.geometry(*args), M.independent_geometry(*args)
            assert a == b and a["path"] == (2 if name == "first_refused" else 3) and a["x_bytes"] == (span if a["path"] == 3 else 0)
        args = (37, 9, itemsize, 8, BASE + 1, 12, 1, 2 * BASE, 12, 1)
        assert M.geometry(*args) == M.independent_geometry(*args) and M.geometry(*args)["path"] == 2


def test_partial_widths():
    assert [M.partial_widths(n, mis, 4) for n, mis in ((8, 0), (9, 0), (9, 1), (9, 3), (2, 1), (4, 2), (133, 0))] == \
        [(0, 0), (0, 1), (3, 2), (1, 0), (2, 0), (2, 2), (0, 1)]
    assert [M.partial_widths(n, mis, 8) for n, mis in ((4, 0), (5, 0), (5, 1), (4, 1))] == [(0, 0), (0, 1), (1, 0), (1, 1)]


# =========================================================================================================== exact data
def test_factors_are_pairwise_different_integers_in_the_exact_range():
    f = M.factors(M.MAX_COLS)
    assert f[:4].tolist() == [1.0, -2.0, 3.0, -4.0] and np.unique(f).size == M.MAX_COLS and np.abs(f).max() == 160
    assert np.array_equal(f, np.round(f))
    assert 300 * 2 * 3 * 160 == 288_000 < 2 ** 22            # the longest row of the shape systems, at its worst
    systems = [M.column_system(), M.column_system(small=True)]
    systems += [M.team_system(team, which) for team in M.TEAMS for which in ("wide", "narrow")]
    systems += [M.small_shape_system(lanes, up, un) for lanes in M.EC_LANES for up, un in ((False, False), (True, True))]
    systems += [M.dense_system(m, up, seed=m) for m in (5, 50) for up in (False, True)]
    for s in systems:
        B = M.block_rhs(s, M.MAX_COLS)                        # (asserts the module's condition)
        assert M.sum_of_products(s) * 160 <= 288_000
        for dt in (np.float32, np.float64):
            assert np.array_equal(B.astype(dt).astype(np.float64), B)
            assert np.array_equal(M.block_x(s, 7).astype(dt).astype(np.float64), M.block_x(s, 7))
    with pytest.raises(AssertionError):
        M.factors(M.MAX_COLS + 1)


def test_exact_violations_sees_swapped_shifted_and_dropped_columns():
    s = M.column_system(small=True)
    X = M.block_x(s, 9).astype(np.float32)
    assert not M.exact_violations(X, s)
    for bad in (X[:, [1, 0] + list(range(2, 9))], np.roll(X, 1, axis=1), np.concatenate([X[:, :8], X[:, :1]], axis=1), -X):
        assert M.exact_violations(np.ascontiguousarray(bad), s)
    Y = X.copy()
    Y[17, 8] = np.nextafter(Y[17, 8], np.float32(np.inf))
    assert "row 17, column 8" in M.exact_violations(Y, s)[0]


# ============================================================================================================ the model
@pytest.mark.parametrize("itemsize", [4, 8])
def test_model_is_exact_on_the_column_ladder(itemsize):
    """(a) on the 44-row system: every n and every shift on the pieces path; the layout subset on the element path."""
    s = M.column_system(small=True)
    V = M.V_of(itemsize)
    ran = set()
    for n in M.column_ns():
        for shift in range(V):
            for variant in ("R",) + (("xL",) if n in M.layout_subset(itemsize) and shift == 0 else ()):
                geo = _geo(s, n, itemsize, shift, shift, variant)
                st = {}
                X = _model(s, n, itemsize, geo, stats=st)
                assert not M.exact_violations(X, s), (n, shift, variant)
                front, back = M.partial_widths(n, geo["mis"], itemsize)
                if geo["path"] == 3:
                    assert st["passes"] == geo["passes"] * s.m and st["widths"] == {front, back} - {0}
                    assert st["whole"] == s.m * ((n - front - back) // V)
                else:
                    assert st["whole"] == 0
                ran.add((n, shift, variant))
    assert len(ran) == len(M.column_ns()) * V + len(M.layout_subset(itemsize))


def test_model_is_exact_on_the_ec_table():
    """(b) on the one-level shape systems: every (logC, E) of every lane class, lower / explicit and upper / unit."""
    ran = set()
    for lanes in M.EC_LANES:
        for up, un in ((False, False), (True, True)):
            s = M.small_shape_system(lanes, up, un)
            assert set(s.shape_of[s.level == 1]) == {x.name for x in T.row_shapes(lanes, un)}
            for mis in (0, 1):
                itemsize = 4 if (mis + up) % 2 == 0 else 8
                for n in M.ec_ns(itemsize, mis):
                    geo = _geo(s, n, itemsize, mis, mis)
                    assert not M.exact_violations(_model(s, n, itemsize, geo), s), (lanes, up, un, mis, n)
                    ran.add((lanes, geo["logC"], geo["E"]))
    assert ran == {(g, lc, e) for g in M.EC_LANES for lc, e in M.ec_table(g).items()}


def test_model_is_exact_on_the_team_and_reach_systems():
    for team in M.TEAMS:
        for which in ("wide", "narrow"):
            s = M.team_system(team, which)
            for itemsize in (4, 8):
                n = M.team_n(team, itemsize)
                geo = _geo(s, n, itemsize, 0, 0)
                assert geo["E"] << geo["logC"] == team
                if which == "narrow" or team == 64:
                    assert not M.exact_violations(_model(s, n, itemsize, geo), s)
    for itemsize in (4, 8):
        for name, span in M.reach_spans().items():
            m, n, xrs = M.reach_shape(span, itemsize)
            for up in (False, True):
                s = M.dense_system(m, up, seed=m)
                for shift in (0, 1):
                    geo = M.geometry(m, n, itemsize, s.lanes, BASE + shift * itemsize, xrs, 1, 2 * BASE, n, 1)
                    assert not M.exact_violations(_model(s, n, itemsize, geo), s), (name, itemsize, up, shift)


# ===================================================================================================== rung completeness
@pytest.mark.parametrize("itemsize", [4, 8])
def test_column_rungs_are_complete(itemsize):
    s = M.column_system()
    t = M.limits()
    V = M.V_of(itemsize)
    assert s.widths == [130, 3, 5, 2, 130] and s.lanes == 4 and not s.upper
    narrow = T.trsv_limits()["narrow"]
    assert [(e - l, w) for l, e, w in T.groups_of(s.widths, narrow)] == [(1, True), (3, False), (1, True)]
    rungs = M.column_rungs(itemsize)
    assert len(set(rungs)) == len(rungs)
    assert {(n, xs) for n, xs, bs, v in rungs if v == "R"} == {(n, sh) for n in range(1, 134) for sh in range(V)}
    geos = {r: _geo(s, r[0], itemsize, r[1], r[2], r[3]) for r in rungs}
    pieces = {r: g for r, g in geos.items() if g["path"] == 3}
    assert set(pieces) == {r for r in rungs if r[0] >= V and r[3] in ("R", "bL", "inplace")}
    assert {g["path"] for r, g in geos.items() if r[3] in ("odd", "xL") or (r[0] < V and r[3] != "contig")} == {2}
    assert {r for r, g in geos.items() if g["path"] == 1} == {(1, sh, sh, "contig") for sh in range(V)}
    # every (logC, E) of four lanes per row, 1 / 2 / 3 passes, every misalignment -- each on the pieces path WITH a partial unit
    with_partial = {r: g for r, g in pieces.items() if any(M.partial_widths(r[0], g["mis"], itemsize))}
    # (one unit lane means one unit: a whole one, or the element path)
    assert {(g["logC"], g["E"]) for g in with_partial.values()} == {(lc, 4) for lc in range(1, 5)}
    assert {(g["logC"], g["E"]) for g in pieces.values()} == {(g["logC"], g["E"]) for g in geos.values() if g["path"] == 2} == \
        {(lc, 4) for lc in range(5)}
    assert {1, 2, 3} <= {g["passes"] for g in with_partial.values()}
    assert {g["mis"] for g in with_partial.values()} == set(range(V))
    for mis in range(V):                                      # every front / back width at every misalignment that allows it
        widths = {M.partial_widths(r[0], mis, itemsize) for r, g in pieces.items() if g["mis"] == mis}
        assert {w[0] for w in widths} == {(V - mis) % V} and {w[1] for w in widths} == set(range(V))
    assert {M.partial_widths(r[0], g["mis"], itemsize)[0] for r, g in pieces.items()} == set(range(V))
    for passes in (2, 3):                                     # more than one pass of the unit loop on each kind of last unit
        assert {M.partial_widths(r[0], g["mis"], itemsize)[1] for r, g in pieces.items() if g["passes"] == passes} == set(range(V))
    # B's pieces aligned like X's and not; every variant of the subset on every shift
    assert {(g["mis"], g["b_piece"]) for r, g in pieces.items() if r[3] == "R"} == {(mis, b) for mis in range(V) for b in (0, 1)}
    assert {g["b_piece"] for r, g in pieces.items() if r[3] == "bL"} == {0}
    assert {g["b_piece"] for r, g in pieces.items() if r[3] == "inplace"} == {1}
    sub = M.layout_subset(itemsize)
    assert set(TU.N_SWEEP) - {257} <= set(sub)
    for C in (1, 2, 4, 8, 16):                                # the last n of C units and the first n of C + 1
        assert {C * V, C * V + 1} <= set(sub)
    assert {2 * t["max_c"] * V, 2 * t["max_c"] * V + 1} <= set(sub)
    assert {(n, xs, v) for n, xs, bs, v in rungs if v not in ("R", "contig")} == \
        {(n, xs, v) for n in sub for xs in range(V) for v in ("odd", "xL", "bL", "inplace")}
    # the rungs the mutations and the issue's gaps hang on reach what they are meant to reach
    named = {"three_passes_partial": (2 * t["max_c"] * V + V + 1, 0, 0, "R"), "mis_top": (2 * V + 1, V - 1, V - 1, "R"),
             "b_other_shift": (2 * V, 0, 1, "R"), "one_whole_unit": (V, 0, 0, "R")}
    g = geos[named["three_passes_partial"]]
    assert g["passes"] == 3 and g["units"] > 2 * t["max_c"] and g["path"] == 3
    assert M.partial_widths(named["three_passes_partial"][0], 0, itemsize) == (0, 1)
    g = geos[named["mis_top"]]
    assert g["mis"] == V - 1 and M.partial_widths(2 * V + 1, V - 1, itemsize)[0] == 1
    assert geos[named["b_other_shift"]]["b_piece"] == 0 and geos[named["one_whole_unit"]]["units"] == 1
    assert any(g["passes"] == 3 and g["units"] == 2 * t["max_c"] + 1 for g in pieces.values())


def test_ec_rungs_are_complete():
    """(b): the column counts reach every (logC, E) of every lane class at both misalignments and both value types, one of
    them in two passes; the shape systems hold the row lengths and diagonal positions around every E."""
    t = M.limits()
    for lanes in M.EC_LANES:
        table = M.ec_table(lanes)
        assert len(table) == 5 and table[0] == lanes and table[4] == 4
        if lanes == 64:
            assert [table[lc] for lc in range(5)] == [64, 32, 16, 8, 4]
        s = T.shape_system(lanes, False, False)
        for itemsize in (4, 8):
            for mis in (0, 1):
                geos = [_geo(s, n, itemsize, mis, mis) for n in M.ec_ns(itemsize, mis)]
                assert [(g["logC"], g["E"]) for g in geos[:5]] == sorted(table.items())
                assert [g["passes"] for g in geos] == [1] * 5 + [2] and geos[5]["logC"] == 4
                assert all(g["mis"] == mis for g in geos if g["path"] == 3) and [g["path"] for g in geos[1:]] == [3] * 5
        for up, un in ((False, False), (True, False), (False, True), (True, True)):
            M.assert_shapes_around_every_E(T.shape_system(lanes, up, un), lanes, set(table.values()))
            M.assert_shapes_around_every_E(M.small_shape_system(lanes, up, un), lanes, set(table.values()), runs=False)


def test_team_rungs_are_complete():
    t = M.limits()
    for team in M.TEAMS:
        wide, wlimit, narrow, nlimit = M.team_widths(team)
        per_wg, per_chain = t["level_threads"] // team, t["chain_threads"] // team
        assert wide[1:] == [per_wg - 1, per_wg, per_wg + 1, 2 * per_wg - 1, 2 * per_wg, 2 * per_wg + 1]
        assert all(w for _, _, w in T.groups_of(wide, wlimit)) and len(T.groups_of(wide, wlimit)) == len(wide)
        assert T.groups_of(narrow, nlimit) == [(0, len(narrow), False)] and narrow[2] == per_chain + 1
        assert any((w * team) % t["wave"] for w in wide[1:]) or team == t["wave"]      # the exit cuts inside a wavefront
        for which, widths in (("wide", wide), ("narrow", narrow)):
            s = M.team_system(team, which)
            assert s.widths == widths and s.lanes == 4
            assert np.array_equal(T.levels_of(s.rowptr, s.colind, s.m, s.upper), s.level)
        for itemsize in (4, 8):
            g = _geo(M.team_system(team, "wide"), M.team_n(team, itemsize), itemsize, 0, 0)
            assert (g["E"], 1 << g["logC"], g["path"]) == (4, team // 4, 3)


def test_reach_rungs_are_complete():
    t = M.limits()
    spans = M.reach_spans()
    assert spans == {"below_2^31": 2 ** 31 - 16, "above_2^31": 2 ** 31 + 16, "last_admitted": 0xFFFFFFF0,
                     "first_refused": 0xFFFFFFF0 + 16}
    assert M.reach_shape(0xFFFFFFF0, 4, m_range=range(5, 6)) == (5, 12, 268_435_452)       # the shape the ladder was asked for
    for itemsize in (4, 8):
        V = M.V_of(itemsize)
        for name, span in spans.items():
            m, n, xrs = M.reach_shape(span, itemsize)
            assert 5 <= m <= 50 and n >= 2 * V and ((m - 1) * xrs + n) * itemsize == span and (xrs * itemsize) % t["piece"] == 0
            far = span - t["piece"]                            # byte offset of the last row's last unit: what the lower system's
            assert (far >= 2 ** 31) == (name != "below_2^31")  # last store, and the gather of the upper system's row 0, address
            assert far + t["piece"] == ((m - 1) * xrs + n) * itemsize and (m - 1) * xrs * itemsize > 2 ** 31 - 40 * t["piece"]
            for up in (False, True):
                s = M.dense_system(m, up, seed=m)
                r = 0 if up else m - 1
                assert (m - 1 - r) in s.colind[s.rowptr[r]:s.rowptr[r + 1]].tolist()     # ... gathers the row furthest away


# ============================================================================================================ mutations
def _fails(s, n, itemsize, shift, mutation):
    geo = _geo(s, n, itemsize, shift, shift)
    assert not M.exact_violations(_model(s, n, itemsize, geo), s)
    return bool(M.exact_violations(_model(s, n, itemsize, geo, mutation), s)), geo


@pytest.mark.parametrize("itemsize", [4, 8])
def test_each_mutation_of_the_model_fails_its_rung(itemsize):
    V = M.V_of(itemsize)
    # the tree strides by o: rung (b), four lanes per row, two units
    s = M.small_shape_system(4, False, False)
    n = M.ec_ns(itemsize, 0)[1]
    failed, geo = _fails(s, n, itemsize, 0, "tree_stride")
    assert failed and (geo["logC"], geo["E"]) == (1, 4)
    failed, geo = _fails(s, M.ec_ns(itemsize, 0)[0], itemsize, 0, "tree_stride")
    assert not failed and geo["logC"] == 0                    # ... and no rung of ONE unit lane can see it
    for lanes in (8, 64):
        s8 = M.small_shape_system(lanes, True, True)
        failed, geo = _fails(s8, M.ec_ns(itemsize, 1)[3], itemsize, 1, "tree_stride")
        assert failed and geo["logC"] == 3 and geo["E"] == 8
    # a unit starts at u V + mis: rung (a), n = 2 V + 1 at shift 1
    c = M.column_system(small=True)
    assert (2 * V + 1, 1, 1, "R") in M.column_rungs(itemsize)
    failed, geo = _fails(c, 2 * V + 1, itemsize, 1, "lo_plus_mis")
    assert failed and geo["mis"] == 1
    assert not _fails(c, 2 * V + 1, itemsize, 0, "lo_plus_mis")[0]
    # the last partial unit dropped: rung (a), n = 2 V + 1 at shift 0
    failed, geo = _fails(c, 2 * V + 1, itemsize, 0, "drop_last_partial")
    assert failed and geo["units"] == 3 and M.partial_widths(2 * V + 1, 0, itemsize) == (0, 1)
    assert not _fails(c, 2 * V, itemsize, 0, "drop_last_partial")[0]
    # ... and at three passes (the rung n = 2 MAX_C V + V + 1 exists for this)
    top = M.column_ns()[-1]
    failed, geo = _fails(c, top, itemsize, 0, "drop_last_partial")
    assert failed and geo["passes"] >= 3
