"""The ladders of tests/ladder_tt.py checked without a GPU: the limits are read from the sources, every generator holds the rungs
it claims, the exact data stay in the exact range, the references return the known answers (oracle.transpose round-trips,
oracle.triangular_solve and trsm_util.emulate at every lane count return x_true exactly), and the checkers bite: a correct
result passes, the same result corrupted the way a subtly wrong kernel would corrupt it fails.

  corruption                                              caught by
  two equal-column entries swapped (stability)            transpose_violations: columns (= source rows) and value bits
  one row offset off by one                               transpose_violations: row offsets
  one element outside a scaled view changed               the whole-base comparison of scale_data
  the first stored diagonal used instead of the last      exact_violations (the earlier entry holds NaN)
  one dependency dropped                                  exact_violations (no value and no x is zero: the sum changes)
  one entry of the other triangle included                exact_violations (those entries hold NaN)
  one row solved a level early                            exact_violations (x is prefilled with NaN: the row reads it)
"""
import numpy as np
import pytest

import ladder_tt as T
import trsm_util as TU
from oracle import oracle


# =============================================================================================================== limits
def test_limits_are_read_from_the_sources():
    t = T.transpose_limits()
    assert t["tile"] == t["waves"] * t["rounds"] * 64 == 4096 and t["wave"] == 512 and t["round"] == 64
    assert (t["mark_stride"], t["xcds"], t["gap_lane"], t["gap_wave"], t["fill_items"], t["bits"]) == (512, 8, 8, 4096, 4, 8)
    assert (t["scale_blocks_per_cu"], t["scale_block"], t["scale_per_f32"], t["scale_per_f64"]) == (16, 256, 4, 2)
    s = T.trsv_limits()
    assert s["lane_steps"] == [(6, 4, 8), (24, 8, 16), (96, 16, 64)] and s["slots"] == {4: 4, 8: 4, 16: 2, 64: 1}
    assert (s["narrow"], s["max_run"], s["hist_levels"], s["kahn_narrow"], s["kahn_batch"]) == (128, 4096, 4096, 2048, 16)
    assert (s["coop_threads"], s["kahn_rows_per_block"], s["kahn_max_blocks"]) == (1024, 32, 512)
    assert [T.passes_of(n) for n in T.COLUMN_NS] == [1, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4] and T.passes_of(T.BYTE_N) == 4
    assert [T.lanes_of(z, 10) for z in (0, 60, 61, 240, 241, 960, 961)] == [4, 4, 8, 8, 16, 16, 64]
    assert [T.pipelined_pass(3, g) for g in (4, 8, 16, 64)] == [3072, 1536, 384, 48]


# ============================================================================================================ transpose
def test_column_and_entry_cases_hold_their_rungs():
    t = T.transpose_limits()
    cols = {c.name: c for c in T.column_cases()}
    assert [cols[f"n{n}"].n for n in T.COLUMN_NS] == list(T.COLUMN_NS)
    for n in T.COLUMN_NS:
        c = cols[f"n{n}"]
        assert {0, n - 1} <= set(c.colind.tolist()) and c.nnz > t["tile"] and c.nnz % t["tile"]
    for byte in range(4):
        c = cols[f"byte{byte}"].colind.astype(np.int64)
        others = c & ~(0xFF << (8 * byte))
        assert np.unique(others).size == 1 and np.unique(c).size == (256 if byte < 3 else 2) and cols[f"byte{byte}"].passes == 4
    ent = {c.name: c for c in T.entry_cases()}
    tile = t["tile"]
    for z in list(range(1, 10)) + [1023, 1024, 1025, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile + 1] + \
            [k * tile + o for k in (t["xcds"] - 1, t["xcds"], t["xcds"] + 1, 2 * t["xcds"] - 1, 2 * t["xcds"], 2 * t["xcds"] + 1)
             for o in (-1, 0, 1)]:
        assert ent[f"nnz{z}"].nnz == z
    assert ent["nnz0"].nnz == 0 and ent["nnz0"].m > 0 and ent["nnz0"].n > 0
    assert ent["m0"].m == 0 and ent["m0"].n > 0 and ent["m1"].m == 1 and ent["m1"].nnz > 0 and ent["m1_empty"].nnz == 0
    for c in list(cols.values()) + list(ent.values()):
        assert c.nnz < 2 ** 24 and np.array_equal(c.values(np.float32).astype(np.int64), np.arange(c.nnz))   # distinct values


def test_row_cases_hold_their_rungs():
    t = T.transpose_limits()
    tile = t["tile"]
    rows = {c.name: c for c in T.row_cases()}
    c = rows["start_at_tile"]
    assert {tile, 2 * tile} <= set(c.rowptr.tolist())                     # a row starts at a tile's first entry, one ends at its last
    c = rows["span3"]
    assert T.in_tile_starts(c, 1).size == 0 and T.in_tile_starts(c, 2).size == 0 and np.diff(c.rowptr).max() == 3 * tile
    for tl in (0, 1):
        assert {63, 64, 65, 511, 512, 513} <= set(T.in_tile_starts(rows["carries"], tl).tolist())
    for k in (t["mark_stride"] + 1, 2 * t["mark_stride"] + 1):
        c = rows[f"starts{k}"]
        first_row_of_next_tile = int(np.searchsorted(c.rowptr, tile, side="right")) - 1
        assert first_row_of_next_tile == k                                 # the marking loop walks j = 1 ... k
    c = rows["empties3000"]
    at = np.flatnonzero(c.rowptr[:-1] == 5)
    assert at.size == 3001 and (np.diff(c.rowptr)[at[:-1]] == 0).all() and np.diff(c.rowptr)[at[-1]] > 0
    c = rows["empties_tile_edge"]
    lens = np.diff(c.rowptr)
    assert lens[0] == 0 and lens[-1] == 0 and (c.rowptr[:-1] == tile).sum() == 11 and (lens[c.rowptr[:-1] == tile] == 0).sum() == 10
    c = rows["empties_trailing_full_tile"]
    assert c.nnz == tile and (c.rowptr[:-1] == tile).sum() == 600


def test_gap_and_bucket_cases_hold_their_rungs():
    t = T.transpose_limits()
    gaps = {c.name: c for c in T.gap_cases()}
    for g in T.GAP_LENS:
        inner, lead, trail = T.gap_lens(gaps[f"gap{g}"])
        assert lead == g and trail == g and set(T.GAP_LENS) <= set(inner.tolist()) and 0 in inner     # (0: a repeated column)
    for lim in (t["gap_lane"], t["gap_wave"]):
        assert {lim - 1, lim, lim + 1} <= set(T.GAP_LENS)
    assert set(range(1, 11)) | {63, 64, 65, 4098} <= set(T.GAP_LENS) and max(T.GAP_LENS) > 20 * t["gap_wave"]
    c = gaps["long_full"]
    inner, lead, trail = T.gap_lens(c)
    n_long = int((inner > t["gap_wave"]).sum()) + (lead > t["gap_wave"]) + (trail > t["gap_wave"])
    assert n_long == (c.n + 1) // (t["gap_wave"] + 1)                       # no matrix of n columns has more
    assert n_long <= c.n // t["long_div"] + t["long_slack"]                  # ... and the list has room for them
    assert int((T.gap_lens(gaps["long_few"])[0] > t["gap_wave"]).sum()) + 1 == 3
    b = {c.name: c for c in T.bucket_cases()}
    assert np.unique(b["one_column"].colind).size == 1 and b["one_column"].nnz > 2 * t["tile"]
    assert sorted(b["digits_once"].colind.tolist()) == list(range(256))
    c2 = b["digits_once_two_passes"].colind
    assert sorted((c2 & 255).tolist()) == list(range(256)) and sorted((c2 >> 8).tolist()) == list(range(256))
    d = b["duplicates_on_edges"]
    assert d.m == 1
    for edge in (t["round"], t["wave"], t["tile"]):
        assert d.colind[edge - 1] == d.colind[edge]
    st = T.state_cases()
    assert [c.passes for c in st] == [4, 1, 2, 2] and st[1].nnz < t["tile"] < st[0].nnz
    assert len(T.ALIGN_SHIFTS) == 19 and T.alignment_case().nnz > 2 * t["tile"]


def _stable_transpose(case, dtype):
    rows = np.repeat(np.arange(case.m), np.diff(case.rowptr))
    order = np.argsort(case.colind, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(case.colind, minlength=case.n))]).astype(np.int32)
    return rp, rows[order].astype(np.int32), case.values(dtype)[order]


def test_oracle_transpose_is_the_stable_sort_and_round_trips():
    picks = [c for c in T.entry_cases() + T.row_cases() + T.gap_cases() + T.bucket_cases()
             if c.name in ("nnz4097", "m0", "nnz0", "carries", "empties3000", "gap9", "duplicates_on_edges", "one_column")]
    assert len(picks) == 8
    for c in picks:
        for dt in (np.float32, np.float64):
            ref = T.transpose_reference(c, dt)
            assert not T.transpose_violations(c, ref, _stable_transpose(c, dt)), c.name
            back = oracle.transpose((c.n, c.m), ref[0], ref[1], ref[2])
            assert np.array_equal(back[0], c.rowptr)                          # (A^T)^T: A's rows, columns sorted, ties in order
            rows = np.repeat(np.arange(c.m), np.diff(c.rowptr))
            order = np.lexsort((np.arange(c.nnz), c.colind, rows))
            assert np.array_equal(back[1], c.colind[order]) and np.array_equal(back[2], c.values(dt)[order])


def test_transpose_checker_fails_on_seeded_mutations():
    c = [x for x in T.bucket_cases() if x.name == "duplicates_on_edges"][0]
    ref = T.transpose_reference(c, np.float32)
    assert T.transpose_violations(c, tuple(a.copy() for a in ref), ref) == []
    rp, ci, va = (a.copy() for a in ref)
    col = int(c.colind[T.transpose_limits()["wave"]])
    p = int(rp[col])                                                           # two entries of one column (one source row): swapped
    assert rp[col + 1] - p >= 2 and ci[p] == ci[p + 1]
    va[[p, p + 1]] = va[[p + 1, p]]
    assert any("values" in m for m in T.transpose_violations(c, (rp, ci, va), ref))
    c2 = [x for x in T.row_cases() if x.name == "carries"][0]
    ref2 = T.transpose_reference(c2, np.float64)
    rp, ci, va = (a.copy() for a in ref2)
    q = int(np.flatnonzero(np.diff(rp) >= 2)[0])
    ci[[rp[q], rp[q] + 1]] = ci[[rp[q] + 1, rp[q]]]                            # equal column, different source rows: swapped
    va[[rp[q], rp[q] + 1]] = va[[rp[q] + 1, rp[q]]]
    assert T.transpose_violations(c2, (rp, ci, va), ref2)
    rp = ref2[0].copy()
    rp[17] += 1
    assert any("row offsets" in m for m in T.transpose_violations(c2, (rp, ref2[1], ref2[2]), ref2))


def test_scale_cases_and_data():
    t = T.transpose_limits()
    cases = T.scale_cases(256)
    assert {(vt, n, off) for vt in ("f32", "f64") for n in range(71) for off in range(5)} <= set(cases)
    for vt, per in (("f32", 4), ("f64", 2)):
        full = 256 * t["scale_blocks_per_cu"] * t["scale_block"] * per
        assert {(vt, n, 1) for n in (full - 1, full, full + 1, full + 5, 2 * full + 3)} <= set(cases)
    base, want = T.scale_data(9, 3, np.float32)
    assert base.size == 9 + 3 + 5 and np.array_equal(want[:3], base[:3]) and np.array_equal(want[12:], base[12:])
    assert np.array_equal(want[3:12], base[3:12] * np.float32(-1.75)) and np.abs(base).max() <= 8
    assert np.array_equal(base, np.round(base))


# ===================================================================================================== triangular solve
def _strict(sysm):
    rows = np.repeat(np.arange(sysm.m), np.diff(sysm.rowptr))
    return rows, (sysm.colind > rows) if sysm.upper else (sysm.colind < rows)


def _check_structure(sysm):
    """What every system claims: the designed levels are the levels by definition, with the designed widths; entry kinds match
    the triangle; the decorations hold NaN; the exact range holds."""
    lev = T.levels_of(sysm.rowptr, sysm.colind, sysm.m, sysm.upper)
    assert np.array_equal(lev, sysm.level) and np.bincount(lev).tolist() == sysm.widths
    rows, strict = _strict(sysm)
    diag = sysm.colind == rows
    assert np.array_equal(sysm.kind == 1, strict) and np.array_equal(sysm.kind >= 2, diag)
    ev = sysm.exact_values
    assert np.isnan(ev[sysm.kind == 0]).all() and np.isnan(ev[sysm.kind == 3]).all()          # other triangle, earlier diagonal
    assert np.isin(ev[strict], [-2, -1, 1, 2]).all() and np.isin(sysm.x_true, [-3, -2, -1, 1, 2, 3]).all()
    if sysm.unit:
        assert np.isnan(ev[diag]).all()
    else:
        assert np.isin(ev[sysm.kind == 2], [0.5, 1, 2, 4]).all()
        assert np.array_equal(np.bincount(rows[sysm.kind == 2], minlength=sysm.m), np.ones(sysm.m))
    # the diagonal entry that is read is the LAST stored one of its row
    last_diag = np.full(sysm.m, -1)
    np.maximum.at(last_diag, rows[diag], np.flatnonzero(diag))
    assert np.array_equal(np.sort(last_diag[last_diag >= 0]), np.flatnonzero(sysm.kind == 2))
    anyorder = np.bincount(rows[strict], weights=np.abs(ev[strict] * sysm.x_true[sysm.colind[strict]]), minlength=sysm.m)
    assert anyorder.max(initial=0) < 2 ** 22 and np.array_equal(sysm.b * 4, np.round(sysm.b * 4)) and np.abs(sysm.b).max() < 2 ** 24
    assert sysm.alpha in T.ALPHAS and T.lanes_of(sysm.nnz, sysm.m) == sysm.lanes
    assert np.isfinite(sysm.random_values).all()


@pytest.mark.parametrize("lanes", [4, 8, 16, 64])
def test_row_shape_systems_hold_every_shape_where_they_claim(lanes):
    G = lanes
    assert set(T.strict_counts(G)) == set(range(0, 2 * G + 3)) | {3 * G - 1, 3 * G, 3 * G + 1, 300}
    for upper in (False, True):
        for unit in (False, True):
            sysm = T.shape_system(lanes, upper, unit)
            _check_structure(sysm)
            shapes = {s.name: s for s in T.row_shapes(lanes, unit)}
            widths, k = T.shape_widths(lanes, unit)
            narrow = T.trsv_limits()["narrow"]
            assert max(widths[1:1 + k]) < narrow <= widths[1 + k] and max(widths[2 + k:]) < narrow
            for lo, hi in ((1, 1 + k), (1 + k, 2 + k), (2 + k, 2 + 2 * k)):
                assert set(sysm.shape_of[(sysm.level >= lo) & (sysm.level < hi)]) == set(shapes)
            rows, strict = _strict(sysm)
            n_strict = np.bincount(rows[strict], minlength=sysm.m)
            slots, pairs = set(), set()
            for r in np.flatnonzero(sysm.level >= 1):
                s = shapes[sysm.shape_of[r]]
                seg = slice(sysm.rowptr[r], sysm.rowptr[r + 1])
                dpos = np.flatnonzero(sysm.colind[seg] == r).tolist()
                want = [sysm.rowptr[r + 1] - sysm.rowptr[r] - 1 if p == "last" else p for p in s.dpos]
                assert n_strict[r] == s.strict and dpos == want, (r, s.name)
                if dpos:
                    slots.add((s.strict, T.slot_of(dpos[-1], G), dpos[-1] if dpos[-1] <= 2 * G else "far"))
                if len(dpos) == 2:
                    pairs.add((T.slot_of(dpos[0], G), T.slot_of(dpos[1], G)))
                    assert dpos[0] % G != dpos[1] % G                          # on different lanes
            assert (n_strict[sysm.level == 0] == 0).all()
            assert set(n_strict[sysm.level >= 1].tolist()) == set(T.strict_counts(G)) - {0}
            for s in (1, G + 1, 2 * G + 2):                                    # first, G - 1 | G, 2G - 1 | 2G: the edges of c0, c1, loop
                assert {(s, "c0", 0), (s, "c0", G - 1), (s, "c1", G), (s, "c1", 2 * G - 1), (s, "loop", 2 * G)} <= slots
            assert pairs == {("c0", "c1"), ("c1", "loop"), ("loop", "loop")}
            if unit:
                assert any(len(shapes[n].dpos) == 0 for n in set(sysm.shape_of[sysm.level >= 1]))
            # not sorted by level: the rows of the wide level are spread over the index range
            idx = np.flatnonzero(sysm.level == 1 + k)
            assert idx.min() < sysm.m // 4 and idx.max() > 3 * sysm.m // 4 and (np.diff(sysm.level) < 0).sum() > (sysm.level >= 1).sum() // 4
    lo_sys, up_sys = T.shape_system(lanes, False, False), T.shape_system(lanes, True, False)
    lens = np.diff(lo_sys.rowptr)                                              # the upper variant is the index mirror
    assert np.array_equal(np.diff(up_sys.rowptr), lens[::-1]) and np.array_equal(up_sys.level, lo_sys.level[::-1])
    r0 = lo_sys.m - 1
    assert np.array_equal(lo_sys.m - 1 - up_sys.colind[up_sys.rowptr[0]:up_sys.rowptr[1]],
                          lo_sys.colind[lo_sys.rowptr[r0]:lo_sys.rowptr[r0 + 1]])


def test_width_sequence_mean_and_kahn_systems_hold_their_rungs():
    t = T.trsv_limits()
    for lanes in (4, 8, 16, 64):
        sysm, P = T.width_system(lanes, 3, lanes in (8, 64), lanes in (16, 64))
        _check_structure(sysm)
        assert {1, 2, 3, 4, 5, t["narrow"] - 1, t["narrow"], t["narrow"] + 1, P - 1, P, P + 1, 2 * P + 1} <= set(sysm.widths)
        assert P == T.pipelined_pass(3, lanes)
    got = {}
    for limit, extra, lanes, sysm in T.mean_cases():
        _check_structure(sysm)
        assert sysm.nnz == limit * sysm.m + extra
        got[(limit, extra)] = T.lanes_of(sysm.nnz, sysm.m)
    assert got == {(6, 0): 4, (6, 1): 8, (24, 0): 8, (24, 1): 16, (96, 0): 16, (96, 1): 64}
    for i, widths in enumerate(T.SEQUENCES):
        sysm = T.sequence_system(i)
        _check_structure(sysm)
        assert sysm.widths == widths
    assert {len(w) for w in T.SEQUENCES} == {1, 2, 3, 4, 5} and T.NARROW_W < t["narrow"] <= T.WIDE_W
    assert {(a >= t["narrow"], b >= t["narrow"]) for w in T.SEQUENCES for a, b in zip(w, w[1:])} == \
        {(False, False), (False, True), (True, False), (True, True)}
    names = [n for n, _ in T.kahn_cases()]
    K, batch, edge = t["kahn_narrow"], t["kahn_batch"], t["kahn_rows_per_block"] * t["kahn_max_blocks"]
    assert {K - 1, K, K + 1} <= set(dict(T.kahn_cases())["frontiers"])
    for k in (batch - 1, batch, batch + 1):
        assert dict(T.kahn_cases())[f"wide{k}"] == [K] * k + [3]
    assert {"m1", "m31", "m32", "m33", f"m{edge - 1}", f"m{edge}", f"m{edge + 1}"} <= set(names)
    for i in (0, 4, 5, 6, 7):
        _check_structure(T.kahn_system(i))
        assert T.kahn_system(i).m == sum(T.kahn_cases()[i][1])


def test_long_runs_and_what_the_plan_must_report():
    t = T.trsv_limits()
    assert T.groups_of([3, 3, 130, 130, 5, 200, 1], 128) == [(0, 2, False), (2, 3, True), (3, 4, True), (4, 5, False),
                                                              (5, 6, True), (6, 7, False)]
    assert T.groups_of([127], 128) == [(0, 1, False)] and T.groups_of([128], 128) == [(0, 1, True)]
    launches = {}
    for i, (name, widths) in enumerate(T.long_run_cases()):
        sysm = T.long_run_system(i)
        _check_structure(sysm)
        pi = T.predicted_info(sysm.rowptr, sysm.colind, sysm.m, sysm.upper)
        assert pi["levels"] == len(widths) and pi["max_level_width"] == max(widths) and pi["lanes_per_row"] == 4
        launches[name] = (pi["launches_per_solve"],
                          T.predicted_info(sysm.rowptr, sysm.colind, sysm.m, sysm.upper, coop=False)["launches_per_solve"])
    run, hist = t["max_run"], t["hist_levels"]
    assert launches == {f"wide_then_{run}": (1, 2), f"wide_then_{run + 1}": (2, 2), f"{run}_then_wide": (1, 2),
                        f"{run + 1}_then_wide": (2, 2), **{f"chain{k}": (1, 1) for k in range(hist - 1, hist + 3)}}
    s = T.sequence_system(7)                                                   # [130, 3, 130]
    assert T.predicted_info(s.rowptr, s.colind, s.m, s.upper, narrow=100000)["launches_per_solve"] == 1
    assert T.predicted_info(s.rowptr, s.colind, s.m, s.upper, coop=False)["launches_per_solve"] == 3


# ------------------------------------------------------------------------------------------------- references and checkers
def _host_solve(sysm, mutation=None, row=None):
    """The solve by levels in float64 with x prefilled with NaN (as the GPU tests prefill it), optionally wrong in one row."""
    rp, ci, v = sysm.rowptr, sysm.colind, sysm.exact_values
    x = np.full(sysm.m, np.nan)
    order = np.argsort(sysm.level, kind="stable").tolist()
    if mutation == "level_early":                                               # solved with the rows of the level before its own
        order.remove(row)
        order.insert(int(np.searchsorted(np.sort(sysm.level), sysm.level[row] - 1, side="left")), row)
    for r in order:
        dot, d, first_d, dropped = 0.0, 0.0, None, False
        for p in range(rp[r], rp[r + 1]):
            c = ci[p]
            strict = (c > r) if sysm.upper else (c < r)
            if strict:
                if r == row and mutation == "drop_dependency" and not dropped:
                    dropped = True
                    continue
                dot += v[p] * x[c]
            elif c == r:
                first_d = v[p] if first_d is None else first_d
                d = v[p]
            elif r == row and mutation == "other_triangle":
                dot += v[p] * x[c]
        if r == row and mutation == "first_diagonal":
            d = first_d
        t = sysm.b[r] - sysm.alpha * dot
        x[r] = t if sysm.unit else t / (sysm.alpha * d)
    return x


@pytest.mark.parametrize("lanes", [4, 8, 16, 64])
def test_references_return_x_true_and_the_checker_bites(lanes):
    for upper, unit in ((False, False), (True, True), (True, False)):
        sysm = T.shape_system(lanes, upper, unit)
        assert T.exact_violations(_host_solve(sysm), sysm) == []
        M = T.as_scipy(sysm, sysm.exact_values)
        for dt in (np.float32, np.float64):
            x = oracle.triangular_solve((sysm.m, sysm.m), sysm.rowptr, sysm.colind, sysm.exact_values.astype(dt),
                                        sysm.b.astype(dt), upper=upper, unit=unit,
                                        scale_a=None if sysm.alpha == 1.0 else sysm.alpha)
            assert T.exact_violations(x, sysm) == [], (upper, unit, dt)
        if (upper, unit) != (True, False):
            X = TU.emulate(M, T.block_rhs(sysm), upper, unit, np.float32, scale_a=None if sysm.alpha == 1.0 else sysm.alpha,
                           lanes=lanes)
            assert T.exact_violations(X, sysm) == [] and X.shape == (sysm.m, 3)
        if (upper, unit) != (False, False):
            continue
        shapes = {s.name: s for s in T.row_shapes(lanes, unit)}
        pair = int(np.flatnonzero([len(shapes.get(n, T.Shape(1)).dpos) == 2 for n in sysm.shape_of])[0])
        padded = int(np.flatnonzero((sysm.level >= 1) & (np.bincount(
            np.repeat(np.arange(sysm.m), np.diff(sysm.rowptr))[sysm.kind == 0], minlength=sysm.m) > 0))[0])
        deep = int(np.flatnonzero(sysm.level == 2)[0])
        for mutation, row in (("first_diagonal", pair), ("drop_dependency", deep), ("other_triangle", padded), ("level_early", deep)):
            bad = T.exact_violations(_host_solve(sysm, mutation, row), sysm)
            assert bad and f"first at [{row}]" in bad[0], (mutation, row, bad)
    small = T.sequence_system(6)                                                # emulate at EVERY lane count on a small system
    for g in (4, 8, 16, 64):
        X = TU.emulate(T.as_scipy(small, small.exact_values), small.b[:, None], small.upper, small.unit, np.float64,
                       scale_a=None if small.alpha == 1.0 else small.alpha, lanes=g)
        assert T.exact_violations(X[:, 0], small) == []
