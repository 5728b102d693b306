"""The tile ladders of tests/ladder_sliced.py checked without a GPU: the restated tiling finds every advertised rung in every
family, the restatement agrees with what the existing GPU tests pin (22 slices of 96 for an asked width of 100 on 2 111
columns; the exception rule of test_gpu_spmv._enc8_exceptions), the integer data stay in the exact range, and a host model
of expand -> reduce passes the exact check as it is and fails it for every seeded mistake on the family built for it:

  mistake                                              family
  the last block of a run dropped                      runs
  one group too few / too many at a batch tail         groups (UB = 4 and 8)
  a duplicate added without its flag (lost addend)     dups
  an exception dropped / added by every K part         row_codes (one-byte codes, K = 2)
  a slice's first / last column off by one             col_edges
  a pad row landing on H - 1                           row_edges
  a K part boundary off by one group                   groups (K = 3)
"""
import numpy as np
import pytest

import ladder as L
import ladder_sliced as LS

VTS = ["f32", "f64"]


def _exact(fam):
    values, x = LS.exact_data(fam)
    assert set(np.unique(values)) <= {-1.0, 1.0} and set(np.unique(x)) <= {-2.0, -1.0, 1.0, 2.0}
    ref, _ = L.spmv_reference(fam.rowptr, fam.colind, values, x, fam.shape)
    return values, x, ref


def _model_check(fam, values, x, ref, **kw):
    y = LS.model_spmv((fam.rowptr, fam.colind), values, x, fam.tiling(), **kw)
    L.check_exact(fam.vt, L.cast(fam.vt, y), ref, f"{fam.name} {kw}")


def _fails(fam, values, x, ref, **kw):
    with pytest.raises(AssertionError, match="differ from the exact result"):
        _model_check(fam, values, x, ref, **kw)


# ------------------------------------------------------------------------------------------------------- restatement
def test_constants_come_from_the_sources():
    c = LS.constants()
    assert c["PB_GRP"] == 256 and LS.blk("f32") == 32 and LS.blk("f64") == 16 and LS.gblk("f32") == 8 and LS.gblk("f64") == 16
    assert c["HOT_WIN"] == 64 * c["HOT_EPL"] and c["PB_STAGE_SP"] < c["PB_STAGE_MAX_S"] and c["PB_EXC_CAP"] > 1
    assert c["PB_LDS_BYTES"] % 1024 == 0


def test_pick_tiling_and_bin_height():
    assert LS.pick_tiling(2111, 100) == (22, 96)                     # not 100: what test_spmv_sliced_many_tiles pins
    assert LS.pick_tiling(6400, 64) == (100, 64)
    assert LS.pick_tiling(20480, 20480) == (1, 20480) and LS.pick_tiling(20481, 20480) == (2, 10244)
    assert LS.pick_tiling(40961, 20480) == (3, 13656)
    env = {"SPBLAS_GFX950_SLICE_COLS": "100", "SPBLAS_GFX950_SLICE_ROWS": "64"}
    for vt in VTS:
        t = LS.tiling(vt, 1500, 2111, 20000, env)
        assert (t.S, t.W, t.H, t.NB) == (22, 96, 64, 24)
    # SLICE_ROWS is taken only below the rows a bin may hold: 80 KiB / 4 wave-bins / sizeof(T) - 64
    env = {"SPBLAS_GFX950_SLICE_COLS": "64", "SPBLAS_GFX950_SLICE_ROWS": "4000"}
    assert LS.tiling("f32", 8000, 6400, 14000, env).H == 4000
    t = LS.tiling("f64", 8000, 6400, 14000, env)
    assert t.max_rows == 2496 and t.H == 2000 and t.NB == 4           # 4 bins of at most 2 496 rows: 2 000 each
    assert LS.tiling("f64", 1000, 256, 100, {"SPBLAS_GFX950_SLICE_ROWS": "1000", "SPBLAS_GFX950_PB_RWAVES": "8"}).H == 1000
    assert LS.tiling("f64", 2000, 256, 100, {"SPBLAS_GFX950_SLICE_ROWS": "1300", "SPBLAS_GFX950_PB_RWAVES": "8"}).H == 1000
    # value-free tiles: the height comes from PB_VF_ROWS (SLICE_ROWS switches them off)
    vf = {"SPBLAS_GFX950_PB_VFREE": "2", "SPBLAS_GFX950_PB_VF_ROWS": "37", "SPBLAS_GFX950_SLICE_COLS": "64"}
    assert LS.tiling("f32", 1000, 256, 5000, vf).H == 37 and LS.tiling("f32", 1000, 256, 5000, vf).rw == 1
    # the slice-aligned geometry: S between 0.9 x and 1 x the CU count is rounded up to it (fp64: 160 KiB slices)
    t = LS.tiling("f64", 1000, 245 * 20480, 1000, {}, cus=256)
    assert t.slice_aligned and t.S == 256 and t.W == LS.cdiv(LS.cdiv(245 * 20480, 256), 4) * 4
    assert not LS.tiling("f32", 1000, 245 * 20480, 1000, {}, cus=256).slice_aligned


def test_exception_rule_agrees_with_the_one_in_test_gpu_spmv():
    from test_gpu_spmv import _enc8_exceptions
    rng = np.random.default_rng(23)                                  # the matrix of test_spmv_sliced_row_encodings
    m, n, W, H = 8000, 6400, 64, 4000
    lens = np.full(m, 2)
    lens[rng.random(m) < 0.1] = 0
    lens[4321] = 300
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    colind = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    for vt in VTS:
        t = LS.tiling("f32", m, n, int(rowptr[-1]), {"SPBLAS_GFX950_SLICE_COLS": str(W), "SPBLAS_GFX950_SLICE_ROWS": str(H)})
        assert (t.S, t.W, t.H, t.NB) == (100, W, H, 2)
        t.vt = vt                                                    # (that test restates both block sizes at H = 4 000)
        theirs = _enc8_exceptions(rowptr, colind, W, H, LS.blk(vt))
        ours = LS.enc8_exceptions(rowptr, colind, t)
        assert ours.tolist() == [theirs[b] for b in range(t.NB)] and ours.max() > 0


@pytest.mark.parametrize("vt", VTS)
def test_row_map_and_variable_bin_families(vt):
    win = L.thresholds()["window_" + vt]
    fam = LS.hub_len(vt)                                     # PB_HUB_LEN +- 1 under variable bins
    p = fam.predicted()
    lens = np.diff(fam.rowptr)
    A = LS.HUB_LEN_ASKED
    assert A > win and {A - 1, A, A + 1} <= set(lens.tolist()) and p["variable_bins"] == 1 and p["tiled_rows"] == fam.shape[0]
    assert p["hub_len"] == A and p["hub_rows"] == 1 and p["placed_entries"] == fam.nnz - (A + 1)
    fam = LS.split_rows(vt)                                  # pieces of PB_SPLIT_LEN
    Lp = LS.SPLIT_LEN_ASKED
    rp, pieces, split = LS.row_map(vt, fam.rowptr, fam.env)
    lens = np.diff(fam.rowptr)
    assert split == Lp and [int(lens[r]) for r in fam.meta["at"]] == [2 * Lp - 1, 2 * Lp + 1, 3 * Lp - 1, 3 * Lp + 1, 9 * Lp - 1, 9 * Lp + 1]
    assert [int(pieces[r]) for r in fam.meta["at"]] == [2, 3, 3, 4, 9, 10] and pieces[50] == pieces[51] == 1 and pieces[0] == 1
    assert np.diff(rp).max() == Lp and np.diff(rp).sum() == fam.nnz
    t, _, binrow, hub, mapped = LS.plan_rows(vt, fam.rowptr, fam.shape, fam.env)
    first = np.cumsum(pieces) - pieces
    for r in fam.meta["at"][4:]:                             # 9 and 10 pieces, bins of 8 rows: they fall into different bins
        b = np.searchsorted(binrow, [first[r], first[r] + pieces[r] - 1], side="right")
        assert b[0] != b[1], r
    p = fam.predicted()
    assert mapped and hub == 0 and p["tiled_rows"] == int(pieces.sum()) and p["variable_bins"] == 1 and p["placed_entries"] == fam.nnz
    fam = LS.compact_rows(vt)                                # empty rows out
    lens = np.diff(fam.rowptr)
    rp, pieces, split = LS.row_map(vt, fam.rowptr, fam.env)
    assert split == 0 and np.array_equal(pieces, (lens > 0).astype(int)) and (np.diff(rp) > 0).all()
    z = np.flatnonzero(lens == 0)                            # the stretches of empty rows: (first row, length)
    starts = z[np.concatenate([[True], np.diff(z) > 1])]
    ends = z[np.concatenate([np.diff(z) > 1, [True]])]
    runs_ = [(int(a), int(b - a + 1)) for a, b in zip(starts, ends)]
    assert runs_[0][0] == 0 and runs_[0][1] > 1                                          # leading
    assert runs_[-1][0] + runs_[-1][1] == lens.size and runs_[-1][1] > 1                 # trailing
    assert any(n_ > 16 for a, n_ in runs_[1:-1])                                         # a stretch longer than a bin
    assert sum(1 for a, n_ in runs_[1:-1] if n_ == 1) >= 10                              # alone between full rows
    p = fam.predicted()
    assert p["tiled_rows"] == int((lens > 0).sum()) and p["n_bins"] == LS.cdiv(p["tiled_rows"], 16) and p["variable_bins"] == 1
    # a family that pins the arithmetic bins would leave them without the pin: rows of 257 entries among rows of 1
    fam = LS.dups(vt)
    env = {k: v for k, v in fam.env.items() if k != "SPBLAS_GFX950_PB_VARBINS"}
    assert fam.predicted()["variable_bins"] == 0 and LS.predicted_info(vt, fam.rowptr, fam.colind, fam.shape, env)["variable_bins"] == 1


# ---------------------------------------------------------------------------------------------------------- the rungs
@pytest.mark.parametrize("vt", VTS)
def test_runs_family_holds_every_run_length_in_every_position(vt):
    fam = LS.runs(vt)
    t = fam.tiling()
    cnt = LS.tile_counts(fam.rowptr, fam.colind, t)
    assert (t.S, t.W, t.H) == (4, 64, 37) and np.array_equal(cnt, fam.meta["spec"])
    b = LS.blk(vt)
    assert LS.run_counts(vt) == [0, 1, 3, 4, 5, b - 1, b, b + 1, 2 * b - 1, 2 * b + 1]
    for c, pos in fam.rungs:
        assert (cnt[fam.meta["pos_slice"][pos]] == c).any(), (c, pos)
    assert len(fam.rungs) == 30
    assert cnt[-1, -1] == 0 and cnt[1:, -1].sum() == 0 and cnt[0, -2] == 0      # the ends of A' and of P are empty tiles
    assert LS.compact_stream_entries(cnt) > cnt.sum()                          # runs that are no multiple of 4
    p = fam.predicted()
    assert p["placed_entries"] == fam.nnz and p["hub_rows"] == 0 and p["n_bins"] == cnt.shape[1]
    assert p["expand_blocks"] == int(LS.cdiv(cnt, b).sum()) and p["reduce_blocks"] % LS.gblk(vt) == 0


@pytest.mark.parametrize("vt", VTS)
def test_groups_family_holds_every_group_count(vt):
    fam = LS.groups(vt)
    t = fam.tiling()
    cnt = LS.tile_counts(fam.rowptr, fam.colind, t)
    got = LS.groups_per_bin(vt, cnt)
    grp, b = LS.constants()["PB_GRP"], LS.blk(vt)
    assert [int(g) for g in got] == [g for g, _ in fam.meta["spec"]]
    assert [int(e) for e in cnt.sum(axis=0)] == [g * grp - d for g, d in fam.meta["spec"]]
    have = set(int(g) for g in got)
    assert have == set(range(35))
    for ub in (1, 2, 4, 8):                              # two batches of UB groups in flight, loads past the end clamped
        assert {0, 1, ub - 1, ub + 1, 2 * ub - 1, 2 * ub + 1, 4 * ub - 1, 4 * ub + 1} <= have
    for g in range(1, 35):
        assert {d for gg, d in fam.meta["spec"] if gg == g} == {0, 1, b, b + 1}, g
    assert fam.nnz < 700_000 and fam.predicted()["reduce_blocks"] == int(got.sum()) * LS.gblk(vt)
    for rw in ("4", "8"):                                # the asked height holds for either workgroup shape
        assert fam.tiling({"SPBLAS_GFX950_PB_RWAVES": rw}).H == 500


@pytest.mark.parametrize("vt", VTS)
@pytest.mark.parametrize("case", list(LS.COL_EDGE_CASES))
def test_column_edge_family(vt, case):
    fam = LS.col_edges(vt, case)
    t = fam.tiling()
    n, w_ask, empty = LS.COL_EDGE_CASES[case]
    assert (t.S, t.W) == (fam.meta["S"], fam.meta["W"]) and t.NB == 3
    cols = set(fam.colind.tolist())
    want = {c for s in range(t.S + 1) for c in (s * t.W - 1, s * t.W, s * t.W + 1) if 0 <= c < n} | {0, n - 1}
    want = {c for c in want if c // t.W not in empty}
    assert cols == want == fam.rungs
    cnt = LS.tile_counts(fam.rowptr, fam.colind, t)
    for s in range(t.S):
        assert (cnt[s] > 0).all() != (s in empty), s      # every bin meets every slice that is not left empty
    last_width = n - (t.S - 1) * t.W
    if case == "last_slice_1_col":
        assert last_width == 1 and t.W == 64
    if case == "last_slice_w_minus_1":
        assert last_width == t.W - 1
    if case == "asked_100_gets_96":
        assert (t.S, t.W) == (22, 96) and w_ask == 100
    if case == "empty_slices":
        assert empty == (0, 5, 9) and t.S == 10
    if case.startswith("natural"):
        assert "SPBLAS_GFX950_SLICE_COLS" not in fam.env and t.S == LS.cdiv(n, 20480) and t.W == LS.cdiv(LS.cdiv(n, t.S), 4) * 4


@pytest.mark.parametrize("vt", VTS)
@pytest.mark.parametrize("case", list(LS.ROW_EDGE_CASES))
def test_row_edge_family(vt, case):
    fam = LS.row_edges(vt, case)
    t = fam.tiling()
    k, d, empty = LS.ROW_EDGE_CASES[case]
    m, H = fam.shape[0], t.H
    assert H == 64 and m == k * H + d and t.NB == LS.cdiv(m, H)
    lens = np.diff(fam.rowptr)
    for b in range(t.NB):
        for lr in (0, H - 1):
            r = b * H + lr
            if r < m:
                assert (lens[r] > 0) != (b in empty), (b, lr)
    cnt = LS.tile_counts(fam.rowptr, fam.colind, t)
    assert [b for b in range(t.NB) if cnt[:, b].sum() == 0] == list(empty)
    if d == 1:
        assert m - (t.NB - 1) * H == 1 and lens[m - 1] > 0            # a last bin of one row, and it holds entries


@pytest.mark.parametrize("vt", VTS)
def test_duplicates_family_places_every_multiplicity(vt):
    fam = LS.dups(vt)
    t = fam.tiling()
    b, grp, H = LS.blk(vt), LS.constants()["PB_GRP"], fam.meta["H"]
    assert t.H == H and t.S == 2
    bn_of, s_of, r_of, order = LS._tile_entries(fam.rowptr, fam.colind, t)
    seen = set()
    for bn, (c, name, o) in enumerate(fam.meta["spec"]):
        e = order[(bn_of[order] == bn) & (s_of[order] == 0)]           # the run of slice 0, in stream order
        pos = np.flatnonzero(r_of[e] == o)                              # positions of the duplicated row in the bin's stream
        assert pos.size == c and pos[0] == o and pos[-1] == o + c - 1, (c, name)
        if name.startswith("quad"):
            assert o % 4 == int(name[-1])
        if name == "block_edge" and c > 1:
            assert pos[0] // b != pos[-1] // b
        if name == "group_edge" and c > 1:
            assert pos[0] // grp != pos[-1] // grp
        if name == "next_slice":
            e1 = order[(bn_of[order] == bn) & (s_of[order] == 1)]
            assert (r_of[e1] == o).sum() == c
            if c <= b:                                                    # ... and both runs lie in the bin's first group
                assert LS.cdiv(c, b) * b + c <= grp
        if name == "two_rows":
            assert (r_of[e] == o + 1).sum() == c
        seen.add((c, name))
    assert seen == fam.rungs == {(c, nm) for c in LS.DUP_COUNTS for nm in list(LS.dup_placements(vt)) + ["next_slice", "two_rows"]}
    assert LS.DUP_COUNTS == (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257) and np.diff(fam.rowptr).max() == 2 * 257


@pytest.mark.parametrize("vt", VTS)
def test_row_code_family_holds_the_exception_counts(vt):
    cap = LS.constants()["PB_EXC_CAP"]
    for overflow in (False, True):
        fam = LS.row_codes(vt, overflow)
        t = fam.tiling()
        assert t.H == fam.meta["H"] == (4000 if vt == "f32" else t.max_rows) and t.NB == len(fam.meta["spec"]) and t.S == 16
        exc = LS.enc8_exceptions(fam.rowptr, fam.colind, t)
        for bn, e in enumerate(fam.meta["spec"]):
            if isinstance(e, int):
                assert exc[bn] == e, (bn, e, exc)
        assert set(int(e) for e in exc[2:]) == fam.rungs == {0, 1, cap - 1, cap} | ({cap + 1} if overflow else set())
        assert (exc.max() > cap) == overflow
        # bin 0: one block with the advances 0, 1, 254, 255, 256, 509, 510, 511; bin 1: a block whose base is row H - 1
        r0 = np.repeat(np.arange(t.m), np.diff(fam.rowptr))
        first = r0[r0 < t.H]
        assert np.diff(first).tolist() == list(LS.ROW_ADVANCES) and 0 < exc[0] <= cap
        assert (r0 == 2 * t.H - 1).sum() == 2 and exc[1] == 0


@pytest.mark.parametrize("vt", VTS)
def test_skew_span_hub_and_slice_aligned_families(vt):
    cus = 256
    fam = LS.skew_cols(vt)
    t = fam.tiling()
    cnt = LS.tile_counts(fam.rowptr, fam.colind, t)
    assert cnt.sum(axis=1).max() * t.S > 3 * cnt.sum() and cnt.sum(axis=1).argmax() == 3
    p = fam.predicted(cus=cus)
    heavy = int(LS.cdiv(cnt[3], LS.blk(vt)).sum())
    assert p["expand_items"] > t.S + heavy // max(LS.cdiv(p["expand_blocks"], 2 * cus), 4 * t.W // LS.blk(vt)) - 1   # parts
    assert p["reduce_items"] == 0
    fam = LS.skew_rows(vt)
    t = fam.tiling()
    per_group = LS.tile_counts(fam.rowptr, fam.colind, t).sum(axis=0).reshape(-1, 4).sum(axis=1)
    assert per_group.argmax() == 1 and per_group.max() * per_group.size > 3 * per_group.sum() and per_group.max() > 24576
    p = fam.predicted(cus=cus)
    assert p["reduce_items"] == per_group.size - 1 + 2 and p["expand_items"] == 0      # the heavy group in two parts
    for span in LS.BIN_SPANS:
        fam = LS.bin_span_family(vt, span)
        assert LS.bin_span(fam.rowptr, fam.tiling()) == span == fam.meta["span"] and fam.tiling().NB == 2
    assert LS.BIN_SPANS == (65535, 65536, 65537)
    fam = LS.hub_rows(vt)
    win = L.thresholds()["window_" + vt]
    lens = np.diff(fam.rowptr)
    assert {win - 1, win, win + 1} <= set(lens.tolist()) and lens.max() == win + 1
    p = fam.predicted()
    assert p["hub_rows"] == 2 == int((lens > win).sum()) and p["hub_len"] == win and p["placed_entries"] == fam.nnz - 2 * (win + 1)
    names = set()
    for f in LS.all_families(vt) + [LS.groups(vt)]:                   # nothing else has hub rows or a work list
        names.add(f.name)
        if f.name == "hot_split":
            continue                                                  # (its tiles are A_rest's: the test below)
        p = f.predicted()
        assert (p["hub_rows"] > 0) == (f.name in ("hub_rows", "hub_len")), f.name
        # (many_slices: 2 500 slices with less than one entry each on average -- three in one slice are 3 x the mean)
        assert (p["expand_items"] > 0) == (f.name in ("skew_cols", "many_slices")), f.name
        assert (p["reduce_items"] > 0) == (f.name == "skew_rows"), f.name
    assert len(names) == 16 + len(LS.COL_EDGE_CASES) + len(LS.ROW_EDGE_CASES)
    # many_slices: more slices than the staged scatter takes, and no more than a plan takes at all
    fam = LS.many_slices(vt)
    t = fam.tiling()
    assert LS.constants()["PB_STAGE_MAX_S"] < t.S == fam.meta["S"] <= 16384 and t.W == 4 and t.NB == 3
    cnt = LS.tile_counts(fam.rowptr, fam.colind, t)
    per_slice = cnt.sum(axis=1)
    assert (per_slice > 0).sum() > t.S // 2 and per_slice[0] > 0 and per_slice[-1] > 0 and (per_slice == 0).any()
    assert {0, fam.shape[1] - 1} <= set(fam.colind.tolist())
    # many_groups: the reduce list longer than 2 x the CUs, sorted under PB_LPT, with split groups
    for cus in (256, 304):
        fam = LS.many_groups(vt, cus)
        t, rp, binrow, hub, mapped = LS.plan_rows(vt, fam.rowptr, fam.shape, fam.env, cus)
        ngroups = LS.cdiv(t.NB, t.rw)
        assert t.variable_bins == 1 and not mapped and hub == 0 and ngroups > 2 * cus and t.NB > 2 * cus
        assert t.NB > LS.cdiv(fam.shape[0], t.H)                      # bins cut on the entry count as well as every H rows
        p = fam.predicted(cus=cus)
        assert p["reduce_items"] > ngroups and p["expand_items"] == 0  # more items than groups: some group is cut into parts
        assert fam.predicted({"SPBLAS_GFX950_PB_LPT": "0"}, cus)["reduce_items"] == p["reduce_items"] > 2 * cus
    if vt == "f64":
        fam = LS.slice_aligned(vt, cus)
        t = LS.tiling(vt, fam.shape[0], fam.shape[1], fam.nnz, fam.env, cus)
        assert t.slice_aligned and t.S == cus and 0.9 * cus <= LS.pick_tiling(fam.shape[1], t.max_cols)[0] < cus
        cnt = LS.tile_counts(fam.rowptr, fam.colind, t)
        assert (cnt.sum(axis=1) == 6).all() and fam.predicted(cus=cus)["expand_items"] == cus
        assert {0, fam.shape[1] - 1, t.W - 1, t.W} <= set(fam.colind.tolist())


@pytest.mark.parametrize("vt", VTS)
def test_hot_split_family_makes_the_sample_take_its_hot_columns(vt):
    fam = LS.hot_split(vt)
    win = LS.constants()["HOT_WIN"]
    pos = LS.hot_sample_positions(fam.nnz)
    assert pos.size >= fam.nnz // 16 - 32 and np.unique(pos).size == pos.size and (np.diff(pos.reshape(-1, 32)) == 1).all()
    cnt = np.bincount(fam.colind[pos], minlength=fam.shape[1])
    assert (cnt[list(LS.HOT_COLS)] >= 2).all() and np.delete(cnt, LS.HOT_COLS).max() <= 1     # it MUST take these, and only these
    assert LS.hot_columns(fam.colind, fam.shape[1]).tolist() == sorted(LS.HOT_COLS)
    rows = np.repeat(np.arange(fam.shape[0]), np.diff(fam.rowptr))
    hot_per_row = np.bincount(rows[np.isin(fam.colind, LS.HOT_COLS)], minlength=fam.shape[0])
    assert np.array_equal(hot_per_row, fam.meta["hot_per_row"])
    assert hot_per_row[:5].tolist() == [win - 1, win, win + 1, 2 * win - 1, 2 * win + 1]
    lens = np.diff(fam.rowptr)
    assert hot_per_row[5] == lens[5] > 0 and hot_per_row[6] == 0 < lens[6]                  # hot-only, cold-only
    assert hot_per_row[0] > 0 and hot_per_row[-1] > 0 and (lens[7:10] == 0).all()
    assert hot_per_row[11:201].sum() == 0 and lens[11:201].sum() > 0 and hot_per_row[201] > 0   # a long run without hot entries
    rest_rowptr, rest_colind = fam.meta["rest"]
    assert rest_rowptr[-1] == rest_colind.size == fam.nnz - hot_per_row.sum()
    p = LS.predicted_info(vt, rest_rowptr, rest_colind, fam.shape, fam.env)
    assert p["placed_entries"] == rest_colind.size and p["n_slices"] == 16 and p["n_bins"] == 4
    # a matrix without repeated columns has nothing to split
    assert LS.hot_columns(np.arange(5000) % 4999, 5000).size == 0


# ------------------------------------------------------------------------------------------------- the checkers bite
@pytest.mark.parametrize("vt", VTS)
def test_model_passes_and_seeded_mistakes_fail_runs_cols_rows_dups(vt):
    fam = LS.runs(vt)
    data = _exact(fam)
    _model_check(fam, *data)
    _model_check(fam, *data, ub=2, K=3)
    _fails(fam, *data, mistake="last_block_dropped")
    fam = LS.col_edges(vt, "asked_100_gets_96")
    data = _exact(fam)
    _model_check(fam, *data)
    _fails(fam, *data, mistake="first_column_off_by_one")
    _fails(fam, *data, mistake="last_column_off_by_one")
    fam = LS.row_edges(vt, "m_kH")
    data = _exact(fam)
    _model_check(fam, *data)
    _fails(fam, *data, mistake="pad_on_last_row")
    fam = LS.dups(vt)
    data = _exact(fam)
    _model_check(fam, *data)
    _model_check(fam, *data, enc8=True, K=2)
    _fails(fam, *data, mistake="duplicate_without_flag")


@pytest.mark.parametrize("vt", VTS)
def test_model_passes_and_seeded_mistakes_fail_groups(vt):
    fam = LS.groups(vt)
    data = _exact(fam)
    _model_check(fam, *data)
    for ub in (4, 8):
        _fails(fam, *data, ub=ub, mistake="batch_tail_one_group_short")
        _fails(fam, *data, ub=ub, mistake="batch_tail_one_group_more")
    _model_check(fam, *data, ub=1, K=3)
    _fails(fam, *data, K=3, mistake="part_boundary_off_by_one")


@pytest.mark.parametrize("vt", VTS)
def test_model_passes_and_seeded_mistakes_fail_row_codes(vt):
    fam = LS.row_codes(vt)
    data = _exact(fam)
    _model_check(fam, *data, enc8=True)
    _model_check(fam, *data, enc8=True, K=2)
    _fails(fam, *data, enc8=True, mistake="exception_dropped")
    _fails(fam, *data, enc8=True, K=2, mistake="exception_by_every_part")
