"""CPU: the window ladder of the hot-column split (tests/ladder_hot.py) holds what it claims.  The host model of the multiply
equals a plain float64 CSR product on every family, every family reaches the rung it is named for (asserted from the
restated inspect, not from the specification it was built from), the restated sample equals a direct count, and every
seeded mistake of the model fails a named rung.
"""
import numpy as np
import pytest

import ladder as L
import ladder_hot as H
import ladder_sliced as LS

VTS = ["f32", "f64"]
WIN = H.constants()["HOT_WIN"]
_DATA = {}


def _data(fam):
    key = (fam.name, fam.vt)
    if key not in _DATA:
        values, x = LS.exact_data(fam)
        ref = L.spmv_reference(fam.rowptr, fam.colind, values, x, fam.shape)[0]
        _DATA[key] = (values, x, ref)
    return _DATA[key]


def _lay(name, vt):
    fam = H.family(name, vt)
    n_splits, lays = H.layouts(fam)
    return fam, n_splits, lays[0]


def _all_names(vt):
    return H.SMALL + H.WALKS + H.SHARES + H.hot_list_names(vt) + ["walk_default"]


def test_constants_and_the_cap():
    """The formula of hot_max_cols gives 16 320 fp64 and 36 736 fp32 columns; the comments of the source say the same."""
    assert H.hot_max_cols("f64") == 16320 and H.hot_max_cols("f32") == 36736
    src = L._src("spmv_hot.hip")
    assert "36 800" not in src and src.count("36 736 fp32") == 2
    assert WIN == 256 and H.constants()["ROW_SLOTS"] == 2 and H.constants()["FIX_LANES"] == 16


@pytest.mark.parametrize("vt", VTS)
def test_model_equals_the_csr_product_on_every_family(vt):
    for name in _all_names(vt):
        fam, n_splits, lay = _lay(name, vt)
        assert (n_splits == 0) == (name in H.REFUSED), name
        if lay.refused:
            assert lay.refused == H.REFUSED[name], (name, lay.refused)
            continue
        values, x, ref = _data(fam)
        assert np.array_equal(H.model_spmv(fam, lay, values, x), ref), name
        assert np.array_equal(H.model_spmv(fam, lay, values, x, alpha=-2.0), -2.0 * ref), name


@pytest.mark.parametrize("vt", VTS)
def test_restated_sample_equals_a_direct_count(vt):
    """hot_sample_positions: whole lines of 32 entries, one of every 16, never an entry twice; the counts of the restatement
    are those of a loop over the sampled entries; the builder met every candidate exactly as often as it was asked to."""
    for name in ("clipped", "share_exact", "hot_list_65", "depth2", "thr_rises_kept"):
        fam, _, lay = _lay(name, vt)
        pos = LS.hot_sample_positions(fam.nnz)
        assert np.unique(pos).size == pos.size and (pos[::32] % 32 == 0).all()
        assert set(np.unique(pos // 512).tolist()) == set(range(H.cdiv(fam.nnz, 512))) or fam.nnz % 512
        direct = {}
        for p in pos.tolist():
            direct[int(fam.colind[p])] = direct.get(int(fam.colind[p]), 0) + 1
        assert {c: int(v) for c, v in enumerate(lay.cnt) if v} == direct, name
    fam, _, lay = _lay("clipped", vt)
    assert sorted(lay.cnt[lay.hot_cols].tolist()) == sorted(H.CLIP_COUNTS) and lay.k == 5


@pytest.mark.parametrize("vt", VTS)
def test_row_start_families_reach_their_rungs(vt):
    for name in ("starts_plus", "starts_minus"):
        fam, _, lay = _lay(name, vt)
        st = H.window_stats(lay)
        assert set((lay.hot_rowptr[:-1] % WIN).tolist()) == set(range(WIN)), name
        full = np.arange(lay.nwin) < lay.n_hot // WIN
        assert (st["starts"][full] >= 1).sum() >= full.sum() - 1 and st["starts"].max() <= 2, name
        assert (st["head"][full].sum() >= WIN - 2) and (st["tail"][full].sum() >= WIN - 2), name
    fam, _, lay = _lay("pairs", vt)
    gaps = set()
    for w in range(lay.nwin):
        s = lay.hot_rowptr[lay.win_row[w]:lay.win_row[w + 1]]
        gaps.update(np.diff(s).tolist())
    assert set(H.PAIR_GAPS) <= gaps
    fam, _, lay = _lay("nibbles", vt)
    start = np.zeros(lay.nwin * WIN, bool)
    start[lay.hot_rowptr[:-1]] = True
    nib = start.reshape(lay.nwin, 64, 4)
    for w, (ln, pat) in enumerate(fam.meta["spec"], start=1):
        assert sum(int(nib[w, ln, j]) << j for j in range(4)) == pat
        others = nib[w].copy()
        others[ln] = False
        assert not others.any()
    assert {(ln, pat) for ln, pat in fam.meta["spec"]} == {(ln, pat) for ln in H.NIBBLE_LANES for pat in range(16)}


@pytest.mark.parametrize("vt", VTS)
def test_starts_per_window_and_the_four_kinds_of_window(vt):
    fam, _, lay = _lay("starts_per_window", vt)
    st = H.window_stats(lay)
    aligned = st["start_on_0"] & st["end_on_last"]
    shifted = st["head"] & st["tail"]
    assert set(H.START_COUNTS) <= set(st["starts"][aligned].tolist()), sorted(set(st["starts"][aligned].tolist()))
    # (a window with a head has an entry that starts no row: at most HOT_WIN - 1 starts)
    assert set(H.START_COUNTS) - {WIN} <= set(st["starts"][shifted].tolist()), sorted(set(st["starts"][shifted].tolist()))
    assert (st["starts"] > 128).any() and st["starts"].max() == WIN
    kinds = set()
    for name in ("starts_per_window", "pairs", "long_rows"):
        s2 = H.window_stats(_lay(name, vt)[2])
        kinds |= set(zip(s2["head"][s2["starts"] > 0].tolist(), s2["tail"][s2["starts"] > 0].tolist()))
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("vt", VTS)
def test_long_rows_and_ends_reach_their_rungs(vt):
    fam, _, lay = _lay("long_rows", vt)
    st = H.window_stats(lay)
    span = (lay.hot_rowptr[1:] - 1) // WIN - lay.hot_rowptr[:-1] // WIN
    for k in H.LONG_SPANS:
        at = np.flatnonzero(span == k)
        assert at.size >= 2 and (np.diff(at) == 1).any(), k            # two of them back to back
    assert span.max() > H.constants()["FIX_LANES"] and st["plain"].sum() > 100
    assert span[-1] == 3 and lay.n_hot % WIN not in (0,) and st["plain"][-1], "the last window: partial, without a start"
    assert not np.isin(fam.colind[fam.rowptr[-2]:], lay.hot_cols[:1]).all()
    for case, n_hot in H.END_CASES.items():
        lay = _lay("ends_" + case, vt)[2]
        assert lay.n_hot == n_hot and lay.nwin == n_hot // WIN + 1
    assert {_lay("ends_" + c, vt)[2].n_hot % WIN for c in H.END_CASES} >= {0, 1, WIN - 1}
    assert {_lay("ends_" + c, vt)[2].nwin for c in H.END_CASES} >= {1, 2, 15, 16, 17}
    assert _lay("one_hot_row", vt)[2].m_hot == 1
    for v in H.M_HOT_CASES:
        assert _lay(f"scan_block_{v}", vt)[2].m_hot == v
    fam, _, lay = _lay("gaps", vt)
    hot_n = fam.meta["hot_per_row"]
    lens = np.diff(fam.rowptr)
    assert hot_n[0] > 0 and hot_n[-1] > 0 and (np.diff(lay.hot_rows) > 5000).sum() == 2
    assert ((hot_n > 0) & (lens == hot_n)).any() and ((hot_n == 0) & (lens > 0)).any() and (lens == 0).sum() > 10000
    assert np.array_equal(lay.hot_rows, np.flatnonzero(hot_n))


@pytest.mark.parametrize("vt", VTS)
def test_walk_families_reach_their_rungs(vt):
    for k, r in H.WALK_CASES:
        fam, _, lay = _lay(f"walk_{k}_{r}", vt)
        assert lay.nwin == 16 * k + r and lay.grid == 1
        per_wave = H.walk_counts(lay.nwin, lay.grid)
        assert per_wave.sum() == lay.nwin and set(per_wave.tolist()) == ({k, k + 1} if r else {k})
        st = H.window_stats(lay)
        assert st["plain"].any() or k == 1
    for cus in (256, 304, 64):
        fam = H.family("walk_default", vt, cus)
        lay = H.layouts(fam, cus)[1][0]
        assert lay.nwin == 2 * 16 * cus + 3 and lay.grid == cus
        per_wave = H.walk_counts(lay.nwin, lay.grid)
        assert sorted(set(per_wave.tolist())) == [2, 3] and (per_wave == 3).sum() == 3


@pytest.mark.parametrize("vt", VTS)
def test_hot_list_families_reach_their_rungs(vt):
    kmax = H.hot_max_cols(vt)
    for k in H.k_rungs(vt):
        fam, _, lay = _lay(f"hot_list_{k}", vt)
        assert lay.k == k and lay.thr == 2 and lay.hot_cols.size == k
        assert fam.meta["sampled_cold_once"] > 0 or k <= 2              # columns sampled once are never hot
        assert (lay.cnt[np.setdiff1d(np.arange(fam.shape[1]), lay.hot_cols)] <= 1).all()
    assert {4095, 4096, 4097, 8193} <= set(H.k_rungs(vt)) and 4 * H.constants()["HOT_THREADS"] == 4096
    fam, n_splits, lay = _lay("thr_rises_kept", vt)
    assert n_splits == 1 and lay.thr == 3 and lay.k == fam.meta["n_heavy"] and (lay.cnt >= 2).sum() == kmax + 1
    fam, n_splits, lay = _lay("thr_rises_refused", vt)
    assert n_splits == 0 and lay.refused == "sample" and lay.thr == 3 and (lay.cnt >= 2).sum() == kmax + 1
    for mod in H.N_MOD:
        fam, _, lay = _lay(f"col_edges_{mod}", vt)
        n = fam.shape[1]
        assert n % 256 == mod and lay.hot_cols.tolist() == [0, 63, 64, n - 1]


@pytest.mark.parametrize("vt", VTS)
def test_coverage_families_reach_their_rungs(vt):
    pct = H.constants()["MIN_PCT"]
    fam, n_splits, lay = _lay("share_exact", vt)
    assert n_splits == 1 and lay.mass * 100 == lay.sampled * pct
    fam, n_splits, lay = _lay("share_minus_one", vt)
    assert n_splits == 0 and lay.refused == "sample" and (lay.mass + 1) * 100 == lay.sampled * pct
    fam, n_splits, lay = _lay("share_promise", vt)
    assert lay.refused == "matrix" and lay.mass == lay.sampled and (pct - 1) * fam.nnz <= lay.n_hot * 100 < pct * fam.nnz
    fam, n_splits, lay = _lay("share_all_hot", vt)
    assert lay.refused == "matrix" and lay.n_hot == fam.nnz
    fam = H.family("depth2", vt)
    n_splits, lays = H.layouts(fam)
    assert n_splits == 2 and lays[1].hot_cols.tolist() == sorted(fam.meta["second"].tolist())
    assert lays[1].min_pct == H.constants()["MIN_PCT2"] and lays[1].n_hot * 100 < lays[0].rest_colind.size * pct
    assert H.depth(vt, fam.rowptr, fam.colind, fam.shape, {k: v for k, v in fam.env.items() if "DEPTH" not in k})[0] == 1


# what each seeded mistake must break: (family, why)
BITES = {"no_carry_into_dpp_row": ("starts_plus", "a row that runs across lane 16, 32 or 48 loses what the lanes before carry"),
         "rows_beyond_second_slot_dropped": ("starts_per_window", "a window with more than 128 row starts"),
         "fixup_stops_after_16_windows": ("long_rows", "a row that covers 17 windows beyond its own"),
         "runs_on_with_ge": ("starts_per_window", "a row that ends on the last entry of its window")}


@pytest.mark.parametrize("mistake", list(BITES))
@pytest.mark.parametrize("vt", VTS)
def test_every_mistake_fails_its_rung(vt, mistake):
    name, _ = BITES[mistake]
    fam, _, lay = _lay(name, vt)
    values, x, ref = _data(fam)
    y = H.model_spmv(fam, lay, values, x, mistake=mistake)
    bad = np.flatnonzero(y != ref)
    assert bad.size > 0, mistake
    st = H.window_stats(lay)
    hot_idx = np.searchsorted(lay.hot_rows, bad)
    assert np.array_equal(lay.hot_rows[hot_idx], bad)                  # only rows with hot entries can differ
    row_win = lay.hot_rowptr[hot_idx] // WIN
    if mistake == "rows_beyond_second_slot_dropped":
        assert (st["starts"][row_win] > 128).all()
    if mistake == "fixup_stops_after_16_windows":
        span = (lay.hot_rowptr[1:] - 1) // WIN - lay.hot_rowptr[:-1] // WIN
        assert np.array_equal(hot_idx, np.flatnonzero(span > 16))
    if mistake == "runs_on_with_ge":
        ends = lay.hot_rowptr[hot_idx + 1]
        assert ((ends % WIN == 0) | (ends == lay.n_hot)).all() and (ends % WIN == 0).sum() >= 10
    # and the other families of the same group stay right where the mistake cannot show
    if mistake == "fixup_stops_after_16_windows":
        f2, _, l2 = _lay("starts_plus", vt)
        v2, x2, r2 = _data(f2)
        assert np.array_equal(H.model_spmv(f2, l2, v2, x2, mistake=mistake), r2)


@pytest.mark.parametrize("vt", VTS)
def test_pads_of_a_plain_window_stay_out_of_the_sum(vt):
    """x = inf on the first hot column: the pads behind the last entry are 0 * xs[0] = NaN.  The last window of long_rows is a
    plain reduction over a partial window: a model that sums the pads too makes the last row NaN although it never
    references that column."""
    fam, _, lay = _lay("long_rows", vt)
    values, x, _ = _data(fam)
    x = x.copy()
    x[lay.hot_cols[0]] = np.inf
    rows = np.repeat(np.arange(fam.shape[0]), np.diff(fam.rowptr))
    touched = np.zeros(fam.shape[0], bool)
    touched[rows[fam.colind == lay.hot_cols[0]]] = True
    assert not touched[-1] and touched.any() and not touched.all()
    with np.errstate(invalid="ignore"):
        good = H.model_spmv(fam, lay, values, x)
        bad = H.model_spmv(fam, lay, values, x, mistake="pads_in_plain_reduction")
    assert np.array_equal(~np.isfinite(good), touched)
    assert not np.isfinite(bad[-1]) and np.array_equal(~np.isfinite(bad[:-1]), touched[:-1])
