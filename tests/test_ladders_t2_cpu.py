"""CPU: the ladder of the two-pass transposed SpMV (tests/ladder_t2.py) proved before it judges a kernel.

* the host model of hist -> scan -> plan -> scatter -> accumulate equals scipy's A^T x on every family: the integer set exactly,
  the row-probe set as the row map;
* every family holds what its name claims (derived from the restated geometry: item lengths, lo mod 4, row-start positions,
  cut flags, the item count against max_items);
* the restated reciprocal division equals col // W for every slice width, on both sides of every slice edge;
* every wrong model of MUTATIONS fails the checker on the families named for it.
"""
import numpy as np
import pytest

import ladder_t2 as LT

CUS = 256            # only the default geometry (no _T2_W hook) of a matrix with few columns depends on the CU count
C = LT.constants()
T = C["TILE"]
F = LT.families()
NAN = float("nan")


def _vts(fam):
    """fp32 always; fp64 where its geometry differs (the slice width the LDS holds is half as wide)."""
    if fam.only:
        return [fam.only]
    return ["f32", "f64"] if fam.geometry("f32", CUS) != fam.geometry("f64", CUS) else ["f32"]


def _agrees(fam, vt, mut=None, kinds=("ints", "probe"), stats=None):
    """True when the (mutated) model gives the exact result on every data set of the family; beta = 0 runs over a y of NaN."""
    for kind, ff in LT.cases(fam):
        if kind not in kinds or (LT.is_wide(fam) and kind == "probe"):
            continue
        g = ff.geometry(vt, CUS)
        assert g["path"] == "two_pass", (ff.name, g)
        values, x = LT.host_data(ff, kind)[:2]
        y0 = LT.y_start(ff.shape[1])
        for alpha, beta in ((-2.0, 0.5),) if kind == "ints" else ((1.0, 0.0),):
            ref, _ = LT.reference(ff, kind, alpha, beta, y0)
            if kind == "probe" and (alpha, beta) == (1.0, 0.0):
                assert np.array_equal(ref, LT.row_map(ff)), ff.name
            start = y0 if beta != 0.0 else np.full(ff.shape[1], NAN)
            y = LT.model(ff.rowptr, ff.colind, ff.shape, values, x, alpha, beta, start, g, mut=mut, stats=stats)
            if not np.array_equal(y, ref):
                return False
    return True


TWO_PASS = [n for n, f in F.items() if f.geometry(f.only or "f32", CUS)["path"] == "two_pass"]


def test_constants_are_read_from_the_source():
    assert (T, C["THREADS"], C["SMAX"]) == (8192, 1024, 1024)
    assert (LT.wcap("f32"), LT.wcap("f64"), LT.wide_w("f32"), LT.wide_w("f64")) == (19456, 9728, 38912, 19456)
    assert len(F) > 150 and len(TWO_PASS) == len(F) - 3


def test_model_equals_scipy_on_every_family():
    for name in TWO_PASS:
        fam = F[name]
        for vt in _vts(fam):
            st = {}
            assert _agrees(fam, vt, stats=st), (name, vt)
            g = LT.cases(fam)[1][1].geometry(vt, CUS) if not LT.is_wide(fam) else fam.geometry(vt, CUS)
            assert st["n_items"] <= LT.max_items(g, fam.nnz), name
            assert np.unique(st["place"]).size == fam.nnz, f"{name}: two entries share a place in the workspace"


@pytest.mark.parametrize("alpha,beta", LT.ALPHA_BETA)
def test_model_alpha_beta(alpha, beta):
    for name in ("shares_seg64", "slices_empty_between_W192", "tiles_16_full"):
        fam = F[name]
        g = fam.geometry("f32", CUS)
        values, x = LT.host_data(fam, "ints")[:2]
        y0 = LT.y_start(fam.shape[1])
        ref, _ = LT.reference(fam, "ints", alpha, beta, y0)
        y = LT.model(fam.rowptr, fam.colind, fam.shape, values, x, alpha, beta, y0 if beta else np.full(y0.size, NAN), g)
        assert np.array_equal(y, ref), name


def test_accumulate_loop_covers_every_position_once():
    for L in (1, 2, 3, 4, 5, 4095, 4096, 4097, 4099, 4100, 4101, 8191, 8192, 8193, 8196, 12292, 16383, 16384, 16385, 65536):
        for lo in (0, 1, 2, 3, 1001):
            assert np.array_equal(np.sort(LT.coverage(lo, lo + L)), np.arange(lo, lo + L)), (L, lo)


def test_tile_permutation_is_one():
    for ntile in list(range(1, 70)) + [1000, 1001, 1007]:
        assert sorted(LT.t2_tile_of(b, ntile) for b in range(ntile)) == list(range(ntile))
    assert [LT.t2_tile_of(b, 16) for b in range(4)] == [0, 2, 4, 6] and LT.t2_tile_of(16, 17) == 16
    assert all(LT.t2_tile_of(b, nt) == b for nt in (7, 8, 9, 15) for b in range(nt))        # per = 0 or 1: the identity


def test_reciprocal_division_equals_division():
    k = np.arange(0, C["SMAX"] + 1, dtype=np.int64)
    bad_raw = 0
    for W in range(64, LT.wide_w("f32") + 1, 64):
        cols = np.concatenate([k * W - 1, k * W, k * W + 1])
        cols = cols[(cols >= 0) & (cols <= LT.INT32_MAX)]
        assert np.array_equal(LT.t2_slice(cols, W), cols // W), W
        bad_raw += int(not np.array_equal(LT.t2_slice(cols, W, corrected=False), cols // W))
    assert bad_raw > 500          # (the correction is needed for every width that is no power of two)


# ----------------------------------------------------------------------------------------------- what the families hold
def _d(name, vt="f32"):
    return LT.derived(F[name], F[name].geometry(vt, CUS))


def test_tile_families():
    for nnz in (1, 2, 63, 64, 65, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1):
        assert F[f"tiles_nnz_{nnz}"].nnz == nnz
    for nt in (7, 8, 9, 15, 16, 17):
        full, part = F[f"tiles_{nt}_full"], F[f"tiles_{nt}_partial"]
        assert full.nnz == nt * T and (nt - 1) * T < part.nnz < nt * T
        assert full.geometry("f32", CUS)["ntile"] == part.geometry("f32", CUS)["ntile"] == nt
        assert full.distinct and part.distinct


def test_row_start_families():
    named = {0, 1, 62, 63, 64, 65, 127, 128, 1023, 1024, 1025, T - 65, T - 64, T - 1}
    assert _d("starts_named")["start_positions"] == named
    assert _d("starts_named")["start_mod_64"] == {0, 1, 62, 63} and {0, 1, 1023} <= _d("starts_named")["start_mod_1024"]
    for p in named:
        assert _d(f"starts_only_{p}")["start_positions"] == {0, 5, p}
    assert _d("starts_lane0")["start_mod_64"] == {0} and len(_d("starts_lane0")["start_positions"]) == 128
    assert _d("starts_lane63")["start_mod_64"] == {0, 63} and len(_d("starts_lane63")["start_positions"]) == 129
    assert {p // 64 % 2 for p in _d("starts_even_segments")["start_positions"]} == {0}
    assert {p // 64 % 2 for p in _d("starts_odd_segments")["start_positions"] - {0}} == {1}
    assert {p // 64 for p in _d("starts_segment_0")["start_positions"]} == {0}
    assert {p // 64 for p in _d("starts_segment_127")["start_positions"] - {0}} == {127}
    assert max(np.diff(sorted(_d("starts_stretch_2048")["start_positions"]))) >= 2048
    ones = F["rows_of_length_1"]
    assert (np.diff(ones.rowptr) == 1).all() and ones.nnz > 2 * T
    assert F["row_is_one_tile"].rowptr.tolist()[1:3] == [T, 2 * T]
    r3 = F["row_spans_three_tiles"].rowptr
    assert r3[1] < T and r3[2] > 3 * T                       # tiles 1 and 2 hold no row start at all
    re_ = F["row_ends_on_last_position"].rowptr
    assert {T, 2 * T, 3 * T} <= set(re_.tolist())
    assert F["one_row"].shape[0] == 1 and F["one_row"].nnz > T
    last = F["last_of_100000_rows"]
    assert last.shape[0] == 100000 and (np.diff(last.rowptr)[:-1] == 0).all() and last.nnz == 70
    for fam in F.values():
        if fam.name.startswith(("starts_", "row", "one_row", "last_of", "tiles_", "empty_")):
            assert fam.distinct, fam.name              # the row probe runs on the family itself


def test_empty_row_families():
    where = {"tile_position_0": T, "mid_wavefront": T + 1037, "tile_last_position": 2 * T - 1, "tile_end": 2 * T,
             "before_first_entry": 0}
    for k in (1, 2, 1023, 1024, 1025, 5000):
        for w, p in where.items():
            rp = F[f"empty_{k}_{w}"].rowptr
            assert int((rp == p).sum()) == k + 1 and int((np.diff(rp) == 0).sum()) == k, (k, w)
        rp = F[f"empty_{k}_behind_last_entry"].rowptr
        assert int((rp[1:] == rp[-1]).sum()) == k + 1 and rp[-1] == 2 * T
        assert F[f"empty_{k}_tile_end"].nnz == 2 * T + 5
    assert (T + 1037) % 64 not in (0, 63)


def test_slice_families():
    for S in (1, 2, 3, 63, 64, 65, 959, 960, 961, 1023, 1024):
        for tail, n in (("", 64 * S), ("_last_of_1", 64 * (S - 1) + 1)):
            fam = F[f"slices_W64_S{S}{tail}"]
            g = fam.geometry("f32", CUS)
            assert (g["W"], g["S"], fam.shape[1]) == (64, S, n) and g == fam.geometry("f64", CUS)
            cols = set(fam.colind.tolist())
            edge = {0, 63, 64, 65, (S - 1) * 64 - 1, (S - 1) * 64, n - 1}
            assert {c for c in edge if 0 <= c < n} <= cols and fam.distinct
            assert set(LT.derived(fam, g)["shares"]) <= {1, 2, 3}                # no slice without an entry here
    for W in (128, 192, 320, 4096, 9728, 19456):
        for S in (1, 3, 65):
            fam = F[f"slices_W{W}_S{S}"]
            g32, g64 = fam.geometry("f32", CUS), fam.geometry("f64", CUS)
            assert (g32["W"], g32["S"], g32["w_hook_ignored"]) == (W, S, 0)
            if W > LT.wcap("f64"):           # refused for fp64: the default width instead, and the readback says so
                assert g64["w_hook_ignored"] == 1 and g64["W"] != W
            else:
                assert g64 == g32
    assert F["slices_n_1"].shape[1] == 1 and F["slices_n_below_W"].shape[1] < F["slices_n_below_W"].W
    for W in (64, 192):
        fam = F[f"slices_empty_between_W{W}"]
        share = np.bincount(LT.t2_slice(fam.colind, W), minlength=65)
        assert share[0] > 0 and share[64] > 0 and (share[1:64] == 0).all()
    g = F["slices_1025_falls_back"].geometry("f32", CUS)
    assert (g["path"], g["why"], g["S"]) == ("scatter", "does_not_fit", C["SMAX"] + 1)
    for vt in ("f32", "f64"):
        fam, more = F[f"widest_{vt}"], F[f"widest_{vt}_plus_1"]
        for cus in (64, 256, 304):
            g = fam.geometry(vt, cus)
            assert fam.W is None and (g["path"], g["W"], g["S"]) == ("two_pass", LT.wide_w(vt), C["SMAX"])
            g = more.geometry(vt, cus)
            assert (g["path"], g["why"]) == ("scatter", "does_not_fit") and more.shape[1] == fam.shape[1] + 1
        assert fam.shape[1] == C["SMAX"] * LT.wide_w(vt) and fam.nnz < 4000
        assert set(np.unique(fam.colind % LT.wide_w(vt)).tolist()) <= {0, 1, LT.wide_w(vt) - 1}      # slice edges only


def test_segment_and_item_families():
    for seg in (64, 100, 4096, 8192):
        d = _d(f"shares_seg{seg}")
        want = {0, 1, seg - 1, seg, seg + 1, 2 * seg - 1, 2 * seg, 2 * seg + 1, 10 * seg + 3}
        assert d["shares"] == want and d["cut"] == {0, 1}
        assert F[f"shares_seg{seg}"].geometry("f32", CUS)["seg"] == seg
    dseg = C["seg_min"]
    assert F["shares_default_seg"].geometry("f32", CUS)["seg"] == dseg == F["shares_default_seg_exact"].geometry("f64", CUS)["seg"]
    assert _d("shares_default_seg")["shares"] == {0, 1, dseg - 1, dseg + 1} and _d("shares_default_seg")["cut"] == {0, 1}
    assert dseg in _d("shares_default_seg_exact")["shares"] and _d("shares_default_seg_exact")["cut"] == {0}
    d = _d("all_1024_slices_cut")
    assert d["cut"] == {1} and d["n_items"] == 2048 and d["item_lengths"] == {64, 1}
    fam = F["worst_case_item_count"]
    d, g = _d(fam.name), fam.geometry("f32", CUS)
    assert d["shares"] == {1, 65, 129} and d["n_items"] == sum(1 + (i % 3) for i in range(1024))
    assert LT.max_items(g, fam.nnz) - d["n_items"] == 1 + sum(((i % 3) * 64 + 1) for i in range(1024)) // 64 - sum(i % 3 for i in range(1024))
    fam = F["cut_slice_is_narrow_last"]
    d, g = _d(fam.name), fam.geometry("f32", CUS)
    assert fam.shape[1] - (g["S"] - 1) * g["W"] == 10 and [it[3] for it in d["items"] if it[0] == g["S"] - 1] == [1] * 4
    lengths = (1, 2, 3, 4, 5, 4095, 4096, 4097, 4099, 4100, 4101, 8191, 8192, 8193, 8196, 12292, 16383, 16384, 16385)
    for r in range(4):
        items = _d(f"item_lengths_uncut_lo{r}")["items"]
        for L in lengths:
            assert any(hi - lo == L and lo % 4 == r and not cut for _, lo, hi, cut in items), (r, L)
        for tag, group in (("1_5", lengths[:5]), ("4096", lengths[5:11]), ("8192", lengths[11:16]), ("16384", lengths[16:])):
            fam = F[f"item_lengths_last_segment_{tag}_lo{r}"]
            seg = fam.seg
            items = _d(fam.name)["items"]
            for L in group:     # the last segment of a cut slice, behind one full segment
                assert any(hi - lo == L and lo % 4 == r and cut and items[i - 1][:1] == (s_,) and
                           items[i - 1][2] - items[i - 1][1] == seg for i, (s_, lo, hi, cut) in enumerate(items) if i), (r, tag, L)
    fam = F["segment_in_one_column"]
    st = {}
    assert _agrees(fam, "f32", kinds=("ints",), stats=st)
    assert st["items"][0] == (0, 0, T, 1) and set(fam.colind[:T].tolist()) == {7} and st["place"][:T].max() < T
    for S, nt in ((89, 23), (64, 32), (683, 3), (64, 64), (241, 17)):
        g = F[f"scan_{S}x{nt}"].geometry("f32", CUS)
        assert (g["S"], g["ntile"]) == (S, nt)
    assert sorted(S * nt for S, nt in ((89, 23), (64, 32), (683, 3), (64, 64), (241, 17))) == [2047, 2048, 2049, 4096, 4097]


def test_cases_stay_small():
    for fam in F.values():
        assert fam.nnz <= 20 * T or fam.name.startswith("scan_"), fam.name
        assert fam.shape[1] <= 2_000_000 or LT.is_wide(fam), fam.name


# ------------------------------------------------------------------------------------------------------------- mutations
BITES = {
    "no_segment_carry": ["starts_segment_0", "starts_lane63", "starts_stretch_2048", "row_is_one_tile"],
    "no_pair_carry": ["starts_even_segments", "starts_only_0", "starts_stretch_2048"],
    "first_row_wins": ["empty_1_mid_wavefront", "empty_1024_tile_position_0", "empty_5000_tile_last_position",
                       "empty_2_before_first_entry", "last_of_100000_rows"],
    "r_lo_not_stepped_back": ["row_spans_three_tiles", "starts_only_64", "tiles_9_partial"],
    "raw_quotient": ["slices_W192_S3", "slices_W320_S65", "slices_W9728_S3"],
    "empty_slice_without_item": ["slices_empty_between_W64", "slices_empty_between_W192", "shares_seg64"],
    "last_segment_not_clipped": ["shares_seg64", "shares_seg8192", "cut_slice_is_narrow_last", "all_1024_slices_cut"],
    "cut_slice_written_directly": ["all_1024_slices_cut", "shares_seg100", "item_lengths_last_segment_4096_lo1"],
    "vector_bound_off_by_4": ["item_lengths_uncut_lo0", "item_lengths_uncut_lo3", "item_lengths_last_segment_8192_lo2"],
    "tile_of_in_one_pass": ["tiles_16_full", "tiles_17_partial", "scan_64x32"],
}


def test_every_mutation_has_families():
    assert set(BITES) == set(LT.MUTATIONS)


@pytest.mark.parametrize("mut", LT.MUTATIONS)
def test_wrong_models_fail(mut):
    for name in BITES[mut]:
        assert _agrees(F[name], "f32"), name                      # the model itself passes there ...
        assert not _agrees(F[name], "f32", mut=mut), f"{mut} goes unnoticed on {name}"     # ... and the wrong one does not
