"""Window ladder for the hot-column split of the SLICED SpMV (csrc/spmv_hot.hip): matrices built from a specification of the
HOT part -- which entries sit in candidate columns, how often the inspect's sample meets each candidate --, a host
restatement of the inspect (sample -> counts -> threshold and K under the LDS cap -> both coverage tests -> hot list, split,
hot_rows, hot_rowptr, win_row, crossing rows, grid) and a host model of the multiply (row-start bitmap, a lane's nibble, the
inclusive segmented scan in lane order with the carry into a lane's first segment, head / tail, the two row slots per lane
plus the loop beyond them, the fixup's strided sum).  tests/test_gpu_hot_ladders.py holds the device against the restatement
through spblas_gfx950_plan_hot_layout and runs the families; tests/test_ladders_hot_cpu.py proves on the host that every family
reaches the rung it is named for and that the model fails a named rung when one of MISTAKES is seeded.

A_hot is cut into windows of HOT_WIN entries, one wavefront each; a wavefront walks the windows w, w + 16 * grid, ...  The
families, by what they put on an edge:

  row starts   starts_plus / starts_minus: HOT_WIN + 1 rows of HOT_WIN + 1 / HOT_WIN - 1 hot entries -- a start on every
               position of a window, a head and a tail in every window; pairs: two starts d apart for every d of PAIR_GAPS;
               nibbles: all sixteen start patterns of a lane's four entries on the lanes of NIBBLE_LANES
  per window   starts_per_window: windows with every count of START_COUNTS (rows of one and two entries), window-aligned (a
               start on position 0 and an end on the last: no head, no tail) and shifted by one entry (head and tail)
  long rows    rows that cover every count of LONG_SPANS windows beyond their own, two of them back to back, windows without
               a start in between, and a last row that runs to the end of a partial last window
  ends         n_hot mod HOT_WIN in {0, 1, HOT_WIN - 1}, nwin in {1, 2, 15, 16, 17}, one hot row, hot rows around the scan's
               block of 2 048, 5 000 empty rows between hot rows, first and last row hot, hot-only and cold-only rows
  walk         SPBLAS_GFX950_PB_HOT_GRID=1: 16 k + r windows, k = 1 ... 9, r in {0, 1, 15} (every wavefront walks k or k + 1);
               walk_default: 2 * 16 * CUs + 3 windows under the default grid
  hot list     K of K_RUNGS up to the LDS cap; one column more than fits, at the lowest count: the threshold rises by one --
               once with the rest still carrying its share, once refused; hot columns 0, 63, 64, n - 1 with n mod 256 of
               N_MOD; columns sampled 1 021 ... 1 024 and 5 000 times (the clipped last bucket)
  coverage     the sample's share exactly the limit and one reference less; a sample that promises everything on a matrix that
               holds 14 per cent; every entry hot; SPBLAS_GFX950_PB_HOT_DEPTH=2: the remainder split again

Checks and data come from tests/ladder.py and tests/ladder_sliced.py (exact_data: integers without zeros whose partial sums
stay below 2^24 in any order); no tolerance is introduced here.
"""
import re

import numpy as np

import ladder as L
import ladder_sliced as LS

PRE = "SPBLAS_GFX950_"
PAIR_GAPS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
NIBBLE_LANES = (0, 15, 16, 31, 32, 63)
START_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
LONG_SPANS = (1, 2, 15, 16, 17, 18, 32, 33)
END_CASES = {"nwin_1": 100, "mod_255": 255, "mod_0": 256, "mod_1": 257, "nwin_15": 14 * 256 + 5, "nwin_16": 15 * 256 + 255,
             "nwin_17": 16 * 256}
WALK_CASES = [(k, r) for k in range(1, 10) for r in (0, 1, 15)]
N_MOD = (1, 63, 64, 65)
CLIP_COUNTS = (1021, 1022, 1023, 1024, 5000)
MISTAKES = ("no_carry_into_dpp_row", "rows_beyond_second_slot_dropped", "fixup_stops_after_16_windows", "runs_on_with_ge",
            "pads_in_plain_reduction")
cdiv = LS.cdiv

# ------------------------------------------------------------------------------------------------------------ constants
_CONST = {}


def _need(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the source no longer has the expected form; update tests/ladder_hot.py"
    return m


def constants():
    """Every constant the hot split depends on, parsed from csrc/spmv_hot.hip (and the window count from csrc/spmv.hip)."""
    if _CONST:
        return _CONST
    hot = L._src("spmv_hot.hip")
    flat = re.sub(r"\s+", " ", hot)
    c = {}
    c["HOT_EPL"] = int(_need(r"#define HOT_EPL (\d+)", hot, "HOT_EPL").group(1))
    _need(r"static constexpr int HOT_WIN = 64 \* HOT_EPL;", hot, "HOT_WIN")
    c["HOT_WIN"] = 64 * c["HOT_EPL"]
    c["HOT_THREADS"] = int(_need(r"static constexpr int HOT_THREADS = (\d+);", hot, "HOT_THREADS").group(1))
    _need(r"static constexpr int HOT_WAVES = HOT_THREADS / 64;", hot, "HOT_WAVES")
    c["HOT_WAVES"] = c["HOT_THREADS"] // 64
    c["HOT_LDS"] = int(_need(r"static constexpr int HOT_LDS = (\d+) \* 1024;", hot, "HOT_LDS").group(1)) * 1024
    c["HOT_HIST"] = int(_need(r"static constexpr int HOT_HIST = (\d+);", hot, "HOT_HIST").group(1))
    _need(r"return \(HOT_LDS - HOT_WAVES \* HOT_WIN \* \(int\) sizeof\(T\) - HOT_WAVES \* HOT_WIN / 8\) / \(int\) sizeof\(T\) / 64 \* 64;",
          flat, "hot_max_cols")
    c["MIN_PCT"] = int(_need(r'hot_env\("SPBLAS_GFX950_PB_HOT_MIN_PCT", (\d+)\)', hot, "the share of a first split").group(1))
    c["MIN_PCT2"] = int(_need(r'hot_env\("SPBLAS_GFX950_PB_HOT_MIN_PCT2", (\d+)\)', hot, "the share of a second split").group(1))
    c["ROW_SLOTS"] = int(_need(r"for \(int k = 0; k < (\d+); \+\+k\) if \(rb \+ lane \+ 64 \* k < r_end\)", flat,
                               "the row slots of a lane").group(1))
    beyond = [int(v) for v in re.findall(r"for \(int r = rb \+ (\d+) \+ lane; r < (?:re|r_end); r \+= 64\)", flat)]
    assert beyond == [64 * c["ROW_SLOTS"]] * 2, "the loops beyond the row slots: update tests/ladder_hot.py"
    c["FIX_LANES"] = int(_need(r"for \(int64_t w = w0 \+ 1 \+ lig; w <= w1; w \+= (\d+)\)", flat, "the fixup's stride").group(1))
    _need(r"const int lig = threadIdx.x & 15;", flat, "the fixup's lane group")
    assert c["FIX_LANES"] == 16, "the fixup's lane group: update tests/ladder_hot.py"
    c["SCAN_BLOCK"] = int(_need(r"const int64_t nb = cdiv\(n, (\d+)\);", L._src("scan.hpp"), "the scan's block").group(1))
    for what, pat in (
            ("the threshold walk", r"for \(int c = HOT_HIST - 1; c >= 2; --c\) \{ if \(cols \+ h_hist\[\(size_t\) c\] > \(unsigned long long\) kmax\) break;"),
            ("the clipped bucket", r"const int b = v < HOT_HIST - 1 \? v : HOT_HIST - 1;"),
            ("the sample's share", r"if \(cols == 0 \|\| sampled == 0 \|\| mass \* 100 < sampled \* \(unsigned long long\) min_pct\)"),
            ("the matrix's share", r"if \(n_hot \* 100 < nnz \* \(long long\) min_pct \|\| n_rest < 1\)"),
            ("the column flags", r"flag\[c\] = cnt\[c\] >= thr;"),
            ("the crossing rows", r"cross = p0 / HOT_WIN != \(p1 - 1\) / HOT_WIN;"),
            ("runs_on", r"const bool runs_on = cur.e > whi;"),
            ("the head", r"if \(cur.a > wlo\) part_head\[w\] = strip\[\(int\) \(cur.a - wlo\) - 1\];"),
            ("the grid", r"return cdiv\(nwin, HOT_WAVES\) < cus \? cdiv\(nwin, HOT_WAVES\) : cus;"),
            ("the walk", r"hot_walk<T, O>\(\(int64_t\) blockIdx.x \* HOT_WAVES \+ wave, nwin - 1, \(int64_t\) gridDim.x \* HOT_WAVES,"),
            ("the LDS fill", r"for \(int i0 = 0; i0 < K; i0 \+= 4 \* HOT_THREADS\)")):
        _need(pat, flat, what)
    _need(r"pl->nwin = nnz / pl->win \+ 1;", L._src("spmv.hip"), "the window count")
    _need(r"if \(\(int64_t\) rowptr\[mid\] < target\)", L._src("spmv.hip"), "the first row of a window")
    _CONST.update(c)
    return _CONST


def hot_max_cols(vt):
    """hot_max_cols<T>(): what LDS holds next to the 16 scan strips and their row-start bitmaps, a multiple of 64."""
    c, item = constants(), LS.ITEM[vt]
    return (c["HOT_LDS"] - c["HOT_WAVES"] * c["HOT_WIN"] * item - c["HOT_WAVES"] * c["HOT_WIN"] // 8) // item // 64 * 64


def k_rungs(vt):
    kmax = hot_max_cols(vt)
    return (1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, kmax - 1, kmax)


# ------------------------------------------------------------------------------------------------- restated inspect
class Layout:
    """What hot_build_typed lays out: thr, k, hot_cols, is_hot (per entry), n_hot, hot_rows, m_hot, hot_rowptr, nwin, win_row,
    cross_rows, grid -- or refused = "sample" / "matrix" / "rows" with the counts known up to there."""
    refused = None


def sample_counts(colind, n):
    """cnt[c]: how often hot_sample_kernel meets column c."""
    colind = np.asarray(colind, np.int64)
    return np.bincount(colind[LS.hot_sample_positions(colind.size)], minlength=n)


def inspect(vt, rowptr, colind, shape, env=None, cus=256, level=0):
    """The inspect of one split, restated; `level` 0: the caller's matrix, 1: the remainder of a first split."""
    env = env or {}
    c = constants()
    rowptr, colind = np.asarray(rowptr, np.int64), np.asarray(colind, np.int64)
    m, n = shape
    nnz = colind.size
    lay = Layout()
    lay.cnt = cnt = sample_counts(colind, n)
    clipped = np.minimum(cnt, c["HOT_HIST"] - 1)
    hist = np.bincount(clipped, minlength=c["HOT_HIST"])
    mass_of = np.bincount(clipped, weights=cnt, minlength=c["HOT_HIST"]).astype(np.int64)
    sampled = int(mass_of[1:].sum())
    kmax = hot_max_cols(vt)
    cols = mass = 0
    thr = c["HOT_HIST"]
    for b in range(c["HOT_HIST"] - 1, 1, -1):
        if cols + hist[b] > kmax:
            break
        cols, mass, thr = cols + int(hist[b]), mass + int(mass_of[b]), b
    lay.thr, lay.k, lay.mass, lay.sampled = thr, cols, mass, sampled
    min_pct = int(env.get(PRE + "PB_HOT_MIN_PCT2", c["MIN_PCT2"])) if level > 0 else int(env.get(PRE + "PB_HOT_MIN_PCT", c["MIN_PCT"]))
    lay.min_pct = min_pct
    if cols == 0 or sampled == 0 or mass * 100 < sampled * min_pct:
        lay.refused = "sample"
        return lay
    lay.hot_cols = np.flatnonzero(cnt >= thr)
    assert lay.hot_cols.size == cols
    lay.is_hot = np.isin(colind, lay.hot_cols)
    lay.n_hot = n_hot = int(lay.is_hot.sum())
    if n_hot * 100 < nnz * min_pct or nnz - n_hot < 1:
        lay.refused = "matrix"
        return lay
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(rowptr))
    per_row = np.bincount(rows[lay.is_hot], minlength=m)
    lay.hot_rows = np.flatnonzero(per_row > 0)
    lay.m_hot = m_hot = int(lay.hot_rows.size)
    if m_hot < 1:
        lay.refused = "rows"
        return lay
    lay.hot_rowptr = np.concatenate([[0], np.cumsum(per_row[lay.hot_rows])]).astype(np.int64)
    win = c["HOT_WIN"]
    lay.nwin = nwin = n_hot // win + 1
    # first row of A_hot whose first entry is at or behind w * HOT_WIN (a binary search over the m_hot row starts)
    lay.win_row = np.append(np.searchsorted(lay.hot_rowptr[:m_hot], np.arange(nwin, dtype=np.int64) * win, side="left"), m_hot)
    p0, p1 = lay.hot_rowptr[:-1], lay.hot_rowptr[1:]
    lay.cross_rows = np.flatnonzero(p0 // win != (p1 - 1) // win)
    g = int(env.get(PRE + "PB_HOT_GRID", 0))
    lay.grid = g if g > 0 else min(cdiv(nwin, c["HOT_WAVES"]), cus)
    lay.rest_rowptr = np.concatenate([[0], np.cumsum(np.diff(rowptr) - per_row)]).astype(np.int64)
    lay.rest_colind = colind[~lay.is_hot]
    return lay


def depth(vt, rowptr, colind, shape, env=None, cus=256):
    """Splits the plan ends up with under SPBLAS_GFX950_PB_HOT_DEPTH (default 1): (count, layouts level by level)."""
    env = env or {}
    want = int(env.get(PRE + "PB_HOT_DEPTH", 1))
    lays, level = [], 0
    while level < want and colind.size > 0 and shape[0] >= 2:
        lay = inspect(vt, rowptr, colind, shape, env, cus, level)
        if lay.refused:
            break
        lays.append(lay)
        rowptr, colind, level = lay.rest_rowptr, lay.rest_colind, level + 1
    return len(lays), lays


def expected_counts(lay, n_splits=1):
    """counts[8] of spblas_gfx950_plan_hot_layout."""
    if lay.refused:
        return dict.fromkeys(("thr", "k", "n_hot", "m_hot", "nwin", "n_cross", "grid", "depth"), 0)
    return {"thr": lay.thr, "k": lay.k, "n_hot": lay.n_hot, "m_hot": lay.m_hot, "nwin": lay.nwin,
            "n_cross": int(lay.cross_rows.size), "grid": lay.grid, "depth": n_splits}


def walk_counts(nwin, grid):
    """Windows every wavefront of the launch walks: wavefront j of `grid` workgroups of 16 takes j, j + 16 grid, ..."""
    waves = 16 * grid
    return np.array([len(range(j, nwin, waves)) for j in range(waves)])


def window_stats(lay):
    """Per window: row starts, whether a row runs in from before (head), whether the last row runs on (tail)."""
    win = constants()["HOT_WIN"]
    w = np.arange(lay.nwin, dtype=np.int64)
    rb, re_ = lay.win_row[:-1], lay.win_row[1:]
    wlo, whi = w * win, np.minimum((w + 1) * win, lay.n_hot)
    a, e = lay.hot_rowptr[rb], lay.hot_rowptr[re_]
    return {"starts": re_ - rb, "head": (re_ > rb) & (a > wlo), "tail": (re_ > rb) & (e > whi), "plain": (re_ == rb) & (whi > wlo),
            "start_on_0": (re_ > rb) & (a == wlo), "end_on_last": (re_ > rb) & (e == whi) & (whi - wlo == win)}


# ------------------------------------------------------------------------------------------- host model of the multiply
def _dpp_rows(a, n):
    """row_shr:n inside the 16-lane rows; lanes without a source read 0."""
    r = a.reshape(a.shape[0], 4, 16)
    out = np.zeros_like(r)
    out[:, :, n:] = r[:, :, :16 - n]
    return out.reshape(a.shape)


def model_hot(lay, values, colind, x, alpha=1.0, mistake=None):
    """alpha * A_hot x as pb_hot_rows_kernel + pb_hot_fixup_kernel put it together, per row of y, in float64.  Every window:
    products of four consecutive entries per lane; row starts into a bitmap (the rows rb + lane, rb + 64 + lane from the two
    slots, the others from the loop beyond); a lane's nibble; the in-lane scan; the segmented scan over lanes (row_shr 1, 2, 4, 8
    in the 16-lane rows, lane 15 of rows 0 and 2 into rows 1 and 3, lane 31 into the upper half); the carry of the lane before
    into a lane's first segment; a row that ends in its window read at its last entry; head / tail for the fixup, which adds
    the heads of the later windows in 16 strided sums.  A window without a start is a plain sum of its live entries."""
    assert mistake is None or mistake in MISTAKES
    c = constants()
    win, epl, slots = c["HOT_WIN"], c["HOT_EPL"], c["ROW_SLOTS"]
    nwin, n_hot, m_hot, rp = lay.nwin, lay.n_hot, lay.m_hot, lay.hot_rowptr
    hv, hc = np.zeros(nwin * win), np.zeros(nwin * win, np.int64)
    hv[:n_hot] = np.asarray(values, np.float64)[lay.is_hot]
    hc[:n_hot] = np.searchsorted(lay.hot_cols, np.asarray(colind, np.int64)[lay.is_hot])
    xs = np.asarray(x, np.float64)[lay.hot_cols]
    with np.errstate(invalid="ignore"):
        prod = hv * xs[hc]                                    # (pads: 0 * xs[0])
    live = np.arange(nwin * win) < n_hot
    w = np.arange(nwin, dtype=np.int64)
    rb, re_ = lay.win_row[:-1], lay.win_row[1:]
    wlo, whi = w * win, np.minimum((w + 1) * win, n_hot)
    a, e = rp[rb], rp[re_]
    plain = rb == re_
    row_win = rp[:m_hot] // win
    slot_of = np.arange(m_hot) - rb[row_win]
    seen = np.ones(m_hot, bool)
    if mistake == "rows_beyond_second_slot_dropped":
        seen = slot_of < 64 * slots
    start = np.zeros(nwin * win, bool)
    start[rp[:m_hot][seen]] = True
    nib = start.reshape(nwin, 64, epl)
    t = prod.reshape(nwin, 64, epl).copy()
    for j in range(1, epl):
        t[:, :, j] = np.where(nib[:, :, j], t[:, :, j], t[:, :, j - 1] + t[:, :, j])
    v, f = t[:, :, epl - 1].copy(), nib.any(axis=2)
    lane = np.arange(64)
    lir = lane & 15
    for n_ in (1, 2, 4, 8):
        vp, fp, take = _dpp_rows(v, n_), _dpp_rows(f, n_), lir >= n_
        v, f = np.where(take & ~f, v + vp, v), np.where(take, f | fp, f)
    vp, fp = np.zeros_like(v), np.zeros_like(f)                # row_bcast:15 into rows 1 and 3
    vp[:, 16:32], vp[:, 48:64], fp[:, 16:32], fp[:, 48:64] = v[:, 15:16], v[:, 47:48], f[:, 15:16], f[:, 47:48]
    take = (lane & 16) != 0
    v, f = np.where(take & ~f, v + vp, v), np.where(take, f | fp, f)
    vp, fp = np.zeros_like(v), np.zeros_like(f)                # row_bcast:31 into the upper half
    vp[:, 32:], fp[:, 32:] = v[:, 31:32], f[:, 31:32]
    take = lane >= 32
    v, f = np.where(take & ~f, v + vp, v), np.where(take, f | fp, f)
    carry = np.zeros_like(v)                                  # wave_shr:1
    carry[:, 1:] = v[:, :-1]
    if mistake == "no_carry_into_dpp_row":
        carry[:, lir == 0] = 0.0
    seg_open = np.cumsum(nib, axis=2) == 0                      # no row start in the lane up to and including entry j
    strip = np.where(seg_open, t + carry[:, :, None], t).reshape(nwin, win)
    head, tail = np.zeros(nwin), np.zeros(nwin)
    in_sum = np.ones(nwin * win, bool) if mistake == "pads_in_plain_reduction" else live
    with np.errstate(invalid="ignore"):
        head[plain] = np.where(in_sum, prod, 0.0).reshape(nwin, win).sum(axis=1)[plain]
    has_head = ~plain & (a > wlo)
    head[has_head] = strip[w[has_head], (a - wlo - 1)[has_head]]
    runs_on = ~plain & ((e >= whi) if mistake == "runs_on_with_ge" else (e > whi))
    tail[runs_on] = strip[w[runs_on], (whi - wlo - 1)[runs_on]]
    r_end = re_ - runs_on
    y = np.zeros(m_hot)
    r = np.arange(m_hot)
    whole = (r < r_end[row_win]) & seen
    idx = rp[1:][whole] - wlo[row_win[whole]] - 1
    assert ((0 <= idx) & (idx < win)).all()
    y[whole] += alpha * strip[row_win[whole], idx]
    reach = c["FIX_LANES"] if mistake == "fixup_stops_after_16_windows" else nwin
    for rr in lay.cross_rows:
        w0, w1 = rp[rr] // win, (rp[rr + 1] - 1) // win
        s = sum(head[w0 + 1 + lig:min(w1, w0 + reach) + 1:c["FIX_LANES"]].sum() for lig in range(c["FIX_LANES"]))
        y[rr] += alpha * (s + tail[w0])
    return y


def model_spmv(fam, lay, values, x, alpha=1.0, mistake=None):
    """y = alpha A x of a split plan: the rest in float64 from its CSR arrays, the hot part through model_hot."""
    m = fam.shape[0]
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(fam.rowptr))
    cold = ~lay.is_hot
    y = alpha * np.bincount(rows[cold], weights=(values * x[fam.colind])[cold], minlength=m)
    y[lay.hot_rows] += model_hot(lay, values, fam.colind, x, alpha, mistake)
    return y


# -------------------------------------------------------------------------------------------------------------- builder
SMALL_TILES = {PRE + "SLICE_COLS": 512, PRE + "SLICE_ROWS": 64}      # the hooks of ladder_sliced.hot_split for A_rest


def entry_layout(hot_n, cold_n):
    """(row of every entry, whether it is a slot for a candidate column): even rows hold their hot entries first, odd rows last."""
    hot_n, cold_n = np.asarray(hot_n, np.int64), np.asarray(cold_n, np.int64)
    lens = hot_n + cold_n
    rows = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    j = np.arange(rows.size) - np.repeat(np.cumsum(lens) - lens, lens)
    return rows, np.where(rows % 2 == 0, j < hot_n[rows], j >= cold_n[rows])


def sampled_mask(nnz):
    s = np.zeros(nnz, bool)
    s[LS.hot_sample_positions(nnz)] = True
    return s


def spread(total, k, lo=2):
    """`total` sampled references over k columns, as even as it goes, each at least `lo`."""
    assert k >= 1 and total >= lo * k, (total, k)
    out = np.full(k, total // k, np.int64)
    out[:total % k] += 1
    return out


def build(name, vt, m, n, rows, slot, cand, samp, env=None, rungs=(), fill=None, **meta):
    """A family from its specification.  rows / slot: per entry (CSR order) its row and whether it is a slot for a candidate
    column; cand / samp: the candidate columns and how often the sample is to meet each (their sum = the sampled slots: every
    sampled slot is placed).  The slots the sample does not read take the columns of `fill` (default: the candidates sampled
    at least twice) in turn; every other entry takes a column of its own, referenced nowhere else."""
    rows, slot = np.asarray(rows, np.int64), np.asarray(slot, bool)
    cand, samp = np.asarray(cand, np.int64), np.asarray(samp, np.int64)
    nnz = rows.size
    sampled = sampled_mask(nnz)
    hs, hu, cold = np.flatnonzero(slot & sampled), np.flatnonzero(slot & ~sampled), np.flatnonzero(~slot)
    assert hs.size == int(samp.sum()), (name, hs.size, int(samp.sum()))
    cols = np.full(nnz, -1, np.int64)
    rng = np.random.default_rng(7)
    cols[hs] = np.repeat(cand, samp)[rng.permutation(hs.size)]
    fill = cand[samp >= 2] if fill is None else np.asarray(fill, np.int64)
    if hu.size:
        cols[hu] = fill[(np.arange(hu.size) * 7 + 3) % fill.size]
    pool = np.setdiff1d(np.arange(n, dtype=np.int64), cand)
    assert pool.size >= cold.size, (name, pool.size, cold.size)
    cols[cold] = pool[rng.permutation(pool.size)[:cold.size]]
    full = {PRE + "PB_HOT": 1}
    if n <= 16384 and m <= 20000:
        full.update(SMALL_TILES)
    full.update(env or {})
    f = LS.Family(name, vt, m, n, rows, cols, full, set(rungs), **meta)
    f.meta["sampled_cold_once"] = int((sampled & ~slot).sum())
    return f


def from_hot_lens(name, vt, hot_lens, k=8, n=8192, cold_every=3, gaps=None, env=None, rungs=(), cand=None, tail_cold=0, **meta):
    """The rows of A_hot have hot_lens entries, in that order; matrix row i of them also holds a cold entry when i is a
    multiple of cold_every.  gaps: {index of a hot row: (empty rows, cold-only rows) put in front of it}; tail_cold cold-only
    rows follow the last hot row.  k candidate columns
    spread over [0, n), all sampled about equally often (fewer when the sample is too small for two references each)."""
    hot_lens = np.asarray(hot_lens, np.int64)
    hot_n, cold_n = [], []
    for i, h in enumerate(hot_lens.tolist()):
        if gaps and i in gaps:
            e, c_ = gaps[i]
            hot_n += [0] * (e + c_)
            cold_n += [0] * e + [2] * c_
        hot_n.append(h)
        cold_n.append(1 if i % cold_every == 0 else 0)
    hot_n, cold_n = np.array(hot_n + [0] * tail_cold, np.int64), np.array(cold_n + [2] * tail_cold, np.int64)
    rows, slot = entry_layout(hot_n, cold_n)
    hs = int((slot & sampled_mask(rows.size)).sum())
    if int(cold_n.sum()) + k > n - 64:
        n = (int(cold_n.sum()) + k + 4096) // 256 * 256
    k = max(1, min(k, hs // 2))
    if cand is None:
        cand = np.unique(np.concatenate([[0, n - 1], (np.arange(k) * (n // k) + 77) % n]))[:k] if k > 2 else np.array([77, n - 1])[:k]
    return build(name, vt, hot_n.size, n, rows, slot, cand, spread(hs, len(cand)), env, rungs, hot_per_row=hot_n, **meta)


def rows_from_starts(starts, n_hot):
    """Row lengths of A_hot from the positions its rows start on (the first is 0)."""
    s = np.unique(np.concatenate([[0], np.asarray(starts, np.int64)]))
    return np.diff(np.append(s, n_hot))


# ------------------------------------------------------------------------------------------------------------- families
def starts_plus(vt):
    win = constants()["HOT_WIN"]
    return from_hot_lens("starts_plus", vt, [win + 1] * (win + 1), rungs=range(win))


def starts_minus(vt):
    win = constants()["HOT_WIN"]
    return from_hot_lens("starts_minus", vt, [win - 1] * (win + 1), rungs=range(win))


def pairs(vt):
    """Per gap d and offset o in {0, 3}: a window with starts on o and o + d (and on 0), the second row running to its end."""
    win = constants()["HOT_WIN"]
    lens = []
    for d in PAIR_GAPS:
        for o in (0, 3):
            lens += ([o] if o else []) + [d, win - o - d]
    return from_hot_lens("pairs", vt, lens, rungs=PAIR_GAPS)


def nibbles(vt):
    """One window per (lane, pattern): row starts on the entries 4 lane + j of the set bits j; nothing else starts there, so
    the row before runs in across the window's first entry unless the pattern itself starts it."""
    c = constants()
    win, epl = c["HOT_WIN"], c["HOT_EPL"]
    starts, spec = [], []
    for ln in NIBBLE_LANES:
        for pat in range(1 << epl):
            w = len(spec) + 1                       # (window 0 holds the first row's start and nothing of the ladder)
            spec.append((ln, pat))
            starts += [w * win + epl * ln + j for j in range(epl) if pat >> j & 1]
    n_hot = (len(spec) + 1) * win + 9
    return from_hot_lens("nibbles", vt, rows_from_starts(starts, n_hot), rungs=spec, spec=spec)


def starts_per_window(vt):
    """Per count s of START_COUNTS one window with exactly s starts, rows of one and two entries (s < HOT_WIN / 2: and a last
    row that fills the window).  First aligned -- every window starts a row on position 0 and ends one on its last --, then,
    behind a single entry, the same again: every window has a head of one entry and a tail."""
    win = constants()["HOT_WIN"]
    block = []
    for s in START_COUNTS:
        if 2 * s >= win:
            lens = [1] * (2 * s - win) + [2] * (win - s)
        else:
            lens = [1 + i % 2 for i in range(s - 1)]
            lens.append(win - sum(lens))
        assert len(lens) == s and sum(lens) == win
        block += lens
    return from_hot_lens("starts_per_window", vt, block + [win + 1] + block + [5], rungs=START_COUNTS, cold_every=7)


def long_rows(vt):
    """Per span k: a row that starts on position 100 and ends k windows later, at once a second one of k windows, a short row
    up to the window's end.  The last row runs through three windows without a start into a partial last window."""
    win = constants()["HOT_WIN"]
    lens = []
    for k in LONG_SPANS:
        lens += [100, k * win + 100, k * win + 30, 26]
    lens += [3 * win + 77]
    f = from_hot_lens("long_rows", vt, lens, rungs=LONG_SPANS)
    # the first hot column stays out of the last row and of every fourth one (for the run with a non-finite x there)
    cols, counts = np.unique(f.colind, return_counts=True)
    first, second = cols[counts > 1][:2]
    for r in list(range(1, f.shape[0], 4)) + [f.shape[0] - 1]:
        row = f.colind[f.rowptr[r]:f.rowptr[r + 1]]
        row[row == first] = second
    return f


def ends(vt, case):
    """n_hot of END_CASES in rows of 7 hot entries (the last one shorter)."""
    n_hot = END_CASES[case]
    lens = [7] * (n_hot // 7) + ([n_hot % 7] if n_hot % 7 else [])
    return from_hot_lens("ends_" + case, vt, lens, rungs={case}, cold_every=2)


def one_hot_row(vt):
    """m_hot = 1: one row of 300 hot entries among cold-only rows."""
    return from_hot_lens("one_hot_row", vt, [300], tail_cold=40, rungs={1}, k=4)


M_HOT_CASES = tuple(constants()["SCAN_BLOCK"] + d for d in (-1, 0, 1))


def scan_block(vt, m_hot):
    """m_hot around the 2 048 items of the scan's block: rows of two hot entries."""
    return from_hot_lens(f"scan_block_{m_hot}", vt, [2] * m_hot, rungs={m_hot}, cold_every=5)


def gaps(vt):
    """First and last row hot, 5 000 empty rows between hot rows, hot-only rows (every row but each third), cold-only rows."""
    lens = [9, 300, 5, 4, 600, 3, 11]
    return from_hot_lens("gaps", vt, lens, gaps={1: (5000, 0), 3: (0, 30), 4: (5000, 7), 6: (1, 1)}, rungs={"gaps"})


def walk(vt, k, r):
    """16 k + r windows for SPBLAS_GFX950_PB_HOT_GRID=1: rows of 1 ... 9 entries, every 40th of 300 and every 97th of 700 (windows
    without a start)."""
    win = constants()["HOT_WIN"]
    n_hot = (16 * k + r - 1) * win + 77
    return from_hot_lens(f"walk_{k}_{r}", vt, _mixed_rows(n_hot), env={PRE + "PB_HOT_GRID": 1}, rungs={(k, r)})


def _mixed_rows(n_hot):
    lens, total, i = [], 0, 0
    while total < n_hot:
        h = 700 if i % 97 == 96 else 300 if i % 40 == 39 else 1 + i % 9
        h = min(h, n_hot - total)
        lens.append(h)
        total += h
        i += 1
    return lens


def walk_default(vt, cus):
    """2 * 16 * CUs + 3 windows under the default grid: every wavefront walks two windows, three of them a third."""
    win = constants()["HOT_WIN"]
    nwin = 2 * 16 * cus + 3
    return from_hot_lens("walk_default", vt, _mixed_rows((nwin - 1) * win + 131), k=64, cold_every=4, rungs={nwin}, cus=cus)


def hot_list(vt, k):
    """K hot columns, every one sampled twice or three times: rows of 12 hot entries and a cold one in every fourth."""
    m = cdiv(k * 34, 12) + 8
    while True:
        hot_n, cold_n = np.full(m, 12, np.int64), (np.arange(m) % 4 == 0).astype(np.int64)
        rows, slot = entry_layout(hot_n, cold_n)
        hs = int((slot & sampled_mask(rows.size)).sum())
        if hs >= 2 * k + k // 8:
            break
        m += max(8, m // 16)
    n = (k + int(cold_n.sum()) + 4096) // 256 * 256 + 3
    cand = np.unique(np.concatenate([[0, n - 1], 1 + (np.arange(k, dtype=np.int64) * ((n - 2) // k))]))[:k] if k > 2 else np.array([5, n - 1])[:k]
    assert cand.size == k
    return build(f"hot_list_{k}", vt, m, n, rows, slot, cand, spread(hs, k), rungs={k})


def thr_rises(vt, kept):
    """hot_max_cols + 1 columns qualify: a few sampled HEAVY times, all the others twice.  The columns sampled twice no longer
    fit, so the threshold rises to 3 and only the heavy ones are taken: kept -- they carry the share -- or, with fewer of them,
    refused by the sample's test, where the ordinary tiled plan is built."""
    kmax, heavy = hot_max_cols(vt), 1000
    pct = constants()["MIN_PCT"]
    n_heavy = 1
    while True:                                  # the smallest count of heavy columns that carries the share
        n_light = kmax + 1 - n_heavy
        if n_heavy * heavy * 100 >= (n_heavy * heavy + 2 * n_light) * pct:
            break
        n_heavy += 1
    if not kept:
        n_heavy -= 1
    n_light = kmax + 1 - n_heavy
    total = n_heavy * heavy + 2 * n_light
    m = cdiv(total * 16, 12)
    while True:                                  # rows of 12 slots, no cold entries but one: as many rows as the sample needs
        hot_n = np.full(m, 12, np.int64)
        cold_n = np.zeros(m, np.int64)
        cold_n[1] = 1
        rows, slot = entry_layout(hot_n, cold_n)
        sm = sampled_mask(rows.size)
        hs = int((slot & sm).sum())
        if hs >= total:
            break
        m += 8
    extra = np.flatnonzero(slot & sm)[total:]    # sampled slots beyond what the rung needs become entries of their own
    slot[extra] = False
    n = (2 * (kmax + 1) + int((~slot).sum()) + 4096) // 256 * 256
    cand = np.arange(kmax + 1, dtype=np.int64) * 2 + 1
    samp = np.concatenate([np.full(n_heavy, heavy), np.full(n_light, 2)]).astype(np.int64)
    return build("thr_rises_" + ("kept" if kept else "refused"), vt, m, n, rows, slot, cand, samp, fill=cand[:n_heavy],
                 rungs={"kept" if kept else "refused"}, n_heavy=n_heavy)


def col_edges(vt, mod):
    """Hot columns 0, 63, 64 and n - 1 with n = 1 024 + mod: the last word of hot_colmap_kernel's bitmap is partial."""
    n = 1024 + mod
    return from_hot_lens(f"col_edges_{mod}", vt, [9] * 120, k=4, n=n, cand=np.array([0, 63, 64, n - 1]), rungs={mod},
                         env=SMALL_TILES)


def clipped(vt):
    """Five columns sampled 1 021, 1 022, 1 023, 1 024 and 5 000 times (the last bucket of the histogram holds the last three),
    many times in one row."""
    total = sum(CLIP_COUNTS)
    m = 64
    while True:
        hot_n, cold_n = np.full(m, 2400, np.int64), np.full(m, 3, np.int64)
        rows, slot = entry_layout(hot_n, cold_n)
        sm = sampled_mask(rows.size)
        if int((slot & sm).sum()) >= total:
            break
        m += 1
    slot[np.flatnonzero(slot & sm)[total:]] = False
    n = (int((~slot).sum()) + 4096) // 256 * 256
    return build("clipped", vt, m, n, rows, slot, np.array([10, 200, 3000, 4000, n - 2]), np.array(CLIP_COUNTS), rungs=CLIP_COUNTS)


def share(vt, which):
    """30 720 entries (60 groups of 16 lines), 1 920 of them sampled.  exact: 288 sampled references in 96 hot columns -- the
    sample's share is the limit exactly; minus_one: 287; promise: every sampled entry hot, but 14 per cent of the matrix;
    all_hot: no entry left."""
    nnz, m = 30720, 960
    rows = np.repeat(np.arange(m, dtype=np.int64), nnz // m)
    sm = sampled_mask(nnz)
    assert int(sm.sum()) == nnz // 16
    slot = np.zeros(nnz, bool)
    spos, upos = np.flatnonzero(sm), np.flatnonzero(~sm)
    pct = constants()["MIN_PCT"]
    if which in ("exact", "minus_one"):
        assert nnz // 16 * pct % 100 == 0
        want = nnz // 16 * pct // 100 - (1 if which == "minus_one" else 0)
        slot[spos[::6][:want]] = True
        slot[upos[::5]] = True                                 # 5 760 unsampled slots: the matrix holds more than the limit
        k = 96
    elif which == "promise":
        slot[spos] = True
        slot[upos[:cdiv(nnz * (pct - 1), 100) - spos.size]] = True
        assert nnz * (pct - 1) <= int(slot.sum()) * 100 < nnz * pct
        k = 50
    else:
        slot[:] = True
        k = 50
    hs = int((slot & sm).sum())
    n = 32768 + 64
    cand = np.arange(k, dtype=np.int64) * 97 + 5
    return build("share_" + which, vt, m, n, rows, slot, cand, spread(hs, k), rungs={which})


def depth2(vt):
    """SPBLAS_GFX950_PB_HOT_DEPTH=2.  Eight columns take a third of the entries; four more are referenced only where the first
    sample does not look, a tenth of the remainder (more than the second limit, less than the first): the second sample,
    over the arrays of the remainder, finds them."""
    m, per = 600, 40
    rows = np.repeat(np.arange(m, dtype=np.int64), per)
    nnz = rows.size
    sm = sampled_mask(nnz)
    j = np.arange(nnz) % per
    slot = j < 14
    n = 32768
    cand = np.array([0, 77, 511, 512, 4095, 4096, 6000, n - 1])
    f = build("depth2", vt, m, n, rows, slot, cand, spread(int((slot & sm).sum()), cand.size),
              env={PRE + "PB_HOT_DEPTH": 2}, rungs={2})
    second = np.array([9, 640, 8000, 20001])
    at = np.flatnonzero(~slot & ~sm & (j % 10 == 5))
    f.colind[at] = second[np.arange(at.size) % second.size]
    f.meta["second"] = second
    return f


SMALL = ["starts_plus", "starts_minus", "pairs", "nibbles", "starts_per_window", "long_rows", "one_hot_row", "gaps", "clipped",
         "depth2"] + ["ends_" + c_ for c_ in END_CASES] + [f"scan_block_{v}" for v in M_HOT_CASES] + \
    [f"col_edges_{v}" for v in N_MOD]
WALKS = [f"walk_{k}_{r}" for k, r in WALK_CASES]
REFUSED = {"thr_rises_refused": "sample", "share_minus_one": "sample", "share_promise": "matrix", "share_all_hot": "matrix"}
SHARES = ["share_exact", "share_minus_one", "share_promise", "share_all_hot"]


def hot_list_names(vt):
    return [f"hot_list_{k}" for k in k_rungs(vt)] + ["thr_rises_kept", "thr_rises_refused"]


_FAMILIES = {}


def family(name, vt, cus=256):
    """Families by name, built once per process (host arrays; never written to)."""
    key = (name, vt, cus if name == "walk_default" else 0)
    if key in _FAMILIES:
        return _FAMILIES[key]
    if name.startswith("ends_"):
        f = ends(vt, name[5:])
    elif name.startswith("scan_block_"):
        f = scan_block(vt, int(name[11:]))
    elif name.startswith("col_edges_"):
        f = col_edges(vt, int(name[10:]))
    elif name.startswith("walk_") and name != "walk_default":
        f = walk(vt, *[int(v) for v in name[5:].split("_")])
    elif name == "walk_default":
        f = walk_default(vt, cus)
    elif name.startswith("hot_list_"):
        f = hot_list(vt, int(name[9:]))
    elif name.startswith("thr_rises_"):
        f = thr_rises(vt, name.endswith("kept"))
    elif name.startswith("share_"):
        f = share(vt, name[6:])
    else:
        f = globals()[name](vt)
    assert f.name == name, (f.name, name)
    _FAMILIES[key] = f
    return f


_LAYOUTS = {}


def layouts(fam, cus=256):
    """(splits, their layouts) of a family under its own hooks; when the first split is refused: (0, [that layout])."""
    key = (fam.name, fam.vt, cus)
    if key not in _LAYOUTS:
        n_, lays = depth(fam.vt, fam.rowptr, fam.colind, fam.shape, fam.env, cus)
        if not lays:
            lays = [inspect(fam.vt, fam.rowptr, fam.colind, fam.shape, fam.env, cus)]
        _LAYOUTS[key] = (n_, lays)
    return _LAYOUTS[key]
