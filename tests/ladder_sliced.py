"""Tile ladders for the SLICED SpMV plan (csrc/spmv_sliced.hip): deterministic matrices built from a TILE specification, a host
restatement of the tiling that says which rung every matrix holds, and a host model of the launch pair that shows the
checkers fail what they must (tests/test_ladders_sliced_cpu.py); tests/test_gpu_sliced_ladders.py runs them on the device.

The plan cuts the columns into S slices of W and the rows into NB bins of H.  The entries of tile (slice, bin) form a RUN;
in the expand's stream A' (slice-major) a run occupies its count rounded up to 4 entries, in the product stream P
(bin-major) it is padded to whole BLOCKS of 128 bytes (BLK entries), and a bin's runs together to whole GROUPS of PB_GRP
entries.  The reduce walks a bin's groups in two batches of UB groups in flight, clamps the loads past the end, may cut the
stream into K parts, adds entries whose row repeats inside a group atomically (duplicate flags) and -- with one-byte row
codes -- the entries the codes cannot reach from a per-bin exception list.  The row-length ladder of tests/ladder.py walks
through ONE slice and never meets any of these edges; the families below put an input on each:

  runs         per-tile entry counts 0, 1, 3, 4, 5, BLK - 1, BLK, BLK + 1, 2 BLK - 1, 2 BLK + 1 in the first, a middle and the
               last slice of a bin; the last tiles of A' and of P are empty
  groups       one bin per group count 0 ... 34, padded from g PB_GRP - d entries, d in {0, 1, BLK, BLK + 1}
  col_edges    entries on s W - 1, s W, s W + 1 for every slice edge, on columns 0 and n - 1; last slices of 1 and W - 1 columns,
               whole slices empty, an asked width pick_tiling changes (100 -> 96), the natural widths around 20 480 and 40 960
  row_edges    entries on local rows 0, H - 1 and the first row of the next bin; m = k H - 1, k H, k H + 1; empty bins first,
               middle and last
  dups         one row holding c entries of one tile, c in {1 ... 5, 63, 64, 65, 255, 256, 257}, starting on each position of a
               lane's quad, straddling a block edge and a group edge, met again in the next slice's run, two such rows in a row
  row_codes    H asked 4 000: row advances 0, 1, 254, 255, 256, 509, 510, 511 inside a block, a block base on row H - 1, bins
               with exactly 0, 1, PB_EXC_CAP - 1, PB_EXC_CAP exceptions, and (a matrix of its own) PB_EXC_CAP + 1

  hub_rows     rows of window - 1, window, window + 1 entries in arithmetic bins: the longer ones stay out of the tiles
  hub_len      PB_HUB_LEN - 1, PB_HUB_LEN, PB_HUB_LEN + 1 entries under variable bins
  split_rows   rows of k L - 1 and k L + 1 entries, k = 2, 3, 9, cut into pieces of L = PB_SPLIT_LEN that fall into different bins
  compact      PB_COMPACT=1 with empty rows leading, trailing, in stretches and alone between full rows
  skew_cols / skew_rows   one slice / one group of bins above 3 x the mean: the expand's and the reduce's work lists
  many_groups  variable bins in more than 2 x the CUs groups with one heavy stretch: the reduce list sorted heaviest first
               (PB_LPT=0: in group order) with split groups, and the scatter's bin order
  bin_span     a bin whose rows span 65 535, 65 536, 65 537 entries of the caller's arrays (16-bit staging)
  slice_aligned  fp64, a slice count just below the CU count: rounded up to it, one expand work item per slice
  many_slices  more slices than the staged scatter takes: the direct scatter, unasked
  hot_split    PB_HOT=1: rows with HOT_WIN - 1 ... 2 HOT_WIN + 1 entries in columns the sample must take

Families that are not about the row map pin the arithmetic bins (SPBLAS_GFX950_PB_VARBINS=0) next to the geometry hooks
SLICE_COLS / SLICE_ROWS; row_map() and plan_rows() restate the row map and the variable-height bins for those that are.

Checks and data come from tests/ladder.py (cast / wide / check_exact / check_random / exact_spmv_data / max_partial_sum /
spmv_reference); no tolerance is introduced here.  exact_data() takes the zeros out of the integer data, so that every
single entry counts in the bit-exact run.
"""
import re

import numpy as np

import ladder as L

ITEM = {"f32": 4, "f64": 8}
GROUP_COUNTS = range(0, 35)
RUN_POSITIONS = ("first", "middle", "last")
DUP_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257)
ROW_ADVANCES = (0, 1, 254, 255, 256, 509, 510, 511)
ARITHMETIC = {"SPBLAS_GFX950_PB_VARBINS": "0"}


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ constants
def _one(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the source no longer has the expected form; update tests/ladder_sliced.py"
    return int(m.group(1))


_CONST = {}


def constants():
    """Every constant the tiling depends on, parsed from csrc/spmv_sliced.hip and csrc/spmv_hot.hip."""
    if _CONST:
        return _CONST
    src, hot = L._src("spmv_sliced.hip"), L._src("spmv_hot.hip")
    c = {}
    c["PB_GRP"] = _one(r"static constexpr int PB_GRP = (\d+);", src, "PB_GRP")
    c["BLK_BYTES"] = _one(r"static constexpr int BLK = (\d+) / \(int\) sizeof\(T\);", src, "pb_geom::BLK")
    assert _one(r"static constexpr int GBLK = (\d+) / BLK;", src, "pb_geom::GBLK") == c["PB_GRP"]
    c["PB_EXC_CAP"] = _one(r"static constexpr int PB_EXC_CAP = (\d+);", src, "PB_EXC_CAP")
    c["PB_STAGE_MAX_S"] = _one(r"static constexpr int PB_STAGE_MAX_S = (\d+);", src, "PB_STAGE_MAX_S")
    c["PB_STAGE_SP"] = _one(r"static constexpr int PB_STAGE_SP = (\d+);", src, "PB_STAGE_SP")
    c["PB_LDS_BYTES"] = _one(r"static constexpr int PB_LDS_BYTES = (\d+) \* 1024;", src, "PB_LDS_BYTES") * 1024
    c["PB_RWAVES_DEFAULT"] = _one(r"static constexpr int PB_RWAVES_DEFAULT = (\d+);", src, "PB_RWAVES_DEFAULT")
    c["RUN_MIN"] = _one(r'env_int\("SPBLAS_GFX950_PB_RUN_MIN", (\d+)\)', src, "the shortest mean run")
    c["BINS_FILL"] = _one(r'nb_fill = env_int\("SPBLAS_GFX950_PB_BINS", (\d+)\)', src, "the bins that fill the chip")
    c["HOT_EPL"] = _one(r"#define HOT_EPL (\d+)", hot, "HOT_EPL")
    assert re.search(r"static constexpr int HOT_WIN = 64 \* HOT_EPL;", hot), "HOT_WIN: update tests/ladder_sliced.py"
    c["HOT_WIN"] = 64 * c["HOT_EPL"]
    # the forms the restatement below copies: fail loudly when they move
    flat = re.sub(r"\s+", " ", src)
    for what, pat in (
            ("pick_tiling", r"int64_t w = cdiv\(extent, p\); w = cdiv\(w, align\) \* align; if \(w > max_elems\)"),
            ("the slice call of pick_tiling", r"pick_tiling\(n, w_env > 0 && w_env < max_cols \? w_env : max_cols, xround, xround, 4, &S, &W\)"),
            ("the rows a bin may hold", r"int max_rows = rlds / RW / \(int\) sizeof\(T\) - 64;"),
            ("the bin height", r"if \(h_env > 0 && h_env < max_rows\) hh = h_env;"),
            ("blocks per run", r"aoff\[i\] = \(cnt\[i\] \+ blk - 1\) / blk;"),
            ("groups per bin", r"bintot\[b\] = \(carry \+ gblk - 1\) / gblk \* gblk;"),
            ("the compact stream", r"eoff\[i\] = \(cnt\[i\] \+ 3\) & ~3;"),
            ("the exception rule", r"D_j = min\(r_j, D_\{j-1\} \+ 255\)")):
        assert re.search(pat, flat), f"{what}: the source no longer has the expected form; update tests/ladder_sliced.py"
    _CONST.update(c)
    return _CONST


def blk(vt):
    """Entries per 128-byte block of the product stream."""
    return constants()["BLK_BYTES"] // ITEM[vt]


def gblk(vt):
    """Blocks per reduce group."""
    return constants()["PB_GRP"] // blk(vt)


# --------------------------------------------------------------------------------------------------------------- tiling
def pick_tiling(extent, max_elems, round_to=1, round_from=1, align=4):
    """(pieces, width) -- pick_tiling of spmv_sliced.hip: as few pieces as fit max_elems, the width a multiple of `align`."""
    p = max(1, cdiv(extent, max_elems))
    rounded = p > round_from
    if rounded:
        p = cdiv(p, round_to) * round_to
    w = cdiv(cdiv(extent, p), align) * align
    if w > max_elems:
        w = max_elems // align * align
    if w < align:
        w = align
    if not rounded or w * p < extent:
        p = cdiv(extent, w)
    return int(p), int(w)


class Tiling:
    pass


def tiling(vt, m, n, nnz, env=None, cus=256):
    """S, W, H, NB of the plan sliced_build_typed builds for an m x n matrix of nnz entries under the hooks in `env`:
    SPBLAS_GFX950_SLICE_COLS, SLICE_ROWS, PB_RWAVES, and -- value-free tiles, PB_VFREE=2 -- PB_VF_ROWS / PB_VF_WAVES."""
    env = env or {}
    c, item = constants(), ITEM[vt]
    lds = c["PB_LDS_BYTES"]
    wide32 = item == 4 and cdiv(n, lds // 4) >= 100
    xlds = 160 * 1024 if item == 8 or wide32 else lds
    max_cols = min(xlds // item, 65536)
    rw = int(env.get("SPBLAS_GFX950_PB_RWAVES", c["PB_RWAVES_DEFAULT"]))
    if rw not in (4, 8):
        rw = c["PB_RWAVES_DEFAULT"]
    max_rows = min(lds // rw // item - 64, 32000)
    w_env, h_env = int(env.get("SPBLAS_GFX950_SLICE_COLS", 0)), int(env.get("SPBLAS_GFX950_SLICE_ROWS", 0))
    S, W = pick_tiling(n, w_env if 0 < w_env < max_cols else max_cols)
    aligned = False
    if w_env <= 0 and xlds > lds and S <= cus and S * 10 >= cus * 9:
        w2 = cdiv(cdiv(n, cus), 4) * 4
        if w2 <= max_cols and cdiv(n, w2) <= cus:
            W, S, aligned = w2, cdiv(n, w2), True
    vf_rows = int(env.get("SPBLAS_GFX950_PB_VF_ROWS", 0))
    if int(env.get("SPBLAS_GFX950_PB_VFREE", 1)) == 2 and h_env <= 0:
        # value-free tiles: a bin is a workgroup's, as tall as the LDS window of the caller's values allows (the widest window
        # is measured on the device; the families keep it far below the capacity, so no shrinking step is restated)
        waves = int(env.get("SPBLAS_GFX950_PB_VF_WAVES", 8))
        waves = waves if waves in (4, 8) else 8
        elems = (160 * 1024 - 64) // item
        avg = nnz / m if m > 0 else 0.0
        hh = int((elems - waves * 64 - 16) / (avg * 1.02 + waves))
        hh = min(hh, elems // (2 * waves) - 64, 32000)
        if vf_rows > 0:
            hh = min(hh, vf_rows)
        H, rw = hh, 1
    else:
        nb = max(cdiv(m, max_rows), min(c["BINS_FILL"], nnz // (S * c["RUN_MIN"])), 1)
        hh = cdiv(max(m, 1), nb)
        if 0 < h_env < max_rows:
            hh = h_env
        H = max(1, min(hh, max_rows))
    t = Tiling()
    t.vt, t.m, t.n, t.S, t.W, t.H, t.NB, t.rw, t.slice_aligned = vt, m, n, int(S), int(W), int(H), int(cdiv(max(m, 1), H)), rw, aligned
    t.max_rows, t.max_cols = max_rows, max_cols
    return t


def row_map(vt, rowptr, env=None):
    """The row map of sliced_build_typed: (rowptr of the compact rows, pieces per row of y, split length in use).  Empty rows
    are taken out when they are more than a quarter of the rows (or PB_COMPACT says so), rows longer than PB_SPLIT_LEN become
    pieces of that length when the longest row is long against the mean; PB_VARBINS=0 switches both off.  No row map: the
    caller's rowptr, one piece per row, 0."""
    env = env or {}
    rowptr = np.asarray(rowptr, np.int64)
    lens = np.diff(rowptr)
    m, nnz = lens.size, int(rowptr[-1])
    empty, longest = int((lens == 0).sum()), int(lens.max()) if m else 0
    compact = int(env.get("SPBLAS_GFX950_PB_COMPACT", -1))
    if compact < 0:
        compact = int(empty * 4 > m)
    if empty == 0 or m - empty < 2:
        compact = 0
    split = int(env.get("SPBLAS_GFX950_PB_SPLIT_LEN", 32 if ITEM[vt] == 4 else 2048))
    avg0 = nnz / m if m else 0.0
    if split < 8 or longest <= 2 * split or longest <= 16.0 * avg0 + 64.0:
        split = 0
    if str(env.get("SPBLAS_GFX950_PB_VARBINS", "-1")) == "0" or m < 2:
        compact = split = 0
    if not compact and split == 0:
        return rowptr, np.ones(m, np.int64), 0
    pieces = np.where(lens == 0, 0 if compact else 1, np.where((split > 0) & (lens > split), cdiv(lens, max(split, 1)), 1))
    first = np.repeat(rowptr[:-1], pieces)
    j = np.arange(first.size) - np.repeat(np.cumsum(pieces) - pieces, pieces)
    return np.append(first + j * split, nnz), pieces, split if (pieces > 1).any() else 0


def plan_rows(vt, rowptr, shape, env=None, cus=256):
    """(tiling over the plan's rows, their rowptr, first row of every bin, hub length, row map in use) -- arithmetic bins, or
    the variable heights: a new bin every H rows and wherever the entry count before a row crosses a multiple of E."""
    env = env or {}
    rowptr = np.asarray(rowptr, np.int64)
    m, n = shape
    lens0 = np.diff(rowptr)
    nnz = int(rowptr[-1])
    rp, pieces, split = row_map(vt, rowptr, env)
    mapped = rp is not rowptr
    mc = rp.size - 1
    t = tiling(vt, mc, n, nnz, env, cus)
    empty, longest = int((lens0 == 0).sum()), int(lens0.max()) if m else 0
    varbins = int(env.get("SPBLAS_GFX950_PB_VARBINS", -1))
    if varbins < 0:
        varbins = int(longest > 16.0 * (nnz / mc if mc else 0.0) + 64.0 or empty * 4 > m)
    if mc < 2 or (t.NB < 2 and not mapped):
        varbins = 0
    if mapped:
        varbins = 1
    if int(env.get("SPBLAS_GFX950_PB_VFREE", 1)) == 2:
        assert not mapped, "value-free tiles take no row map"
        varbins = 0
    if varbins:
        E = max(8192, min(nnz // constants()["BINS_FILL"], 98304))
        r = np.arange(mc)
        flag = (r % t.H == 0) | (rp[:-1] // E != np.concatenate([[0], rp[:-2]]) // E)
        flag[0] = True
        binrow = np.append(np.flatnonzero(flag), mc)
        t.NB = binrow.size - 1
    else:
        binrow = np.minimum(np.arange(t.NB + 1, dtype=np.int64) * t.H, mc)
    win = L.thresholds()["window_" + vt]
    n_long = int((lens0 > win).sum())
    hub_len = win if n_long else 0
    if split > 0:
        hub_len = 0
    elif varbins and n_long:
        hub2 = max(win, int(env.get("SPBLAS_GFX950_PB_HUB_LEN", 16384)))
        if longest <= hub2:
            hub_len = 0
        elif hub2 > win or mapped:
            hub_len = hub2
    t.variable_bins, t.binrow, t.mapped = int(bool(varbins)), binrow, mapped
    return t, rp, binrow, hub_len, mapped


def tile_counts(rowptr, colind, t, hub_len=0, binrow=None):
    """cnt[slice, bin]: the entries of every tile (rows longer than hub_len > 0 stay out of the tiles).  `rowptr`: the rows
    the plan tiles (compact rows and pieces under a row map); `binrow`: first row of every bin (default: every H rows)."""
    rowptr = np.asarray(rowptr, np.int64)
    lens = np.diff(rowptr)
    nnz = int(rowptr[-1])
    rows = np.searchsorted(rowptr, np.arange(nnz), side="right") - 1
    cols = np.asarray(colind[:nnz], np.int64)
    keep = lens[rows] <= hub_len if hub_len > 0 else np.ones(nnz, bool)
    bins = rows // t.H if binrow is None else np.searchsorted(binrow, rows, side="right") - 1
    key = (cols[keep] // t.W) * t.NB + bins[keep]
    return np.bincount(key, minlength=t.S * t.NB).reshape(t.S, t.NB)


def predicted_info(vt, rowptr, colind, shape, env=None, cus=256):
    """The keys of plan.info() / plan.sliced_info() the restatement covers."""
    env = env or {}
    t, rp, binrow, hub_len, mapped = plan_rows(vt, rowptr, shape, env, cus)
    lens = np.diff(rp)
    hubs = int((lens > hub_len).sum()) if hub_len else 0
    cnt = tile_counts(rp, colind, t, hub_len, binrow)
    b, g = blk(vt), gblk(vt)
    blocks = cdiv(cnt, b)
    x_items, r_items = work_lists(vt, cnt, t, env, cus)
    return {"expand_items": x_items, "reduce_items": r_items, "n_slices": t.S, "rows_per_bin": t.H, "n_bins": t.NB,
            "variable_bins": t.variable_bins, "expand_blocks": int(blocks.sum()),
            "reduce_blocks": int((cdiv(blocks.sum(axis=0), g) * g).sum()), "placed_entries": int(cnt.sum()),
            "hub_rows": hubs, "hub_len": hub_len, "tiled_rows": rp.size - 1}


def work_lists(vt, cnt, t, env=None, cus=256):
    """(expand items, reduce items) of the plan's work lists, 0 where it has none.  Expand: one item per non-empty slice when
    the slices are aligned to the CUs and even; parts of at most `target` blocks per slice when one slice holds more than 3 x
    the mean.  Reduce: when one group of RW bins holds more than 3 x the mean, a group of tot entries is cut into
    (tot + target / 2) / target parts, target = max(total / 768, 16 384), as long as a part keeps 4 groups per bin; variable
    bins in more than 2 x the CUs groups get the list for its heaviest-first order alone from 1.5 x the mean on (PB_LPT)."""
    env = env or {}
    b, grp = blk(vt), constants()["PB_GRP"]
    per_slice, total = cnt.sum(axis=1), int(cnt.sum())
    sblocks = cdiv(cnt, b).sum(axis=1)
    x_items = 0
    if t.slice_aligned and total > 0 and int(per_slice.max()) * t.S <= 1.05 * total:
        x_items = int((sblocks > 0).sum())
    elif total > 0 and int(per_slice.max()) * t.S > 3 * total:
        target = max(cdiv(int(sblocks.sum()), 2 * cus), 4 * t.W // b)
        for nb in sblocks[sblocks > 0]:
            parts = max(1, cdiv(int(nb), target))
            per = cdiv(int(nb), parts)
            x_items += sum(1 for k in range(parts) if min(k * per, nb) < min((k + 1) * per, nb))
    r_items = 0
    ngroups = cdiv(t.NB, t.rw)
    vfree = int(env.get("SPBLAS_GFX950_PB_VFREE", 1)) == 2
    tot_g = np.add.reduceat(cnt.sum(axis=0), np.arange(0, t.NB, t.rw)) if t.NB else np.zeros(0, np.int64)
    big = int(tot_g.max()) * ngroups if t.NB else 0
    # variable bins with more groups than the chip holds at once: a list in heaviest-first order even when no group is cut
    lpt = bool(int(env.get("SPBLAS_GFX950_PB_LPT", 1)) and getattr(t, "variable_bins", 0) and ngroups > 2 * cus and
               big > (3 * total) // 2)
    if not vfree and total > 0 and ngroups > 1 and (big > 3 * total or lpt):
        target = max(total // 768, 16384)
        kg = [min(256, max(1, min((int(tg) + target // 2) // target, max(1, int(tg) // (t.rw * 4 * grp))))) for tg in tot_g]
        if lpt and big <= 3 * total:
            kg = [1] * len(kg)
        if any(k > 1 for k in kg) or lpt:
            r_items = sum(kg)
    return x_items, r_items


def source_position_bytes(vt, cnt, t):
    """What a plan that keeps the source position of every entry adds to info()["device_bytes"]: 4 B per entry of the compact
    stream A' (the runs rounded up to 4, plus one block of slack) and the bin-major run table (8 B per tile)."""
    return 4 * (compact_stream_entries(cnt) + blk(vt)) + 8 * t.S * t.NB


def groups_per_bin(vt, cnt):
    return cdiv(cdiv(cnt, blk(vt)).sum(axis=0), gblk(vt))


def compact_stream_entries(cnt):
    """Entries of the expand's stream A': every run rounded up to 4."""
    return int(((cnt + 3) & ~3).sum())


def _tile_entries(rowptr, colind, t):
    """Per entry: (bin, slice, local row), and the order of the product stream (bin-major, runs in slice order, a run's entries
    by row -- the staged scatter's order; CSR order within a row)."""
    lens = np.diff(rowptr)
    rows = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    cols = np.asarray(colind[:rows.size], np.int64)
    b, s = rows // t.H, cols // t.W
    order = np.lexsort((np.arange(rows.size), rows, s, b))
    return b, s, rows - b * t.H, order


def enc8_exceptions(rowptr, colind, t):
    """Entries per bin the one-byte row codes cannot reach: inside a block of a run (sorted by row) the decoder follows
    D_j = min(r_j, D_{j-1} + 255); entry j is an exception iff r_j - D_{j-1} >= 255."""
    b, s, r, order = _tile_entries(rowptr, colind, t)
    out = np.zeros(t.NB, np.int64)
    bl = blk(t.vt)
    key = (b * t.S + s)[order]
    rr = r[order]
    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if key.size else np.zeros(0, np.int64)
    ends = np.append(starts[1:], key.size)
    for lo, hi in zip(starts, ends):
        for k0 in range(lo, hi, bl):
            d = rr[k0]
            for rj in rr[k0 + 1:min(k0 + bl, hi)]:
                if rj - d >= 255:
                    out[key[lo] // t.S] += 1
                    d += 255
                else:
                    d = rj
    return out


def bin_span(rowptr, t):
    """Widest stretch of the caller's arrays one bin's rows cover (decides 16-bit staging)."""
    edges = np.minimum(np.arange(t.NB + 1, dtype=np.int64) * t.H, t.m)
    return int(np.diff(np.asarray(rowptr, np.int64)[edges]).max())


# ------------------------------------------------------------------------------------------------------------- families
class Family:
    """name, vt, rowptr (int64), colind (int32), shape, env (the hooks of the inspect call), rungs (what it claims to hold)."""

    def __init__(self, name, vt, m, n, rows, cols, env, rungs, **meta):
        rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        assert rows.size == cols.size and (rows.size == 0 or (0 <= rows.min() and rows.max() < m and 0 <= cols.min() and cols.max() < n))
        order = np.argsort(rows, kind="stable")
        self.rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int64)
        self.colind = cols[order].astype(np.int32)
        self.name, self.vt, self.shape, self.rungs, self.meta = name, vt, (int(m), int(n)), rungs, meta
        self.env = dict(ARITHMETIC, **{k: str(v) for k, v in env.items()})
        self.nnz = int(rows.size)

    def tiling(self, extra=None):
        return tiling(self.vt, self.shape[0], self.shape[1], self.nnz, dict(self.env, **(extra or {})))

    def predicted(self, extra=None, cus=256):
        return predicted_info(self.vt, self.rowptr, self.colind, self.shape, dict(self.env, **(extra or {})), cus)


def exact_data(fam):
    """(values, x) of ladder.exact_spmv_data with every 0 replaced by 1: still integers from {-1, 1} and {-2 ... 2} whose
    partial sums stay exact in any order (asserted again), but no product is 0 -- a rung that rests on ONE entry (the entry
    that straddles a block edge, the last entry of a run) changes the integer result when that entry is lost or doubled."""
    values, x = L.exact_spmv_data(fam.rowptr, fam.colind, fam.shape[1])
    values, x = np.where(values == 0, 1.0, values), np.where(x == 0, 1.0, x)
    seq, anyorder = L.max_partial_sum(fam.rowptr, fam.colind, values, x)
    assert anyorder < 2 ** 24 and seq < 2 ** 24 and (values * x[fam.colind] != 0).all()
    return values, x


def _hooks(w, h):
    return {"SPBLAS_GFX950_SLICE_COLS": w, "SPBLAS_GFX950_SLICE_ROWS": h}


def _tile(b, s, count, H, W, row_step=7, row0=0):
    """(rows, cols) of `count` entries of tile (s, b): local rows row0, row0 + row_step, ... modulo H, columns walking the slice."""
    k = np.arange(count, dtype=np.int64)
    return b * H + (row0 + k * row_step) % H, s * W + (k * 5 + b) % W


def runs(vt):
    """Every run length of run_counts(vt) in the first, a middle and the last slice of a bin of 4 slices; the other tiles of the
    bin walk the same counts.  The last bin has one entry in slice 0: the last tiles of A' (slice-major) and of P are empty."""
    S, W, H = 4, 64, 37
    counts = run_counts(vt)
    pos_slice = {"first": 0, "middle": 2, "last": S - 1}
    rows, cols, spec = [], [], []
    for i, c in enumerate(counts):
        for pos in RUN_POSITIONS:
            b = len(spec)
            tile = [counts[(i + 3 * s + b) % len(counts)] for s in range(S)]
            tile[pos_slice[pos]] = c
            spec.append(tile)
    spec.append([0, 2 * blk(vt), 0, 0])      # an empty first tile, empty last tiles
    spec.append([1, 0, 0, 0])
    for b, tile in enumerate(spec):
        for s, c in enumerate(tile):
            r, cc = _tile(b, s, c, H, W, row0=3 * s)
            rows.append(r)
            cols.append(cc)
    m = len(spec) * H
    rungs = {(c, pos) for c in counts for pos in RUN_POSITIONS}
    return Family("runs", vt, m, S * W, np.concatenate(rows), np.concatenate(cols), _hooks(W, H), rungs, spec=np.array(spec).T,
                  pos_slice=pos_slice)


def run_counts(vt):
    b = blk(vt)
    return [0, 1, 3, 4, 5, b - 1, b, b + 1, 2 * b - 1, 2 * b + 1]


def group_deltas(vt):
    return (0, 1, blk(vt), blk(vt) + 1)


def groups(vt):
    """One bin per (g, d): g PB_GRP - d entries, cut on block boundaries over 4 slices (the remainder goes to slice (g + i) % 4),
    so that the bin's blocks round up to exactly g groups.  Rows repeat inside the tiles (H = 500): duplicate flags everywhere."""
    S, W, H = 4, 64, 500
    grp, b = constants()["PB_GRP"], blk(vt)
    rows, cols, spec = [], [], []
    for g in GROUP_COUNTS:
        for i, d in enumerate(group_deltas(vt)):
            e = g * grp - d
            if e < 0 or (g > 0 and cdiv(e, b) <= (g - 1) * gblk(vt)):
                continue
            q, rem = divmod(e, b)
            tile = [(q // S + (1 if s < q % S else 0)) * b for s in range(S)]
            tile[(g + i) % S] += rem
            bn = len(spec)
            spec.append((g, d, tile))
            for s, c in enumerate(tile):
                r, cc = _tile(bn, s, c, H, W, row_step=3, row0=s)
                rows.append(r)
                cols.append(cc)
    m = len(spec) * H
    rungs = {(g, d) for g, d, _ in spec}
    return Family("groups", vt, m, S * W, np.concatenate(rows), np.concatenate(cols), _hooks(W, H), rungs,
                  spec=[(g, d) for g, d, _ in spec])


COL_EDGE_CASES = {
    # name: (n, asked width or 0 for the natural one, slices left empty)
    "last_slice_1_col": (15 * 64 + 1, 64, ()),      # (pick_tiling evens the widths out: 16 pieces keep 64)
    "last_slice_w_minus_1": (16 * 64 - 1, 64, ()),
    "asked_100_gets_96": (2111, 100, ()),
    "empty_slices": (10 * 64, 64, (0, 5, 9)),
    "natural_20480": (20480, 0, ()),
    "natural_20481": (20481, 0, ()),
    "natural_40960": (40960, 0, ()),
    "natural_40961": (40961, 0, ()),
}


def col_edges(vt, case):
    """Entries on s W - 1, s W, s W + 1 for every slice edge and on columns 0 and n - 1 (those of the slices left empty taken
    out); every bin of 3 sees every such column, 4 per row."""
    n, w_ask, empty = COL_EDGE_CASES[case]
    S, W = pick_tiling(n, w_ask if w_ask else tiling(vt, 2, n, 0).max_cols)
    edge = sorted({c for s in range(S + 1) for c in (s * W - 1, s * W, s * W + 1) if 0 <= c < n} | {0, n - 1})
    edge = np.array([c for c in edge if c // W not in empty], np.int64)
    H = cdiv(edge.size, 2) + 1             # 4 columns per row, every column twice per bin
    m = 3 * H - 1
    rows = np.repeat(np.arange(m, dtype=np.int64), 4)
    cols = edge[(4 * (rows % H) + np.tile(np.arange(4), m)) % edge.size]
    env = {"SPBLAS_GFX950_SLICE_ROWS": H}
    if w_ask:
        env["SPBLAS_GFX950_SLICE_COLS"] = w_ask
    return Family("col_edges_" + case, vt, m, n, rows, cols, env, set(edge.tolist()), S=S, W=W, empty=empty, edge=edge)


ROW_EDGE_CASES = {"m_kH_minus_1": (3, -1, ()), "m_kH": (3, 0, ()), "m_kH_plus_1": (3, 1, ()), "empty_bins": (5, 0, (0, 2, 4))}


def row_edges(vt, case):
    """Entries on local rows 0, 1, H - 2, H - 1 of every bin (2 per slice and row), m = k H + d; `empty_bins`: bins 0, 2 and 4 of
    5 hold nothing.  m = k H + 1 leaves a last bin of one row."""
    k, d, empty = ROW_EDGE_CASES[case]
    S, W, H = 3, 64, 64
    m = k * H + d
    rows, cols = [], []
    for b in range(cdiv(m, H)):
        if b in empty:
            continue
        for lr in (0, 1, H - 2, H - 1):
            r = b * H + lr
            if r < m:
                for s in range(S):
                    rows += [r, r]
                    cols += [s * W + (lr + b) % W, s * W + (3 * lr + 7) % W]
    rungs = {r for r in set(rows)}
    return Family("row_edges_" + case, vt, m, S * W, rows, cols, _hooks(W, H), rungs, empty=empty, H=H)


def dup_placements(vt):
    """name -> entries ahead of the duplicated row in its run (= its first position in the bin's stream)."""
    b, grp = blk(vt), constants()["PB_GRP"]
    return {"quad0": 0, "quad1": 1, "quad2": 2, "quad3": 3, "block_edge": b - 1, "group_edge": grp - 1}


def dups(vt):
    """One bin per (c, placement): `o` rows of one entry each, then ONE row of c entries, all in the tile of slice 0 -- sorted by
    row the duplicated row starts on position o of the bin's stream.  `next_slice`: the row has c entries in slice 0 and c in
    slice 1; `two_rows`: rows 0 and 1 hold c entries each."""
    S, W, H = 2, 64, 300
    rows, cols, spec = [], [], []
    for c in DUP_COUNTS:
        for name, o in list(dup_placements(vt).items()) + [("next_slice", 0), ("two_rows", 0)]:
            b = len(spec)
            spec.append((c, name, o))
            k = np.arange(c, dtype=np.int64)
            rows.append(b * H + np.arange(o, dtype=np.int64))
            cols.append((np.arange(o, dtype=np.int64) * 3 + b) % W)
            rows.append(np.full(c, b * H + o))
            cols.append((k * 5 + 1) % W)
            if name == "next_slice":
                rows.append(np.full(c, b * H + o))
                cols.append(W + (k * 3) % W)
            if name == "two_rows":
                rows.append(np.full(c, b * H + o + 1))
                cols.append((k * 7 + 2) % W)
    m = len(spec) * H
    return Family("dups", vt, m, S * W, np.concatenate(rows), np.concatenate(cols), _hooks(W, H),
                  {(c, name) for c, name, _ in spec}, spec=spec, H=H)


def row_codes(vt, overflow=False):
    """H asked 4 000 (the plan takes it where a bin may hold that many rows, else its own maximum: the family is built for
    the height tiling() restates).  16 slices; a tile is ONE block: a first entry on local row 0 and J entries each 255 rows
    beyond the one before -- J exceptions.  Bins: the row advances of ROW_ADVANCES inside one block; a block base on row
    H - 1; exactly 0, 1, PB_EXC_CAP - 1 and PB_EXC_CAP exceptions; overflow=True adds a bin with PB_EXC_CAP + 1."""
    S, W, h_ask = 16, 64, 4000
    cap, b = constants()["PB_EXC_CAP"], blk(vt)
    H = h_ask if h_ask < tiling(vt, 2, S * W, 0).max_rows else tiling(vt, 2, S * W, 0).max_rows
    jmax = min(b - 1, (H - 1) // 255)
    assert S * jmax > cap
    wanted = [0, 1, cap - 1, cap] + ([cap + 1] if overflow else [])
    rows, cols, spec = [], [], []
    adv = np.cumsum((0,) + ROW_ADVANCES)
    assert adv[-1] < H and adv.size <= b
    rows.append(adv)                                       # bin 0: the advances, one block of slice 0
    cols.append(np.arange(adv.size) % W)
    spec.append("advances")
    rows.append(np.array([H + H - 1, H + H - 1, H + 5, H + 5 + 254]))     # bin 1: slice 1 holds one block whose base is row H - 1
    cols.append(np.array([W + 1, W + 2, 3, 4]))
    spec.append("base_on_last_row")
    for e in wanted:
        bn, left = len(spec), e
        spec.append(e)
        for s in range(S):
            j = min(jmax, left)
            left -= j
            rows.append(bn * H + np.concatenate([[0], 255 * np.arange(1, j + 1)]))
            cols.append(s * W + np.arange(j + 1) % W)
    m = len(spec) * H
    return Family("row_codes" + ("_overflow" if overflow else ""), vt, m, S * W, np.concatenate(rows), np.concatenate(cols),
                  _hooks(W, h_ask), set(wanted), spec=spec, H=H)


def many_slices(vt):
    """2 500 slices of 4 columns: more than the staged scatter takes (PB_STAGE_MAX_S), so the plan scatters directly without
    being told to.  3 bins of 100 rows (the last one row short), 8 entries per row spread over the slices."""
    W, H, S = 4, 100, constants()["PB_STAGE_MAX_S"] + 452
    n, m = S * W, 3 * H - 1
    rows = np.repeat(np.arange(m, dtype=np.int64), 8)
    cols = (rows * 37 + np.tile(np.arange(8), m) * (n // 8 + 1)) % n
    cols[:2], cols[-2:] = (0, n - 1), (n - 1, 0)
    return Family("many_slices", vt, m, n, rows, cols, _hooks(W, H), {S}, S=S)


def skew_cols(vt):
    """One slice of 8 with more than 3 x the mean: the expand takes its work list, the heavy slice cut into parts."""
    S, W, H, NB = 8, 64, 100, 6
    rows, cols = [], []
    for b in range(NB):
        for s in range(S):
            r, c = _tile(b, s, 3000 + b if s == 3 else 37 + s + b, H, W, row_step=3, row0=s)
            rows.append(r)
            cols.append(c)
    return Family("skew_cols", vt, NB * H, S * W, np.concatenate(rows), np.concatenate(cols), _hooks(W, H), {"expand_parts"})


def skew_rows(vt):
    """One group of 4 bins among 5 with more than 3 x the mean and more than 1.5 x 16 384 entries: the reduce takes its work
    list, the heavy group's streams cut in two parts whose partial rows pb_combine_items_kernel adds."""
    S, W, H, NB = 4, 64, 200, 20
    rows, cols = [], []
    for b in range(NB):
        for s in range(S):
            r, c = _tile(b, s, 2500 + 3 * s + b if 4 <= b < 8 else 20 + s, H, W, row_step=3, row0=s)
            rows.append(r)
            cols.append(c)
    return Family("skew_rows", vt, NB * H, S * W, np.concatenate(rows), np.concatenate(cols), _hooks(W, H), {"reduce_parts"})


def many_groups(vt, cus):
    """Variable bins in more groups than 2 x the CU count (4 rows per bin, 2 entries per row), one stretch of 16 rows of 9 000
    entries in the middle (each a bin of its own: the entry count crosses a multiple of 8 192 inside every one): the reduce's work list is longer than 2 x the CUs -- sorted heaviest first, or, PB_LPT=0, left in
    group order --, its heavy groups are cut into parts, and the scatter takes the bins in heaviest-first order too."""
    S, W, H = 4, 64, 4
    ngroups = 2 * cus + 40
    m = ngroups * 4 * H
    lens = np.full(m, 2, np.int64)
    lens[m // 2:m // 2 + 16] = 9000
    lens[[0, m - 1]] = 0
    env = dict(_hooks(W, H), SPBLAS_GFX950_PB_SPLIT_LEN=0)
    return _plain_family("many_groups", vt, lens, S * W, env, {"sorted_reduce_list", "bin_order"}, step=37, cus=cus)


BIN_SPANS = (65535, 65536, 65537)


def bin_span_family(vt, span):
    """Two bins of 1 000 rows; the rows of the first span exactly `span` entries of the caller's arrays (positions are staged
    as 16-bit words below 65 536), the second holds a few hundred."""
    S, W, H = 4, 64, 1000
    lens = np.full(2 * H, 0, np.int64)
    lens[:H] = span // H
    lens[:span % H] += 1
    lens[H:] = np.arange(H) % 2
    rows = np.repeat(np.arange(2 * H, dtype=np.int64), lens)
    k = np.arange(rows.size, dtype=np.int64)
    return Family(f"bin_span_{span}", vt, 2 * H, S * W, rows, (k * 37 + rows) % (S * W), _hooks(W, H), {span}, span=span)


def hub_rows(vt):
    """Arithmetic bins: rows of window - 1, window, window + 1 (twice) entries among rows of 3 -- the rows longer than the
    row-block window stay out of the tiles (hub_rows = 2) and pb_hub_rows_kernel adds them."""
    S, W, H = 8, 512, 64
    win = L.thresholds()["window_" + vt]
    m, n = 3 * H, S * W
    lens = np.full(m, 3, np.int64)
    lens[[5, 70, 130, 131]] = (win - 1, win, win + 1, win + 1)
    lens[[0, 63, 64, 191]] = 0
    rows = np.repeat(np.arange(m, dtype=np.int64), lens)
    k = np.arange(rows.size, dtype=np.int64)
    return Family("hub_rows", vt, m, n, rows, (k * 613 + 7 * rows) % n, _hooks(W, H), {win - 1, win, win + 1}, win=win)


def _plain_family(name, vt, lens, n, env, rungs, step=613, **meta):
    lens = np.asarray(lens, np.int64)
    rows = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    k = np.arange(rows.size, dtype=np.int64)
    f = Family(name, vt, lens.size, n, rows, (k * step + 7 * rows) % n, env, rungs, **meta)
    del f.env["SPBLAS_GFX950_PB_VARBINS"]             # these families are about the row map and the variable bins
    return f


HUB_LEN_ASKED = 3000
SPLIT_LEN_ASKED = 40


def hub_len(vt):
    """Variable bins (the longest row is long against the mean), no pieces (PB_SPLIT_LEN=0): rows of PB_HUB_LEN - 1, PB_HUB_LEN
    and PB_HUB_LEN + 1 entries -- only the last stays out of the tiles."""
    S, W, H = 8, 512, 64
    lens = np.full(3 * H, 3, np.int64)
    lens[[9, 80, 150]] = (HUB_LEN_ASKED - 1, HUB_LEN_ASKED, HUB_LEN_ASKED + 1)
    lens[[0, 64, 191]] = 0
    env = dict(_hooks(W, H), SPBLAS_GFX950_PB_SPLIT_LEN=0, SPBLAS_GFX950_PB_HUB_LEN=HUB_LEN_ASKED)
    return _plain_family("hub_len", vt, lens, S * W, env, {HUB_LEN_ASKED - 1, HUB_LEN_ASKED, HUB_LEN_ASKED + 1})


def split_rows(vt):
    """PB_SPLIT_LEN = 40: rows of 2, 3 and 9 x 40 - 1 and + 1 entries become pieces (the last one of 39 entries or of 1); bins of
    8 compact rows, so the pieces of a row fall into different bins.  Rows of 40 and fewer entries stay whole."""
    S, W, H, Lp = 4, 64, 8, SPLIT_LEN_ASKED
    lens = np.full(100, 2, np.int64)
    at = (3, 14, 30, 45, 60, 83)
    lens[list(at)] = [k * Lp + d for k in (2, 3, 9) for d in (-1, 1)]
    lens[[50, 51]] = (Lp, Lp - 1)
    lens[[0, 99]] = 0
    env = dict(_hooks(W, H), SPBLAS_GFX950_PB_SPLIT_LEN=Lp)
    return _plain_family("split_rows", vt, lens, S * W, env, {k * Lp + d for k in (2, 3, 9) for d in (-1, 1)}, step=37, at=at)


def compact_rows(vt):
    """PB_COMPACT=1: the empty rows are taken out of the tiles -- leading, trailing, in stretches, alone between full rows --
    and must come back as 0 (beta = 0) from pb_empty_rows_kernel."""
    S, W, H = 4, 64, 16
    lens = np.full(200, 5, np.int64)
    lens[:7] = 0
    lens[190:] = 0
    lens[40:75] = 0
    lens[100:130:2] = 0
    lens[[150, 152, 177]] = 0
    env = dict(_hooks(W, H), SPBLAS_GFX950_PB_COMPACT=1)
    return _plain_family("compact_rows", vt, lens, S * W, env, {"leading", "trailing", "stretch", "alone"}, step=37)


def slice_aligned(vt, cus):
    """fp64 at the natural width: a slice count between 0.9 x and 1 x the CU count is rounded up to the CU count and, the
    slices being even, the expand takes one work item per slice.  Few entries: 6 per slice, on its first and last columns."""
    assert vt == "f64"
    n = (cus - cus // 20) * tiling(vt, 2, 1, 0).max_cols
    t = tiling(vt, 2, n, 0, {}, cus)
    assert t.slice_aligned and t.S == cus
    H = 50
    m = 3 * H - 1
    s = np.arange(t.S, dtype=np.int64)
    last = np.minimum((s + 1) * t.W, n) - 1
    cols = np.stack([s * t.W, s * t.W + 1, last, s * t.W + 2, last - 1, s * t.W]).T.reshape(-1)
    rows = (np.arange(cols.size, dtype=np.int64) * 7) % m
    rows[:3] = (0, H - 1, m - 1)
    return Family("slice_aligned", vt, m, n, rows, cols, {"SPBLAS_GFX950_SLICE_ROWS": H}, {t.S}, S=t.S, W=t.W)


# ------------------------------------------------------------------------------------------------------------ hot split
HOT_COLS = (0, 77, 511, 512, 4095, 4096, 6000, 8191)


def hot_sample_positions(nnz):
    """The entries hot_sample_kernel reads: one line of 32 consecutive entries out of every 16, its place hashed per group."""
    t = np.arange(cdiv(cdiv(nnz, 16), 256) * 256, dtype=np.int64)
    g = t >> 5
    hsh = (g.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    p = (g * 16 + (hsh >> np.uint64(28)).astype(np.int64)) * 32 + (t & 31)
    return p[p < nnz]


def hot_columns(colind, n, min_pct=15):
    """The columns the split takes (spmv_hot.hip: sampled at least twice, as long as they fit LDS -- the families stay far
    below that --, and only if they carry min_pct of the sample and of the matrix); empty: no split."""
    src = L._src("spmv_hot.hip")
    assert re.search(r"const int64_t p = \(g \* 16 \+ \(hsh >> 28\)\) \* 32 \+ \(t & 31\);", src) and \
        re.search(r"for \(int c = HOT_HIST - 1; c >= 2; --c\)", src) and re.search(r"flag\[c\] = cnt\[c\] >= thr;", src) and \
        _one(r'hot_env\("SPBLAS_GFX950_PB_HOT_MIN_PCT", (\d+)\)', src, "the share a split must carry") == min_pct, \
        "the hot-column rule: the source no longer has the expected form; update tests/ladder_sliced.py"
    colind = np.asarray(colind, np.int64)
    cnt = np.bincount(colind[hot_sample_positions(colind.size)], minlength=n)
    hot = np.flatnonzero(cnt >= 2)
    assert hot.size < 16000
    n_hot = int(np.isin(colind, hot).sum())
    if hot.size == 0 or cnt[hot].sum() * 100 < cnt.sum() * min_pct or n_hot * 100 < colind.size * min_pct or n_hot == colind.size:
        return np.zeros(0, np.int64)
    return hot


def hot_split(vt):
    """PB_HOT=1: eight columns on slice edges referenced by most entries (each sampled more than once), every other column
    referenced at most once (never sampled twice).  Rows with HOT_WIN - 1, HOT_WIN, HOT_WIN + 1, 2 HOT_WIN - 1 and
    2 HOT_WIN + 1 hot entries come first -- the windows of A_hot cut through them --, then a hot-only and a cold-only row,
    empty rows, 190 rows without a hot entry, and a last row with some.  meta: hot_per_row, the CSR arrays of A_rest."""
    S, W, H = 16, 512, 64
    win = constants()["HOT_WIN"]
    m, n = 4 * H, S * W
    hot_n = np.zeros(m, np.int64)
    cold_n = np.zeros(m, np.int64)
    hot_n[:5] = (win - 1, win, win + 1, 2 * win - 1, 2 * win + 1)
    cold_n[:5] = (2, 0, 1, 0, 3)
    hot_n[5], cold_n[6] = 7, 9
    hot_n[10], cold_n[10] = 3, 3
    cold_n[11:201] = np.arange(190) % 3
    hot_n[201], hot_n[m - 1], cold_n[m - 1] = 5, 4, 1
    cold_cols = np.setdiff1d(np.arange(n), HOT_COLS)
    cold_cols = cold_cols[(np.arange(cold_n.sum()) * 31) % cold_cols.size]       # 31 and the count are coprime: all distinct
    assert np.unique(cold_cols).size == cold_cols.size
    rows, cols, is_hot = [], [], []
    taken = 0
    for r in range(m):
        h, c = int(hot_n[r]), int(cold_n[r])
        cc = np.concatenate([np.asarray(HOT_COLS)[(np.arange(h) + r) % len(HOT_COLS)], cold_cols[taken:taken + c]])
        hh = np.concatenate([np.ones(h, bool), np.zeros(c, bool)])
        mix = np.argsort((np.arange(h + c) * 7) % max(h + c, 1), kind="stable")     # hot and cold entries interleaved
        rows.append(np.full(h + c, r))
        cols.append(cc[mix])
        is_hot.append(hh[mix])
        taken += c
    rows, cols, is_hot = np.concatenate(rows), np.concatenate(cols), np.concatenate(is_hot)
    f = Family("hot_split", vt, m, n, rows, cols, dict(_hooks(W, H), SPBLAS_GFX950_PB_HOT=1), {"hot"},
               hot_per_row=hot_n, cold_per_row=cold_n)
    rest_rowptr = np.concatenate([[0], np.cumsum(cold_n)]).astype(np.int64)
    f.meta["rest"] = (rest_rowptr, f.colind[~np.isin(f.colind, HOT_COLS)])
    return f


def all_families(vt):
    """Every family that does not depend on the CU count (slice_aligned, many_groups), but `groups`, which runs through plans
    of its own."""
    f = [runs(vt), dups(vt), row_codes(vt), row_codes(vt, overflow=True), many_slices(vt), hub_rows(vt), hub_len(vt),
         split_rows(vt), compact_rows(vt), skew_cols(vt), skew_rows(vt), hot_split(vt)]
    f += [bin_span_family(vt, s) for s in BIN_SPANS]
    f += [col_edges(vt, c) for c in COL_EDGE_CASES]
    f += [row_edges(vt, c) for c in ROW_EDGE_CASES]
    return f


# ----------------------------------------------------------------------------------------------- host model of the pair
MISTAKES = ("last_block_dropped", "batch_tail_one_group_short", "batch_tail_one_group_more", "duplicate_without_flag",
            "exception_dropped", "exception_by_every_part", "first_column_off_by_one", "last_column_off_by_one",
            "pad_on_last_row", "part_boundary_off_by_one")
PAD_PRODUCT = 1.0      # what a pad's slot of the product stream holds in the model: the stream is not cleared


def model_spmv(fam_or_arrays, values, x, t, ub=4, K=1, enc8=False, mistake=None):
    """y of a host model of expand -> reduce over the restated tiling, in float64.  expand: product of every entry into its slot
    of the product stream (runs padded to blocks, bins to groups; pads carry row H and a non-zero product).  reduce: per bin and
    part, groups in two batches of `ub`; inside a group every unflagged entry does read-add-write (all reads first), flagged
    ones -- a row met before in the group -- add atomically; with one-byte codes the exceptions stay out of the main pass and
    part 0 adds them.  `mistake` seeds one of MISTAKES."""
    rowptr, colind = fam_or_arrays
    assert mistake is None or mistake in MISTAKES
    bl, grp = blk(t.vt), constants()["PB_GRP"]
    b, s, r, order = _tile_entries(rowptr, colind, t)
    cols = np.asarray(colind, np.int64)
    xc = cols.copy()
    if mistake == "first_column_off_by_one":
        first = cols == s * t.W
        xc[first] = np.maximum(cols[first] - 1, 0)
    if mistake == "last_column_off_by_one":
        last = cols == np.minimum((s + 1) * t.W, t.n) - 1
        xc[last] = np.maximum(cols[last] - 1, 0)
    prod = values * x[xc]
    y = np.zeros(t.m)
    pad_row = t.H - 1 if mistake == "pad_on_last_row" else t.H
    key = (b * t.S + s)[order]
    bounds = np.searchsorted(key, np.arange(t.NB * t.S + 1))
    for bn in range(t.NB):
        P, R, X = [], [], []                            # the bin's stream: products, rows, exception marks
        for sl in range(t.S):
            lo, hi = bounds[bn * t.S + sl], bounds[bn * t.S + sl + 1]
            if hi == lo:
                continue
            e = order[lo:hi]
            p, rr = prod[e].copy(), r[e].copy()
            pad = cdiv(p.size, bl) * bl - p.size
            p, rr = np.concatenate([p, np.full(pad, PAD_PRODUCT)]), np.concatenate([rr, np.full(pad, pad_row)])
            if mistake == "last_block_dropped":
                p[-bl:] = 0.0
            ex = np.zeros(p.size, bool)
            if enc8:
                for k0 in range(0, hi - lo, bl):
                    d = rr[k0]
                    for j in range(k0 + 1, min(k0 + bl, hi - lo)):
                        if rr[j] - d >= 255:
                            ex[j] = True
                            d += 255
                        else:
                            d = rr[j]
            P.append(p), R.append(rr), X.append(ex)
        if not P:
            continue
        P, R, X = np.concatenate(P), np.concatenate(R), np.concatenate(X)
        pad = cdiv(P.size, grp) * grp - P.size
        P, R, X = np.concatenate([P, np.full(pad, PAD_PRODUCT)]), np.concatenate([R, np.full(pad, pad_row)]), \
            np.concatenate([X, np.zeros(pad, bool)])
        ng = P.size // grp
        r1 = min(t.H, t.m - bn * t.H)
        for k in range(K):
            acc = np.zeros(t.H + 1)
            g_lo, g_hi = ng * k // K, ng * (k + 1) // K
            if mistake == "part_boundary_off_by_one" and k > 0:
                g_lo += 1
            for g0 in range(g_lo, g_hi, ub):
                last = g0 + ub >= g_hi
                stop = g_hi + (-1 if mistake == "batch_tail_one_group_short" and last else
                               1 if mistake == "batch_tail_one_group_more" and last else 0)
                for g in range(g0, g0 + ub):
                    if g >= stop:
                        break
                    gg = min(g, g_hi - 1)                  # loads past the end are clamped to the last group
                    p, rr, ex = P[gg * grp:(gg + 1) * grp], R[gg * grp:(gg + 1) * grp], X[gg * grp:(gg + 1) * grp]
                    live = ~ex
                    first_of_row = np.zeros(grp, bool)
                    first_of_row[np.unique(np.where(live, rr, -1), return_index=True)[1]] = True
                    plain = live & first_of_row
                    flagged = live & ~first_of_row
                    if mistake == "duplicate_without_flag" and (flagged & (rr < t.H)).any():
                        j = np.flatnonzero(flagged & (rr < t.H))[0]     # the later plain store wins: the earlier addend is lost
                        earlier = np.flatnonzero(plain & (rr == rr[j]))[0]
                        plain[earlier], plain[j], flagged[j] = False, True, False
                    acc[rr[plain]] += p[plain]
                    np.add.at(acc, rr[flagged], p[flagged])
            if enc8 and (k == 0 or mistake == "exception_by_every_part") and mistake != "exception_dropped":
                np.add.at(acc, R[X], P[X])
            y[bn * t.H:bn * t.H + r1] += acc[:r1]
    return y
