"""Block ladder of the fp32 panel / band path of csrc/spmm.hip: the matrices, the probe restated, a host model.

constants()   MM_RB, MM_KT, MM_MAXT, MM_NP, EB, the admission divisor, the default and the clamp of BAND_CH, the LDS of a
              workgroup and the matrix-core kernel's row cap, parsed from spmm.hip: a changed constant moves the rungs or fails.
knobs(env)    what spmm_inspect_typed reads from the environment at every inspect, restated.
probe(...)    spmm_panel_probe_kernel restated: per block of 32 rows the kind (0 row-group kernel, 1 entry loop / tile kernel,
              2 matrix cores), the tile count (17 on overflow, 0 after the cheap reject), the ascending tile ids, (cmin, cmax).
blk / Family  a block is its per-row entry counts, the column set they come from and where repeated (row, column) pairs go;
              Family strings blocks (and filler blocks that do not qualify) into CSR arrays with int32 or int64 offsets.
families      one small matrix each, nearly all blocks empty or filler; every block that makes a claim (its kind, tile count,
              window width, branch of the band kernel) carries it, tests/test_ladders_mm_cpu.py holds the claims against probe().
reference()   fp64: repeated pairs summed, only stored entries multiplied, alpha * sum + beta * C.
host_model()  the three kernels' arithmetic ORDER does not matter for the integer data sets, their STRUCTURE does: which entries
              a branch can see.  The model follows that structure (staged rows of the single-chunk branch, tile groups of the wide
              branch, the tagged dense tile of the matrix-core kernel) and takes three mutations the ladder must catch.
"""
import re
from functools import lru_cache

import numpy as np
import scipy.sparse as sps

import ladder as L

E = "SPBLAS_GFX950_SPMM_"
NS = (1, 3, 4, 128, 130, 257)
NMAX = max(NS)
ALPHA_BETA = ((1.0, 0.0), (-2.0, 0.5), (1.0, 1.0))
SELECTIONS = {"band_8_waves": {}, "band_4_waves": {E + "BAND_WAVES": "4"}, "band_16_waves": {E + "BAND_WAVES": "16"},
              "band_mfma": {E + "BAND_DENSE": "0"}, "tiles": {E + "BAND": "0"}}
ROW_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200)
PAIR_DISTANCES = (1, 63, 64, 65, 87, 128)


# --------------------------------------------------------------------------------------------------------------- constants
@lru_cache(maxsize=None)
def constants():
    s = L._src("spmm.hip")
    c = {}
    for name in ("MM_RB", "MM_KT", "MM_MAXT", "MM_NP", "MM_DENSE_CH"):
        c[name], = L._two(r"static constexpr int %s = (\d+);" % name, s, name)
    c["EB"], = L._two(r"constexpr int EB = (\d+);", s, "EB")
    c["ADMIT_DIV"], = L._two(r"int min_per_tile = MM_RB \* MM_KT / (\d+);", s, "default admission")
    c["CH_DEFAULT"], c["CH_MIN"], c["CH_MAX"] = L._two(
        r"int ch = c \? std::atoi\(c\) : (\d+);\s*pl->mm_band_ch = ch < (\d+) \? \2 : \(ch > (\d+) \? \3 : ch\);", s, "BAND_CH")
    c["LDS_BYTES"] = 1024 * L._two(r"static constexpr int MM_LDS_BYTES = (\d+) \* 1024;", s, "MM_LDS_BYTES")[0]
    assert re.search(r"std::min\(pl->mm_band_ch, MM_LDS_BYTES / 512 - pl->mm_band_waves\)", s), "the LDS cap of BAND_CH moved"
    assert re.search(r"const int G = CH / MM_KT < 4 \? CH / MM_KT : 4;", s), "the wide branch's group size moved"
    assert re.search(r"const bool single = w\.y - w\.x < CH;", s), "the branch switch of spmm_band_kernel moved"
    c["MIN_DEFAULT"] = c["MM_RB"] * c["MM_KT"] // c["ADMIT_DIV"]
    c["WINDOW"] = L.thresholds()["window_f32"]
    return c


def _atoi(v):
    m = re.match(r"\s*[+-]?\d+", v or "")
    return int(m.group()) if m else 0


def knobs(env):
    """{min_per_tile, band, band_ch, band_waves, dense_pm} as spmm_inspect_typed derives them from the environment."""
    c = constants()
    mpt = _atoi(env.get(E + "PANEL_MIN"))
    band = not (E + "BAND" in env and _atoi(env[E + "BAND"]) == 0)
    ch = _atoi(env[E + "BAND_CH"]) if E + "BAND_CH" in env else c["CH_DEFAULT"]
    waves = {4: 4, 16: 16}.get(_atoi(env.get(E + "BAND_WAVES")), 8)
    ch = min(max(ch, c["CH_MIN"]), c["CH_MAX"], c["LDS_BYTES"] // 512 - waves)
    pm = 1001 if not band or E + "BAND_DENSE" not in env else _atoi(env[E + "BAND_DENSE"])
    return {"min_per_tile": mpt if mpt > 0 else c["MIN_DEFAULT"], "band": int(band), "band_ch": ch, "band_waves": waves,
            "dense_pm": pm}


def group_size(ch):
    return min(ch // constants()["MM_KT"], 4)


# ------------------------------------------------------------------------------------------------------------------- probe
def long_len_of(rowptr):
    """What the probe is given as long_len: the plan's window when some row is longer than it, else 0."""
    win = constants()["WINDOW"]
    return win if (np.diff(rowptr) > win).any() else 0


def probe(rowptr, colind, m, long_len, min_per_tile, band_ch, dense_pm, mutation=None):
    """spmm_panel_probe_kernel: (kind[nblk], nt[nblk], tiles (list of ascending id arrays), win[nblk, 2], panel_nnz)."""
    c = constants()
    RB, KT, MAXT = c["MM_RB"], c["MM_KT"], c["MM_MAXT"]
    nblk = -(-m // RB)
    kind, nt = np.zeros(nblk, np.uint8), np.zeros(nblk, np.int32)
    tiles, win, panel_nnz = [np.zeros(0, np.int32)] * nblk, np.zeros((nblk, 2), np.int32), 0
    lens = np.diff(rowptr)
    dense_ch = min(band_ch, c["MM_DENSE_CH"])
    for b in range(nblk):
        r0, r1 = b * RB, min(b * RB + RB, m)
        p0, p1 = int(rowptr[r0]), int(rowptr[r1])
        cnt = p1 - p0
        if (long_len > 0 and (lens[r0:r1] > long_len).any()) or cnt < min_per_tile:
            continue                                  # has_long / the cheap reject: no scan, count 0
        cols = colind[p0:p1].astype(np.int64)
        ids = np.unique(cols // KT)
        if len(ids) > MAXT:
            nt[b] = MAXT + 1
            continue
        nt[b], tiles[b] = len(ids), ids.astype(np.int32)
        cmin, cmax = int(cols.min()), int(cols.max())
        win[b] = cmin, cmax
        if cnt < min_per_tile * len(ids):
            continue
        W = cmax - cmin + 1
        fits = (W if mutation == "w_not_wp" else (W + 3) & ~3) <= dense_ch
        dense = fits and cnt * 1000 >= dense_pm * RB * W
        kind[b] = 2 if dense else 1
        panel_nnz += cnt
    return kind, nt, tiles, win, panel_nnz


def probe_family(f, env, mutation=None):
    kn = knobs(env)
    return probe(f.rowptr, f.colind, f.m, long_len_of(f.rowptr), kn["min_per_tile"], kn["band_ch"], kn["dense_pm"], mutation)


# ----------------------------------------------------------------------------------------------------------------- builder
class Blk:
    def __init__(self, lens, cols, dups=(), puts=(), **claim):
        self.lens, self.cols, self.dups, self.puts, self.claim = list(lens), cols, list(dups), list(puts), claim


def order_cols(cols):
    """The column set with its anchors first -- smallest, largest, first and last column of every tile -- so that a block of
    a few dozen entries already has the window and the tiles its specification names."""
    cols = np.unique(np.asarray(cols, dtype=np.int64))
    KT = constants()["MM_KT"]
    anchors = [cols[0], cols[-1]]
    for t in np.unique(cols // KT):
        tc = cols[cols // KT == t]
        anchors += [tc[0], tc[-1]]
    seen, first = set(), []
    for a in anchors:
        if int(a) not in seen:
            seen.add(int(a))
            first.append(int(a))
    return np.array(first + [int(x) for x in cols if int(x) not in seen], dtype=np.int64)


def blk(lens, cols, dups=(), puts=(), **claim):
    """lens: entries of each row (at most 32 rows; fewer only in the last block).  cols: the column set; entry e of the block
    (counted through its rows) takes order_cols(cols)[e % len], so a row no longer than the set has distinct columns and a
    longer one repeats.  dups: (row, i, j) gives entry j of the row the column of its entry i; puts: (row, j, column) puts entry j of
    the row on a column outside the set."""
    return Blk(lens, order_cols(cols), dups, puts, **claim)


def span(c0, W):
    return np.arange(c0, c0 + W)


def tile_cols(ids, k):
    KT = constants()["MM_KT"]
    return np.concatenate([np.arange(t * KT, min(t * KT + KT, k)) for t in ids])


def spread(total, rows=32, cap=None):
    """`total` entries over `rows` rows as evenly as possible."""
    base, rem = divmod(total, rows)
    lens = [base + (1 if r < rem else 0) for r in range(rows)]
    assert cap is None or max(lens) <= cap
    return lens


def filler(i, k):
    """A block that does not qualify: empty, 32 single entries (the cheap reject), or 200 entries over 16 tiles (too thin)."""
    KT = constants()["MM_KT"]
    nkt = k // KT
    if i % 3 == 0:
        return Blk([0] * 32, np.zeros(1, np.int64), kind=0, nt=0)
    if i % 3 == 1:
        return Blk([1] * 32, (np.arange(32) * 37 + 11 * i) % k, kind=0, nt=0)
    ids = [(5 * i + 3 * q) % nkt for q in range(16)] if nkt >= 48 else list(range(min(16, nkt)))
    return blk(spread(200), tile_cols(sorted(set(ids)), k), kind=0)


class Family:
    def __init__(self, name, env, k, blocks):
        self.name, self.env, self.k, self.blocks = name, dict(env), k, blocks
        rp, ci = [0], []
        for i, b in enumerate(blocks):
            assert len(b.lens) == 32 or (i == len(blocks) - 1 and 0 < len(b.lens) < 32), "only the last block is partial"
            e = 0
            for r, n_ in enumerate(b.lens):
                row = b.cols[(e + np.arange(n_)) % len(b.cols)]
                for (dr, di, dj) in b.dups:
                    if dr == r:
                        row[dj] = row[di]
                for (pr, pj, pc) in b.puts:
                    if pr == r:
                        row[pj] = pc
                ci.append(row)
                rp.append(rp[-1] + n_)
                e += n_
        self.rowptr = np.array(rp, dtype=np.int64)
        self.colind = np.concatenate(ci).astype(np.int32) if ci else np.zeros(0, np.int32)
        self.m, self.nnz = len(rp) - 1, int(rp[-1])
        self.shape = (self.m, k)
        self.claims = {i: b.claim for i, b in enumerate(blocks) if b.claim}
        assert self.nnz >= 256, f"{name}: the probe only runs from 256 entries"
        assert self.colind.size == 0 or (0 <= self.colind.min() and self.colind.max() < k), name

    def arrays(self, offsets=np.int32):
        return self.rowptr.astype(offsets), self.colind


def with_filler(blocks, k, every=1):
    out = []
    for i, b in enumerate(blocks):
        out.append(b)
        if i % every == every - 1:
            out.append(filler(i, k))
    return out


MIN64 = {E + "PANEL_MIN": "64"}
K0 = 64 * 120      # columns of most families: 120 tiles


# ---------------------------------------------------------------------------------------------------------------- families
@lru_cache(maxsize=None)
def fam_admission(mpt):
    """nt = 1 ... 16 tiles with mpt * nt - 1 / exact / + 1 entries; 17 tiles; fewer than mpt entries in the block."""
    env = {} if mpt == constants()["MIN_DEFAULT"] else {E + "PANEL_MIN": str(mpt)}
    blocks = []
    for nt in range(1, 17):
        for d in (-1, 0, 1):
            ids = [(7 * nt + 3 * q) % 120 for q in range(nt)]          # scattered, non-adjacent
            blocks.append(blk(spread(mpt * nt + d, cap=64 * nt), tile_cols(ids, K0), kind=0 if d < 0 else 1, nt=0 if (nt, d) == (1, -1) else nt))
    blocks.append(blk(spread(17 * mpt + 10), tile_cols([5 * q for q in range(17)], K0), kind=0, nt=17))
    blocks.append(blk(spread(mpt - 1), tile_cols([9], K0), kind=0, nt=0))
    return Family(f"admission_{mpt}", env, K0, with_filler(blocks, K0, every=4))


@lru_cache(maxsize=None)
def fam_long_row(other):
    """A block holding a row of exactly `window` entries (repeated columns) qualifies whether or not a longer row elsewhere
    sets n_long; a block holding a row of window + 1 entries never does."""
    win = constants()["WINDOW"]
    body = [4] * 31
    blocks = [blk([win] + body, tile_cols(range(20, 36), K0), kind=1, nt=16), filler(1, K0)]
    if other:
        blocks += [blk(body + [win + 1], tile_cols(range(40, 56), K0), kind=0, nt=0), filler(2, K0),
                   blk(spread(300), tile_cols([70, 71], K0), kind=1, nt=2),
                   blk([3] * 7 + [win + 200] + [3] * 24, tile_cols(range(80, 120), K0), kind=0, nt=0)]
    f = Family(f"long_row_{'with' if other else 'without'}_other", MIN64, K0, blocks)
    assert (long_len_of(f.rowptr) > 0) == other
    return f


def _window_block(c0, W, k, **claim):
    nt = (c0 + W - 1) // 64 - c0 // 64 + 1
    return blk([2 * nt + 1] * 32, span(c0, W), W=W, nt=nt, kind=1, **claim)


@lru_cache(maxsize=None)
def fam_window(ch, kmod):
    """W = ch - 1, ch, ch + 1 at kmin mod 4 = 0 ... 3, at column 0 and ending on column k - 1 (k mod 64 = kmod)."""
    k = 64 * 119 + (kmod if kmod else 64)
    blocks = []
    for W in (ch - 1, ch, ch + 1):
        br = "single" if W - 1 < ch else "wide"
        for a in range(4):
            blocks.append(_window_block(64 * (10 + 7 * a) + 20 + a, W, k, branch=br))
        blocks.append(_window_block(0, W, k, branch=br))
        blocks.append(_window_block(k - W, W, k, branch=br))
    return Family(f"window_ch{ch}_k{kmod}", dict(MIN64, **{E + "BAND_CH": str(ch)}), k, with_filler(blocks, k, every=3))


@lru_cache(maxsize=None)
def fam_wide(ch, kmod):
    """The wide branch: nt around the group size G = min(ch / 64, 4) and its multiples, scattered tiles, the first and the last
    tile of k (a wrap-around), a last tile cut by k; the anchors put entries on columns 64 t and 64 t + 63 of every tile."""
    G = group_size(ch)
    k = 64 * 119 + (kmod if kmod else 64)
    blocks = []
    for nt in sorted({n_ for n_ in (G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 16) if 2 <= n_ <= 16}):
        ids = [3 + 7 * q for q in range(nt)]
        blocks.append(blk([2 * nt + 1] * 32, tile_cols(ids, k), kind=1, nt=nt, branch="wide"))
        blocks.append(blk([2 * nt + 1] * 32, tile_cols([0] + ids[1:-1] + [119], k), kind=1, nt=nt, branch="wide"))
    blocks.append(blk([7] * 32, np.concatenate([span(0, 30), span(k - 30, 30)]), kind=1, branch="wide"))
    # entries on the last column of a tile and the first of the next one: 64 t - 1, 64 t, and 64 t + 63 far away
    blocks.append(blk([11] * 32, np.array([64 * 30 - 1, 64 * 30, 64 * 30 + 63, 64 * 50 - 1, 64 * 50, 64 * 50 + 63, 64 * 90]),
                      kind=1, nt=5, branch="wide"))
    return Family(f"wide_ch{ch}_k{kmod}", dict(MIN64, **{E + "BAND_CH": str(ch)}), k, with_filler(blocks, k, every=2))


COLMODES = {"w120": ({}, lambda: span(64 * 33 + 2, 120), "single"),             # one chunk at the default 128 rows
            "tiles4": ({}, lambda: tile_cols([12, 40, 41, 97], K0), "wide"),     # 256 columns in scattered tiles
            "w244": ({E + "BAND_CH": "312"}, lambda: span(64 * 60 + 1, 244), "single")}  # no natural repeats up to 244


@lru_cache(maxsize=None)
def fam_row_shapes(colmode):
    """Every row length on every row position 0 ... 31 (every wave and slot for 4, 8 and 16 waves); a wave whose rows are all
    empty; a block whose only non-empty row is the last."""
    env, cols, br = COLMODES[colmode]
    nl = len(ROW_LENGTHS)
    blocks = [blk([ROW_LENGTHS[(r + s) % nl] for r in range(32)], cols(), kind=1, branch=br) for s in range(nl)]
    blocks.append(blk([0 if 8 <= r < 16 else 12 for r in range(32)], cols(), kind=1, branch=br))
    blocks.append(blk([0] * 31 + [260], cols(), kind=1, branch=br))
    return Family(f"row_shapes_{colmode}", dict(MIN64, **env), K0, with_filler(blocks, K0, every=2))


@lru_cache(maxsize=None)
def fam_repeated(colmode):
    """Repeated (row, column) pairs 1, 63, 64, 65, 87 and 128 entries apart in every row / in one wave's rows only, a triple,
    a row that is one column throughout."""
    env, cols, br = COLMODES[colmode]
    blocks = []
    # (140 entries per row in a window of 120 columns: more entries than slots, which the per-mille rule calls dense whatever
    # its threshold -- these blocks reach the matrix-core kernel under the default knobs)
    kind = 2 if colmode == "w120" else 1
    for d in PAIR_DISTANCES:
        blocks.append(blk([140] * 32, cols(), [(r, 3 + r % 5, 3 + r % 5 + d) for r in range(32)], kind=kind, branch=br))
    for d in (1, 87):
        blocks.append(blk([140] * 32, cols(), [(r, 3, 3 + d) for r in range(4, 8)], kind=kind, branch=br))
    blocks.append(blk([140] * 32, cols(), [(r, 2, 66) for r in range(32)] + [(r, 2, 131) for r in range(32)], kind=kind, branch=br))
    blocks.append(blk([6] * 31 + [70], cols(), [(31, 0, j) for j in range(1, 70)], kind=1, branch=br))
    return Family(f"repeated_{colmode}", dict(MIN64, **env), K0, with_filler(blocks, K0, every=2))


def _dense_entries(c0, W):
    """Entries that admit a window of W columns from c0 at 64 per tile and make it dense at 250 per mille."""
    return max(8 * W + 1, 64 * ((c0 + W - 1) // 64 - c0 // 64 + 1) + 1)


@lru_cache(maxsize=None)
def fam_dense(ch, pm):
    """The matrix-core rule: entries * 1000 against pm * 32 * W at -1 / 0 / +1 entry; W = ch - 4 ... ch + 1 (Wp <= ch decides
    alone); Wp in {4, 28, 32, 36, 60, 64, 68, 128} with W = Wp and W = Wp - 1 (the padded tail)."""
    env = dict(MIN64, **{E + "BAND_CH": str(ch), E + "BAND_DENSE": str(pm)})
    blocks = []
    dch = min(ch, constants()["MM_DENSE_CH"])
    if pm > 0:
        W = 100 if ch >= 100 else 60
        edge = -(-pm * 32 * W // 1000)                       # the fewest entries that make the block dense
        for d in (-1, 0, 1):
            blocks.append(blk(spread(edge + d, cap=W), span(64 * 20 + 8, W), kind=2 if d >= 0 else 1, W=W))
    for W in range(dch - 4, dch + 2):
        fits = (W + 3) & ~3 <= dch
        blocks.append(blk(spread(_dense_entries(64 * 50 + 3, W), cap=W), span(64 * 50 + 3, W), kind=2 if fits else 1, W=W))
    for Wp in (4, 28, 32, 36, 60, 64, 68, 128):
        for W in (Wp, Wp - 1):
            if (W + 3) & ~3 <= dch:
                blocks.append(blk(spread(_dense_entries(64 * 70 + 1, W), cap=W), span(64 * 70 + 1, W), kind=2, W=W))
    # repeated pairs in the dense tile: 1 and 87 entries apart (rows of 96 in a window of 100: one natural repeat-free set)
    if dch >= 100:
        blocks.append(blk([96] * 32, span(64 * 90, 100), [(r, 3, 90) for r in range(0, 32, 7)], kind=2, W=100))
        blocks.append(blk([96] * 32, span(64 * 90, 100), [(r, 5, 6) for r in range(8, 12)], kind=2, W=100))
        blocks.append(blk([96] * 32, span(64 * 90, 100), [(r, 1, 66) for r in range(32)] + [(r, 1, 95) for r in range(32)],
                          kind=2, W=100))
    return Family(f"dense_ch{ch}_pm{pm}", env, K0, with_filler(blocks, K0, every=2))


@lru_cache(maxsize=None)
def fam_partial(mrem, only=False):
    """m mod 32 = mrem with the partial last block qualifying (m = 31: the only block)."""
    last = blk(spread(max(9 * mrem, 140), rows=mrem), tile_cols([17, 18], K0), kind=1, nt=2)
    blocks = [last] if only else [blk([9] * 32, span(300, 90), kind=1), filler(1, K0), filler(2, K0), last]
    return Family(f"partial_{mrem}{'_only' if only else ''}", MIN64, K0, blocks)


def _q(i, dense=False):
    """A qualifying block of the list families; dense: also dense in its window at 250 per mille."""
    return blk([9] * 32, span(64 * (i % 100) + 5, 30 if dense else 100), kind=2 if dense else 1)


@lru_cache(maxsize=None)
def fam_lists(nq, mix=False):
    """nq qualifying blocks alternating with filler (the row-group kernel must skip exactly those); mix: dense and entry-loop
    blocks interleaved (BAND_DENSE=250)."""
    env = dict(MIN64, **({E + "BAND_DENSE": "250"} if mix else {}))
    blocks = with_filler([_q(i, dense=mix and i % 2 == 0) for i in range(nq)], K0)
    return Family(f"lists_{nq}{'_mixed' if mix else ''}", env, K0, blocks)


@lru_cache(maxsize=None)
def fam_all_panel(but_one):
    blocks = [_q(i) for i in range(11)]
    if but_one:
        blocks[6] = filler(1, K0)
    return Family(f"all_panel{'_but_one' if but_one else ''}", MIN64, K0, blocks)


@lru_cache(maxsize=None)
def fam_nblk(nblk):
    """nblk blocks, a handful qualifying (the first, the last, one in 97, around each multiple of 256): the list kernels'
    workgroups and the scan's partials."""
    blocks = []
    for i in range(nblk):
        if i in (0, nblk - 1) or i % 97 == 0 or i % 256 in (0, 255):
            blocks.append(_q(i))
        else:
            blocks.append(Blk([0] * 32, np.zeros(1, np.int64)) if i % 5 else filler(1, K0))
    return Family(f"nblk_{nblk}", MIN64, K0, blocks)


INF_ROW, INF_COL = 64 * 40 + 101, 1     # the element of B that holds the infinity of fam_inf


@lru_cache(maxsize=None)
def fam_inf():
    """One row of B (INF_ROW) that ONE row of the matrix references.  Block 0 is a window of 101 columns that ends right below
    that row: for the matrix-core kernel it lies in the zero-padded tail W ... Wp of the staged window and must not be loaded.
    Block 2 holds the referencing row (row 5 of the block); its 31 other rows leave the column out."""
    c0 = 64 * 40
    a = blk([30] * 32, span(c0, 101), kind=1, W=101)
    cols = np.array([x for x in range(c0 + 60, c0 + 161) if x != INF_ROW])
    b = blk([30] * 32, cols, puts=[(5, 17, INF_ROW)], kind=1, W=101)
    return Family("inf", MIN64, K0, [a, filler(1, K0), b, filler(2, K0)])


GROUPS = {
    "admission": lambda ch: [fam_admission(constants()["MIN_DEFAULT"]), fam_admission(64), fam_long_row(True), fam_long_row(False)],
    "window": lambda ch: [fam_window(ch(c_), km) for c_, km in ((64, 0), (100, 0), (128, 0), (128, 1), (128, 63), (312, 0))],
    "wide": lambda ch: [fam_wide(ch(64), 1), fam_wide(ch(128), 63), fam_wide(ch(128), 1), fam_wide(ch(312), 0)],
    "row_shapes": lambda ch: [fam_row_shapes(cm) for cm in COLMODES],
    "repeated": lambda ch: [fam_repeated(cm) for cm in ("w244", "tiles4", "w120")],
    "dense": lambda ch: [fam_dense(128, 250), fam_dense(128, 0), fam_dense(100, 250), fam_dense(102, 250), fam_dense(64, 0),
                         fam_dense(312, 0)],
    "partial": lambda ch: [fam_partial(r) for r in (1, 2, 4, 8, 31)] + [fam_partial(31, only=True)],
    "lists": lambda ch: [fam_lists(nq) for nq in list(range(1, 18)) + [63, 64, 65]] + [fam_lists(9, mix=True), fam_lists(64, mix=True),
                                                                                      fam_all_panel(False), fam_all_panel(True)],
    "nblk": lambda ch: [fam_nblk(nb) for nb in (255, 256, 257, 2047, 2048, 2049)],
}


def group(name, selection="band_8_waves"):
    """The families of a group as built for a kernel selection: the window and wide families are laid around the chunk that
    selection really stages (16 waves leave room for 304 rows, not 312)."""
    sel = SELECTIONS[selection]
    return GROUPS[name](lambda c_: knobs(dict(sel, **{E + "BAND_CH": str(c_)}))["band_ch"])


def env_of(f, selection):
    """The environment of an inspect: the selection's knobs under the family's own (a family that sets a knob keeps it)."""
    return dict(SELECTIONS[selection], **f.env)


# -------------------------------------------------------------------------------------------------- data, reference, model
def exact_data(f, seed=7):
    """(values, B k x NMAX, C0 m x NMAX): small integers, every partial sum below 2^24 in any order."""
    rng = np.random.default_rng(seed)
    values = rng.choice(L.EXACT_VALUES, f.nnz)
    B = rng.integers(-2, 3, (f.k, NMAX)).astype(np.float64)
    C0 = rng.integers(-3, 4, (f.m, NMAX)).astype(np.float64)
    assert 2 * 2 * max(int(np.diff(f.rowptr).max()), 1) * 2 + 8 < 2 ** 24
    return values, B, C0


def random_data(f, seed=8):
    rng = np.random.default_rng(seed)
    return L.random_real(rng, f.nnz), L.random_real(rng, (f.k, NMAX)), L.random_real(rng, (f.m, NMAX))


def reference(f, values, B, alpha=1.0, beta=0.0, C0=None):
    """(C, sum |a||b| scaled) in fp64: repeated pairs summed, only stored entries multiplied, alpha * sum + beta * C0."""
    v = np.asarray(values, dtype=np.float64)
    A = sps.csr_matrix((v, f.colind, f.rowptr), shape=f.shape)
    Aabs = sps.csr_matrix((np.abs(v), f.colind, f.rowptr), shape=f.shape)
    with np.errstate(invalid="ignore"):
        C, absr = alpha * (A @ B), abs(alpha) * (Aabs @ np.abs(B))
    if beta != 0.0:
        C, absr = C + beta * C0, absr + abs(beta) * np.abs(C0)
    return C, absr


def host_model(f, values, B, env, mutation=None):
    """A B as the kernels the environment selects would compute it, structure for structure (fp64; NaN where a branch would
    read what it never staged).  Mutations: 'later_only' (the dense tile keeps only the later entry of a repeated pair more
    than a batch apart), 'le_ch' (the band kernel takes its single-chunk branch for w.y - w.x <= CH), 'w_not_wp' (probe)."""
    c = constants()
    kn = knobs(env)
    ch = kn["band_ch"]
    kind, nt, tiles, win, _ = probe_family(f, env, mutation)
    values = np.asarray(values, dtype=np.float64)
    C = np.zeros((f.m, B.shape[1]))
    for b in range(len(kind)):
        r0, r1 = b * 32, min(b * 32 + 32, f.m)
        rows = [(r, f.colind[f.rowptr[r]:f.rowptr[r + 1]].astype(np.int64), values[f.rowptr[r]:f.rowptr[r + 1]])
                for r in range(r0, r1)]
        cmin, cmax = int(win[b, 0]), int(win[b, 1])
        if kind[b] == 0:
            for r, cc, vv in rows:
                C[r] = vv @ B[cc] if len(cc) else 0.0
        elif not kn["band"]:               # tile kernel: the listed tiles, one after the other
            for r, cc, vv in rows:
                for t in tiles[b]:
                    sel = cc // c["MM_KT"] == t
                    C[r] += vv[sel] @ B[cc[sel]]
        elif kind[b] == 1:
            single = cmax - cmin <= ch if mutation == "le_ch" else cmax - cmin < ch
            if single:                                        # CH rows staged from cmin on
                for r, cc, vv in rows:
                    C[r] = vv @ B[cc] if len(cc) else 0.0
                    if (cc - cmin >= ch).any():
                        C[r] = np.nan
            else:
                G = group_size(ch)
                for g0 in range(0, int(nt[b]), G):
                    grp = tiles[b][g0:g0 + G]
                    for r, cc, vv in rows:
                        sel = np.isin(cc // c["MM_KT"], grp)
                        C[r] += vv[sel] @ B[cc[sel]]
        else:                                                 # dense 32 x Wp tile, built wave by wave (8 waves, 4 rows each)
            W = cmax - cmin + 1
            Wp = (W + 3) & ~3
            At = np.zeros((32, Wp))
            for w0 in range(0, 32, 4):
                mine = [x for x in rows if w0 <= x[0] - r0 < w0 + 4]
                dup = False
                for r, cc, vv in mine:
                    claimed = set()
                    for base in range(0, len(cc), 64):
                        batch = [int(x) for x in cc[base:base + 64]]
                        if mutation != "later_only":
                            dup |= any(x in claimed for x in batch)       # a tag of an earlier batch in the slot
                        dup |= len(set(batch)) < len(batch)               # the read-back finds another lane's tag
                        claimed.update(batch)
                for r, cc, vv in mine:
                    if dup:
                        np.add.at(At[r - r0], cc - cmin, vv)
                    else:
                        At[r - r0, cc - cmin] = vv                        # (a later store wins)
            Bt = np.zeros((Wp, B.shape[1]))
            Bt[:W] = B[cmin:cmin + W]
            C[r0:r1] = (At @ Bt)[:r1 - r0]
    return C
