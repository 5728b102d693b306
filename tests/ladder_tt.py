"""Deterministic ladders for csrc/transpose.hip (the radix transpose and scale_kernel) and for the level plan of csrc/sptrsv.hip
(which csrc/sptrsm.hip shares), next to tests/ladder.py and in its style: tests/test_gpu_tt_ladders.py runs them on the device,
tests/test_ladders_tt_cpu.py proves on the host that the generators hold every rung they claim and that the checkers bite.
Every limit is READ from the sources (transpose_limits, trsv_limits); a pattern that no longer matches fails with the name of
this file.

TRANSPOSE.  A case is (name, m, n, rowptr, colind, passes it must take); the value of entry p is float(p), so with fewer than
2^24 entries every value is distinct and a misplaced entry or a stability error changes a bit.  Families (*_cases()):
columns (the pass counts 1 ... 4 and one case per byte that alone decides the order), entries (around the tile, the XCD remap's
body and remainder), rows against tiles (round / wave / tile carries of the row-of-entry reconstruction, the marking loop's
stride, thousands of empty rows on one position), gaps (every class of spt_rowptr_fill_kernel as interior, leading and
trailing gap; the list of long gaps as full as n admits), buckets.  transpose_violations compares the bits of all three arrays with
oracle.transpose.

SCALE.  scale_cases(): n = 0 ... 70 x start offset 0 ... 4, and n around the capped grid.

TRIANGULAR SOLVE.  trsv_system(widths, shapes, lanes): a CSR matrix whose level sets have exactly the given widths, whose rows
of level >= 1 take the given shapes (number of strict entries, in-row positions of the stored diagonal entries) in turn, and
whose mean row length selects `lanes` lanes per row; the rows of a level are spread over the index range (an "anchor" row per
level keeps every later level reachable: row indices are the ranks of random keys, the anchor of level l has key l * eps), the
upper variant is the index mirror.  EXACT data: x_true in {+-1, +-2, +-3}, strict entries in {+-1, +-2}, diagonals in
{0.5, 1, 2, 4}, alpha in {1, -2, 0.5}, b = T x_true in float64: every product a x and every partial sum of them, in any order,
is an integer below 2^22 (asserted); alpha and the diagonal are powers of two, so alpha * dot, b - alpha * dot (multiples of
1/4 below 2^24) and the division are exact too -- the device x must EQUAL x_true under any lane count and any schedule.
Entries of the other triangle, diagonal entries stored before the last one and the stored diagonal of a unit solve hold NaN.
levels_of() restates the level sets from their definition, predicted_info() what spblas_gfx950_sptrsv_info must report.
"""
import os
import re

import numpy as np
import scipy.sparse as sps

import ladder as L

CSRC = L.CSRC


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _get(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the source no longer has the expected form; update tests/ladder_tt.py"
    return [int(g) for g in m.groups()]


# ============================================================================================================ transpose
def transpose_limits():
    """Every size csrc/transpose.hip branches on."""
    src = _src("transpose.hip")
    flat = re.sub(r"\s+", " ", src)
    t = {}
    t["waves"], = _get(r"constexpr int SPT_WAVES = (\d+);", src, "SPT_WAVES")
    t["rounds"], = _get(r"constexpr int SPT_ROUNDS = (\d+);\s*constexpr int SPT_TILE = SPT_WAVES \* SPT_ROUNDS \* 64;", src,
                        "SPT_ROUNDS / SPT_TILE of transpose_radix")
    t["round"] = 64
    t["wave"] = t["rounds"] * 64                      # entries a wave owns
    t["tile"] = t["waves"] * t["wave"]
    t["mark_stride"], = _get(r"for \(int j = 1 \+ tid; j <= r_hi - r_lo; j \+= (\d+)\)", src, "the marking loop")
    t["xcds"], = _get(r"const int64_t per = ntiles / (\d+), body = per \* \1;", src, "the XCD remap")
    t["gap_lane"], = _get(r"if \(len > 0 && len <= (\d+)\)", src, "the lane-filled gaps")
    t["gap_wave"], = _get(r"if \(len > (\d+)\) \{ const unsigned slot = atomicAdd\(n_longs, 1u\);", flat, "the long gaps")
    g2 = _get(r"__ballot\(len > (\d+) && len <= (\d+)\)", src, "the wave-filled gaps")
    assert g2 == [t["gap_lane"], t["gap_wave"]], "gap classes disagree; update tests/ladder_tt.py"
    t["fill_items"], = _get(r"const int64_t t0 = (\d+) \* q;", src, "work items per lane of spt_rowptr_fill_kernel")
    t["long_div"], t["long_slack"] = _get(r"long_b = al\(\(size_t\) \(n / (\d+) \+ (\d+)\) \* sizeof\(int4\)\)", src,
                                          "the room of the long-gap list")
    t["bits"], = _get(r"const int passes = \(bits \+ 7\) / (\d+);", src, "bits per pass")
    t["scale_blocks_per_cu"], = _get(r"spblas_gfx950_scale\(.*?const int64_t cap = \(int64_t\) \(handle->num_cus > 0 \? "
                                     r"handle->num_cus : 256\) \* (\d+);", flat, "the grid cap of scale")
    t["scale_per_f32"], t["scale_per_f64"] = _get(r"const int64_t per = value_type == SPBLAS_GFX950_F32 \? (\d+) : (\d+);",
                                                  src, "elements per lane of scale")
    t["scale_block"], = _get(r"int64_t blocks = cdiv\(cdiv\(n, per\), (\d+)\);", src, "the block of scale")
    return t


def passes_of(n):
    """transpose_radix: bits = the least b >= 1 with 2^b >= n; one pass per 8 bits."""
    bits = 1
    while bits < 32 and (1 << bits) < n:
        bits += 1
    return (bits + 7) // 8


class TCase:
    def __init__(self, name, m, n, rowptr, colind, tags=()):
        self.name, self.m, self.n = name, int(m), int(n)
        self.rowptr = np.asarray(rowptr, np.int64)
        self.colind = np.asarray(colind, np.int32)
        self.tags = set(tags)
        self.passes = passes_of(n)
        assert self.rowptr.size == m + 1 and self.rowptr[0] == 0 and self.rowptr[-1] == self.colind.size
        assert (np.diff(self.rowptr) >= 0).all() and self.colind.size < 2 ** 24
        assert self.colind.size == 0 or (self.colind.min() >= 0 and self.colind.max() < n)

    @property
    def nnz(self):
        return int(self.colind.size)

    def values(self, dtype):
        return np.arange(self.nnz, dtype=dtype)


def _row_lens(rng, nnz, hi=12):
    """Random row lengths 0 ... hi that sum to nnz."""
    lens = []
    left = nnz
    while left > 0:
        chunk = rng.integers(0, hi + 1, max(8, 2 * left // max(hi, 1) + 8))
        c = np.cumsum(chunk)
        k = int(np.searchsorted(c, left, side="left"))
        if k < chunk.size:
            chunk = chunk[:k + 1]
            chunk[-1] -= c[k] - left
            lens.append(chunk)
            left = 0
        else:
            lens.append(chunk)
            left -= int(c[-1])
    return np.concatenate(lens) if lens else np.zeros(0, np.int64)


def _case(name, n, colind, lens=None, rng=None, tags=()):
    colind = np.asarray(colind, np.int64)
    if lens is None:
        lens = _row_lens(rng, colind.size)
    lens = np.asarray(lens, np.int64)
    assert lens.sum() == colind.size, (name, lens.sum(), colind.size)
    return TCase(name, lens.size, n, np.concatenate([[0], np.cumsum(lens)]), colind, tags)


def _ends(rng, n, nnz):
    """nnz random columns below n with column 0 and column n - 1 in use (when nnz allows)."""
    c = rng.integers(0, n, nnz)
    if nnz >= 2:
        i, j = rng.choice(nnz, 2, replace=False)
        c[i], c[j] = 0, n - 1
    elif nnz == 1 and n == 1:
        c[0] = 0
    return c


COLUMN_NS = (1, 2, 255, 256, 257, 65535, 65536, 65537, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1)
BYTE_N = 2 ** 24 + 300          # four passes; the columns base and base + 2^24 differ in the fourth byte alone


def column_cases(seed=71):
    """Family 1: every n of COLUMN_NS (5 000 entries: one whole tile and a partial one), columns 0 and n - 1 in use; and four
    cases of BYTE_N columns whose entries differ in ONE byte of the column, so that one pass alone decides the order."""
    rng = np.random.default_rng(seed)
    out = [_case(f"n{n}", n, _ends(rng, n, 5000), rng=rng, tags={"columns"}) for n in COLUMN_NS]
    base = 0x00214325
    for byte in range(4):
        d = rng.integers(0, 256 if byte < 3 else 2, 5000)
        cols = ((base if byte < 3 else 0x25) & ~(0xFF << (8 * byte))) | (d << (8 * byte))
        assert np.unique(cols).size == (256 if byte < 3 else 2) and cols.max() < BYTE_N
        out.append(_case(f"byte{byte}", BYTE_N, cols, rng=rng, tags={"columns", f"byte{byte}"}))
    return out


def entry_counts():
    T = transpose_limits()["tile"]
    s = set(range(1, 10)) | {1023, 1024, 1025, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1}
    for k in (7, 8, 9, 15, 16, 17):
        s |= {k * T - 1, k * T, k * T + 1}
    return sorted(s)


def entry_cases(seed=72, n=300):
    """Family 2: every count of entry_counts() on n = 300 columns (two passes), nnz = 0 with n > 0, m = 0, m = 1."""
    rng = np.random.default_rng(seed)
    out = [_case(f"nnz{z}", n, _ends(rng, n, z), rng=rng, tags={"entries"}) for z in entry_counts()]
    out.append(_case("nnz0", n, [], lens=[0] * 7, tags={"entries", "empty"}))
    out.append(_case("m0", n, [], lens=[], tags={"entries", "empty"}))
    out.append(_case("m0_n0", 0, [], lens=[], tags={"entries", "empty"}))
    out.append(_case("m1", n, _ends(rng, n, 700), lens=[700], tags={"entries"}))
    out.append(_case("m1_empty", n, [], lens=[0], tags={"entries", "empty"}))
    return out


def row_cases(seed=73, n=300):
    """Family 3: rows against tiles.  The lists of row lengths are written out; row_starts(case) gives the positions to check."""
    t = transpose_limits()
    T, rng = t["tile"], np.random.default_rng(seed)
    specs = {}
    specs["start_at_tile"] = [T - 7, 7, 9, T - 9, 5]                   # rows start at T and 2T, rows end at T - 1 and 2T - 1
    specs["span3"] = [100, 3 * T, 50]                                   # tiles 1 and 2 (entries T ... 3T - 1) hold no row start
    carry = [63, 1, 1, 446, 1, 1]                                       # starts at 63, 64, 65, 511, 512, 513
    specs["carries"] = carry + [T - 513] + carry + [T - 513] + [11]     # ... in tile 0 and in tile 1
    for k in (t["mark_stride"] + 1, 2 * t["mark_stride"] + 1):
        specs[f"starts{k}"] = [40] + [1] * (k - 1) + [T - 40 - (k - 1) + 10] + [T]   # k row starts inside tile 0 (one at 0)
    specs["empties3000"] = [5] + [0] * 3000 + [7, 3]                    # the last of 3001 rows at position 5 owns the entry
    specs["empties_tile_edge"] = [0] * 10 + [T] + [0] * 10 + [20] + [0] * 10   # leading, on the tile boundary, trailing
    specs["empties_trailing_full_tile"] = [0, 0, T - 1, 1] + [0] * 600  # empty rows behind the last entry of a whole tile
    out = []
    for name, lens in specs.items():
        z = int(np.sum(lens))
        out.append(_case(name, n, _ends(rng, n, z), lens=lens, tags={"rows"}))
    return out


def in_tile_starts(case, tile):
    """In-tile positions of the rows that start inside the given tile (a position once per row, empty rows included)."""
    T = transpose_limits()["tile"]
    p = case.rowptr[:-1]
    return p[(p >= tile * T) & (p < min((tile + 1) * T, max(case.nnz, 1)))] - tile * T


GAP_LENS = tuple(range(1, 11)) + (63, 64, 65, 4095, 4096, 4097, 4098, 100_000)


def gap_lens(case):
    """(interior gap lengths, leading, trailing) as spt_rowptr_fill_kernel sees them: len = hi - lo + 1 of work item t, with
    lo = column of entry t - 1 + 1 (0 for t = 0) and hi = column of entry t (n for t = nnz), over the SORTED columns."""
    c = np.sort(case.colind.astype(np.int64))
    if c.size == 0:
        return np.zeros(0, np.int64), case.n + 1, case.n + 1
    return np.diff(c), int(c[0]) + 1, case.n - int(c[-1])


def gap_cases(seed=74):
    """Family 4: for every g of GAP_LENS one case whose LEADING and TRAILING gaps are g and whose interior holds every length
    of GAP_LENS (each occupied column 1 ... 3 times, entries dealt to rows at random); "long_full": as many gaps above the wave
    limit as n = 2^24 admits; "long_few": three of them on a narrow matrix."""
    t = transpose_limits()
    assert {t["gap_lane"], t["gap_lane"] + 1, t["gap_wave"], t["gap_wave"] + 1} <= set(GAP_LENS)
    rng = np.random.default_rng(seed)
    out = []
    for g in GAP_LENS:
        cols = np.cumsum(np.concatenate([[g - 1], rng.permutation(GAP_LENS)]))
        n = int(cols[-1]) + g
        entries = rng.permutation(np.repeat(cols, rng.integers(1, 4, cols.size)))
        out.append(_case(f"gap{g}", n, entries, rng=rng, tags={"gaps"}))
    step = t["gap_wave"] + 1
    n = 2 ** 24
    cols = np.arange(step - 1, n, step)                                  # leading gap `step`, every interior gap `step`
    out.append(_case("long_full", n, rng.permutation(np.repeat(cols, 2)), rng=rng, tags={"gaps", "long_full"}))
    out.append(_case("long_few", 3 * step + 2, rng.permutation(np.repeat(np.arange(step - 1, 3 * step, step), 3)), rng=rng,
                     tags={"gaps"}))
    return out


def bucket_cases(seed=75):
    """Family 5: every entry in one column; a tile in which each of the 256 digits occurs exactly once (one and two passes);
    one row with the same column on both sides of a round, a wave and a tile boundary."""
    t = transpose_limits()
    T, rng = t["tile"], np.random.default_rng(seed)
    out = [_case("one_column", 70_000, np.full(2 * T + 5, 4321), rng=rng, tags={"buckets"})]
    out.append(_case("digits_once", 256, rng.permutation(256), rng=rng, tags={"buckets"}))
    out.append(_case("digits_once_two_passes", 65536, rng.permutation(256) * 256 + rng.permutation(256), rng=rng,
                     tags={"buckets"}))
    z = T + 300
    cols = rng.integers(0, 300, z)
    for edge, col in ((t["round"], 17), (t["wave"], 18), (T, 19)):
        cols[edge - 1] = cols[edge] = col
    out.append(_case("duplicates_on_edges", 300, cols, lens=[z], tags={"buckets"}))
    return out


def state_cases(seed=76):
    """Family 7: a large four-pass case, a one-tile one-pass case, a case with long gaps, one without (run in this order,
    each twice, on one handle)."""
    rng = np.random.default_rng(seed)
    T = transpose_limits()["tile"]
    big = _case("state_big4", 2 ** 24 + 1, _ends(rng, 2 ** 24 + 1, 20 * T + 77), rng=rng, tags={"state"})
    small = _case("state_tile1", 200, _ends(rng, 200, 900), rng=rng, tags={"state"})
    longs = _case("state_longs", 50_000, _ends(rng, 50_000, 30), rng=rng, tags={"state"})
    dense = _case("state_no_longs", 40_000, np.concatenate([rng.permutation(40_000), _ends(rng, 40_000, 500)]), rng=rng,
                  tags={"state"})
    assert (gap_lens(longs)[0] > 4096).any() and max(gap_lens(dense)[0].max(), *gap_lens(dense)[1:]) <= 8
    return [big, small, longs, dense]


def alignment_case(seed=77):
    T = transpose_limits()["tile"]
    rng = np.random.default_rng(seed)
    return _case("alignment", 300, _ends(rng, 300, 2 * T + 3), rng=rng, tags={"alignment"})


ALIGN_SHIFTS = [(s,) * 5 for s in range(4)] + [tuple(s if i == k else 0 for i in range(5)) for k in range(5) for s in (1, 2, 3)]


def transpose_reference(case, dtype):
    from oracle import oracle
    return oracle.transpose((case.m, case.n), case.rowptr.astype(np.int32), case.colind, case.values(dtype))


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def transpose_violations(case, got, ref):
    """Messages (empty: passes) of the bit-for-bit comparison of (row offsets, columns, values) with the reference's."""
    out = []
    for g, r, what in zip(got, ref, ("row offsets", "columns", "values")):
        g, r = np.asarray(g), np.asarray(r)
        if g.shape != r.shape:
            out.append(f"{case.name}: {what}: shape {g.shape} != {r.shape}")
            continue
        bad = np.flatnonzero(_u(g) != _u(r))
        if bad.size:
            out.append(f"{case.name}: {what}: {bad.size} differ, first at {bad[:5].tolist()}: {g[bad[:5]].tolist()} != "
                       f"{r[bad[:5]].tolist()}")
    return out


# ================================================================================================================ scale
def scale_cases(num_cus):
    """(vt, n, offset) of the scale ladder: n = 0 ... 70 x offset 0 ... 4, and n around the capped grid (cap blocks of a block of
    lanes x elements per lane): cap * elements - 1, + 0, + 1, + 5, and twice that + 3."""
    t = transpose_limits()
    out = []
    for vt, per in (("f32", t["scale_per_f32"]), ("f64", t["scale_per_f64"])):
        out += [(vt, n, off) for n in range(71) for off in range(5)]
        full = num_cus * t["scale_blocks_per_cu"] * t["scale_block"] * per
        out += [(vt, n, off) for n in (full - 1, full, full + 1, full + 5, 2 * full + 3) for off in (0, 1)]
    return out


def scale_data(n, off, dtype, seed=0):
    """(base array, expected base array): n + off + 5 small integers, the view [off, off + n) times -1.75."""
    rng = np.random.default_rng(seed + n + 7 * off)
    base = rng.integers(-8, 9, n + off + 5).astype(dtype)
    want = base.copy()
    want[off:off + n] *= dtype(-1.75)
    return base, want


# ===================================================================================================== triangular solve
def trsv_limits():
    """Every size csrc/sptrsv.hip branches on."""
    src = _src("sptrsv.hip")
    flat = re.sub(r"\s+", " ", src)
    t = {}
    t["kahn_narrow"], = _get(r"#define TRSV_NARROW (\d+)", src, "TRSV_NARROW")
    t["coop_threads"], = _get(r"#define TRSV_COOP_THREADS (\d+)", src, "TRSV_COOP_THREADS")
    a = _get(r"avg > (\d+) \? (\d+) : \(avg > (\d+) \? (\d+) : \(avg > (\d+) \? (\d+) : (\d+)\)\)", src, "lanes per row")
    t["lane_steps"] = [(a[4], a[6], a[5]), (a[2], a[5], a[3]), (a[0], a[3], a[1])]       # (mean limit, lanes at or below, above)
    r = _get(r"constexpr int R = G <= (\d+) \? (\d+) : \(G <= (\d+) \? (\d+) : (\d+)\);", src, "row slots per lane group")
    t["slots"] = {g: (r[1] if g <= r[0] else r[3] if g <= r[2] else r[4]) for g in (4, 8, 16, 64)}
    t["narrow"], = _get(r'env_int\("SPBLAS_GFX950_TRSV_NARROW", (\d+)\)', src, "the narrow limit")
    t["max_run"], = _get(r'env_int\("SPBLAS_GFX950_TRSV_COOP_MAX_RUN", (\d+)\)', src, "the longest narrow run")
    h = _get(r"__shared__ int lh\[(\d+)\];", src, "the LDS histogram of the inspect")
    t["hist_levels"] = h[0]
    t["kahn_batch"], = _get(r"const int batch = (\d+);", src, "Kahn's batch of launches")
    t["kahn_rows_per_block"], t["kahn_max_blocks"] = _get(
        r"const int adv_grid = \(int\) \(cdiv\(m, (\d+)\) < (\d+) \?", src, "Kahn's advance grid")
    assert re.search(r"pl->coop_ok && ng > 1 && !capturing", flat) and \
        re.search(r"info\[2\] = plan->coop_ok && plan->groups.size\(\) > 1 \? 1 :", flat), \
        "launches per solve: the source no longer has the expected form; update tests/ladder_tt.py"
    return t


def lanes_of(nnz, m):
    avg = nnz / m if m > 0 else 0.0
    lanes = trsv_limits()["lane_steps"][0][1]
    for limit, _, above in trsv_limits()["lane_steps"]:
        if avg > limit:
            lanes = above
    return lanes


def pipelined_pass(grid, lanes):
    """Rows one pipelined pass of trsv_coop_kernel covers: grid x (threads / G) x R."""
    t = trsv_limits()
    return grid * (t["coop_threads"] // lanes) * t["slots"][lanes]


TARGET_MEAN = {4: 4.0, 8: 12.0, 16: 40.0, 64: 110.0}


class Shape:
    """One row of level >= 1: `strict` entries of the solve's triangle (>= 1) and the in-row positions of its stored diagonal
    entries (ascending; the LAST is the one the solve reads, "last" = the row's last position, () = none stored).  The row is
    padded with entries of the other triangle up to the furthest position asked for."""

    def __init__(self, strict, dpos=("last",), name=None):
        self.strict, self.dpos = int(strict), tuple(dpos)
        self.name = name or f"s{strict}_d{'_'.join(str(p) for p in dpos) or 'none'}"


def strict_counts(lanes):
    return sorted(set(range(0, 2 * lanes + 3)) | {3 * lanes - 1, 3 * lanes, 3 * lanes + 1, 300})


def row_shapes(lanes, unit):
    """The row-shape rungs for `lanes` lanes per row: every strict count of strict_counts (0 is a level-0 row: the generator's
    own rows), each with the diagonal last; the diagonal first, last, at position G - 1, G, 2G - 1, 2G on three strict counts;
    none stored (unit solves); stored twice with the pair in (c0, c1), (c1, loop), (loop, loop)."""
    G = lanes
    out = [Shape(s) for s in strict_counts(G) if s > 0]
    for s in (1, G + 1, 2 * G + 2):
        for p in (0, G - 1, G, 2 * G - 1, 2 * G):
            out.append(Shape(s, (p,)))
        out.append(Shape(s, (1, G + 2), f"s{s}_pair_c0_c1"))
        out.append(Shape(s, (G + 1, 2 * G + 3), f"s{s}_pair_c1_loop"))
        out.append(Shape(s, (2 * G + 1, 3 * G + 2), f"s{s}_pair_loop_loop"))
        if unit:
            out.append(Shape(s, ()))
    names = [x.name for x in out]
    assert len(set(names)) == len(names)
    return out


def slot_of(pos, lanes):
    """Where trsv_coop_kernel holds in-row position `pos`: the first two entries per lane are pipelined, the rest looped."""
    return "c0" if pos < lanes else "c1" if pos < 2 * lanes else "loop"


class System:
    pass


def trsv_system(widths, shapes, lanes, upper=False, unit=False, seed=0, nnz_total=None, alpha=1.0):
    """See the module docstring.  widths[l] = rows of level l (level 0 needs 2 rows, or 1 when no row asks for padding);
    shapes are dealt to the rows of levels >= 1 in turn, level by level; the rows of level 0 hold their diagonal and as many
    entries of the other triangle as bring the matrix to nnz_total entries (default: TARGET_MEAN[lanes] per row) -- level 0
    is NOT widened: a ladder whose shapes are too long for the mean must ask for a wider level 0 (asserted).  Returns a System:
    rowptr, colind (int32), m, level (designed level per row), shape_of (name per row), exact (values, b, x_true),
    random (values, b)."""
    rng = np.random.default_rng(seed)
    widths = [int(w) for w in widths]
    assert widths and min(widths) >= 1
    nl, m = len(widths), int(sum(widths))
    level = np.repeat(np.arange(nl), widths)
    first = np.concatenate([[0], np.cumsum(widths)])[:-1]
    # keys -> row indices: the anchor (first row) of level l has key l * eps, the others are uniform above it
    key = rng.random(m) * 0.999 + 0.0005
    key[first] = np.arange(nl) * (0.0004 / nl)
    cap = widths[0] >= 2
    if cap:
        key[1] = 2.0                                     # the highest index: a plain level-0 row (no other triangle there)
    idx = np.empty(m, np.int64)
    idx[np.argsort(key, kind="stable")] = np.arange(m)
    # shapes
    n_shaped = m - widths[0]
    sid = np.arange(n_shaped) % max(len(shapes), 1)
    strict = np.zeros(m, np.int64)
    d1 = np.full(m, -1, np.int64)                         # position of an earlier (NaN) diagonal entry, -1: none
    d2 = np.full(m, -2, np.int64)                         # position of the diagonal entry read; -2: last position, -1: none
    strict[widths[0]:] = np.array([s.strict for s in shapes], np.int64)[sid] if n_shaped else 0
    shape_of = np.array(["level0"] * m, dtype=object)
    if n_shaped:
        for k, s in enumerate(shapes):
            rows = widths[0] + np.flatnonzero(sid == k)
            shape_of[rows] = s.name
            assert s.strict >= 1, "a row of level >= 1 has a strict entry"
            if len(s.dpos) == 0:
                assert unit, "a row without a stored diagonal needs a unit solve"
                d2[rows] = -1
            elif s.dpos[-1] != "last":
                d2[rows] = s.dpos[-1]
            if len(s.dpos) == 2:
                d1[rows] = s.dpos[0]
    top = int(np.argmax(idx))
    if not cap and (d2[top] >= 0 or d1[top] >= 0):        # the highest index cannot be padded: plain shape there
        d1[top], d2[top], shape_of[top] = -1, -2, f"s{strict[top]}_dlast"
    nd = (d1 >= 0).astype(np.int64) + (d2 != -1)
    far = np.maximum(d1, d2)                              # furthest position asked for
    other = np.maximum(0, far + 1 - strict - nd)
    base_total = int((strict + nd + other).sum())
    if nnz_total is None:
        nnz_total = int(round(TARGET_MEAN[lanes] * m))
    extra = nnz_total - base_total
    assert extra >= 0, f"{base_total} entries before padding, {nnz_total} wanted: widen level 0 or shorten the shapes"
    free = np.arange(widths[0])
    free = free[idx[free] != m - 1]
    assert extra == 0 or free.size, "no level-0 row can take padding"
    if extra:
        other[free] += extra // free.size
        other[free[:extra % free.size]] += 1
    length = strict + nd + other
    d2 = np.where(d2 == -2, length - 1, d2)
    assert (d2 < length).all() and ((d1 < d2) | (d1 < 0)).all()
    rowptr_d = np.concatenate([[0], np.cumsum(length)])   # in "designed" row order
    nnz = int(rowptr_d[-1])
    assert nnz == nnz_total and lanes_of(nnz, m) == lanes, (nnz, m, lanes_of(nnz, m), lanes)
    row_e = np.repeat(np.arange(m), length)
    pos = np.arange(nnz) - rowptr_d[:-1][row_e]
    is_d1 = pos == d1[row_e]
    is_d2 = pos == d2[row_e]
    j = pos - (is_d1 | (pos > d1[row_e]) & (d1[row_e] >= 0)) * 1 - ((pos > d2[row_e]) & (d2[row_e] >= 0)) * 1
    nondiag = ~(is_d1 | is_d2)
    cnt = (strict + other)[row_e]
    rot = rng.integers(0, 1 << 30, m)[row_e]
    is_strict = nondiag & (((j + rot) % np.maximum(cnt, 1)) < strict[row_e])
    is_other = nondiag & ~is_strict
    assert np.array_equal(np.bincount(row_e[is_strict], minlength=m), strict)
    col = np.full(nnz, -1, np.int64)
    col[is_d1 | is_d2] = idx[row_e[is_d1 | is_d2]]
    # strict entries: the first of a row reads level l - 1, the others any earlier level; always a smaller index
    se = np.flatnonzero(is_strict)
    first_of_row = np.ones(se.size, bool)
    first_of_row[1:] = row_e[se[1:]] != row_e[se[:-1]]
    order_by_idx = np.argsort(idx)
    for l in range(1, nl):
        mine = se[level[row_e[se]] == l]
        if not mine.size:
            continue
        f = first_of_row[np.searchsorted(se, mine)]
        prev = np.sort(idx[level == l - 1])
        below = np.sort(idx[level < l])
        for pool, sel in ((prev, f), (below, ~f)):
            e = mine[sel]
            k = np.searchsorted(pool, idx[row_e[e]])
            assert (k >= 1).all()
            col[e] = pool[(rng.random(e.size) * k).astype(np.int64)]
    oe = np.flatnonzero(is_other)
    ri = idx[row_e[oe]]
    assert (ri < m - 1).all()
    col[oe] = ri + 1 + (rng.random(oe.size) * (m - 1 - ri)).astype(np.int64)
    assert (col >= 0).all() and (col < m).all()
    # values
    x_true = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], m)                # by row INDEX
    ev = np.full(nnz, np.nan)
    ev[is_strict] = rng.choice([-2.0, -1.0, 1.0, 2.0], int(is_strict.sum()))
    dv = rng.choice([0.5, 1.0, 2.0, 4.0], m)                                  # by designed row
    if not unit:
        ev[is_d2] = dv[row_e[is_d2]]
    rv = rng.uniform(-1.0, 1.0, nnz)
    rv[is_d1] = 0.0                                        # (scipy's diagonal() adds stored duplicates: the earlier one is 0)
    absrow = np.bincount(row_e[is_strict], weights=np.abs(rv[is_strict]), minlength=m)
    rv[is_d2] = (absrow + 1.0 + rng.random(m))[row_e[is_d2]]
    if unit:
        rv[is_strict] *= 0.1 / np.maximum(absrow, 1.0)[row_e[is_strict]]
    # designed order -> index order (and the index mirror for the upper triangle)
    new_row = idx[row_e]
    if upper:
        new_row, col, x_true = m - 1 - new_row, m - 1 - col, x_true[::-1].copy()
    perm = np.argsort(new_row, kind="stable")
    sysm = System()
    sysm.m, sysm.nnz, sysm.upper, sysm.unit, sysm.lanes, sysm.alpha = m, nnz, upper, unit, lanes, float(alpha)
    row_index = (m - 1 - idx) if upper else idx
    sysm.rowptr = np.concatenate([[0], np.cumsum(np.bincount(new_row, minlength=m))]).astype(np.int32)
    sysm.colind = col[perm].astype(np.int32)
    sysm.level = np.empty(m, np.int64)
    sysm.level[row_index] = level
    sysm.shape_of = np.empty(m, dtype=object)
    sysm.shape_of[row_index] = shape_of
    sysm.widths = widths
    sysm.kind = np.where(is_strict, 1, np.where(is_d2, 2, np.where(is_d1, 3, 0)))[perm]   # 1 strict, 2 diagonal read, 3 earlier
    sysm.x_true = x_true
    sysm.exact_values = ev[perm]
    sysm.random_values = rv[perm]
    # b = T x_true in float64, T = alpha (S + D) or alpha S + I
    rows_i = np.repeat(np.arange(m), np.diff(sysm.rowptr))
    st = sysm.kind == 1
    dot = np.bincount(rows_i[st], weights=sysm.exact_values[st] * x_true[sysm.colind[st]], minlength=m)
    anyorder = np.bincount(rows_i[st], weights=np.abs(sysm.exact_values[st] * x_true[sysm.colind[st]]), minlength=m)
    assert anyorder.max(initial=0.0) < 2 ** 22, "exact data leave the exact range"
    if unit:
        sysm.b = alpha * dot + x_true
    else:
        dg = np.zeros(m)
        dg[rows_i[sysm.kind == 2]] = sysm.exact_values[sysm.kind == 2]
        sysm.b = alpha * (dot + dg * x_true)
    assert np.array_equal(sysm.b * 4, np.round(sysm.b * 4)) and np.abs(sysm.b).max() < 2 ** 24
    return sysm


def levels_of(rowptr, colind, m, upper):
    """The level of every row from the definition: 0 without strict entries, else 1 + the deepest level among the rows read."""
    rowptr, colind = np.asarray(rowptr, np.int64), np.asarray(colind, np.int64)
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    s = (colind > rows) if upper else (colind < rows)
    r, c = rows[s], colind[s]
    lev = np.zeros(m, np.int64)
    if not r.size:
        return lev
    starts = np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1]]))
    owners = r[starts]
    while True:
        new = np.zeros(m, np.int64)
        new[owners] = np.maximum.reduceat(lev[c] + 1, starts)
        if np.array_equal(new, lev):
            return lev
        lev = new


def groups_of(widths, narrow):
    """The launch groups of the plan: every level of >= narrow rows alone, every run of narrower levels one group.  Returns
    [(first level, end level, wide)]."""
    out, l, n = [], 0, len(widths)
    while l < n:
        wide = widths[l] >= narrow
        e = l + 1
        if not wide:
            while e < n and widths[e] < narrow:
                e += 1
        out.append((l, e, wide))
        l = e
    return out


def predicted_info(rowptr, colind, m, upper, narrow=None, coop=True):
    """What _TrsvPlan.info() must report; coop=False: the cooperative launch is switched off or not available."""
    t = trsv_limits()
    narrow = t["narrow"] if narrow is None else narrow
    lev = levels_of(rowptr, colind, m, upper)
    widths = np.bincount(lev).tolist() if m else []
    groups = groups_of(widths, narrow)
    run = max([e - l for l, e, wide in groups if not wide], default=0)
    one = coop and run <= t["max_run"] and len(groups) > 1
    return {"levels": len(widths), "max_level_width": max(widths, default=0), "lanes_per_row": lanes_of(int(rowptr[-1]), m),
            "launches_per_solve": 1 if one else len(groups)}


def as_scipy(sysm, values):
    """The system as a scipy CSR matrix that keeps the stored order and the duplicates."""
    M = sps.csr_matrix((np.asarray(values, np.float64).copy(), sysm.colind.copy(), sysm.rowptr.copy()), shape=(sysm.m, sysm.m))
    M.has_canonical_format = True
    return M


def exact_violations(x, sysm):
    """Messages (empty: passes): x must equal x_true bit for bit (x_true has no zero: no sign of zero to allow for)."""
    x = np.asarray(x)
    want = sysm.x_true.astype(x.dtype)
    if x.ndim == 2:
        want = np.stack([want * f for f in BLOCK_FACTORS[:x.shape[1]]], axis=1).astype(x.dtype)
    bad = np.argwhere(_u(x) != _u(want))
    if not bad.size:
        return []
    i = tuple(int(v) for v in bad[0])
    return [f"{bad.shape[0]} elements differ from x_true, first at {list(i)} (level {sysm.level[i[0]]}, shape "
            f"{sysm.shape_of[i[0]]}): {x[i]} != {want[i]}"]


BLOCK_FACTORS = (1.0, -2.0, 0.5)      # column j of the block of right-hand sides is b times this: x_true times this, exactly


def block_rhs(sysm):
    return np.stack([sysm.b * f for f in BLOCK_FACTORS], axis=1)


# ------------------------------------------------------------------------------------------- the systems of the GPU tests
_SYSTEMS = {}
ALPHAS = (1.0, -2.0, 0.5)
NARROW_W, WIDE_W = 3, 130           # a narrow and a wide level of the sequences
SEQUENCES = [[NARROW_W], [WIDE_W], [NARROW_W, NARROW_W], [NARROW_W, WIDE_W], [WIDE_W, NARROW_W], [WIDE_W, WIDE_W],
             [NARROW_W, WIDE_W, NARROW_W], [WIDE_W, NARROW_W, WIDE_W], [NARROW_W, NARROW_W, WIDE_W],
             [WIDE_W, NARROW_W, NARROW_W], [NARROW_W, NARROW_W, WIDE_W, WIDE_W], [WIDE_W, WIDE_W, NARROW_W, NARROW_W],
             [NARROW_W, WIDE_W, NARROW_W, WIDE_W], [WIDE_W, NARROW_W, NARROW_W, NARROW_W, WIDE_W],
             [NARROW_W, NARROW_W, WIDE_W, NARROW_W, NARROW_W], [WIDE_W] * 5, [1]]


def _cached(key, make):
    if key not in _SYSTEMS:
        _SYSTEMS[key] = make()
    return _SYSTEMS[key]


def alpha_of(*k):
    return ALPHAS[sum(int(x) for x in k) % 3]


def shape_widths(lanes, unit):
    """([level 0, a run of narrow levels that holds every shape once, one wide level that holds every shape, the same narrow
    run], levels per run)."""
    n = len(row_shapes(lanes, unit))
    k = -(-n // 100)
    run = [n // k + (1 if i < n % k else 0) for i in range(k)]
    return [2000 if lanes == 4 else 600] + run + [max(130, n)] + run, len(run)


def shape_system(lanes, upper, unit):
    """C1: every row shape of row_shapes in a run of narrow levels (workgroup 0 / the chain kernel), in a wide level and in a last
    narrow run, behind a level 0 wide enough for the mean that selects `lanes`."""
    return _cached(("shapes", lanes, upper, unit),
                   lambda: trsv_system(shape_widths(lanes, unit)[0], row_shapes(lanes, unit), lanes, upper, unit, seed=lanes,
                                       alpha=alpha_of(lanes, upper, unit)))


def mean_cases():
    """[(limit, extra entries, lanes expected, system)]: nnz = limit * m takes the lower lane count, one entry more the higher."""
    out = []
    shapes = [Shape(1), Shape(2), Shape(5, (0,))]
    widths = [300, 40, 130]
    m = sum(widths)
    for limit, at, above in trsv_limits()["lane_steps"]:
        for extra, lanes in ((0, at), (1, above)):
            out.append((limit, extra, lanes, _cached(("mean", limit, extra), lambda: trsv_system(
                widths, shapes, lanes, seed=limit + extra, nnz_total=limit * m + extra, alpha=alpha_of(limit, extra)))))
    return out


def width_system(lanes, grid, upper=False, unit=False):
    """C2: (system, P).  Levels of 1 ... 5, narrow - 1, narrow, narrow + 1 rows and of P - 1, P, P + 1, 2P + 1 rows, P the pipelined pass
    of a grid of `grid` workgroups.  (A grid of more than 8 workgroups: only the wide rungs, P is thousands of rows.)"""
    def make():
        P = pipelined_pass(grid, lanes)
        small = grid <= 8
        narrow = trsv_limits()["narrow"]
        widths = ([200, 1, 2, 3, 4, 5, narrow - 1, narrow, narrow + 1] if small else [4096]) + [P - 1, P, P + 1, 2 * P + 1, 3]
        shapes = [Shape(1), Shape(2), Shape(3, (0,)), Shape(1, (lanes,))] + ([Shape(2 * lanes + 1)] if small else [])
        m = sum(widths)
        limit = {4: 5, 8: 6, 16: 24, 64: 96}[lanes]
        total = (6 * m if lanes == 4 else None) if small else int(limit * m + m // 2)
        return trsv_system(widths, shapes, lanes, upper, unit, seed=100 + lanes, nnz_total=total, alpha=alpha_of(lanes, grid)), P
    return _cached(("widths", lanes, grid, upper, unit), make)


def sequence_system(i):
    """C3: SEQUENCES[i]; triangle and diagonal kind alternate with i."""
    widths = SEQUENCES[i]
    return _cached(("seq", i), lambda: trsv_system(widths, [Shape(1), Shape(2, (0,)), Shape(9)], 4, bool(i & 1), bool(i & 2),
                                                   seed=200 + i, nnz_total=1 if widths == [1] else 6 * sum(widths),
                                                   alpha=alpha_of(i)))


def long_run_cases():
    """C3: [(name, widths)]: a narrow run of max_run and of max_run + 1 levels behind and in front of one wide level; chains around
    the levels the inspect's LDS histogram holds."""
    t = trsv_limits()
    run, hist = t["max_run"], t["hist_levels"]
    return [(f"wide_then_{k}", [WIDE_W] + [1] * k) for k in (run, run + 1)] + \
           [(f"{k}_then_wide", [1] * k + [WIDE_W]) for k in (run, run + 1)] + \
           [(f"chain{k}", [1] * k) for k in (hist - 1, hist, hist + 1, hist + 2)]


def long_run_system(i):
    name, widths = long_run_cases()[i]
    return _cached(("long", name), lambda: trsv_system(widths, [Shape(1), Shape(2)], 4, upper=bool(i & 1), seed=300 + i,
                                                       alpha=alpha_of(i)))


def kahn_cases():
    """C4: [(name, widths)] for SPBLAS_GFX950_TRSV_KAHN=1."""
    t = trsv_limits()
    K, batch = t["kahn_narrow"], t["kahn_batch"]
    edge = t["kahn_rows_per_block"] * t["kahn_max_blocks"]
    cases = [("frontiers", [K - 1, K + 1, K, K - 1, K, 5])]
    cases += [(f"wide{k}", [K] * k + [3]) for k in (batch - 1, batch, batch + 1)]
    cases += [("m1", [1])] + [(f"m{m}", [16, m - 16]) for m in (31, 32, 33)]
    cases += [(f"m{m}", [K * 4, m - K * 4]) for m in (edge - 1, edge, edge + 1)]
    return cases


def kahn_system(i):
    name, widths = kahn_cases()[i]
    return _cached(("kahn", name), lambda: trsv_system(widths, [Shape(1), Shape(2), Shape(3, (1,))], 4, upper=bool(i & 1),
                                                       unit=bool(i & 2), seed=400 + i,
                                                       nnz_total=1 if widths == [1] else None, alpha=alpha_of(i)))
