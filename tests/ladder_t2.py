"""The ladder of the plan-free transposed SpMV in its two-pass form (csrc/spmv.hip: t2_hist -> scan -> t2_plan -> t2_scatter ->
t2_accumulate): families built from specifications, the geometry restated on the host, and a host model of the kernel chain.

The edges of this code are not row lengths but TILES of T2_TILE consecutive entries, SLICES of W columns and SEGMENTS of `seg`
entries of a slice's run.  Every family parks entries, row starts, columns or slice shares on one of those edges; none is a
random draw.  The constants are read from the source (constants()), so the ladder follows the code.

geometry()   W, S, ntile, seg and the path, restated from spmv_typed: what spblas_gfx950_spmv_t_last must report.
model()      hist -> scan -> plan -> scatter -> accumulate in numpy, with the workgroup -> tile permutation, the reciprocal
             division, the marks + two-level running maximum of the row recovery, the counted placement, the item list and the
             accumulate loop's vector body and tail as the kernels have them; `mut` swaps one step for a wrong one
             (MUTATIONS), which tests/test_ladders_t2_cpu.py needs to show that the families bite.
Data sets    `ints`: small integer values and x; `probe`: all values 1, no column with two entries, x[i] = 1 + i mod 251, so
             y[col] IS the row the kernel took the entry for.  Every partial sum stays below 2^24 (asserted), so the order of
             addition cannot matter and y must match bit for bit.  `random`: uniform values under the existing parity bound.
             A family whose columns repeat (hot columns, n below nnz) runs the probe on probe_matrix(): the same rows, the
             columns replaced by distinct ones spread over all slices.
"""
import math
import os
import re

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE = "SPBLAS_GFX950_SPMV_T2"
HOOKS = (PRE, PRE + "_W", PRE + "_SEG")
INT32_MAX = 2 ** 31 - 1
ALPHA_BETA = ((1.0, 0.0), (-2.0, 0.5), (1.0, 1.0), (0.0, 0.5))

_CONST = {}


def cdiv(a, b):
    return -(-a // b)


def constants():
    """The numbers spmv_typed and the t2_* kernels branch on, parsed from csrc/spmv.hip."""
    if _CONST:
        return _CONST
    with open(os.path.join(ROOT, "spblas-reference_amd", "csrc", "spmv.hip")) as f:
        src = f.read()

    def grab(pattern, what):
        m = re.search(pattern, src)
        assert m, f"{what}: csrc/spmv.hip no longer has the expected form; update tests/ladder_t2.py"
        return [int(g) for g in m.groups()]

    c = _CONST
    c["TILE"], c["THREADS"], c["SMAX"] = grab(r"constexpr int T2_TILE = (\d+), T2_THREADS = (\d+), T2_SMAX = (\d+);", "T2_*")
    c["wcap_kib"], = grab(r"const int64_t Wcap = \((\d+) \* 1024\) / \(int64_t\) sizeof\(T\);", "Wcap")
    c["w_min"], = grab(r"Wsl = Wsl < (\d+) \? \1 : Wsl > Wcap \? Wcap : Wsl;", "default W")
    c["w_max"], c["wide_kib"] = grab(r"std::min<int64_t>\((\d+), \((\d+) \* 1024\) / \(int64_t\) sizeof\(T\)\)\);", "wide W")
    c["seg_min"], c["seg_mul"] = grab(r"unsigned seg = \(unsigned\) std::max<int64_t>\((\d+), (\d+) \* cdiv\(nnz, Ssl\)\);", "seg")
    c["w_hook_min"], = grab(r"if \(w_env >= (\d+) && w_env <= Wcap\)", "_T2_W hook")
    c["seg_hook_min"], = grab(r'env_int_spmv\("SPBLAS_GFX950_SPMV_T2_SEG", 0\) >= (\d+)\)', "_T2_SEG hook")
    c["want_nnz_shift"], c["want_n"] = grab(r"nnz >= \(\(int64_t\) (\d+) << 20\) && n >= (\d+)\);", "size rule")
    assert c["TILE"] == 8 * c["THREADS"] and c["TILE"] // 64 == 128, "the row recovery is restated for 128 segments of 64"
    return c


def wcap(vt):
    return constants()["wcap_kib"] * 1024 // (4 if vt == "f32" else 8)


def wide_w(vt):
    """The widest slice of the default geometry (more columns than SMAX slices of Wcap hold)."""
    c = constants()
    return min(c["w_max"], c["wide_kib"] * 1024 // (4 if vt == "f32" else 8))


def geometry(vt, shape, nnz, env, cus):
    """What spmv_typed decides for an un-inspected op = T call: the dict api._Handle.spmv_t_last() reports (without n_items)."""
    c = constants()
    m, n = shape
    t2 = int(env.get(PRE, -1))
    W = (cdiv(n, 2 * cus) + 63) & ~63
    W = c["w_min"] if W < c["w_min"] else min(W, wcap(vt))
    if cdiv(n, W) > c["SMAX"]:
        W = min((cdiv(n, c["SMAX"]) + 63) & ~63, wide_w(vt))
    ignored = 0
    if t2 == 1:
        w_env = int(env.get(PRE + "_W", 0))
        if c["w_hook_min"] <= w_env <= wcap(vt):
            W = w_env & ~63
        else:
            ignored = int(w_env != 0)
    S, ntile = cdiv(n, W), cdiv(nnz, c["TILE"])
    fits = m > 0 and 0 < nnz < INT32_MAX - c["TILE"] and S <= c["SMAX"] and ntile < INT32_MAX and S * ntile < INT32_MAX
    want = t2 == 1 or (t2 != 0 and nnz >= (c["want_nnz_shift"] << 20) and n >= c["want_n"])
    seg = 0
    if fits and want:
        seg = max(c["seg_min"], c["seg_mul"] * cdiv(nnz, S))
        if t2 == 1 and int(env.get(PRE + "_SEG", 0)) >= c["seg_hook_min"]:
            seg = int(env[PRE + "_SEG"])
    return {"path": "two_pass" if fits and want else "scatter",
            "why": None if fits and want else ("not_wanted" if not want else "does_not_fit"),
            "W": W, "S": S, "ntile": ntile, "seg": seg, "w_hook_ignored": ignored}


def max_items(g, nnz):
    return g["S"] + nnz // g["seg"] + 1


def t2_tile_of(b, ntile):
    per = ntile // 8
    return (b & 7) * per + (b >> 3) if b < per * 8 else b


def t2_slice(col, W, corrected=True):
    """col / W by the reciprocal rec = floor(2^32 / W), which under-estimates by at most one; in 32-bit unsigned arithmetic."""
    col = np.asarray(col, dtype=np.uint64)
    rec = (1 << 32) // W
    q = (col * np.uint64(rec)) >> np.uint64(32)
    if corrected:
        q = q + (((col - q * np.uint64(W)) & np.uint64(0xffffffff)) >= np.uint64(W))
    return q.astype(np.int64)


def coverage(lo, hi, vector_bound_off=0):
    """The workspace positions one work item reads, in the order of t2_accumulate_kernel's loops: 1 024 lanes, four consecutive
    entries per lane, two accesses 4 096 apart per round of the vector body, then the guarded tail.  Exactly [lo, hi), each once,
    when the loop is right."""
    e = lo + 4 * np.arange(1024, dtype=np.int64)
    four = np.arange(4, dtype=np.int64)
    out = []
    room = hi - (4096 + 4 - vector_bound_off) - e                      # a lane runs the vector body while room >= 0
    rounds = np.where(room >= 0, room // 8192 + 1, 0)
    for k in range(int(rounds.max(initial=0))):
        base = e[rounds > k] + 8192 * k
        out.append((base[:, None] + four).ravel())
        out.append((base[:, None] + 4096 + four).ravel())
    e = e + 8192 * rounds
    while (e < hi).any():
        p = (e[e < hi][:, None] + four).ravel()
        out.append(p[p < hi])
        e = e + 4096
    return np.concatenate(out) if out else np.zeros(0, np.int64)


MUTATIONS = ("no_segment_carry", "no_pair_carry", "first_row_wins", "r_lo_not_stepped_back", "raw_quotient",
             "empty_slice_without_item", "last_segment_not_clipped", "cut_slice_written_directly", "vector_bound_off_by_4",
             "tile_of_in_one_pass")


def plan_items(counts_per_slice, seg, mut=None):
    """[(slice, lo, hi, cut)] of t2_plan_kernel from the slices' shares (their runs lie back to back in slice order)."""
    items, off = [], 0
    for i, c in enumerate(counts_per_slice):
        c = int(c)
        t = (0 if mut == "empty_slice_without_item" else 1) if c == 0 else cdiv(c, seg)
        for q in range(t):
            lo = off + q * seg
            hi = lo + seg if mut == "last_segment_not_clipped" else min(lo + seg, off + c)
            items.append((i, lo, hi, int(t > 1)))
        off += c
    return items


def model(rowptr, colind, shape, values, x, alpha, beta, y0, g, mut=None, stats=None):
    """y = alpha A^T x + beta y0 (float64; y0 may hold NaN where beta = 0) the way the kernel chain computes it under the
    geometry g.  stats (a dict) receives n_items, the item list and every entry's place in the workspace."""
    c = constants()
    T = c["TILE"]
    m, n = shape
    nnz = colind.size
    W, S, ntile, seg = g["W"], g["S"], g["ntile"], g["seg"]
    rowptr = np.asarray(rowptr, np.int64)
    sl = t2_slice(colind, W, corrected=mut != "raw_quotient")
    tile_row = np.append(np.searchsorted(rowptr[:m], np.arange(ntile, dtype=np.int64) * T, "left"), m)
    # ---- t2_hist: workgroup b counts tile t2_tile_of(b) into counts[slice][tile]
    counts = np.zeros((S, ntile), np.int64)
    for b in range(ntile):
        t = t2_tile_of(b, ntile)
        counts[:, b if mut == "tile_of_in_one_pass" else t] = np.bincount(sl[t * T:min(t * T + T, nnz)], minlength=S)[:S]
    # ---- scan_counts_i32: exclusive, slice-major, the total behind the last
    offsets = np.concatenate([[0], np.cumsum(counts.ravel())])
    # ---- t2_plan: items; the cut slices' part of y scaled here
    share = offsets[(np.arange(S) + 1) * ntile] - offsets[np.arange(S) * ntile]
    items = plan_items(share, seg, mut)
    y = np.array(y0, dtype=np.float64, copy=True)
    for i in sorted({it[0] for it in items if it[3]}):
        c0, c1 = i * W, min(i * W + W, n)
        y[c0:c1] = 0.0 if beta == 0.0 else beta * y[c0:c1]
    # ---- t2_scatter: the row of every entry from marks + running maxima, products placed by the scanned counts
    prod = np.full(nnz + seg + 2 * T + 8, np.nan)       # (NaN behind the workspace: a read past a run shows)
    lcol = np.zeros(prod.size, np.int64)
    xpad = np.append(np.asarray(x, np.float64), np.nan)
    place = np.zeros(nnz, np.int64)
    for b in range(ntile):
        tile = t2_tile_of(b, ntile)
        e0, e1 = tile * T, min(tile * T + T, nnz)
        count = e1 - e0
        r_lo, r_hi = int(tile_row[tile]), min(int(tile_row[tile + 1]), m)
        if mut != "r_lo_not_stepped_back":
            r_lo = r_lo - 1 if r_lo > 0 else 0
        j = np.arange(1, r_hi - r_lo + 1, dtype=np.int64)
        pos = rowptr[r_lo + j] - e0
        ok = (pos >= 0) & (pos < count)
        mark = np.zeros(T, np.int64)
        if mut == "first_row_wins":
            first = np.full(T, np.iinfo(np.int64).max)
            np.minimum.at(first, pos[ok], j[ok])
            mark = np.where(first == np.iinfo(np.int64).max, 0, first)
        else:
            np.maximum.at(mark, pos[ok], j[ok])
        inc = np.maximum.accumulate(mark.reshape(T // 64, 64), axis=1)      # inside the wavefronts
        ends = inc[:, 63]
        a, bb = ends[0::2], ends[1::2]                                      # the last wavefront: two segment ends per lane
        incl = np.maximum.accumulate(np.maximum(a, bb))
        exc = np.concatenate([[0], incl[:-1]])
        pre = np.zeros(T // 64, np.int64)
        pre[0::2] = exc
        pre[1::2] = exc if mut == "no_pair_carry" else np.maximum(exc, a)
        if mut == "no_segment_carry":
            pre[:] = 0
        rrow = np.maximum(inc, pre[:, None]).ravel()[:count]
        xv = xpad[np.minimum(r_lo + rrow, m)]
        s = sl[e0:e1]
        order = np.argsort(s, kind="stable")
        piece = np.bincount(s, minlength=S)
        rank = np.empty(count, np.int64)
        rank[order] = np.arange(count) - np.repeat(np.concatenate([[0], np.cumsum(piece)[:-1]]), piece)
        at = offsets[s * ntile + tile] + rank
        place[e0:e1] = at
        prod[at] = alpha * np.asarray(values[e0:e1], np.float64) * xv
        lcol[at] = (colind[e0:e1].astype(np.int64) - s * W) & 0xffff
    # ---- t2_accumulate
    for (i, lo, hi, cut) in items:
        c0, c1 = i * W, min(i * W + W, n)
        if hi - lo <= 4096 and mut != "vector_bound_off_by_4":                 # (the tail alone: [lo, hi) in order)
            at = np.arange(lo, hi)
        else:
            at = coverage(lo, hi, 4 if mut == "vector_bound_off_by_4" else 0)
        acc = np.bincount(lcol[at], weights=prod[at], minlength=W)[:c1 - c0] if at.size else np.zeros(c1 - c0)
        if cut and mut != "cut_slice_written_directly":
            nz = acc != 0
            y[c0:c1][nz] += acc[nz]
        else:
            y[c0:c1] = acc if beta == 0.0 else acc + beta * y[c0:c1]
    if stats is not None:
        stats.update(n_items=len(items), items=items, place=place, tile_row=tile_row, share=share)
    return y


# ------------------------------------------------------------------------------------------------------------------ families
class Fam:
    def __init__(self, name, rowptr, colind, n, W=None, seg=None, only=None, note=""):
        self.name, self.note, self.only = name, note, only        # only: the one value type the family is built for
        self.rowptr = np.asarray(rowptr, np.int64)
        self.colind = np.asarray(colind, np.int64).astype(np.int32)
        self.shape = (self.rowptr.size - 1, int(n))
        self.nnz = int(self.rowptr[-1])
        self.W, self.seg = W, seg
        assert self.rowptr[0] == 0 and self.colind.size == self.nnz and (np.diff(self.rowptr) >= 0).all()
        assert self.nnz == 0 or (0 <= self.colind.min() and self.colind.max() < n)
        self.distinct = np.unique(self.colind).size == self.nnz

    def env(self, t2="1"):
        e = {PRE: t2}
        if self.W is not None:
            e[PRE + "_W"] = str(self.W)
        if self.seg is not None:
            e[PRE + "_SEG"] = str(self.seg)
        return e

    def geometry(self, vt, cus):
        return geometry(vt, self.shape, self.nnz, self.env(), cus)

    def probe(self):
        """The family the row probe runs on: this one when no column repeats, else the same rows with distinct columns spread
        over all slices of an n widened to nnz (and slices widened until SMAX of them hold n)."""
        if self.distinct:
            return self
        n = max(self.shape[1], self.nnz)
        W = max(self.W or constants()["w_min"], (cdiv(n, constants()["SMAX"]) + 63) & ~63)
        return Fam(self.name + "/probe", self.rowptr, spread(self.nnz, n), n, W=W, seg=self.seg)


def spread(count, n):
    """`count` columns in [0, n), distinct when n >= count, neighbours far apart: e -> e * g mod n with g coprime to n."""
    if n == 1:
        return np.zeros(count, np.int64)
    g = int(n * 0.6180339887) | 1
    while math.gcd(g, n) != 1:
        g += 2
    return (np.arange(count, dtype=np.int64) * g) % n


def shuffle(a):
    """A fixed permutation of a (the stride walk of spread): entries of one slice end up in every tile."""
    a = np.asarray(a)
    return a[spread(a.size, a.size)] if a.size > 1 else a


ROW_PATTERN = (3, 0, 1, 17, 64, 2, 129, 0, 0, 5, 63, 65, 1, 1, 700)


def rows_cyc(nnz, pattern=ROW_PATTERN):
    """rowptr of rows whose lengths cycle through `pattern` until nnz entries are placed."""
    reps = nnz // max(1, sum(pattern)) + 2
    ends = np.cumsum(np.tile(np.asarray(pattern, np.int64), reps))
    ends = ends[:np.searchsorted(ends, nnz, "left")]
    return np.concatenate([[0], ends[ends < nnz], [nnz]])


def rows_from_starts(starts, nnz):
    """rowptr of the rows that start at the given entry positions (a position given k + 1 times: k empty rows before the row
    that owns the entry); a row starts at 0 in any case."""
    s = np.sort(np.asarray(list(starts), np.int64))
    if s.size == 0 or s[0] != 0:
        s = np.concatenate([[0], s])
    return np.concatenate([s, [nnz]])


def _fams():
    c = constants()
    T = c["TILE"]
    F = {}

    def add(name, rowptr, colind, n, **kw):
        assert name not in F, name
        F[name] = Fam(name, rowptr, colind, n, **kw)

    def rows_family(name, rowptr, W=4096):
        nnz = int(rowptr[-1])
        n = max(nnz, 2 * W + 1)
        add(name, rowptr, spread(nnz, n), n, W=W)

    # ---- tiles and the XCD mapping
    for nnz in (1, 2, 63, 64, 65, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1):
        rows_family(f"tiles_nnz_{nnz}", rows_cyc(nnz))
    for nt in (7, 8, 9, 15, 16, 17):
        rows_family(f"tiles_{nt}_full", rows_cyc(nt * T))
        rows_family(f"tiles_{nt}_partial", rows_cyc(nt * T - 37))
    # ---- row starts inside a tile (the second of three, so that the row before the tile's first start reaches in)
    named = (0, 1, 62, 63, 64, 65, 127, 128, 1023, 1024, 1025, T - 65, T - 64, T - 1)
    rows_family("starts_named", rows_from_starts([T + p for p in named], 3 * T))
    for p in named:
        rows_family(f"starts_only_{p}", rows_from_starts([5, T + p], 2 * T + 11))
    rows_family("starts_lane0", rows_from_starts([T + 64 * k for k in range(128)], 3 * T))
    rows_family("starts_lane63", rows_from_starts([T + 64 * k + 63 for k in range(128)], 3 * T))
    rows_family("starts_even_segments", rows_from_starts([T + 64 * k + 17 for k in range(0, 128, 2)], 3 * T))
    rows_family("starts_odd_segments", rows_from_starts([T + 64 * k + 40 for k in range(1, 128, 2)], 3 * T))
    rows_family("starts_segment_0", rows_from_starts([T + 5, T + 40], 3 * T))
    rows_family("starts_segment_127", rows_from_starts([T + 127 * 64 + 3, T + 127 * 64 + 60], 3 * T))
    rows_family("starts_stretch_2048", rows_from_starts([T + 150, T + 150 + 2300, T + 7000], 3 * T))
    rows_family("rows_of_length_1", np.arange(2 * T + 101, dtype=np.int64))
    rows_family("row_is_one_tile", np.array([0, T, 2 * T, 2 * T + 5]))
    rows_family("row_spans_three_tiles", np.array([0, T - 10, 3 * T + 10, 3 * T + 500]))
    rows_family("row_ends_on_last_position", np.array([0, 5, T, T + 7, 2 * T, 2 * T + 1, 3 * T, 3 * T + 9]))
    rows_family("one_row", np.array([0, T + 3]))
    rows_family("last_of_100000_rows", np.concatenate([np.zeros(100000, np.int64), [70]]))
    # ---- empty rows sharing one start position
    for k in (1, 2, 1023, 1024, 1025, 5000):
        places = {"tile_position_0": (T, 3 * T), "mid_wavefront": (T + 1000 + 37, 3 * T), "tile_last_position": (2 * T - 1, 3 * T),
                  "tile_end": (2 * T, 2 * T + 5), "before_first_entry": (0, T + 9), "behind_last_entry": (2 * T, 2 * T)}
        for where, (p, nnz) in places.items():
            if p == 0:              # k empty rows, then the row that owns entry 0
                rp = rows_from_starts([0] * (k + 1) + [3, 200], nnz)
            elif p == nnz:          # k rows that start (and end) behind the last entry
                rp = np.concatenate([rows_from_starts([3, 200, T + 1], nnz), np.full(k, nnz, np.int64)])
            else:                   # ... then the row that owns entry p
                rp = rows_from_starts([3, 200, p - 50] + [p] * (k + 1), nnz)
            rows_family(f"empty_{k}_{where}", rp)

    # ---- slices: entries on the slice edges, columns 0, W - 1, W, W + 1, ..., n - 1
    def edge_columns(W, S, n):
        ks = np.arange(S + 1, dtype=np.int64) * W
        cols = np.unique(np.concatenate([ks - 1, ks, ks + 1, [0, n - 1]]))
        return shuffle(cols[(cols >= 0) & (cols < n)])

    def slices_family(name, W, S, n, **kw):
        cols = edge_columns(W, S, n)
        add(name, rows_cyc(cols.size, (2, 0, 1, 5, 3)), cols, n, W=W, **kw)

    for S in (1, 2, 3, 63, 64, 65, 959, 960, 961, 1023, 1024):
        slices_family(f"slices_W64_S{S}", 64, S, 64 * S)
        slices_family(f"slices_W64_S{S}_last_of_1", 64, S, 64 * (S - 1) + 1)
    for W in (128, 192, 320, 4096, 9728, 19456):
        for S in (1, 3, 65):
            slices_family(f"slices_W{W}_S{S}", W, S, W * S)       # (W = 19456: fp32 only; fp64 must report the hook ignored)
            slices_family(f"slices_W{W}_S{S}_last_of_1", W, S, W * (S - 1) + 1)
    add("slices_n_1", rows_cyc(300), np.zeros(300, np.int64), 1, W=64)
    add("slices_n_below_W", rows_cyc(1000), spread(1000, 1000), 1000, W=4096)
    for W in (64, 192):      # only the first and the last slice hold entries
        cols = np.concatenate([np.arange(0, W, 3), np.arange(64 * W, 65 * W, 5)])
        add(f"slices_empty_between_W{W}", rows_cyc(cols.size, (2, 0, 1, 5, 3)), shuffle(cols), 65 * W, W=W)
    slices_family("slices_1025_falls_back", 64, 1025, 64 * 1025)
    for vt in ("f32", "f64"):           # the widest default geometry: no _T2_W hook
        Ww = wide_w(vt)
        slices_family(f"widest_{vt}", Ww, c["SMAX"], c["SMAX"] * Ww, only=vt)
        F[f"widest_{vt}"].W = None
        slices_family(f"widest_{vt}_plus_1", Ww, c["SMAX"], c["SMAX"] * Ww + 1, only=vt)
        F[f"widest_{vt}_plus_1"].W = None

    # ---- segments and items: slice shares side by side
    def shares_family(name, shares, W, seg, n=None, mix=True, **kw):
        S = len(shares)
        n = S * W if n is None else n
        cols = np.concatenate([i * W + np.arange(sh, dtype=np.int64) % min(W, n - i * W) for i, sh in enumerate(shares)])
        cols = shuffle(cols) if mix else cols
        add(name, rows_cyc(cols.size), cols, n, W=W, seg=seg, **kw)

    for seg in (64, 100, 4096, 8192):
        shares_family(f"shares_seg{seg}", [0, 1, seg - 1, seg, seg + 1, 2 * seg - 1, 2 * seg, 2 * seg + 1, 10 * seg + 3], 4096, seg)
    dseg = c["seg_min"]      # the default segment of a small matrix
    shares_family("shares_default_seg", [0, 1, dseg - 1, dseg + 1, 0, 0, 0, 0], 4096, None)
    shares_family("shares_default_seg_exact", [dseg, 3, dseg // 2, 0, 0, 0, 0, 0], 4096, None)
    shares_family("all_1024_slices_cut", [65] * 1024, 64, 64)
    shares_family("worst_case_item_count", [(i % 3) * 64 + 1 for i in range(1024)], 64, 64)
    shares_family("cut_slice_is_narrow_last", [10, 70, 200], 4096, 64, n=2 * 4096 + 10)
    # ---- item lengths of the accumulate loop, every lo mod 4
    lengths = (1, 2, 3, 4, 5, 4095, 4096, 4097, 4099, 4100, 4101, 8191, 8192, 8193, 8196, 12292, 16383, 16384, 16385)

    def padded(first, runs):
        """Shares: `first`, then the runs (tuples of shares kept together) with a filler share before each that brings the
        run's start back to first mod 4."""
        out, pos = [first], first
        for run in runs:
            pad = (first - pos) % 4 or 4
            out.append(pad)
            out.extend(run)
            pos += pad + sum(run)
        return out

    for r in range(4):
        shares_family(f"item_lengths_uncut_lo{r}", padded(r or 4, [(L,) for L in lengths]), 9728, 32768, note=f"lo mod 4 = {r}")
        for tag, group, seg in (("1_5", lengths[:5], 64), ("4096", lengths[5:11], 4104), ("8192", lengths[11:16], 12292),
                                ("16384", lengths[16:], 16388)):
            shares_family(f"item_lengths_last_segment_{tag}_lo{r}", padded(r or 4, [(seg + L,) for L in group]), 9728, seg,
                          note=f"lo mod 4 = {r} (seg = {seg} is a multiple of 4)")
    T_ = T
    cols = np.concatenate([np.full(T_, 7, np.int64), spread(T_, 9728), 9728 + spread(300, 9728)])
    add("segment_in_one_column", rows_cyc(cols.size), cols, 2 * 9728, W=9728, seg=8192)
    # ---- scan edges: S * ntile on the block edges of scan_counts_i32
    for S, nt in ((89, 23), (64, 32), (683, 3), (64, 64), (241, 17)):
        nnz = nt * T - 1000
        add(f"scan_{S}x{nt}", rows_cyc(nnz), spread(nnz, 64 * S), 64 * S, W=64)
    # ---- state between calls on one handle: 17 tiles x 1 024 slices (most of them cut), then 1 tile x 1 slice
    add("state_17x1024", rows_cyc(17 * T - 37), spread(17 * T - 37, 64 * 1024), 64 * 1024, W=64, seg=64)
    add("state_1x1", rows_cyc(100), spread(100, 50), 50, W=64, seg=64)
    return F


_FAMILIES = {}


def families():
    """{name: Fam}, built once."""
    if not _FAMILIES:
        _FAMILIES.update(_fams())
    return _FAMILIES


def is_wide(fam):
    return fam.name.startswith("widest_")


# ----------------------------------------------------------------------------------------------------------------- data sets
LIMIT = 2 ** 24


def y_start(n):
    """The y a beta != 0 call starts from: small even integers, none of them 0 (beta * y0 stays an integer for beta = 0.5)."""
    v = 2.0 * (1 + np.arange(n, dtype=np.int64) % 3)
    return np.where((np.arange(n) // 3) % 2 == 0, v, -v)


def data(fam, kind):
    """(values, x) of the data set `kind` in float64 (numbers fp32 holds exactly); the probe set belongs to fam.probe()."""
    m = fam.shape[0]
    rng = np.random.default_rng(77)
    if kind == "probe":
        assert fam.distinct and fam.shape[1] >= fam.nnz
        return np.ones(fam.nnz), 1.0 + np.arange(m) % 251
    if kind == "ints":
        return rng.integers(-2, 3, fam.nnz).astype(np.float64), rng.integers(-3, 4, m).astype(np.float64)
    assert kind == "random"
    return rng.uniform(-1, 1, fam.nnz).astype(np.float32).astype(np.float64), \
        rng.uniform(-1, 1, m).astype(np.float32).astype(np.float64)


def cases(fam):
    """[(data set, the family it runs on)]: ints and random on the family, the probe on fam.probe()."""
    return [("ints", fam), ("probe", fam.probe()), ("random", fam)]


_HOST = {}


def host_data(fam, kind):
    """(values, x, A^T x, |A|^T |x|, entries per column) in float64 from scipy, never through the library; computed once per
    family and data set, shared by every case and never written to."""
    key = (fam.name, kind)
    if key not in _HOST:
        if fam.shape[1] > 10_000_000:        # the widest geometry: its vectors of n take 320 MB each; keep one family's
            for k_ in [k_ for k_ in _HOST if k_[0].startswith("widest_")]:
                del _HOST[k_]
        values, x = data(fam, kind)
        A = sps.csr_matrix((values, fam.colind, fam.rowptr), shape=fam.shape)
        Aabs = sps.csr_matrix((np.abs(values), fam.colind, fam.rowptr), shape=fam.shape)
        out = (values, x, A.T @ x, Aabs.T @ np.abs(x), np.bincount(fam.colind, minlength=fam.shape[1]))
        for a_ in out:
            a_.setflags(write=False)
        _HOST[key] = out
    return _HOST[key]


def reference(fam, kind, alpha, beta, y0):
    """(alpha A^T x + beta y0, the sum of the terms' magnitudes) in float64; beta = 0 does not read y0.  The exact sets are
    asserted to stay in the range where every partial sum is exact in fp32."""
    _, _, atx, absatx, _ = host_data(fam, kind)
    ref = alpha * atx + (beta * y0 if beta != 0.0 else 0.0)
    mag = abs(alpha) * absatx + (abs(beta) * np.abs(y0) if beta != 0.0 else 0.0)
    if kind != "random":
        assert_exact_range(mag)
    return ref + 0.0, mag


def row_map(fam):
    """What the probe set must give for alpha = 1, beta = 0: 1 + (row of the entry in column c) mod 251, 0 for an empty column."""
    want = np.zeros(fam.shape[1])
    want[fam.colind] = 1.0 + np.repeat(np.arange(fam.shape[0]), np.diff(fam.rowptr)) % 251
    return want


def assert_exact_range(mag):
    """Every partial sum of every element, in any order, is an integer (or half of one) below 2^24: exact in fp32."""
    assert float(np.max(mag, initial=0.0)) < LIMIT, "the exact data set leaves the range in which fp32 sums are exact"


def derived(fam, g):
    """What a family holds, from the restated geometry: the sets the CPU tests assert."""
    T = constants()["TILE"]
    sl = t2_slice(fam.colind, g["W"])
    share = np.bincount(sl, minlength=g["S"])
    items = plan_items(share, g["seg"])
    starts = np.unique(fam.rowptr[:-1][np.diff(fam.rowptr) > 0]) % T
    return {"item_lengths": {hi - lo for _, lo, hi, _ in items}, "lo_mod_4": {lo % 4 for _, lo, hi, _ in items if hi > lo},
            "cut": {cut for *_, cut in items}, "n_items": len(items), "shares": set(share.tolist()),
            "start_mod_64": set((starts % 64).tolist()), "start_mod_1024": set((starts % 1024).tolist()),
            "start_positions": set(starts.tolist()), "items": items}
