"""Deterministic column ladders for the block triangular solve of csrc/sptrsm.hip (trsm_solve_typed / trsm_row), next to
tests/ladder_tt.py and in its style: tests/test_gpu_trsm_ladders.py runs them on the device, tests/test_ladders_trsm_cpu.py
proves on the host that the rung lists hold what they claim and that a wrong kernel would be seen.  Nothing here needs a GPU.

limits()      every constant the geometry depends on, READ from the sources (a pattern that no longer matches fails with
              the name of this file).
geometry()    what trsm_solve_typed decides -- path, mis, units, logC, E, b_piece, x_bytes, passes of the unit loop --
              restated from the definitions in the file's head comment: what spblas_gfx950_sptrsm_last must report.  The GPU
              tests compare the two BEFORE they look at X.
model_solve() a host model of trsm_row in the value type: the team of E x C lanes, units of V columns that start at
              u V - mis, whole and partial units, entry p on entry lane (p - p0) mod E, the xor tree over the entry lanes with
              the diagonal travelling along ("the last stored wins"), lane e = 0 subtracting and dividing, the unit loop in
              passes of C.  `mutation` breaks it in one named way; the CPU tests show that each mutation fails a named rung.
              The GPU tests do NOT compare against the model: they compare against x_true * f_j.

EXACT DATA.  The systems are ladder_tt.trsv_system's (or dense_system's, same data rules): x_true in {+-1, +-2, +-3}, strict
entries in {+-1, +-2}, diagonals and alpha powers of two.  Column j of B is b * f_j with f_j = (-1)^j (j + 1), j < MAX_COLS:
pairwise different, so a swapped or shifted column is seen; an integer, so no power of two is needed.  block_rhs asserts this
module's own condition: max |f_j| times the largest sum of |products| of a row stays below 2^22, so every partial sum in any
order is an integer fp32 holds, alpha * dot and b - alpha * dot are multiples of 1/4 below 2^24, and the division is exact:
X must EQUAL x_true * f_j under any (E, C), any unit split and any path.

WINDOWS.  B and X are windows of wider 1-D tensors (window(), after test_gpu_sptrsm.py::_window) whose every element holds a
NaN bit pattern; the shifts of B and X are chosen independently, so that B's pieces are aligned like X's or not.
"""
import re

import numpy as np

import ladder_tt as T
import trsm_util as TU

MAX_COLS = 160
NAN_BITS = {4: 0x7FC12345, 8: 0x7FF8123456789ABC}
UINT_OF = {4: np.uint32, 8: np.uint64}


# ------------------------------------------------------------------------------------------------------------------ limits
def _get(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the source no longer has the expected form; update tests/ladder_trsm.py"
    return [int(g, 0) for g in m.groups()]


_LIMITS = None


def limits():
    """Every size csrc/sptrsm.hip's geometry depends on."""
    global _LIMITS
    if _LIMITS is not None:
        return dict(_LIMITS)
    src = T._src("sptrsm.hip")
    flat = re.sub(r"\s+", " ", src)
    t = {}
    t["max_c"], = _get(r"#define TRSM_MAX_C (\d+)", src, "TRSM_MAX_C")
    t["chain_threads"], = _get(r"#define TRSM_CHAIN_THREADS (\d+)", src, "TRSM_CHAIN_THREADS")
    t["wave"], = _get(r"#define SPB_WAVE (\d+)", T._src("common.hpp"), "SPB_WAVE")
    pieces = [int(g) for g in re.findall(r"constexpr int V = (\d+) / \(int\) sizeof\(T\);", src)]
    assert len(pieces) == 2 and len(set(pieces)) == 1, \
        "the 16-byte piece: the source no longer has the expected form; update tests/ladder_trsm.py"
    t["piece"] = pieces[0]
    a = _get(r"const bool vec = xcs == 1 && \(xrs \* \(int64_t\) sizeof\(T\)\) % (\d+) == 0 && xaddr % sizeof\(T\) == 0 && "
             r"n >= V && x_span <= \(int64_t\) (0x[0-9A-Fa-f]+)u;", flat, "the rule of the 16-byte pieces")
    t["reach"] = a[1]
    b = _get(r"a\.mis = vec \? \(int\) \(\(xaddr % (\d+)\) / sizeof\(T\)\) : 0;", flat, "the misalignment")
    c = _get(r"a\.b_piece = vec && bcs == 1 && \(brs \* \(int64_t\) sizeof\(T\)\) % (\d+) == 0 && baddr % (\d+) == xaddr % (\d+);",
             flat, "the rule of B's pieces")
    assert {a[0], b[0], *c} == {t["piece"]}, "piece sizes disagree; update tests/ladder_trsm.py"
    _get(r"while \(\(1 << logC\) < a\.units && \(1 << logC\) < TRSM_MAX_C\) \+\+logC;", flat, "the unit lanes of a team")
    _get(r"a\.E = pl->lanes < \(SPB_WAVE >> logC\) \? pl->lanes : \(SPB_WAVE >> logC\);", flat, "the entry lanes of a team")
    _get(r"a\.units = \(int\) cdiv\(n \+ a\.mis, V\);", flat, "the units of a row")
    _get(r"const int64_t x_span = \(\(pl->m - 1\) \* xrs \+ n\) \* \(int64_t\) sizeof\(T\);", flat, "the span of X")
    lv = _get(r"__launch_bounds__\((\d+)\) void trsm_level_kernel\(int f0, int f1, trsm_args<T> a\) \{ const int team = a\.E << "
              r"a\.logC; const int idx = f0 \+ \(int\) blockIdx\.x \* \((\d+) / team\) \+ \(int\) threadIdx\.x / team;", flat,
              "the level kernel")
    lv += _get(r"dim3\(\(unsigned\) cdiv\(f1 - f0, (\d+) / team\)\), dim3\((\d+)\), 0, s, f0, f1, a\)", flat,
               "the launch of the level kernel")
    assert len(set(lv)) == 1, "the level kernel's workgroup sizes disagree; update tests/ladder_trsm.py"
    t["level_threads"] = lv[0]
    _get(r"idx < f1; idx \+= TRSM_CHAIN_THREADS / team\)", flat, "the chain kernel's row loop")
    _get(r"if \(n == 1 && \(m == 1 \|\| \(brs == 1 && xrs == 1\)\)\)", flat, "the forward to the vector solve")
    _LIMITS = t
    return dict(t)


def V_of(itemsize):
    return limits()["piece"] // itemsize


# ---------------------------------------------------------------------------------------------------------------- geometry
def _cdiv(a, b):
    return -(-a // b)


def geometry(m, n, itemsize, lanes, xaddr, xrs, xcs, baddr, brs, bcs):
    """What spblas_gfx950_sptrsm_last must report after a solve with these operands (strides in elements, as the C ABI gets
    them), from the definitions: X is read in 16-byte pieces if it is layout_right with rows a multiple of 16 bytes apart,
    an element-aligned base, at least one whole unit of columns and all of it within reach of one buffer descriptor; `mis` is
    the pointer's distance to the 16-byte boundary below it, in elements; a row is cut into ceil((n + mis) / V) units; a team
    has C = the least power of two >= min(units, TRSM_MAX_C) unit lanes and E = min(lanes per row, wave / C) entry lanes."""
    t = limits()
    if n == 1 and (m == 1 or (brs == 1 and xrs == 1)):
        return dict(path=1, mis=0, units=0, logC=0, E=0, b_piece=0, x_bytes=0, passes=0)
    piece, V = t["piece"], t["piece"] // itemsize
    span = ((m - 1) * xrs + n) * itemsize
    vec = xcs == 1 and (xrs * itemsize) % piece == 0 and xaddr % itemsize == 0 and n >= V and span <= t["reach"]
    mis = (xaddr % piece) // itemsize if vec else 0
    units = _cdiv(n + mis, V)
    C = 1
    while C < units and C < t["max_c"]:
        C *= 2
    b_piece = vec and bcs == 1 and (brs * itemsize) % piece == 0 and baddr % piece == xaddr % piece
    return dict(path=3 if vec else 2, mis=mis, units=units, logC=C.bit_length() - 1, E=min(lanes, t["wave"] // C),
                b_piece=int(b_piece), x_bytes=span if vec else 0, passes=_cdiv(units, C))


def partial_widths(n, mis, itemsize):
    """(columns of the partial unit in front, columns of the partial unit behind) of a row of n columns whose first whole unit
    starts at column (V - mis) % V; a row inside ONE partial unit reports it as the front one."""
    V = V_of(itemsize)
    front = min((V - mis) % V, n)
    back = (n - front) % V
    return front, back


def abi_strides(layout, ld, n):
    """(row stride, column stride) the C ABI receives for an (m, n) window, m > 1, of leading dimension ld: a column-major
    single column is a contiguous vector."""
    if layout == "R":
        return ld, 1
    return (1, 1) if n == 1 else (1, ld)


# ------------------------------------------------------------------------------------------------------------- exact data
def factors(n):
    """f_j = (-1)^j (j + 1), j < n."""
    assert 0 <= n <= MAX_COLS
    j = np.arange(n)
    return np.where(j % 2 == 0, 1.0, -1.0) * (j + 1)


def sum_of_products(sysm):
    """The largest sum over a row of |a x_true| over the strict entries the solve reads."""
    rows = np.repeat(np.arange(sysm.m), np.diff(sysm.rowptr))
    st = sysm.kind == 1
    return float(np.bincount(rows[st], weights=np.abs(sysm.exact_values[st] * sysm.x_true[sysm.colind[st]]),
                             minlength=sysm.m).max(initial=0.0))


def block_rhs(sysm, n):
    """B (m x n, float64) = b f_j by column; asserts the module's condition for exactness."""
    f = factors(n)
    worst = sum_of_products(sysm) * (np.abs(f).max() if n else 0.0)
    assert worst < 2 ** 22, f"sum of |products| {worst} leaves the exact range"
    B = sysm.b[:, None] * f[None, :]
    assert np.array_equal(B * 4, np.round(B * 4)) and np.abs(B).max(initial=0.0) < 2 ** 22
    return B


def block_x(sysm, n):
    """X the solve must return: x_true f_j by column (float64; every element is an integer below 2^10)."""
    return sysm.x_true[:, None] * factors(n)[None, :]


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT_OF[a.dtype.itemsize])


def exact_violations(X, sysm):
    """Messages (empty: passes): X (m x n, the value type) must equal x_true f_j bit for bit."""
    X = np.asarray(X)
    want = block_x(sysm, X.shape[1]).astype(X.dtype)
    bad = np.argwhere(_u(X) != _u(want))
    if not bad.size:
        return []
    r, c = (int(v) for v in bad[0])
    return [f"{bad.shape[0]} elements differ from x_true f_j, first at row {r}, column {c} (level {sysm.level[r]}, shape "
            f"{sysm.shape_of[r]}): {X[r, c]} != {want[r, c]}; columns off: {sorted(set(bad[:, 1].tolist()))[:12]}"]


def dense_system(m, upper, seed=0, alpha=1.0):
    """A full triangle of m rows (m levels of one row: one single-workgroup launch) under ladder_tt's data rules, as a
    ladder_tt.System.  Lower: the last row gathers every other row of X and stores furthest; upper: row 0 gathers the last row."""
    rng = np.random.default_rng(5000 + seed)
    rows = np.repeat(np.arange(m), np.arange(1, m + 1))
    cols = np.concatenate([np.arange(r + 1) for r in range(m)])
    if upper:
        rows, cols = m - 1 - rows[::-1], m - 1 - cols[::-1]
    s = T.System()
    s.m, s.nnz, s.upper, s.unit, s.alpha = m, int(rows.size), upper, False, float(alpha)
    s.lanes = T.lanes_of(s.nnz, m)
    s.rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    s.colind = cols.astype(np.int32)
    s.kind = np.where(cols == rows, 2, 1)
    s.exact_values = np.where(cols == rows, rng.choice([0.5, 1.0, 2.0, 4.0], rows.size), rng.choice([-2.0, -1.0, 1.0, 2.0], rows.size))
    s.x_true = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], m)
    s.level = (m - 1 - np.arange(m)) if upper else np.arange(m)
    s.widths = [1] * m
    s.shape_of = np.array([f"s{k}_dlast" for k in s.level], dtype=object)
    s.b = alpha * np.bincount(rows, weights=s.exact_values * s.x_true[cols], minlength=m)
    assert np.array_equal(s.b * 4, np.round(s.b * 4))
    assert np.array_equal(T.levels_of(s.rowptr, s.colind, m, upper), s.level)
    return s


# --------------------------------------------------------------------------------------------------------------- the model
MUTATIONS = ("tree_stride", "lo_plus_mis", "drop_last_partial")


def model_solve(sysm, B, dtype, geo, mutation=None, stats=None):
    """trsm_row for every row, in the value type: B (m x n) -> X (m x n).  geo = geometry(...) of the call (mis, units, logC,
    E and the path: 3 = whole units are pieces).  stats (a dict) receives the number of whole and partial units stored and the
    widths of the partial ones.  mutation: None, or one of MUTATIONS --
      tree_stride        the xor tree strides by o instead of o << logC (partners in the wrong lanes);
      lo_plus_mis        a unit starts at u V + mis instead of u V - mis;
      drop_last_partial  the partial unit behind the last whole one is never stored."""
    assert mutation is None or mutation in MUTATIONS
    with np.errstate(all="ignore"):          # (a mutated model reads X it has not solved yet: NaN, as the device would)
        return _model_solve(sysm, B, dtype, geo, mutation, stats)


def _model_solve(sysm, B, dtype, geo, mutation, stats):
    dtype = np.dtype(dtype).type
    m, n = B.shape
    V = V_of(np.dtype(dtype).itemsize)
    mis, units, logC, E, vec = geo["mis"], geo["units"], geo["logC"], geo["E"], geo["path"] == 3
    C = 1 << logC
    rp, ci = sysm.rowptr.astype(np.int64), sysm.colind.astype(np.int64)
    vals = sysm.exact_values.astype(dtype)
    alpha = dtype(sysm.alpha)
    Bt = np.asarray(B).astype(dtype)
    X = np.full((m, n), np.nan, dtype)
    cl = np.arange(C)
    k = np.arange(V)
    lane = np.arange(E * C)                      # t = (e << logC) | cl
    if stats is not None:
        stats.update(whole=0, partial=0, widths=set(), passes=0)
    for r in (range(m - 1, -1, -1) if sysm.upper else range(m)):
        p0, p1 = int(rp[r]), int(rp[r + 1])
        for u0 in range(0, units, C):
            u = u0 + cl
            lo = u * V + mis if mutation == "lo_plus_mis" else u * V - mis
            j0 = np.maximum(lo, 0)
            j1 = np.where(u < units, np.minimum(lo + V, n), j0)
            j1 = np.maximum(j1, j0)
            if mutation == "drop_last_partial":
                last = (u == units - 1) & (j1 - j0 < V) & (u > 0)
                j1 = np.where(last, j0, j1)
            cols = lo[:, None] + k[None, :]                                   # (C, V)
            live = (cols >= j0[:, None]) & (cols < j1[:, None])
            safe = np.where(live, cols, 0)
            acc = np.zeros((E, C, V), dtype)
            dpos = np.full(E, -1, np.int64)
            dval = np.zeros(E, dtype)
            for q0 in range(p0, p1, E):                                       # lane e takes entries p0 + e, p0 + e + E, ...
                p = np.arange(q0, min(q0 + E, p1))
                e = p - q0
                c, av = ci[p], vals[p]
                strict = (c >= 0) & (c < m) & ((c > r) if sysm.upper else (c < r))
                if strict.any():
                    xs = X[c[strict]][:, safe]                                # (entries, C, V)
                    prod = av[strict][:, None, None] * xs
                    acc[e[strict]] += np.where(live[None], prod, dtype(0))
                d = ~strict & (c == r)
                dpos[e[d]], dval[e[d]] = p[d], av[d]                          # the last stored diagonal entry wins
            acc = acc.reshape(E * C, V)
            dpos, dval = np.repeat(dpos, C), np.repeat(dval, C)
            o = E >> 1
            while o:
                partner = lane ^ (o if mutation == "tree_stride" else o << logC)
                acc = acc + acc[partner]
                other, oval = dpos[partner], dval[partner]
                take = other > dpos
                dpos, dval = np.where(take, other, dpos), np.where(take, oval, dval)
                o >>= 1
            # entry lane 0 of every unit lane: t = cl
            bv = np.where(live, Bt[r][safe], dtype(0))
            xv = bv - alpha * acc[:C]
            if not sysm.unit:
                xv = xv / (alpha * np.where(dpos[:C] >= 0, dval[:C], dtype(0)))[:, None]
            X[r, cols[live]] = xv[live]
            if stats is not None:
                w = (j1 - j0)[j1 > j0]
                whole = vec & (w == V)
                stats["whole"] += int(whole.sum())
                stats["partial"] += int((~whole).sum())
                stats["widths"] |= set(w[~whole].tolist())
                stats["passes"] += 1
    return X


def independent_geometry(m, n, itemsize, lanes, xaddr, xrs, xcs, baddr, brs, bcs):
    """A second restatement of geometry(), written from the kernel's side: the columns are walked one by one, every column is
    given the 16-byte slot its ADDRESS falls into, and the units, the team and the passes are counted from that."""
    t = limits()
    if n == 1 and (m == 1 or (brs, xrs) == (1, 1)):
        return dict(path=1, mis=0, units=0, logC=0, E=0, b_piece=0, x_bytes=0, passes=0)
    per_piece = t["piece"] // itemsize
    last_byte = xaddr + ((m - 1) * xrs + (n - 1) * xcs) * itemsize + itemsize        # one past X's last element
    rows_aligned = all(((r * xrs) * itemsize) % t["piece"] == 0 for r in range(min(m, 3)))
    pieces = xcs == 1 and rows_aligned and xaddr % itemsize == 0 and n >= per_piece and last_byte - xaddr <= t["reach"]
    if pieces:
        slots = sorted({(xaddr + j * itemsize) // t["piece"] for j in range(n)})          # 16-byte slots row 0 touches
        mis = (xaddr - slots[0] * t["piece"]) // itemsize
    else:
        slots = sorted({j // per_piece for j in range(n)})
        mis = 0
    units = len(slots)
    logC = 0
    while 2 ** logC < min(units, t["max_c"]):
        logC += 1
    E = lanes
    while E * 2 ** logC > t["wave"]:
        E //= 2
    passes = len(range(0, units, 2 ** logC))
    b_same = pieces and bcs == 1 and all(((baddr + r * brs * itemsize) - (xaddr + r * xrs * itemsize)) % t["piece"] == 0
                                         for r in range(min(m, 3)))
    return dict(path=3 if pieces else 2, mis=mis, units=units, logC=logC, E=E, b_piece=int(b_same),
                x_bytes=last_byte - xaddr if pieces else 0, passes=passes)


# ---------------------------------------------------------------------------------------------------------------- windows
def poisoned(numel, torch_dtype, device):
    """A 1-D tensor whose every element holds the NaN bit pattern of its size."""
    import torch
    size = torch.empty((), dtype=torch_dtype).element_size()
    itype = torch.int32 if size == 4 else torch.int64
    bits = int(np.array(NAN_BITS[size], UINT_OF[size]).astype(np.int32 if size == 4 else np.int64))
    return torch.full((numel,), bits, dtype=itype, device=device).view(torch_dtype)


def window(flat, shift, m, n, ld, layout):
    """An (m, n) window into the 1-D tensor `flat`, `shift` elements past its start: row-major with row stride ld >= n ('R')
    or column-major with column stride ld >= m ('L')."""
    if layout == "R":
        return flat[shift:shift + m * ld].view(m, ld)[:, :n]
    return flat[shift:shift + n * ld].view(n, ld)[:, :m].t()


def window_numel(shift, m, n, ld, layout, slack=5):
    return shift + (m if layout == "R" else n) * ld + slack


def ld_for(extent, itemsize, odd=False):
    """A leading dimension >= extent: a multiple of 16 bytes with room to spare, or an odd one."""
    V = V_of(itemsize)
    ld = _cdiv(extent, V) * V + V
    return ld + 1 + (ld % 2) if odd else ld


# ----------------------------------------------------------------------------------------------------------- the rung lists
# (a) column x misalignment
COLUMN_WIDTHS = {False: [130, 3, 5, 2, 130], True: [20, 3, 5, 2, 14]}


def column_system(small=False):
    """A lower system of 270 rows, four lanes per row: level 0 (wide), a run of narrow levels of 3, 5 and 2 rows (one
    single-workgroup launch) and one wide level.  Rows of 1, 2, 3, 5 and 9 strict entries (more than the four entry lanes), the
    diagonal first, last and stored twice.  small: the same shapes on 44 rows, for the host model."""
    shapes = [T.Shape(1), T.Shape(2, (0,)), T.Shape(9), T.Shape(3, (1, 5), "s3_pair"), T.Shape(5)]
    return T._cached(("trsm_columns", small), lambda: T.trsv_system(COLUMN_WIDTHS[small], shapes, 4, seed=900, alpha=-2.0))


def column_ns(itemsize=4):
    """1 ... 2 TRSM_MAX_C V + V + 1 of fp32 (133), for both value types."""
    t = limits()
    return list(range(1, 2 * t["max_c"] * V_of(4) + V_of(4) + 2))


def layout_subset(itemsize):
    """The column counts that also run with an odd leading dimension, layout_left operands and in place: trsm_util.N_SWEEP
    (inside the ladder's range) and the column counts at which the unit count changes its team or its passes."""
    t = limits()
    V, top = V_of(itemsize), column_ns()[-1]
    s = {n for n in TU.N_SWEEP if n <= top}
    C = 1
    edges = set()
    while C <= t["max_c"]:
        edges |= {C, C + 1}
        C *= 2
    edges |= {2 * t["max_c"], 2 * t["max_c"] + 1}
    for units in edges:                          # the last n of `units` units and the first of one more, at mis = 0
        s |= {n for n in (units * V - 1, units * V, units * V + 1) if 1 <= n <= top}
    return sorted(s)


def column_rungs(itemsize):
    """[(n, X shift, B shift, variant)] of ladder (a).  variant 'R': X and B layout_right windows with 16-byte-multiple leading
    dimensions (the pieces path from n = V on); on layout_subset also 'odd' (X layout_right, odd leading dimension), 'xL' (X
    layout_left), 'bL' (B layout_left) and 'inplace' (B is X); at n = 1 also 'contig' (two contiguous vectors: the call is
    forwarded to the vector solve)."""
    V = V_of(itemsize)
    sub = set(layout_subset(itemsize))
    out = []
    for n in column_ns():
        for s in range(V):
            out.append((n, s, s, "R"))
            out.append((n, s, (s + 1) % V, "R"))
            if n in sub:
                out += [(n, s, s, v) for v in ("odd", "xL", "bL", "inplace")]
            if n == 1:
                out.append((n, s, s, "contig"))
    return out


def rung_operands(m, n, xs, bs, variant, itemsize):
    """((X layout, ldx), (B layout, ldb)) of a rung of ladder (a); in place B takes X's."""
    if variant == "contig":
        return ("R", n), ("R", n)
    ldr, ldl = ld_for(n, itemsize), ld_for(m, itemsize)
    x = ("L", ldl) if variant == "xL" else ("R", ld_for(n, itemsize, odd=True)) if variant == "odd" else ("R", ldr)
    b = x if variant == "inplace" else ("L", ldl) if variant == "bL" else ("R", ldr)
    return x, b


# (b) the (E, C) table
EC_LANES = (4, 8, 16, 64)


def ec_table(lanes):
    """{logC: E} the rule E = min(lanes, wave >> logC) yields."""
    t = limits()
    return {lc: min(lanes, t["wave"] >> lc) for lc in range(t["max_c"].bit_length())}


def small_shape_system(lanes, upper, unit):
    """Every row shape of ladder_tt.row_shapes once, in ONE level behind a level 0 just wide enough for the mean that selects
    `lanes`: ladder_tt.shape_system at a size the host model solves in a moment."""
    w0 = {4: 260, 8: 60, 16: 40, 64: 40}[lanes]
    shapes = T.row_shapes(lanes, unit)
    return T._cached(("trsm_small_shapes", lanes, upper, unit),
                     lambda: T.trsv_system([w0, len(shapes)], shapes, lanes, upper, unit, seed=lanes,
                                           alpha=T.alpha_of(lanes, upper, unit)))


def assert_shapes_around_every_E(s, G, Es, runs=True):
    """The system holds, in each of its level groups, rows of k E - 1, k E and k E + 1 strict entries for every entry-lane count
    E of its class and every multiple k E <= 2 G + 2, and stored diagonals on entry lane 0 and E - 1, in the first and in a
    later round, and pairs of stored diagonals on different lanes."""
    rows = np.repeat(np.arange(s.m), np.diff(s.rowptr))
    strict = np.bincount(rows[s.kind == 1], minlength=s.m)
    pos = np.arange(s.nnz) - s.rowptr[:-1].astype(np.int64)[rows]
    groups = [s.level >= 1]
    if runs:
        widths, k = T.shape_widths(G, s.unit)
        groups = [(s.level >= 1) & (s.level < 1 + k), s.level == 1 + k, s.level >= 2 + k]
    for g in groups:
        have = set(strict[g].tolist())
        assert set(range(1, 2 * G + 3)) <= have
        dread = {(int(pos[p]), int(strict[rows[p]])) for p in np.flatnonzero((s.kind == 2) & g[rows])}
        pairs = {}
        for p in np.flatnonzero(((s.kind == 2) | (s.kind == 3)) & g[rows]):
            pairs.setdefault(int(rows[p]), []).append(int(pos[p]))
        pairs = [v for v in pairs.values() if len(v) == 2]
        assert pairs or s.unit
        for E in Es:
            assert E <= G
            for kE in range(E, 2 * G + 3, E):
                assert {kE - 1, kE, kE + 1} - {0} <= have, (G, E, kE)
            lanes_first = {p % E for p, _ in dread if p < E}
            lanes_later = {p % E for p, _ in dread if p >= E}
            assert {0, E - 1} <= lanes_first and {0, E - 1} <= lanes_later, (G, E)
            assert s.unit or any(a % E != b % E for a, b in pairs)


def ec_ns(itemsize, mis):
    """Column counts for ladder (b) at misalignment mis: one per logC = 0 ... log2(TRSM_MAX_C) -- 1, 2, 3, 7 and MAX_C units,
    each with a partial unit behind where the count allows it -- and one that takes two passes (MAX_C + 3 units)."""
    t = limits()
    V = V_of(itemsize)
    units = [1, 2, 3, 7, t["max_c"], t["max_c"] + 3]
    return [max(u * V - mis - (1 if u > 1 else 0), 1) for u in units]


# (c) level widths around the teams of a workgroup
TEAMS = (4, 16, 64)


def team_n(team, itemsize):
    """A column count at which four lanes per row make a team of `team` lanes (E = 4, C = team / 4), with a partial unit behind."""
    C = team // 4
    return V_of(itemsize) if C == 1 else C * V_of(itemsize) - 1


def team_widths(team):
    """(widths of the wide system, narrow limit to inspect it under, widths of the narrow system, its narrow limit): wide levels
    of k (256 / team) - 1, + 0, + 1 rows for k = 1, 2 behind level 0; a narrow level of 1024 / team + 1 rows inside one run."""
    t = limits()
    per_wg, per_chain = t["level_threads"] // team, t["chain_threads"] // team
    wide = [max(2 * per_wg + 2, 40)] + [k * per_wg + d for k in (1, 2) for d in (-1, 0, 1)]
    narrow = [max(per_chain // 2, 20), 2, per_chain + 1, 3]
    return wide, min(wide[1:]), narrow, 100000


def team_system(team, which):
    wide, _, narrow, _ = team_widths(team)
    shapes = [T.Shape(1), T.Shape(2, (0,)), T.Shape(5)]
    return T._cached(("trsm_team", team, which), lambda: T.trsv_system(
        wide if which == "wide" else narrow, shapes, 4, upper=which == "narrow" and team == 16, seed=950 + team,
        alpha=T.alpha_of(team)))


# (d) the reach of the buffer descriptor
def reach_spans():
    """{name: bytes X spans}: the last span below 2^31, the first whose offsets carry the sign bit, the last one admitted to the
    pieces path and the first one refused."""
    t = limits()
    return {"below_2^31": 2 ** 31 - t["piece"], "above_2^31": 2 ** 31 + t["piece"], "last_admitted": t["reach"],
            "first_refused": t["reach"] + t["piece"]}


def reach_shape(span, itemsize, m_range=range(5, 51)):
    """(m, n, xrs) with ((m - 1) xrs + n) itemsize == span, xrs a multiple of the piece, m in 5 ... 50 and n >= 2 V the smallest
    that fits (span is a multiple of the piece, so n is a multiple of V: whole units when X is aligned)."""
    t = limits()
    V = V_of(itemsize)
    for n in range(2 * V, 40 * V, V):
        for m in m_range:
            rest = span - n * itemsize
            if rest % (t["piece"] * (m - 1)) == 0:
                return m, n, rest // ((m - 1) * itemsize)
    raise AssertionError(f"no shape of 5 ... 50 rows spans {span} bytes")
