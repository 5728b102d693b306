"""Generators and checkers for ILU(0) (csrc/ilu0.hip): tests/test_ilu0_cpu.py proves them on the host, tests/test_gpu_ilu0.py runs
them on the device.  Every limit of the kernel is READ from its source (ilu0_limits); the level plan's limits come from
tests/ladder_tt.py (trsv_limits: the plan is the lower solve's).

PATTERNS are (rowptr, colind) in int32 with strictly ascending columns in every row and a stored diagonal.

EXACT FAMILIES.  exact_system(rowptr, colind, seed): L on the strict lower part of the pattern P with entries in {+-1, +-2}, U on
the upper part with entries in {+-1, +-2} and a diagonal in {+-1/2, +-1, +-2, 4}, A = (L U) restricted to P.  (L U)_ij sums l_it u_tj
over exactly the t with (i, t) and (t, j) in P, which are the updates ILU(0) applies, so ILU(0) of A on P is L and U; every
intermediate is a multiple of 1/2 far below 2^24, so the factor must EQUAL them bit for bit in fp32 and fp64 under any lane
count and any schedule.  zero_pivots=(r, ...) puts a zero on U's diagonal there: the rows that do not depend on such a row stay
exact (independent_rows).

RESIDUAL CHECK for random data (residual_violations): from the returned L and U, in float64, for every (i, j) in P
    |sum_t l_it u_tj - a_ij| <= (terms + 2) eps (|a_ij| + sum_t |l_it u_tj|)
t over the columns present in row i's lower part (plus the implied l_ii = 1) and in column j of U; eps = 2^-23 / 2^-52.  That is
the rounding of a chain of `terms` fmas and one division; ILU(0) is unique when the pivots are non-zero, so the residual pins
the factors.
"""
import os
import re

import numpy as np
import scipy.sparse as sps

import ladder_tt as TT

CSRC = TT.CSRC
EPS = {np.dtype(np.float32): 2.0 ** -23, np.dtype(np.float64): 2.0 ** -52}


def ilu0_limits():
    """Every size csrc/ilu0.hip branches on."""
    with open(os.path.join(CSRC, "ilu0.hip")) as f:
        src = f.read()

    def get(pattern, what):
        m = re.search(pattern, src)
        assert m, f"{what}: the source no longer has the expected form; update tests/ilu_util.py"
        return int(m.group(1))
    t = {"lds_per_lane": get(r"#define ILU0_LDS_PER_LANE (\d+)", "ILU0_LDS_PER_LANE"),
         "level_threads": get(r"#define ILU0_LEVEL_THREADS (\d+)", "ILU0_LEVEL_THREADS"),
         "chain_threads": get(r"#define ILU0_CHAIN_THREADS (\d+)", "ILU0_CHAIN_THREADS")}
    assert re.search(r"if \(len <= G \* ILU0_LDS_PER_LANE\)", src), "the fast path's cap: update tests/ilu_util.py"
    return t


def lds_cap(lanes):
    """The longest row (entries) the fast path of a team of `lanes` lanes holds in LDS."""
    return lanes * ilu0_limits()["lds_per_lane"]


# ================================================================================================================ patterns
def pattern_from_rows(rows, m=None):
    """rows[i] = iterable of columns; the diagonal is added, columns are sorted and made unique."""
    m = len(rows) if m is None else m
    out = [np.unique(np.concatenate([np.asarray(list(r), np.int64), [i]])) for i, r in enumerate(rows)]
    assert all(o.size == 0 or (o[0] >= 0 and o[-1] < m) for o in out)
    rowptr = np.concatenate([[0], np.cumsum([o.size for o in out])]).astype(np.int32)
    colind = (np.concatenate(out) if out else np.zeros(0)).astype(np.int32)
    return rowptr, colind


def check_pattern(rowptr, colind):
    m = rowptr.size - 1
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    assert rowptr[0] == 0 and rowptr[-1] == colind.size
    same = rows[1:] == rows[:-1]
    assert (colind[1:][same] > colind[:-1][same]).all(), "columns not strictly ascending"
    assert colind.size == 0 or (colind.min() >= 0 and colind.max() < m)
    assert np.bincount(rows[colind == rows], minlength=m).min(initial=1) == 1, "a row without a diagonal"


def diag_positions(rowptr, colind):
    m = rowptr.size - 1
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    d = np.flatnonzero(colind == rows)
    assert d.size == m
    return d


def _near(rng, lo, hi, count):
    """`count` distinct integers of [lo, hi), as close to `hi` as a window of twice the count allows (`near_hi`), ascending."""
    if count <= 0:
        return np.zeros(0, np.int64)
    assert hi - lo >= count
    w = min(hi - lo, 2 * count + 6)
    return np.sort(hi - 1 - rng.choice(w, count, replace=False))


def _near_above(rng, i, m, count):
    """`count` distinct integers of (i, m), as close to i as a window of twice the count allows, ascending."""
    if count <= 0:
        return np.zeros(0, np.int64)
    assert m - 1 - i >= count
    w = min(m - 1 - i, 2 * count + 6)
    return np.sort(i + 1 + rng.choice(w, count, replace=False))


def shaped_pattern(specs, limit, seed=0, margin=None):
    """A pattern whose row margin + s holds specs[s] = (strict-lower entries, entries right of the diagonal), the columns drawn
    from a window next to the diagonal (so that pivot rows and target rows share columns), between `margin` filler rows in front
    and as many behind; the filler rows are sized so that the matrix holds EXACTLY limit x m entries.  Returns (rowptr, colind,
    first shaped row)."""
    rng = np.random.default_rng(seed)
    ns = len(specs)
    big = max(max(lo, up) for lo, up in specs) if specs else 0
    margin = big + 8 if margin is None else margin
    shaped = sum(lo + up + 1 for lo, up in specs)
    nf = 2 * margin
    # fillers hold at least their diagonal: limit * (nf + ns) >= shaped + nf
    while limit * (nf + ns) < shaped + nf + (limit - 1) * 8:
        nf += 16
    m = nf + ns
    front = nf // 2
    total = limit * m
    fill_len = np.full(nf, (total - shaped) // nf, np.int64)
    fill_len[:(total - shaped) % nf] += 1
    assert fill_len.min() >= 1 and fill_len.max() <= margin, (fill_len.min(), fill_len.max(), margin)
    rows, f = [], 0
    for i in range(m):
        if front <= i < front + ns:
            lo, up = specs[i - front]
        else:
            extra = int(fill_len[f]) - 1
            f += 1
            up = min(m - 1 - i, (extra + 1) // 2)
            lo = extra - up
            if lo > i:
                lo, up = i, extra - i
        assert lo <= i and up <= m - 1 - i, (i, lo, up, m)
        rows.append(np.concatenate([_near(rng, 0, i, lo), _near_above(rng, i, m, up)]))
    rowptr, colind = pattern_from_rows(rows)
    assert int(rowptr[-1]) == total
    check_pattern(rowptr, colind)
    return rowptr, colind, front


def interleave(rowptr, colind, copies):
    """`copies` independent copies of a pattern, row i of copy c at index i * copies + c: every level is `copies` times as wide."""
    m = rowptr.size - 1
    lens = np.repeat(np.diff(rowptr), copies)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = np.repeat(np.arange(m * copies), lens)
    src_row, c = rows // copies, rows % copies
    pos = np.arange(rp[-1]) - rp[:-1][rows]
    ci = colind[rowptr[:-1][src_row] + pos].astype(np.int64) * copies + c
    return rp, ci.astype(np.int32)


def add_entry(rowptr, colind, row, col):
    """One more entry (row, col), which the pattern must not hold yet."""
    p0, p1 = int(rowptr[row]), int(rowptr[row + 1])
    assert col not in colind[p0:p1]
    at = p0 + int(np.searchsorted(colind[p0:p1], col))
    rp = rowptr.copy()
    rp[row + 1:] += 1
    return rp, np.insert(colind, at, col).astype(np.int32)


def level_pattern(widths, seed=0, shuffle=True, lower=(1, 3), upper=(0, 3), long_rows=0, long_len=0):
    """A pattern whose lower level sets have exactly the given widths.  The rows of a level are spread over the index range when
    `shuffle` (the first row of level l keeps its place in front of the first of level l + 1, so every level stays reachable).
    A row of level l >= 1 reads one row of level l - 1 and lower[0] - 1 ... lower[1] - 1 rows of earlier levels, and holds
    upper[0] ... upper[1] entries right of the diagonal (fewer where the index range ends).  The long_rows rows of the deepest level with the smallest
    indices get long_len more entries right of the diagonal (which change no level).  Returns (rowptr, colind, level of every row)."""
    rng = np.random.default_rng(seed)
    widths = [int(w) for w in widths]
    nl, m = len(widths), int(sum(widths))
    level = np.repeat(np.arange(nl), widths)
    first = np.concatenate([[0], np.cumsum(widths)])[:-1]
    key = rng.random(m) * 0.999 + 0.0005 if shuffle else np.arange(m) / (m + 1.0) * 0.999 + 0.0005
    key[first] = np.arange(nl) * (0.0004 / nl)
    idx = np.empty(m, np.int64)
    idx[np.argsort(key, kind="stable")] = np.arange(m)
    lev_of_index = np.empty(m, np.int64)
    lev_of_index[idx] = level
    by_level = [np.sort(idx[level == l]) for l in range(nl)]
    below = [np.sort(idx[level < l]) for l in range(nl)]
    rows = []
    for i in range(m):
        l = int(lev_of_index[i])
        cols = []
        if l > 0:
            prev = by_level[l - 1]
            k = int(np.searchsorted(prev, i))
            assert k >= 1
            cols.append(prev[rng.integers(0, k)])
            pool = below[l]
            k = int(np.searchsorted(pool, i))
            n_more = int(rng.integers(lower[0], lower[1] + 1)) - 1
            if n_more > 0:
                cols.extend(pool[rng.integers(0, k, n_more)])
        n_up = min(m - 1 - i, int(rng.integers(upper[0], upper[1] + 1)))
        if n_up:
            cols.extend(i + 1 + rng.choice(m - 1 - i, n_up, replace=False))
        rows.append(cols)
    if long_rows:
        for i in by_level[nl - 1][:long_rows]:
            i = int(i)
            have = set(int(c) for c in rows[i])
            room = np.array([c for c in range(i + 1, m) if c not in have])
            assert room.size >= long_len, "no room right of the diagonal: use a longer index range"
            rows[i] = list(rows[i]) + list(rng.choice(room, long_len, replace=False))
    rowptr, colind = pattern_from_rows(rows)
    check_pattern(rowptr, colind)
    got = TT.levels_of(rowptr, colind, m, False)
    assert np.array_equal(got, lev_of_index), "level_pattern: the designed levels are not the levels"
    return rowptr, colind, lev_of_index


def laplacian7(nx, ny, nz):
    """The pattern of the 7-point Laplacian on an nx x ny x nz grid in natural order."""
    n = nx * ny * nz
    i = np.arange(n)
    x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
    cand = [(i - nx * ny, z > 0), (i - nx, y > 0), (i - 1, x > 0), (i, np.ones(n, bool)), (i + 1, x < nx - 1),
            (i + nx, y < ny - 1), (i + nx * ny, z < nz - 1)]
    cols = np.stack([c for c, _ in cand], axis=1)
    keep = np.stack([k for _, k in cand], axis=1)
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return rowptr, cols[keep].astype(np.int32)


def random_pattern(m, per_row, seed=0, band=None):
    """m rows with the diagonal and per_row - 1 other columns spread over both triangles, inside a band around the diagonal when
    given.  Small matrices hold exactly per_row entries in every row; large ones draw with replacement and drop the repeats (a
    few rows are an entry short)."""
    rng = np.random.default_rng(seed)
    band = m if band is None else band
    W = min(m, 2 * band + 1)
    if m * W <= 4_000_000:
        start = np.clip(np.arange(m) - W // 2, 0, m - W)
        keys = rng.random((m, W))
        keys[np.arange(m), np.arange(m) - start] = -1.0          # the diagonal is always taken
        take = np.sort(np.argpartition(keys, per_row - 1, axis=1)[:, :per_row], axis=1)
        rowptr = (np.arange(m + 1) * per_row).astype(np.int32)
        return rowptr, (take + start[:, None]).astype(np.int32).ravel()
    k = per_row - 1
    off = rng.integers(1, band, (m, k)) * rng.choice([-1, 1], (m, k))
    cols = np.arange(m)[:, None] + off
    cols = np.where((cols < 0) | (cols >= m), np.arange(m)[:, None] - off, cols)
    cols = np.clip(cols, 0, m - 1)
    cols = np.concatenate([cols, np.arange(m)[:, None]], axis=1)
    cols.sort(axis=1)
    keep = np.ones_like(cols, bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return rowptr, cols[keep].astype(np.int32)


# ================================================================================================================== values
def _rows_of(rowptr):
    return np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))


def split_lu(rowptr, colind, values):
    """(L with its unit diagonal, U) of a factor stored on the pattern, as float64 scipy CSR matrices that keep explicit zeros."""
    m = rowptr.size - 1
    rows = _rows_of(rowptr)
    v = np.asarray(values[:colind.size], np.float64)
    lo = colind < rows
    L = sps.csr_matrix((np.concatenate([v[lo], np.ones(m)]), (np.concatenate([rows[lo], np.arange(m)]),
                                                              np.concatenate([colind[lo], np.arange(m)]))), shape=(m, m))
    U = sps.csr_matrix((v[~lo], (rows[~lo], colind[~lo])), shape=(m, m))
    return L, U


def _at_pattern(C, rowptr, colind):
    """The entries of the sparse matrix C at the pattern's positions, in the pattern's order (0 where C holds none)."""
    m = rowptr.size - 1
    P = sps.csr_matrix((np.ones(colind.size), colind.astype(np.int64), rowptr.astype(np.int64)), shape=(m, m))
    R = C.multiply(P).tocoo()
    keys = _rows_of(rowptr).astype(np.int64) * m + colind
    at = np.searchsorted(keys, R.row.astype(np.int64) * m + R.col)
    out = np.zeros(colind.size)
    out[at] = R.data
    return out


def exact_system(rowptr, colind, seed=0, zero_pivots=()):
    """(A's values, the expected LU values), both float64, for the exact family on this pattern."""
    rng = np.random.default_rng(seed)
    rows = _rows_of(rowptr)
    lu = rng.choice([-2.0, -1.0, 1.0, 2.0], colind.size)
    d = colind == rows
    lu[d] = rng.choice([-0.5, 0.5, -1.0, 1.0, -2.0, 2.0, 4.0], int(d.sum()))
    if len(zero_pivots):
        lu[diag_positions(rowptr, colind)[np.asarray(zero_pivots)]] = 0.0
    L, U = split_lu(rowptr, colind, lu)
    a = _at_pattern(L @ U, rowptr, colind)
    assert np.abs(a).max(initial=0.0) < 2 ** 20 and np.array_equal(a * 2, np.round(a * 2)), "exact data leave the exact range"
    return a, lu


def independent_rows(rowptr, colind, bad_rows):
    """Mask of the rows whose factor does not depend on any of bad_rows (a row depends on the rows of its strict-lower columns)."""
    m = rowptr.size - 1
    bad = np.zeros(m, bool)
    bad[np.asarray(bad_rows, np.int64)] = True
    tainted = np.zeros(m, bool)
    for i in range(m):
        c = colind[rowptr[i]:rowptr[i + 1]]
        c = c[c < i]
        tainted[i] = c.size > 0 and bool((bad[c] | tainted[c]).any())
    return ~tainted   # a bad row that reads clean rows only is itself still exact


def dominant_values(rowptr, colind, seed=0):
    """Random values with a dominant diagonal (float64)."""
    rng = np.random.default_rng(seed)
    rows = _rows_of(rowptr)
    v = rng.uniform(-1.0, 1.0, colind.size)
    d = colind == rows
    v[d] = 0.0
    absrow = np.bincount(rows, weights=np.abs(v), minlength=rowptr.size - 1)
    v[d] = (absrow + 1.0 + rng.random(rowptr.size - 1)) * rng.choice([-1.0, 1.0], rowptr.size - 1)
    return v


def host_ilu0(rowptr, colind, values, dtype=np.float64, skip_update=None):
    """The definition, in IKJ order, in `dtype` (each update rounded once: the product is formed in float64).  skip_update =
    (i, k): that one pivot step of row i leaves the rest of the row alone (a wrong factor for the checker's own test)."""
    dtype = np.dtype(dtype)
    m = rowptr.size - 1
    lu = np.asarray(values[:colind.size]).astype(dtype).copy()
    diag = diag_positions(rowptr, colind)
    for i in range(m):
        p0, p1 = int(rowptr[i]), int(rowptr[i + 1])
        cols = colind[p0:p1]
        w = lu[p0:p1]
        for q in range(int(diag[i]) - p0):
            k = int(cols[q])
            with np.errstate(all="ignore"):
                w[q] = w[q] / lu[diag[k]]
            if skip_update == (i, k):
                continue
            kc = colind[diag[k] + 1:rowptr[k + 1]]
            kv = lu[diag[k] + 1:rowptr[k + 1]]
            pos = np.searchsorted(cols, kc)
            hit = pos < cols.size
            hit[hit] = cols[pos[hit]] == kc[hit]
            with np.errstate(all="ignore"):
                w[pos[hit]] = (w[pos[hit]].astype(np.float64) - np.float64(w[q]) * kv[hit].astype(np.float64)).astype(dtype)
    return lu


def products_at_pattern(rowptr, colind, lu_values):
    """For every (i, j) of the pattern: (sum_t l_it u_tj, sum_t |l_it u_tj|, number of terms), t over the columns present in row
    i's lower part (plus the implied l_ii = 1) and in column j of U.  The triples (i, t, j) are expanded and summed in extended
    precision (the 64-bit significand of x86 long double: the checker's own rounding is 2^-11 of an fp64 step)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "no extended precision on this host: sum the terms exactly instead"
    m, nnz = rowptr.size - 1, colind.size
    rows = _rows_of(rowptr)
    lu = np.asarray(lu_values[:nnz], np.float64)
    d = diag_positions(rowptr, colind)
    low = colind < rows
    Li = np.concatenate([rows[low], np.arange(m)])
    Lt = np.concatenate([colind[low].astype(np.int64), np.arange(m)])
    Lv = np.concatenate([lu[low], np.ones(m)])
    cnt = (rowptr[1:].astype(np.int64) - d)[Lt]                    # row t of U: positions d[t] ... rowptr[t + 1] - 1
    src = np.repeat(np.arange(Li.size), cnt)
    up = d[Lt[src]] + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    keys = rows.astype(np.int64) * m + colind
    key = Li[src].astype(np.int64) * m + colind[up]
    at = np.minimum(np.searchsorted(keys, key), nnz - 1)
    hit = keys[at] == key
    at, prod = at[hit], Lv[src][hit].astype(np.longdouble) * lu[up][hit].astype(np.longdouble)
    order = np.argsort(at, kind="stable")
    at, prod = at[order], prod[order]
    starts = np.flatnonzero(np.concatenate([[True], at[1:] != at[:-1]]))
    total, mag, terms = np.zeros(nnz, np.longdouble), np.zeros(nnz, np.longdouble), np.zeros(nnz, np.int64)
    total[at[starts]] = np.add.reduceat(prod, starts)
    mag[at[starts]] = np.add.reduceat(np.abs(prod), starts)
    terms[at[starts]] = np.diff(np.concatenate([starts, [at.size]]))
    return total, mag, terms


def residual_violations(rowptr, colind, a_values, lu_values, dtype, limit=5):
    """Messages (empty: passes) of the residual check of the module docstring."""
    eps = EPS[np.dtype(dtype)]
    lu = np.asarray(lu_values[:colind.size], np.float64)
    a = np.asarray(a_values[:colind.size], np.float64)
    if not np.isfinite(lu).all():
        return [f"{int((~np.isfinite(lu)).sum())} entries of the factor are not finite"]
    if not colind.size:
        return []
    total, mag, terms = products_at_pattern(rowptr, colind, lu)
    assert terms.min() >= 1
    rows = _rows_of(rowptr)
    bound = (terms + 2) * eps * (np.abs(a) + mag.astype(np.float64))
    res = np.abs(total - a.astype(np.longdouble)).astype(np.float64)
    bad = np.flatnonzero(res > bound)
    return [f"{bad.size} entries miss the residual bound; ({int(rows[p])}, {int(colind[p])}): residual {res[p]:.3e} > bound "
            f"{bound[p]:.3e}" for p in bad[:limit]]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def exact_violations(got, want, rowptr=None, colind=None, rows_mask=None, limit=5):
    """Messages (empty: passes): got must equal want bit for bit (-0.0 and +0.0 differ; the exact families hold no zero except a
    designed zero pivot, which is +0.0 on both sides).  rows_mask restricts the comparison to those rows."""
    got = np.asarray(got)
    want = np.asarray(want).astype(got.dtype)
    if got.shape != want.shape:
        return [f"shape {got.shape} != {want.shape}"]
    diff = bits(got) != bits(want)
    if rows_mask is not None:
        diff &= np.repeat(rows_mask, np.diff(rowptr))
    bad = np.flatnonzero(diff)
    if not bad.size:
        return []
    where = ""
    if rowptr is not None:
        r = int(np.searchsorted(rowptr, bad[0], side="right") - 1)
        where = f" (row {r}, column {int(colind[bad[0]])}, in-row position {int(bad[0] - rowptr[r])} of {int(rowptr[r + 1] - rowptr[r])})"
    return [f"{bad.size} entries differ, first at {int(bad[0])}{where}: {got[bad[0]]} != {want[bad[0]]}"] + \
           [f"  at {int(p)}: {got[p]} != {want[p]}" for p in bad[1:limit]]


# ======================================================================================================= the ladders' rungs
LIMITS = (6, 24, 96)      # the mean row lengths at which the plan changes its lanes per row (ladder_tt.trsv_limits: lane_steps)


def lane_cases():
    """[(limit, extra, lanes)]: limit x m entries take the lower lane count, one entry more the higher."""
    steps = TT.trsv_limits()["lane_steps"]
    assert [s[0] for s in steps] == list(LIMITS), "the lane steps moved: update tests/ilu_util.py"
    return [(limit, extra, at if extra == 0 else above) for limit, at, above in steps for extra in (0, 1)]


def lower_counts(G):
    return sorted(set(range(0, 2 * G + 3)) | {3 * G - 1, 3 * G + 1, 300})


def upper_counts(G):
    return sorted({0, 1, G - 1, G, G + 1, 2 * G + 1, 300})


def shape_specs(G):
    """(strict-lower, right-of-diagonal) counts of the target rows for G lanes per row: every lower count of the ladder with the
    upper counts in turn, every upper count with three lower counts, and rows of cap - 1, cap, cap + 1 entries (cap = the fast
    path's LDS room) split both ways.  Every shaped row is also a pivot row of the rows behind it."""
    lows, ups = lower_counts(G), upper_counts(G)
    specs = [(lo, ups[i % len(ups)]) for i, lo in enumerate(lows)]
    specs += [(lo, up) for up in ups for lo in (1, G + 1, 2 * G + 2)]
    cap = lds_cap(G)
    for n in (cap - 1, cap, cap + 1):
        specs += [(n - 1 - 2, 2), (3, n - 1 - 3), ((n - 1) // 2, n - 1 - (n - 1) // 2)]
    specs += [(300, 300), (0, 0)]
    return specs


def shape_system(limit, extra, copies=1, seed=0):
    """The row-shape ladder for the lane count that `limit x m + extra` entries select.  Returns (rowptr, colind, lanes, specs,
    first shaped row, copies)."""
    lanes = [c[2] for c in lane_cases() if c[:2] == (limit, extra)][0]
    specs = shape_specs(lanes)
    rowptr, colind, front = shaped_pattern(specs, limit, seed=seed + limit + extra)
    if copies > 1:
        rowptr, colind = interleave(rowptr, colind, copies)
    if extra:
        m = rowptr.size - 1
        rowptr, colind = add_entry(rowptr, colind, 0, m - 1) if (m - 1) not in colind[:rowptr[1]] else \
            add_entry(rowptr, colind, 1, m - 1)
    m = rowptr.size - 1
    assert int(rowptr[-1]) == limit * m + extra and TT.lanes_of(int(rowptr[-1]), m) == lanes
    check_pattern(rowptr, colind)
    return rowptr, colind, lanes, specs, front, copies


def predicted_info(rowptr, colind):
    """What ilu0_info must report: the lower level sets restated on the host, one launch per plan group."""
    m = rowptr.size - 1
    lev = TT.levels_of(rowptr, colind, m, False)
    widths = np.bincount(lev).tolist() if m else []
    return {"levels": len(widths), "max_level_width": max(widths, default=0),
            "launches_per_factor": len(TT.groups_of(widths, TT.trsv_limits()["narrow"])),
            "lanes_per_row": TT.lanes_of(int(rowptr[-1]), m)}
