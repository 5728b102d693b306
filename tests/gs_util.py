"""The host model, the structure check and the generators of the multicolour Gauss-Seidel sweeps (csrc/gauss_seidel.hip):
tests/test_gs_cpu.py proves on the host that they hold what they claim, tests/test_gpu_gauss_seidel.py runs them on the device.

THE RECURRENCE (host_gauss_seidel).  sigma(i) = perm[i] when a perm is given, else i; colour c is the positions
color_ptr[c] .. color_ptr[c + 1] - 1.  One row update is
    dot = sum of a_rc * x_c over the stored entries of row r with c != r         (repeated off-diagonal entries are summed)
    g   = (b_r - dot) / d_r                                                       d_r = the row's one stored diagonal entry
    x_r = g  if omega == 1 (the old x_r is not read),  else  x_r = fma(omega, g - x_r, x_r)
forward: colours 0 .. C - 1 one after the other, backward: C - 1 .. 0, symmetric: forward then backward; `sweeps` repeats that.
The model is SEQUENTIAL in colour order and restates the recurrence in numpy in the given dtype, every operation rounded once,
the entries of a row added one after the other in the stored order or (perm_seed) in a random order.  The fma: for float32 the
product is formed exactly in float64 and the sum rounded to float64, then to float32; for float64 product and sum are rounded
separately -- neither differs from a true fma on the dyadic systems (every intermediate is exact there: that is what the CPU
test proves), and on the dominant systems the difference is one rounding inside the bound.  It also returns the per-row scale
    S_r = max over the updates of (|b_r| + sum |a_rc| |x_c|) / |d_r|                                           (float64)

DYADIC SYSTEMS (dyadic_system).  Off-diagonal entries +-1, diagonal in {+-1, +-2}, integer b and x0 in [-4, 4], omega in
{1, 0.5, 1.5}.  The colouring is built directly: colour 0 holds "quiet" rows with a diagonal entry only (with omega = 1 their
value b / d never changes), the rows of the later colours read at most 4 rows of OTHER non-quiet colours (earlier and later
ones, so forward, backward and Jacobi all differ) and only rows of at most 4 off-diagonal entries are read that way; the further
entries of long rows read quiet rows, some of them twice.  So the iterates stay small dyadic numbers.  Row shapes: 0 ... 2 G + 2,
3 G - 1, 3 G + 1 and 300 off-diagonal entries, each with the diagonal stored first, in the middle and last; filler rows (quiet
rows, or rows of 300 entries over quiet rows) bring nnz / m into the lane class asked for.  One colour is empty.  Every case --
the four lane classes, the three omega, the three directions -- stays exact in float32 for 2 sweeps (no case had to be
reduced to 1): tests/test_gs_cpu.py proves it.

DOMINANT SYSTEMS (dominant_system).  Values uniform in (-1, 1), |d_r| >= 2 sum |a_rc| + 0.5, at most 9 stored entries per row.
With the error e of the iterate, one update gives |e_r| <= (1 - omega) |e_r| + omega max|e| / 2: at omega = 1 the iteration
contracts by 1/2 in the maximum norm, at 0 < omega < 1 by 1 - omega / 2.  A per-update rounding error is bounded by
(k + 2) 2^-24 S_r < 1e-6 S_r for k <= 9 entries (1e-12 S_r in float64), so the errors sum to at most 2 tol max_r S_r at omega = 1
(and, the per-update error itself scaled by omega, to (6.6e-7 omega + 1.2e-7) / (omega / 2) < 2e-6 for omega >= 0.75).
"""
import numpy as np

import multicolor_util as M
from sweeps_util import TOL, bits, bit_violations  # noqa: F401  (re-exported for the tests)

OMEGAS = (1.0, 0.5, 1.5)
DIRECTIONS = ("forward", "backward", "symmetric")
TARGET_MEAN = {4: 4.0, 8: 12.0, 16: 40.0, 64: 110.0}


class System:
    pass


def _entry_rows(rowptr):
    return np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))


# ====================================================================================================== the host recurrence
def host_gauss_seidel(rowptr, colind, values, b, x0, color_ptr, perm, sweeps, omega, direction, dtype, perm_seed=None):
    """(x after `sweeps` sweeps in `dtype`, S in float64)."""
    assert direction in DIRECTIONS and sweeps >= 0
    dtype = np.dtype(dtype)
    rowptr, colind = np.asarray(rowptr, np.int64), np.asarray(colind, np.int64)
    color_ptr = np.asarray(color_ptr, np.int64)
    m = rowptr.size - 1
    sigma = np.arange(m) if perm is None else np.asarray(perm, np.int64)
    rows = _entry_rows(rowptr)
    vals = np.asarray(values)[:colind.size].astype(dtype)
    b = np.asarray(b).astype(dtype)
    x = np.asarray(x0).astype(dtype).copy()
    d = np.zeros(m, dtype)
    dp = np.flatnonzero(colind == rows)
    d[rows[dp]] = vals[dp]
    oe = np.flatnonzero(colind != rows)
    if perm_seed is not None:
        key = np.random.default_rng(perm_seed).random(oe.size)
        oe = oe[np.lexsort((key, rows[oe]))]
    sr, sc, sv = rows[oe], colind[oe], vals[oe]
    first = np.searchsorted(sr, np.arange(m))
    rank = np.arange(oe.size) - first[sr]
    ncol = color_ptr.size - 1
    color_of = np.empty(m, np.int64)
    color_of[sigma] = np.repeat(np.arange(ncol), np.diff(color_ptr))
    ec = color_of[sr]
    by_rank = []
    for c in range(ncol):
        e = np.flatnonzero(ec == c)
        by_rank.append([e[rank[e] == k] for k in range(int(rank[e].max(initial=-1)) + 1)])
    absb, absd = np.abs(b.astype(np.float64)), np.abs(d.astype(np.float64))
    S = np.zeros(m)
    w = dtype.type(omega)

    def update(c):
        nonlocal S
        r = sigma[color_ptr[c]:color_ptr[c + 1]]
        if r.size == 0:
            return
        dot = np.zeros(m, dtype)
        mag = np.zeros(m)
        with np.errstate(all="ignore"):
            for e in by_rank[c]:
                dot[sr[e]] = dot[sr[e]] + sv[e] * x[sc[e]]
                mag[sr[e]] += np.abs(sv[e].astype(np.float64) * x[sc[e]].astype(np.float64))
            S[r] = np.fmax(S[r], (absb[r] + mag[r]) / absd[r])
            g = (b[r] - dot[r]) / d[r]
            if w == 1:
                x[r] = g
            else:
                t = g - x[r]
                if dtype == np.float32:
                    x[r] = (np.float64(w) * t.astype(np.float64) + x[r].astype(np.float64)).astype(np.float32)
                else:
                    x[r] = w * t + x[r]

    for _ in range(sweeps):
        if direction != "backward":
            for c in range(ncol):
                update(c)
        if direction != "forward":
            for c in range(ncol - 1, -1, -1):
                update(c)
    return x, S


def host_jacobi(rowptr, colind, values, b, x0):
    """One Jacobi sweep in float64 (every row reads the OLD iterate): what a kernel that reads a stale x would compute."""
    rows = _entry_rows(np.asarray(rowptr))
    vals, x0 = np.asarray(values, np.float64), np.asarray(x0, np.float64)
    off = colind != rows
    m = rowptr.size - 1
    dot = np.bincount(rows[off], weights=vals[off] * x0[colind[off]], minlength=m)
    d = np.zeros(m)
    d[rows[~off]] = vals[~off]
    return (np.asarray(b, np.float64) - dot) / d


# ======================================================================================================= the structure check
def structure_violations(rowptr, colind, color_ptr, perm=None):
    """The five conditions of spblas_gfx950_gs_create, restated on the host.  Messages (empty: passes)."""
    rowptr, colind, color_ptr = (np.asarray(t, np.int64) for t in (rowptr, colind, color_ptr))
    m, nnz = rowptr.size - 1, colind.size
    out = []
    if color_ptr.size < 1 or color_ptr[0] != 0 or color_ptr[-1] != m or (np.diff(color_ptr) < 0).any():
        out.append("color_ptr does not run from 0 to m without descending")
    if perm is not None:
        perm = np.asarray(perm, np.int64)
        if perm.size != m or not np.array_equal(np.sort(perm), np.arange(m)):
            out.append("perm is not a permutation of 0 .. m - 1")
    if m and (rowptr[0] != 0 or rowptr[-1] != nnz or (np.diff(rowptr) < 0).any()):
        out.append("the row offsets do not describe the entries")
    elif ((colind < 0) | (colind >= m)).any():
        out.append("a column lies outside [0, m)")
    if out:
        return out
    rows = _entry_rows(rowptr)
    ndiag = np.bincount(rows[colind == rows], minlength=m)
    if (ndiag != 1).any():
        out.append(f"row {int(np.flatnonzero(ndiag != 1)[0])} has {int(ndiag[ndiag != 1][0])} stored diagonal entries")
    sigma = np.arange(m) if perm is None else perm
    color_of = np.empty(m, np.int64)
    color_of[sigma] = np.repeat(np.arange(color_ptr.size - 1), np.diff(color_ptr))
    clash = (colind != rows) & (color_of[rows] == color_of[colind])
    if clash.any():
        p = int(np.flatnonzero(clash)[0])
        out.append(f"entry ({int(rows[p])}, {int(colind[p])}) joins two rows of colour {int(color_of[rows[p]])}")
    return out


# ================================================================================================================ assembling
def _finish(prow, color_ptr, b, x0, rng, shuffle=True):
    """prow: per POSITION (cols as positions, values), or the position-space CSR triple (rowptr, cols, values).  Deals the
    positions to random row indices (perm: position -> row) and returns the System: A's arrays (rowptr, colind, values; rows
    unsorted), perm, color_ptr, b, x0 in A's order, and B = P A P^T (b_rowptr, b_colind, b_values with ascending columns,
    equal columns in source order -- what permute gives --, pb, px0)."""
    if isinstance(prow, tuple):
        prp, pcols, pvals = (np.asarray(t) for t in prow)
    else:
        prp = np.concatenate([[0], np.cumsum([c.size for c, _ in prow])])
        pcols = np.concatenate([c for c, _ in prow] + [np.zeros(0, np.int64)]).astype(np.int64)
        pvals = np.concatenate([v for _, v in prow] + [np.zeros(0)]).astype(np.float64)
    m = prp.size - 1
    perm = (rng.permutation(m) if shuffle else np.arange(m)).astype(np.int32)
    inverse = np.empty(m, np.int64)
    inverse[perm] = np.arange(m)
    lens = np.diff(prp)[inverse]                      # A's row r is position inverse[r]
    y = System()
    y.m, y.perm, y.color_ptr = m, perm, np.asarray(color_ptr, np.int32)
    y.rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    src = np.repeat(prp[:-1][inverse], lens) + (np.arange(int(lens.sum())) - np.repeat(y.rowptr[:-1].astype(np.int64), lens))
    y.colind = perm[pcols[src]].astype(np.int32)
    y.values = pvals[src].astype(np.float64)
    y.nnz = int(y.colind.size)
    y.b, y.x0 = np.empty(m), np.empty(m)
    y.b[perm], y.x0[perm] = b, x0
    y.pb, y.px0 = np.asarray(b, np.float64), np.asarray(x0, np.float64)
    # B: the position-space rows with their columns sorted, equal columns in A's stored order (= the order here)
    prows = np.repeat(np.arange(m), np.diff(prp))
    o = np.lexsort((np.arange(pcols.size), pcols, prows))
    y.b_rowptr, y.b_colind, y.b_values = prp.astype(np.int32), pcols[o].astype(np.int32), pvals[o].astype(np.float64)
    y.lanes = M.lanes_for(y.rowptr, y.colind)
    return y


def reference(y, sweeps, omega, direction, dtype=np.float64, on_b=False, **kw):
    """host_gauss_seidel on A with perm (the result in A's order) or on B without one (in B's order)."""
    if on_b:
        return host_gauss_seidel(y.b_rowptr, y.b_colind, y.b_values, y.pb, y.px0, y.color_ptr, None, sweeps, omega, direction,
                                 dtype, **kw)
    return host_gauss_seidel(y.rowptr, y.colind, y.values, y.b, y.x0, y.color_ptr, y.perm, sweeps, omega, direction, dtype, **kw)


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ============================================================================================================ dyadic systems
def shape_counts(G):
    return list(range(0, 2 * G + 3)) + [3 * G - 1, 3 * G + 1, 300]


def _place(cols, vals, i, dval, where):
    """The stored row: the diagonal entry (i, dval) first, in the middle or last among the off-diagonal ones."""
    at = {"first": 0, "middle": cols.size // 2, "last": cols.size}[where]
    return np.insert(cols, at, i), np.insert(vals, at, dval)


def dyadic_system(lanes, seed=0, colours=4, chain=4):
    """(module docstring) colours - 1 non-quiet colours behind the quiet colour 0, one EMPTY colour in the middle."""
    def make():
        rng = np.random.default_rng(1000 + 7 * lanes + seed)
        counts = [(k, w) for k in shape_counts(lanes) for w in ("first", "middle", "last")]
        nshape = len(counts)
        base_nnz = sum(k + 1 for k, _ in counts)
        nq, nfill = 40, 0            # quiet rows / filler rows of 300 entries
        target = TARGET_MEAN[lanes]
        if (base_nnz + nq) / (nshape + nq) > target:
            nq = int(np.ceil((base_nnz - target * nshape) / (target - 1.0)))
        else:
            nfill = int(np.ceil((target * (nshape + nq) - base_nnz - nq) / (301.0 - target)))
        counts = counts + [(300, "last")] * nfill
        order = rng.permutation(len(counts))
        counts = [counts[j] for j in order]
        # positions: [quiet | colour 1 | colour 2 | (empty) | colour 3 ...]; shaped rows dealt round robin to the colours
        nshaped = len(counts)
        ncol_live = colours - 1
        colour_of_shaped = np.arange(nshaped) % ncol_live
        sizes = np.bincount(colour_of_shaped, minlength=ncol_live)
        live_ptr = nq + np.concatenate([[0], np.cumsum(sizes)])
        pos_of = np.empty(nshaped, np.int64)
        for c in range(ncol_live):
            pos_of[colour_of_shaped == c] = live_ptr[c] + np.arange(sizes[c])
        m = nq + nshaped
        # the rows a chain entry may read: non-quiet rows of at most `chain` off-diagonal entries, by colour
        short = [pos_of[(colour_of_shaped == c) & np.array([k <= chain for k, _ in counts])] for c in range(ncol_live)]
        prow = [None] * m
        for i in range(nq):
            prow[i] = (np.array([i]), np.array([rng.choice([-2.0, -1.0, 1.0, 2.0])]))
        for j, (k, where) in enumerate(counts):
            i, c = int(pos_of[j]), int(colour_of_shaped[j])
            nchain = min(chain, k) if k <= chain else min(chain, 2)
            others = np.concatenate([short[o] for o in range(ncol_live) if o != c])
            cc = rng.choice(others, nchain, replace=False) if nchain else np.zeros(0, np.int64)
            q = rng.integers(0, nq, k - nchain)
            if q.size >= 3:
                q[-1] = q[0]                              # a repeated off-diagonal entry, apart in the row
            cols = np.concatenate([cc, q]).astype(np.int64)
            vals = rng.choice([-1.0, 1.0], k)
            p = rng.permutation(k)
            prow[i] = _place(cols[p], vals[p], i, rng.choice([-2.0, -1.0, 1.0, 2.0]), where)
        # color_ptr with an empty colour in the middle
        ptr = [0] + [int(t) for t in live_ptr]
        mid = len(ptr) // 2
        ptr = ptr[:mid + 1] + [ptr[mid]] + ptr[mid + 1:]
        b = rng.integers(-4, 5, m).astype(np.float64)
        x0 = rng.integers(-4, 5, m).astype(np.float64)
        y = _finish(prow, ptr, b, x0, rng)
        y.quiet = y.perm[:nq].astype(np.int64)              # A's rows that are quiet
        assert y.lanes == lanes, (y.lanes, lanes, y.nnz / y.m)
        return y
    return cached(("dyadic", lanes, seed, colours, chain), make)


def colored_chain(n=9, colours=3):
    """Tridiagonal, row i of colour i % colours, d in {1, 2}, off-diagonal +-1: forward, backward and a Jacobi sweep all differ."""
    def make():
        rng = np.random.default_rng(5)
        color = np.arange(n) % colours
        pos = np.argsort(color, kind="stable")            # position -> chain index
        where = np.empty(n, np.int64)
        where[pos] = np.arange(n)                         # chain index -> position
        prow = []
        for p in range(n):
            i = int(pos[p])
            nb = [j for j in (i - 1, i + 1) if 0 <= j < n]
            cols = np.array([where[j] for j in nb] + [p])
            vals = np.array([rng.choice([-1.0, 1.0]) for _ in nb] + [float(1 + i % 2)])
            prow.append((cols, vals))
        ptr = np.concatenate([[0], np.cumsum(np.bincount(color, minlength=colours))])
        return _finish(prow, ptr, rng.integers(-4, 5, n).astype(np.float64), rng.integers(1, 5, n).astype(np.float64), rng)
    return cached(("chain", n, colours), make)


# ========================================================================================================== dominant systems
def dominant_system(m, colours=6, seed=0, max_off=8):
    def make():
        rng = np.random.default_rng(seed)
        color = np.sort(rng.integers(0, colours, m))
        ptr = np.concatenate([[0], np.cumsum(np.bincount(color, minlength=colours))])
        prow = []
        for i in range(m):
            k = int(rng.integers(0, max_off + 1))
            cols = rng.integers(0, m, k)
            cols = cols[color[cols] != color[i]]
            a = rng.uniform(-1.0, 1.0, cols.size)
            dv = (2.0 * np.abs(a).sum() + 0.5 + rng.random()) * rng.choice([-1.0, 1.0])
            c = np.concatenate([cols, [i]])
            v = np.concatenate([a, [dv]])
            p = rng.permutation(c.size)
            prow.append((c[p], v[p]))
        return _finish(prow, ptr, rng.uniform(-1.0, 1.0, m), rng.uniform(-1.0, 1.0, m), rng)
    return cached(("dominant", m, colours, seed, max_off), make)


def max_bound_violations(got, ref64, S, dtype, what="", limit=4):
    """Messages (empty: passes): |got_r - ref_r| <= 2 tol max_r S_r for EVERY row (a non-finite element fails)."""
    got = np.asarray(got, np.float64)
    bound = 2.0 * TOL[np.dtype(dtype)] * float(np.max(S, initial=0.0))
    with np.errstate(all="ignore"):
        err = np.abs(got - ref64)
        bad = np.flatnonzero(~(err <= bound))
    return [f"{what}: {bad.size} rows miss 2 tol max S = {bound:.3e}, first at {bad[:limit].tolist()}: error "
            f"{err[bad[:limit]].tolist()}"] if bad.size else []


# ======================================================================================================= multicolour fixtures
def multicolor_fixtures():
    return {"grid5_9x7": M.grid5(9, 7), "lap7_5x4x3": M.laplacian7(5, 4, 3), "random_300x6": M.random_rows(300, 6, seed=2),
            "ring_257": M.ring(257), "star_300": M.star(300)}


def multicolor_system(name):
    """A fixture of multicolor_util with dominant values, coloured by the host model: A with perm, and host_permuted B."""
    def make():
        rowptr, colind = multicolor_fixtures()[name]
        m = rowptr.size - 1
        rng = np.random.default_rng(len(name))
        rows = _entry_rows(rowptr)
        values = rng.uniform(-1.0, 1.0, colind.size)
        offsum = np.bincount(rows, weights=np.where(colind != rows, np.abs(values), 0.0), minlength=m)
        dg = colind == rows
        values[dg] = (2.0 * offsum[rows[dg]] + 0.5 + rng.random(int(dg.sum()))) * rng.choice([-1.0, 1.0], int(dg.sum()))
        perm, _, color_ptr = M.order_from_colors(M.model_colors(rowptr, colind))
        y = System()
        y.m, y.nnz, y.rowptr, y.colind, y.values = m, int(colind.size), rowptr.astype(np.int32), colind.astype(np.int32), values
        y.perm, y.color_ptr = perm.astype(np.int32), color_ptr.astype(np.int32)
        y.b, y.x0 = rng.uniform(-1.0, 1.0, m), rng.uniform(-1.0, 1.0, m)
        y.pb, y.px0 = y.b[perm], y.x0[perm]
        y.b_rowptr, y.b_colind, pos = M.host_permute(rowptr, colind, perm)
        y.b_values = values[pos]
        y.lanes = M.lanes_for(rowptr, colind)
        return y
    return cached(("multicolor", name), make)


# ============================================================================================ violations of the inspect's checks
def bad_color_ptrs(color_ptr):
    cp = np.asarray(color_ptr, np.int32)
    a, b, c = cp.copy(), cp.copy(), cp.copy()
    a[0] = 1                                   # does not start at 0
    b[-1] -= 1                                 # does not end at m
    k = int(np.flatnonzero(np.diff(cp) > 0)[1])
    c[k], c[k + 1] = cp[k + 1], cp[k]          # descends
    return [a, b, c]


def bad_perms(perm):
    p = np.asarray(perm, np.int32)
    a, b, c = p.copy(), p.copy(), p.copy()
    a[3] = a[7]                                # one row twice
    b[5] = p.size                              # too large
    c[0] = -1
    return [a, b, c]


def bad_structures(rowptr, colind):
    m = rowptr.size - 1
    rp1 = rowptr.copy()
    rp1[-1] -= 1                               # offsets that do not describe nnz entries
    rp2 = rowptr.copy()
    k = int(np.flatnonzero(np.diff(rowptr) > 1)[0])
    rp2[k], rp2[k + 1] = rowptr[k + 1], rowptr[k]     # descending offsets
    ci1, ci2 = colind.copy(), colind.copy()
    ci1[len(ci1) // 2] = m                     # a column >= m
    ci2[3] = -1
    return [(rp1, colind), (rp2, colind), (rowptr, ci1), (rowptr, ci2)]


def bad_diagonals(rowptr, colind):
    """A row without a stored diagonal entry, and one with two."""
    rows = _entry_rows(rowptr)
    lens = np.diff(rowptr)
    r = int(np.flatnonzero(lens >= 3)[0])
    p = np.arange(rowptr[r], rowptr[r + 1])
    dpos = int(p[colind[p] == r][0])
    other = int(p[colind[p] != r][0])
    none = colind.copy()
    none[dpos] = colind[other]                 # the diagonal replaced by a repeat of an off-diagonal entry
    two = colind.copy()
    two[other] = r
    assert rows[dpos] == r
    return [(rowptr, none), (rowptr, two)]


def same_colour_pairs(y):
    """One coupled pair planted inside the first, a middle and the last NON-EMPTY colour: (where, rowptr, colind) with one
    off-diagonal entry of a row redirected to another row of its own colour (the first colour's rows are quiet, so there the
    entry is added)."""
    cp = np.asarray(y.color_ptr, np.int64)
    live = [c for c in range(cp.size - 1) if cp[c + 1] - cp[c] >= 2]
    out = []
    for where, c in (("first", live[0]), ("middle", live[len(live) // 2]), ("last", live[-1])):
        members = y.perm[cp[c]:cp[c + 1]].astype(np.int64)
        lens = np.diff(y.rowptr)[members]
        if (lens >= 2).any():
            r = int(members[np.flatnonzero(lens >= 2)[0]])
            mate = int(members[0] if members[0] != r else members[1])
            p = np.arange(y.rowptr[r], y.rowptr[r + 1])
            ci = y.colind.copy()
            ci[int(p[y.colind[p] != r][0])] = mate
            out.append((where, y.rowptr, ci))
        else:
            r, mate = int(members[0]), int(members[1])
            at = int(y.rowptr[r + 1])
            rp = y.rowptr.copy()
            rp[r + 1:] += 1
            out.append((where, rp, np.insert(y.colind, at, mate).astype(np.int32)))
    return out


# ============================================================================================================== shape systems
def small_system(color_sizes, k=1, seed=0, diag=(1.0, 2.0)):
    """Rows of at most k off-diagonal entries (+-1) over rows of OTHER colours, the diagonal from +-diag, integer b and x0: small
    enough chains that one sweep at any omega and two at omega = 1 stay exact (tests/test_gs_cpu.py).  color_sizes may hold
    zeros: empty colours."""
    def make():
        rng = np.random.default_rng(seed)
        sizes = np.asarray(color_sizes, np.int64)
        ptr = np.concatenate([[0], np.cumsum(sizes)])
        m = int(ptr[-1])
        color = np.repeat(np.arange(sizes.size), sizes)
        live = np.flatnonzero(sizes > 0)
        cols = rng.integers(0, m, (m, k))
        signs = rng.choice([-1.0, 1.0], (m, k))
        dv = rng.choice(list(diag), m) * rng.choice([-1.0, 1.0], m)
        keep = (color[cols] != color[:, None]) if live.size > 1 else np.zeros((m, k), bool)
        where = rng.integers(0, 3, m)                        # the diagonal first / in the middle / last
        nk = keep.sum(1)
        at = np.choose(where, [np.zeros(m, np.int64), nk // 2, nk])
        prp = np.concatenate([[0], np.cumsum(nk + 1)])
        pc, pv = np.empty(int(prp[-1]), np.int64), np.empty(int(prp[-1]))
        rank = np.cumsum(keep, 1) - 1
        slot = prp[:-1, None] + rank + (rank >= at[:, None])
        pc[slot[keep]], pv[slot[keep]] = cols[keep], signs[keep]
        pc[prp[:-1] + at], pv[prp[:-1] + at] = np.arange(m), dv
        prow = (prp, pc, pv)
        return _finish(prow, ptr, rng.integers(-4, 5, m).astype(np.float64), rng.integers(-4, 5, m).astype(np.float64), rng)
    return cached(("small", tuple(int(s) for s in color_sizes), k, seed, tuple(diag)), make)


def shape_systems(num_cus):
    """name -> System: the sizes at which the launch arithmetic of gs_sweep changes.  All of them take 4 lanes per row (G = 4:
    64 rows per workgroup); `grid_stride` is one colour of CUs x 16 x 64 + 1 rows, so one lane group takes the grid stride and
    the software pipeline's hand-over to a next row."""
    rpb = 256 // 4
    return {
        "one_row": small_system([1]),
        "diagonal_one_colour": small_system([37]),
        "empty_first": small_system([0, 9, 5, 7], k=2, seed=1),
        "empty_middle": small_system([9, 0, 0, 5, 7], k=2, seed=2),
        "empty_last": small_system([9, 5, 7, 0], k=2, seed=3),
        "block_minus_1": small_system([rpb - 1, 3], k=2, seed=4),
        "block_exact": small_system([rpb, 3], k=2, seed=5),
        "block_plus_1": small_system([rpb + 1, 3], k=2, seed=6),
        "forty_colours": small_system([1] * 40, k=1, seed=7, diag=(1.0,)),
        "grid_stride": small_system([num_cus * 16 * rpb + 1, 8], k=1, seed=8),
    }
