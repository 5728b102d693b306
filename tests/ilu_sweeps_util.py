"""Host model and generators for ilu0_sweeps (spblas_gfx950_ilu0_sweeps, csrc/ilu0.hip): tests/test_ilu0_sweeps_cpu.py proves them
on the host, tests/test_gpu_ilu0_sweeps.py compares the device with them BIT FOR BIT.

THE DEFINITION (host_sweeps).  LU(0) = A; for k = 1 .. s every row i reads the previous iterate only:
    w = row i of A
    for q over the strict-lower entries of row i, column c ascending:
        w[c] = w[c] / LU(k-1)[c][c]                                               one division in `dtype`
        for j in the columns of row c with j > c, if j is also a column of row i:
            w[j] = fma(-w[c], LU(k-1)[c][j], w[j])                                one correctly rounded fma
    row i of LU(k) = w
host_ilu0_fma is the exact factor (IKJ) with the same two operations.  ilu_util.host_ilu0 is NOT this: it forms the product in
float64, which is no fma in fp64 and a double rounding in fp32.

THE FMA.  fma_exact rounds Fraction(w) - Fraction(mult) * Fraction(u) once (round_once).  Rational arithmetic on every update of
every family would take minutes, so host_sweeps takes the hits of one pivot step together (fma_many): the difference is formed in
the 64-bit significand of x86 long double, whose two roundings are at most 2^-63 (|w| + |mult u|) away from the exact value; where
the interval of four times that width around it rounds to ONE number of `dtype`, that number is the correctly rounded result, and
the few other hits go through fma_exact.  test_ilu0_sweeps_cpu.py compares the two routes on whole families.  Data stay finite and
far inside the normal range (checked), so division and fma are the only roundings.

FAMILIES (families()).  All have structural matches on most pivot steps, so that the iterates really differ: every generator
asserts that the iterates 1, 2, 3, 4 differ pairwise in at least 5 % of the entries -- a wrong buffer parity or a sweep too few
cannot pass.  Values are ilu_util.dominant_values.
"""
import functools
from fractions import Fraction

import numpy as np

import ilu_util as U
import ladder_tt as TT
import spblas_reference_amd as sp

ILU0_SWEEPS = sp.ilu0_sweeps     # this module models that operation: on a backend without it, it cannot be imported

DTYPES = (np.float32, np.float64)
SWEEPS = (1, 2, 3, 4)
MIN_DIFFERENT = 0.05


# ================================================================================================================== rounding
def round_once(fr, dtype):
    """The Fraction `fr`, rounded to nearest (ties to even) in fp32 / fp64, as a numpy scalar of that type."""
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return np.float64(float(fr))        # float(Fraction) is correctly rounded
    assert dtype == np.float32
    c = np.float32(float(fr))               # rounded twice: right, or one step off
    if fr == 0:
        return c
    with np.errstate(all="ignore"):
        cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    best = None
    for x in cands:
        err = abs(Fraction(float(x)) - fr)
        even = (int(U.bits(np.array([x], np.float32))[0]) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[1]):
            best = (err, even, x)
    return best[2]


def fma_exact(w, mult, u, dtype):
    """round_once(w - mult * u): what fma(-mult, u, w) returns."""
    return round_once(Fraction(float(w)) - Fraction(float(mult)) * Fraction(float(u)), dtype)


def fma_many(w, mult, u, dtype):
    """fma_exact for arrays w, u and a scalar mult (see the module docstring); all values finite."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "no extended precision on this host: use fma_exact on every hit"
    dtype = np.dtype(dtype)
    wl, ul, ml = w.astype(np.longdouble), u.astype(np.longdouble), np.longdouble(mult)
    prod = ml * ul
    diff = wl - prod
    delta = (np.abs(wl) + np.abs(prod)) * np.longdouble(2.0 ** -61)
    lo, hi = (diff - delta).astype(dtype), (diff + delta).astype(dtype)
    out = lo.copy()
    for p in np.flatnonzero(U.bits(lo) != U.bits(hi)):
        out[p] = fma_exact(w[p], mult, u[p], dtype)
    return out


# ============================================================================================================ the recurrence
@functools.lru_cache(maxsize=None)
def _steps_cached(rp_bytes, ci_bytes):
    rowptr, colind = np.frombuffer(rp_bytes, np.int32), np.frombuffer(ci_bytes, np.int32)
    diag = U.diag_positions(rowptr, colind)
    out = []
    for i in range(rowptr.size - 1):
        p0, p1 = int(rowptr[i]), int(rowptr[i + 1])
        cols = colind[p0:p1]
        row = []
        for q in range(int(diag[i]) - p0):
            k = int(cols[q])
            src = np.arange(int(diag[k]) + 1, int(rowptr[k + 1]))
            pos = np.searchsorted(cols, colind[src])
            hit = pos < cols.size
            hit[hit] = cols[pos[hit]] == colind[src][hit]
            row.append((int(diag[k]), src[hit], pos[hit]))
        out.append(row)
    return diag, out


def steps_of(rowptr, colind):
    """(diagonal positions, per row the list over its strict-lower entries q of (position of the pivot, positions of the pivot
    row's matching upper entries, in-row positions of the entries they update))."""
    return _steps_cached(np.ascontiguousarray(rowptr, np.int32).tobytes(), np.ascontiguousarray(colind, np.int32).tobytes())


def _row(a_row, row_steps, pivots, dtype, fma, drop=None):
    w = a_row.copy()
    for q, (kd, src, dst) in enumerate(row_steps):
        w[q] = w[q] / pivots[kd]
        if src.size:
            if drop is not None and drop[0] == q:
                keep = np.ones(src.size, bool)
                keep[drop[1] % src.size] = False
                src, dst = src[keep], dst[keep]
            if fma == "fraction":
                for s_, d_ in zip(src, dst):
                    w[d_] = fma_exact(w[d_], w[q], pivots[s_], dtype)
            else:
                w[dst] = fma_many(w[dst], w[q], pivots[src], dtype)
    return w


def host_sweeps(rowptr, colind, a, s, dtype, all_iterates=False, mutate=None, fma="fast"):
    """LU(s) of the definition, in `dtype` (or the list LU(0) .. LU(s)).  fma = "fraction": every update through fma_exact.
    mutate (a WRONG recurrence, for the tests of the tests): "gauss_seidel" reads the iterate being written, "from_prev" starts
    a row from the previous iterate instead of A, ("drop", i, q, n) leaves out the n-th hit of pivot step q of row i."""
    dtype = np.dtype(dtype)
    a = np.asarray(a[:colind.size]).astype(dtype)
    assert np.isfinite(a).all()
    _, steps = steps_of(rowptr, colind)
    its = [a.copy()]
    for _ in range(s):
        prev = its[-1]
        new = prev.copy() if mutate == "gauss_seidel" else np.empty_like(prev)
        for i in range(rowptr.size - 1):
            p0, p1 = int(rowptr[i]), int(rowptr[i + 1])
            start = prev if mutate == "from_prev" else a
            drop = mutate[2:] if isinstance(mutate, tuple) and mutate[0] == "drop" and mutate[1] == i else None
            with np.errstate(all="raise"):
                new[p0:p1] = _row(start[p0:p1], steps[i], new if mutate == "gauss_seidel" else prev, dtype, fma, drop)
        mag = np.abs(new[new != 0])
        assert np.isfinite(new).all() and (mag.size == 0 or (mag.min() > 1e-30 and mag.max() < 1e30)), "data leave the safe range"
        its.append(new)
    return its if all_iterates else its[-1]


def host_ilu0_fma(rowptr, colind, a, dtype, fma="fast"):
    """The exact ILU(0) in IKJ order with one division per lower entry and one correctly rounded fma per update."""
    dtype = np.dtype(dtype)
    lu = np.asarray(a[:colind.size]).astype(dtype).copy()
    _, steps = steps_of(rowptr, colind)
    for i in range(rowptr.size - 1):
        p0, p1 = int(rowptr[i]), int(rowptr[i + 1])
        with np.errstate(all="raise"):
            lu[p0:p1] = _row(lu[p0:p1], steps[i], lu, dtype, fma)
    return lu


def levels_of(rowptr, colind):
    return TT.levels_of(rowptr, colind, rowptr.size - 1, False)


def differing(x, y):
    """Share of the entries whose bits differ."""
    return float((U.bits(x) != U.bits(y)).mean())


# =============================================================================================================== generators
def mirrored(rowptr, colind):
    """The pattern with (j, i) added for every (i, j): structurally symmetric."""
    m = rowptr.size - 1
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    both = [[] for _ in range(m)]
    for i, j in zip(rows.tolist(), colind.tolist()):
        both[i].append(j)
        both[j].append(i)
    rp, ci = U.pattern_from_rows(both)
    U.check_pattern(rp, ci)
    return rp, ci


def mirrored_levels(widths, total, seed=0):
    """A structurally symmetric pattern (plus a few unmirrored upper entries) with EXACTLY `total` entries whose lower level sets
    have the given widths: ilu_util.level_pattern without upper entries, lower entries added -- first those that close a
    triangle (i reads c, c reads d: i reads d), then any row of a lower level in front -- until mirroring them gives total or
    total - 1 entries, the mirror image, and one unmirrored upper entry where the count is odd.  Upper entries change no level."""
    rng = np.random.default_rng(seed)
    rowptr, colind, lev = U.level_pattern(widths, seed=seed, lower=(1, 2), upper=(0, 0))
    m = rowptr.size - 1
    low = [set(int(c) for c in colind[rowptr[i]:rowptr[i + 1]] if c < i) for i in range(m)]
    budget = (total - m) // 2
    have = sum(len(s) for s in low)
    assert have <= budget, (have, budget)
    allowed = [np.flatnonzero((np.arange(m) < i) & (lev < lev[i])) for i in range(m)]
    room = [i for i in range(m) if allowed[i].size > len(low[i])]
    while have < budget:
        assert room, "no room for more lower entries: use more rows"
        i = room[int(rng.integers(len(room)))]
        close = sorted(set().union(*[low[c] for c in low[i]]) - low[i]) if 0 < len(low[i]) <= 6 else []
        if close:
            d = close[int(rng.integers(len(close)))]
        else:
            d = int(allowed[i][int(rng.integers(allowed[i].size))])
            while d in low[i]:
                d = int(allowed[i][int(rng.integers(allowed[i].size))])
        low[i].add(d)
        have += 1
        if len(low[i]) == allowed[i].size:
            room.remove(i)
    rows = [set(s) for s in low]
    for i in range(m):
        for c in low[i]:
            rows[c].add(i)
    count = m + sum(len(s) for s in rows)
    assert total - count in (0, 1)
    if total - count:
        i = next(i for i in range(m) if len(rows[i] | {i}) < m - i and any(j not in rows[i] for j in range(i + 1, m)))
        rows[i].add(next(j for j in range(i + 1, m) if j not in rows[i]))
    rp, ci = U.pattern_from_rows(rows)
    U.check_pattern(rp, ci)
    assert int(rp[-1]) == total and np.array_equal(levels_of(rp, ci), lev)
    return rp, ci, lev


def shape_specs(G):
    """The rungs of ilu_util.shape_specs(G) the sweeps need: strict-lower counts 0, 1, G - 1, G, G + 1, and the evenly split rows
    of G x 8 entries (the last the fast path holds) and G x 8 + 1 (the first of the long path, 4 G lower entries)."""
    all_specs = U.shape_specs(G)
    cap = U.lds_cap(G)
    out = []
    for lo in (0, 1, G - 1, G, G + 1):
        out.append(next(s for s in all_specs if s[0] == lo and max(s) < 300))
    for n in (cap, cap + 1):
        s = ((n - 1) // 2, n - 1 - (n - 1) // 2)
        assert s in all_specs
        out.append(s)
    return out


def shaped(limit, extra, seed=0):
    """ilu_util.shape_system with the rungs of shape_specs above: limit x m + extra entries, hence the lane count of that case."""
    lanes = [c[2] for c in U.lane_cases() if c[:2] == (limit, extra)][0]
    specs = shape_specs(lanes)
    rowptr, colind, front = U.shaped_pattern(specs, limit, seed=seed + limit + extra)
    if extra:
        m = rowptr.size - 1
        rowptr, colind = U.add_entry(rowptr, colind, 0, m - 1) if (m - 1) not in colind[:rowptr[1]] else \
            U.add_entry(rowptr, colind, 1, m - 1)
    m = rowptr.size - 1
    assert int(rowptr[-1]) == limit * m + extra and TT.lanes_of(int(rowptr[-1]), m) == lanes
    lens = np.diff(rowptr)[front:front + len(specs)]
    lows = (U.diag_positions(rowptr, colind) - rowptr[:-1])[front:front + len(specs)]
    cap = U.lds_cap(lanes)
    assert lens.max() == cap + 1 and cap in lens.tolist() and int(lows[lens == cap + 1][0]) >= 2 * lanes
    assert {0, 1, lanes - 1, lanes, lanes + 1} <= set(lows.tolist())
    return rowptr, colind, lanes


class Family:
    """A pattern with values, its levels and lane count, and (lazily, once) the host iterates per dtype."""

    def __init__(self, name, rowptr, colind, seed, lanes=None):
        self.name, self.rowptr, self.colind = name, rowptr, colind
        self.m, self.nnz = rowptr.size - 1, int(colind.size)
        self.values = U.dominant_values(rowptr, colind, seed=seed)
        self.levels = levels_of(rowptr, colind)
        self.n_levels = int(self.levels.max()) + 1
        self.lanes = TT.lanes_of(self.nnz, self.m)
        assert lanes is None or lanes == self.lanes, (name, lanes, self.lanes)
        self._its, self._exact = {}, {}

    def exact(self, dtype):
        """host_ilu0_fma, computed once per dtype."""
        key = np.dtype(dtype)
        if key not in self._exact:
            self._exact[key] = host_ilu0_fma(self.rowptr, self.colind, self.values, dtype)
        return self._exact[key]

    def iterates(self, dtype, upto=max(SWEEPS) + 1):
        """[LU(0) .. LU(upto)] of host_sweeps, computed once per dtype; the generator's own check runs on the first call."""
        key = np.dtype(dtype)
        have = self._its.get(key)
        if have is None or len(have) <= upto:
            have = host_sweeps(self.rowptr, self.colind, self.values, upto, dtype, all_iterates=True)
            self._its[key] = have
            if upto >= max(SWEEPS):
                for x in SWEEPS:
                    for y in SWEEPS:
                        if x < y:
                            share = differing(have[x], have[y])
                            assert share >= MIN_DIFFERENT, f"{self.name}: iterates {x} and {y} differ in {share:.1%} of the entries"
        return have


LEVEL_WIDTHS = [70, 50, 3, 2, 2, 3, 40, 40, 30, 30, 30]


def _make_families():
    fams = []
    for dims in ((6, 5, 4), (12, 12, 12)):
        rp, ci = U.laplacian7(*dims)
        fams.append(Family("laplacian%dx%dx%d" % dims, rp, ci, seed=sum(dims), lanes=4 if dims == (6, 5, 4) else 8))
    m = sum(LEVEL_WIDTHS)
    for limit, extra, lanes in U.lane_cases():
        rp, ci, _ = mirrored_levels(LEVEL_WIDTHS, limit * m + extra, seed=limit + extra)
        fams.append(Family(f"levels-{limit}m+{extra}", rp, ci, seed=limit + extra + 1, lanes=lanes))
    for limit, extra, lanes in U.lane_cases():
        if (limit, extra) in ((6, 1), (96, 0)):       # lanes 8 and 16 have their shapes at (24, 0) and (24, 1); at a mean of
            # 6 entries the filler rows around 8-lane shapes share too few columns for the iterates to differ after sweep 3
            continue
        rp, ci, lanes_ = shaped(limit, extra)
        fams.append(Family(f"shapes-{limit}m+{extra}", rp, ci, seed=limit + extra + 2, lanes=lanes_))
    assert {f.lanes for f in fams if f.name.startswith("levels")} == {4, 8, 16, 64}
    assert {f.lanes for f in fams if f.name.startswith("shapes")} == {4, 8, 16, 64}
    return fams


_FAMILIES = None


def families():
    global _FAMILIES
    if _FAMILIES is None:
        _FAMILIES = _make_families()
    return _FAMILIES


def family(name):
    return next(f for f in families() if f.name == name)


FAMILY_NAMES = ["laplacian6x5x4", "laplacian12x12x12"] + [f"levels-{l}m+{e}" for l in U.LIMITS for e in (0, 1)] + \
    ["shapes-6m+0", "shapes-24m+0", "shapes-24m+1", "shapes-96m+1"]
SMALL = ["laplacian6x5x4", "levels-6m+0", "shapes-6m+0"]       # where the all-Fraction route is affordable
