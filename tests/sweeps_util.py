"""Generators, the host recurrence and checkers for triangular_solve_sweeps (csrc/sptrsv_sweeps.hip): tests/test_sweeps_cpu.py
proves on the host that the generators hold what they claim, tests/test_gpu_sweeps.py runs them on the device.

THE RECURRENCE (host_sweeps).  T = the triangle triangular_solve reads, alpha = A's scaled() factor,
    dot       = sum of a_rc * v_c over the stored entries of row r with 0 <= c < m and c strictly inside the triangle
    row(r, v) = (b_r - alpha * dot) / (alpha * d_r)       explicit diagonal: the LAST stored diagonal entry, none stored: 0
    row(r, v) =  b_r - alpha * dot                        unit diagonal
    x0_r = row(r, 0) with dot = 0 (nothing is read),   xk_r = row(r, x(k-1)),  k = 1 ... s        (Jacobi: the PREVIOUS iterate)
restated in numpy in the given dtype, every operation rounded once, the entries of a row added one after the other in the
stored order or (perm_seed) in a random order.  It also returns the per-row scale
    S_r = max over the sweeps of (|b_r| + |alpha| sum |a_rc| |x_prev_c|) / |alpha d_r|          (float64; unit: no d_r)

DYADIC SYSTEMS (sweep_system).  Strict entries +-1, the diagonal read in {+-1, +-2}, integer b in [-4, 4], alpha in
{1, -2, 0.5}.  Up to `chain` = 4 strict entries of a row read ANY earlier row (they make the levels); the further strict entries
of the long row shapes of tests/ladder_tt.py read rows of level 0, whose iterate never changes -- so the iterates stay small
dyadic numbers: for s <= 4 every product, every partial sum in any order and both divisions are exact in float32 (the CPU test
proves it: float32 and float64, stored and permuted order, give identical values).  Entries of the OTHER triangle bring nnz / m
to the mean that selects the lane count asked for; they, diagonal entries stored before the last one and the stored diagonal of
a unit system hold NaN: a mask that leaks shows.

DOMINANT SYSTEMS (dominant_system).  Values uniform in (-1, 1), |d_r| >= 2 sum |a_rc| + 0.5 (unit: sum |a_rc| <= 1/4): the
iteration contracts by 1/2, so an error of tol * S_r per sweep sums to at most 2 tol S_r = tol S_r / (1 - 1/2).
"""
import numpy as np

import ladder_tt as TT

ALPHAS = (1.0, -2.0, 0.5)
TOL = {np.dtype(np.float32): 1e-6, np.dtype(np.float64): 1e-12}      # the project's tolerances


class SweepSystem:
    pass


def _entry_rows(rowptr):
    return np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))


# ====================================================================================================== the host recurrence
def host_sweeps(rowptr, colind, values, b, s, uplo, diag, alpha, dtype, perm_seed=None, all_iterates=False):
    """(x after s sweeps in `dtype`, S in float64).  uplo: "lower" / "upper", diag: "explicit" / "unit".  perm_seed: the strict
    entries of every row are added in a random order instead of the stored one.  all_iterates: a list of x0 ... xs instead."""
    assert uplo in ("lower", "upper") and diag in ("explicit", "unit") and s >= 0
    dtype = np.dtype(dtype)
    rowptr, colind = np.asarray(rowptr, np.int64), np.asarray(colind, np.int64)
    m = rowptr.size - 1
    rows = _entry_rows(rowptr)
    vals = np.asarray(values)[:colind.size].astype(dtype)
    inside = (colind >= 0) & (colind < m)
    strict = inside & ((colind > rows) if uplo == "upper" else (colind < rows))
    # the last stored diagonal entry of every row (none: 0)
    d = np.zeros(m, dtype)
    dp = np.flatnonzero(colind == rows)
    d[rows[dp]] = vals[dp]                      # ascending positions: the last assignment wins
    se = np.flatnonzero(strict)
    if perm_seed is not None:
        key = np.random.default_rng(perm_seed).random(se.size)
        se = se[np.lexsort((key, rows[se]))]
    sr, sc, sv = rows[se], colind[se], vals[se]
    first = np.searchsorted(sr, np.arange(m))
    cnt = np.bincount(sr, minlength=m)
    rank = np.arange(se.size) - first[sr]
    by_rank = [np.flatnonzero(rank == k) for k in range(int(cnt.max(initial=0)))]
    alpha_t = dtype.type(alpha)
    b = np.asarray(b).astype(dtype)
    unit = diag == "unit"
    absden = np.ones(m) if unit else np.abs(np.float64(alpha_t) * d.astype(np.float64))

    def finish(dot):
        with np.errstate(all="ignore"):
            v = b - alpha_t * dot
            return v if unit else v / (alpha_t * d)

    with np.errstate(all="ignore"):
        S = np.abs(b.astype(np.float64)) / absden
    x = finish(np.zeros(m, dtype))
    its = [x]
    for _ in range(s):
        dot = np.zeros(m, dtype)
        with np.errstate(all="ignore"):
            for e in by_rank:
                dot[sr[e]] = dot[sr[e]] + sv[e] * x[sc[e]]
            mag = np.bincount(sr, weights=np.abs(sv.astype(np.float64) * x[sc].astype(np.float64)), minlength=m)
            S = np.fmax(S, (np.abs(b.astype(np.float64)) + abs(float(alpha_t)) * mag) / absden)
        x = finish(dot)
        its.append(x)
    return (its if all_iterates else x), S


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def bit_violations(got, want, what="", limit=4):
    """Messages (empty: passes): got must equal want bit for bit, except that -0.0 and +0.0 count as equal (b_r - alpha * dot
    with a contracted multiply-add may round an exact zero to the other sign)."""
    got = np.asarray(got)
    want = np.asarray(want).astype(got.dtype)
    if got.shape != want.shape:
        return [f"{what}: shape {got.shape} != {want.shape}"]
    bad = np.flatnonzero((bits(got) != bits(want)) & ~((got == 0) & (want == 0)))
    return [f"{what}: {bad.size} elements differ, first at {bad[:limit].tolist()}: {got[bad[:limit]].tolist()} != "
            f"{want[bad[:limit]].tolist()}"] if bad.size else []


def bound_violations(got, ref64, S, dtype, what="", limit=4):
    """Messages (empty: passes): |got_r - ref_r| <= 2 tol S_r for EVERY row (a non-finite element fails)."""
    got = np.asarray(got, np.float64)
    bound = 2.0 * TOL[np.dtype(dtype)] * S
    with np.errstate(all="ignore"):
        bad = np.flatnonzero(~(np.abs(got - ref64) <= bound))
    return [f"{what}: {bad.size} rows miss 2 tol S_r, first at {bad[:limit].tolist()}: error "
            f"{np.abs(got - ref64)[bad[:limit]].tolist()} > {bound[bad[:limit]].tolist()}"] if bad.size else []


# ========================================================================================================== dyadic systems
def sweep_system(shapes, n_level0, lanes, upper=False, unit=False, alpha=1.0, seed=0, chain=4):
    """A dyadic system (module docstring) of n_level0 rows without strict entries and one row per shape of `shapes`
    (ladder_tt.Shape: strict entries, in-row positions of the stored diagonal entries), dealt to random indices behind a block
    of eight level-0 rows; nnz / m selects `lanes` lanes per row.  Returns a SweepSystem: m, nnz, rowptr, colind (int32),
    values, b (float64), uplo, diag, alpha, lanes, levels (the level of every row), shape_of (name per row)."""
    rng = np.random.default_rng(seed)
    ns = len(shapes)
    m = n_level0 + ns
    assert n_level0 >= 10
    # index of every shaped row: anywhere in [8, m - 1); the last index is a plain level-0 row (it has no other triangle)
    shaped_at = np.sort(rng.choice(np.arange(8, m - 1), ns, replace=False)) if ns else np.zeros(0, np.int64)
    shape_at = {int(i): shapes[k] for k, i in enumerate(rng.permutation(shaped_at))}
    is_l0 = np.ones(m, bool)
    is_l0[shaped_at] = False
    l0_rows = np.flatnonzero(is_l0)
    strict_n = np.zeros(m, np.int64)
    n_diag = np.ones(m, np.int64)
    need = np.zeros(m, np.int64)            # other-triangle entries a row needs for its diagonal positions
    for i, sh in shape_at.items():
        assert sh.strict >= 1 and (unit or len(sh.dpos) > 0)
        strict_n[i] = sh.strict
        n_diag[i] = len(sh.dpos)
        far = max([p for p in sh.dpos if p != "last"], default=-1)
        need[i] = max(0, far + 1 - sh.strict - len(sh.dpos) + (1 if "last" in sh.dpos else 0))
    base = int((strict_n + n_diag + need).sum())
    target = max(base, int(round(TT.TARGET_MEAN[lanes] * m)))
    pad = need.copy()
    extra = target - base
    takers = np.arange(m - 1)                  # every row but the last has columns of the other triangle
    pad[takers] += extra // takers.size
    pad[takers[:extra % takers.size]] += 1
    assert pad[m - 1] == 0
    cols, vals, shape_of = [], [], np.array(["level0"] * m, dtype=object)
    for i in range(m):
        sh = shape_at.get(i)
        length = int(strict_n[i] + n_diag[i] + pad[i])
        dpos = [0] if sh is None and not pad[i] else (["last"] if sh is None else list(sh.dpos))
        dpos = [length - 1 if p == "last" else p for p in dpos]
        assert all(0 <= p < length for p in dpos) and len(set(dpos)) == len(dpos)
        c = np.full(length, -1, np.int64)
        v = np.full(length, np.nan)
        c[dpos] = i
        if dpos and not unit:
            v[dpos[-1]] = rng.choice([-2.0, -1.0, 1.0, 2.0])
        free = np.flatnonzero(c < 0)
        st = rng.choice(free, int(strict_n[i]), replace=False) if strict_n[i] else np.zeros(0, np.int64)
        ot = np.setdiff1d(free, st)
        if st.size:
            shape_of[i] = sh.name
            k = min(chain, st.size)
            c[st[:k]] = rng.integers(0, i, k)                                   # any earlier row: these make the levels
            earlier_l0 = l0_rows[:np.searchsorted(l0_rows, i)]
            c[st[k:]] = earlier_l0[rng.integers(0, earlier_l0.size, st.size - k)]
            v[st] = rng.choice([-1.0, 1.0], st.size)
        if ot.size:
            c[ot] = rng.integers(i + 1, m, ot.size)
        cols.append(c)
        vals.append(v)
    lens = np.array([c.size for c in cols])
    colind = np.concatenate(cols)
    values = np.concatenate(vals)
    row_of = np.repeat(np.arange(m), lens)
    b = rng.integers(-4, 5, m).astype(np.float64)
    if upper:    # the index mirror
        row_of, colind, b = m - 1 - row_of, m - 1 - colind, b[::-1].copy()
        shape_of = shape_of[::-1].copy()
        perm = np.argsort(row_of, kind="stable")
        row_of, colind, values = row_of[perm], colind[perm], values[perm]
    y = SweepSystem()
    y.m, y.nnz = m, int(colind.size)
    y.rowptr = np.concatenate([[0], np.cumsum(np.bincount(row_of, minlength=m))]).astype(np.int32)
    y.colind, y.values, y.b = colind.astype(np.int32), values, b
    y.uplo, y.diag, y.alpha, y.lanes = "upper" if upper else "lower", "unit" if unit else "explicit", float(alpha), lanes
    y.shape_of = shape_of
    y.levels = TT.levels_of(y.rowptr, y.colind, m, upper)
    assert y.nnz == target and TT.lanes_of(y.nnz, m) == lanes, (y.nnz, m, TT.lanes_of(y.nnz, m), lanes)
    return y


def dyadic_system(m, lanes, upper=False, unit=False, alpha=1.0, seed=0):
    """m rows, at most 4 strict entries per row (1 ... 4 in turn, the diagonal last), a fifth of the rows at level 0."""
    n0 = max(10, m // 5)
    shapes = [TT.Shape(1 + k % 4) for k in range(m - n0)]
    return sweep_system(shapes, n0, lanes, upper, unit, alpha, seed)


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def shape_sweep_system(lanes, upper, unit):
    """The row shapes of ladder_tt.row_shapes(lanes, unit) -- strict counts 0 ... 2 G + 2 and beyond, the diagonal in every lane
    slot, stored twice, not stored -- on about 600 rows."""
    def make():
        shapes = TT.row_shapes(lanes, unit)
        return sweep_system(shapes, max(600 - len(shapes), 320), lanes, upper, unit, ALPHAS[(lanes + upper + 2 * unit) % 3],
                            seed=500 + lanes + 2 * upper + unit)
    return cached(("shapes", lanes, upper, unit), make)


# ======================================================================================================== dominant systems
def dominant_system(m, per_row, upper=False, unit=False, alpha=1.0, seed=0, window=None):
    """Random values with |d_r| >= 2 sum |a_rc| + 0.5 (unit: sum |a_rc| <= 1/4); per_row strict entries in rows that have as
    many earlier rows (inside `window` rows before r when given: deeper levels), one entry of the other triangle per row."""
    rng = np.random.default_rng(seed)
    cols, vals = [], []
    for i in range(m):
        k = min(per_row, i)
        lo = 0 if window is None else max(0, i - window)
        c = rng.integers(lo, i, k) if k else np.zeros(0, np.int64)
        a = rng.uniform(-1.0, 1.0, k)
        if unit:
            a *= 0.25 / max(np.abs(a).sum(), 0.25)
            dv = np.nan
        else:
            dv = (2.0 * np.abs(a).sum() + 0.5 + rng.random()) * rng.choice([-1.0, 1.0])
        oc = rng.integers(i + 1, m, 1) if i < m - 1 else np.zeros(0, np.int64)
        c = np.concatenate([c, oc, [i]])
        a = np.concatenate([a, np.full(oc.size, np.nan), [dv]])
        p = rng.permutation(c.size)
        cols.append(c[p])
        vals.append(a[p])
    lens = np.array([c.size for c in cols])
    colind, values = np.concatenate(cols), np.concatenate(vals)
    row_of = np.repeat(np.arange(m), lens)
    b = rng.uniform(-1.0, 1.0, m)
    if upper:
        row_of, colind, b = m - 1 - row_of, m - 1 - colind, b[::-1].copy()
        perm = np.argsort(row_of, kind="stable")
        row_of, colind, values = row_of[perm], colind[perm], values[perm]
    y = SweepSystem()
    y.m, y.nnz = m, int(colind.size)
    y.rowptr = np.concatenate([[0], np.cumsum(np.bincount(row_of, minlength=m))]).astype(np.int32)
    y.colind, y.values, y.b = colind.astype(np.int32), values, b
    y.uplo, y.diag, y.alpha = "upper" if upper else "lower", "unit" if unit else "explicit", float(alpha)
    y.lanes = TT.lanes_of(y.nnz, m)
    y.levels = TT.levels_of(y.rowptr, y.colind, m, upper)
    return y


def chain_system(m=70, upper=False):
    """Bidiagonal: d = 1, off-diagonal 1, b = e_0 (upper: the mirror).  One row per level; xs_r = (-1)^r on rows <= s, 0 below."""
    rowptr = np.concatenate([[0, 1], 1 + 2 * np.arange(1, m)]).astype(np.int32)
    colind = np.concatenate([[0], np.stack([np.arange(m - 1), np.arange(1, m)], axis=1).ravel()]).astype(np.int64)
    values = np.ones(colind.size)
    b = np.zeros(m)
    b[0] = 1.0
    row_of = _entry_rows(rowptr)
    if upper:
        row_of, colind, b = m - 1 - row_of, m - 1 - colind, b[::-1].copy()
        perm = np.argsort(row_of, kind="stable")
        colind = colind[perm]
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(row_of, minlength=m))]).astype(np.int32)
    y = SweepSystem()
    y.m, y.nnz, y.rowptr, y.colind, y.values, y.b = m, int(colind.size), rowptr, colind.astype(np.int32), values, b
    y.uplo, y.diag, y.alpha, y.lanes = "upper" if upper else "lower", "explicit", 1.0, 4
    y.levels = TT.levels_of(rowptr, colind, m, upper)
    return y


def chain_closed_form(m, s, upper=False):
    r = np.arange(m)
    x = np.where(r <= s, (-1.0) ** r, 0.0)
    return x[::-1].copy() if upper else x


def of_tt(sysm):
    """A ladder_tt System (shape_system, width_system, sequence_system) as the arguments of host_sweeps / the device call."""
    y = SweepSystem()
    y.m, y.nnz, y.rowptr, y.colind, y.values, y.b = sysm.m, sysm.nnz, sysm.rowptr, sysm.colind, sysm.exact_values, sysm.b
    y.uplo, y.diag, y.alpha, y.lanes = "upper" if sysm.upper else "lower", "unit" if sysm.unit else "explicit", sysm.alpha, sysm.lanes
    y.levels = sysm.level
    y.x_true = sysm.x_true
    return y


def reference(y, s, dtype, **kw):
    return host_sweeps(y.rowptr, y.colind, y.values, y.b, s, y.uplo, y.diag, y.alpha, dtype, **kw)
