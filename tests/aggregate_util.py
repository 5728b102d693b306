"""Generators, the host model and the checkers of aggregate / coarsen (tests/test_aggregate_cpu.py proves them on the host,
tests/test_gpu_aggregate.py compares the device with them bit for bit, tests/test_gpu_aggregate_stream.py runs STREAM_CASES).

The model restates what csrc/aggregate.hip documents: the strength rule in numpy OF THE VALUE TYPE (products only, in the
documented order), the rounds on whole arrays (T1, T2, roots, two propagation steps -- every step reads the arrays of the step
before, as separate launches do), the two assignment phases and the ordered sums of coarsen.  model(..., mistake=...) seeds
the mistakes the ladder must catch.  greedy_roots is the sequential algorithm the rounds must equal: greedy MIS on the square
of the strong graph in descending key order.  check_aggregation / check_coarse look at a result alone and share no code with
the model: they walk Python sets and scalars of the value type."""
import functools

import numpy as np
import scipy.sparse as sps

import ilu_util as U
import multicolor_util as MC

keys = MC.keys
lanes_for = MC.lanes_for
MISTAKES = ("t_not_through_covered", "one_sided", "phase2_reads_phase2", "phase2_smallest_key", "sums_descending")


# ============================================================================================================== generators
def _rows(rowptr):
    return np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))


def with_values(pattern, diag=4.0, off=-1.0):
    """(rowptr, colind, values): `diag` on the diagonal entries, `off` elsewhere."""
    rowptr, colind = pattern
    return rowptr, colind, np.where(colind == _rows(rowptr), diag, off).astype(np.float64)


def path(n):
    return with_values(MC.chain(n), 2.0)


def grid5(nx, ny):
    return with_values(MC.grid5(nx, ny), 4.0)


def lap7(n):
    return with_values(MC.laplacian7(n, n, n), 6.0)


def hub(leaves):
    return with_values(MC.star(leaves), float(leaves))


def random_graph(m, per_row, seed):
    """per_row distinct columns per row (the diagonal among them), unsymmetric; off-diagonal values of magnitude 1 / 2 / 4 with
    random signs, diagonal 8: theta = 0.25 keeps |a| >= 2 (a^2 >= 4 = (1/16 * 8) * 8), drops |a| = 1."""
    rowptr, colind = MC.random_rows(m, per_row, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    v = rng.choice([1.0, 2.0, 4.0], colind.size) * rng.choice([-1.0, 1.0], colind.size)
    return rowptr, colind, np.where(colind == _rows(rowptr), 8.0, v)


def upper_bidiagonal(n):
    """a_ii and a_i,i+1 only: every edge of row i + 1 to row i comes from A^T."""
    rows = [[i, i + 1] if i + 1 < n else [i] for i in range(n)]
    return with_values(MC.from_rows(rows), 2.0)


def repeated_entries(m=60, seed=4):
    """Unsorted rows with the diagonal stored twice (FIRST 4, then 1000: only the first counts) and neighbours repeated."""
    rowptr, colind = MC.loops_and_duplicates(m, seed)
    v = np.full(colind.size, -1.0)
    rows = _rows(rowptr)
    first = np.ones(colind.size, bool)
    seen = set()
    for p in np.flatnonzero(colind == rows):
        first[p] = int(rows[p]) not in seen
        seen.add(int(rows[p]))
    v[colind == rows] = 1000.0
    v[(colind == rows) & first] = 4.0
    return rowptr, colind, v


def diagonal(n):
    return with_values(MC.diagonal_only(n), 3.0)


def empty_rows(n=50):
    """A path on the even vertices; the odd rows are empty (no entry, no diagonal)."""
    rows = [[] for _ in range(n)]
    for i in range(0, n, 2):
        rows[i] = [j for j in (i - 2, i, i + 2) if 0 <= j < n]
    return with_values(MC.from_rows(rows), 2.0)


def anisotropic(nx, ny, weak=0.0078125):
    """5-point operator, -1 along x and -weak along y, diagonal 2 + 2 weak: with theta = 0.25 only the x couplings are strong."""
    rowptr, colind = MC.grid5(nx, ny)
    rows = _rows(rowptr)
    d = np.abs(colind - rows)
    return rowptr, colind, np.where(d == 0, 2.0 + 2.0 * weak, np.where(d == 1, -1.0, -weak))


def threshold(dtype):
    """A path of 12 rows, diagonal 4, theta = 0.25: t2 = 1/16 and (t2 * 4) * 4 = 1.  Entries (i, i + 1) and (i + 1, i) are 1 for
    even i -- exactly on the threshold, strong -- and the largest value of the type below 1 for odd i: one ulp short, weak."""
    rowptr, colind, v = path(12)
    rows = _rows(rowptr)
    lo = np.minimum(rows, colind)
    below = np.nextafter(np.dtype(dtype).type(1), np.dtype(dtype).type(0))
    v = np.where(colind == rows, 4.0, np.where(lo % 2 == 0, 1.0, np.float64(below)))
    return rowptr, colind, v


def lane_rungs():
    """[(G, m, (rowptr, colind, values))]: every team width of lanes_per_row, m at k * (256 / G) - 1 / exact / + 1."""
    out = []
    for per_row, G, k in ((5, 4, 2), (10, 8, 2), (30, 16, 3), (100, 64, 32)):
        for dm in (-1, 0, 1):
            m = k * (256 // G) + dm
            g = random_graph(m, per_row, seed=per_row + dm)
            assert lanes_for(g[0], g[1]) == G
            out.append((G, m, g))
    return out


# ================================================================================================================ the model
def strength(rowptr, colind, values, theta, dtype):
    """(strong[nnz] bool, d[m]) in numpy of the value type: a*a >= (t2 * |d_i|) * |d_j| with t2 = T(theta * theta)."""
    T = np.dtype(dtype).type
    m = rowptr.size - 1
    rows = _rows(rowptr)
    v = np.asarray(values[:colind.size]).astype(dtype)
    d = np.zeros(m, dtype)
    on = np.flatnonzero(colind == rows)
    r, first = np.unique(rows[on], return_index=True)
    d[r] = v[on[first]]
    t2 = T(float(theta) * float(theta))
    with np.errstate(all="ignore"):
        rhs = (t2 * np.abs(d[rows])) * np.abs(d[colind])
        strong = (colind != rows) & (v * v >= rhs)
    return strong, d


def _edges(rowptr, colind, strong, one_sided=False):
    """(src, dst): dst is a neighbour of src; both directions of every strong entry unless one_sided."""
    rows = _rows(rowptr)
    r, c = rows[strong], colind[strong].astype(np.int64)
    if one_sided:
        return r, c
    return np.concatenate([r, c]), np.concatenate([c, r])


def _spread(x, src, dst):
    """out[v] = max of x over {v} + N(v)."""
    out = x.copy()
    np.maximum.at(out, src, x[dst])
    return out


def model(rowptr, colind, values, theta=0.0, dtype=np.float32, mistake=None):
    """dict(agg, root, n_agg, rounds, largest, smallest, singletons, strong_entries, state): the rounds as the device runs
    them."""
    assert mistake is None or mistake in MISTAKES
    m = rowptr.size - 1
    strong, _ = strength(rowptr, colind, values, theta, dtype)
    src, dst = _edges(rowptr, colind, strong, one_sided=mistake == "one_sided")
    key = keys(m)
    state = np.zeros(m, np.int8)
    rounds = 0
    while (state == 0).any():
        t1 = _spread(np.where(state == 0, key, np.uint64(0)), src, dst)
        if mistake == "t_not_through_covered":
            t1 = np.where(state == 0, t1, np.uint64(0))
        t2 = _spread(t1, src, dst)
        state = np.where((state == 0) & (t2 == key), 1, state).astype(np.int8)
        near = _spread((state == 1).astype(np.int8), src, dst)
        near2 = _spread(near, src, dst)
        state = np.where((state == 0) & (near2 > 0), 2, state).astype(np.int8)
        rounds += 1
        assert rounds <= m
    root = np.flatnonzero(state == 1).astype(np.int32)
    ids = (np.cumsum(state == 1) - 1).astype(np.int64)
    agg1 = _spread(np.where(state == 1, ids, -1), src, dst)
    agg = agg1.copy()
    rest = np.flatnonzero(agg1 < 0)
    if mistake == "phase2_reads_phase2":
        for v in rest:                                   # in place: a later vertex sees what an earlier one just took
            nb = dst[src == v]
            nb = nb[agg[nb] >= 0]
            agg[v] = agg[nb[np.argmax(key[nb])]] if nb.size else -1
    elif rest.size:
        if mistake == "phase2_smallest_key":
            inv = np.where(agg1 >= 0, ~key, np.uint64(0))
            best = np.zeros(m, np.uint64)
            np.maximum.at(best, src, inv[dst])
            best = ~best
        else:
            best = np.zeros(m, np.uint64)
            np.maximum.at(best, src, np.where(agg1 >= 0, key, np.uint64(0))[dst])
        agg[rest] = agg1[(best[rest] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    sizes = np.bincount(agg[agg >= 0], minlength=root.size)
    return dict(agg=agg.astype(np.int32), root=root, n_agg=int(root.size), rounds=rounds, state=state,
                largest=int(sizes.max()) if m else 0, smallest=int(sizes.min()) if m else 0,
                singletons=int((sizes == 1).sum()), strong_entries=int(strong.sum()))


def greedy_roots(rowptr, colind, values, theta=0.0, dtype=np.float32):
    """Sequential greedy MIS on the square of the strong graph, vertices visited in descending key order."""
    m = rowptr.size - 1
    strong, _ = strength(rowptr, colind, values, theta, dtype)
    src, dst = _edges(rowptr, colind, strong)
    A = sps.csr_matrix((np.ones(src.size), (src, dst)), shape=(m, m))
    G2 = (A + A @ A).tocsr()
    is_root = np.zeros(m, bool)
    for v in np.argsort(keys(m))[::-1]:
        nb = G2.indices[G2.indptr[v]:G2.indptr[v + 1]]
        if not is_root[nb[nb != v]].any():
            is_root[v] = True
    return np.flatnonzero(is_root).astype(np.int32)


def host_coarsen(rowptr, colind, values, agg, n_agg, dtype, mistake=None):
    """(c_rowptr, c_colind, c_values, seg_ptr, order): entries sorted by (agg[row], agg[col], position); every coarse value is
    its terms added one after the other in that order, in the value type, from the first term."""
    nnz = int(colind.size)
    agg = np.asarray(agg, np.int64)
    rows = _rows(rowptr)
    I, J = agg[rows], agg[colind]
    order = np.lexsort((np.arange(nnz), J, I))
    Is, Js = I[order], J[order]
    head = np.ones(nnz, bool)
    head[1:] = (Is[1:] != Is[:-1]) | (Js[1:] != Js[:-1])
    seg = np.flatnonzero(head)
    seg_ptr = np.append(seg, nnz).astype(np.int64)
    c_rowptr = np.concatenate([[0], np.cumsum(np.bincount(Is[seg], minlength=n_agg))]).astype(np.int32)
    v = np.asarray(values[:nnz]).astype(dtype)[order]
    lens = np.diff(seg_ptr)
    first = seg_ptr[:-1] if mistake != "sums_descending" else seg_ptr[1:] - 1
    step = 1 if mistake != "sums_descending" else -1
    s = v[first].copy() if nnz else np.zeros(0, dtype)
    with np.errstate(all="ignore"):
        for k in range(1, int(lens.max()) if nnz else 0):
            sel = lens > k
            s[sel] = s[sel] + v[first[sel] + step * k]
    return c_rowptr, Js[seg].astype(np.int32), s, seg_ptr.astype(np.int32), order.astype(np.int32)


def dense_galerkin(rowptr, colind, values, agg, n_agg):
    """P^T A P as a dense float64 array."""
    m = rowptr.size - 1
    A = sps.csr_matrix((np.asarray(values[:colind.size], np.float64), colind.astype(np.int64), rowptr.astype(np.int64)),
                       shape=(m, m))
    P = sps.csr_matrix((np.ones(m), (np.arange(m), np.asarray(agg, np.int64))), shape=(m, n_agg))
    return (P.T @ A @ P).toarray()


@functools.lru_cache(maxsize=None)
def through_covered():
    """(rowptr, colind, values, u, w): a small graph in which, after the first round, two undecided vertices u and w are joined
    only through a covered vertex, and in which a T1 that does not pass through covered vertices makes both of them roots.
    Found by a fixed search over small random graphs (host-checked by tests/test_aggregate_cpu.py)."""
    for seed in range(2000):
        rng = np.random.default_rng(seed)
        m = 14
        edges = [(int(a), int(b)) for a, b in rng.integers(0, m, (16, 2)) if a != b]
        g = with_values(MC.from_edges(m, edges), 4.0)
        good, bad = model(*g), model(*g, mistake="t_not_through_covered")
        if np.array_equal(good["root"], bad["root"]):
            continue
        adj = {v: set() for v in range(m)}
        for a, b in edges:
            adj[a].add(b)
            adj[b].add(a)
        extra = sorted(set(bad["root"].tolist()) - set(good["root"].tolist()))
        for u in extra:
            for w in bad["root"].tolist():
                if w != u and w not in adj[u] and adj[u] & adj[w]:
                    return g + (u, w)
    raise AssertionError("no such graph found")


# ============================================================================================================ the checkers
def check_aggregation(rowptr, colind, values, theta, dtype, agg, root, n_agg):
    """Messages (empty: passes), from the result alone.  The strong graph is rebuilt here entry by entry with scalars of the
    value type."""
    T = np.dtype(dtype).type
    m = rowptr.size - 1
    agg, root = np.asarray(agg), np.asarray(root)
    out = []
    if agg.size != m or root.size != n_agg:
        return ["a result has the wrong length"]
    if m and (agg.min() < 0 or agg.max() >= n_agg):
        return ["an entry of agg lies outside [0, n_agg): a vertex is left undecided"]
    d = [T(0)] * m
    for i in range(m):
        for p in range(rowptr[i], rowptr[i + 1]):
            if colind[p] == i:
                d[i] = T(values[p])
                break
    t2 = T(float(theta) * float(theta))
    adj = [set() for _ in range(m)]
    with np.errstate(all="ignore"):
        for i in range(m):
            for p in range(rowptr[i], rowptr[i + 1]):
                j = int(colind[p])
                a = T(values[p])
                if j != i and bool(a * a >= (t2 * abs(d[i])) * abs(d[j])):
                    adj[i].add(j)
                    adj[j].add(i)
    rootset = set(int(r) for r in root)
    if len(rootset) != n_agg or (n_agg > 1 and not (np.diff(root) > 0).all()):
        out.append("the roots do not ascend")
    for k, r in enumerate(root):
        if agg[r] != k:
            out.append(f"root {int(r)} is not in aggregate {k}: the ids do not ascend with the root index")
            break
    for r in rootset:
        ball = set(adj[r])
        for u in adj[r]:
            ball |= adj[u]
        ball.discard(r)
        if ball & rootset:
            out.append(f"roots {r} and {min(ball & rootset)} are closer than 3")
            break
    for v in range(m):
        r = int(root[agg[v]])
        if v == r or r in adj[v]:
            continue
        if not any(agg[u] == agg[v] and (u == r or r in adj[u]) for u in adj[v]):
            out.append(f"vertex {v} is neither its root, nor next to it, nor next to a phase-1 member of aggregate {int(agg[v])}")
            break
    # maximality: every vertex lies within distance 2 of a root
    for v in range(m):
        ball = {v} | adj[v]
        for u in adj[v]:
            ball |= adj[u]
        if not ball & rootset:
            out.append(f"vertex {v} has no root within distance 2: the set is not maximal")
            break
    return out


def check_coarse(n_agg, c_rowptr, c_colind):
    out = []
    c_rowptr, c_colind = np.asarray(c_rowptr), np.asarray(c_colind)
    if c_rowptr.size != n_agg + 1 or c_rowptr[0] != 0 or c_rowptr[-1] != c_colind.size or (np.diff(c_rowptr) < 0).any():
        return ["the row offsets do not describe the entries"]
    if c_colind.size and (c_colind.min() < 0 or c_colind.max() >= n_agg):
        out.append("a column lies outside [0, n_agg)")
    for i in range(n_agg):
        if not (np.diff(c_colind[c_rowptr[i]:c_rowptr[i + 1]]) > 0).all():
            out.append(f"row {i}: the columns are not ascending and duplicate free")
            break
    return out


# ===================================================================================================== stream-order cases
# What tests/test_gpu_aggregate_stream.py runs, by exported name (the aggregation names are not in the table of
# tests/stream_util.py; tests/test_aggregate_cpu.py asserts that every one of them is listed here).
STREAM_CASES = {
    "coarsen_values_late_inputs": ("coarsen",),
    "coarsen_structure_late": ("coarsen_structure",),
    "prolongator_late": ("aggregate",),
    "coarsen_plan_dies_behind_its_last_use": ("coarsen", "coarsen_inspect"),
    "aggregate_plan_dies_behind_its_last_use": ("aggregate",),
}
STREAM_EXEMPT = {"aggregate_t": "the holder of an aggregation (its prolongator() is covered under aggregate)"}
