"""Generators, the host model and the checkers of the multicolour ordering and the symmetric permutation
(tests/test_multicolor_cpu.py proves them on the host, tests/test_gpu_multicolor.py compares the device with them).

The device colours by rounds (Jones-Plassmann with fixed priorities, csrc/multicolor.hip).  The model here is deliberately NOT a
restatement of the rounds: it is sequential greedy colouring in descending key order, which the rounds must reproduce bit for bit
whatever their schedule -- a vertex takes its colour after all its neighbours of larger key and before all of smaller key.
check_order looks at the result alone and shares no code with the model."""
import numpy as np
import scipy.sparse as sps

import ilu_util as U
import ladder_tt as TT


# ===================================================================================================================== key
def keys(m):
    """key(v) = (uint64(h(v)) << 32) | v with h(v) = mix(uint32(v + 1) * 0x9E3779B1), all in 32-bit wraparound arithmetic."""
    v = np.arange(m, dtype=np.uint64)
    M = np.uint64(0xFFFFFFFF)
    x = ((v + np.uint64(1)) * np.uint64(0x9E3779B1)) & M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M
    x ^= x >> np.uint64(16)
    return (x << np.uint64(32)) | v


def lanes_for(rowptr, colind):
    """Lanes per vertex: the library's one rule, spb::lanes_per_row, as tests/ladder_tt.py reads it from csrc/sptrsv.hip."""
    return TT.lanes_of(colind.size, rowptr.size - 1)


# ============================================================================================================== generators
def from_rows(rows):
    """CSR pattern of the given column lists, kept exactly as given (order, repeats, self loops)."""
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    colind = np.asarray([c for r in rows for c in r], dtype=np.int32).reshape(-1)
    return rowptr, colind


def from_edges(m, edges, diagonal=True):
    """Symmetric pattern with sorted rows: both directions of every edge, plus the diagonal."""
    rows = [set([i]) if diagonal else set() for i in range(m)]
    for a, b in edges:
        rows[a].add(b)
        rows[b].add(a)
    return from_rows([sorted(r) for r in rows])


def diagonal_only(m):
    return from_rows([[i] for i in range(m)])


def chain(m):
    return from_edges(m, [(i, i + 1) for i in range(m - 1)])


def ring(m):
    return from_edges(m, [(i, (i + 1) % m) for i in range(m)])


def grid5(nx, ny):
    idx = lambda x, y: y * nx + x
    e = [(idx(x, y), idx(x + 1, y)) for y in range(ny) for x in range(nx - 1)]
    e += [(idx(x, y), idx(x, y + 1)) for y in range(ny - 1) for x in range(nx)]
    return from_edges(nx * ny, e)


def laplacian7(nx, ny, nz):
    return U.laplacian7(nx, ny, nz)


def star(leaves):
    return from_edges(leaves + 1, [(0, i) for i in range(1, leaves + 1)])


def complete(m):
    return from_rows([list(range(m)) for _ in range(m)])


def strict_lower(rowptr, colind):
    """Only the entries left of the diagonal: every edge is stored in one direction, no diagonal."""
    rows = U._rows_of(rowptr)
    keep = colind < rows
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=rowptr.size - 1))]).astype(np.int32)
    return rp, colind[keep].astype(np.int32)


def one_sided(m=40, seed=3):
    """The diagonal and, for some pairs i < j, a_ji WITHOUT a_ij."""
    rng = np.random.default_rng(seed)
    rows = [[i] for i in range(m)]
    for j in range(1, m):
        for i in rng.choice(j, min(j, 2), replace=False):
            rows[j].append(int(i))
    return from_rows(rows)


def loops_and_duplicates(m=60, seed=4):
    """Unsorted rows with the self loop stored twice and some neighbours repeated, some of them in one direction only."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(m):
        nb = [int(c) for c in rng.choice(m, 4, replace=False)]
        rows.append([i] + nb + [nb[0], i, nb[2], nb[0]])
    return from_rows(rows)


def random_rows(m, per_row, seed=0):
    """per_row distinct random columns in every row (the diagonal among them), unsymmetric."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(m):
        c = set(int(x) for x in rng.choice(m, per_row - 1, replace=False))
        c.add(i)
        rows.append(sorted(c))
    return from_rows(rows)


def slow_path(m=300):
    """A path whose j-th vertex is the vertex of the j-th largest key: every vertex but the first waits for its predecessor, so
    a round that sees no colour of its own launch frees exactly one vertex."""
    order = np.argsort(keys(m))[::-1]
    return from_edges(m, [(int(order[j]), int(order[j + 1])) for j in range(m - 1)])


def lane_patterns():
    """(lanes, pattern) with nnz / m in each band of the lane rule."""
    out = []
    for per_row, lanes in ((5, 4), (10, 8), (30, 16), (100, 64)):
        p = random_rows(260, per_row, seed=per_row)
        assert lanes_for(*p) == lanes
        out.append((lanes, p))
    return out


def fixtures():
    """name -> (rowptr, colind): every pattern the colouring is compared on."""
    f = {
        "empty": (np.zeros(1, np.int32), np.zeros(0, np.int32)),
        "one_row": diagonal_only(1),
        "diagonal_5": diagonal_only(5),
        "chain_70": chain(70),
        "grid5_9x7": grid5(9, 7),
        "lap7_5x4x3": laplacian7(5, 4, 3),
        "lap7_12": laplacian7(12, 12, 12),
        "star_300": star(300),
        "grid5_9x7_strict_lower": strict_lower(*grid5(9, 7)),
        "one_sided": one_sided(),
        "loops_and_duplicates": loops_and_duplicates(),
        "random_2000x6": random_rows(2000, 6, seed=1),
        "slow_path_300": slow_path(300),
    }
    for m in (255, 256, 257, 1023, 1024, 1025):
        f[f"ring_{m}"] = ring(m)
    for m in (17, 65, 130):
        f[f"complete_{m}"] = complete(m)
    for lanes, p in lane_patterns():
        f[f"lanes_{lanes}"] = p
    return f


# ================================================================================================================ the model
def neighbours(rowptr, colind):
    """Symmetrised adjacency (A + A^T without the diagonal, repeats merged) as a scipy CSR matrix."""
    m = rowptr.size - 1
    if m == 0:
        return sps.csr_matrix((0, 0))
    A = sps.csr_matrix((np.ones(colind.size), colind.astype(np.int64), rowptr.astype(np.int64)), shape=(m, m))
    S = (A + A.T).tolil()
    S.setdiag(0)
    S = S.tocsr()
    S.eliminate_zeros()
    return S


def model_colors(rowptr, colind):
    """Sequential greedy colouring, vertices visited in descending key order."""
    m = rowptr.size - 1
    S = neighbours(rowptr, colind)
    color = np.full(m, -1, np.int32)
    for v in np.argsort(keys(m))[::-1]:
        used = set(color[S.indices[S.indptr[v]:S.indptr[v + 1]]].tolist())
        c = 0
        while c in used:
            c += 1
        color[v] = c
    return color


def order_from_colors(color):
    """(perm, inverse, color_ptr) of the stable sort by colour."""
    m = color.size
    perm = np.argsort(color, kind="stable").astype(np.int32)
    inverse = np.empty(m, np.int32)
    inverse[perm] = np.arange(m, dtype=np.int32)
    ncol = int(color.max()) + 1 if m else 0
    color_ptr = np.concatenate([[0], np.cumsum(np.bincount(color, minlength=ncol))]).astype(np.int32)
    return perm, inverse, color_ptr


# ============================================================================================================ the checkers
def check_order(rowptr, colind, color, perm, inverse, color_ptr):
    """Messages (empty: passes).  No stored off-diagonal entry, in either direction, joins two rows of one colour; every colour
    0 .. colours - 1 is used; perm is a permutation sorted by (colour, index), inverse its inverse; color_ptr matches the counts."""
    m = rowptr.size - 1
    out = []
    color, perm, inverse, color_ptr = (np.asarray(t) for t in (color, perm, inverse, color_ptr))
    if color.size != m or perm.size != m or inverse.size != m:
        return ["a result has the wrong length"]
    if m and color.min() < 0:
        out.append("a vertex is left uncoloured")
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    off = rows != colind
    clash = off & (color[rows] == color[colind])
    if clash.any():
        p = int(np.flatnonzero(clash)[0])
        out.append(f"entry ({int(rows[p])}, {int(colind[p])}) joins two rows of colour {int(color[rows[p]])}")
    ncol = int(color.max()) + 1 if m else 0
    if color_ptr.size != ncol + 1:
        out.append(f"color_ptr has {color_ptr.size} entries for {ncol} colours")
    elif not np.array_equal(np.diff(color_ptr), np.bincount(color, minlength=ncol)) or color_ptr[0] != 0:
        out.append("color_ptr does not match the class sizes")
    elif ncol and np.diff(color_ptr).min() == 0:
        out.append("a colour below the largest is unused")
    if not np.array_equal(np.sort(perm), np.arange(m)):
        out.append("perm is not a permutation")
    else:
        k = color[perm].astype(np.int64) * max(m, 1) + perm
        if not (np.diff(k) > 0).all():
            out.append("perm is not sorted by (colour, index)")
        if not np.array_equal(inverse[perm], np.arange(m)):
            out.append("inverse is not the inverse of perm")
    return out


def host_permute(rowptr, colind, perm):
    """B = P A P^T on the host: (b_rowptr, b_colind, map) with row i of B = row perm[i] of A, column c renamed inverse[c], columns
    ascending, equal columns in source order; map[p] = position in A's arrays of B's entry p."""
    m = rowptr.size - 1
    perm = np.asarray(perm, np.int64)
    inverse = np.empty(m, np.int64)
    inverse[perm] = np.arange(m)
    lens = np.diff(rowptr)[perm]
    b_rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    b_colind = np.empty(colind.size, np.int32)
    pos = np.empty(colind.size, np.int32)
    for i in range(m):
        s0, s1 = int(rowptr[perm[i]]), int(rowptr[perm[i] + 1])
        c = inverse[colind[s0:s1]]
        o = np.argsort(c, kind="stable")
        b_colind[b_rowptr[i]:b_rowptr[i + 1]] = c[o]
        pos[b_rowptr[i]:b_rowptr[i + 1]] = s0 + o
    return b_rowptr, b_colind, pos


def level_counts(rowptr, colind):
    """(lower, upper): the number of levels of the two triangular dependency graphs (row i after the rows of its strict-lower
    columns / of its strict-upper columns)."""
    m = rowptr.size - 1
    lo = np.zeros(m, np.int64)
    up = np.zeros(m, np.int64)
    for i in range(m):
        c = colind[rowptr[i]:rowptr[i + 1]]
        c = c[c < i]
        lo[i] = lo[c].max() + 1 if c.size else 0
    for i in range(m - 1, -1, -1):
        c = colind[rowptr[i]:rowptr[i + 1]]
        c = c[c > i]
        up[i] = up[c].max() + 1 if c.size else 0
    return (int(lo.max()) + 1, int(up.max()) + 1) if m else (0, 0)


def permutation_matrices():
    """name -> (rowptr, colind) for the permutation tests: rows of 0, 1, 63, 64, 65 and 300 entries, with and without repeated
    columns; `distinct` tells whether every row's columns are."""
    rng = np.random.default_rng(8)
    m = 320
    lens = [0, 1, 63, 64, 65, 300]
    rows = []
    for i in range(m):
        n = lens[i % len(lens)] if i < 60 else int(rng.integers(0, 9))
        rows.append([int(c) for c in rng.choice(m, n, replace=False)])     # unsorted, distinct
    dup = [list(r) for r in rows]
    for i in range(0, m, 3):
        if len(dup[i]) >= 2:
            dup[i][-1] = dup[i][0]                                            # a repeated column, apart in the row
            if len(dup[i]) >= 5:
                dup[i][2] = dup[i][0]
    return {"distinct": from_rows(rows), "duplicates": from_rows(dup), "lap7_5x4x3": laplacian7(5, 4, 3),
            "empty": (np.zeros(1, np.int32), np.zeros(0, np.int32)), "no_entries": (np.zeros(8, np.int32), np.zeros(0, np.int32))}
