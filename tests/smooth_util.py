"""The host model, the dense reference, the bound and the generators of smooth_prolongator (tests/test_smooth_cpu.py proves them on
the host, tests/test_gpu_smooth.py compares the device with the model bit for bit, tests/test_gpu_smooth_stream.py runs
STREAM_CASES).

The model restates what include/spblas_gfx950.h documents for spblas_gfx950_smooth_*, in numpy OF THE VALUE TYPE T:
    structure  row i of P holds one entry for every distinct aggregate among {agg[i]} and {agg[j] : (i, j) stored}, ascending
    strong     the rule of aggregate (aggregate_util.strength): j != i and a * a >= (t2 * |d_i|) * |d_j|
    dF_i       T(0) plus, in ascending stored position, every entry with j == i (repeats included) or weak
    smoothed   dF_i finite and non-zero:  s_i = T(omega) / dF_i, base_i = T(1) - T(omega);  else s_i = 0, base_i = 1
    P(i, J)    fma(-s_i, acc, b),  acc = T(0) plus the strong entries of row i with agg[j] == J in ascending position,
               b = base_i if J == agg[i] else 0
The ONE fma is exact: the product and the sum as fractions.Fraction, rounded once to T with ties to even (this interpreter has no
math.fma, and a detour through float64 rounds twice for float32).  model(..., mistake=...) seeds the mistakes the cases must
catch."""
from fractions import Fraction

import numpy as np
import scipy.sparse as sps

import aggregate_util as A

MISTAKES = ("dF_skips_weak", "sums_descending", "own_marker_dropped", "diag_in_acc")
STAGE_PER_LANE = 8      # SM_STAGE_PER_LANE of csrc/smooth.hip: a team of G lanes stages a row of up to 8 * G entries in LDS
_FMT = {np.dtype(np.float32): (24, -126, 127), np.dtype(np.float64): (53, -1022, 1023)}


def stage_capacity(lanes):
    return STAGE_PER_LANE * lanes


# ============================================================================================================ exact rounding
def round_fraction(x, dtype):
    """The value of type `dtype` nearest to the Fraction x, ties to even (overflow gives +-inf, a tiny x a signed zero)."""
    T = np.dtype(dtype).type
    p, emin, emax = _FMT[np.dtype(dtype)]
    if x == 0:
        return T(0)
    sign, ax = (-1 if x < 0 else 1), abs(x)
    e = ax.numerator.bit_length() - ax.denominator.bit_length()          # 2^e <= ax < 2^(e + 1) after the correction below
    if Fraction(2) ** e > ax:
        e -= 1
    q = max(e, emin) - (p - 1)                                            # the exponent of the last kept bit
    scaled = ax / Fraction(2) ** q
    n, rest = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rest
    if twice > scaled.denominator or (twice == scaled.denominator and n % 2 == 1):
        n += 1
    if n * Fraction(2) ** q >= Fraction(2) ** (emax + 1):                 # rounded up past the largest finite value
        return T(sign * np.inf)
    with np.errstate(all="ignore"):
        out = np.ldexp(np.float64(n), q)                                  # exact: n has at most p bits (or is 2^p)
    out = T(out)
    return T(-out) if sign < 0 else out


def fma(a, b, c, dtype):
    """fma(a, b, c) of scalars of the value type: a * b + c with ONE rounding.  Non-finite operands go through float64, which
    gives the right infinity / NaN (no rounding is involved)."""
    T = np.dtype(dtype).type
    a, b, c = T(a), T(b), T(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return T(np.float64(a) * np.float64(b) + np.float64(c))
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        # an exact zero is +0 (round to nearest) unless a zero product and a zero addend are both negative
        both_zero = (a == 0 or b == 0) and c == 0
        return T(-0.0) if both_zero and (np.signbit(a) != np.signbit(b)) and np.signbit(c) else T(0)
    return round_fraction(exact, dtype)


# ============================================================================================================== generators
def hub_with_agg(leaves, n_agg=37):
    """hub(leaves) and a map that spreads its rows over n_agg aggregates: the hub row holds n_agg entries of P, each of many
    terms, far past any staging capacity."""
    g = A.hub(leaves)
    m = g[0].size - 1
    return g, (np.arange(m) * 7 % n_agg).astype(np.int32), n_agg


def row_lengths(lengths, seed=0):
    """(rowptr, colind, values): row i holds lengths[i] distinct columns, the diagonal among them when lengths[i] >= 1, in random
    (unsorted) order; off-diagonal values of magnitude 1 / 2 / 4 with random signs, diagonal 8."""
    m = len(lengths)
    rng = np.random.default_rng(seed)
    assert max(lengths) <= m
    cols = []
    for i, n in enumerate(lengths):
        if n == 0:
            cols.append(np.zeros(0, np.int64))
            continue
        others = rng.choice(m - 1, n - 1, replace=False)
        others = np.where(others >= i, others + 1, others)
        c = np.concatenate([[i], others])
        cols.append(rng.permutation(c))
    colind = np.concatenate(cols).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    rows = A._rows(rowptr)
    v = rng.choice([1.0, 2.0, 4.0], colind.size) * rng.choice([-1.0, 1.0], colind.size)
    return rowptr, colind, np.where(colind == rows, 8.0, v)


def capacity_rows(lanes):
    """(graph, lengths): rows of 0, 1, 2 entries and of the staging capacity - 1 / exact / + 1 for a team of `lanes` lanes, filled
    up with rows of a length that makes lanes_per_row pick `lanes`."""
    cap = stage_capacity(lanes)
    typical = {4: 5, 8: 10, 16: 30, 64: 100}[lanes]
    special = [0, 1, 2, cap - 1, cap, cap + 1]
    m = max(cap + 8, 600 if lanes == 64 else 300)
    lengths = special + [typical] * (m - len(special))
    g = row_lengths(lengths, seed=lanes)
    assert A.lanes_for(g[0], g[1]) == lanes
    return g, lengths


def graph_laplacian(m, per_row, seed):
    """A weighted graph Laplacian with zero row sums: symmetric pattern, off-diagonal -w (w a small power of two), the diagonal
    the exact sum of the row's weights."""
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(m), per_row)
    dst = rng.integers(0, m, src.size)
    keep = src != dst
    w = rng.choice([0.5, 1.0, 2.0], src.size)[keep]
    W = sps.coo_matrix((w, (src[keep], dst[keep])), shape=(m, m)).tocsr()
    W = (W + W.T).tocsr()
    L = (sps.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()
    L.sort_indices()
    return L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.astype(np.float64)


def cancelling_row():
    """path(12) with theta = 0.25 in which row 5's two off-diagonal entries are weak (-1/2 each against a diagonal of 1 between
    diagonals of 64) and cancel the diagonal: dF_5 = 0, so row 5 of P is the row of T."""
    rp, ci, v = A.path(12)
    rows = A._rows(rp)
    v = np.where(ci == rows, 64.0, -1.0)
    v[(rows == 5) & (ci == 5)] = 1.0
    v[(rows == 5) & (ci != 5)] = -0.5
    return rp, ci, v


def two_diagonals():
    """grid5(5, 4) with a second stored diagonal entry (value 3, after the first of 4) in every row: d uses the first, dF both."""
    rp, ci, v = A.grid5(5, 4)
    m = rp.size - 1
    rows = A._rows(rp)
    new_ci, new_v, new_rp = [], [], [0]
    for i in range(m):
        sel = rows == i
        new_ci += ci[sel].tolist() + [i]
        new_v += v[sel].tolist() + [3.0]
        new_rp.append(len(new_ci))
    return np.array(new_rp, np.int32), np.array(new_ci, np.int32), np.array(new_v)


def without_diagonal(g):
    rp, ci, v = g
    rows = A._rows(rp)
    keep = ci != rows
    m = rp.size - 1
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=m))]).astype(np.int32)
    return rp2, ci[keep], v[keep]


def foreign_rows(m=40):
    """A path whose row i lies in an aggregate none of its stored entries point into: row i stores only (i, i + 1) (the last row
    nothing), agg = i % 3.  Every row needs the own-aggregate marker."""
    rows = [[i + 1] if i + 1 < m else [] for i in range(m)]
    import multicolor_util as MC
    rp, ci = MC.from_rows(rows)
    return (rp, ci, np.full(ci.size, -1.0)), (np.arange(m) % 3).astype(np.int32), 3


# ================================================================================================================ the model
def _ordered_masked_sums(v, mask, first, lens, dtype, descending=False):
    """out[r] = T(0) plus v[first[r] + k] for k = 0 .. lens[r] - 1 where mask is set, added one after the other (descending: from
    the last position down)."""
    out = np.zeros(first.size, dtype)
    with np.errstate(all="ignore"):
        for k in range(int(lens.max()) if lens.size else 0):
            sel = np.flatnonzero(lens > k)
            idx = first[sel] + (lens[sel] - 1 - k if descending else k)
            take = mask[idx]
            out[sel[take]] = out[sel[take]] + v[idx[take]]
    return out


def structure(rowptr, colind, agg, n_agg, mistake=None):
    """(p_rowptr, p_colind, seg_ptr, order, pos): the extended list sorted by (row, aggregate, position); pos = -1 is the
    own-aggregate marker, which stands first in its run."""
    m, nnz = rowptr.size - 1, int(colind.size)
    agg = np.asarray(agg, np.int64)
    rows = A._rows(rowptr)
    x_row = np.concatenate([np.arange(m), rows])
    x_col = np.concatenate([agg, agg[colind]]) if m else np.zeros(0, np.int64)
    x_pos = np.concatenate([np.full(m, -1), np.arange(nnz)])
    if mistake == "own_marker_dropped":
        x_row, x_col, x_pos = x_row[m:], x_col[m:], x_pos[m:]
    order = np.lexsort((x_pos, x_col, x_row))
    r, c, pos = x_row[order], x_col[order], x_pos[order]
    head = np.ones(r.size, bool)
    head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    seg = np.flatnonzero(head)
    seg_ptr = np.append(seg, r.size).astype(np.int64)
    p_rowptr = np.concatenate([[0], np.cumsum(np.bincount(r[seg], minlength=m))]).astype(np.int32)
    return p_rowptr, c[seg].astype(np.int32), seg_ptr, order, pos


def model(rowptr, colind, values, agg, n_agg, omega, theta=0.0, dtype=np.float32, mistake=None):
    """dict(p_rowptr, p_colind, p_values, terms, smoothed, dF, s, absum): the smoothed prolongator as the device computes it.
    terms[e] = strong entries added into entry e; absum[e] = the float64 sum of their magnitudes."""
    assert mistake is None or mistake in MISTAKES
    T = np.dtype(dtype).type
    m, nnz = rowptr.size - 1, int(colind.size)
    agg = np.asarray(agg, np.int64)
    rows = A._rows(rowptr)
    v = np.asarray(values[:nnz]).astype(dtype)
    strong, _ = A.strength(rowptr, colind, values, theta, dtype)
    diag = colind == rows
    lumped = ~strong if mistake != "dF_skips_weak" else diag
    in_acc = strong if mistake != "diag_in_acc" else (strong | diag)
    if mistake == "diag_in_acc":
        lumped = ~in_acc
    desc = mistake == "sums_descending"
    dF = _ordered_masked_sums(v, lumped, rowptr[:-1].astype(np.int64), np.diff(rowptr).astype(np.int64), dtype, desc)
    smoothed = np.isfinite(dF) & (dF != 0)
    w = T(omega)
    with np.errstate(all="ignore"):
        s = np.where(smoothed, w / np.where(smoothed, dF, T(1)), T(0)).astype(dtype)
        base = np.where(smoothed, T(1) - w, T(1)).astype(dtype)
    p_rowptr, p_colind, seg_ptr, order, pos = structure(rowptr, colind, agg, n_agg, mistake)
    n_e = p_colind.size
    e_row = np.repeat(np.arange(m), np.diff(p_rowptr))
    # sorted positions -> values / masks (the marker holds no value)
    sv = np.where(pos >= 0, v[np.maximum(pos, 0)] if nnz else T(0), T(0)).astype(dtype)
    sm = np.where(pos >= 0, in_acc[np.maximum(pos, 0)] if nnz else False, False)
    acc = _ordered_masked_sums(sv, sm, seg_ptr[:-1], np.diff(seg_ptr), dtype, desc)
    own = pos[seg_ptr[:-1]] < 0 if n_e else np.zeros(0, bool)
    if mistake == "own_marker_dropped":
        own = p_colind == agg[e_row]
    b = np.where(own, base[e_row], T(0)).astype(dtype)
    neg_s = (-s[e_row]).astype(dtype)
    # b == 0 and a finite non-zero product: the fma is the product rounded once, which numpy's multiplication is; else exact
    with np.errstate(all="ignore"):
        prod = (neg_s * acc).astype(dtype)
    plain = (b == 0) & ~np.signbit(b) & (neg_s != 0) & (acc != 0) & np.isfinite(neg_s) & np.isfinite(acc)
    out = np.where(plain, prod, T(0)).astype(dtype)
    for e in np.flatnonzero(~plain):
        out[e] = fma(neg_s[e], acc[e], b[e], dtype)
    terms = np.add.reduceat(sm.astype(np.int64), seg_ptr[:-1]) if n_e else np.zeros(0, np.int64)
    absum = np.add.reduceat(np.where(sm, np.abs(sv.astype(np.float64)), 0.0), seg_ptr[:-1]) if n_e else np.zeros(0)
    return dict(p_rowptr=p_rowptr, p_colind=p_colind, p_values=out, terms=terms, smoothed=smoothed, dF=dF, s=s, absum=absum,
                b=b, rows=e_row)


# ============================================================================================================ the reference
def dense_reference(rowptr, colind, values, agg, n_agg, omega, theta, dtype):
    """(I - omega D_F^-1 A_F) T as a dense float64 array, from the values and omega AS ROUNDED TO the value type; the strength
    of an entry is the value type's (a classification, not arithmetic).  A row whose float64 dF is zero or not finite is T's."""
    m, nnz = rowptr.size - 1, int(colind.size)
    rows = A._rows(rowptr)
    v = np.asarray(values[:nnz]).astype(dtype).astype(np.float64)
    strong, _ = A.strength(rowptr, colind, values, theta, dtype)
    w = float(np.dtype(dtype).type(omega))
    Tm = np.zeros((m, n_agg))
    Tm[np.arange(m), np.asarray(agg, np.int64)] = 1.0
    dF = np.bincount(rows[~strong], weights=v[~strong], minlength=m) if nnz else np.zeros(m)
    AF = sps.csr_matrix((np.where(strong, v, 0.0), colind.astype(np.int64), rowptr.astype(np.int64)), shape=(m, m)).toarray()
    ok = np.isfinite(dF) & (dF != 0)
    with np.errstate(all="ignore"):
        scale = np.where(ok, w / np.where(ok, dF, 1.0), 0.0)
    P = Tm * np.where(ok, 1.0 - w, 1.0)[:, None] - (scale[:, None] * AF) @ Tm
    return P


def bound(mod, dtype):
    """Per entry of the model: (k + 3) u (|b| + |s_i| sum|a_ij|) in float64, k the contributing terms, u the unit roundoff of the
    value type.  It covers the rounding of base_i and of s_i, the k - 1 additions of acc and the fma, for a dF that is exact."""
    u = np.finfo(dtype).eps / 2
    s = np.abs(mod["s"].astype(np.float64))[mod["rows"]]
    return (mod["terms"] + 3) * u * (np.abs(mod["b"].astype(np.float64)) + s * mod["absum"])


def against_reference(mod, ref, dtype):
    """Messages (empty: passes): every entry of the model within its bound of the reference, and the reference zero elsewhere."""
    rows, cols = mod["rows"], mod["p_colind"].astype(np.int64)
    out = []
    mask = np.zeros(ref.shape, bool)
    mask[rows, cols] = True
    if (ref[~mask] != 0).any():
        out.append("the reference holds an entry outside the pattern")
    diff = np.abs(mod["p_values"].astype(np.float64) - ref[rows, cols])
    bad = ~(diff <= bound(mod, dtype))
    if bad.any():
        e = int(np.flatnonzero(bad)[0])
        out.append(f"entry {e} (row {int(rows[e])}, column {int(cols[e])}) is off by {diff[e]:.3e}")
    return out


def check_structure(m, n_agg, p_rowptr, p_colind):
    p_rowptr, p_colind = np.asarray(p_rowptr), np.asarray(p_colind)
    if p_rowptr.size != m + 1 or p_rowptr[0] != 0 or p_rowptr[-1] != p_colind.size or (np.diff(p_rowptr) < 0).any():
        return ["the row offsets do not describe the entries"]
    out = []
    if p_colind.size and (p_colind.min() < 0 or p_colind.max() >= n_agg):
        out.append("a column lies outside [0, n_agg)")
    for i in range(m):
        if not (np.diff(p_colind[p_rowptr[i]:p_rowptr[i + 1]]) > 0).all():
            out.append(f"row {i}: the columns are not strictly ascending")
            break
    return out


# ================================================================================================================ two-grid
def two_grid_iterations(rowptr, colind, values, P, rtol=1e-8, maxiter=500):
    """CG iterations on A x = 1 preconditioned by one two-grid cycle in float64: forward Gauss-Seidel, the exact coarse
    correction with A_c = P^T A P, backward Gauss-Seidel."""
    import scipy.sparse.linalg as spla
    m = rowptr.size - 1
    Am = sps.csr_matrix((np.asarray(values, np.float64), colind.astype(np.int64), rowptr.astype(np.int64)), shape=(m, m))
    P = sps.csr_matrix(P)
    Ac = (P.T @ Am @ P).tocsc()
    solve_c = spla.factorized(Ac)
    Lo, Up = sps.tril(Am, format="csr"), sps.triu(Am, format="csr")

    def cycle(r):
        x = spla.spsolve_triangular(Lo, r, lower=True)
        x = x + P @ solve_c(P.T @ (r - Am @ x))
        return x + spla.spsolve_triangular(Up, r - Am @ x, lower=False)

    count = [0]

    def cb(_):
        count[0] += 1

    x, info = spla.cg(Am, np.ones(m), rtol=rtol, atol=0.0, maxiter=maxiter, M=spla.LinearOperator((m, m), matvec=cycle),
                      callback=cb)
    assert info == 0
    return count[0]


def as_csr(mod, m, n_agg):
    return sps.csr_matrix((mod["p_values"].astype(np.float64), mod["p_colind"].astype(np.int64),
                           mod["p_rowptr"].astype(np.int64)), shape=(m, n_agg))


# ===================================================================================================== stream-order cases
# What tests/test_gpu_smooth_stream.py runs, by exported name (tests/test_smooth_cpu.py asserts that every name of
# spblas_reference_amd.SMOOTH_EXPORTS is listed here).
STREAM_CASES = {
    "smooth_values_late_inputs": ("smooth_prolongator",),
    "smooth_structure_late": ("smooth_prolongator_structure",),
    "smooth_plan_dies_behind_its_last_use": ("smooth_prolongator", "smooth_prolongator_inspect"),
}
