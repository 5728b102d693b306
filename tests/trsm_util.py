"""Helpers of the tests of triangular_solve with a block of right-hand sides (tests/test_sptrsm_cpu.py, test_gpu_sptrsm.py):
the systems of tests/test_gpu_sptrsv.py as named generators, the checker -- the project's own bound of
test_gpu_sptrsv.py::check applied to EVERY column and EVERY row -- and a numpy emulation of a lane-wide solve in the value
type, with which the checker is proved on the CPU.  Nothing here needs a GPU."""
import numpy as np
import scipy.sparse as sps

import util
from oracle import oracle

# every column count the sweep uses: around the 16-byte piece (4 fp32 / 2 fp64), around the 16 unit lanes of a team
# (64 fp32 / 32 fp64 columns), a count that needs several passes, odd counts for the partial units
N_SWEEP = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 100, 257)


def tri_system(n, density, upper, rng, dominant=True):
    """test_gpu_sptrsv.py::tri_system: a random strict triangle under a dominant diagonal."""
    A = sps.random(n, n, density=density, format="csr", random_state=rng, dtype=np.float64)
    S = sps.triu(A, 1) if upper else sps.tril(A, -1)
    rowsum = np.asarray(abs(S).sum(axis=1)).ravel()
    d = rowsum + 1.0 + rng.random(n) if dominant else rng.random(n) + 1.0
    return (S + sps.diags(d)).tocsr()


def _contraction(M, upper):
    """test_triangular_systems: with the implicit unit diagonal the strict part is scaled so the solve stays contractive."""
    n = M.shape[0]
    return ((sps.triu(M, 1) if upper else sps.tril(M, -1)) * 0.1 + sps.eye(n)).tocsr()


def _long_rows(n, upper, rng):
    """test_long_rows_and_empty_rows: rows of up to ~0.3 n entries (64 lanes per row in the plan), every tenth row empty of
    strict entries, and -- whatever the diagonal mode -- a stored diagonal of 1."""
    S = sps.tril(sps.random(n, n, density=0.3, random_state=rng, format="csr"), -1) * (0.5 / n)
    keep = sps.diags((np.arange(n) % 10 != 3).astype(np.float64))
    S = (keep @ S).tocsr()
    S.eliminate_zeros()
    M = (S + sps.eye(n)).tocsr()
    return M.T.tocsr() if upper else M


GENERATORS = ("tri1", "tri17", "tri500", "tri3000", "long1500", "chain5000", "diag2000")


def system(name, upper, unit, seed=0):
    """The named system as a CSR matrix in float64 (general position: tests cast the values to the type under test)."""
    rng = np.random.default_rng(1000 + seed)
    if name.startswith("tri"):
        n = int(name[3:])
        dens = {1: 1.0, 17: 0.3, 500: 0.02, 3000: 0.004}[n]
        M = tri_system(n, dens, upper, rng)
        return _contraction(M, upper) if unit else M
    if name == "long1500":
        return _long_rows(1500, upper, rng)
    if name == "chain5000":  # bidiagonal: one row per level, the single-workgroup kernel all the way
        n = 5000
        L = sps.diags([np.full(n - 1, -0.5), np.full(n, 1.0 if unit else 2.0)], [-1, 0]).tocsr()
        return L.T.tocsr() if upper else L
    if name == "diag2000":   # one level of n rows
        n = 2000
        return sps.diags(np.ones(n) if unit else rng.random(n) + 1.0).tocsr()
    raise KeyError(name)


def rhs(m, n, seed=0):
    """B (m x n, float64): every column different, entries in [0.5, 1.5)."""
    return np.random.default_rng(2000 + seed).random((m, n)) + 0.5


def triangle(M, upper, unit, dtype, scale_a=None):
    """T, the triangle the solve reads, in float64 over the values as the type under test holds them."""
    M = M.tocsr()
    n = M.shape[0]
    Md = M.astype(dtype).astype(np.float64) * (1.0 if scale_a is None else float(dtype(scale_a)))
    T = (sps.triu(Md, 1) if upper else sps.tril(Md, -1)) + (sps.eye(n) if unit else sps.diags(Md.diagonal()))
    return T.tocsr()


def oracle_block(M, B, upper, unit, dtype, scale_a=None):
    """oracle.triangular_solve of every column (the reference's sequential loop in the value type)."""
    M = M.tocsr()
    vals = M.data.astype(dtype)
    Bt = np.asarray(B).astype(dtype)
    return np.stack([oracle.triangular_solve(M.shape, M.indptr, M.indices, vals, np.ascontiguousarray(Bt[:, j]), upper=upper,
                                             unit=unit, scale_a=scale_a) for j in range(Bt.shape[1])], axis=1) \
        if Bt.shape[1] else np.zeros(Bt.shape, dtype)


def violations(M, B, X, upper, unit, dtype, scale_a=None, ref=None):
    """The bound of test_gpu_sptrsv.py::check on every (row, column).  Returns a list of messages, empty when X passes:
    (1) backward error  |b - T x| <= max(TOL, 0.5 k eps) (|b| + |T| |x|)  per row and column, k = entries of the row + 2;
    (2) forward error against the oracle's column, at most max(100 TOL, 0.5 k_max eps) on the scale
        max(|ref|, 1e-3 max|ref of that column| + 1e-30)."""
    dtype = np.dtype(dtype).type
    X = np.asarray(X)
    out = []
    if X.shape != np.asarray(B).shape:
        return [f"shape {X.shape} != {np.asarray(B).shape}"]
    if not np.all(np.isfinite(X)):
        out.append(f"{np.count_nonzero(~np.isfinite(X))} non-finite elements")
        return out
    T = triangle(M, upper, unit, dtype, scale_a)
    Bd, Xd = np.asarray(B).astype(dtype).astype(np.float64), X.astype(np.float64)
    resid = np.abs(T @ Xd - Bd)
    norm = np.abs(Bd) + abs(T) @ np.abs(Xd)
    k = np.diff(T.indptr) + 2
    tol = np.maximum(util.TOL[np.dtype(dtype)], 0.5 * k * np.finfo(dtype).eps)[:, None]
    bad = ~(resid <= tol * norm)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        out.append(f"backward: {int(bad.sum())} elements, first (row {r}, column {c}): resid {resid[r, c]:.3g} "
                   f"bound {(tol * norm)[r, c]:.3g}")
    if ref is None:
        ref = oracle_block(M, B, upper, unit, dtype, scale_a)
    ref = np.asarray(ref).astype(np.float64)
    ftol = max(100 * util.TOL[np.dtype(dtype)], 0.5 * float(k.max()) * float(np.finfo(dtype).eps))
    scale = np.maximum(np.abs(ref), np.abs(ref).max(axis=0, keepdims=True) * 1e-3 + 1e-30) if ref.size else ref
    err = np.abs(Xd - ref) / scale if ref.size else ref
    if ref.size and err.max() > ftol:
        r, c = np.unravel_index(err.argmax(), err.shape)
        out.append(f"forward: max rel err vs oracle {err.max():.3g} at (row {r}, column {c}), bound {ftol:.3g}")
    return out


def emulate(M, B, upper, unit, dtype, scale_a=None, lanes=8):
    """The device's arithmetic on the CPU, in the value type: a row's strict entries are dealt to `lanes` lanes (entry p to
    lane p mod lanes), every lane adds its products in order, the lanes are added by a tree (lane i += lane i ^ o for
    o = lanes/2 .. 1), then  x = (b - alpha dot) / (alpha d)  with d the last stored diagonal entry.  All columns at once."""
    dtype = np.dtype(dtype).type
    M = M.tocsr()
    m = M.shape[0]
    vals, rp, ci = M.data.astype(dtype), M.indptr, M.indices
    Bt = np.asarray(B).astype(dtype)
    X = np.zeros_like(Bt)
    alpha = dtype(1 if scale_a is None else scale_a)
    for r in (range(m - 1, -1, -1) if upper else range(m)):
        part = np.zeros((lanes, Bt.shape[1]), dtype)
        d = dtype(0)
        for q, p in enumerate(range(rp[r], rp[r + 1])):
            c = ci[p]
            if (c > r) if upper else (c < r):
                part[q % lanes] += vals[p] * X[c]
            elif c == r:
                d = vals[p]
        o = lanes // 2
        while o:
            part = part + part[np.arange(lanes) ^ o]
            o //= 2
        v = Bt[r] - alpha * part[0]
        X[r] = v if unit else v / (alpha * d)
    return X
