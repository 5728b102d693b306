"""-m gpu tests of triangular_solve / triangular_solve_inspect with a block of right-hand sides: B and X are (m, n) tensors,
X(:, j) = inv(T) B(:, j) in one solve (spblas_gfx950_sptrsm_solve, csrc/sptrsm.hip).  Every parity case fails on a backend
without the feature: 2-D operands raise there.

The checker is tests/trsm_util.py::violations -- the bound of test_gpu_sptrsv.py::check on every row of every column
(tests/test_sptrsm_cpu.py proves it on the CPU).  The sweep crosses value type x triangle x diagonal x system x column count
x (B layout, X layout) in full; only plan-free / inspected is PAIRED with them (it alternates with the column count and the
layout pair, starting at an offset that differs from case to case), so each of the two runs every column count, every
layout pair and every system, for each value type, but not every combination of them."""
import gc
import os

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import gpu_util as G
import spblas_reference_amd as sp
import trsm_util as TU
import util
from oracle import oracle

pytestmark = pytest.mark.gpu

LAYOUTS = (("R", "R"), ("L", "L"), ("R", "L"), ("L", "R"))
TD = {np.float32: torch.float32, np.float64: torch.float64}


def _tags(upper, unit):
    return (sp.upper_triangle if upper else sp.lower_triangle,
            sp.implicit_unit_diagonal if unit else sp.explicit_diagonal)


def dense(host, layout):
    """host (m, n) on the device as a row-major ('R') or column-major ('L') tensor of shape (m, n)."""
    t = G.dev(np.ascontiguousarray(host))
    return t if layout == "R" else t.t().contiguous().t()


def nan_like(m, n, dtype, layout):
    t = torch.full((m, n) if layout == "R" else (n, m), float("nan"), dtype=dtype, device="cuda")
    return t if layout == "R" else t.t()


def bits(a):
    """The bytes of a host array (bit-for-bit comparisons, NaN included)."""
    return np.ascontiguousarray(a).view(np.uint8)


def on_device(M, dtype):
    M = M.tocsr()
    return G.csr_on_device(M.data.astype(dtype), M.indptr.astype(np.int32), M.indices.astype(np.int32), M.shape, M.nnz)


def solve_block(a, B_host, upper, unit, dtype, lb="R", lx="R", info=None):
    """One block solve; info=None is the plan-free call.  Returns X on the host."""
    uplo, diag = _tags(upper, unit)
    d_b = dense(B_host.astype(dtype), lb)
    d_x = nan_like(B_host.shape[0], B_host.shape[1], d_b.dtype, lx)
    if info is None:
        sp.triangular_solve(a, uplo, diag, d_b, d_x)
    else:
        sp.triangular_solve(info, a, uplo, diag, d_b, d_x)
    return G.host(d_x)


# ---- parity sweep ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TU.GENERATORS)
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parity_sweep(gpu, dtype, upper, unit, name):
    gi = TU.GENERATORS.index(name)
    M = TU.system(name, upper, unit)
    m = M.shape[0]
    nmax = max(TU.N_SWEEP)
    B = TU.rhs(m, nmax, seed=gi)
    ref = TU.oracle_block(M, B, upper, unit, dtype)   # column j of a block solve is the solve of column j alone
    a = on_device(M, dtype)
    uplo, diag = _tags(upper, unit)
    info = sp.triangular_solve_inspect(a, uplo, diag, dense(B[:, :2].astype(dtype), "R"), nan_like(m, 2, TD[dtype], "R"))
    state = info.state_
    shift = gi + 2 * int(upper) + int(unit)
    for ni, n in enumerate(TU.N_SWEEP):
        for li, (lb, lx) in enumerate(LAYOUTS):
            inspected = (ni + li + shift) % 2 == 0
            X = solve_block(a, B[:, :n], upper, unit, dtype, lb, lx, info if inspected else None)
            bad = TU.violations(M, B[:, :n], X, upper, unit, dtype, ref=ref[:, :n])
            assert not bad, f"n {n}, B {lb}, X {lx}, {'inspected' if inspected else 'plan-free'}: {bad}"
    assert info.state_ is state   # the inspected plan served every column count and layout


# ---- windows and alignment ---------------------------------------------------------------------------------------------
NAN_BITS = {np.float32: (np.uint32, 0x7FC12345), np.float64: (np.uint64, 0x7FF8123456789ABC)}


def _window(flat, shift, m, n, ld, layout):
    """An (m, n) window into the 1-D tensor `flat`, `shift` elements past its start: row-major with row stride ld >= n, or
    column-major with column stride ld >= m.  Returns the window and the boolean mask of flat's elements inside it."""
    idx = torch.arange(flat.numel(), device="cuda")
    if layout == "R":
        w = flat[shift:shift + m * ld].view(m, ld)[:, :n]
        inside = (idx >= shift) & (idx < shift + m * ld) & ((idx - shift) % ld < n)
    else:
        w = flat[shift:shift + n * ld].view(n, ld)[:, :m].t()
        inside = (idx >= shift) & (idx < shift + n * ld) & ((idx - shift) % ld < m)
    return w, inside


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_windows_of_wider_tensors_at_every_alignment(gpu, dtype, shift):
    """Row stride > n, column stride > m, base pointers 0 / 1 / 2 elements past an allocation's start (so the first 16-byte
    piece of a row begins at column 0, 3, 2 in fp32 and 0, 1, 0 in fp64), leading dimensions that allow 16-byte pieces (a
    multiple of 4) and that do not (odd).  What lies outside the windows holds a NaN pattern before the solve and the same
    bits after it; B keeps all of its bits."""
    utype, bits = NAN_BITS[dtype]
    upper, unit = shift == 1, shift == 2
    M = TU.system("tri500", upper, unit)
    m = M.shape[0]
    a = on_device(M, dtype)
    uplo, diag = _tags(upper, unit)
    tdtype = TD[dtype]
    itype = torch.int32 if dtype is np.float32 else torch.int64
    signed_bits = int(np.array(bits, utype).astype(np.int32 if dtype is np.float32 else np.int64))
    for n in (3, 8, 17, 37):
        B = TU.rhs(m, n, seed=n)
        ref = TU.oracle_block(M, B, upper, unit, dtype)
        for lb, lx in LAYOUTS:
            for pad in (4, 7):   # leading dimension = extent rounded up to a multiple of 4, plus 4 (aligned) or 7 (odd)
                ldb = ((n if lb == "R" else m) + 3) // 4 * 4 + pad
                ldx = ((n if lx == "R" else m) + 3) // 4 * 4 + pad
                size = lambda ld, lay: shift + (m if lay == "R" else n) * ld + 5
                fb = torch.full((size(ldb, lb),), signed_bits, dtype=itype, device="cuda").view(tdtype)
                fx = torch.full((size(ldx, lx),), signed_bits, dtype=itype, device="cuda").view(tdtype)
                wb, inb = _window(fb, shift, m, n, ldb, lb)
                wx, inx = _window(fx, shift, m, n, ldx, lx)
                wb.copy_(G.dev(B.astype(dtype)))
                fb0 = fb.view(itype).clone()
                sp.triangular_solve(a, uplo, diag, wb, wx)
                torch.cuda.synchronize()
                what = f"n {n}, B {lb} ld {ldb}, X {lx} ld {ldx}, shift {shift}"
                assert bool((fx.view(itype)[~inx] == signed_bits).all()), what + ": written outside the window of X"
                assert bool((fb.view(itype) == fb0).all()), what + ": B changed"
                bad = TU.violations(M, B, G.host(wx), upper, unit, dtype, ref=ref)
                assert not bad, f"{what}: {bad}"


# ---- edge counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_contiguous_column_is_the_vector_solve_bit_for_bit(gpu, dtype):
    rng = np.random.default_rng(31)
    n, k = 60000, 6   # a few hundred levels: the vector solve's default (one cooperative launch) is what must be matched
    rows = np.repeat(np.arange(n), k)
    cols = (rng.random(n * k) * rows).astype(np.int64)
    keep = cols < rows
    S = sps.csr_matrix(((rng.random(keep.sum()) - 0.5) * (0.5 / k), (rows[keep], cols[keep])), shape=(n, n))
    for M, upper in ((S + sps.diags(1.0 + rng.random(n))).tocsr(), False), (TU.system("tri3000", True, False), True):
        a = on_device(M, dtype)
        uplo, diag = _tags(upper, False)
        b = G.dev((rng.random(M.shape[0]) + 0.5).astype(dtype))
        xv = torch.full_like(b, float("nan"))
        info = sp.triangular_solve_inspect(a, uplo, diag, b, xv)
        sp.triangular_solve(info, a, uplo, diag, b, xv)
        for make in (lambda t: t.view(-1, 1), lambda t: t.view(1, -1).t()):   # (m, 1) row-major and column-major
            xm = torch.full_like(b, float("nan"))
            sp.triangular_solve(info, a, uplo, diag, make(b), make(xm))
            assert np.array_equal(bits(G.host(xm)), bits(G.host(xv)))
        # ... and a strided single column is NOT the vector solve, but solves the same system
        wide = torch.full((M.shape[0], 3), float("nan"), dtype=b.dtype, device="cuda")
        sp.triangular_solve(info, a, uplo, diag, b.view(-1, 1), wide[:, 1:2])
        assert not TU.violations(M, G.host(b)[:, None], G.host(wide[:, 1:2]), upper, False, dtype)
        assert bool(torch.isnan(wide[:, 0]).all()) and bool(torch.isnan(wide[:, 2]).all())


def test_zero_columns_leave_x_untouched(gpu):
    M = TU.system("tri500", False, False)
    a = on_device(M, np.float32)
    wide_b = torch.rand((500, 4), device="cuda")
    wide_x = torch.full((500, 4), float("nan"), device="cuda")
    info = sp.triangular_solve_inspect(a, sp.lower_triangle, sp.explicit_diagonal, wide_b[:, :0], wide_x[:, :0])
    sp.triangular_solve(info, a, sp.lower_triangle, sp.explicit_diagonal, wide_b[:, :0], wide_x[:, :0])
    sp.triangular_solve(a, sp.lower_triangle, sp.explicit_diagonal, wide_b.t()[:0].t(), wide_x.t()[:0].t())
    torch.cuda.synchronize()
    assert bool(torch.isnan(wide_x).all())


# ---- determinism and column independence -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["R", "L"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_same_bits_twice_duplicated_columns_and_a_poisoned_column(gpu, dtype, layout):
    for name, upper, unit in (("tri3000", False, False), ("long1500", True, True), ("chain5000", False, False)):
        M = TU.system(name, upper, unit)
        m = M.shape[0]
        a = on_device(M, dtype)
        uplo, diag = _tags(upper, unit)
        info = sp.triangular_solve_inspect(a, uplo, diag, nan_like(m, 2, TD[dtype], "R"), nan_like(m, 2, TD[dtype], "R"))
        for n in (5, 8, 17, 33):
            base = TU.rhs(m, 2, seed=n)
            B = base[:, np.arange(n) % 2]            # columns 0, 2, 4, ... equal, columns 1, 3, 5, ... equal
            X1 = solve_block(a, B, upper, unit, dtype, layout, layout, info)
            X2 = solve_block(a, B, upper, unit, dtype, layout, layout, info)
            assert np.array_equal(bits(X1), bits(X2)), f"{name} n {n}: two solves differ"
            for j in range(2, n):
                assert np.array_equal(bits(X1[:, j]), bits(X1[:, j % 2])), \
                    f"{name} n {n}: column {j} differs from its duplicate {j % 2}"
            assert not TU.violations(M, B, X1, upper, unit, dtype)
            # a column of NaN / inf changes no bit of any other column
            for poison in (np.nan, np.inf):
                j = n // 2
                Bp = B.copy()
                Bp[:, j] = poison
                Xp = solve_block(a, Bp, upper, unit, dtype, layout, layout, info)
                others = np.arange(n) != j
                assert np.array_equal(bits(Xp[:, others]), bits(X1[:, others])), \
                    f"{name} n {n}: a column of {poison} changed another column"
                assert not np.isfinite(Xp[:, j]).any()


# ---- exactness ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["R", "L"])
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("upper", [False, True])
def test_dyadic_golden_block_is_bit_exact(gpu, upper, unit, layout):
    """tests/golden/trsv_general_dyadic.npz with the columns b * 2^j, j = -3 .. 3: every x is a dyadic rational computed
    exactly in any summation order, so every column equals the oracle's (and the golden x times 2^j) bit for bit."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "trsv_general_dyadic.npz"))
    n = int(g["shape"][0])
    a = G.csr_on_device(g["values"], g["rowptr"], g["colind"], (n, n), len(g["values"]))
    scales = np.float32(2.0) ** np.arange(-3, 4, dtype=np.float32)
    B = (g["b"][:, None] * scales[None, :]).astype(np.float32)
    X = solve_block(a, B, upper, unit, np.float32, layout, layout)
    key = f"x_{'upper' if upper else 'lower'}_{'unit' if unit else 'explicit'}"
    for j in range(7):
        ref = oracle.triangular_solve((n, n), g["rowptr"], g["colind"], g["values"], np.ascontiguousarray(B[:, j]),
                                      upper=upper, unit=unit)
        assert np.array_equal(X[:, j], ref), f"column {j}"
        assert np.array_equal(X[:, j], g[key] * scales[j]), f"column {j} against the golden x"


# ---- views -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["R", "L"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scaled_matrix_scaled_rhs_and_in_place(gpu, dtype, layout):
    M = TU.system("tri3000", False, False)
    m, n = M.shape[0], 9
    B = TU.rhs(m, n, seed=5)
    a = on_device(M, dtype)
    lo, ex = sp.lower_triangle, sp.explicit_diagonal
    for alpha in (2.0, -0.5):   # scaled(alpha, A): x = inv(alpha T) b
        d_b, d_x = dense(B.astype(dtype), layout), nan_like(m, n, TD[dtype], layout)
        sp.triangular_solve(sp.scaled(alpha, a), lo, ex, d_b, d_x)
        assert not TU.violations(M, B, G.host(d_x), False, False, dtype, scale_a=alpha)
    # scaled(s, B): X = inv(T) (s B), applied to X afterwards; also on a window of a wider tensor
    s = -3.0
    sB = (dtype(s) * B.astype(dtype)).astype(np.float64)
    d_b, d_x = dense(B.astype(dtype), layout), nan_like(m, n, TD[dtype], layout)
    sp.triangular_solve(a, lo, ex, sp.scaled(s, d_b), d_x)
    assert not TU.violations(M, sB, G.host(d_x), False, False, dtype)
    wide = nan_like(m, n + 3, d_b.dtype, layout)
    sp.triangular_solve(a, lo, ex, sp.scaled(s, d_b), wide[:, 1:n + 1])
    assert not TU.violations(M, sB, G.host(wide[:, 1:n + 1]), False, False, dtype)
    assert bool(torch.isnan(wide[:, 0]).all()) and bool(torch.isnan(wide[:, n + 1:]).all())
    # in place: B is X
    d_bx = dense(B.astype(dtype), layout)
    sp.triangular_solve(a, lo, ex, d_bx, d_bx)
    assert not TU.violations(M, B, G.host(d_bx), False, False, dtype)


# ---- plan sharing ------------------------------------------------------------------------------------------------------
def test_one_info_serves_vector_and_matrix_solves_alternately(gpu):
    rng = np.random.default_rng(41)
    M = TU.system("tri3000", True, False)
    m = M.shape[0]
    a = on_device(M, np.float64)
    up, ex = sp.upper_triangle, sp.explicit_diagonal
    b, x = G.dev(rng.random(m) + 0.5), torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
    B = TU.rhs(m, 6)
    for first in ("vector", "matrix"):   # a plan made by either form of inspect serves both forms of solve
        if first == "vector":
            info = sp.triangular_solve_inspect(a, up, ex, b, x)
        else:
            info = sp.triangular_solve_inspect(a, up, ex, dense(B, "L"), nan_like(m, 6, torch.float64, "R"))
        state = info.state_
        for _ in range(3):
            X = solve_block(a, B, True, False, np.float64, "R", "L", info)
            assert not TU.violations(M, B, X, True, False, np.float64)
            assert info.state_ is state
            x.fill_(float("nan"))
            sp.triangular_solve(info, a, up, ex, b, x)
            assert not TU.violations(M, G.host(b)[:, None], G.host(x)[:, None], True, False, np.float64)
            assert info.state_ is state
        info.state_.check_status()


# ---- graphs ------------------------------------------------------------------------------------------------------------
def _capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


@pytest.mark.parametrize("layout", ["R", "L"])
def test_matrix_solve_with_inspect_is_capturable(gpu, layout):
    rng = np.random.default_rng(21)
    n, k, cols = 30000, 6, 8
    rows = np.repeat(np.arange(n), k)
    cc = (rng.random(n * k) * rows).astype(np.int64)
    keep = cc < rows
    S = sps.csr_matrix(((rng.random(keep.sum()) - 0.5) * (0.5 / k), (rows[keep], cc[keep])), shape=(n, n))
    M = (S + sps.diags(1.0 + rng.random(n))).tocsr()
    a = on_device(M, np.float32)
    lo, ex = sp.lower_triangle, sp.explicit_diagonal
    b = dense(np.zeros((n, cols), np.float32), layout)
    x = nan_like(n, cols, torch.float32, layout)
    info = sp.triangular_solve_inspect(a, lo, ex, b, x)
    assert info.state_.info()["levels"] > 20
    solve = lambda: sp.triangular_solve(info, a, lo, ex, b, x)
    g = _capture(solve)   # (its warm-up call is the one eager solve that sizes the plan's control words)
    for seed in range(4):
        B = TU.rhs(n, cols, seed=seed)
        b.copy_(G.dev(B.astype(np.float32)))
        x.fill_(float("nan"))
        if seed == 2:
            solve()   # an ordinary solve between replays
        else:
            g.replay()
        torch.cuda.synchronize()
        bad = TU.violations(M, B, G.host(x), False, False, np.float32)
        assert not bad, f"replay {seed}: {bad}"


def test_first_matrix_solve_of_a_plan_cannot_be_recorded(gpu):
    M = TU.system("tri3000", False, False)
    m = M.shape[0]
    a = on_device(M, np.float32)
    lo, ex = sp.lower_triangle, sp.explicit_diagonal
    b, x = torch.ones((m, 4), device="cuda"), torch.zeros((m, 4), device="cuda")
    info = sp.triangular_solve_inspect(a, lo, ex, b, x)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(Exception):
        with torch.cuda.graph(g):
            sp.triangular_solve(info, a, lo, ex, b, x)
    torch.cuda.synchronize()
    sp.triangular_solve(info, a, lo, ex, b, x)   # the plan is still usable
    assert not TU.violations(M, np.ones((m, 4)), G.host(x), False, False, np.float32)


# ---- status ------------------------------------------------------------------------------------------------------------
def test_status_is_clean_after_matrix_solves(gpu):
    """The block solve has no device-side wait that could give up; the plan's status word, shared with the vector solve,
    reads 0 after it (spblas_gfx950_sptrsv_status)."""
    M = TU.system("tri3000", False, False)
    a = on_device(M, np.float32)
    B = TU.rhs(3000, 8)
    b, x = dense(B.astype(np.float32), "R"), nan_like(3000, 8, torch.float32, "R")
    info = sp.triangular_solve_inspect(a, sp.lower_triangle, sp.explicit_diagonal, b, x)
    info.state_.check_status()
    for _ in range(3):
        sp.triangular_solve(info, a, sp.lower_triangle, sp.explicit_diagonal, b, x)
        info.state_.check_status()
    assert not TU.violations(M, B, G.host(x), False, False, np.float32)


# ---- bench size --------------------------------------------------------------------------------------------------------
def test_lower_block_solve_at_bench_size_every_row_and_column(gpu):
    """The 4 M-row matrix of test_gpu_sptrsv.py::test_lower_solve_at_bench_size_every_row (same construction and seed) with
    n = 8 right-hand sides, fp32, both operands layout_right.  Every row of every column: (1) the backward bound evaluated
    in float64 on the device over the triangle the reference reads; (2) the forward bound against the oracle's column."""
    m, k, n = 4_000_000, 8, 8
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = torch.arange(m, device="cuda").repeat_interleave(k)
    cols = (torch.rand(m * k, device="cuda", generator=g, dtype=torch.float64) * rows.double()).long().clamp_(min=0)
    cols = torch.minimum(cols, rows)
    vals = (torch.rand(m * k, device="cuda", generator=g) - 0.5) * (0.5 / k)
    rp = torch.arange(m + 1, device="cuda", dtype=torch.int64) * (k + 1)
    colind = torch.empty(m * (k + 1), dtype=torch.int32, device="cuda")
    values = torch.empty(m * (k + 1), device="cuda")
    colind.view(m, k + 1)[:, :k] = cols.view(m, k).int()
    colind.view(m, k + 1)[:, k] = torch.arange(m, device="cuda", dtype=torch.int32)
    values.view(m, k + 1)[:, :k] = vals.view(m, k)
    values.view(m, k + 1)[:, k] = 1.0 + torch.rand(m, device="cuda", generator=g)
    del rows, cols, vals
    nnz = m * (k + 1)
    a = sp.csr_view(values, rp.int(), colind, (m, m), nnz)
    b = torch.rand((m, n), device="cuda", generator=g)
    x = torch.full((m, n), float("nan"), device="cuda")
    info = sp.triangular_solve_inspect(a, sp.lower_triangle, sp.explicit_diagonal, b, x)
    sp.triangular_solve(info, a, sp.lower_triangle, sp.explicit_diagonal, b, x)
    info.state_.check_status()
    assert bool(torch.isfinite(x).all())
    row_of = torch.arange(m, device="cuda").repeat_interleave(k + 1)
    pos = torch.arange(nnz, device="cuda") % (k + 1)
    read = (colind.long() < row_of) | (pos == k)
    kk = torch.zeros(m, dtype=torch.float64, device="cuda").index_add_(0, row_of, read.double()) + 2
    tol = torch.clamp(0.5 * kk * float(np.finfo(np.float32).eps), min=util.TOL[np.dtype(np.float32)])
    rp_h, ci_h, v_h = rp.int().cpu().numpy(), colind.cpu().numpy(), values.cpu().numpy()
    ftol = max(100 * util.TOL[np.dtype(np.float32)], 0.5 * (k + 3) * float(np.finfo(np.float32).eps))
    for j in range(n):
        xd, bd = x[:, j].double(), b[:, j].double()
        term = torch.where(read, values.double() * xd[colind.long()], torch.zeros((), dtype=torch.float64, device="cuda"))
        tx = torch.zeros(m, dtype=torch.float64, device="cuda").index_add_(0, row_of, term)
        norm = bd.abs().index_add_(0, row_of, term.abs())
        bad = ~((tx - bd).abs() <= tol * norm)
        assert not bool(bad.any()), (f"column {j}: {int(bad.sum())} rows out of the backward-error bound, first "
                                     f"{torch.nonzero(bad).flatten()[:5].tolist()}")
        del term, tx, norm, bad
        ref = oracle.triangular_solve((m, m), rp_h, ci_h, v_h, b[:, j].cpu().numpy()).astype(np.float64)
        scale = np.maximum(np.abs(ref), np.abs(ref).max() * 1e-3 + 1e-30)
        err = np.abs(xd.cpu().numpy() - ref) / scale
        assert err.max() <= ftol, f"column {j}: max rel err vs oracle {err.max()} at row {err.argmax()}"
    del row_of, pos, read, kk, tol
    torch.cuda.empty_cache()


# ---- more than 2^31 elements -------------------------------------------------------------------------------------------
def test_more_than_two_to_the_31_elements(gpu):
    """m = 2^21, n = 1025, fp32: m * n > 2^31, so every element offset into B and X has to be 64-bit.  Block-diagonal matrix
    of 4 x 4 lower blocks (4 levels of m / 4 rows).  Checked on the device in float64, in slabs of columns: the backward
    bound on every (row, column), and the forward bound against a float64 forward substitution of the blocks."""
    m, n = 1 << 21, 1025
    need = 2 * m * n * 4 + 10 * 2 ** 30
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB are free")
    nb = m // 4
    g = torch.Generator(device="cuda").manual_seed(7)
    # row 4 i + q holds columns 4 i .. 4 i + q: q strict entries, then the diagonal
    lens = torch.tensor([1, 2, 3, 4], device="cuda").repeat(nb)
    rp = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    rp[1:] = torch.cumsum(lens, 0)
    nnz = int(rp[-1])
    row_of = torch.arange(m, device="cuda").repeat_interleave(lens)
    pos = torch.arange(nnz, device="cuda") - rp[row_of]
    colind = (row_of - row_of % 4 + pos).int()
    isdiag = colind.long() == row_of
    values = torch.where(isdiag, 1.0 + torch.rand(nnz, device="cuda", generator=g),
                         (torch.rand(nnz, device="cuda", generator=g) - 0.5) * 0.5)
    a = sp.csr_view(values, rp.int(), colind, (m, m), nnz)
    b = torch.rand((m, n), device="cuda", generator=g)
    x = torch.full((m, n), float("nan"), device="cuda")
    assert b.numel() > 2 ** 31
    info = sp.triangular_solve_inspect(a, sp.lower_triangle, sp.explicit_diagonal, b, x)
    assert info.state_.info()["levels"] == 4
    sp.triangular_solve(info, a, sp.lower_triangle, sp.explicit_diagonal, b, x)
    torch.cuda.synchronize()
    # dense 4 x 4 blocks in float64: L[i, q, p]
    L = torch.zeros((nb, 4, 4), dtype=torch.float64, device="cuda")
    L[row_of // 4, row_of % 4, pos] = values.double()
    tol, ftol = util.TOL[np.dtype(np.float32)], 100 * util.TOL[np.dtype(np.float32)]   # (k <= 6: 0.5 k eps is below both)
    for j0 in range(0, n, 64):
        xs = x[:, j0:j0 + 64].double().view(nb, 4, -1)
        bs = b[:, j0:j0 + 64].double().view(nb, 4, -1)
        assert bool(torch.isfinite(xs).all()), f"columns {j0}..: unsolved elements"
        resid = (torch.bmm(L, xs) - bs).abs()
        norm = bs.abs() + torch.bmm(L.abs(), xs.abs())
        bad = ~(resid <= tol * norm)
        assert not bool(bad.any()), f"columns {j0}..: {int(bad.sum())} elements out of the backward-error bound"
        ref = torch.zeros_like(xs)
        for q in range(4):
            acc = bs[:, q, :].clone()
            for p in range(q):
                acc -= L[:, q, p, None] * ref[:, p, :]
            ref[:, q, :] = acc / L[:, q, q, None]
        scale = torch.maximum(ref.abs(), ref.abs().amax(dim=(0, 1), keepdim=True) * 1e-3 + 1e-30)
        err = ((xs - ref).abs() / scale).max()
        assert float(err) <= ftol, f"columns {j0}..: max rel err vs the float64 substitution {float(err)}"
        del xs, bs, resid, norm, bad, ref, scale
    del b, x, L
    torch.cuda.empty_cache()


# ---- leaks -------------------------------------------------------------------------------------------------------------
def test_200_matrix_solves_do_not_grow_device_memory(gpu):
    rng = np.random.default_rng(1)
    tn = 20000
    S = sps.tril(sps.random(tn, tn, density=0.0005, format="csr", random_state=rng), -1)
    T = (S + sps.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsr()
    a = on_device(T, np.float32)
    lo, ex = sp.lower_triangle, sp.explicit_diagonal
    bs = {lay: dense(TU.rhs(tn, 8).astype(np.float32), lay) for lay in "RL"}
    xs = {lay: nan_like(tn, 8, torch.float32, lay) for lay in "RL"}

    def cycle(i):
        lay = "RL"[i % 2]
        if i % 10 == 0:   # now and then a fresh plan as well: create / solve / destroy
            sp.triangular_solve(a, lo, ex, bs[lay], xs[lay])
        else:
            sp.triangular_solve(info, a, lo, ex, bs[lay], xs["RL"[(i // 2) % 2]])

    info = sp.triangular_solve_inspect(a, lo, ex, bs["R"], xs["R"])
    for i in range(20):   # warm-up: pools and caches reach their size
        cycle(i)
    torch.cuda.synchronize()
    gc.collect()
    free0, _ = torch.cuda.mem_get_info()
    for i in range(200):
        cycle(i)
    torch.cuda.synchronize()
    gc.collect()
    free1, _ = torch.cuda.mem_get_info()
    lost = free0 - free1
    assert lost < 8 * 2 ** 20, f"free device memory fell by {lost / 2**20:.1f} MiB over 200 matrix solves"
