"""-m gpu tests of ilu0_inspect / ilu0 / ilu0_status (spblas_gfx950_ilu0_*, csrc/ilu0.hip).  Every test fails on a backend without
the feature: the names do not exist there.

Generators and checkers: tests/ilu_util.py (proved on the host by tests/test_ilu0_cpu.py).  The exact families must come back
BIT FOR BIT in fp32 and fp64 (the expected factor is known by construction, nothing is factored on the host here); random data
pass the residual bound of ilu_util.residual_violations.  In every call `lu` is prefilled with NaN and all arrays are longer than
nnz, with NaN (values) and a wild column behind the end."""
import os
import subprocess

import numpy as np
import pytest
import torch

import gpu_util as G
import ilu_util as U
import ladder_tt as TT
import spblas_reference_amd as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
PAD = 5


class Dev:
    """A pattern on the device with over-long arrays; views for A (values `a`) and for a NaN-filled LU over the same structure."""

    def __init__(self, rowptr, colind, a_values, dtype):
        self.rowptr, self.colind, self.dtype = rowptr, colind, np.dtype(dtype)
        self.m, self.nnz = rowptr.size - 1, int(colind.size)
        self.d_rp = G.dev(rowptr.astype(np.int32))
        self.d_ci = G.dev(np.concatenate([colind.astype(np.int32), np.full(PAD, 2 ** 30, np.int32)]))
        self.a_host = np.concatenate([np.asarray(a_values, np.float64), np.full(PAD, np.nan)]).astype(dtype)
        self.d_a = G.dev(self.a_host)
        self.a = sp.csr_view(self.d_a, self.d_rp, self.d_ci, (self.m, self.m), self.nnz)

    def new_lu(self):
        d_lu = torch.full((self.nnz + PAD,), float("nan"), dtype=self.d_a.dtype, device="cuda")
        return sp.csr_view(d_lu, self.d_rp, self.d_ci, (self.m, self.m), self.nnz)

    def factor(self, info=None, inplace=False):
        """One factor call; returns the LU values on the host (nnz of them) after checking what must stay untouched."""
        lu = self.a if inplace else self.new_lu()
        if info is None:
            sp.ilu0(self.a, lu)
        else:
            sp.ilu0(info, self.a, lu)
        got = G.host(lu.values())
        assert np.isnan(got[self.nnz:]).all(), "the factor wrote behind nnz"
        if not inplace:
            assert np.array_equal(U.bits(G.host(self.d_a)), U.bits(self.a_host)), "an out-of-place factor changed A's values"
        return got[:self.nnz]


def run_exact(rowptr, colind, dtype, seed=0, expect_lanes=None):
    a_vals, want = U.exact_system(rowptr, colind, seed=seed)
    d = Dev(rowptr, colind, a_vals, dtype)
    info = sp.ilu0_inspect(d.a)
    pred = U.predicted_info(rowptr, colind)
    assert info.state_.info() == pred
    if expect_lanes is not None:
        assert pred["lanes_per_row"] == expect_lanes
    got = d.factor(info)
    assert U.exact_violations(got, want, rowptr, colind) == []
    assert sp.ilu0_status(info) == -1
    return d, info, got


# ---- row shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("limit,extra,lanes", U.lane_cases())
def test_row_shapes_in_a_narrow_run(gpu, limit, extra, lanes, dtype):
    """Every rung of ilu_util.shape_specs for each lane count the plan can choose (means of exactly 6 / 24 / 96 and one entry
    more), target rows and pivot rows alike, rows of cap - 1, cap, cap + 1 entries around the fast path's LDS room: the shaped
    rows depend on each other, so they run in the single-workgroup kernel."""
    rowptr, colind, G_, specs, front, _ = U.shape_system(limit, extra)
    assert G_ == lanes
    cap = U.lds_cap(lanes)
    lens = np.diff(rowptr)[front:front + len(specs)]
    assert {cap - 1, cap, cap + 1} <= set(lens.tolist()) and lens.max() == 601
    run_exact(rowptr, colind, dtype, seed=limit + extra, expect_lanes=lanes)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("limit,extra", [(6, 0), (6, 1), (24, 1)])
def test_row_shapes_in_wide_levels(gpu, limit, extra, dtype):
    """The same ladders, 130 independent copies interleaved: every level is at least `narrow` rows wide and takes the launch per
    level."""
    copies = TT.trsv_limits()["narrow"] + 2
    rowptr, colind, lanes, specs, front, _ = U.shape_system(limit, extra, copies=copies)
    d, info, _ = run_exact(rowptr, colind, dtype, seed=limit + extra + 7, expect_lanes=lanes)
    inf = info.state_.info()
    assert inf["launches_per_factor"] == inf["levels"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lanes,upper", [(4, (0, 3)), (8, (9, 12)), (16, (30, 40)), (64, (110, 120))])
def test_wide_and_narrow_levels_at_every_lane_count(gpu, lanes, upper, dtype):
    """Wide -> narrow -> wide with rows not sorted by level, at a mean row length for each lane count; two rows of the last
    (wide) level are longer than the fast path's LDS room and read pivot rows, so the long path does real pivot work in the
    launch per level at every lane count."""
    widths = [400, 130, 3, 2, 140]
    rowptr, colind, lev = U.level_pattern(widths, seed=lanes, upper=upper, long_rows=2, long_len=U.lds_cap(lanes) + 3)
    long_rows = np.flatnonzero(np.diff(rowptr) > U.lds_cap(lanes))
    assert long_rows.size == 2 and (lev[long_rows] == len(widths) - 1).all()
    assert (U.diag_positions(rowptr, colind)[long_rows] > rowptr[long_rows]).all()      # each has strict-lower entries
    run_exact(rowptr, colind, dtype, seed=lanes, expect_lanes=lanes)


# ---- match patterns --------------------------------------------------------------------------------------------------
def match_pattern_rows(n_pivot_cols=9):
    """One (pivot row, second pivot row, target row) triple per case on 80 rows: rows c and 10 + c are pivot rows with the upper
    columns K, row 40 + c is the target with the lower columns {c, 10 + c} and, right of them, the columns the case asks for."""
    m = 80
    rng = np.random.default_rng(5)
    rows = [[] for _ in range(m)]
    cases = ["all", "none", "first", "last", "alternating", "beyond", "extra"]
    for c, case in enumerate(cases):
        t = 40 + c
        pool = np.arange(20, 70)
        K = np.sort(rng.choice(pool, n_pivot_cols, replace=False))
        rest = np.setdiff1d(pool, K)
        if case == "all":
            T = K
        elif case == "none":
            T = rest[::3]
        elif case == "first":
            T = np.concatenate([K[:1], rest[rest > K[0]][::4]])
        elif case == "last":
            T = np.concatenate([K[-1:], rest[rest < K[-1]][::4]])
        elif case == "alternating":
            T = np.concatenate([K[::2], rest[::5]])
        elif case == "beyond":
            T = K[K < 50]
            K = np.concatenate([K, [72, 75, 79]])
        else:
            T = np.concatenate([K, rest[::2]])
        rows[c] = list(K)
        rows[10 + c] = list(K)
        rows[t] = [c, 10 + c] + [int(x) for x in T if x != t]
    return rows, cases


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_pivot_cols", [3, 9, 21])
def test_match_patterns(gpu, n_pivot_cols, dtype):
    """Pivot columns against target columns: all hit, none, only the first, only the last, alternating, pivot columns beyond the
    target's last column, target entries the pivot row lacks -- with fewer pivot columns than lanes and several strides of them."""
    rows, cases = match_pattern_rows(n_pivot_cols)
    rowptr, colind = U.pattern_from_rows(rows)
    run_exact(rowptr, colind, dtype, seed=n_pivot_cols)


# ---- levels ------------------------------------------------------------------------------------------------------------
def _level_cases():
    n = TT.trsv_limits()["narrow"]
    return [[300, n - 1], [300, n], [300, n + 1], [5], [5, 3], [200, 3, 3], [200, 3, 130, 2], [130] * 5, [200, 130, 3, 3, 140],
            [3, 3, 200, 4]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(_level_cases())))
def test_level_widths_and_sequences(gpu, case, dtype):
    widths = _level_cases()[case]
    rowptr, colind, _ = U.level_pattern(widths, seed=case)
    d, info, _ = run_exact(rowptr, colind, dtype, seed=case)
    assert info.state_.info()["launches_per_factor"] == len(TT.groups_of(widths, TT.trsv_limits()["narrow"]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [4096, 4097])
def test_bidiagonal_chain_is_one_long_narrow_run(gpu, m, dtype):
    rowptr, colind = U.pattern_from_rows([[i - 1] if i else [] for i in range(m)])
    d, info, _ = run_exact(rowptr, colind, dtype, seed=m)
    assert info.state_.info()["levels"] == m and info.state_.info()["launches_per_factor"] == 1


# ---- degenerate shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_shapes(gpu, dtype):
    empty = Dev(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), dtype)
    info = sp.ilu0_inspect(empty.a)
    assert info.state_.info()["levels"] == 0
    assert empty.factor(info).size == 0 and sp.ilu0_status(info) == -1
    run_exact(*U.pattern_from_rows([[]]), dtype)                               # m = 1
    run_exact(*U.pattern_from_rows([[] for _ in range(300)]), dtype)           # a diagonal matrix
    run_exact(*U.pattern_from_rows([list(range(64))] * 64), dtype, seed=3)     # one dense 64 x 64 block


# ---- in place and determinism ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place_out_of_place_and_repeated_calls_give_the_same_bits(gpu, dtype):
    rowptr, colind = U.random_pattern(3000, 12, seed=1, band=200)
    vals = U.dominant_values(rowptr, colind, seed=2)
    d = Dev(rowptr, colind, vals, dtype)
    info = sp.ilu0_inspect(d.a)
    first = d.factor(info)
    second = d.factor(info)
    plan_free = d.factor(None)
    inplace = d.factor(info, inplace=True)
    for other in (second, plan_free, inplace):
        assert np.array_equal(U.bits(first), U.bits(other))
    assert U.residual_violations(rowptr, colind, vals.astype(dtype), first, dtype) == []


# ---- use with the solves -----------------------------------------------------------------------------------------------
def _no_fill_patterns():
    m = 200
    tri = [[i - 1, i + 1] if 0 < i < m - 1 else ([1] if i == 0 else [m - 2]) for i in range(m)]
    arrow = [[m - 1] for _ in range(m - 1)] + [list(range(m - 1))]
    return {"tridiagonal": tri, "arrow": arrow}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["tridiagonal", "arrow"])
def test_factor_then_two_solves_on_the_one_lu_view(gpu, name, dtype):
    """A no-fill exact family: A = L U in full, so with b = L (U x_true) in float64 the two triangular solves on the ONE LU view
    must return the dyadic x_true exactly -- as vectors and as a block of three columns."""
    rowptr, colind = U.pattern_from_rows(_no_fill_patterns()[name])
    m = rowptr.size - 1
    a_vals, want = U.exact_system(rowptr, colind, seed=11)
    L, Up = U.split_lu(rowptr, colind, want)
    assert (L @ Up).nnz <= colind.size, "the family has fill"
    x_true = np.random.default_rng(3).choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], m)
    b = L @ (Up @ x_true)
    d = Dev(rowptr, colind, a_vals, dtype)
    lu = d.new_lu()
    info = sp.ilu0_inspect(d.a)
    sp.ilu0(info, d.a, lu)
    assert U.exact_violations(G.host(lu.values())[:d.nnz], want, rowptr, colind) == []
    lo, up = (sp.lower_triangle, sp.implicit_unit_diagonal), (sp.upper_triangle, sp.explicit_diagonal)
    td = d.d_a.dtype
    d_b, d_y, d_x = G.dev(b.astype(dtype)), torch.full((m,), float("nan"), dtype=td, device="cuda"), \
        torch.full((m,), float("nan"), dtype=td, device="cuda")
    sp.triangular_solve(lu, *lo, d_b, d_y)
    sp.triangular_solve(lu, *up, d_y, d_x)
    assert np.array_equal(U.bits(G.host(d_x)), U.bits(x_true.astype(dtype)))
    B = np.stack([b * f for f in TT.BLOCK_FACTORS], axis=1).astype(dtype)
    d_B = G.dev(B)
    d_Y, d_X = torch.full_like(d_B, float("nan")), torch.full_like(d_B, float("nan"))
    sp.triangular_solve(lu, *lo, d_B, d_Y)
    sp.triangular_solve(lu, *up, d_Y, d_X)
    X_true = np.stack([x_true * f for f in TT.BLOCK_FACTORS], axis=1).astype(dtype)
    assert np.array_equal(U.bits(G.host(d_X)), U.bits(X_true))


# ---- pivots --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("zeros", [(150,), (230, 90), (0,)])
def test_zero_pivots_are_reported_and_do_not_stop_the_factorisation(gpu, zeros, dtype):
    rowptr, colind, _ = U.level_pattern([200, 130, 40, 30], seed=9)
    a_vals, want = U.exact_system(rowptr, colind, seed=9, zero_pivots=zeros)
    d = Dev(rowptr, colind, a_vals, dtype)
    info = sp.ilu0_inspect(d.a)
    assert sp.ilu0_status(info) == -1       # nothing factored yet
    got = d.factor(info)
    assert sp.ilu0_status(info) == min(zeros)
    clean = U.independent_rows(rowptr, colind, zeros)
    for z in zeros:      # the zero pivots are independent of each other
        others = [o for o in zeros if o != z]
        assert not others or U.independent_rows(rowptr, colind, others)[z]
    assert 0 < clean.sum() < clean.size
    assert U.exact_violations(got, want, rowptr, colind, rows_mask=clean) == []
    # a clean matrix on the same plan reports -1 again
    a2, want2 = U.exact_system(rowptr, colind, seed=10)
    d.d_a[:d.nnz].copy_(G.dev(a2.astype(dtype)))
    d.a_host[:d.nnz] = a2.astype(dtype)
    assert U.exact_violations(d.factor(info), want2, rowptr, colind) == []
    assert sp.ilu0_status(info) == -1


# ---- structure errors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["unsorted", "duplicate", "no_diagonal", "column_out_of_range"])
def test_structure_errors_are_value_errors(gpu, what):
    rowptr, colind = U.pattern_from_rows([[i - 1, i + 1] if 0 < i < 49 else [] for i in range(50)])
    colind = colind.copy()
    p = int(rowptr[20])                      # row 20 holds 19, 20, 21
    if what == "unsorted":
        colind[p], colind[p + 1] = colind[p + 1], colind[p]
    elif what == "duplicate":
        colind[p + 2] = 20
    elif what == "no_diagonal":
        colind[p + 1] = 21
        colind[p + 2] = 22
    else:
        colind[p + 2] = 50
    d = Dev(rowptr, colind, np.ones(colind.size), np.float32)
    with pytest.raises(ValueError):
        sp.ilu0_inspect(d.a)
    with pytest.raises(ValueError):
        sp.ilu0(d.a, d.new_lu())


def test_factor_refuses_other_structure_arrays_than_the_plans(gpu):
    """The plan holds positions into the arrays it was made from: equal sizes at other addresses are a PLAN_MISMATCH."""
    from spblas_reference_amd import _capi
    rowptr, colind = U.pattern_from_rows([[i - 1] if i else [] for i in range(50)])
    d = Dev(rowptr, colind, np.ones(colind.size), np.float32)
    info = sp.ilu0_inspect(d.a)
    plan, lib = info.state_, _capi.lib()
    call = lambda rp, ci: lib.spblas_gfx950_ilu0_factor(plan.hd.h, plan.plan, d.m, d.nnz, rp.data_ptr(), ci.data_ptr(),
                                                        d.d_a.data_ptr(), d.d_a.data_ptr(), _capi.F32)
    assert call(d.d_rp.clone(), d.d_ci) == _capi.PLAN_MISMATCH
    assert call(d.d_rp, d.d_ci.clone()) == _capi.PLAN_MISMATCH
    assert call(d.d_rp, d.d_ci) == _capi.SUCCESS
    torch.cuda.synchronize()


# ---- graph ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_factor_and_both_solves_in_one_graph(gpu, dtype):
    """After one eager call of each solve (the first solve of a plan sizes its control words), factor + lower solve + upper solve
    are captured ONCE -- the factor from its very first call -- and replayed after A's values were rewritten in place: the
    factor and x are those of the new values, and the status word is the replay's own.  A factor call therefore only enqueues
    its copy, the reset of the status word and the level launches, and synchronises nothing."""
    rowptr, colind = U.pattern_from_rows(_no_fill_patterns()["tridiagonal"])
    m = rowptr.size - 1
    systems = []
    for seed in (21, 22):
        a_vals, want = U.exact_system(rowptr, colind, seed=seed)
        L, Up = U.split_lu(rowptr, colind, want)
        x_true = np.random.default_rng(seed).choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], m)
        systems.append((a_vals, want, L @ (Up @ x_true), x_true))
    d = Dev(rowptr, colind, systems[0][0], dtype)
    lu = d.new_lu()
    td = d.d_a.dtype
    d_b = G.dev(systems[0][2].astype(dtype))
    d_y = torch.full((m,), float("nan"), dtype=td, device="cuda")
    d_x = torch.full((m,), float("nan"), dtype=td, device="cuda")
    info = sp.ilu0_inspect(d.a)
    lo_info = sp.triangular_solve_inspect(lu, sp.lower_triangle, sp.implicit_unit_diagonal, d_b, d_y)
    up_info = sp.triangular_solve_inspect(lu, sp.upper_triangle, sp.explicit_diagonal, d_y, d_x)
    lower = lambda: sp.triangular_solve(lo_info, lu, sp.lower_triangle, sp.implicit_unit_diagonal, d_b, d_y)
    upper = lambda: sp.triangular_solve(up_info, lu, sp.upper_triangle, sp.explicit_diagonal, d_y, d_x)
    lu.values()[:d.nnz].copy_(d.d_a[:d.nnz])     # something finite for the eager solves
    lower()
    upper()
    torch.cuda.synchronize()
    lu.values().fill_(float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.ilu0(info, d.a, lu)
        lower()
        upper()
    for a_vals, want, b, x_true in (systems[1], systems[0], systems[1]):
        d.d_a[:d.nnz].copy_(G.dev(a_vals.astype(dtype)))
        d_b.copy_(G.dev(b.astype(dtype)))
        lu.values().fill_(float("nan"))
        d_x.fill_(float("nan"))
        g.replay()
        assert U.exact_violations(G.host(lu.values())[:d.nnz], want, rowptr, colind) == []
        assert np.array_equal(U.bits(G.host(d_x)), U.bits(x_true.astype(dtype)))
        assert sp.ilu0_status(info) == -1


# ---- random --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,per_row,band", [(2000, 6, None), (2000, 24, None), (2000, 96, None), (2 ** 18, 9, 4000)])
def test_random_diagonally_dominant_matrices_pass_the_residual_check(gpu, m, per_row, band, dtype):
    rowptr, colind = U.random_pattern(m, per_row, seed=per_row, band=band)
    vals = U.dominant_values(rowptr, colind, seed=per_row + 1).astype(dtype)
    d = Dev(rowptr, colind, vals, dtype)
    info = sp.ilu0_inspect(d.a)
    if m <= 2000:      # (restating the levels of the large matrix on the host would take longer than the rest of the test)
        assert info.state_.info() == U.predicted_info(rowptr, colind)
    assert info.state_.info()["lanes_per_row"] == TT.lanes_of(int(rowptr[-1]), m)
    got = d.factor(info)
    assert sp.ilu0_status(info) == -1
    assert U.residual_violations(rowptr, colind, vals, got, dtype) == []


# ---- the C++ example -------------------------------------------------------------------------------------------------------
def test_device_ilu0_example_runs(gpu):
    exe = os.path.join(ROOT, "examples", "device_ilu0")
    assert os.path.exists(exe), "examples/device_ilu0 is not built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
