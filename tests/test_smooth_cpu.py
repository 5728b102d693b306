"""Host-side proof of tests/smooth_util.py (no GPU): the model of smooth_prolongator equals the dense float64 reference of
(I - omega D_F^-1 A_F) T within its bound, each seeded mistake of the model fails a named case, the row sums of P are 1 on a
graph Laplacian, and a two-grid cycle with the smoothed P needs fewer CG iterations than with the tentative one."""
import os
from fractions import Fraction

import numpy as np
import pytest

import aggregate_util as A
import multicolor_util as MC
import smooth_util as S
import spblas_reference_amd as sp
from spblas_reference_amd import _build

DTYPES = [np.float32, np.float64]
OMEGA = 2.0 / 3.0


def cases():
    """name -> (graph, theta): the matrices the model is compared with the reference on (aggregates from the aggregate model)."""
    return {
        "lap7_6": (A.lap7(6), 0.0), "anisotropic_12x12": (A.anisotropic(12, 12), 0.25),
        "random_200x6": (A.random_graph(200, 6, 5), 0.25), "repeated_entries": (A.repeated_entries(), 0.25),
        "threshold_f32": (A.threshold(np.float32), 0.25), "threshold_f64": (A.threshold(np.float64), 0.25),
        "empty_rows": (A.empty_rows(), 0.0), "upper_bidiagonal_30": (A.upper_bidiagonal(30), 0.0),
    }


CASES = cases()


def aggregates(g, theta, dtype):
    got = A.model(g[0], g[1], g[2], theta, dtype)
    return got["agg"], got["n_agg"]


# ---- the exact fma -----------------------------------------------------------------------------------------------------------
def test_the_fma_rounds_once():
    # float32: (1 + 2^-23) + 2^-24 (1 - 2^-46) lies just below a tie.  Once: 1 + 2^-23.  Through float64 the sum first rounds
    # onto the tie, then to even: 1 + 2^-22.
    a, b, c = np.float32(2.0 ** -12 * (1 + 2.0 ** -23)), np.float32(2.0 ** -12 * (1 - 2.0 ** -23)), np.float32(1 + 2.0 ** -23)
    assert S.fma(a, b, c, np.float32) == np.float32(1 + 2.0 ** -23)
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(1 + 2.0 ** -22)
    # float64: the product's low half survives
    x = np.float64(1 + 2.0 ** -30)
    assert S.fma(x, x, np.float64(-1), np.float64) == np.float64(2.0 ** -29 + 2.0 ** -60) and x * x - 1 == 2.0 ** -29
    rng = np.random.default_rng(0)
    for dtype in DTYPES:
        T = np.dtype(dtype).type
        for _ in range(300):
            a, b, c = (T(t) for t in rng.standard_normal(3))
            r = S.fma(a, b, c, dtype)
            exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
            err = abs(Fraction(float(r)) - exact)
            for other in (np.nextafter(r, T(-np.inf)), np.nextafter(r, T(np.inf))):
                assert err <= abs(Fraction(float(other)) - exact)
    assert S.round_fraction(Fraction(1, 2 ** 150), np.float32) == 0 and S.round_fraction(Fraction(2) ** 128, np.float32) == np.inf
    assert S.round_fraction(Fraction(3, 2 ** 150), np.float32) == np.float32(2.0 ** -148)      # a tie: to even
    assert np.isnan(S.fma(np.float32(0), np.float32(np.inf), np.float32(1), np.float32))


# ---- model against the dense reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_the_dense_reference_within_the_bound(name, dtype):
    g, theta = CASES[name]
    agg, n = aggregates(g, theta, dtype)
    m = g[0].size - 1
    for omega in (OMEGA, 0.5, 1.0):
        mod = S.model(g[0], g[1], g[2], agg, n, omega, theta, dtype)
        assert S.check_structure(m, n, mod["p_rowptr"], mod["p_colind"]) == []
        ref = S.dense_reference(g[0], g[1], g[2], agg, n, omega, theta, dtype)
        assert S.against_reference(mod, ref, dtype) == [], (name, omega)
    if dtype == np.float64 and name == "lap7_6":
        diff = np.abs(mod["p_values"] - ref[mod["rows"], mod["p_colind"]])
        assert diff.max() <= 2.3e-16


def test_omega_zero_is_the_tentative_prolongator_on_the_pattern():
    g, theta = CASES["random_200x6"]
    agg, n = aggregates(g, theta, np.float32)
    mod = S.model(g[0], g[1], g[2], agg, n, 0.0, theta, np.float32)
    own = mod["p_colind"] == agg[mod["rows"]]
    assert (mod["p_values"][own] == 1).all() and (mod["p_values"][~own] == 0).all() and own.sum() == 200
    assert not np.signbit(mod["p_values"]).any()


def test_structure_is_the_union_of_the_own_aggregate_and_the_neighbours_aggregates():
    g, theta = CASES["repeated_entries"]
    agg, n = aggregates(g, theta, np.float32)
    p_rowptr, p_colind, seg_ptr, order, pos = S.structure(g[0], g[1], agg, n)
    for i in range(g[0].size - 1):
        want = sorted({int(agg[i])} | {int(agg[j]) for j in g[1][g[0][i]:g[0][i + 1]]})
        assert p_colind[p_rowptr[i]:p_rowptr[i + 1]].tolist() == want
    own = pos[seg_ptr[:-1]] < 0
    assert own.sum() == g[0].size - 1                       # every row's marker heads the run of its own aggregate
    # identity map: A's pattern plus the diagonal
    rp, ci, v = A.upper_bidiagonal(9)
    ident = np.arange(9, dtype=np.int32)
    mod = S.model(rp, ci, v, ident, 9, OMEGA, 0.0, np.float64)
    assert np.array_equal(mod["p_rowptr"], rp) and np.array_equal(mod["p_colind"], ci)


def test_special_rows():
    # empty rows are a single 1; a row without diagonal and without weak entries has dF = 0: T's row
    g, theta = CASES["empty_rows"]
    agg, n = aggregates(g, theta, np.float64)
    mod = S.model(g[0], g[1], g[2], agg, n, OMEGA, theta, np.float64)
    for i in range(1, 50, 2):
        e0, e1 = mod["p_rowptr"][i], mod["p_rowptr"][i + 1]
        assert e1 - e0 == 1 and mod["p_values"][e0] == 1 and mod["p_colind"][e0] == agg[i] and not mod["smoothed"][i]
    nd = S.without_diagonal(A.grid5(5, 4))
    mod = S.model(*nd, np.zeros(20, np.int32), 1, OMEGA, 0.0, np.float32)
    assert not mod["smoothed"].any() and (mod["p_values"] == 1).all() and mod["p_colind"].size == 20
    # the cancelling row
    g = S.cancelling_row()
    mod = S.model(*g, (np.arange(12) // 2).astype(np.int32), 6, OMEGA, 0.25, np.float32)
    assert mod["dF"][5] == 0 and not mod["smoothed"][5] and mod["smoothed"].sum() == 11
    e0, e1 = mod["p_rowptr"][5], mod["p_rowptr"][6]
    assert mod["p_values"][e0:e1].tolist() == [1.0 if c == 2 else 0.0 for c in mod["p_colind"][e0:e1]]
    # two stored diagonals: d uses the first (4), dF both (7)
    g = S.two_diagonals()
    mod = S.model(*g, np.zeros(20, np.int32), 1, 1.0, 0.0, np.float64)
    assert (mod["dF"] == 7).all() and (A.strength(*g, 0.0, np.float64)[1] == 4).all()
    # NaN / inf in one value touch their own row only (the entry is off-diagonal: no other row reads it)
    g, theta = CASES["lap7_6"]
    agg, n = aggregates(g, theta, np.float32)
    clean = S.model(*g, agg, n, OMEGA, 0.0, np.float32)
    rows = A._rows(g[0])
    p = int(np.flatnonzero((rows == 40) & (g[1] != 40))[0])
    for bad in (np.nan, np.inf):
        v = g[2].copy()
        v[p] = bad
        mod = S.model(g[0], g[1], v, agg, n, OMEGA, 0.0, np.float32)
        assert set(mod["rows"][mod["p_values"] != clean["p_values"]].tolist()) == {40}
    # ... and on the diagonal it reaches the rows that read d_40 through the strength rule as well
    v = g[2].copy()
    v[int(np.flatnonzero((rows == 40) & (g[1] == 40))[0])] = np.nan
    mod = S.model(g[0], g[1], v, agg, n, OMEGA, 0.0, np.float32)
    changed = set(mod["rows"][mod["p_values"] != clean["p_values"]].tolist())
    assert 40 in changed and changed <= {40} | set(rows[g[1] == 40].tolist())
    assert not mod["smoothed"][40]


def test_threshold_entries_one_ulp_below_are_lumped_and_entries_on_it_are_not():
    for dtype in DTYPES:
        g = A.threshold(dtype)
        agg = (np.arange(12) // 2).astype(np.int32)
        mod = S.model(*g, agg, 6, 0.5, 0.25, dtype)
        T = np.dtype(dtype).type
        below = np.nextafter(T(1), T(0))
        # interior row i: one neighbour strong (value 1), the other one ulp short and lumped: dF = 4 + below
        assert (mod["dF"][1:11] == T(4) + below).all() and mod["dF"][0] == 4 and mod["dF"][11] == 4
        assert (mod["terms"] <= 1).all() and mod["terms"].sum() == 12


# ---- seeded mistakes ---------------------------------------------------------------------------------------------------------
def _differs(g, agg, n, omega, theta, dtype, mistake):
    good = S.model(g[0], g[1], g[2], agg, n, omega, theta, dtype)
    bad = S.model(g[0], g[1], g[2], agg, n, omega, theta, dtype, mistake=mistake)
    if bad["p_colind"].size != good["p_colind"].size:
        return True
    return not np.array_equal(good["p_values"], bad["p_values"])


def test_dF_skips_weak_fails_the_anisotropic_case():
    g, theta = CASES["anisotropic_12x12"]
    agg, n = aggregates(g, theta, np.float32)
    assert _differs(g, agg, n, OMEGA, theta, np.float32, "dF_skips_weak")
    bad = S.model(g[0], g[1], g[2], agg, n, OMEGA, theta, np.float32, mistake="dF_skips_weak")
    assert S.against_reference(bad, S.dense_reference(g[0], g[1], g[2], agg, n, OMEGA, theta, np.float32), np.float32) != []


def order_sensitive():
    """One row (1, [2^24, 1, -2^24] off the diagonal 1) whose three strong entries lie in one foreign aggregate: ascending,
    ((2^24 + 1) - 2^24) is 0 in float32; descending, ((-2^24 + 1) + 2^24) is 1."""
    rp = np.array([0, 4, 5, 6, 7], np.int32)
    ci = np.array([0, 1, 2, 3, 1, 2, 3], np.int32)
    v = np.array([1.0, 2.0 ** 24, 1.0, -2.0 ** 24, 1.0, 1.0, 1.0])
    return (rp, ci, v), np.array([0, 1, 1, 1], np.int32), 2


def test_sums_descending_fails_the_order_sensitive_row():
    g, agg, n = order_sensitive()
    good = S.model(*g, agg, n, 1.0, 0.0, np.float32)
    bad = S.model(*g, agg, n, 1.0, 0.0, np.float32, mistake="sums_descending")
    assert good["p_values"][:2].tolist() == [0.0, 0.0] and bad["p_values"][:2].tolist() == [0.0, -1.0]
    assert S.model(*g, agg, n, 1.0, 0.0, np.float64)["p_values"][:2].tolist() == [0.0, -1.0]
    # The order of a sum moves a value by rounding only, so the float64 reference cannot tell the two orders apart: both lie
    # inside its bound.  That is why the device is compared with the model bit for bit and not with the reference alone.
    ref = S.dense_reference(*g, agg, n, 1.0, 0.0, np.float32)
    assert S.against_reference(good, ref, np.float32) == [] and S.against_reference(bad, ref, np.float32) == []


def test_own_marker_dropped_fails_the_foreign_rows():
    g, agg, n = S.foreign_rows()
    good = S.model(*g, agg, n, OMEGA, 0.0, np.float32)
    bad = S.model(*g, agg, n, OMEGA, 0.0, np.float32, mistake="own_marker_dropped")
    assert good["p_colind"].size == 2 * 40 - 1 and bad["p_colind"].size == 39
    assert S.against_reference(good, S.dense_reference(*g, agg, n, OMEGA, 0.0, np.float32), np.float32) == []


def test_diag_in_acc_fails_the_laplacian():
    g, theta = CASES["lap7_6"]
    agg, n = aggregates(g, theta, np.float64)
    assert _differs(g, agg, n, OMEGA, theta, np.float64, "diag_in_acc")
    bad = S.model(g[0], g[1], g[2], agg, n, OMEGA, theta, np.float64, mistake="diag_in_acc")
    assert S.against_reference(bad, S.dense_reference(g[0], g[1], g[2], agg, n, OMEGA, theta, np.float64), np.float64) != []


# ---- what the feature is for -------------------------------------------------------------------------------------------------
def test_row_sums_are_one_on_a_graph_laplacian():
    g = S.graph_laplacian(300, 4, 1)
    for dtype in DTYPES:
        agg, n = aggregates(g, 0.0, dtype)
        mod = S.model(*g, agg, n, OMEGA, 0.0, dtype)
        sums = np.add.reduceat(mod["p_values"].astype(np.float64), mod["p_rowptr"][:-1])
        slack = np.add.reduceat(S.bound(mod, dtype), mod["p_rowptr"][:-1])
        assert (np.abs(sums - 1) <= slack).all() and mod["smoothed"].all()


def test_the_smoothed_prolongator_cuts_the_two_grid_iterations():
    plain, smooth = [], []
    for n in (8, 12, 16):
        g = A.lap7(n)
        m = n ** 3
        agg, k = aggregates(g, 0.0, np.float64)
        mod = S.model(*g, agg, k, OMEGA, 0.0, np.float64)
        T0 = S.model(*g, agg, k, 0.0, 0.0, np.float64)                     # omega = 0: T on P's pattern
        plain.append(S.two_grid_iterations(*g, S.as_csr(T0, m, k)))
        smooth.append(S.two_grid_iterations(*g, S.as_csr(mod, m, k)))
    print("two-grid CG iterations at 8 / 12 / 16: plain", plain, "smoothed", smooth)
    assert all(s < p for s, p in zip(smooth, plain))
    assert smooth[2] - smooth[0] <= plain[2] - plain[0]


# ---- generators and layers ---------------------------------------------------------------------------------------------------
def test_capacity_rows_reach_every_team_width_and_both_paths():
    for lanes in (4, 8, 16, 64):
        g, lengths = S.capacity_rows(lanes)
        cap = S.stage_capacity(lanes)
        assert np.diff(g[0]).tolist() == lengths and {0, 1, 2, cap - 1, cap, cap + 1} <= set(lengths)
    g, agg, n = S.hub_with_agg(5000)
    assert np.diff(g[0]).max() == 5001 > S.stage_capacity(A.lanes_for(g[0], g[1]))


def test_source_example_and_exports_are_in_place():
    assert "smooth.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "smooth.hip"))
    assert "device_smoothed_aggregation" in _build.EXAMPLES
    with open(os.path.join(_build.CSRC, "smooth.hip")) as f:
        assert f"#define SM_STAGE_PER_LANE {S.STAGE_PER_LANE}\n" in f.read()
    for name in sp.SMOOTH_EXPORTS:
        assert hasattr(sp, name)
    covered = {n for names in S.STREAM_CASES.values() for n in names}
    assert sorted(set(sp.SMOOTH_EXPORTS) ^ covered) == []


def test_host_side_refusals_need_no_gpu():
    with pytest.raises(TypeError):
        sp.smooth_prolongator_inspect(object(), None, 1)
    with pytest.raises(TypeError):
        sp.smooth_prolongator(sp.operation_info_t(), None, None, 0.5)
    with pytest.raises(TypeError):
        sp.smooth_prolongator_structure(sp.operation_info_t(), None)
