"""Host-side proof of tests/aggregate_util.py (no GPU): the model of the rounds equals sequential greedy MIS on the square of the
strong graph, every rung of tests/test_gpu_aggregate.py is reached by its generator, each seeded mistake of the model fails a
named rung, and the checkers pass the model and fail broken results."""
import os

import numpy as np
import pytest

import aggregate_util as A
import multicolor_util as MC
import spblas_reference_amd as sp
from spblas_reference_amd import _build

DTYPES = [np.float32, np.float64]


def rungs():
    """name -> (rowptr, colind, values, theta): the graphs the device is compared on."""
    r = {f"path_{n}": A.path(n) + (0.0,) for n in range(1, 41)}
    r.update({
        "grid5_7x9": A.grid5(7, 9) + (0.0,), "lap7_5": A.lap7(5) + (0.0,), "hub_300": A.hub(300) + (0.0,),
        "upper_bidiagonal_30": A.upper_bidiagonal(30) + (0.0,), "repeated_entries": A.repeated_entries() + (0.25,),
        "diagonal_9": A.diagonal(9) + (0.0,), "empty_rows": A.empty_rows() + (0.0,), "one_row": A.diagonal(1) + (0.0,),
        "through_covered": A.through_covered()[:3] + (0.0,), "anisotropic_12x6": A.anisotropic(12, 6) + (0.25,),
        "random_2000x3": A.random_graph(2000, 3, 1) + (0.0,), "random_2000x10_theta": A.random_graph(2000, 10, 2) + (0.25,),
    })
    return r


RUNGS = rungs()


# ---- the rounds equal sequential greedy on G^2 ---------------------------------------------------------------------------------
def test_model_equals_sequential_greedy_on_random_graphs():
    rng = np.random.default_rng(0)
    seen_rounds = set()
    for k in range(300):
        m = int(rng.integers(1, 61))
        edges = [(int(a), int(b)) for a, b in rng.integers(0, m, (int(rng.integers(0, 2 * m + 1)), 2)) if a != b]
        g = A.with_values(MC.from_edges(m, edges), 4.0)
        got = A.model(*g)
        assert np.array_equal(got["root"], A.greedy_roots(*g)), k
        assert A.check_aggregation(*g, 0.0, np.float32, got["agg"], got["root"], got["n_agg"]) == [], k
        seen_rounds.add(got["rounds"])
    assert len(seen_rounds) >= 3                                     # the rounds are exercised, not one-shot graphs


@pytest.mark.parametrize("name", ["path_40", "grid5_7x9", "lap7_5", "hub_300", "upper_bidiagonal_30", "repeated_entries",
                                  "empty_rows", "through_covered", "anisotropic_12x6", "random_2000x3", "random_2000x10_theta"])
def test_model_equals_sequential_greedy_on_the_rungs(name):
    rp, ci, v, theta = RUNGS[name]
    for dtype in DTYPES:
        got = A.model(rp, ci, v, theta, dtype)
        assert np.array_equal(got["root"], A.greedy_roots(rp, ci, v, theta, dtype))
        if rp.size - 1 <= 400:
            assert A.check_aggregation(rp, ci, v, theta, dtype, got["agg"], got["root"], got["n_agg"]) == []


def test_the_16_cubed_laplacian_has_the_aggregates_the_issue_quotes():
    g = A.lap7(16)
    got = A.model(*g)
    assert np.array_equal(got["root"], A.greedy_roots(*g))
    assert (got["n_agg"], got["smallest"], got["largest"]) == (394, 5, 17) and 2 <= got["rounds"] <= 5


# ---- every rung is reached ---------------------------------------------------------------------------------------------------
def test_lane_rungs_cover_every_team_width_and_the_block_edges():
    rungs = A.lane_rungs()
    assert sorted({G for G, _, _ in rungs}) == [4, 8, 16, 64]
    for G, m, g in rungs:
        assert A.lanes_for(g[0], g[1]) == G and (m + 1) % (256 // G) in (0, 1, 2)


def test_threshold_entries_are_strong_and_one_ulp_below_is_weak():
    for dtype in DTYPES:
        rp, ci, v = A.threshold(dtype)
        strong, d = A.strength(rp, ci, v, 0.25, dtype)
        rows = A._rows(rp)
        lo = np.minimum(rows, ci)
        off = ci != rows
        assert (d == 4).all() and strong[off & (lo % 2 == 0)].all() and not strong[off & (lo % 2 == 1)].any()
        assert (v[off & (lo % 2 == 1)].astype(dtype) < 1).all()
        got = A.model(rp, ci, v, 0.25, dtype)
        assert got["n_agg"] == 6 and got["largest"] == 2                # the strong pairs, nothing else


def test_anisotropic_aggregates_are_line_segments():
    rp, ci, v = A.anisotropic(12, 6)
    got = A.model(rp, ci, v, 0.25)
    for k in range(got["n_agg"]):
        members = np.flatnonzero(got["agg"] == k)
        assert len(set(members // 12)) == 1 and (np.diff(members) == 1).all()
    assert A.model(rp, ci, v, 0.0)["n_agg"] < got["n_agg"]            # with theta = 0 the y couplings join rows


def test_special_values():
    rp, ci, v = A.grid5(7, 9)
    rows = A._rows(rp)
    # a missing diagonal: d = 0 makes every entry of that row and column strong whatever theta is
    keep = ~((rows == 10) & (ci == 10))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=63))]).astype(np.int32)
    strong, d = A.strength(rp2, ci[keep], v[keep], 2.0, np.float32)
    assert d[10] == 0 and strong[rows[keep] == 10].all() and strong[ci[keep] == 10].all()
    assert not strong[(rows[keep] != 10) & (ci[keep] != 10)].any()      # theta = 2: (4 * 4) * 4 > 1
    # one NaN entry is weak, its mirror stays strong (theta = 0)
    vn = v.copy()
    p = int(np.flatnonzero((rows == 5) & (ci == 6))[0])
    vn[p] = np.nan
    strong, _ = A.strength(rp, ci, vn, 0.0, np.float32)
    assert not strong[p] and strong[(rows == 6) & (ci == 5)].all() and strong.sum() == (ci != rows).sum() - 1
    # theta = 0: explicit zeros are strong
    assert A.strength(rp, ci, np.where(ci == rows, v, 0.0), 0.0, np.float64)[0].sum() == (ci != rows).sum()


def test_through_covered_rung_is_what_it_says():
    rp, ci, v, u, w = A.through_covered()
    good = A.model(rp, ci, v)
    assert u not in good["root"] or w not in good["root"]


# ---- seeded mistakes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake,rung", [("t_not_through_covered", "through_covered"), ("one_sided", "upper_bidiagonal_30")])
def test_a_wrong_graph_walk_fails_its_rung(mistake, rung):
    rp, ci, v, theta = RUNGS[rung]
    good, bad = A.model(rp, ci, v, theta), A.model(rp, ci, v, theta, mistake=mistake)
    assert not np.array_equal(good["agg"], bad["agg"])
    assert A.check_aggregation(rp, ci, v, theta, np.float32, bad["agg"], bad["root"], bad["n_agg"]) != []
    assert not np.array_equal(bad["root"], A.greedy_roots(rp, ci, v, theta))


@pytest.mark.parametrize("mistake,rung", [("phase2_reads_phase2", "random_2000x3"), ("phase2_smallest_key", "grid5_7x9")])
def test_a_wrong_second_phase_fails_its_rung(mistake, rung):
    rp, ci, v, theta = RUNGS[rung]
    good, bad = A.model(rp, ci, v, theta), A.model(rp, ci, v, theta, mistake=mistake)
    assert np.array_equal(good["root"], bad["root"]) and not np.array_equal(good["agg"], bad["agg"])


def triple():
    """diag(2^24, 1, -2^24) in one aggregate: ((2^24 + 1) - 2^24) is 0 in float32, ((-2^24 + 1) + 2^24) is 1."""
    rp, ci = MC.diagonal_only(3)
    return rp, ci, np.array([2.0 ** 24, 1.0, -2.0 ** 24]), np.zeros(3, np.int32), 1


def test_descending_sums_fail_the_order_sensitive_triple():
    rp, ci, v, agg, n = triple()
    assert A.host_coarsen(rp, ci, v, agg, n, np.float32)[2].tolist() == [0.0]
    assert A.host_coarsen(rp, ci, v, agg, n, np.float32, mistake="sums_descending")[2].tolist() == [1.0]
    assert A.host_coarsen(rp, ci, v, agg, n, np.float64)[2].tolist() == [1.0]


# ---- coarsen model and checkers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid5_7x9", "repeated_entries", "empty_rows", "random_2000x3"])
def test_host_coarsen_equals_the_dense_galerkin_product_on_small_integers(name):
    rp, ci, _, theta = RUNGS[name]
    rng = np.random.default_rng(3)
    v = rng.integers(-8, 9, ci.size).astype(np.float64)
    got = A.model(rp, ci, RUNGS[name][2], theta)
    c_rp, c_ci, c_v, seg_ptr, order = A.host_coarsen(rp, ci, v, got["agg"], got["n_agg"], np.float32)
    assert A.check_coarse(got["n_agg"], c_rp, c_ci) == []
    D = A.dense_galerkin(rp, ci, v, got["agg"], got["n_agg"])
    rows = np.repeat(np.arange(got["n_agg"]), np.diff(c_rp))
    assert np.array_equal(D[rows, c_ci], c_v.astype(np.float64))
    mask = np.zeros_like(D, bool)
    mask[rows, c_ci] = True
    assert (D[~mask] == 0).all() and c_v.sum() == v.sum()
    assert (np.diff(order[seg_ptr[0]:seg_ptr[1]]) > 0).all()           # ascending source position inside a coarse entry


def test_checkers_fail_broken_results():
    rp, ci, v, theta = RUNGS["grid5_7x9"]
    got = A.model(rp, ci, v, theta)
    ok = lambda agg, root: A.check_aggregation(rp, ci, v, theta, np.float32, agg, root, root.size)
    assert ok(got["agg"], got["root"]) == []
    agg = got["agg"].copy()
    agg[got["root"][0]] = 1
    assert ok(agg, got["root"]) != []
    far = got["agg"].copy()
    far[0], far[62] = far[62], far[0]
    assert ok(far, got["root"]) != []
    assert ok(got["agg"], got["root"][::-1].copy()) != []
    undecided = got["agg"].copy()
    undecided[5] = -1
    assert ok(undecided, got["root"]) != []
    assert A.check_coarse(2, [0, 2, 3], [1, 0, 1]) != [] and A.check_coarse(2, [0, 2, 3], [0, 0, 1]) != []
    assert A.check_coarse(2, [0, 2, 3], [0, 1, 1]) == []


# ---- layers -----------------------------------------------------------------------------------------------------------------
def test_source_example_and_exports_are_in_place():
    assert "aggregate.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "aggregate.hip"))
    assert "device_aggregate" in _build.EXAMPLES
    for name in sp.AGGREGATION_EXPORTS:
        assert hasattr(sp, name)
    # every aggregation name has a stream-order case of its own or a reasoned exemption (tests/test_gpu_aggregate_stream.py)
    covered = {n for names in A.STREAM_CASES.values() for n in names}
    assert sorted(set(sp.AGGREGATION_EXPORTS) - covered - set(A.STREAM_EXEMPT)) == []
    assert sorted((covered | set(A.STREAM_EXEMPT)) - set(sp.AGGREGATION_EXPORTS)) == []


def test_host_side_refusals_need_no_gpu():
    with pytest.raises(TypeError):
        sp.aggregate(object())
    with pytest.raises(TypeError):
        sp.coarsen_inspect(object(), None, 1)
    with pytest.raises(TypeError):
        sp.coarsen(sp.operation_info_t(), None, None)
