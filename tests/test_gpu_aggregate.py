"""-m gpu tests of aggregate / coarsen_inspect / coarsen_structure / coarsen (spblas_gfx950_aggregate_* / coarsen_*,
csrc/aggregate.hip).  Every test fails on a backend without the feature: the names do not exist there.

The host model, the generators and the independent checkers are tests/aggregate_util.py, proved by tests/test_aggregate_cpu.py.
agg, root and info() must equal the model and pass the checker; A_c must equal the model's BIT FOR BIT.  Every output array is
longer than its result and poisoned behind it.  The one tolerance of this file is worked out where it is used."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import aggregate_util as A
import gpu_util as G
import ilu_util as U
import multicolor_util as MC
import spblas_reference_amd as sp
from spblas_reference_amd import _capi

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TD = {np.float32: torch.float32, np.float64: torch.float64}
PAD = 5
WILD = 2 ** 30
_MODEL = {}


def model(key, g, theta, dtype):
    """The model's answer for a rung, computed once and left unchanged."""
    k = (key, theta, np.dtype(dtype).name)
    if k not in _MODEL:
        _MODEL[k] = A.model(g[0], g[1], g[2], theta, dtype)
    return _MODEL[k]


def on_device(g, dtype=np.float32):
    """csr_view over over-long arrays: a wild column and NaN behind nnz."""
    rowptr, colind, values = g[:3]
    m, nnz = rowptr.size - 1, int(colind.size)
    d_v = G.dev(np.concatenate([np.asarray(values, np.float64), np.full(PAD, np.nan)]).astype(dtype))
    d_ci = G.dev(np.concatenate([colind.astype(np.int32), np.full(PAD, WILD, np.int32)]))
    return sp.csr_view(d_v, G.dev(rowptr.astype(np.int32)), d_ci, (m, m), nnz)


def empty_c(n, nnz, dtype):
    """A_c's arrays, poisoned throughout: rowptr / colind with WILD, values with NaN."""
    return sp.csr_view(torch.full((nnz + PAD,), float("nan"), dtype=TD[dtype], device="cuda"),
                       torch.full((n + 1 + PAD,), WILD, dtype=torch.int32, device="cuda"),
                       torch.full((nnz + PAD,), WILD, dtype=torch.int32, device="cuda"), (n, n), nnz)


def check_against_model(key, g, theta, dtype, check=True):
    want = model(key, g, theta, dtype)
    res = sp.aggregate(on_device(g, dtype), theta)
    agg, root = G.host(res.agg), G.host(res.root)
    assert agg.dtype == np.int32 and np.array_equal(agg, want["agg"]), f"{key}: {int((agg != want['agg']).sum())} rows differ"
    assert np.array_equal(root, want["root"]) and res.n_agg == want["n_agg"]
    info = res.info()
    for f, name in (("aggregates", "n_agg"), ("rounds", "rounds"), ("largest", "largest"), ("smallest", "smallest"),
                    ("singletons", "singletons"), ("strong_entries", "strong_entries")):
        assert info[f] == want[name], (key, f, info[f], want[name])
    assert info["lanes_per_row"] == A.lanes_for(g[0], g[1])
    if check:
        assert A.check_aggregation(g[0], g[1], g[2], theta, dtype, agg, root, res.n_agg) == []
    return res, want


# ---- graph rungs -------------------------------------------------------------------------------------------------------------
def test_paths_of_1_to_40_rows(gpu):
    for n in range(1, 41):
        check_against_model(f"path_{n}", A.path(n), 0.0, np.float32)


GRAPHS = {
    "grid5_7x9": lambda: A.grid5(7, 9), "lap7_5": lambda: A.lap7(5), "hub_300": lambda: A.hub(300),
    "hub_5000": lambda: A.hub(5000), "upper_bidiagonal_30": lambda: A.upper_bidiagonal(30),
    "repeated_entries": A.repeated_entries, "diagonal_9": lambda: A.diagonal(9), "empty_rows": A.empty_rows,
    "one_row": lambda: A.diagonal(1), "through_covered": lambda: A.through_covered()[:3],
    "random_2000x3": lambda: A.random_graph(2000, 3, 1), "random_2000x10": lambda: A.random_graph(2000, 10, 2),
    "random_2000x40": lambda: A.random_graph(2000, 40, 3),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_aggregates_equal_the_model(gpu, name, dtype):
    g = GRAPHS[name]()
    small = g[0].size <= 2001 and g[1].size <= 30000    # (the checker walks Python sets: not the large hub, not 40 per row)
    res, want = check_against_model(name, g, 0.0, dtype, check=small)
    if name == "diagonal_9":
        assert res.n_agg == 9 and res.info()["singletons"] == 9
    if name == "hub_5000":
        assert res.n_agg == 1 and res.info()["largest"] == 5001
    if name == "one_row":
        assert res.n_agg == 1 and res.info()["rounds"] == 1
    if name == "through_covered":
        _, _, _, u, w = A.through_covered()
        assert not (u in want["root"] and w in want["root"])


@pytest.mark.parametrize("rung", A.lane_rungs(), ids=lambda r: f"G{r[0]}_m{r[1]}")
def test_every_team_width_at_the_block_edges(gpu, rung):
    G_, m, g = rung
    res, _ = check_against_model(f"lanes_{G_}_{m}", g, 0.0, np.float32, check=False)
    assert res.info()["lanes_per_row"] == G_
    check_against_model(f"lanes_{G_}_{m}", g, 0.25, np.float32, check=False)


def test_empty_matrix(gpu):
    a = sp.csr_view(torch.zeros(0, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
                    torch.zeros(0, dtype=torch.int32, device="cuda"), (0, 0), 0)
    res = sp.aggregate(a)
    assert res.n_agg == 0 and res.agg.numel() == 0 and res.root.numel() == 0 and res.info()["rounds"] == 0
    info = sp.coarsen_inspect(a, res.agg, 0)
    assert tuple(info.shape) == (0, 0) and info.nnz == 0


def test_repeated_calls_give_identical_bits_and_rounds(gpu):
    for name in ("random_2000x10", "lap7_5"):
        a = on_device(GRAPHS[name]())
        first, second = sp.aggregate(a, 0.25), sp.aggregate(a, 0.25)
        assert torch.equal(first.agg, second.agg) and torch.equal(first.root, second.root) and first.info() == second.info()


# ---- theta rungs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_anisotropic_aggregates_are_line_segments(gpu, dtype):
    g = A.anisotropic(12, 6)
    res, _ = check_against_model("anisotropic", g, 0.25, dtype)
    agg = G.host(res.agg)
    for k in range(res.n_agg):
        members = np.flatnonzero(agg == k)
        assert len(set(members // 12)) == 1 and (np.diff(members) == 1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_entries_on_the_threshold_are_strong_and_one_ulp_below_weak(gpu, dtype):
    g = A.threshold(dtype)
    res, want = check_against_model("threshold", g, 0.25, dtype)
    assert res.n_agg == 6 and res.info()["strong_entries"] == 12 and res.info()["largest"] == 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("theta", [0, 0.25, 2])
def test_thetas_missing_diagonal_and_nan(gpu, theta, dtype):
    rp, ci, v = A.random_graph(500, 8, 7)
    check_against_model("random_500x8", (rp, ci, v), theta, dtype, check=False)
    rows = A._rows(rp)
    keep = ~((rows == 10) & (ci == 10))                               # row 10 loses its diagonal
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=500))]).astype(np.int32)
    check_against_model("missing_diagonal", (rp2, ci[keep], v[keep]), theta, dtype, check=False)
    vn = v.copy()
    vn[int(np.flatnonzero(ci != rows)[40])] = np.nan                   # one NaN off-diagonal entry: weak
    res, want = check_against_model("one_nan", (rp, ci, vn), theta, dtype, check=False)
    if theta == 0:
        assert res.info()["strong_entries"] == int((ci != rows).sum()) - 1


def test_theta_refusals(gpu):
    a = on_device(A.grid5(7, 9))
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sp.aggregate(a, bad)
    with pytest.raises(TypeError):
        sp.aggregate(a, "0.25")
    lib, hd, plan = _capi.lib(), sp.api._Handle.current(a.rowptr().device), ctypes.c_void_p()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    create = lambda h, pl, m, nnz, rp, ci, v, th, vt: lib.spblas_gfx950_aggregate_create(h, pl, m, nnz, rp, ci, v,
                                                                                           ctypes.c_double(th), vt)
    ok = (hd.h, ctypes.byref(plan), 63, a.size(), p(a.rowptr()), p(a.colind()), p(a.values()))
    # the statuses in their documented order
    assert create(None, None, -1, 0, None, None, None, -1.0, _capi.C32) == _capi.NOT_SUPPORTED
    assert create(None, None, -1, 0, None, None, None, -1.0, _capi.F32) == _capi.INVALID_HANDLE
    assert create(hd.h, None, -1, 0, None, None, None, -1.0, _capi.F32) == _capi.INVALID_POINTER
    assert create(*ok[:2], -1, *ok[3:], -1.0, 99) == _capi.INVALID_SIZE
    assert create(*ok, -1.0, 99) == _capi.INVALID_VALUE
    assert create(*ok, -1.0, _capi.F32) == _capi.INVALID_VALUE
    assert create(*ok, float("nan"), _capi.F32) == _capi.INVALID_VALUE
    assert plan.value is None
    assert create(*ok, 0.0, _capi.F32) == _capi.SUCCESS
    try:
        arr = (ctypes.c_int64 * 8)()
        assert lib.spblas_gfx950_aggregate_info(None, arr) == _capi.INVALID_POINTER
        assert lib.spblas_gfx950_aggregate_info(plan, arr) == 0 and arr[7] == 63
        n = int(arr[0])
        agg = torch.full((63 + PAD,), WILD, dtype=torch.int32, device="cuda")
        root = torch.full((n + PAD,), WILD, dtype=torch.int32, device="cuda")
        assert lib.spblas_gfx950_aggregate_copy(None, plan, p(agg), p(root)) == _capi.INVALID_HANDLE
        assert lib.spblas_gfx950_aggregate_copy(hd.h, None, p(agg), p(root)) == _capi.INVALID_POINTER
        assert lib.spblas_gfx950_aggregate_copy(hd.h, plan, None, None) == 0
        assert lib.spblas_gfx950_aggregate_copy(hd.h, plan, p(agg), p(root)) == 0
        want = model("grid5_7x9", A.grid5(7, 9), 0.0, np.float32)
        assert np.array_equal(G.host(agg)[:63], want["agg"]) and (G.host(agg)[63:] == WILD).all()
        assert np.array_equal(G.host(root)[:n], want["root"]) and (G.host(root)[n:] == WILD).all()
        pr = torch.full((64 + PAD,), WILD, dtype=torch.int32, device="cuda")
        pc = torch.full((63 + PAD,), WILD, dtype=torch.int32, device="cuda")
        pv = torch.full((63 + PAD,), float("nan"), device="cuda")
        prol = lambda h, pl, m, r, c, v, vt: lib.spblas_gfx950_aggregate_prolongator(h, pl, m, r, c, v, vt)
        assert prol(None, None, 0, None, None, None, _capi.C32) == _capi.NOT_SUPPORTED
        assert prol(None, plan, 63, p(pr), p(pc), p(pv), _capi.F32) == _capi.INVALID_HANDLE
        assert prol(hd.h, None, 63, p(pr), p(pc), p(pv), _capi.F32) == _capi.INVALID_POINTER
        assert prol(hd.h, plan, 63, p(pr), None, p(pv), _capi.F32) == _capi.INVALID_POINTER
        assert prol(hd.h, plan, 62, p(pr), p(pc), p(pv), 99) == _capi.PLAN_MISMATCH
        assert prol(hd.h, plan, 63, p(pr), p(pc), p(pv), 99) == _capi.INVALID_VALUE
        assert (G.host(pr) == WILD).all()
        assert prol(hd.h, plan, 63, p(pr), p(pc), p(pv), _capi.F32) == 0
        assert np.array_equal(G.host(pr)[:64], np.arange(64)) and (G.host(pr)[64:] == WILD).all()
        assert np.array_equal(G.host(pc)[:63], want["agg"]) and (G.host(pc)[63:] == WILD).all()
        assert (G.host(pv)[:63] == 1).all() and np.isnan(G.host(pv)[63:]).all()
    finally:
        assert lib.spblas_gfx950_aggregate_destroy(None, plan) == _capi.INVALID_HANDLE
        assert lib.spblas_gfx950_aggregate_destroy(hd.h, plan) == 0
    assert lib.spblas_gfx950_aggregate_destroy(hd.h, None) == 0


def test_structure_errors_and_operand_types(gpu):
    rp, ci, v = A.grid5(7, 9)
    bad = ci.copy()
    bad[7] = 63
    with pytest.raises(ValueError):
        sp.aggregate(on_device((rp, bad, v)))
    rp2 = rp.copy()
    rp2[-1] -= 1
    with pytest.raises(ValueError):
        sp.aggregate(on_device((rp2, ci, v)))
    agg = torch.zeros(63, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        sp.coarsen_inspect(on_device((rp, bad, v)), agg, 1)
    for td in (torch.complex64, torch.float16, torch.bfloat16):
        mk = sp.csr_view(torch.ones(ci.size, dtype=td, device="cuda"), G.dev(rp), G.dev(ci), (63, 63), ci.size)
        with pytest.raises(TypeError):
            sp.aggregate(mk)
        with pytest.raises(TypeError):
            sp.coarsen_inspect(mk, agg, 1)
    a = on_device((rp, ci, v))
    for wrap in (sp.scaled(2.0, a), sp.transposed(a)):
        with pytest.raises(TypeError):
            sp.aggregate(wrap)
    rect = sp.csr_view(a.values(), a.rowptr(), a.colind(), (63, 64), a.size())
    with pytest.raises(ValueError):
        sp.aggregate(rect)
    with pytest.raises(TypeError):
        sp.coarsen_inspect(a, agg.long(), 1)
    with pytest.raises(ValueError):
        sp.coarsen_inspect(a, agg[:62], 1)


# ---- coarsen -----------------------------------------------------------------------------------------------------------------
def coarse(a, agg_dev, n_agg, dtype):
    info = sp.coarsen_inspect(a, agg_dev, n_agg)
    assert tuple(info.shape) == (n_agg, n_agg) and info.result_nnz() == info.nnz
    c = empty_c(n_agg, info.nnz, dtype)
    sp.coarsen_structure(info, c)
    sp.coarsen(info, a, c)
    return info, c


def host_c(c, n, nnz):
    rp, ci, v = G.host(c.rowptr()), G.host(c.colind()), G.host(c.values())
    assert (rp[n + 1:] == WILD).all() and (ci[nnz:] == WILD).all() and np.isnan(v[nnz:]).all(), "written behind the end"
    return rp[:n + 1], ci[:nnz], v[:nnz]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["grid5_7x9", "repeated_entries", "empty_rows", "hub_300", "random_2000x10", "lap7_5"])
def test_small_integers_equal_the_model_and_the_dense_product_bit_for_bit(gpu, name, dtype):
    g = GRAPHS[name]()
    rp, ci = g[0], g[1]
    vals = np.random.default_rng(3).integers(-8, 9, ci.size).astype(np.float64)
    res = sp.aggregate(on_device(g, dtype))
    a = on_device((rp, ci, vals), dtype)
    info, c = coarse(a, res.agg, res.n_agg, dtype)
    agg = G.host(res.agg)
    w_rp, w_ci, w_v, _, _ = A.host_coarsen(rp, ci, vals, agg, res.n_agg, dtype)
    c_rp, c_ci, c_v = host_c(c, res.n_agg, info.nnz)
    assert info.nnz == w_ci.size and np.array_equal(c_rp, w_rp) and np.array_equal(c_ci, w_ci)
    assert np.array_equal(U.bits(c_v), U.bits(w_v))
    assert A.check_coarse(res.n_agg, c_rp, c_ci) == []
    assert c_v.sum() == vals.sum()                                       # the entry sum is preserved (small integers: exact)
    if res.n_agg <= 500:
        D = A.dense_galerkin(rp, ci, vals, agg, res.n_agg)
        rows = np.repeat(np.arange(res.n_agg), np.diff(c_rp))
        mask = np.zeros_like(D, bool)
        mask[rows, c_ci] = True
        assert np.array_equal(D[rows, c_ci], c_v.astype(np.float64)) and (D[~mask] == 0).all()
    assert np.array_equal(U.bits(G.host(a.values())[:ci.size]), U.bits(vals.astype(dtype))), "A's values changed"


def test_the_order_sensitive_triple(gpu):
    rp, ci = MC.diagonal_only(3)
    v = np.array([2.0 ** 24, 1.0, -2.0 ** 24])
    agg = torch.zeros(3, dtype=torch.int32, device="cuda")
    for dtype, want in ((np.float32, 0.0), (np.float64, 1.0)):       # ((2^24 + 1) - 2^24): 0 in float32, 1 in float64
        info, c = coarse(on_device((rp, ci, v), dtype), agg, 1, dtype)
        assert info.nnz == 1 and host_c(c, 1, 1)[2].tolist() == [want]
        assert A.host_coarsen(rp, ci, v, np.zeros(3, np.int32), 1, dtype)[2].tolist() == [want]


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_values_equal_the_model_and_stay_inside_the_summation_bound(gpu, dtype):
    """Against the float64 sum: recursive summation of n terms is off by at most (n - 1) eps sum|a| to first order (Higham,
    Accuracy and Stability, eq. 4.4 with gamma_{n-1} ~ (n - 1) u, u = eps / 2: the bound below is twice that)."""
    g = A.random_graph(2000, 10, 2)
    rp, ci = g[0], g[1]
    vals = np.random.default_rng(9).standard_normal(ci.size)
    res = sp.aggregate(on_device(g, dtype), 0.25)
    agg = G.host(res.agg)
    a = on_device((rp, ci, vals), dtype)
    info, c = coarse(a, res.agg, res.n_agg, dtype)
    w_rp, w_ci, w_v, seg_ptr, order = A.host_coarsen(rp, ci, vals, agg, res.n_agg, dtype)
    c_rp, c_ci, c_v = host_c(c, res.n_agg, info.nnz)
    assert np.array_equal(c_rp, w_rp) and np.array_equal(c_ci, w_ci) and np.array_equal(U.bits(c_v), U.bits(w_v))
    v64 = vals.astype(dtype).astype(np.float64)[order]
    exact = np.add.reduceat(v64, seg_ptr[:-1])
    bound = np.add.reduceat(np.abs(v64), seg_ptr[:-1]) * (np.diff(seg_ptr) - 1) * np.finfo(dtype).eps
    assert (np.abs(c_v.astype(np.float64) - exact) <= bound).all()


def test_user_made_maps_empty_aggregates_and_the_extremes(gpu):
    g = A.grid5(7, 9)
    rp, ci, _ = g
    m, nnz = 63, int(ci.size)
    vals = np.random.default_rng(4).integers(-8, 9, nnz).astype(np.float64)
    a = on_device((rp, ci, vals))
    rng = np.random.default_rng(5)
    maps = {"one": (np.zeros(m, np.int32), 1), "identity": (np.arange(m, dtype=np.int32), m),
            "user": (rng.integers(0, 9, m).astype(np.int32), 9),
            "empty_aggregates": ((rng.integers(0, 5, m) * 3 + 1).astype(np.int32), 17)}       # 0, 2, 3, 5, ... hold no row
    for name, (agg, n) in maps.items():
        info, c = coarse(a, G.dev(agg), n, np.float32)
        w_rp, w_ci, w_v, _, _ = A.host_coarsen(rp, ci, vals, agg, n, np.float32)
        c_rp, c_ci, c_v = host_c(c, n, info.nnz)
        assert np.array_equal(c_rp, w_rp) and np.array_equal(c_ci, w_ci) and np.array_equal(U.bits(c_v), U.bits(w_v)), name
        assert A.check_coarse(n, c_rp, c_ci) == []
        if name == "one":
            assert info.nnz == 1 and c_v[0] == vals.sum()
        if name == "identity":                                            # sorted rows: A itself
            assert np.array_equal(c_rp, rp) and np.array_equal(c_ci, ci) and np.array_equal(c_v, vals.astype(np.float32))
        if name == "empty_aggregates":
            assert (np.diff(c_rp)[[0, 2, 3, 5]] == 0).all()
    for bad in (np.full(m, 9, np.int32), np.full(m, -1, np.int32)):
        with pytest.raises(ValueError):
            sp.coarsen_inspect(a, G.dev(bad), 9)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edited_values_on_one_info_eagerly_and_in_a_graph(gpu, dtype):
    g = A.random_graph(2000, 10, 2)
    rp, ci = g[0], g[1]
    nnz = int(ci.size)
    rng = np.random.default_rng(6)
    a = on_device((rp, ci, rng.standard_normal(nnz)), dtype)
    res = sp.aggregate(on_device(g, dtype))
    agg = G.host(res.agg)
    info = sp.coarsen_inspect(a, res.agg, res.n_agg)
    plan, cn, n = info.state_, info.nnz, res.n_agg
    # the coarse value array lies inside a longer NaN-patterned one whose pattern must keep its bits
    big = torch.full((cn + 2 * PAD,), float("nan"), dtype=TD[dtype], device="cuda")
    pattern = U.bits(G.host(big)).copy()
    c = sp.csr_view(big[PAD:PAD + cn], torch.full((n + 1,), WILD, dtype=torch.int32, device="cuda"),
                    torch.full((cn,), WILD, dtype=torch.int32, device="cuda"), (n, n), cn)
    g0, g1 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    p = sp.csr_view(torch.zeros(2000, dtype=TD[dtype], device="cuda"), torch.zeros(2001, dtype=torch.int32, device="cuda"),
                    torch.zeros(2000, dtype=torch.int32, device="cuda"), (2000, n), 2000)
    with torch.cuda.graph(g0):                         # recorded from the FIRST call of each
        sp.coarsen_structure(info, c)
        res.prolongator(p)
    with torch.cuda.graph(g1):
        sp.coarsen(info, a, c)
    assert (G.host(c.colind()) == WILD).all() and np.array_equal(U.bits(G.host(big)), pattern)    # recording ran nothing
    g0.replay()
    w_rp, w_ci, _, _, _ = A.host_coarsen(rp, ci, np.zeros(nnz), agg, n, dtype)
    assert np.array_equal(G.host(c.rowptr()), w_rp) and np.array_equal(G.host(c.colind()), w_ci)
    assert np.array_equal(G.host(p.rowptr()), np.arange(2001)) and np.array_equal(G.host(p.colind()), agg)
    assert (G.host(p.values()) == 1).all()
    for replay in (False, True, False, True):
        new = rng.standard_normal(nnz).astype(dtype)
        a.values()[:nnz].copy_(G.dev(new))
        big.fill_(float("nan"))
        c.colind().fill_(WILD)                                # the value pass must not touch the structure
        g1.replay() if replay else sp.coarsen(info, a, c)
        assert info.state_ is plan
        got = G.host(big)
        assert np.array_equal(U.bits(got[PAD:PAD + cn]), U.bits(A.host_coarsen(rp, ci, new, agg, n, dtype)[2]))
        assert np.array_equal(U.bits(got[:PAD]), pattern[:PAD]) and np.array_equal(U.bits(got[PAD + cn:]), pattern[PAD + cn:])
        assert (G.host(c.colind()) == WILD).all()
    # an info made for other arrays is replaced by a new inspect
    a2 = on_device((rp, ci, rng.standard_normal(nnz)), dtype)
    sp.coarsen(info, a2, c)
    assert info.state_ is not plan and info.nnz == cn
    # prolongator(dtype) allocates and returns the same matrix
    q = res.prolongator(TD[dtype])
    assert tuple(q.shape()) == (2000, n) and torch.equal(q.colind(), res.agg) and bool((q.values() == 1).all())


def test_inspects_raise_inside_a_capture(gpu):
    g = A.grid5(7, 9)
    a = on_device(g)
    res = sp.aggregate(a)                                   # the handle exists before the capture
    torch.cuda.synchronize()
    raised = []
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for call in (lambda: sp.aggregate(a), lambda: sp.coarsen_inspect(a, res.agg, res.n_agg)):
            try:
                call()
                raised.append(None)
            except Exception as e:  # noqa: BLE001
                raised.append(e)
    assert all(isinstance(e, sp.BackendError) and "not supported" in str(e).lower() for e in raised), raised
    assert sp.aggregate(a).n_agg == res.n_agg               # and outside the capture everything works as before


def test_coarsen_calls_check_their_plan_and_their_buffers(gpu):
    g = A.lap7(5)
    a = on_device(g)
    res = sp.aggregate(a)
    info = sp.coarsen_inspect(a, res.agg, res.n_agg)
    plan, lib, nnz, cn = info.state_, _capi.lib(), a.size(), info.nnz
    c = empty_c(res.n_agg, cn, np.float32)
    av, cv = a.values().data_ptr(), c.values().data_ptr()
    h = plan.hd.h
    val = lambda hh, pl, n, x, k, y, vt: lib.spblas_gfx950_coarsen_values(hh, pl, n, x, k, y, vt)
    # the statuses in their documented order
    assert val(None, None, nnz - 1, None, cn, None, _capi.C32) == _capi.NOT_SUPPORTED
    assert val(None, None, nnz - 1, None, cn, None, _capi.F32) == _capi.INVALID_HANDLE
    assert val(h, None, nnz, av, cn, cv, _capi.F32) == _capi.INVALID_POINTER
    assert val(h, plan.plan, nnz - 1, None, cn, cv, 99) == _capi.INVALID_POINTER
    assert val(h, plan.plan, nnz - 1, av, cn, cv, 99) == _capi.PLAN_MISMATCH
    assert val(h, plan.plan, nnz, av, cn - 1, cv, 99) == _capi.PLAN_MISMATCH
    assert val(h, plan.plan, nnz, av, cn, av, 99) == _capi.INVALID_VALUE
    assert val(h, plan.plan, nnz, av, cn, av, _capi.F32) == _capi.INVALID_VALUE      # no in-place form
    assert np.isnan(G.host(c.values())).all()
    assert val(h, plan.plan, nnz, av, cn, cv, _capi.F32) == _capi.SUCCESS
    st = lambda hh, pl, r, cc: lib.spblas_gfx950_coarsen_structure(hh, pl, r, cc)
    assert st(None, plan.plan, c.rowptr().data_ptr(), c.colind().data_ptr()) == _capi.INVALID_HANDLE
    assert st(h, None, c.rowptr().data_ptr(), c.colind().data_ptr()) == _capi.INVALID_POINTER
    assert st(h, plan.plan, None, c.colind().data_ptr()) == _capi.INVALID_POINTER
    arr = (ctypes.c_int64 * 4)()
    assert lib.spblas_gfx950_coarsen_info(None, arr) == _capi.INVALID_POINTER
    assert lib.spblas_gfx950_coarsen_info(plan.plan, arr) == 0 and list(arr) == [res.n_agg, cn, 125, nnz]
    create = lambda hh, out, m, n, rp, ci, ag, k: lib.spblas_gfx950_coarsen_create(hh, out, m, n, rp, ci, ag, k)
    out = ctypes.c_void_p()
    ptrs = (a.rowptr().data_ptr(), a.colind().data_ptr(), res.agg.data_ptr())
    assert create(None, None, -1, nnz, None, None, None, -1) == _capi.INVALID_HANDLE
    assert create(h, None, -1, nnz, *ptrs, -1) == _capi.INVALID_POINTER
    assert create(h, ctypes.byref(out), -1, nnz, *ptrs, -1) == _capi.INVALID_SIZE
    assert create(h, ctypes.byref(out), 125, nnz, *ptrs, -1) == _capi.INVALID_SIZE
    assert create(h, ctypes.byref(out), 125, nnz, *ptrs, res.n_agg - 1) == _capi.INVALID_VALUE
    assert out.value is None
    assert lib.spblas_gfx950_coarsen_destroy(None, plan.plan) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_coarsen_destroy(h, None) == 0
    # Python: a_c must not alias A's arrays
    alias = sp.csr_view(a.values()[:cn], c.rowptr(), c.colind(), (res.n_agg, res.n_agg), cn)
    with pytest.raises(ValueError):
        sp.coarsen(info, a, alias)
    with pytest.raises(TypeError):
        sp.coarsen(sp.operation_info_t(), a, c)
    with pytest.raises(TypeError):
        sp.coarsen(info, a, empty_c(res.n_agg, cn, np.float64))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_coarse_matrix_equals_the_route_through_transpose_and_two_spgemms(gpu, dtype):
    """A_c against multiply(transpose(P), multiply(A, P)) of the existing operations: both are sums of the same terms in
    different orders (the products with P's ones are exact), so each is within (terms - 1) u sum|a| of the exact sum, u = eps / 2
    (Higham, Accuracy and Stability, section 4.2: any order of recursive summation), and they differ by at most twice that:
    (terms - 1) eps sum|a| per entry."""
    g = A.lap7(12)
    rp, ci = g[0], g[1]
    m, nnz = rp.size - 1, int(ci.size)
    vals = np.random.default_rng(8).standard_normal(nnz)
    a = on_device((rp, ci, vals), dtype)
    res = sp.aggregate(on_device(g, dtype))
    n = res.n_agg
    info, c = coarse(a, res.agg, n, dtype)
    p = res.prolongator(TD[dtype])
    a_exact = sp.csr_view(a.values()[:nnz], a.rowptr(), a.colind()[:nnz], (m, m), nnz)

    def product(x, y, shape):
        rp_ = torch.zeros(shape[0] + 1, dtype=torch.int32, device="cuda")
        z = sp.csr_view(None, rp_, None, shape, 0)
        st = sp.multiply_compute(x, y, z)
        k = st.result_nnz()
        z.update(torch.zeros(k, dtype=TD[dtype], device="cuda"), rp_, torch.zeros(k, dtype=torch.int32, device="cuda"), shape, k)
        sp.multiply_fill(st, x, y, z)
        return z

    ap = product(a_exact, p, (m, n))
    pt = sp.csr_view(torch.zeros(m, dtype=TD[dtype], device="cuda"), torch.zeros(n + 1, dtype=torch.int32, device="cuda"),
                     torch.zeros(m, dtype=torch.int32, device="cuda"), (n, m), m)
    sp.transpose(p, pt)
    ref = product(pt, ap, (n, n))
    import scipy.sparse as sps
    R = sps.csr_matrix((G.host(ref.values()).astype(np.float64), G.host(ref.colind()), G.host(ref.rowptr())), shape=(n, n))
    c_rp, c_ci, c_v = host_c(c, n, info.nnz)
    C = sps.csr_matrix((c_v.astype(np.float64), c_ci, c_rp), shape=(n, n))
    agg = G.host(res.agg)
    _, _, _, seg_ptr, order = A.host_coarsen(rp, ci, vals, agg, n, dtype)
    bound = np.add.reduceat(np.abs(vals.astype(dtype).astype(np.float64)[order]), seg_ptr[:-1]) * \
        (np.diff(seg_ptr) - 1) * np.finfo(dtype).eps
    rows = np.repeat(np.arange(n), np.diff(c_rp))
    diff = np.abs(np.asarray(R[rows, c_ci]).ravel() - c_v)
    assert R.nnz == C.nnz and (diff <= bound).all()


def test_create_destroy_cycles_do_not_leak_device_memory(gpu):
    g = A.lap7(24)
    a = on_device(g)
    res0 = sp.aggregate(a)
    info0 = sp.coarsen_inspect(a, res0.agg, res0.n_agg)
    c = empty_c(res0.n_agg, info0.nnz, np.float32)
    del res0, info0

    def cycle():
        res = sp.aggregate(a)
        info = sp.coarsen_inspect(a, res.agg, res.n_agg)
        sp.coarsen_structure(info, c)
        sp.coarsen(info, a, c)
        del res, info

    for _ in range(5):      # warm-up: pools and the handle's scratch reach their size
        cycle()
    torch.cuda.synchronize()
    gc.collect()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(200):
        cycle()
    torch.cuda.synchronize()
    gc.collect()
    free1, _ = torch.cuda.mem_get_info()
    lost = free0 - free1
    # one cycle allocates ~1.5 MB of plans and work arrays: a leak of any of them shows over 200 cycles
    assert lost < 8 * 2 ** 20, f"free device memory fell by {lost / 2**20:.1f} MiB over 200 cycles"
